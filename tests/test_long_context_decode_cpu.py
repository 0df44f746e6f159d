"""Cached generate() over text contexts of more than 287 tokens without a GPU: the rows form of the single-query attention kernel
(amdnuwa_attn_rows, csrc/decode.hip) is exported, declared and registered, its argument checks answer before anything is launched
(arguments, then the envelope, then the workspace), its workspace is the single-row formula over one chunk of queries, the ABI version
is unchanged, both class switches are off by default, the eligibility predicate of the row program's long form asks for geometry
alone, and the fixtures g21a / g21b load and carry their condition on the inputs."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
CHUNK = 2048                      # query rows per set of launches: the workspace is that of one chunk
FIXTURES = ('g21a_generate_long_context', 'g21b_generate_long_context_reversible')


@pytest.fixture(scope='module')
def L():
    from nuwa_pytorch_amd import _lib
    return _lib.lib()


def _call(L, B=2, R=33, T=300, heads=8, dh=64, ptr=ctypes.c_void_p(16), ws=ctypes.c_void_p(16), ws_bytes=1 << 40, **over):
    """argument list of amdnuwa_attn_rows with every pointer `ptr` (never dereferenced on the host); over: name -> value"""
    inner = heads * dh
    a = dict(B=B, R=R, T=T, heads=heads, dim_head=dh, scale=0.125, q=ptr, q_lo=None, ldq=inner, kv=ptr, kv_lo=None, cache_rows=320,
             first_row=ptr, key_mask=None, null_k=ptr, null_v=ptr, w_th=ptr, th_bias=None, o=ptr, o_lo=None, ldo=inner, workspace=ws,
             workspace_bytes=ws_bytes, stream=None)
    assert not set(over) - set(a), over
    a.update(over)
    return L.amdnuwa_attn_rows(*a.values())


def test_entry_points_are_exported_declared_and_registered(L):
    from nuwa_pytorch_amd import _lib
    from nuwa_pytorch_amd import kernels as K
    header = open(os.path.join(ROOT, 'include', 'amdnuwa.h')).read()
    for name in ('amdnuwa_attn_rows', 'amdnuwa_attn_rows_workspace_bytes'):
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES
        assert re.search(r'\b' + name + r'\s*\(', header), name
    assert callable(K.attn_rows) and K.ATTN_ROWS_CHUNK == CHUNK
    assert L.amdnuwa_abi_version() == 21                      # purely additive


def test_argument_checks_answer_before_any_launch(L):
    assert _call(L, ptr=None) == ARG
    for name in ('q', 'kv', 'first_row', 'null_k', 'null_v', 'w_th', 'o'):
        assert _call(L, **{name: None}) == ARG, name
    for name in ('B', 'R', 'T', 'heads', 'dh', 'cache_rows'):
        for v in (0, -3):
            assert _call(L, **{name: v}) == ARG, (name, v)
    assert _call(L, cache_rows=299) == ARG and _call(L, cache_rows=300, ws=None) == WORKSPACE      # cache_rows < T / == T
    lo = ctypes.c_void_p(32)
    for one_side in ('q_lo', 'kv_lo', 'o_lo'):                # the lo images come together or not at all
        assert _call(L, **{one_side: lo}) == ARG, one_side
    assert _call(L, q_lo=lo, o_lo=lo) == ARG and _call(L, kv_lo=lo, o_lo=lo) == ARG and _call(L, q_lo=lo, kv_lo=lo) == ARG
    assert _call(L, ldq=8) == ARG and _call(L, ldo=8) == ARG
    assert _call(L, B=1 << 16, R=1 << 15) == ARG              # B * R = 2^31: the q / o row index is an int
    assert _call(L, B=(1 << 16) - 1, R=1 << 15, ws=None) == WORKSPACE          # just under it: past the argument checks
    assert _call(L, heads=9) == UNSUPPORTED
    assert _call(L, dh=48) == UNSUPPORTED
    need = L.amdnuwa_attn_rows_workspace_bytes(2, 33, 300, 8, 64)
    assert need > 16
    assert _call(L, ws_bytes=need - 1) == WORKSPACE
    assert _call(L, ws=None) == WORKSPACE
    assert _call(L, ws_bytes=16) == WORKSPACE
    assert _call(L, q_lo=lo, kv_lo=lo, o_lo=lo, ws_bytes=16) == WORKSPACE      # all three lo images: past the argument checks
    assert _call(L, R=1, ws=None, ws_bytes=0) == WORKSPACE                     # no row is special: R = 1 launches too
    # arguments first, the envelope second, the workspace last
    assert _call(L, heads=9, q=None) == ARG and _call(L, dh=48, cache_rows=0) == ARG and _call(L, heads=9, dh=48, kv_lo=lo) == ARG
    assert _call(L, heads=9, R=0) == ARG
    assert _call(L, heads=9, ws=None, ws_bytes=0) == UNSUPPORTED


@pytest.mark.parametrize('heads,dh', [(8, 64), (3, 64), (2, 32), (5, 32)])
def test_workspace_is_the_single_row_formula_over_one_chunk(L, heads, dh):
    ws = lambda B, R, T: L.amdnuwa_attn_rows_workspace_bytes(B, R, T, heads, dh)
    for B, R in ((1, 1), (2, 17), (3, 40), (2, 33), (2, 1024), (2, 1025), (32, 2305), (65600, 2)):
        for T in (1, 127, 128, 300, 512):
            assert ws(B, R, T) == L.amdnuwa_attn_decode_rows_workspace_bytes(min(B * R, CHUNK), T, heads, dh), (B, R, T)
            assert ws(B, R, T) > 0
    assert ws(0, 5, 10) == 0 and ws(2, 0, 10) == 0 and ws(2, 5, 0) == 0


def test_both_class_switches_are_off_by_default():
    from nuwa_pytorch_amd import NUWA, NUWAVideoAudio
    assert NUWA.generate_long_context_cache is False
    assert NUWAVideoAudio.generate_long_context_cache is False
    assert NUWA.generate_use_cache is True and NUWA.generate_slide_cache is True and NUWAVideoAudio.generate_use_cache is True


def test_long_context_is_a_keyword_last_in_every_signature_and_off():
    from nuwa_pytorch_amd import decode
    for cls in (decode.IncrementalDecoder, decode.DualIncrementalDecoder, decode.GuidedStepper, decode.DualGuidedStepper):
        params = list(inspect.signature(cls.__init__).parameters.values())
        assert params[-1].name == 'long_context' and params[-1].default is False, cls.__name__
        assert params[-1].kind is inspect.Parameter.KEYWORD_ONLY, cls.__name__


def test_eligibility_is_geometry_alone():
    """the long form of the row program asks what the rows kernels take -- not causal, more keys than the packed images hold, at most 8
    heads of 32 or 64 -- in every precision mode and with the training route's speed thresholds at their defaults"""
    import nuwa_pytorch_amd as A
    from nuwa_pytorch_amd import decode
    from nuwa_pytorch_amd.nuwa_pytorch import Attention
    attn = lambda **kw: Attention(**{**dict(dim=64, heads=2, dim_head=32), **kw})
    assert Attention.long_pairs_min == 1 << 23 and Attention.long_wgs_min == 128          # the defaults: not lowered for this test
    prev = A.get_precision()
    try:
        for mode in ('bf16x3', 'bf16x3-fwd', 'bf16'):
            A.set_precision(mode)
            m = attn()
            assert decode.long_context_ok(m, 288) and decode.long_context_ok(m, 320) and decode.long_context_ok(m, 100000), mode
            assert decode.long_context_ok(attn(heads=8, dim_head=64), 512), mode
            assert decode.long_context_ok(attn(heads=3), 300), mode
            assert not decode.long_context_ok(m, 287) and not decode.long_context_ok(m, 8) and not decode.long_context_ok(m, None), mode
            assert not decode.long_context_ok(attn(causal=True), 320), mode
            assert not decode.long_context_ok(attn(heads=9), 320), mode
            assert not decode.long_context_ok(attn(dim_head=48), 320), mode
        # what the training route answers for the same block at a generate-sized shape: no -- which is why the row program asks on its own
        A.set_precision('bf16x3')
        assert not attn()._long_hip_ok(320, 33, 2)
        A.set_precision('bf16')
        assert not attn()._long_hip_ok(320, 33, 2)
    finally:
        A.set_precision(prev)
    assert decode.X_PACKED_MAX_KEYS == 287


@pytest.mark.parametrize('name', FIXTURES)
def test_fixtures_load_and_carry_their_condition_on_the_inputs(name):
    import torch
    from golden_util import load
    Ar, P, _ = load(name)
    assert float(Ar['min_gap']) >= 3e-3
    assert bool(Ar['reversible']) == name.endswith('reversible')
    text = Ar['text']
    assert tuple(text.shape) == (2, 300) and bool((text[0] != 0).all()) and bool((text[1, :120] != 0).all()) and bool((text[1, 120:] == 0).all())
    assert tuple(Ar['video_ids'].shape) == (2, 80) and int(Ar['num_frames']) == 5 and float(Ar['cond_scale']) == 2.
    assert tuple(Ar['cond_logits'].shape) == (2, 48, 64) and bool(torch.isfinite(Ar['cond_logits']).all())
    assert tuple(P['text_abs_pos_emb.embed.weight'].shape)[0] == 300 if 'text_abs_pos_emb.embed.weight' in P else True
    assert not any(k.startswith('vae.') for k in P)
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', name + '.npz')) < 1 << 20
