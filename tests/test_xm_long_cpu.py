"""Single-query attention over any number of cached rows (amdnuwa_attn_decode_rows, csrc/decode.hip; np.py:339-378, 908-1067) without a
GPU: the entry point and its workspace function are exported, declared and registered, their argument checks answer before anything is
launched, the ABI version is unchanged, and the routing predicates of the two consumers (decode._XmDirection, the training route of
CrossModalityCrossAttention) take context frames of more than 287 rows."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
SPLIT = 128


@pytest.fixture(scope='module')
def L():
    from nuwa_pytorch_amd import _lib
    return _lib.lib()


def _call(L, B=2, T=300, heads=8, dh=64, ptr=ctypes.c_void_p(16), ws=ctypes.c_void_p(16), ws_bytes=1 << 40, **over):
    """argument list of amdnuwa_attn_decode_rows with every pointer `ptr` (never dereferenced on the host); over: name -> value"""
    inner = heads * dh
    a = dict(B=B, T=T, heads=heads, dim_head=dh, scale=dh ** -0.5, q=ptr, q_lo=None, ldq=inner, kv=ptr, kv_lo=None, cache_rows=T + 5,
             first_row=ptr, key_mask=None, null_k=ptr, null_v=ptr, w_th=ptr, th_bias=None, o=ptr, o_lo=None, ldo=inner, workspace=ws,
             workspace_bytes=ws_bytes, stream=None)
    a.update(over)
    return L.amdnuwa_attn_decode_rows(*a.values())


def test_entry_points_are_exported_declared_and_registered(L):
    from nuwa_pytorch_amd import _lib
    from nuwa_pytorch_amd import kernels as K
    header = open(os.path.join(ROOT, 'include', 'amdnuwa.h')).read()
    for name in ('amdnuwa_attn_decode_rows', 'amdnuwa_attn_decode_rows_workspace_bytes'):
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES
        assert re.search(r'\b' + name + r'\s*\(', header), name
    assert callable(K.attn_decode_rows)
    assert L.amdnuwa_abi_version() == 21                      # purely additive


def test_argument_checks_answer_before_any_launch(L):
    assert _call(L, ptr=None) == ARG
    for name in ('q', 'kv', 'first_row', 'null_k', 'null_v', 'w_th', 'o'):
        assert _call(L, **{name: None}) == ARG, name
    assert _call(L, T=0) == ARG
    assert _call(L, cache_rows=299) == ARG                    # the window cannot fit
    assert _call(L, ldq=8) == ARG and _call(L, ldo=8) == ARG
    assert _call(L, heads=9) == UNSUPPORTED
    assert _call(L, dh=48) == UNSUPPORTED
    assert _call(L, heads=1, dh=32, B=0) == OK
    assert _call(L, B=0, ws=None, ws_bytes=0) == OK           # nothing to do: no workspace needed
    need = L.amdnuwa_attn_decode_rows_workspace_bytes(2, 300, 8, 64)
    assert _call(L, ws_bytes=need - 1) == WORKSPACE
    assert _call(L, ws=None) == WORKSPACE
    assert _call(L, ws_bytes=16) == WORKSPACE


@pytest.mark.parametrize('heads,dh', [(8, 64), (3, 64), (1, 32), (5, 32)])
def test_workspace_follows_the_documented_formula(L, heads, dh):
    """4 * B * (heads * (T + 1) + splits * (2 * heads + heads * dim_head)) bytes, splits = ceil((T + 1) / 128): fp32 scores, the per-split
    softmax statistics and the per-split partial output rows"""
    from nuwa_pytorch_amd import kernels as K
    assert K.ATTN_DECODE_ROWS_SPLIT == SPLIT
    ws = lambda B, T: L.amdnuwa_attn_decode_rows_workspace_bytes(B, T, heads, dh)
    for B in (1, 3, 8):
        for T in (1, 31, 126, 127, 128, 288, 289, 1000, 4096):
            splits = -(-(T + 1) // SPLIT)
            assert K.attn_decode_rows_splits(T) == splits
            assert ws(B, T) == 4 * B * (heads * (T + 1) + splits * (2 * heads + heads * dh)), (B, T)
    # one more slot past a split boundary opens one more split: one more statistics block and one more partial row per sample
    assert ws(1, 128) - ws(1, 127) == 4 * (heads + 2 * heads + heads * dh)
    assert ws(1, 127) - ws(1, 126) == 4 * heads
    assert ws(0, 10) == 0 and ws(2, 0) == 0


def test_cached_direction_takes_wide_frames():
    """decode._XmDirection used to refuse context_chunk_size + 1 > 288 (NotImplementedError: generate() then recomputed the prefix); it
    now keeps a device-side first row instead of packed images for such frames, and is unchanged up to 287 rows.  Its buffers are plain
    tensors: built on the CPU here, nothing is launched"""
    from nuwa_pytorch_amd import decode
    from nuwa_pytorch_amd.video_audio import CrossModalityCrossAttention as X
    mk = lambda cc, **kw: X(**{**dict(dim=32, chunk_size=4, context_chunk_size=cc, heads=2, dim_head=32), **kw})
    wide = decode._XmDirection(mk(289), 2, 1 + 2 * 289, 'cpu', True)
    assert wide.long and wide.first.dtype == torch.int32 and tuple(wide.first.shape) == (1,) and not hasattr(wide, 'pk')
    assert tuple(wide.kv.hi.shape) == (2, 288 + 1 + 2 * 289, 2 * 64) and wide.kv.lo is not None
    short = decode._XmDirection(mk(287), 2, 1 + 2 * 287, 'cpu', True)
    assert not short.long and short.g.T == 287 and short.g.JP == 288 and tuple(short.corr.shape) == (2, 32)
    assert wide.needs_eager_row(0) and wide.needs_eager_row(1)            # the start token; the first row of a frame moves the window
    for bad in (mk(289, heads=9), mk(289, dim_head=48), mk(289, norm=True)):
        with pytest.raises(NotImplementedError):
            decode._XmDirection(bad, 2, 10, 'cpu', True)


def test_training_route_predicate_without_gpu(monkeypatch):
    """CrossModalityCrossAttention._long_hip_ok(batch * frames, chunk_size, context_chunk_size): more than 287 keys, the cattn kernels'
    precision modes and envelope, and the measured size gate (long_pairs_min, long_wgs_min: Attention's values)"""
    import nuwa_pytorch_amd as A
    from nuwa_pytorch_amd.video_audio import CrossModalityCrossAttention as X
    assert X.long_pairs_min == 1 << 23 and X.long_wgs_min == 128
    mk = lambda **kw: X(**{**dict(dim=32, chunk_size=4, context_chunk_size=289, heads=2, dim_head=32), **kw})
    prev = A.get_precision()
    try:
        A.set_precision('bf16')
        m = mk()
        assert m._long_hip_ok(1280, 32, 1024)
        assert not m._long_hip_ok(6, 4, 289) and not m._long_hip_ok(20, 4, 400)
        assert not m._long_hip_ok(1 << 20, 64, 287)
        monkeypatch.setattr(X, 'long_pairs_min', 0)
        monkeypatch.setattr(X, 'long_wgs_min', 0)
        assert m._long_hip_ok(6, 4, 289) and not m._long_hip_ok(6, 4, 287)
        assert not mk(heads=9)._long_hip_ok(6, 4, 289) and not mk(dim_head=48)._long_hip_ok(6, 4, 289)
        A.set_precision('bf16x3-fwd')
        assert m._long_hip_ok(6, 4, 289)
        A.set_precision('bf16x3')
        assert not m._long_hip_ok(6, 4, 289)                  # the parity mode keeps the torch-op formulation
    finally:
        A.set_precision(prev)


def test_module_on_cpu_tensors_keeps_the_torch_formulation():
    """off the GPU a wide frame runs the torch-op forward, whatever the gate: same numbers as the oracle"""
    import nuwa_pytorch_amd as A
    from nuwa_pytorch_amd.video_audio import CrossModalityCrossAttention as X
    from oracle import nuwa_oracle as O
    torch.manual_seed(0)
    m = X(dim=32, chunk_size=4, context_chunk_size=289, heads=2, dim_head=32)
    with torch.no_grad():
        m.talking_heads.bias.normal_(0, 0.3)
    x, ctx = torch.randn(2, 1 + 8, 32), torch.randn(2, 1 + 2 * 289, 32)
    with torch.no_grad():
        y = m(x, ctx)
    y_ref = O.cross_modality_cross_attention(x, ctx, dict(m.state_dict()), 2, 4, 289)
    assert float((y - y_ref).abs().max() / y_ref.abs().max()) <= 1e-5
    assert A.get_precision() in A.kernels.MODES
