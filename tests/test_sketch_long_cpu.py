"""NUWASketch.generate past max_video_frames without a GPU: the rows form of the single-query SparseCross2DNA kernel
(amdnuwa_cross2dna_rows, csrc/decode.hip) is exported, declared and registered, its argument checks answer before anything is launched
(arguments, then the envelope, then the workspace), its workspace follows the formula of the header, the ABI version is unchanged, and
the class switch that routes the long call onto the cached row program is on."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
SPLIT = 128
CHUNK = 2048                      # query rows per set of launches: the workspace is that of one chunk


@pytest.fixture(scope='module')
def L():
    from nuwa_pytorch_amd import _lib
    return _lib.lib()


def _call(L, B=2, R=33, J=300, heads=8, dh=64, ptr=ctypes.c_void_p(16), ws=ctypes.c_void_p(16), ws_bytes=1 << 40, **over):
    """argument list of amdnuwa_cross2dna_rows with every pointer `ptr` (never dereferenced on the host); over: name -> value"""
    inner = heads * dh
    a = dict(B=B, R=R, J=J, heads=heads, dim_head=dh, scale=dh ** -0.5, q=ptr, q_lo=None, ldq=inner, kv=ptr, kv_lo=None, ctx_rows=192,
             slot_rows=ptr, n_pos=16, key_mask=None, null_k=ptr, null_v=ptr, w_th=ptr, o=ptr, o_lo=None, ldo=inner, workspace=ws,
             workspace_bytes=ws_bytes, stream=None)
    assert not set(over) - set(a), over
    a.update(over)
    return L.amdnuwa_cross2dna_rows(*a.values())


def test_entry_points_are_exported_declared_and_registered(L):
    from nuwa_pytorch_amd import _lib
    from nuwa_pytorch_amd import kernels as K
    header = open(os.path.join(ROOT, 'include', 'amdnuwa.h')).read()
    for name in ('amdnuwa_cross2dna_rows', 'amdnuwa_cross2dna_rows_workspace_bytes'):
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES
        assert re.search(r'\b' + name + r'\s*\(', header), name
    assert callable(K.cross2dna_rows) and K.CROSS2DNA_ROWS_CHUNK == CHUNK
    assert L.amdnuwa_abi_version() == 21                      # purely additive


def test_argument_checks_answer_before_any_launch(L):
    assert _call(L, ptr=None) == ARG
    for name in ('q', 'kv', 'slot_rows', 'null_k', 'null_v', 'w_th', 'o'):
        assert _call(L, **{name: None}) == ARG, name
    for name in ('B', 'R', 'J', 'n_pos', 'ctx_rows'):
        for v in (0, -3):
            assert _call(L, **{name: v}) == ARG, (name, v)
    lo = ctypes.c_void_p(32)
    for one_side in ('q_lo', 'kv_lo', 'o_lo'):                # the lo images come together or not at all
        assert _call(L, **{one_side: lo}) == ARG, one_side
    assert _call(L, q_lo=lo, o_lo=lo) == ARG and _call(L, kv_lo=lo, o_lo=lo) == ARG and _call(L, q_lo=lo, kv_lo=lo) == ARG
    assert _call(L, ldq=8) == ARG and _call(L, ldo=8) == ARG
    assert _call(L, heads=9) == UNSUPPORTED
    assert _call(L, dh=48) == UNSUPPORTED
    need = L.amdnuwa_cross2dna_rows_workspace_bytes(2, 33, 300, 8, 64)
    assert _call(L, ws_bytes=need - 1) == WORKSPACE
    assert _call(L, ws=None) == WORKSPACE
    assert _call(L, ws_bytes=16) == WORKSPACE
    assert _call(L, q_lo=lo, kv_lo=lo, o_lo=lo, ws_bytes=16) == WORKSPACE      # all three lo images: past the argument checks
    # arguments first, the envelope second, the workspace last
    assert _call(L, heads=9, q=None) == ARG and _call(L, dh=48, n_pos=0) == ARG and _call(L, heads=9, dh=48, kv_lo=lo) == ARG
    assert _call(L, heads=9, R=0) == ARG
    assert _call(L, heads=9, ws=None, ws_bytes=0) == UNSUPPORTED
    # R = 1 is <bos> alone, the caller's row: OK without a launch and without a workspace -- but after the checks
    assert _call(L, R=1, ws=None, ws_bytes=0) == OK
    assert _call(L, R=1, q=None) == ARG and _call(L, R=1, heads=9) == UNSUPPORTED


@pytest.mark.parametrize('heads,dh', [(8, 64), (3, 64), (1, 32), (5, 32)])
def test_workspace_follows_the_documented_formula(L, heads, dh):
    """4 * min(B * R, 2048) * (heads * (J + 1) + splits * (2 * heads + heads * dim_head)) bytes, splits = ceil((J + 1) / 128): the single-row
    formula with the query rows of one chunk in place of B"""
    ws = lambda B, R, J: L.amdnuwa_cross2dna_rows_workspace_bytes(B, R, J, heads, dh)
    for B, R in ((1, 2), (2, 17), (3, 40), (2, 33), (2, 1024), (2, 1025), (32, 2305), (65600, 2)):
        for J in (1, 24, 127, 128, 300):
            splits = -(-(J + 1) // SPLIT)
            rows = min(B * R, CHUNK)
            assert ws(B, R, J) == 4 * rows * (heads * (J + 1) + splits * (2 * heads + heads * dh)), (B, R, J)
            assert ws(B, R, J) == L.amdnuwa_cross2dna_decode_workspace_bytes(rows, J, heads, dh)
    assert ws(0, 5, 10) == 0 and ws(2, 0, 10) == 0 and ws(2, 5, 0) == 0


def test_sketch_generate_slides_on_the_cached_path_by_default():
    from nuwa_pytorch_amd import NUWA, NUWASketch
    assert NUWASketch.generate_slide_cache is True
    assert NUWA.generate_slide_cache is True
    assert NUWASketch._sample_video is NUWA._sample_video    # the one token loop
