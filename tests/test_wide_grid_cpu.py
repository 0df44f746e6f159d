"""Token grids wider than one workgroup row (W * heads * 4 > 512: the column-tiled window kernels) without a GPU: what
amdnuwa_s3_supported answers and what the amdnuwa_sparse3dna_* / amdnuwa_cross2dna_* entry points return before they touch the device.
The geometry check comes before the pointer check, so null operands tell the two apart: AMDNUWA_ERR_ARG (-1) = geometry accepted,
AMDNUWA_ERR_UNSUPPORTED (-2) = refused."""
import ctypes

import pytest

ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
WIDE = [(1, 17, 17, 8), (2, 20, 20, 8), (2, 32, 32, 8), (1, 64, 64, 8), (1, 40, 40, 4), (1, 48, 48, 3)]


def _geom(F, H, W, heads, dh=64, kernel=(3, 3, 3), dilation=(1, 1, 1), noncausal=0, B=2, ntok=None):
    from nuwa_pytorch_amd import _lib
    g = _lib.S3Geom()
    g.B, g.ntok = B, (1 + F * H * W if ntok is None else ntok)
    g.F, g.H, g.W = F, H, W
    g.kf, g.kh, g.kw = kernel
    g.df, g.dh, g.dw = dilation
    g.heads, g.dim_head, g.scale, g.noncausal = heads, dh, dh ** -0.5, noncausal
    return g


def _fwd(L, g, lo):
    """amdnuwa_sparse3dna_fwd with null operands (k_lo = a non-null marker in the hi + lo form: only compared with NULL before the
    operand check fails)"""
    k_lo = ctypes.c_void_p(16) if lo else None
    return L.amdnuwa_sparse3dna_fwd(ctypes.byref(g), None, None, None, None, k_lo, None, 64, None, None, None, 64, None)


def _bwd(L, g, lo):
    """amdnuwa_sparse3dna_bwd with non-null operand markers and a NULL workspace: nothing is dereferenced before the workspace check"""
    one = ctypes.c_void_p(16)
    x = one if lo else None
    return L.amdnuwa_sparse3dna_bwd(ctypes.byref(g), one, one, one, x, x, x, 64, one, one, x, 64, one, one, one, x, x, x, 64, one, 0, None, 0, None)


def _xfwd(L, g, lo):
    k_lo = ctypes.c_void_p(16) if lo else None
    return L.amdnuwa_cross2dna_fwd(ctypes.byref(g), None, None, 64, g.kf * g.H * g.W, None, None, k_lo, None, 64, None, None, None, None,
                                   None, None, None, None, 64, None)


def _xbwd(L, g, lo):
    one = ctypes.c_void_p(16)
    x = one if lo else None
    return L.amdnuwa_cross2dna_bwd(ctypes.byref(g), one, x, 64, g.kf * g.H * g.W, one, one, x, x, 64, one, x, one, x, None, one, one, x, 64,
                                   one, x, 64, one, one, x, x, 64, one, one, one, None, 0, None)


@pytest.mark.parametrize('lo', [0, 1])
@pytest.mark.parametrize('F,H,W,heads', WIDE)
def test_wide_grids_are_accepted(F, H, W, heads, lo):
    from nuwa_pytorch_amd import _lib
    L = _lib.lib()
    for dh in (32, 64):
        g = _geom(F, H, W, heads, dh=dh)
        assert L.amdnuwa_s3_supported(ctypes.byref(g), lo) == 1
        assert _fwd(L, g, lo) == ARG                                   # null operands, not an unsupported geometry
        assert _bwd(L, g, lo) in (ARG, WORKSPACE)
        assert L.amdnuwa_sparse3dna_bwd_workspace_bytes(ctypes.byref(g)) > 0
        # the symmetric window (sketch encoder) and SparseCross2DNA on the same map
        g = _geom(F, H, W, heads, dh=dh, noncausal=1)
        assert L.amdnuwa_s3_supported(ctypes.byref(g), lo) == 1
        assert _fwd(L, g, lo) == ARG
        gx = _geom(1, H, W, heads, dh=dh, kernel=(2, 3, 3), ntok=1 + H * W)
        assert L.amdnuwa_s3_supported(ctypes.byref(gx), lo) == 1
        assert _xfwd(L, gx, lo) == ARG
        assert _xbwd(L, gx, lo) in (ARG, WORKSPACE)
        assert L.amdnuwa_cross2dna_bwd_workspace_bytes(ctypes.byref(gx)) > 0


@pytest.mark.parametrize('lo', [0, 1])
def test_every_width_up_to_64_with_every_head_count(lo):
    """the required envelope: W 1..64, heads 1..8, dim_head 32 / 64 with the decoder's 3 x 3 x 3 window"""
    from nuwa_pytorch_amd import _lib
    L = _lib.lib()
    for W in range(1, 65):
        for heads in range(1, 9):
            for dh in (32, 64):
                g = _geom(1, 2, W, heads, dh=dh)
                assert L.amdnuwa_s3_supported(ctypes.byref(g), lo) == 1, (W, heads, dh)
                assert _fwd(L, g, lo) == ARG, (W, heads, dh)


@pytest.mark.parametrize('lo', [0, 1])
def test_what_stays_outside(lo):
    from nuwa_pytorch_amd import _lib
    L = _lib.lib()
    for g in (_geom(1, 65, 65, 8), _geom(1, 20, 20, 9), _geom(1, 20, 20, 8, dh=48), _geom(1, 65, 65, 3, noncausal=1)):
        assert L.amdnuwa_s3_supported(ctypes.byref(g), lo) == 0
        assert _fwd(L, g, lo) == UNSUPPORTED
        assert _bwd(L, g, lo) == UNSUPPORTED
        assert L.amdnuwa_sparse3dna_bwd_workspace_bytes(ctypes.byref(g)) == 0
    g = _geom(2, 16, 16, 8)                                            # the decoder's 16 x 16 map: as before
    assert L.amdnuwa_s3_supported(ctypes.byref(g), lo) == 1
    assert _fwd(L, g, lo) == ARG
    # fp16 forms and the MFMA band kernels stay with the 16-wide map
    for W in (17, 20, 32, 64):
        g = _geom(2, W, W, 8)
        assert L.amdnuwa_s3_f16_supported(ctypes.byref(g)) == 0
        assert L.amdnuwa_sparse3dna_bwd_f16_supported(ctypes.byref(g)) == 0


def test_lds_limit_is_that_of_the_launched_tile():
    """W 32, 8 x 64, kernel (5,5,5): a tile is 16 queries x 126 slots x 8 heads -> SP + DP are 126 KiB + 2 KiB of reduction space, plus the
    20 staged columns: 40 KiB as hi + lo pairs (168 KiB: over the 158 KiB budget), 20 KiB in bf16 (148 KiB: fits).  `_supported` and the
    entry points agree in both forms, for the sparse3dna pair and the cross2dna pair."""
    from nuwa_pytorch_amd import _lib
    L = _lib.lib()
    g = _geom(2, 32, 32, 8, kernel=(5, 5, 5))
    gx = _geom(1, 32, 32, 8, kernel=(5, 5, 5), ntok=1 + 32 * 32)
    assert L.amdnuwa_s3_supported(ctypes.byref(g), 1) == 0 and L.amdnuwa_s3_supported(ctypes.byref(gx), 1) == 0
    assert _fwd(L, g, 1) == UNSUPPORTED and _bwd(L, g, 1) == UNSUPPORTED
    assert _xfwd(L, gx, 1) == UNSUPPORTED and _xbwd(L, gx, 1) == UNSUPPORTED
    assert L.amdnuwa_s3_supported(ctypes.byref(g), 0) == 1 and L.amdnuwa_s3_supported(ctypes.byref(gx), 0) == 1
    assert _fwd(L, g, 0) == ARG and _bwd(L, g, 0) in (ARG, WORKSPACE)
    assert _xfwd(L, gx, 0) == ARG and _xbwd(L, gx, 0) in (ARG, WORKSPACE)
    for lo in (0, 1):
        # a halo as wide as a tile: 33 columns x 8 heads = 3 tiles of 11, kw 5 at dilation 4 -> 27 staged columns (108 KiB key side)
        g = _geom(2, 33, 33, 8, kernel=(3, 3, 5), dilation=(1, 1, 4))
        assert L.amdnuwa_s3_supported(ctypes.byref(g), lo) == 1
        assert _fwd(L, g, lo) == ARG and _bwd(L, g, lo) in (ARG, WORKSPACE)
        # a halo that no LDS holds: 400 columns
        g = _geom(2, 32, 32, 8, kernel=(3, 3, 3), dilation=(1, 1, 200))
        assert L.amdnuwa_s3_supported(ctypes.byref(g), lo) == 0
        assert _fwd(L, g, lo) == UNSUPPORTED and _bwd(L, g, lo) == UNSUPPORTED


def test_workspace_counts_one_partial_per_row_and_tile():
    """ds + P' [B][nq][J][heads] fp32, then heads^2 + 2 * inner floats of partials per (row, tile) workgroup: 32 columns x 8 heads = 2 tiles"""
    from nuwa_pytorch_amd import _lib
    L = _lib.lib()
    B, F, H, W, heads, dh, J = 2, 2, 32, 32, 8, 64, 28
    g = _geom(F, H, W, heads, dh=dh, B=B)
    nq, inner, parts = F * H * W, heads * dh, B * F * H * 2
    want = (2 * B * nq * J * heads + parts * heads * heads + 2 * parts * inner) * 4 + 256 + L.amdnuwa_colsum_workspace_bytes(B * nq, J * heads)
    assert L.amdnuwa_sparse3dna_bwd_workspace_bytes(ctypes.byref(g)) == want
