"""Attention dropout inside the Sparse3DNA MFMA band kernels, without a GPU: the two fp16-form entry points
(amdnuwa_sparse3dna_fwd_f16_drop / _bwd_f16_drop) are declared, exported and refuse bad arguments before they touch the device, and
ops.S3Inner.plan gives a block with live attention dropout the plan of its dropout-free twin at band geometry (16-wide grid, 8 heads x 64)
and the bare plan everywhere else.  The plans are built the way tests/test_block_plan_cpu.py builds them."""
import ctypes
import math

import pytest
import torch

from nuwa_pytorch_amd import kernels as K, nuwa_pytorch as NP, ops
from test_block_plan_cpu import apply_switch

OK, ARG, UNSUPPORTED = 0, -1, -2
DIM = 512


def _geom(F, H, W, heads, dh=64, kernel=(3, 3, 3), dilation=(1, 1, 1), noncausal=0, B=2):
    from nuwa_pytorch_amd import _lib
    g = _lib.S3Geom()
    g.B, g.ntok = B, 1 + F * H * W
    g.F, g.H, g.W = F, H, W
    g.kf, g.kh, g.kw = kernel
    g.df, g.dh, g.dw = dilation
    g.heads, g.dim_head, g.scale = heads, dh, dh ** -0.5
    g.rel_bias, g.d_rel_bias, g.noncausal = None, None, noncausal
    return g


def _fwd16(L, g, keep, scale):
    return L.amdnuwa_sparse3dna_fwd_f16_drop(ctypes.byref(g), None, None, None, 1536, None, None, None, 512, 0, keep, scale, None)


def _bwd16(L, g, keep, scale):
    return L.amdnuwa_sparse3dna_bwd_f16_drop(ctypes.byref(g), None, None, None, 1536, None, None, 512, None, None, None, 1536, None, 0,
                                             None, None, 0, keep, scale, None)


def test_f16_drop_entry_points_are_declared_and_exported():
    """fails on the parent commit: the symbols do not exist"""
    from nuwa_pytorch_amd import _lib
    hdr = open(_lib.HERE + '/../include/amdnuwa.h').read()
    so = ctypes.CDLL(_lib.lib()._name)
    for name, base in (('amdnuwa_sparse3dna_fwd_f16_drop', 'amdnuwa_sparse3dna_fwd_f16'), ('amdnuwa_sparse3dna_bwd_f16_drop', 'amdnuwa_sparse3dna_bwd_f16')):
        assert name in _lib.SIGNATURES and f'int {name}(' in hdr and hasattr(so, name)
        res, args = _lib.SIGNATURES[name]
        bres, bargs = _lib.SIGNATURES[base]
        # the arguments of the unmasked call, then keep and drop_scale in front of the stream
        assert res is bres and args[:-1] == bargs[:-1] + [ctypes.c_void_p, ctypes.c_float] and args[-1] is bargs[-1]
    assert _lib.ABI_VERSION == _lib.lib().amdnuwa_abi_version()                      # additive entry points: the version agrees everywhere


def test_f16_drop_entry_points_check_their_arguments_before_the_device():
    """fails on the parent commit: the symbols do not exist.  Null operands throughout: nothing here can reach a launch"""
    from nuwa_pytorch_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(32)
    some = ctypes.c_void_p((ctypes.addressof(buf) + 7) & ~7)                         # a non-null, 8-byte aligned keep pointer: never dereferenced
    band = _geom(2, 16, 16, 8)
    assert L.amdnuwa_s3_f16_supported(ctypes.byref(band)) == 1 and L.amdnuwa_sparse3dna_bwd_f16_supported(ctypes.byref(band)) == 1
    for call in (_fwd16, _bwd16):
        assert call(L, band, None, 1.25) == ARG                                      # keep == NULL
        for bad in (0.5, math.inf, -math.inf, math.nan, 0.0, 0.999):
            assert call(L, band, some, bad) == ARG, bad                              # drop_scale not finite or < 1
        assert call(L, band, some, 1.25) == ARG                                      # accepted so far: the null operands are refused next
    # outside the band kernels' geometry: refused as the unmasked fp16 calls refuse it, before any argument is looked at
    refused = [_geom(2, 4, 4, 2, dh=32), _geom(1, 3, 20, 8, dh=32), _geom(2, 16, 16, 4), _geom(2, 16, 16, 8, dh=32), _geom(2, 16, 16, 8, noncausal=1),
               _geom(2, 16, 16, 8, kernel=(3, 3, 5)), _geom(33, 1, 1, 8, kernel=(7, 1, 1))]
    for g in refused:
        assert L.amdnuwa_s3_f16_supported(ctypes.byref(g)) == 0
        for keep, scale in ((some, 1.25), (None, 1.25), (some, 0.5)):
            assert _fwd16(L, g, keep, scale) == UNSUPPORTED and _bwd16(L, g, keep, scale) == UNSUPPORTED
    # the fp16-gradient backward takes no relative-position bias, masked or not
    rel = _geom(2, 16, 16, 8)
    rel.rel_bias = ctypes.cast(buf, ctypes.c_void_p)
    assert L.amdnuwa_sparse3dna_bwd_f16_supported(ctypes.byref(rel)) == 0 and _bwd16(L, rel, some, 1.25) == UNSUPPORTED
    # the bf16 masked entry points keep their checks at band geometry (a masked band launch reads the mask as 8-byte words: a misaligned one is
    # an argument error, here hidden behind the null operands)
    assert L.amdnuwa_s3_drop_supported(ctypes.byref(band), 0) == 1


def _s3_plan(vs, heads, dh, mode, dropout, train=True, rel=False):
    m = NP.Sparse3DNA(dim=DIM, video_shape=vs, kernel_size=(3, 3, 3), dilation=1, heads=heads, dim_head=dh, causal=True, rel_pos_bias=rel, dropout=dropout)
    m.train(train)
    B, n = 1, vs[0] * vs[1] * vs[2]
    own, p = dict(m._meta(B, n, 'cpu')), m._plan_params()
    own['shift'] = None                        # (what SandwichBlockFn.forward does to its meta before it plans)
    with apply_switch(mode, ''):
        plan = ops.block_plan('s3', B * n, DIM, p, own)
    return plan, own, m


@pytest.mark.parametrize('mode', ['bf16x3-fwd', 'bf16', 'bf16x3'])
def test_plan_with_dropout_at_band_geometry_is_the_dropout_free_plan(monkeypatch, mode):
    """(2, 16, 16), 8 x 64, kernel 3, drop_p = 0.05: field for field the plan without drop_p.  In 'bf16x3-fwd' that is the fp16-gradient
    plan, which the parent commit replaces by the bare one (this case fails there)"""
    monkeypatch.setattr(ops, 'f16_weights_ok', lambda *ws: True)          # (the weights' fp16 range verdict, as test_block_plan_cpu.py sets it)
    torch.manual_seed(0)
    drop, meta, m = _s3_plan((2, 16, 16), 8, 64, mode, 0.05)
    assert meta['drop_p'] == pytest.approx(0.05) and K.s3_f16_supported(meta['geom'])
    plain, meta0, m0 = _s3_plan((2, 16, 16), 8, 64, mode, 0.0)
    assert 'drop_p' not in meta0
    for f in ops.Plan._fields:
        if f != 'guarded':
            assert getattr(drop, f) == getattr(plain, f), f
    assert [id(w) for w in drop.guarded] == [id(w) for w in (m.to_q.weight, m.to_kv.weight, m.to_out.weight)] and len(plain.guarded) == 3
    if mode == 'bf16x3-fwd':
        assert drop[:2] == ('only', True) and drop.a16 and drop.core16 and drop.o16 == 'only'
    else:
        assert drop[:2] == (False, False) and not drop.a16 and not drop.core16 and not drop.o16


@pytest.mark.parametrize('heads,dh,vs', [(2, 32, (2, 16, 16)), (8, 64, (4, 8, 8))])
def test_plan_with_dropout_off_band_geometry_stays_bare(monkeypatch, heads, dh, vs):
    monkeypatch.setattr(ops, 'f16_weights_ok', lambda *ws: True)
    torch.manual_seed(0)
    drop, meta, m = _s3_plan(vs, heads, dh, 'bf16x3-fwd', 0.05)
    assert meta['drop_p'] == pytest.approx(0.05) and not K.s3_f16_supported(meta['geom'])
    bare = ops.Plan(guarded=drop.guarded)
    assert drop == bare and len(drop.guarded) == 3
    # eval mode carries no drop_p at all
    _, meta_e, _ = _s3_plan(vs, heads, dh, 'bf16x3-fwd', 0.05, train=False)
    assert 'drop_p' not in meta_e
