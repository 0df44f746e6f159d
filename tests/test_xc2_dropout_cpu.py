"""Attention dropout inside SparseCross2DNA, without a GPU: the restatement of tests/xc2_dropout_util.py against the oracle and against
the module's PyTorch-op formulation with a fixed mask, the routing predicates of the module (train / eval, p, dropout_on_kernels, what
the library answers), and what amdnuwa_cross2dna_fwd_drop / _bwd_drop return before they launch anything.

Bound of the module comparison: module and restatement are two fp32 formulations of the same sums of at most a few hundred products per
output element on O(1) data: 1e-5 of the largest reference value (fp32 eps 6e-8 x the roundings on the way, with room), max-abs error over
max-abs reference as gpu_util.rel_err -- the bound of tests/test_attn_dropout_cpu.py for the same kind of comparison."""
import ctypes

import pytest
import torch

import test_s3_entry_contract_cpu as T
import xc2_dropout_util as XU
from attn_dropout_util import FixedMaskDropout
from gpu_util import rel_err

TOL = 1e-5


@pytest.fixture(scope='module')
def O():
    from oracle import nuwa_oracle
    return nuwa_oracle


def _inputs(fmap, heads, dh, kernel, frames, n, dim=32, seed=0, masked=True):
    from nuwa_pytorch_amd.nuwa_pytorch import SparseCross2DNA
    torch.manual_seed(seed)
    m = SparseCross2DNA(dim=dim, image_size=fmap, heads=heads, dim_head=dh, kernel_size=kernel, dilation=1, dropout=0.25)
    Tn = frames * fmap * fmap
    g = torch.Generator().manual_seed(seed + 1)
    x, ctx = torch.randn(2, n, dim, generator=g), torch.randn(2, Tn, dim, generator=g)
    cmask = torch.rand(2, Tn, generator=g) > 0.3 if masked else None
    keep = torch.rand(2, n - 1, frames * kernel * kernel + 1, heads, generator=g) >= 0.25          # kernel order
    return m, x, ctx, cmask, keep


# ---------------------------------------------------------------------------------------------------
# 1. the restatement
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('fmap,heads,dh,kernel,dil,frames,n', [(4, 2, 8, 3, 1, 2, 1 + 3 * 16), (4, 2, 8, 3, 2, 2, 1 + 21), (5, 3, 8, 5, 1, 1, 1 + 25 + 9)])
def test_restatement_with_a_full_mask_is_the_oracle(O, fmap, heads, dh, kernel, dil, frames, n):
    m, x, ctx, cmask, _ = _inputs(fmap, heads, dh, kernel, frames, n)
    P = {k: v.detach().clone() for k, v in m.state_dict().items()}
    tpf, J = fmap * fmap, frames * kernel * kernel + 1
    ones = XU.keep_to_bgfij(torch.ones(2, n - 1, J, heads), tpf)
    for cm in (cmask, None):
        want = O.sparse_cross_2dna(x, ctx, P, heads, fmap, kernel, dil, context_mask=cm)
        assert torch.equal(XU.sparse_cross_2dna_drop(x, ctx, P, heads, fmap, kernel, dil, ones, 1.0, context_mask=cm), want)
    # a mask does what nn.Dropout does to the mixed map: a fully dropped query outputs 0 in front of to_out, and the <bos> row ignores it
    keep = torch.ones(2, n - 1, J, heads)
    keep[1, 3] = 0
    eye = {**P, 'to_out.weight': torch.eye(heads * dh)}
    got = XU.sparse_cross_2dna_drop(x, ctx, eye, heads, fmap, kernel, dil, XU.keep_to_bgfij(keep, tpf), 2.0, context_mask=cmask)
    ref = O.sparse_cross_2dna(x, ctx, eye, heads, fmap, kernel, dil, context_mask=cmask)
    assert bool((got[1, 4] == 0).all()) and torch.equal(got[:, 0], ref[:, 0]) and torch.equal(got[0, 1:], ref[0, 1:] * 2.0)


def test_float64_core_restatement_with_a_full_mask_is_peaked_utils():
    """cross2dna_core_drop64 (the reference of the GPU kernel test) is peaked_util.cross2dna_core64 when nothing is dropped"""
    import peaked_util as PU
    from attn_dropout_util import keep_to_bhij
    fmap, kern, dil, frames, heads, dh, n = 4, 3, 2, 2, 2, 8, 1 + 21
    g = torch.Generator().manual_seed(3)
    q, k, v = (torch.randn(2, m_, heads, dh, generator=g).double() for m_ in (n, frames * 16, frames * 16))
    nk, nv, wth = torch.randn(heads, dh, generator=g).double(), torch.randn(heads, dh, generator=g).double(), torch.randn(heads, heads, generator=g).double()
    mask = torch.rand(2, frames * 16, generator=g) > 0.3
    idx, valid = PU.cross2dna_window(fmap, kern, dil, frames, n)
    want = PU.cross2dna_core64(q, k, v, nk, nv, wth, mask, idx, valid, dh ** -0.5)
    ones = keep_to_bhij(torch.ones(2, n - 1, frames * kern * kern + 1, heads))
    assert torch.equal(XU.cross2dna_core_drop64(q, k, v, nk, nv, wth, mask, idx, valid, dh ** -0.5, ones, 1.0), want)
    keep = torch.ones(2, n - 1, frames * kern * kern + 1, heads)
    keep[0, 5] = 0
    got = XU.cross2dna_core_drop64(q, k, v, nk, nv, wth, mask, idx, valid, dh ** -0.5, keep_to_bhij(keep), 2.0)
    assert bool((got[0, 5] == 0).all()) and torch.equal(got[1], want[1] * 2.0)


def test_mask_layout():
    keep = torch.rand(2, 21, 19, 3) > 0.5                     # kernel order [B, nq, J, heads]; 21 queries on a 4 x 4 map: 2 query frames
    k5 = XU.keep_to_bgfij(keep, 16)
    assert k5.shape == (2, 3, 2, 16, 19)
    assert bool(k5[1, 2, 1, 4, 6] == keep[1, 16 + 4, 6, 2]) and bool(k5[0, 1, 0, 15, 0] == keep[0, 15, 0, 1])
    assert bool(k5[:, :, 1, 5:].all())                         # the padding rows


@pytest.mark.parametrize('fmap,heads,dh,kernel,frames,n,masked', [(4, 2, 8, 3, 2, 1 + 3 * 16, True), (4, 2, 8, 3, 2, 1 + 21, False),
                                                                    (5, 3, 8, 5, 1, 1 + 25 + 9, True)])
def test_restatement_equals_the_torch_formulation_under_a_fixed_mask(fmap, heads, dh, kernel, frames, n, masked):
    """sparse_cross_2dna_drop == SparseCross2DNA._forward_torch with FixedMaskDropout of the same mask, forward and every gradient"""
    m, x, ctx, cmask, keep = _inputs(fmap, heads, dh, kernel, frames, n, masked=masked)
    s = 1.0 / 0.75
    k5 = XU.keep_to_bgfij(keep, fmap * fmap)
    m.dropout = FixedMaskDropout(k5, s)
    m.train()
    xm, cm_ = x.clone().requires_grad_(True), ctx.clone().requires_grad_(True)
    y = m._forward_torch(xm, context=cm_, context_mask=cmask)
    dy = torch.randn(y.shape, generator=torch.Generator().manual_seed(5))
    y.backward(dy)
    assert m.dropout.calls == 1
    P = {k: v.detach().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    xr, cr = x.clone().requires_grad_(True), ctx.clone().requires_grad_(True)
    yr = XU.sparse_cross_2dna_drop(xr, cr, P, heads, fmap, kernel, 1, k5, s, context_mask=cmask)
    yr.backward(dy)
    errs = {'y': rel_err(y, yr), 'dx': rel_err(xm.grad, xr.grad), 'dctx': rel_err(cm_.grad, cr.grad)}
    for k, p in m.named_parameters():
        errs['grad.' + k] = rel_err(p.grad, P[k].grad)
    print(errs)
    assert len(errs) == 9 and all(e <= TOL for e in errs.values()), errs


# ---------------------------------------------------------------------------------------------------
# 2. routing predicates
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('answer', [True, False])
def test_hip_ok_follows_cross2dna_drop_supported_in_training(monkeypatch, answer):
    """library stubbed: in train mode with p > 0 the module asks cross2dna_drop_supported (for the window's geometry, in the current
    precision mode) and nothing else; dropout_on_kernels = False answers False without asking; eval / p = 0 ask s3_supported as before"""
    from nuwa_pytorch_amd import kernels as K
    from nuwa_pytorch_amd.nuwa_pytorch import SparseCross2DNA
    asked = dict(drop=[], plain=[])
    monkeypatch.setattr(K, 'cross2dna_drop_supported', lambda g, lo=None: (asked['drop'].append((g.F, g.H, g.W, g.kf, g.kh, g.kw, g.dh, g.dw, g.heads, g.dim_head, lo)), answer)[1])
    monkeypatch.setattr(K, 's3_supported', lambda *a, **k: (asked['plain'].append((a, k)), not answer)[1])
    m = SparseCross2DNA(dim=32, image_size=4, heads=2, dim_head=32, kernel_size=3, dilation=2, dropout=0.25).train()
    assert SparseCross2DNA.dropout_on_kernels is True
    assert m._hip_ok(32) is answer
    assert asked['drop'] == [(1, 4, 4, 2, 3, 3, 2, 2, 2, 32, None)] and not asked['plain']
    assert m._hip_ok(0) is False and m._hip_ok(33) is False and len(asked['drop']) == 1       # not whole sketch frames: nobody is asked
    m.dropout_on_kernels = False                                                             # the A/B switch: today's torch-op route
    assert m._hip_ok(32) is False and len(asked['drop']) == 1 and not asked['plain']
    m.dropout_on_kernels = True
    m.eval()
    assert m._hip_ok(32) is (not answer) and len(asked['plain']) == 1 and len(asked['drop']) == 1
    m.train()
    m.dropout.p = 0.0
    assert m._hip_ok(32) is (not answer) and len(asked['plain']) == 2 and len(asked['drop']) == 1


def test_hip_ok_and_meta_with_the_library_loaded():
    from nuwa_pytorch_amd import kernels as K
    from nuwa_pytorch_amd.nuwa_pytorch import SparseCross2DNA
    x, ctx = torch.zeros(2, 1 + 21, 32), torch.zeros(2, 32, 32)
    m = SparseCross2DNA(dim=32, image_size=4, heads=2, dim_head=32, kernel_size=3, dropout=0.25).train()
    assert m._hip_ok(32) is True
    meta = m._meta(2, 22, x.device, context=ctx)
    assert meta['drop_p'] == 0.25 and meta['kind'] == 'xc2'
    g = meta['geom']
    assert K.cross2dna_drop_supported(g, lo=False) and K.cross2dna_drop_supported(g, lo=True)
    # drop_p only while the mask is live
    m.dropout_on_kernels = False
    assert 'drop_p' not in m._meta(2, 22, x.device, context=ctx) and m._hip_ok(32) is False
    m.dropout_on_kernels = True
    assert 'drop_p' not in m.eval()._meta(2, 22, x.device, context=ctx) and m._hip_ok(32) is True
    m.train().dropout.p = 0.0
    assert 'drop_p' not in m._meta(2, 22, x.device, context=ctx) and m._hip_ok(32) is True
    # a head size the kernels do not take: the torch-op route, with or without dropout
    m48 = SparseCross2DNA(dim=32, image_size=4, heads=2, dim_head=48, kernel_size=3, dropout=0.25).train()
    assert m48._hip_ok(32) is False and m48.eval()._hip_ok(32) is False
    # the window at the LDS limit (tests/test_gpu_modules.py::test_sparse_cross_2dna_window_at_the_lds_limit): the masked forms follow it
    big = SparseCross2DNA(dim=64, image_size=16, heads=8, dim_head=64, kernel_size=5, dropout=0.25).train()
    import nuwa_pytorch_amd as A
    try:
        for mode, ok_frames, bad_frames in (('bf16', 5, 6), ('bf16x3', 4, 5)):
            A.set_precision(mode)
            assert big._hip_ok(ok_frames * 256) is True and big._hip_ok(bad_frames * 256) is False
            assert big.eval()._hip_ok(ok_frames * 256) is True and big._hip_ok(bad_frames * 256) is False
            big.train()
    finally:
        A.set_precision('bf16')


def test_sandwich_norm_fuses_the_block_with_live_dropout():
    from nuwa_pytorch_amd.nuwa_pytorch import SandwichNorm, SparseCross2DNA
    sn = SandwichNorm(dim=32, fn=SparseCross2DNA(dim=32, image_size=4, heads=2, dim_head=32, kernel_size=3, dropout=0.25)).train()
    ctx = torch.zeros(2, 32, 32)
    assert sn._inner(ctx, seq_len=22) == (sn.fn, None)
    sn.fn.dropout_on_kernels = False
    assert sn._inner(ctx, seq_len=22) is None


# ---------------------------------------------------------------------------------------------------
# 3. entry contract of the two masked entries
# ---------------------------------------------------------------------------------------------------

def test_supported_query_answers_as_s3_supported():
    L = T._L()
    n = 0
    for fn, gname, gkw, extra, want in T.QUERIES:
        if fn != 'amdnuwa_s3_supported':
            continue
        g = T.geom(gname, **gkw) if gname is not None else None
        assert L.amdnuwa_cross2dna_drop_supported(ctypes.byref(g) if g is not None else None, *extra) == want, (gname, gkw, extra)
        n += 1
    assert n == 22


@pytest.mark.parametrize('entry', sorted(XU.DROP_OF))
def test_masked_cross_entries_return_what_the_unmasked_ones_return(entry):
    """every cross case of the table, with a valid mask (keep non-null, drop_scale 1.25): the code of the unmasked entry"""
    L = T._L()
    plain = XU.DROP_OF[entry]
    rows = [(c, want) for e, c, want in T.TABLE if e == plain]
    assert len(rows) >= 35
    got = []
    for case, want in rows:
        gname, gkw, over = T.CASES[case]
        g = T.geom(gname, **gkw) if gname is not None else None
        assert want != T.OK or g.B <= 0, 'a case may not reach a launch'
        assert T.call(L, plain, g, over) == want                     # (the unmasked entry keeps its code)
        got.append((case, XU.call_drop(T, L, entry, g, over)))
    assert got == rows


@pytest.mark.parametrize('entry', sorted(XU.DROP_OF))
def test_mask_checks_of_the_masked_cross_entries(entry):
    """keep NULL / drop_scale not finite or < 1: ARG, behind the geometry and UNSUPPORTED answers, in front of the workspace one, at B = 0 too"""
    L = T._L()
    names = set(XU.drop_params(T)[entry].split())
    got, want_all = [], []
    for name, gname, gkw, over, want in XU.MASK_CASES:
        if not all(n in names or n == 'all_lo' or (n == 'ws_short' and 'workspace' in names) for n in over):
            continue
        g = T.geom(gname, **gkw)
        assert want != XU.OK or g.B <= 0, 'a case may not reach a launch'
        got.append((name, XU.call_drop(T, L, entry, g, over)))
        want_all.append((name, want))
    assert got == want_all and len(got) == (15 if 'workspace' in names else 13)


def test_wrappers_validate_the_mask_before_the_library(monkeypatch):
    """K.cross2dna_fwd / _bwd: a mask of the wrong shape or dtype is a ValueError (no device needed: the check precedes every allocation
    that matters -- here everything lives on the CPU and the library is never reached)"""
    from nuwa_pytorch_amd import kernels as K
    g = K.s3_geom(2, 22, (2, 4, 4), (2, 3, 3), (1, 1, 1), 2, 32, causal=False)
    q = K.BF(torch.zeros(44, 64, dtype=torch.bfloat16), None)
    kv = K.BF(torch.zeros(64, 128, dtype=torch.bfloat16), None)
    nul = K.BF(torch.zeros(64, dtype=torch.bfloat16), None)
    wth = torch.eye(2)
    monkeypatch.setattr(K, '_s3_call', lambda *a, **k: pytest.fail('the library was reached'))
    for bad in (torch.ones(2, 21, 19, 3, dtype=torch.bool), torch.ones(2, 22, 19, 2, dtype=torch.bool), torch.ones(2, 21, 19, 2)):
        with pytest.raises(ValueError):
            K.cross2dna_fwd(g, q, kv, nul, nul, None, wth, 32, keep=bad, drop_scale=1.25)
        with pytest.raises(ValueError):
            K.cross2dna_bwd(g, q, kv, nul, nul, None, wth, q, 32, keep=bad, drop_scale=1.25)
