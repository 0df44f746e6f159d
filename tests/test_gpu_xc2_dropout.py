"""Attention dropout inside the SparseCross2DNA kernels on the MI355X: the masked forms of the VALU window kernels under S3Args::xmode
(amdnuwa_cross2dna_fwd_drop / _bwd_drop; row and column-tiled, bf16 and hi + lo operands) against the float64 restatement of
tests/xc2_dropout_util.py, then SparseCross2DNA in training (stand-alone and fused into a SandwichNorm) and a tiny NUWASketch with the
README's dropout switches, plain and reversible.  Every run is forward + backward at B = 2 under guard_util.guard.

Metric: gpu_util.report (max-abs error / max-abs reference).  Kernel bounds are those test_gpu_guarded_buffers.py::
test_cross2dna_operands_in_guarded_buffers applies to the same kernels without a mask: 2e-2 forward / 7e-2 gradients in bf16, 1e-3 / 2e-3
as hi + lo pairs.  The mask only scales entries by 0 or 1 / (1 - p); the reference carries the same factor, so the relative bounds are
unchanged.  Module bounds: the MODES of test_gpu_modules.py.

Measured on an MI355X (the largest of the four cases; the test prints each case's figures):
    bf16      o 4.1e-3   dq 3.7e-3   dk 3.5e-3   dv 3.7e-3   d_null_k 1.9e-7   d_null_v 1.4e-7   dW_th 2.9e-7
    hi + lo   o 5.9e-6   dq 5.9e-6   dk 5.9e-6   dv 6.0e-6   d_null_k 3.3e-7   d_null_v 1.6e-7   dW_th 2.4e-7"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import peaked_util as PU  # noqa: E402
import xc2_dropout_util as XU  # noqa: E402
from attn_dropout_util import keep_to_bhij  # noqa: E402
from gpu_util import report, to_bf_pair, bf_value  # noqa: E402
from guard_util import guard, guarded  # noqa: E402
from test_gpu_modules import MODES, SKETCH_KW  # noqa: E402

DEV = 'cuda'
P_DROP = 0.25
S = 1.0 / (1.0 - P_DROP)
B_ = 2


@pytest.fixture(scope='module')
def A():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import nuwa_pytorch_amd
    return nuwa_pytorch_amd


@pytest.fixture(scope='module')
def K(A):
    from nuwa_pytorch_amd import kernels
    return kernels


# ---------------------------------------------------------------------------------------------------
# 1. kernels
# ---------------------------------------------------------------------------------------------------

# name: (fmap, kernel, dilation, sketch frames, heads, dim_head, n, key mask)
# X1: row kernel, the smallest shape of peaked_util.XC2_SHAPES, 30 % of the keys hidden; X2: dilation, the sequence ends inside a frame,
# sample 1's context fully hidden (the conditioning-dropout case: only the null slot is left); X3: J = 26, more query frames than sketch
# frames; X4: 20 columns x 8 heads = 640 threads, two column tiles of 10 (sparse3dna_wide.hip)
CASES = {
    'X1': (4, 3, 1, 2, 2, 32, 1 + 3 * 16, 'rand'),
    'X2': (4, 3, 2, 2, 2, 32, 1 + 21, 'sample1'),
    'X3': (8, 5, 1, 1, 8, 64, 1 + 64 + 9, None),
    'X4': (20, 3, 1, 2, 8, 32, 1 + 3 * 20, 'rand'),
}
assert CASES['X1'][:7] == PU.XC2_SHAPES[0]


def _geom(K, case):
    fmap, kern, dil, frames, heads, dh, n, _ = CASES[case]
    return K.s3_geom(B_, n, (-(-(n - 1) // (fmap * fmap)), fmap, fmap), (frames, kern, kern), (1, dil, dil), heads, dh, causal=False)


def _mask(case, ones=False):
    """kernel-order keep mask [B, nq, J, heads], built as test_gpu_attn_dropout._mask: Bernoulli(0.75) from a fixed generator, query row
    r0 = nq // 3 of sample 0 fully dropped, (sample 1, query r1 = 2 nq // 3, head 1) with only the null slot kept.  At X4 (nq = 60 on rows
    of 20 columns) both r0 = 20 and r1 = 40 are column 0 of their row, i.e. the FIRST column tile; so X4 drops one more query in full,
    r0 + 13 of sample 0 (column 13: the second tile), and keeps only the null slot at (sample 1, r1 + 13, head 1) as well.
    Returns (keep, fully dropped queries of sample 0, null-only queries of sample 1)."""
    fmap, kern, _, frames, heads, _, n, _ = CASES[case]
    nq, J = n - 1, frames * kern * kern + 1
    if ones:
        return torch.ones(B_, nq, J, heads, dtype=torch.bool), [], []
    g = torch.Generator().manual_seed(sum(map(ord, case)))
    keep = torch.rand(B_, nq, J, heads, generator=g) < 0.75
    r0, r1 = [nq // 3], [2 * nq // 3]
    if case == 'X4':
        r0.append(r0[0] + 13)
        r1.append(r1[0] + 13)
    for r in r0:
        keep[0, r] = False
    for r in r1:
        keep[1, r, :, 1] = False
        keep[1, r, 0, 1] = True
    return keep, r0, r1


_REF = {}


def _reference(case, x3, masked):
    """inputs (as the values the 16-bit operands hold) and the float64 restatement's results for one case (computed once, read-only)"""
    key = (case, x3, masked)
    if key in _REF:
        return _REF[key]
    fmap, kern, dil, frames, heads, dh, n, masking = CASES[case]
    T = frames * fmap * fmap
    g = torch.Generator().manual_seed(41 + sum(map(ord, case)))
    val = lambda t: bf_value(to_bf_pair(t, x3))                  # what a bf16 / hi + lo operand holds of t
    q, dO = val(torch.randn(B_, n, heads, dh, generator=g)), val(torch.randn(B_, n, heads, dh, generator=g))
    k, v = val(torch.randn(B_, T, heads, dh, generator=g)), val(torch.randn(B_, T, heads, dh, generator=g))
    nk, nv = val(torch.randn(heads, dh, generator=g)), val(torch.randn(heads, dh, generator=g))
    wth = torch.randn(heads, heads, generator=g) * 0.5 + torch.eye(heads)
    kmask = None
    if masking == 'rand':
        kmask = torch.rand(B_, T, generator=g) > 0.3
    elif masking == 'sample1':
        kmask = torch.ones(B_, T, dtype=torch.bool)
        kmask[1] = False
    keep, r0, r1 = _mask(case, ones=not masked)
    idx, valid = PU.cross2dna_window(fmap, kern, dil, frames, n)
    leaf = lambda t: t.double().requires_grad_(True)
    q64, k64, v64, nk64, nv64, w64 = (leaf(t) for t in (q, k, v, nk, nv, wth))
    o = XU.cross2dna_core_drop64(q64, k64, v64, nk64, nv64, w64, kmask, idx, valid, dh ** -0.5, keep_to_bhij(keep).double(), S if masked else 1.0)
    o.backward(dO[:, 1:].double())
    _REF[key] = dict(q=q, k=k, v=v, nk=nk, nv=nv, wth=wth, dO=dO, kmask=kmask, keep=keep, r0=r0, r1=r1, o=o.detach(), dq=q64.grad[:, 1:],
                     dk=k64.grad, dv=v64.grad, dnk=nk64.grad, dnv=nv64.grad, dwth=w64.grad)
    return _REF[key]


def _run(K, case, x3, R, keep, scale, dO=None):
    """forward + backward of one case under the guard, every operand between NaN bands -> fp32 values by name, and the raw parts"""
    fmap, kern, dil, frames, heads, dh, n, _ = CASES[case]
    T, inner = frames * fmap * fmap, heads * dh
    g = _geom(K, case)
    gd_ = lambda t: guarded(t, device=DEV) if t is not None else None
    pair = lambda t: K.BF(*(gd_(p) for p in to_bf_pair(t, x3)[:2]))
    kw = {} if keep is None else dict(keep=gd_(keep.to(torch.uint8)), drop_scale=scale)
    with guard(K) as gd:
        qp = pair(R['q'].reshape(B_ * n, inner))
        kvp = pair(torch.cat((R['k'].reshape(B_ * T, inner), R['v'].reshape(B_ * T, inner)), 1))
        dop = pair((R['dO'] if dO is None else dO).reshape(B_ * n, inner))
        nk, nv = pair(R['nk'].reshape(-1)), pair(R['nv'].reshape(-1))
        m8, w = gd_(R['kmask'].to(torch.uint8)) if R['kmask'] is not None else None, gd_(R['wth'])
        o = K.cross2dna_fwd(g, qp, kvp, nk, nv, m8, w, T, **kw)
        dq, dkv, dnk, dnv, dwth = K.cross2dna_bwd(g, qp, kvp, nk, nv, m8, w, dop, T, **kw)
        assert gd.made() > 0
    rows = lambda p: bf_value(p).reshape(B_, n, heads, dh)[:, 1:].cpu()             # row 0 (<bos>) is the caller's: not written, not compared
    dkvv = bf_value(dkv).cpu()
    out = dict(o=rows(o), dq=rows(dq), dk=dkvv[:, :inner].reshape(B_, T, heads, dh), dv=dkvv[:, inner:].reshape(B_, T, heads, dh),
               dnk=dnk.reshape(heads, dh).cpu(), dnv=dnv.reshape(heads, dh).cpu(), dwth=dwth.cpu())
    bits = lambda p: [p.hi.reshape(B_, n, inner)[:, 1:].cpu()] + ([p.lo.reshape(B_, n, inner)[:, 1:].cpu()] if p.lo is not None else [])
    raw = bits(o) + bits(dq) + [t.cpu() for t in (dkv.hi, dkv.lo, dnk, dnv, dwth) if t is not None]
    return out, raw


def _same_bits(a, b):
    iv = lambda t: t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)
    return a.shape == b.shape and torch.equal(iv(a), iv(b))


NAMES = ('o', 'dq', 'dk', 'dv', 'dnk', 'dnv', 'dwth')


@pytest.mark.parametrize('x3', [False, True])
@pytest.mark.parametrize('case', list(CASES))
def test_masked_cross2dna_kernels_against_float64(K, case, x3):
    """test 1: o, dq, dk, dv, d_null_k, d_null_v and dW_th of the masked kernels against the float64 restatement (rows 1 .. n - 1)"""
    fmap, kern, dil, frames, heads, dh, n, _ = CASES[case]
    g = _geom(K, case)
    assert K.cross2dna_drop_supported(g, lo=x3)
    assert (g.W * heads * 4 > 512) == (case == 'X4')
    R = _reference(case, x3, True)
    got, _ = _run(K, case, x3, R, R['keep'], S)
    tol_o, tol_g = (1e-3, 2e-3) if x3 else (2e-2, 7e-2)
    tag = f'[{case},x3={x3}]'
    errs = {nm: report(f'xc2drop_{nm}' + tag, got[nm], R[nm], tol_o if nm == 'o' else tol_g) for nm in NAMES}
    print('xc2drop' + tag, {k: f'{v:.2e}' for k, v in errs.items()})
    # where only the null slot is kept (sample 1, query r1, head 1) the output is P'_0 s v_null: finite, and not zero
    for r in R['r1']:
        assert bool(torch.isfinite(got['o'][1, r, 1]).all()) and float(got['o'][1, r, 1].abs().max()) > 0


@pytest.mark.parametrize('x3', [False, True])
@pytest.mark.parametrize('case', list(CASES))
def test_fully_dropped_query_is_exactly_zero_everywhere(K, case, x3):
    """test 2: the fully dropped query outputs 0 and has dq = 0; with another dO row there, dW_th, d_null_k, d_null_v (and dk, dv) keep
    their bits -- the query contributes exactly nothing"""
    fmap, kern, dil, frames, heads, dh, n, _ = CASES[case]
    R = _reference(case, x3, True)
    got, raw = _run(K, case, x3, R, R['keep'], S)
    assert len(R['r0']) == (2 if case == 'X4' else 1)
    if case == 'X4':                                          # the two dropped queries sit in different column tiles of their row
        tw = 10
        assert sorted((r % fmap) // tw for r in R['r0']) == [0, 1]
    dO2 = R['dO'].clone()
    for r in R['r0']:
        assert float(got['o'][0, r].abs().max()) == 0.0 and float(got['dq'][0, r].abs().max()) == 0.0
        dO2[0, 1 + r] = bf_value(to_bf_pair(torch.randn(heads, dh, generator=torch.Generator().manual_seed(1)) * 3, False))
    got2, _ = _run(K, case, x3, R, R['keep'], S, dO=dO2)
    for nm in ('dwth', 'dnk', 'dnv', 'dk', 'dv'):
        assert _same_bits(got2[nm], got[nm]), nm
    for r in R['r0']:
        assert float(got2['dq'][0, r].abs().max()) == 0.0


@pytest.mark.parametrize('x3', [False, True])
@pytest.mark.parametrize('case', list(CASES))
def test_full_mask_at_scale_one_is_the_unmasked_kernels_bit_for_bit(K, case, x3):
    """test 3: an all-ones mask at drop_scale = 1 gives the bits of the unmasked wrappers on every output; a masked run repeats its bits"""
    R = _reference(case, x3, False)
    _, plain = _run(K, case, x3, R, None, 1.0)
    _, ones = _run(K, case, x3, R, R['keep'], 1.0)
    assert bool(R['keep'].all()) and len(plain) == len(ones) == (9 if x3 else 6)
    for a, b in zip(plain, ones):
        assert _same_bits(a, b)
    assert all(bool(torch.isfinite(t.float()).all()) for t in ones)
    Rm = _reference(case, x3, True)
    _, m1 = _run(K, case, x3, Rm, Rm['keep'], S)
    _, m2 = _run(K, case, x3, Rm, Rm['keep'], S)
    assert len(m1) == len(m2) == len(ones) and all(_same_bits(a, b) for a, b in zip(m1, m2))
    assert not all(_same_bits(a, b) for a, b in zip(m1, ones))


def test_wrappers_refuse_a_bad_mask(K):
    """test 4: a mask of the wrong shape is a ValueError of the wrapper; drop_scale < 1 is AMDNUWA_ERR_ARG from the library, by entry name"""
    fmap, kern, dil, frames, heads, dh, n, _ = CASES['X2']
    T, inner = frames * fmap * fmap, heads * dh
    g = _geom(K, 'X2')
    J = frames * kern * kern + 1
    z = lambda *s: to_bf_pair(torch.zeros(*s, device=DEV), False)
    q, kv, nul, wth = z(B_ * n, inner), z(B_ * T, 2 * inner), z(inner), torch.eye(heads, device=DEV)
    good = torch.ones(B_, n - 1, J, heads, dtype=torch.bool, device=DEV)
    with pytest.raises(ValueError):
        K.cross2dna_fwd(g, q, kv, nul, nul, None, wth, T, keep=good[:, :, :, :1], drop_scale=S)
    with pytest.raises(ValueError):
        K.cross2dna_bwd(g, q, kv, nul, nul, None, wth, q, T, keep=good[:, :-1], drop_scale=S)
    with pytest.raises(RuntimeError, match='amdnuwa_cross2dna_fwd_drop'):
        K.cross2dna_fwd(g, q, kv, nul, nul, None, wth, T, keep=good, drop_scale=0.5)
    with pytest.raises(RuntimeError, match='amdnuwa_cross2dna_bwd_drop'):
        K.cross2dna_bwd(g, q, kv, nul, nul, None, wth, q, T, keep=good, drop_scale=0.5)


# ---------------------------------------------------------------------------------------------------
# 2. the module in train() mode
# ---------------------------------------------------------------------------------------------------

@pytest.fixture
def spies(monkeypatch, K):
    """what ran: keep arguments of the kernel wrappers, (node, kind, drop_p) of the library nodes, calls of ops._attn_keep_mask and of
    SparseCross2DNA._forward_torch"""
    from nuwa_pytorch_amd import ops
    from nuwa_pytorch_amd.nuwa_pytorch import SparseCross2DNA
    seen = dict(fwd=[], bwd=[], nodes=[], draws=[], torch=[])
    f0, b0, inner0, block0, t0 = K.cross2dna_fwd, K.cross2dna_bwd, ops.InnerFn.forward, ops.SandwichBlockFn.forward, SparseCross2DNA._forward_torch
    monkeypatch.setattr(K, 'cross2dna_fwd', lambda *a, **k: (seen['fwd'].append(k.get('keep') is not None), f0(*a, **k))[1])
    monkeypatch.setattr(K, 'cross2dna_bwd', lambda *a, **k: (seen['bwd'].append(k.get('keep') is not None), b0(*a, **k))[1])
    monkeypatch.setattr(ops.InnerFn, 'forward', staticmethod(
        lambda ctx, x, context, meta, *p: (seen['nodes'].append(('inner', meta['kind'], meta.get('drop_p'))), inner0(ctx, x, context, meta, *p))[1]))
    monkeypatch.setattr(ops.SandwichBlockFn, 'forward', staticmethod(
        lambda ctx, x, resid, context, meta, *p: (seen['nodes'].append(('block', meta['kind'], meta.get('drop_p'))), block0(ctx, x, resid, context, meta, *p))[1]))
    monkeypatch.setattr(SparseCross2DNA, '_forward_torch', lambda self, *a, **k: (seen['torch'].append(1), t0(self, *a, **k))[1])
    seen['draw0'] = ops._attn_keep_mask
    return seen


def _fixed_mask(monkeypatch, seen, keep):
    from nuwa_pytorch_amd import ops

    def fixed(B, nq, J, heads, p, device):
        seen['draws'].append((B, nq, J, heads, p))
        assert tuple(keep.shape) == (B, nq, J, heads)
        return keep.to(device)
    monkeypatch.setattr(ops, '_attn_keep_mask', fixed)


def _grads_of(mod):
    return {n: p.grad.clone() for n, p in mod.named_parameters() if p.grad is not None}


# (fmap, heads, dim_head, kernel, dilation, sketch frames, n, key mask): X1's geometry; the 16 x 16 map of test_gpu_modules.XC2_CASES
MOD_CASES = {'X1': (4, 2, 32, 3, 1, 2, 1 + 3 * 16, 'rand'), 'M16': (16, 8, 64, 3, 2, 2, 1 + 300, 'frame')}
DIM = 64
_MREF = {}


def _module_case(name, fused):
    """module, inputs, fixed mask and the fp32 restatement's results (computed once per (case, fused), read-only)"""
    from nuwa_pytorch_amd.nuwa_pytorch import SandwichNorm, SparseCross2DNA
    fmap, heads, dh, kernel, dil, frames, n, masking = MOD_CASES[name]
    torch.manual_seed(0)
    attn = SparseCross2DNA(dim=DIM, image_size=fmap, heads=heads, dim_head=dh, kernel_size=kernel, dilation=dil, dropout=P_DROP)
    m = SandwichNorm(dim=DIM, fn=attn) if fused else attn
    with torch.no_grad():
        for k, p in m.named_parameters():
            if 'norm' in k:
                p.add_(0.1 * torch.randn_like(p))
    if (name, fused) in _MREF:
        return (m, attn) + _MREF[(name, fused)]
    T = frames * fmap * fmap
    g = torch.Generator().manual_seed(n + fmap)
    x, ctx, dy = torch.randn(B_, n, DIM, generator=g), torch.randn(B_, T, DIM, generator=g), torch.randn(B_, n, DIM, generator=g)
    cmask = torch.rand(B_, T, generator=g) > 0.3
    if masking == 'frame':                           # sample 1 hides its last sketch frame (the sketch_mask of NUWASketch.forward)
        cmask = torch.ones(B_, T, dtype=torch.bool)
        cmask[1, (frames - 1) * fmap * fmap:] = False
    keep = torch.rand(B_, n - 1, frames * kernel * kernel + 1, heads, generator=g) >= P_DROP
    keep[0, 11] = False
    k5 = XU.keep_to_bgfij(keep, fmap * fmap)
    P = {k: v.detach().clone().requires_grad_(True) for k, v in attn.state_dict().items()}
    xr, cr = x.clone().requires_grad_(True), ctx.clone().requires_grad_(True)
    if fused:
        N = {k: v.detach().clone().requires_grad_(True) for k, v in m.state_dict().items() if 'norm' in k}
        h = F.layer_norm(xr, (DIM,), N['prenorm.weight'], N['prenorm.bias'])
        yr = xr + F.layer_norm(XU.sparse_cross_2dna_drop(h, cr, P, heads, fmap, kernel, dil, k5, S, context_mask=cmask), (DIM,),
                               N['postnorm.weight'], N['postnorm.bias'])
        want = {**{'fn.' + k: v for k, v in P.items()}, **N}
    else:
        yr = XU.sparse_cross_2dna_drop(xr, cr, P, heads, fmap, kernel, dil, k5, S, context_mask=cmask)
        want = P
    yr.backward(dy)
    _MREF[(name, fused)] = (x, ctx, dy, cmask, keep, yr.detach(), xr.grad, cr.grad, {k: v.grad for k, v in want.items()})
    return (m, attn) + _MREF[(name, fused)]


@pytest.mark.parametrize('mode,tol,gtol', MODES)
@pytest.mark.parametrize('fused', [False, True])
@pytest.mark.parametrize('name', list(MOD_CASES))
def test_sparse_cross_2dna_trains_with_dropout_on_the_masked_kernels(A, K, spies, monkeypatch, name, fused, mode, tol, gtol):
    """test 5: stand-alone (ops.InnerFn) and inside a SandwichNorm through fused_residual (one fused node): y, dx, dcontext and every
    parameter gradient against the restatement with the same mask; on the parent commit the module takes _forward_torch"""
    m, attn, x, ctx, dy, cmask, keep, yr, dxr, dcr, want = _module_case(name, fused)
    m = m.to(DEV).train()
    _fixed_mask(monkeypatch, spies, keep)
    A.set_precision(mode)
    try:
        xd, cd = x.to(DEV).requires_grad_(True), ctx.to(DEV).requires_grad_(True)
        with guard(K) as gd:
            y = m.fused_residual(xd, context=cd, context_mask=cmask.to(DEV)) if fused else m(xd, context=cd, context_mask=cmask.to(DEV))
            y.backward(dy.to(DEV))
            assert gd.made() > 0
        tag = f'xc2_drop[{name},fused={fused},{mode}]'
        report(tag + '.y', y, yr, tol)
        report(tag + '.dx', xd.grad, dxr, gtol)
        report(tag + '.dctx', cd.grad, dcr, gtol)
        got = _grads_of(m)
        assert set(got) == set(want) and len(got) == (10 if fused else 6)
        for k, gr in got.items():
            report(tag + f'.grad.{k}', gr, want[k], gtol)
    finally:
        A.set_precision('bf16')
    assert spies['nodes'] == [('block' if fused else 'inner', 'xc2', P_DROP)]
    assert spies['fwd'] == [True] and spies['bwd'] == [True] and len(spies['draws']) == 1 and not spies['torch']


@pytest.mark.parametrize('mode', [m[0] for m in MODES])
def test_eval_and_the_switch_take_the_other_routes(A, spies, monkeypatch, mode):
    """.eval(): bit-equal to a dropout = 0 twin on the unmasked wrappers, nothing drawn; dropout_on_kernels = False in training: the
    PyTorch-op formulation (the parent's route), no library node, nothing drawn by ops"""
    from nuwa_pytorch_amd import ops
    from nuwa_pytorch_amd.nuwa_pytorch import SparseCross2DNA
    monkeypatch.setattr(ops, '_attn_keep_mask', lambda *a: (spies['draws'].append(a), spies['draw0'](*a))[1])
    g = torch.Generator().manual_seed(9)
    x, ctx = torch.randn(2, 22, DIM, generator=g).to(DEV), torch.randn(2, 32, DIM, generator=g).to(DEV)
    A.set_precision(mode)
    try:
        outs = []
        for p in (P_DROP, 0.0):
            torch.manual_seed(0)
            m = SparseCross2DNA(dim=DIM, image_size=4, heads=2, dim_head=32, kernel_size=3, dropout=p).to(DEV).eval()
            with torch.no_grad():
                outs.append(m(x, context=ctx))
        assert torch.equal(outs[0], outs[1])
        assert not spies['draws'] and spies['fwd'] == [False, False] and not spies['torch']
        assert spies['nodes'] == [('inner', 'xc2', None)] * 2
        torch.manual_seed(0)
        m = SparseCross2DNA(dim=DIM, image_size=4, heads=2, dim_head=32, kernel_size=3, dropout=P_DROP).to(DEV).train()
        m.dropout_on_kernels = False
        y = m(x.clone().requires_grad_(True), context=ctx)
        y.sum().backward()
        assert spies['torch'] == [1] and len(spies['nodes']) == 2 and len(spies['fwd']) == 2 and not spies['bwd'] and not spies['draws']
        assert bool(torch.isfinite(y).all()) and not torch.equal(y.detach(), outs[1])
    finally:
        A.set_precision('bf16')


# ---------------------------------------------------------------------------------------------------
# 3. whole model: the README example's switches
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('reversible', [False, True])
def test_sketch_model_trains_with_the_readme_dropout(A, K, spies, monkeypatch, reversible):
    """test 6: one forward(return_loss=True), backward and FusedAdamW step of a tiny NUWASketch with attn_dropout = ff_dropout = 0.05.
    Every SparseCross2DNA block runs the masked kernels (none takes _forward_torch, as all of them do on the parent commit); the reversible
    decoder's recomputation draws the masks of the forward, and the device generator leaves the backward where it entered"""
    from nuwa_pytorch_amd import ops
    from nuwa_pytorch_amd.optimizer import FusedAdamW
    phase, drawn = ['fwd'], []
    monkeypatch.setattr(ops, '_attn_keep_mask', lambda *a: (drawn.append((phase[0], spies['draw0'](*a))), drawn[-1][1])[1])
    torch.manual_seed(0)
    vae = A.VQGanVAE(dim=32, image_size=16, num_layers=2, vq_codebook_size=64, vq_codebook_dim=32, use_vgg_and_gan=False)
    sketch_vae = A.VQGanVAE(dim=32, image_size=16, num_layers=2, vq_codebook_size=48, vq_codebook_dim=32, use_vgg_and_gan=False)
    m = A.NUWASketch(vae=vae, sketch_vae=sketch_vae, attn_dropout=0.05, ff_dropout=0.05, **{**SKETCH_KW, 'dec_reversible': reversible}).to(DEV).train()
    depth = SKETCH_KW['dec_depth']
    g = torch.Generator().manual_seed(1)
    sketch_ids = torch.randint(0, 48, (2, 2 * 16), generator=g).to(DEV)
    m.sketch_vae.get_video_indices = lambda frames: sketch_ids                   # the tokenizer is checked on its own (g7 tests)
    vid = torch.randint(0, 64, (2, 3 * 16), generator=g).to(DEV)
    sketch = torch.zeros(2, 2, 3, 16, 16, device=DEV)
    smask = torch.tensor([[True, True], [True, False]], device=DEV)
    params = [p for k, p in m.named_parameters() if not k.startswith(('vae.', 'sketch_vae.'))]
    opt = FusedAdamW(params, lr=1e-3)
    A.set_precision('bf16x3-fwd')
    try:
        with guard(K) as gd:
            loss = m(sketch=sketch, sketch_mask=smask, video=vid, return_loss=True, cond_dropout_prob=0.)
            torch.cuda.synchronize()
            state_fwd = torch.cuda.get_rng_state().clone()
            phase[0] = 'bwd'
            loss.backward()
            torch.cuda.synchronize()
            state_bwd = torch.cuda.get_rng_state().clone()
            assert gd.made() > 0
        before = [p.detach().clone() for p in params[:4]]
        opt.step()
        torch.cuda.synchronize()
    finally:
        A.set_precision('bf16')
    assert bool(torch.isfinite(loss.detach()))
    trainable = [p for p in params if p.requires_grad]
    assert len(trainable) > 40 and all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in trainable)
    assert all(bool(torch.isfinite(p).all()) for p in params) and any(not torch.equal(a, p.detach()) for a, p in zip(before, params[:4]))
    # every SparseCross2DNA block on the masked kernels, as a fused node; the reversible decoder runs each forward twice
    runs = 2 * depth if reversible else depth
    assert spies['fwd'] == [True] * runs and spies['bwd'] == [True] * depth and not spies['torch']
    assert [nd for nd in spies['nodes'] if nd[1] == 'xc2'] == [('block', 'xc2', 0.05)] * runs
    # masks: J = 2 * 9 + 1 = 19 slots mark the cross blocks' draws (a causal Sparse3DNA with dropout would draw 28-slot masks through the same function)
    xf = [k for ph, k in drawn if ph == 'fwd' and k.shape[2] == 19]
    xb = [k for ph, k in drawn if ph == 'bwd' and k.shape[2] == 19]
    assert len(xf) == depth and len(xb) == (depth if reversible else 0)
    assert all(tuple(k.shape) == (2, 3 * 16 - 1, 19, SKETCH_KW['dec_heads']) for k in xf)
    if reversible:                                   # the recomputation walks the blocks backwards and draws each block's forward mask again
        for kf_, kb_ in zip(xf, reversed(xb)):
            assert torch.equal(kf_, kb_)
        allf, allb = [k for ph, k in drawn if ph == 'fwd'], [k for ph, k in drawn if ph == 'bwd']
        assert len(allf) == len(allb) and all(any(a.shape == b.shape and torch.equal(a, b) for b in allb) for a in allf)
    assert not any(torch.equal(a, b) for i, a in enumerate(xf) for b in xf[i + 1:])          # (distinct draws per block)
    assert torch.equal(state_fwd.cpu(), state_bwd.cpu())
