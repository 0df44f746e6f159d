"""Attention dropout inside the Sparse3DNA MFMA band kernels on the MI355X: the masked (DROP) forms of the two-row forward tiles, the one-row
forward kernel and the query-side backward, in the bf16 form, the fp16 forward and the fp16-gradient backward, against the fp64 restatement
of tests/attn_dropout_util.py on the values the kernels read; then Sparse3DNA at band geometry in training, and a two-layer NUWA on a
16 x 16 token map with the README's dropout switches.

All kernel cases: B = 2, 8 heads x 64, W = 16, operands bf16-rounded (and exact in fp16: values below 2^-10 are set to 0), everything under
the guard bands and NaN prefill of guard_util -- a mask read for an absent query reads the 0xFF band (a nonzero byte: "keep") or a
neighbour's row, a missed store leaves NaN.  Which forward kernel a case reaches follows the library's tile rule (two-row tiles where H
splits into 2 * dh, else the one-row kernel): T / Tp / D / Tb the tiles, R (H = 3) the one-row kernel.

Metric: gpu_util.report (max-abs error / max-abs reference).  Bounds are those of the tests of the same kernels without a mask:
bf16 form 2^-7 forward, 2^-6 dq / dk / dv / dW_th / d(bias) (test_sparse3dna_core_rel_pos_bias_on_the_mfma_kernels); fp16 forward 6e-4
against the restatement and 3e-3 against the hi + lo kernel (test_sparse3dna_fwd_f16_core); fp16-gradient backward TOL_S3 of
test_gpu_attention_bwd16.py with the reference built as there (dO rounded to fp16 at scale S).  A mask only multiplies entries by 0 or s."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from attn_dropout_util import keep_to_bhij, sparse3dna_core_drop, sparse3dna_drop  # noqa: E402
from gpu_util import report, bf_round, to_bf_pair, bf_value  # noqa: E402
from guard_util import guard, guarded  # noqa: E402

DEV = 'cuda'
MODES = [('bf16x3', 1e-3, 2e-3), ('bf16x3-fwd', 1e-3, 7e-2), ('bf16', 2e-2, 7e-2)]          # tests/test_gpu_attn_dropout.py
B_, HEADS, DH = 2, 8, 64
INNER = HEADS * DH
S = 1.0 / 0.75

# name: (grid, kernel, dilation, ntok, rel_bias)
CASES = {
    'T': ((2, 2, 16), (3, 3, 3), (1, 1, 1), 65, False),        # two-row forward tiles, packed workspace
    'Tp': ((2, 2, 16), (3, 3, 3), (1, 1, 1), 41, False),       # the sequence ends inside a grid row: absent queries, a tile whose second row is absent
    'R': ((2, 3, 16), (3, 3, 3), (1, 1, 1), 97, False),        # odd H: the one-row forward kernel
    'D': ((2, 4, 16), (3, 3, 3), (1, 2, 2), 129, False),       # two-row tiles at dh = 2, taps cut by the left border
    'Tb': ((2, 2, 16), (3, 3, 3), (1, 1, 1), 65, True),        # BIAS instantiations, fp32 workspace, d_rel_bias
}
J_ = 28


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


@pytest.fixture(scope='module')
def O():
    from oracle import nuwa_oracle
    return nuwa_oracle


def _mask(case, ones=False):
    """kernel-order keep mask [B, nq, J, heads]: Bernoulli(0.75) from a fixed generator; query r0 of sample 0 fully dropped; (sample 1,
    query r1, head 1) keeps only the <bos> slot; query r2 of sample 1 has the <bos> slot alone dropped, for all heads (the <bos> slot
    takes its own path, PM0, in the band backward)"""
    n = CASES[case][3]
    nq = n - 1
    if ones:
        return torch.ones(B_, nq, J_, HEADS, dtype=torch.bool), None, None, None
    g = torch.Generator().manual_seed(100 + sum(map(ord, case)))
    keep = torch.rand(B_, nq, J_, HEADS, generator=g) < 0.75
    r0, r1, r2 = nq // 3, 2 * nq // 3, nq // 2
    keep[0, r0] = False
    keep[1, r1, :, 1] = False
    keep[1, r1, 0, 1] = True
    keep[1, r2] = True
    keep[1, r2, 0] = False
    return keep, r0, r1, r2


_REF, _S = {}, {}


def _inputs(case):
    shape, kern, dil, n, rel_bias = CASES[case]
    torch.manual_seed(71 + sum(map(ord, case)))
    qkv = bf_round(torch.randn(B_, n, 3, HEADS, DH))
    do = bf_round(torch.randn(B_, n, HEADS, DH))
    qkv[qkv.abs() < 2 ** -10] = 0                     # bf16 values that are fp16 values too: both operand forms read the same numbers
    assert torch.equal(qkv.half().float(), qkv)
    wth = torch.randn(HEADS, HEADS) * 0.5 + torch.eye(HEADS)
    rel = torch.randn(HEADS, J_ - 1) * 0.7 if rel_bias else None                 # oracle layout (h, K)
    return qkv, do, wth, rel


def _grad_scale(do):
    """S of the production rule for this dO (ops._grad_scale), as tests/test_gpu_attention_bwd16.py takes it"""
    from nuwa_pytorch_amd import ops
    return float(ops._grad_scale(do.reshape(-1, INNER).to(DEV))[0])


def _reference(O, case, masked):
    """inputs and the fp64 restatement's results for one case (computed once, read-only): gradients for the bf16-rounded dO and for the
    dO the fp16-gradient backward reads, fp16(S dO) / S"""
    key = (case, masked)
    if key in _REF:
        return _REF[key]
    shape, kern, dil, n, rel_bias = CASES[case]
    qkv, do, wth, rel = _inputs(case)
    keep, r0, r1, r2 = _mask(case, ones=not masked)
    q64 = qkv.double().requires_grad_(True)
    w64 = wth.double().requires_grad_(True)
    rel64 = rel.double().requires_grad_(True) if rel_bias else None
    idx = O.neighbor_table(shape, kern, dil, causal=True)
    o = sparse3dna_core_drop(q64[:, :, 0], q64[:, :, 1], q64[:, :, 2], w64, idx, DH ** -0.5, keep_to_bhij(keep).double(),
                             S if masked else 1.0, rel_pos_bias=rel64)
    ins = [q64, w64] + ([rel64] if rel_bias else [])
    gr = torch.autograd.grad(o, ins, do.double(), retain_graph=True)
    R = dict(qkv=qkv, do=do, wth=wth, rel=rel, keep=keep, r0=r0, r1=r1, r2=r2, o=o.detach(), dqkv=gr[0], dwth=gr[1],
             drel=gr[2] if rel_bias else None)
    if not rel_bias:
        if case not in _S:
            _S[case] = _grad_scale(do)
        S16 = _S[case]
        do16 = (do * S16).half().float() / S16
        g16 = torch.autograd.grad(o, [q64, w64], do16.double())
        R.update(S16=S16, dqkv16=g16[0], dwth16=g16[1])
    _REF[key] = R
    return R


def _geom(K, case):
    shape, kern, dil, n, _ = CASES[case]
    g = K.s3_geom(B_, n, shape, kern, dil, HEADS, DH)
    assert K.s3_f16_supported(g) and K.s3_drop_supported(g, lo=False)          # a band-kernel geometry
    return g, n


def _rel_dev(R):
    return guarded(torch.cat((torch.zeros(1, HEADS), R['rel'].t()), 0).contiguous(), device=DEV) if R['rel'] is not None else None


def _kw(keep, scale):
    return {} if keep is None else dict(keep=guarded(keep.to(torch.uint8), device=DEV), drop_scale=scale)


def _bits(t):
    return t.view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _same_bits(xs, ys):
    assert len(xs) == len(ys) >= 1
    for a, b in zip(xs, ys):
        assert a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------------
# 1. the bf16 band kernels (amdnuwa_sparse3dna_fwd_drop / _bwd_drop at band geometry)
# ---------------------------------------------------------------------------------------------------

def _run_bf16(K, case, R, keep, scale, do=None):
    g, n = _geom(K, case)
    qkv = K.BF(guarded(R['qkv'].reshape(B_ * n, 3 * INNER).to(torch.bfloat16), device=DEV), None)
    dO = K.BF(guarded((R['do'] if do is None else do).reshape(B_ * n, INNER).to(torch.bfloat16), device=DEV), None)
    wth, rel = guarded(R['wth'], device=DEV), _rel_dev(R)
    kw = _kw(keep, scale)
    with guard(K) as gd:
        o = K.sparse3dna_fwd(g, qkv, wth, rel_bias=rel, **kw)
        dqkv, dwth, drel = K.sparse3dna_bwd(g, qkv, wth, dO, rel_bias=rel, **kw)
        assert gd.made() > 0
    assert o.lo is None and dqkv.lo is None
    raw = [t for t in (o.hi, dqkv.hi, dwth, drel) if t is not None]
    return o.hi.float(), dqkv.hi.float(), dwth, drel, raw


@pytest.mark.parametrize('case', list(CASES))
def test_masked_band_kernels_bf16(K, O, case):
    _, _, _, n, rel_bias = CASES[case]
    R = _reference(O, case, True)
    o, dqkv, dwth, drel, raw = _run_bf16(K, case, R, R['keep'], S)
    tag = f'[{case}]'
    # ---- values
    report('s3band_drop.fwd' + tag, o.reshape(B_, n, HEADS, DH), R['o'], 2 ** -7)
    gq = R['dqkv'].reshape(B_ * n, 3 * INNER)
    for nm, sl in (('dq', slice(0, INNER)), ('dk', slice(INNER, 2 * INNER)), ('dv', slice(2 * INNER, 3 * INNER))):
        report(f's3band_drop.{nm}' + tag, dqkv[:, sl], gq[:, sl], 2 ** -6)
    report('s3band_drop.dwth' + tag, dwth, R['dwth'], 2 ** -6)
    if rel_bias:
        report('s3band_drop.drel' + tag, drel[1:].t(), R['drel'], 2 ** -6)
    # ---- exact zeros: the fully dropped query (sample 0, token row r0 + 1) outputs 0 and has dq = 0; <bos> outputs its value row
    row = 1 + R['r0']
    assert float(o.reshape(B_, n, INNER)[0, row].abs().max()) == 0.0
    assert float(dqkv.reshape(B_, n, 3 * INNER)[0, row, :INNER].abs().max()) == 0.0
    assert torch.equal(o.reshape(B_, n, INNER)[:, 0].cpu(), R['qkv'][:, 0, 2].reshape(B_, INNER))
    # ... and adds exactly 0 to dW_th (and d(bias)): another dO row there leaves their bits
    do2 = R['do'].clone()
    do2[0, row] = bf_round(torch.randn(HEADS, DH, generator=torch.Generator().manual_seed(1)) * 3)
    _, dqkv2, dwth2, drel2, _ = _run_bf16(K, case, R, R['keep'], S, do=do2)
    assert torch.equal(dwth2, dwth)
    if rel_bias:
        assert torch.equal(drel2, drel)
    assert float(dqkv2.reshape(B_, n, 3 * INNER)[0, row, :INNER].abs().max()) == 0.0
    # ---- repeatability
    *_, raw3 = _run_bf16(K, case, R, R['keep'], S)
    _same_bits(raw, raw3)


@pytest.mark.parametrize('case', list(CASES))
def test_full_mask_at_scale_one_is_the_unmasked_band_kernels_bit_for_bit_bf16(K, O, case):
    """fails on the parent commit: there the masked call runs the VALU kernels, whose bits differ from the band kernels'"""
    R = _reference(O, case, False)
    assert bool(R['keep'].all())
    *_, plain = _run_bf16(K, case, R, None, 1.0)
    *_, ones = _run_bf16(K, case, R, R['keep'], 1.0)
    _same_bits(plain, ones)
    assert len(ones) == (4 if CASES[case][4] else 3) and all(bool(torch.isfinite(t.float()).all()) for t in ones)


def test_valu_route_stays_behind_its_tuning_key(K, O):
    """tuning key 26 = 1: a masked call at band geometry runs the masked VALU kernels (the route of the parent commit): same values at the
    bf16 bounds, other bits than the band route"""
    from nuwa_pytorch_amd import _lib
    L = _lib.lib()
    R = _reference(O, 'T', True)
    n = CASES['T'][3]
    o_b, dqkv_b, *_ = _run_bf16(K, 'T', R, R['keep'], S)
    assert L.amdnuwa_get_tuning(26) == 0
    L.amdnuwa_set_tuning(26, 1)
    try:
        o_v, dqkv_v, dwth_v, _, _ = _run_bf16(K, 'T', R, R['keep'], S)
    finally:
        L.amdnuwa_set_tuning(26, 0)
    report('s3band_drop.valu_route.fwd', o_v.reshape(B_, n, HEADS, DH), R['o'], 2 ** -7)
    report('s3band_drop.valu_route.dqkv', dqkv_v, R['dqkv'].reshape(B_ * n, 3 * INNER), 2 ** -6)
    assert not torch.equal(o_v, o_b) or not torch.equal(dqkv_v, dqkv_b)


# ---------------------------------------------------------------------------------------------------
# 2. the fp16 forward (amdnuwa_sparse3dna_fwd_f16_drop), all three output forms
# ---------------------------------------------------------------------------------------------------

def _run_f16_fwd(K, case, R, keep, scale, o_f16=False):
    g, n = _geom(K, case)
    q16 = guarded(R['qkv'].reshape(B_ * n, 3 * INNER).half(), device=DEV)
    qkv = K.BF(None, None, q16)
    wth, rel = guarded(R['wth'], device=DEV), _rel_dev(R)
    with guard(K) as gd:
        o = K.sparse3dna_fwd(g, qkv, wth, rel_bias=rel, o_f16=o_f16, **_kw(keep, scale))
        assert gd.made() > 0
    return o


@pytest.mark.parametrize('case', list(CASES))
def test_masked_band_forward_f16(K, O, case):
    """on the parent commit the wrapper raises RuntimeError for keep together with the fp16 operand form"""
    _, _, _, n, _ = CASES[case]
    R = _reference(O, case, True)
    o = _run_f16_fwd(K, case, R, R['keep'], S)
    assert o.hi is not None and o.lo is not None and o.f16 is None
    val = bf_value(o)
    tag = f'[{case}]'
    report('s3band_drop.fwd_f16' + tag, val.reshape(B_, n, HEADS, DH), R['o'], 6e-4)
    # against the masked hi + lo (VALU) kernel on the same values, as test_sparse3dna_fwd_f16_core does without a mask
    g, _ = _geom(K, case)
    pair = K.BF(*(guarded(p, device=DEV) for p in to_bf_pair(R['qkv'].reshape(B_ * n, 3 * INNER), True)[:2]))
    with guard(K) as gd:
        o3 = K.sparse3dna_fwd(g, pair, guarded(R['wth'], device=DEV), rel_bias=_rel_dev(R), **_kw(R['keep'], S))
        assert gd.made() > 0
    report('s3band_drop.fwd_f16_vs_x3' + tag, val, bf_value(o3), 3e-3)
    # exact zeros, <bos>
    row = 1 + R['r0']
    assert float(val.reshape(B_, n, INNER)[0, row].abs().max()) == 0.0
    assert torch.equal(val.reshape(B_, n, INNER)[:, 0].cpu(), R['qkv'][:, 0, 2].reshape(B_, INNER))
    # the other two output forms: the same bf16 copy; the fp16 copy is the fp16 rounding of the value the pair carries (pair: ~2^-17)
    ob = _run_f16_fwd(K, case, R, R['keep'], S, o_f16=True)
    oo = _run_f16_fwd(K, case, R, R['keep'], S, o_f16='only')
    assert ob.lo is None and oo.hi is None and oo.lo is None
    _same_bits([o.hi, ob.f16], [ob.hi, oo.f16])
    assert bool(((ob.f16.float() - val).abs() <= 2 ** -11 * val.abs() + 2 ** -24).all())
    assert float(ob.f16.reshape(B_, n, INNER)[0, row].float().abs().max()) == 0.0
    # repeatability
    o2 = _run_f16_fwd(K, case, R, R['keep'], S)
    _same_bits([o.hi, o.lo], [o2.hi, o2.lo])


@pytest.mark.parametrize('case', list(CASES))
def test_full_mask_at_scale_one_is_the_unmasked_forward_bit_for_bit_f16(K, O, case):
    R = _reference(O, case, False)
    for form in (False, True, 'only'):
        plain = _run_f16_fwd(K, case, R, None, 1.0, o_f16=form)
        ones = _run_f16_fwd(K, case, R, R['keep'], 1.0, o_f16=form)
        parts = lambda o: [t for t in (o.hi, o.lo, o.f16) if t is not None]
        _same_bits(parts(plain), parts(ones))
        assert len(parts(ones)) == (1 if form == 'only' else 2) and all(bool(torch.isfinite(t.float()).all()) for t in parts(ones))


# ---------------------------------------------------------------------------------------------------
# 3. the fp16-gradient backward (amdnuwa_sparse3dna_bwd_f16_drop); it takes no bias
# ---------------------------------------------------------------------------------------------------

G16_CASES = [c for c in CASES if not CASES[c][4]]


def _run_bwd16(K, case, R, keep, scale, do=None):
    """-> (dqkv / S as fp32, dwth, the raw fp16 / fp32 arrays)"""
    g, n = _geom(K, case)
    assert K.s3_bwd16_supported(g)
    S16 = R['S16']
    q16 = guarded(R['qkv'].reshape(B_ * n, 3 * INNER).half(), device=DEV)
    dO16 = guarded(((R['do'] if do is None else do).reshape(B_ * n, INNER) * S16).half(), device=DEV)
    s2 = torch.tensor([S16, 1.0 / S16], dtype=torch.float32, device=DEV)
    with guard(K) as gd:
        dqkv, dwth = K.sparse3dna_bwd16(g, q16, guarded(R['wth'], device=DEV), dO16, s2, **_kw(keep, scale))
        assert gd.made() > 0
    return dqkv.float() / S16, dwth, [dqkv, dwth]


@pytest.mark.parametrize('case', G16_CASES)
def test_masked_band_backward_f16_gradients(K, O, case):
    from test_gpu_attention_bwd16 import TOL_S3
    n = CASES[case][3]
    R = _reference(O, case, True)
    K.f16_sat_count()
    dqkv, dwth, raw = _run_bwd16(K, case, R, R['keep'], S)
    assert K.f16_sat_count() == 0, 'fp16 stores saturated'
    tag = f'[{case}]'
    gq = R['dqkv16'].reshape(B_ * n, 3 * INNER)
    for nm, sl in (('dq', slice(0, INNER)), ('dk', slice(INNER, 2 * INNER)), ('dv', slice(2 * INNER, 3 * INNER))):
        report(f's3band_drop.bwd16.{nm}' + tag, dqkv[:, sl], gq[:, sl], TOL_S3[nm])
    report('s3band_drop.bwd16.dwth' + tag, dwth, R['dwth16'], TOL_S3['dwth'])
    row = 1 + R['r0']
    assert float(dqkv.reshape(B_, n, 3 * INNER)[0, row, :INNER].abs().max()) == 0.0
    do2 = R['do'].clone()
    do2[0, row] = bf_round(torch.randn(HEADS, DH, generator=torch.Generator().manual_seed(1)) * 0.9 * float(R['do'].abs().max()) / 4)
    dqkv2, dwth2, _ = _run_bwd16(K, case, R, R['keep'], S, do=do2)           # (inside max|dO|: the same scale S applies)
    assert torch.equal(dwth2, dwth)
    assert float(dqkv2.reshape(B_, n, 3 * INNER)[0, row, :INNER].abs().max()) == 0.0
    *_, raw3 = _run_bwd16(K, case, R, R['keep'], S)
    _same_bits(raw, raw3)


@pytest.mark.parametrize('case', G16_CASES)
def test_full_mask_at_scale_one_is_the_unmasked_backward_bit_for_bit_f16(K, O, case):
    R = _reference(O, case, False)
    *_, plain = _run_bwd16(K, case, R, None, 1.0)
    *_, ones = _run_bwd16(K, case, R, R['keep'], 1.0)
    _same_bits(plain, ones)
    assert all(bool(torch.isfinite(t.float()).all()) for t in ones)


def test_masked_backward_f16_does_not_saturate_at_drop_scale_two(K):
    """the inputs of test_sparse3dna_bwd16_vs_oracle's first case under a Bernoulli(0.5) mask at drop_scale = 2: dP' leaves for fp16 as 0 or
    the unmasked value (the factor 2 is applied in fp32 behind the conversion), so the counter stays where it is without a mask"""
    from test_gpu_attention_bwd16 import S3_CASES, S3Case, _s2
    shape, kern, dil, n, B = S3_CASES[0]
    c = S3Case(K, shape, kern, dil, n, B, seed=40)
    J = kern[0] * kern[1] * kern[2] + 1
    keep = (torch.rand(B, c.n - 1, J, HEADS, generator=torch.Generator().manual_seed(5)) < 0.5).to(torch.uint8).to(DEV)
    dO16 = (c.dO.to(DEV) * c.S).half()
    K.f16_sat_count()
    K.sparse3dna_bwd16(c.g, c.q_dev, c.w_dev, dO16, _s2(c.S))
    assert K.f16_sat_count() == 0
    dqkv, dwth = K.sparse3dna_bwd16(c.g, c.q_dev, c.w_dev, dO16, _s2(c.S), keep=keep, drop_scale=2.0)
    assert K.f16_sat_count() == 0, 'fp16 stores saturated under the mask'
    assert bool(torch.isfinite(dqkv.float()).all()) and bool(torch.isfinite(dwth).all())


# ---------------------------------------------------------------------------------------------------
# 4. Sparse3DNA at band geometry in training
# ---------------------------------------------------------------------------------------------------

P_DROP = 0.05


def _module(A, p, dim=64):
    torch.manual_seed(0)
    return A.Sparse3DNA(dim=dim, video_shape=(2, 2, 16), heads=HEADS, dim_head=DH, causal=True, dropout=p)


@pytest.fixture
def plans(monkeypatch):
    from nuwa_pytorch_amd import ops
    seen, plan0 = [], ops.block_plan
    monkeypatch.setattr(ops, 'block_plan', lambda *a, **k: (lambda pl: (seen.append(pl), pl)[1])(plan0(*a, **k)))
    return seen


@pytest.mark.parametrize('mode,tol,gtol', MODES)
@pytest.mark.parametrize('fused,dim,n', [(False, 64, 65), (True, 256, 64)])
def test_sparse3dna_trains_with_dropout_on_the_band_kernels(A, O, plans, monkeypatch, fused, dim, n, mode, tol, gtol):
    """stand-alone (ops.InnerFn: in 'bf16x3-fwd' the fp16 core with the bf16 backward) and as SandwichNorm(.) through the fused residual node
    (there 'bf16x3-fwd' plans the fp16-gradient backward, the third branch of S3Inner that carries the mask: its fp16 weight-gradient
    products want 128 rows or more, a multiple of 64, and a width of 256 or more -- 2 x 64 rows of width 256, the sequence one short of full)"""
    from nuwa_pytorch_amd import ops, video_audio as VA
    from nuwa_pytorch_amd.nuwa_pytorch import SandwichNorm
    import torch.nn.functional as F
    b, shape = 2, (2, 2, 16)
    attn, attn0 = _module(A, P_DROP, dim), _module(A, 0.0, dim)
    m, twin = (SandwichNorm(dim=dim, fn=attn), SandwichNorm(dim=dim, fn=attn0)) if fused else (attn, attn0)
    if fused:
        with torch.no_grad():
            for (k, p), (_, p0) in zip(m.named_parameters(), twin.named_parameters()):
                if 'norm' in k:
                    p.add_(0.1 * torch.randn_like(p))
                    p0.copy_(p)
    g = torch.Generator().manual_seed(8)
    x, dy = torch.randn(b, n, dim, generator=g), torch.randn(b, n, dim, generator=g)
    keep = torch.rand(b, n - 1, J_, HEADS, generator=g) >= 0.25             # (a denser mask than p would draw: every head of every row loses slots)
    keep[1, 20] = False
    s = 1.0 / (1.0 - P_DROP)
    P = {k: v.detach().clone().requires_grad_(True) for k, v in attn.state_dict().items() if v.is_floating_point()}
    xr = x.clone().requires_grad_(True)
    if fused:
        N = {k: v.detach().clone().requires_grad_(True) for k, v in m.state_dict().items() if 'norm' in k}
        h = F.layer_norm(xr, (dim,), N['prenorm.weight'], N['prenorm.bias'])
        yr = xr + F.layer_norm(sparse3dna_drop(h, P, shape, 3, 1, HEADS, keep_to_bhij(keep), s, O), (dim,), N['postnorm.weight'], N['postnorm.bias'])
        want = {**{'fn.' + k: v for k, v in P.items()}, **N}
    else:
        yr = sparse3dna_drop(xr, P, shape, 3, 1, HEADS, keep_to_bhij(keep), s, O)
        want = P
    yr.backward(dy)
    m, twin = m.to(DEV).train(), twin.to(DEV).train()
    torch_branch = []
    attn.dropout.register_forward_hook(lambda *a: torch_branch.append(1))
    draws = []

    def fixed(B, nq, J, heads, p, device):
        draws.append((B, nq, J, heads, p))
        assert tuple(keep.shape) == (B, nq, J, heads)
        return keep.to(device)
    monkeypatch.setattr(ops, '_attn_keep_mask', fixed)
    A.set_precision(mode)
    try:
        xd = x.to(DEV).requires_grad_(True)
        y = VA._residual(m, xd) if fused else m(xd)
        tag = f's3band_drop.module[fused={fused},{mode}]'
        report(tag + '.y', y, yr.detach(), tol)
        y.backward(dy.to(DEV))
        report(tag + '.dx', xd.grad, xr.grad, gtol)
        got = {k: p.grad for k, p in m.named_parameters() if p.grad is not None}
        assert set(got) == {k for k in want if want[k].grad is not None} and len(got) == (9 if fused else 5)
        for k, gr in got.items():
            report(tag + f'.grad.{k}', gr, want[k].grad, gtol)
        assert len(plans) == 1 and draws == [(b, n - 1, J_, HEADS, P_DROP)] and not torch_branch
        assert plans[0].bwd16 == (fused and mode == 'bf16x3-fwd') and plans[0].core16 == (mode == 'bf16x3-fwd')
        # the plan of the dropout-free twin, field for field (the guarded weights are each module's own)
        run = (lambda blk: VA._residual(blk, xd.detach())) if fused else (lambda blk: blk(xd.detach()))
        with torch.no_grad():
            run(twin)
        assert len(plans) == 2 and plans[0]._replace(guarded=()) == plans[1]._replace(guarded=())
        # .eval(): bit-equal to the twin, no mask drawn
        m.eval(), twin.eval()
        with torch.no_grad():
            assert torch.equal(run(m), run(twin))
        assert len(draws) == 1 and not torch_branch
    finally:
        A.set_precision('bf16')


# ---------------------------------------------------------------------------------------------------
# 5. a two-layer NUWA on a 16 x 16 token map with the README's dropout switches
# ---------------------------------------------------------------------------------------------------

def _nuwa_step(A, reversible):
    torch.manual_seed(0)
    vae = A.VQGanVAE(dim=32, image_size=64, num_layers=2, vq_codebook_size=64, vq_codebook_dim=32, use_vgg_and_gan=False)
    m = A.NUWA(vae=vae, dim=64, text_num_tokens=50, text_max_seq_len=8, max_video_frames=2, text_enc_depth=1, dec_depth=2,
               enc_reversible=True, dec_reversible=reversible, dec_heads=HEADS, dec_dim_head=DH, text_enc_heads=2, text_enc_dim_head=32,
               sparse_3dna_kernel_size=3, attn_dropout=0.05, ff_dropout=0.05).to(DEV).train()
    assert m.video_fmap_size == 16
    g = torch.Generator().manual_seed(1)
    text = torch.randint(1, 50, (2, 8), generator=g).to(DEV)
    ids = torch.randint(0, 64, (2, 2 * 256), generator=g).to(DEV)
    torch.manual_seed(2)
    loss = m(text=text, video=ids, return_loss=True, cond_dropout_prob=0.)
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}, \
        [k for k, p in m.named_parameters() if p.grad is None and not k.startswith('vae.')]


@pytest.mark.parametrize('reversible', [False, True])
def test_nuwa_trains_with_the_readme_dropout_on_a_16x16_map(A, K, monkeypatch, reversible):
    """one training step: a finite loss, a gradient on every parameter, and two steps from the same seed bit-equal (in the reversible stack
    the recomputed forward replays the masks: RngReplay).  The decoder's window attention runs at band geometry in the fp16 operand form.
    The stacks build their Sparse3DNA without the dropout argument, as the reference's Transformer does (np.py:1108-1118, 1222-1232):
    attn_dropout reaches the text encoder's and the cross attention, ff_dropout the FeedForwards, and the window attention of a NUWA model
    draws no mask -- the masked band kernels are reached through Sparse3DNA(dropout=...) itself (the module test above)."""
    seen = []
    f0 = K.sparse3dna_fwd
    monkeypatch.setattr(K, 'sparse3dna_fwd', lambda g, qkv, *a, **k: (seen.append((k.get('keep') is not None, qkv.f16 is not None)), f0(g, qkv, *a, **k))[1])
    # attn_dropout > 0 puts the text cross-attention on its PyTorch-op route, whose 1 x 1 talking-heads Conv2d has a weight gradient the
    # convolution library computes differently run to run unless it is asked for its deterministic algorithms
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    A.set_precision('bf16x3-fwd')
    try:
        loss, grads, missing = _nuwa_step(A, reversible)
        first = list(seen)
        loss2, grads2, _ = _nuwa_step(A, reversible)
    finally:
        A.set_precision('bf16')
        torch.backends.cudnn.deterministic = det
    assert bool(torch.isfinite(loss)) and not missing, missing
    assert len(grads) > 40 and all(bool(torch.isfinite(v).all()) for v in grads.values())
    assert len(first) >= 2 and all(f16 and not masked for masked, f16 in first), first
    assert torch.equal(loss, loss2) and set(grads) == set(grads2)
    for k in grads:
        assert torch.equal(grads[k], grads2[k]), k
