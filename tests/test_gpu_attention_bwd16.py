"""The fp16-gradient attention backward of the compliant mode ('bf16x3-fwd', kernels.DEFAULT_BWD_F16 = 'fsx') against the oracle.

Every attention gradient of the benchmarked step comes from these kernels:
  3DNA blocks             amdnuwa_sparse3dna_bwd_f16                              (K.sparse3dna_bwd16)
  cross-attention blocks  amdnuwa_xattn6_pack_bwd_f16 -> amdnuwa_xattn6_bwd_f16   (K.xattn6_pack_bwd, K.xattn6_bwd16)
                          -> fp16 chunk-major dK / dV TN products -> unpack       (K.xattn_kv_grads16, K.xattn_unpack(null_last=True))
The operands are fp16 values (what the forward hands over), dO16 = fp16(S dO) with S the production rule (ops._grad_scale), and the
reference is autograd through the oracle on exactly the values the kernels read: q16.float() and dO16.float() / S.  Every case asserts
that the fp16 path takes it -- a gate change fails these tests instead of skipping them.

Tolerances are max-abs error / max-abs reference (gpu_util.report).  The cap is 2^-8 (the bf16 kernels' tests use 2^-6): the operands are
exact and each intermediate or output is rounded to fp16 once.  The cross-attention dk / dv are read as the unpack kernel's hi + lo pair
(the block keeps the hi part: a bf16 rounding after these kernels, 2^-9).  The values in TOL_S3 / TOL_X are about twice the worst errors
measured on the MI355X, capped at 2^-8."""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from gpu_util import report, record, rel_err, rel_l2  # noqa: E402

DEV = 'cuda'
HEADS, DH = 8, 64
INNER = HEADS * DH
CAP = 2 ** -8
TOL_S3 = dict(dq=1.2e-3, dk=8e-4, dv=8e-4, dwth=9e-4)                       # measured 5.8e-4, 3.9e-4, 3.6e-4, 4.3e-4
TOL_X = dict(dq=1.4e-3, dk=1.2e-3, dv=1.1e-3, dnull_k=8e-4, dnull_v=8e-4, dwth=9e-4)   # 6.8e-4, 5.9e-4, 5.4e-4, 4.0e-4, 3.5e-4, 4.4e-4
TOL_S_INVARIANT = 2 ** -10
F16_MAX = 65504.0


@pytest.fixture(scope='module')
def K():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from nuwa_pytorch_amd import kernels
    return kernels


@pytest.fixture(scope='module')
def O():
    from oracle import nuwa_oracle
    return nuwa_oracle


def _s2(S):
    return torch.tensor([S, 1.0 / S], dtype=torch.float32, device=DEV)


def _prod_scale(dO):
    """S of the production rule (S * max|dO| in [2^-4, 2^-3)) for this dO"""
    from nuwa_pytorch_amd import ops
    return float(ops._grad_scale(dO.to(DEV))[0])


def _wth():
    return torch.randn(HEADS, HEADS) * 0.5 + torch.eye(HEADS)


# ---------------------------------------------------------------------------------------------------
# 3DNA: amdnuwa_sparse3dna_bwd_f16
# ---------------------------------------------------------------------------------------------------

# (video shape, kernel, dilation, n or None = the full video + nothing, B)
S3_CASES = [((2, 16, 16), (5, 3, 3), (1, 1, 1), None, 2), ((3, 16, 16), (3, 3, 3), (2, 2, 2), 530, 2),
            ((3, 16, 16), (5, 3, 3), (4, 4, 4), 300, 2), ((4, 16, 16), (3, 3, 3), (1, 2, 1), None, 3),
            ((10, 16, 16), (5, 3, 3), (2, 1, 4), 2000, 2), ((10, 16, 16), (5, 3, 3), (4, 4, 4), None, 2)]


class S3Case:
    def __init__(self, K, shape, kern, dil, n, B, seed, v_scale=1.0):
        self.shape, self.kern, self.dil, self.B = shape, kern, dil, B
        self.n = n = shape[0] * shape[1] * shape[2] if n is None else n
        torch.manual_seed(seed)
        qkv = torch.randn(B * n, 3, INNER)
        qkv[:, 2] *= v_scale
        self.qkv16 = qkv.reshape(B * n, 3 * INNER).half()
        self.wth = _wth()
        self.dO = torch.randn(B * n, INNER)
        self.g = K.s3_geom(B, n, shape, kern, dil, HEADS, DH)
        assert K.s3_bwd16_supported(self.g), f'the fp16 3DNA backward must take {shape} {kern} {dil} n={n} B={B}'
        self.S = _prod_scale(self.dO)
        self.q_dev, self.w_dev = self.qkv16.to(DEV), self.wth.to(DEV)

    def run(self, K, S, dO=None):
        """-> (dq, dk, dv) fp32 [B*n, inner] divided by S, dwth, and the fp16 arrays as the kernel left them"""
        dO = self.dO if dO is None else dO
        dO16 = (dO.to(DEV) * S).half()
        dqkv, dwth = K.sparse3dna_bwd16(self.g, self.q_dev, self.w_dev, dO16, _s2(S))
        return [dqkv[:, i * INNER:(i + 1) * INNER].float() / S for i in range(3)], dwth, dqkv

    def ref(self, O, S):
        """oracle gradients on the values the kernel reads at scale S"""
        B, n = self.B, self.n
        dO = (self.dO * S).half().float() / S
        qkv = self.qkv16.float().reshape(B, n, 3, HEADS, DH).requires_grad_(True)
        w = self.wth.clone().requires_grad_(True)
        idx = O.neighbor_table(self.shape, self.kern, self.dil, causal=True)
        o = O.sparse3dna_core(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], w, idx, DH ** -0.5)
        o.backward(dO.reshape(B, n, HEADS, DH))
        gq = qkv.grad.reshape(B * n, 3 * INNER)
        return [gq[:, i * INNER:(i + 1) * INNER] for i in range(3)], w.grad


def _s3_report(tag, got, ref, tol=None):
    (dq, dk, dv), dwth = got
    (rq, rk, rv), rwth = ref
    tol = tol or TOL_S3
    for nm, a, b in (('dq', dq, rq), ('dk', dk, rk), ('dv', dv, rv)):
        report(f's3_bwd16.{nm}{tag}', a, b, tol[nm])
    report(f's3_bwd16.dwth{tag}', dwth, rwth, tol['dwth'])


@pytest.mark.parametrize('case', range(len(S3_CASES)))
def test_sparse3dna_bwd16_vs_oracle(K, O, case):
    shape, kern, dil, n, B = S3_CASES[case]
    c = S3Case(K, shape, kern, dil, n, B, seed=40 + case)
    K.f16_sat_count()
    d, dwth, _ = c.run(K, c.S)
    assert K.f16_sat_count() == 0, 'fp16 stores saturated'
    _s3_report(f'[{shape[0]}x16x16,{kern[0]}{kern[1]}{kern[2]},d{dil[0]}{dil[1]}{dil[2]},n={c.n},B={B}]', (d, dwth), c.ref(O, c.S))


# ---------------------------------------------------------------------------------------------------
# cross attention: xattn6_pack_bwd (fp16 images) -> xattn6_bwd16 -> xattn_kv_grads16 -> xattn_unpack(null_last=True)
# ---------------------------------------------------------------------------------------------------

# (B, n, T).  The fp16 backward's kernels take T from 128 (JP / 32 >= 5 key chunks of 32, key T the null key): T = 128 puts the null key
# alone into the last chunk, 159 fills the last chunk, 160 / 161 open a new one, 287 is the module gate's largest T.
X_CASES = [(2, 100, 128), (3, 70, 159), (2, 130, 160), (2, 33, 161), (4, 300, 200), (2, 2560, 256), (3, 17, 287)]


class XCase:
    def __init__(self, K, B, n, T, seed, round_null=True, qk_scale=1.0):
        self.B, self.n, self.T = B, n, T
        torch.manual_seed(seed)
        self.q16 = (torch.randn(B * n, INNER) / qk_scale).half()
        kv = torch.randn(B * T, 2, INNER)
        kv[:, 0] *= qk_scale
        self.kv16 = kv.reshape(B * T, 2 * INNER).half()
        nk, nv = torch.randn(HEADS, DH), torch.randn(HEADS, DH)
        # the forward reads null_k / null_v in fp32, the fp16 backward images round them: fp16 values leave the two consistent
        self.nk, self.nv = (nk.half().float(), nv.half().float()) if round_null else (nk, nv)
        self.wth = _wth()
        mask = torch.rand(B, T) > 0.3                   # ~30 % of the keys masked
        mask[0, T - 64:] = False                        # text padding: a masked tail
        mask[-1] = False                                # a fully masked sample attends only the null key
        self.mask = mask
        self.dO = torch.randn(B * n, INNER)
        self.g = K.x_geom(B, n, T, HEADS, DH)
        assert K.xattn6_on() and K.xattn6_supported(self.g) and K.xattn_bwd16_ok(self.g) and not K.xattn2_bwd_rc_ok(self.g), \
            f'the fp16 cross-attention backward must take B={B} n={n} T={T}'
        self.S = _prod_scale(self.dO)
        self.dev = dict(q=self.q16.to(DEV), kv=self.kv16.to(DEV), nk=self.nk.to(DEV), nv=self.nv.to(DEV), w=self.wth.to(DEV),
                        m8=mask.to(torch.uint8).to(DEV))

    def run(self, K, S, dO=None, pack_mask=None):
        """the block's chain (ops.XInner fwd / bwd with meta['bwd16']) -> dict of fp16 / fp32 results; dq / dk / dv / dnull divided by S"""
        d, g = self.dev, self.g
        dO = self.dO if dO is None else dO
        dO16 = (dO.to(DEV) * S).half()
        s2 = _s2(S)
        _, stats = K.xattn6_fwd(g, d['q'], K.xattn6_pack(g, d['kv'], d['m8']), d['nk'], d['nv'], d['w'], o_f16='only')
        pk = K.xattn6_pack_bwd(g, d['kv'], d['nk'], d['nv'], d['m8'] if pack_mask is None else pack_mask)
        dq16, dS, Pm, dwth = K.xattn6_bwd16(g, d['q'], dO16, pk, d['w'], stats, s2)
        dKp, dVp = K.xattn_kv_grads16(g, dS, Pm, d['q'], dO16, s2)
        dkv, dnk, dnv = K.xattn_unpack(g, dKp, dVp, lo=True, permuted=True, null_last=True)
        dkv = (dkv.hi.float() + dkv.lo.float()).reshape(self.B, self.T, 2, INNER)
        return dict(dq16=dq16, dq=dq16.float() / S, dk=dkv[:, :, 0], dv=dkv[:, :, 1], dnull_k=dnk, dnull_v=dnv, dwth=dwth,
                    dS=K.xattn_rows(g, dS), Pm=K.xattn_rows(g, Pm), stats=stats)

    def ref(self, O, S):
        B, n, T = self.B, self.n, self.T
        dO = (self.dO * S).half().float() / S
        q = self.q16.float().reshape(B, n, HEADS, DH).requires_grad_(True)
        kv = self.kv16.float().reshape(B, T, 2, HEADS, DH).requires_grad_(True)
        nk, nv, w = (t.clone().requires_grad_(True) for t in (self.nk, self.nv, self.wth))
        o = O.attention_core(q, kv[:, :, 0], kv[:, :, 1], nk, nv, w, self.mask, DH ** -0.5)
        o.backward(dO.reshape(B, n, HEADS, DH))
        gkv = kv.grad.reshape(B, T, 2, INNER)
        return dict(dq=q.grad.reshape(B * n, INNER), dk=gkv[:, :, 0], dv=gkv[:, :, 1], dnull_k=nk.grad, dnull_v=nv.grad, dwth=w.grad)


def _x_report(tag, got, ref, tol=None):
    tol = tol or TOL_X
    for nm in ('dq', 'dk', 'dv', 'dnull_k', 'dnull_v', 'dwth'):
        report(f'xattn_bwd16.{nm}{tag}', got[nm], ref[nm], tol[nm])


@pytest.mark.parametrize('case', range(len(X_CASES)))
def test_cross_attention_bwd16_vs_oracle(K, O, case):
    B, n, T = X_CASES[case]
    c = XCase(K, B, n, T, seed=60 + case)
    K.f16_sat_count()
    r = c.run(K, c.S)
    assert K.f16_sat_count() == 0, 'fp16 stores saturated'
    ref = c.ref(O, c.S)
    _x_report(f'[{B},{n},{T}]', r, ref)
    # masked keys take no part: their dk / dv rows are exactly zero
    off = ~c.mask.to(DEV)
    assert int(off.sum()) > 0 and bool((r['dk'][off] == 0).all()) and bool((r['dv'][off] == 0).all()), 'masked keys must get zero dk / dv'
    # the fully masked sample attends only the null key: softmax over one key, no gradient reaches its queries
    last = slice((B - 1) * n, B * n)
    assert float(r['dq'][last].abs().max()) <= TOL_X['dq'] * float(ref['dq'].abs().max()), 'fully masked sample: dq must vanish'


def test_cross_attention_bwd16_unrounded_null_key(K, O):
    """the forward reads null_k / null_v in fp32, the fp16 backward's images round them to fp16: the mismatch stays inside the tolerance"""
    c = XCase(K, 2, 130, 200, seed=71, round_null=False)
    assert not torch.equal(c.nk.half().float(), c.nk)
    K.f16_sat_count()
    r = c.run(K, c.S)
    assert K.f16_sat_count() == 0, 'fp16 stores saturated'
    _x_report('[unrounded null key]', r, c.ref(O, c.S))


# ---------------------------------------------------------------------------------------------------
# scale handling and edge values
# ---------------------------------------------------------------------------------------------------

# S x 2^-8 puts S max|dO| at [2^-12, 2^-11): most fp16 values are then subnormal (normal from 2^-14) and lose bits -- outside what the
# production rule makes, so the runs agree to 2^-8 there, to 2^-10 from 2^-4 up (the saturation counter stays 0 through 2^8)
S_EXPONENTS = {-8: CAP, -4: TOL_S_INVARIANT, 0: TOL_S_INVARIANT, 4: TOL_S_INVARIANT, 8: TOL_S_INVARIANT}


def test_sparse3dna_bwd16_scale_invariance(K, O):
    """S x 2^k: gradients / S agree with each other (a missing or doubled 1 / S, or a wrong power-of-two factor, moves them by 2^j) and each
    meets the oracle tolerance"""
    c = S3Case(K, (3, 16, 16), (5, 3, 3), (2, 2, 2), 530, 2, seed=81)
    ref = c.ref(O, c.S)
    K.f16_sat_count()
    base = c.run(K, c.S)
    for k, tol in S_EXPONENTS.items():
        S = c.S * 2.0 ** k
        d, dwth, _ = c.run(K, S)
        assert K.f16_sat_count() == 0, f'fp16 stores saturated at S x 2^{k}'
        for nm, a, b in zip(('dq', 'dk', 'dv'), d, base[0]):
            report(f's3_bwd16.S_invariance.{nm}[2^{k}]', a, b, tol)
        report(f's3_bwd16.S_invariance.dwth[2^{k}]', dwth, base[1], tol)
        _s3_report(f'[S x 2^{k}]', (d, dwth), ref, None if k > -8 else dict.fromkeys(TOL_S3, CAP))


def test_cross_attention_bwd16_scale_invariance(K, O):
    c = XCase(K, 2, 300, 256, seed=82)
    ref = c.ref(O, c.S)
    K.f16_sat_count()
    base = c.run(K, c.S)
    for k, tol in S_EXPONENTS.items():
        r = c.run(K, c.S * 2.0 ** k)
        assert K.f16_sat_count() == 0, f'fp16 stores saturated at S x 2^{k}'
        for nm in ('dq', 'dk', 'dv', 'dnull_k', 'dnull_v', 'dwth'):
            report(f'xattn_bwd16.S_invariance.{nm}[2^{k}]', r[nm], base[nm], tol)
        _x_report(f'[S x 2^{k}]', r, ref, None if k > -8 else dict.fromkeys(TOL_X, CAP))


def _check_saturated(name, got16, exact_scaled):
    """a counted saturating store: finite, never beyond +-65504, and +-65504 with the right sign wherever S * gradient is clearly beyond it"""
    got = got16.float().cpu()
    assert bool(torch.isfinite(got).all()), f'{name}: a saturating store must stay finite'
    assert float(got.abs().max()) == F16_MAX, f'{name}: expected values clamped to 65504'
    over = exact_scaled.abs() > 1.01 * F16_MAX
    assert int(over.sum()) > 0, f'{name}: the case must drive S * gradient beyond the fp16 range'
    assert torch.equal(got[over], torch.sign(exact_scaled[over]) * F16_MAX), f'{name}: out-of-range values must clamp to +-65504'


@pytest.mark.parametrize('which,k,q_scale,k_scale,v_scale', [('dq', 17, 1 / 16, 16.0, 1.0), ('dk', 17, 16.0, 1 / 16, 1.0),
                                                          ('dv', 18, 1.0, 1.0, 0.25)])
def test_sparse3dna_bwd16_saturates_and_counts(K, O, which, k, q_scale, k_scale, v_scale):
    """amdnuwa.h (sparse3dna_bwd_f16): dq / dk / dv leave as fp16(S gradient), saturating and counted.  S x 2^k with q / k / v scaled so
    that one output's S * gradient leaves the fp16 range while the scores and dP = dO . v stay as in production (scores unchanged: q and
    k scaled inversely)"""
    c = S3Case(K, (3, 16, 16), (3, 3, 3), (2, 2, 2), 530, 2, seed=83)
    qkv = c.qkv16.float().reshape(-1, 3, INNER) * torch.tensor([q_scale, k_scale, v_scale])[None, :, None]
    c.qkv16 = qkv.reshape(-1, 3 * INNER).half()
    c.q_dev = c.qkv16.to(DEV)
    S = c.S * 2.0 ** k                                 # S max|dO| in [2^(k-4), 2^(k-3)): dO16 itself stays finite
    (rq, rk, rv), _ = c.ref(O, S)
    K.f16_sat_count()
    _, _, dqkv = c.run(K, S)
    assert K.f16_sat_count() > 0, 'saturated stores must be counted'
    for i, (nm, r) in enumerate((('dq', rq), ('dk', rk), ('dv', rv))):
        got = dqkv[:, i * INNER:(i + 1) * INNER]
        if nm == which:
            _check_saturated(f's3 {nm}', got, r * S)
        else:
            assert bool(torch.isfinite(got).all()) and float(got.float().abs().max()) <= F16_MAX, f's3 {nm}'


def test_cross_attention_bwd16_saturates_and_counts(K, O):
    """amdnuwa.h (xattn6_bwd_f16): dq leaves as fp16(S dq), saturating and counted (dS / Pm are plain conversions: kept in range here --
    q / 16 and k x 16 leave the scores, dS and dP' = dO . V as in production and multiply dq by 16)"""
    c = XCase(K, 2, 300, 256, seed=84, qk_scale=16.0)
    S = c.S * 2.0 ** 18
    ref = c.ref(O, S)
    K.f16_sat_count()
    r = c.run(K, S)
    assert K.f16_sat_count() > 0, 'saturated stores must be counted'
    _check_saturated('xattn dq', r['dq16'], ref['dq'] * S)


def test_sparse3dna_bwd16_keeps_nan(K):
    """a NaN in one row of dO: that query's dq is NaN (not +-65504, not finite); the other sample is bit-identical to the clean run"""
    c = S3Case(K, (3, 16, 16), (5, 3, 3), (1, 1, 1), 530, 2, seed=85)
    row = c.n + 77                                     # sample 1
    dO = c.dO.clone()
    dO[row, 5] = float('nan')
    clean, bad = c.run(K, c.S)[0], c.run(K, c.S, dO)[0]
    assert bool(torch.isnan(bad[0][row]).all()), 'the NaN row of dO must give a NaN dq row'
    s0 = slice(0, c.n)
    for nm, a, b in zip(('dq', 'dk', 'dv'), clean, bad):
        assert torch.equal(a[s0], b[s0]), f'{nm} of the other sample changed'


def test_cross_attention_bwd16_keeps_nan(K):
    c = XCase(K, 3, 100, 200, seed=86)
    row = c.n + 41                                     # sample 1
    dO = c.dO.clone()
    dO[row, 300] = float('nan')
    clean, bad = c.run(K, c.S), c.run(K, c.S, dO)
    assert bool(torch.isnan(bad['dq'][row]).all()), 'the NaN row of dO must give a NaN dq row'
    for s in (0, 2):
        q, kv = slice(s * c.n, (s + 1) * c.n), slice(s, s + 1)
        assert torch.equal(clean['dq16'][q], bad['dq16'][q]), f'dq of sample {s} changed'
        assert torch.equal(clean['dk'][kv], bad['dk'][kv]) and torch.equal(clean['dv'][kv], bad['dv'][kv]), f'dk / dv of sample {s} changed'


# ---------------------------------------------------------------------------------------------------
# batch independence and reproducibility (the checks the bf16 siblings have)
# ---------------------------------------------------------------------------------------------------

PICK = (0, 7, 15)
REPEATS = 5


def test_sparse3dna_bwd16_at_batch_16_equals_one_sample_and_repeats(K):
    B, n = 16, 2560
    torch.manual_seed(3)
    wth = _wth().to(DEV)
    for dil in ((1, 1, 1), (2, 2, 2), (4, 4, 4)):
        qkv16 = torch.randn(B * n, 3 * INNER, device=DEV).half()
        dO = torch.randn(B * n, INNER, device=DEV)
        S = _prod_scale(dO)
        s2, dO16 = _s2(S), (dO * S).half()
        g, g1 = K.s3_geom(B, n, (10, 16, 16), (5, 3, 3), dil, HEADS, DH), K.s3_geom(1, n, (10, 16, 16), (5, 3, 3), dil, HEADS, DH)
        assert K.s3_bwd16_supported(g) and K.s3_bwd16_supported(g1)
        dqkv, dwth = K.sparse3dna_bwd16(g, qkv16, wth, dO16, s2)
        for s in PICK:
            rows = slice(s * n, (s + 1) * n)
            d1, _ = K.sparse3dna_bwd16(g1, qkv16[rows].contiguous(), wth, dO16[rows].contiguous(), s2)
            assert torch.equal(dqkv[rows], d1), f'3DNA fp16 backward, dilation {dil[0]}, sample {s}'
        for _ in range(REPEATS - 1):
            d2, w2 = K.sparse3dna_bwd16(g, qkv16, wth, dO16, s2)
            assert torch.equal(d2, dqkv) and torch.equal(w2.view(torch.int32), dwth.view(torch.int32)), \
                f'3DNA fp16 backward not reproducible, dilation {dil[0]}'


def test_cross_attention_bwd16_at_batch_16_equals_one_sample_and_repeats(K):
    B, n, T = 16, 2560, 256

    class Big(XCase):
        def __init__(self):
            self.B, self.n, self.T = B, n, T
            torch.manual_seed(4)
            self.q16, self.kv16 = torch.randn(B * n, INNER).half(), torch.randn(B * T, 2 * INNER).half()
            self.nk, self.nv, self.wth = torch.randn(HEADS, DH).half().float(), torch.randn(HEADS, DH).half().float(), _wth()
            self.mask = torch.rand(B, T) > 0.2
            self.mask[:, T - 64:] = False                  # the benchmark's text padding
            self.dO = torch.randn(B * n, INNER)
            self.g = K.x_geom(B, n, T, HEADS, DH)
            self.S = _prod_scale(self.dO)
            self.dev = dict(q=self.q16.to(DEV), kv=self.kv16.to(DEV), nk=self.nk.to(DEV), nv=self.nv.to(DEV), w=self.wth.to(DEV),
                            m8=self.mask.to(torch.uint8).to(DEV))

    c = Big()
    assert K.xattn_bwd16_ok(c.g) and not K.xattn2_bwd_rc_ok(c.g)
    full = c.run(K, c.S)
    keys = ('stats', 'dq16', 'dS', 'Pm')
    for s in PICK:
        one = XCase.__new__(XCase)
        one.B, one.n, one.T, one.S = 1, n, T, c.S
        one.dO = c.dO[s * n:(s + 1) * n]
        one.g = K.x_geom(1, n, T, HEADS, DH)
        assert K.xattn_bwd16_ok(one.g)
        one.dev = dict(c.dev, q=c.dev['q'][s * n:(s + 1) * n].contiguous(), kv=c.dev['kv'][s * T:(s + 1) * T].contiguous(),
                       m8=c.dev['m8'][s:s + 1].contiguous())
        r1 = one.run(K, c.S)
        for k in keys:
            a = full[k][s * n:(s + 1) * n] if k == 'dq16' else full[k][s:s + 1]
            assert torch.equal(a, r1[k]), f'cross attention fp16 backward, {k} of sample {s}'
        # (dk / dv: the batched TN product over the queries may split that reduction by the batch's size -- fp32 order only)
        for k in ('dk', 'dv'):
            report(f'xattn_bwd16.batch16_vs_single.{k}[{s}]', full[k][s:s + 1], r1[k], 5e-5)
    for _ in range(REPEATS - 1):
        r = c.run(K, c.S)
        for k in keys + ('dk', 'dv', 'dnull_k', 'dnull_v', 'dwth'):
            assert torch.equal(r[k], full[k]), f'cross attention fp16 backward not reproducible: {k}'


# ---------------------------------------------------------------------------------------------------
# the module: one cfg-3 decoder layer, B = 2, ragged context mask, dilations 1 and 4
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dil', [1, 4])
def test_fp16_gradient_backward_module_with_masks_batch_and_dilation(K, O, monkeypatch, dil):
    """'fsx' against '' (the bf16 backward) on one cfg-3 layer: same forward bits, every gradient inside the mode's bound (1.4e-2), the 3DNA
    and cross-attention blocks' own weight gradients no worse than the bf16 backward's, no saturation -- and both fp16 kernels did run"""
    import nuwa_pytorch_amd as A
    import nuwa_pytorch_amd.nuwa_pytorch as M
    dim, video_shape, kernel, T, b = 512, (10, 16, 16), (5, 3, 3), 256, 2
    torch.manual_seed(0)
    tr = M.Transformer(dim=dim, depth=1, causal=True, heads=HEADS, dim_head=DH, cross_attend=True, sparse_3dna_attn=True,
                       sparse_3dna_kernel_size=kernel, sparse_3dna_video_shape=video_shape, sparse_3dna_dilations=(dil,),
                       shift_video_tokens=True)
    with torch.no_grad():
        for n_, p in tr.named_parameters():
            if 'norm' in n_ or n_.endswith('.bias'):
                p.add_(0.1 * torch.randn_like(p))
    P = {k: v.detach().cpu().clone() for k, v in tr.state_dict().items()}
    n = video_shape[0] * video_shape[1] * video_shape[2]
    g = torch.Generator().manual_seed(7 + dil)
    x = torch.randn(b, n, dim, generator=g)
    ctx = torch.randn(b, T, dim, generator=g)
    mask = torch.rand(b, T, generator=g) > 0.3
    mask[0, 190:] = False                                      # ragged: text padding on sample 0 ...
    mask[1] = False                                            # ... and sample 1 sees only the null key
    dy = torch.randn(b, n, dim, generator=g)
    cfg = dict(video_shape=video_shape, kernel_size=kernel, dilations=(dil,), heads=HEADS, depth=1, shift=True)
    Pr = {k: (v.clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in P.items()}
    xr, cr = x.clone().requires_grad_(True), ctx.clone().requires_grad_(True)
    O.decoder_layer(xr, O.sub(Pr, 'layers.0'), cfg, 0, cr, mask).backward(dy)
    tr = tr.to(DEV)
    calls = {'s3': 0, 'x': 0}
    s3_bwd16, x_bwd16 = K.sparse3dna_bwd16, K.xattn6_bwd16

    def spy_s3(*a, **k):
        calls['s3'] += 1
        return s3_bwd16(*a, **k)

    def spy_x(*a, **k):
        calls['x'] += 1
        return x_bwd16(*a, **k)
    monkeypatch.setattr(K, 'sparse3dna_bwd16', spy_s3)
    monkeypatch.setattr(K, 'xattn6_bwd16', spy_x)
    saved = K._BWD_F16
    A.set_precision('bf16x3-fwd')
    try:
        def run(classes):
            K.set_bwd_f16(classes)
            tr.zero_grad(set_to_none=True)
            xd, cd = x.to(DEV).requires_grad_(True), ctx.to(DEV).requires_grad_(True)
            y = tr.forward_layers(xd, context=cd, context_mask=mask.to(DEV))
            y.backward(dy.to(DEV))
            pairs = [('dx', xd.grad, xr.grad), ('dcontext', cd.grad, cr.grad)] + \
                [(k, p.grad, Pr[k].grad) for k, p in tr.named_parameters() if Pr[k].grad is not None]
            return y.detach().clone(), {k: (rel_err(a, b), rel_l2(a, b)) for k, a, b in pairs}
        K.f16_sat_count()
        y0, e0 = run('')
        assert calls == {'s3': 0, 'x': 0}
        y1, e1 = run('fsx')
        assert calls['s3'] >= 1 and calls['x'] >= 1, f'the fp16 attention kernels did not run: {calls}'
        assert K.f16_sat_count() == 0, 'fp16 stores saturated'
        assert torch.equal(y0, y1), 'the fp16-gradient switch must not change the forward'
        for k, (e, l2) in e1.items():
            record(f'cfg3.bwd16_module[d{dil}].{k}', e, l2, 1.4e-2)
        worst = max(e1, key=lambda k: e1[k][0])
        assert e1[worst][0] <= 1.4e-2, (worst, e1[worst])
        for k in e1:
            if k.startswith('layers.0.0.') or k.startswith('layers.0.1.'):          # the 3DNA and the cross-attention block
                assert e1[k][0] <= max(1.05 * e0[k][0], 2e-3), (k, e1[k], e0[k])
    finally:
        K._BWD_F16 = saved
        A.set_precision('bf16')


# ---------------------------------------------------------------------------------------------------
# the context cast (ops._ctx_to_bf) reused across precision modes
# ---------------------------------------------------------------------------------------------------

def test_context_cast_cache_follows_the_precision_mode(K):
    """one context tensor through bf16 -> bf16x3-fwd -> bf16 -> bf16x3 -> bf16x3-fwd: every run equals, bit for bit, a run in the same mode
    on a fresh copy of the context (the cached cast must never hand a hi-only copy to a mode that needs hi + lo, or the reverse)"""
    import nuwa_pytorch_amd as A
    import nuwa_pytorch_amd.nuwa_pytorch as M
    dim, video_shape, T, b = 512, (10, 16, 16), 256, 1
    torch.manual_seed(0)
    tr = M.Transformer(dim=dim, depth=1, causal=True, heads=HEADS, dim_head=DH, cross_attend=True, sparse_3dna_attn=True,
                       sparse_3dna_kernel_size=(5, 3, 3), sparse_3dna_video_shape=video_shape, sparse_3dna_dilations=(2,),
                       shift_video_tokens=True).to(DEV)
    n = video_shape[0] * video_shape[1] * video_shape[2]
    g = torch.Generator().manual_seed(5)
    x = torch.randn(b, n, dim, generator=g).to(DEV)
    context = torch.randn(b, T, dim, generator=g).to(DEV).requires_grad_(True)
    mask = torch.ones(b, T, dtype=torch.bool, device=DEV)
    mask[:, 200:] = False
    dy = torch.randn(b, n, dim, generator=g).to(DEV)

    def run(mode, c):
        A.set_precision(mode)
        tr.zero_grad(set_to_none=True)
        c.grad = None
        xd = x.clone().requires_grad_(True)
        y = tr.forward_layers(xd, context=c, context_mask=mask)
        y.backward(dy)
        out = [y.detach().clone(), xd.grad.clone(), c.grad.clone()] + [p.grad.clone() for p in tr.parameters() if p.grad is not None]
        return out

    modes = ('bf16', 'bf16x3-fwd', 'bf16', 'bf16x3', 'bf16x3-fwd')
    try:
        shared = [run(m, context) for m in modes]              # (first: a fresh copy in between would evict the shared tensor's entry)
        for m, got in zip(modes, shared):
            want = run(m, context.detach().clone().requires_grad_(True))
            assert len(got) == len(want) and all(torch.equal(a, b_) for a, b_ in zip(got, want)), f'mode {m}: the reused context differs'
    finally:
        A.set_precision('bf16')


# ---------------------------------------------------------------------------------------------------
# the GELU behind the GEGLU kernels (common.h norm_cdf_f: |Phi error| <= 3e-7 absolute) over the whole gate range
# ---------------------------------------------------------------------------------------------------

PHI_ERR = 3e-7


def _gate_grid(n):
    x = torch.linspace(-9.0, 9.0, n - 16, dtype=torch.float64)
    tiny = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 1e-12, -1e-12, 1e-7, -1e-7, 1e-4, -1e-4, 0.01, -0.01, 4.5, -4.5, 6.0, -6.0],
                        dtype=torch.float64)
    return torch.cat((x, tiny))


def _gelu64(x):
    """fp64 gelu(x) = x Phi(x) and gelu'(x) = Phi(x) + x phi(x)"""
    phi_cdf = 0.5 * torch.special.erfc(-x / math.sqrt(2.0))
    pdf = torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    return x * phi_cdf, phi_cdf + x * pdf, pdf


def test_gelu_over_the_whole_gate_range(K):
    """geglu_fwd / geglu_bwd (hi + lo pairs) and the epilogue of gemm_nt_geglu_bwd16 (fp16) against fp64 erfc, per element: the header's
    3e-7 bound on Phi (times |x| in gelu), the exponential's relative error in x phi(x), and the rounding of the output format"""
    from nuwa_pytorch_amd.kernels import BF
    FP = 128
    R = 64
    x64 = _gate_grid(R * FP)
    # bf16 hi + lo pairs: the gate values the pair represents exactly
    xf = x64.float()
    hi = xf.to(torch.bfloat16)
    lo = (xf - hi.float()).to(torch.bfloat16)
    xv = hi.double() + lo.double()
    gate = torch.stack((hi, lo)).reshape(2, R, FP)
    one = torch.ones(R, FP, dtype=torch.bfloat16)
    u = BF(torch.cat((one, gate[0]), 1).to(DEV), torch.cat((torch.zeros_like(one), gate[1]), 1).to(DEV))
    y, dy, pdf = _gelu64(xv.reshape(R, FP))
    ax = xv.abs().reshape(R, FP)
    pair_round = 2.0 ** -16                                        # a hi + lo bf16 pair holds 16 significant bits
    K.set_precision('bf16x3')
    try:
        o = K.geglu_fwd(u, FP)
        got = o.hi.double().cpu() + o.lo.double().cpu()
        bound = PHI_ERR * ax + pair_round * y.abs() + 1e-30
        err = (got - y).abs()
        assert bool((err <= bound).all()), f'geglu_fwd: worst x = {float(xv.reshape(R, FP)[(err / bound).argmax() // FP, (err / bound).argmax() % FP]):.6g}'
        dgg = BF(torch.ones(R, FP, dtype=torch.bfloat16, device=DEV), torch.zeros(R, FP, dtype=torch.bfloat16, device=DEV))
        du = K.geglu_bwd(u, dgg, FP)
        got = du.hi.double().cpu() + du.lo.double().cpu()
        for nm, g_, r_, b_ in (('gelu', got[:, :FP], y, PHI_ERR * ax + pair_round * y.abs()),
                               ("gelu'", got[:, FP:], dy, PHI_ERR + 1e-6 * ax * pdf + pair_round * dy.abs())):
            assert bool(((g_ - r_).abs() <= b_ + 1e-30).all()), f'geglu_bwd {nm}: max err {float((g_ - r_).abs().max()):.3e}'
    finally:
        K.set_precision('bf16')
    # the fp16-gradient FF backward: du = fp16(S du) from the GEMM epilogue, dgg = dy16 @ w2T16^T = 1 exactly; gates as bf16
    xb = x64.float().to(torch.bfloat16)
    xv = xb.double().reshape(R, FP)
    y, dy, pdf = _gelu64(xv)
    ub = K.geglu_interleave(torch.cat((torch.ones(R, FP, dtype=torch.bfloat16), xb.reshape(R, FP)), 1), FP, dim=1).to(DEV)
    Kd = 64
    dy16 = torch.zeros(R, Kd, dtype=torch.float16, device=DEV)
    dy16[:, 0] = 1.0
    w2T16 = torch.zeros(FP, Kd, dtype=torch.float16, device=DEV)
    w2T16[:, 0] = 1.0
    assert K.gemm_nt_f16ops_ok(R, FP, Kd, out_bf16=True, geglu_bwd=True)
    du = K.geglu_deinterleave(K.gemm_nt_geglu_bwd16(dy16, w2T16, ub, FP).double().cpu(), FP, dim=1)
    f16_round = 2.0 ** -11
    ax = xv.abs()
    for nm, g_, r_, b_ in (('gelu', du[:, :FP], y, PHI_ERR * ax + f16_round * y.abs()),
                           ("gelu'", du[:, FP:], dy, PHI_ERR + 1e-6 * ax * pdf + f16_round * dy.abs())):
        assert bool(((g_ - r_).abs() <= b_ + 2.0 ** -25).all()), f'gemm_nt_geglu_bwd16 {nm}: max err {float((g_ - r_).abs().max()):.3e}'
