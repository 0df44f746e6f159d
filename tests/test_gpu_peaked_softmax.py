"""Every trainer and decoder attention kernel against float64 on peaked and shifted softmax rows (tests/peaked_util.py), on the MI355X.

The other GPU tests feed torch.randn queries and keys: scores of standard deviation 1, a mean row maximum of the probabilities of
0.02 .. 0.18, a running-maximum rescale factor close to 1 everywhere and no score that would overflow exp without the maximum
subtracted.  Here the rows are sharp, the maximum moves at every key tile (or sits in the first one, or in the masked / causally
invisible keys, or in the null slot) and the scores reach 134 nats.

Tolerances (max-abs error / max-abs reference, logged as gpu_util.report does) are the numbers the flat-input test of the same kernel
and mode asserts (named beside each use): q, k and the null key are exact in every operand type, P <= 1 and the output is a convex mix
of V, so the rounding model behind those numbers does not depend on sharpness.  Three rules are derived, each computed from the float64
reference of the case (peaked_util.x3_shift_term, shift_dq_term, floors):
  * hi + lo modes on the shift recipes add 2^-21 * max |score in the log2 domain| (four fp32 ulps of a score of order 190: fp32 score
    resolution is what limits P there): +9e-5 .. 1.2e-4; measured worst 9.4e-5 against 1e-4 + 1.2e-4;
  * 16-bit dq on the shift recipes adds 2 eps scale max sum_j |dS_ij| |k_jd| / max |dq| (the 96 u common to all keys cancels out of dq
    only while dS is exact; P' and dS are rounded to 16 bits before the product with k): +0.035 .. 0.068 in bf16, +0.009 .. 0.011 in
    fp16; measured 0.017 .. 0.028 (flat bound 2^-6) and 1.8e-3 .. 2.6e-3 (flat bounds 1.2e-3 / 1.4e-3);
  * a gradient whose reference vanishes is measured against the size it has where it does not: d null_k / d null_v against max |dk| /
    max |dv|, and on null_peak dq, dk, dv against the ramp_up reference's maxima (their own maxima are 1e-5 .. 1e-7 of those).  These
    comparisons are absolute ones and carry no relative information (zeros would pass); where a reference does not vanish the test
    asserts that its denominator is its own maximum (dq, dk, dv off null_peak; d null_v on null_peak).
A case collects every comparison before it fails, so one run shows all figures."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import peaked_util as PU  # noqa: E402
from gpu_util import LOG, bf_value, rel_err, rel_l2, record, to_bf_pair  # noqa: E402
from test_gpu_attention_bwd16 import TOL_S3, TOL_X  # noqa: E402

DEV = 'cuda'
SHIFTS = ('shift', 'shift_null0')


@pytest.fixture(scope='module')
def K():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from nuwa_pytorch_amd import kernels
    return kernels


class Checks:
    """report() every comparison of a case (each lands in the parity log), fail at the end with all that missed"""

    def __init__(self, tag, scores, recipe):
        self.tag, self.recipe, self.failed = tag, recipe, []
        self.scores(scores)

    def scores(self, s):
        """the float64 scores of the case the next comparisons belong to: the hi + lo term of the shift recipes comes from them"""
        self.x3_extra = PU.x3_shift_term(s) if self.recipe in SHIFTS else 0.0

    def __call__(self, name, got, ref, tol, x3=False, floor=0.0, extra=0.0, own=False):
        """gpu_util.report with the denominator max(max |ref|, floor) (peaked_util.floors) and the derived additions to tol.
        own=True: this reference does not vanish, so the floor must be inactive (the error is relative to the tensor's own maximum)"""
        name, got = f'peaked.{name}{self.tag}', got.detach().double().cpu()
        tol = tol + (self.x3_extra if x3 else 0.0) + extra
        assert got.shape == ref.shape, f'{name}: shape {tuple(got.shape)} vs {tuple(ref.shape)}'
        assert not own or floor <= float(ref.abs().max()), f'{name}: floor {floor:.3e} above max |ref| {float(ref.abs().max()):.3e}'
        den = max(float(ref.abs().max()), floor, 1e-30)
        e, l2 = float((got - ref).abs().max()) / den, float((got - ref).norm()) / max(float(ref.norm()), floor, 1e-30)
        finite = bool(torch.isfinite(got).all())
        record(name, e, l2, tol, finite)
        if not finite:
            self.failed.append(f'{name}: non-finite values')
        elif not e <= tol:
            self.failed.append(f'{name}: rel err {e:.3e} (l2 {l2:.3e}) > tol {tol:.1e}')

    def done(self):
        assert not self.failed, '\n'.join(self.failed)


def _dev(t, dt=None):
    return (t if dt is None else t.to(dt)).contiguous().to(DEV)


def _flat(t, rows):
    return t.reshape(rows, -1)


def _bf16(t):
    return _dev(t, torch.bfloat16)


def _grad_scale(K, dO):
    from nuwa_pytorch_amd import ops
    return float(ops._grad_scale(dO.to(DEV))[0])


def _s2(S):
    return torch.tensor([S, 1.0 / S], dtype=torch.float32, device=DEV)


# ---------------------------------------------------------------------------------------------------
# cross-attention: three generations
# ---------------------------------------------------------------------------------------------------

def _xattn_gen1_gen2(K, c, chk, x3, gen2=True):
    """xattn_pack -> xattn_fwd / xattn_bwd / xattn_kv_grads -> xattn_unpack, and (bf16, gen2) the second design xattn2_fwd / xattn2_bwd.
    Tolerances: test_gpu_kernels.py::test_cross_attention_core"""
    B, n, T, heads, dh = c.B, c.n, c.T, c.heads, c.dh
    inner = heads * dh
    rnd = PU.exact if x3 else PU.bf_round
    ref = c.reference(rnd)
    fl = PU.floors(c, rnd)
    sx = PU.shift_dq_term(ref, 2.0 ** -9) if c.recipe in SHIFTS and not x3 else 0.0
    m = 'x3' if x3 else 'bf16'
    g = K.x_geom(B, n, T, heads, dh)
    qp = to_bf_pair(_dev(_flat(c.q, B * n)), x3)
    kvp = to_bf_pair(_dev(torch.stack((c.k, rnd(c.v)), 2).reshape(B * T, 2 * inner)), x3)
    dop = to_bf_pair(_dev(_flat(rnd(c.dO), B * n)), x3)
    w, nk, nv = _dev(c.wth), _dev(c.nk), _dev(rnd(c.nv))
    pk = K.xattn_pack(g, kvp, nk, nv, _dev(c.mask, torch.uint8))
    val = (lambda p: bf_value(p)) if x3 else (lambda p: p.hi.float())
    ref_kv = torch.stack((ref['dk'], ref['dv']), 2)
    o, P, Pm = K.xattn_fwd(g, qp, pk, w)
    chk(f'xattn_fwd.{m}', val(o).reshape(B, n, heads, dh), ref['o'], 5e-5 if x3 else 2 ** -7, x3)
    dq, dS, dwth = K.xattn_bwd(g, dop, pk, w, P)
    chk(f'xattn_dq.{m}', val(dq).reshape(B, n, heads, dh), ref['dq'], 1e-4 if x3 else 2 ** -6, x3, floor=fl['dq'], extra=sx)
    chk(f'xattn_dwth.{m}', dwth, ref['dwth'], 2e-4 if x3 else 2 ** -6, x3)
    dKp, dVp = K.xattn_kv_grads(g, dS, Pm, qp, dop)
    dkv, dnk, dnv = K.xattn_unpack(g, dKp, dVp, lo=x3)
    chk(f'xattn_dkv.{m}', val(dkv).reshape(B, T, 2, heads, dh), ref_kv, 1e-4 if x3 else 2 ** -6, x3, floor=fl['dkv'])
    chk(f'xattn_dnull_k.{m}', dnk, ref['dnk'], 1e-4 if x3 else 2 ** -6, x3, floor=fl['dnk'])
    chk(f'xattn_dnull_v.{m}', dnv, ref['dnv'], 1e-4 if x3 else 2 ** -6, x3, floor=fl['dnv'], own=c.recipe == 'null_peak')
    if x3 or not gen2:
        return
    assert K.xattn2_supported(g, qp), 'the second design must take this geometry'
    o2, stats = K.xattn2_fwd(g, qp, pk, w)
    chk('xattn2_fwd', o2.hi.float().reshape(B, n, heads, dh), ref['o'], 2 ** -7)
    dq2, dS2, Pm2, dwth2 = K.xattn2_bwd(g, qp, dop, pk, w, stats)
    chk('xattn2_dq', dq2.hi.float().reshape(B, n, heads, dh), ref['dq'], 2 ** -6, floor=fl['dq'], extra=sx)
    chk('xattn2_dwth', dwth2, ref['dwth'], 2 ** -6)
    dKp2, dVp2 = K.xattn_kv_grads(g, dS2, Pm2, qp, dop)
    dkv2, dnk2, dnv2 = K.xattn_unpack(g, dKp2, dVp2, lo=False, permuted=True)
    chk('xattn2_dkv', dkv2.hi.float().reshape(B, T, 2, heads, dh), ref_kv, 2 ** -6, floor=fl['dkv'])
    chk('xattn2_dnull_k', dnk2, ref['dnk'], 2 ** -6, floor=fl['dnk'])
    chk('xattn2_dnull_v', dnv2, ref['dnv'], 2 ** -6, floor=fl['dnv'], own=c.recipe == 'null_peak')


def _xattn6(K, c, chk):
    """xattn6_pack -> xattn6_fwd on fp16 and on bf16 operands, xattn6_pack_bwd -> xattn6_bwd on the bf16 forward's statistics.
    Tolerances: test_cross_attention_xattn6_fwd (1e-3 fp16, 2^-7 bf16), test_cross_attention_xattn6_bwd (2^-6)"""
    B, n, T, heads, dh = c.B, c.n, c.T, c.heads, c.dh
    inner = heads * dh
    g = K.x_geom(B, n, T, heads, dh)
    assert K.xattn6_supported(g)
    m8, w, nk = _dev(c.mask, torch.uint8), _dev(c.wth), _dev(c.nk)
    for f16 in (True, False):
        dt, rnd = (torch.float16, PU.f16_round) if f16 else (torch.bfloat16, PU.bf_round)
        ref = c.reference(rnd)
        fl = PU.floors(c, rnd)
        sx = PU.shift_dq_term(ref, 2.0 ** -9) if c.recipe in SHIFTS else 0.0
        q16 = _dev(_flat(c.q, B * n), dt)
        kv16 = _dev(torch.stack((c.k, c.v), 2).reshape(B * T, 2 * inner), dt)
        nv = _dev(rnd(c.nv))
        o, stats = K.xattn6_fwd(g, q16, K.xattn6_pack(g, kv16, m8), nk, nv, w)
        chk(f'xattn6_fwd.{"f16" if f16 else "bf16"}', bf_value(o).reshape(B, n, heads, dh), ref['o'], 1e-3 if f16 else 2 ** -7)
    if not K.xattn6_bwd_ok(g):
        return False
    qp, kvp = K.BF(q16, None), K.BF(kv16, None)
    dop = K.BF(_bf16(_flat(c.dO, B * n)), None)
    pkb = K.xattn6_pack_bwd(g, kv16, nk, nv, m8)
    dq, dS, Pm, dwth = K.xattn6_bwd(g, qp, dop, pkb, w, stats)
    chk('xattn6_bwd.dq', dq.hi.float().reshape(B, n, heads, dh), ref['dq'], 2 ** -6, floor=fl['dq'], extra=sx)
    chk('xattn6_bwd.dwth', dwth, ref['dwth'], 2 ** -6)
    dKp, dVp = K.xattn_kv_grads(g, dS, Pm, qp, dop)
    dkv, dnk, dnv = K.xattn_unpack(g, dKp, dVp, lo=False, permuted=True, null_last=True)
    chk('xattn6_bwd.dkv', dkv.hi.float().reshape(B, T, 2, heads, dh), torch.stack((ref['dk'], ref['dv']), 2), 2 ** -6, floor=fl['dkv'])
    chk('xattn6_bwd.dnull_k', dnk, ref['dnk'], 2 ** -6, floor=fl['dnk'])
    chk('xattn6_bwd.dnull_v', dnv, ref['dnv'], 2 ** -6, floor=fl['dnv'], own=c.recipe == 'null_peak')
    return True


def _xattn_bwd16(K, c, chk):
    """the fp16-gradient form: xattn6_fwd (fp16) -> xattn6_pack_bwd (fp16 images) -> xattn6_bwd16 -> xattn_kv_grads16 -> xattn_unpack.
    Tolerances: test_gpu_attention_bwd16.py TOL_X; reference on the values the kernels read (dO16 / S)"""
    B, n, T, heads, dh = c.B, c.n, c.T, c.heads, c.dh
    inner = heads * dh
    g = K.x_geom(B, n, T, heads, dh)
    if not K.xattn_bwd16_ok(g):
        return False
    dO = _flat(c.dO, B * n)
    S = _grad_scale(K, dO)
    dO16 = (dO.to(DEV) * S).half()
    ref = c.reference(PU.f16_round, dO=(dO16.float().cpu() / S).reshape(B, n, heads, dh), key='bwd16')
    fl = PU.floors(c, PU.f16_round, dO=(dO16.float().cpu() / S).reshape(B, n, heads, dh), key='bwd16')
    sx = PU.shift_dq_term(ref, 2.0 ** -11) if c.recipe in SHIFTS else 0.0
    q16 = _dev(_flat(c.q, B * n), torch.float16)
    kv16 = _dev(torch.stack((c.k, c.v), 2).reshape(B * T, 2 * inner), torch.float16)
    m8, w, nk, nv = _dev(c.mask, torch.uint8), _dev(c.wth), _dev(c.nk), _dev(PU.f16_round(c.nv))
    s2 = _s2(S)
    K.f16_sat_count()
    _, stats = K.xattn6_fwd(g, q16, K.xattn6_pack(g, kv16, m8), nk, nv, w, o_f16='only')
    pk = K.xattn6_pack_bwd(g, kv16, nk, nv, m8)
    dq16, dS, Pm, dwth = K.xattn6_bwd16(g, q16, dO16, pk, w, stats, s2)
    dKp, dVp = K.xattn_kv_grads16(g, dS, Pm, q16, dO16, s2)
    dkv, dnk, dnv = K.xattn_unpack(g, dKp, dVp, lo=True, permuted=True, null_last=True)
    assert K.f16_sat_count() == 0, 'fp16 stores saturated'
    dkv = bf_value(dkv).reshape(B, T, 2, heads, dh)
    chk('xattn_bwd16.dq', (dq16.float() / S).reshape(B, n, heads, dh), ref['dq'], TOL_X['dq'], floor=fl['dq'], extra=sx)
    chk('xattn_bwd16.dk', dkv[:, :, 0], ref['dk'], TOL_X['dk'], floor=fl['dk'])
    chk('xattn_bwd16.dv', dkv[:, :, 1], ref['dv'], TOL_X['dv'], floor=fl['dv'])
    chk('xattn_bwd16.dnull_k', dnk, ref['dnk'], TOL_X['dnull_k'], floor=fl['dnk'])
    chk('xattn_bwd16.dnull_v', dnv, ref['dnv'], TOL_X['dnull_v'], floor=fl['dnv'], own=c.recipe == 'null_peak')
    chk('xattn_bwd16.dwth', dwth, ref['dwth'], TOL_X['dwth'])
    return True


@pytest.mark.parametrize('n,T', PU.X_SHAPES)
@pytest.mark.parametrize('recipe', PU.RECIPES)
def test_cross_attention_kernels(K, recipe, n, T):
    """8 heads x 64, B = 2, keys across one to nine 32-key chunks (33: two chunks, 130 / 256 / 287: the fp16 backward's range and the
    packed kernels' limit), a key mask on sample 1 (every key of sample 0 hidden on masked_peak)"""
    c = PU.AttentionCase(recipe, 2, n, T, 8, 64, seed=n + T)
    c.check()
    chk = Checks(f'[{recipe},{n}x{T}]', c.scores, recipe)
    _xattn_gen1_gen2(K, c, chk, False)
    _xattn_gen1_gen2(K, c, chk, True)
    ran6 = _xattn6(K, c, chk)
    ran16 = _xattn_bwd16(K, c, chk)
    slots = K.x_geom(2, n, T, 8, 64).JP                 # the padded key slots: the M of the batched dK / dV product on chunk-major dS / P'
    assert ran6 == (128 < slots <= 384), 'xattn6_bwd runs where the whole-M TN kernel takes its chunk-major arrays: 128 < JP <= 384'
    assert ran16 == ran6, 'the fp16-gradient chain takes the same contexts'
    chk.done()


@pytest.mark.parametrize('n,T', [(70, 33), (130, 287)])
@pytest.mark.parametrize('recipe', PU.RECIPES)
def test_cross_attention_first_generation_4x32(K, recipe, n, T):
    c = PU.AttentionCase(recipe, 2, n, T, 4, 32, seed=n + T + 1)
    c.check()
    chk = Checks(f'[{recipe},{n}x{T},4x32]', c.scores, recipe)
    _xattn_gen1_gen2(K, c, chk, False, gen2=False)
    _xattn_gen1_gen2(K, c, chk, True, gen2=False)
    chk.done()


# ---------------------------------------------------------------------------------------------------
# cattn: causal and rectangular
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('recipe,heads,dh,n,T,causal,masked', PU.CATTN_PARAMS)
def test_cattn_kernels(K, recipe, heads, dh, n, T, causal, masked):
    """cattn_fwd on fp16 and bf16 operands and cattn_bwd.  On the causal ramp every query's invisible future holds the largest scores.
    Tolerances: test_cattn_kernels_against_the_oracle / test_rectangular_kernels_against_the_oracle (1e-3 fp16, 2e-2 bf16, 7e-2 backward)"""
    B, inner = 2, heads * dh
    c = PU.AttentionCase(recipe, B, n, T, heads, dh, seed=n + T + heads, masked=masked, causal=causal)
    c.check()
    chk = Checks(f'[{recipe},{heads}x{dh},{n}x{T},c={int(causal)},m={int(masked)}]', c.scores, recipe)
    g = K.cattn_geom(B, n, heads, dh, causal=causal, n_keys=None if causal else T)
    assert K.cattn_supported(g)
    md = _dev(c.mask, torch.uint8) if masked else None
    w, nk = _dev(c.wth), _dev(c.nk)
    for f16 in (True, False):
        dt, rnd = (torch.float16, PU.f16_round) if f16 else (torch.bfloat16, PU.bf_round)
        ref = c.reference(rnd)
        fl, sx = PU.floors(c, rnd), 0.0                # (the flat 7e-2 of the backward needs no shift term)
        qd = _dev(_flat(c.q, B * n), dt)
        kvd = _dev(torch.cat((_flat(c.k, B * T), _flat(c.v, B * T)), 1), dt)
        nv = _dev(rnd(c.nv))
        o, stats = K.cattn_fwd(g, qd, kvd[:, :inner], kvd[:, inner:], nk, nv, w, md)
        chk(f'cattn_fwd.{"f16" if f16 else "bf16"}', bf_value(o).reshape(B, n, heads, dh), ref['o'], 1e-3 if f16 else 2e-2)
    dO = _bf16(_flat(c.dO, B * n))
    dq, dkv, dwth, dnk, dnv = K.cattn_bwd(g, qd, kvd[:, :inner], kvd[:, inner:], dO, nk, nv, w, stats, md)
    chk('cattn_bwd.dq', dq.hi.float().reshape(B, n, heads, dh), ref['dq'], 7e-2, floor=fl['dq'], extra=sx)
    dkvg = dkv.hi.float().reshape(B, T, 2, heads, dh)
    chk('cattn_bwd.dk', dkvg[:, :, 0], ref['dk'], 7e-2, floor=fl['dk'])
    chk('cattn_bwd.dv', dkvg[:, :, 1], ref['dv'], 7e-2, floor=fl['dv'])
    chk('cattn_bwd.dW', dwth, ref['dwth'], 7e-2)
    chk('cattn_bwd.dnull_k', dnk, ref['dnk'], 7e-2, floor=fl['dnk'])
    chk('cattn_bwd.dnull_v', dnv, ref['dnv'], 7e-2, floor=fl['dnv'], own=c.recipe == 'null_peak')
    chk.done()


# ---------------------------------------------------------------------------------------------------
# Sparse3DNA
# ---------------------------------------------------------------------------------------------------

def _rel_dev(c):
    """oracle layout (h, J - 1) -> kernel layout [J, heads], slot 0 = <bos>"""
    return None if c.rel is None else torch.cat((torch.zeros(1, c.heads), c.rel.t()), 0).contiguous().to(DEV)


def _qkv(c, rnd):
    R = c.B * c.n
    return torch.cat((_flat(c.q, R), _flat(c.k, R), _flat(rnd(c.v), R)), 1)


@pytest.mark.parametrize('shape', range(len(PU.S3_SHAPES)))
@pytest.mark.parametrize('recipe', PU.S3_RECIPES)
def test_sparse3dna_kernels(K, recipe, shape):
    """sparse3dna_fwd / sparse3dna_bwd in the bf16 and the hi + lo form (the narrow VALU kernel, the MFMA band kernels, the wide-grid
    kernels); on the MFMA geometries also the fp16 core, the multi-row tiles (2 and 4 rows), the packed backward workspace against the
    fp32 pair and the fp16-gradient backward.  The ramp runs over the token index; `null` is the <bos> slot.
    Tolerances: test_sparse3dna_core (2^-7 / 2^-6, 3e-5 / 5e-5, dW_th 1e-4), with the bias test_sparse3dna_core_rel_pos_bias_on_the_mfma_kernels
    and test_wide_sparse3dna_core_rel_pos_bias (dW_th and d(bias) 2^-6 bf16, 1e-4 hi + lo), test_sparse3dna_fwd_f16_core (6e-4),
    test_sparse3dna_fwd_multi_row_tiles (2^-7 / 6e-4), test_gpu_attention_bwd16.py TOL_S3"""
    from nuwa_pytorch_amd import _lib
    L = _lib.lib()
    vshape, kern, dil, heads, dh, n = PU.S3_SHAPES[shape]
    c = PU.S3Case(recipe, vshape, kern, dil, heads, dh, n, seed=shape)
    c.check()
    B, n, inner = c.B, c.n, heads * dh
    chk = Checks(f'[{recipe},{vshape},{dil},{n}]', c.scores, recipe)
    g = K.s3_geom(B, n, vshape, kern, dil, heads, dh)
    w, rel = _dev(c.wth), _rel_dev(c)
    mfma = vshape[2] == 16 and (heads, dh) == (8, 64)
    cols = (('dq', slice(0, inner)), ('dk', slice(inner, 2 * inner)), ('dv', slice(2 * inner, 3 * inner)))
    for x3 in (False, True):
        rnd = PU.exact if x3 else PU.bf_round
        ref = c.reference(rnd)
        fl = PU.floors(c, rnd)
        sx = PU.shift_dq_term(ref, 2.0 ** -9) if c.recipe in SHIFTS and not x3 else 0.0
        m = 'x3' if x3 else 'bf16'
        assert K.s3_supported(vshape, kern, dil, heads, dh, lo=x3)
        qkvp = to_bf_pair(_dev(_qkv(c, rnd)), x3)
        dop = to_bf_pair(_dev(_flat(rnd(c.dO), B * n)), x3)
        val = (lambda p: bf_value(p)) if x3 else (lambda p: p.hi.float())
        o = K.sparse3dna_fwd(g, qkvp, w, rel_bias=rel)
        chk(f's3_fwd.{m}', val(o).reshape(B, n, heads, dh), ref['o'], 3e-5 if x3 else 2 ** -7, x3)
        dqkv, dwth, drel = K.sparse3dna_bwd(g, qkvp, w, dop, rel_bias=rel)
        got = val(dqkv)
        for nm, sl in cols:
            chk(f's3_bwd_{nm}.{m}', got[:, sl].reshape(B, n, heads, dh), ref[nm], 5e-5 if x3 else 2 ** -6, x3, floor=fl[nm], extra=sx if nm == 'dq' else 0.0)
        chk(f's3_bwd_dwth.{m}', dwth, ref['dwth'], 1e-4 if rel is None or x3 else 2 ** -6, x3)
        if rel is not None:
            chk(f's3_bwd_drel.{m}', drel[1:].t(), ref['drel'], 1e-4 if x3 else 2 ** -6, x3)
        if mfma and not x3:
            try:                                        # tuning key 24 = 1: the fp32 ds / P' pair instead of the packed words -- same bits
                L.amdnuwa_set_tuning(24, 1)
                d32, w32, _ = K.sparse3dna_bwd(g, qkvp, w, dop, rel_bias=rel)
            finally:
                L.amdnuwa_set_tuning(24, 0)
            assert torch.equal(d32.hi, dqkv.hi) and torch.equal(w32, dwth), 'packed backward workspace differs from the fp32 pair'
    if mfma:
        assert K.s3_f16_supported(g)
        ref = c.reference(PU.f16_round)
        q16 = _qkv(c, PU.f16_round)
        qkv16 = K.BF(_bf16(q16), None, _dev(q16, torch.float16))
        qkvb = to_bf_pair(_dev(_qkv(c, PU.bf_round)), False)
        ref_b = c.reference(PU.bf_round)
        o = K.sparse3dna_fwd(g, qkv16, w, rel_bias=rel)
        chk('s3_fwd_f16', bf_value(o).reshape(B, n, heads, dh), ref['o'], 6e-4)
        for rows in (2, 4):                             # tuning key 16: query rows per workgroup of the MFMA forward
            try:
                L.amdnuwa_set_tuning(16, rows)
                o16 = K.sparse3dna_fwd(g, qkv16, w, rel_bias=rel)
                ob = K.sparse3dna_fwd(g, qkvb, w, rel_bias=rel)
            finally:
                L.amdnuwa_set_tuning(16, 0)
            chk(f's3_tile{rows}.f16', bf_value(o16).reshape(B, n, heads, dh), ref['o'], 6e-4)
            chk(f's3_tile{rows}.bf16', ob.hi.float().reshape(B, n, heads, dh), ref_b['o'], 2 ** -7)
        if rel is None:
            assert K.s3_bwd16_supported(g)
            dO = _flat(c.dO, B * n)
            S = _grad_scale(K, dO)
            dO16 = (dO.to(DEV) * S).half()
            r16 = c.reference(PU.f16_round, dO=(dO16.float().cpu() / S).reshape(B, n, heads, dh), key='bwd16')
            fl = PU.floors(c, PU.f16_round, dO=(dO16.float().cpu() / S).reshape(B, n, heads, dh), key='bwd16')
            sx = PU.shift_dq_term(r16, 2.0 ** -11) if c.recipe in SHIFTS else 0.0
            K.f16_sat_count()
            d16, dwth16 = K.sparse3dna_bwd16(g, qkv16.f16, w, dO16, _s2(S))
            assert K.f16_sat_count() == 0, 'fp16 stores saturated'
            for nm, sl in cols:
                chk(f's3_bwd16.{nm}', (d16[:, sl].float() / S).reshape(B, n, heads, dh), r16[nm], TOL_S3[nm], floor=fl[nm], extra=sx if nm == 'dq' else 0.0)
            chk('s3_bwd16.dwth', dwth16, r16['dwth'], TOL_S3['dwth'])
    chk.done()


@pytest.mark.parametrize('shape', range(len(PU.XC2_SHAPES)))
@pytest.mark.parametrize('recipe', PU.RECIPES)
def test_cross2dna_kernels(K, recipe, shape):
    """cross2dna_fwd / cross2dna_bwd (SparseCross2DNA's windowed queries: the window kernels pointed at the sketch context, with a null
    key and a key mask) in the bf16 and the hi + lo form, on the narrow VALU, the MFMA and the wide-grid kernels.  Row 0 of every
    sample (<bos>) is the module's glue arithmetic: the kernels leave it alone and it is not compared.
    Tolerances: test_sparse_cross_2dna_hip_vs_oracle / test_wide_sparse_cross_2dna_hip_vs_oracle (2e-2 / 7e-2 bf16, 1e-3 / 2e-3 hi + lo)"""
    fmap, kern, dil, frames, heads, dh, n = PU.XC2_SHAPES[shape]
    c = PU.Cross2DNACase(recipe, fmap, kern, dil, frames, heads, dh, n, seed=20 + shape)
    c.check()
    B, T, inner = c.B, c.T, heads * dh
    chk = Checks(f'[{recipe},{fmap},{kern},{dil},{frames},{n}]', c.scores, recipe)
    tpf = fmap * fmap
    g = K.s3_geom(B, n, (-(-(n - 1) // tpf), fmap, fmap), (frames, kern, kern), (1, dil, dil), heads, dh, causal=False)
    m8, w = _dev(c.mask, torch.uint8), _dev(c.wth)
    for x3 in (False, True):
        rnd = PU.exact if x3 else PU.bf_round
        ref = c.reference(rnd)
        fl = PU.floors(c, rnd)
        m = 'x3' if x3 else 'bf16'
        tol, gtol = (1e-3, 2e-3) if x3 else (2e-2, 7e-2)
        assert K.s3_supported((1, fmap, fmap), (frames, kern, kern), (1, dil, dil), heads, dh, causal=False, lo=x3)
        qp = to_bf_pair(_dev(_flat(c.q, B * n)), x3)
        kvp = to_bf_pair(_dev(torch.cat((_flat(c.k, B * T), _flat(rnd(c.v), B * T)), 1)), x3)
        dop = to_bf_pair(_dev(_flat(rnd(c.dO), B * n)), x3)
        nk, nv = to_bf_pair(_dev(c.nk.reshape(-1)), x3), to_bf_pair(_dev(rnd(c.nv).reshape(-1)), x3)
        rows = lambda p: bf_value(p).reshape(B, n, heads, dh)[:, 1:]
        o = K.cross2dna_fwd(g, qp, kvp, nk, nv, m8, w, T)
        chk(f'cross2dna_fwd.{m}', rows(o), ref['o'], tol, x3)
        dq, dkv, dnk, dnv, dwth = K.cross2dna_bwd(g, qp, kvp, nk, nv, m8, w, dop, T)
        chk(f'cross2dna_bwd.dq.{m}', rows(dq), ref['dq'], gtol, x3, floor=fl['dq'])
        dkv = bf_value(dkv)
        chk(f'cross2dna_bwd.dk.{m}', dkv[:, :inner].reshape(B, T, heads, dh), ref['dk'], gtol, x3, floor=fl['dk'])
        chk(f'cross2dna_bwd.dv.{m}', dkv[:, inner:].reshape(B, T, heads, dh), ref['dv'], gtol, x3, floor=fl['dv'])
        chk(f'cross2dna_bwd.dnull_k.{m}', dnk.reshape(heads, dh), ref['dnk'], gtol, x3, floor=fl['dnk'])
        chk(f'cross2dna_bwd.dnull_v.{m}', dnv.reshape(heads, dh), ref['dnv'], gtol, x3, floor=fl['dnv'], own=recipe == 'null_peak')
        chk(f'cross2dna_bwd.dwth.{m}', dwth, ref['dwth'], gtol, x3)
    chk.done()


# ---------------------------------------------------------------------------------------------------
# the single-query kernels
# ---------------------------------------------------------------------------------------------------

S3_DECODE_SHAPES = [((3, 4, 4), (3, 3, 3), (1, 1, 1), 2, 32), ((2, 8, 8), (5, 3, 3), (1, 2, 4), 4, 32)]


@pytest.mark.parametrize('shape', range(len(S3_DECODE_SHAPES)))
@pytest.mark.parametrize('recipe', PU.S3_RECIPES)
def test_s3_decode(K, recipe, shape):
    """s3_decode fed row by row against every row of the window attention.  Tolerances: test_s3_decode_rows_equal_full_attention"""
    vshape, kern, dil, heads, dh = S3_DECODE_SHAPES[shape]
    c = PU.S3Case(recipe, vshape, kern, dil, heads, dh, None, seed=10 + shape)
    c.check()
    B, n, inner = c.B, c.n, heads * dh
    chk = Checks(f'[{recipe},{vshape},{dil}]', c.scores, recipe)
    g = K.s3_geom(B, n, vshape, kern, dil, heads, dh)
    w, rel = _dev(c.wth), _rel_dev(c)
    pos = torch.zeros(1, dtype=torch.int32, device=DEV)
    for x3 in (False, True):
        rnd = PU.exact if x3 else PU.bf_round
        flat = _dev(_qkv(c, rnd)).reshape(B, n, 3 * inner)
        cache = K.zeros_bf((B, n, 2 * inner), DEV, lo=x3)
        rows = []
        for t in range(n):
            pos.fill_(t)
            rows.append(bf_value(K.s3_decode(g, to_bf_pair(flat[:, t].contiguous(), x3), cache, pos, w, rel)))
        chk(f's3_decode.{"x3" if x3 else "bf16"}', torch.stack(rows, 1).reshape(B, n, heads, dh), c.reference(rnd)['o'], 3e-5 if x3 else 2 ** -7, x3)
    chk.done()


@pytest.mark.parametrize('T', PU.XDEC_T)
@pytest.mark.parametrize('recipe', PU.RECIPES)
def test_xattn_decode(K, recipe, T):
    """one query per sample over the packed keys.  Tolerances: test_xattn_decode_equals_cross_attention_core"""
    B, heads, dh = 3, 8, 64
    inner = heads * dh
    c = PU.AttentionCase(recipe, B, 1, T, heads, dh, seed=T)
    c.check()
    chk = Checks(f'[{recipe},T={T}]', c.scores, recipe)
    g = K.x_geom(B, 1, T, heads, dh)
    for x3 in (False, True):
        rnd = PU.exact if x3 else PU.bf_round
        kvp = to_bf_pair(_dev(torch.stack((c.k, rnd(c.v)), 2).reshape(B * T, 2 * inner)), x3)
        pk = K.xattn_pack(g, kvp, _dev(c.nk), _dev(rnd(c.nv)), _dev(c.mask, torch.uint8))
        o = K.xattn_decode(g, to_bf_pair(_dev(_flat(c.q, B)), x3), pk, _dev(c.wth))
        chk(f'xattn_decode.{"x3" if x3 else "bf16"}', bf_value(o).reshape(B, 1, heads, dh), c.reference(rnd)['o'], 3e-5 if x3 else 2 ** -7, x3)
    chk.done()


@pytest.mark.parametrize('T,heads,dh', [(T, 8, 64) for T in PU.ROWS_T] + [(300, 5, 32)])
@pytest.mark.parametrize('recipe', PU.RECIPES)
def test_attn_decode_rows(K, recipe, T, heads, dh):
    """T + 1 = 127, 128, 129 slots around one 128-slot split, 301 and 1001 slots over three and eight splits (the ramps cross them: the
    join of the splits rescales by exp2(m_split - m) at every one); with and without the talking-heads bias and the key mask; the
    window starts at cache row 5 and every row outside it is NaN.  Tolerances: test_kernel_against_the_fp32_formula"""
    B, inner, first, extra = 3, heads * dh, 5, 7
    gen = torch.Generator().manual_seed(T)
    bias = torch.randn(heads, generator=gen) * 0.3
    fd = torch.full((1,), first, dtype=torch.int32, device=DEV)
    chk = None
    for masked in (True, False):
        if recipe == 'masked_peak' and not masked:
            continue
        c = PU.AttentionCase(recipe, B, 1, T, heads, dh, seed=T + heads, masked=masked)
        c.check()
        chk = chk or Checks(f'[{recipe},T={T},{heads}x{dh}]', c.scores, recipe)
        chk.scores(c.scores)
        for x3 in (False, True):
            rnd = PU.exact if x3 else PU.bf_round
            kv = torch.full((B, first + T + extra, 2 * inner), float('nan'))
            kv[:, first:first + T] = torch.cat((c.k.reshape(B, T, inner), rnd(c.v).reshape(B, T, inner)), -1)
            kvp, qp = to_bf_pair(_dev(kv), x3), to_bf_pair(_dev(_flat(c.q, B)), x3)
            for use_bias in (False, True):
                o = K.attn_decode_rows(qp, kvp, fd, T, heads, dh, _dev(c.nk), _dev(rnd(c.nv)), _dev(c.wth), th_bias=_dev(bias) if use_bias else None,
                                       mask_u8=_dev(c.mask, torch.uint8) if masked else None)
                ref = c.reference(rnd, th_bias=bias.double() if use_bias else None, key=(rnd, use_bias))['o']
                chk(f'attn_decode_rows.{"x3" if x3 else "bf16"}[bias={int(use_bias)},mask={int(masked)}]', bf_value(o).reshape(B, 1, heads, dh), ref,
                    3e-5 if x3 else 2 ** -7, x3)
    chk.done()


# ---------------------------------------------------------------------------------------------------
# record only: genuine fp32 q and k (nonzero lo planes), sharp gains 1 .. 8, 'bf16x3' against 'bf16x3-fwd'
# ---------------------------------------------------------------------------------------------------

GAINS = (1, 2, 4, 8)


def _err(got, ref):
    got = got.detach().cpu()
    assert bool(torch.isfinite(got).all())
    return rel_err(got, ref), rel_l2(got, ref)


def _sweep_table(name, table):
    import json
    import os
    for mode, rows in table.items():
        for gain, errs in rows.items():
            for k, (e, l2) in errs.items():
                record(f'peaked.sweep.{name}[{mode},gain={gain}].{k}', e, l2, None)
    path = os.path.join(os.path.dirname(LOG), 'peaked_softmax_sweep.json')        # beside the parity log
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        old = json.load(open(path)) if os.path.exists(path) else {}
        old[name] = {m: {str(gn): {k: v[0] for k, v in errs.items()} for gn, errs in rows.items()} for m, rows in table.items()}
        json.dump(old, open(path, 'w'), indent=1, sort_keys=True)
    except OSError:
        pass
    for gain in GAINS:
        for k, (e, _) in table['bf16x3'][gain].items():
            assert e <= table['bf16x3-fwd'][gain][k][0], (name, gain, k, e, table['bf16x3-fwd'][gain][k][0])


def test_sweep_cross_attention_fp32_inputs(K):
    """'bf16x3': the hi + lo kernels (xattn_fwd / xattn_bwd / xattn_kv_grads) on the fp32 values.  'bf16x3-fwd': the fp16 forward core
    (xattn6_fwd) on the fp16 copies and the bf16 backward (xattn6_bwd), which rebuilds P from bf16 scores against the statistics the
    more exact forward saved.  Reference: float64 on the unrounded fp32 values.  Asserted: finite, and 'bf16x3' no worse than
    'bf16x3-fwd' at each gain; the figures go to the parity log and to peaked_softmax_sweep.json beside it"""
    B, n, T, heads, dh = 2, 130, 256, 8, 64
    inner = heads * dh
    table = {'bf16x3': {}, 'bf16x3-fwd': {}}
    for gain in GAINS:
        c = PU.AttentionCase('flat', B, n, T, heads, dh, seed=77)
        gen = torch.Generator().manual_seed(78)
        c.q, c.k, c.nk = torch.randn(B, n, heads, dh, generator=gen), torch.randn(B, T, heads, dh, generator=gen) * gain, torch.randn(heads, dh, generator=gen)
        ref = c.reference(PU.exact, key=('sweep', gain))
        ref_kv = torch.stack((ref['dk'], ref['dv']), 2)
        g = K.x_geom(B, n, T, heads, dh)
        q32, kv32 = _dev(_flat(c.q, B * n)), _dev(torch.stack((c.k, c.v), 2).reshape(B * T, 2 * inner))
        dO32 = _dev(_flat(c.dO, B * n))
        m8, w, nk, nv = _dev(c.mask, torch.uint8), _dev(c.wth), _dev(c.nk), _dev(c.nv)
        qp, kvp, dop = to_bf_pair(q32, True), to_bf_pair(kv32, True), to_bf_pair(dO32, True)
        pk = K.xattn_pack(g, kvp, nk, nv, m8)
        o, P, Pm = K.xattn_fwd(g, qp, pk, w)
        dq, dS, _ = K.xattn_bwd(g, dop, pk, w, P)
        dkv, _, _ = K.xattn_unpack(g, *K.xattn_kv_grads(g, dS, Pm, qp, dop), lo=True)
        table['bf16x3'][gain] = dict(o=_err(bf_value(o).reshape(B, n, heads, dh), ref['o']), dq=_err(bf_value(dq).reshape(B, n, heads, dh), ref['dq']),
                                     dkv=_err(bf_value(dkv).reshape(B, T, 2, heads, dh), ref_kv))
        assert K.xattn6_bwd_ok(g)
        o, stats = K.xattn6_fwd(g, q32.half(), K.xattn6_pack(g, kv32.half(), m8), nk, nv, w)
        qb, kvb, dob = K.BF(q32.to(torch.bfloat16), None), kv32.to(torch.bfloat16), K.BF(dO32.to(torch.bfloat16), None)
        dq, dS, Pm, _ = K.xattn6_bwd(g, qb, dob, K.xattn6_pack_bwd(g, kvb, nk, nv, m8), w, stats)
        dkv, _, _ = K.xattn_unpack(g, *K.xattn_kv_grads(g, dS, Pm, qb, dob), lo=False, permuted=True, null_last=True)
        table['bf16x3-fwd'][gain] = dict(o=_err(bf_value(o).reshape(B, n, heads, dh), ref['o']), dq=_err(dq.hi.float().reshape(B, n, heads, dh), ref['dq']),
                                         dkv=_err(dkv.hi.float().reshape(B, T, 2, heads, dh), ref_kv))
    _sweep_table('cross_attention[130x256,8x64]', table)


def test_sweep_sparse3dna_fp32_inputs(K):
    """the same for Sparse3DNA on (2,16,16) / (5,3,3): 'bf16x3' = sparse3dna_fwd / sparse3dna_bwd on hi + lo pairs, 'bf16x3-fwd' = the
    fp16 core forward and the bf16 backward on the bf16 copies.  sparse3dna_bwd takes no statistics from the forward (it recomputes the
    softmax itself), so here the 'bf16x3-fwd' row is the fp16 forward and an independent bf16 backward, not a statistics mismatch"""
    vshape, kern, dil, heads, dh = (2, 16, 16), (5, 3, 3), (1, 1, 1), 8, 64
    inner = heads * dh
    table = {'bf16x3': {}, 'bf16x3-fwd': {}}
    cols = (('dq', slice(0, inner)), ('dk', slice(inner, 2 * inner)), ('dv', slice(2 * inner, 3 * inner)))
    for gain in GAINS:
        c = PU.S3Case('flat', vshape, kern, dil, heads, dh, None, seed=79)
        B, n = c.B, c.n
        gen = torch.Generator().manual_seed(80)
        c.q, c.k = torch.randn(B, n, heads, dh, generator=gen), torch.randn(B, n, heads, dh, generator=gen) * gain
        ref = c.reference(PU.exact, key=('sweep', gain))
        g = K.s3_geom(B, n, vshape, kern, dil, heads, dh)
        w = _dev(c.wth)
        qkv32, dO32 = _dev(_qkv(c, PU.exact)), _dev(_flat(c.dO, B * n))
        sh = lambda t: t.reshape(B, n, heads, dh)
        qkvp, dop = to_bf_pair(qkv32, True), to_bf_pair(dO32, True)
        o = K.sparse3dna_fwd(g, qkvp, w)
        d = bf_value(K.sparse3dna_bwd(g, qkvp, w, dop)[0])
        table['bf16x3'][gain] = dict(o=_err(sh(bf_value(o)), ref['o']), **{nm: _err(sh(d[:, sl]), ref[nm]) for nm, sl in cols})
        o = K.sparse3dna_fwd(g, K.BF(qkv32.to(torch.bfloat16), None, qkv32.half()), w)
        d = K.sparse3dna_bwd(g, K.BF(qkv32.to(torch.bfloat16), None), w, K.BF(dO32.to(torch.bfloat16), None))[0].hi.float()
        table['bf16x3-fwd'][gain] = dict(o=_err(sh(bf_value(o)), ref['o']), **{nm: _err(sh(d[:, sl]), ref[nm]) for nm, sl in cols})
    _sweep_table('sparse3dna[(2,16,16),(5,3,3)]', table)
