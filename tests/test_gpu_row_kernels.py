"""The row-reducing kernels against float64 on ill-conditioned rows (tests/row_inputs_util.py), on the MI355X: the LayerNorm family
(elementwise.hip), GEGLU on every finite bf16 gate (elementwise.hip, dropout.hip, the GEMM epilogues of gemm.hip), cross entropy in all
three kernels, fused linear + cross entropy (the CE epilogue of gemm.hip), the two VAE norms (vae.hip) and amdnuwa_colsum.

The other GPU tests feed these kernels randn * 2 + 0.5 rows, randn * 3 logits and randn gates against fp32 torch.  Here a row's mean is a
thousand times its spread, its variance lies below eps, one channel is 4096, the logits overflow exp() unless the maximum is subtracted,
the target lies 60 nats below the maximum, and the gate takes every finite bf16 value.

Tolerances are the flat numbers the existing test of the same quantity asserts (named beside each use) plus the terms derived in
row_inputs_util.py, each computed from the float64 reference of the case.  Where a reference vanishes by construction (dx on the two
special gradients) the error is measured against the randn-gradient reference's maximum: that comparison is ABSOLUTE and carries no
relative information.  A case collects every comparison before it fails (test_gpu_peaked_softmax.Checks, which is why the entries of
the parity log (gpu_util.LOG) read 'peaked.rows. ...').  Statistics, GEGLU and row losses are bounded per row / per element: their log
entries hold the worst error / bound ratio against a tolerance of 1."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import row_inputs_util as RU  # noqa: E402
from gpu_util import bf_value, record, to_bf_pair  # noqa: E402
from test_gpu_peaked_softmax import Checks  # noqa: E402

DEV = 'cuda'


@pytest.fixture(scope='module')
def K():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from nuwa_pytorch_amd import kernels
    return kernels


class RowChecks(Checks):
    """Checks without a softmax recipe; every entry is logged as 'peaked.rows.<name>[case]'"""

    def __init__(self, tag):
        super().__init__(tag, None, 'rows')

    def __call__(self, name, *a, **k):
        super().__call__('rows.' + name, *a, **k)


def _dev(t, dt=None):
    return (t if dt is None else t.to(dt)).contiguous().to(DEV)


def _mx(t):
    return float(t.abs().max())


def _ratio(chk, name, ratio, ok=True, what='err / bound'):
    """a per-row / per-element bound: log the worst error / bound ratio against 1 and collect the failure"""
    name = f'peaked.rows.{name}{chk.tag}'
    record(name, ratio, ratio, 1.0, bool(ok))
    if not ok:
        chk.failed.append(f'{name}: non-finite values')
    elif not ratio <= 1.0:
        chk.failed.append(f'{name}: {what} {ratio:.3e} > 1')


def _same(chk, name, a, b):
    if not torch.equal(a, b):
        chk.failed.append(f'rows.{name}{chk.tag}: not bit-identical ({int((a != b).sum())} of {a.numel()} differ)')


def _s2(S):
    return torch.tensor([S, 1.0 / S], dtype=torch.float32, device=DEV)


def _pair_value(t):
    """the value a hi + lo pair holds for the fp32 number t (what a pair-writing kernel must produce for an exact result t)"""
    hi = t.to(torch.bfloat16)
    return hi.float() + (t - hi.float()).to(torch.bfloat16).float()


# ---------------------------------------------------------------------------------------------------
# A. LayerNorm family
# ---------------------------------------------------------------------------------------------------

def _ln_stats(chk, name, mean, rstd, f):
    e = RU.ln_stat_errors(mean.cpu(), rstd.cpu(), f)
    fin = bool(torch.isfinite(mean).all() and torch.isfinite(rstd).all())
    _ratio(chk, f'{name}.mean', e['mean'], fin)
    _ratio(chk, f'{name}.rstd', e['rstd'], fin)


def _ln_backward(K, chk, x, xd, m, r, wd, w, f, tag, ia=None, flat_dx=3e-5):
    """ln_bwd on the three gradient kinds: bf pair out + dsum, and the fp32 accumulate form.  Flat tolerances: test_layernorm_fwd_bwd's
    ln_bwd_dx_bf 3e-5, ln_bwd_dw / db 1e-5, ln_bwd_dsum 1e-4, ln_bwd_dx_acc 1e-5 (stable: test_stable_layernorm's dx 2e-5, dw 1e-5)"""
    R, D = x.shape
    ref0 = RU.ln_bwd64(RU.ln_dy('randn', f, w), f, w)
    dres = torch.randn(R, D, generator=torch.Generator().manual_seed(11))
    for kind in RU.DY_KINDS:
        dy = RU.ln_dy(kind, f, w)
        ref = RU.ln_bwd64(dy, f, w)
        # (dx and its column sums vanish on the two special gradients: measured against the randn reference -- absolute comparisons)
        fl = {q: (_mx(ref0[q]) if kind != 'randn' and q in ('dx', 'dsum') else 0.0) for q in ('dx', 'dw', 'db', 'dsum')}
        den = {q: max(_mx(ref[q]), fl[q]) for q in fl}
        term = {q: RU.ln_term(q, f, w, den[q], dy) for q in fl}
        dyd = _dev(dy)
        if ia is None:
            dx, dw, db, ds = K.ln_bwd(dyd, xd, m, r, wd, to_bf=True, want_dsum=True)
            chk(f'ln_bwd_dx_bf.{tag}{kind}', bf_value(dx), ref['dx'], flat_dx, floor=fl['dx'], extra=term['dx'], own=kind == 'randn')
            chk(f'ln_bwd_dsum.{tag}{kind}', ds, ref['dsum'], 1e-4, floor=fl['dsum'], extra=term['dsum'], own=kind == 'randn')
            dx2, dw2, db2, _ = K.ln_bwd(dyd, xd, m, r, wd, dres=_dev(dres))
            ref_acc = ref['dx'] + dres.double()
            chk(f'ln_bwd_dx_acc.{tag}{kind}', dx2, ref_acc, 1e-5, extra=RU.ln_term('dx', f, w, _mx(ref_acc)))
            _same(chk, f'ln_bwd_dw(acc form == bf form).{tag}{kind}', dw2, dw)
        else:
            dx, dw, db, _ = K.ln_bwd(dyd, xd, m, r, wd, inv_amax=ia)
            chk(f'stable_ln_dx.{tag}{kind}', dx, ref['dx'], 2e-5, floor=fl['dx'], extra=term['dx'], own=kind == 'randn')
        chk(f'ln_bwd_dw.{tag}{kind}', dw, ref['dw'], 1e-5, extra=term['dw'])
        chk(f'ln_bwd_db.{tag}{kind}', db, ref['db'], 1e-5)


@pytest.mark.parametrize('D', RU.LN_D)
@pytest.mark.parametrize('recipe', RU.LN_RECIPES)
def test_layernorm_family_on_ill_conditioned_rows(K, recipe, D):
    """ln_fwd (pre, post + resid, minus), ln_post_pre_fwd, ln_bwd (bf pair out, dres accumulate, want_dsum), ln_bwd_chain and the
    fp16-gradient forms; R = 37 leaves the last workgroup one row, D covers NV = 1, 2, 4 ragged and full and the NV border 256"""
    R = RU.LN_R
    x = RU.ln_rows(recipe, R, D)
    w, b = RU.ln_params(D)
    gen = torch.Generator().manual_seed(7)
    resid = torch.randn(R, D, generator=gen)
    f = RU.ln64(x, w, b)
    RU.check_ln_conditions(recipe, x, f)
    chk = RowChecks(f'[{recipe},{D}]')
    xd, wd, bd, rd = _dev(x), _dev(w), _dev(b), _dev(resid)
    ty = lambda ref: RU.ln_term('y', f, w, _mx(ref))
    K.set_precision('bf16x3')
    try:
        out, m, r, _ = K.ln_fwd(xd, wd, bd)
        chk('ln_fwd_pre', bf_value(out), f['y'], 2e-5, extra=ty(f['y']))                                # ln_fwd_pre 2e-5
        _ln_stats(chk, 'ln_fwd_pre', m, r, f)
        yo, m2, r2 = K.ln_fwd(xd, wd, bd, resid=rd)
        post = f['y'] + resid.double()
        chk('ln_fwd_post', yo, post, 2e-6, extra=ty(post))                                              # ln_fwd_post 2e-6
        _same(chk, 'mean(post == pre)', m2, m)
        _same(chk, 'rstd(post == pre)', r2, r)
        ym, _, _ = K.ln_fwd(xd, wd, bd, resid=rd, minus=True)
        yn, _, _ = K.ln_fwd(xd, wd, bd, resid=-rd)
        _same(chk, 'ln_fwd_post_minus == -(post of -resid)', ym, -yn)
        chk('ln_fwd_post_minus', ym, resid.double() - f['y'], 2e-6, extra=ty(resid.double() - f['y']))  # ln_fwd_post_minus 2e-6
        if recipe == 'const':
            # x - mean == 0 exactly: the output is b (as a hi + lo pair / added to the residual in one fp32 rounding), rstd == eps^-1/2
            _same(chk, 'const: pre == pair(b)', bf_value(out).cpu(), _pair_value(b)[None].expand(R, D))
            _same(chk, 'const: post == resid + b', yo.cpu(), resid + b)
            _same(chk, 'const: mean == 3', m.cpu(), torch.full((R,), 3.0))
        _ln_backward(K, chk, x, xd, m2, r2, wd, w, f, '')
        # ---- chained backward: pre-norm backward of block k + 1 (rows x) and post-norm backward of block k (rows y_prev) in one pass
        yprev = RU.ln_rows(recipe, R, D, seed=1)
        wp, _bp = RU.ln_params(D, seed=1)
        fp = RU.ln64(yprev, wp, torch.zeros(D))
        dh, g = RU.ln_dy('randn', f, w, seed=2), RU.ln_dy('randn', f, w, seed=3)
        ypd, wpd, dhd, gd = _dev(yprev), _dev(wp), _dev(dh), _dev(g)
        _, mp, rp = K.ln_fwd(ypd, wpd, _dev(torch.zeros(D)), resid=torch.zeros(R, D, device=DEV))
        dx, dw, db, dyp, dwp, dbp, dsp = K.ln_bwd_chain(dhd, xd, m2, r2, wd, gd, ypd, mp, rp, wpd, want_dsum=True)
        dx_a, dw_a, db_a, _ = K.ln_bwd(dhd, xd, m2, r2, wd, dres=gd)
        dy_a, dwp_a, dbp_a, dsp_a = K.ln_bwd(dx_a, ypd, mp, rp, wpd, to_bf=True, want_dsum=True)
        _same(chk, 'ln_bwd_chain.dx == separate', dx, dx_a)
        _same(chk, 'ln_bwd_chain.dy_prev.hi == separate', dyp.hi, dy_a.hi)
        _same(chk, 'ln_bwd_chain.dy_prev.lo == separate', dyp.lo, dy_a.lo)
        for nm, u, v in (('dw', dw, dw_a), ('db', db, db_a), ('dwp', dwp, dwp_a), ('dbp', dbp, dbp_a), ('dsp', dsp, dsp_a)):
            chk(f'ln_bwd_chain.{nm}_vs_separate', u, v.double().cpu(), 2e-6)                            # ln_bwd_chain.* 2e-6
        r1 = RU.ln_bwd64(dh, f, w)
        dx_ref = g.double() + r1['dx']
        chk('ln_bwd_chain.dx', dx, dx_ref, 2e-5, extra=RU.ln_term('dx', f, w, _mx(dx_ref)))             # ln_bwd_chain.dx 2e-5
        chk('ln_bwd_chain.dw', dw, r1['dw'], 2e-5, extra=RU.ln_term('dw', f, w, _mx(r1['dw']), dh))     # ln_bwd_chain.dw 2e-5
        # (the second stage's input is the fp32 dx the first stage wrote: its float64 reference starts from those values)
        r2_ = RU.ln_bwd64(dx.cpu(), fp, wp)
        scale = max(_mx(dx_ref), 1.0)            # ln_term's dx form assumes a unit-size gradient: this stage's is of size max|dx|
        chk('ln_bwd_chain.dy_prev', bf_value(dyp), r2_['dx'], 3e-5, extra=scale * RU.ln_term('dx', fp, wp, _mx(r2_['dx'])))   # 3e-5
        chk('ln_bwd_chain.dw_prev', dwp, r2_['dw'], 2e-5, extra=RU.ln_term('dw', fp, wp, _mx(r2_['dw']), dx.cpu()))
        chk('ln_bwd_chain.db_prev', dbp, r2_['db'], 2e-5)
        # ---- fp16 gradients: dy_out = fp16(S dx), saturating and counted; dh_in = fp16(S dh); fp32 dy scaled by the device scalar 1 / S
        S = 2.0 ** 10
        s2 = _s2(S)
        dy = RU.ln_dy('randn', f, w)
        ref = RU.ln_bwd64(dy, f, w)
        K.f16_sat_count()
        dy16, dw16, db16, ds16 = K.ln_bwd(_dev(dy), xd, m2, r2, wd, to_f16=s2, want_dsum=True)
        sat = K.f16_sat_count()
        top = S * _mx(ref['dx'])
        dx32, dw32, db32, _ = K.ln_bwd(_dev(dy), xd, m2, r2, wd)
        _same(chk, 'ln_bwd.f16_out: dw == fp32 form', dw16, dw32)
        _same(chk, 'ln_bwd.f16_out: db == fp32 form', db16, db32)
        lim = RU.F16_MAX / S
        den16 = min(_mx(ref['dx']), lim)
        # (+ half the spacing of fp16's subnormals, 2^-25 / S: on the huge rows dx is 2^-40 of dy)
        chk('ln_bwd.f16_out', dy16.t.float() / S, ref['dx'].clamp(-lim, lim), 2 ** -10,                 # ln_bwd.f16_out 2^-10
            extra=RU.ln_term('dx', f, w, den16) + 2.0 ** -25 / S / den16)
        # saturation is reported exactly where the float64 S dx leaves fp16's range (1 % either side of 65504 is left undecided)
        if top > RU.F16_MAX * 1.01 and sat == 0:
            chk.failed.append(f'rows.f16_sat_count{chk.tag}: 0 although S max|dx| = {top:.3e}')
        if top < RU.F16_MAX * 0.99 and sat != 0:
            chk.failed.append(f'rows.f16_sat_count{chk.tag}: {sat} although S max|dx| = {top:.3e}')
        if recipe == 'near_const':
            assert top > RU.F16_MAX * 1.01
        if recipe in ('offset', 'outlier', 'huge'):
            assert top < RU.F16_MAX * 0.99
        dh16 = K.G16((_dev(dh) * S).half(), s2)
        dhv = dh16.t.float().cpu() / S
        got, gw, gb, _ = K.ln_bwd(dh16, xd, m2, r2, wd, dres=gd)
        r16 = RU.ln_bwd64(dhv, f, w)
        acc = g.double() + r16['dx']
        chk('ln_bwd.f16_in', got, acc, 1e-5, extra=RU.ln_term('dx', f, w, _mx(acc)))                    # ln_bwd_dx_acc 1e-5
        chk('ln_bwd.f16_in.dw', gw, r16['dw'], 1e-5, extra=RU.ln_term('dw', f, w, _mx(r16['dw']), dhv))
        sc = K.ln_bwd(_dev(dy), xd, m2, r2, wd, dres=gd, dy_scale2=s2)
        pl = K.ln_bwd(_dev(dy) * (1.0 / S), xd, m2, r2, wd, dres=gd)
        _same(chk, 'ln_bwd.dy_scale2 == pre-scaled dy (a power of two)', sc[0], pl[0])
        _same(chk, 'ln_bwd.dy_scale2.dw', sc[1], pl[1])
    finally:
        K.set_precision('bf16')
    # ---- post-norm + residual fused with the next pre-norm (the default 'bf16' mode, as test_layernorm_post_pre_chain: h is bf16)
    w2, b2 = RU.ln_params(D, seed=2)
    xo_a, m_a, r_a = K.ln_fwd(xd, wd, bd, resid=rd)
    h_a, m1_a, r1_a, _ = K.ln_fwd(xo_a, _dev(w2), _dev(b2))
    xo, mm, rr, h, m1, r1 = K.ln_post_pre_fwd(xd, rd, wd, bd, _dev(w2), _dev(b2))
    for name, u, v in (('xo', xo, xo_a), ('m', mm, m_a), ('r', rr, r_a), ('h', h.hi, h_a.hi), ('m1', m1, m1_a), ('r1', r1, r1_a)):
        _same(chk, f'ln_post_pre.{name} == separate', u, v)
    chk('ln_post_pre.x', xo, post, 2e-5, extra=ty(post))                                                # ln_post_pre.x 2e-5
    f2 = RU.ln64(xo.cpu(), w2, b2)                      # (the second norm's input is the fp32 row the first wrote)
    chk('ln_post_pre.h', h.hi.float(), f2['y'], 8e-3, extra=RU.ln_term('y', f2, w2, _mx(f2['y'])))      # ln_post_pre.h 8e-3
    _ln_stats(chk, 'ln_post_pre.next', m1, r1, f2)
    chk.done()


def test_layernorm_token_shift_on_offset_rows(K):
    """(ntok, fmap) = (23, 4) at D = 64 on the offset recipe: the forward shift folded into the pre-norm store, the inverse shift into the
    backward's gradient read (test_layernorm_fwd_with_folded_token_shift 2e-5, test_layernorm_bwd_inverse_shift 1e-5)"""
    from oracle import nuwa_oracle as O
    B, ntok, fmap, D = 2, 23, 4, 64
    R = B * ntok
    x = RU.ln_rows('offset', R, D)
    w, b = RU.ln_params(D)
    f = RU.ln64(x, w, b)
    RU.check_ln_conditions('offset', x, f)
    chk = RowChecks('[offset,shift]')
    xs = x.double().reshape(B, ntok, D).requires_grad_(True)
    hs = O.shift_video_tokens(O.layer_norm(xs, w.double(), b.double()), fmap)
    g = torch.randn(B, ntok, D, generator=torch.Generator().manual_seed(5))
    hs.backward(g.double())
    K.set_precision('bf16x3')
    try:
        out, m, r, _ = K.ln_fwd(_dev(x), _dev(w), _dev(b), shift=(ntok, fmap))
        chk('ln_fwd_shift', bf_value(out).reshape(B, ntok, D), hs.detach(), 2e-5, extra=RU.ln_term('y', f, w, _mx(hs.detach())))
        dx, dw, db, _ = K.ln_bwd(_dev(g.reshape(R, D)), _dev(x), m, r, _dev(w), shift=(ntok, fmap))
        ref = xs.grad.reshape(R, D)
        chk('ln_bwd_inverse_shift', dx, ref, 1e-5, extra=RU.ln_term('dx', f, w, _mx(ref)))
    finally:
        K.set_precision('bf16')
    chk.done()


@pytest.mark.parametrize('D', RU.LN_D)
@pytest.mark.parametrize('recipe', RU.STABLE_RECIPES)
def test_stable_layernorm_on_outlier_and_negative_rows(K, recipe, D):
    """StableLayerNorm divides by the row maximum (no abs): 4096 on the outlier rows, a negative number where every entry is negative
    (test_stable_layernorm: fwd 2e-5, dx 2e-5, dw 1e-5)"""
    R = RU.LN_R
    x = RU.ln_rows(recipe, R, D)
    w, b = RU.ln_params(D)
    f = RU.ln64(x, w, b, stable=True)
    RU.check_ln_conditions(recipe, x, f, stable=True)
    chk = RowChecks(f'[stable,{recipe},{D}]')
    K.set_precision('bf16x3')
    try:
        xd, wd = _dev(x), _dev(w)
        out, m, r, ia = K.ln_fwd(xd, wd, _dev(b), stable=True)
        chk('stable_ln_fwd', bf_value(out), f['y'], 2e-5, extra=RU.ln_term('y', f, w, _mx(f['y'])))
        _ln_stats(chk, 'stable_ln', m, r, f)
        chk('stable_ln_inv_amax', ia, f['ia'], 1e-6)                       # one fp32 division
        _ln_backward(K, chk, x, xd, m, r, wd, w, f, '', ia=ia)
    finally:
        K.set_precision('bf16')
    chk.done()


# ---------------------------------------------------------------------------------------------------
# B. GEGLU: every finite bf16 gate
# ---------------------------------------------------------------------------------------------------

BF_EPS, PAIR_EPS, F16_EPS = 2.0 ** -8, 2.0 ** -16, 2.0 ** -11


def _gg(chk, name, got, r, key, eps, out_max=RU.BF16_MAX):
    bd = RU.geglu_bounds(r, eps, out_max, floor=2.0 ** -25 if out_max == RU.F16_MAX else 2.0 ** -126)
    got = got.detach().float().cpu()
    worst, ok = RU.geglu_errors(got, r[key], bd[key], bd['ok'][key], out_max)
    _ratio(chk, name, worst, ok)
    if eps == PAIR_EPS and key == 'y':
        # logged beside the documented |abs error| of norm_cdf_f: the part of the error the pair's rounding cannot explain, per unit of
        # |a g| -- a lower estimate of the largest Phi error among the 65280 gates (the assertion is the per-element bound above)
        ag = (r['a'] * r['g']).abs()
        sel = bd['ok'][key] & (ag > 1e-30) & torch.isfinite(got)
        est = float((((got.double() - r[key]).abs() - RU.out_rounding(r[key], eps)).clamp(min=0) / ag.clamp(min=1e-30))[sel].max())
        record(f'peaked.rows.{name}.phi_abs_error{chk.tag}', est, est, RU.PHI_B, True)


def _gg_du(chk, name, du, r, FP, eps):
    du = du.detach().float().cpu()
    _gg(chk, f'{name}.da', du[:, :FP], r, 'da', eps)
    _gg(chk, f'{name}.dg', du[:, FP:], r, 'dg', eps)


def _zero_below_minus_9(chk, name, y, r):
    """gates at or below -9: Phi rounds to 0 exactly, the output is +-0 times a"""
    sel = r['g'] <= -9.0
    if not bool((y.detach().float().cpu()[sel] == 0).all()):
        chk.failed.append(f'rows.{name}{chk.tag}: a gate <= -9 gave a nonzero output')


def test_geglu_on_every_finite_bf16_gate(K):
    """geglu_fwd / geglu_bwd plain and hi + lo, [a | g] and interleaved, the generic kernels (FP = 12), the dropout forms with every
    element kept and scale 1"""
    FP = RU.GEGLU_FP
    u, d = RU.geglu_inputs()
    r = RU.geglu64(u, d, FP)
    chk = RowChecks('[all bf16 gates]')
    R = u.shape[0]
    uil = K.geglu_interleave(u, FP, dim=1).contiguous()
    keep = torch.ones(R, FP, dtype=torch.bool, device=DEV)
    for lo, eps in ((False, BF_EPS), (True, PAIR_EPS)):
        m = 'x3' if lo else 'bf16'
        ub, db, ub_il = to_bf_pair(_dev(u), lo), to_bf_pair(_dev(d), lo), to_bf_pair(_dev(uil), lo)
        o = K.geglu_fwd(ub, FP)
        val = bf_value if lo else (lambda p: p.hi.float())
        _gg(chk, f'geglu_fwd.{m}', val(o), r, 'y', eps)
        _zero_below_minus_9(chk, f'geglu_fwd.{m}', val(o), r)
        du = K.geglu_bwd(ub, db, FP)
        _gg_du(chk, f'geglu_bwd.{m}', val(du), r, FP, eps)
        o_il = K.geglu_fwd(ub_il, FP, interleaved=True)
        _same(chk, f'geglu_il_fwd.{m}.hi == [a|g] form', o_il.hi, o.hi)
        du_il = K.geglu_bwd(ub_il, db, FP, interleaved=True)
        _same(chk, f'geglu_il_bwd.{m}.hi == [a|g] form', K.geglu_deinterleave(du_il.hi, FP, dim=1), du.hi)
        if lo:
            _same(chk, 'geglu_il_fwd.x3.lo', o_il.lo, o.lo)
            _same(chk, 'geglu_il_bwd.x3.lo', K.geglu_deinterleave(du_il.lo, FP, dim=1), du.lo)
        # dropout with every element kept and scale 1: the identity on the gate output, the plain backward on the gradient
        # (a pair is re-split from hi + lo: the same VALUE -- a tie may split differently, and an overflowed pair (inf, -inf) reads as NaN)
        od = K.geglu_dropout_fwd(o, keep, 1.0)
        fin = torch.isfinite(val(o))
        _same(chk, f'geglu_dropout_fwd.{m}', val(od)[fin], val(o)[fin])
        if not lo:
            _same(chk, 'geglu_dropout_fwd.bf16.hi', od.hi, o.hi)
        dud = K.geglu_il_bwd_dropout(ub_il, db, keep, 1.0, FP)
        _same(chk, f'geglu_il_bwd_dropout.{m}.hi == geglu_il_bwd', dud.hi, du_il.hi)
        if lo:
            _same(chk, 'geglu_il_bwd_dropout.x3.lo', dud.lo, du_il.lo)
        _gg_du(chk, f'geglu_il_bwd_dropout.{m}', K.geglu_deinterleave(val(dud), FP, dim=1), r, FP, eps)
    # the generic kernels: FP % 8 != 0
    FP2 = 12
    u2 = torch.cat((u[:, :FP].reshape(-1, FP2), u[:, FP:].reshape(-1, FP2)), 1).contiguous()
    d2 = d.reshape(-1, FP2).contiguous()
    r2 = RU.geglu64(u2, d2, FP2)
    for lo, eps in ((False, BF_EPS), (True, PAIR_EPS)):
        m = 'x3' if lo else 'bf16'
        ub, db = to_bf_pair(_dev(u2), lo), to_bf_pair(_dev(d2), lo)
        val = bf_value if lo else (lambda p: p.hi.float())
        o = K.geglu_fwd(ub, FP2)
        _gg(chk, f'geglu_fwd_generic.{m}', val(o), r2, 'y', eps)
        _zero_below_minus_9(chk, f'geglu_fwd_generic.{m}', val(o), r2)
        _gg_du(chk, f'geglu_bwd_generic.{m}', val(K.geglu_bwd(ub, db, FP2)), r2, FP2, eps)
    # the fp16 dropout form on an fp16 gate output: the fp16 copy is the input, the bf16 copy its rounding
    u16, _ = RU.geglu_inputs(fp16_exact=True)
    r16 = RU.geglu64(u16, d, FP)
    g16 = _dev(r16['y'].clamp(-RU.F16_MAX, RU.F16_MAX).float(), torch.float16)
    o16, ob = K.geglu_dropout_fwd_f16(g16.clone(), keep, 1.0)
    _same(chk, 'geglu_dropout_fwd_f16.f16', o16, g16)
    _same(chk, 'geglu_dropout_fwd_f16.bf16', ob, g16.float().to(torch.bfloat16))
    chk.done()


def test_geglu_gemm_epilogues_on_every_finite_bf16_gate(K):
    """the gate in the FF1 / GEGLU-backward GEMM epilogues: A = u, W = the identity, so the product is exact and the epilogue sees exactly
    these gates (tuning key 0 = 7: the 256 x 256 tile family for every size, as test_gemm_nt_long_k_kernel_equals_the_ring)"""
    from nuwa_pytorch_amd import _lib
    L = _lib.lib()
    FP = RU.GEGLU_FP
    u, d = RU.geglu_inputs()
    uil = K.geglu_interleave(u, FP, dim=1).contiguous()
    r = RU.geglu64(u, d, FP)
    R = u.shape[0]
    chk = RowChecks('[all bf16 gates, GEMM epilogue]')
    eye2, eye1 = torch.eye(2 * FP), torch.eye(FP)
    try:
        L.amdnuwa_set_tuning(0, 7)
        # FF1, bf16: u = A I^T (exact) and a * gelu(gate) from the epilogue
        A, W = to_bf_pair(_dev(uil), False), to_bf_pair(_dev(eye2), False)
        gg = K.empty_bf((R, FP), DEV, lo=False)
        uo = K.gemm_nt(A, W, out_bf16=True, geglu_out=gg)
        _same(chk, 'gemm_geglu.bf16: u == A', uo.hi, A.hi)
        _gg(chk, 'gemm_geglu.bf16', gg.hi.float(), r, 'y', BF_EPS)
        _zero_below_minus_9(chk, 'gemm_geglu.bf16', gg.hi.float(), r)
        _same(chk, 'gemm_geglu.bf16 == geglu_il_fwd', gg.hi, K.geglu_fwd(A, FP, interleaved=True).hi)
        # FF1 on the hi + lo ring ('bf16x3-fwd'): the gate runs on the fp32 accumulators, hi + lo gate output
        K.set_precision('bf16x3-fwd')
        A3, W3 = to_bf_pair(_dev(uil), True), to_bf_pair(_dev(eye2), True)
        gg3 = K.empty_bf((R, FP), DEV, lo=True)
        uo3 = K.gemm_nt(A3, W3, out_bf16=True, geglu_out=gg3)
        _same(chk, 'gemm_geglu.x3: u.hi == A', uo3.hi, A3.hi)
        _gg(chk, 'gemm_geglu.x3', bf_value(gg3), r, 'y', PAIR_EPS)
        _zero_below_minus_9(chk, 'gemm_geglu.x3', bf_value(gg3), r)
        K.set_precision('bf16')
        # GEGLU backward: dgg = dy I^T (exact), du from the epilogue
        Dy, W1 = to_bf_pair(_dev(d), False), to_bf_pair(_dev(eye1), False)
        du = K.gemm_nt_geglu_bwd(Dy, W1, A, FP)
        _gg_du(chk, 'gemm_geglu_bwd.bf16', K.geglu_deinterleave(du.hi.float(), FP, dim=1), r, FP, BF_EPS)
        _same(chk, 'gemm_geglu_bwd.bf16 == geglu_il_bwd', du.hi, K.geglu_bwd(A, Dy, FP, interleaved=True).hi)
        # fp16 operands: the gates fp16 holds exactly
        assert K.gemm_nt_f16ops_ok(R, 2 * FP, 2 * FP, out_bf16=True, gate=True), 'the fp16-operand gate must take [510, 256] x [256, 256]'
        u16, _ = RU.geglu_inputs(fp16_exact=True)
        # (values of the [a] plane are randn: fp16 holds their bf16 roundings exactly unless they are below 2^-14)
        a16 = u16[:, :FP]
        u16 = torch.cat((torch.where(a16.abs() < 2.0 ** -14, torch.zeros_like(a16), a16), u16[:, FP:]), 1)
        r16 = RU.geglu64(u16, d, FP)
        assert torch.equal(u16.half().float(), u16)
        A16 = _dev(K.geglu_interleave(u16, FP, dim=1), torch.float16)
        uo16, gg16, ggb = K.gemm_nt_f16ops(A16, _dev(eye2, torch.float16), out_bf16=True, gate=True)
        _same(chk, 'gemm_geglu.f16ops: u == A', uo16.float(), A16.float())
        _gg(chk, 'gemm_geglu.f16ops.f16', gg16.float(), r16, 'y', F16_EPS, out_max=RU.F16_MAX)
        _gg(chk, 'gemm_geglu.f16ops.bf16', ggb.float(), r16, 'y', BF_EPS)
    finally:
        K.set_precision('bf16')
        L.amdnuwa_set_tuning(0, 0)
    chk.done()


# ---------------------------------------------------------------------------------------------------
# C. cross entropy
# ---------------------------------------------------------------------------------------------------

def _ce(K, x, t, grad_scale, lo=True, want_grad=True, row_loss=None):
    """amdnuwa_ce_fwd through the C entry (kernels.ce_fwd keeps the row losses to itself) -> row_loss, loss, dl"""
    from nuwa_pytorch_amd import _lib
    R, C = x.shape
    row_loss = torch.empty(R, dtype=torch.float32, device=DEV) if row_loss is None else row_loss
    loss = torch.empty((), dtype=torch.float32, device=DEV)
    dl = K.empty_bf((R, C), DEV, lo=lo) if want_grad else K.BF(None, None)
    p = lambda v: None if v is None else v.data_ptr()
    K.check(_lib.lib().amdnuwa_ce_fwd(p(x), p(t), p(row_loss), p(loss), p(dl.hi), p(dl.lo), R, C, C, float(grad_scale),
                                      torch.cuda.current_stream().cuda_stream), 'amdnuwa_ce_fwd')
    return row_loss, loss, dl


def _ce_case(K, chk, name, x, t, row_buf=None):
    R, C = x.shape
    r = RU.ce64(x, t)
    xd, td = _dev(x), _dev(t)
    row, loss, dl = _ce(K, xd, td, 1.0 / R, row_loss=row_buf)
    tol = RU.ce_row_tol(x)
    err = float((row.double().cpu() - r['row']).abs().max())
    _ratio(chk, f'{name}.row_loss', err / tol, bool(torch.isfinite(row).all()))
    # the mean: test_cross_entropy's ce_loss 1e-6 (relative) + the rows' absolute tolerance
    lerr = abs(float(loss) - float(r['loss']))
    _ratio(chk, f'{name}.loss', lerr / (1e-6 * abs(float(r['loss'])) + tol), bool(torch.isfinite(loss)))
    chk(f'{name}.dlogits', bf_value(dl), r['dl'], 3e-5)                     # test_cross_entropy's ce_dlogits 3e-5: p does not see a shift
    return row, loss, dl, r


@pytest.mark.parametrize('R,C', RU.CE_SHAPES)
@pytest.mark.parametrize('recipe', RU.CE_RECIPES)
def test_cross_entropy_on_shifted_and_peaked_rows(K, recipe, R, C):
    """C = 4, 2048 | 2052 (the <2> / <8> register kernels), 8192 | 8196 and 12292 (the register / three-pass border and beyond)"""
    x, t = RU.ce_logits(recipe, R, C)
    chk = RowChecks(f'[{recipe},{R},{C}]')
    RU.check_ce_conditions(recipe, x, t, RU.ce64(x, t))
    _ce_case(K, chk, 'ce', x, t)
    bad = t.clone()
    bad[R // 2] = C                                                         # an id outside the vocabulary still poisons the loss
    row, loss, _ = _ce(K, _dev(x), _dev(bad), 1.0 / R, want_grad=False)
    if not (bool(torch.isnan(loss)) and bool(torch.isnan(row[R // 2])) and int(torch.isnan(row).sum()) == 1):
        chk.failed.append(f'rows.ce{chk.tag}: an out-of-range id must give a NaN loss (and only its row)')
    chk.done()


@pytest.mark.parametrize('recipe', RU.CE_RECIPES)
def test_cross_entropy_register_and_three_pass_kernels_agree(K, recipe):
    """the same 8192 logits through ce_fwd_reg_kernel<8> (C = 8192) and ce_fwd_kernel (C = 8196, four -3e38 columns appended: their
    exponentials are exactly 0): the kernels share their arithmetic and its order, so row losses and dlogits agree bit for bit"""
    R, C = 9, 8192
    x, t = RU.ce_logits(recipe, R, C)
    xp = torch.cat((x, torch.full((R, 4), -3e38)), 1).contiguous()
    chk = RowChecks(f'[{recipe},reg vs three-pass]')
    row_a, loss_a, dl_a = _ce(K, _dev(x), _dev(t), 1.0 / R)
    row_b, loss_b, dl_b = _ce(K, _dev(xp), _dev(t), 1.0 / R)
    _same(chk, 'row_loss', row_a, row_b)
    _same(chk, 'loss', loss_a, loss_b)
    _same(chk, 'dlogits.hi', dl_a.hi, dl_b.hi[:, :C])
    _same(chk, 'dlogits.lo', dl_a.lo, dl_b.lo[:, :C])
    _same(chk, 'dlogits of the appended columns', dl_b.hi[:, C:].float(), torch.zeros(R, 4, device=DEV))
    chk.done()


def test_cross_entropy_mean_over_many_rows_and_an_unaligned_row_buffer(K):
    """mean_kernel: 16389 rows run its four-way unrolled float4 loop, its single-float4 loop and its scalar tail; a row-loss buffer one
    float past a 16-byte boundary takes the scalar path for every row"""
    chk = RowChecks('[mean]')
    x, t = RU.ce_logits('shift', 16389, 8)
    _ce_case(K, chk, 'ce[16389,8]', x, t)
    x, t = RU.ce_logits('shift', 301, 64)
    buf = torch.empty(304 + 1, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    row = buf[1:302]
    assert row.data_ptr() % 16 == 4
    _, loss_u, _, _ = _ce_case(K, chk, 'ce[301,64,unaligned]', x, t, row_buf=row)
    row_al, loss_al, _ = _ce(K, _dev(x), _dev(t), 1.0 / 301)
    _same(chk, 'unaligned rows == aligned rows', row, row_al)
    # (the two paths add the same numbers in different orders: equal to the mean's tolerance, not bit for bit)
    _ratio(chk, 'ce.loss(unaligned vs aligned)', abs(float(loss_u) - float(loss_al)) / (1e-6 * abs(float(loss_al))))
    chk.done()


# ---------------------------------------------------------------------------------------------------
# D. fused linear + cross entropy
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('C', RU.LCE_C)
@pytest.mark.parametrize('recipe', RU.LCE_RECIPES + ('rounded',))
def test_fused_linear_cross_entropy_on_ramped_and_shifted_logits(K, recipe, C):
    """linear_ce on the bf16 ring, on the hi + lo ring ('bf16x3-fwd') and with the fp16 dlogits pass: the per-64-column (max, sum exp)
    pairs merge across blocks whose maximum climbs 24 nats (or sits in the first / the last block), at logits of up to 130.
    Flat tolerances: test_fused_linear_cross_entropy(_hi_lo): loss 2e-6, dlogits 2^-8, loss_vs_unfused 2e-6, dlogits_vs_unfused 2^-7"""
    R = RU.LCE_R
    h, w, t = RU.lce_operands(recipe, C)
    chk = RowChecks(f'[{recipe},{C}]')
    td = _dev(t)
    prev = K.get_precision()

    def run(mode, hb, wb, r, w16=None, rounded16=False):
        RU.check_lce_conditions(recipe, C, r, t)
        out = K.linear_ce(hb, wb, td, 1.0 / R, w16=w16)
        assert out is not None, 'the fused kernels must take this call'
        loss, dl = out
        ulp2 = 2 * RU.ulp32(r['logits'].abs().max())
        chk(f'linear_ce.{mode}.loss', loss.reshape(1), r['loss'].reshape(1), 2e-6, extra=ulp2 / abs(float(r['loss'])))
        chk(f'linear_ce.{mode}.dlogits', dl.hi.float(), r['dl'], 2 ** -8, extra=RU.lce_delta(r, rounded16) / (R * _mx(r['dl'])))
        again = K.linear_ce(hb, wb, td, 1.0 / R, w16=w16)
        _same(chk, f'linear_ce.{mode}: loss repeatable', again[0], loss)
        _same(chk, f'linear_ce.{mode}: dlogits repeatable', again[1].hi, dl.hi)
        return loss, dl

    try:
        # bf16 ring: the operand values this mode sees are the bf16 roundings (the recipes are bf16-exact; 'rounded' is rounded here)
        hb, wb = to_bf_pair(_dev(h), False), to_bf_pair(_dev(w), False)
        rb = RU.lce64(hb.hi.float().cpu(), wb.hi.float().cpu(), t)
        loss, dl = run('bf16', hb, wb, rb)
        lg = K.gemm_nt(hb, wb)
        loss_u, dl_u = K.ce_fwd(lg, td, 1.0 / R)
        chk('linear_ce.bf16.loss_vs_unfused', loss.reshape(1), loss_u.reshape(1).double().cpu(), 2e-6, extra=2 * RU.ulp32(rb['logits'].abs().max()) / abs(float(rb['loss'])))
        chk('linear_ce.bf16.dlogits_vs_unfused', dl.hi.float(), dl_u.hi.float().double().cpu(), 2 ** -7)
        # hi + lo ring
        K.set_precision('bf16x3-fwd')
        h3, w3 = to_bf_pair(_dev(h), True), to_bf_pair(_dev(w), True)
        r3 = RU.lce64(bf_value(h3).cpu(), bf_value(w3).cpu(), t)
        loss3, dl3 = run('x3', h3, w3, r3)
        lg3 = K.gemm_nt(h3, w3)
        loss_u3, dl_u3 = K.ce_fwd(lg3, td, 1.0 / R, lo=False)
        chk('linear_ce.x3.loss_vs_unfused', loss3.reshape(1), loss_u3.reshape(1).double().cpu(), 2e-6, extra=2 * RU.ulp32(r3['logits'].abs().max()) / abs(float(r3['loss'])))
        chk('linear_ce.x3.dlogits_vs_unfused', dl3.hi.float(), dl_u3.hi.float().double().cpu(), 2 ** -7)
        # the dlogits pass on ONE fp16 MFMA per product, against the lse of the hi + lo pass: same loss bit for bit
        w16 = _dev(w).half().contiguous()
        loss16, dl16 = run('x3_f16', h3, w3, r3, w16=w16, rounded16=recipe == 'rounded')
        _same(chk, 'linear_ce.x3_f16: loss16 == loss', loss16, loss3)
    finally:
        K.set_precision(prev)
    chk.done()


# ---------------------------------------------------------------------------------------------------
# E. VAE norms, colsum
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('recipe', RU.VAE_RECIPES)
def test_vae_norms_on_offset_and_constant_images(K, recipe):
    """groupnorm (test_groupnorm's smallest shapes, 1e-5) and chan_layernorm in its register form (C = 64, 64 positions) and its generic
    form (C = 32 on a 5 x 5 map; the VQGanAttention block test's 2e-5)"""
    import torch.nn.functional as F
    from nuwa_pytorch_amd import _lib
    L = _lib.lib()
    chk = RowChecks(f'[{recipe}]')
    for (N, C, H, G, leaky) in ((2, 64, 8, 16, True), (3, 32, 5, 16, False)):
        x = RU.image_rows(recipe, (N, C, H, H))
        w, b = RU.ln_params(C)
        f = RU.groupnorm64(x, w, b, G)
        ref = F.leaky_relu(f['y'], 0.1) if leaky else f['y']
        y = K.groupnorm_fwd(_dev(x), _dev(w), _dev(b), G, 1e-5, leaky=leaky)
        chk(f'groupnorm[{C}/{G}]', y, ref, 1e-5, extra=RU.norm_term(f, w, _mx(ref)))
        if recipe == 'const':
            bref = b.reshape(1, C, 1, 1).expand(N, C, H, H)
            _same(chk, f'groupnorm[{C}/{G}] const == b', y.cpu(), F.leaky_relu(bref, 0.1) if leaky else bref)
    for (N, C, H, kind) in ((2, 64, 8, 'register'), (3, 32, 5, 'generic')):
        x = RU.image_rows(recipe, (N, C, H, H))
        resid = torch.randn(N, C, H, H, generator=torch.Generator().manual_seed(9))
        w, b = RU.ln_params(C)
        f = RU.chan_ln64(x, w, b, resid)
        xd, rd, wd, bd = _dev(x), _dev(resid), _dev(w), _dev(b)
        y = torch.empty_like(xd)
        K.check(L.amdnuwa_chan_layernorm(xd.data_ptr(), wd.data_ptr(), bd.data_ptr(), rd.data_ptr(), y.data_ptr(), N, C, H * H,
                                         1e-5, torch.cuda.current_stream().cuda_stream), 'amdnuwa_chan_layernorm')
        # (the generic kernel adds the C channels one after another: row_inputs_util.norm_term's running-sum form)
        chk(f'chan_layernorm[{kind}]', y, f['y'], 2e-5, extra=RU.norm_term(f, w, _mx(f['y']), seq=C if kind == 'generic' else None))
        if recipe == 'const':
            _same(chk, f'chan_layernorm[{kind}] const == resid + b', y.cpu(), resid + b.reshape(1, C, 1, 1))
    chk.done()


@pytest.mark.parametrize('R', RU.COLSUM_R)
def test_colsum_on_offset_columns(K, R):
    """amdnuwa_colsum, both accumulate settings through the C entry, bit-repeatable; it feeds the bias gradients, d rel_pos_bias and the
    talking-heads / null-key gradients of three attention families"""
    from nuwa_pytorch_amd import _lib
    L = _lib.lib()
    chk = RowChecks(f'[{R}]')
    st = torch.cuda.current_stream().cuda_stream
    for D in RU.COLSUM_D:
        x = RU.ln_rows('offset', R, D)
        ref = x.double().sum(0)
        xd = _dev(x)
        out = K.colsum(xd)
        chk(f'colsum[{D}]', out, ref, RU.colsum_tol(x, ref))                # R 2^-24 max|x| / max|ref| + the flat 1e-6
        _same(chk, f'colsum[{D}] repeatable', K.colsum(xd), out)
        nb = L.amdnuwa_colsum_workspace_bytes(R, D)
        ws = K.workspace(nb, DEV)
        base = torch.randn(D, generator=torch.Generator().manual_seed(3)) * 1000.0
        acc = _dev(base)
        K.check(L.amdnuwa_colsum(xd.data_ptr(), acc.data_ptr(), R, D, 1, ws.data_ptr(), nb, st), 'amdnuwa_colsum')
        # out + sum in one fp32 addition of the overwrite form's result
        _same(chk, f'colsum[{D}] accumulate == base + overwrite', acc, _dev(base) + out)
        ov = torch.full((D,), float('nan'), device=DEV)
        K.check(L.amdnuwa_colsum(xd.data_ptr(), ov.data_ptr(), R, D, 0, ws.data_ptr(), nb, st), 'amdnuwa_colsum')
        _same(chk, f'colsum[{D}] overwrite ignores the old contents', ov, out)
    chk.done()
