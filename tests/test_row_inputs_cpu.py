"""The ill-conditioned row recipes of tests/row_inputs_util.py without a GPU: the float64 restatements agree with torch (and the oracle) on
flat inputs, every recipe meets the condition that makes it the recipe it claims to be, and a plain fp32 two-pass model of each kernel's
arithmetic passes the tolerance rules test_gpu_row_kernels.py asserts -- so the rules admit a correct fp32 implementation on every recipe
before a GPU is involved.  The flat tolerances are the ones the existing GPU tests assert (named in test_gpu_row_kernels.py)."""
import math

import pytest
import torch
import torch.nn.functional as F

import row_inputs_util as RU


def _rel(got, ref, den=None):
    den = float(ref.abs().max()) if den is None else den
    return float((got.double() - ref).abs().max()) / max(den, 1e-300)


# ---- restatements ------------------------------------------------------------------------------------------------------------------------

def test_float64_restatements_agree_with_torch_and_the_oracle():
    from oracle import nuwa_oracle as O
    torch.manual_seed(0)
    x, dy = torch.randn(9, 48), torch.randn(9, 48)
    w, b = RU.ln_params(48)
    xd = x.double().requires_grad_(True)
    wd, bd = w.double().requires_grad_(True), b.double().requires_grad_(True)
    y = F.layer_norm(xd, (48,), wd, bd, RU.EPS)
    y.backward(dy.double())
    f = RU.ln64(x, w, b)
    g = RU.ln_bwd64(dy, f, w)
    assert _rel(f['y'], y.detach()) < 1e-13 and _rel(f['y'], O.layer_norm(x.double(), w.double(), b.double())) < 1e-13
    assert _rel(g['dx'], xd.grad) < 1e-12 and _rel(g['dw'], wd.grad) < 1e-12 and _rel(g['db'], bd.grad) < 1e-12
    xs = x.double().requires_grad_(True)
    ys = O.stable_layer_norm(xs, w.double(), b.double())
    ys.backward(dy.double())
    fs = RU.ln64(x, w, b, stable=True)
    assert _rel(fs['y'], ys.detach()) < 1e-13 and _rel(RU.ln_bwd64(dy, fs, w)['dx'], xs.grad) < 1e-12
    # GEGLU
    u, d = torch.randn(7, 24).double().requires_grad_(True), torch.randn(7, 12)
    yg = u[:, :12] * F.gelu(u[:, 12:])
    yg.backward(d.double())
    r = RU.geglu64(u.detach(), d, 12)
    assert _rel(r['y'], yg.detach()) < 1e-13 and _rel(torch.cat((r['da'], r['dg']), 1), u.grad) < 1e-13
    # cross entropy
    lg, t = RU.ce_logits('flat', 9, 64)
    lgd = lg.double().requires_grad_(True)
    loss = F.cross_entropy(lgd, t)
    loss.backward()
    c = RU.ce64(lg, t)
    assert abs(float(c['loss'] - loss.detach())) < 1e-13 and _rel(c['dl'], lgd.grad) < 1e-12
    # the VAE norms, colsum's tolerance helper
    xi = torch.randn(2, 32, 5, 5)
    w2, b2 = torch.randn(32), torch.randn(32)
    assert _rel(RU.groupnorm64(xi, w2, b2, 16)['y'], F.group_norm(xi.double(), 16, w2.double(), b2.double(), RU.EPS)) < 1e-13
    cl = RU.chan_ln64(xi, w2, b2, None)['y']
    assert _rel(cl, F.layer_norm(xi.double().permute(0, 2, 3, 1), (32,), w2.double(), b2.double(), RU.EPS).permute(0, 3, 1, 2)) < 1e-13
    assert RU.ulp32(1.0) == 2.0 ** -23 and RU.ulp32(100.0) == 2.0 ** -17 and RU.ulp32(-3.0) == 2.0 ** -22


# ---- A. LayerNorm ------------------------------------------------------------------------------------------------------------------------

# flat tolerances of test_gpu_kernels.py: ln_fwd_post 2e-6 (fp32 y), ln_bwd_dx_acc 1e-5, ln_bwd_dw / db 1e-5, ln_bwd_dsum 1e-4
FLAT = dict(y=2e-6, dx=1e-5, dw=1e-5, db=1e-5, dsum=1e-4)


@pytest.mark.parametrize('D', RU.LN_D)
@pytest.mark.parametrize('recipe', RU.LN_RECIPES + ('negative',))
def test_layernorm_recipes_and_the_fp32_model(recipe, D):
    stable = recipe == 'negative'
    for st in ((True,) if stable else ((False, True) if recipe == 'outlier' else (False,))):
        x = RU.ln_rows(recipe, RU.LN_R, D)
        w, b = RU.ln_params(D)
        f = RU.ln64(x, w, b, stable=st)
        RU.check_ln_conditions(recipe, x, f, stable=st)
        m = RU.ln_model32(x, w, b, stable=st)
        assert bool(torch.isfinite(m['y']).all())
        if recipe == 'const':
            assert torch.equal(m['y'], b[None].expand_as(m['y']))
        den = float(f['y'].abs().max())
        assert _rel(m['y'], f['y']) <= FLAT['y'] + RU.ln_term('y', f, w, den), (recipe, D, st)
        e = RU.ln_stat_errors(m['mean'], m['rstd'], f)
        assert e['mean'] <= 1.0 and e['rstd'] <= 1.0, (recipe, D, st, e)
        ref0 = RU.ln_bwd64(RU.ln_dy('randn', f, w), f, w)
        for kind in RU.DY_KINDS:
            dy = RU.ln_dy(kind, f, w)
            ref = RU.ln_bwd64(dy, f, w)
            got = RU.ln_bwd_model32(dy, m, w)
            for q in ('dx', 'dw', 'db', 'dsum'):
                own = float(ref[q].abs().max())
                # the reference of dx (and of its column sums) vanishes on the two special gradients: measured against the randn reference
                # (an ABSOLUTE comparison); dw / db keep their own maximum
                den = float(ref0[q].abs().max()) if (kind != 'randn' and q in ('dx', 'dsum')) else own
                if kind != 'randn' and q in ('dx', 'dsum') and recipe != 'const':
                    assert own <= den, (recipe, D, kind, q, own, den)
                if den == 0.0:
                    assert float(got[q].abs().max()) == 0.0
                    continue
                tol = FLAT[q] + RU.ln_term(q, f, w, den, dy)
                assert bool(torch.isfinite(got[q]).all()) and _rel(got[q], ref[q], den) <= tol, (recipe, D, st, kind, q, _rel(got[q], ref[q], den), tol)


def test_fp16_gradient_saturation_follows_the_reference():
    """with S = 2^10 (unit-size dy lands at 2^10 in fp16): near_const -- like every recipe whose rstd is eps^-1/2 -- pushes S dx past 65504,
    the well-scaled recipes stay inside"""
    S = 2.0 ** 10
    for recipe, expect in (('near_const', True), ('offset', False), ('outlier', False), ('huge', False)):
        x = RU.ln_rows(recipe, RU.LN_R, 260)
        w, b = RU.ln_params(260)
        f = RU.ln64(x, w, b)
        top = S * float(RU.ln_bwd64(RU.ln_dy('randn', f, w), f, w)['dx'].abs().max())
        assert (top > RU.F16_MAX * 1.01) == expect and (top < RU.F16_MAX * 0.99) == (not expect), (recipe, top)


# ---- B. GEGLU ----------------------------------------------------------------------------------------------------------------------------

def test_every_bf16_gate_through_the_fp32_model_of_norm_cdf_f():
    g = RU.all_bf16_gates()
    assert g.numel() == RU.GEGLU_R * RU.GEGLU_FP and torch.unique(g.view(torch.int32)).numel() == 65280
    assert bool((g.to(torch.bfloat16).float() == g).all())
    c, e = RU.norm_cdf_model32(g)
    y, dy = RU.gelu_model32(g)
    assert all(bool(torch.isfinite(t).all()) for t in (c, e, y, dy))
    gd = g.double()
    r = RU.geglu64(torch.cat((torch.ones_like(g), g))[None], torch.ones(1, g.numel()), g.numel())
    e_phi = float((c.double() - r['phi'][0]).abs().max())
    e_der = float((dy.double() - r['dphi'][0]).abs().max())
    assert e_phi <= RU.PHI_B and e_der <= RU.PHI_B, (e_phi, e_der)
    # gelu itself: |err| <= |g| B + fp32 rounding
    assert bool(((y.double() - gd * r['phi'][0]).abs() <= gd.abs() * RU.PHI_B + RU.out_rounding(gd * r['phi'][0], 0.0)).all())
    assert bool((y[g <= -9.0] == 0).all())                                  # gates at or below -9: exactly +-0
    g16 = RU.all_bf16_gates(fp16_exact=True)
    assert bool((g16.half().float() == g16).all()) and float(g16.abs().max()) <= RU.F16_MAX
    assert torch.unique(g16).numel() >= 2 * 29 * 128                        # 29 binades x 128 significands x 2 signs (and zero)


def test_geglu_bounds_admit_the_fp32_model_on_all_three_output_types():
    u, d = RU.geglu_inputs()
    r = RU.geglu64(u, d, RU.GEGLU_FP)
    a, g = u[:, :RU.GEGLU_FP], u[:, RU.GEGLU_FP:]
    y, dphi = RU.gelu_model32(g)
    outs = dict(y=a * y, da=d * y, dg=d * a * dphi)
    for eps, rnd in ((2.0 ** -8, lambda t: t.to(torch.bfloat16).float()), (2.0 ** -24, lambda t: t)):
        bd = RU.geglu_bounds(r, eps)
        for k, v in outs.items():
            worst, fin = RU.geglu_errors(rnd(v), r[k], bd[k], bd['ok'][k])
            assert fin and worst <= 1.0, (k, eps, worst)
    assert int((~RU.geglu_bounds(r, 2.0 ** -8)['ok']['y']).sum()) < 200     # only gates of the top binade times |a| > 1 leave the type's range


# ---- C. cross entropy --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('R,C', RU.CE_SHAPES)
@pytest.mark.parametrize('recipe', RU.CE_RECIPES)
def test_cross_entropy_recipes_and_the_fp32_model(recipe, R, C):
    x, t = RU.ce_logits(recipe, R, C)
    r = RU.ce64(x, t)
    RU.check_ce_conditions(recipe, x, t, r)
    m = RU.ce_model32(x, t, 1.0 / R)
    assert bool(torch.isfinite(m['row']).all()) and bool(torch.isfinite(m['dl']).all())
    assert float((m['row'].double() - r['row']).abs().max()) <= RU.ce_row_tol(x), (recipe, R, C)
    assert _rel(m['dl'], r['dl']) <= 3e-5                                   # test_cross_entropy's ce_dlogits


# ---- D. fused linear + cross entropy -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('C', RU.LCE_C)
@pytest.mark.parametrize('recipe', RU.LCE_RECIPES + ('rounded',))
def test_linear_ce_recipes_and_the_fp32_model(recipe, C):
    from peaked_util import bf_exact
    h, w, t = RU.lce_operands(recipe, C)
    if recipe != 'rounded':
        assert torch.equal(bf_exact(h), h) and torch.equal(bf_exact(w), w) and torch.equal(w.half().float(), w)
    else:
        assert not torch.equal(w.half().float(), w)
    r = RU.lce64(h, w, t)
    RU.check_lce_conditions(recipe, C, r, t)
    m = RU.lce_model32(h, w, t, 1.0 / RU.LCE_R)
    # loss: test_fused_linear_cross_entropy's 2e-6 (relative) + two fp32 ulps of the largest logit (absolute)
    assert abs(float(m['loss'].double() - r['loss'])) <= 2e-6 * abs(float(r['loss'])) + 2 * RU.ulp32(r['logits'].abs().max())
    # dlogits in fp32 (the kernels round them to bf16: 2^-8 there): a flat 1e-6 here + delta / (R max|ref|)
    tol = 1e-6 + RU.lce_delta(r) / (RU.LCE_R * float(r['dl'].abs().max()))
    assert _rel(m['dl'], r['dl']) <= tol, (recipe, C, _rel(m['dl'], r['dl']), tol)
    # the fp16 pass on rounded operands: logits from fp16-rounded h and w against the float64 logits of the fp32 operands
    if recipe == 'rounded':
        m16 = RU.lce_model32(h.half().float(), w.half().float(), t, 1.0 / RU.LCE_R)
        tol16 = 1e-6 + RU.lce_delta(r, rounded16=True) / (RU.LCE_R * float(r['dl'].abs().max()))
        assert _rel(m16['dl'], r['dl']) <= tol16, (_rel(m16['dl'], r['dl']), tol16)


# ---- E. VAE norms, colsum ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('recipe', RU.VAE_RECIPES)
def test_vae_norm_recipes_and_the_fp32_model(recipe):
    for shape, G in (((2, 64, 8, 8), 16), ((3, 32, 5, 5), 16)):
        x = RU.image_rows(recipe, shape)
        w, b = RU.ln_params(shape[1])
        f = RU.groupnorm64(x, w, b, G)
        den = float(f['y'].abs().max())
        assert _rel(RU.norm_model32(x, w, b, G), f['y']) <= 1e-5 + RU.norm_term(f, w, den), (recipe, shape)       # test_groupnorm's 1e-5
        c = RU.chan_ln64(x, w, b, None)
        assert _rel(RU.norm_model32(x, w, b), c['y']) <= 1e-5 + RU.norm_term(c, w, float(c['y'].abs().max())), (recipe, shape)
        # the generic kernel's running sum over the channels: its own (re-derived) term; on near_const at C = 32 it misses the tree rule
        seq = _rel(RU.chan_ln_seq_model32(x, w, b), c['y'])
        assert seq <= 1e-5 + RU.norm_term(c, w, float(c['y'].abs().max()), seq=shape[1]), (recipe, shape, seq)
        if recipe == 'near_const' and shape[1] == 32:
            assert seq > 2e-5 + RU.norm_term(c, w, float(c['y'].abs().max())), seq
        if recipe == 'const':
            assert torch.equal(RU.norm_model32(x, w, b), b.reshape(1, -1, 1, 1).expand(shape))


@pytest.mark.parametrize('R', RU.COLSUM_R)
def test_colsum_tolerance_admits_fp32_summation(R):
    for D in RU.COLSUM_D:
        x = RU.ln_rows('offset', R, D)
        ref = x.double().sum(0)
        assert _rel(RU.colsum_model32(x), ref) <= RU.colsum_tol(x, ref), (R, D)
