"""Ill-conditioned rows for the row-reducing kernels (LayerNorm family, GEGLU, cross entropy, fused linear + cross entropy, the VAE norms,
colsum): the recipes, the float64 references on them, the conditions that keep a test on them from being vacuous, the derived tolerance
terms, and a plain fp32 two-pass model of each kernel's arithmetic.  No GPU.  Shared by test_row_inputs_cpu.py and test_gpu_row_kernels.py.

Every input is built in fp32 on the CPU; the float64 reference runs on those same fp32 values, so a comparison measures the kernel's
arithmetic alone.  Every derived term is computed from the float64 reference of the case, never from a kernel's output.

LayerNorm rows (LN_RECIPES; D channels, noise = torch.randn):
  offset        1024 + noise                       row mean 1000 times the spread: the mean's fp32 resolution (2^-14) shows in x - mean
  offset_small  -64 + 2^-6 noise                   the same ratio 4096 at a small scale, negative mean
  near_const    3 + 2^-12 noise                    variance 6e-8, well below eps = 1e-5: rstd ~ 315 = eps^-1/2
  const         3.0 everywhere                     x - mean == 0 exactly: y == b, rstd == eps^-1/2, dx finite
  outlier       noise, one channel = 4096 per row  a "massive activation": channel 0 (lane 0's first slot) on even rows, channel D - 1
                                                   (the last valid slot of a ragged D) on odd rows
  tiny / huge   2^-40 noise / 2^40 noise
  negative      -(1 + |noise|)                     StableLayerNorm only: every entry negative, so the row maximum (amax, no abs) is negative
Gradients (DY_KINDS): randn; inv_w (dy = 1 / w: w dy is constant, the float64 dx is ~ 0 through the first projection); xhat_over_w
(dy = xhat / w: dx ~ 0 through the second projection).

The mean-resolution rule.  A row's mean is carried in fp32: it is off by up to four half-ulps, 2^-22 |mean|, so xhat = (x - mean) rstd is
off by dxh = 2^-22 |mean| rstd in every channel of the row (a common shift).  That shift reaches
  y = xhat w + b        as dxh max|w|                                  (ln_term 'y')
  dx                    as rstd dxh max|w|                             (ln_term 'dx': the same term with rstd once more; |dy| is of unit size)
  dw = sum_r dy xhat    as max_c sum_r |dy_rc| dxh_r                   (ln_term 'dw')
  dsum = sum_r dx       as sum_r rstd_r dxh_r max|w|                   (ln_term 'dsum')
each divided by the maximum of the float64 reference (or by the floor that replaces it where the reference vanishes).  db = sum_r dy does
not see the mean.  rstd itself sees the mean only in second order (a two-pass variance about a shifted mean grows by shift^2)."""
import math

import torch

EPS = 1e-5
LN_R = 37
LN_D = (48, 256, 260, 516, 772, 1024)
LN_RECIPES = ('offset', 'offset_small', 'near_const', 'const', 'outlier', 'tiny', 'huge')
STABLE_RECIPES = ('outlier', 'negative')
DY_KINDS = ('randn', 'inv_w', 'xhat_over_w')
F16_MAX = 65504.0


def ulp32(v):
    """spacing of fp32 numbers at |v| (a normal number)"""
    return 2.0 ** (math.floor(math.log2(abs(float(v)))) - 23)


# ---- A. LayerNorm ------------------------------------------------------------------------------------------------------------------

def ln_rows(recipe, R, D, seed=0):
    z = torch.randn(R, D, generator=torch.Generator().manual_seed(100 + seed))
    if recipe == 'offset':
        x = 1024.0 + z
    elif recipe == 'offset_small':
        x = -64.0 + 2.0 ** -6 * z
    elif recipe == 'near_const':
        x = 3.0 + 2.0 ** -12 * z
    elif recipe == 'const':
        x = torch.full((R, D), 3.0)
    elif recipe == 'outlier':
        x = z.clone()
        x[0::2, 0] = 4096.0
        x[1::2, D - 1] = 4096.0
    elif recipe == 'tiny':
        x = 2.0 ** -40 * z
    elif recipe == 'huge':
        x = 2.0 ** 40 * z
    elif recipe == 'negative':
        x = -(1.0 + z.abs())
    else:
        raise ValueError(recipe)
    return x.float().contiguous()


def ln_params(D, seed=0):
    """w (|w| >= 1/4, random sign: 1 / w stays of unit size) and b, fp32"""
    g = torch.Generator().manual_seed(200 + seed)
    w = torch.randn(D, generator=g)
    w = torch.where(w.abs() < 0.25, torch.where(w < 0, -0.25, 0.25), w)
    return w.float().contiguous(), torch.randn(D, generator=g).float().contiguous()


def ln64(x, w, b, eps=EPS, stable=False):
    """float64 LayerNorm (StableLayerNorm: x / amax first, amax detached) -> dict(y, mean, rstd, xh, ia)"""
    x, w, b = x.double(), w.double(), b.double()
    ia = torch.ones(x.shape[0], dtype=torch.float64)
    if stable:
        ia = 1.0 / x.amax(-1)
        x = x * ia[:, None]
    mean = x.mean(-1)
    d = x - mean[:, None]
    rstd = ((d * d).mean(-1) + eps) ** -0.5
    xh = d * rstd[:, None]
    return dict(y=xh * w + b, mean=mean, rstd=rstd, xh=xh, ia=ia, mean_abs=x.abs().mean(-1))


def ln_bwd64(dy, f, w):
    """float64 backward of ln64 (f = its result): dx, dw, db, dsum"""
    dy, w = dy.double(), w.double()
    g = dy * w
    m1, m2 = g.mean(-1, keepdim=True), (g * f['xh']).mean(-1, keepdim=True)
    dx = (f['rstd'] * f['ia'])[:, None] * (g - m1 - f['xh'] * m2)
    return dict(dx=dx, dw=(dy * f['xh']).sum(0), db=dy.sum(0), dsum=dx.sum(0))


def ln_dy(kind, f, w, seed=0):
    """the gradient of one kind as fp32 values (f: the float64 forward, for xhat)"""
    R, D = f['xh'].shape
    if kind == 'randn':
        return torch.randn(R, D, generator=torch.Generator().manual_seed(300 + seed)).float()
    if kind == 'inv_w':
        return (1.0 / w.double())[None].expand(R, D).float().contiguous()
    if kind == 'xhat_over_w':
        return (f['xh'] / w.double()).float().contiguous()
    raise ValueError(kind)


def ln_term(what, f, w, den, dy=None):
    """the mean-resolution term of `what` ('y', 'dx', 'dw', 'dsum'; 'db' and everything else: 0) over the denominator den"""
    if den == 0.0:
        return 0.0                 # (a reference that is exactly zero -- dw on the const rows, where xhat == 0 -- is met exactly or not at all)
    dxh = 2.0 ** -22 * f['mean'].abs() * f['rstd']
    wmax = float(w.abs().max())
    if what == 'y':
        t = float(dxh.max()) * wmax
    elif what == 'dx':
        t = float((dxh * f['rstd'] * f['ia'].abs()).max()) * wmax
    elif what == 'dw':
        t = float((dy.double().abs() * dxh[:, None]).sum(0).max())
    elif what == 'dsum':
        t = float((dxh * f['rstd'] * f['ia'].abs()).sum()) * wmax
    else:
        return 0.0
    return t / den


def ln_stat_errors(mean, rstd, f):
    """per-row errors of the saved statistics and their bounds -> dict(mean=(worst ratio err / bound), rstd=...).
    mean: |err| <= 2^-20 mean_k |x_k|.  A worst-case bound: the longest chain of additions a channel passes through in the row kernels is
    two inside its float4, three across a lane's float4 slots, six wave steps and the division, 12 roundings of at most 2^-24 sum_k |x_k|
    each -- 16 are allowed.  That IS a relative bound where the mean dominates the row (offset, offset_small, near_const, const) and an
    absolute resolution where the mean is a cancelling sum (noise rows, the outlier rows whose one channel sets the size of every
    partial sum it has entered).
    rstd: relative 1e-6 (eight fp32 ulps: the sum of squares, the division, the reciprocal square root) plus the second-order effect of
    the mean, (2^-22 mean)^2 rstd^2 / 2."""
    em = (mean.double() - f['mean']).abs() / (2.0 ** -20 * f['mean_abs']).clamp(min=1e-300)
    bound_r = 1e-6 + 0.5 * (2.0 ** -22 * f['mean']) ** 2 * f['rstd'] ** 2
    er = ((rstd.double() - f['rstd']).abs() / f['rstd']) / bound_r
    return dict(mean=float(em.max()), rstd=float(er.max()))


def check_ln_conditions(recipe, x, f, stable=False):
    """what makes `recipe` the recipe it claims to be, on the float64 forward (figures returned for the log)"""
    ratio = float((f['mean'].abs() * f['rstd']).max())
    var = (1.0 / f['rstd'] ** 2 - EPS)
    out = dict(mean_rstd=ratio, rstd_max=float(f['rstd'].max()), var_min=float(var.min()))
    assert bool(torch.isfinite(x).all())
    if stable:
        amax = x.double().amax(-1)
        assert float(amax.abs().min()) > 0.0, 'a StableLayerNorm row with amax == 0'
        if recipe == 'negative':
            assert float(x.max()) < 0.0
        return out
    if recipe in ('offset', 'offset_small'):
        assert ratio >= 900.0, (recipe, ratio)
    if recipe == 'near_const':
        assert float(var.max()) < EPS / 100 and 300.0 < float(f['rstd'].min()) and ratio >= 900.0, (recipe, out)
    if recipe == 'const':
        assert float(f['xh'].abs().max()) == 0.0 and abs(float(f['rstd'][0]) - EPS ** -0.5) < 1e-9
    if recipe == 'outlier':
        R, D = x.shape
        assert bool((x[0::2, 0] == 4096.0).all()) and bool((x[1::2, D - 1] == 4096.0).all())
        assert float(f['xh'].abs().max()) > 0.9 * math.sqrt(D - 1)          # one channel holds nearly all of the row's variance
    if recipe == 'tiny':
        assert float(var.max()) < 1e-20
    if recipe == 'huge':
        assert float(var.min()) > 1e20
    return out


def ln_model32(x, w, b, eps=EPS, stable=False):
    """the kernels' arithmetic as a plain fp32 two-pass model (torch fp32 on the CPU): sum / D, sum of squared differences / D, rsqrt"""
    x, ia = x.float(), None
    if stable:
        m = x.amax(-1, keepdim=True)
        ia = (1.0 / m).reshape(-1)
        x = x / m
    D = x.shape[1]
    mean = x.sum(-1, keepdim=True) / D
    d = x - mean
    rstd = torch.rsqrt((d * d).sum(-1, keepdim=True) / D + eps)
    return dict(y=d * rstd * w + b, mean=mean.reshape(-1), rstd=rstd.reshape(-1), xh=d * rstd, ia=ia)


def ln_bwd_model32(dy, m, w):
    dy = dy.float()
    D = dy.shape[1]
    g = dy * w
    m1, m2 = g.sum(-1, keepdim=True) / D, (g * m['xh']).sum(-1, keepdim=True) / D
    sc = m['rstd'] if m['ia'] is None else m['rstd'] * m['ia']
    dx = sc[:, None] * (g - m1 - m['xh'] * m2)
    return dict(dx=dx, dw=(dy * m['xh']).sum(0), db=dy.sum(0), dsum=dx.sum(0))


# ---- B. GEGLU: every finite bf16 gate ---------------------------------------------------------------------------------------------------

GEGLU_FP, GEGLU_R = 128, 510
PHI_B = 3e-7 + 2.0 ** -22          # the documented |abs error| of norm_cdf_f + one ulp each of the hardware reciprocal and exp2 at Phi <= 1
BF16_MAX = float(torch.finfo(torch.bfloat16).max)


def all_bf16_gates(seed=0, fp16_exact=False):
    """every finite bf16 value once (65280 = 510 x 128), shuffled, as fp32.  fp16_exact: only those fp16 holds exactly as a normal number
    or zero (|g| in [2^-14, 65504]), repeated cyclically to the same count"""
    bits = torch.arange(65536, dtype=torch.int32)
    bits = bits[((bits >> 7) & 0xFF) != 0xFF]                    # exponent 255: inf / nan
    v = (bits << 16).view(torch.float32)
    assert v.numel() == 65280 and bool(torch.isfinite(v).all())
    if fp16_exact:
        v = v[(v == 0) | ((v.abs() >= 2.0 ** -14) & (v.abs() <= F16_MAX))]
        assert bool((v.half().float() == v).all())
        v = v.repeat(-(-65280 // v.numel()))[:65280]
    perm = torch.randperm(65280, generator=torch.Generator().manual_seed(400 + seed))
    return v[perm].contiguous()


def geglu_inputs(FP=GEGLU_FP, seed=0, fp16_exact=False):
    """u = [a | g] fp32 (bf16-exact) [R, 2 FP] with the gate plane = all_bf16_gates, and dgg [R, FP] (randn rounded to bf16)"""
    g = all_bf16_gates(seed, fp16_exact).reshape(-1, FP)
    gen = torch.Generator().manual_seed(500 + seed)
    a = torch.randn(g.shape, generator=gen).to(torch.bfloat16).float()
    d = torch.randn(g.shape, generator=gen).to(torch.bfloat16).float()
    return torch.cat((a, g), 1).contiguous(), d.contiguous()


def phi64(g):
    g = g.double()
    return 0.5 * torch.special.erfc(-g / math.sqrt(2.0))


def geglu64(u, d, FP):
    """float64 erfc reference -> dict(y = a gelu(g), da = d gelu(g), dg = d a gelu'(g), a, g, d, phi, dphi)"""
    a, g, d = u[:, :FP].double(), u[:, FP:].double(), d.double()
    phi = phi64(g)
    # gelu'(g) = Phi(g) + g pdf(g); the exponent is clamped where pdf underflows anyway (g^2 overflows float64 beyond 1e154 only)
    dphi = phi + g * torch.exp(-0.5 * g.clamp(-1e3, 1e3) ** 2) / math.sqrt(2.0 * math.pi)
    return dict(y=a * g * phi, da=d * g * phi, dg=d * a * dphi, a=a, g=g, d=d, phi=phi, dphi=dphi)


def out_rounding(ref, eps, floor=2.0 ** -126):
    """rounding of an output type with relative half-ulp eps (bf16 2^-8, a hi + lo pair 2^-16, fp16 2^-11), plus four fp32 roundings of the
    products, plus an absolute floor: the smallest normal fp32 (a flushed subnormal) or half the type's subnormal spacing (fp16: 2^-25)"""
    return ref.abs() * (eps + 4 * 2.0 ** -24) + floor


def geglu_bounds(r, eps, out_max=BF16_MAX, floor=2.0 ** -126):
    """per-element bounds: |y err| <= |a| |g| B + rounding, |da err| <= |d| |g| B + rounding, |dg err| <= |d| |a| B + rounding; `ok` marks the
    elements whose float64 value the output type can hold.  A product beyond the type's largest finite number overflows: that is the
    type's answer, not the kernel's (infinity, the largest finite number from a saturating fp16 store -- or NaN from a hi + lo pair,
    whose lo part is the fp32 value minus an infinite hi part)"""
    B = PHI_B
    return dict(y=(r['a'] * r['g']).abs() * B + out_rounding(r['y'], eps, floor),
                da=(r['d'] * r['g']).abs() * B + out_rounding(r['da'], eps, floor),
                dg=(r['d'] * r['a']).abs() * B + out_rounding(r['dg'], eps, floor),
                ok={k: r[k].abs() * (1 + 2 * eps) < out_max for k in ('y', 'da', 'dg')})


def geglu_errors(got, ref, bound, ok, out_max=BF16_MAX):
    """-> (worst err / bound over the representable elements, True when those are all finite and the rest overflowed as the type does:
    no finite value below the type's maximum, an infinity on the reference's side)"""
    got = got.double()
    fin = bool(torch.isfinite(got[ok]).all())
    over, rover = got[~ok], ref[~ok]
    inf = torch.isinf(over)
    over_ok = bool((~torch.isfinite(over) | (over.abs() >= 0.99 * out_max)).all()) and bool((torch.sign(over[inf]) == torch.sign(rover[inf])).all())
    sel = ok & torch.isfinite(got)
    ratio = ((got - ref).abs() / bound)[sel]
    return (float(ratio.max()) if ratio.numel() else 0.0), fin and over_ok


def norm_cdf_model32(x):
    """common.h norm_cdf_f in fp32 numpy-free torch arithmetic (exact-rounded reciprocal and exp2) -> (Phi, e = exp(-x^2 / 2))"""
    x = x.float()
    f = lambda c: torch.tensor(c, dtype=torch.float32)
    w = x.abs() * f(0.8493218002880191)
    t = 1.0 / (f(0.2727374808792225) * w + 1.0)
    e = torch.exp2(-(w * w))
    ph = t * (t * (t * (t * (t * f(0.5307027145) + f(-0.7265760135)) + f(0.7107068705)) + f(-0.142248368)) + f(0.127414796))
    q = 0.5 - ph * e
    return 0.5 + torch.copysign(q, x), e


def gelu_model32(g):
    """-> gelu(g), gelu'(g) of the fp32 model"""
    c, e = norm_cdf_model32(g)
    g = g.float()
    return g * c, g * torch.tensor(0.3989422804014327, dtype=torch.float32) * e + c


# ---- C. cross entropy ------------------------------------------------------------------------------------------------------------------

CE_SHAPES = [(9, 4), (9, 2048), (9, 2052), (9, 8192), (9, 8196), (5, 12292)]
CE_RECIPES = ('shift', 'shift_neg', 'peak_target', 'peak_other', 'edge_max', 'tie')


def ce_targets(R, C, seed=0):
    t = torch.randint(0, C, (R,), generator=torch.Generator().manual_seed(600 + seed))
    t[0], t[-1] = 0, C - 1
    return t


def ce_logits(recipe, R, C, seed=0):
    """3 randn logits fp32 [R, C] with the recipe applied, and the targets (row 0 -> 0, last row -> C - 1)"""
    gen = torch.Generator().manual_seed(700 + seed)
    x = 3.0 * torch.randn(R, C, generator=gen)
    t = ce_targets(R, C, seed)
    rows = torch.arange(R)
    if recipe == 'shift':
        x = x + 96.0
    elif recipe == 'shift_neg':
        x = x - 96.0
    elif recipe == 'peak_target':
        x[rows, t] += 60.0
    elif recipe == 'peak_other':
        x[rows, (t + 1 + rows % max(C - 1, 1)) % C if C > 1 else t] += 60.0
    elif recipe == 'edge_max':
        # the row maximum (by 30 nats) in column 0, in column C - 1, in the last partial 1024-column stride segment, in turn
        last_seg = (C - 1) // 1024 * 1024
        cols = [0, C - 1, min(last_seg + 1, C - 1)]
        x[rows, torch.tensor([cols[r % 3] for r in range(R)])] = 30.0
    elif recipe == 'tie':
        # two equal maxima per row
        c1 = rows % C
        c2 = (c1 + C // 2) % C
        x[rows, c1] = 20.0
        x[rows, c2] = 20.0
    elif recipe != 'flat':
        raise ValueError(recipe)
    return x.float().contiguous(), t


def ce64(x, t, grad_scale=None):
    """float64 row losses [R], mean loss, dlogits (softmax - onehot) * grad_scale (default 1 / R)"""
    x = x.double()
    R, C = x.shape
    lse = torch.logsumexp(x, -1)
    row = lse - x[torch.arange(R), t]
    p = torch.exp(x - lse[:, None])
    p[torch.arange(R), t] -= 1.0
    return dict(row=row, loss=row.mean(), dl=p * (1.0 / R if grad_scale is None else grad_scale), lse=lse)


def ce_row_tol(x):
    """absolute tolerance of a row loss: two fp32 ulps of the largest |logit| (lse and the target logit are each one fp32 number of
    that size)"""
    return 2.0 * ulp32(x.abs().max())


def check_ce_conditions(recipe, x, t, r):
    R, C = x.shape
    rows = torch.arange(R)
    p_t = torch.exp(-r['row'])
    out = dict(max_abs_logit=float(x.abs().max()), mean_p_target=float(p_t.mean()), max_row_loss=float(r['row'].max()))
    assert int(t[0]) == 0 and int(t[-1]) == C - 1
    if recipe == 'shift':
        assert float(x.min()) > 88.8 - 30, out          # exp() of every logit near the maximum overflows fp32 unless the maximum is subtracted
        assert float(x.max()) > 96.0
    if recipe == 'shift_neg':
        assert float(x.max()) < -80.0                   # exp() of every logit underflows to zero unless the maximum is subtracted
    if recipe == 'peak_target' and C > 4:
        assert float(p_t.min()) > 1 - 1e-12             # loss ~ 0, p - onehot cancels
    if recipe == 'peak_other' and C > 4:
        assert float(r['row'].min()) > 35.0, out        # the target sits dozens of nats below the maximum
    if recipe == 'edge_max':
        am = x.argmax(-1)
        assert {int(a) for a in am} >= {0, C - 1}
        assert C <= 1024 or any(int(a) >= (C - 1) // 1024 * 1024 and int(a) < C - 1 for a in am)
    if recipe == 'tie':
        top = x.topk(2, -1).values
        assert bool((top[:, 0] == top[:, 1]).all()) or C < 2
    return out


def ce_model32(x, t, grad_scale):
    """the kernels' arithmetic in plain fp32: max, sum exp(x - max), lse = max + log(sum), p = exp(x - max) / sum"""
    x = x.float()
    R = x.shape[0]
    m = x.amax(-1, keepdim=True)
    e = torch.exp(x - m)
    s = e.sum(-1, keepdim=True)
    row = (m + torch.log(s)).reshape(-1) - x[torch.arange(R), t]
    p = e * (1.0 / s)
    p[torch.arange(R), t] -= 1.0
    return dict(row=row, loss=row.sum() / R, dl=p * torch.tensor(grad_scale, dtype=torch.float32))


# ---- D. fused linear + cross entropy -----------------------------------------------------------------------------------------------------

LCE_R, LCE_K = 300, 64
LCE_C = (192, 576)
LCE_RECIPES = ('ramp_up', 'ramp_down', 'shift', 'peak_target', 'peak_other', 'last_block')


def lce_operands(recipe, C, seed=0, R=LCE_R, Kd=LCE_K):
    """h [R, K], w [C, K] fp32 and targets.  As peaked_util.qk with its scale K^-1/2 folded into h: u a unit vector, h = randn K^-1/2 + u
    (h . u = 1 + O(K^-1/2)), w_c = randn + a_c u, rounded with bf_exact LAST: exact in bf16 and fp16, and as hi + lo pairs with zero lo
    parts, so every mode sees the same values and logit_c = a_c + O(1) + a_c O(K^-1/2).  'rounded': genuine fp32 h and w on the ramp
    (nonzero lo parts; w16 = w.half() is a rounding)"""
    from peaked_util import bf_exact, unit
    gen = torch.Generator().manual_seed(800 + seed)
    u = unit(1, Kd, gen)[0]
    h = torch.randn(R, Kd, generator=gen) * Kd ** -0.5 + u
    w = torch.randn(C, Kd, generator=gen)
    t = torch.randint(0, C, (R,), generator=gen)
    t[0], t[1], t[-1] = 0, C - 1, C - 1
    a = torch.linspace(0, 24, C)
    if recipe == 'ramp_down':
        a = a.flip(0)
    elif recipe == 'shift':
        a = a + 96.0
    elif recipe == 'last_block':
        a = torch.zeros(C)
        a[C - 64:] = 24.0
    elif recipe not in ('ramp_up', 'peak_target', 'peak_other', 'rounded'):
        raise ValueError(recipe)
    w = w + a[:, None] * u
    # a peak is one column per ROW, which a weight matrix cannot give: the peaked recipes move the rows' TARGETS onto / off the one column
    # that carries +48 (column C // 3, inside the second 64-column block)
    peak = C // 3
    if recipe in ('peak_target', 'peak_other'):
        w[peak] += 48.0 * u
        if recipe == 'peak_target':
            t[2:-1] = peak
        else:
            t[t == peak] = peak + 1
    if recipe != 'rounded':
        h, w = bf_exact(h), bf_exact(w)
    return h.float().contiguous(), w.float().contiguous(), t


def lce64(h, w, t):
    """float64 logits, cross entropy on them, and amp = max_(r, c) sum_k |h_rk w_ck| (what one rounding of a product is relative to)"""
    lg = h.double() @ w.double().t()
    r = ce64(lg, t)
    r['logits'] = lg
    r['amp'] = float((h.double().abs() @ w.double().abs().t()).max())
    return r


def lce_delta(r, rounded16=False):
    """first-order bound of the error of a probability, dp = p dlogit <= dlogit: two fp32 ulps of the largest logit (the logit itself and
    the lse it is compared with) + four fp32 roundings of the accumulated products; on genuinely rounded fp16 operands two operand
    roundings of 2^-11"""
    d = 2.0 * ulp32(r['logits'].abs().max()) + 4 * 2.0 ** -24 * r['amp']
    return d + (2 * 2.0 ** -11 * r['amp'] if rounded16 else 0.0)


def check_lce_conditions(recipe, C, r, t):
    lg = r['logits']
    nblk = C // 64
    bmax = lg.reshape(lg.shape[0], nblk, 64).amax(-1)
    run = bmax.cummax(-1).values
    rise = float((bmax[:, 1:] > run[:, :-1]).double().mean())
    out = dict(max_logit=float(lg.abs().max()), block_rise=rise, max_row_loss=float(r['row'].max()), amp=r['amp'])
    if recipe in ('ramp_up', 'shift', 'rounded'):
        assert rise >= 0.9, (recipe, out)
    if recipe == 'ramp_down':
        assert rise <= 0.02, (recipe, out)
    if recipe == 'shift':
        assert out['max_logit'] >= 90.0
    if recipe == 'last_block':
        assert bool((bmax.argmax(-1) == nblk - 1).all())
    if recipe == 'peak_target':
        assert float(torch.exp(-r['row'][2:-1]).min()) > 0.999
    if recipe == 'peak_other':
        assert float(r['row'].median()) > 15.0, out
    return out


def lce_model32(h, w, t, grad_scale):
    """fp32 logits, per-64-column (max, sum exp) pairs merged in block order, p = exp(logit - lse)"""
    lg = (h.float() @ w.float().t())
    R, C = lg.shape
    b = lg.reshape(R, C // 64, 64)
    bm = b.amax(-1)
    bs = torch.exp(b - bm[..., None]).sum(-1)
    m, s = bm[:, 0], bs[:, 0]
    for j in range(1, C // 64):
        mn = torch.maximum(m, bm[:, j])
        s = s * torch.exp(m - mn) + bs[:, j] * torch.exp(bm[:, j] - mn)
        m = mn
    lse = m + torch.log(s)
    row = lse - lg[torch.arange(R), t]
    p = torch.exp(lg - lse[:, None])
    p[torch.arange(R), t] -= 1.0
    return dict(row=row, loss=row.sum() / R, dl=p * torch.tensor(grad_scale, dtype=torch.float32))


# ---- E. VAE norms, colsum --------------------------------------------------------------------------------------------------------------

VAE_RECIPES = ('offset', 'near_const', 'const')
COLSUM_R = (1, 255, 256, 257, 1000)
COLSUM_D = (1, 16, 17, 64, 520)


def image_rows(recipe, shape, seed=0):
    """an NCHW tensor whose every entry follows the LayerNorm recipe (so every group / every position's channel vector does)"""
    n = 1
    for s in shape:
        n *= s
    return ln_rows(recipe, 1, n, seed).reshape(shape).contiguous()


def groupnorm64(x, w, b, G, eps=EPS):
    """float64 nn.GroupNorm -> y, and the per-(n, group) statistics for the term"""
    N, C = x.shape[:2]
    xg = x.double().reshape(N, G, -1)
    mean = xg.mean(-1)
    d = xg - mean[..., None]
    rstd = ((d * d).mean(-1) + eps) ** -0.5
    xh = (d * rstd[..., None]).reshape(x.shape)
    bc = (1, C) + (1,) * (x.dim() - 2)
    return dict(y=xh * w.double().reshape(bc) + b.double().reshape(bc), mean=mean.reshape(-1), rstd=rstd.reshape(-1))


def chan_ln64(x, g, b, resid, eps=EPS):
    """float64 LayerNormChan over dim 1 (+ residual): (x - mean) / sqrt(var + eps) * g + b"""
    x = x.double()
    mean = x.mean(1, keepdim=True)
    d = x - mean
    rstd = ((d * d).mean(1, keepdim=True) + eps) ** -0.5
    bc = (1, -1) + (1,) * (x.dim() - 2)
    y = d * rstd * g.double().reshape(bc) + b.double().reshape(bc)
    return dict(y=y + (0 if resid is None else resid.double()), mean=mean.reshape(-1), rstd=rstd.reshape(-1))


def norm_term(f, w, den, seq=None):
    """ln_term 'y' for any normalisation whose statistics are f['mean'], f['rstd'].  seq = C: the mean is ONE thread's running sum over C
    channels (chan_layernorm's generic kernel), not a tree: the partial sums grow to C |mean| and addition k rounds by up to
    2^-24 k |mean|, so the mean is off by up to 2^-24 |mean| (C + 1) / 2 instead of the tree's 2^-22 |mean| (C = 32: four times that; the
    fp32 model of the running sum misses the tree rule on near_const, test_row_inputs_cpu.py)"""
    res = 2.0 ** -22 if seq is None else 2.0 ** -24 * (seq + 1) / 2
    return float((res * f['mean'].abs() * f['rstd']).max()) * float(w.abs().max()) / max(den, 1e-300)


def chan_ln_seq_model32(x, w, b):
    """chan_layernorm's generic kernel in fp32: one running sum over the channels, one running sum of squared differences"""
    x = x.float()
    C = x.shape[1]
    bc = (1, C) + (1,) * (x.dim() - 2)
    s = torch.zeros_like(x[:, :1])
    for c in range(C):
        s = s + x[:, c:c + 1]
    mean = s / C
    q = torch.zeros_like(s)
    for c in range(C):
        d = x[:, c:c + 1] - mean
        q = q + d * d
    return (x - mean) / torch.sqrt(q / C + EPS) * w.reshape(bc) + b.reshape(bc)


def norm_model32(x, w, b, groups=None):
    """fp32 two-pass model of groupnorm (groups given) / chan_layernorm (None)"""
    x = x.float()
    N, C = x.shape[:2]
    bc = (1, C) + (1,) * (x.dim() - 2)
    if groups is None:
        mean = x.sum(1, keepdim=True) / C
        d = x - mean
        return d / torch.sqrt((d * d).sum(1, keepdim=True) / C + EPS) * w.reshape(bc) + b.reshape(bc)
    xg = x.reshape(N, groups, -1)
    n = xg.shape[-1]
    mean = xg.sum(-1, keepdim=True) / n
    d = xg - mean
    xh = d * torch.rsqrt((d * d).sum(-1, keepdim=True) / n + EPS)
    return xh.reshape(x.shape) * w.reshape(bc) + b.reshape(bc)


def colsum_model32(x):
    """amdnuwa_colsum's order in fp32: min(R, 256) partial sums over the rows r = b (mod 256), the partials added in four interleaved
    groups of 64, the 64 group sums in order"""
    R, D = x.shape
    nb = min(R, 256)
    part = torch.zeros(nb, D)
    for r in range(R):
        part[r % nb] = part[r % nb] + x[r]
    grp = torch.zeros(64, D)
    for b in range(nb):
        grp[b % 64] = grp[b % 64] + part[b]
    s = torch.zeros(D)
    for g in range(64):
        s = s + grp[g]
    return s


def colsum_tol(x, ref):
    """R 2^-24 max|x| / max|ref| (R fp32 additions of numbers of size max|x|) plus the flat 1e-6"""
    return x.shape[0] * 2.0 ** -24 * float(x.abs().max()) / float(ref.abs().max()) + 1e-6
