"""Clip + AdamW step (csrc/optim.hip, nuwa_pytorch_amd/optimizer.py): the float64 reference, the cases, the derived bounds, the conditions
that keep a test on them from being vacuous, and numpy fp32 models of the kernels' arithmetic.  No GPU.  Shared by test_adamw_cpu.py and
test_gpu_adamw_values.py.  The models are used on the CPU only, to show that the bounds can be met; a GPU result is never compared with one.

The reference.  adamw64 is one AdamW step in float64 AT THE fp32 VALUES THE C ENTRY RECEIVES: float32(lr), float32(beta1), float32(beta2),
float32(eps), float32(weight_decay), with both bias corrections 1 - beta^t formed from those same fp32 betas.  What is left between it and the
kernel is the kernel's own rounding.  u = 2^-24 below is the largest relative error of one fp32 rounding (round to nearest).

Per-element bounds (adamw_bounds), counting the roundings of `upd` in adamw_kernel; primes are the updated values, every quantity on the
right is the float64 reference's.  a = 1 - b1 and c = 1 - b2 are exact in fp32 for every beta of the case list (Sterbenz: beta >= 1/2, or
beta == 0; check_case asserts it).  e_g is the relative error of the effective gradient g1 = k g: 0 when the clip coefficient is exactly 1,
else the norm's bound + 3 u for the coefficient (the 1e-6f constant, the addition, the division) + u for the product.
  m' = m + a (g1 - m)         the difference, the product, the sum:   |dm'| <= u (|m'| + 2 a (|g1| + |m|)) + a |g1| e_g
                              (never below u (1 - b1) |g1|, so a cancelling m' does not shrink it to nothing)
  v' = b2 v + c g1 g1         three products and the sum:             |dv'| <= u (v' + b2 v + 2 c g1^2) + 2 c g1^2 e_g
  D = 1 - lr wd               the product and the difference (D in (1/2, 1]: half an ulp is u / 2); exact when wd == 0
  p1 = p D,  p' = p1 - U      one rounding each:                      u (|p1| + |p'|) + |p| u (1/2 + lr wd) [wd != 0]
  U = step (m' / den),  step = lr / bc1,  den = sqrt(v') / sqrt(bc2) + eps
      step: bc1 as fp32 and the division, 2 u;  U and the quotient: u each;  sqrt(v'): rv / 2 + u with rv = |dv'| / v';
      sqrt(bc2): bc2 as fp32 (u / 2 under the root) and the root, 1.5 u;  their quotient u;  the sum with eps u.  With
      w = (den - eps) / den <= 1:   |dU| <= |U| (5 u + w (3.5 u + rv / 2)) + step |dm'| / den
  |dp'| <= u (|p1| + |p'| + |p| (1/2 + lr wd) [wd != 0]) + |dU|
Every bound is first order; (1 + 2^-16) covers the products of two such terms (each at most about 10 u relative), and 2^-126 is added for
a result in the subnormal range, flushed or not.  A fused multiply-add drops a rounding and stays inside.

Bound on the norm (norm_depth).  The sum of squares adds nonnegative terms, so its relative error is at most u times the number of
roundings on the longest path from one element to the result: the square (1), the two levels inside a float4 (2), the per-thread loop
(ceil(n4 / 1024) accumulations, and one more for a ragged tail), wave_sum (6), block_sum_256 (2), the finalize stride loop
(ceil(nchunks / 1024)) and its 10-level tree.  The root halves that and adds a rounding of its own: |dnorm| / norm <= (depth / 2 + 1) u,
times (1 + depth u) for the second order.  The depth is computed from the case's shapes.

Domain: the float64 comparison covers the fp32 normal range only, 1e-12 <= |g1| <= 1e12 for every nonzero effective gradient, so that g1^2
neither underflows nor overflows (check_case asserts it per case)."""
import math

import numpy as np

U = 2.0 ** -24
TINY = 2.0 ** -126
SECOND = 1.0 + 2.0 ** -16
CHUNK = 65536

NUMELS = (1, 3, 4, 5, 255, 256, 1023, 1024, 1025, 65535, 65536, 65537, 131072, 131073)
MANY = (1023, 1024, 1025, 2049, 4100)            # tensors of MANY_N elements: nchunks on both sides of 1024 and of 4096
MANY_N = 5
RECIPES = ('randn', 'scales', 'one_per_chunk', 'const', 'zeros')
STEPS = (1, 2, 10, 1000, 100000)
SCALES = (1e-6, 1.0, 1e4)
CLIPS = (None, 'zero', 'far', 0.9, 0.01)          # max_grad_norm: None, 0, 1e9 x the norm's size, 0.9 x the norm, 0.01 x the norm
CONST = 2.0 ** -12
ONE = 2.0 ** -10


def value_shapes():
    """every NUMELS entry once as a 2-D parameter (decay group) and once as a 1-D one (no decay)"""
    return [(1, n) for n in NUMELS] + [(n,) for n in NUMELS]


def _case(name, recipe, t, lr, wd, eps, betas, clip, wd_edit=False):
    return dict(name=name, recipe=recipe, t=t, lr=lr, wd=wd, eps=eps, betas=betas, clip=clip, wd_edit=wd_edit)


# one launch over value_shapes() each; together they hold every step count, lr, wd, eps, beta pair, recipe and clip kind of the issue
CASES = [
    _case('randn_t1', 'randn', 1, 3e-4, 0.01, 1e-8, (0.9, 0.999), None),
    _case('scales_t2_clip0.9', 'scales', 2, 3e-4, 0.1, 1e-8, (0.9, 0.999), 0.9, wd_edit=True),
    _case('randn_t10_far', 'randn', 10, 1e-2, 0.1, 1e-3, (0.5, 0.9), 'far'),
    _case('scales_t1000_clip0.01', 'scales', 1000, 3e-4, 0.01, 1e-8, (0.9, 0.999), 0.01),
    _case('randn_t100000_zero', 'randn', 100000, 1e-2, 0.0, 1e-3, (0.0, 0.999), 'zero'),
    _case('scales_mixed', 'scales', 'mixed', 3e-4, 0.01, 1e-8, (0.9, 0.999), None),
    _case('one_per_chunk_t1_clip0.9', 'one_per_chunk', 1, 1e-2, 0.1, 1e-8, (0.9, 0.999), 0.9),
    _case('const_t2_clip0.01', 'const', 2, 3e-4, 0.01, 1e-3, (0.5, 0.9), 0.01),
    _case('const_t1_b0', 'const', 1, 1e-2, 0.1, 1e-8, (0.0, 0.999), None),
    _case('zeros_t1', 'zeros', 1, 3e-4, 0.01, 1e-8, (0.9, 0.999), None),
    _case('zeros_t1_far', 'zeros', 1, 1e-2, 0.1, 1e-8, (0.9, 0.999), 'far'),
]


def f32(x):
    """the double that holds float32(x)"""
    return float(np.float32(x))


def hyper32(lr, betas, eps):
    return dict(lr=f32(lr), b1=f32(betas[0]), b2=f32(betas[1]), eps=f32(eps))


def case_steps(case, nparams):
    """the step count of every parameter AFTER the step under test"""
    if case['t'] == 'mixed':
        return [STEPS[i % len(STEPS)] for i in range(nparams)]
    return [case['t']] * nparams


def _rng(seed):
    return np.random.default_rng(seed)


def _randn(rng, n):
    """standard normal fp32, |z| >= 2^-10 so that the smallest scale under the hardest clip stays inside the domain (1e-6 x 2^-10 x 0.01 > 1e-12)"""
    z = rng.standard_normal(n).astype(np.float32)
    return np.where(np.abs(z) < 2.0 ** -10, np.copysign(np.float32(2.0 ** -10), z), z).astype(np.float32)


def make_grads(recipe, numels, seed=0):
    """fp32 gradients, one flat array per tensor"""
    rng = _rng(1000 + seed)
    out = []
    for i, n in enumerate(numels):
        if recipe == 'randn':
            g = _randn(rng, n)
        elif recipe == 'scales':
            g = (_randn(rng, n) * np.float32(SCALES[i % 3])).astype(np.float32)
        elif recipe == 'one_per_chunk':
            g = np.zeros(n, dtype=np.float32)
            for k, c0 in enumerate(range(0, n, CHUNK)):
                cn = min(CHUNK, n - c0)
                g[c0 + (cn - 1 if (i + k) % 2 else (7 * i) % cn)] = ONE * (-1) ** i      # the chunk's last element, or one early in it
        elif recipe == 'const':
            g = np.full(n, CONST, dtype=np.float32)
        elif recipe == 'zeros':
            g = np.zeros(n, dtype=np.float32)
        else:
            raise ValueError(recipe)
        out.append(g)
    return out


def make_params(numels, seed=0):
    """weights of the size an initialiser gives (0.02 randn), every 7th one 2^-10 of that: an update is then larger than the rounding of
    the weight it moves, which is what lets an order-of-operations mistake show"""
    rng = _rng(2000 + seed)
    out = []
    for n in numels:
        p = (0.02 * rng.standard_normal(n)).astype(np.float32)
        p[::7] *= np.float32(2.0 ** -10)
        out.append(p)
    return out


def make_state(recipe, numels, steps, hyper, seed=0):
    """moments of the size a run of steps[i] - 1 updates on such gradients holds: m ~ 0.3 s (1 - b1^t) randn, v ~ s^2 (1 - b2^t) [0.5, 1.5)"""
    rng = _rng(3000 + seed)
    ms, vs = [], []
    for i, (n, t) in enumerate(zip(numels, steps)):
        tp = t - 1
        if tp == 0 or recipe == 'zeros':
            ms.append(np.zeros(n, dtype=np.float32)); vs.append(np.zeros(n, dtype=np.float32))
            continue
        s = {'scales': SCALES[i % 3], 'const': CONST, 'one_per_chunk': ONE}.get(recipe, 1.0)
        ms.append((0.3 * s * (1 - hyper['b1'] ** tp) * rng.standard_normal(n)).astype(np.float32))
        vs.append((s * s * (1 - hyper['b2'] ** tp) * (0.5 + rng.random(n))).astype(np.float32))
    return ms, vs


# ---- the float64 reference ---------------------------------------------------------------------------------------------------------------

def norm64(grads):
    return math.sqrt(sum(float(np.sum(np.asarray(g, dtype=np.float64) ** 2)) for g in grads))


def clip64(norm, max_norm):
    """min(1, max_norm / (norm + 1e-6)); 1 when max_norm <= 0 (include/amdnuwa.h)"""
    if max_norm is None or max_norm <= 0:
        return 1.0
    return min(1.0, max_norm / (norm + 1e-6))


def max_norm_of(kind, norm):
    """the max_grad_norm argument of a clip kind, as the fp32 value the entry receives (None stays None)"""
    if kind is None:
        return None
    if kind == 'zero':
        return 0.0
    if kind == 'far':
        return f32(1e9 * max(norm, 1.0))
    return f32(kind * norm)


def adamw64(p, g, m, v, hyper, t, clip, wd=0.0, variant=None):
    """one AdamW step in float64 at the fp32-rounded hyper-parameters -> dict(p, m, v) and the intermediates the bounds need.
    variant (for the vacuity checks only): 'decay_after' decays after the update, 'eps_inside' puts eps under the root"""
    p, g, m, v = (np.asarray(x, dtype=np.float64) for x in (p, g, m, v))
    lr, b1, b2, eps, wd = hyper['lr'], hyper['b1'], hyper['b2'], hyper['eps'], f32(wd)
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    g1 = g * clip
    D = 1.0 - lr * wd
    p1 = p if variant == 'decay_after' else p * D
    m2 = m + (1.0 - b1) * (g1 - m)
    v2 = b2 * v + (1.0 - b2) * g1 * g1
    step = lr / bc1
    if variant == 'eps_inside':
        den = np.sqrt(v2 / bc2 + eps)
    else:
        den = np.sqrt(v2) / math.sqrt(bc2) + eps
    upd = step * (m2 / den)
    p2 = p1 - upd
    if variant == 'decay_after':
        p2 = p2 * D
    return dict(p=p2, m=m2, v=v2, p0=p, p1=p1, g1=g1, m0=m, v0=v, upd=upd, den=den, step=step, D=D, wd=wd)


def adamw_bounds(r, hyper, e_g=0.0):
    """per-element bounds on p, m, v of the reference result r (module docstring)"""
    a, c, b2, lr = 1.0 - hyper['b1'], 1.0 - hyper['b2'], hyper['b2'], hyper['lr']
    ag, g2 = np.abs(r['g1']), r['g1'] * r['g1']
    dm = U * (np.abs(r['m']) + 2 * a * (ag + np.abs(r['m0']))) + a * ag * e_g
    dv = U * (r['v'] + b2 * r['v0'] + 2 * c * g2) + 2 * c * g2 * e_g
    rv = np.divide(dv, r['v'], out=np.zeros_like(dv), where=r['v'] > 0)
    w = (r['den'] - hyper['eps']) / r['den']
    du = np.abs(r['upd']) * (5 * U + w * (3.5 * U + rv / 2)) + r['step'] * dm / r['den']
    dp = U * (np.abs(r['p1']) + np.abs(r['p']) + (np.abs(r['p0']) * (0.5 + lr * r['wd']) if r['wd'] != 0 else 0.0)) + du
    return dict(p=dp * SECOND + TINY, m=dm * SECOND + TINY, v=dv * SECOND + TINY)


def chunk_ns(numels):
    out = []
    for n in numels:
        out += [min(CHUNK, n - c0) for c0 in range(0, n, CHUNK)]
    return out


def norm_depth(numels):
    """roundings on the longest path of the two-stage sum of squares (module docstring)"""
    ns = chunk_ns(numels)
    loop = max(-(-(n & ~3) // 1024) + (1 if n % 4 else 0) for n in ns)
    return 1 + 2 + loop + 6 + 2 + -(-len(ns) // 1024) + 10


def norm_bound(numels):
    """relative bound on the norm"""
    d = norm_depth(numels)
    return (d / 2 + 1) * U * (1 + d * U)


def clip_rel_bound(numels, clip):
    """e_g: the relative error of the effective gradient k g"""
    return 0.0 if clip == 1.0 else norm_bound(numels) + 4 * U


# ---- conditions --------------------------------------------------------------------------------------------------------------------------

def check_case(case, grads, clip):
    """hyper-parameters whose 1 - beta is exact in fp32, effective gradients inside the domain"""
    h = hyper32(case['lr'], case['betas'], case['eps'])
    for b in (h['b1'], h['b2']):
        assert f32(1.0 - b) == 1.0 - b, f'1 - {b} is not an fp32 number'
    for g in grads:
        nz = np.abs(np.asarray(g, dtype=np.float64)[g != 0]) * clip
        if nz.size:
            assert 1e-12 <= float(nz.min()) and float(nz.max()) <= 1e12, (case['name'], float(nz.min()), float(nz.max()))
    if case['recipe'] == 'zeros':
        assert all(not g.any() for g in grads)
    return h


def worst(got, ref, bound):
    """largest |got - ref| / bound"""
    return float(np.max(np.abs(np.asarray(got, dtype=np.float64) - ref) / bound)) if np.size(ref) else 0.0


def t_observable(hyper, t):
    """does a step count off by one change a bias correction by more than 100 u?  (at t = 100000 both corrections are 1 to 40 digits, and
    for beta1 == 0 the first is 1 at every t: there an off-by-one count computes the same step and no test can see it)"""
    rel = lambda b: abs((1 - b ** (t + 1)) - (1 - b ** t)) / (1 - b ** t) if b > 0 else 0.0
    return max(rel(hyper['b1']), rel(hyper['b2']) / 2) > 100 * U


# ---- numpy fp32 models of the kernels --------------------------------------------------------------------------------------------------------

F = np.float32


def bias_corrections32(b1, b2, t):
    """what _upload writes into the chunk table: (1 - beta^t) in double, rounded to fp32.  b1, b2: the doubles the power is taken of"""
    return F(1.0 - b1 ** t), F(1.0 - b2 ** t)


def adamw_model32(p, g, m, v, lr, b1, b2, eps, wd, bc1, bc2, k):
    """adamw_kernel's upd in numpy fp32, expression by expression (no fused multiply-add); every argument an fp32 value"""
    p, g, m, v = (np.asarray(x, dtype=F) for x in (p, g, m, v))
    lr, b1, b2, eps, wd, bc1, bc2, k = (F(x) for x in (lr, b1, b2, eps, wd, bc1, bc2, k))
    one = F(1.0)
    decay, step, sb = one - lr * wd, lr / bc1, np.sqrt(bc2)
    g = g * k
    p = p * decay
    m = m + (one - b1) * (g - m)
    v = b2 * v + (one - b2) * g * g
    p = p - step * (m / (np.sqrt(v) / sb + eps))
    return p, m, v


_LANES = np.arange(256)


def _block_sum_model(s):
    """wave_sum (a butterfly over lane ^ 1, 2, 4, 8, 16, 32: the mirrors pair lanes that already hold equal values) and block_sum_256"""
    for k in (1, 2, 4, 8, 16, 32):
        s = s + s[_LANES ^ k]
    return (s[0] + s[64]) + (s[128] + s[192])


def sumsq_chunk_model32(g):
    """grad_sumsq_kernel on one chunk: thread t takes elements 4 t + 1024 k, then the ragged tail, then the block reduction"""
    g = np.asarray(g, dtype=F)
    n = g.size
    n4 = n & ~3
    s = np.zeros(256, dtype=F)
    if n4:
        it = -(-n4 // 1024)
        x = np.zeros(it * 1024, dtype=F)
        x[:n4] = g[:n4]
        x = x.reshape(it, 256, 4)
        for k in range(it):
            q = x[k] * x[k]
            s = s + ((q[:, 0] + q[:, 1]) + (q[:, 2] + q[:, 3]))
    if n > n4:
        s[:n - n4] = s[:n - n4] + g[n4:] * g[n4:]
    return _block_sum_model(s)


def finalize_model32(partials, max_norm):
    """grad_norm_finalize_kernel: the 1024-thread stride loop, the 10-level tree, the root and the coefficient"""
    partials = np.asarray(partials, dtype=F)
    n = partials.size
    it = max(-(-n // 1024), 1)
    x = np.zeros(it * 1024, dtype=F)
    x[:n] = partials
    x = x.reshape(it, 1024)
    red = np.zeros(1024, dtype=F)
    for k in range(it):
        red = red + x[k]
    k = 512
    while k > 0:
        red[:k] = red[:k] + red[k:2 * k]
        k >>= 1
    norm = np.sqrt(red[0])
    mn = F(0.0 if max_norm is None else max_norm)
    coef = min(F(1.0), mn / (norm + F(1e-6))) if mn > 0 else F(1.0)
    return F(norm), F(coef)


def norm_model32(grads, max_norm=None):
    parts = []
    for g in grads:
        g = np.asarray(g, dtype=F).reshape(-1)
        parts += [sumsq_chunk_model32(g[c0:c0 + CHUNK]) for c0 in range(0, g.size, CHUNK)]
    return finalize_model32(parts, max_norm)


# ---- one case, assembled -------------------------------------------------------------------------------------------------------------------

def case_data(case, seed=0, shapes=None):
    """everything a test of one case needs, in the optimiser's parameter order (value_shapes(): the 2-D tensors first): shapes, numels,
    per-tensor decay and step counts, fp32 p / g / m / v (flat), the float64 norm, the max_grad_norm argument and the float64 coefficient"""
    shapes = value_shapes() if shapes is None else list(shapes)
    numels = [int(np.prod(s)) for s in shapes]
    h = hyper32(case['lr'], case['betas'], case['eps'])
    steps = case_steps(case, len(shapes))
    g = make_grads(case['recipe'], numels, seed)
    m, v = make_state(case['recipe'], numels, steps, h, seed)
    norm = norm64(g)
    max_norm = max_norm_of(case['clip'], norm)
    clip = clip64(norm, max_norm)
    check_case(case, g, clip)
    return dict(shapes=shapes, numels=numels, hyper=h, steps=steps, wds=[case['wd'] if len(s) >= 2 else 0.0 for s in shapes],
                p=make_params(numels, seed), g=g, m=m, v=v, norm=norm, max_norm=max_norm, clip=clip)
