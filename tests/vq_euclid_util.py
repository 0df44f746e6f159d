"""Inputs and the float64 judge of the Euclidean VQ lookup tests (plain helper, like gpu_util.py).

make_cluster: a codebook cloud `off + spread * randn` and rows that are a code plus `noise * randn`.  Away from the origin
(off = 100, spread = 0.05) the cloud is what an EMA-trained Euclidean codebook over post-activation features looks like, and what
the expanded fp32 form ||x||^2 - 2 x.c + ||c||^2 cannot resolve (test_vq_euclid_cpu.py pins that).

judge64: squared distances in float64 as the direct sum over (x - c)^2 -- no expansion, nothing shared with the code under test.
The per-row bound
    tol = 4 (Dc + 4) 2^-24 (||x - mu||^2 + max_c ||c - mu||^2),      mu = the float64 column mean of the codebook,
is the worst case of an fp32 fma chain of length Dc over centred operands (|x'.c'| and 1/2 ||c'||^2 are both at most half the
bracket; the + 4 covers the roundings of the centring, of half and of the final subtraction), doubled for d^2 = ||x - mu||^2 - 2 s.
It is derived, not measured.  A row is SURE when its top-2 gap of squared distances exceeds 2 tol: then no arithmetic inside the bound
can swap the two, so the index is checked for equality there; best_dist must be within tol of the float64 distance on every row."""
import functools

import torch

UNSHIFTED = [(1, 5, 2), (100, 64, 16), (64, 130, 32), (7, 33, 256), (131, 1000, 256), (300, 8192, 256)]
# (R, Cn, Dc, off, spread, noise, seed)
SHIFTED = [(300, 1000, 256, 100., .05, .05, 11), (300, 1000, 256, 100., .05, .02, 12), (64, 130, 32, 100., .05, .02, 13),
           (300, 8192, 256, 100., .05, .02, 15)]
CASES = [(R, Cn, Dc, 0., 1., .5, 20 + i) for i, (R, Cn, Dc) in enumerate(UNSHIFTED)] + SHIFTED
GUARDED = [c for c in CASES if c[:3] in ((7, 33, 256), (131, 1000, 256)) or (c[:3] == (64, 130, 32) and c[3] == 0.)]


def case_id(c):
    return 'x'.join(str(v) for v in c[:3]) + ('-shifted' + str(c[6]) if c[3] else '')


def make_cluster(R, Cn, Dc, off, spread, noise, seed):
    g = torch.Generator().manual_seed(seed)
    cb = torch.randn(Cn, Dc, generator=g) * spread + off
    pick = torch.randint(0, Cn, (R,), generator=g)
    x = cb[pick] + noise * torch.randn(R, Dc, generator=g)
    return x, cb


def judge64(x, cb):
    """-> idx64 [R], gap [R] (second smallest minus smallest squared distance), tol [R], d2 [R] (the smallest), all float64 on the CPU"""
    x, cb = x.detach().cpu().double(), cb.detach().cpu().double()
    R, Dc = x.shape
    step = max(1, (1 << 24) // (cb.shape[0] * Dc))
    idx, gap, d2 = [], [], []
    for i in range(0, R, step):
        d = (x[i:i + step, None, :] - cb[None]).square().sum(-1)
        two = d.topk(min(2, d.shape[1]), dim=-1, largest=False)
        idx.append(two.indices[:, 0])
        d2.append(two.values[:, 0])
        gap.append(two.values[:, -1] - two.values[:, 0])
    mu = cb.mean(0)
    tol = 4 * (Dc + 4) * 2.0 ** -24 * ((x - mu).square().sum(-1) + (cb - mu).square().sum(-1).max())
    return torch.cat(idx), torch.cat(gap), tol, torch.cat(d2)


@functools.lru_cache(maxsize=None)
def judged(case):
    """(x, cb, idx64, sure, tol, d2) of one case tuple, computed once per process; treat the tensors as read-only"""
    x, cb = make_cluster(*case)
    idx, gap, tol, d2 = judge64(x, cb)
    return x, cb, idx, gap > 2 * tol, tol, d2


def check_lookup(idx, dist, ref, tag):
    """the assertions of test 1: ids equal on sure rows, sure share >= 0.99, best_dist within tol on every row; prints the figures first"""
    _, _, idx64, sure, tol, d2 = ref
    idx, dist = idx.cpu(), dist.cpu().double()
    share = float(sure.double().mean())
    wrong = int((idx[sure] != idx64[sure]).sum())
    err = float(((dist - d2).abs() / tol).max())
    print(f'{tag}: sure share {share:.4f}, wrong on sure rows {wrong}, worst |best_dist - d64| / tol {err:.3e}')
    assert bool(torch.isfinite(dist).all()), f'{tag}: non-finite best_dist'
    assert share >= 0.99, f'{tag}: sure share {share}'
    assert wrong == 0, f'{tag}: {wrong} sure rows with another index than float64'
    assert err <= 1.0, f'{tag}: best_dist off by {err:.3e} tol'


def uncentred_f32(x, cb):
    """the pick of the fp32 expanded form around the origin (what torch.cdist computes)"""
    d = x.square().sum(-1, keepdim=True) - 2 * (x @ cb.t()) + cb.square().sum(-1)[None]
    return d.argmin(-1)


def centred_f32(x, cb):
    """an fp32 restatement of the device algorithm: the same score around the fp32 column mean"""
    mu = cb.mean(0)
    xs, cs = x - mu, cb - mu
    s = xs @ cs.t() - 0.5 * cs.square().sum(-1)[None]
    v, i = s.max(-1)
    return i, xs.square().sum(-1) - 2 * v
