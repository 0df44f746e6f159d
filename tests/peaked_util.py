"""Attention inputs whose softmax rows are peaked or shifted (a trained model's, not torch.randn's), the float64 references on them and
the conditions that keep a test on them from being vacuous.  Shared by test_peaked_inputs_cpu.py (no GPU) and test_gpu_peaked_softmax.py.

Every recipe is built in fp32 on the CPU and q, k and the null key are rounded to bf16 as the LAST step (entries below the smallest
normal fp16 value are flushed to zero); afterwards only powers of two multiply them.  Such values are exact in bf16, in fp16 and as
hi + lo pairs, so every q . k product is exact in every precision mode and the score error of a kernel is fp32 accumulation alone.
v, dO and the null value keep their fp32 values: the caller rounds them to the operand type of the mode it tests (not at all in the
hi + lo mode, so the lo planes stay nonzero).

u is a per-head unit vector with random-sign entries dim_head^-0.5; noise is torch.randn.
  sharp        k <- 4 k: the scores have standard deviation 4
  ramp_up      q_i = noise + sqrt(dim_head) u, k_j = noise + a_j u, a = linspace(0, 24, T) over the key / token index: scores a_j + O(1)
               nats, the row maximum moves at every 64-key tile / 128-slot split (and sits in the causally invisible future)
  ramp_down    the same with a reversed: the maximum sits in the first tile, later tiles contribute tails only
  shift        ramp_up with 96 u added to every key and to the null key: scores of 96 .. 134 nats (exp overflows fp32 unless the
               maximum is subtracted)
  shift_null0  shift with the null key left alone: its probability underflows to 0
  masked_peak  ramp_up where the keys the key mask hides get a_j + 48 (one sample with every key hidden)
  null_peak    ramp_up with null_k = noise + 48 u: the null slot holds the row maximum by about 24 nats
  flat         plain noise (the base of the large relative-position-bias variant of Sparse3DNA)
"""
import math

import torch
import torch.nn.functional as F

RECIPES = ('sharp', 'ramp_up', 'ramp_down', 'shift', 'shift_null0', 'masked_peak', 'null_peak')

# the shapes of test_gpu_peaked_softmax.py (the smallest that cross the tile, chunk and split borders of each kernel family)
X_SHAPES = [(n, T) for n in (70, 130) for T in (33, 130, 256, 287)]                  # cross-attention: (queries, keys), B = 2, 8 x 64
# cattn (heads, dim_head, queries, keys, causal): causal n = 33, 257, 600 and rectangular (257, 33), (70, 513), (64, 1000).  The production
# geometry 8 x 64 runs the short, the one-tile-plus-one and the longest lengths; 2 x 32 and 5 x 32 one causal and one rectangular length each
CATTN_CASES = [(5, 32, 33, 33, True), (2, 32, 257, 257, True), (8, 64, 33, 33, True), (8, 64, 257, 257, True), (8, 64, 600, 600, True),
               (5, 32, 257, 33, False), (2, 32, 70, 513, False), (8, 64, 257, 33, False), (8, 64, 64, 1000, False)]
# (masked_peak needs a key mask: without one no key is hidden, and on the causal kernels ramp_up already puts the maximum into
# every query's invisible future)
CATTN_PARAMS = [(r, *c, m) for r in RECIPES for c in CATTN_CASES for m in (False, True) if m or r != 'masked_peak']
# Sparse3DNA (video shape, kernel, dilation, heads, dim_head, n): the narrow VALU kernel, two MFMA cases, two wide-grid cases
S3_SHAPES = [((3, 4, 4), (3, 3, 3), (1, 1, 1), 2, 32, None), ((2, 16, 16), (5, 3, 3), (1, 1, 1), 8, 64, None),
             ((3, 16, 16), (3, 3, 3), (4, 4, 4), 8, 64, 300), ((1, 17, 17), (3, 3, 3), (1, 1, 1), 8, 32, None),
             ((2, 20, 20), (3, 3, 3), (2, 2, 2), 8, 64, None)]
# SparseCross2DNA (feature map, kernel, dilation, sketch frames, heads, dim_head, n with <bos>): narrow VALU, MFMA with dilation and a
# partial last frame, wide grid (the geometries of test_sparse_cross_2dna_hip_vs_oracle / test_wide_sparse_cross_2dna_hip_vs_oracle)
XC2_SHAPES = [(4, 3, 1, 2, 2, 32, 1 + 3 * 16), (16, 3, 2, 2, 8, 64, 1 + 300), (20, 3, 1, 2, 8, 32, 451)]
S3_RECIPES = ('sharp', 'ramp_up', 'ramp_down', 'shift', 'shift_null0', 'null_peak', 'big_bias')
XDEC_T = [33, 256]
ROWS_T = [126, 127, 128, 300, 1000]
TILE = 64
LOG2E = math.log2(math.e)


def bf_exact(t):
    """round to bf16; flush what fp16 would hold as a subnormal (|x| < 2^-14), so the value is exact in bf16 AND fp16"""
    t = t.to(torch.bfloat16).float()
    return torch.where(t.abs() < 2.0 ** -14, torch.zeros_like(t), t)


def unit(heads, dh, gen):
    return (torch.randint(0, 2, (heads, dh), generator=gen).float() * 2 - 1) * dh ** -0.5


def qk(recipe, B, n, T, heads, dh, seed, mask=None, bos=False):
    """-> q (B, n, h, d), k (B, T, h, d), null_k (h, d) fp32, exact in bf16 / fp16.  mask (B, T) bool: True = visible (masked_peak).
    bos=True (Sparse3DNA: the <bos> row 0 of k plays the null key): null_k is None and what the recipe does to the null key is
    done to k[:, 0]"""
    gen = torch.Generator().manual_seed(seed)
    q = torch.randn(B, n, heads, dh, generator=gen)
    k = torch.randn(B, T, heads, dh, generator=gen)
    nk = torch.randn(heads, dh, generator=gen)
    u = unit(heads, dh, gen)
    gain = 1.0
    if recipe == 'sharp':
        gain = 4.0
    elif recipe != 'flat':
        assert recipe in RECIPES, recipe
        a = torch.linspace(0, 24, T)
        if recipe == 'ramp_down':
            a = a.flip(0)
        a = a[None].expand(B, T).clone()
        if recipe == 'masked_peak':
            a = a + 48.0 * (~mask).float()
        null_a = 0.0
        if recipe in ('shift', 'shift_null0'):
            a = a + 96.0
            null_a = 96.0 if recipe == 'shift' else 0.0
        if recipe == 'null_peak':
            null_a = 48.0
        q = q + math.sqrt(dh) * u
        if bos:
            a[:, 0] = null_a
        k = k + a[:, :, None, None] * u
        nk = nk + null_a * u
    q, k, nk = bf_exact(q), bf_exact(k) * gain, bf_exact(nk)
    return q, k, (None if bos else nk)


# ---- float64 scores and the conditions ----------------------------------------------------------------------------------------------

def attention_scores(q, k, nk, mask, scale, causal=False):
    """float64 scores in nats (B, h, n, 1 + T), slot 0 = the null key, -inf where the key mask or causality hides the key"""
    B, n = q.shape[:2]
    T = k.shape[1]
    s = torch.einsum('bihd,bjhd->bhij', q, k) * scale
    s0 = torch.einsum('bihd,hd->bhi', q, nk) * scale
    if mask is not None:
        s = s.masked_fill(~mask[:, None, None, :], float('-inf'))
    if causal:
        s = s.masked_fill(torch.ones(n, T, dtype=torch.bool).triu_(T - n + 1), float('-inf'))
    return torch.cat((s0[..., None], s), -1)


def sparse3dna_scores(q, k, idx, scale, rel=None):
    """float64 scores of the window (B, h, n - 1, J), slot 0 = <bos>, -inf on taps in the padding; rel: (h, J - 1) or None"""
    B, n, h, d = q.shape
    tab = idx[:n - 1]
    valid = tab >= 0
    kg = k[:, (tab.clamp(min=0) + 1).reshape(-1)].reshape(B, n - 1, -1, h, d)
    kk = torch.cat((k[:, :1, None].expand(B, n - 1, 1, h, d), kg), 2)
    s = torch.einsum('bihd,bijhd->bhij', q[:, 1:] * scale, kk)
    if rel is not None:
        s = s + F.pad(rel, (1, 0))[None, :, None, :]
    return s.masked_fill(~F.pad(valid, (1, 0), value=True)[None, None], float('-inf'))


def attention_core64(q, k, v, nk, nv, wth, mask, scale, causal=False, th_bias=None, keep=None):
    """oracle.attention_core (np.py:339-378) restated in float64 throughout -- the oracle casts its softmax to fp32 whatever it is
    given; test_peaked_inputs_cpu.py pins this restatement to it.  th_bias (h,): the talking-heads bias of the single-query kernel,
    added to every slot after the head mix (test_gpu_xm_long._formula)"""
    assert q.dtype == torch.float64
    B, n, h, d = q.shape
    s = attention_scores(q, k, nk, mask, scale, causal)
    if keep is not None:
        s.retain_grad()
        keep['s'] = s
    attn = torch.einsum('gh,bhij->bgij', wth, s.softmax(-1))
    if th_bias is not None:
        attn = attn + th_bias[None, :, None, None]
    vv = torch.cat((nv[None, None].expand(B, 1, h, d), v), 1)
    return torch.einsum('bgij,bjgd->bigd', attn, vv)


def sparse3dna_core64(q, k, v, wth, idx, scale, rel=None, keep=None):
    """oracle.sparse3dna_core (np.py:488-608) restated in float64 throughout; row 0 (<bos>) returns v[:, 0]"""
    assert q.dtype == torch.float64
    B, n, h, d = q.shape
    tab = idx[:n - 1]
    s = sparse3dna_scores(q, k, idx, scale, rel)
    if keep is not None:
        s.retain_grad()
        keep['s'] = s
    attn = torch.einsum('gh,bhij->bgij', wth, s.softmax(-1))
    vg = v[:, (tab.clamp(min=0) + 1).reshape(-1)].reshape(B, n - 1, -1, h, d) * (tab >= 0)[None, :, :, None, None].to(v.dtype)
    vv = torch.cat((v[:, :1, None].expand(B, n - 1, 1, h, d), vg), 2)
    return torch.cat((v[:, :1], torch.einsum('bgij,bijgd->bigd', attn, vv)), 1)


def cross2dna_window(fmap, kernel, dil, frames, n):
    """-> idx (n - 1, frames * kernel^2) context row of every window slot of the queries 1 .. n - 1, valid (same shape; False = padding).
    Query i sits at feature-map position (i - 1) % fmap^2 and sees the kernel x kernel taps around it in EVERY sketch frame"""
    from oracle import nuwa_oracle as O
    tpf = fmap * fmap
    tab = O.neighbor_table((1, fmap, fmap), (1, kernel, kernel), (1, dil, dil), causal=False)[(torch.arange(n - 1)) % tpf]      # (n - 1, kn)
    idx = (torch.arange(frames) * tpf)[None, :, None] + tab.clamp(min=0)[:, None, :]
    return idx.reshape(n - 1, -1), (tab >= 0)[:, None, :].expand(-1, frames, -1).reshape(n - 1, -1)


def cross2dna_scores(q, k, nk, mask, idx, valid, scale):
    """float64 scores (B, h, n - 1, 1 + J) of the windowed queries, slot 0 = the null key, -inf on padding taps and hidden keys"""
    B, n, h, d = q.shape
    kg = k[:, idx.reshape(-1)].reshape(B, n - 1, -1, h, d)
    s = torch.einsum('bihd,bijhd->bhij', q[:, 1:] * scale, kg)
    s0 = torch.einsum('bihd,hd->bhi', q[:, 1:] * scale, nk)
    vis = valid[None].expand(B, -1, -1) if mask is None else valid[None] & mask[:, idx.reshape(-1)].reshape(B, n - 1, -1)
    return torch.cat((s0[..., None], s.masked_fill(~vis[:, None], float('-inf'))), -1)


def cross2dna_core64(q, k, v, nk, nv, wth, mask, idx, valid, scale, keep=None):
    """the windowed queries of oracle.sparse_cross_2dna (np.py:832-901) in float64 throughout: rows 1 .. n - 1 -> (B, n - 1, h, d).  The
    <bos> query (row 0: full attention, no talking heads) is glue arithmetic of the module, not the kernels'"""
    assert q.dtype == torch.float64
    B, n, h, d = q.shape
    s = cross2dna_scores(q, k, nk, mask, idx, valid, scale)
    if keep is not None:
        s.retain_grad()
        keep['s'] = s
    attn = torch.einsum('gh,bhij->bgij', wth, s.softmax(-1))
    vg = v[:, idx.reshape(-1)].reshape(B, n - 1, -1, h, d)
    vv = torch.cat((nv[None, None, None].expand(B, n - 1, 1, h, d), vg), 2)
    return torch.einsum('bgij,bijgd->bigd', attn, vv)


def _rows_with_a_choice(s, min_slots=2):
    return torch.isfinite(s).sum(-1) >= min_slots


def row_max_stats(s, min_slots=2):
    """(mean row maximum of softmax(s), fraction of rows whose maximum exceeds 0.999) over the rows that see at least min_slots slots (a
    row that sees one -- a fully masked sample, the first causal row -- has probability 1 by definition)"""
    rows = _rows_with_a_choice(s, min_slots)
    pmax = s.softmax(-1).amax(-1)[rows]
    return float(pmax.mean()), float((pmax > 0.999).double().mean())


def tile_rise_fraction(s, tile=TILE, min_keys=16):
    """over the keys in tiles of `tile` (the null slot left out): the fraction of tile transitions at which the running row maximum
    rises, counted where the entered tile holds at least min_keys visible keys and some earlier key was visible.  None: no transition"""
    s = s[..., 1:]
    T = s.shape[-1]
    nt = -(-T // tile)
    s = F.pad(s, (0, nt * tile - T), value=float('-inf')).reshape(*s.shape[:-1], nt, tile)
    tmax, cnt = s.amax(-1), torch.isfinite(s).sum(-1)
    run = tmax.cummax(-1).values
    ok = (cnt[..., 1:] >= min_keys) & torch.isfinite(run[..., :-1])
    if int(ok.sum()) == 0:
        return None
    return float(((tmax[..., 1:] > run[..., :-1]) & ok).sum() / ok.sum())


def max_log2_score(s):
    return float(s[torch.isfinite(s)].abs().max()) * LOG2E


def shift_dq_term(ref, eps):
    """the derived addition to a 16-bit tolerance of dq on the shift recipes.  dq_i = scale * sum_j dS_ij k_j, and the rows of dS sum to
    zero, so the 96 u every key carries cancels out of dq -- exactly only while dS is exact.  The backward kernels round the
    probabilities and dS to the 16-bit operand type (two roundings of relative size eps = 2^-9 bf16 / 2^-11 fp16) before the product
    with k, whose entries are 12 .. 15 here instead of O(1): the error of dq is at most 2 eps scale max_(i,d) sum_j |dS_ij| |k_jd|,
    ref['dq_amp'] holds that sum over max |dq|.  On flat inputs the same term is part of what the flat tolerance covers"""
    return 2.0 * eps * ref['dq_amp']


def floors(c, rnd, dO=None, key=None):
    """denominators below which a gradient's own maximum says nothing about its error (error = max |got - ref| / max(max |ref|, floor)).
      * the null key is one more row of the key image and its gradient one more row of dK summed over the samples (likewise null_v and
        dV): on the ramps the null slot's probability is e^-24 and max |d null_k| is 1e-7 of max |dk|, so the null gradients are
        measured against the larger of their own maximum and that of dk / dv;
      * on null_peak every probability but the null slot's is e^-24: dq, dk, dv and d null_k vanish (1e-5 of their size on ramp_up, which
        is the same case with the null key where it was) while the roundings of P and dO . V keep their absolute size, so they are
        measured against the ramp_up reference's maxima.
    On every other recipe the floors of dq / dk / dv are 0: error relative to the tensor's own maximum, as gpu_util.report."""
    ref = c.reference(rnd, dO=dO, key=key)
    mx = lambda r, k: float(r[k].abs().max()) if r is not None and r.get(k) is not None else 0.0
    comp = c.companion().reference(rnd, dO=dO, key=key) if c.recipe == 'null_peak' else None
    f = dict(dq=mx(comp, 'dq'), dk=mx(comp, 'dk'), dv=mx(comp, 'dv'))
    assert c.recipe == 'null_peak' or f['dq'] == f['dk'] == f['dv'] == 0.0      # off null_peak dq, dk, dv are relative to their own maxima
    f['dkv'] = max(f['dk'], f['dv'])
    f['dnk'] = max(mx(ref, 'dk'), f['dk'])
    f['dnv'] = max(mx(ref, 'dv'), f['dv'])
    return f


def x3_shift_term(s):
    """the derived addition to a hi + lo ('x3') tolerance on the shift recipes: 2^-21 * max |score in the log2 domain| -- four fp32 ulps
    of the score, the resolution that limits P where scores are of order 100"""
    return 2.0 ** -21 * max_log2_score(s)


def check_conditions(recipe, s, dq_ref, tiles=True, min_slots=2):
    """the conditions on the float64 reference under which a comparison on `recipe` means something (figures returned for the log)"""
    # (shift_null0 drives the null slot's probability to 0 by design: a row is then as peaked as its OTHER slots make it)
    mean_max, frac_one = row_max_stats(s[..., 1:] if recipe == 'shift_null0' else s, min_slots)
    out = dict(mean_row_max=mean_max, frac_rows_above_0999=frac_one, max_dq=float(dq_ref.abs().max()))
    if recipe == 'sharp':
        assert mean_max >= 0.4, (recipe, mean_max)
    if recipe == 'big_bias':
        # (one bias row serves every query of a head: a head whose two largest taps lie 7 nats apart saturates all its rows, so the
        # share of saturated rows is a property of the eight bias rows drawn, not of the recipe -- sharpness and gradients are asked)
        assert mean_max >= 0.4 and out['max_dq'] >= 0.5, (recipe, out)
    elif recipe != 'null_peak':
        assert frac_one <= 0.05, (recipe, frac_one)
        assert out['max_dq'] >= 0.5, (recipe, out['max_dq'])
    if tiles and recipe in ('ramp_up', 'ramp_down'):
        T = s.shape[-1] - 1
        rise = tile_rise_fraction(s)
        out['tile_rise'] = rise
        if recipe == 'ramp_up' and T >= 128 and (T % TILE == 0 or T % TILE >= 16):
            assert rise is not None and rise >= 0.9, (recipe, T, rise)
        if recipe == 'ramp_down' and rise is not None:
            assert rise <= 0.01, (recipe, T, rise)
    if recipe in ('shift', 'shift_null0'):
        out['max_score'] = float(s[torch.isfinite(s)].max())
        assert out['max_score'] >= 90.0, (recipe, out['max_score'])
    if recipe == 'null_peak':
        rows = _rows_with_a_choice(s)
        lead = (s[..., 0] - s[..., 1:].amax(-1))[rows]
        out['null_lead'] = float(lead.median())
        assert out['null_lead'] >= 12.0, (recipe, out['null_lead'])
    return out


# ---- cases: inputs + float64 reference ---------------------------------------------------------------------------------------------

def _wth(heads, gen):
    return torch.randn(heads, heads, generator=gen) * 0.5 + torch.eye(heads)


def key_mask(recipe, B, T, seed, all_hidden_sample=True):
    """(B, T) bool, about 30 % of the keys hidden; sample 0 sees every key -- or, on masked_peak, none (the null key alone)"""
    gen = torch.Generator().manual_seed(1000 + seed)
    m = torch.rand(B, T, generator=gen) > 0.3
    m[0] = not (recipe == 'masked_peak' and all_hidden_sample)
    return m


class AttentionCase:
    """null key + T keys (cross-attention, cattn, the single-query kernels): inputs of one recipe and the float64 oracle on them"""

    def __init__(self, recipe, B, n, T, heads, dh, seed, masked=True, causal=False):
        self.recipe, self.B, self.n, self.T, self.heads, self.dh, self.causal = recipe, B, n, T, heads, dh, causal
        self._args = (B, n, T, heads, dh, seed, masked, causal)
        self.scale = dh ** -0.5
        self.mask = key_mask(recipe, B, T, seed) if masked else None
        assert self.mask is not None or recipe != 'masked_peak'
        self.q, self.k, self.nk = qk(recipe, B, n, T, heads, dh, seed, self.mask)
        gen = torch.Generator().manual_seed(2000 + seed)
        self.v = torch.randn(B, T, heads, dh, generator=gen)
        self.nv = torch.randn(heads, dh, generator=gen)
        self.dO = torch.randn(B, n, heads, dh, generator=gen)
        self.wth = _wth(heads, gen)
        self.scores = attention_scores(self.q.double(), self.k.double(), self.nk.double(), self.mask, self.scale, causal)
        self._refs = {}

    def reference(self, rnd, dO=None, key=None, th_bias=None):
        """float64 autograd through attention_core64 with v, null_v and dO rounded by `rnd` (dO given: used as it is) -> dict"""
        key = key or rnd
        if key not in self._refs:
            d = lambda t: t.double().requires_grad_(True)
            q, k, v, nk, nv, w = d(self.q), d(self.k), d(rnd(self.v)), d(self.nk), d(rnd(self.nv)), d(self.wth)
            keep = {}
            o = attention_core64(q, k, v, nk, nv, w, self.mask, self.scale, causal=self.causal, th_bias=th_bias, keep=keep)
            o.backward((rnd(self.dO) if dO is None else dO).double())
            kk = torch.cat((nk.detach()[None, None].expand(self.B, 1, -1, -1), k.detach()), 1)
            amp = self.scale * float(torch.einsum('bhij,bjhd->bihd', keep['s'].grad.abs(), kk.abs()).max())
            self._refs[key] = dict(o=o.detach(), dq=q.grad, dk=k.grad, dv=v.grad, dnk=nk.grad, dnv=nv.grad, dwth=w.grad,
                                   dq_amp=amp / float(q.grad.abs().max()))
        return self._refs[key]

    def companion(self):
        """the ramp_up case of the same shape and seed: null_peak is that case with the null key moved (same v, dO, head mix)"""
        if not hasattr(self, '_comp'):
            self._comp = AttentionCase('ramp_up', *self._args)
        return self._comp

    def check(self, tiles=True):
        return check_conditions(self.recipe, self.scores, self.reference(bf_round)['dq'], tiles)


class S3Case:
    """Sparse3DNA window attention (<bos> in slot 0): qkv of one recipe, the float64 oracle on them"""

    def __init__(self, recipe, shape, kern, dil, heads, dh, n, seed, B=2):
        big_bias, recipe = recipe == 'big_bias', ('flat' if recipe == 'big_bias' else recipe)
        self.recipe, self.shape, self.kern, self.dil, self.heads, self.dh, self.B = recipe, shape, kern, dil, heads, dh, B
        self._args = (shape, kern, dil, heads, dh, n, seed, B)
        self.n = n = shape[0] * shape[1] * shape[2] if n is None else n
        self.scale = dh ** -0.5
        self.q, self.k, _ = qk(recipe, B, n, n, heads, dh, seed, bos=True)
        gen = torch.Generator().manual_seed(2000 + seed)
        self.v = torch.randn(B, n, heads, dh, generator=gen)
        self.dO = torch.randn(B, n, heads, dh, generator=gen)
        self.wth = _wth(heads, gen)
        J = kern[0] * kern[1] * kern[2] + 1
        self.rel = 8.0 * torch.randn(heads, J - 1, generator=gen) if big_bias else None          # oracle layout (h, K)
        self._refs = {}

    def table(self):
        if not hasattr(self, 'idx'):
            from oracle import nuwa_oracle as O
            self.idx = O.neighbor_table(self.shape, self.kern, self.dil, causal=True)
            self.scores = sparse3dna_scores(self.q.double(), self.k.double(), self.idx, self.scale, None if self.rel is None else self.rel.double())
        return self.idx

    def reference(self, rnd, dO=None, key=None):
        key = key or rnd
        if key not in self._refs:
            d = lambda t: t.double().requires_grad_(True)
            q, k, v, w = d(self.q), d(self.k), d(rnd(self.v)), d(self.wth)
            rel = d(self.rel) if self.rel is not None else None
            keep = {}
            o = sparse3dna_core64(q, k, v, w, self.table(), self.scale, rel=rel, keep=keep)
            o.backward((rnd(self.dO) if dO is None else dO).double())
            tab, kd = self.idx[:self.n - 1], k.detach().abs()
            kg = kd[:, (tab.clamp(min=0) + 1).reshape(-1)].reshape(self.B, self.n - 1, -1, self.heads, self.dh)
            kk = torch.cat((kd[:, :1, None].expand(self.B, self.n - 1, 1, self.heads, self.dh), kg), 2)
            amp = self.scale * float(torch.einsum('bhij,bijhd->bihd', keep['s'].grad.abs(), kk).max())
            self._refs[key] = dict(o=o.detach(), dq=q.grad, dk=k.grad, dv=v.grad, dwth=w.grad, drel=None if rel is None else rel.grad,
                                   dq_amp=amp / float(q.grad.abs().max()))
        return self._refs[key]

    def companion(self):
        if not hasattr(self, '_comp'):
            self._comp = S3Case('ramp_up', *self._args)
        return self._comp

    def check(self):
        """(the row statistics count the rows whose window holds at least 5 visible slots: at the low corner of the video, and in most
        of a dilation-4 window over 300 tokens, a query sees <bos> and one to three taps, and two slots a few nats apart are one-hot
        whatever the recipe -- 44 % of the two-slot rows of the ramp, none of the rows with 5 slots or more)"""
        self.table()
        return check_conditions('big_bias' if self.rel is not None else self.recipe, self.scores, self.reference(bf_round)['dq'], tiles=False,
                                min_slots=5)


class Cross2DNACase:
    """SparseCross2DNA's windowed queries: a null key, a key mask and a window at once.  The ramp runs over the context row, so within a
    window it climbs from sketch frame to sketch frame; the keys the mask hides (and the null key) carry the peak as in AttentionCase"""

    def __init__(self, recipe, fmap, kern, dil, frames, heads, dh, n, seed, B=2):
        self.recipe, self.fmap, self.kern, self.dil, self.frames, self.heads, self.dh, self.n, self.B = recipe, fmap, kern, dil, frames, heads, dh, n, B
        self._args = (fmap, kern, dil, frames, heads, dh, n, seed, B)
        self.T = T = frames * fmap * fmap
        self.scale = dh ** -0.5
        self.mask = key_mask(recipe, B, T, seed)
        self.q, self.k, self.nk = qk(recipe, B, n, T, heads, dh, seed, self.mask)
        gen = torch.Generator().manual_seed(2000 + seed)
        self.v = torch.randn(B, T, heads, dh, generator=gen)
        self.nv = torch.randn(heads, dh, generator=gen)
        self.dO = torch.randn(B, n, heads, dh, generator=gen)
        self.wth = _wth(heads, gen)
        self.idx, self.valid = cross2dna_window(fmap, kern, dil, frames, n)
        self.scores = cross2dna_scores(self.q.double(), self.k.double(), self.nk.double(), self.mask, self.idx, self.valid, self.scale)
        self._refs = {}

    def reference(self, rnd, dO=None, key=None):
        """float64 autograd through cross2dna_core64; o and dq hold the rows 1 .. n - 1, dk / dv / d null the windowed queries' share"""
        key = key or rnd
        if key not in self._refs:
            d = lambda t: t.double().requires_grad_(True)
            q, k, v, nk, nv, w = d(self.q), d(self.k), d(rnd(self.v)), d(self.nk), d(rnd(self.nv)), d(self.wth)
            o = cross2dna_core64(q, k, v, nk, nv, w, self.mask, self.idx, self.valid, self.scale)
            o.backward((rnd(self.dO) if dO is None else dO).double()[:, 1:])
            self._refs[key] = dict(o=o.detach(), dq=q.grad[:, 1:], dk=k.grad, dv=v.grad, dnk=nk.grad, dnv=nv.grad, dwth=w.grad)
        return self._refs[key]

    def companion(self):
        if not hasattr(self, '_comp'):
            self._comp = Cross2DNACase('ramp_up', *self._args)
        return self._comp

    def check(self):
        """(row statistics over the rows that see at least 5 slots, as S3Case.check: a corner window under a 30 % mask can be left with
        the null key and a tap or two)"""
        return check_conditions(self.recipe, self.scores, self.reference(bf_round)['dq'], tiles=False, min_slots=5)


def bf_round(t):
    return t.to(torch.bfloat16).float()


def f16_round(t):
    return t.half().float()


def exact(t):
    return t
