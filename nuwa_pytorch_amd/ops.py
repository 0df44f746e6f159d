"""autograd.Function wrappers that sequence the libamdnuwa kernels for the decoder sub-blocks.

Each decoder sub-block of the reference (Transformer.forward np.py:1174-1180)

        x = SandwichNorm(fn)(x, ...) + x          fn in {Shift(Sparse3DNA), Attention(context), Shift(FeedForward)}

is ONE autograd node here (`SandwichBlockFn`): pre-LN -> GEMM(s) [token shift folded into the GEMM
loader] -> attention core / GEGLU -> GEMM -> post-LN + residual, with a hand-written backward that
calls the backward kernels.  The residual stream, LayerNorm statistics, softmax and all accumulators
are fp32; GEMM / attention operands are bf16 (plus a bf16 residual in 'bf16x3' parity mode).

The same inner stages also back the standalone modules (Sparse3DNA, Attention, FeedForward,
LayerNorm wrappers) through `InnerFn`, so `Sparse3DNA(...)(x)` alone works as in the reference.
"""
from collections import namedtuple
import functools
import os
import warnings
import weakref

import torch
from torch.autograd import Function

from . import kernels as K
from .kernels import BF


def _ru(v, m):
    return (v + m - 1) // m * m


def _in_phase(name):
    """run an autograd node's forward / backward body inside K.phase(name) (see kernels.phase: the mixed precision mode allocates
    and consumes hi-only operands in backward code)"""
    def deco(fn):
        @functools.wraps(fn)
        def wrapped(*a, **k):
            with K.phase(name):
                return fn(*a, **k)
        return wrapped
    return deco


def _storage_key(p):
    """what identifies the memory a tensor reads: (address of its first element, autograd version, identity of its storage).  Host-only."""
    return (p.data_ptr(), p._version, p.untyped_storage()._cdata)


class WeightCache:
    """bf16 (hi[/lo]) operand copies of fp32 master weights; rebuilt when a parameter changes (an in-place write bumps `_version`, a new
    storage has another identity), when weights_changed() says so, or when the precision mode changes.

    An entry HOLDS the storages it was built from: while it lives neither their addresses nor their identities can be handed out again, so a
    parameter that was given a new storage (`p.data = t`, `module.half().float()`, `.to(device)`) can never present the key of the old one
    -- not even when the allocator would have returned the old block."""

    EPOCH = 0          # bumped by weights_changed(): writes that neither autograd's version counter nor the storage identity shows

    def __init__(self):
        self._store = {}

    def get(self, key, params, builder):
        ver = tuple(_storage_key(p) for p in params) + (K.get_precision(), WeightCache.EPOCH, K._BWD_F16)
        ent = self._store.get(key)
        if ent is None or ent[0] != ver:
            with torch.no_grad():
                ent = (ver, builder(), tuple(p.untyped_storage() for p in params))
            self._store[key] = ent
        return ent[1]

    def clear(self):
        self._store.clear()


def weights_changed():
    """Tell the package that weights (or a context tensor) were written in a way torch cannot see: in place through `.data`, through a raw
    pointer, by another library.  Everything derived from tensor CONTENTS is dropped and rebuilt on the next call: every WeightCache entry
    (bf16 hi / lo casts, transposes, the interleaved FeedForward weight, fp16 copies and pairs), the fp16 range verdicts and the bf16 copy of
    the context.  Writes torch sees (optimizer.step(), load_state_dict, `with torch.no_grad(): p.mul_(..)`, a new storage) need no call."""
    WeightCache.EPOCH += 1
    _F16_RANGE.clear()
    _ctx_cast_reset()


def _cast(w):
    out = K.empty_bf(tuple(w.shape), w.device)
    K.cast_pad(w.detach(), out)
    return out


def _cast_t(w):
    out = K.empty_bf((w.shape[1], w.shape[0]), w.device)
    K.transpose_cast(w.detach(), out)
    return out


# fp16 range guard of the 'bf16x3-fwd' forward (its FeedForward / 3DNA q-k-v products run single fp16 MFMAs on fp16 copies of the
# weights).  fp16 ends at 65504 -- a larger weight would become inf -- and loses significand bits below 6.1e-5, so a weight
# tensor takes the fp16 form only while its largest magnitude lies in [F16_WMIN, F16_WMAX]; otherwise the block runs the bf16 hi + lo
# (3-MFMA) products, which have fp32's range.  One device -> host transfer per call of f16_ranges_prefetch() covers every weight
# whose memory (storage, address, version: _storage_key) has not been judged yet: Transformer.forward_layers calls it once per step for the
# whole stack.
# (Activations are covered in the kernels: every fp16 activation store saturates at +-65504, csrc/common.h pack2_f16_sat.)
F16_WMAX = 6.0e4
F16_WMIN = 2.0 ** -10
_F16_RANGE = {}


_F16_ALSO = []


def f16_prefetch_also(*ws):
    """weights to be judged together with the next f16_ranges_prefetch() call (no transfer of their own): NUWA.forward registers
    to_logits.weight here before the decoder stack runs"""
    _F16_ALSO.extend(ws)


def f16_ranges_prefetch(ws):
    todo, seen = [], set()
    ws = list(ws) + _F16_ALSO
    del _F16_ALSO[:]
    for w in ws:
        if _f16_known(w) is None and id(w) not in seen and w.is_cuda:
            seen.add(id(w))
            todo.append(w)
    if not todo:
        return
    with torch.no_grad():
        am = torch.stack(torch._foreach_norm([w.detach() for w in todo], float('inf'))).cpu().tolist()     # ONE synchronisation
    for w, a in zip(todo, am):
        _f16_record(w, bool(F16_WMIN <= a <= F16_WMAX))       # (NaN compares false)
    # the stream is drained at this point anyway (once per optimiser step): look at the fp16 saturation monitor of the step before
    nsat = K.f16_sat_count(reset=True)
    if nsat:
        warnings.warn(f'nuwa_pytorch_amd: {nsat} thread(s) clamped a value beyond +-65504 in a counted fp16 store of the last step (LayerNorm copies, the cross-attention '
                      "output copy or fp16 gradients of the 'bf16x3-fwd' mode; the q / k / v and gate copies clamp without counting): the step ran on saturated values; set_precision('bf16x3') has fp32's range",
                      RuntimeWarning, stacklevel=3)


def _f16_drop(ref, slot):
    """the judged tensor died: release its verdict (and the storage it holds)"""
    ent = _F16_RANGE.get(slot)
    if ent is not None and ent[0] is ref:
        del _F16_RANGE[slot]


def _f16_record(w, ok):
    """ONE verdict per tensor object (slot id(w), released when the object dies): the object by weak reference, the key of the memory it was
    judged on, that storage itself -- held, so that neither its address nor its identity can come back under a new storage while the
    verdict stands (see WeightCache) -- and the verdict.  Judging the object again replaces the entry and lets the old storage go."""
    slot = id(w)
    _F16_RANGE[slot] = (weakref.ref(w, lambda ref, slot=slot: _f16_drop(ref, slot)), _storage_key(w), w.untyped_storage(), ok)


def _f16_known(w):
    """the verdict recorded for THIS tensor object on the memory it reads now, or None: a verdict is tied to the object by a weak reference
    (a new tensor at a dead one's id does not inherit it) and to the storage, the address and the version it was judged on"""
    ent = _F16_RANGE.get(id(w))
    return ent[3] if ent is not None and ent[0]() is w and ent[1] == _storage_key(w) else None


def f16_weights_ok(*ws):
    f16_ranges_prefetch(ws)
    return all(_f16_known(w) is True for w in ws)


def _f16_to_pair(h):
    """an activation that arrived as a bf16 + fp16 copy pair, for a block that has to run hi + lo products after all (its weights
    left the fp16 range): hi + lo with lo = bf16(fp16 value - hi) carries the fp16 value exactly (11 significand bits)"""
    if h.lo is None and h.f16 is not None:
        return BF(h.hi, (h.f16.float() - h.hi.float()).to(torch.bfloat16))
    return h


# =================================================================================================
# inner stages.  fwd(h: BF [R, D], ...) -> (y fp32 [R, D], saved) ; bwd(saved, dy: BF) -> (dh fp32, grads)
# =================================================================================================

# What a block runs is decided ONCE per forward call, by the plan() of its kind (block_plan below), from the precision mode, the A/B switches,
# the kernels' support queries and the fp16 range verdicts of its weights -- and never cached: modes and switches may change between calls.
# SandwichBlockFn / InnerFn put the record into meta['plan']; the kind's fwd dispatches on it and its bwd on the copy saved with the node.
#   h16      form of the LayerNorm output the block reads: False = bf16 hi[/lo], True = bf16 + fp16 copy pair, 'only' = the fp16 copy alone
#   bwd16    the backward runs on fp16 gradients (kernels.G16) against the single fp16 copies the forward leaves
#   guarded  the weights the fp16 range guard judges (Inner.guarded: Transformer.forward_layers prefetches their verdicts)
#   a16      the first product runs fp16 operands: the 3DNA q / k / v projection, both FeedForward products, the two-MFMA ('f16x2') cross-
#            attention q product (False: gemm_nt on bf16 hi[/lo])
#   core16   q / k / v leave their projection with an fp16 copy and the attention core runs fp16 MFMAs
#   o16      the core's output is a bf16 + fp16 copy pair for the two-MFMA to_out ('only': the fp16 copy alone)
#   core, pack, lean, bwd   cross attention: the forward core (X_CORES), the images packed ('x6b16' / 'x6b': the xattn6 backward's own, from the
#            fp16 / bf16 copy of k / v; 'x1': xattn_pack with lean=), the backward (X_BWDS)
_PLAN = dict(h16=False, bwd16=False, guarded=(), a16=False, core16=False, o16=False, core=None, pack=None, lean=False, bwd=None)
Plan = namedtuple('Plan', list(_PLAN), defaults=list(_PLAN.values()))
X_CORES = ('x6_f16_only', 'x6_f16', 'x6_bf16', 'x2_f16', 'x2_bf16', 'x1_stats', 'x1_p')      # kernel generation _ operand form / what it keeps
X_BWDS = ('x6_16', 'x6', 'x2', 'x2_rc', 'x1')               # xattn6 on fp16 gradients, xattn6, xattn2, xattn2 recomputing the key side, xattn1


def block_plan(kind, R, D, p, meta, has_resid=False, ln=True):
    """the Plan of one block of R rows x D columns.  has_resid: a block of a reversible stack (separate residual input) keeps the bf16 backward
    -- not chained, every one of them would take its own gradient scale: one amax pass per block, -2.7 % on cfg 4.  ln=False: no LayerNorm in
    front (InnerFn: the standalone modules), the input is a plain bf16 hi[/lo] cast.  Kinds without a plan() have no choice to make."""
    plan = getattr(INNERS[kind], 'plan', None)
    return plan(R, D, p, meta, has_resid, ln) if plan is not None else Plan()


# Where the dropout keep masks come from.  'torch' (default): torch.rand(...) >= p, the draw every release so far made.  'device': the Philox
# generator kernels of csrc/keepmask.hip write the masks in the layouts the masked kernels read -- no fp32 uniforms, no pack passes, no
# transposes; the keep decision is the function of (seed, logical element) stated in include/amdnuwa.h.  Another generator samples other masks
# from a seed, so the route is opt-in (set_keep_mask_source / AMDNUWA_KEEP_MASK_SOURCE).
KEEP_MASK_SOURCES = ('torch', 'device')
_KEEP_MASK_SOURCE = os.environ.get('AMDNUWA_KEEP_MASK_SOURCE', 'torch')
if _KEEP_MASK_SOURCE not in KEEP_MASK_SOURCES:
    raise ValueError(f'AMDNUWA_KEEP_MASK_SOURCE={_KEEP_MASK_SOURCE!r}: expected one of {KEEP_MASK_SOURCES}')


def set_keep_mask_source(name):
    global _KEEP_MASK_SOURCE
    if name not in KEEP_MASK_SOURCES:
        raise ValueError(name)
    _KEEP_MASK_SOURCE = name


def get_keep_mask_source():
    return _KEEP_MASK_SOURCE


def _keep_seed(device):
    """the two seed words of one generated mask: ONE tiny draw from torch's generator of that device, left on the device (the generator kernel
    reads them; nothing synchronises).  torch.manual_seed, RngReplay's recorded states and a forked stream therefore govern the generated
    masks exactly as they govern a torch.rand draw"""
    return torch.randint(0, 1 << 32, (2,), dtype=torch.int64, device=device)


def _attn_keep_mask(B, nq, J, heads, p, device):
    """keep mask of the nn.Dropout(p) on the window attention map (np.py:558, 748), in the kernels' [B, query, slot, head] order (torch's RNG
    stream, or under set_keep_mask_source('device') the generator kernel seeded from it; tests replace this function by a fixed mask)"""
    if _KEEP_MASK_SOURCE == 'device':
        return K.keep_mask_linear(B * nq * J * heads, K.keep_threshold(p), _keep_seed(device)).view(torch.bool).view(B, nq, J, heads)
    return torch.rand((B, nq, J, heads), device=device) >= p


class S3Inner:
    """to_q/to_kv -> Sparse3DNA core -> to_out (np.py:481-613).  params: to_q.w, to_kv.w, talking_heads.w,
    to_out.w, to_out.b.  meta['drop_p'] (attention dropout in training): the masked form of whatever core the plan picks; the mask is saved
    for the backward (so RngReplay's recomputed forward and the backward read the same one)"""
    nparams = 5

    @staticmethod
    def weights(cache, p):
        wq, wkv, wth, wo, bo = p[:5]

        def build():
            inner, D = wq.shape
            qkv = K.empty_bf((3 * inner, D), wq.device)
            K.cast_pad(wq.detach(), qkv, row0=0)
            K.cast_pad(wkv.detach(), qkv, row0=inner)
            qkvT = K.empty_bf((D, 3 * inner), wq.device)
            K.transpose_cast(wq.detach(), qkvT, col0=0)
            K.transpose_cast(wkv.detach(), qkvT, col0=inner)
            out = dict(qkv=qkv, qkvT=qkvT, out=_cast(wo), outT=_cast_t(wo))
            if K.mixed() and f16_weights_ok(wq, wkv):   # fp16 copy for the fp16-operand q / k / v projection of 'bf16x3-fwd'
                out['qkv_16'] = torch.cat((wq.detach(), wkv.detach()), 0).to(torch.float16).contiguous()
            if K.mixed() and f16_weights_ok(wo):        # fp16 hi + lo pair for the two-MFMA to_out product
                out['out_16'] = K.f16_pair(wo)
            if K.bwd_f16('s') and 'qkv_16' in out and 'out_16' in out:    # transposes for the dgrad products of the fp16-gradient backward
                out['qkvT_16'] = out['qkv_16'].t().contiguous()
                out['outT_16'] = wo.detach().t().contiguous().to(torch.float16)
            return out
        return cache.get('s3', (wq, wkv, wo), build)

    @staticmethod
    def guarded(p):
        return (p[0], p[1], p[3])

    @staticmethod
    def plan(R, D, p, meta, has_resid=False, ln=True):
        """a16: 'bf16x3-fwd' runs the q / k / v projection on single fp16 MFMAs (bf16 + fp16 copies out) feeding the fp16 core.  bwd16 (class
        's'): that, the two-MFMA to_out, no relative-position bias, and the band kernels and the five backward products take the shapes"""
        wq, wkv, wo = S3Inner.guarded(p)
        g, inner = meta['geom'], wq.shape[0]
        if g.heads > K.S3_MAX_HEADS:
            # many heads (Sparse3DNA.many_heads): the VALU kernels of sparse3dna_mh.hip on bf16 hi[/lo] operands, nothing else
            return Plan(guarded=(wq, wkv, wo))
        if meta.get('drop_p') and not K.s3_f16_supported(g):
            # live attention dropout off the band geometry: the masked core is the VALU window kernels on bf16 hi[/lo] operands -- no fp16
            # core (and so no fp16 projections around it), no fp16-gradient backward.  At band geometry the band kernels have masked forms in
            # every operand form, and the block gets the plan it gets without dropout.
            return Plan(guarded=(wq, wkv, wo))
        a16 = bool(meta.get('shift') is None and K.qkv_f16() and K.s3_f16_supported(g) and K.gemm_nt_f16ops_ok(R, 3 * inner, D, out_bf16=True) and
                   f16_weights_ok(wq, wkv))
        core16 = a16 or bool(K.cores_f16() and K.want_lo() and K.s3_f16_supported(g))
        o16 = bool(core16 and K.proj_f16x2('o') and K.gemm_nt_f16x2_ok(R, wo.shape[0], inner, out_bf16=False) and f16_weights_ok(wo))
        b16 = bool(ln and a16 and o16 and not has_resid and K.bwd_f16('s') and len(p) == 5 and
                   K.s3_bwd16_supported(g) and K.gemm_nt_f16ops_ok(R, 3 * inner, D, out_bf16=False, out_f16=True) and
                   K.gemm_nt_f16ops_ok(R, inner, D, out_bf16=False, out_f16=True) and K.gemm_nt_f16ops_ok(R, D, 3 * inner, out_bf16=False, out_f16=True) and
                   K.gemm_tn16_ok(R, D, inner) and K.gemm_tn16_ok(R, 3 * inner, D))
        return Plan('only' if b16 else ln and a16, b16, (wq, wkv, wo), a16, core16, 'only' if b16 else o16)

    @staticmethod
    def fwd(h, p, meta):
        W = S3Inner.weights(meta['cache'], p)
        wth, bo = p[2], p[4]
        g = meta['geom']
        rel = p[5].detach().contiguous() if len(p) > 5 else None          # [J, heads] relative-position bias (optional)
        pl = meta['plan']
        # attn_dropout > 0 in training (np.py:558, 748): nn.Dropout on the mixed attention map, inside the core.  The mask rides behind the three
        # saved tensors of every branch.
        drop_p = float(meta.get('drop_p') or 0.0)
        dev = h.f16.device if h.hi is None else h.hi.device
        keep = _attn_keep_mask(g.B, g.ntok - 1, g.kf * g.kh * g.kw + 1, g.heads, drop_p, dev) if drop_p else None
        dkw = dict(keep=keep, drop_scale=1.0 / (1.0 - drop_p)) if drop_p else {}
        tail = (keep,) if drop_p else ()
        if pl.bwd16:
            # fp16-gradient backward: ONE (fp16) copy of h, of q / k / v and of the core's output
            qkv = K.BF(None, None, K.gemm_nt_f16ops(h.f16, W['qkv_16'], out_f16=True))
            o = K.sparse3dna_fwd(g, qkv, wth.detach().reshape(g.heads, g.heads).contiguous(), o_f16='only', **dkw)
            y = K.gemm_nt_f16x2(o.f16, W['out_16'], bias=bo.detach())
            return y, (K.BF(None, None, h.f16), qkv, o) + tail
        assert h.hi is not None, 'a bf16 backward needs the bf16 copy of the LayerNorm output'
        if pl.a16:
            h16 = h.f16 if h.f16 is not None else K.hilo_to_f16(h)
            qkv = K.gemm_nt_f16ops(h16, W['qkv_16'], out_bf16=True, copy_f16=True)
        else:       # core16: q / k / v leave the 3-MFMA projection as a bf16 copy (backward) + an fp16 copy, and the core runs single fp16 MFMAs
            h = _f16_to_pair(h)
            qkv = K.gemm_nt(h, W['qkv'], out_bf16=True, shift=meta.get('shift'), out_f16=pl.core16)
        # two-MFMA to_out (o16): the fp16 core hands its output over as a bf16 copy (backward) + an fp16 copy (this product's A operand)
        if g.heads > K.S3_MAX_HEADS:
            o = K.sparse3dna_mh_fwd(g, qkv, wth.detach().reshape(g.heads, g.heads).contiguous(), rel_bias=rel)
        else:
            o = K.sparse3dna_fwd(g, qkv, wth.detach().reshape(g.heads, g.heads).contiguous(), rel_bias=rel, o_f16=pl.o16, **dkw)
        y = K.gemm_nt_f16x2(o.f16, W['out_16'], bias=bo.detach()) if pl.o16 else K.gemm_nt(o, W['out'], bias=bo.detach(), out_bf16=_fast())
        return y, tuple(_sv(h, qkv, o)) + tail

    @staticmethod
    def bwd(saved, dy, p, meta, need_dbias=True, dy_f32=None):
        h, qkv, o = saved[:3]
        keep = saved[3] if len(saved) > 3 else None          # attention dropout: the keep mask of the forward
        W = S3Inner.weights(meta['cache'], p)
        wq, wkv, wth, wo, bo = p[:5]
        rel = p[5].detach().contiguous() if len(p) > 5 else None
        g = meta['geom']
        inner = g.heads * g.dim_head
        if meta['plan'].bwd16:
            # fp16-gradient backward: dy = fp16(S dy); every product on the fp16 MFMA against the fp16 copies the forward left
            s2 = dy.s2
            d_o = K.gemm_nt_f16ops(dy.t, W['outT_16'], out_f16=True)
            dwo = torch.empty_like(wo)
            K.gemm_tn16(dy.t, o.f16, dwo, s2)
            dqkv, dwth = K.sparse3dna_bwd16(g, qkv.f16, wth.detach().reshape(g.heads, g.heads).contiguous(), d_o, s2, keep=keep,
                                            drop_scale=1.0 / (1.0 - float(meta['drop_p'])) if keep is not None else 1.0)
            dh = K.G16(K.gemm_nt_f16ops(dqkv, W['qkvT_16'], out_f16=True), s2)
            dwqkv = torch.empty((3 * inner, wq.shape[1]), dtype=torch.float32, device=wq.device)
            K.gemm_tn16(dqkv, h.f16, dwqkv, s2)
            return dh, None, [dwqkv[:inner], dwqkv[inner:], dwth.reshape(wth.shape), dwo, None]
        d_o = K.gemm_nt(dy, W['outT'], out_bf16=True)
        dwo = torch.empty_like(wo)
        K.gemm_tn(dy, o, dwo)
        if g.heads > K.S3_MAX_HEADS:
            dqkv, dwth, drel = K.sparse3dna_mh_bwd(g, qkv, wth.detach().reshape(g.heads, g.heads).contiguous(), d_o, rel_bias=rel)
        else:
            dqkv, dwth, drel = K.sparse3dna_bwd(g, qkv, wth.detach().reshape(g.heads, g.heads).contiguous(), d_o, rel_bias=rel, keep=keep,
                                                drop_scale=1.0 / (1.0 - float(meta['drop_p'])) if keep is not None else 1.0)
        dh = K.gemm_nt(dqkv, W['qkvT'], out_bf16=_fast_bwd())
        sh = meta.get('shift')
        dwqkv = torch.empty((3 * inner, wq.shape[1]), dtype=torch.float32, device=wq.device)   # one wgrad GEMM for [to_q; to_kv]
        K.gemm_tn(dqkv, h, dwqkv, shift=sh)
        dwq, dwkv = dwqkv[:inner], dwqkv[inner:]
        dbo = K.colsum(dy_f32) if (need_dbias and dy_f32 is not None) else None
        grads = [dwq, dwkv, dwth.reshape(wth.shape), dwo, dbo]
        if rel is not None:
            grads.append(drel)
        return dh, None, grads


def _rotary_bf(t, freqs, B, n, heads_total, inverse=False):
    """apply_rotary_pos_emb (np.py:144-153) to a bf16 [B*n, heads_total*dh] activation (every dh-wide head chunk: q, k AND v
    heads alike -- quirk Q11); inverse=True applies the transpose (the backward of the rotation).  Text-encoder sized tensors."""
    x = t.hi.float() if t.lo is None else t.hi.float() + t.lo.float()
    R, Cc = x.shape
    x = x.view(B, n, heads_total, Cc // heads_total)
    rd = freqs.shape[-1]
    c, sn = freqs.cos()[None, :, None, :], freqs.sin()[None, :, None, :]
    a, rest = x[..., :rd], x[..., rd:]
    rh = torch.cat((-a[..., rd // 2:], a[..., :rd // 2]), dim=-1)
    a = a * c - rh * sn if inverse else a * c + rh * sn
    out = K.empty_bf((R, Cc), x.device, lo=t.lo is not None)
    K.cast_pad(torch.cat((a, rest), dim=-1).reshape(R, Cc).contiguous(), out)
    return out


class XInner:
    """to_q(x), to_kv(context) -> cross-attention core -> to_out (np.py:315-379, context given).
    params: null_k, null_v, talking_heads.w, to_q.w, to_kv.w, to_out.w"""
    nparams = 6

    @staticmethod
    def weights(cache, p):
        nk, nv, wth, wq, wkv, wo = p

        def build():
            out = dict(q=_cast(wq), qT=_cast_t(wq), kv=_cast(wkv), kvT=_cast_t(wkv), out=_cast(wo), outT=_cast_t(wo))
            if K.mixed() and f16_weights_ok(wq, wo):    # fp16 hi + lo pairs for the two-MFMA q and to_out products of 'bf16x3-fwd'
                out['q_16'], out['out_16'] = K.f16_pair(wq), K.f16_pair(wo)
                if K.bwd_f16('x'):                      # ... and fp16 transposes for the dgrad products of the fp16-gradient backward
                    out['qT_16'] = wq.detach().t().contiguous().to(torch.float16)
                    out['outT_16'] = wo.detach().t().contiguous().to(torch.float16)
            return out
        return cache.get('x', (wq, wkv, wo), build)

    @staticmethod
    def guarded(p):
        return (p[3], p[5])

    @staticmethod
    def plan(R, D, p, meta, has_resid=False, ln=True):
        """a16: 'bf16x3-fwd' with the two-MFMA switch on -- the q projection takes the LayerNorm output as ONE fp16 value when the fp16 core
        follows, the product fits the ring and the weights sit inside the fp16 range.  The core: the third design (xattn6: images in LDS order,
        null key as a rank-one term) wherever the second ran, on fp16 operands (core16) in 'bf16x3-fwd' or bf16 ones in 'bf16'; the first
        design for the other geometries and for hi + lo operands.  bwd16 (class 'x'): the two-MFMA q and to_out products around the fp16 xattn6
        core, fp32 null key / value, and the fp16 backward kernels take the shapes"""
        nk, (wq, wo) = p[0], XInner.guarded(p)
        g, inner, lo, rot = meta['xgeom'], wq.shape[0], K.want_lo(), meta.get('rotary')          # (lo: h, q and the context carry lo parts)
        x2s, rc = K.xattn2_supported(g), K.xattn2_bwd_rc_ok(g)
        core16 = bool(K.cores_f16() and lo and rot is None and x2s)
        a16 = bool(core16 and K.proj_f16x2('q') and not meta.get('self_kv') and K.gemm_nt_f16x2_ok(R, inner, D, out_bf16=True) and f16_weights_ok(wq, wo))
        o16 = bool(core16 and K.proj_f16x2('o') and K.gemm_nt_f16x2_ok(R, wo.shape[0], inner, out_bf16=False) and f16_weights_ok(wq, wo))
        x6 = bool(K.xattn6_on() and K.xattn6_supported(g) and (core16 or (x2s and not lo)) and nk.dtype == torch.float32)
        if ln and a16 and o16 and x6 and not has_resid and K.bwd_f16('x') and K.xattn_bwd16_ok(g) and not rc and \
                K.gemm_nt_f16ops_ok(R, inner, D, out_bf16=False, out_f16=True) and K.gemm_nt_f16ops_ok(R, D, inner, out_bf16=False, out_f16=True) and \
                K.gemm_tn16_ok(R, D, inner) and K.gemm_tn16_ok(R, inner, D):
            return Plan('only', True, (wq, wo), True, True, 'only', 'x6_f16_only', 'x6b16', False, 'x6_16')
        if core16:
            core = 'x6_f16' if x6 else 'x2_f16'
        elif x2s and not lo:                  # fast mode: statistics only, the backward recomputes the probabilities
            core = 'x6_bf16' if x6 else 'x2_bf16'
        else:                                 # 3-MFMA forward: 'bf16x3-fwd' keeps the statistics for xattn2_bwd on the hi parts, else P / P' for xattn_bwd
            core = 'x1_stats' if K.mixed() and x2s else 'x1_p'
        x6b = bool(x6 and K.xattn6_bwd_ok(g) and not rc)        # the bf16 backward on its own images (bf16 [key][d] tiles in LDS order)
        lean = False if x6b else 'bwd' if x6 and not rc else core16 and not rc
        bwd = 'x1' if core == 'x1_p' else 'x2_rc' if rc else 'x6' if x6b else 'x2'
        return Plan(ln and a16, False, (wq, wo), a16, core16, o16, core, 'x6b' if x6b else 'x1', lean, bwd)

    @staticmethod
    def fwd(h, p, meta):
        W = XInner.weights(meta['cache'], p)
        nk, nv, wth = p[0], p[1], p[2]
        g, pl = meta['xgeom'], meta['plan']
        ctx = h if meta.get('self_kv') else meta['ctx_bf']          # self-attention (text encoder): keys / values from the same rows
        rot, m8 = meta.get('rotary'), meta['mask_u8']
        nk2, nv2 = nk.detach().reshape(g.heads, g.dim_head).contiguous(), nv.detach().reshape(g.heads, g.dim_head).contiguous()
        wth2 = wth.detach().reshape(g.heads, g.heads).contiguous()
        if pl.bwd16:
            # fp16-gradient backward: ONE (fp16) copy of h, of q and of the core's output; the backward's images come from the fp16 copy of k / v
            q16 = K.gemm_nt_f16x2(h.f16, W['q_16'], out_f16=True)
            kv = K.gemm_nt(ctx, W['kv'], out_bf16=True, out_f16=True)
            pk = K.xattn6_pack_bwd(g, kv.f16, nk2, nv2, m8)
            o, stats = K.xattn6_fwd(g, q16, K.xattn6_pack(g, kv.f16, m8), nk2, nv2, wth2, o_f16='only')
            y = K.gemm_nt_f16x2(o.f16, W['out_16'])
            return y, (K.BF(None, None, h.f16), K.hi_only(ctx), K.BF(None, None, q16), pk, stats, None, o)
        assert h.hi is not None, 'a bf16 backward needs the bf16 copy of the LayerNorm output'
        if pl.a16:      # two MFMAs: fp16 LayerNorm output x the weight as an fp16 hi + lo pair; q leaves as a bf16 copy + an fp16 copy
            q = K.gemm_nt_f16x2(h.f16 if h.f16 is not None else K.hilo_to_f16(h), W['q_16'], out_bf16=True, copy_f16=True)
        else:
            h = _f16_to_pair(h)
            q = K.gemm_nt(h, W['q'], out_bf16=True, out_f16=pl.core16)
        kv = K.gemm_nt(ctx, W['kv'], out_bf16=True, out_f16=pl.core16)    # (context rows: B * T of them, a 3-MFMA product either way)
        if rot is not None:
            q = _rotary_bf(q, rot, g.B, g.n, g.heads)
            kv = _rotary_bf(kv, rot, g.B, g.T, 2 * g.heads)
        pk = K.xattn6_pack_bwd(g, kv.hi, nk2, nv2, m8) if pl.pack == 'x6b' else K.xattn_pack(g, kv, nk2, nv2, m8, lean=pl.lean)
        Pm = None
        if pl.core == 'x6_f16':         # the forward core on single fp16 MFMAs, hi + lo (or o16) output, statistics for the bf16 backward
            o, P = K.xattn6_fwd(g, q.f16, K.xattn6_pack(g, kv.f16, m8), nk2, nv2, wth2, o_f16=pl.o16)
        elif pl.core == 'x2_f16':
            o, P = K.xattn2_fwd_f16(g, q, pk, wth2, o_f16=pl.o16)
        elif pl.core == 'x6_bf16':
            o, P = K.xattn6_fwd(g, q.hi, K.xattn6_pack(g, kv.hi, m8), nk2, nv2, wth2, lo=False)
        elif pl.core == 'x2_bf16':
            o, P = K.xattn2_fwd(g, q, pk, wth2)
        elif pl.core == 'x1_stats':
            o, P = K.xattn_fwd(g, q, pk, wth2, want_stats=True)
        else:
            o, P, Pm = K.xattn_fwd(g, q, pk, wth2, save=meta.get('save', True))
        if pl.core in ('x2_f16', 'x1_stats'):
            pk.drop_lo()
        y = K.gemm_nt_f16x2(o.f16, W['out_16']) if pl.o16 else K.gemm_nt(o, W['out'], out_bf16=_fast())
        return y, _sv(h, ctx, q, pk, P, Pm, o)

    @staticmethod
    def bwd(saved, dy, p, meta, need_dbias=False, dy_f32=None):
        h, ctx, q, pk, P, Pm, o = saved
        W = XInner.weights(meta['cache'], p)
        nk, nv, wth, wq, wkv, wo = p
        g = meta['xgeom']
        wth2 = wth.detach().reshape(g.heads, g.heads).contiguous()
        bwd = meta['plan'].bwd                  # the route the forward chose (and packed the images for)
        if bwd == 'x6_16':
            # fp16-gradient backward: dy = fp16(S dy); every large product on the fp16 MFMA against the fp16 copies the forward left
            s2 = dy.s2
            d_o = K.gemm_nt_f16ops(dy.t, W['outT_16'], out_f16=True)
            dwo = torch.empty_like(wo)
            K.gemm_tn16(dy.t, o.f16, dwo, s2)
            dq, dS, Pm, dwth = K.xattn6_bwd16(g, q.f16, d_o, pk, wth2, P, s2)
            dKp, dVp = K.xattn_kv_grads16(g, dS, Pm, q.f16, d_o, s2)
            dkv, dnk, dnv = K.xattn_unpack(g, dKp, dVp, lo=False, permuted=True, null_last=True)       # (context-sized from here on: bf16 as before)
            dh = K.G16(K.gemm_nt_f16ops(dq, W['qT_16'], out_f16=True), s2)
            dwq, dwkv = torch.empty_like(wq), torch.empty_like(wkv)
            K.gemm_tn16(dq, h.f16, dwq, s2)
            K.gemm_tn(dkv, ctx, dwkv)
            dctx = K.gemm_nt(dkv, W['kvT'])
            return dh, dctx, [dnk.reshape(nk.shape), dnv.reshape(nv.shape), dwth.reshape(wth.shape), dwq, dwkv, dwo]
        d_o = K.gemm_nt(dy, W['outT'], out_bf16=True)
        dwo = torch.empty_like(wo)
        K.gemm_tn(dy, o, dwo)
        if bwd == 'x2_rc':
            dq, dKp, dVp, dwth = K.xattn2_bwd_rc(g, q, d_o, pk, wth2, P)         # no dS / Pm arrays: the key side recomputes them
        else:
            if bwd == 'x1':
                dq, dS, dwth = K.xattn_bwd(g, d_o, pk, wth2, P)
            else:                               # dS / Pm columns in the kernel's chunk-permuted key order
                dq, dS, Pm, dwth = (K.xattn6_bwd if bwd == 'x6' else K.xattn2_bwd)(g, q, d_o, pk, wth2, P)
            dKp, dVp = K.xattn_kv_grads(g, dS, Pm, q, d_o)
        dkv, dnk, dnv = K.xattn_unpack(g, dKp, dVp, lo=dy.lo is not None, permuted=bwd in ('x6', 'x2'), null_last=bwd == 'x6')
        rot = meta.get('rotary')
        if rot is not None:
            dq = _rotary_bf(dq, rot, g.B, g.n, g.heads, inverse=True)
            dkv = _rotary_bf(dkv, rot, g.B, g.T, 2 * g.heads, inverse=True)
        dh = K.gemm_nt(dq, W['qT'], out_bf16=_fast_bwd())
        dwq, dwkv = torch.empty_like(wq), torch.empty_like(wkv)
        K.gemm_tn(dq, h, dwq)
        K.gemm_tn(dkv, ctx, dwkv)
        dctx = K.gemm_nt(dkv, W['kvT'])
        if meta.get('self_kv'):                  # the key/value rows ARE the query rows: one gradient for h
            dh = _as_f32(dh) + dctx
            dctx = None
        return dh, dctx, [dnk.reshape(nk.shape), dnv.reshape(nv.shape), dwth.reshape(wth.shape), dwq, dwkv, dwo]


def cattn_pack_keep(keep_bhij):
    """the mask arrays of the masked cattn kernels from a boolean keep mask [B, heads, n, T + 1] over (output head, query, key slot; slot 0 = the
    null key): (keep [B, n, KP], keep_t [B, T, NP], keep0 [B, n]) uint8, bit g = head g kept, KP / NP = T / n rounded up to 32, padding zero"""
    B, heads, n, J = keep_bhij.shape
    T = J - 1
    packed = torch.zeros((B, n, J), dtype=torch.uint8, device=keep_bhij.device)
    for g in range(heads):
        packed += keep_bhij[:, g].to(torch.uint8) * (1 << g)
    keep = torch.zeros((B, n, -(-T // 32) * 32), dtype=torch.uint8, device=packed.device)
    keep[:, :, :T] = packed[:, :, 1:]
    keep_t = torch.zeros((B, T, -(-n // 32) * 32), dtype=torch.uint8, device=packed.device)
    keep_t[:, :, :n] = packed[:, :, 1:].transpose(1, 2)
    return keep, keep_t, packed[:, :, 0].contiguous()


_CATTN_DRAW_MAX = 1 << 26          # most fp32 values of one transient draw of _cattn_keep_mask (256 MB)


def _cattn_keep_mask(B, n, T, heads, p, device):
    """keep mask of the nn.Dropout(p) on the mixed attention map [B, heads, n, T + 1] (np.py:370-374), as the mask arrays of the masked cattn
    kernels (cattn_pack_keep).  Drawn from torch's RNG stream a batch chunk at a time, so the transient fp32 draw stays bounded; tests replace
    this function by a fixed mask.  Under set_keep_mask_source('device') the generator kernel writes the three arrays directly, seeded from
    torch's RNG stream: no uniforms, no pack passes, no transposed copy"""
    if _KEEP_MASK_SOURCE == 'device':
        return K.keep_mask_cattn(B, n, T, heads, K.keep_threshold(p), _keep_seed(device))
    bc = max(1, min(B, _CATTN_DRAW_MAX // max(1, heads * n * (T + 1))))
    parts = [cattn_pack_keep(torch.rand((min(bc, B - b0), heads, n, T + 1), device=device) >= p) for b0 in range(0, B, bc)]
    return tuple(torch.cat(ts, 0) if len(ts) > 1 else ts[0] for ts in zip(*parts))


class CInner:
    """to_q(x), to_kv(x or context) -> plain attention core with linear memory (cattn: causal self-attention, or non-causal attention of the
    n rows over any number of keys -- their own or, with meta['has_ctx'], the T rows of meta['ctx_bf']) -> to_out (np.py:315-379).  params: null_k, null_v, talking_heads.w, to_q.w, to_kv.w, to_out.w  (the layout and weight cache of XInner).
    'bf16x3-fwd': hi + lo projections with an fp16 copy, the core on fp16 MFMAs, two-MFMA to_out; the backward on the bf16 hi parts.
    'bf16': bf16 throughout.  ('bf16x3' keeps the torch-op formulation: Attention._causal_hip_ok.)
    meta['drop_p'] (attention dropout in training, Attention.dropout_on_kernels): the masked forms of the same kernels; the mask arrays ride behind
    the saved tensors (so RngReplay's recomputed forward and the backward read the same ones)."""
    nparams = 6

    @staticmethod
    def _small(p, g):
        nk, nv, wth = p[0], p[1], p[2]
        return (nk.detach().float().reshape(g.heads, g.dim_head).contiguous(), nv.detach().float().reshape(g.heads, g.dim_head).contiguous(),
                wth.detach().float().reshape(g.heads, g.heads).contiguous())

    @staticmethod
    def fwd(h, p, meta):
        W = XInner.weights(meta['cache'], p)
        g = meta['cgeom']
        rot = meta.get('rotary')
        R, D, _ = K.bf_rows_cols(h)
        inner = g.heads * g.dim_head
        assert h.hi is not None, 'a bf16 backward needs the bf16 copy of the LayerNorm output'
        h = _f16_to_pair(h)
        has_ctx = bool(meta.get('has_ctx'))
        ctx = meta['ctx_bf'] if has_ctx else h              # (the context's copy is hi-only or hi + lo as the precision mode wants: _ctx_to_bf)
        assert not (has_ctx and rot is not None), 'rotary embeddings belong to self-attention'
        assert K.bf_rows_cols(ctx)[0] == g.B * K.cattn_keys(g)
        f16 = K.cores_f16() and h.lo is not None and ctx.lo is not None
        q = K.gemm_nt(h, W['q'], out_bf16=True, out_f16=f16 and rot is None)
        kv = K.gemm_nt(ctx, W['kv'], out_bf16=True, out_f16=f16 and rot is None)
        if rot is not None:
            q = _rotary_bf(q, rot, g.B, g.n, g.heads)
            kv = _rotary_bf(kv, rot, g.B, g.n, 2 * g.heads)
            if f16:
                q, kv = BF(q.hi, q.lo, K.hilo_to_f16(q)), BF(kv.hi, kv.lo, K.hilo_to_f16(kv))
        nk2, nv2, wth2 = CInner._small(p, g)
        drop_p = float(meta.get('drop_p') or 0.0)
        keep = _cattn_keep_mask(g.B, g.n, K.cattn_keys(g), g.heads, drop_p, h.hi.device) if drop_p else None
        dkw = dict(keep=keep, drop_scale=1.0 / (1.0 - drop_p)) if drop_p else {}
        o16 = False
        if f16:             # fp16 core; the output as a bf16 copy + an fp16 copy (two-MFMA to_out) or a bf16 hi + lo pair (3-MFMA to_out)
            o16 = K.proj_f16x2('o') and 'out_16' in W and K.gemm_nt_f16x2_ok(R, p[5].shape[0], p[5].shape[1], out_bf16=False)
            o, stats = K.cattn_fwd(g, q.f16, kv.f16[:, :inner], kv.f16[:, inner:], nk2, nv2, wth2, meta['mask_u8'], o_f16=o16, **dkw)
        else:
            o, stats = K.cattn_fwd(g, q.hi, kv.hi[:, :inner], kv.hi[:, inner:], nk2, nv2, wth2, meta['mask_u8'], lo=False, **dkw)
        y = K.gemm_nt_f16x2(o.f16, W['out_16']) if o16 else K.gemm_nt(o, W['out'], out_bf16=_fast())
        return y, (K.hi_only(h), K.hi_only(ctx) if has_ctx else None, K.hi_only(q), K.hi_only(kv), stats, K.hi_only(o)) + ((keep,) if drop_p else ())

    @staticmethod
    def bwd(saved, dy, p, meta, need_dbias=False, dy_f32=None):
        h, ctx, q, kv, stats, o = saved[:6]
        keep = saved[6] if len(saved) > 6 else None          # attention dropout: the mask arrays of the forward
        W = XInner.weights(meta['cache'], p)
        nk, nv, wth, wq, wkv, wo = p
        g = meta['cgeom']
        inner = g.heads * g.dim_head
        nk2, nv2, wth2 = CInner._small(p, g)
        dy = K.hi_only(dy)
        d_o = K.gemm_nt(dy, W['outT'], out_bf16=True)
        dwo = torch.empty_like(wo)
        K.gemm_tn(dy, o, dwo)
        dq, dkv, dwth, dnk, dnv = K.cattn_bwd(g, q.hi, kv.hi[:, :inner], kv.hi[:, inner:], d_o.hi, nk2, nv2, wth2, stats, meta['mask_u8'], keep=keep,
                                              drop_scale=1.0 / (1.0 - float(meta['drop_p'])) if keep is not None else 1.0)
        rot = meta.get('rotary')
        if rot is not None:
            dq = _rotary_bf(dq, rot, g.B, g.n, g.heads, inverse=True)
            dkv = _rotary_bf(dkv, rot, g.B, g.n, 2 * g.heads, inverse=True)
        dh = K.gemm_nt(dq, W['qT'], out_bf16=_fast_bwd())
        dwq, dwkv = torch.empty_like(wq), torch.empty_like(wkv)
        K.gemm_tn(dq, h, dwq)
        K.gemm_tn(dkv, h if ctx is None else ctx, dwkv)
        dctx = K.gemm_nt(dkv, W['kvT'])
        if ctx is None:
            dh, dctx = _as_f32(dh) + dctx, None             # the key / value rows ARE the query rows: one gradient for h
        return dh, dctx, [dnk.reshape(nk.shape), dnv.reshape(nv.shape), dwth.reshape(wth.shape), dwq, dwkv, dwo]


def _ff_keep_mask(R, C, p, device):
    """keep mask of nn.Dropout(p) over the GEGLU output [R, C] (torch's RNG stream, or under set_keep_mask_source('device') the generator
    kernel seeded from it; tests replace this function by a fixed mask)"""
    if _KEEP_MASK_SOURCE == 'device':
        return K.keep_mask_linear(R * C, K.keep_threshold(p), _keep_seed(device)).view(torch.bool).view(R, C)
    return torch.rand((R, C), device=device) >= p


def _ff_drop(t_f32, keep, p):
    """nn.Dropout in training: kept entries times 1 / (1 - p) (one fp32 multiply, as torch does), the others exactly 0"""
    return torch.where(keep, t_f32 * (1.0 / (1.0 - p)), torch.zeros((), dtype=t_f32.dtype, device=t_f32.device))


class FFInner:
    """Linear -> GEGLU -> Linear (np.py:255-286).  params: net.0.w (2*FFI, D), net.3.w (D, FFI).
    The inner width is zero-padded to FP = roundup(FFI, 32) inside the bf16 copies."""
    nparams = 2

    @staticmethod
    def weights(cache, p):
        w1, w2 = p

        def build():
            D, FFI = w2.shape
            FP = _ru(FFI, 32)
            dev = w1.device
            # FF1 rows in the interleaved-by-8 order (8 value rows, their 8 gate rows, ...): a lane of the GEMM epilogue owns 16
            # contiguous output columns, so it holds values AND gates and can apply the GEGLU gate itself
            w1pad = torch.zeros((2 * FP, D), dtype=torch.float32, device=dev)
            w1pad[:FFI] = w1.detach()[:FFI]
            w1pad[FP:FP + FFI] = w1.detach()[FFI:]
            w1il = K.geglu_interleave(w1pad, FP, dim=0).contiguous()
            w1p = K.zeros_bf((2 * FP, D), dev)
            K.cast_pad(w1il, w1p, row0=0)
            w1T = K.zeros_bf((D, 2 * FP), dev)
            K.transpose_cast(w1il, w1T, col0=0)
            w2p = K.zeros_bf((D, FP), dev)
            K.cast_pad(w2.detach(), w2p, Cp=FP)
            w2T = K.zeros_bf((FP, D), dev)
            K.transpose_cast(w2.detach(), w2T)
            out = dict(w1=w1p, w1T=w1T, w2=w2p, w2T=w2T, FP=FP, FFI=FFI)
            if K.mixed() and f16_weights_ok(w1, w2):    # fp16 copies for the fp16-operand forward GEMMs of 'bf16x3-fwd'
                out['w1_16'] = w1il.to(torch.float16).contiguous()
                w2pad = torch.zeros((D, FP), dtype=torch.float32, device=dev)
                w2pad[:, :FFI] = w2.detach()
                out['w2_16'] = w2pad.to(torch.float16)
                if K.bwd_f16('f'):                      # ... and their transposes for the dgrad products of the fp16-gradient backward
                    out['w1T_16'] = out['w1_16'].t().contiguous()
                    out['w2T_16'] = out['w2_16'].t().contiguous()
            return out
        return cache.get('ff', (w1, w2), build)

    @staticmethod
    def guarded(p):
        return (p[0], p[1])

    @staticmethod
    def plan(R, D, p, meta, has_resid=False, ln=True):
        """a16: 'bf16x3-fwd' wants the fp16-operand forward, both products run on the 256x256 ring and the weights sit inside the fp16 range.
        bwd16 (class 'f'): that, no live dropout (the fp16 GEGLU-backward epilogue has no mask input) and the four backward products fit"""
        w1, w2 = p
        FFI = w2.shape[1]
        FP = _ru(FFI, 32)
        a16 = bool(meta.get('shift') is None and K.ff_f16() and K.gemm_nt_f16ops_ok(R, 2 * FP, D, out_bf16=True, gate=True) and
                   K.gemm_nt_f16ops_ok(R, D, FP, out_bf16=False) and f16_weights_ok(w1, w2))
        b16 = bool(ln and a16 and not has_resid and not meta.get('drop_p') and K.bwd_f16('f') and
                   K.gemm_nt_f16ops_ok(R, FP, D, out_bf16=True, geglu_bwd=True) and K.gemm_nt_f16ops_ok(R, D, 2 * FP, out_bf16=False, out_f16=True) and
                   K.gemm_tn16_ok(R, D, FFI, lda=D, ldb=FP) and K.gemm_tn16_ok(R, 2 * FP, D))
        return Plan('only' if b16 else ln and a16, b16, (w1, w2), a16)

    @staticmethod
    def fwd(h, p, meta):
        W = FFInner.weights(meta['cache'], p)
        R, D, _ = K.bf_rows_cols(h)
        drop_p = float(meta.get('drop_p') or 0.0)
        pl = meta['plan']
        if pl.a16:
            # 'bf16x3-fwd': both FeedForward products on single fp16 MFMAs (h arrives with an fp16 copy from the LayerNorm store);
            # u and the gate output also leave as bf16 copies for the bf16 backward
            h16 = h.f16 if h.f16 is not None else K.hilo_to_f16(h)
            if pl.bwd16:
                # fp16-gradient backward: ONE copy of h and of the gate output (fp16); u stays bf16 (read element-wise by the gate's backward)
                u, gg16, _ = K.gemm_nt_f16ops(h16, W['w1_16'], out_bf16=True, gate=True, gate_bf16=False)
                y = K.gemm_nt_f16ops(gg16, W['w2_16'])
                return y, (K.BF(None, None, h16), K.BF(u, None), K.BF(None, None, gg16))
            assert h.hi is not None, 'a bf16 backward needs the bf16 copy of the LayerNorm output'
            if drop_p:          # ff_dropout > 0 in training (np.py:276): nn.Dropout on the GEGLU output, between the two products
                keep = _ff_keep_mask(R, W['FP'], drop_p, h16.device)
                if K.ff_drop_torch():        # (A/B switch: the torch element-wise formulation, the same bits)
                    u, gg16, ggb = K.gemm_nt_f16ops(h16, W['w1_16'], out_bf16=True, gate=True)
                    gf = _ff_drop(gg16.float(), keep, drop_p)
                    gg16, ggb = gf.to(torch.float16), gf.to(torch.bfloat16)
                else:
                    # one mask kernel: the dropped fp16 copy in place and the dropped bf16 copy from the same fp32 product (the GEMM's own --
                    # undropped -- bf16 copy of the gate output would have no reader: not written)
                    u, gg16, _ = K.gemm_nt_f16ops(h16, W['w1_16'], out_bf16=True, gate=True, gate_bf16=False)
                    gg16, ggb = K.geglu_dropout_fwd_f16(gg16, keep, 1.0 / (1.0 - drop_p))
                return K.gemm_nt_f16ops(gg16, W['w2_16']), (K.BF(h.hi, None), K.BF(u, None), K.BF(ggb, None), keep)
            u, gg16, ggb = K.gemm_nt_f16ops(h16, W['w1_16'], out_bf16=True, gate=True)
            y = K.gemm_nt_f16ops(gg16, W['w2_16'])
            return y, (K.BF(h.hi, None), K.BF(u, None), K.BF(ggb, None))
        h = _f16_to_pair(h)
        gg = K.empty_bf((h.hi.shape[0], W['FP']), h.hi.device)
        u = K.gemm_nt(h, W['w1'], out_bf16=True, shift=meta.get('shift'), geglu_out=gg)   # u (interleaved layout) and a * gelu(gate)
        if drop_p:
            keep = _ff_keep_mask(R, W['FP'], drop_p, h.hi.device)
            if K.ff_drop_torch():
                ggd = K.empty_bf((h.hi.shape[0], W['FP']), h.hi.device)
                K.cast_pad(_ff_drop(_bf_val(gg), keep, drop_p).contiguous(), ggd)
            else:
                ggd = K.geglu_dropout_fwd(gg, keep, 1.0 / (1.0 - drop_p))
            return K.gemm_nt(ggd, W['w2'], out_bf16=_fast()), (*_sv(h, u, ggd), keep)
        y = K.gemm_nt(gg, W['w2'], out_bf16=_fast())
        return y, _sv(h, u, gg)

    @staticmethod
    def bwd(saved, dy, p, meta, need_dbias=False, dy_f32=None):
        h, u, gg = saved[:3]
        keep = saved[3] if len(saved) > 3 else None          # FeedForward dropout: the keep mask of the forward (gg is the DROPPED gate output)
        W = FFInner.weights(meta['cache'], p)
        w1, w2 = p
        FP, FFI = W['FP'], W['FFI']
        if meta['plan'].bwd16:
            # fp16-gradient backward: dy = fp16(S dy); every product on the fp16 MFMA against the fp16 copies the forward left
            s2 = dy.s2
            du = K.gemm_nt_geglu_bwd16(dy.t, W['w2T_16'], u.hi, FP)
            dw2 = torch.empty_like(w2)
            K.gemm_tn16(dy.t, gg.f16, dw2, s2, N2=FFI)
            dh = K.G16(K.gemm_nt_f16ops(du, W['w1T_16'], out_f16=True), s2)
            dw1p = torch.empty((2 * FP, w1.shape[1]), dtype=torch.float32, device=w1.device)
            K.gemm_tn16(du, h.f16, dw1p, s2)
            d = K.geglu_deinterleave(dw1p, FP, dim=0)
            return dh, None, [torch.cat((d[:FFI], d[FP:FP + FFI]), 0), dw2]
        if keep is not None:
            dgg = K.gemm_nt(dy, W['w2T'], out_bf16=True)
            if K.ff_drop_torch():
                dgd = K.empty_bf(tuple(dgg.hi.shape), dgg.hi.device)
                K.cast_pad(_ff_drop(_bf_val(dgg), keep, float(meta['drop_p'])).contiguous(), dgd)
                du = K.geglu_bwd(u, dgd, FP, interleaved=True)
            else:               # the mask, its rounding and the gate's backward in one pass over u and the undropped dgg
                du = K.geglu_il_bwd_dropout(u, dgg, keep, 1.0 / (1.0 - float(meta['drop_p'])), FP)
        elif FUSE_GEGLU_BWD:
            du = K.gemm_nt_geglu_bwd(dy, W['w2T'], u, FP)      # dgg = dy W2 and the gate's backward in one pass
        else:
            du = K.geglu_bwd(u, K.gemm_nt(dy, W['w2T'], out_bf16=True), FP, interleaved=True)
        dw2 = torch.empty_like(w2)
        K.gemm_tn(dy, gg, dw2, N2=FFI)
        dh = K.gemm_nt(du, W['w1T'], out_bf16=_fast_bwd())
        sh = meta.get('shift')
        # one wgrad GEMM over the padded, interleaved [8 values | 8 gates | ...] row order, then back to the parameter's layout
        dw1p = torch.empty((2 * FP, w1.shape[1]), dtype=torch.float32, device=w1.device)

        def wgrad():
            K.gemm_tn(du, h, dw1p, shift=sh)
            d = K.geglu_deinterleave(dw1p, FP, dim=0)
            return torch.cat((d[:FFI], d[FP:FP + FFI]), 0)
        dw1 = wgrad()
        return dh, None, [dw1, dw2]


def _bf_val(t):
    """fp32 value of a BF pair"""
    return t.hi.float() if t.lo is None else t.hi.float() + t.lo.float()


def _bf_put(dst, index, value):
    """dst[index] = value (fp32) for a BF pair, rows selected by `index`"""
    hi = value.to(torch.bfloat16)
    dst.hi[index] = hi
    if dst.lo is not None:
        dst.lo[index] = (value - hi.float()).to(torch.bfloat16)


def _to_bf(value):
    out = K.empty_bf(tuple(value.shape), value.device)
    K.cast_pad(value.contiguous(), out)
    return out


class XC2Inner:
    """to_q(x), to_kv(sketch context) -> SparseCross2DNA core -> to_out (np.py:761-901).
    params: null_k, null_v, talking_heads.w, to_q.w, to_kv.w, to_out.w  (the layout of XInner)
    The windowed queries run on the 3DNA kernels pointed at the context (amdnuwa_cross2dna_*); the single <bos> query of every
    sample -- full attention over all context tokens, no talking heads (np.py:813-830) -- is B rows of glue arithmetic on torch ops
    between the kernels, forward and backward.  meta['drop_p'] (attention dropout in training, np.py:888-892): the masked forms of the same
    kernels; the mask is drawn here, covers the windowed queries only (the <bos> glue knows no dropout) and rides behind the saved tensors,
    so RngReplay's recomputed forward and the backward read the same one."""
    nparams = 6

    @staticmethod
    def _null(p, lo):
        nk, nv = p[0], p[1]
        mk = lambda t: _to_bf(t.detach().reshape(1, -1).float())
        a, b = mk(nk), mk(nv)
        return K.BF(a.hi.reshape(-1), None if a.lo is None else a.lo.reshape(-1)), K.BF(b.hi.reshape(-1), None if b.lo is None else b.lo.reshape(-1))

    @staticmethod
    def _bos_scores(q0, kf, nkf, keep, scale):
        """q0 [B,h,d], kf [B,T,h,d], nkf [h,d] -> softmax over [null | context] per (sample, head): [B,h,T+1]"""
        s = torch.cat((torch.einsum('bhd,hd->bh', q0, nkf)[..., None], torch.einsum('bhd,bthd->bht', q0, kf)), dim=-1) * scale
        if keep is not None:
            s = s.masked_fill(~torch.nn.functional.pad(keep, (1, 0), value=True)[:, None, :], -torch.finfo(torch.float32).max)
        return s.softmax(dim=-1)

    @staticmethod
    def fwd(h, p, meta):
        W = XInner.weights(meta['cache'], p)
        g, T = meta['geom'], meta['ctx_T']
        heads, dh = g.heads, g.dim_head
        inner = heads * dh
        wth2 = p[2].detach().reshape(heads, heads).contiguous()
        q = K.gemm_nt(h, W['q'], out_bf16=True)
        kv = K.gemm_nt(meta['ctx_bf'], W['kv'], out_bf16=True)
        nk, nv = XC2Inner._null(p, q.lo is not None)
        drop_p = float(meta.get('drop_p') or 0.0)
        keep_a = _attn_keep_mask(g.B, g.ntok - 1, g.kf * g.kh * g.kw + 1, heads, drop_p, q.hi.device) if drop_p else None
        dkw = dict(keep=keep_a, drop_scale=1.0 / (1.0 - drop_p)) if drop_p else {}
        o = K.cross2dna_fwd(g, q, kv, nk, nv, meta['mask_u8'], wth2, T, **dkw)
        # <bos> query rows
        rows0 = torch.arange(g.B, device=q.hi.device) * g.ntok
        q0 = _bf_val(K.BF(q.hi[rows0], None if q.lo is None else q.lo[rows0])).reshape(g.B, heads, dh)
        kvf = _bf_val(kv).reshape(g.B, T, 2, heads, dh)
        keep = meta['mask_u8'].bool() if meta['mask_u8'] is not None else None
        P0 = XC2Inner._bos_scores(q0, kvf[:, :, 0], _bf_val(nk).reshape(heads, dh), keep, g.scale)
        o0 = P0[..., :1] * _bf_val(nv).reshape(1, heads, dh) + torch.einsum('bht,bthd->bhd', P0[..., 1:], kvf[:, :, 1])
        _bf_put(o, rows0, o0.reshape(g.B, inner))
        y = K.gemm_nt(o, W['out'], out_bf16=_fast())
        return y, tuple(_sv(h, q, kv, nk, nv, o, P0)) + ((keep_a,) if drop_p else ())

    @staticmethod
    def bwd(saved, dy, p, meta, need_dbias=False, dy_f32=None):
        h, q, kv, nk, nv, o, P0 = saved[:7]
        keep_a = saved[7] if len(saved) > 7 else None        # attention dropout: the keep mask of the forward
        W = XInner.weights(meta['cache'], p)
        nkp, nvp, wth, wq, wkv, wo = p
        g, T = meta['geom'], meta['ctx_T']
        heads, dh = g.heads, g.dim_head
        inner = heads * dh
        wth2 = wth.detach().reshape(heads, heads).contiguous()
        d_o = K.gemm_nt(dy, W['outT'], out_bf16=True)
        dwo = torch.empty_like(wo)
        K.gemm_tn(dy, o, dwo)
        dkw = dict(keep=keep_a, drop_scale=1.0 / (1.0 - float(meta['drop_p']))) if keep_a is not None else {}
        dq, dkv, dnk, dnv, dwth = K.cross2dna_bwd(g, q, kv, nk, nv, meta['mask_u8'], wth2, d_o, T, **dkw)
        # <bos> query rows: softmax attention backward on B rows
        rows0 = torch.arange(g.B, device=q.hi.device) * g.ntok
        sub = lambda t: _bf_val(K.BF(t.hi[rows0], None if t.lo is None else t.lo[rows0])).reshape(g.B, heads, dh)
        q0, dO0 = sub(q), sub(d_o)
        kvf = _bf_val(kv).reshape(g.B, T, 2, heads, dh)
        nkf, nvf = _bf_val(nk).reshape(heads, dh), _bf_val(nv).reshape(heads, dh)
        dP = torch.cat((torch.einsum('bhd,hd->bh', dO0, nvf)[..., None], torch.einsum('bhd,bthd->bht', dO0, kvf[:, :, 1])), dim=-1)
        dS = P0 * (dP - (P0 * dP).sum(-1, keepdim=True)) * g.scale
        dq0 = dS[..., :1] * nkf[None] + torch.einsum('bht,bthd->bhd', dS[..., 1:], kvf[:, :, 0])
        _bf_put(dq, rows0, dq0.reshape(g.B, inner))
        # the <bos> query's share of dK / dV is a separate (small) term: it goes through the two products below as its own operand instead
        # of being added into the kernel's bf16 dkv and rounded a second time
        dkv0 = _to_bf(torch.stack((torch.einsum('bht,bhd->bthd', dS[..., 1:], q0), torch.einsum('bht,bhd->bthd', P0[..., 1:], dO0)),
                                  dim=2).reshape(g.B * T, 2 * inner))
        dnk = dnk + torch.einsum('bh,bhd->hd', dS[..., 0], q0).reshape(-1)
        dnv = dnv + torch.einsum('bh,bhd->hd', P0[..., 0], dO0).reshape(-1)
        dh_ = K.gemm_nt(dq, W['qT'], out_bf16=_fast_bwd())
        dwq, dwkv = torch.empty_like(wq), torch.empty_like(wkv)
        K.gemm_tn(dq, h, dwq)
        K.gemm_tn(dkv, meta['ctx_bf'], dwkv)
        K.gemm_tn(dkv0, meta['ctx_bf'], dwkv, beta=1.0)
        dctx = K.gemm_nt(dkv, W['kvT']) + K.gemm_nt(dkv0, W['kvT'])
        return dh_, dctx, [dnk.reshape(nkp.shape), dnv.reshape(nvp.shape), dwth.reshape(wth.shape), dwq, dwkv, dwo]


INNERS = {'s3': S3Inner, 'xattn': XInner, 'ff': FFInner, 'xc2': XC2Inner, 'cattn': CInner}

FUSE_LINEAR_CE = os.environ.get('AMDNUWA_FUSE_LINEAR_CE', '1') != '0'   # to_logits + cross entropy without the fp32 logits (A/B switch)
# ... in 'bf16x3-fwd' (hi + lo logits): OFF by default.  The fused form needs the three-MFMA product twice (statistics, then dlogits -- the
# latter on one fp16 MFMA) where the unfused one writes the fp32 logits once and reads them once: measured 532.5-534.1 against 530.2-530.7 ms
# per step at b = 128, for 9 GB less peak memory (243 -> 234 GB).  AMDNUWA_FUSE_LINEAR_CE_X3 = 1 turns it on -- a trainer that runs the WHOLE
# reference step at b = 128 wants it: with tokenizer, text encoder and optimiser state next to the decoder the unfused step sits at 244 GiB of
# 288 and ran 708-919 ms depending on how often the allocator had to retry; fused it runs 701-713 ms at 235 GiB (tools/full_step.py turns it on
# from b = 112).  'auto' = fused when the fp32 logits + bf16 dlogits would push the device past AMDNUWA_FUSE_LINEAR_CE_X3_MEM_FRAC of its memory.
_F = os.environ.get('AMDNUWA_FUSE_LINEAR_CE_X3', '0')
FUSE_LINEAR_CE_X3 = True if _F == '1' else ('auto' if _F == 'auto' else False)
FUSE_LINEAR_CE_X3_MEM_FRAC = float(os.environ.get('AMDNUWA_FUSE_LINEAR_CE_X3_MEM_FRAC', '0.82'))


def _fuse_ce_x3(rows, classes, device):
    if FUSE_LINEAR_CE_X3 != 'auto':
        return bool(FUSE_LINEAR_CE_X3)
    if device.type != 'cuda':
        return False
    need = rows * classes * (4 + 2)             # fp32 logits + bf16 dlogits
    total = torch.cuda.get_device_properties(device).total_memory
    return torch.cuda.memory_allocated(device) + need > FUSE_LINEAR_CE_X3_MEM_FRAC * total


FUSE_GEGLU_BWD = os.environ.get('AMDNUWA_FUSE_GEGLU_BWD', '1') != '0'   # gate backward inside the dgg GEMM epilogue (A/B switch)
CHAIN_BWD = os.environ.get('AMDNUWA_CHAIN_BWD', '1') != '0'      # chain the LayerNorm backwards across block boundaries (A/B switch)
def _fast():
    """fast bf16 mode: the GEMMs that feed a LayerNorm (to_out / FF w2 outputs, dgrad outputs) write bf16 and the LN kernels
    read bf16 -- half the epilogue and LN traffic.  Parity mode (bf16x3) keeps those tensors in fp32."""
    return K.fast_io()


def _fast_bwd():
    """dgrad GEMM outputs that feed a LayerNorm backward are bf16 unless the BACKWARD itself runs 3-MFMA products ('bf16x3')"""
    return K.get_precision() != 'bf16x3'


def _sv(*ts):
    """what an inner stage keeps for its backward: in the mixed mode ('bf16x3-fwd') the hi parts only -- the lo parts die with the
    forward of the block"""
    return tuple(K.hi_only(t) for t in ts) if K.mixed() else ts


def _as_f32(t):
    return t.hi.float() if isinstance(t, K.BF) else t


GRAD_SCALE_LOG2 = float(os.environ.get('AMDNUWA_GRAD_SCALE_LOG2', '-4'))      # S * max|g| in [2^x, 2^(x+1))


def _grad_scale(g2):
    """device tensor {S, 1 / S} for the fp16 gradients of one backward pass: S = the power of two with S * max|g| in [2^-4, 2^-3), g = the
    residual-stream gradient entering the first block of the pass (kernels.G16).  No host synchronisation.
    Why that low (round 5 used [8, 16)): the gradients INSIDE the blocks are larger than the stream's -- a post-norm backward multiplies by
    w / std(y), and the cross-attention block's y is small -- and they grow towards layer 0: on the random-init cfg-3 stack (24 layers)
    |S g| of the cross-attention blocks' dy climbs from 1.2e3 at the top to beyond 65504 at layers 0 and 1 with [8, 16) (tools/grad_range.py,
    profiles/r06l_grad_range.txt: saturation counter 36).  Seven bits lower the largest tensor peaks at 2^9 and the smallest (|S g| max 0.1)
    still keeps 8 significant bits -- bf16's -- down to 2^-12 of its own maximum (fp16 is normal to 6.1e-5, subnormal to 6e-8)."""
    a = g2.detach().abs().amax().float()
    ok = torch.isfinite(a) & (a > 0)
    e = torch.floor(torch.log2(torch.where(ok, a, torch.ones_like(a))))
    S = torch.where(ok, torch.exp2((GRAD_SCALE_LOG2 - e).clamp(-60.0, 60.0)), torch.ones_like(a))
    return torch.stack((S, 1.0 / S)).contiguous()


def _takes_ctx(meta):
    """does the inner stage project keys / values from a context tensor (and so want its BF copy in meta['ctx_bf'])?"""
    return (meta['kind'] in ('xattn', 'xc2') and not meta.get('self_kv')) or (meta['kind'] == 'cattn' and bool(meta.get('has_ctx')))


def _ctx_rows(meta):
    """rows per sample of the context an inner stage read"""
    if meta['kind'] == 'xc2':
        return meta['ctx_T']
    return K.cattn_keys(meta['cgeom']) if meta['kind'] == 'cattn' else meta['xgeom'].T


_CTX_CAST = [None, -1, None, None]      # (weak reference to the context tensor, the key of its memory, its BF copy, its storage -- held, see WeightCache)


def _ctx_cast_reset():
    _CTX_CAST[:] = [None, -1, None, None]


def _ctx_cast_drop(ref):
    """the context tensor died: release its copy"""
    if _CTX_CAST[0] is ref:
        _ctx_cast_reset()


def _ctx_to_bf(context):
    """context fp32 [B, T, D] -> BF [B*T, D].  Every cross-attention block of a stack receives the SAME context tensor: its cast (27 us at
    cfg 3, b = 128) runs once per tensor object, storage and version, not once per layer (the copy is read-only: kv projection, its weight
    gradient).  The copy is hi-only or hi + lo as the precision mode wants: a copy cast in another mode is not reused.  weights_changed()
    drops it."""
    ref = _CTX_CAST[0]
    lo = K.want_lo()
    if ref is not None and ref() is context and _CTX_CAST[1] == _storage_key(context) and (_CTX_CAST[2].lo is not None) == lo:
        return _CTX_CAST[2]
    B, T, D = context.shape
    out = K.empty_bf((B * T, D), context.device, lo=lo)
    K.cast_pad(context.detach().reshape(B * T, D), out)
    try:
        _CTX_CAST[:] = [weakref.ref(context, _ctx_cast_drop), _storage_key(context), out, context.untyped_storage()]
    except TypeError:
        _ctx_cast_reset()
    return out


# =================================================================================================
# fused decoder sub-block:  x_out = x + postLN(inner(shift(preLN(x))))
# =================================================================================================

class SandwichBlockFn(Function):
    """x_out = (resid if given else x) + postLN(inner(shift(preLN(x)))).
    args: x [B, n, D] fp32, resid (or None), context (or None), meta dict, pre_w, pre_b, post_w, post_b, *inner params"""

    @staticmethod
    @_in_phase('fwd')
    def forward(ctx, x, resid, context, meta, pre_w, pre_b, post_w, post_b, *p):
        inner = INNERS[meta['kind']]
        B, n, D = x.shape
        x2 = x.detach().contiguous().reshape(B * n, D)
        r2_ = x2 if resid is None else resid.detach().contiguous().reshape(B * n, D)
        meta = dict(meta)
        if _takes_ctx(meta):
            meta['ctx_bf'] = _ctx_to_bf(context)
        # the token shift is folded into the pre-LN's STORE: h = shift(LN(x)) is what the forward GEMM and the weight-gradient
        # GEMM consume (plain loaders); only the pre-LN backward still reads its incoming gradient through the inverse shift
        ctx.shift = sh = meta.get('shift')
        if sh is not None:
            meta['shift'] = None
        # block chaining (Transformer.forward_layers): the previous block's post-norm kernel may already have produced this
        # block's h = shift(LN(x)) while the new stream row was in its registers, and this block does the same for the next
        hin, nxt, hout = meta.pop('handoff_in', None), meta.pop('next_pre', None), meta.pop('handoff_out', None)
        ctx.prev_ctx = None
        plan = block_plan(meta['kind'], B * n, D, p, meta, resid is not None)
        if hin is not None and hin.get('ptr') == x.data_ptr() and hin.get('ver') == x._version and hin.get('shift') == sh \
                and resid is None and K.bf_rows_cols(hin['h'])[:2] == (B * n, D) and (hin['h'].hi is not None or plan.bwd16):
            h, m1, r1 = hin['h'], hin['m1'], hin['r1']
            ctx.prev_ctx = hin.get('ctx')          # the backward chains the two LayerNorm backwards of this boundary too
            if plan.bwd16 and h.f16 is None:       # a hand-off without the fp16 copy (a predecessor that did not plan for this block): bf16 backward
                plan = block_plan(meta['kind'], B * n, D, p, meta, True)           # (has_resid gates bwd16 and nothing else: every plan() keeps that)
        else:
            h, m1, r1, _ = K.ln_fwd(x2, pre_w.detach(), pre_b.detach(), shift=sh, f16=plan.h16)
        meta['plan'], ctx.bw16 = plan, plan.bwd16
        y, saved = inner.fwd(h, p, meta)
        if nxt is not None and hout is not None:
            # the form the next block reads its LayerNorm output in: ITS plan, from the (kind, params, meta, has_resid) fused_residual handed over
            # (None: a block the chain does not plan for -- it gets the bf16 hi[/lo] form)
            nxt16 = block_plan(nxt[3][0], B * n, D, *nxt[3][1:]).h16 if nxt[3] is not None else False
            xo, m2, r2, hn, mn, rn = K.ln_post_pre_fwd(y, r2_, post_w.detach(), post_b.detach(), nxt[0].detach(),
                                                       nxt[1].detach(), next_shift=nxt[2], next_f16=nxt16)
            hout.update(h=hn, m1=mn, r1=rn, ptr=xo.data_ptr(), ver=xo._version, shift=nxt[2], ctx=ctx if CHAIN_BWD else None)
        else:
            xo, m2, r2 = K.ln_fwd(y, post_w.detach(), post_b.detach(), resid=r2_, minus=bool(meta.get('resid_minus')))
        ctx.meta, ctx.inner_saved, ctx.p = meta, saved, p
        ctx.has_ctx = context is not None
        ctx.has_resid = resid is not None
        ctx.y_bf = isinstance(y, K.BF)
        ctx.save_for_backward(x2, y.hi if ctx.y_bf else y, m1, r1, m2, r2, pre_w, post_w)
        ctx.shape = (B, n, D)
        return xo.reshape(B, n, D)

    @staticmethod
    @_in_phase('bwd')
    def backward(ctx, g):
        x2, y, m1, r1, m2, r2, pre_w, post_w = ctx.saved_tensors
        if ctx.y_bf:
            y = K.BF(y, None)
        B, n, D = ctx.shape
        meta, p = ctx.meta, ctx.p
        inner = INNERS[meta['kind']]
        g2 = g.contiguous().reshape(B * n, D)
        want_bias = meta['kind'] == 's3'
        ho, ctx.bwd_handoff = getattr(ctx, 'bwd_handoff', None), None
        bw16 = getattr(ctx, 'bw16', False)
        s2 = ho.get('s2') if ho is not None else None          # the gradient scale of this backward pass (fp16-gradient blocks)
        # (only where this block or the one its chained LayerNorm backward feeds runs on fp16 gradients: a reversible stack -- no such block --
        #  paid one amax pass over the stream per block for a scale nobody read: cfg 4 -4 %)
        if s2 is None and (bw16 or getattr(ctx.prev_ctx, 'bw16', False)):
            s2 = _grad_scale(g2)
        if ho is not None and ho['ptr'] == g2.data_ptr() and ho['ver'] == g2._version and isinstance(ho['dy'], K.G16) == bw16:   # the next block's backward already ran this post-norm backward
            dy, dpost_w, dpost_b, dsum = ho['dy'], ho['dw'], ho['db'], ho['dsum']
        else:
            dy, dpost_w, dpost_b, dsum = K.ln_bwd(g2, y, m2, r2, post_w.detach(), to_bf=not bw16, want_dsum=want_bias,
                                                  to_f16=s2 if bw16 else None)
        meta = dict(meta)
        dh, dctx, grads = inner.bwd(ctx.inner_saved, dy, p, meta, need_dbias=False)
        if want_bias:
            grads[4] = dsum                      # to_out.bias grad = column sums of d(to_out output)
        prev = ctx.prev_ctx
        p16 = prev is not None and getattr(prev, 'bw16', False) and s2 is not None
        if prev is not None and not ctx.has_resid and (isinstance(dh, (K.BF, K.G16)) or not prev.y_bf) and (not isinstance(dh, K.BF) or dh.lo is None) \
                and not (isinstance(dh, K.G16) and prev.y_bf):
            # pre-norm backward of this block + post-norm backward of the previous block on the same gradient row
            _, py, _, _, pm2, pr2, _, ppost_w = prev.saved_tensors
            dx, dpre_w, dpre_b, dyp, dwp, dbp, dsp = K.ln_bwd_chain(
                dh, x2, m1, r1, pre_w.detach(), g2, K.BF(py, None) if prev.y_bf else py, pm2, pr2, ppost_w.detach(),
                shift=ctx.shift, want_dsum=prev.meta['kind'] == 's3', out_f16=s2 if p16 else None)
            prev.bwd_handoff = dict(ptr=dx.data_ptr(), ver=dx._version, dy=dyp, dw=dwp, db=dbp, dsum=dsp, s2=s2)
        else:
            # (dx_add: a gradient the caller would add to dx anyway -- the reversible reconstruction's dy1 + dL/dy1 -- rides in as the pre-norm
            #  backward's accumulator, as the residual-stream gradient does on the plain stack: no separate add pass over the stream)
            add = getattr(ctx, 'dx_add', None)
            ctx.dx_add = None
            if add is not None:
                add = add.detach().contiguous().reshape(B * n, D)
            dx, dpre_w, dpre_b, _ = K.ln_bwd(dh, x2, m1, r1, pre_w.detach(), dres=(add if ctx.has_resid else g2), shift=ctx.shift)
        ctx.prev_ctx = None
        dcontext = None
        if ctx.has_ctx:
            dcontext = dctx.reshape(B, _ctx_rows(meta), D)
        ctx.inner_saved = None
        dresid = g if ctx.has_resid else None
        return (dx.reshape(B, n, D), dresid, dcontext, None, dpre_w, dpre_b, dpost_w, dpost_b, *grads)


# =================================================================================================
# standalone inner module call:  y = inner(x)  (fp32 in / fp32 out), e.g. Sparse3DNA(x) on its own
# =================================================================================================

class InnerFn(Function):
    @staticmethod
    @_in_phase('fwd')
    def forward(ctx, x, context, meta, *p):
        inner = INNERS[meta['kind']]
        B, n, D = x.shape
        x2 = x.detach().contiguous().reshape(B * n, D)
        meta = dict(meta)
        if _takes_ctx(meta):
            meta['ctx_bf'] = _ctx_to_bf(context)
        h = K.empty_bf((B * n, D), x.device)
        K.cast_pad(x2, h)
        meta['plan'] = block_plan(meta['kind'], B * n, D, p, meta, ln=False)
        y, saved = inner.fwd(h, p, meta)
        ctx.meta, ctx.inner_saved, ctx.p = meta, saved, p
        ctx.has_ctx = context is not None
        ctx.shape = (B, n, D)
        y = _as_f32(y)
        return y.reshape(B, n, y.shape[-1])

    @staticmethod
    @_in_phase('bwd')
    def backward(ctx, g):
        B, n, D = ctx.shape
        meta, p = ctx.meta, ctx.p
        inner = INNERS[meta['kind']]
        g2 = g.contiguous().reshape(B * n, -1)
        dy = K.empty_bf(tuple(g2.shape), g.device)
        K.cast_pad(g2, dy)
        meta = dict(meta)
        dh, dctx, grads = inner.bwd(ctx.inner_saved, dy, p, meta, need_dbias=True, dy_f32=g2)
        dcontext = dctx.reshape(B, _ctx_rows(meta), -1) if ctx.has_ctx else None
        ctx.inner_saved = None
        return (_as_f32(dh).reshape(B, n, D), dcontext, None, *grads)


# =================================================================================================
# LayerNorm / StableLayerNorm as standalone nodes (fp32 in -> fp32 out)
# =================================================================================================

class LayerNormFn(Function):
    @staticmethod
    @_in_phase('fwd')
    def forward(ctx, x, w, b, stable):
        shp = x.shape
        x2 = x.detach().contiguous().reshape(-1, shp[-1])
        zero = torch.zeros_like(x2)
        if stable:
            raise RuntimeError('use StableLNLogitsFn / stable_ln_bf')
        out, m, r = K.ln_fwd(x2, w.detach(), b.detach(), resid=zero)
        ctx.save_for_backward(x2, m, r, w)
        ctx.shp = shp
        return out.reshape(shp)

    @staticmethod
    @_in_phase('bwd')
    def backward(ctx, g):
        x2, m, r, w = ctx.saved_tensors
        g2 = g.contiguous().reshape(x2.shape)
        dx, dw, db, _ = K.ln_bwd(g2, x2, m, r, w.detach())
        return dx.reshape(ctx.shp), dw, db, None


class StableLNFn(Function):
    """StableLayerNorm (np.py:88-95) -> fp32 output (value of the bf16 hi[/lo] pair the logits GEMM consumes is
    produced separately in LogitsFn; standalone use returns fp32)."""

    @staticmethod
    @_in_phase('fwd')
    def forward(ctx, x, w, b):
        shp = x.shape
        x2 = x.detach().contiguous().reshape(-1, shp[-1])
        out, m, r, ia = K.ln_fwd(x2, w.detach(), b.detach(), stable=True)
        ctx.save_for_backward(x2, m, r, ia, w)
        ctx.shp = shp
        y = out.hi.float()
        if out.lo is not None:
            y = y + out.lo.float()
        return y.reshape(shp)

    @staticmethod
    @_in_phase('bwd')
    def backward(ctx, g):
        x2, m, r, ia, w = ctx.saved_tensors
        g2 = g.contiguous().reshape(x2.shape)
        dx, dw, db, _ = K.ln_bwd(g2, x2, m, r, w.detach(), inv_amax=ia)
        return dx.reshape(ctx.shp), dw, db


# =================================================================================================
# final StableLayerNorm + to_logits (+ cross entropy)   np.py:1182, 1958-1963
# =================================================================================================

def _logits_f16x2(W, wl, R, D):
    """'bf16x3-fwd' with the two-MFMA switch on: to_logits takes the final LayerNorm output as ONE fp16 value and the weight as an fp16
    hi + lo pair (built once per weight version; None = outside the fp16 range)"""
    if not K.proj_f16x2('l'):
        return False
    if 'w_16' not in W:
        W['w_16'] = K.f16_pair(wl) if f16_weights_ok(wl) else None
    return W['w_16'] is not None and K.gemm_nt_f16x2_ok(R, wl.shape[0], D, out_bf16=False)


class LogitsFn(Function):
    """x [B, n, D] -> logits [B, n, C] fp32 (StableLayerNorm then Linear without bias)"""

    @staticmethod
    @_in_phase('fwd')
    def forward(ctx, x, nw, nb, wl, cache):
        B, n, D = x.shape
        x2 = x.detach().contiguous().reshape(B * n, D)
        W = cache.get('logits', (wl,), lambda: dict(w=_cast(wl), wT=_cast_t(wl)))
        lx2 = _logits_f16x2(W, wl, B * n, D)
        hn, m, r, ia = K.ln_fwd(x2, nw.detach(), nb.detach(), stable=True, f16=lx2)
        logits = K.gemm_nt_f16x2(hn.f16, W['w_16']) if lx2 else K.gemm_nt(hn, W['w'])
        ctx.save_for_backward(x2, m, r, ia, nw, wl)
        ctx.hn, ctx.W, ctx.shape = _sv(hn)[0], W, (B, n, D)
        return logits.reshape(B, n, -1)

    @staticmethod
    @_in_phase('bwd')
    def backward(ctx, g):
        x2, m, r, ia, nw, wl = ctx.saved_tensors
        B, n, D = ctx.shape
        g2 = g.contiguous().reshape(B * n, -1)
        dl = K.empty_bf(tuple(g2.shape), g.device)
        K.cast_pad(g2, dl)
        dhn = K.gemm_nt(dl, ctx.W['wT'])
        dwl = torch.empty_like(wl)
        K.gemm_tn(dl, ctx.hn, dwl)
        dx, dnw, dnb, _ = K.ln_bwd(dhn, x2, m, r, nw.detach(), inv_amax=ia)
        ctx.hn = None
        return dx.reshape(B, n, D), dnw, dnb, dwl, None


class LogitsLossFn(Function):
    """x [B, n, D], targets [B, n] -> scalar mean cross-entropy.  dlogits is produced in the forward
    (bf16 hi[/lo], already divided by the number of targets) so the fp32 logits are read only once."""

    @staticmethod
    @_in_phase('fwd')
    def forward(ctx, x, targets, nw, nb, wl, cache):
        B, n, D = x.shape
        x2 = x.detach().contiguous().reshape(B * n, D)
        W = cache.get('logits', (wl,), lambda: dict(w=_cast(wl), wT=_cast_t(wl)))
        fuse_x3 = K.mixed() and _fuse_ce_x3(B * n, wl.shape[0], x.device)
        if fuse_x3 and 'w16' not in W:       # fp16 copy for the dlogits pass of the fused cross entropy (None: outside the fp16 range)
            W['w16'] = wl.detach().to(torch.float16).contiguous() if f16_weights_ok(wl) else None
        use_fused = fuse_x3 if K.mixed() else FUSE_LINEAR_CE
        lx2 = not use_fused and _logits_f16x2(W, wl, B * n, D)
        hn, m, r, ia = K.ln_fwd(x2, nw.detach(), nb.detach(), stable=True, f16=lx2)
        if targets.dtype != torch.int64:
            raise TypeError(f'cross-entropy targets must be int64 token ids, got {targets.dtype}')
        if targets.numel() != B * n:
            raise ValueError(f'{targets.numel()} targets for {B * n} logit rows')
        t = targets.contiguous().reshape(-1)            # ids outside [0, C) give a NaN loss (the kernel never reads out of bounds)
        want_grad = any(ctx.needs_input_grad)
        fused = K.linear_ce(hn, W['w'], t, 1.0 / (B * n), want_grad=want_grad, w16=W.get('w16')) if use_fused else None
        if fused is not None:                           # 'bf16' (and 'bf16x3-fwd' on request): logits produced twice inside the GEMM ring, never written (np.py:1958-1963)
            loss, dl = fused
        else:
            logits = K.gemm_nt_f16x2(hn.f16, W['w_16']) if lx2 else K.gemm_nt(hn, W['w'])
            loss, dl = K.ce_fwd(logits, t, 1.0 / (B * n), want_grad=want_grad, lo=False if K.mixed() else None)
            del logits
        ctx.save_for_backward(x2, m, r, ia, nw, wl)
        ctx.hn, ctx.dl, ctx.W, ctx.shape = _sv(hn)[0], dl, W, (B, n, D)
        return loss

    @staticmethod
    @_in_phase('bwd')
    def backward(ctx, g):
        x2, m, r, ia, nw, wl = ctx.saved_tensors
        B, n, D = ctx.shape
        assert ctx.dl.hi is not None
        dhn = K.gemm_nt(ctx.dl, ctx.W['wT'])
        dwl = torch.empty_like(wl)
        K.gemm_tn(ctx.dl, ctx.hn, dwl)
        gs = g.detach().reshape(1).float().contiguous()
        K.scale_by_device_scalar(dwl, gs)
        # the upstream gradient of the loss rides into the final norm's backward as a device scalar (it cost a read-modify-write pass over dhn)
        dx, dnw, dnb, _ = K.ln_bwd(dhn, x2, m, r, nw.detach(), inv_amax=ia, dy_scale2=torch.cat((gs, gs)))
        ctx.hn = ctx.dl = None
        return dx.reshape(B, n, D), None, dnw, dnb, dwl, None


# =================================================================================================
# embedding assemble  (np.py:1940-1944)
# =================================================================================================

class EmbedAssembleFn(Function):
    """ids [B, n-1] int64 -> x [B, n, D] fp32 = cat(bos, pos[:n-1] + frac_gradient(emb(ids)))"""

    @staticmethod
    @_in_phase('fwd')
    def forward(ctx, ids, W, ax1, ax2, ax3, bos, video_shape, frac):
        B, n1 = ids.shape
        ntok = n1 + 1
        F, H, Wd = video_shape
        ids_c = ids.contiguous()
        x = K.embed_fwd(ids_c, W.detach(), ax1.detach(), ax2.detach(), ax3.detach(), bos.detach(), B, ntok, H, Wd, frac)
        ctx.save_for_backward(ids_c)
        ctx.meta = (B, ntok, F, H, Wd, frac, W.shape, ax1.shape, ax2.shape, ax3.shape, bos.shape)
        return x.reshape(B, ntok, -1)

    @staticmethod
    @_in_phase('bwd')
    def backward(ctx, g):
        (ids,) = ctx.saved_tensors
        B, ntok, F, H, Wd, frac, ws, s1, s2, s3, sb = ctx.meta
        dev = g.device
        g2 = g.contiguous().reshape(B * ntok, -1)
        dW = torch.zeros(ws, dtype=torch.float32, device=dev)
        d1, d2, d3 = (torch.zeros(s, dtype=torch.float32, device=dev) for s in (s1, s2, s3))
        db = torch.zeros(sb, dtype=torch.float32, device=dev)
        K.embed_bwd(ids, g2, dW, d1, d2, d3, db, B, ntok, F, H, Wd, frac)
        return None, dW, d1, d2, d3, db, None, None
