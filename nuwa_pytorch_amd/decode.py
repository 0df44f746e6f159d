"""Key/value-cached token-by-token decoding for NUWA.generate (reference np.py:1841-1915).

The reference recomputes the whole prefix -- twice, for classifier-free guidance -- for every sampled token.  Every stage of
the decoder is causal (Sparse3DNA taps, np.py:420-457; ShiftVideoTokens, np.py:210-253) or row-wise (cross-attention over the
text, FeedForward, the norms), so row `pos` of the decoder depends only on rows <= pos.  IncrementalDecoder keeps, per layer,
  * the pre-norm outputs of the two token-shifted blocks (the shift reads the rows one grid row up / one token left),
  * the Sparse3DNA key / value rows,
  * the packed text keys / values of the cross-attention (computed once) -- or, for a context of more than 287 tokens and
    long_context=True, the to_kv rows themselves, attended in place (amdnuwa_attn_decode_rows; amdnuwa_attn_rows in the prefill),
and computes ONE new row per call with the same libamdnuwa kernels the training path uses (GEMMs, LayerNorms, GEGLU, the
cross-attention core with n = 1) plus the two single-row kernels of csrc/decode.hip.  The row index lives in device memory,
so the per-token work of a whole guided step can be captured once in a HIP graph and replayed for every token.

Past max_video_frames NUWA.generate slides its frame window (np.py:1873-1881): every kept token moves one frame earlier, its position
embedding changes and with it every cached row of every layer.  IncrementalDecoder.prefill / GuidedStepper.prefill rebuild the caches
with ONE full-sequence pass over the rows the new window already determines -- the same block walk as step() (IncrementalDecoder._walk)
in its R-rows mode: the rows forms of the two norm / cache kernels (amdnuwa_prefill_ln, amdnuwa_prefill_kv) and the full-sequence
attention cores of the training path, in the operand forms of the single row -- after which the captured row step serves the new
frame's tokens again.  NUWASketch.generate slides the same way (np.py:2470-2474): its SparseCross2DNA blocks take the rows form of their
single-row kernel (amdnuwa_cross2dna_rows), the window read in place.

NUWAVideoAudio.generate (np.py:2111-2222) decodes two interleaved streams through the DualModalityDecoder (np.py:1299-1487).  Every
stage is row-causal there too: the audio window attention looks back only, and the chunked video <-> audio attention lets frame t
of one stream see frame t - 1 of the other (np.py:908-1067), which is complete -- and final -- by the time any row of frame t is
computed, because the sampler alternates one video frame / one audio frame.  DualIncrementalDecoder therefore keeps one
IncrementalDecoder per modality (own position counter) and links the two at the cross-modality layers: each stream stores its
layer-input rows projected with the OTHER direction's to_kv, and attends the other stream's stored rows of the matching frame."""
import os
from functools import partial

import torch
import torch.nn.functional as F

from . import kernels as K
from . import ops


class _Block:
    """one sub-block of a row program: out_slot <- out_slot + post(inner(pre(in_slot)));  pre / post = None for the un-normed modules
    of the reversible dual decoder's cross-modality layer"""
    __slots__ = ('kind', 'pre', 'post', 'inner', 'fmap', 'hcache', 'kvcache', 'geom', 'pk', 'xg', 'o_const', 'xm', 'src', 'dst',
                 'store_before', 'store_after', 'c2', 'wth', 'rel', 'long', 'ctx_kv', 'first0', 'mask_u8', 'nk', 'nv')


X_PACKED_MAX_KEYS = 287             # context keys (+ the null key = 288 slots) the packed key images of amdnuwa_xattn_decode hold


def long_context_ok(mod, n_keys):
    """Can a text cross-attention block `mod` (nuwa_pytorch.Attention) over a context of n_keys rows take the LONG form of the row program
    (long_context=True: the to_kv rows attended in place)?  Geometry alone -- what amdnuwa_attn_decode_rows / amdnuwa_attn_rows take, for
    contexts the packed images do not hold.  Unlike Attention._long_hip_ok it asks neither for a precision mode nor for a shape large
    enough to be the faster TRAINING route (long_pairs_min, long_wgs_min): one query row per sample never is."""
    return (not mod.causal) and n_keys is not None and n_keys > X_PACKED_MAX_KEYS and mod.heads <= 8 and mod.dim_head in (32, 64)


def _cast_row(x, lo):
    out = K.empty_bf(tuple(x.shape), x.device, lo=lo)
    K.cast_pad(x, out)
    return out


def _repeat_rows(o, R):
    """BF row [B, inner] -> the same row R times, sample-major [B * R, inner]: materialised, a writable copy also at R = 1"""
    return K.BF(*(None if t is None else t[:, None].repeat(1, R, 1).reshape(t.shape[0] * R, -1) for t in (o.hi, o.lo)))


def _row_program(dec, context, xm=None):
    """The row program of a decoder: ({stream: [block spec, ...]}, halves, combine); a single-stream decoder is stream 'v'.  A spec is the
    dict IncrementalDecoder's `block_list` takes: `mod`, `context`, `xm`, `dst`, `store_before` / `store_after`.
    Transformer: (attention, cross-attention, feed-forward) per layer, one residual.  ReversibleTransformer (np.py:1184-1295): (f, g) pairs,
    y1 = x1 + f(x2), y2 = x2 + g(y1), output = the SUM of the halves.  DualModalityDecoder (np.py:1299-1487) and
    ReversibleDualModalityDecoder (np.py:1489-1655 + reversible_video_audio.py; output = the mean of the halves): two streams, linked at
    the cross-modality layers through xm(module, context stream) -> _XmDirection."""
    from .nuwa_pytorch import ReversibleTransformer, ShiftVideoTokens, Transformer
    from .video_audio import DualModalityDecoder, ReversibleDualModalityDecoder
    v, a = [], []
    if isinstance(dec, Transformer):
        v += [dict(mod=sn, context=ctx_arg) for attn, cross, ff in dec.layers
              for sn, ctx_arg in ((attn, None), (cross, context), (ff, None)) if sn is not None]
        return {'v': v}, 1, 0.5                     # (one residual: nothing to combine)
    if isinstance(dec, ReversibleTransformer):
        for f, g in dec.layers:
            is_cross = not isinstance(f.fn, ShiftVideoTokens)
            v += [dict(mod=f, context=context if is_cross else None, dst=0), dict(mod=g, dst=1)]
        return {'v': v}, 2, 1.0
    if isinstance(dec, DualModalityDecoder):
        for blocks, kind in zip(dec.layers, dec.layer_types):
            if kind == 'intra_modality':
                for lst, (attn, cross, ff) in zip((v, a), blocks):
                    lst += [dict(mod=attn), dict(mod=cross, context=context), dict(mod=ff)]
            else:                               # both directions read the layer INPUT of the other stream (np.py:1467-1470)
                (v_x, v_ff), (a_x, a_ff) = blocks
                v_from_a, a_from_v = xm(v_x.fn, 'a'), xm(a_x.fn, 'v')
                v += [dict(mod=v_x, xm=v_from_a, store_before=(a_from_v,)), dict(mod=v_ff)]
                a += [dict(mod=a_x, xm=a_from_v, store_before=(v_from_a,)), dict(mod=a_ff)]
        return {'v': v, 'a': a}, 1, 0.5
    if isinstance(dec, ReversibleDualModalityDecoder):
        for (f, g, j, k), kind in zip(dec.layers, dec.layer_types):
            if kind == 'intra_modality_self_attn':
                v += [dict(mod=f, dst=0), dict(mod=g, dst=1)]
                a += [dict(mod=j, dst=0), dict(mod=k, dst=1)]
            elif kind == 'intra_modality_cross_attn':
                v += [dict(mod=f, context=context, dst=0), dict(mod=g, dst=1)]
                a += [dict(mod=j, context=context, dst=0), dict(mod=k, dst=1)]
            else:
                # un-normed modules; video: y1 = x1 + f(x2, ctx = audio m2), y2 = x2 + k(y1); audio: n1 = m1 + j(m2, ctx = the
                # UPDATED video half y2), n2 = m2 + g(n1) -- `k` / `g` crossed over as in reversible_video_audio.py:241-244
                v_from_a, a_from_v = xm(f, 'a'), xm(j, 'v')
                v += [dict(mod=f, xm=v_from_a, dst=0), dict(mod=k, dst=1, store_after=(a_from_v,))]
                a += [dict(mod=j, xm=a_from_v, dst=0, store_before=(v_from_a,)), dict(mod=g, dst=1)]
        return {'v': v, 'a': a}, 2, 0.5
    raise NotImplementedError(type(dec).__name__)


class IncrementalDecoder:
    """One decoder pass (conditioned or not) over a growing sequence.  transformer: nuwa_pytorch.Transformer or ReversibleTransformer
    whose blocks are all on the fused HIP path; context [B, T, D] fp32 and context_mask [B, T] bool as in Transformer.forward.

    Instead of `transformer`, `block_list` gives the row program explicitly (_row_program lays out all four decoders): dicts with `mod`
    (a SandwichNorm block, or a bare FeedForward / CrossModalityCrossAttention), optional `context` (text rows for a cross-attention), `xm`
    (_XmDirection this block attends through), `dst` (the residual half it adds into: reversible stacks keep two, np.py's reversible.py;
    the block reads the OTHER half), `store_before` / `store_after` (_XmDirection objects that take this row's input / output as context);
    `combine` scales the sum of the two halves at the end (1 for the ReversibleTransformer, 0.5 for the reversible dual decoder).

    long_context=True: a text cross-attention over more than 287 context keys (long_context_ok) becomes the long form of kind 'x' --
    to_kv(context) kept as rows [B, T, 2 * inner] and attended in place, one query by amdnuwa_attn_decode_rows (window start: a device-side
    zero, so the step stays capturable), R queries per sample by amdnuwa_attn_rows.  False (the default): such a context is refused and
    generate() keeps the recompute loop.  Contexts of at most 287 keys take the packed images whatever the switch says."""

    def __init__(self, transformer, batch, max_rows, context, context_mask, pos_dev, block_list=None, halves=1, combine=0.5, *,
                 long_context=False):
        from .nuwa_pytorch import Attention, FeedForward, Sparse3DNA, SandwichNorm, SparseCross2DNA
        from .video_audio import SparseCausal2DNA
        dev = context.device
        if block_list is None:
            lists, halves, combine = _row_program(transformer, context)
            block_list = lists['v']
        self.B, self.rows, self.pos_dev, self.halves, self.combine = batch, max_rows, pos_dev, halves, combine
        lo = self.lo = K.want_lo()
        D = context.shape[-1]
        ctx_bf = ops._ctx_to_bf(context)
        mask_u8 = context_mask.to(torch.uint8).contiguous() if context_mask is not None else None
        # the text-masked pass of classifier-free guidance: every query sees only the learned null key, so the attention
        # output is the same row for every position -- (sum_h W_th[g, h]) * null_v[g] -- and is computed once
        all_masked = context_mask is not None and not bool(context_mask.any())
        self.blocks = []
        for spec in block_list:
            mod, ctx_arg = spec['mod'], spec.get('context')
            blk = _Block()
            blk.kvcache = blk.geom = blk.pk = blk.xg = blk.o_const = blk.hcache = blk.fmap = blk.c2 = blk.wth = blk.rel = None
            blk.long, blk.ctx_kv, blk.first0, blk.mask_u8, blk.nk, blk.nv = False, None, None, None, None, None
            blk.xm = spec.get('xm')
            blk.dst = spec.get('dst', 0)
            blk.src = (1 - blk.dst) if halves == 2 else 0
            blk.store_before, blk.store_after = spec.get('store_before', ()), spec.get('store_after', ())
            if isinstance(mod, SandwichNorm):
                blk.pre = (mod.prenorm.weight.detach(), mod.prenorm.bias.detach())
                blk.post = (mod.postnorm.weight.detach(), mod.postnorm.bias.detach())
                if blk.xm is not None:
                    inner, fmap = mod.fn, None
                else:
                    found = mod._inner(ctx_arg, seq_len=max_rows, batch=batch)
                    if found is None and isinstance(mod.fn, SparseCausal2DNA) and mod.fn._hip_ok():
                        found = (mod.fn, None)                         # audio tower built without the channel shift
                    if found is None and long_context and ctx_arg is not None and isinstance(mod.fn, Attention) and \
                            long_context_ok(mod.fn, ctx_arg.shape[1]):
                        # _inner answers for the TRAINING route of a long context (speed thresholds, precision mode); a single row
                        # asks for the geometry alone
                        found = (mod.fn, None)
                    if found is None:
                        raise NotImplementedError('IncrementalDecoder: a decoder block is not on the libamdnuwa path')
                    inner, fmap = found
            else:                                                      # bare module: no norms, no shift
                blk.pre = blk.post = None
                inner, fmap = mod, None
                if not (blk.xm is not None or (isinstance(mod, FeedForward) and not mod._dropout_active())):
                    raise NotImplementedError(f'IncrementalDecoder: no single-row path for a bare {type(mod).__name__}')
            blk.inner, blk.fmap = inner, fmap
            blk.hcache = K.zeros_bf((batch, max_rows, D), dev, lo=lo) if fmap is not None else None
            if blk.xm is not None:
                blk.kind = 'xm'
            elif isinstance(inner, (SparseCausal2DNA, Sparse3DNA)):
                if isinstance(inner, SparseCausal2DNA):             # the audio window attention IS a 3DNA over a (time, 1, 1) grid
                    grid = ((max(max_rows - 1, 1), 1, 1), (inner.kernel_size[0], 1, 1), (inner.dilation[0], 1, 1))
                elif not inner.causal:
                    raise NotImplementedError('IncrementalDecoder needs causal Sparse3DNA')
                else:
                    grid = (inner.video_shape, inner.kernel_size, inner.dilation)
                if inner.heads > 8:
                    # the single-row kernels (csrc/decode.hip) stop at 8 heads: declined here, at construction -- whatever the other blocks
                    # of the stack are -- and not by a launch in mid-sampling
                    raise NotImplementedError(f'IncrementalDecoder: no single-row path for {type(inner).__name__} with {inner.heads} heads (up to 8)')
                blk.kind = 's3'
                blk.geom = K.s3_geom(batch, max_rows, *grid, inner.heads, inner.dim_head)
                blk.kvcache = K.zeros_bf((batch, max_rows, 2 * inner.heads * inner.dim_head), dev, lo=lo)
                p = inner._params()
                blk.wth = p[2].detach().reshape(inner.heads, inner.heads).contiguous()
                blk.rel = p[5].detach().contiguous() if len(p) > 5 else None
            elif isinstance(inner, Attention):
                if inner.causal:
                    # plain causal self-attention has no cached single-row path (it would need a device-side key count and rotary embeddings
                    # on top of amdnuwa_attn_decode_rows; no model's generate() builds such a stack): the recompute loop, whatever long_context says
                    raise NotImplementedError('IncrementalDecoder: no single-row path for plain (causal) self-attention')
                T = context.shape[1]
                blk.long = T > X_PACKED_MAX_KEYS
                if blk.long and not (long_context and long_context_ok(inner, T)):
                    # the packed key images of the single-query kernel (xattn_decode) hold at most 288 slots.  A longer context is attended in
                    # place (the long form below) when the caller asks for it with long_context=True and the geometry is the rows kernels';
                    # otherwise generate() keeps the recompute loop
                    raise NotImplementedError('IncrementalDecoder: no single-row path for cross-attention over more than 287 context keys')
                blk.kind = 'x'
                p = inner._params()
                W = ops.XInner.weights(inner._cache, p)
                hd, dh = inner.heads, inner.dim_head
                blk.wth = p[2].detach().reshape(hd, hd).contiguous()
                blk.nk, blk.nv = p[0].detach().reshape(hd, dh).contiguous(), p[1].detach().reshape(hd, dh).contiguous()
                kv = K.gemm_nt(ctx_bf, W['kv'], out_bf16=True)                 # text keys / values: once per sequence
                q0 = K.zeros_bf((batch, hd * dh), dev, lo=lo) if all_masked else None
                if blk.long:
                    # the rows to_kv(context) leaves ARE the layout the rows kernels read: no pack.  The window is the whole context, its
                    # first row a device-side zero -- the same buffers at every row, so the step replays from a captured graph
                    blk.ctx_kv = K.BF(kv.hi.reshape(batch, T, 2 * hd * dh), None if kv.lo is None else kv.lo.reshape(batch, T, 2 * hd * dh))
                    blk.first0 = torch.zeros(1, dtype=torch.int32, device=dev)
                    blk.mask_u8 = mask_u8
                    if all_masked:                                             # (mask_u8 is all zero here)
                        blk.o_const = self._attend_long(blk, q0, None)
                        blk.ctx_kv = None                                      # never read again: every later row is the constant
                else:
                    blk.xg = K.x_geom(batch, 1, T, hd, dh)
                    blk.pk = K.xattn_pack(blk.xg, kv, blk.nk, blk.nv, mask_u8)
                    if all_masked:
                        blk.o_const = K.xattn_decode(blk.xg, q0, blk.pk, blk.wth)
            elif isinstance(inner, SparseCross2DNA):
                blk.kind = 'xc2'
                blk.c2 = _Cross2DNARows(inner, batch, ctx_bf, mask_u8, all_masked, lo)
            elif isinstance(inner, FeedForward):
                blk.kind = 'ff'
            else:
                raise NotImplementedError(f'IncrementalDecoder: no single-row path for {type(inner).__name__}')
            self.blocks.append(blk)
        self.bos_row_differs = any(b.kind == 'xc2' for b in self.blocks)       # row 0 takes another code path: not one graph for all rows

    @staticmethod
    def _attend_long(blk, q, R):
        """the long form of an 'x' block: q BF [B, inner] (R None) or [B * R, inner] -> o alike; the context rows read in place"""
        inner = blk.inner
        T = blk.ctx_kv.hi.shape[1]
        if R is None:
            return K.attn_decode_rows(q, blk.ctx_kv, blk.first0, T, inner.heads, inner.dim_head, blk.nk, blk.nv, blk.wth,
                                      mask_u8=blk.mask_u8, scale=inner.scale)
        return K.attn_rows(q, blk.ctx_kv, blk.first0, T, R, inner.heads, inner.dim_head, blk.nk, blk.nv, blk.wth, mask_u8=blk.mask_u8,
                           scale=inner.scale)

    def _norm(self, y, resid, post, nxt, R):
        """-> (x, h).  x = resid + post-norm(y) (post None: none, x = y) and, in the same launch, h = the operand rows of block `nxt`: its
        pre-norm of x + its token shift through its cache (cache write + gather); h = None when `nxt` is None or un-normed.
        R None: the row at pos_dev (decode_ln); R: rows 0 .. R-1 of every sample, cache rows [0, R) written (prefill_ln)"""
        pre, cache, fmap = (nxt.pre, nxt.hcache, nxt.fmap or 0) if nxt is not None and nxt.pre is not None else (None, None, 0)
        if R is None:
            return K.decode_ln(y, resid, post, pre, cache=cache, pos_dev=self.pos_dev, fmap=fmap)
        return K.prefill_ln(y, resid, post, pre, R, cache=cache, fmap=fmap)

    def _enter(self, x, nxt, R):
        """the operand rows of block `nxt` from its fp32 input rows: pre-norm (+ token shift), or a plain cast for an un-normed block"""
        if nxt is None:
            return None
        return _cast_row(x, self.lo) if nxt.pre is None else self._norm(x, None, None, nxt, R)[1]

    def _walk(self, x, R=None, bos=False):
        """The one loop over the blocks.  R None: x fp32 [B, D], the row at pos_dev of every sample, single-row kernels against the caches
        (step).  R: x [B * R, D], sample-major rows 0 .. R-1 (prefill).  The modes differ in _norm and in the attention core of 's3', 'x'
        (long form: the rows form of its single-row kernel) and 'xc2' (its rows program, _Cross2DNARows.attend_rows); only the single row
        has 'xm' blocks and store hooks (prefill refuses them before it gets here)."""
        B, fast, blocks = self.B, ops._fast(), self.blocks
        state = [x] * self.halves
        h = self._enter(x, blocks[0], R)
        for i, blk in enumerate(blocks):
            inner = blk.inner
            for d in blk.store_before:
                d.store(state[blk.src], self.pos_dev)
            raw = blk.post is None                  # (an un-normed block adds its fp32 output itself)
            out16 = fast and not raw
            if blk.kind == 's3':
                p = inner._params()
                W = ops.S3Inner.weights(inner._cache, p)
                g = blk.geom
                qkv = K.gemm_nt(h, W['qkv'], out_bf16=True)
                if R is None:
                    o = K.s3_decode(g, qkv, blk.kvcache, self.pos_dev, blk.wth, blk.rel)
                else:
                    K.prefill_kv(qkv, blk.kvcache, R)
                    g = K.s3_geom(B, R, (g.F, g.H, g.W), (g.kf, g.kh, g.kw), (g.df, g.dh, g.dw), g.heads, g.dim_head)
                    o = K.sparse3dna_fwd(g, qkv, blk.wth, rel_bias=blk.rel)
                y = K.gemm_nt(o, W['out'], bias=p[4].detach(), out_bf16=out16)
            elif blk.kind == 'xm':
                y = blk.xm.attend(h)
            elif blk.kind == 'x':
                W = ops.XInner.weights(inner._cache, inner._params())
                g = blk.xg
                if blk.o_const is not None:         # the all-masked pass: the same row for every position
                    o = blk.o_const if R is None else _repeat_rows(blk.o_const, R)
                else:
                    q = K.gemm_nt(h, W['q'], out_bf16=True)
                    if blk.long:                    # more than 287 context keys: the to_kv rows in place, one query or R per sample
                        o = self._attend_long(blk, q, R)
                    elif R is None:
                        o = K.xattn_decode(g, q, blk.pk, blk.wth)
                    else:
                        # blk.pk was packed with an n = 1 geometry: the key images depend on (B, T, heads, dim_head) alone, so R queries attend them
                        o = K.xattn_fwd(K.x_geom(B, R, g.T, g.heads, g.dim_head), q, blk.pk, blk.wth, save=False)[0]
                y = K.gemm_nt(o, W['out'], out_bf16=out16)
            elif blk.kind == 'xc2':
                W = ops.XInner.weights(inner._cache, inner._params())
                o = blk.c2.attend(h, W, self.pos_dev, bos) if R is None else blk.c2.attend_rows(h, W, R)
                y = K.gemm_nt(o, W['out'], out_bf16=out16)
            else:
                W = ops.FFInner.weights(inner._cache, inner._params())
                u = K.gemm_nt(h, W['w1'], out_bf16=True)
                gg = K.geglu_fwd(u, W['FP'], interleaved=True)
                y = K.gemm_nt(gg, W['w2'], out_bf16=out16)
            nxt = blocks[i + 1] if i + 1 < len(blocks) else None
            if not raw:
                # post-norm + residual, the next block's pre-norm and its token shift (cache write + gather): one launch
                x, h = self._norm(y, state[blk.dst], blk.post, nxt, R)
                if nxt is not None and nxt.pre is None:
                    h = _cast_row(x, self.lo)
            else:
                x = state[blk.dst] + y
                h = self._enter(x, nxt, R)
            state[blk.dst] = x
            for d in blk.store_after:
                d.store(x, self.pos_dev)
        return x if self.halves == 1 else (state[0] + state[1]) * self.combine

    def step(self, x, bos=False):
        """x fp32 [B, D]: decoder input row `pos` of every sample -> that row after all layers (before the final norm).
        bos: this is row 0 (only a SparseCross2DNA block cares: its <bos> query attends to the whole context; the position itself
        lives in device memory and is not read on the host)"""
        return self._walk(x, None, bos)

    def prefill(self, x_rows):
        """x_rows fp32 [B, R, D]: the decoder input rows 0 .. R-1 of every sample -> those rows after all layers (before the final norm),
        [B, R, D]; rows [0, R) of every block's hcache / kvcache are left as R step() calls at pos = 0 .. R-1 would have left them.

        The mirror of step() over R rows: the same operand forms (the hi (+ lo) bf16 pair of K.want_lo(), never the fp16 forms of the
        training forward), the norms / shift / cache writes by the rows form of the single-row kernels (prefill_ln, prefill_kv) and the
        attention cores by the full-sequence kernels of the training path.  This is the pass NUWA.generate runs when its frame window
        slides: every kept token moves one frame earlier, so every hidden state and cached row changes.  The position counter is the
        caller's (GuidedStepper.prefill sets it to R)."""
        B, R, D = x_rows.shape
        if B != self.B or not 1 <= R <= self.rows:
            raise ValueError(f'IncrementalDecoder.prefill: {B} x {R} rows do not fit caches of {self.B} x {self.rows} rows')
        if any(b.kind == 'xm' or b.store_before or b.store_after or (b.kind == 'xc2' and getattr(b, 'c2', None) is None) for b in self.blocks):
            raise NotImplementedError('IncrementalDecoder.prefill: no full-sequence cache prefill for cross-modality blocks, store hooks '
                                      'or a SparseCross2DNA block without a rows program')
        return self._walk(x_rows.reshape(B * R, D).contiguous(), R).reshape(B, R, D)


XC2_PACKED_MAX_SLOTS = 287          # window slots (+ the null key = 288) the packed key images of amdnuwa_xattn_decode hold
XC2_DECODE_PACKED_DEFAULT = False   # the side windows of at most XC2_PACKED_MAX_SLOTS slots take when the switch below is not set


def xc2_decode_packed():
    """A/B switch AMDNUWA_XC2_DECODE_PACKED (1 / 0): SparseCross2DNA rows gather + pack their window and attend it with
    amdnuwa_xattn_decode, as before amdnuwa_cross2dna_decode existed, for windows the packed images hold; read when a row program is built"""
    return os.environ.get('AMDNUWA_XC2_DECODE_PACKED', '1' if XC2_DECODE_PACKED_DEFAULT else '0') == '1'


def cross2dna_slot_rows(nbr, frames):
    """nbr (tpf, k^2): the in-frame neighbour positions of every feature-map position, -1 = 'same' padding (SparseCross2DNA._nbr) ->
    int32 (tpf, frames * k^2): the context row of every window slot, slot order (frame, tap) as np.py:855, -1 kept for padding"""
    tpf = nbr.shape[0]
    return torch.cat([torch.where(nbr >= 0, nbr + a * tpf, nbr) for a in range(frames)], dim=1).to(torch.int32).contiguous()


class _Cross2DNARows:
    """SparseCross2DNA (np.py:761-901) for one new query row per sample (NUWASketch.generate, np.py:2440-2512).  The block is row-wise:
    query row pos (> 0) sits at feature-map position i = (pos - 1) mod fmap^2 and attends to the learned null key + the kernel^2
    neighbourhood of i in EVERY sketch frame.  to_kv(context) is computed once; per row amdnuwa_cross2dna_decode attends the window IN
    PLACE: it reads the slot table (context row of every slot of every position, -1 = padding) and the position on the device -- the step
    stays capturable in a HIP graph -- and takes any number of slots.  With AMDNUWA_XC2_DECODE_PACKED=1 a window of at most 287 slots
    takes the earlier path instead: gather the window's rows, pack them with amdnuwa_xattn_pack (padding slots and masked sketch tokens
    through its key mask), attend with amdnuwa_xattn_decode.  Row 0 (<bos>) attends to ALL context tokens without talking heads
    (np.py:826-849): B rows of glue arithmetic, as in the training path (ops.XC2Inner).  With every context token masked (the
    second pass of classifier-free guidance) both outputs are constants, computed once.

    attend_rows is the rows form for the cache prefill of a sliding window (IncrementalDecoder.prefill): rows 0 .. R-1 of every sample in
    one pass -- one to_q GEMM, the <bos> glue on rows b * R, amdnuwa_cross2dna_rows for the others."""

    def __init__(self, mod, batch, ctx_bf, mask_u8, all_masked, lo):
        dev = ctx_bf.hi.device
        self.mod, self.B, self.lo = mod, batch, lo
        h, dh = mod.heads, mod.dim_head
        self.inner = h * dh
        tpf = self.tpf = mod.image_size ** 2
        T = ctx_bf.hi.shape[0] // batch
        if T % tpf:
            raise NotImplementedError('cached decoding: the sketch context is not a whole number of frames')
        self.slot_rows = cross2dna_slot_rows(mod._nbr.to(dev), T // tpf)     # (tpf, fs * k^2) context rows of every window slot
        J = self.slot_rows.shape[1]
        self.packed = xc2_decode_packed() and J <= XC2_PACKED_MAX_SLOTS
        p = mod._params()
        self.nk, self.nv = p[0].detach().reshape(h, dh).contiguous(), p[1].detach().reshape(h, dh).contiguous()
        self.wth = p[2].detach().reshape(h, h).contiguous()
        self.mask_u8 = mask_u8 if mask_u8 is not None else torch.ones((batch, T), dtype=torch.uint8, device=dev)
        self.o_const = self.o_bos = self.kv = None
        if self.packed:
            self.win_idx = self.slot_rows.clamp(min=0).long()
            self.win_ok = (self.slot_rows >= 0).to(torch.uint8)              # 0 = the slot is 'same' padding
            self.xg = K.x_geom(batch, 1, J, h, dh)
        if all_masked:
            q0 = K.zeros_bf((batch, self.inner), dev, lo=lo)
            if self.packed:
                kv0 = K.zeros_bf((batch * J, 2 * self.inner), dev, lo=lo)
                pk = K.xattn_pack(self.xg, kv0, self.nk, self.nv, torch.zeros((batch, J), dtype=torch.uint8, device=dev))
                self.o_const = K.xattn_decode(self.xg, q0, pk, self.wth)
            else:                                                            # every row hidden: none is read
                self.o_const = K.cross2dna_decode(q0, K.zeros_bf((batch, T, 2 * self.inner), dev, lo=lo), self.slot_rows,
                                                  torch.ones(1, dtype=torch.int32, device=dev), h, dh, self.nk, self.nv, self.wth,
                                                  mask_u8=torch.zeros((batch, T), dtype=torch.uint8, device=dev), scale=mod.scale)
            self.o_bos = ops._to_bf(self.nv.float().reshape(1, self.inner).expand(batch, -1).contiguous())      # softmax over the null key alone
        else:
            W = ops.XInner.weights(mod._cache, p)
            kv = K.gemm_nt(ctx_bf, W['kv'], out_bf16=True)                   # sketch keys / values: once per sequence
            self.kv = K.BF(kv.hi.reshape(batch, T, 2 * self.inner), None if kv.lo is None else kv.lo.reshape(batch, T, 2 * self.inner))

    def _attend_bos(self, q):
        """q BF [B, inner]: the <bos> queries -> o BF [B, inner]: all context tokens, no talking heads (np.py:826-849), glue arithmetic"""
        B, inner, mod = self.B, self.inner, self.mod
        hd, dh = mod.heads, mod.dim_head
        q0 = ops._bf_val(q).reshape(B, hd, dh)
        kvf = ops._bf_val(self.kv).reshape(B, -1, 2, hd, dh)
        P0 = ops.XC2Inner._bos_scores(q0, kvf[:, :, 0], self.nk.float(), self.mask_u8.bool(), mod.scale)
        o0 = P0[..., :1] * self.nv.float()[None] + torch.einsum('bht,bthd->bhd', P0[..., 1:], kvf[:, :, 1])
        o = ops._to_bf(o0.reshape(B, inner).contiguous())
        return o if self.lo else K.BF(o.hi, None)

    def attend_rows(self, h, W, R):
        """The rows form (cache prefill): h BF [B * R, D], the pre-normed operand rows 0 .. R-1 of every sample, sample-major -> o BF
        [B * R, inner].  One to_q GEMM over all rows; rows b * R are the <bos> program of attend(bos=True), rows 1 .. R-1 of every sample
        ONE call of amdnuwa_cross2dna_rows, each bit-identical to the single-row kernel at pos = r.  The window is read in place whatever
        AMDNUWA_XC2_DECODE_PACKED says (self.kv exists on both routes).  On the text-masked guidance pass both outputs are constants:
        nothing is launched."""
        B, inner, mod = self.B, self.inner, self.mod
        first = lambda t: None if t is None else t.reshape(B, R, inner)[:, 0]
        if self.o_const is not None:
            o = _repeat_rows(self.o_const, R)                                      # (a copy also at R = 1: row 0 is overwritten below)
            first(o.hi)[:] = self.o_bos.hi
            if o.lo is not None:
                first(o.lo)[:] = self.o_bos.lo if self.o_bos.lo is not None else 0
            return o
        q = K.gemm_nt(h, W['q'], out_bf16=True)
        o = K.cross2dna_rows(q, self.kv, self.slot_rows, R, mod.heads, mod.dim_head, self.nk, self.nv, self.wth, mask_u8=self.mask_u8,
                             scale=mod.scale)
        o0 = self._attend_bos(K.BF(first(q.hi).contiguous(), None if q.lo is None else first(q.lo).contiguous()))
        first(o.hi).copy_(o0.hi)
        if o.lo is not None:
            first(o.lo).copy_(o0.lo)
        return o

    def attend(self, h, W, pos_dev, bos):
        """h BF [B, D] (pre-normed operand row) -> o BF [B, inner]"""
        if self.o_const is not None:
            return self.o_bos if bos else self.o_const
        q = K.gemm_nt(h, W['q'], out_bf16=True)
        B, inner, mod = self.B, self.inner, self.mod
        hd, dh = mod.heads, mod.dim_head
        if bos:
            return self._attend_bos(q)
        if not self.packed:
            return K.cross2dna_decode(q, self.kv, self.slot_rows, pos_dev, hd, dh, self.nk, self.nv, self.wth, mask_u8=self.mask_u8,
                                      scale=mod.scale)
        i = torch.remainder(pos_dev.long() - 1, self.tpf)                    # device-side feature-map position of this row
        idx = self.win_idx.index_select(0, i)[0]
        J = idx.shape[0]
        kvw = K.BF(self.kv.hi.index_select(1, idx).reshape(B * J, 2 * inner),
                   None if self.kv.lo is None else self.kv.lo.index_select(1, idx).reshape(B * J, 2 * inner))
        m = (self.mask_u8.index_select(1, idx) * self.win_ok.index_select(0, i)).contiguous()
        pk = K.xattn_pack(self.xg, kvw, self.nk, self.nv, m)
        return K.xattn_decode(self.xg, q, pk, self.wth)


class _XmDirection:
    """One direction of a cross-modality layer (CrossModalityCrossAttention `mod`, np.py:908-1067) for row-at-a-time decoding: the
    QUERY stream calls attend(), the CONTEXT stream calls store() with the rows `mod` would see as context.  Query row r (0 = start
    token) belongs to frame (r - 1) // chunk_size and attends a learned null key + context frame f of the sequence
    [context_chunk_size - 1 zero rows, the context stream's rows]: i.e. the other stream one frame EARLIER (frame 0: zero rows + its
    start token), complete by the time any query row of frame f exists.  The start-token row outputs 0.  The Conv3d talking heads
    carry a BIAS: it adds bias[g] * (null_v[g] + sum_j v_j[g]) to the head output, a per-frame constant kept as a correction row.

    A frame of more than 287 context rows (context_chunk_size + 1 > 288 slots: a token map of 17 x 17 or more) does not fit the packed
    key images of the short kernel: those rows are attended IN PLACE by amdnuwa_attn_decode_rows, which reads the window of self.kv that
    starts at the device-side row f * cc and takes the bias inside its mix -- no pack, no correction row."""

    def __init__(self, mod, batch, ctx_rows, dev, lo):
        from torch import nn
        if not (isinstance(mod.norm, nn.Identity) and isinstance(mod.context_norm, nn.Identity) and mod.has_start_token and
                mod.context_has_start_token and mod.dim_head in (32, 64) and mod.heads <= 8):
            raise NotImplementedError('cached decoding: this CrossModalityCrossAttention configuration is not on the libamdnuwa path')
        self.mod, self.B, self.lo = mod, batch, lo
        self.c, self.cc = mod.chunk_size, mod.context_chunk_size
        h, dh = mod.heads, mod.dim_head
        self.inner = h * dh
        self.nk, self.nv = mod.null_k.detach().reshape(h, dh).contiguous(), mod.null_v.detach().reshape(h, dh).contiguous()
        self.wth, self.th_bias = mod.talking_heads.weight.detach().reshape(h, h).contiguous(), mod.talking_heads.bias.detach().contiguous()
        # context rows under mod.to_kv: cc - 1 zero rows (to_kv has no bias), then context row r at cc - 1 + r, so that context
        # frame f is rows [f * cc, (f + 1) * cc)
        self.kv = K.zeros_bf((batch, self.cc - 1 + ctx_rows, 2 * self.inner), dev, lo=lo)
        # n_ctx / n_q: HOST row counters (advanced by the decoder that owns the streams, never inside a captured graph);
        # pk / corr: persistent buffers, re-packed in place at every frame border (a captured step keeps reading them);
        # first: the long form's window start f * cc, rewritten in place at every frame border for the same reason
        self.n_ctx, self.n_q, self.frame = 0, 0, -1
        self.long = self.cc + 1 > 288
        if self.long:
            self.first = torch.zeros(1, dtype=torch.int32, device=dev)
        else:
            self.g = K.x_geom(batch, 1, self.cc, mod.heads, mod.dim_head)
            self.pk = K.PackedKV(self.g, dev, lo)
            self.corr = torch.zeros((batch, mod.to_out.weight.shape[0]), dtype=torch.float32, device=dev)

    def _weights(self):
        m, h = self.mod, self.mod.heads
        p = (m.null_k.detach().reshape(h, 1, -1), m.null_v.detach().reshape(h, 1, -1), m.talking_heads.weight.detach().reshape(h, h, 1, 1),
             m.to_q.weight, m.to_kv.weight, m.to_out.weight)
        return ops.XInner.weights(m._cache, p)

    def store(self, x, pos_dev):
        """x fp32 [B, D]: the context stream's row `pos_dev` (its position counter, in device memory: the write is indexed on the device
        so that the step can be replayed from a captured graph)"""
        kv = K.gemm_nt(_cast_row(x, self.lo), self._weights()['kv'], out_bf16=True)
        at = (pos_dev + (self.cc - 1)).long()
        self.kv.hi.index_copy_(1, at, kv.hi[:, None])
        if self.kv.lo is not None:
            self.kv.lo.index_copy_(1, at, kv.lo[:, None])

    def _pack(self, f):
        m, cc = self.mod, self.cc
        if self.n_ctx < f * cc + 1:
            raise RuntimeError('cached decoding: the other stream has not produced the frame this row attends')
        if self.long:
            self.first.fill_(f * cc)
            self.frame = f
            return
        sl = slice(f * cc, (f + 1) * cc)
        kv = K.BF(self.kv.hi[:, sl].reshape(self.B * cc, 2 * self.inner).contiguous(),
                  self.kv.lo[:, sl].reshape(self.B * cc, 2 * self.inner).contiguous() if self.kv.lo is not None else None)
        h, dh = m.heads, m.dim_head
        K.xattn_pack(self.g, kv, self.nk, self.nv, None, out=self.pk)
        v = kv.hi[:, self.inner:].float()
        if kv.lo is not None:
            v = v + kv.lo[:, self.inner:].float()
        vsum = m.null_v.detach().reshape(1, h, dh) + v.reshape(self.B, cc, h, dh).sum(1)
        self.corr.copy_(F.linear((m.talking_heads.bias.detach()[None, :, None] * vsum).reshape(self.B, self.inner), m.to_out.weight.detach()))
        self.frame = f

    def needs_eager_row(self, r):
        """query row r cannot be replayed from the graph of an ordinary row: the start token (outputs 0) or the first row of a frame (packs, or moves the window)"""
        return r == 0 or (r - 1) // self.c != self.frame

    def attend(self, h):
        """h BF [B, D]: the operand row of query row n_q (pre-normed by the caller where the block has norms) -> fp32 [B, D]"""
        r, m = self.n_q, self.mod
        if r == 0:
            return torch.zeros((self.B, m.to_out.weight.shape[0]), dtype=torch.float32, device=h.hi.device)
        f = (r - 1) // self.c
        if f != self.frame:
            self._pack(f)
        W = self._weights()
        q = K.gemm_nt(h, W['q'], out_bf16=True)
        if self.long:
            o = K.attn_decode_rows(q, self.kv, self.first, self.cc, m.heads, m.dim_head, self.nk, self.nv, self.wth, th_bias=self.th_bias)
            return K.gemm_nt(o, W['out'], out_bf16=False)
        o = K.xattn_decode(self.g, q, self.pk, self.wth)
        return K.gemm_nt(o, W['out'], out_bf16=False) + self.corr


class DualIncrementalDecoder:
    """One pass (conditioned or text-masked) of the dual decoder -- DualModalityDecoder (np.py:1299-1487) or
    ReversibleDualModalityDecoder (np.py:1489-1655 + reversible_video_audio.py) -- over two growing sequences: step('v' | 'a', x)
    takes the decoder input row of the next position of that stream and returns the row after all layers (before the final norm)."""

    def __init__(self, dec, batch, rows_v, rows_a, context, context_mask, *, long_context=False):
        dev, lo = context.device, K.want_lo()
        self.pos = {'v': torch.zeros(1, dtype=torch.int32, device=dev), 'a': torch.zeros(1, dtype=torch.int32, device=dev)}
        rows = {'v': rows_v, 'a': rows_a}
        lists, halves, combine = _row_program(dec, context, lambda mod, ctx_stream: _XmDirection(mod, batch, rows[ctx_stream], dev, lo))
        self.streams = {key: IncrementalDecoder(None, batch, rows[key], context, context_mask, self.pos[key], block_list=lists[key],
                                                halves=halves, combine=combine, long_context=long_context) for key in 'va'}

    def directions(self, which):
        """(_XmDirection objects this stream QUERIES through, those it STORES context rows for)"""
        blocks = self.streams[which].blocks
        return [b.xm for b in blocks if b.xm is not None], [d for b in blocks for d in tuple(b.store_before) + tuple(b.store_after)]

    def needs_eager_row(self, which):
        return any(d.needs_eager_row(d.n_q) for d in self.directions(which)[0])

    def step(self, which, x, tick=True):
        """one row of stream `which`.  tick=False: the device work only (capturable in a HIP graph: no host-side state changes); the
        caller then calls tick() once per issued or replayed row"""
        out = self.streams[which].step(x.contiguous())
        self.pos[which] += 1
        if tick:
            self.tick(which)
        return out

    def tick(self, which):
        """host bookkeeping of the row step() has just been issued (or replayed) for"""
        q, st = self.directions(which)
        for d in q:
            d.n_q += 1
        for d in st:
            d.n_ctx += 1


class _CapturedStep:
    """step(body, checkpoint): `body` -- the device work of one row step, reading and writing persistent buffers only -- captured once in a
    HIP graph and replayed for every later call.  The first call warms up on a side stream (workspaces, weight caches, lazy module
    state), puts back what the warm-up moved and captures; the rows the warm-up wrote are rewritten by the real step at the same
    position.  checkpoint() is called before the warm-up and returns the function that rewinds it (device counters; buffers the body
    overwrites).  eager (graph switched off by the owner, or set here by a failed capture, which warns once): the body's kernels are
    launched one by one.  graph: the captured graph or None; the call returns the body's output (replayed: the static buffer the graph
    writes).  The callables are passed per call, not kept, so that the owner is not part of a reference cycle and its caches are freed
    with its last reference."""

    def __init__(self, what, eager=False):
        self.what, self.graph, self.out, self.eager = what, None, None, eager

    def __call__(self, body, checkpoint):
        if self.eager:
            return body()
        if self.graph is None:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                rewind = checkpoint()
                body()
                rewind()
            torch.cuda.current_stream().wait_stream(s)
            try:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):               # capture records, it does not execute: the replay below is the step itself
                    self.out = body()
                self.graph = g
            except RuntimeError as e:                   # same kernels, launched one by one
                import warnings
                warnings.warn(f'nuwa_pytorch_amd: HIP graph capture of the {self.what} failed ({e}); launching eagerly')
                self.eager = True
                torch.cuda.synchronize()
                return body()
        self.graph.replay()
        return self.out


class DualGuidedStepper:
    """The per-token work of NUWAVideoAudio.generate: advance(which, x_row) feeds the next input row of one stream and returns the
    logits for that stream's next token; with cond_scale != 1 the final-normed conditioned output row is the input of a second,
    text-masked pass (np.py:2176-2186) and the two logits are mixed."""

    def __init__(self, model, text_embeds, text_mask, rows_v, rows_a, cond_scale, graph=True, *, long_context=False):
        self.m, self.cond_scale = model, cond_scale
        dec = model.video_audio_transformer
        B, D = text_embeds.shape[0], text_embeds.shape[-1]
        self.cond = DualIncrementalDecoder(dec, B, rows_v, rows_a, text_embeds, text_mask, long_context=long_context)
        self.uncond = DualIncrementalDecoder(dec, B, rows_v, rows_a, text_embeds, torch.zeros_like(text_mask).bool(),
                                             long_context=long_context) if cond_scale != 1 else None
        # One captured HIP graph per stream for its ORDINARY rows (every row but a stream's start token and the first row of a frame,
        # where a cross-modality direction re-packs the other stream's frame on the host): static input / output buffers, positions
        # and context-row writes indexed on the device.
        self.x_in = {k: torch.zeros(B, D, dtype=torch.float32, device=text_embeds.device) for k in 'va'}
        self.captured = {k: _CapturedStep('dual decode step', eager=not graph) for k in 'va'}

    def _logits(self, which, hidden):
        m, dec = self.m, self.m.video_audio_transformer
        if which == 'v':
            nrm, lin, cache = dec.video_norm.norm, m.to_video_logits, m._cache_v
        else:
            nrm, lin, cache = dec.audio_norm.norm, m.to_audio_logits, m._cache_a
        return ops.LogitsFn.apply(hidden[:, None].contiguous(), nrm.weight, nrm.bias, lin.weight, cache)[:, 0]

    def _body(self, which):
        dec = self.m.video_audio_transformer
        hidden = self.cond.step(which, self.x_in[which], tick=False)
        logits = self._logits(which, hidden)
        if self.uncond is not None:
            nrm = dec.video_norm if which == 'v' else dec.audio_norm
            uh = self.uncond.step(which, nrm(hidden[:, None])[:, 0], tick=False)
            ul = self._logits(which, uh)
            logits = ul + (logits - ul) * self.cond_scale
        return logits

    def _tick(self, which):
        self.cond.tick(which)
        if self.uncond is not None:
            self.uncond.tick(which)

    def _checkpoint(self, which):
        """before a warm-up run of _body(which) -> the function that rewinds it: the stream's position in every pass"""
        def rewind():
            for d in (self.cond, self.uncond):
                if d is not None:
                    d.pos[which] -= 1
        return rewind

    def advance(self, which, x_row):
        self.x_in[which].copy_(x_row)
        eager = any(c.eager for c in self.captured.values()) or self.cond.needs_eager_row(which) or \
            (self.uncond is not None and self.uncond.needs_eager_row(which))
        if eager:
            logits = self._body(which)
        else:
            step = self.captured[which]
            logits = step(partial(self._body, which), partial(self._checkpoint, which))
            if step.graph is not None:                  # the graph's static output: the caller keeps a stream's logits across replays
                logits = logits.clone()
        self._tick(which)
        return logits


def position_schedule(tokens_per_frame, max_frames, total):
    """int32 [total] (host): entry t = the position-embedding row of the decoder input that FOLLOWS step t -- the window index of the token
    step t samples, slide_plan(t + 1)[0] - 1 (inside the window simply t)"""
    from .nuwa_pytorch import slide_plan
    return torch.tensor([slide_plan(t + 1, tokens_per_frame, max_frames)[0] - 1 for t in range(total)], dtype=torch.int32)


def kept_logits(filter_thres, num_classes):
    """how many of the largest logits sample_top_fraction keeps"""
    return max(int((1 - filter_thres) * num_classes), 1)


class GuidedStepper:
    """The per-token work of NUWA.generate (and NUWASketch.generate, np.py:2440-2512: same decoder, sketch context): conditioned pass -> logits; if cond_scale != 1 the reference feeds the final-normed
    conditioned OUTPUT row into a second, text-masked pass (np.py:1894-1898) and mixes the two logits.  One call = one new row.
    graph=True captures the step in a HIP graph after a warm-up call (static input / output buffers, device-side position).

    sampler = dict(total, tokens_per_frame, max_frames, filter_thres, temperature) adds the SAMPLING TAIL of the token to the step
    (amdnuwa_sample_next_row, the last launch of _body and so of the captured graph): it samples the token from the guided logits as
    nuwa_pytorch.sample_top_fraction does, writes it to column t of `ids` [B, total] and leaves the next decoder input row -- token
    embedding + position row pos_idx[t] -- in x_in; t is the device-side counter step_dev, advanced inside the graph like pos_dev.  The
    caller then drives the whole call with advance(): per token one draw of the uniforms `u` (none when one logit is kept) and one replay.
    A shape the kernel does not take leaves device_sampler False and the caller on the torch tail."""

    def __init__(self, nuwa, text_embeds, text_mask, max_rows, cond_scale, graph=True, sampler=None, *, long_context=False):
        dev = text_embeds.device
        B, D = text_embeds.shape[0], text_embeds.shape[-1]
        self.nuwa, self.cond_scale, self.max_rows = nuwa, cond_scale, max_rows
        self.pos_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        tr = nuwa.video_transformer
        self.cond = IncrementalDecoder(tr, B, max_rows, text_embeds, text_mask, self.pos_dev, long_context=long_context)
        self.uncond = None
        if cond_scale != 1:
            self.uncond = IncrementalDecoder(tr, B, max_rows, text_embeds, torch.zeros_like(text_mask).bool(), self.pos_dev,
                                             long_context=long_context)
        self.x_in = torch.zeros(B, D, dtype=torch.float32, device=dev)
        self._captured = _CapturedStep('decode step', eager=not graph)
        self._calls = 0
        self.device_sampler = False
        if sampler is not None:
            self._init_sampler(B, dev, **sampler)

    def _init_sampler(self, B, dev, total, tokens_per_frame, max_frames, filter_thres, temperature):
        nuwa = self.nuwa
        if not 0 < temperature < float('inf'):         # the kernel refuses it as an argument; the torch tail does what it always did
            return
        self.emb = nuwa.image_embedding.embed.weight.detach()
        self.pos_table = nuwa.video_pos_emb().detach().contiguous()
        C = nuwa.to_logits.weight.shape[0]
        self.keep, self.temperature = kept_logits(filter_thres, C), float(temperature)
        self.ids = torch.zeros((B, total), dtype=torch.int64, device=dev)
        self.u = torch.zeros((B, self.keep), dtype=torch.float32, device=dev) if self.keep > 1 else None
        self.pos_idx = position_schedule(tokens_per_frame, max_frames, total).to(dev)
        self.step_dev = torch.full((1,), -1, dtype=torch.int32, device=dev)
        # one launch at step -1 (out of range: nothing is written) asks the kernel whether it takes this shape
        probe = torch.zeros((B, C), dtype=torch.float32, device=dev)
        self.device_sampler = self.emb.shape[0] >= C and self.emb.is_contiguous() and self._sample(probe, allow_unsupported=True)
        self.step_dev.zero_()

    def _sample(self, logits, allow_unsupported=False):
        return K.sample_next_row(logits, self.keep, self.temperature, self.u, self.emb, self.pos_table, self.pos_idx, self.step_dev,
                                 self.ids, self.x_in, allow_unsupported=allow_unsupported)

    def _body(self, bos=False):
        nuwa = self.nuwa
        hidden = self.cond.step(self.x_in, bos)
        logits = nuwa._final(hidden[:, None])[:, 0]
        if self.uncond is not None:
            cond_out = nuwa.video_transformer.norm(hidden[:, None])[:, 0].contiguous()
            uh = self.uncond.step(cond_out, bos)
            ul = nuwa._final(uh[:, None])[:, 0]
            logits = ul + (logits - ul) * self.cond_scale
        self.pos_dev += 1
        if self.device_sampler:                        # the token and the next input row: x_in is read above, rewritten here
            self._sample(logits)
            self.step_dev += 1
        return logits

    def prefill(self, rows):
        """rows fp32 [B, R, D] = decoder input rows 0 .. R-1 of a (new) window: one full-sequence pass per decoder fills cache rows [0, R)
        (IncrementalDecoder.prefill; with guidance the text-masked pass is fed the conditioned pass's final-normed output, np.py:1894-1898)
        and the position becomes R -- the next call is row R.  Caches, x_in and pos_dev are persistent buffers, so a graph captured
        before the prefill keeps serving the rows after it.  Cache rows >= R keep the previous window's data: row r is written by the
        step at position r before any later step reads it (every stage looks back only)."""
        R = rows.shape[1]
        hidden = self.cond.prefill(rows)
        if self.uncond is not None:
            self.uncond.prefill(self.nuwa.video_transformer.norm(hidden).contiguous())
        self.pos_dev.fill_(R)                          # (outside any capture)
        self._calls += 1
        return hidden

    def __call__(self, x_row):
        """x_row fp32 [B, D] = decoder input row at the current position -> logits [B, C] for the next token"""
        self.x_in.copy_(x_row)
        return self._run()

    def advance(self, x_row=None):
        """device_sampler: one whole token -- the row step on x_in (x_row: the <bos> row of the first call; afterwards the row the step
        before left there), the sample into ids[:, t] and the next input row.  The uniforms are drawn here, outside the graph, from the
        default generator exactly as sample_top_fraction's torch.rand_like(vals) draws them (same shape, same dtype; the row step between
        the two draws nothing), so a seeded call samples what the torch tail samples"""
        if x_row is not None:
            self.x_in.copy_(x_row)
        if self.u is not None:
            self.u.uniform_()
        self._run()

    @property
    def graph(self):
        """the captured graph of the row step, or None (graph=False, not captured yet, or the capture failed)"""
        return self._captured.graph

    def _checkpoint(self):
        """before a warm-up run of _body -> the function that rewinds it: the position; with the device sampler the warm-up's tail has also
        replaced the input row and counted a token: both back (the id it wrote is rewritten by the real step, from the same uniforms)"""
        x_keep = self.x_in.clone() if self.device_sampler else None

        def rewind():
            self.pos_dev -= 1
            if self.device_sampler:
                self.x_in.copy_(x_keep)
                self.step_dev -= 1
        return rewind

    def _run(self):
        first = self._calls == 0
        self._calls += 1
        if first and self.cond.bos_row_differs:        # NUWASketch: the <bos> row of a SparseCross2DNA block is its own program --
            return self._body(True)                    # launched eagerly; the graph is captured at row 1 and serves every later row
        return self._captured(self._body, self._checkpoint)
