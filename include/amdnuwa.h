/*
 * libamdnuwa -- C-ABI of the MI355X (gfx950) NUWA video-decoder training hot path.
 *
 * The reference (lucidrains/nuwa-pytorch) has no FFI / operator registry: its boundary for this
 * path is the set of nn.Module classes in nuwa_pytorch/nuwa_pytorch.py (np.py) and
 * nuwa_pytorch/vqgan_vae.py (vq.py).  Each entry point below replaces the *body* of one of
 * those modules' forward (or its autograd backward) and cites the lines it replaces.  The
 * Python package `nuwa_pytorch_amd` keeps the module classes / signatures / state-dict keys
 * and calls these functions through ctypes (see INTEGRATION.md for the reference-side stub).
 *
 * Conventions
 *   - plain pointers to DEVICE memory + sizes + an explicit hipStream_t; nothing allocates,
 *     nothing synchronises, nothing throws; return 0 on success, <0 = AMDNUWA_ERR_*, >0 = hipError_t.
 *   - bf16 tensors are passed as uint16_t*; "hi/lo" pairs are the bf16 split of an fp32 value
 *     (value ~= hi + lo).  A NULL lo pointer selects the plain-bf16 operand path; non-NULL lo
 *     on both operands selects the 3-MFMA parity path (hi*hi + hi*lo + lo*hi).
 *   - activations are row-major [rows, features] with an explicit leading dimension in elements.
 *   - token rows of the video decoder: row = sample * ntok + i, i = 0 is <bos>, i = 1 + p is the
 *     token at raster position p = (f*H + y)*W + w.
 */
#ifndef AMDNUWA_H
#define AMDNUWA_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* amdnuwa_stream;   /* == hipStream_t */

int amdnuwa_abi_version(void);                 /* bumps when any signature or documented argument meaning below changes (13: tuning keys 0..31,
                                                * amdnuwa_xattn_unpack's flag bit 1, chunk-permuted dS / Pm columns of amdnuwa_xattn2_bwd;
                                                * 14: amdnuwa_linear_ce_x3 added; 15: the two-MFMA products -- amdnuwa_gemm_desc.ab_f16 with Blo, amdnuwa_gemm_nt_f16x2_supported,
                                                *     o_lo_f16 on the two fp16 forward cores; 16: the fp16-gradient backward; 17: amdnuwa_gemm_desc.a_chunk32, amdnuwa_gemm_tn_chunked_a_supported,
                                                *     amdnuwa_xattn2_bwd_ex, AMDNUWA_LN_RESID_MINUS, tuning key 25; 18: the amdnuwa_xattn6_* family; 19: amdnuwa_sparse3dna_bwd_f16, amdnuwa_xattn6_bwd_f16, amdnuwa_xattn6_pack_bwd_f16, o == NULL in the two fp16 forward cores,
                                                *     ab_f16 on the whole-M TN kernel with alpha_dev in its direct epilogue, c_f16 on the two-MFMA NT product;
                                                * 20: the amdnuwa_cattn_* family, 21: amdnuwa_cattn_geom.n_keys; ABI 21 also accepts token grids of up to 64 columns in the
                                                *     window kernels -- amdnuwa_s3_geom / amdnuwa_s3_supported below: a wider accepted range, no signature or struct change;
                                                *     amdnuwa_attn_decode_rows and its _workspace_bytes were added at 21 as well: purely additive; so were amdnuwa_prefill_ln and
                                                *     amdnuwa_prefill_kv, the cache prefill of a sliding generate() window, and amdnuwa_cross2dna_decode with its
                                                *     _workspace_bytes, the single-query SparseCross2DNA over a window of any size, and amdnuwa_sample_next_row, the
                                                *     sampling tail of a generate() token, and amdnuwa_vq_nearest_l2 with its _workspace_bytes, the Euclidean
                                                *     code lookup of the tokenizer, and amdnuwa_cross2dna_rows with its _workspace_bytes, the rows form of
                                                *     amdnuwa_cross2dna_decode for the cache prefill of NUWASketch.generate, and amdnuwa_attn_rows with its _workspace_bytes,
                                                *     the rows form of amdnuwa_attn_decode_rows for the cache prefill of a generate() over a long text context, and
                                                *     amdnuwa_cross2dna_fwd_drop / _bwd_drop with amdnuwa_cross2dna_drop_supported, attention dropout inside SparseCross2DNA) */
const char* amdnuwa_error_string(int code);
/* runtime tuning knobs (A/B benchmarking only; 0 = the library's auto policy everywhere):
 *   key 0  NT GEMM variant: 2 direct-to-LDS BK 32 (128x128 tiles), 5 register-staged 128x128, 7 the 256x256 ring family for every size,
 *          11 its K-step 64 form with staggered wave rows, 12 the four-wave long-K kernel for every K % 64 == 0
 *          (1, 3, 4, 6, 8, 9, 10: A/B variants of rounds 2-4, removed in round 6 -- 1 runs as 2, 10 as 5, the others as 7; hi + lo operands
 *          reach their 256x256 ring under 0 and 7 only and take the 128x128 kernel under every other value; fp16 operands are accepted under
 *          0, 7, 11, 6 and 10, the last two on the persistent or plain ring)
 *   key 1  TN split-K workgroup slots        key 2  TN minimum token rows per split
 *   key 3  Sparse3DNA forward: 1 = keep the VALU (dot2) kernel        key 13 hi + lo NT GEMM: 1 = first-generation 128x128 kernel
 *   key 4  Sparse3DNA backward: 1 = VALU kernels, 2 = MFMA query side + VALU key side, 4 = MFMA query side + RECOMPUTING MFMA key side
 *          (no ds / P' workspace: 1.5x instead of 2.85x the algorithmic HBM bytes, 15-22 % slower; 0 = MFMA kernels with the workspace)
 *   key 5  cross-attention forward: 1 = generic (not unrolled) kernel
 *   key 6  TN GEMM variant: 1 register-staged, 2 direct-to-LDS 128x128, 3 256x256 ring
 *   key 7  NT probe: bit 0 skips the epilogue stores, bit 1 skips the main loop (tools/gemm_probe.py; results are garbage)
 *   key 8  TN 256x256 ring: 2 = staggered wave rows instead of the lock-step schedule
 *   key 9  3DNA MFMA forward probe: bits 0 / 1 / 2 skip the score / softmax+mix / apply phase (garbage results), bit 3 = fragment-shaped
 *          key loads in the score pass instead of the staged ones
 *   key 14 NT start-phase step in ~0.25 us units (0 = off)        key 15 VAE kernels: 1 = first (VALU) forms, 2 = tiled vqattn
 *   key 16 Sparse3DNA MFMA forward: query rows per workgroup (0 = auto = 2 where H splits into dh * rows; 1 / 2 / 4 forced): a tile of rows
 *          of one residue class of y stages every key / value row once for the rows that tap it
 *   key 17 3DNA backward timing probes (garbage results): bit 0 no score sweeps, 1 no ds / P' workspace stores, 2 no dq apply sweep,
 *          3 no dW_th sums; key side: bit 4 no coefficient gathers, 5 no q / dO row fetch
 *   key 18 (unused since ABI 18: the cross-attention timing probes were run-time branches inside the chunk loops -- removed)
 *   key 19 3DNA MFMA query-side backward: 1 = the three separate item passes (P' mix, dW_th, dP mix) instead of the fused one
 *   key 20 NT 256x256 ring as a PERSISTENT kernel (one workgroup per CU walks the tile list, the DMA ring runs on across tile borders):
 *          0 = auto (more tiles than CUs and K <= 1024), 1 = never, 2 = always
 *   key 22 NT long-K kernel (four waves of 128x128, K-step 64, hand-placed main loop: gemm_nt_w4k_kernel): 0 = auto (K >= 1024 and K % 64 == 0),
 *          1 = never (8-wave ring), 2 = for every K % 32 == 0 from 96 up        key 23 TN four-wave kernel (gemm_tn_w4k_kernel): 1 = keep the 8-wave ring
 *   key 24 Sparse3DNA MFMA backward workspace: 0 = ONE array of (bf16 ds | bf16 P') words (round 5), 1 = the two fp32 arrays (same dK / dV bits)
 *   key 25 batched narrow TN (N <= 64, 128 < M <= 384: the cross attention's dK / dV): 1 = 128-row tiles instead of one workgroup per batch element,
 *          2 = always through the split-K reduction (no direct store of a one-split result), 3 = the general whole-M kernel also where the lean
 *          form applies (whole 32-row K-steps per split, plane offsets below 4 GiB: gemm_tn_wmf_kernel, bit-identical results)
 *   key 26 Sparse3DNA attention dropout (amdnuwa_sparse3dna_fwd_drop / _bwd_drop) at the geometry of the MFMA band kernels: 1 = keep the masked
 *          VALU window kernels there (0 = the masked band kernels, as the unmasked calls)
 * (keys run 0..31; the K-step 64 form of the 256x256 ring stages full 128-byte DMA lines in two 64 KiB stages, `auto` uses it for
 *  1024 <= K < 2048; any non-zero key 0 disables the few-row weight-streaming path that M <= 32 normally takes) */
int amdnuwa_set_tuning(int key, int value);
/* fp16 saturation monitor: number of threads (since the last reset) that handed a value beyond +-65504 to one of the library's saturating
 * COUNTED fp16 stores: the LayerNorm fp16 copies, the fp16-gradient epilogues (GEMM EPI 4 / 5, LayerNorm backward) and the fp16 copy of
 * the cross-attention output (amdnuwa_xattn6_fwd).  The forward GEMM epilogue copies (q / k / v, the FeedForward gate), the Sparse3DNA output
 * copy and amdnuwa_xattn2_fwd_f16 clamp to +-65504 as well but are NOT counted (one more live register there sends the persistent ring to
 * scratch): their inputs are LayerNorm outputs times weights inside the checked fp16 range.  0 in a healthy run: a saturated value is DEFINED
 * (clamped) but no longer the reference's arithmetic.  Synchronises the device; reset != 0 clears the counters. */
unsigned long long amdnuwa_f16_sat_count(int reset);
int amdnuwa_get_tuning(int key);

/* opt-in HIP-event launch timer: while armed, _begin/_end bracket one launch on `stream` with an
 * event pair; _collect synchronises and returns the summed kernel time and the launch count. */
void amdnuwa_timer_arm(int on);
int amdnuwa_timer_begin(amdnuwa_stream stream);
int amdnuwa_timer_end(amdnuwa_stream stream);
int amdnuwa_timer_collect(double* total_ms, long long* launches);
/* ABI 18: the same per launch -- ms[i] = duration of the i-th bracketed launch since the last collect (cap >= their number) */
int amdnuwa_timer_collect_each(double* ms, long long cap, long long* launches);

/* ------------------------------------------------------------------------------------------
 * GEMM (replaces every nn.Linear on the path: np.py:274-277 FeedForward, np.py:311-313 Attention,
 * np.py:401-405 Sparse3DNA, np.py:1819 to_logits; and their autograd backward)
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    const uint16_t* A; const uint16_t* Alo; long long strideA; int lda;
    const uint16_t* B; const uint16_t* Blo; long long strideB; int ldb;
    void* C; uint16_t* Clo; long long strideC; int ldc;
    int c_is_bf16;          /* 0: C is float*, 1: C (and optional Clo) are bf16 */
    const float* bias;      /* NT only, fp32 output only; may be NULL */
    float alpha, beta;      /* beta: TN only (C = beta*C + alpha*A^T B) */
    int M, N, K;
    int batch;              /* >=1; operand/result strides are per batch element */
    int shift_ntok;         /* >0: fold ShiftVideoTokens (np.py:185-253) into the loader of the */
    int shift_fmap;         /*     activation operand (A for NT, B for TN); ntok = rows per sample */
    int batch_inner;        /* >0: two-level batch: element z lives at (z / batch_inner) * stride +   */
    long long strideA_inner, strideB_inner, strideC_inner;   /*  (z % batch_inner) * stride_inner      */
    /* NT, bf16 C, batch <= 1: GEGLU gate (np.py:255-258) applied to the product.  C = u [M, N] is in the interleaved-by-8 layout
     * (see amdnuwa_geglu_il_fwd) and C2 [M, N/2] (bf16 hi[/lo], row pitch ldc2) = a * gelu_erf(gate); NULL = plain GEMM. */
    uint16_t* C2; uint16_t* C2lo; int ldc2;
    /* ... and its backward: with geglu_u != NULL the product is dgg = d(a * gelu(gate)) [M, N] and C2 [M, 2N] (pitch ldc2)
     * receives du = (dgg * gelu(gate) | dgg * a * gelu'(gate)) in the interleaved layout, computed from geglu_u [M, 2N]
     * (pitch ld_u, hi[/lo]).  When amdnuwa_gemm_nt_fused(d) != 0 this happens in the GEMM epilogue and C is NOT written;
     * otherwise C receives dgg and the stand-alone kernel follows. */
    const uint16_t* geglu_u; const uint16_t* geglu_u_lo; int ld_u;
    /* NT, bf16 C, hi + lo operands: with c_lo_f16 != 0 Clo receives the fp16 rendering of the FULL product value (not the bf16
     * residual) -- the operand form of the fp16 attention cores of the 'bf16x3-fwd' mode (amdnuwa_sparse3dna_fwd_f16,
     * amdnuwa_xattn2_fwd_f16): q / k / v leave the projection GEMM as a bf16 copy (for the bf16 backward) and an fp16 copy (for the
     * forward core).  Only the 256x256 hi + lo ring does this: ask amdnuwa_gemm_nt_f16_fused() first; otherwise run the plain
     * hi + lo product and amdnuwa_hilo_to_f16(). */
    int c_lo_f16;
    /* NT: ab_f16 != 0: A and B hold FP16 values (Alo / Blo / Clo must be NULL) and the product runs on the fp16 MFMA.  C: fp32, or
     * bf16 with the optional GEGLU output computed on the fp32 accumulators: C2 receives its FP16 copy (the next GEMM's A operand),
     * C2lo -- if not NULL -- its bf16 copy (the backward's operand).  Without C2, a non-NULL Clo receives the FP16 copy of the bf16
     * output itself (q / k / v: bf16 for the backward, fp16 for the forward attention core).  The FeedForward GEMMs (reference nuwa_pytorch.py:255-286) of
     * the 'bf16x3-fwd' forward.  256x256 ring only: amdnuwa_gemm_nt_f16ops_supported() first, AMDNUWA_ERR_UNSUPPORTED otherwise. */
    int ab_f16;
    /* ab_f16 with Blo != NULL: the TWO-MFMA form -- A = fp16 values (an activation rounded to 11 significand bits), B / Blo = an fp16
     * hi + lo pair with hi + lo = the fp32 weight to ~22 bits; per 32-chunk of k the products lo*a, hi*a accumulate in fp32.  C: fp32
     * (+ bias), or bf16 whose optional Clo receives the FP16 rendering of the output.  What the 'bf16x3-fwd' mode runs for to_out, the
     * cross-attention q / kv projections and to_logits (reference nuwa_pytorch.py:370-379, 611-613, 1956) when its two-MFMA switch is
     * on.  amdnuwa_gemm_nt_f16x2_supported() first; AMDNUWA_ERR_UNSUPPORTED otherwise. */
    /* Round 5 (ABI 16), the fp16-gradient backward.  NT with ab_f16 and c_is_bf16: c_f16 != 0 -> C (and the GEGLU-backward output C2) hold
     * FP16 values, saturating, instead of bf16 (Clo / C2lo NULL): dgrad products whose operands are fp16(S * gradient) and an fp16 weight.
     * The GEGLU backward (geglu_u) is available on the fp16-operand ring as well then (geglu_u stays bf16: it is read element-wise).
     * TN: ab_f16 != 0 -> A and B hold fp16 values (weight gradients from fp16 gradients and the fp16 activation copies).
     * alpha_dev (TN): optional DEVICE scalar multiplied into alpha by the split-K reduction (1 / S of the gradient scale). */
    int c_f16;
    const float* alpha_dev;
    /* ABI 17, TN only: a_chunk32 != 0 -> A is stored in planes of 32 columns, element (token row g, column c) at
     * A[(c / 32) * K * 32 + g * 32 + c % 32] (lda unused; batch strides as before).  The layout amdnuwa_xattn2_bwd_ex writes its dS / Pm in
     * with flag bit 0.  amdnuwa_gemm_tn_chunked_a_supported() first; AMDNUWA_ERR_UNSUPPORTED otherwise. */
    int a_chunk32;
} amdnuwa_gemm_desc;

/* C[M,N] = alpha * A[M,K] . B[N,K]^T (+ bias).  K, lda, ldb multiples of 8. */
int amdnuwa_gemm_nt(const amdnuwa_gemm_desc* d, amdnuwa_stream stream);
/* 1 when the C2 (GEGLU) output of this product is produced inside the GEMM epilogue, 0 when the library will run GEMM + gate kernel */
int amdnuwa_gemm_nt_fused(const amdnuwa_gemm_desc* d);
int amdnuwa_gemm_nt_f16ops_supported(const amdnuwa_gemm_desc* d);
int amdnuwa_gemm_nt_f16x2_supported(const amdnuwa_gemm_desc* d);
/* 1 when amdnuwa_gemm_nt() honours d->c_lo_f16 for this product (it returns AMDNUWA_ERR_UNSUPPORTED otherwise) */
int amdnuwa_gemm_nt_f16_fused(const amdnuwa_gemm_desc* d);
/* out[r][c] = fp16(hi[r][c] + lo[r][c]) over an [R, C] view (row pitches ld_in / ld_out elements, C % 8 == 0) */
int amdnuwa_hilo_to_f16(const uint16_t* hi, const uint16_t* lo, int ld_in, uint16_t* out, int ld_out, long long R, int C, amdnuwa_stream stream);
/* C[M,N] (fp32) = beta*C + alpha * A[K,M]^T . B[K,N]   (reduction over the K token rows, split-K
 * through `workspace`, fixed summation order => deterministic).  lda, ldb multiples of 8; operand rows
 * must be readable up to the next multiple of 8 columns (padding content is irrelevant). */
/* 1 when amdnuwa_gemm_tn() takes this product with ab_f16 != 0 (fp16 operands: the four-wave kernel's shapes -- no token shift, token rows
 * a multiple of 64, both output dimensions >= 256); it returns AMDNUWA_ERR_UNSUPPORTED otherwise */
int amdnuwa_gemm_tn_f16_supported(const amdnuwa_gemm_desc* d);
/* 1 when amdnuwa_gemm_tn takes this product with A in planes of 32 columns (a_chunk32): batched, N <= 64, 128 < M <= 384 (the whole-M kernel) */
int amdnuwa_gemm_tn_chunked_a_supported(const amdnuwa_gemm_desc* d);
size_t amdnuwa_gemm_tn_workspace_bytes(const amdnuwa_gemm_desc* d);
int amdnuwa_gemm_tn(const amdnuwa_gemm_desc* d, void* workspace, size_t workspace_bytes, amdnuwa_stream stream);

/* ------------------------------------------------------------------------------------------
 * Row kernels: LayerNorm of SandwichNorm (np.py:112-128) fused with the residual add of
 * Transformer.forward (np.py:1175-1180); StableLayerNorm (np.py:88-95); GEGLU (np.py:255-258);
 * Embedding/AxialPositionalEmbedding/<bos> assemble (np.py:1659-1709, 1940-1944);
 * F.cross_entropy (np.py:1963).  fp32 statistics, bf16 hi[/lo] outputs where a GEMM consumes them.
 * ---------------------------------------------------------------------------------------- */
/* mode 0: out_hi[/lo] = LN(x)*w+b (bf16).  mode 1: out_f32 = resid + LN(x)*w+b.
 * stable != 0 (mode 0 only): x is first divided by its row amax (saved as 1/amax).
 * Input-type flags (fast bf16 mode keeps GEMM outputs in bf16): OR AMDNUWA_LN_X_BF16 into `mode` (ln_fwd) or into
 * `stable` (ln_bwd) when x points at bf16 values; OR AMDNUWA_LN_DY_BF16 into ln_bwd's `stable` when dy does. */
/* Token shift folded into the pre-norm's store / the pre-norm backward's reads (shift_ntok = rows per sample, 0 = none):
 * shift_fmap > 0: ShiftVideoTokens (np.py:185-253) on a fmap x fmap grid, <bos> row untouched; shift_fmap == -1: ShiftAudioTokens
 * (np.py:157-183): the first half of the channels of row i comes from row i - 1 (zeros for row 0), every row takes part. */
#define AMDNUWA_LN_X_BF16 16
#define AMDNUWA_LN_DY_BF16 32
/* ln_fwd (mode 0) / ln_post_pre_fwd: the second 16-bit output (out_lo / h_lo) receives the FP16 rendering of the normalised row
 * instead of the bf16 residual -- the A operand of the fp16-operand GEMMs (amdnuwa_gemm_desc.ab_f16) */
#define AMDNUWA_LN_LO_F16 64
/* Round 5, fp16 everywhere a block needs ONE 16-bit copy.  AMDNUWA_LN_OUT_F16 -- in ln_fwd's `mode` / ln_post_pre_fwd's `flags`: out_hi /
 * h_hi itself receives the FP16 rendering (saturating; out_lo / h_lo must be NULL): the block's forward GEMM, its weight-gradient GEMM and
 * nothing else read it.  In ln_bwd_f16's `stable`: dx_hi receives fp16(S * dx) (dx_lo NULL).  AMDNUWA_LN_DY_F16 (ln_bwd_f16's `stable`):
 * dy points at fp16(S * value).  S travels as a DEVICE pointer scale2 = {S, 1 / S} (NULL = 1): a power of two chosen once per backward
 * pass by the host side from the residual-stream gradient, without a host synchronisation (nuwa_pytorch_amd/ops.py: _grad_scale). */
#define AMDNUWA_LN_OUT_F16 128
#define AMDNUWA_LN_DY_F16 256
/* ln_bwd_f16's `stable`: the fp32 dy is multiplied by the device scalar scale2[1] on the way in (the upstream gradient of the loss entering the
 * final norm's backward: no separate scaling pass over dy) */
#define AMDNUWA_LN_DY_SCALED 512
/* ln_fwd's `mode` (with bit 0, the post-norm form): out_f32 = resid - LN(x) instead of resid + LN(x): a reversible block's input recomputed from
 * its output (rev.py:77-106: x2 = y2 - g(y1), x1 = y1 - f(x2)) without negation passes over the stream */
#define AMDNUWA_LN_RESID_MINUS 1024
int amdnuwa_ln_fwd(const float* x, const float* resid, const float* w, const float* b, uint16_t* out_hi,
                   uint16_t* out_lo, float* out_f32, float* mean, float* rstd, float* inv_amax, long long R, int D,
                   int mode, int stable, float eps, int shift_ntok, int shift_fmap, amdnuwa_stream stream);
/* shift_ntok > 0 (mode 0): the bf16 output is written THROUGH the forward token shift of ShiftVideoTokens (np.py:210-253), i.e.
 * out = shift(LN(x)): rows are tokens of samples of shift_ntok rows (<bos> first), shift_fmap = tokens per grid row / column */
/* Post-norm + residual of one block fused with the pre-norm (+ token shift) of the NEXT block (Transformer.forward runs the
 * blocks back to back, np.py:1175-1180): out_f32 = resid + LN(y; w, b) with (mean, rstd) saved as mode 1 does, then
 * h = shift(LN(out_f32; next_w, next_b)) in bf16 hi[/lo] with (next_mean, next_rstd) saved as mode 0 does.
 * flags: AMDNUWA_LN_X_BF16 when y points at bf16 values. */
int amdnuwa_ln_post_pre_fwd(const float* y, const float* resid, const float* w, const float* b, float* out_f32,
                            float* mean, float* rstd, const float* next_w, const float* next_b, uint16_t* h_hi,
                            uint16_t* h_lo, float* next_mean, float* next_rstd, long long R, int D, int flags, float eps,
                            int shift_ntok, int shift_fmap, amdnuwa_stream stream);
/* Chained backward across a block boundary (the mirror of amdnuwa_ln_post_pre_fwd): the pre-norm backward of block k+1,
 *   dx = g + dLN(dh; x, mean, rstd, w)        (dh read through the inverse token shift when shift_ntok > 0; dw, db its weight grads)
 * and, on the same row while it is in registers, the post-norm backward of block k,
 *   dy_prev = dLN(dx; y_prev, mean_prev, rstd_prev, w_prev)   (bf16 hi[/lo]; dw_prev, db_prev; dsum_prev = column sums, optional).
 * inputs_bf16: 0 = dh and y_prev point at fp32 values, 1 = both at bf16 values (the all-bf16 mode), 2 = dh bf16 and y_prev fp32
 * (the 'bf16x3-fwd' mode: fp32 post-norm inputs from its 3-MFMA forward, bf16 dgrad outputs in its backward). */
size_t amdnuwa_ln_bwd_chain_workspace_bytes(long long R, int D);
int amdnuwa_ln_bwd_chain(const void* dh, const float* x, const float* mean, const float* rstd, const float* w, const float* g,
                         float* dx, float* dw, float* db, const void* y_prev, const float* mean_prev, const float* rstd_prev,
                         const float* w_prev, uint16_t* dy_prev_hi, uint16_t* dy_prev_lo, float* dw_prev, float* db_prev,
                         float* dsum_prev, long long R, int D, int shift_ntok, int shift_fmap, int inputs_bf16, void* workspace,
                         size_t workspace_bytes, amdnuwa_stream stream);
/* the same with fp16 gradients: inputs_bf16 = 3 -> dh points at fp16(S * value) (y_prev fp32); dy_prev_f16 != 0 -> dy_prev_hi receives
 * fp16(S * dy_prev), saturating (dy_prev_lo NULL).  inputs_bf16 0..2 / dy_prev_f16 = 0 / scale2 = NULL is amdnuwa_ln_bwd_chain. */
int amdnuwa_ln_bwd_chain_f16(const void* dh, const float* x, const float* mean, const float* rstd, const float* w, const float* g,
                             float* dx, float* dw, float* db, const void* y_prev, const float* mean_prev, const float* rstd_prev,
                             const float* w_prev, uint16_t* dy_prev_hi, uint16_t* dy_prev_lo, float* dw_prev, float* db_prev,
                             float* dsum_prev, long long R, int D, int shift_ntok, int shift_fmap, int inputs_bf16, int dy_prev_f16,
                             const float* scale2, void* workspace, size_t workspace_bytes, amdnuwa_stream stream);
size_t amdnuwa_ln_bwd_workspace_bytes(long long R, int D);
/* dy fp32; shift_ntok > 0 reads dy through the inverse token shift.  Exactly one of dx_hi (bf16
 * hi[/lo] output) / dx_acc (fp32) is non-NULL; dx_acc = (dres ? dres : dx_acc) + dx.  dw, db, dsum
 * (= column sums of dx) may be NULL; accumulate != 0 adds into them. */
int amdnuwa_ln_bwd(const float* dy, const float* x, const float* mean, const float* rstd, const float* inv_amax,
                   const float* w, uint16_t* dx_hi, uint16_t* dx_lo, float* dx_acc, const float* dres, float* dw,
                   float* db, float* dsum, long long R, int D, int shift_ntok, int shift_fmap, int stable, int accumulate, void* workspace,
                   size_t workspace_bytes, amdnuwa_stream stream);
/* amdnuwa_ln_bwd with the fp16-gradient flags of `stable` (AMDNUWA_LN_DY_F16, AMDNUWA_LN_OUT_F16) and the device scale pair */
int amdnuwa_ln_bwd_f16(const float* dy, const float* x, const float* mean, const float* rstd, const float* inv_amax,
                       const float* w, uint16_t* dx_hi, uint16_t* dx_lo, float* dx_acc, const float* dres, float* dw,
                       float* db, float* dsum, long long R, int D, int shift_ntok, int shift_fmap, int stable, int accumulate,
                       const float* scale2, void* workspace, size_t workspace_bytes, amdnuwa_stream stream);
size_t amdnuwa_colsum_workspace_bytes(long long R, int D);
int amdnuwa_colsum(const float* x, float* out, long long R, int D, int accumulate, void* workspace,
                   size_t workspace_bytes, amdnuwa_stream stream);
/* u = [a | g], each FP columns wide: o = a * gelu_erf(g) */
int amdnuwa_geglu_fwd(const uint16_t* u_hi, const uint16_t* u_lo, uint16_t* o_hi, uint16_t* o_lo, long long R, int FP,
                      amdnuwa_stream stream);
/* the same on the interleaved-by-8 layout of u: columns [16 q, 16 q + 8) hold a_{8q..8q+7}, [16 q + 8, 16 q + 16) their gates
 * (FP % 8 == 0).  The FF1 weight rows are permuted accordingly, so a lane of the GEMM epilogue holds a value and its gate. */
int amdnuwa_geglu_il_fwd(const uint16_t* u_hi, const uint16_t* u_lo, uint16_t* o_hi, uint16_t* o_lo, long long R, int FP,
                         amdnuwa_stream stream);
int amdnuwa_geglu_il_bwd(const uint16_t* u_hi, const uint16_t* u_lo, const uint16_t* d_hi, const uint16_t* d_lo,
                         uint16_t* du_hi, uint16_t* du_lo, long long R, int FP, amdnuwa_stream stream);
int amdnuwa_geglu_bwd(const uint16_t* u_hi, const uint16_t* u_lo, const uint16_t* d_hi, const uint16_t* d_lo,
                      uint16_t* du_hi, uint16_t* du_lo, long long R, int FP, amdnuwa_stream stream);
/* FeedForward dropout (np.py:276: nn.Dropout on the GEGLU output, between the two products), csrc/dropout.hip.
 * out = keep ? in * scale : 0 over an [R, C] view.  keep: one byte per element (non-zero = kept; a torch.bool tensor) with its own
 * row pitch ld_keep (bytes); scale = 1 / (1 - p), finite and >= 1.  Two forms:
 *   in_f16 != 0: `in` holds fp16 values; out_f16 (required, may be `in` itself) receives the fp16 copy -- saturating at +-65504,
 *                NaN kept -- and `out` the bf16 copy, both rounded from the same fp32 product; in_lo and out_lo must be NULL;
 *   in_f16 == 0: `in` (+ in_lo, optional) is a bf16 hi[/lo] pair, `out` (+ out_lo, optional) receives the hi[/lo] split of
 *                amdnuwa_cast_pad; out_f16 must be NULL.
 * C % 8 == 0; every row pitch (elements; ld_keep in bytes) >= C and a multiple of 8; the 16-bit tensors 16-byte aligned, keep 8-byte
 * aligned (16-byte accesses of the tensors, 8 mask bytes next to them).  A dropped element is exactly +0 whatever its input. */
int amdnuwa_geglu_dropout_fwd(const uint16_t* in, const uint16_t* in_lo, int ld_in, int in_f16, const uint8_t* keep, int ld_keep,
                              float scale, uint16_t* out, uint16_t* out_lo, int ld_out, uint16_t* out_f16, int ld_f16,
                              long long R, int C, amdnuwa_stream stream);
/* amdnuwa_geglu_il_bwd with that mask folded in: d_hi[/d_lo] is the UNDROPPED gradient dgg [R, FP] of the dropout's output; the kernel
 * forms dgd = round(keep ? dgg * scale : 0) in registers -- rounded to bf16 hi, or to the hi + lo pair when the lo parts are given, the
 * form a separate mask pass would have stored -- and writes du from u (interleaved-by-8) and dgd.  u_lo, d_lo and du_lo: all or none.
 * FP % 8 == 0; ld_keep (bytes) >= FP and a multiple of 8. */
int amdnuwa_geglu_il_bwd_dropout(const uint16_t* u_hi, const uint16_t* u_lo, const uint16_t* d_hi, const uint16_t* d_lo,
                                 const uint8_t* keep, int ld_keep, float scale, uint16_t* du_hi, uint16_t* du_lo,
                                 long long R, int FP, amdnuwa_stream stream);
/* Dropout keep masks from a counter-based generator, in a kernel of their own (csrc/keepmask.hip; added at ABI 21, purely additive).
 * They serve every nn.Dropout the library runs on masked kernels -- reference nuwa_pytorch.py:276 (FeedForward), :554-564 and :746-752
 * (Sparse3DNA, SparseCausal2DNA), :888-892 (SparseCross2DNA) and :370-374 (Attention) -- and write the layouts those kernels read today.
 *
 * THE DECISION FUNCTION.  Philox4x32-10 with the standard constants: multipliers 0xD2511F53 (on counter word 0) and 0xCD9E8D57 (on word 2),
 * Weyl key increments 0x9E3779B9 and 0xBB67AE85, ten rounds, the key bumped between rounds; key = (seed word 0, seed word 1), the low 32
 * bits of the two 64-bit words `seed` points to on the device.  For the logical element e (64-bit):
 *     word = output word (e mod 4) of Philox(counter = (floor(e / 4) mod 2^32, floor(e / 4) >> 32, 0, 0), key);   keep  <=>  word >= thr
 * with thr = min(2^32 - 1, round(p * 2^32)), computed by the caller in ONE place (kernels.keep_threshold); the kept values are scaled by
 * drop_scale = 1 / (1 - p) as before.  Known answers (counter; key -> output words in order):
 *     0 0 0 0; 0 0 -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8        ffffffff x 4; ffffffff x 2 -> 408f276d 41c83b0e a20bc7c6 6d5451fd
 *     243f6a88 85a308d3 13198a2e 03707344; a4093822 299f31d0 -> d16cfe09 94fdcceb 5001e420 24126ea1
 * Logical elements:
 *     FeedForward mask [R, C]                       e = r * C + c
 *     window / SparseCross2DNA mask [B, nq, J, heads]   e = ((b * nq + i) * J + j) * heads + g         (the storage index)
 *     cattn                                         e = ((b * n + i) * (T + 1) + j) * 8 + g, j = 0 the null slot, always 8 head lanes
 * The decision depends on (seed, e) alone: not on the launch, the output's alignment, or how a caller splits a batch (e0 / b_first).  A
 * later in-kernel generator has to reproduce exactly this function.  The kernels READ the seed: the host never synchronises.
 *
 * amdnuwa_keep_mask_linear: keep[i] = 1 if element e0 + i is kept, else 0, for i < count; any count > 0, any alignment of keep (16-byte
 * stores between a byte-wise head and tail).
 * amdnuwa_keep_mask_cattn: the three arrays of amdnuwa_cattn_fwd_drop / _bwd_drop for samples b_first .. b_first + B - 1 (b above = b_first +
 * the array's sample index): keep [B][n][KP], keep_t [B][T][NP] (the same bytes transposed), keep0 [B][n]; KP / NP = T / n rounded up to 32;
 * bit g = head g kept; every padding byte and every bit at or above `heads` zero.  keep and keep_t are both written in 16-byte pieces of
 * contiguous rows (one 64 x 64 tile transposed through LDS), keep / keep_t bases 4-byte aligned.
 * NULL arrays or seed, heads outside 1 .. 8, non-positive sizes, a negative e0 / b_first, a misaligned keep / keep_t (cattn) or seed:
 * AMDNUWA_ERR_ARG before anything is launched. */
int amdnuwa_keep_mask_linear(uint8_t* keep, long long count, long long e0, uint32_t thr, const uint64_t* seed, amdnuwa_stream stream);
int amdnuwa_keep_mask_cattn(uint8_t* keep, uint8_t* keep_t, uint8_t* keep0, int B, int n, int T, int heads, long long b_first,
                            uint32_t thr, const uint64_t* seed, amdnuwa_stream stream);
/* dst[r][c<C] = bf16(src[r][c]), zero for C <= c < Cp */
int amdnuwa_cast_pad(const float* src, int ld_src, uint16_t* hi, uint16_t* lo, int ld_dst, long long R, int C, int Cp,
                     amdnuwa_stream stream);
/* dst[c][r] = bf16(src[r][c]) */
int amdnuwa_transpose_cast(const float* src, int ld_src, uint16_t* hi, uint16_t* lo, int ld_dst, int R, int C,
                           amdnuwa_stream stream);
int amdnuwa_embed_fwd(const long long* ids, const float* W, const float* ax1, const float* ax2, const float* ax3,
                      const float* bos, float* x, int B, int ntok, int D, int H, int Wd, float frac,
                      amdnuwa_stream stream);
size_t amdnuwa_embed_bwd_workspace_bytes(int ntok, int D);
/* sorted_ids / perm (both [B*(ntok-1)], optional): the token ids stably sorted and their original flat positions -> the
 * token-embedding gradient is summed in a fixed order (deterministic); NULL selects fp32 atomics */
int amdnuwa_embed_bwd(const long long* ids, const long long* sorted_ids, const long long* perm, const float* dx, float* dW,
                      float* dax1, float* dax2, float* dax3, float* dbos, int B, int ntok, int D, int F, int H, int Wd,
                      float frac, void* workspace, size_t workspace_bytes, amdnuwa_stream stream);
/* row_loss[r] = lse(logits[r]) - logits[r][t]; *loss = mean(row_loss);
 * dl (optional, bf16 hi[/lo], ld = ld_dl) = (softmax - onehot) * grad_scale */
int amdnuwa_ce_fwd(const float* logits, const long long* targets, float* row_loss, float* loss, uint16_t* dl_hi,
                   uint16_t* dl_lo, long long R, int C, int ld_dl, float grad_scale, amdnuwa_stream stream);
int amdnuwa_scale_by_device_scalar(float* x, size_t n, const float* scalar, amdnuwa_stream stream);
/* Fused to_logits + cross entropy (np.py:1958 `self.to_logits(...)` feeding np.py:1963 `F.cross_entropy`) WITHOUT the fp32 logits in
 * memory: logits = h[R,K] . w[C,K]^T (bf16 operands, fp32 accumulate) are produced twice inside the 256x256 MFMA ring -- pass 1 keeps
 * per-(row, 64-column block) (max, sum exp) and the target logit, pass 2 writes dlogits = (softmax - onehot) * grad_scale as bf16
 * [R, ld_dl] (skipped when dlogits is NULL).  row_loss[r] = lse - logit[target]; *loss = mean (fixed order).  A target outside
 * [0, C) makes its row loss (and the mean) NaN.  Needs C % 64 == 0, K % 32 == 0 (else AMDNUWA_ERR_UNSUPPORTED: use gemm_nt + ce_fwd). */
size_t amdnuwa_linear_ce_workspace_bytes(long long R, int C);
int amdnuwa_linear_ce(const uint16_t* h, int ldh, const uint16_t* w, int ldw, const long long* targets, long long R, int C, int K,
                      float grad_scale, float* row_loss, float* loss, uint16_t* dlogits, int ld_dl, void* workspace,
                      size_t workspace_bytes, amdnuwa_stream stream);
/* The same with both operands as bf16 hi + lo pairs: the to_logits of the 'bf16x3-fwd' mode, whose logits (and so the loss) must stay
 * inside the 1e-3 bound while its backward takes a plain bf16 dlogits.  Pass 1 (statistics, lse, loss) runs three MFMAs per product
 * on the hi + lo ring.  Pass 2 (dlogits): with h_f16 / w_f16 (fp16 renderings of the same operands, same leading dimensions; both or
 * neither) ONE fp16 MFMA per product against the exact lse of pass 1 -- the error of an fp16 product sits below the bf16 rounding of
 * dlogits itself; with both NULL the hi + lo ring again.  Same workspace, same outputs as amdnuwa_linear_ce. */
int amdnuwa_linear_ce_x3(const uint16_t* h_hi, const uint16_t* h_lo, const uint16_t* h_f16, int ldh, const uint16_t* w_hi,
                         const uint16_t* w_lo, const uint16_t* w_f16, int ldw, const long long* targets, long long R, int C, int K,
                         float grad_scale, float* row_loss, float* loss, uint16_t* dlogits, int ld_dl, void* workspace,
                         size_t workspace_bytes, amdnuwa_stream stream);

/* ------------------------------------------------------------------------------------------
 * Sparse3DNA core (np.py:488-608, incl. the unfoldNd gather np.py:526-534): causal (or symmetric) 3-D nearby
 * attention with <bos> key/value, fp32 softmax and talking heads.  q/k/v/o are token-row major
 * [B*ntok, ld] with head h in columns [h*dim_head, (h+1)*dim_head); q is UNSCALED.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    int B, ntok;            /* ntok = 1 (<bos>) + number of video tokens present (<= F*H*W) */
    int F, H, W;            /* token grid (max_frames, fmap, fmap) */
    int kf, kh, kw;         /* kernel size */
    int df, dh, dw;         /* dilation */
    int heads, dim_head;    /* heads 1..8 (9..16: the amdnuwa_sparse3dna_mh_* entries); dim_head in {32, 64}; W*heads*4 <= 512 (one workgroup per grid row) or W <= 64 (column tiles) */
    float scale;            /* dim_head ** -0.5 */
    /* relative-position bias (Sparse3DNA(rel_pos_bias=True), np.py:512-516, 542): rel_bias[j][head] is added to the score of
     * key slot j (j = 0 is <bos>: pass 0 there), fp32 [kf*kh*kw + 1][heads] or NULL.  The backward writes its gradient
     * (column sums of ds over every query) to d_rel_bias when that is non-NULL. */
    const float* rel_bias;
    float* d_rel_bias;
    /* 0: causal window -- every tap at or before the query on each axis (Sparse3DNA(causal=True), np.py:427);
     * 1: symmetric 'same' window, tap t of an axis at offset (t - (k-1)/2) * dilation (causal=False, np.py:429: the sketch
     *    encoder of NUWASketch).  Row 0 stays the <bos> key/value; taps that leave the grid are masked, taps inside the grid but
     *    past the end of the sequence read the reference's zero padding (score 0, value 0). */
    int noncausal;
} amdnuwa_s3_geom;

/* 1 when the window kernels (amdnuwa_sparse3dna_*, amdnuwa_cross2dna_*) take this geometry in the given operand form
 * (lo_operands != 0: bf16 hi + lo pairs): head size 32 / 64, 1..8 heads, W * heads * 4 <= 512 or W <= 64, and the window's LDS tables (they grow with
 * J = kf*kh*kw + 1 key slots: Sparse3DNA / SparseCross2DNA kernel sizes, reference nuwa_pytorch.py:382-394, 761-790) within the
 * CU's 160 KiB for the forward AND both backward kernels.  A row with W * heads * 4 <= 512 is one workgroup; a wider one is cut
 * into NT = ceil(W / floor(128 / heads)) column tiles of TW = ceil(W / NT) queries, and the tables are those of ONE tile: TW
 * queries, TW + (kw-1)*dw staged columns (the halo the kw taps reach, in the causal and the symmetric window alike).  The entry
 * points themselves return AMDNUWA_ERR_UNSUPPORTED exactly for the geometries this query rejects. */
int amdnuwa_s3_supported(const amdnuwa_s3_geom* g, int lo_operands);
int amdnuwa_sparse3dna_fwd(const amdnuwa_s3_geom* g, const uint16_t* q, const uint16_t* k, const uint16_t* v,
                           const uint16_t* q_lo, const uint16_t* k_lo, const uint16_t* v_lo, int ld,
                           const float* w_th, uint16_t* o, uint16_t* o_lo, int ldo, amdnuwa_stream stream);
/* the forward core on SINGLE fp16 MFMAs (the MFMA band kernel with fp16 operands): q / k / v hold fp16 values (the second copy
 * amdnuwa_gemm_nt writes with c_lo_f16), o leaves as a bf16 hi + lo pair (o_lo may be NULL).  Geometry of the band kernels only
 * (causal window, 16-wide grid, 8 heads x 64, kw <= 3): amdnuwa_s3_f16_supported() says whether it applies.  The forward
 * Sparse3DNA core (reference nuwa_pytorch.py:488-608) of the 'bf16x3-fwd' mode. */
int amdnuwa_s3_f16_supported(const amdnuwa_s3_geom* g);
/* o_lo_f16 != 0: o_lo receives the FP16 rendering of the output instead of the bf16 residual -- the A operand of the two-MFMA to_out
 * product (amdnuwa_gemm_desc.ab_f16 with Blo); o stays the bf16 copy the backward reads. */
int amdnuwa_sparse3dna_fwd_f16(const amdnuwa_s3_geom* g, const uint16_t* q_f16, const uint16_t* k_f16, const uint16_t* v_f16, int ld,
                               const float* w_th, uint16_t* o, uint16_t* o_lo, int ldo, int o_lo_f16, amdnuwa_stream stream);
size_t amdnuwa_sparse3dna_bwd_workspace_bytes(const amdnuwa_s3_geom* g);
int amdnuwa_sparse3dna_bwd(const amdnuwa_s3_geom* g, const uint16_t* q, const uint16_t* k, const uint16_t* v,
                           const uint16_t* q_lo, const uint16_t* k_lo, const uint16_t* v_lo, int ld,
                           const float* w_th, const uint16_t* dO, const uint16_t* dO_lo, int lddo, uint16_t* dq,
                           uint16_t* dk, uint16_t* dv, uint16_t* dq_lo, uint16_t* dk_lo, uint16_t* dv_lo, int ldd,
                           float* dw_th, int accumulate, void* workspace, size_t workspace_bytes,
                           amdnuwa_stream stream);
/* ABI 19, the fp16-gradient form of the backward (reference nuwa_pytorch.py:488-608 differentiated; block class 's' of the 'bf16x3-fwd' mode):
 * q / k / v are the fp16 arrays the fp16 forward read -- the block then keeps ONE 16-bit copy of them --, dO_f16 = fp16(S dO), and dq / dk / dv
 * leave as fp16(S gradient), saturating and counted by amdnuwa_f16_sat_count; dw_th leaves as fp32 WITHOUT the factor.  scale2 = device
 * pointer to {S, 1 / S} (S a power of two, see amdnuwa_gemm_desc.alpha_dev).  Same workspace as amdnuwa_sparse3dna_bwd.  Band-kernel
 * geometry without a relative-position bias only: amdnuwa_sparse3dna_bwd_f16_supported(), AMDNUWA_ERR_UNSUPPORTED otherwise.
 * amdnuwa_sparse3dna_fwd_f16 accepts o == NULL together with o_lo_f16 (the fp16 copy is then the only output). */
int amdnuwa_sparse3dna_bwd_f16_supported(const amdnuwa_s3_geom* g);
int amdnuwa_sparse3dna_bwd_f16(const amdnuwa_s3_geom* g, const uint16_t* q_f16, const uint16_t* k_f16, const uint16_t* v_f16, int ld,
                               const float* w_th, const uint16_t* dO_f16, int lddo, uint16_t* dq_f16, uint16_t* dk_f16, uint16_t* dv_f16,
                               int ldd, float* dw_th, int accumulate, const float* scale2, void* workspace, size_t workspace_bytes,
                               amdnuwa_stream stream);
/* Many-head form of the causal window (additive, ABI unchanged): 9 .. 16 heads on VALU kernels of their own (csrc/sparse3dna_mh.hip),
 * every geometry in column tiles of at most floor(128 / heads) columns.  Argument lists, operand forms (bf16, or hi + lo pairs when the
 * lo pointers are given), workspace layout, return codes and their order are those of amdnuwa_sparse3dna_fwd / _bwd, rel_bias /
 * d_rel_bias of the geometry included.  Envelope: heads 9 .. 16, dim_head 32 / 64, causal only (g->noncausal == 0), W <= 64, and the
 * tile's LDS tables within the CU's 160 KiB: amdnuwa_s3mh_supported() says whether it applies, the entries answer
 * AMDNUWA_ERR_UNSUPPORTED outside it -- for heads <= 8 too, which amdnuwa_sparse3dna_fwd / _bwd serve.  No fp16 operand form, no
 * fp16-gradient form, no masked (attention dropout) form, no SparseCross2DNA form, no cached decoding. */
int amdnuwa_s3mh_supported(const amdnuwa_s3_geom* g, int lo_operands);
size_t amdnuwa_sparse3dna_mh_bwd_workspace_bytes(const amdnuwa_s3_geom* g);
int amdnuwa_sparse3dna_mh_fwd(const amdnuwa_s3_geom* g, const uint16_t* q, const uint16_t* k, const uint16_t* v,
                              const uint16_t* q_lo, const uint16_t* k_lo, const uint16_t* v_lo, int ld,
                              const float* w_th, uint16_t* o, uint16_t* o_lo, int ldo, amdnuwa_stream stream);
int amdnuwa_sparse3dna_mh_bwd(const amdnuwa_s3_geom* g, const uint16_t* q, const uint16_t* k, const uint16_t* v,
                              const uint16_t* q_lo, const uint16_t* k_lo, const uint16_t* v_lo, int ld,
                              const float* w_th, const uint16_t* dO, const uint16_t* dO_lo, int lddo, uint16_t* dq,
                              uint16_t* dk, uint16_t* dv, uint16_t* dq_lo, uint16_t* dk_lo, uint16_t* dv_lo, int ldd,
                              float* dw_th, int accumulate, void* workspace, size_t workspace_bytes,
                              amdnuwa_stream stream);
/* Attention dropout inside the causal window (the `self.dropout(attn)` of reference nuwa_pytorch.py:554-564, Sparse3DNA, and 746-752,
 * SparseCausal2DNA as a (time, 1, 1) grid; additive at ABI 21).  With P = softmax over the J slots and P' = W_th . P, the V product and dV take
 * P'' = keep . P' . drop_scale, and the backward takes dP' = keep . (dO . V^T) . drop_scale; everything below dP' is amdnuwa_sparse3dna_bwd's.
 * keep: uint8 [B][ntok - 1][J][heads], the index order of the ds / P' workspace, nonzero = keep (the caller draws it; the same array goes to the
 * forward and to the backward); drop_scale = 1 / (1 - p), finite and >= 1.  Slots hidden by the causal padding ignore the mask; the <bos>
 * query row still outputs its own value row.  An all-ones mask with drop_scale = 1 gives the bits of amdnuwa_sparse3dna_fwd / _bwd, at every
 * geometry: a masked call runs the masked form of the kernel the unmasked call picks under exactly the same conditions -- the MFMA band kernels
 * (16-wide grid, 8 heads x 64, kw <= 3, bf16 operands; also with a relative-position bias and d_rel_bias, which put the backward on the fp32
 * workspace) and the VALU window kernels (row and column-tiled, bf16 and hi + lo operands) everywhere else.  Tuning key 26 = 1 keeps the VALU
 * kernels at band geometry (A/B runs).  The recomputing key side (tuning key 4 = 4) rebuilds P' from statistics and knows no mask: a masked call
 * takes the workspace key side whatever that key says.  Every geometry amdnuwa_s3_supported() takes, causal only (g->noncausal:
 * AMDNUWA_ERR_UNSUPPORTED) -- amdnuwa_s3_drop_supported().  keep == NULL or a drop_scale that is not finite or < 1: AMDNUWA_ERR_ARG; the band
 * kernels read the 8 mask bytes of a (query, slot) as one word, so at band geometry a keep that is not 8-byte aligned is AMDNUWA_ERR_ARG too.
 * The backward uses the workspace of amdnuwa_sparse3dna_bwd_workspace_bytes(). */
int amdnuwa_s3_drop_supported(const amdnuwa_s3_geom* g, int lo_operands);
int amdnuwa_sparse3dna_fwd_drop(const amdnuwa_s3_geom* g, const uint16_t* q, const uint16_t* k, const uint16_t* v,
                                const uint16_t* q_lo, const uint16_t* k_lo, const uint16_t* v_lo, int ld,
                                const float* w_th, uint16_t* o, uint16_t* o_lo, int ldo, const uint8_t* keep, float drop_scale,
                                amdnuwa_stream stream);
int amdnuwa_sparse3dna_bwd_drop(const amdnuwa_s3_geom* g, const uint16_t* q, const uint16_t* k, const uint16_t* v,
                                const uint16_t* q_lo, const uint16_t* k_lo, const uint16_t* v_lo, int ld,
                                const float* w_th, const uint16_t* dO, const uint16_t* dO_lo, int lddo, uint16_t* dq,
                                uint16_t* dk, uint16_t* dv, uint16_t* dq_lo, uint16_t* dk_lo, uint16_t* dv_lo, int ldd,
                                float* dw_th, int accumulate, void* workspace, size_t workspace_bytes, const uint8_t* keep,
                                float drop_scale, amdnuwa_stream stream);
/* The same mask in the fp16 operand forms (additive at ABI 21): the arguments of amdnuwa_sparse3dna_fwd_f16 / amdnuwa_sparse3dna_bwd_f16 plus keep
 * and drop_scale, with the meaning above (keep 8-byte aligned).  Geometry of amdnuwa_s3_f16_supported() / amdnuwa_sparse3dna_bwd_f16_supported(),
 * AMDNUWA_ERR_UNSUPPORTED otherwise; keep == NULL or a drop_scale that is not finite or < 1: AMDNUWA_ERR_ARG, before the device is touched.  All
 * three output forms of the forward (o + o_lo, o + fp16 o_lo, fp16 o_lo alone).  In the backward the 0 / 1 of the mask is applied before dP'
 * leaves for fp16 and drop_scale in fp32 behind it, so the fp16 range of dP' (|S dO| . 2^-6) and the saturation counter are those of the unmasked
 * call.  An all-ones mask with drop_scale = 1 gives the bits of the unmasked calls. */
int amdnuwa_sparse3dna_fwd_f16_drop(const amdnuwa_s3_geom* g, const uint16_t* q_f16, const uint16_t* k_f16, const uint16_t* v_f16, int ld,
                                    const float* w_th, uint16_t* o, uint16_t* o_lo, int ldo, int o_lo_f16, const uint8_t* keep,
                                    float drop_scale, amdnuwa_stream stream);
int amdnuwa_sparse3dna_bwd_f16_drop(const amdnuwa_s3_geom* g, const uint16_t* q_f16, const uint16_t* k_f16, const uint16_t* v_f16, int ld,
                                    const float* w_th, const uint16_t* dO_f16, int lddo, uint16_t* dq_f16, uint16_t* dk_f16, uint16_t* dv_f16,
                                    int ldd, float* dw_th, int accumulate, const float* scale2, void* workspace, size_t workspace_bytes,
                                    const uint8_t* keep, float drop_scale, amdnuwa_stream stream);

/* SparseCross2DNA (np.py:761-901): NUWASketch's decoder cross-attention.  Queries = the video rows q [B*ntok, ldq] (row 0 of every
 * sample is <bos>); keys / values = the sketch context k, v [B*ctx_rows, ldkv], ctx_rows = g->kf * H * W (g->kf = sketch frames).
 * Query (f, y, x) attends to the learned null key / value (key slot 0; null_k / null_v: bf16 [heads*dim_head]) and, in EVERY context
 * frame a, to the g->kh x g->kw neighbourhood of (y, x) with dilation (g->dh, g->dw) and 'same' zero padding -- slot
 * 1 + (a*kh + b)*kw + c; key_mask [B][ctx_rows] (1 = visible, NULL = all) masks slots; fp32 softmax; talking heads w_th [heads][heads].
 * g->df, g->noncausal and g->rel_bias are ignored (rel_bias must be NULL).  Row 0 of every sample (the <bos> query attends to ALL
 * context tokens, without talking heads: np.py:813-830) is NOT read or written here: the caller owns o / dq rows b*ntok.
 * Backward: dq rows 1.., dk / dv [B*ctx_rows, lddkv], d_null_k / d_null_v fp32 [heads*dim_head], dw_th fp32 [heads*heads]. */
int amdnuwa_cross2dna_fwd(const amdnuwa_s3_geom* g, const uint16_t* q, const uint16_t* q_lo, int ldq, int ctx_rows,
                          const uint16_t* k, const uint16_t* v, const uint16_t* k_lo, const uint16_t* v_lo, int ldkv,
                          const uint16_t* null_k, const uint16_t* null_k_lo, const uint16_t* null_v, const uint16_t* null_v_lo,
                          const uint8_t* key_mask, const float* w_th, uint16_t* o, uint16_t* o_lo, int ldo, amdnuwa_stream stream);
size_t amdnuwa_cross2dna_bwd_workspace_bytes(const amdnuwa_s3_geom* g);
int amdnuwa_cross2dna_bwd(const amdnuwa_s3_geom* g, const uint16_t* q, const uint16_t* q_lo, int ldq, int ctx_rows,
                          const uint16_t* k, const uint16_t* v, const uint16_t* k_lo, const uint16_t* v_lo, int ldkv,
                          const uint16_t* null_k, const uint16_t* null_k_lo, const uint16_t* null_v, const uint16_t* null_v_lo,
                          const uint8_t* key_mask, const float* w_th, const uint16_t* dO, const uint16_t* dO_lo, int lddo,
                          uint16_t* dq, uint16_t* dq_lo, int lddq, uint16_t* dk, uint16_t* dv, uint16_t* dk_lo, uint16_t* dv_lo,
                          int lddkv, float* d_null_k, float* d_null_v, float* dw_th, void* workspace, size_t workspace_bytes,
                          amdnuwa_stream stream);
/* Attention dropout inside SparseCross2DNA (the `self.dropout(attn)` of reference nuwa_pytorch.py:888-892, behind the talking-heads mix of
 * the windowed queries; additive at ABI 21).  With P = softmax over the J = kf*kh*kw + 1 slots and P' = W_th . P, the V product and dV take
 * P'' = keep . P' . drop_scale and the backward takes dP' = keep . (dO . V^T) . drop_scale; everything below dP' -- dq, dk / dv over the
 * context, d_null_k, d_null_v, dw_th -- is amdnuwa_cross2dna_bwd's.  keep: uint8 [B][ntok - 1][J][heads], the index order of the ds / P'
 * workspace, nonzero = keep (the caller draws it; the same array goes to the forward and to the backward); drop_scale = 1 / (1 - p), finite
 * and >= 1.  The arguments are those of amdnuwa_cross2dna_fwd / _bwd with keep and drop_scale in front of the stream, the checks and their
 * order are theirs, and keep == NULL or a drop_scale that is not finite or < 1 is AMDNUWA_ERR_ARG (behind the geometry and UNSUPPORTED
 * answers, in front of the workspace one, at B = 0 as well).  The mask has no alignment rule: the cross route runs the masked forms of the
 * VALU window kernels (row and column-tiled, bf16 and hi + lo operands) and never a band kernel.  Slots hidden by key_mask or by the 'same'
 * padding have P = 0 and ignore the mask; the <bos> query row (nuwa_pytorch.py:826-844: no dropout, no talking heads) stays the caller's and has no
 * row in keep.  An all-ones mask with drop_scale = 1 gives the bits of amdnuwa_cross2dna_fwd / _bwd.  amdnuwa_cross2dna_drop_supported()
 * answers as amdnuwa_s3_supported() (g->noncausal is ignored, as in the entries); the backward uses the workspace of
 * amdnuwa_cross2dna_bwd_workspace_bytes(). */
int amdnuwa_cross2dna_drop_supported(const amdnuwa_s3_geom* g, int lo_operands);
int amdnuwa_cross2dna_fwd_drop(const amdnuwa_s3_geom* g, const uint16_t* q, const uint16_t* q_lo, int ldq, int ctx_rows,
                               const uint16_t* k, const uint16_t* v, const uint16_t* k_lo, const uint16_t* v_lo, int ldkv,
                               const uint16_t* null_k, const uint16_t* null_k_lo, const uint16_t* null_v, const uint16_t* null_v_lo,
                               const uint8_t* key_mask, const float* w_th, uint16_t* o, uint16_t* o_lo, int ldo, const uint8_t* keep,
                               float drop_scale, amdnuwa_stream stream);
int amdnuwa_cross2dna_bwd_drop(const amdnuwa_s3_geom* g, const uint16_t* q, const uint16_t* q_lo, int ldq, int ctx_rows,
                               const uint16_t* k, const uint16_t* v, const uint16_t* k_lo, const uint16_t* v_lo, int ldkv,
                               const uint16_t* null_k, const uint16_t* null_k_lo, const uint16_t* null_v, const uint16_t* null_v_lo,
                               const uint8_t* key_mask, const float* w_th, const uint16_t* dO, const uint16_t* dO_lo, int lddo,
                               uint16_t* dq, uint16_t* dq_lo, int lddq, uint16_t* dk, uint16_t* dv, uint16_t* dk_lo, uint16_t* dv_lo,
                               int lddkv, float* d_null_k, float* d_null_v, float* dw_th, void* workspace, size_t workspace_bytes,
                               const uint8_t* keep, float drop_scale, amdnuwa_stream stream);

/* ------------------------------------------------------------------------------------------
 * Incremental decoding for NUWA.generate (np.py:1841-1915).  The reference recomputes the whole prefix for every sampled
 * token; every decoder stage is causal, so row `pos` only needs cached rows < pos.  `pos` (row index inside each sample,
 * 0 = <bos>) is read from DEVICE memory so one captured HIP graph serves every token.
 * ---------------------------------------------------------------------------------------- */
/* ShiftVideoTokens (np.py:210-253) for the single new row: h [B, D] (bf16 hi[/lo]) is stored as row pos of
 * cache [B, cache_rows, D] and out [B, D] = shift(h)[pos] (first channel quarter from row pos - fmap, second from pos - 1,
 * zero at the frame border; <bos> unchanged). */
int amdnuwa_decode_shift(const uint16_t* h_hi, const uint16_t* h_lo, uint16_t* cache_hi, uint16_t* cache_lo,
                         uint16_t* out_hi, uint16_t* out_lo, const int* pos, int B, int cache_rows, int D, int fmap,
                         amdnuwa_stream stream);
/* The norms around a block for the one new row per sample, in one launch (SandwichNorm, np.py:112-128, + the residual add of
 * Transformer.forward, np.py:1175-1180):  x_new = resid + LN(y; w, b)  [skipped when resid == NULL: x_new = y, fp32];
 * h = LN(x_new; next_w, next_b)  [skipped when next_w == NULL];  with cache_hi != NULL h also becomes row pos of
 * cache [B, cache_rows, D] and out = shift(h)[pos] as amdnuwa_decode_shift does, else out = h.  y: fp32 or (y_is_bf16) bf16.
 * fmap = -1 selects ShiftAudioTokens (np.py:157-183): the first half of the channels comes from row pos - 1 (<bos> included). */
int amdnuwa_decode_ln(const void* y, int y_is_bf16, const float* resid, const float* w, const float* b, const float* next_w,
                      const float* next_b, float* x_new, uint16_t* cache_hi, uint16_t* cache_lo, uint16_t* out_hi,
                      uint16_t* out_lo, const int* pos, int B, int cache_rows, int D, int fmap, float eps,
                      amdnuwa_stream stream);
/* Sparse3DNA core (np.py:488-608) for the single new query: qkv [B, 3*inner] (q | k | v of row pos, q unscaled); its k | v
 * join kv_cache [B, cache_rows, 2*inner]; o [B, inner] = attention over <bos> + the causal taps read from the cache
 * (g->rel_bias as in amdnuwa_sparse3dna_fwd; g->ntok is ignored). */
int amdnuwa_s3_decode(const amdnuwa_s3_geom* g, const uint16_t* qkv, const uint16_t* qkv_lo, uint16_t* kv_cache,
                      uint16_t* kv_cache_lo, int cache_rows, const int* pos, const float* w_th, uint16_t* o,
                      uint16_t* o_lo, amdnuwa_stream stream);
/* Cache prefill (added at ABI 21, purely additive): what R successive single-row calls at pos = 0 .. R-1 leave behind, for R rows per
 * sample at once -- the pass NUWA.generate runs when its frame window slides (np.py:1873-1881): every kept token moves one frame earlier,
 * so every cached row changes.  Rows are sample-major: row = sample * R + i.
 * amdnuwa_prefill_ln is amdnuwa_decode_ln without `pos`: y / resid / x_new / out are [B*R, D]; with cache_hi != NULL exactly rows [0, R) of
 * cache [B, cache_rows, D] (R <= cache_rows) become h and out = shift(h) (fmap as in amdnuwa_decode_ln), else out = h.  Per row the arithmetic
 * and its order are those of amdnuwa_decode_ln: x_new, the cache rows and out are BIT-IDENTICAL to the R single-row calls.  The shift of row i
 * reads the h of rows i - 1 and i - fmap, which other workgroups write: the entry point runs two stream-ordered launches (norms + cache
 * write, then the gather); no atomics, two runs are bit-identical.  AMDNUWA_ERR_ARG: a null or non-positive argument, R > cache_rows;
 * AMDNUWA_ERR_UNSUPPORTED: D % 16 != 0 or D > 4096. */
int amdnuwa_prefill_ln(const void* y, int y_is_bf16, const float* resid, const float* w, const float* b, const float* next_w,
                       const float* next_b, float* x_new, uint16_t* cache_hi, uint16_t* cache_lo, uint16_t* out_hi,
                       uint16_t* out_lo, int B, int R, int cache_rows, int D, int fmap, float eps, amdnuwa_stream stream);
/* amdnuwa_prefill_kv copies the k | v columns of qkv [B*R, 3*inner] (bf16 hi, lo image optional: NULL on both sides or on neither) into
 * rows [0, R) of kv_cache [B, cache_rows, 2*inner], the layout amdnuwa_s3_decode keeps; 16-byte vectors, inner % 8 == 0
 * (AMDNUWA_ERR_UNSUPPORTED otherwise).  AMDNUWA_ERR_ARG: a null or non-positive argument, R > cache_rows. */
int amdnuwa_prefill_kv(const uint16_t* qkv, const uint16_t* qkv_lo, uint16_t* kv_cache, uint16_t* kv_cache_lo, int B, int R,
                       int cache_rows, int inner, amdnuwa_stream stream);

/* ------------------------------------------------------------------------------------------
 * Text cross-attention core (Attention.forward with context, np.py:339-378): learned null key/value
 * at key slot 0, context key mask, fp32 softmax, talking heads, attn @ v.  q/o are token-row major
 * [B*n, ld]; keys/values are packed per (sample, head) by amdnuwa_xattn_pack.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
    int B, n, T;            /* queries per sample, context length */
    int JP;                 /* amdnuwa_xattn_jp(T): T+1 rounded up to a multiple of 32 (<= 288) */
    int heads, dim_head;    /* heads <= 8, dim_head in {32, 64} */
    float scale;
} amdnuwa_xattn_geom;

typedef struct {            /* all [B][heads][JP][dim_head] (Kp, Vp) or [B][heads][dim_head][JP] (Kt, Vt), bf16 */
    uint16_t *Kp, *Kp_lo, *Kt, *Kt_lo, *Vp, *Vp_lo, *Vt, *Vt_lo;
    uint8_t* valid;         /* [B][JP] */
} amdnuwa_xattn_kv;

int amdnuwa_xattn_jp(int T);
/* kv: [B*T, ldkv] bf16, keys in columns [0, inner), values in [inner, 2*inner) (= to_kv(context)); ldkv % 8 == 0 and 16-byte
 * aligned bases (the kernels move 16-byte pieces), AMDNUWA_ERR_ARG otherwise -- the same holds for amdnuwa_xattn_unpack */
int amdnuwa_xattn_pack(const amdnuwa_xattn_geom* g, const uint16_t* kv, const uint16_t* kv_lo, int ldkv,
                       const float* null_k, const float* null_v, const uint8_t* context_mask,
                       const amdnuwa_xattn_kv* packed, amdnuwa_stream stream);
/* the same with kv_f16 = the fp16 rendering of to_kv(context) in place of the bf16 residuals: the *_lo images of `packed` become fp16
 * images (what amdnuwa_xattn2_fwd_f16 reads); the hi images stay the bf16 ones the backward kernels read */
int amdnuwa_xattn_pack_f16(const amdnuwa_xattn_geom* g, const uint16_t* kv, const uint16_t* kv_f16, int ldkv,
                           const float* null_k, const float* null_v, const uint8_t* context_mask,
                           const amdnuwa_xattn_kv* packed, amdnuwa_stream stream);
/* P / Pm (optional): softmax probabilities before / after talking heads, [B][heads][n][JP] bf16 hi[/lo],
 * saved for the backward */
int amdnuwa_xattn_fwd(const amdnuwa_xattn_geom* g, const uint16_t* q, const uint16_t* q_lo, int ldq,
                      const amdnuwa_xattn_kv* packed, const float* w_th, uint16_t* o, uint16_t* o_lo, int ldo,
                      uint16_t* P, uint16_t* P_lo, uint16_t* Pm, uint16_t* Pm_lo, amdnuwa_stream stream);
/* the same, plus (optional) the softmax statistics [B][heads][n][2] fp32 = (row max of the scaled, masked scores in the log2
 * domain, 1 / row sum of exp): what amdnuwa_xattn2_bwd recomputes the probabilities from.  This is how the 'bf16x3-fwd' mode
 * pairs the 3-MFMA forward (Attention.forward, reference nuwa_pytorch.py:339-378) with the recomputing bf16 backward: P / Pm may
 * then be NULL and nothing of size n x JP is saved */
int amdnuwa_xattn_fwd_stats(const amdnuwa_xattn_geom* g, const uint16_t* q, const uint16_t* q_lo, int ldq,
                            const amdnuwa_xattn_kv* packed, const float* w_th, uint16_t* o, uint16_t* o_lo, int ldo,
                            uint16_t* P, uint16_t* P_lo, uint16_t* Pm, uint16_t* Pm_lo, float* stats, amdnuwa_stream stream);
size_t amdnuwa_xattn_bwd_workspace_bytes(const amdnuwa_xattn_geom* g);
/* query side of the backward: dq and ds = dL/dsim [B][heads][n][JP]; dK/dV follow as batched
 * amdnuwa_gemm_tn over ds / Pm, then amdnuwa_xattn_unpack */
int amdnuwa_xattn_bwd(const amdnuwa_xattn_geom* g, const uint16_t* dO, const uint16_t* dO_lo, int lddo,
                      const amdnuwa_xattn_kv* packed, const float* w_th, const uint16_t* P, const uint16_t* P_lo,
                      uint16_t* dS, uint16_t* dS_lo, uint16_t* dq, uint16_t* dq_lo, int lddq, float* dw_th,
                      int accumulate, void* workspace, size_t workspace_bytes, amdnuwa_stream stream);
/* accumulate: bit 0 = add into dnull_k / dnull_v instead of overwriting them; bit 1 = the rows of dKp / dVp follow the chunk-permuted
 * key order in which amdnuwa_xattn2_bwd writes its dS / Pm columns (key 32 c + kk at row 32 c + 8 ((kk & 15) >> 2) + 4 (kk >> 4) + (kk & 3):
 * the order a lane of the kernel holds its 8 slots, one 16-byte store each); amdnuwa_xattn_bwd and amdnuwa_xattn2_bwd_rc use the plain order;
 * bit 2 (ABI 18) = key order of amdnuwa_xattn6_bwd: context key t at position t, the null key at position T (else: null key 0, context key t at t + 1) */
int amdnuwa_xattn_unpack(const amdnuwa_xattn_geom* g, const float* dKp, const float* dVp, uint16_t* dkv,
                         uint16_t* dkv_lo, int ldkv, float* dnull_k, float* dnull_v, int accumulate,
                         amdnuwa_stream stream);

/* ---- cross-attention core, second design (fast bf16 mode only: heads == 8, dim_head == 64, T + 1 <= 288) --------------
 * One wave = 16 queries x all heads, head mix in registers, K/V chunks shared through a direct-to-LDS ring; the forward saves
 * only the softmax statistics stats[B][heads][n][2] = (row max, 1 / row sum) and the backward recomputes the probabilities.
 * _bwd writes dS and Pm ([B][heads][n][JP] bf16, as amdnuwa_xattn_bwd / _fwd do) for the batched dK / dV GEMMs, dq, and the
 * per-workgroup talking-heads partials part_th (reduce with amdnuwa_colsum or the Python side). */
int amdnuwa_xattn2_supported(const amdnuwa_xattn_geom* g);
int amdnuwa_xattn2_fwd(const amdnuwa_xattn_geom* g, const uint16_t* q, int ldq, const amdnuwa_xattn_kv* packed,
                       const float* w_th, uint16_t* o, int ldo, float* stats, amdnuwa_stream stream);
/* the same core on SINGLE fp16 MFMAs: q_f16 [B*n, ldq] and the *_lo images of `packed` (written by amdnuwa_xattn_pack_f16) hold fp16
 * values; o leaves as a bf16 hi + lo pair (o_lo may be NULL).  The forward cross-attention core of the 'bf16x3-fwd' mode: with
 * the hi + lo projection GEMMs around it the full-depth logits stay within 1e-3 of the fp32 reference (tools/error_budget.py) */
/* o_lo_f16: as for amdnuwa_sparse3dna_fwd_f16 */
int amdnuwa_xattn2_fwd_f16(const amdnuwa_xattn_geom* g, const uint16_t* q_f16, int ldq, const amdnuwa_xattn_kv* packed,
                           const float* w_th, uint16_t* o, uint16_t* o_lo, int ldo, int o_lo_f16, float* stats, amdnuwa_stream stream);
size_t amdnuwa_xattn2_bwd_workspace_bytes(const amdnuwa_xattn_geom* g);
/* dS / Pm [B][heads][n][JP]: the keys of every 32-key chunk in the order the kernel's lanes hold them (position 8 g + e of a chunk = key
 * (e < 4 ? 4 g + e : 16 + 4 g + e - 4)): batched amdnuwa_gemm_tn over them yields dKp / dVp rows in the same order, which
 * amdnuwa_xattn_unpack undoes when its flag bit 1 is set */
int amdnuwa_xattn2_bwd(const amdnuwa_xattn_geom* g, const uint16_t* q, int ldq, const uint16_t* dO, int lddo,
                       const amdnuwa_xattn_kv* packed, const float* w_th, const float* stats, uint16_t* dS, uint16_t* Pm,
                       uint16_t* dq, int lddq, float* part_th, size_t part_bytes, amdnuwa_stream stream);
/* ABI 17: the same with flags.  Bit 0: dS / Pm are written CHUNK-MAJOR, [B][heads][JP / 32][n][32] (same chunk-permuted key order inside a
 * chunk): a store instruction of the kernel then covers 1 KiB of contiguous memory (16 queries x 64 B) instead of sixteen 64-byte pieces at
 * the 2 JP-byte row pitch (xattn3_bwd 2035 -> 1878 us at b = 128).  Read them with amdnuwa_gemm_tn and a_chunk32.  AMDNUWA_ERR_UNSUPPORTED when
 * the shape is not supported. */
int amdnuwa_xattn2_bwd_ex(const amdnuwa_xattn_geom* g, const uint16_t* q, int ldq, const uint16_t* dO, int lddo,
                          const amdnuwa_xattn_kv* packed, const float* w_th, const float* stats, uint16_t* dS, uint16_t* Pm,
                          uint16_t* dq, int lddq, float* part_th, size_t part_bytes, int flags, amdnuwa_stream stream);
/* The recomputing backward without the dS / Pm arrays (n % 32 == 0): the query side as above (dq, part_th) leaves nb / delta per
 * (head, query) in `nbd` (>= amdnuwa_xattn2_bwd_rc_stats_bytes), and a key-side kernel -- one workgroup per 32 keys of a sample,
 * the queries streamed through LDS -- recomputes ds and P' from them and accumulates dKp / dVp ([B][heads][JP][dim_head] fp32,
 * dKp already scaled: the inputs of amdnuwa_xattn_unpack).  Same rounding points as _bwd + the two batched amdnuwa_gemm_tn;
 * 3 GB less written and read back per layer call at b = 128. */
int amdnuwa_xattn2_bwd_rc_supported(const amdnuwa_xattn_geom* g);
size_t amdnuwa_xattn2_bwd_rc_stats_bytes(const amdnuwa_xattn_geom* g);
int amdnuwa_xattn2_bwd_rc(const amdnuwa_xattn_geom* g, const uint16_t* q, int ldq, const uint16_t* dO, int lddo,
                          const amdnuwa_xattn_kv* packed, const float* w_th, const float* stats, uint16_t* dq, int lddq,
                          float* part_th, size_t part_bytes, float* nbd, size_t nbd_bytes, float* dKp, float* dVp,
                          amdnuwa_stream stream);
/* ---- cross-attention core, third design ("xattn6", ABI 18; reference nuwa_pytorch.py:339-378): heads == 8, dim_head == 64, ANY context
 * length T >= 1 (g->JP is ignored).  Keys / values travel as images in the kernels' LDS order, written once per layer call by
 * amdnuwa_xattn6_pack from the 16-bit to_kv(context) rows: K6 / V6 [B][nch][heads][32][64] 16-bit with nch = amdnuwa_xattn6_nch(T) =
 * 2 * ceil(T / 64) chunks of 32 keys (K [key][d]; V transposed, key slots in the lanes' order; bank swizzles baked in),
 * vbits [B][nch]: bit j of word c = context key 32 c + j exists and passes context_mask.  The learned null key / value (np.py:343-347) are
 * NOT image rows: the kernels take null_k / null_v [heads][dim_head] fp32 and treat the null key as a rank-one term.
 * f16 != 0: q16 / kv16 and the images are fp16 and every MFMA is the fp16 one ('bf16x3-fwd'); else bf16.
 * stats [B][heads][n][2] as amdnuwa_xattn2_fwd writes them (any reference maximum m in the log2 domain, 1 / sum of exp2(s - m) incl. the
 * null key): what amdnuwa_xattn2_bwd* recompute the probabilities from.  o / o_lo / o_lo_f16 as amdnuwa_xattn2_fwd_f16. */
typedef struct { uint16_t *K6, *V6; uint32_t* vbits; } amdnuwa_xattn6_kv;
int amdnuwa_xattn6_supported(const amdnuwa_xattn_geom* g);
int amdnuwa_xattn6_nch(int T);
size_t amdnuwa_xattn6_image_bytes(const amdnuwa_xattn_geom* g);      /* bytes of K6 (and of V6); vbits: B * nch words */
int amdnuwa_xattn6_pack(const amdnuwa_xattn_geom* g, const uint16_t* kv16, int ldkv, const uint8_t* context_mask, int f16,
                        const amdnuwa_xattn6_kv* out, amdnuwa_stream stream);
int amdnuwa_xattn6_fwd(const amdnuwa_xattn_geom* g, const uint16_t* q16, int ldq, const amdnuwa_xattn6_kv* kv, const float* null_k,
                       const float* null_v, const float* w_th, uint16_t* o, uint16_t* o_lo, int ldo, int o_lo_f16, float* stats,
                       int f16, amdnuwa_stream stream);
/* The query side of the recomputing backward on the same recipe (bf16; replaces amdnuwa_xattn2_bwd_ex with flag bit 0 where g->JP / 32 <= 64):
 * amdnuwa_xattn6_pack_bwd writes K6 / V6 [B][JP / 32][heads][32][64] bf16 ([key][d] tiles in LDS order; positions 0..T-1 = the context keys,
 * position T = the null key: the key order of its dS / Pm, which amdnuwa_xattn_unpack reads with flag bit 2 set) and vbits [B][JP / 32]; amdnuwa_xattn6_bwd takes them, q / dO [B*n, ld] bf16
 * and the forward's statistics and writes dq, dS / Pm CHUNK-MAJOR ([B][heads][JP / 32][n][32], chunk-permuted slots, lane groups without a
 * key unwritten -- exactly amdnuwa_xattn2_bwd_ex's flag-bit-0 layout) and the talking-heads partials part_th (>= _workspace_bytes). */
size_t amdnuwa_xattn6_bwd_image_bytes(const amdnuwa_xattn_geom* g);
int amdnuwa_xattn6_pack_bwd(const amdnuwa_xattn_geom* g, const uint16_t* kv, int ldkv, const float* null_k, const float* null_v,
                            const uint8_t* context_mask, const amdnuwa_xattn6_kv* out, amdnuwa_stream stream);
size_t amdnuwa_xattn6_bwd_workspace_bytes(const amdnuwa_xattn_geom* g);
int amdnuwa_xattn6_bwd(const amdnuwa_xattn_geom* g, const uint16_t* q, int ldq, const uint16_t* dO, int lddo, const amdnuwa_xattn6_kv* kv,
                       const float* null_k, const float* null_v, const float* w_th, const float* stats, uint16_t* dS, uint16_t* Pm, uint16_t* dq, int lddq, float* part_th,
                       size_t part_bytes, amdnuwa_stream stream);
/* ABI 19, the fp16-gradient form (block class 'x' of the 'bf16x3-fwd' mode): images from the FP16 copy of to_kv(context)
 * (amdnuwa_xattn6_pack_bwd_f16; the null key / value rounded to fp16), q = the fp16 copy the forward read, dO = fp16(S dO); dq leaves as
 * fp16(S dq), saturating and counted by amdnuwa_f16_sat_count, dS as fp16(S dS) and Pm as fp16 through the plain converter; the V image carries the
 * factor 2^-6 (the kernel's dP' = dO . V then stays inside fp16 where dO does) and the part_th partials the factor S / 64.  Every MFMA is
 * the fp16 one.  The dK / dV products over dS / Pm then run amdnuwa_gemm_tn with ab_f16 + a_chunk32 and alpha_dev = 1 / S.
 * amdnuwa_xattn6_fwd accepts o == NULL together with o_lo_f16 (the fp16 copy is then the only output). */
int amdnuwa_xattn6_pack_bwd_f16(const amdnuwa_xattn_geom* g, const uint16_t* kv_f16, int ldkv, const float* null_k, const float* null_v,
                                const uint8_t* context_mask, const amdnuwa_xattn6_kv* out, amdnuwa_stream stream);
int amdnuwa_xattn6_bwd_f16(const amdnuwa_xattn_geom* g, const uint16_t* q_f16, int ldq, const uint16_t* dO_f16, int lddo, const amdnuwa_xattn6_kv* kv,
                           const float* null_k, const float* null_v, const float* w_th, const float* stats, uint16_t* dS, uint16_t* Pm, uint16_t* dq,
                           int lddq, float* part_th, size_t part_bytes, amdnuwa_stream stream);
/* ---- plain attention core with linear memory ("cattn", ABI 20; reference nuwa_pytorch.py:339-378, the causal mask of :364-367 when
 * g->causal): keys = [learned null key | the T key rows], query i sees the null key and rows 0..i (causal) or every row, minus rows
 * whose key_mask byte is 0 (key_mask [B][T] or NULL; the null key is never masked); fp32 softmax per head, then the heads x heads
 * talking-heads mix, then the product with V.  ANY n >= 1, heads 1..8, dim_head 32 or 64.
 * ABI 21, the rectangular form: g->n_keys = T key rows per sample taken from another tensor (a context); 0 means T = n, self-attention,
 * exactly the ABI 20 behaviour.  With T != n: q16 / dO / o / dq are [B*n, ld], k16 / v16 / dk / dv [B*T, ldkv], stats stays
 * [B][heads][n][2]; causal != 0 is then unsupported (amdnuwa_cattn_supported returns 0, the entry points AMDNUWA_ERR_UNSUPPORTED).
 * q16 / k16 / v16 are 16-bit rows straight out of the projection GEMMs (k16 and v16 share ldkv: two column ranges of to_kv's output);
 * f16 != 0: fp16 operands and fp16 MFMAs ('bf16x3-fwd'), else bf16.  Nothing of size n x T is written: the forward makes two passes over
 * the keys and leaves stats [B][heads][n][2] = (maximum of the scaled scores in the log2 domain incl. the null key, 1 / sum of exp2), the backward
 * recomputes the probabilities from q, k and stats.  o / o_lo / o_lo_f16 as amdnuwa_xattn6_fwd (o == NULL with o_lo_f16: the fp16 copy alone). */
typedef struct {
    int B, n;               /* samples, query rows per sample */
    int heads, dim_head;    /* heads 1..8, dim_head in {32, 64} */
    float scale;
    int causal;             /* != 0: query i sees keys 0..i (needs n_keys == 0 or n_keys == n) */
    int n_keys;             /* ABI 21: key rows per sample; 0 = n (self-attention) */
} amdnuwa_cattn_geom;
int amdnuwa_cattn_supported(const amdnuwa_cattn_geom* g);
int amdnuwa_cattn_fwd(const amdnuwa_cattn_geom* g, const uint16_t* q16, int ldq, const uint16_t* k16, const uint16_t* v16, int ldkv,
                      const uint8_t* key_mask, const float* null_k, const float* null_v, const float* w_th, uint16_t* o, uint16_t* o_lo,
                      int ldo, int o_lo_f16, float* stats, int f16, amdnuwa_stream stream);
/* The recomputing backward on bf16 operands (q / dO [B*n, ld], k / v [B*T, ldkv] bf16, stats from the forward): a query-stationary sweep for
 * delta[h][i] = sum_j P_h dP_h (the head mix sits between P and O, so O . dO does not give it), one for dq, key-stationary sweeps over the
 * query tiles (causal: those at or below the diagonal) for dk and dv.  The query-stationary sweeps run B * ceil(n / 64) workgroups, the
 * key-stationary ones B * ceil(T / 64); only the former leave partials, so the workspace grows with n and does not depend on T.
 *  dq / dk / dv leave as bf16 rows (dk and dv share lddkv); dw_th is [8][8] fp32 with
 * dW_th[g][h] at 8 g + h (rows / columns >= heads are zero), dnull_k / dnull_v [heads][dim_head] fp32.  No atomics: per-workgroup partials
 * inside `workspace` (>= _workspace_bytes, AMDNUWA_ERR_WORKSPACE otherwise) are reduced in a fixed order, two runs are bit-identical. */
size_t amdnuwa_cattn_bwd_workspace_bytes(const amdnuwa_cattn_geom* g);
int amdnuwa_cattn_bwd(const amdnuwa_cattn_geom* g, const uint16_t* q, int ldq, const uint16_t* k, const uint16_t* v, int ldkv,
                      const uint16_t* dO, int lddo, const uint8_t* key_mask, const float* null_k, const float* null_v, const float* w_th,
                      const float* stats, uint16_t* dq, int lddq, uint16_t* dk, uint16_t* dv, int lddkv, float* dw_th, float* dnull_k,
                      float* dnull_v, void* workspace, size_t workspace_bytes, amdnuwa_stream stream);
/* Attention dropout inside the cattn kernels (added at ABI 21, purely additive; np.py:370-374, `self.dropout(self.talking_heads(attn))`:
 * the mask acts AFTER the talking-heads mix).  With M[g][i][j] in {0, 1} the keep bit of output head g, query i, key row j, M0[g][i] that
 * of the null slot and s = drop_scale = 1 / (1 - p):
 *   forward   A''[g] = M . s . A'[g] feeds the product with V (A' = the mixed probabilities), the null term takes M0 . s . A'0[g];
 *   backward  dv = A''^T dO;  dA'[g] = M . s . (dO_g . V_g) and dA'0[g] = M0 . s . (dO_g . null_v_g) before anything reads them, so delta,
 *             dq, dk, dW_th and dnull_k follow unchanged; dnull_v sums the masked A'0.  The statistics pass is untouched.
 * The caller draws the mask and hands the SAME arrays to the forward and the backward; one byte per (query, key) pair, bit g set = head g kept:
 *   keep   [B][n][KP], KP = 32 * ceil(T / 32)   read by the query-stationary sweeps (forward, delta, dq)
 *   keep_t [B][T][NP], NP = 32 * ceil(n / 32)   the same bytes transposed, read by the key-stationary sweeps (dk, dv)
 *   keep0  [B][n]                               the null slot
 * uint8, every base 4-byte aligned (a lane's eight streamed rows are two aligned 32-bit loads per tile on either side).  Padding bytes, bits
 * at or above `heads`, and the bytes of masked or causally hidden pairs never influence an output.  An all-ones mask with drop_scale = 1
 * gives the bits of the unmasked calls.  Envelope = amdnuwa_cattn_supported (amdnuwa_cattn_drop_supported answers the same); a NULL or
 * misaligned mask array, or a drop_scale that is not finite or below 1: AMDNUWA_ERR_ARG before anything is launched.  _bwd_drop runs on the
 * workspace amdnuwa_cattn_bwd_workspace_bytes reports. */
int amdnuwa_cattn_drop_supported(const amdnuwa_cattn_geom* g);
int amdnuwa_cattn_fwd_drop(const amdnuwa_cattn_geom* g, const uint16_t* q16, int ldq, const uint16_t* k16, const uint16_t* v16, int ldkv,
                           const uint8_t* key_mask, const float* null_k, const float* null_v, const float* w_th, uint16_t* o, uint16_t* o_lo,
                           int ldo, int o_lo_f16, float* stats, int f16, const uint8_t* keep, const uint8_t* keep0, float drop_scale,
                           amdnuwa_stream stream);
int amdnuwa_cattn_bwd_drop(const amdnuwa_cattn_geom* g, const uint16_t* q, int ldq, const uint16_t* k, const uint16_t* v, int ldkv,
                           const uint16_t* dO, int lddo, const uint8_t* key_mask, const float* null_k, const float* null_v, const float* w_th,
                           const float* stats, uint16_t* dq, int lddq, uint16_t* dk, uint16_t* dv, int lddkv, float* dw_th, float* dnull_k,
                           float* dnull_v, void* workspace, size_t workspace_bytes, const uint8_t* keep, const uint8_t* keep_t,
                           const uint8_t* keep0, float drop_scale, amdnuwa_stream stream);
/* Text cross-attention (Attention.forward with context, np.py:339-378) for ONE query row per sample (g->n must be 1):
 * q [B, ldq] unscaled, keys / values as packed by amdnuwa_xattn_pack (Kp / Vp images and the valid map), o [B, ldo]. */
int amdnuwa_xattn_decode(const amdnuwa_xattn_geom* g, const uint16_t* q, const uint16_t* q_lo, int ldq,
                         const amdnuwa_xattn_kv* packed, const float* w_th, uint16_t* o, uint16_t* o_lo, int ldo,
                         amdnuwa_stream stream);
/* Single-query attention over ANY number of cached rows: Attention.forward with context (np.py:339-378) and one chunk of
 * CrossModalityCrossAttention (np.py:908-1067) for ONE query row per sample (added at ABI 21, purely additive).  Slot 0 is the learned null
 * key (null_k / null_v [heads][dim_head] fp32, always visible); slot 1 + t is row first_row[0] + t of the cache kv [B][cache_rows][2 * inner]
 * (k | v, bf16 hi with an optional lo image: the layout amdnuwa_s3_decode keeps), t < T.  first_row lives in DEVICE memory so that a captured
 * launch can be replayed for another window; a window that leaves [0, cache_rows) writes nothing.  key_mask [B][T] (0 = hidden) or NULL.
 * Scores q . k * scale, fp32 softmax over the T + 1 slots, P'[g][j] = sum_h w_th[g][h] P[h][j] + th_bias[g] (th_bias [heads] or NULL: the
 * bias of the reference's Conv3d talking heads reaches every slot, null and masked ones included), o[g] = sum_j P'[g][j] v_j[g].
 * q [B, ldq] unscaled and o [B, ldo] are bf16 hi (+ lo) rows.  heads 1..8, dim_head 32 / 64, any T >= 1; otherwise AMDNUWA_ERR_UNSUPPORTED.
 * The T + 1 slots are cut into splits of 128, one workgroup per (split, sample); the split count depends on T alone, partial results meet
 * in index order and there are no atomics: two runs are bit-identical.  workspace: >= _workspace_bytes =
 * 4 * B * (heads * (T + 1) + ceil((T + 1) / 128) * (2 * heads + heads * dim_head)) bytes (scores, per-split statistics, per-split partial
 * rows), AMDNUWA_ERR_WORKSPACE otherwise. */
size_t amdnuwa_attn_decode_rows_workspace_bytes(int B, int T, int heads, int dim_head);
int amdnuwa_attn_decode_rows(int B, int T, int heads, int dim_head, float scale, const uint16_t* q, const uint16_t* q_lo, int ldq,
                             const uint16_t* kv, const uint16_t* kv_lo, int cache_rows, const int* first_row, const uint8_t* key_mask,
                             const float* null_k, const float* null_v, const float* w_th, const float* th_bias, uint16_t* o,
                             uint16_t* o_lo, int ldo, void* workspace, size_t workspace_bytes, amdnuwa_stream stream);
/* The ROWS FORM of amdnuwa_attn_decode_rows (added at ABI 21, purely additive): decoder rows 0 .. R-1 of every sample in one call -- the
 * cache prefill of a NUWA.generate / NUWAVideoAudio.generate whose frame window slides over a text context of more than 287 tokens.  q and o
 * are [B * R, ld] bf16 hi (+ lo) rows, sample-major: row b * R + r is decoder row r of sample b.  All R rows of a sample attend the SAME
 * window: the null key plus rows first_row[0] .. first_row[0] + T - 1 of that sample's kv [B][cache_rows][2 * inner]; key_mask [B][T] or
 * NULL.  No row is special (text cross-attention treats <bos> like any other row): rows 0 .. R-1 are all read and written.  kv, first_row
 * (DEVICE memory), null_k, null_v, w_th, th_bias and scale are those of amdnuwa_attn_decode_rows.  The kernels are the single row's, told by
 * the launch which query a workgroup serves: the same loads, expression trees, 128-slot splits and meeting order, no atomics -- row (b, r)
 * of o is BIT-IDENTICAL to amdnuwa_attn_decode_rows on q[b * R + r] alone, with and without the lo images, and two runs are bit-identical.
 * A window that leaves [0, cache_rows) writes nothing.  Queries are indexed on the x dimension of the grid and taken in chunks of 2048
 * (three launches per chunk on `stream`, which share the workspace), so B * R may exceed 65 535; it must fit an int.  Arguments are checked
 * first (a null pointer, a non-positive B / R / T / heads / dim_head, cache_rows < T, lo images not given together, ld < heads * dim_head:
 * AMDNUWA_ERR_ARG), then the envelope (heads 1..8, dim_head 32 / 64, otherwise AMDNUWA_ERR_UNSUPPORTED), then the workspace:
 * >= _workspace_bytes = the single-row formula with min(B * R, 2048) -- one chunk -- in place of B, AMDNUWA_ERR_WORKSPACE otherwise. */
size_t amdnuwa_attn_rows_workspace_bytes(int B, int R, int T, int heads, int dim_head);
int amdnuwa_attn_rows(int B, int R, int T, int heads, int dim_head, float scale, const uint16_t* q, const uint16_t* q_lo, int ldq,
                      const uint16_t* kv, const uint16_t* kv_lo, int cache_rows, const int* first_row, const uint8_t* key_mask,
                      const float* null_k, const float* null_v, const float* w_th, const float* th_bias, uint16_t* o, uint16_t* o_lo, int ldo,
                      void* workspace, size_t workspace_bytes, amdnuwa_stream stream);
/* SparseCross2DNA (np.py:761-901, rows after <bos>) for ONE query row per sample, its window read IN PLACE (added at ABI 21, purely
 * additive).  The query of decoder row pos[0] (DEVICE memory, >= 1: a captured launch serves every row) sits at feature-map position
 * i = (pos[0] - 1) mod n_pos.  Slot 0 is the learned null key, always visible; slot 1 + j is context row slot_rows[i][j] of the sample, read
 * from kv [B][ctx_rows][2 * inner] (k | v: to_kv of the sketch rows, bf16 hi with an optional lo image).  slot_rows [n_pos][J] int32 lives in
 * device memory; a negative entry is 'same' padding: the slot is hidden, contributes nothing, and NO address is formed from it.  key_mask
 * [B][ctx_rows] (0 = hidden; indexed by CONTEXT ROW, not by slot) or NULL; a row the mask hides may still be read.  Scores q . k * scale,
 * fp32 softmax over the J + 1 slots, P'[g][j] = sum_h w_th[g][h] P[h][j] (no bias), o[g] = sum_j P'[g][j] v_j[g].  pos[0] < 1, or any
 * entry of slot_rows[i] >= ctx_rows, writes nothing (the <bos> row is the caller's).  q [B, ldq] unscaled, o [B, ldo]: bf16 hi (+ lo) rows;
 * the lo images of q, kv and o are given together or not at all.  heads 1..8, dim_head 32 / 64, any J >= 1, any n_pos >= 1; otherwise
 * AMDNUWA_ERR_UNSUPPORTED (arguments are checked first: a null or non-positive one is AMDNUWA_ERR_ARG).  The kernels are those of
 * amdnuwa_attn_decode_rows with the slot -> row mapping exchanged: splits of 128 slots, the split count a function of J alone, partial results
 * met in index order, no atomics -- two runs are bit-identical.  workspace: >= _workspace_bytes =
 * 4 * B * (heads * (J + 1) + ceil((J + 1) / 128) * (2 * heads + heads * dim_head)) bytes, AMDNUWA_ERR_WORKSPACE otherwise. */
size_t amdnuwa_cross2dna_decode_workspace_bytes(int B, int J, int heads, int dim_head);
int amdnuwa_cross2dna_decode(int B, int J, int heads, int dim_head, float scale, const uint16_t* q, const uint16_t* q_lo, int ldq,
                             const uint16_t* kv, const uint16_t* kv_lo, int ctx_rows, const int* slot_rows, int n_pos, const int* pos,
                             const uint8_t* key_mask, const float* null_k, const float* null_v, const float* w_th, uint16_t* o,
                             uint16_t* o_lo, int ldo, void* workspace, size_t workspace_bytes, amdnuwa_stream stream);
/* The ROWS FORM of amdnuwa_cross2dna_decode (added at ABI 21, purely additive): decoder rows 1 .. R-1 of every sample in one call, the
 * window read in place -- the cache prefill of a NUWASketch.generate whose frame window slides.  q and o are [B * R, ld] bf16 hi (+ lo)
 * rows, sample-major: the query of row r (1 <= r < R) of sample b is row b * R + r, sits at feature-map position (r - 1) mod n_pos and
 * attends through slot_rows[(r - 1) mod n_pos], exactly as the single-row call does at pos[0] = r.  There is no device-side position: the
 * rows are given by the launch.  Row 0 of every sample (<bos>) is NEITHER READ NOR WRITTEN, it stays with the caller; R == 1 returns
 * AMDNUWA_OK without a launch (and needs no workspace).  kv, slot_rows, key_mask, null_k, null_v, w_th and scale are those of
 * amdnuwa_cross2dna_decode.  The kernels are the single row's, told by the launch which query a workgroup serves: the same loads,
 * expression trees, 128-slot splits and meeting order, no atomics -- row (b, r) of o is BIT-IDENTICAL to amdnuwa_cross2dna_decode on
 * q[b * R + r] at pos[0] = r, with and without the lo images, and two runs are bit-identical.  A query whose table row has an entry
 * >= ctx_rows writes nothing (decided per query row, alike in all three launches; the other rows are served); negative entries are padding
 * and never become an address.  Queries are indexed on the x dimension of the grid and taken in chunks of 2048 (three launches per chunk on
 * `stream`, which share the workspace), so B * (R - 1) may exceed 65 535; B * R must fit an int.  Arguments are checked first (a null
 * pointer, a non-positive B / R / J / heads / dim_head / ctx_rows / n_pos, lo images not given together, ld < heads * dim_head:
 * AMDNUWA_ERR_ARG), then the envelope (heads 1..8, dim_head 32 / 64, otherwise AMDNUWA_ERR_UNSUPPORTED), then the workspace:
 * >= _workspace_bytes = the single-row formula with min(B * R, 2048) -- one chunk -- in place of B,
 * 4 * min(B * R, 2048) * (heads * (J + 1) + ceil((J + 1) / 128) * (2 * heads + heads * dim_head)) bytes, AMDNUWA_ERR_WORKSPACE otherwise. */
size_t amdnuwa_cross2dna_rows_workspace_bytes(int B, int R, int J, int heads, int dim_head);
int amdnuwa_cross2dna_rows(int B, int R, int J, int heads, int dim_head, float scale, const uint16_t* q, const uint16_t* q_lo, int ldq,
                           const uint16_t* kv, const uint16_t* kv_lo, int ctx_rows, const int* slot_rows, int n_pos,
                           const uint8_t* key_mask, const float* null_k, const float* null_v, const float* w_th, uint16_t* o,
                           uint16_t* o_lo, int ldo, void* workspace, size_t workspace_bytes, amdnuwa_stream stream);
/* The end of one generate() token on the device (np.py:55-65, 1713-1720, 1883-1908; added at ABI 21, purely additive): sample a class from
 * the guided logits and assemble the decoder input row that follows.  logits [B][ld] fp32 (C classes, ld >= C); keep >= 1, keep <= C;
 * temperature > 0; u [B][keep] fp32 uniforms, NULL exactly when keep == 1; emb [C][D] and pos [P][D] fp32; pos_idx [cap] int32 and step [1]
 * int32 in DEVICE memory; ids [B][cap] int64; x_next [B][D] fp32.  With t = step[0]:
 *   1. the keep largest logits of each row in descending order, equal values by lower class index first (-0 counts as +0, NaN as the largest);
 *   2. score_j = v_j / temperature + g(u[b][j]) for the rank-j logit v_j, g(u) = -logf(max(-logf(max(u, 1e-20)), 1e-20));
 *   3. the FIRST maximum of the scores (keep == 1: the largest logit itself, nothing is drawn);
 *   4. ids[b][t] = its class, x_next[b] = emb[class] + pos[pos_idx[t]] (one fp32 add per element).
 * t outside [0, cap) or pos_idx[t] outside [0, P) writes NOTHING, in every workgroup alike.  step is read, never advanced: the caller advances
 * it on the stream (inside its captured graph), so that one captured launch serves every token.  One workgroup per sample, no atomics, every
 * reduction of a fixed shape: two runs are bit-identical.  No workspace.  Arguments are checked first (a null pointer, a non-positive size,
 * keep outside [1, C], ld < C, u given with keep == 1 or missing otherwise, a temperature that is not a positive finite number:
 * AMDNUWA_ERR_ARG); then the envelope: C <= 16384, D % 4 == 0, emb / pos / x_next 16-byte aligned, otherwise AMDNUWA_ERR_UNSUPPORTED. */
int amdnuwa_sample_next_row(int B, int C, int keep, float temperature, const float* logits, int ld, const float* u, const float* emb,
                            int D, const float* pos, int P, const int* pos_idx, int cap, const int* step, long long* ids, float* x_next,
                            amdnuwa_stream stream);

/* ---- frozen VQGanVAE tokenizer (VQGanVAE.get_video_indices -> encode, reference vqgan_vae.py:431-435, 452-458), exact fp32 ---- */
typedef struct {
    int N, Cin, H, W, Cout, KH, KW, stride, pad;
    int Ho, Wo;             /* must equal (H + 2*pad - KH) / stride + 1 etc. */
    int leaky;              /* fuse LeakyReLU(0.1) (vqgan_vae.py:94-95) */
} amdnuwa_conv_desc;
/* nn.Conv2d forward, NCHW fp32, square stride/padding (replaces the encoders' convs, vqgan_vae.py:352-365, 228-242) */
int amdnuwa_conv2d_fwd(const amdnuwa_conv_desc* d, const float* x, const float* w, const float* bias, float* y,
                       amdnuwa_stream stream);
/* nn.GroupNorm(groups, C) [+ LeakyReLU(0.1)] on [N][C][HW] fp32 (ResBlock, vqgan_vae.py:233-237) */
int amdnuwa_groupnorm_fwd(const float* x, const float* w, const float* b, float* y, int N, int C, int HW, int groups,
                          float eps, int leaky, amdnuwa_stream stream);
/* cosine-similarity code lookup: indices[r] = argmax_c <l2norm(x[r]), l2norm(codebook[c])>, lowest index on exact ties
 * (eval path of vector_quantize_pytorch.VectorQuantize as called at vqgan_vae.py:368-378, 433); best_sim optional */
int amdnuwa_vq_argmax(const float* x, const float* codebook, long long* indices, float* best_sim, long long R,
                      int n_codes, int code_dim, amdnuwa_stream stream);
/* the same with a workspace (inverse code norms + per-slice partial arg-max): code_dim 256 runs a kernel that keeps the rows in
 * registers as MFMA operands and cuts the code axis into slices; other widths fall through to amdnuwa_vq_argmax */
size_t amdnuwa_vq_argmax_workspace_bytes(long long R, int n_codes);
int amdnuwa_vq_argmax_ws(const float* x, const float* codebook, long long* indices, float* best_sim, long long R, int n_codes,
                         int code_dim, void* workspace, size_t workspace_bytes, amdnuwa_stream stream);
/* Euclidean code lookup (added at ABI 21, purely additive; vq_use_cosine_sim = False of vqgan_vae.py:368-378):
 * indices[r] = argmin_c ||x[r] - codebook[c]||^2, lowest index on exact ties -- the pick of (-torch.cdist(x, codebook)).argmax(-1) in
 * exact arithmetic.  x [R][code_dim], codebook [n_codes][code_dim] fp32; best_dist [R] optional (NULL: not written) = the SQUARED
 * distance to the picked code.  Computed as the arg-max of the centred score
 *     s(r, c) = (x[r] - mu) . (codebook[c] - mu) - 1/2 ||codebook[c] - mu||^2,   mu = column mean of the codebook,
 * products on the exact-fp32 MFMA, best_dist = max(||x[r] - mu||^2 - 2 s, 0).  Why centred: distances do not change under a common
 * shift, fp32 arithmetic does.  The usual expansion ||x||^2 - 2 x.c + ||c||^2 around the origin (torch.cdist's) carries 1/2 ||c||^2,
 * and on a codebook that sits in a tight cloud away from the origin (codes 100 + 0.05 randn, 256 dims: 1/2 ||c||^2 = 1.3e6, ulp 0.125,
 * distances apart by ~1) it mispicks 296 of 300 rows that float64 separates beyond doubt; around mu the same arithmetic picks all right.
 * Deterministic: mu and the code norms come from fixed-order sums (no atomics), equal codes get bit-equal scores wherever they sit, two
 * calls agree bit for bit.  Nothing outside [R] of the outputs is written.
 * Envelope: code_dim even; 256 runs the register-resident-rows kernel over slices of the code axis, every other width a kernel with two
 * 64-row tiles in LDS (code_dim <= 316, as amdnuwa_vq_argmax; more: AMDNUWA_ERR_UNSUPPORTED); tuning key 15 = 1 selects that kernel for 256 too.  Errors come
 * before the device is touched: NULL x / codebook / indices, n_codes <= 0, code_dim <= 0 or odd -> AMDNUWA_ERR_ARG; R <= 0 -> OK, nothing
 * done; workspace NULL or smaller than _workspace_bytes (0 for non-positive arguments) -> AMDNUWA_ERR_WORKSPACE. */
size_t amdnuwa_vq_nearest_l2_workspace_bytes(long long R, int n_codes, int code_dim);
int amdnuwa_vq_nearest_l2(const float* x, const float* codebook, long long* indices, float* best_dist, long long R, int n_codes,
                          int code_dim, void* workspace, size_t workspace_bytes, amdnuwa_stream stream);

/* VQGanAttention block of the encoder (vqgan_vae.py:244-286), exact fp32: in-place l2 normalisation of rows (q and k over the
 * spatial axis), the per-(image, head) attention core with the continuous-position bias [heads][P][P] precomputed from the
 * module's parameters and the learned log-scale, and LayerNormChan (+ residual) over the channel axis of an NCHW tensor. */
/* rows: `groups` groups of rows_per_group consecutive rows of length len, group g starting at row g * group_stride_rows */
int amdnuwa_rows_l2norm(float* x, int groups, int rows_per_group, int group_stride_rows, int len, amdnuwa_stream stream);
/* attention core: qkv [N][3 heads dim_head][P] (q, k already normalised), bias [heads][P][P], scale [heads], out [N][heads dim_head][P].
 * Envelope: dim_head 1 ... 64 (more: UNSUPPORTED), ANY P >= 1.  Where k and v of one head fit LDS (2 dim_head P 4 B <= 160 KiB, i.e.
 * P <= 320 at dim_head 64) the resident kernels run (P = 256, dim_head = 64: f32 MFMA; else VALU); every other shape runs the
 * query-tiled, key-streaming f32 MFMA kernel (online softmax, keys in index order: deterministic, an image's bits do not depend on N).
 * Tuning key 15 = 2 sends every shape to the tiled kernel. */
int amdnuwa_vqattn_core(const float* qkv, const float* bias, const float* scale, float* out, int N, int heads, int dim_head,
                        int P, amdnuwa_stream stream);
/* the same core on a square side x side map (P = side^2) with the bias as a relative-offset table [heads][2 side - 1][2 side - 1]:
 * bias(i, j) = table[h][y_i - y_j + side - 1][x_i - x_j + side - 1].  Always the tiled kernel, the head's table in LDS.
 * Envelope: dim_head 1 ... 64, side 1 ... 64 (beyond either: UNSUPPORTED). */
int amdnuwa_vqattn_core_rel(const float* qkv, const float* table, const float* scale, float* out, int N, int heads, int dim_head,
                            int side, amdnuwa_stream stream);
int amdnuwa_chan_layernorm(const float* x, const float* g, const float* b, const float* resid, float* y, int N, int C, int HW,
                           float eps, amdnuwa_stream stream);

/* VQGanVAE.decode pieces (vqgan_vae.py:437-441, GLUResBlock 212-226): nn.GLU over the channel axis of [N][2C][HW] and the
 * x2 bilinear nn.Upsample (align_corners=False) of an NCHW tensor; the rest of the decoder reuses conv2d / groupnorm / vqattn */
int amdnuwa_glu_chan(const float* x, float* y, int N, int C, int HW, amdnuwa_stream stream);
int amdnuwa_upsample_bilinear2x(const float* x, float* y, int N, int C, int H, int W, amdnuwa_stream stream);

/* ---- optimiser step of the trainer (row f2; reference train_nuwa.py:253-255 + optimizer.py:6-31) -------------------------------
 * "multi-tensor apply": a DEVICE table of chunks (<= 65536 elements each is a good size), every chunk pointing into one fp32
 * parameter / gradient / first- / second-moment tensor.  g == NULL marks a parameter without gradient this step (skipped). */
typedef struct {
    float* p; const float* g; float* m; float* v;
    long long n;
    float weight_decay;     /* 0 for the ndim < 2 parameters (optimizer.py:6-9) */
    float bias_correction1, bias_correction2;   /* 1 - beta^t with t = number of updates THIS parameter has received (torch keeps
                                                    the step count per parameter: one skipped for lack of a gradient lags behind) */
} amdnuwa_adamw_chunk;
/* Alignment: p, g, m and v need the 4-byte alignment of a float and nothing more.  A chunk whose pointers all lie on 16-byte borders
 * (g alone for amdnuwa_grad_norm) runs the float4 loops; any other chunk -- a gradient that is a view at an odd element offset of a
 * flat bucket, say -- runs the same arithmetic on float accesses, the same elements in the same order, with bit-identical results.  The test
 * is per chunk, so keep tensors of more than 65536 elements on 16-byte borders as a whole (chunk k starts 262144 k bytes in). */
/* out2[0] = global L2 norm of all gradients, out2[1] = min(1, max_norm / (norm + 1e-6)) (1 if max_norm <= 0; NaN if the norm is); fixed-order
 * reduction; partials: nchunks floats of scratch.  Everything stays on the device. */
int amdnuwa_grad_norm(const amdnuwa_adamw_chunk* chunks, int nchunks, float max_norm, float* partials, float* out2,
                      amdnuwa_stream stream);
int amdnuwa_scale_grads(const amdnuwa_adamw_chunk* chunks, int nchunks, const float* coef, amdnuwa_stream stream);
/* torch.optim.AdamW semantics (decoupled decay); gradients are multiplied by *clip_coef (device scalar, may be NULL) on the fly */
int amdnuwa_adamw_step(const amdnuwa_adamw_chunk* chunks, int nchunks, float lr, float beta1, float beta2, float eps,
                       const float* clip_coef, amdnuwa_stream stream);

/* ---- gradient exchange of the data-parallel step on RCCL (one process per GPU; SURVEY.md section 8 row e) --------------------
 * The reference has no multi-GPU code of its own (train_nuwa.py runs one device); this is what nuwa_pytorch_amd/distributed.py's
 * GradReducer(collective='native') puts under its flat fp32 buckets instead of torch.distributed.  librccl is dlopen()ed at the
 * first call (amdnuwa_comm_available() == 0 and AMDNUWA_ERR_UNSUPPORTED without it).  Rank 0 draws the 128-byte id, the host side
 * hands it to every rank (any channel: a torch.distributed object broadcast, a file, MPI), every rank calls _init on ITS device.
 * All collectives are in place, enqueued on `stream`, and return before the data moved; AMDNUWA_ERR_COMM = an RCCL error
 * (amdnuwa_comm_last_error() has its text, per thread). */
#define AMDNUWA_COMM_ID_BYTES 128
#define AMDNUWA_ERR_COMM -4
typedef struct amdnuwa_comm amdnuwa_comm;
int amdnuwa_comm_available(void);
const char* amdnuwa_comm_last_error(void);
int amdnuwa_comm_unique_id(void* id_out, size_t bytes);
int amdnuwa_comm_init(amdnuwa_comm** out, const void* id, size_t id_bytes, int rank, int world, int device);
int amdnuwa_comm_rank(const amdnuwa_comm* c);
int amdnuwa_comm_world(const amdnuwa_comm* c);
/* buf[0..count) <- sum (average != 0: mean, ncclAvg -- no separate division pass) over the ranks */
int amdnuwa_comm_allreduce(amdnuwa_comm* c, float* buf, size_t count, int average, amdnuwa_stream stream);
/* the same result over a store of world * shard floats as reduce-scatter + all-gather (rank r reduces buf + r * shard) */
int amdnuwa_comm_reduce_scatter_allgather(amdnuwa_comm* c, float* buf, size_t shard, int average, amdnuwa_stream stream);
/* bytes of buf <- rank `root`'s (the initial parameter broadcast) */
int amdnuwa_comm_broadcast(amdnuwa_comm* c, void* buf, size_t bytes, int root, amdnuwa_stream stream);
int amdnuwa_comm_destroy(amdnuwa_comm* c);

#ifdef __cplusplus
}
#endif
#endif
