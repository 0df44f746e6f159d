// Incremental (one new token per sample) decoding kernels for NUWA.generate (np.py:1841-1915) with a key/value cache.
//
// The reference recomputes the whole prefix twice per sampled token.  Every decoder stage is causal -- Sparse3DNA only looks
// at taps <= the query position (np.py:420-457), ShiftVideoTokens only at the row above / to the left (np.py:210-253), and
// cross-attention / FeedForward are row-wise -- so row `pos` of the decoder can be computed from cached rows < pos:
//   * decode_shift_kernel : caches the new pre-norm row and emits its token-shifted form
//   * s3_decode_kernel    : caches the new key / value row and runs the 3DNA attention of the single new query
// The position is read from DEVICE memory so that one captured HIP graph serves every token of the sequence.
// Past max_video_frames generate() slides its frame window (np.py:1873-1881): every kept token moves one frame earlier and every cached row
// changes.  The caches are then rebuilt by one full-sequence pass whose norms / shift / cache writes are the ROWS forms of the kernels above:
//   * prefill_ln_kernel + prefill_shift_kernel : decode_ln_kernel for rows 0 .. R-1 of every sample at once.  Both norms are ONE body
//                                                (ln_body), so a row is bit-identical to the single-row step
//   * prefill_kv_kernel                        : the k | v columns of R projected rows into the 3DNA cache
// The token-shift rule is stated once (ShiftRule) for decode_shift_kernel, the single-row norm and prefill_shift_kernel.
#include "common.h"
#include "../../include/amdnuwa.h"

namespace {

__device__ __forceinline__ float ld_hl(const bf16_t* hi, const bf16_t* lo, size_t i) {
    return lo ? bf2f(hi[i]) + bf2f(lo[i]) : bf2f(hi[i]);
}
__device__ __forceinline__ void st_hl(bf16_t* hi, bf16_t* lo, size_t i, float v) {
    if (lo) { bf16_t h, l; f2bf_hilo(v, h, l); hi[i] = h; lo[i] = l; }
    else hi[i] = f2bf(v);
}

// ---- the token-shift rule, stated once ---------------------------------------------------------------------------------------
// Channel e of row i of a sample (row 0 is <bos>) takes the same channel of row i - back(e):  back > 0: that many rows back;
// back == 0: zeros;  back < 0: not shifted, the row keeps its own value.  Only the first two channel quarters are ever shifted.
//   fmap > 0  ShiftVideoTokens (np.py:210-253): first quarter <- the token one grid row up (i - fmap), second quarter <- the token to
//             the left (i - 1), zero at the frame border; <bos> is not shifted
//   fmap < 0  ShiftAudioTokens (np.py:157-183): first half <- row i - 1, <bos> included; zeros for row 0
// The row's part (two divisions) is the constructor's, so that a loop over channels pays for it once.
struct ShiftRule {
    int qd, up, left;
    __device__ __forceinline__ ShiftRule(int i, int D, int fmap) : qd(D >> 2), up(-1), left(-1) {
        if (fmap > 0) {
            if (i > 0) { const int p = i - 1, wq = p % fmap, yq = (p / fmap) % fmap; up = yq > 0 ? fmap : 0; left = wq > 0 ? 1 : 0; }
        } else {
            up = left = i > 0 ? 1 : 0;
        }
    }
    __device__ __forceinline__ int back(int e) const { return e < qd ? up : e < 2 * qd ? left : -1; }
};

// h_new [B, D] (row `pos` of every sample) -> cache[b][pos] and out[b] = shift(h)[pos]
__global__ __launch_bounds__(256) void decode_shift_kernel(const bf16_t* __restrict__ h_hi, const bf16_t* __restrict__ h_lo,
                                                           bf16_t* __restrict__ c_hi, bf16_t* __restrict__ c_lo,
                                                           bf16_t* __restrict__ o_hi, bf16_t* __restrict__ o_lo,
                                                           const int* __restrict__ pos_p, int cache_rows, int D, int fmap) {
    const int b = blockIdx.x, pos = pos_p[0];
    if (pos < 0 || pos >= cache_rows) return;
    const size_t crow = ((size_t)b * cache_rows + pos) * D, nrow = (size_t)b * D;
    const ShiftRule rule(pos, D, fmap);
    for (int c = threadIdx.x; c < D; c += blockDim.x) {
        const bf16_t hv = h_hi[nrow + c], lv = h_lo ? h_lo[nrow + c] : (bf16_t)0;
        c_hi[crow + c] = hv;
        if (c_lo) c_lo[crow + c] = lv;
        bf16_t oh = hv, ol = lv;
        const int back = rule.back(c);
        if (back >= 0) {
            const size_t srow = crow - (size_t)back * D;
            oh = back ? c_hi[srow + c] : (bf16_t)0;
            ol = (back && c_lo) ? c_lo[srow + c] : (bf16_t)0;
        }
        o_hi[nrow + c] = oh;
        if (o_lo) o_lo[nrow + c] = ol;
    }
}

// ---- the norms around a block, for the one new row of every sample, in ONE launch ------------------------------------------
//   x_new = resid + LN(y; w, b)                     (post-norm + residual of the block that just ran; skipped when resid == NULL:
//                                                    then x_new = y, the fp32 decoder input row)
//   h     = LN(x_new; next_w, next_b)               (pre-norm of the next block)
//   cache[b][pos] = h ; out = shift(h)[pos]         (when the next block is token-shifted: cache != NULL)
// One workgroup (256 threads) per row; D <= 4096.  ln_body is the one body of both forms:
//   ROWS = false (decode_ln_kernel)  : row blockIdx.x is sample blockIdx.x at the device-side position pos_p[0]; the shifted channels of out
//                                      are gathered from the cache in the same launch (earlier rows: earlier launches)
//   ROWS = true  (prefill_ln_kernel) : row blockIdx.x is row blockIdx.x % R of sample blockIdx.x / R; h goes to the cache row AND to out
//                                      un-shifted -- the shifted channels are other rows' h, which other workgroups of this launch write;
//                                      prefill_shift_kernel gathers them in a second, stream-ordered launch
__device__ __forceinline__ float block_sum(float v, float* red) {
    v = wave_sum(v);
    const int wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[wave] = v;
    __syncthreads();
    float t = 0.f;
    for (int i = 0; i < nw; ++i) t += red[i];
    return t;
}

template <bool YBF, bool ROWS>
__device__ __forceinline__ void ln_body(const void* __restrict__ y_, const float* __restrict__ resid, const float* __restrict__ w,
                                        const float* __restrict__ b, const float* __restrict__ w2, const float* __restrict__ b2,
                                        float* __restrict__ x_new, bf16_t* __restrict__ c_hi, bf16_t* __restrict__ c_lo,
                                        bf16_t* __restrict__ o_hi, bf16_t* __restrict__ o_lo, const int* __restrict__ pos_p, int R,
                                        int cache_rows, int D, int fmap, float eps) {
    __shared__ float red[8];
    constexpr int MAXI = 4;                         // 4 x 256 threads x 4 elements = 4096
    const int bidx = blockIdx.x, tid = threadIdx.x;
    const size_t row = (size_t)bidx * D;
    float4 v[MAXI];
    float s = 0.f;
#pragma unroll
    for (int it = 0; it < MAXI; ++it) {
        const int e = (tid + it * 256) * 4;
        v[it] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (e < D) {
            if (YBF) {
                const uint2 u = *reinterpret_cast<const uint2*>((const bf16_t*)y_ + row + e);
                v[it] = make_float4(lo_f(u.x), hi_f(u.x), lo_f(u.y), hi_f(u.y));
            } else {
                v[it] = *reinterpret_cast<const float4*>((const float*)y_ + row + e);
            }
            s += (v[it].x + v[it].y) + (v[it].z + v[it].w);
        }
    }
    if (resid) {
        const float mean = block_sum(s, red) / D;
        float q = 0.f;
#pragma unroll
        for (int it = 0; it < MAXI; ++it) {
            const int e = (tid + it * 256) * 4;
            if (e < D) {
                const float a = v[it].x - mean, b_ = v[it].y - mean, c = v[it].z - mean, d = v[it].w - mean;
                q += (a * a + b_ * b_) + (c * c + d * d);
            }
        }
        const float rstd = rsqrtf(block_sum(q, red) / D + eps);
        s = 0.f;
#pragma unroll
        for (int it = 0; it < MAXI; ++it) {
            const int e = (tid + it * 256) * 4;
            if (e < D) {
                const float4 wv = *reinterpret_cast<const float4*>(w + e), bv = *reinterpret_cast<const float4*>(b + e);
                const float4 rv = *reinterpret_cast<const float4*>(resid + row + e);
                v[it] = make_float4(rv.x + ((v[it].x - mean) * rstd * wv.x + bv.x), rv.y + ((v[it].y - mean) * rstd * wv.y + bv.y),
                                    rv.z + ((v[it].z - mean) * rstd * wv.z + bv.z), rv.w + ((v[it].w - mean) * rstd * wv.w + bv.w));
                *reinterpret_cast<float4*>(x_new + row + e) = v[it];
                s += (v[it].x + v[it].y) + (v[it].z + v[it].w);
            }
        }
    }
    if (!w2) return;                                 // last block of the stack: no next pre-norm
    const float mean2 = block_sum(s, red) / D;
    float q2 = 0.f;
#pragma unroll
    for (int it = 0; it < MAXI; ++it) {
        const int e = (tid + it * 256) * 4;
        if (e < D) {
            const float a = v[it].x - mean2, b_ = v[it].y - mean2, c = v[it].z - mean2, d = v[it].w - mean2;
            q2 += (a * a + b_ * b_) + (c * c + d * d);
        }
    }
    const float rstd2 = rsqrtf(block_sum(q2, red) / D + eps);
    int smp = bidx, pos = 0;                         // the cache row: (sample, row of the sample)
    if constexpr (ROWS) {
        smp = bidx / R;
        pos = bidx % R;
    } else if (c_hi) {
        pos = pos_p[0];
        if (pos < 0 || pos >= cache_rows) return;
    }
    const ShiftRule rule(pos, D, fmap);              // (read by the single-row form alone)
    const size_t crow = ((size_t)smp * cache_rows + pos) * D;
#pragma unroll
    for (int it = 0; it < MAXI; ++it) {
        const int e = (tid + it * 256) * 4;
        if (e >= D) continue;
        const float4 wv = *reinterpret_cast<const float4*>(w2 + e), bv = *reinterpret_cast<const float4*>(b2 + e);
        const float h[4] = {(v[it].x - mean2) * rstd2 * wv.x + bv.x, (v[it].y - mean2) * rstd2 * wv.y + bv.y,
                            (v[it].z - mean2) * rstd2 * wv.z + bv.z, (v[it].w - mean2) * rstd2 * wv.w + bv.w};
        bf16_t hh[4], hl[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (o_lo) f2bf_hilo(h[i], hh[i], hl[i]);
            else { hh[i] = f2bf(h[i]); hl[i] = 0; }
        }
        uint2 oh = make_uint2(pack2(hh[0], hh[1]), pack2(hh[2], hh[3])), ol = make_uint2(pack2(hl[0], hl[1]), pack2(hl[2], hl[3]));
        if (c_hi) {
            *reinterpret_cast<uint2*>(c_hi + crow + e) = oh;
            if (c_lo) *reinterpret_cast<uint2*>(c_lo + crow + e) = ol;
            if constexpr (!ROWS) {
                const int back = rule.back(e);       // D % 16 == 0: a 4-element group never straddles a quarter
                if (back >= 0) {
                    const size_t srow = crow - (size_t)back * D;
                    oh = back ? *reinterpret_cast<const uint2*>(c_hi + srow + e) : make_uint2(0u, 0u);
                    ol = (back && c_lo) ? *reinterpret_cast<const uint2*>(c_lo + srow + e) : make_uint2(0u, 0u);
                }
            }
        }
        *reinterpret_cast<uint2*>(o_hi + row + e) = oh;
        if (o_lo) *reinterpret_cast<uint2*>(o_lo + row + e) = ol;
    }
}

template <bool YBF>
__global__ __launch_bounds__(256) void decode_ln_kernel(const void* __restrict__ y_, const float* __restrict__ resid, const float* __restrict__ w,
                                                        const float* __restrict__ b, const float* __restrict__ w2, const float* __restrict__ b2,
                                                        float* __restrict__ x_new, bf16_t* __restrict__ c_hi, bf16_t* __restrict__ c_lo,
                                                        bf16_t* __restrict__ o_hi, bf16_t* __restrict__ o_lo, const int* __restrict__ pos_p,
                                                        int cache_rows, int D, int fmap, float eps) {
    ln_body<YBF, false>(y_, resid, w, b, w2, b2, x_new, c_hi, c_lo, o_hi, o_lo, pos_p, 0, cache_rows, D, fmap, eps);
}

// the rows form: R rows per sample in one launch (its shifted channels: prefill_shift_kernel, below)
template <bool YBF>
__global__ __launch_bounds__(256) void prefill_ln_kernel(const void* __restrict__ y_, const float* __restrict__ resid, const float* __restrict__ w,
                                                         const float* __restrict__ b, const float* __restrict__ w2, const float* __restrict__ b2,
                                                         float* __restrict__ x_new, bf16_t* __restrict__ c_hi, bf16_t* __restrict__ c_lo,
                                                         bf16_t* __restrict__ o_hi, bf16_t* __restrict__ o_lo, int R, int cache_rows, int D, float eps) {
    ln_body<YBF, true>(y_, resid, w, b, w2, b2, x_new, c_hi, c_lo, o_hi, o_lo, nullptr, R, cache_rows, D, 0, eps);
}

// ---- single-query attention pieces shared by the 3DNA and the text cross-attention decode kernels -------------------------
// q . k over DH (multiple of 8) bf16 values, 16 B per load; qrow: fp32 in LDS
template <int DHT>
__device__ __forceinline__ float dot_q_k(const float* qrow, const bf16_t* khi, const bf16_t* klo, int DH) {
    float acc = 0.f;
    if constexpr (DHT > 0) {                           // compile-time width: every 16 B load is in flight before the first FMA
        constexpr int NV = DHT > 0 ? DHT / 8 : 1;
        uint4 h[NV], l[NV];
#pragma unroll
        for (int v = 0; v < DHT / 8; ++v) h[v] = *reinterpret_cast<const uint4*>(khi + v * 8);
        if (klo) {
#pragma unroll
            for (int v = 0; v < DHT / 8; ++v) l[v] = *reinterpret_cast<const uint4*>(klo + v * 8);
        }
#pragma unroll
        for (int v = 0; v < DHT / 8; ++v) {
            float k[8] = {lo_f(h[v].x), hi_f(h[v].x), lo_f(h[v].y), hi_f(h[v].y), lo_f(h[v].z), hi_f(h[v].z), lo_f(h[v].w), hi_f(h[v].w)};
            if (klo) {
                k[0] += lo_f(l[v].x); k[1] += hi_f(l[v].x); k[2] += lo_f(l[v].y); k[3] += hi_f(l[v].y);
                k[4] += lo_f(l[v].z); k[5] += hi_f(l[v].z); k[6] += lo_f(l[v].w); k[7] += hi_f(l[v].w);
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) acc = fmaf(qrow[v * 8 + e], k[e], acc);
        }
        return acc;
    }
    for (int d = 0; d < DH; d += 8) {
        const uint4 h = *reinterpret_cast<const uint4*>(khi + d);
        float k[8] = {lo_f(h.x), hi_f(h.x), lo_f(h.y), hi_f(h.y), lo_f(h.z), hi_f(h.z), lo_f(h.w), hi_f(h.w)};
        if (klo) {
            const uint4 l = *reinterpret_cast<const uint4*>(klo + d);
            k[0] += lo_f(l.x); k[1] += hi_f(l.x); k[2] += lo_f(l.y); k[3] += hi_f(l.y);
            k[4] += lo_f(l.z); k[5] += hi_f(l.z); k[6] += lo_f(l.w); k[7] += hi_f(l.w);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) acc = fmaf(qrow[d + e], k[e], acc);
    }
    return acc;
}

// acc[0 .. 8) += pj * V[off .. off+8): one 16 B load per image
__device__ __forceinline__ void pv_row(float (&acc)[8], float pj, const bf16_t* vhi, const bf16_t* vlo, size_t off) {
    const uint4 h = *reinterpret_cast<const uint4*>(vhi + off);
    float v[8] = {lo_f(h.x), hi_f(h.x), lo_f(h.y), hi_f(h.y), lo_f(h.z), hi_f(h.z), lo_f(h.w), hi_f(h.w)};
    if (vlo) {
        const uint4 l = *reinterpret_cast<const uint4*>(vlo + off);
        v[0] += lo_f(l.x); v[1] += hi_f(l.x); v[2] += lo_f(l.y); v[3] += hi_f(l.y);
        v[4] += lo_f(l.z); v[5] += hi_f(l.z); v[6] += lo_f(l.w); v[7] += hi_f(l.w);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = fmaf(pj, v[e], acc[e]);
}

// out[c0 .. c0+8) += sum over this thread's slots of P'[j] * V_j[c0 .. c0+8): 16 B loads, no branch (masked slots carry
// P' == 0 exactly and point at finite rows), eight loads in flight
template <typename RowOf>
__device__ __forceinline__ void pv_chunk(float (&acc)[8], const float* pmg, const bf16_t* vhi, const bf16_t* vlo, int j0, int jstep,
                                         int J, RowOf row_off) {
#pragma unroll 8
    for (int j = j0; j < J; j += jstep) pv_row(acc, pmg[j], vhi, vlo, row_off(j));
}

// pv_chunk over slots whose rows come from a table (krow[j], < 0 = no row): such a slot is SKIPPED -- its P' is exactly 0 (a mix
// without bias) -- so that no address is ever formed from it; row r starts at r * pitch + col
__device__ __forceinline__ void pv_chunk_tab(float (&acc)[8], const float* pmg, const int* krow, const bf16_t* vhi, const bf16_t* vlo,
                                             int j0, int jstep, int J, size_t pitch, size_t col) {
#pragma unroll 4
    for (int j = j0; j < J; j += jstep) {
        const int r = krow[j];
        if (r >= 0) pv_row(acc, pmg[j], vhi, vlo, (size_t)r * pitch + col);
    }
}

// the slot groups' partial sums meet in LDS: red [ngrp][inner], then one thread per channel writes the output
__device__ __forceinline__ void pv_finish(const float (&acc)[8], float* red, int grp, int ngrp, int c0, int inner, bf16_t* o,
                                          bf16_t* ol, size_t obase) {
    if (grp < ngrp)
#pragma unroll
        for (int e = 0; e < 8; ++e) red[grp * inner + c0 + e] = acc[e];
    __syncthreads();
    for (int c = threadIdx.x; c < inner; c += blockDim.x) {
        float t = 0.f;
        for (int gi = 0; gi < ngrp; ++gi) t += red[gi * inner + c];
        st_hl(o, ol, obase + c, t);
    }
}

// softmax over the J slots of every head (fp32, masked slots -> exactly 0; np.py:554 / 366), one wave per head round-robin;
// then the talking-heads mix pm[g][j] = sum_h W[g,h] P[h][j] (np.py:556-558 / 368-370).  s, pm: [NH][JS] in LDS
__device__ __forceinline__ void softmax_mix(float* s, float* pm, const int* ok, const float* wth, int NH, int J, int JS) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    for (int h = wave; h < NH; h += nw) {
        float m = -3.4028234663852886e38f;
        for (int j = lane; j < J; j += 64) m = fmaxf(m, s[h * JS + j]);
        m = wave_max(m);
        float sum = 0.f;
        for (int j = lane; j < J; j += 64) {
            const float e = ok[j] ? __expf(s[h * JS + j] - m) : 0.f;
            s[h * JS + j] = e;
            sum += e;
        }
        const float inv = 1.f / wave_sum(sum);
        for (int j = lane; j < J; j += 64) s[h * JS + j] *= inv;
    }
    __syncthreads();
    for (int idx = tid; idx < NH * J; idx += blockDim.x) {
        const int g = idx / J, j = idx - g * J;
        float acc = 0.f;
        for (int h = 0; h < NH; ++h) acc = fmaf(wth[g * NH + h], s[h * JS + j], acc);
        pm[g * JS + j] = acc;
    }
    __syncthreads();
}

struct S3DecArgs {
    const bf16_t *qkv, *qkvl;        // new row [B, 3*inner]: q | k | v  (q unscaled)
    bf16_t *kv, *kvl;                // cache [B, cache_rows, 2*inner]: k | v
    bf16_t *o, *ol;                  // [B, inner]
    const float *wth, *rel;
    const int* pos;
    int cache_rows, H, W, kf, kh, kw, df, dh, dw, heads, dim_head, J;
    float scale;
};

// one workgroup (512 threads) per sample.
// LDS: q [NH][DH+1] | s [NH][J] | pm [NH][J] | krow [J] (key row per slot, -1 = masked) | ok [J] | red [4096]
template <int DHT>
__global__ __launch_bounds__(512) void s3_decode_kernel(S3DecArgs a) {
    extern __shared__ float sm[];
    const int inner = a.heads * a.dim_head, J = a.J, NH = a.heads, DH = a.dim_head, QS = DH + 1;
    float* qs = sm;
    float* s = qs + NH * QS;
    float* pm = s + NH * J;
    int* krow = reinterpret_cast<int*>(pm + NH * J);
    int* ok = krow + J;
    const int b = blockIdx.x, tid = threadIdx.x, pos = a.pos[0];
    if (pos < 0 || pos >= a.cache_rows) return;
    const size_t nrow = (size_t)b * 3 * inner;
    bf16_t* kvb = a.kv + (size_t)b * a.cache_rows * 2 * inner;
    bf16_t* kvlb = a.kvl ? a.kvl + (size_t)b * a.cache_rows * 2 * inner : nullptr;
    // 1. the new key / value row joins the cache
    for (int c = tid; c < 2 * inner; c += blockDim.x) {
        kvb[(size_t)pos * 2 * inner + c] = a.qkv[nrow + inner + c];
        if (kvlb) kvlb[(size_t)pos * 2 * inner + c] = a.qkvl[nrow + inner + c];
    }
    if (pos == 0) {                  // <bos> query: its output is its own value row (np.py:499, 608)
        for (int c = tid; c < inner; c += blockDim.x) {
            a.o[(size_t)b * inner + c] = a.qkv[nrow + 2 * inner + c];
            if (a.ol) a.ol[(size_t)b * inner + c] = a.qkvl ? a.qkvl[nrow + 2 * inner + c] : (bf16_t)0;
        }
        return;
    }
    for (int c = tid; c < inner; c += blockDim.x) qs[(c / DH) * QS + c % DH] = ld_hl(a.qkv, a.qkvl, nrow + c) * a.scale;
    // 2. key row of every slot: slot 0 is <bos>, slot 1 + (ta, tb, tc) the causal tap (np.py:420-457)
    const int p = pos - 1, w0 = p % a.W, y0 = (p / a.W) % a.H, f0 = p / (a.W * a.H);
    for (int j = tid; j < J; j += blockDim.x) {
        int r = 0;
        if (j > 0) {
            const int t = j - 1, tc = t % a.kw, tb = (t / a.kw) % a.kh, ta = t / (a.kw * a.kh);
            const int ff = f0 - (a.kf - 1 - ta) * a.df, yy = y0 - (a.kh - 1 - tb) * a.dh, ww = w0 - (a.kw - 1 - tc) * a.dw;
            r = (ff < 0 || yy < 0 || ww < 0) ? -1 : 1 + (ff * a.H + yy) * a.W + ww;
        }
        krow[j] = r;
        ok[j] = r >= 0;
    }
    __syncthreads();
    // 3. scores (fp32): consecutive threads take the heads of one key row (contiguous 2 * DH bytes each)
    for (int idx = tid; idx < NH * J; idx += blockDim.x) {
        const int j = idx / NH, h = idx - j * NH, r = krow[j];
        float sc = -3.4028234663852886e38f;
        if (r >= 0) {
            const size_t base = (size_t)r * 2 * inner + (size_t)h * DH;
            sc = dot_q_k<DHT>(qs + h * QS, kvb + base, kvlb ? kvlb + base : nullptr, DH) + ((a.rel && j > 0) ? a.rel[(size_t)j * NH + h] : 0.f);
        }
        s[h * J + j] = sc;
    }
    __syncthreads();
    softmax_mix(s, pm, ok, a.wth, NH, J, J);
    // 4. o[g] = sum_j P'[g, j] v_j[g]: thread = (8-channel chunk, slot group)
    {
        const int nchunk = inner / 8, ngrp = blockDim.x / nchunk;
        const int ch = tid % nchunk, grp = tid / nchunk, c0 = ch * 8, g = c0 / DH;
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (grp < ngrp)
            pv_chunk(acc, pm + g * J, kvb, kvlb, grp, ngrp, J,
                     [&](int j) { return (size_t)max(krow[j], 0) * 2 * inner + inner + c0; });
        pv_finish(acc, reinterpret_cast<float*>(ok + J), grp, ngrp, c0, inner, a.o, a.ol, (size_t)b * inner);
    }
}

struct XDecArgs {
    const bf16_t *q, *ql;            // [B, ldq] unscaled
    const bf16_t *Kp, *Kpl, *Vp, *Vpl;   // [B][NH][JP][DH]
    const uint8_t* valid;            // [B][JP]
    bf16_t *o, *ol;                  // [B, ldo]
    const float* wth;
    int ldq, ldo, J, JP, heads, dim_head;
    float scale;
};

// text cross-attention of ONE query per sample (Attention.forward with context, np.py:339-378): null key at slot 0, key mask,
// fp32 softmax, talking heads; 1024 threads per sample (the work is a chain of memory latencies: width hides them).
// LDS: q [NH][DH+1] | s [NH][J] | pm [NH][J] | ok [J] | red [8192]
template <int DHT>
__global__ __launch_bounds__(1024) void xattn_decode_kernel(XDecArgs a) {
    extern __shared__ float sm[];
    const int NH = a.heads, DH = a.dim_head, J = a.J, JP = a.JP, inner = NH * DH, QS = DH + 1;
    float* qs = sm;
    float* s = qs + NH * QS;
    float* pm = s + NH * J;
    int* ok = reinterpret_cast<int*>(pm + NH * J);
    const int b = blockIdx.x, tid = threadIdx.x;
    for (int c = tid; c < inner; c += blockDim.x) qs[(c / DH) * QS + c % DH] = ld_hl(a.q, a.ql, (size_t)b * a.ldq + c) * a.scale;
    for (int j = tid; j < J; j += blockDim.x) ok[j] = a.valid[(size_t)b * JP + j] != 0;
    __syncthreads();
    const size_t kb = (size_t)b * NH * JP * DH;
    for (int idx = tid; idx < NH * J; idx += blockDim.x) {       // consecutive threads: consecutive key rows of one head
        const int h = idx / J, j = idx - h * J;
        float sc = -3.4028234663852886e38f;
        if (ok[j]) {
            const size_t base = kb + ((size_t)h * JP + j) * DH;
            sc = dot_q_k<DHT>(qs + h * QS, a.Kp + base, a.Kpl ? a.Kpl + base : nullptr, DH);
        }
        s[h * J + j] = sc;
    }
    __syncthreads();
    softmax_mix(s, pm, ok, a.wth, NH, J, J);
    // o[g][d] = sum_j P'[g][j] V[g][j][d]: thread = (8-channel chunk, slot group)
    {
        const int nchunk = inner / 8, ngrp = blockDim.x / nchunk;
        const int ch = tid % nchunk, grp = tid / nchunk, c0 = ch * 8, g = c0 / DH, d = c0 - g * DH;
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        const size_t vb = kb + (size_t)g * JP * DH + d;
        if (grp < ngrp) pv_chunk(acc, pm + g * J, a.Vp, a.Vpl, grp, ngrp, J, [&](int j) { return vb + (size_t)j * DH; });
        pv_finish(acc, reinterpret_cast<float*>(ok + J), grp, ngrp, c0, inner, a.o, a.ol, (size_t)b * a.ldo);
    }
}

// ---- single-query attention over ANY number of cached rows (Attention / CrossModalityCrossAttention, np.py:339-378, 908-1067) ----
// The keys of a sample are cut into splits of ROWS_SPLIT slots (slot 0 = the learned null key, slot 1 + t = cache row first + t), one
// workgroup per (split, sample).  The talking-heads mix sits between the softmax and P.V, so a split cannot finish on its own maximum:
//   rows_stats_kernel  : scores of the split (kept in the workspace, [B][J][NH] fp32) and its per-head (max, sum of exponentials)
//   rows_apply_kernel  : merges the statistics of all splits IN INDEX ORDER, P = exp(s - M) / Z, P' = W P + bias, partial o of the split
//   rows_reduce_kernel : sums the partial rows in index order and rounds the output
// No atomics, the split count depends on T alone: two runs are bit-identical.  The first row comes from device memory (graph replay).
//
// The three kernels are templated on the slot -> cache-row mapping.  TAB = false is the contiguous window above.  TAB = true serves
// SparseCross2DNA (np.py:761-901) for the query of decoder row pos (device memory, >= 1): slot 1 + t is context row tab[i][t] of the sample,
// i = (pos - 1) mod n_pos the query's feature-map position; a negative entry is 'same' padding -- hidden, never turned into an address --
// and the key mask is indexed by context row.  Every workgroup reads the table row of i ONCE, keeps its own split's entries in LDS and
// checks all of them against cache_rows on the way, so that all workgroups of the three launches agree on whether anything is written.
//
// Both mappings have a ROWS FORM (RowsArgs::R > 0): the launch serves R query rows of every sample at once, the cache prefill of a sliding
// generate() window.  TAB (amdnuwa_cross2dna_rows, NUWASketch): rows 1 .. R-1, each at its own decoder row.  Contiguous window
// (amdnuwa_attn_rows, text cross-attention over a long context): rows 0 .. R-1, all on the window at the device-side first row.  Only the
// bookkeeping differs -- which sample's context, which q / o row, which workspace row and (TAB) which decoder row a workgroup serves come
// from blockIdx.x (rows_who) instead of (blockIdx.y, the device-side position); the loads, the expression trees, the 128-slot splits and the
// order in which partial results meet are the single row's own code, so row (b, r) is bit-identical to the single-row launch on q[b * R + r]
// (TAB: at pos = r).
constexpr int ROWS_SPLIT = 128;
constexpr int ROWS_CHUNK = 2048;     // rows form: queries per set of three launches (bounds the workspace, not the result)
constexpr float ROWS_NEG = -3.4028234663852886e38f;

struct RowsArgs {
    const bf16_t *q, *ql;            // [B, ldq] unscaled
    const bf16_t *kv, *kvl;          // [B, cache_rows, 2*inner]: k | v
    const int* first;                // device: cache row of slot 1
    const uint8_t* mask;             // [B, T] (TAB: [B, cache_rows], by context row) or NULL
    const float *nk, *nv, *wth, *bias;
    bf16_t *o, *ol;                  // [B, ldo]
    float *sc, *st, *part;           // workspace: scores [B][J][NH] | stats [B][nsplit][NH][2] | partial rows [B][nsplit][inner]
    int ldq, ldo, cache_rows, T, heads, dim_head, nsplit;
    float scale;
    const int* tab;                  // TAB: [n_pos][T] cache row of every slot, < 0 = padding; `first` then holds the decoder row
    int n_pos;
    int R, u0;                       // rows form (R > 0; 0 = one row per sample): blockIdx.x counts (query, split) from query u0 on.  TAB: query u =
};                                   // sample u / (R-1), decoder row 1 + u % (R-1), `first` is not read; window: sample u / R, q / o row u

// what a workgroup serves: split sp of the query at row qr of q / o, which belongs to sample b (kv, mask) and keeps its scores, statistics
// and partial rows in workspace row wr; pos = its decoder row in the rows form, -1 = read the device-side one
struct RowsWho { int sp, b, qr, wr, pos; };

template <bool TAB>
__device__ __forceinline__ RowsWho rows_who(const RowsArgs& a, bool reduce) {
    RowsWho w;
    if (a.R > 0) {
        const int ul = reduce ? (int)blockIdx.x : (int)blockIdx.x / a.nsplit, u = a.u0 + ul;
        w.sp = reduce ? 0 : (int)blockIdx.x - ul * a.nsplit;
        if constexpr (TAB) {
            w.b = u / (a.R - 1);
            w.pos = 1 + u - w.b * (a.R - 1);
            w.qr = w.b * a.R + w.pos;
        } else {                     // every row of a sample attends the window at the device-side first row
            w.b = u / a.R;
            w.pos = -1;
            w.qr = u;
        }
        w.wr = ul;
    } else {
        w.sp = reduce ? 0 : (int)blockIdx.x;
        w.b = w.qr = w.wr = reduce ? (int)blockIdx.x : (int)blockIdx.y;
        w.pos = -1;
    }
    return w;
}

__device__ __forceinline__ bool rows_window_ok(const RowsArgs& a, int first) {
    return first >= 0 && (long long)first + a.T <= (long long)a.cache_rows;
}

// first <- the device-side row (pos < 0) or pos; false (for every thread of every workgroup that serves this query alike): nothing is written.
// TAB: krow[j] <- the cache row of slot j0 + j for j < Jl (-1 for the null key's slot 0), visible to the whole workgroup on return
template <bool TAB>
__device__ __forceinline__ bool rows_begin(const RowsArgs& a, int* krow, int j0, int Jl, int pos, int& first) {
    first = pos < 0 ? a.first[0] : pos;
    if constexpr (!TAB) {
        return rows_window_ok(a, first);
    } else {
        if (first < 1) return false;
        const int* tab = a.tab + (size_t)((first - 1) % a.n_pos) * a.T;
        int bad = 0;
        for (int t = threadIdx.x; t < a.T; t += blockDim.x) {        // consecutive threads, consecutive entries
            const int r = tab[t], j = t + 1 - j0;
            bad |= r >= a.cache_rows;
            if (j >= 0 && j < Jl) krow[j] = r;
        }
        if (j0 == 0 && Jl > 0 && threadIdx.x == 0) krow[0] = -1;
        return __syncthreads_or(bad) == 0;
    }
}

// is slot j0 + j of sample b visible?  slot 0, the null key, always is
template <bool TAB>
__device__ __forceinline__ bool rows_slot_ok(const RowsArgs& a, const int* krow, int b, int j0, int j) {
    const int jg = j0 + j;
    if constexpr (TAB) return jg == 0 || (krow[j] >= 0 && (!a.mask || a.mask[(size_t)b * a.cache_rows + krow[j]] != 0));
    else return jg == 0 || !a.mask || a.mask[(size_t)b * a.T + jg - 1] != 0;
}

template <int DHT, bool TAB>
__global__ __launch_bounds__(256) void rows_stats_kernel(RowsArgs a) {
    __shared__ float qs[8 * 65];
    __shared__ float s[8 * ROWS_SPLIT];
    __shared__ int ok[ROWS_SPLIT];
    __shared__ int krow[ROWS_SPLIT];
    const int NH = a.heads, DH = a.dim_head, inner = NH * DH, QS = DH + 1, J = a.T + 1;
    const RowsWho who = rows_who<TAB>(a, false);
    const int sp = who.sp, b = who.b, wr = who.wr, tid = threadIdx.x;
    const int j0 = sp * ROWS_SPLIT, Jl = min(ROWS_SPLIT, J - j0);
    int first;
    if (!rows_begin<TAB>(a, krow, j0, Jl, who.pos, first)) return;
    for (int c = tid; c < inner; c += blockDim.x) qs[(c / DH) * QS + c % DH] = ld_hl(a.q, a.ql, (size_t)who.qr * a.ldq + c) * a.scale;
    for (int j = tid; j < Jl; j += blockDim.x) ok[j] = rows_slot_ok<TAB>(a, krow, b, j0, j);
    __syncthreads();
    const size_t kvb = (size_t)b * a.cache_rows * 2 * inner;
    for (int idx = tid; idx < NH * Jl; idx += blockDim.x) {       // consecutive threads: the heads of one key row (contiguous)
        const int j = idx / NH, h = idx - j * NH, jg = j0 + j;
        float sc = ROWS_NEG;
        if (ok[j]) {
            if (jg == 0) {
                sc = 0.f;
                for (int d = 0; d < DH; ++d) sc = fmaf(qs[h * QS + d], a.nk[h * DH + d], sc);
            } else {
                const size_t row = TAB ? (size_t)krow[j] : (size_t)(first + jg - 1);
                const size_t base = kvb + row * 2 * inner + (size_t)h * DH;
                sc = dot_q_k<DHT>(qs + h * QS, a.kv + base, a.kvl ? a.kvl + base : nullptr, DH);
            }
        }
        s[h * ROWS_SPLIT + j] = sc;
        a.sc[((size_t)wr * J + jg) * NH + h] = sc;
    }
    __syncthreads();
    const int lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    for (int h = wave; h < NH; h += nw) {
        float m = ROWS_NEG;
        for (int j = lane; j < Jl; j += 64) m = fmaxf(m, s[h * ROWS_SPLIT + j]);
        m = wave_max(m);
        float sum = 0.f;
        for (int j = lane; j < Jl; j += 64) sum += ok[j] ? __expf(s[h * ROWS_SPLIT + j] - m) : 0.f;
        sum = wave_sum(sum);
        if (lane == 0) {
            float* st = a.st + (((size_t)wr * a.nsplit + sp) * NH + h) * 2;
            st[0] = m;
            st[1] = sum;
        }
    }
}

template <bool TAB>
__global__ __launch_bounds__(256) void rows_apply_kernel(RowsArgs a) {
    __shared__ float pr[8 * ROWS_SPLIT];
    __shared__ float pm[8 * ROWS_SPLIT];
    __shared__ float red[2048];                                   // [slot group][inner]: 256 / (inner / 8) groups
    __shared__ float mz[16];
    __shared__ int ok[ROWS_SPLIT];
    __shared__ int krow[ROWS_SPLIT];
    const int NH = a.heads, DH = a.dim_head, inner = NH * DH, J = a.T + 1;
    const RowsWho who = rows_who<TAB>(a, false);
    const int sp = who.sp, b = who.b, wr = who.wr, tid = threadIdx.x;
    const int j0 = sp * ROWS_SPLIT, Jl = min(ROWS_SPLIT, J - j0);
    int first;
    if (!rows_begin<TAB>(a, krow, j0, Jl, who.pos, first)) return;
    if (tid < NH) {                                               // the statistics of all splits meet in index order (eight loads in
        const float* st = a.st + ((size_t)wr * a.nsplit * NH + tid) * 2;   // flight at a time: one thread walks a chain of latencies)
        float M = ROWS_NEG;
        for (int i0 = 0; i0 < a.nsplit; i0 += 8) {
            float mv[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) mv[k] = i0 + k < a.nsplit ? st[(size_t)(i0 + k) * NH * 2] : ROWS_NEG;
#pragma unroll
            for (int k = 0; k < 8; ++k) M = fmaxf(M, mv[k]);
        }
        float Z = 0.f;
        for (int i0 = 0; i0 < a.nsplit; i0 += 8) {
            float mv[8], zv[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const bool in = i0 + k < a.nsplit;
                mv[k] = in ? st[(size_t)(i0 + k) * NH * 2] : ROWS_NEG;
                zv[k] = in ? st[(size_t)(i0 + k) * NH * 2 + 1] : 0.f;
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) Z = fmaf(zv[k], __expf(mv[k] - M), Z);
        }
        mz[tid] = M;
        mz[8 + tid] = 1.f / Z;                                    // (the null key is always visible: Z >= 1 term)
    }
    for (int j = tid; j < Jl; j += blockDim.x) ok[j] = rows_slot_ok<TAB>(a, krow, b, j0, j);
    __syncthreads();
    for (int idx = tid; idx < NH * Jl; idx += blockDim.x) {
        const int j = idx / NH, h = idx - j * NH;
        const float sv = a.sc[((size_t)wr * J + j0 + j) * NH + h];
        pr[h * ROWS_SPLIT + j] = ok[j] ? __expf(sv - mz[h]) * mz[8 + h] : 0.f;
    }
    __syncthreads();
    // talking heads + the Conv3d bias, which reaches EVERY slot (null and masked ones included), as the reference's biased mix does
    for (int idx = tid; idx < NH * Jl; idx += blockDim.x) {
        const int g = idx / Jl, j = idx - g * Jl;
        float acc = 0.f;
        for (int h = 0; h < NH; ++h) acc = fmaf(a.wth[g * NH + h], pr[h * ROWS_SPLIT + j], acc);
        pm[g * ROWS_SPLIT + j] = a.bias ? acc + a.bias[g] : acc;
    }
    __syncthreads();
    const int nchunk = inner / 8, ngrp = blockDim.x / nchunk;
    const int ch = tid % nchunk, grp = tid / nchunk, c0 = ch * 8, g = c0 / DH;
    const int off = sp == 0 ? 1 : 0;                              // slot 0 is the fp32 null value, added below
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (grp < ngrp) {
        const bf16_t* vb = a.kv + (size_t)b * a.cache_rows * 2 * inner;
        const bf16_t* vlb = a.kvl ? a.kvl + (size_t)b * a.cache_rows * 2 * inner : nullptr;
        if constexpr (TAB) {
            pv_chunk_tab(acc, pm + g * ROWS_SPLIT + off, krow + off, vb, vlb, grp, ngrp, Jl - off, (size_t)2 * inner, (size_t)(inner + c0));
        } else {
            const size_t r0 = (size_t)(first + j0 + off - 1);
            pv_chunk(acc, pm + g * ROWS_SPLIT + off, vb, vlb, grp, ngrp, Jl - off, [&](int j) { return (r0 + j) * 2 * inner + inner + c0; });
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) red[grp * inner + c0 + e] = acc[e];
    }
    __syncthreads();
    for (int c = tid; c < inner; c += blockDim.x) {
        float t = 0.f;
        for (int gi = 0; gi < ngrp; ++gi) t += red[gi * inner + c];
        if (sp == 0) t = fmaf(pm[(c / DH) * ROWS_SPLIT], a.nv[c], t);
        a.part[((size_t)wr * a.nsplit + sp) * inner + c] = t;
    }
}

template <bool TAB>
__global__ __launch_bounds__(256) void rows_reduce_kernel(RowsArgs a) {
    const int inner = a.heads * a.dim_head;
    const RowsWho who = rows_who<TAB>(a, true);
    int first;
    if (!rows_begin<TAB>(a, nullptr, 0, 0, who.pos, first)) return;
    for (int c = threadIdx.x; c < inner; c += blockDim.x) {
        const float* part = a.part + (size_t)who.wr * a.nsplit * inner + c;
        float t = 0.f;
        for (int i0 = 0; i0 < a.nsplit; i0 += 8) {                // index order, eight loads in flight
            float pv[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) pv[k] = i0 + k < a.nsplit ? part[(size_t)(i0 + k) * inner] : 0.f;
#pragma unroll
            for (int k = 0; k < 8; ++k) t += pv[k];
        }
        st_hl(a.o, a.ol, (size_t)who.qr * a.ldo + c, t);
    }
}

// ---- cache prefill: the norms, the token shift and the key / value rows of R rows per sample at once --------------------------
// When generate() slides its frame window every kept token moves one frame earlier, so every cached row changes.  The kept rows are
// recomputed in ONE full-sequence pass; these kernels leave the caches exactly as R single-row steps at pos = 0 .. R-1 would have.
//
// The norms are prefill_ln_kernel, the ROWS form of ln_body above: a row is bit-identical to the row step's because it runs the row
// step's own code.
//
// prefill_shift_kernel: the shifted half of out [B*R, D] from the cache rows a finished prefill_ln launch wrote (ShiftRule says from which):
// one thread per vector V (16 bytes, or 8 when a channel quarter is no multiple of 8 elements) of the first D / 2 channels of a row,
// consecutive threads on consecutive vectors.
template <typename V> __device__ __forceinline__ V vec_zero();
template <> __device__ __forceinline__ uint4 vec_zero<uint4>() { return make_uint4(0u, 0u, 0u, 0u); }
template <> __device__ __forceinline__ uint2 vec_zero<uint2>() { return make_uint2(0u, 0u); }

template <typename V>
__global__ __launch_bounds__(256) void prefill_shift_kernel(const bf16_t* __restrict__ c_hi, const bf16_t* __restrict__ c_lo,
                                                            bf16_t* __restrict__ o_hi, bf16_t* __restrict__ o_lo, int B, int R,
                                                            int cache_rows, int D, int fmap) {
    constexpr int EV = sizeof(V) / sizeof(bf16_t);
    const int per_row = (D >> 1) / EV;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)B * R * per_row) return;
    const int e = (int)(idx % per_row) * EV;
    const size_t r = idx / per_row;
    const int i = (int)(r % R), smp = (int)(r / R);
    const int back = ShiftRule(i, D, fmap).back(e);
    if (back < 0) return;                            // <bos> of a video map is not shifted: out keeps h
    const size_t src = ((size_t)smp * cache_rows + (i - back)) * D + e, dst = r * D + e;
    if (back) {
        *reinterpret_cast<V*>(o_hi + dst) = *reinterpret_cast<const V*>(c_hi + src);
        if (o_lo) *reinterpret_cast<V*>(o_lo + dst) = *reinterpret_cast<const V*>(c_lo + src);
    } else {
        *reinterpret_cast<V*>(o_hi + dst) = vec_zero<V>();
        if (o_lo) *reinterpret_cast<V*>(o_lo + dst) = vec_zero<V>();
    }
}

// k | v columns of qkv [B*R, 3*inner] -> rows [0, R) of kv [B, cache_rows, 2*inner]: one 16-byte vector per thread, consecutive
// threads on consecutive vectors of a row (inner % 8 == 0: both the column offset and the row pitches are multiples of 16 bytes)
__global__ __launch_bounds__(256) void prefill_kv_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ qkvl,
                                                         bf16_t* __restrict__ kv, bf16_t* __restrict__ kvl, int B, int R,
                                                         int cache_rows, int inner) {
    const int per_row = inner >> 2;                  // 2 * inner / 8
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)B * R * per_row) return;
    const int c = (int)(idx % per_row) * 8;
    const size_t r = idx / per_row;
    const size_t src = r * 3 * inner + inner + c, dst = ((r / R) * cache_rows + r % R) * 2 * inner + c;
    *reinterpret_cast<uint4*>(kv + dst) = *reinterpret_cast<const uint4*>(qkv + src);
    if (kvl) *reinterpret_cast<uint4*>(kvl + dst) = *reinterpret_cast<const uint4*>(qkvl + src);
}

size_t rows_ws_floats(int B, int T, int heads, int dim_head, int& nsplit) {
    nsplit = (T + 1 + ROWS_SPLIT - 1) / ROWS_SPLIT;
    return (size_t)B * ((size_t)heads * (T + 1) + (size_t)nsplit * (2 * heads + heads * dim_head));
}

// the three launches of one single-query attention: one workgroup per (split, sample), then one per sample; the rows form (a.R > 0)
// counts B queries from a.u0 on, (query, split) on the x dimension -- the y dimension ends at 65 535
template <bool TAB>
void rows_launch(const RowsArgs& a, int B, hipStream_t stream) {
    const dim3 grid = a.R > 0 ? dim3((unsigned)a.nsplit * B) : dim3(a.nsplit, B);
    if (a.dim_head == 64) hipLaunchKernelGGL((rows_stats_kernel<64, TAB>), grid, dim3(256), 0, stream, a);
    else hipLaunchKernelGGL((rows_stats_kernel<32, TAB>), grid, dim3(256), 0, stream, a);
    hipLaunchKernelGGL((rows_apply_kernel<TAB>), grid, dim3(256), 0, stream, a);
    hipLaunchKernelGGL((rows_reduce_kernel<TAB>), dim3(B), dim3(256), 0, stream, a);
}

// ---- what the four attention entry points share.  Each keeps its own B / R checks, says what `first` holds, and sets tab / n_pos / R ----
RowsArgs rows_args(int T, int heads, int dim_head, float scale, const uint16_t* q, const uint16_t* q_lo, int ldq, const uint16_t* kv,
                   const uint16_t* kv_lo, int cache_rows, const int* first, const uint8_t* mask, const float* nk, const float* nv,
                   const float* wth, const float* bias, uint16_t* o, uint16_t* o_lo, int ldo) {
    RowsArgs a{};
    a.q = q; a.ql = q_lo; a.kv = kv; a.kvl = kv_lo; a.first = first; a.mask = mask; a.nk = nk; a.nv = nv;
    a.wth = wth; a.bias = bias; a.o = o; a.ol = o_lo; a.ldq = ldq; a.ldo = ldo; a.cache_rows = cache_rows; a.T = T;
    a.heads = heads; a.dim_head = dim_head; a.scale = scale;
    return a;
}

// the argument checks (AMDNUWA_OK = pass).  TAB: the rows come from a.tab, else from the window at a.first.  amdnuwa_attn_decode_rows
// alone passes lo_agree = false (it never required q_lo / kv_lo / o_lo to agree) and unsupported_first = true (it reports
// ERR_UNSUPPORTED before it looks at the pitches).
template <bool TAB>
int rows_check(const RowsArgs& a, bool lo_agree, bool unsupported_first) {
    if (!a.q || !a.kv || !a.nk || !a.nv || !a.wth || !a.o || a.T < 1 || a.heads <= 0 || a.dim_head <= 0) return AMDNUWA_ERR_ARG;
    if (TAB ? (!a.tab || a.cache_rows <= 0 || a.n_pos <= 0) : (!a.first || a.cache_rows < a.T)) return AMDNUWA_ERR_ARG;
    if (lo_agree && ((a.ql != nullptr) != (a.kvl != nullptr) || (a.ql != nullptr) != (a.ol != nullptr))) return AMDNUWA_ERR_ARG;
    const bool unsupported = a.heads > 8 || (a.dim_head != 32 && a.dim_head != 64);
    if (unsupported && unsupported_first) return AMDNUWA_ERR_UNSUPPORTED;
    const long long inner = (long long)a.heads * a.dim_head;
    if (a.ldq < inner || a.ldo < inner) return AMDNUWA_ERR_ARG;
    return unsupported ? AMDNUWA_ERR_UNSUPPORTED : AMDNUWA_OK;
}

// carves the workspace (scores | stats | partial rows of ws_rows queries) and launches: `total` queries, at once (a.R == 0) or in chunks of
// at most ROWS_CHUNK that share the workspace -- the launches of a stream run in order
template <bool TAB>
int rows_run(RowsArgs& a, int ws_rows, int total, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    const size_t nf = rows_ws_floats(ws_rows, a.T, a.heads, a.dim_head, a.nsplit);
    if (!workspace || workspace_bytes < nf * sizeof(float)) return AMDNUWA_ERR_WORKSPACE;
    a.sc = static_cast<float*>(workspace);
    a.st = a.sc + (size_t)ws_rows * a.heads * (a.T + 1);
    a.part = a.st + (size_t)ws_rows * a.nsplit * a.heads * 2;
    if (a.R > 0)
        for (a.u0 = 0; a.u0 < total; a.u0 += ROWS_CHUNK) rows_launch<TAB>(a, total - a.u0 < ROWS_CHUNK ? total - a.u0 : ROWS_CHUNK, stream);
    else
        rows_launch<TAB>(a, total, stream);
    LAUNCH_CHECK();
    return AMDNUWA_OK;
}

// queries whose scores, statistics and partial rows a rows form keeps at a time: one chunk's (B, R > 0)
int rows_ws_rows(int B, int R) {
    const long long rows = (long long)B * R;
    return (int)(rows < ROWS_CHUNK ? rows : ROWS_CHUNK);
}

}  // namespace

extern "C" size_t amdnuwa_attn_decode_rows_workspace_bytes(int B, int T, int heads, int dim_head) {
    if (B <= 0 || T < 1 || heads <= 0 || dim_head <= 0) return 0;
    int nsplit;
    return rows_ws_floats(B, T, heads, dim_head, nsplit) * sizeof(float);
}

extern "C" int amdnuwa_attn_decode_rows(int B, int T, int heads, int dim_head, float scale, const uint16_t* q, const uint16_t* q_lo,
                                        int ldq, const uint16_t* kv, const uint16_t* kv_lo, int cache_rows, const int* first_row,
                                        const uint8_t* key_mask, const float* null_k, const float* null_v, const float* w_th,
                                        const float* th_bias, uint16_t* o, uint16_t* o_lo, int ldo, void* workspace,
                                        size_t workspace_bytes, hipStream_t stream) {
    RowsArgs a = rows_args(T, heads, dim_head, scale, q, q_lo, ldq, kv, kv_lo, cache_rows, first_row, key_mask, null_k, null_v, w_th,
                           th_bias, o, o_lo, ldo);
    if (const int bad = rows_check<false>(a, /*lo_agree=*/false, /*unsupported_first=*/true)) return bad;
    if (B <= 0) return AMDNUWA_OK;                                                // an empty batch, once its arguments are valid
    return rows_run<false>(a, B, B, workspace, workspace_bytes, stream);
}

extern "C" size_t amdnuwa_attn_rows_workspace_bytes(int B, int R, int T, int heads, int dim_head) {
    return B <= 0 || R <= 0 ? 0 : amdnuwa_attn_decode_rows_workspace_bytes(rows_ws_rows(B, R), T, heads, dim_head);
}

extern "C" int amdnuwa_attn_rows(int B, int R, int T, int heads, int dim_head, float scale, const uint16_t* q, const uint16_t* q_lo, int ldq,
                                 const uint16_t* kv, const uint16_t* kv_lo, int cache_rows, const int* first_row, const uint8_t* key_mask,
                                 const float* null_k, const float* null_v, const float* w_th, const float* th_bias, uint16_t* o,
                                 uint16_t* o_lo, int ldo, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    if (B <= 0 || R <= 0 || (long long)B * R > 0x7fffffffLL) return AMDNUWA_ERR_ARG;   // (the q / o row index is an int)
    RowsArgs a = rows_args(T, heads, dim_head, scale, q, q_lo, ldq, kv, kv_lo, cache_rows, first_row, key_mask, null_k, null_v, w_th,
                           th_bias, o, o_lo, ldo);
    a.R = R;
    if (const int bad = rows_check<false>(a, /*lo_agree=*/true, /*unsupported_first=*/false)) return bad;
    return rows_run<false>(a, rows_ws_rows(B, R), B * R, workspace, workspace_bytes, stream);
}

extern "C" size_t amdnuwa_cross2dna_decode_workspace_bytes(int B, int J, int heads, int dim_head) {
    return amdnuwa_attn_decode_rows_workspace_bytes(B, J, heads, dim_head);
}

extern "C" int amdnuwa_cross2dna_decode(int B, int J, int heads, int dim_head, float scale, const uint16_t* q, const uint16_t* q_lo, int ldq,
                                        const uint16_t* kv, const uint16_t* kv_lo, int ctx_rows, const int* slot_rows, int n_pos,
                                        const int* pos, const uint8_t* key_mask, const float* null_k, const float* null_v,
                                        const float* w_th, uint16_t* o, uint16_t* o_lo, int ldo, void* workspace, size_t workspace_bytes,
                                        hipStream_t stream) {
    if (B <= 0 || !pos) return AMDNUWA_ERR_ARG;
    RowsArgs a = rows_args(J, heads, dim_head, scale, q, q_lo, ldq, kv, kv_lo, ctx_rows, pos, key_mask, null_k, null_v, w_th, nullptr, o,
                           o_lo, ldo);                                            // (`first` holds the decoder row)
    a.tab = slot_rows; a.n_pos = n_pos;
    if (const int bad = rows_check<true>(a, /*lo_agree=*/true, /*unsupported_first=*/false)) return bad;
    return rows_run<true>(a, B, B, workspace, workspace_bytes, stream);
}

extern "C" size_t amdnuwa_cross2dna_rows_workspace_bytes(int B, int R, int J, int heads, int dim_head) {
    return B <= 0 || R <= 0 ? 0 : amdnuwa_attn_decode_rows_workspace_bytes(rows_ws_rows(B, R), J, heads, dim_head);
}

extern "C" int amdnuwa_cross2dna_rows(int B, int R, int J, int heads, int dim_head, float scale, const uint16_t* q, const uint16_t* q_lo,
                                      int ldq, const uint16_t* kv, const uint16_t* kv_lo, int ctx_rows, const int* slot_rows, int n_pos,
                                      const uint8_t* key_mask, const float* null_k, const float* null_v, const float* w_th, uint16_t* o,
                                      uint16_t* o_lo, int ldo, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    if (B <= 0 || R <= 0 || (long long)B * R > 0x7fffffffLL) return AMDNUWA_ERR_ARG;   // (the q / o row index is an int)
    RowsArgs a = rows_args(J, heads, dim_head, scale, q, q_lo, ldq, kv, kv_lo, ctx_rows, nullptr, key_mask, null_k, null_v, w_th, nullptr,
                           o, o_lo, ldo);                                         // (`first` is not read: row r is at decoder row r)
    a.tab = slot_rows; a.n_pos = n_pos; a.R = R;
    if (const int bad = rows_check<true>(a, /*lo_agree=*/true, /*unsupported_first=*/false)) return bad;
    if (R == 1) return AMDNUWA_OK;                                                // <bos> alone: the caller's row, nothing to launch
    return rows_run<true>(a, rows_ws_rows(B, R), B * (R - 1), workspace, workspace_bytes, stream);   // (the workspace is sized by B * R)
}

extern "C" int amdnuwa_decode_shift(const uint16_t* h_hi, const uint16_t* h_lo, uint16_t* cache_hi, uint16_t* cache_lo,
                                    uint16_t* out_hi, uint16_t* out_lo, const int* pos, int B, int cache_rows, int D,
                                    int fmap, hipStream_t stream) {
    if (!h_hi || !cache_hi || !out_hi || !pos || D <= 0 || D % 4 || fmap <= 0 || cache_rows <= 0) return AMDNUWA_ERR_ARG;
    if ((h_lo != nullptr) != (cache_lo != nullptr) || (out_lo && !h_lo)) return AMDNUWA_ERR_ARG;
    if (B <= 0) return AMDNUWA_OK;
    hipLaunchKernelGGL(decode_shift_kernel, dim3(B), dim3(256), 0, stream, h_hi, h_lo, cache_hi, cache_lo, out_hi, out_lo, pos,
                       cache_rows, D, fmap);
    LAUNCH_CHECK();
    return AMDNUWA_OK;
}

extern "C" int amdnuwa_s3_decode(const amdnuwa_s3_geom* g, const uint16_t* qkv, const uint16_t* qkv_lo, uint16_t* kv_cache,
                                 uint16_t* kv_cache_lo, int cache_rows, const int* pos, const float* w_th, uint16_t* o,
                                 uint16_t* o_lo, hipStream_t stream) {
    if (!g || !qkv || !kv_cache || !pos || !w_th || !o) return AMDNUWA_ERR_ARG;
    if (g->heads <= 0 || g->dim_head <= 0 || g->kf <= 0 || g->kh <= 0 || g->kw <= 0 || g->df <= 0 || g->dh <= 0 || g->dw <= 0 ||
        g->F <= 0 || g->H <= 0 || g->W <= 0)
        return AMDNUWA_ERR_ARG;
    if ((qkv_lo != nullptr) != (kv_cache_lo != nullptr)) return AMDNUWA_ERR_ARG;
    if (g->noncausal) return AMDNUWA_ERR_UNSUPPORTED;          // incremental decoding needs every tap behind the query
    if (cache_rows < 1 || cache_rows > 1 + g->F * g->H * g->W) return AMDNUWA_ERR_ARG;
    if (g->B <= 0) return AMDNUWA_OK;
    S3DecArgs a{};
    a.qkv = qkv; a.qkvl = qkv_lo; a.kv = kv_cache; a.kvl = kv_cache_lo; a.o = o; a.ol = o_lo; a.wth = w_th; a.rel = g->rel_bias;
    a.pos = pos; a.cache_rows = cache_rows; a.H = g->H; a.W = g->W; a.kf = g->kf; a.kh = g->kh; a.kw = g->kw;
    a.df = g->df; a.dh = g->dh; a.dw = g->dw; a.heads = g->heads; a.dim_head = g->dim_head; a.scale = g->scale;
    a.J = g->kf * g->kh * g->kw + 1;
    if (g->dim_head % 8 || g->heads * g->dim_head > 4096) return AMDNUWA_ERR_UNSUPPORTED;
    const size_t lds = ((size_t)g->heads * (g->dim_head + 1) + 2 * (size_t)g->heads * a.J + 4096) * sizeof(float) + 2 * (size_t)a.J * sizeof(int);
    if (lds > 160 * 1024) return AMDNUWA_ERR_UNSUPPORTED;
#define S3D(DHT_) do { (void)hipFuncSetAttribute((const void*)s3_decode_kernel<DHT_>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
                       hipLaunchKernelGGL((s3_decode_kernel<DHT_>), dim3(g->B), dim3(512), lds, stream, a); } while (0)
    if (g->dim_head == 64) S3D(64); else if (g->dim_head == 32) S3D(32); else S3D(0);
#undef S3D
    LAUNCH_CHECK();
    return AMDNUWA_OK;
}

extern "C" int amdnuwa_xattn_decode(const amdnuwa_xattn_geom* g, const uint16_t* q, const uint16_t* q_lo, int ldq,
                                    const amdnuwa_xattn_kv* packed, const float* w_th, uint16_t* o, uint16_t* o_lo, int ldo,
                                    hipStream_t stream) {
    if (!g || !q || !packed || !packed->Kp || !packed->Vp || !packed->valid || !w_th || !o) return AMDNUWA_ERR_ARG;
    if (g->heads <= 0 || g->dim_head <= 0 || g->dim_head % 8 || g->T < 0 || g->JP < g->T + 1 || g->n != 1) return AMDNUWA_ERR_ARG;
    if ((q_lo != nullptr) != (packed->Kp_lo != nullptr) || (q_lo != nullptr) != (packed->Vp_lo != nullptr)) return AMDNUWA_ERR_ARG;
    if (g->B <= 0) return AMDNUWA_OK;
    XDecArgs a{};
    a.q = q; a.ql = q_lo; a.Kp = packed->Kp; a.Kpl = packed->Kp_lo; a.Vp = packed->Vp; a.Vpl = packed->Vp_lo;
    a.valid = packed->valid; a.o = o; a.ol = o_lo; a.wth = w_th; a.ldq = ldq; a.ldo = ldo; a.J = g->T + 1; a.JP = g->JP;
    a.heads = g->heads; a.dim_head = g->dim_head; a.scale = g->scale;
    if (g->heads * g->dim_head > 8192) return AMDNUWA_ERR_UNSUPPORTED;
    const size_t lds = ((size_t)g->heads * (g->dim_head + 1) + 2 * (size_t)g->heads * a.J + 8192) * sizeof(float) + (size_t)a.J * sizeof(int);
    if (lds > 160 * 1024) return AMDNUWA_ERR_UNSUPPORTED;
#define XD(DHT_) do { (void)hipFuncSetAttribute((const void*)xattn_decode_kernel<DHT_>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
                      hipLaunchKernelGGL((xattn_decode_kernel<DHT_>), dim3(g->B), dim3(1024), lds, stream, a); } while (0)
    if (g->dim_head == 64) XD(64); else if (g->dim_head == 32) XD(32); else XD(0);
#undef XD
    LAUNCH_CHECK();
    return AMDNUWA_OK;
}

extern "C" int amdnuwa_decode_ln(const void* y, int y_is_bf16, const float* resid, const float* w, const float* b,
                                 const float* next_w, const float* next_b, float* x_new, uint16_t* cache_hi, uint16_t* cache_lo,
                                 uint16_t* out_hi, uint16_t* out_lo, const int* pos, int B, int cache_rows, int D, int fmap,
                                 float eps, hipStream_t stream) {
    if (!y || D <= 0 || D % 4 || D > 4096) return AMDNUWA_ERR_ARG;
    if (resid && (!w || !b || !x_new)) return AMDNUWA_ERR_ARG;
    if (!resid && y_is_bf16) return AMDNUWA_ERR_ARG;                 // without a post-norm, y IS the fp32 stream row
    if (next_w && (!next_b || !out_hi)) return AMDNUWA_ERR_ARG;
    if (!next_w && !resid) return AMDNUWA_ERR_ARG;
    if (cache_hi && (!pos || fmap == 0 || fmap < -1 || cache_rows <= 0 || D % 16 || !next_w)) return AMDNUWA_ERR_ARG;
    if (cache_hi && ((cache_lo != nullptr) != (out_lo != nullptr))) return AMDNUWA_ERR_ARG;
    if (B <= 0) return AMDNUWA_OK;
    if (y_is_bf16)
        hipLaunchKernelGGL((decode_ln_kernel<true>), dim3(B), dim3(256), 0, stream, y, resid, w, b, next_w, next_b, x_new, cache_hi,
                           cache_lo, out_hi, out_lo, pos, cache_rows, D, fmap, eps);
    else
        hipLaunchKernelGGL((decode_ln_kernel<false>), dim3(B), dim3(256), 0, stream, y, resid, w, b, next_w, next_b, x_new, cache_hi,
                           cache_lo, out_hi, out_lo, pos, cache_rows, D, fmap, eps);
    LAUNCH_CHECK();
    return AMDNUWA_OK;
}

extern "C" int amdnuwa_prefill_ln(const void* y, int y_is_bf16, const float* resid, const float* w, const float* b,
                                  const float* next_w, const float* next_b, float* x_new, uint16_t* cache_hi, uint16_t* cache_lo,
                                  uint16_t* out_hi, uint16_t* out_lo, int B, int R, int cache_rows, int D, int fmap, float eps,
                                  hipStream_t stream) {
    if (!y || B <= 0 || R <= 0 || D <= 0) return AMDNUWA_ERR_ARG;
    if (resid && (!w || !b || !x_new)) return AMDNUWA_ERR_ARG;
    if (!resid && y_is_bf16) return AMDNUWA_ERR_ARG;                 // without a post-norm, y IS the fp32 stream row
    if (next_w && (!next_b || !out_hi)) return AMDNUWA_ERR_ARG;
    if (!next_w && !resid) return AMDNUWA_ERR_ARG;
    if (cache_hi && (fmap == 0 || fmap < -1 || cache_rows <= 0 || R > cache_rows || !next_w)) return AMDNUWA_ERR_ARG;
    if (cache_hi && ((cache_lo != nullptr) != (out_lo != nullptr))) return AMDNUWA_ERR_ARG;
    if (!cache_hi && cache_lo) return AMDNUWA_ERR_ARG;
    if (D % 16 || D > 4096) return AMDNUWA_ERR_UNSUPPORTED;
    if ((size_t)B * R > 0x7fffffffu) return AMDNUWA_ERR_UNSUPPORTED;
    if (y_is_bf16)
        hipLaunchKernelGGL((prefill_ln_kernel<true>), dim3(B * R), dim3(256), 0, stream, y, resid, w, b, next_w, next_b, x_new, cache_hi,
                           cache_lo, out_hi, out_lo, R, cache_rows, D, eps);
    else
        hipLaunchKernelGGL((prefill_ln_kernel<false>), dim3(B * R), dim3(256), 0, stream, y, resid, w, b, next_w, next_b, x_new, cache_hi,
                           cache_lo, out_hi, out_lo, R, cache_rows, D, eps);
    if (cache_hi) {
        // second launch, ordered behind the first on the stream: every cache row it reads is complete
        const bool v16 = D % 32 == 0;                                // a channel quarter is a whole number of 16-byte vectors
        const size_t nvec = (size_t)B * R * ((D >> 1) / (v16 ? 8 : 4)), nblk = (nvec + 255) / 256;
        if (nblk > 0x7fffffffu) return AMDNUWA_ERR_UNSUPPORTED;
        if (v16)
            hipLaunchKernelGGL((prefill_shift_kernel<uint4>), dim3((unsigned)nblk), dim3(256), 0, stream, cache_hi, cache_lo, out_hi, out_lo,
                               B, R, cache_rows, D, fmap);
        else
            hipLaunchKernelGGL((prefill_shift_kernel<uint2>), dim3((unsigned)nblk), dim3(256), 0, stream, cache_hi, cache_lo, out_hi, out_lo,
                               B, R, cache_rows, D, fmap);
    }
    LAUNCH_CHECK();
    return AMDNUWA_OK;
}

extern "C" int amdnuwa_prefill_kv(const uint16_t* qkv, const uint16_t* qkv_lo, uint16_t* kv_cache, uint16_t* kv_cache_lo, int B, int R,
                                  int cache_rows, int inner, hipStream_t stream) {
    if (!qkv || !kv_cache || B <= 0 || R <= 0 || cache_rows <= 0 || inner <= 0 || R > cache_rows) return AMDNUWA_ERR_ARG;
    if ((qkv_lo != nullptr) != (kv_cache_lo != nullptr)) return AMDNUWA_ERR_ARG;
    if (inner % 8) return AMDNUWA_ERR_UNSUPPORTED;                   // 16-byte vectors
    const size_t nblk = ((size_t)B * R * (inner >> 2) + 255) / 256;
    if (nblk > 0x7fffffffu) return AMDNUWA_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(prefill_kv_kernel, dim3((unsigned)nblk), dim3(256), 0, stream, qkv, qkv_lo, kv_cache, kv_cache_lo, B, R, cache_rows,
                       inner);
    LAUNCH_CHECK();
    return AMDNUWA_OK;
}
