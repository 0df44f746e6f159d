// Column-tiled forms of the Sparse3DNA / SparseCross2DNA window kernels (sparse3dna.hip) for token grids whose row does not fit one
// workgroup: W * heads * 4 > 512 threads, e.g. the 32 x 32 map of a 256-pixel model with 8 heads.
//
// A workgroup owns TW consecutive columns of one grid row (S3Tile: NT tiles per row, TW * heads * 4 <= 512) -- queries in the forward
// and the query-side backward, keys in the key-side backward.  Thread map: t = ((wt*NH + h)*4 + c), wt = column inside the tile.  Per
// tap plane it stages SW = TW + (kw-1)*dw columns of the key / value row (bwd_kv: of the q / dO row of the attending queries): its own
// columns plus the halo the kw taps reach, ow*dw columns before and (kw-1-ow)*dw after the queries (mirrored on the key side).  The
// staged image has more 16-byte slots than the workgroup has threads, so slot s = t, t + nt, ... goes from global memory straight to
// LDS between the two barriers of a plane (the row kernels prefetch their single slot into registers one plane ahead instead).
// Columns outside the grid are written as zeros and never read.
//
// Everything else is the row kernels' arithmetic in the row kernels' order: score tables SP / DP are [wt][j][h] of the tile, the ds / P'
// workspace keeps its [B][nq][J][NH] layout, the per-workgroup partials (dW_th, <bos> / null dk and dv) are indexed by (row, tile) and
// summed in that fixed order by s3_bwd_fin_kernel.  No atomics; a workgroup reads and writes only its own LDS and its own outputs, so
// nothing depends on which workgroups share a CU.
#include "common.h"
#include "s3_args.h"

namespace {

// (row, tile) of this workgroup: tiles of one row are neighbours in the XCD-contiguous order of xcd_row_id()
struct TilePos { int bid, b, ry, f, y, w0, tw; };
__device__ __forceinline__ TilePos tile_pos(const S3Args& a, int rows) {
    TilePos p;
    p.bid = xcd_row_id();
    const int rt = p.bid / a.NT, tl = p.bid - rt * a.NT;
    p.b = rt / rows; p.ry = rt % rows; p.f = p.ry / a.H; p.y = p.ry % a.H;
    p.w0 = tl * a.TW;
    p.tw = a.W - p.w0 < a.TW ? a.W - p.w0 : a.TW;        // columns of this tile (the last one may be partial)
    return p;
}

// grid columns c0 .. c0 + SW - 1 of one grid row of `src` (rows of `ld` elements), all heads -> the half-split LDS image: half v8 of the
// chunk of (staged column sc, h, c) at v8*HS + ((sc*NH + h)*4 + c)*8, HS = SW*NH*32 (sweep_taps of sparse3dna.hip: conflict-free b128 reads)
template <int CH>
__device__ __forceinline__ void stage_cols(const S3Args& a, const bf16_t* src, const bf16_t* srcl, size_t base_row, int pos0, int c0,
                                           int nrows_left, int ld, bf16_t* st_hi, bf16_t* st_lo) {
    // base_row = tensor row of grid position 0 of the sample, pos0 = grid position of column 0 of the staged row; column wc is read when it
    // lies in the grid and inside the nrows_left rows the sample has from base_row on, else its slot is zero
    const int HS = a.SW * a.NH * 32, nh4 = a.NH * 4, nslot = a.SW * nh4;
    for (int s = threadIdx.x; s < nslot; s += blockDim.x) {
        const int sc = s / nh4, r = s - sc * nh4, wc = c0 + sc;
        const bool ok = wc >= 0 && wc < a.W && pos0 + wc < nrows_left;
        const size_t gi = (base_row + pos0 + wc) * ld + r * CH;
#pragma unroll
        for (int v8 = 0; v8 < CH / 8; ++v8) {
            *reinterpret_cast<uint4*>(st_hi + v8 * HS + s * 8) = ok ? *reinterpret_cast<const uint4*>(src + gi + v8 * 8) : make_uint4(0, 0, 0, 0);
            if (srcl) *reinterpret_cast<uint4*>(st_lo + v8 * HS + s * 8) = ok ? *reinterpret_cast<const uint4*>(srcl + gi + v8 * 8) : make_uint4(0, 0, 0, 0);
        }
    }
}

// Sweep over all taps of the queries of one tile (sweep_taps of the row kernels, with the staged row widened by the halo).
// fn(j, hi, lo, hs) is called for every valid tap slot j >= 1 of this thread's (query, head).
template <int CH, typename Fn>
__device__ __forceinline__ void sweep_taps_w(const S3Args& a, const bf16_t* src, const bf16_t* srcl, const TilePos& p, int w, int h, int c,
                                             bool qvalid, bf16_t* st_hi, Fn&& fn) {
    const int HS = a.SW * a.NH * 32;
    bf16_t* st_lo = st_hi + (CH / 8) * HS;
    const int c0 = p.w0 - a.ow * a.dw;                   // grid column of staged column 0
    const int yr0 = p.y - a.oh * a.dh;
    int fr = (a.xmode ? 0 : p.f) - a.of * a.df;
    for (int ta = 0; ta < a.kf; ++ta, fr += a.df) {
        if (fr < 0 || fr >= a.FK) continue;
        int yr = yr0;
        for (int tb = 0; tb < a.kh; ++tb, yr += a.dh) {
            if (yr < 0 || yr >= a.H) continue;
            const int pos0 = (fr * a.H + yr) * a.W;
            __syncthreads();                             // previous plane fully consumed
            stage_cols<CH>(a, src, srcl, (size_t)p.b * a.kvrows + a.kvoff, pos0, c0, a.kvrows - a.kvoff, a.ldk, st_hi, st_lo);
            __syncthreads();
            if (qvalid) {
                const int jb = 1 + (ta * a.kh + tb) * a.kw;
                int wr = w - a.ow * a.dw;
                const uint8_t* mrow = a.kmask ? a.kmask + (size_t)p.b * a.kvrows + a.kvoff + pos0 : nullptr;
                for (int tc = 0; tc < a.kw; ++tc, wr += a.dw) {
                    if (wr < 0 || wr >= a.W) continue;
                    if (mrow && !mrow[wr]) continue;      // masked key: its slot keeps the mask value (P = 0) in every sweep
                    const int slot = (((wr - c0) * a.NH + h) * 4 + c) * 8;
                    fn(jb + tc, st_hi + slot, srcl ? st_lo + slot : nullptr, HS);
                }
            }
        }
    }
}

// scores + softmax of one tile: fills SP[(wt*J + j)*NH + h] with P (fp32).  Shared by fwd and bwd_q.
template <int DH, bool LO>
__device__ __forceinline__ void scores_softmax_w(const S3Args& a, const TilePos& p, int w, int wt, int h, int c, bool act, bool qvalid,
                                                 const float* qf, const uint32_t* qp, float* SP, bf16_t* st_hi, int J) {
    constexpr int CH = DH / 4;
    const int t = threadIdx.x, nt = blockDim.x;
    for (int e = t; e < a.TW * J * a.NH; e += nt) SP[e] = NEG_MAX;
    __syncthreads();
    auto qk = [&](const bf16_t* khi, const bf16_t* klo, int hs) {
        float s = 0.f;
        if (LO) {
            float kf_[CH];
            load_chunk<CH>(khi, klo, kf_, hs);
#pragma unroll
            for (int e = 0; e < CH; ++e) s += qf[e] * kf_[e];
        } else {
            uint32_t kp[CH / 2];
            load_pk<CH>(khi, kp, hs);
            s = dot_pk<CH>(qp, kp);
        }
        return quad_sum(s);
    };
    if (qvalid) {                                        // <bos> / null key: slot j = 0
        const size_t g = (size_t)p.b * a.k0_bs + h * DH + c * CH;
        const float s = qk(a.k0 + g, a.k0l ? a.k0l + g : nullptr, 8);
        if (c == 0) SP[(wt * J + 0) * a.NH + h] = s * a.scale + (a.bias ? a.bias[h] : 0.f);
    }
    sweep_taps_w<CH>(a, a.k, a.kl, p, w, h, c, qvalid, st_hi, [&](int j, const bf16_t* khi, const bf16_t* klo, int hs) {
        const float s = qk(khi, klo, hs);
        if (c == 0) SP[(wt * J + j) * a.NH + h] = s * a.scale + (a.bias ? a.bias[j * a.NH + h] : 0.f);
    });
    __syncthreads();
    // fp32 softmax over the J slots of each (wt, h): the 4 lanes of the group split j
    if (act) {
        float m = NEG_MAX;
        for (int j = c; j < J; j += 4) m = fmaxf(m, SP[(wt * J + j) * a.NH + h]);
        m = quad_max(m);
        float s = 0.f;
        for (int j = c; j < J; j += 4) s += expf(SP[(wt * J + j) * a.NH + h] - m);
        s = quad_sum(s);
        const float inv = 1.f / s;
        for (int j = c; j < J; j += 4) {
            const int idx = (wt * J + j) * a.NH + h;
            SP[idx] = expf(SP[idx] - m) * inv;
        }
    }
    __syncthreads();
}

template <int DH, bool LO, bool DROP = false>      // DROP: attention dropout, as in s3_fwd_kernel
__global__ __launch_bounds__(512, 4) void s3w_fwd_kernel(S3KArgs<DROP> a) {
    constexpr int CH = DH / 4;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int J = a.kf * a.kh * a.kw + 1;
    const int stage_elems = a.SW * a.NH * DH;
    bf16_t* st_hi = reinterpret_cast<bf16_t*>(smem);
    float* SP = reinterpret_cast<float*>(smem + (size_t)stage_elems * (a.kl ? 4 : 2));
    __shared__ float wsh[64];
    const int t = threadIdx.x, c = t & 3, wh = t >> 2, h = wh % a.NH, wt = wh / a.NH;
    const TilePos p = tile_pos(a, a.F * a.H);
    const int w = p.w0 + wt;
    const bool act = wt < p.tw;
    const int i = 1 + p.ry * a.W + w;
    const bool qvalid = act && i < a.ntok;
    if (t < a.NH * a.NH) wsh[t] = a.wth[t];
    // <bos> output row = its own value (np.py:499, 608): the first tile of the first row writes it
    if (p.ry == 0 && p.w0 == 0 && !a.xmode) {
        const int inner = a.NH * DH;
        for (int e = t; e < inner; e += blockDim.x) {
            const size_t gi = ((size_t)p.b * a.ntok) * a.ld + e, go = ((size_t)p.b * a.ntok) * a.ldo + e;
            a.o[go] = a.v[gi];
            if (a.ol) a.ol[go] = a.vl ? a.vl[gi] : (bf16_t)0;
        }
    }
    if (p.ry * a.W + p.w0 + 1 >= a.ntok) return;   // whole tile beyond the sequence (uniform)
    float qf[CH];
    uint32_t qp[CH / 2];
    if (qvalid) {
        const size_t g = ((size_t)p.b * a.ntok + i) * a.ld + h * DH + c * CH;
        if (LO) load_chunk<CH>(a.q + g, a.ql ? a.ql + g : nullptr, qf); else load_pk<CH>(a.q + g, qp);
    }
    scores_softmax_w<DH, LO>(a, p, w, wt, h, c, act, qvalid, qf, qp, SP, st_hi, J);
    // talking heads: P'[g] = sum_h Wth[g][h] P[h] per (wt, j), in place
    for (int item = t; item < p.tw * J; item += blockDim.x) {
        float pv[8], out[8];
#pragma unroll
        for (int hh = 0; hh < 8; ++hh) pv[hh] = hh < a.NH ? SP[item * a.NH + hh] : 0.f;
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            float s = 0.f;
#pragma unroll
            for (int hh = 0; hh < 8; ++hh) s += (g < a.NH && hh < a.NH ? wsh[g * a.NH + hh] : 0.f) * pv[hh];
            out[g] = s;
        }
        if constexpr (DROP) {
            const int iq = 1 + p.ry * a.W + p.w0 + item / J;
            if (iq < a.ntok) {
                const uint8_t* kp = a.keep + (((size_t)p.b * (a.ntok - 1) + (iq - 1)) * J + item % J) * a.NH;
#pragma unroll
                for (int g = 0; g < 8; ++g) if (g < a.NH) out[g] *= keep_factor(kp[g], a.drop_s);
            }
        }
#pragma unroll
        for (int g = 0; g < 8; ++g) if (g < a.NH) SP[item * a.NH + g] = out[g];
    }
    __syncthreads();
    // P'.V
    float of[CH];
#pragma unroll
    for (int e = 0; e < CH; ++e) of[e] = 0.f;
    auto pv = [&](float pj, const bf16_t* vhi, const bf16_t* vlo, int hs) {
        if (LO) {
            float vf[CH];
            load_chunk<CH>(vhi, vlo, vf, hs);
#pragma unroll
            for (int e = 0; e < CH; ++e) of[e] += pj * vf[e];
        } else {
            uint32_t vp[CH / 2];
            load_pk<CH>(vhi, vp, hs);
            axpy_pk<CH>(of, pj, vp);
        }
    };
    if (qvalid) {
        const size_t g = (size_t)p.b * a.k0_bs + h * DH + c * CH;
        pv(SP[(wt * J + 0) * a.NH + h], a.v0 + g, a.v0l ? a.v0l + g : nullptr, 8);
    }
    sweep_taps_w<CH>(a, a.v, a.vl, p, w, h, c, qvalid, st_hi, [&](int j, const bf16_t* vhi, const bf16_t* vlo, int hs) {
        pv(SP[(wt * J + j) * a.NH + h], vhi, vlo, hs);
    });
    if (qvalid) {
        const size_t g = ((size_t)p.b * a.ntok + i) * a.ldo + h * DH + c * CH;
        store_chunk<CH>(a.o + g, a.ol ? a.ol + g : nullptr, of);
    }
}

template <int DH, bool LO, bool DROP = false>      // DROP: attention dropout, as in s3_bwd_q_kernel
__global__ __launch_bounds__(512, 4) void s3w_bwd_q_kernel(S3KArgs<DROP> a) {
    constexpr int CH = DH / 4;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int J = a.kf * a.kh * a.kw + 1;
    const int stage_elems = a.SW * a.NH * DH;
    const int nsp = a.TW * J * a.NH;
    bf16_t* st_hi = reinterpret_cast<bf16_t*>(smem);
    float* SP = reinterpret_cast<float*>(smem + (size_t)stage_elems * (a.kl ? 4 : 2));   // P, later unchanged
    const int inner = a.NH * DH;
    const int spdp = 2 * nsp > a.TW * inner ? 2 * nsp : a.TW * inner;
    float* DP = SP + nsp;                                                   // dP' -> dP -> ds
    float* RED = SP + spdp;                                                 // [8][64] dW_th partials
    __shared__ float wsh[64];
    const int t = threadIdx.x, c = t & 3, wh = t >> 2, h = wh % a.NH, wt = wh / a.NH;
    const TilePos p = tile_pos(a, a.F * a.H);
    const int w = p.w0 + wt, b = p.b;
    const bool act = wt < p.tw;
    const int i = 1 + p.ry * a.W + w;
    const bool qvalid = act && i < a.ntok;
    const int nq = a.ntok - 1;
    const int nit = p.tw * J;                                               // (query, slot) items of this tile
    if (t < a.NH * a.NH) wsh[t] = a.wth[t];
    float* pth = a.part_th + (size_t)p.bid * a.NH * a.NH;
    float* pk0 = a.part_k0 + (size_t)p.bid * inner;
    float* pv0 = a.part_v0 + (size_t)p.bid * inner;
    if (p.ry == 0 && p.w0 == 0 && !a.xmode) {   // dq of the <bos> row is zero (its query is never used)
        for (int e = t; e < inner; e += blockDim.x) {
            const size_t go = ((size_t)b * a.ntok) * a.ldd + e;
            a.dq[go] = 0;
            if (a.dql) a.dql[go] = 0;
        }
    }
    if (p.ry * a.W + p.w0 + 1 >= a.ntok) {   // tile beyond the sequence: contributes nothing
        for (int e = t; e < a.NH * a.NH; e += blockDim.x) pth[e] = 0.f;
        for (int e = t; e < inner; e += blockDim.x) { pk0[e] = 0.f; pv0[e] = 0.f; }
        return;
    }
    float qf[CH], dof[CH];
#pragma unroll
    for (int e = 0; e < CH; ++e) { qf[e] = 0.f; dof[e] = 0.f; }
    uint32_t qp[CH / 2], dop[CH / 2];            // packed bf16 q / dO for the dot2 path (bf16 operand mode)
#pragma unroll
    for (int e = 0; e < CH / 2; ++e) { qp[e] = 0; dop[e] = 0; }
    if (qvalid) {
        const size_t g = ((size_t)b * a.ntok + i) * a.ld + h * DH + c * CH;
        const size_t gd = ((size_t)b * a.ntok + i) * a.lddo + h * DH + c * CH;
        if (LO) {
            load_chunk<CH>(a.q + g, a.ql ? a.ql + g : nullptr, qf);
            load_chunk<CH>(a.dO + gd, a.dOl ? a.dOl + gd : nullptr, dof);
        } else {
            load_pk<CH>(a.q + g, qp);
            load_pk<CH>(a.dO + gd, dop);
        }
    }
    scores_softmax_w<DH, LO>(a, p, w, wt, h, c, act, qvalid, qf, qp, SP, st_hi, J);
    // P' = mix(P) -> global (needed by bwd_kv); P stays in SP  (DROP: P'' instead, formed after the dO.V sweep below)
    if constexpr (!DROP) {
        for (int item = t; item < nit; item += blockDim.x) {
            const int wq = item / J, j = item % J;
            const int iq = 1 + p.ry * a.W + p.w0 + wq;
            float pv[8];
#pragma unroll
            for (int hh = 0; hh < 8; ++hh) pv[hh] = hh < a.NH ? SP[item * a.NH + hh] : 0.f;
            if (iq < a.ntok) {
                float* dst = a.pm + (((size_t)b * nq + (iq - 1)) * J + j) * a.NH;
#pragma unroll
                for (int g = 0; g < 8; ++g) {
                    float s = 0.f;
#pragma unroll
                    for (int hh = 0; hh < 8; ++hh) s += (g < a.NH && hh < a.NH ? wsh[g * a.NH + hh] : 0.f) * pv[hh];
                    if (g < a.NH) dst[g] = s;
                }
            }
        }
    }
    for (int e = t; e < nsp; e += blockDim.x) DP[e] = 0.f;
    __syncthreads();
    // dP'[wt][j][g] = dO[wt][g] . v_j[g]
    auto dov = [&](const bf16_t* vhi, const bf16_t* vlo, int hs) {
        float s = 0.f;
        if (LO) {
            float vf[CH];
            load_chunk<CH>(vhi, vlo, vf, hs);
#pragma unroll
            for (int e = 0; e < CH; ++e) s += dof[e] * vf[e];
        } else {
            uint32_t vp[CH / 2];
            load_pk<CH>(vhi, vp, hs);
            s = dot_pk<CH>(dop, vp);
        }
        return quad_sum(s);
    };
    if (qvalid) {
        const size_t g = (size_t)b * a.k0_bs + h * DH + c * CH;
        const float s = dov(a.v0 + g, a.v0l ? a.v0l + g : nullptr, 8);
        if (c == 0) DP[(wt * J + 0) * a.NH + h] = s;
    }
    sweep_taps_w<CH>(a, a.v, a.vl, p, w, h, c, qvalid, st_hi, [&](int j, const bf16_t* vhi, const bf16_t* vlo, int hs) {
        const float s = dov(vhi, vlo, hs);
        if (c == 0) DP[(wt * J + j) * a.NH + h] = s;
    });
    __syncthreads();
    if constexpr (DROP) {
        // P'' = keep . mix(P) . s -> global (what bwd_kv takes dV with) and dP' = keep . dP'' . s: one mask byte per entry, read here
        for (int item = t; item < nit; item += blockDim.x) {
            const int wq = item / J, j = item % J;
            const int iq = 1 + p.ry * a.W + p.w0 + wq;
            float pv[8];
#pragma unroll
            for (int hh = 0; hh < 8; ++hh) pv[hh] = hh < a.NH ? SP[item * a.NH + hh] : 0.f;
            if (iq < a.ntok) {
                const size_t ci = (((size_t)b * nq + (iq - 1)) * J + j) * a.NH;
#pragma unroll
                for (int g = 0; g < 8; ++g) {
                    float s = 0.f;
#pragma unroll
                    for (int hh = 0; hh < 8; ++hh) s += (g < a.NH && hh < a.NH ? wsh[g * a.NH + hh] : 0.f) * pv[hh];
                    if (g < a.NH) {
                        const float kf_ = keep_factor(a.keep[ci + g], a.drop_s);
                        a.pm[ci + g] = s * kf_;
                        DP[item * a.NH + g] *= kf_;
                    }
                }
            }
        }
        __syncthreads();
    }
    // dW_th[g][h] partial = sum_{wt,j} dP'[g] * P[h]   (thread = (g,h) pair x item groups)
    {
        const int pair = t & 63, grp = t >> 6, ng = blockDim.x >> 6;
        const int g = pair / a.NH, hh = pair % a.NH;
        float acc = 0.f;
        if (pair < a.NH * a.NH)
            for (int item = grp; item < nit; item += ng) acc += DP[item * a.NH + g] * SP[item * a.NH + hh];
        RED[grp * 64 + pair] = acc;
        __syncthreads();
        if (t < a.NH * a.NH) {
            float s = 0.f;
            for (int k = 0; k < ng; ++k) s += RED[k * 64 + t];
            pth[t] = s;
        }
        __syncthreads();
    }
    // dP[h] = sum_g Wth[g][h] dP'[g]   (in place, item-local)
    for (int item = t; item < nit; item += blockDim.x) {
        float dv_[8], out[8];
#pragma unroll
        for (int g = 0; g < 8; ++g) dv_[g] = g < a.NH ? DP[item * a.NH + g] : 0.f;
#pragma unroll
        for (int hh = 0; hh < 8; ++hh) {
            float s = 0.f;
#pragma unroll
            for (int g = 0; g < 8; ++g) s += (g < a.NH && hh < a.NH ? wsh[g * a.NH + hh] : 0.f) * dv_[g];
            out[hh] = s;
        }
#pragma unroll
        for (int hh = 0; hh < 8; ++hh) if (hh < a.NH) DP[item * a.NH + hh] = out[hh];
    }
    __syncthreads();
    // ds = P * (dP - sum_j P dP)
    if (act) {
        float d = 0.f;
        for (int j = c; j < J; j += 4) d += SP[(wt * J + j) * a.NH + h] * DP[(wt * J + j) * a.NH + h];
        d = quad_sum(d);
        for (int j = c; j < J; j += 4) {
            const int idx = (wt * J + j) * a.NH + h;
            const float dsv = SP[idx] * (DP[idx] - d);
            DP[idx] = dsv;
            if (qvalid) a.ds[(((size_t)b * nq + (i - 1)) * J + j) * a.NH + h] = dsv;
        }
    }
    __syncthreads();
    // dq = scale * sum_j ds_j k_j ;  <bos> partials: dk0 += scale*ds_0*q, dv0 += P'_0*dO
    float dqf[CH];
#pragma unroll
    for (int e = 0; e < CH; ++e) dqf[e] = 0.f;
    float k0c[CH], v0c[CH];
#pragma unroll
    for (int e = 0; e < CH; ++e) { k0c[e] = 0.f; v0c[e] = 0.f; }
    if (qvalid) {
        float kf_[CH];
        const size_t g = (size_t)b * a.k0_bs + h * DH + c * CH;
        load_chunk<CH>(a.k0 + g, a.k0l ? a.k0l + g : nullptr, kf_);
        const float d0 = DP[(wt * J + 0) * a.NH + h];
        float pm0 = 0.f;                                        // P'[wt][0][g = h] = sum_hh Wth[h][hh] P[wt][0][hh]
        for (int hh = 0; hh < a.NH; ++hh) pm0 += wsh[h * a.NH + hh] * SP[(wt * J + 0) * a.NH + hh];
        if constexpr (DROP) pm0 *= keep_factor(a.keep[((size_t)b * nq + (i - 1)) * J * a.NH + h], a.drop_s);
#pragma unroll
        for (int e = 0; e < CH; ++e) {
            const float qe = LO ? qf[e] : ((e & 1) ? hi_f(qp[e >> 1]) : lo_f(qp[e >> 1]));
            const float de = LO ? dof[e] : ((e & 1) ? hi_f(dop[e >> 1]) : lo_f(dop[e >> 1]));
            dqf[e] += d0 * kf_[e];
            k0c[e] = a.scale * d0 * qe;
            v0c[e] = pm0 * de;
        }
    }
    sweep_taps_w<CH>(a, a.k, a.kl, p, w, h, c, qvalid, st_hi, [&](int j, const bf16_t* khi, const bf16_t* klo, int hs) {
        const float dj = DP[(wt * J + j) * a.NH + h];
        if (LO) {
            float kf_[CH];
            load_chunk<CH>(khi, klo, kf_, hs);
#pragma unroll
            for (int e = 0; e < CH; ++e) dqf[e] += dj * kf_[e];
        } else {
            uint32_t kp[CH / 2];
            load_pk<CH>(khi, kp, hs);
            axpy_pk<CH>(dqf, dj, kp);
        }
    });
    if (qvalid) {
#pragma unroll
        for (int e = 0; e < CH; ++e) dqf[e] *= a.scale;
        const size_t g = ((size_t)b * a.ntok + i) * a.ldd + h * DH + c * CH;
        store_chunk<CH>(a.dq + g, a.dql ? a.dql + g : nullptr, dqf);
    }
    // reduce the <bos> partials over the queries of the tile (fixed order), via LDS (reuses the SP / DP space: TW*inner <= spdp floats),
    // one of the two at a time
    float* RK = SP;                       // [tw][inner]
#pragma unroll 1
    for (int which = 0; which < 2; ++which) {
        __syncthreads();
        if (act) {
#pragma unroll
            for (int e = 0; e < CH; ++e) RK[wt * inner + h * DH + c * CH + e] = which ? v0c[e] : k0c[e];
        }
        __syncthreads();
        for (int e = t; e < inner; e += blockDim.x) {
            float sk = 0.f;
            for (int ww = 0; ww < p.tw; ++ww) sk += RK[ww * inner + e];
            (which ? pv0 : pk0)[e] = sk;
        }
    }
}

template <int DH, bool LO>
__global__ __launch_bounds__(512, 4) void s3w_bwd_kv_kernel(S3Args a) {
    constexpr int CH = DH / 4;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int J = a.kf * a.kh * a.kw + 1;
    const int stage_elems = a.SW * a.NH * DH;
    bf16_t* sq_hi = reinterpret_cast<bf16_t*>(smem);
    bf16_t* sq_lo = sq_hi + stage_elems;
    bf16_t* sd_hi = sq_lo + stage_elems;
    bf16_t* sd_lo = sd_hi + stage_elems;
    const int t = threadIdx.x, c = t & 3, wh = t >> 2, h = wh % a.NH, wt = wh / a.NH;
    const TilePos p = tile_pos(a, a.FK * a.H);       // key rows of the grid (the launch covers B * FK * H * NT workgroups)
    const int w = p.w0 + wt, b = p.b, f = p.f, y = p.y;
    const bool act = wt < p.tw;
    const int ik = a.kvoff + p.ry * a.W + w;         // key row index inside the sample
    const bool kvalid = act && ik < a.kvrows;
    const int nq = a.ntok - 1;
    if (p.ry * a.W + p.w0 + a.kvoff >= a.kvrows) return;
    float dkf[CH], dvf[CH];
#pragma unroll
    for (int e = 0; e < CH; ++e) { dkf[e] = 0.f; dvf[e] = 0.f; }
    // planes t = ta*kh + tb; the attending query row of plane t is (f + (of-ta)df, y + (oh-tb)dh)  [of = kf-1 when causal]
    // (xmode: key frame f is tap f of EVERY query frame, so the sweep runs over the query frames instead of the frame taps)
    const int nplanes = (a.xmode ? a.F : a.kf) * a.kh;
    auto plane = [&](int tpl, int& fq, int& yq) {
        const int ta = tpl / a.kh, tb = tpl - ta * a.kh;
        fq = a.xmode ? ta : f + (a.of - ta) * a.df;
        yq = y + (a.oh - tb) * a.dh;
        return fq >= 0 && yq >= 0 && fq < a.F && yq < a.H && (fq * a.H + yq) * a.W + 1 < a.ntok;
    };
    auto slot_plane = [&](int tpl) { return a.xmode ? f * a.kh + (tpl % a.kh) : tpl; };      // tap-plane index inside the J slots
    auto next_plane = [&](int tpl) { int fq, yq; while (tpl < nplanes && !plane(tpl, fq, yq)) ++tpl; return tpl; };
    const int HS = a.SW * a.NH * 32;
    const int c0 = p.w0 - (a.kw - 1 - a.ow) * a.dw;  // grid column of staged column 0: the attending queries sit at w + (ow - tc)*dw
    for (int tp = next_plane(0); tp < nplanes; tp = next_plane(tp + 1)) {
        int fq, yq;
        plane(tp, fq, yq);
        const int pos0 = (fq * a.H + yq) * a.W;
        __syncthreads();
        stage_cols<CH>(a, a.q, a.ql, (size_t)b * a.ntok + 1, pos0, c0, nq, a.ld, sq_hi, sq_lo);
        stage_cols<CH>(a, a.dO, a.dOl, (size_t)b * a.ntok + 1, pos0, c0, nq, a.lddo, sd_hi, sd_lo);
        __syncthreads();
        if (kvalid) {
            for (int tc = 0; tc < a.kw; ++tc) {
                const int wq = w + (a.ow - tc) * a.dw;
                if (wq < 0 || wq >= a.W) continue;
                const int pq = pos0 + wq;
                if (1 + pq >= a.ntok) continue;
                const size_t ci = (((size_t)b * nq + pq) * J + 1 + slot_plane(tp) * a.kw + tc) * a.NH + h;
                const float dsv = a.ds[ci], pmv = a.pm[ci];
                const int slot = (((wq - c0) * a.NH + h) * 4 + c) * 8;
                if (LO) {
                    float qq[CH], dd[CH];
                    load_chunk<CH>(sq_hi + slot, a.ql ? sq_lo + slot : nullptr, qq, HS);
                    load_chunk<CH>(sd_hi + slot, a.dOl ? sd_lo + slot : nullptr, dd, HS);
#pragma unroll
                    for (int e = 0; e < CH; ++e) { dkf[e] += dsv * qq[e]; dvf[e] += pmv * dd[e]; }
                } else {
                    uint32_t qk2[CH / 2], dk2[CH / 2];
                    load_pk<CH>(sq_hi + slot, qk2, HS);
                    load_pk<CH>(sd_hi + slot, dk2, HS);
                    axpy_pk<CH>(dkf, dsv, qk2);
                    axpy_pk<CH>(dvf, pmv, dk2);
                }
            }
        }
    }
    if (kvalid) {
#pragma unroll
        for (int e = 0; e < CH; ++e) dkf[e] *= a.scale;
        const size_t g = ((size_t)b * a.kvrows + ik) * a.lddk + h * DH + c * CH;
        store_chunk<CH>(a.dk + g, a.dkl ? a.dkl + g : nullptr, dkf);
        store_chunk<CH>(a.dv + g, a.dvl ? a.dvl + g : nullptr, dvf);
    }
}

int tile_threads(const S3Args& a) { return ((a.TW * a.NH * 4 + 63) / 64) * 64; }

}  // namespace

int s3w_fwd_launch(const S3Args& a, int dim_head, bool lo, size_t lds, const uint8_t* keep, float drop_s, hipStream_t stream) {
    const dim3 grid((unsigned)((size_t)a.B * a.F * a.H * a.NT)), block(tile_threads(a));
    return s3_dispatch(dim_head, lo, keep != nullptr, [&](auto dh, auto lo_c, auto dr) {
        return s3_launch(s3w_fwd_kernel<dh(), lo_c(), dr()>, grid, block, lds, stream, s3_kargs<dr()>(a, keep, drop_s));
    });
}

// query side over the B*F*H*NT (query row, tile) workgroups, then the key side over the B*FK*H*NT (key row, tile) ones
int s3w_bwd_launch(const S3Args& a, int dim_head, bool lo, size_t lds_q, size_t lds_kv, const uint8_t* keep, float drop_s, hipStream_t stream) {
    const dim3 grid_q((unsigned)((size_t)a.B * a.F * a.H * a.NT)), grid_kv((unsigned)((size_t)a.B * a.FK * a.H * a.NT)), block(tile_threads(a));
    return s3_dispatch(dim_head, lo, keep != nullptr, [&](auto dh, auto lo_c, auto dr) {
        const int rc = s3_launch(s3w_bwd_q_kernel<dh(), lo_c(), dr()>, grid_q, block, lds_q, stream, s3_kargs<dr()>(a, keep, drop_s));
        return rc ? rc : s3_launch(s3w_bwd_kv_kernel<dh(), lo_c()>, grid_kv, block, lds_kv, stream, a);
    });
}
