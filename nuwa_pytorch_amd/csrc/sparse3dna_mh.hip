// Many-head forms of the causal Sparse3DNA window kernels: 9 .. 16 heads (compile-time bound MH = 16, run-time NH), bf16 or hi + lo operands,
// dim_head 32 / 64.  Modelled on the column-tiled kernels of sparse3dna_wide.hip and kept in their arithmetic and summation order: thread map
// t = ((wt*NH + h)*4 + c), halo staging of SW columns per tap plane, score tables SP / DP [wt][j][h], the ds / P' workspace [B][nq][J][NH],
// per-(row, tile) partials summed by s3_bwd_fin_kernel.  EVERY geometry runs as column tiles here (tw <= 128 / heads columns, at most 8 at 16
// heads); a row that fits one workgroup is the case NT = 1, which stages the whole row without halo.
//
// What differs from the 8-head kernels: the talking-heads matrix sits zero-padded as [MH][MH] in LDS and is filled by a strided loop (a
// one-column tile of 16 heads has 64 threads for 256 entries); the head mixes run over 16 inputs in index order with one accumulator, one
// output head per pass of a run-time loop (registers); the dW_th partial reduction loops (item group, pair) units over the threads with a fixed
// NG = 4 item groups, so its summation order does not depend on the block size.  No row-kernel form, no MFMA form, no fp16 form, no dropout,
// no cross (xmode) form.  No atomics: a workgroup writes only its own LDS and its own outputs.
//
// Every address below is formed by a function of s3mh_index.h, which tools/s3mh_index_walk.cpp walks on the CPU for the geometries of
// tests/test_gpu_s3_mh.py.
#include "common.h"
#include "s3_args.h"
#include "s3mh_index.h"

namespace {

constexpr int MH = S3MH_MH;

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

// grid columns c0 .. c0 + SW - 1 of one grid row of `src`, all heads -> the half-split LDS image (stage_cols of sparse3dna_wide.hip)
template <int CH>
__device__ __forceinline__ void stage_cols(const S3Args& a, const bf16_t* src, const bf16_t* srcl, size_t base_row, int pos0, int c0,
                                           int nrows_left, int ld, bf16_t* st_hi, bf16_t* st_lo) {
    const int HS = s3mh_hs(a.SW, a.NH), nh4 = a.NH * 4, nslot = a.SW * nh4;
    for (int s = threadIdx.x; s < nslot; s += blockDim.x) {
        const int sc = s / nh4, r = s - sc * nh4, wc = c0 + sc;
        const bool ok = wc >= 0 && wc < a.W && pos0 + wc < nrows_left;
#pragma unroll
        for (int v8 = 0; v8 < CH / 8; ++v8) {
            const size_t gi = s3mh_g_stage(base_row + pos0 + wc, ld, r, CH, v8);
            const int li = s3mh_st_write(s, v8, HS);
            *reinterpret_cast<uint4*>(st_hi + li) = ok ? *reinterpret_cast<const uint4*>(src + gi) : make_uint4(0, 0, 0, 0);
            if (srcl) *reinterpret_cast<uint4*>(st_lo + li) = ok ? *reinterpret_cast<const uint4*>(srcl + gi) : make_uint4(0, 0, 0, 0);
        }
    }
}

// Sweep over all taps of the queries of one tile; fn(j, hi, lo, hs) is called for every valid tap slot j >= 1 of this thread's (query, head).
template <int CH, typename Fn>
__device__ __forceinline__ void sweep_taps(const S3Args& a, const bf16_t* src, const bf16_t* srcl, const TilePos& p, int w, int h, int c,
                                           bool qvalid, bf16_t* st_hi, Fn&& fn) {
    const int HS = s3mh_hs(a.SW, a.NH);
    bf16_t* st_lo = st_hi + s3mh_stage_elems(a.SW, a.NH, CH * 4);
    const int c0 = s3mh_c0(a.NT, p.w0, a.ow * a.dw);     // grid column of staged column 0
    const int yr0 = p.y - a.oh * a.dh;
    int fr = p.f - a.of * a.df;
    for (int ta = 0; ta < a.kf; ++ta, fr += a.df) {
        if (fr < 0 || fr >= a.F) continue;
        int yr = yr0;
        for (int tb = 0; tb < a.kh; ++tb, yr += a.dh) {
            if (yr < 0 || yr >= a.H) continue;
            const int pos0 = (fr * a.H + yr) * a.W;
            __syncthreads();                             // previous plane fully consumed
            stage_cols<CH>(a, src, srcl, (size_t)p.b * a.ntok + 1, pos0, c0, a.ntok - 1, a.ld, st_hi, st_lo);
            __syncthreads();
            if (qvalid) {
                const int jb = 1 + (ta * a.kh + tb) * a.kw;
                int wr = w - a.ow * a.dw;
                for (int tc = 0; tc < a.kw; ++tc, wr += a.dw) {
                    if (wr < 0 || wr >= a.W) continue;
                    const int slot = s3mh_st_read(wr - c0, h, c, a.NH);
                    fn(jb + tc, st_hi + slot, srcl ? st_lo + slot : nullptr, HS);
                }
            }
        }
    }
}

// the talking-heads matrix, zero-padded to [MH][MH]: rows / columns >= NH stay zero, so the mixes below need no head-count test per term
__device__ __forceinline__ void load_wsh(const S3Args& a, float* wsh) {
    for (int e = threadIdx.x; e < MH * MH; e += blockDim.x) {
        const int g = e / MH, h = e - g * MH;
        wsh[s3mh_wsh(g, h)] = (g < a.NH && h < a.NH) ? a.wth[s3mh_wth(g, h, a.NH)] : 0.f;
    }
}
// sum_h W[g][h] in[h] (TR: W[h][g]) over the MH padded heads, h in index order, one accumulator (the order of the 8-head kernels).  The
// callers hold in[] in registers and loop g at run time, one output head per pass: the matrix row comes from LDS (one address for the
// whole wave) instead of 256 hoisted registers, which spilled under the 128-VGPR bound of __launch_bounds__(512, 4).
template <bool TR>
__device__ __forceinline__ float mix_row(const float* wsh, const float* in, int g) {
    float s = 0.f;
#pragma unroll
    for (int hh = 0; hh < MH; ++hh) s += wsh[TR ? s3mh_wsh(hh, g) : s3mh_wsh(g, hh)] * in[hh];
    return s;
}

// scores + softmax of one tile: fills SP[(wt*J + j)*NH + h] with P (fp32).  Shared by fwd and bwd_q.
template <int DH, bool LO>
__device__ __forceinline__ void scores_softmax(const S3Args& a, const TilePos& p, int w, int wt, int h, int c, bool act, bool qvalid,
                                               const float* qf, const uint32_t* qp, float* SP, bf16_t* st_hi, int J) {
    constexpr int CH = DH / 4;
    const int t = threadIdx.x, nt = blockDim.x;
    for (int e = t; e < s3mh_nsp(a.TW, J, a.NH); e += nt) SP[e] = NEG_MAX;
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
    if (qvalid) {                                        // <bos> key: slot j = 0
        const size_t g = s3mh_g_k0(p.b, a.k0_bs, h, c, DH);
        const float s = qk(a.k0 + g, a.k0l ? a.k0l + g : nullptr, 8);
        if (c == 0) SP[s3mh_tab(wt, 0, h, J, a.NH)] = s * a.scale + (a.bias ? a.bias[s3mh_g_bias(0, a.NH, h)] : 0.f);
    }
    sweep_taps<CH>(a, a.k, a.kl, p, w, h, c, qvalid, st_hi, [&](int j, const bf16_t* khi, const bf16_t* klo, int hs) {
        const float s = qk(khi, klo, hs);
        if (c == 0) SP[s3mh_tab(wt, j, h, J, a.NH)] = s * a.scale + (a.bias ? a.bias[s3mh_g_bias(j, a.NH, h)] : 0.f);
    });
    __syncthreads();
    // fp32 softmax over the J slots of each (wt, h): the 4 lanes of the group split j
    if (act) {
        float m = NEG_MAX;
        for (int j = c; j < J; j += 4) m = fmaxf(m, SP[s3mh_tab(wt, j, h, J, a.NH)]);
        m = quad_max(m);
        float s = 0.f;
        for (int j = c; j < J; j += 4) s += expf(SP[s3mh_tab(wt, j, h, J, a.NH)] - m);
        s = quad_sum(s);
        const float inv = 1.f / s;
        for (int j = c; j < J; j += 4) {
            const int idx = s3mh_tab(wt, j, h, J, a.NH);
            SP[idx] = expf(SP[idx] - m) * inv;
        }
    }
    __syncthreads();
}

template <int DH, bool LO>
__global__ __launch_bounds__(512, 4) void s3mh_fwd_kernel(S3Args a) {
    constexpr int CH = DH / 4;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int J = a.kf * a.kh * a.kw + 1;
    bf16_t* st_hi = reinterpret_cast<bf16_t*>(smem);
    float* SP = reinterpret_cast<float*>(smem + s3mh_off_sp(a.SW, a.NH, DH, LO));
    __shared__ float wsh[MH * MH];
    const int t = threadIdx.x, c = t & 3, wh = t >> 2, h = wh % a.NH, wt = wh / a.NH;
    const TilePos p = tile_pos(a, a.F * a.H);
    const int w = p.w0 + wt;
    const bool act = wt < p.tw;
    const int i = 1 + p.ry * a.W + w;
    const bool qvalid = act && i < a.ntok;
    load_wsh(a, wsh);
    // <bos> output row = its own value row: the first tile of the first row writes it
    if (p.ry == 0 && p.w0 == 0) {
        const int inner = a.NH * DH;
        for (int e = t; e < inner; e += blockDim.x) {
            const size_t gi = s3mh_g_bos(p.b, a.ntok, a.ld, e), go = s3mh_g_bos(p.b, a.ntok, a.ldo, e);
            a.o[go] = a.v[gi];
            if (a.ol) a.ol[go] = a.vl ? a.vl[gi] : (bf16_t)0;
        }
    }
    if (p.ry * a.W + p.w0 + 1 >= a.ntok) return;   // whole tile beyond the sequence (uniform)
    float qf[CH];
    uint32_t qp[CH / 2];
    if (qvalid) {
        const size_t g = s3mh_g_tok(p.b, a.ntok, i, a.ld, h, c, DH);
        if (LO) load_chunk<CH>(a.q + g, a.ql ? a.ql + g : nullptr, qf); else load_pk<CH>(a.q + g, qp);
    }
    scores_softmax<DH, LO>(a, p, w, wt, h, c, act, qvalid, qf, qp, SP, st_hi, J);
    // talking heads: P'[g] = sum_h Wth[g][h] P[h] per (wt, j), in place
    for (int item = t; item < p.tw * J; item += blockDim.x) {
        float pv[MH];
#pragma unroll
        for (int hh = 0; hh < MH; ++hh) pv[hh] = hh < a.NH ? SP[s3mh_tab_item(item, hh, a.NH)] : 0.f;
#pragma unroll 1
        for (int g = 0; g < a.NH; ++g) SP[s3mh_tab_item(item, g, a.NH)] = mix_row<false>(wsh, pv, g);
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
        const size_t g = s3mh_g_k0(p.b, a.k0_bs, h, c, DH);
        pv(SP[s3mh_tab(wt, 0, h, J, a.NH)], a.v0 + g, a.v0l ? a.v0l + g : nullptr, 8);
    }
    sweep_taps<CH>(a, a.v, a.vl, p, w, h, c, qvalid, st_hi, [&](int j, const bf16_t* vhi, const bf16_t* vlo, int hs) {
        pv(SP[s3mh_tab(wt, j, h, J, a.NH)], vhi, vlo, hs);
    });
    if (qvalid) {
        const size_t g = s3mh_g_tok(p.b, a.ntok, i, a.ldo, h, c, DH);
        store_chunk<CH>(a.o + g, a.ol ? a.ol + g : nullptr, of);
    }
}

template <int DH, bool LO>
__global__ __launch_bounds__(512, 4) void s3mh_bwd_q_kernel(S3Args a) {
    constexpr int CH = DH / 4;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int J = a.kf * a.kh * a.kw + 1;
    const int nsp = s3mh_nsp(a.TW, J, a.NH);
    bf16_t* st_hi = reinterpret_cast<bf16_t*>(smem);
    float* SP = reinterpret_cast<float*>(smem + s3mh_off_sp(a.SW, a.NH, DH, LO));           // P, later unchanged
    const int inner = a.NH * DH, nn = a.NH * a.NH;
    float* DP = SP + nsp;                                                   // dP' -> dP -> ds
    float* RED = SP + s3mh_spdp(a.TW, J, a.NH, DH);                         // [NG][NH*NH] dW_th partials
    __shared__ float wsh[MH * MH];
    const int t = threadIdx.x, c = t & 3, wh = t >> 2, h = wh % a.NH, wt = wh / a.NH;
    const TilePos p = tile_pos(a, a.F * a.H);
    const int w = p.w0 + wt, b = p.b;
    const bool act = wt < p.tw;
    const int i = 1 + p.ry * a.W + w;
    const bool qvalid = act && i < a.ntok;
    const int nq = a.ntok - 1;
    const int nit = p.tw * J;                                               // (query, slot) items of this tile
    load_wsh(a, wsh);
    if (p.ry == 0 && p.w0 == 0) {   // dq of the <bos> row is zero (its query is never used)
        for (int e = t; e < inner; e += blockDim.x) {
            const size_t go = s3mh_g_bos(b, a.ntok, a.ldd, e);
            a.dq[go] = 0;
            if (a.dql) a.dql[go] = 0;
        }
    }
    if (p.ry * a.W + p.w0 + 1 >= a.ntok) {   // tile beyond the sequence: contributes nothing
        for (int e = t; e < nn; e += blockDim.x) a.part_th[s3mh_g_part(p.bid, nn, e)] = 0.f;
        for (int e = t; e < inner; e += blockDim.x) { a.part_k0[s3mh_g_part(p.bid, inner, e)] = 0.f; a.part_v0[s3mh_g_part(p.bid, inner, e)] = 0.f; }
        return;
    }
    float qf[CH], dof[CH];
#pragma unroll
    for (int e = 0; e < CH; ++e) { qf[e] = 0.f; dof[e] = 0.f; }
    uint32_t qp[CH / 2], dop[CH / 2];            // packed bf16 q / dO for the dot2 path (bf16 operand mode)
#pragma unroll
    for (int e = 0; e < CH / 2; ++e) { qp[e] = 0; dop[e] = 0; }
    if (qvalid) {
        const size_t g = s3mh_g_tok(b, a.ntok, i, a.ld, h, c, DH);
        const size_t gd = s3mh_g_tok(b, a.ntok, i, a.lddo, h, c, DH);
        if (LO) {
            load_chunk<CH>(a.q + g, a.ql ? a.ql + g : nullptr, qf);
            load_chunk<CH>(a.dO + gd, a.dOl ? a.dOl + gd : nullptr, dof);
        } else {
            load_pk<CH>(a.q + g, qp);
            load_pk<CH>(a.dO + gd, dop);
        }
    }
    scores_softmax<DH, LO>(a, p, w, wt, h, c, act, qvalid, qf, qp, SP, st_hi, J);
    // P' = mix(P) -> global (needed by bwd_kv); P stays in SP
    for (int item = t; item < nit; item += blockDim.x) {
        const int wq = item / J, j = item % J;
        const int iq = 1 + p.ry * a.W + p.w0 + wq;
        if (iq < a.ntok) {
            float pv[MH];
#pragma unroll
            for (int hh = 0; hh < MH; ++hh) pv[hh] = hh < a.NH ? SP[s3mh_tab_item(item, hh, a.NH)] : 0.f;
#pragma unroll 1
            for (int g = 0; g < a.NH; ++g) a.pm[s3mh_g_ws(b, nq, iq - 1, J, j, a.NH, g)] = mix_row<false>(wsh, pv, g);
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
        const size_t g = s3mh_g_k0(b, a.k0_bs, h, c, DH);
        const float s = dov(a.v0 + g, a.v0l ? a.v0l + g : nullptr, 8);
        if (c == 0) DP[s3mh_tab(wt, 0, h, J, a.NH)] = s;
    }
    sweep_taps<CH>(a, a.v, a.vl, p, w, h, c, qvalid, st_hi, [&](int j, const bf16_t* vhi, const bf16_t* vlo, int hs) {
        const float s = dov(vhi, vlo, hs);
        if (c == 0) DP[s3mh_tab(wt, j, h, J, a.NH)] = s;
    });
    __syncthreads();
    // dW_th[g][h] partial = sum_{wt,j} dP'[g] * P[h]: unit u = grp*NH*NH + pair takes the items grp, grp + NG, ... of pair (g, h); the units
    // loop over the threads (64 .. 512 of them for up to NG * 256 units), then pair by pair the NG group sums are added in group order
    {
        for (int u = t; u < S3MH_NG * nn; u += blockDim.x) {
            const int grp = u / nn, pair = u - grp * nn;
            const int g = pair / a.NH, hh = pair - g * a.NH;
            float acc = 0.f;
            for (int item = grp; item < nit; item += S3MH_NG) acc += DP[s3mh_tab_item(item, g, a.NH)] * SP[s3mh_tab_item(item, hh, a.NH)];
            RED[s3mh_red(grp, pair, a.NH)] = acc;
        }
        __syncthreads();
        for (int pair = t; pair < nn; pair += blockDim.x) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < S3MH_NG; ++k) s += RED[s3mh_red(k, pair, a.NH)];
            a.part_th[s3mh_g_part(p.bid, nn, pair)] = s;
        }
        __syncthreads();
    }
    // dP[h] = sum_g Wth[g][h] dP'[g]   (in place, item-local)
    for (int item = t; item < nit; item += blockDim.x) {
        float dv_[MH];
#pragma unroll
        for (int g = 0; g < MH; ++g) dv_[g] = g < a.NH ? DP[s3mh_tab_item(item, g, a.NH)] : 0.f;
#pragma unroll 1
        for (int hh = 0; hh < a.NH; ++hh) DP[s3mh_tab_item(item, hh, a.NH)] = mix_row<true>(wsh, dv_, hh);
    }
    __syncthreads();
    // ds = P * (dP - sum_j P dP)
    if (act) {
        float d = 0.f;
        for (int j = c; j < J; j += 4) d += SP[s3mh_tab(wt, j, h, J, a.NH)] * DP[s3mh_tab(wt, j, h, J, a.NH)];
        d = quad_sum(d);
        for (int j = c; j < J; j += 4) {
            const int idx = s3mh_tab(wt, j, h, J, a.NH);
            const float dsv = SP[idx] * (DP[idx] - d);
            DP[idx] = dsv;
            if (qvalid) a.ds[s3mh_g_ws(b, nq, i - 1, J, j, a.NH, h)] = dsv;
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
        const size_t g = s3mh_g_k0(b, a.k0_bs, h, c, DH);
        load_chunk<CH>(a.k0 + g, a.k0l ? a.k0l + g : nullptr, kf_);
        const float d0 = DP[s3mh_tab(wt, 0, h, J, a.NH)];
        float pm0 = 0.f;                                        // P'[wt][0][g = h] = sum_hh Wth[h][hh] P[wt][0][hh]
        for (int hh = 0; hh < a.NH; ++hh) pm0 += wsh[s3mh_wsh(h, hh)] * SP[s3mh_tab(wt, 0, hh, J, a.NH)];
#pragma unroll
        for (int e = 0; e < CH; ++e) {
            const float qe = LO ? qf[e] : ((e & 1) ? hi_f(qp[e >> 1]) : lo_f(qp[e >> 1]));
            const float de = LO ? dof[e] : ((e & 1) ? hi_f(dop[e >> 1]) : lo_f(dop[e >> 1]));
            dqf[e] += d0 * kf_[e];
            k0c[e] = a.scale * d0 * qe;
            v0c[e] = pm0 * de;
        }
    }
    sweep_taps<CH>(a, a.k, a.kl, p, w, h, c, qvalid, st_hi, [&](int j, const bf16_t* khi, const bf16_t* klo, int hs) {
        const float dj = DP[s3mh_tab(wt, j, h, J, a.NH)];
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
        const size_t g = s3mh_g_tok(b, a.ntok, i, a.ldd, h, c, DH);
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
            for (int e = 0; e < CH; ++e) RK[s3mh_rk(wt, s3mh_col(h, c, DH) + e, inner)] = which ? v0c[e] : k0c[e];
        }
        __syncthreads();
        for (int e = t; e < inner; e += blockDim.x) {
            float sk = 0.f;
            for (int ww = 0; ww < p.tw; ++ww) sk += RK[s3mh_rk(ww, e, inner)];
            (which ? a.part_v0 : a.part_k0)[s3mh_g_part(p.bid, inner, e)] = sk;
        }
    }
}

template <int DH, bool LO>
__global__ __launch_bounds__(512, 4) void s3mh_bwd_kv_kernel(S3Args a) {
    constexpr int CH = DH / 4;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int J = a.kf * a.kh * a.kw + 1;
    const int stage_elems = s3mh_stage_elems(a.SW, a.NH, DH);
    bf16_t* sq_hi = reinterpret_cast<bf16_t*>(smem);     // four regions of stage_elems: q hi, q lo, dO hi, dO lo
    bf16_t* sq_lo = sq_hi + stage_elems;
    bf16_t* sd_hi = sq_lo + stage_elems;
    bf16_t* sd_lo = sd_hi + stage_elems;
    const int t = threadIdx.x, c = t & 3, wh = t >> 2, h = wh % a.NH, wt = wh / a.NH;
    const TilePos p = tile_pos(a, a.F * a.H);            // key rows of the grid (the launch covers B * F * H * NT workgroups)
    const int w = p.w0 + wt, b = p.b, f = p.f, y = p.y;
    const bool act = wt < p.tw;
    const int ik = 1 + p.ry * a.W + w;                   // key row index inside the sample
    const bool kvalid = act && ik < a.ntok;
    const int nq = a.ntok - 1;
    if (p.ry * a.W + p.w0 + 1 >= a.ntok) return;
    float dkf[CH], dvf[CH];
#pragma unroll
    for (int e = 0; e < CH; ++e) { dkf[e] = 0.f; dvf[e] = 0.f; }
    // planes tpl = ta*kh + tb; the attending query row of plane tpl is (f + (of-ta)df, y + (oh-tb)dh)
    const int nplanes = a.kf * a.kh;
    auto plane = [&](int tpl, int& fq, int& yq) {
        const int ta = tpl / a.kh, tb = tpl - ta * a.kh;
        fq = f + (a.of - ta) * a.df;
        yq = y + (a.oh - tb) * a.dh;
        return fq >= 0 && yq >= 0 && fq < a.F && yq < a.H && (fq * a.H + yq) * a.W + 1 < a.ntok;
    };
    auto next_plane = [&](int tpl) { int fq, yq; while (tpl < nplanes && !plane(tpl, fq, yq)) ++tpl; return tpl; };
    const int HS = s3mh_hs(a.SW, a.NH);
    const int c0 = s3mh_c0(a.NT, p.w0, (a.kw - 1 - a.ow) * a.dw);   // the attending queries sit at w + (ow - tc)*dw
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
                const size_t ci = s3mh_g_ws(b, nq, pq, J, 1 + tp * a.kw + tc, a.NH, h);
                const float dsv = a.ds[ci], pmv = a.pm[ci];
                const int slot = s3mh_st_read(wq - c0, h, c, a.NH);
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
        const size_t g = s3mh_g_tok(b, a.ntok, ik, a.ldd, h, c, DH);
        store_chunk<CH>(a.dk + g, a.dkl ? a.dkl + g : nullptr, dkf);
        store_chunk<CH>(a.dv + g, a.dvl ? a.dvl + g : nullptr, dvf);
    }
}

int s3mh_fwd_launch(const S3Args& a, int dim_head, bool lo, size_t lds, hipStream_t stream) {
    const dim3 grid((unsigned)((size_t)a.B * a.F * a.H * a.NT)), block(s3mh_threads(a.TW, a.NH));
    return s3_if(dim_head == 64, [&](auto d64) { return s3_if(lo, [&](auto lo_c) {
        return s3_launch(s3mh_fwd_kernel<d64() ? 64 : 32, lo_c()>, grid, block, lds, stream, a);
    }); });
}

// query side, then key side, both over the B*F*H*NT (row, tile) workgroups
int s3mh_bwd_launch(const S3Args& a, int dim_head, bool lo, size_t lds_q, size_t lds_kv, hipStream_t stream) {
    const dim3 grid((unsigned)((size_t)a.B * a.F * a.H * a.NT)), block(s3mh_threads(a.TW, a.NH));
    return s3_if(dim_head == 64, [&](auto d64) { return s3_if(lo, [&](auto lo_c) {
        const int rc = s3_launch(s3mh_bwd_q_kernel<d64() ? 64 : 32, lo_c()>, grid, block, lds_q, stream, a);
        return rc ? rc : s3_launch(s3mh_bwd_kv_kernel<d64() ? 64 : 32, lo_c()>, grid, block, lds_kv, stream, a);
    }); });
}

// the envelope: 9 .. 16 heads, dim_head 32 / 64, causal, W <= 64 (checks in the order of the return codes of amdnuwa_sparse3dna_fwd / _bwd)
int s3mh_check(const amdnuwa_s3_geom* g) {
    if (!g) return AMDNUWA_ERR_ARG;
    if (g->dim_head != 32 && g->dim_head != 64) return AMDNUWA_ERR_UNSUPPORTED;
    if (g->heads < S3MH_MIN || g->heads > S3MH_MH || g->noncausal || g->W < 1 || g->W > 64) return AMDNUWA_ERR_UNSUPPORTED;
    if (g->kf < 1 || g->kh < 1 || g->kw < 1 || g->df < 1 || g->dh < 1 || g->dw < 1) return AMDNUWA_ERR_ARG;
    if (g->ntok < 1 || g->ntok - 1 > g->F * g->H * g->W) return AMDNUWA_ERR_ARG;
    const S3mhTile tm = s3mh_tile(g);
    const S3Tile tl = s3_tile(g);
    if (tm.nt != tl.nt || tm.tw != tl.tw) return AMDNUWA_ERR_UNSUPPORTED;    // (the partials of the workspace map are counted with s3_tile())
    return AMDNUWA_OK;
}
void s3mh_fill(S3Args& a, const amdnuwa_s3_geom* g) {
    s3_fill_causal(a, g);
    const S3mhTile tm = s3mh_tile(g);
    a.NT = tm.nt; a.TW = tm.tw; a.SW = tm.sw;
}

}  // namespace

extern "C" int amdnuwa_s3mh_supported(const amdnuwa_s3_geom* g, int lo_operands) {
    return s3mh_check(g) == AMDNUWA_OK && s3mh_lds_need(g, lo_operands != 0) <= S3MH_LDS_MAX ? 1 : 0;
}
extern "C" size_t amdnuwa_sparse3dna_mh_bwd_workspace_bytes(const amdnuwa_s3_geom* g) { return s3mh_check(g) ? 0 : s3_ws_bytes(g); }

extern "C" int amdnuwa_sparse3dna_mh_fwd(const amdnuwa_s3_geom* g, const uint16_t* q, const uint16_t* k, const uint16_t* v,
                                         const uint16_t* q_lo, const uint16_t* k_lo, const uint16_t* v_lo, int ld,
                                         const float* w_th, uint16_t* o, uint16_t* o_lo, int ldo, hipStream_t stream) {
    int rc = s3mh_check(g);
    if (rc) return rc;
    const bool lo = k_lo != nullptr;
    if (s3mh_lds_need(g, lo) > S3MH_LDS_MAX) return AMDNUWA_ERR_UNSUPPORTED;
    if (!q || !k || !v || !w_th || !o || ld % 8 || ldo % 8) return AMDNUWA_ERR_ARG;
    if (g->B <= 0) return AMDNUWA_OK;
    if (lo && (!q_lo || !v_lo)) return AMDNUWA_ERR_ARG;
    S3Args a{};
    s3mh_fill(a, g);
    a.q = q; a.k = k; a.v = v; a.ld = ld;
    if (lo) { a.ql = q_lo; a.kl = k_lo; a.vl = v_lo; }
    a.o = o; a.ol = o_lo; a.ldo = ldo; a.wth = w_th;
    s3_bind_self(a, g, nullptr);
    return s3mh_fwd_launch(a, g->dim_head, lo, s3mh_lds(g, lo).fwd, stream);
}

extern "C" int amdnuwa_sparse3dna_mh_bwd(const amdnuwa_s3_geom* g, const uint16_t* q, const uint16_t* k, const uint16_t* v,
                                         const uint16_t* q_lo, const uint16_t* k_lo, const uint16_t* v_lo, int ld,
                                         const float* w_th, const uint16_t* dO, const uint16_t* dO_lo, int lddo,
                                         uint16_t* dq, uint16_t* dk, uint16_t* dv, uint16_t* dq_lo, uint16_t* dk_lo,
                                         uint16_t* dv_lo, int ldd, float* dw_th, int accumulate, void* workspace,
                                         size_t workspace_bytes, hipStream_t stream) {
    int rc = s3mh_check(g);
    if (rc) return rc;
    const bool has_lo = k_lo != nullptr, lo = has_lo || dO_lo != nullptr;
    if (s3mh_lds_need(g, has_lo) > S3MH_LDS_MAX) return AMDNUWA_ERR_UNSUPPORTED;
    if (!q || !k || !v || !w_th || !dO || !dq || !dk || !dv || !dw_th || ld % 8 || lddo % 8 || ldd % 8) return AMDNUWA_ERR_ARG;
    if (!workspace || workspace_bytes < s3_ws_bytes(g)) return AMDNUWA_ERR_WORKSPACE;
    if (g->B <= 0) return AMDNUWA_OK;
    if (has_lo && (!q_lo || !v_lo)) return AMDNUWA_ERR_ARG;
    if (lo && (!has_lo || !dO_lo)) return AMDNUWA_ERR_ARG;          // hi + lo operands need lo parts for q / k / v AND dO
    S3Args a{};
    s3mh_fill(a, g);
    a.q = q; a.k = k; a.v = v; a.ld = ld; a.wth = w_th;
    a.dO = dO; a.lddo = lddo;
    if (lo) { a.ql = q_lo; a.kl = k_lo; a.vl = v_lo; a.dOl = dO_lo; }
    a.dq = dq; a.dk = dk; a.dv = dv; a.dql = dq_lo; a.dkl = dk_lo; a.dvl = dv_lo; a.ldd = ldd;
    a.dwth = dw_th; a.accumulate = accumulate;
    s3_bind_self(a, g, workspace);
    const S3mhLds l = s3mh_lds(g, lo);
    rc = s3mh_bwd_launch(a, g->dim_head, lo, l.bq, l.bkv, stream);
    return rc ? rc : s3_bwd_tail(a, g, workspace, stream);
}
