// FeedForward dropout (np.py:276: nn.Dropout on the GEGLU output, between the two products) as two bandwidth kernels:
//   amdnuwa_geglu_dropout_fwd     out = keep ? in * scale : 0 over the gate output [R, C], in the 16-bit forms the FF2 product reads
//   amdnuwa_geglu_il_bwd_dropout  amdnuwa_geglu_il_bwd with the mask applied to the incoming gradient in registers
// The keep mask is a byte per element (a torch.bool tensor drawn from torch's RNG stream by the caller); scale = 1 / (1 - p).
// One pass, 16-byte loads and stores of the 16-bit tensors (8 elements per lane, 8 mask bytes), no LDS.  The arithmetic is the one of
// the element-wise formulation it replaces, operation by operation (one fp32 multiply, a select, the stores' roundings): the results are
// bit-identical to it, which tests/test_gpu_dropout.py checks.
#include "common.h"
#include "../../include/amdnuwa.h"
#include <cmath>

namespace {

constexpr int ROWS_PER_BLOCK = 4;

inline int grid_for(size_t work, int per_block = 256, int cap = 2048) {
    size_t b = (work + per_block - 1) / per_block;
    return (int)(b < 1 ? 1 : (b > (size_t)cap ? (size_t)cap : b));
}

__device__ __forceinline__ void unpack8_bf(const uint4& v, float* f) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) { f[2 * k] = lo_f(w[k]); f[2 * k + 1] = hi_f(w[k]); }
}
__device__ __forceinline__ void unpack8_f16(const uint4& v, float* f) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) { f[2 * k] = f16lo_f(w[k]); f[2 * k + 1] = f16hi_f(w[k]); }
}
// value of 8 bf16 hi[/lo] elements: hi + lo in fp32, as every reader of a pair forms it
template <bool LO>
__device__ __forceinline__ void load8_bf(const bf16_t* hi, const bf16_t* lo, size_t off, float* f) {
    unpack8_bf(*reinterpret_cast<const uint4*>(hi + off), f);
    if (LO) {
        float l[8];
        unpack8_bf(*reinterpret_cast<const uint4*>(lo + off), l);
#pragma unroll
        for (int k = 0; k < 8; ++k) f[k] += l[k];
    }
}
// the split of amdnuwa_cast_pad (f2bf_hilo: hi = bf16(f), lo = bf16(f - hi)), 8 elements
template <bool LO>
__device__ __forceinline__ void store8_bf(bf16_t* hi, bf16_t* lo, size_t off, const float* f) {
    bf16_t h[8], l[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) f2bf_hilo(f[k], h[k], l[k]);
    *reinterpret_cast<uint4*>(hi + off) = make_uint4(pack2(h[0], h[1]), pack2(h[2], h[3]), pack2(h[4], h[5]), pack2(h[6], h[7]));
    if (LO) *reinterpret_cast<uint4*>(lo + off) = make_uint4(pack2(l[0], l[1]), pack2(l[2], l[3]), pack2(l[4], l[5]), pack2(l[6], l[7]));
}
// the gate copies of the fp16 forward: bf16 by the converter (round to nearest even, NaN kept)
__device__ __forceinline__ void store8_bf_cvt(bf16_t* hi, size_t off, const float* f) {
    *reinterpret_cast<uint4*>(hi + off) = make_uint4(pack2_rne(f[0], f[1]), pack2_rne(f[2], f[3]), pack2_rne(f[4], f[5]), pack2_rne(f[6], f[7]));
}
__device__ __forceinline__ void store8_f16_sat(uint16_t* o, size_t off, const float* f) {
    *reinterpret_cast<uint4*>(o + off) = make_uint4(pack2_f16_sat(f[0], f[1]), pack2_f16_sat(f[2], f[3]), pack2_f16_sat(f[4], f[5]), pack2_f16_sat(f[6], f[7]));
}

// nn.Dropout in training on 8 values: kept entries times scale (ONE fp32 multiply, never contracted into a neighbouring add: the
// hi / lo split below subtracts from the product), the others exactly +0 -- a select, so a dropped NaN or inf becomes 0 as torch.where makes it
__device__ __forceinline__ void drop8(float* f, const uint2& kp, float scale) {
#pragma clang fp contract(off)
    const uint32_t w[2] = {kp.x, kp.y};
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float s = f[k] * scale;
        f[k] = ((w[k >> 2] >> (8 * (k & 3))) & 0xffu) ? s : 0.f;
    }
}

// F16IN: `in` holds fp16 values, the outputs are the fp16 copy o16 (may alias `in`: a lane reads its 16 bytes before it writes them) and the bf16 copy
// o_hi, both rounded from the same fp32 product.  Otherwise `in` is a bf16 hi[/lo] pair and the output a bf16 hi[/lo] pair.
template <bool F16IN, bool ILO, bool OLO>
__global__ __launch_bounds__(256) void geglu_dropout_fwd_kernel(const uint16_t* in, const uint16_t* in_lo, int ld_in,
                                                                const uint8_t* __restrict__ keep, int ld_keep, float scale,
                                                                bf16_t* o_hi, bf16_t* o_lo, int ld_out, uint16_t* o16, int ld_16,
                                                                long long R, int C) {
    const int cpr = C / 8;                                      // 16-byte chunks per row
    const long long chunks = R * cpr;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < chunks; e += (long long)gridDim.x * blockDim.x) {
        const long long r = e / cpr;
        const int c = (int)(e - r * cpr) * 8;
        float f[8];
        if (F16IN) unpack8_f16(*reinterpret_cast<const uint4*>(in + (size_t)r * ld_in + c), f);
        else load8_bf<ILO>(in, in_lo, (size_t)r * ld_in + c, f);
        const uint2 kp = *reinterpret_cast<const uint2*>(keep + (size_t)r * ld_keep + c);
        drop8(f, kp, scale);
        if (F16IN) {
            store8_f16_sat(o16, (size_t)r * ld_16 + c, f);
            store8_bf_cvt(o_hi, (size_t)r * ld_out + c, f);
        } else {
            store8_bf<OLO>(o_hi, o_lo, (size_t)r * ld_out + c, f);
        }
    }
}

// amdnuwa_geglu_il_bwd (elementwise.hip geglu_bwd_kernel<LO, true>: one wave per token row, u in the interleaved-by-8 layout) reading the
// UNDROPPED dgg: dgd = round(keep ? dgg * scale : 0) in the operand format the two-step path stored (bf16 hi, or hi + lo), in registers
template <bool LO>
__global__ __launch_bounds__(256) void geglu_il_bwd_dropout_kernel(const bf16_t* __restrict__ u_hi, const bf16_t* __restrict__ u_lo,
                                                                   const bf16_t* __restrict__ d_hi, const bf16_t* __restrict__ d_lo,
                                                                   const uint8_t* __restrict__ keep, int ld_keep, float scale,
                                                                   bf16_t* __restrict__ du_hi, bf16_t* __restrict__ du_lo, long long R, int FP) {
    const long long row = (long long)blockIdx.x * ROWS_PER_BLOCK + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (row >= R) return;
    const size_t ub = (size_t)row * 2 * FP, db = (size_t)row * FP, kb = (size_t)row * ld_keep;
    for (int c = (threadIdx.x & 63) * 8; c < FP; c += 512) {
        float a[8], g[8], d[8], da[8], dg[8];
        load8_bf<LO>(u_hi, u_lo, ub + 2 * c, a);
        load8_bf<LO>(u_hi, u_lo, ub + 2 * c + 8, g);
        load8_bf<LO>(d_hi, d_lo, db + c, d);
        drop8(d, *reinterpret_cast<const uint2*>(keep + kb + c), scale);
#pragma unroll
        for (int k = 0; k < 8; ++k) {           // what the gate's backward would have read back from the dropped copy
            bf16_t h, l;
            f2bf_hilo(d[k], h, l);
            d[k] = LO ? bf2f(h) + bf2f(l) : bf2f(h);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float y, dy;
            gelu_both_f(g[k], y, dy);
            da[k] = d[k] * y;
            dg[k] = d[k] * a[k] * dy;
        }
        // (the stores of geglu_bwd_kernel: the converter for a hi-only result, the hi / lo split otherwise)
        if (LO) {
            store8_bf<true>(du_hi, du_lo, ub + 2 * c, da);
            store8_bf<true>(du_hi, du_lo, ub + 2 * c + 8, dg);
        } else {
            store8_bf_cvt(du_hi, ub + 2 * c, da);
            store8_bf_cvt(du_hi, ub + 2 * c + 8, dg);
        }
    }
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
inline bool al8(const void* p) { return ((uintptr_t)p & 7u) == 0; }
inline bool scale_ok(float s) { return std::isfinite(s) && s >= 1.f; }

}  // namespace

extern "C" int amdnuwa_geglu_dropout_fwd(const uint16_t* in, const uint16_t* in_lo, int ld_in, int in_f16, const uint8_t* keep, int ld_keep,
                                         float scale, uint16_t* out, uint16_t* out_lo, int ld_out, uint16_t* out_f16, int ld_f16,
                                         long long R, int C, hipStream_t stream) {
    if (!in || !keep || !out) return AMDNUWA_ERR_ARG;
    if (in_f16 ? (!out_f16 || in_lo || out_lo) : (out_f16 != nullptr)) return AMDNUWA_ERR_ARG;
    if (!scale_ok(scale) || C <= 0 || C % 8) return AMDNUWA_ERR_ARG;
    // 16-byte accesses of the 16-bit tensors, 8-byte accesses of the mask: row pitches in multiples of 8 elements, aligned bases
    if (ld_in < C || ld_in % 8 || ld_out < C || ld_out % 8 || ld_keep < C || ld_keep % 8) return AMDNUWA_ERR_ARG;
    if (in_f16 && (ld_f16 < C || ld_f16 % 8)) return AMDNUWA_ERR_ARG;
    if (!al16(in) || !al16(in_lo) || !al16(out) || !al16(out_lo) || !al16(out_f16) || !al8(keep)) return AMDNUWA_ERR_ARG;
    if (R <= 0) return AMDNUWA_OK;
    const dim3 grid(grid_for((size_t)R * (C / 8))), block(256);
#define DROP_FWD(F16IN, ILO, OLO)                                                                                                  \
    hipLaunchKernelGGL((geglu_dropout_fwd_kernel<F16IN, ILO, OLO>), grid, block, 0, stream, in, in_lo, ld_in, keep, ld_keep, scale, \
                       out, out_lo, ld_out, out_f16, ld_f16, R, C)
    if (in_f16) DROP_FWD(true, false, false);
    else if (in_lo && out_lo) DROP_FWD(false, true, true);
    else if (in_lo) DROP_FWD(false, true, false);
    else if (out_lo) DROP_FWD(false, false, true);
    else DROP_FWD(false, false, false);
#undef DROP_FWD
    LAUNCH_CHECK();
    return AMDNUWA_OK;
}

extern "C" int amdnuwa_geglu_il_bwd_dropout(const uint16_t* u_hi, const uint16_t* u_lo, const uint16_t* d_hi, const uint16_t* d_lo,
                                            const uint8_t* keep, int ld_keep, float scale, uint16_t* du_hi, uint16_t* du_lo,
                                            long long R, int FP, hipStream_t stream) {
    if (!u_hi || !d_hi || !du_hi || !keep) return AMDNUWA_ERR_ARG;
    if ((u_lo != nullptr) != (d_lo != nullptr) || (u_lo != nullptr) != (du_lo != nullptr)) return AMDNUWA_ERR_ARG;
    if (!scale_ok(scale) || FP <= 0 || FP % 8 || ld_keep < FP || ld_keep % 8) return AMDNUWA_ERR_ARG;
    if (!al16(u_hi) || !al16(u_lo) || !al16(d_hi) || !al16(d_lo) || !al16(du_hi) || !al16(du_lo) || !al8(keep)) return AMDNUWA_ERR_ARG;
    if (R <= 0) return AMDNUWA_OK;
    const dim3 rg((unsigned)((R + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK));
    if (u_lo) hipLaunchKernelGGL((geglu_il_bwd_dropout_kernel<true>), rg, dim3(256), 0, stream, u_hi, u_lo, d_hi, d_lo, keep, ld_keep, scale, du_hi, du_lo, R, FP);
    else hipLaunchKernelGGL((geglu_il_bwd_dropout_kernel<false>), rg, dim3(256), 0, stream, u_hi, u_lo, d_hi, d_lo, keep, ld_keep, scale, du_hi, du_lo, R, FP);
    LAUNCH_CHECK();
    return AMDNUWA_OK;
}
