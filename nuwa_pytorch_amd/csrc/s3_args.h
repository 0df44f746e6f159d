// Argument block and the lane-level helpers shared by the Sparse3DNA window kernels: the row kernels and the MFMA band kernels of
// sparse3dna.hip, the column-tiled kernels of sparse3dna_wide.hip.  Everything here has internal linkage (one copy per translation unit).
#pragma once
#include <type_traits>
#include "common.h"
#include "../../include/amdnuwa.h"

struct S3Args {
    const bf16_t *q, *k, *v, *ql, *kl, *vl; int ld;       // q/k/v rows: [B*ntok, ld]
    bf16_t *o, *ol; int ldo;                              // fwd out
    int ol_f16;                                           // fp16 forward: ol receives the FP16 rendering of the output (the to_out GEMM's fp16 operand), not the bf16 residual
    const bf16_t *dO, *dOl; int lddo;                     // bwd in
    bf16_t *dq, *dk, *dv, *dql, *dkl, *dvl; int ldd;      // bwd out
    const float* wth;                                     // [NH][NH] talking heads (g, h)
    const float* bias;                                    // [J][NH] relative-position bias per key slot (or NULL)
    float *ds, *pm;                                       // [B][nq][J][NH]
    float* stats;                                         // recomputing key side (MFMA path): [B][nq][NH][4] = (row max, 1 / row sum, delta = sum_j P dP, -);
                                                          // non-NULL = the query side writes these INSTEAD of the ds / pm workspace
    float *part_th, *part_k0, *part_v0;                   // [B*F*H][NH*NH], [B*F*H][NH*DH] x2
    float* dwth;                                          // [NH*NH] accumulated
    int B, ntok, F, H, W, kf, kh, kw, df, dh, dw, NH;
    int of, oh, ow;                                       // tap index of the query's own position per axis: k - 1 (causal) / (k - 1) / 2 (symmetric)
    // key / value side.  Self-attention (Sparse3DNA): the query sequence itself, row 0 = <bos> = key slot 0.  xmode = 1 (SparseCross2DNA,
    // np.py:761-901): keys / values are a context grid of FK = kf frames, tap a of the frame axis IS context frame a (absolute), slot 0
    // is a learned null key / value, keys can be masked, and query row 0 (<bos>) is left to the host (it attends to everything).
    int xmode, FK, kvrows, kvoff, ldk, lddk;              // rows per sample / first grid row / row strides of the k, v (dk, dv) tensors
    const bf16_t *k0, *k0l, *v0, *v0l; long long k0_bs;   // slot-0 key / value rows [NH*DH] and their per-sample stride (elements)
    const uint8_t* kmask;                                 // [B][kvrows] (1 = visible) or NULL
    float *dnull_k, *dnull_v;                             // xmode: gradients of the null key / value [NH*DH] (fp32)
    float scale;
    int accumulate;
    int dbg;                                              // probe only (tuning key 9): bit 0 / 1 / 2 skip phase 1 / 2 / 3 of the MFMA forward
    int ymajor;                                           // MFMA kernels: workgroup order inside a sample is (y, f) instead of (f, y) (tuning key 3 bit 1 = old order)
    int sep_passes;                                       // MFMA query-side backward: the three separate item passes instead of the fused one (tuning key 19 = 1)
    int packed;                                           // MFMA backward (round 5): the ds / P' workspace is ONE array of (bf16 ds | bf16 P') words at `pm`
    const float* gs2;                                     // fp16-gradient backward (round 6, amdnuwa_sparse3dna_bwd_f16): device {S, 1 / S}; q / k / v / dO hold fp16 values,
                                                          // dO = fp16(S dO), dq / dk / dv leave as fp16(S gradient), the workspace words are (fp16 S ds | fp16 P'), dW_th leaves times 1 / S
    int NT, TW, SW;                                       // column tiles of a grid row (sparse3dna_wide.hip): tiles per row, queries (keys) per tile, staged columns of a
                                                          // tile = TW + (kw-1)*dw halo.  NT = 1: one workgroup per row (TW = SW = W); the per-workgroup partials are [row][tile]
};

// Attention dropout (the DROP forms of the VALU forward and query-side backward): keep mask [B][nq][J][NH] in the index order of the ds / P'
// workspace (nonzero = keep) and s = 1 / (1 - p): P'' = keep . P' . s feeds the V product and dV, dP' = keep . dP'' . s.  Only the DROP
// instantiations take the two extra words: the kernel argument of the unmasked ones stays S3Args itself.
struct S3DropArgs : S3Args { const uint8_t* keep; float drop_s; };
template <bool DROP> struct S3KArgsSel { using type = S3Args; };
template <> struct S3KArgsSel<true> { using type = S3DropArgs; };
template <bool DROP> using S3KArgs = typename S3KArgsSel<DROP>::type;
template <bool DROP> inline S3KArgs<DROP> s3_kargs(const S3Args& a, const uint8_t* keep, float drop_s) {
    if constexpr (DROP) {
        S3DropArgs d{};
        static_cast<S3Args&>(d) = a;
        d.keep = keep; d.drop_s = drop_s;
        return d;
    } else {
        return a;
    }
}

// Column tiling of a grid row.  A row whose thread map ((w*heads + h)*4 + c) fits 512 threads is ONE tile without halo (the row kernels of
// sparse3dna.hip); a wider one is cut into nt tiles of tw consecutive columns, tw*heads*4 <= 512, the tiles balanced (tw = ceil(W / nt)).
// A tile stages its own columns plus the halo the kw taps reach: (kw-1)*dw columns in all -- to the left of the queries (right of the keys)
// under the causal window, split (kw-1)/2 : kw-1-(kw-1)/2 around them under the symmetric one -- so sw does not depend on the window form.
struct S3Tile { int tw, nt, sw; };
inline S3Tile s3_tile(const amdnuwa_s3_geom* g) {
    if (g->W * g->heads * 4 <= 512) return {g->W, 1, g->W};
    const int twmax = 128 / g->heads, nt = (g->W + twmax - 1) / twmax, tw = (g->W + nt - 1) / nt;
    long long halo = (long long)(g->kw - 1) * g->dw;
    if (halo > 65536) halo = 65536;                       // (far beyond any LDS: s3_lds_need refuses it, no kernel sees the clipped value)
    return {tw, nt, tw + (int)halo};
}
// key slots of a query: slot 0 (<bos>, or the null key of SparseCross2DNA) + the kf*kh*kw window taps
inline size_t s3_slots(const amdnuwa_s3_geom* g) { return (size_t)g->kf * g->kh * g->kw + 1; }

// One launch of a window kernel: launch_kernel() of common.h with the dynamic-LDS allowance set on every launch.
template <class A>
int s3_launch(void (*kernel)(A), dim3 grid, dim3 block, size_t lds, hipStream_t stream, const A& args) {
    return launch_kernel(kernel, grid, block, lds, true, stream, args);
}
// Run-time choices as compile-time parameters (launch_if of common.h); s3_dispatch() hands f the template parameters
// <DH, LO, DROP> of the VALU kernels as (std::integral_constant<int, 64 or 32>, bool constant, bool constant).
template <class F> int s3_if(bool c, F&& f) { return launch_if(c, f); }
template <class F> int s3_dispatch(int dim_head, bool lo, bool drop, F&& f) {
    return s3_if(dim_head == 64, [&](auto d64) { return s3_if(lo, [&](auto lo_c) { return s3_if(drop, [&](auto dr) {
        return f(std::integral_constant<int, d64() ? 64 : 32>{}, lo_c, dr);
    }); }); });
}

// launchers of the column-tiled kernels (sparse3dna_wide.hip); `a` is complete, a.NT > 1.  lds_* = dynamic LDS bytes of the launch.
// keep != NULL launches the masked (DROP) forms of the forward and of the query-side backward
int s3w_fwd_launch(const S3Args& a, int dim_head, bool lo, size_t lds, const uint8_t* keep, float drop_s, hipStream_t stream);
int s3w_bwd_launch(const S3Args& a, int dim_head, bool lo, size_t lds_q, size_t lds_kv, const uint8_t* keep, float drop_s, hipStream_t stream);
// host-side pieces of sparse3dna.hip that the many-head entry points (sparse3dna_mh.hip, 9 .. 16 heads, causal) reuse, generic in the head count:
// bytes of the backward workspace (the s3_ws() map); geometry fields of `a` for the causal self-attention window (tile fields from s3_tile());
// slot-0 key / value = the <bos> row, and (workspace != NULL) the workspace pointers; final sums of the backward + the d(rel_bias) column sums
size_t s3_ws_bytes(const amdnuwa_s3_geom* g);
void s3_fill_causal(S3Args& a, const amdnuwa_s3_geom* g);
void s3_bind_self(S3Args& a, const amdnuwa_s3_geom* g, void* workspace);
int s3_bwd_tail(const S3Args& a, const amdnuwa_s3_geom* g, void* workspace, hipStream_t stream);

namespace {

// a 16-bit element of an operand array as fp32: bf16, or (F16) fp16
template <bool F16> __device__ __forceinline__ float ld16_t(bf16_t v) { return F16 ? (float)__builtin_bit_cast(_Float16, v) : bf2f(v); }

constexpr float NEG_MAX = -3.4028234663852886e38f;

// Workgroups are handed to the 8 XCDs round-robin by linear id; every XCD has its own L2.  Consecutive query rows share
// almost all of their key / value rows, so the logical row id is remapped to give each XCD one CONTIGUOUS range of rows
// (whole samples): its L2 then holds the few frames in flight instead of an eighth of everything (bijective for any grid).
__device__ __forceinline__ int xcd_row_id() {
    const int nb = gridDim.x, id = blockIdx.x, per = nb >> 3, rem = nb & 7, x = id & 7, k = id >> 3;
    return x * per + (x < rem ? x : rem) + k;
}


// hs = element stride between the 8-element halves of a chunk (8 = contiguous; the LDS stage keeps the two
// 16-byte halves of every chunk in separate regions so that ds_read_b128 lanes are 16 bytes apart: no conflicts)
template <int CH>
__device__ __forceinline__ void load_chunk(const bf16_t* hi, const bf16_t* lo, float* f, int hs = 8) {
#pragma unroll
    for (int v8 = 0; v8 < CH / 8; ++v8) {
        const uint4 u = *reinterpret_cast<const uint4*>(hi + v8 * hs);
        f[v8 * 8 + 0] = lo_f(u.x); f[v8 * 8 + 1] = hi_f(u.x); f[v8 * 8 + 2] = lo_f(u.y); f[v8 * 8 + 3] = hi_f(u.y);
        f[v8 * 8 + 4] = lo_f(u.z); f[v8 * 8 + 5] = hi_f(u.z); f[v8 * 8 + 6] = lo_f(u.w); f[v8 * 8 + 7] = hi_f(u.w);
        if (lo) {
            const uint4 l = *reinterpret_cast<const uint4*>(lo + v8 * hs);
            f[v8 * 8 + 0] += lo_f(l.x); f[v8 * 8 + 1] += hi_f(l.x); f[v8 * 8 + 2] += lo_f(l.y); f[v8 * 8 + 3] += hi_f(l.y);
            f[v8 * 8 + 4] += lo_f(l.z); f[v8 * 8 + 5] += hi_f(l.z); f[v8 * 8 + 6] += lo_f(l.w); f[v8 * 8 + 7] += hi_f(l.w);
        }
    }
}
template <int CH>
__device__ __forceinline__ void store_chunk(bf16_t* hi, bf16_t* lo, const float* f) {
#pragma unroll
    for (int v8 = 0; v8 < CH / 8; ++v8) {
        bf16_t h[8], l[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) f2bf_hilo(f[v8 * 8 + e], h[e], l[e]);
        *reinterpret_cast<uint4*>(hi + v8 * 8) = make_uint4(pack2(h[0], h[1]), pack2(h[2], h[3]), pack2(h[4], h[5]), pack2(h[6], h[7]));
        if (lo) *reinterpret_cast<uint4*>(lo + v8 * 8) = make_uint4(pack2(l[0], l[1]), pack2(l[2], l[3]), pack2(l[4], l[5]), pack2(l[6], l[7]));
    }
}
// reductions over the 4 lanes of a (query, head) group with DPP quad permutes (no LDS traffic)
__device__ __forceinline__ float dpp_quad(float v, int ctrl_b1) {
    const int i = __builtin_bit_cast(int, v);
    const int r = ctrl_b1 ? __builtin_amdgcn_mov_dpp(i, 0xB1, 0xF, 0xF, true)     // quad_perm [1,0,3,2]
                          : __builtin_amdgcn_mov_dpp(i, 0x4E, 0xF, 0xF, true);    // quad_perm [2,3,0,1]
    return __builtin_bit_cast(float, r);
}
__device__ __forceinline__ float quad_sum(float v) {
    v += dpp_quad(v, 1);
    v += dpp_quad(v, 0);
    return v;
}
// factor of one (query, slot, head) entry under attention dropout: s where the mask keeps it, exactly 0 where it drops it
__device__ __forceinline__ float keep_factor(uint8_t k, float s) { return k ? s : 0.f; }
__device__ __forceinline__ float quad_max(float v) {
    v = fmaxf(v, dpp_quad(v, 1));
    v = fmaxf(v, dpp_quad(v, 0));
    return v;
}

// packed bf16 arithmetic (bf16 operand mode): v_dot2_f32_bf16 multiplies two bf16 pairs and accumulates in fp32
template <int CH>
__device__ __forceinline__ void load_pk(const bf16_t* p, uint32_t* pk, int hs = 8) {
#pragma unroll
    for (int v8 = 0; v8 < CH / 8; ++v8) {
        const uint4 u = *reinterpret_cast<const uint4*>(p + v8 * hs);
        pk[v8 * 4 + 0] = u.x; pk[v8 * 4 + 1] = u.y; pk[v8 * 4 + 2] = u.z; pk[v8 * 4 + 3] = u.w;
    }
}
__device__ __forceinline__ float dot2(uint32_t a, uint32_t b, float c) {
    return __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2, a), __builtin_bit_cast(bf16x2, b), c, false);
}
template <int CH>
__device__ __forceinline__ float dot_pk(const uint32_t* a, const uint32_t* b) {
    float s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int i = 0; i < CH / 2; i += 2) { s0 = dot2(a[i], b[i], s0); s1 = dot2(a[i + 1], b[i + 1], s1); }
    return s0 + s1;
}
// acc[e] += coef * v[e] with coef rounded to bf16: one dot2 per element, no unpacking
template <int CH>
__device__ __forceinline__ void axpy_pk(float* acc, float coef, const uint32_t* v) {
    const uint32_t clo = f2bf(coef), chi = clo << 16;
#pragma unroll
    for (int i = 0; i < CH / 2; ++i) {
        acc[2 * i] = dot2(v[i], clo, acc[2 * i]);
        acc[2 * i + 1] = dot2(v[i], chi, acc[2 * i + 1]);
    }
}

}  // namespace
