// Dropout keep masks from a counter-based generator (Philox4x32-10), written in the layouts the masked kernels already read:
//   amdnuwa_keep_mask_linear  one byte (0 / 1) per logical element e0 .. e0 + count - 1: the FeedForward mask [R, C] and the window /
//                             SparseCross2DNA mask [B, nq, J, heads], whose storage index IS the logical index
//   amdnuwa_keep_mask_cattn   keep [B][n][KP], keep_t [B][T][NP], keep0 [B][n] of the masked cattn kernels (bit g = head g kept)
// The decision is a pure function of (seed, logical element) -- include/amdnuwa.h states it -- so it does not depend on the launch shape, on
// the alignment of the output or on how a caller splits the batch.  Plain C++: no LDS in the linear kernel, one 64 x 64 byte tile through LDS
// in the cattn kernel so that keep AND its transpose leave in 16-byte stores of contiguous row segments.  All index arithmetic is 64-bit.
#include "common.h"
#include "../../include/amdnuwa.h"

namespace {

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u, PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;

struct U4 {
    uint32_t x, y, z, w;
};

// Philox4x32-10 of the counter (group mod 2^32, group >> 32, 0, 0) under the key (k0, k1)
__device__ __forceinline__ U4 philox(uint64_t group, uint32_t k0, uint32_t k1) {
    uint32_t c0 = (uint32_t)group, c1 = (uint32_t)(group >> 32), c2 = 0u, c3 = 0u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(PHILOX_M0, c0), l0 = PHILOX_M0 * c0;
        const uint32_t h1 = __umulhi(PHILOX_M1, c2), l1 = PHILOX_M1 * c2;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += PHILOX_W0;
        k1 += PHILOX_W1;
    }
    return U4{c0, c1, c2, c3};
}

// the four decisions of one group as bits 0..3 (bit k: word k >= thr, element 4 * group + k is kept)
__device__ __forceinline__ uint32_t keep4(uint64_t group, uint32_t k0, uint32_t k1, uint32_t thr) {
    const U4 v = philox(group, k0, k1);
    return (v.x >= thr ? 1u : 0u) | (v.y >= thr ? 2u : 0u) | (v.z >= thr ? 4u : 0u) | (v.w >= thr ? 8u : 0u);
}

// bits 0..3 -> four bytes of 0 / 1 (the four shifted copies do not overlap: no carries)
__device__ __forceinline__ uint32_t spread4(uint32_t nib) { return ((nib & 15u) * 0x00204081u) & 0x01010101u; }

// keep[i] for i < count.  head = bytes in front of the first 16-byte aligned address (<= count), chunks = 16-byte pieces behind them, the
// rest is the tail; every piece is one aligned 16-byte store, head and tail bytes are written one per thread.
__global__ __launch_bounds__(256) void keep_linear_kernel(uint8_t* __restrict__ keep, long long count, uint64_t e0, uint32_t thr,
                                                          const uint64_t* __restrict__ seed, int head, long long chunks) {
    const uint32_t k0 = (uint32_t)seed[0], k1 = (uint32_t)seed[1];
    const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t eb = e0 + (uint64_t)head;
    const uint32_t s = (uint32_t)(eb & 3u);                     // (uniform: pieces advance by 16 elements)
    for (long long c = gid; c < chunks; c += (long long)gridDim.x * blockDim.x) {
        const uint64_t g0 = (eb + (uint64_t)c * 16u) >> 2;
        uint32_t bits = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) bits |= keep4(g0 + q, k0, k1, thr) << (4 * q);
        if (s) bits |= keep4(g0 + 4, k0, k1, thr) << 16;        // a piece that starts inside a group ends inside a fifth one
        bits >>= s;
        *reinterpret_cast<uint4*>(keep + head + c * 16) = make_uint4(spread4(bits), spread4(bits >> 4), spread4(bits >> 8), spread4(bits >> 12));
    }
    const long long tail0 = head + chunks * 16;
    const long long edge = head + (count - tail0);              // < 32
    if (gid < edge) {
        const long long i = gid < head ? gid : tail0 + (gid - head);
        const uint64_t e = e0 + (uint64_t)i;
        keep[i] = (uint8_t)((keep4(e >> 2, k0, k1, thr) >> (uint32_t)(e & 3u)) & 1u);
    }
}

constexpr int CT = 64;                  // the tile: 64 queries x 64 key rows, one byte each
constexpr int CPITCH = CT + 4;          // LDS row pitch (bytes; a multiple of 4: rows are written as 32-bit words)

// the byte of (sample, query, key slot) number idx: bit g = element 8 * idx + g is kept, g < heads
__device__ __forceinline__ uint32_t keep_byte(uint64_t idx, int heads, uint32_t k0, uint32_t k1, uint32_t thr) {
    uint32_t b = keep4(2 * idx, k0, k1, thr);
    if (heads > 4) b |= keep4(2 * idx + 1, k0, k1, thr) << 4;
    return b & ((1u << heads) - 1u);
}

template <bool A16>
__device__ __forceinline__ void store16(uint8_t* p, const uint32_t* w) {
    if (A16) {
        *reinterpret_cast<uint4*>(p) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) reinterpret_cast<uint32_t*>(p)[q] = w[q];
    }
}

// one workgroup = one tile of one sample: thread (r, c) = (tid / 4, tid % 4) decides the 16 bytes of query row r, key rows 16 c .. 16 c + 15,
// stores them into keep and into LDS; after the barrier it gathers the 16 bytes of key row r, queries 16 c .. 16 c + 15 and stores them into
// keep_t.  Four neighbouring lanes cover 64 contiguous bytes of a row on either side.  Bytes outside n x T are zero.
template <bool AK16, bool AT16>
__global__ __launch_bounds__(256) void keep_cattn_kernel(uint8_t* __restrict__ keep, uint8_t* __restrict__ keep_t, uint8_t* __restrict__ keep0,
                                                         int n, int T, int heads, uint64_t b_first, uint32_t thr,
                                                         const uint64_t* __restrict__ seed, int KP, int NP, int nti, int ntj) {
    __shared__ uint32_t tile[CT * CPITCH / 4];
    const uint32_t k0 = (uint32_t)seed[0], k1 = (uint32_t)seed[1];
    const uint32_t blk = blockIdx.x;
    const int tj = (int)(blk % (uint32_t)ntj), ti = (int)((blk / (uint32_t)ntj) % (uint32_t)nti);
    const size_t b = blk / ((uint32_t)ntj * (uint32_t)nti);
    const int r = threadIdx.x >> 2, c = (threadIdx.x & 3) * 16;
    {
        const int i = ti * CT + r, t0 = tj * CT + c;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        if (i < n) {
            const uint64_t idx = ((b_first + b) * (uint64_t)n + (uint64_t)i) * (uint64_t)(T + 1) + 1u + (uint64_t)t0;     // slot j = t + 1
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (t0 + k < T) w[k >> 2] |= keep_byte(idx + k, heads, k0, k1, thr) << (8 * (k & 3));
            if (t0 + 16 <= KP) store16<AK16>(keep + (b * n + i) * (size_t)KP + t0, w);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) tile[(r * CPITCH + c) / 4 + q] = w[q];
    }
    if (tj == 0 && threadIdx.x < CT) {                          // the null slot (j = 0) of this tile's queries
        const int i = ti * CT + (int)threadIdx.x;
        if (i < n) keep0[b * n + i] = (uint8_t)keep_byte(((b_first + b) * (uint64_t)n + (uint64_t)i) * (uint64_t)(T + 1), heads, k0, k1, thr);
    }
    __syncthreads();
    {
        const int t = tj * CT + r, i0 = ti * CT + c;
        if (t < T && i0 + 16 <= NP) {
            const uint8_t* bytes = reinterpret_cast<const uint8_t*>(tile);
            uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int k = 0; k < 16; ++k) w[k >> 2] |= (uint32_t)bytes[(c + k) * CPITCH + r] << (8 * (k & 3));
            store16<AT16>(keep_t + (b * T + t) * (size_t)NP + i0, w);
        }
    }
}

inline bool al(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

extern "C" int amdnuwa_keep_mask_linear(uint8_t* keep, long long count, long long e0, uint32_t thr, const uint64_t* seed, hipStream_t stream) {
    if (!keep || !seed || count <= 0 || e0 < 0 || !al(seed, 8)) return AMDNUWA_ERR_ARG;
    long long head = (long long)((16u - ((uintptr_t)keep & 15u)) & 15u);
    if (head > count) head = count;
    const long long chunks = (count - head) / 16;
    long long blocks = (chunks + 255) / 256;
    blocks = blocks < 1 ? 1 : (blocks > 16384 ? 16384 : blocks);
    hipLaunchKernelGGL(keep_linear_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, keep, count, (uint64_t)e0, thr, seed, (int)head, chunks);
    LAUNCH_CHECK();
    return AMDNUWA_OK;
}

extern "C" int amdnuwa_keep_mask_cattn(uint8_t* keep, uint8_t* keep_t, uint8_t* keep0, int B, int n, int T, int heads, long long b_first,
                                       uint32_t thr, const uint64_t* seed, hipStream_t stream) {
    if (!keep || !keep_t || !keep0 || !seed || !al(seed, 8)) return AMDNUWA_ERR_ARG;
    if (heads < 1 || heads > 8 || B <= 0 || n <= 0 || T <= 0 || b_first < 0) return AMDNUWA_ERR_ARG;
    if (!al(keep, 4) || !al(keep_t, 4)) return AMDNUWA_ERR_ARG;
    if (n > INT32_MAX - 64 || T > INT32_MAX - 64) return AMDNUWA_ERR_ARG;
    const int KP = (T + 31) / 32 * 32, NP = (n + 31) / 32 * 32;
    const int nti = (n + CT - 1) / CT, ntj = (T + CT - 1) / CT;
    const unsigned long long blocks = (unsigned long long)B * (unsigned long long)nti * (unsigned long long)ntj;
    if (blocks > 0x7fffffffull) return AMDNUWA_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)blocks), block(256);
#define KEEP_CATTN(AK, AT)                                                                                                          \
    hipLaunchKernelGGL((keep_cattn_kernel<AK, AT>), grid, block, 0, stream, keep, keep_t, keep0, n, T, heads, (uint64_t)b_first, thr, \
                       seed, KP, NP, nti, ntj)
    const bool ak = al(keep, 16), at = al(keep_t, 16);
    if (ak && at) KEEP_CATTN(true, true);
    else if (ak) KEEP_CATTN(true, false);
    else if (at) KEEP_CATTN(false, true);
    else KEEP_CATTN(false, false);
#undef KEEP_CATTN
    LAUNCH_CHECK();
    return AMDNUWA_OK;
}
