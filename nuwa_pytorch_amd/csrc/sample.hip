// The end of a generate() token on the device (np.py:55-65, 1713-1720, 1883-1908): restrict the guided logits to their `keep` largest,
// draw the Gumbel-max sample among them, record the token id and assemble the decoder input row of the NEXT position
// (token embedding + position embedding) -- one launch at the end of the captured row step instead of the topk / rand / log / argmax /
// gather / cat / embedding / add chain of eager launches.  The step index lives in DEVICE memory, like the row position of the kernels
// in decode.hip, so that one captured launch serves every token.
//
// One workgroup per sample; the row's classes live in registers as 64-bit ORDER WORDS
//     word = (sortable image of the fp32 logit) << ibits | (2^ibits - 1 - class)
// which are pairwise distinct and compare as (larger logit first, lower class first on equal logits): top-`keep` selection, the
// descending order of the kept entries and the tie rule are all plain integer comparisons.
//   1. the keep-th largest word by bisection on its bits: one workgroup-wide count per bit (no histogram, no atomics)
//   2. the words >= it -- exactly `keep` -- are compacted into LDS through a workgroup scan and sorted there (bitonic network)
//   3. score_j = v_j / temperature + g(u_j) for the rank-j entry, first maximum by a (score, rank) reduction
//   4. ids[b][t] = class, x_next[b] = emb[class] + pos[pos_idx[t]] in 16-byte vectors
// Every reduction has a fixed shape: two runs are bit-identical.
#include "common.h"
#include "../../include/amdnuwa.h"

namespace {

constexpr int SAMPLE_MAX_C = 16384;
constexpr int SAMPLE_SMALL_BYTES = 512;            // reductions / scan / broadcast words in front of the sorted words

struct SampleArgs {
    const float *logits, *u, *emb, *pos;
    const int *pos_idx, *step;
    long long* ids;
    float* x_next;
    int C, ld, keep, kpad, ibits, D, P, cap;
    float temperature;
};

// fp32 -> uint32 that compares like the float; -0 counts as +0 and every NaN as the largest value (torch.topk's order)
__device__ __forceinline__ uint32_t f2key(float f) {
    if (f != f) return 0xffffffffu;
    const uint32_t u = __float_as_uint(f == 0.f ? 0.f : f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

template <int NT>
__device__ __forceinline__ int block_sum_i(int v, int* red, int& phase) {
    constexpr int NW = NT / 64;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    int* r = red + (phase & 1) * NW;                // two alternating rows: one barrier per call
    ++phase;
    if ((threadIdx.x & 63) == 0) r[threadIdx.x >> 6] = v;
    __syncthreads();
    int t = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) t += r[i];
    return t;
}

// is (sa, ja) a better draw than (sb, jb)?  larger score first, NaN above everything (torch.argmax), the lower rank on equal scores
__device__ __forceinline__ bool better(float sa, int ja, float sb, int jb) {
    const bool na = sa != sa, nb = sb != sb;
    if (na != nb) return na;
    if (!na && sa != sb) return sa > sb;
    return ja < jb;
}

template <int NT, int ITEMS>
__global__ __launch_bounds__(NT) void sample_next_row_kernel(SampleArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int NW = NT / 64;
    int* red = reinterpret_cast<int*>(smem);                               // [2][NW]
    int* wtot = red + 2 * NW;                                              // [NW]
    float* bsc = reinterpret_cast<float*>(wtot + NW);                      // [NW]
    int* bj = reinterpret_cast<int*>(bsc + NW);                            // [NW]
    unsigned long long* bw = reinterpret_cast<unsigned long long*>(smem + 320);        // [NW]
    unsigned long long* sorted = reinterpret_cast<unsigned long long*>(smem + SAMPLE_SMALL_BYTES);
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // the same two words for every workgroup of the launch: all of them write, or none does
    const int t = a.step[0];
    if (t < 0 || t >= a.cap) return;
    const int pi = a.pos_idx[t];
    if (pi < 0 || pi >= a.P) return;

    const unsigned long long imask = (1ull << a.ibits) - 1ull;
    unsigned long long w[ITEMS];
    const float* row = a.logits + (size_t)b * a.ld;
#pragma unroll
    for (int i = 0; i < ITEMS; ++i) {
        const int c = i * NT + tid;                                        // consecutive lanes, consecutive classes
        w[i] = c < a.C ? ((unsigned long long)f2key(row[c]) << a.ibits) | (imask - (unsigned long long)c) : 0ull;   // (0 < every real word)
    }
    int phase = 0;
    unsigned long long win;                                                // the order word of the sampled class
    if (a.keep == 1) {
        unsigned long long m = w[0];
#pragma unroll
        for (int i = 1; i < ITEMS; ++i) m = w[i] > m ? w[i] : m;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const unsigned long long o = __shfl_xor(m, off, 64);
            m = o > m ? o : m;
        }
        if (lane == 0) bw[wave] = m;
        __syncthreads();
        win = bw[0];
#pragma unroll
        for (int i = 1; i < NW; ++i) win = bw[i] > win ? bw[i] : win;
    } else {
        // 1. the keep-th largest word: the largest T with count(word >= T) >= keep, bit by bit from the top
        unsigned long long T = 0ull;
        for (int bit = 31 + a.ibits; bit >= 0; --bit) {
            const unsigned long long cand = T | (1ull << bit);
            int n = 0;
#pragma unroll
            for (int i = 0; i < ITEMS; ++i) n += w[i] >= cand ? 1 : 0;
            if (block_sum_i<NT>(n, red, phase) >= a.keep) T = cand;
        }
        // 2. the words are distinct: exactly `keep` of them are >= T.  Slot = exclusive scan over the threads (a fixed order)
        int mine = 0;
#pragma unroll
        for (int i = 0; i < ITEMS; ++i) mine += w[i] >= T ? 1 : 0;
        int incl = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int o = __shfl_up(incl, off, 64);
            if (lane >= off) incl += o;
        }
        if (lane == 63) wtot[wave] = incl;
        __syncthreads();
        int slot = incl - mine;
#pragma unroll
        for (int i = 0; i < NW; ++i) slot += i < wave ? wtot[i] : 0;
#pragma unroll
        for (int i = 0; i < ITEMS; ++i)
            if (w[i] >= T) {
                if (slot < a.keep) sorted[slot] = w[i];                    // (always true; keeps a store inside the array whatever happens)
                ++slot;
            }
        for (int j = a.keep + tid; j < a.kpad; j += NT) sorted[j] = 0ull;  // padding of the network: below every real word
        __syncthreads();
        // descending bitonic network over kpad = 2^m >= keep words
        for (int size = 2; size <= a.kpad; size <<= 1) {
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int p = tid; p < (a.kpad >> 1); p += NT) {
                    const int lo = 2 * p - (p & (stride - 1)), hi = lo + stride;
                    const bool desc = (lo & size) == 0;
                    const unsigned long long x = sorted[lo], y = sorted[hi];
                    if ((x < y) == desc) { sorted[lo] = y; sorted[hi] = x; }
                }
                __syncthreads();
            }
        }
        // 3. Gumbel-max over the kept entries: uniform j belongs to the rank-j logit
        const float* urow = a.u + (size_t)b * a.keep;
        float bs = 0.f;
        int bjj = 0x7fffffff;
        for (int j = tid; j < a.keep; j += NT) {
            const float v = key2f((uint32_t)(sorted[j] >> a.ibits));
            const float g = -logf(fmaxf(-logf(fmaxf(urow[j], 1e-20f)), 1e-20f));
            const float sc = v / a.temperature + g;
            if (bjj == 0x7fffffff || better(sc, j, bs, bjj)) { bs = sc; bjj = j; }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float os = __shfl_xor(bs, off, 64);
            const int oj = __shfl_xor(bjj, off, 64);
            if (oj != 0x7fffffff && (bjj == 0x7fffffff || better(os, oj, bs, bjj))) { bs = os; bjj = oj; }
        }
        if (lane == 0) { bsc[wave] = bs; bj[wave] = bjj; }
        __syncthreads();
        bs = bsc[0];
        bjj = bj[0];                                                       // wave 0 holds rank 0: never empty
#pragma unroll
        for (int i = 1; i < NW; ++i) {
            const float os = bsc[i];
            const int oj = bj[i];
            if (oj != 0x7fffffff && better(os, oj, bs, bjj)) { bs = os; bjj = oj; }
        }
        win = sorted[bjj];
    }
    // 4. the token id and the next input row
    const int cls = (int)(imask - (win & imask));
    if (tid == 0) a.ids[(size_t)b * a.cap + t] = (long long)cls;
    const float* e = a.emb + (size_t)cls * a.D;
    const float* p = a.pos + (size_t)pi * a.D;
    float* x = a.x_next + (size_t)b * a.D;
    for (int c = tid * 4; c < a.D; c += NT * 4) {
        const float4 ev = *reinterpret_cast<const float4*>(e + c), pv = *reinterpret_cast<const float4*>(p + c);
        *reinterpret_cast<float4*>(x + c) = make_float4(ev.x + pv.x, ev.y + pv.y, ev.z + pv.z, ev.w + pv.w);
    }
}

template <int NT, int ITEMS>
void sample_launch(const SampleArgs& a, int B, size_t lds, hipStream_t stream) {
    (void)hipFuncSetAttribute((const void*)sample_next_row_kernel<NT, ITEMS>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((sample_next_row_kernel<NT, ITEMS>), dim3(B), dim3(NT), lds, stream, a);
}

}  // namespace

extern "C" int amdnuwa_sample_next_row(int B, int C, int keep, float temperature, const float* logits, int ld, const float* u,
                                       const float* emb, int D, const float* pos, int P, const int* pos_idx, int cap, const int* step,
                                       long long* ids, float* x_next, hipStream_t stream) {
    if (!logits || !emb || !pos || !pos_idx || !step || !ids || !x_next) return AMDNUWA_ERR_ARG;
    if (B <= 0 || C <= 0 || keep < 1 || keep > C || ld < C || D <= 0 || P <= 0 || cap <= 0) return AMDNUWA_ERR_ARG;
    if ((u == nullptr) != (keep == 1)) return AMDNUWA_ERR_ARG;
    if (!(temperature > 0.f) || !__builtin_isfinite(temperature)) return AMDNUWA_ERR_ARG;
    if (C > SAMPLE_MAX_C || D % 4) return AMDNUWA_ERR_UNSUPPORTED;
    if (((uintptr_t)emb | (uintptr_t)pos | (uintptr_t)x_next) & 15u) return AMDNUWA_ERR_UNSUPPORTED;       // 16-byte vectors
    SampleArgs a{};
    a.logits = logits; a.u = u; a.emb = emb; a.pos = pos; a.pos_idx = pos_idx; a.step = step; a.ids = ids; a.x_next = x_next;
    a.C = C; a.ld = ld; a.keep = keep; a.D = D; a.P = P; a.cap = cap; a.temperature = temperature;
    a.ibits = 1;
    while ((1 << a.ibits) < C) ++a.ibits;                                  // class index bits: <= 14
    a.kpad = 2;
    while (a.kpad < keep) a.kpad <<= 1;                                    // <= 16384 words = 128 KiB
    const size_t lds = SAMPLE_SMALL_BYTES + (keep == 1 ? 0 : (size_t)a.kpad * sizeof(unsigned long long));
    if (lds > 160 * 1024) return AMDNUWA_ERR_UNSUPPORTED;
    if (C <= 1024) sample_launch<256, 4>(a, B, lds, stream);
    else if (C <= 4096) sample_launch<1024, 4>(a, B, lds, stream);
    else sample_launch<1024, 16>(a, B, lds, stream);
    LAUNCH_CHECK();
    return AMDNUWA_OK;
}
