// Plain attention core with linear memory ("cattn"): np.py:339-378, causal self-attention (np.py:364-367) or non-causal attention of n
// query rows over nk key rows of the same or of another tensor (a context), any lengths, heads 1..8, dim_head 32 / 64.
// Keys = [learned null key | the nk key rows]; fp32 softmax per head, THEN the
// heads x heads talking-heads mix, then the product with V -- so the forward is two passes over the keys (statistics, then apply), and the
// backward recomputes the probabilities from q, k and the statistics.  Nothing of size n x nk is ever written to memory.
//
// One schedule serves every sweep.  A workgroup of four waves owns 64 STATIONARY rows (16 per wave, all heads, operands in registers) and
// streams the other side through LDS 32 rows at a time:
//
//     sweep        stationary (registers)      streamed (LDS)                      result
//     forward      queries: q                  keys: K rows, V^T                   statistics, o
//     delta        queries: q, dO              keys: K rows, V rows                delta, dW_th partials, the null key's dS / A
//     dq           queries: q, dO              keys: K rows, V rows, K^T           dq
//     dv           keys: k                     queries: Q rows, dO^T               dv
//     dk           keys: k, v                  queries: Q rows, dO rows, Q^T       dk
//
// The score tile is computed TRANSPOSED with respect to the stationary side, S^T[y][x] = sum_d Y[y][d] X[x][d] (A operand = 16 streamed rows
// read straight from their row-major LDS copy, B operand = the wave's own rows): two MFMAs leave a lane with 8 streamed rows of ONE
// stationary row -- rows {4 g + e} and {16 + 4 g + e} of the tile, g = lane / 16 -- which IS the B-operand layout of the next product once
// the streamed side's transposed LDS copy stores its 32 rows in that slot order (slot_of).  So probabilities never leave the registers
// between the two MFMAs, and the head mix runs on the lane's own values (VALU: heads x heads FMAs per probability).
// The null key is not a key row: its score is one dot product per (query, head), its value a rank-one term (as in xattn6.hip).
// Rectangular (nk != n): the query-stationary sweeps run ceil(n / 64) workgroups per sample over ceil(nk / 32) key tiles, the key-stationary
// ones ceil(nk / 64) workgroups over ceil(n / 32) query tiles; row bases and ragged-tile predicates are per side (Item).
// Causal: key tiles above the diagonal are never staged; a wave skips tiles that lie wholly above its own 16 rows; the predicate is per element.
// No atomics: dW_th / dnull_k / dnull_v leave as per-workgroup partials reduced in a fixed order (amdnuwa_colsum).
// Attention dropout (template parameter DROP, amdnuwa_cattn_fwd_drop / _bwd_drop): the keep mask multiplies the MIXED probabilities in the one
// place each sweep holds them in registers -- see CDropArgs.  The unmasked instantiations keep their kernel argument and their code.
#include "common.h"
#include "../../include/amdnuwa.h"

// every sweep must round the scores identically (the probabilities are exp2(score - saved maximum)): no implicit contraction
#pragma clang fp contract(off)

namespace {

constexpr int NHM = 8;             // most heads a wave holds
constexpr int YT = 32;             // streamed rows per step
constexpr int XW = 64;             // stationary rows per workgroup
constexpr int TP = 80;             // byte pitch of one column of a transposed tile: 32 slots x 2 bytes + 16 (conflict-free ds_read_b128)
constexpr float NEG = -1.0e30f;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
// A wave holds every head's operands and accumulators (one wave per SIMD): the scheduler may overlap the instructions of ONE head, not hoist the
// LDS reads of all eight (that form spilled)
#define HEAD_FENCE() __builtin_amdgcn_sched_barrier(0)

struct CArgs {
    const uint16_t *q, *k, *v, *dO;          // q / dO [B*n, ld], k / v [B*nk, ldkv] 16-bit rows
    int ldq, ldkv, lddo;
    const uint8_t* mask;                     // [B][nk] key mask or NULL
    const float *null_k, *null_v, *wth;      // [heads][DH], [heads][DH], [heads][heads]
    uint16_t *o, *ol; int ldo, ol_f16;
    float* stats;                            // [B][heads][n][2] = (maximum in the log2 domain, 1 / sum of exp2)
    float* delta;                            // [B][heads][n]
    float *ds0, *a0;                         // [B*n][8]: scale * dS of the null key per head, mixed null probability per head
    uint16_t *dq, *dk, *dv; int lddq, lddkv; // dq [B*n, lddq], dk / dv [B*nk, lddkv]
    float* part_th;                          // [workgroups][64]: dW_th partials, index 8 g + h
    int B, n, nk, heads, causal;             // n query rows and nk key rows per sample (nk == n: self-attention; causal needs it)
    float c1, scale;                         // scale * log2(e), scale
};

// Attention dropout (the DROP forms; np.py:370-374, after the talking-heads mix): A''[g] = keep . s . A'[g] feeds the V product and dv,
// dA'[g] = keep . s . dA''[g] everything of the backward.  One byte per (query, key) pair, bit g = output head g kept; the query-stationary
// sweeps read keep [B][n][KP], the key-stationary ones the same bytes transposed, keep_t [B][nk][NP] (KP / NP = the key / query count
// rounded up to 32), so a lane's eight streamed rows (yrow) are two aligned 32-bit loads per tile on either side; keep0 [B][n] is the null
// slot.  Only the DROP instantiations take the extra words: the kernel argument of the unmasked ones stays CArgs itself.
struct CDropArgs : CArgs { const uint8_t *keep, *keep_t, *keep0; int KP, NP; float drop_s; };
template <bool DROP> struct CKArgsSel { using type = CArgs; };
template <> struct CKArgsSel<true> { using type = CDropArgs; };
template <bool DROP> using CKArgs = typename CKArgsSel<DROP>::type;
// the mask of a dropout call (keep == NULL: an unmasked call)
struct CMask { const uint8_t *keep, *keep_t, *keep0; float s; };
template <bool DROP> inline CKArgs<DROP> c_kargs(const CArgs& a, const CMask& mk) {
    if constexpr (DROP) {
        CDropArgs d{};
        static_cast<CArgs&>(d) = a;
        d.keep = mk.keep; d.keep_t = mk.keep_t; d.keep0 = mk.keep0; d.drop_s = mk.s;
        d.KP = (a.nk + YT - 1) / YT * YT; d.NP = (a.n + YT - 1) / YT * YT;
        return d;
    } else {
        return a;
    }
}

__device__ __forceinline__ bf16x8 lds16(const char* p) { return *reinterpret_cast<const bf16x8*>(p); }
__device__ __forceinline__ bf16x8 ldfrag(const uint16_t* p, bool ok) {
    u32x4 z = {0u, 0u, 0u, 0u};
    if (ok) z = *reinterpret_cast<const u32x4*>(p);
    return __builtin_bit_cast(bf16x8, z);
}
template <bool F16> __device__ __forceinline__ float el(const bf16x8& v, int e) {
    const u32x4 u = __builtin_bit_cast(u32x4, v);
    return (e & 1) ? hi_t<F16>(u[e >> 1]) : lo_t<F16>(u[e >> 1]);
}
template <bool F16> __device__ __forceinline__ bf16x8 pack8(const float (&v)[8]) {
    const u32x4 u = {pack2_t<F16>(v[0], v[1]), pack2_t<F16>(v[2], v[3]), pack2_t<F16>(v[4], v[5]), pack2_t<F16>(v[6], v[7])};
    return __builtin_bit_cast(bf16x8, u);
}
// slot of tile row y in the transposed copies = position of that row among a lane's 8 values (see the head of the file)
__device__ __forceinline__ int slot_of(int y) { return 8 * ((y & 15) >> 2) + 4 * (y >> 4) + (y & 3); }
// tile row of a lane's value e
__device__ __forceinline__ int yrow(int g4, int e) { return (e < 4 ? 4 * g4 + e : 12 + 4 * g4 + e); }
// DROP forms: the keep bytes of a lane's stationary row `row` (an in-range row of keep / keep_t, pitch bytes each) at its eight streamed rows
// of the tile at y0 -- yrow: bytes y0 + 4 g4 .. + 3 and y0 + 16 + 4 g4 .. + 3, inside the pitch because it is a multiple of the tile
__device__ __forceinline__ uint2 keep_words(const uint8_t* __restrict__ base, long row, int pitch, bool rin, int y0, int g4) {
    uint2 kw = make_uint2(0u, 0u);
    if (rin) {
        const uint8_t* p = base + row * pitch + y0 + 4 * g4;
        kw.x = *reinterpret_cast<const uint32_t*>(p); kw.y = *reinterpret_cast<const uint32_t*>(p + 16);
    }
    return kw;
}
// value e of head g under dropout: v . s where the mask keeps it, exactly 0 where it drops it
__device__ __forceinline__ float keep_apply(const uint2& kw, int g, int e, float s, float v) {
    return (((e < 4 ? kw.x : kw.y) >> (8 * (e & 3) + g)) & 1u) ? v * s : 0.f;
}

// 32 rows [row0, row0 + 32) x inner columns of the sample's 16-bit rows -> LDS: row-major copy (pitch bytes per row) and / or the
// transposed copy [column][slot].  Rows beyond the sequence are zeros.  Four loads in flight per thread, then their LDS stores.
template <bool RM, bool TR>
__device__ __forceinline__ void stage_tile(const uint16_t* __restrict__ src, int ld, int row0, int nrows, int inner, char* rm, int pitch, char* tr, int tid) {
    const int ppr = inner >> 3, np = YT * ppr;
#pragma unroll
    for (int i0 = 0; i0 < 8; i0 += 4) {
        u32x4 val[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int p = tid + 256 * (i0 + i), r = p / ppr, c8 = p - r * ppr;
            val[i] = u32x4{0u, 0u, 0u, 0u};
            if (p < np && row0 + r < nrows) val[i] = *reinterpret_cast<const u32x4*>(src + (long)(row0 + r) * ld + c8 * 8);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int p = tid + 256 * (i0 + i), r = p / ppr, c8 = p - r * ppr;
            if (p < np) {
                if (RM) *reinterpret_cast<u32x4*>(rm + r * pitch + c8 * 16) = val[i];
                if (TR) {
                    char* t = tr + (c8 * 8) * TP + 2 * slot_of(r);
#pragma unroll
                    for (int e = 0; e < 8; ++e) *reinterpret_cast<uint16_t*>(t + e * TP) = (uint16_t)(val[i][e >> 1] >> (16 * (e & 1)));
                }
            }
        }
        HEAD_FENCE();
    }
}

// S^T of one head: the lane's 8 streamed rows (yrow) against its stationary row
template <int DH, bool F16>
__device__ __forceinline__ void score8(const char* rm, int pitch, int h, int r16, int g4, const bf16x8 (&xf)[DH / 32], float (&s)[8]) {
    f32x4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < DH / 32; ++ks) {
        const char* p = rm + r16 * pitch + (h * DH + 32 * ks + 8 * g4) * 2;
        c0 = mfma16<F16>(lds16(p), xf[ks], c0);
        c1 = mfma16<F16>(lds16(p + 16 * pitch), xf[ks], c1);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) { s[r] = c0[r]; s[4 + r] = c1[r]; }
}

// the work item of a workgroup: sample b, stationary rows [x0, x0 + 64), streamed tiles [y_begin, y_end)
// nx stationary and ny streamed rows per sample (query side: n and nk; key side: nk and n), rowx / rowy the sample's first row on each side
struct Item { int b, x0, y_begin, y_end, nx, ny; long rowx, rowy; };
template <bool KEYSIDE>
__device__ __forceinline__ Item item_of(const CArgs& a) {
    Item it;
    it.nx = KEYSIDE ? a.nk : a.n; it.ny = KEYSIDE ? a.n : a.nk;
    const int ntx = (it.nx + XW - 1) / XW, NT = (it.ny + YT - 1) / YT;
    it.b = blockIdx.x % a.B;
    int t = blockIdx.x / a.B;
    if (!KEYSIDE) t = ntx - 1 - t;            // causal: the long items first (the key side's natural order already is)
    it.x0 = t * XW;
    it.rowx = (long)it.b * it.nx; it.rowy = (long)it.b * it.ny;
    it.y_begin = 0; it.y_end = NT;
    if (a.causal) {
        if (KEYSIDE) it.y_begin = it.x0 / YT;
        else { const int last = (it.x0 + XW < it.nx ? it.x0 + XW : it.nx) - 1; it.y_end = last / YT + 1; }
    }
    return it;
}

// key validity word of a streamed KEY tile (bit r: key y0 + r exists and passes the mask), written by wave 0
__device__ __forceinline__ void stage_vbits(const CArgs& a, long rowb, int y0, uint32_t* svb, int tid) {
    if (tid < 64) {
        const int key = y0 + tid;
        const bool ok = tid < YT && key < a.nk && (!a.mask || a.mask[rowb + key] != 0);
        const unsigned long long bal = __ballot(ok);
        if (tid == 0) *svb = (uint32_t)bal;
    }
}

// element predicate of a lane for one streamed tile, bit e.  query side: x = the lane's query, streamed rows = keys; key side: x = the lane's key
template <bool KEYSIDE>
__device__ __forceinline__ unsigned valid_bits(const CArgs& a, int x, bool xok, int y0, int g4, uint32_t vb) {
    unsigned vm = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int yr = yrow(g4, e), y = y0 + yr;
        bool ok = xok;
        if (KEYSIDE) ok = ok && y < a.n && (!a.causal || x <= y);
        else ok = ok && ((vb >> yr) & 1u) && (!a.causal || y <= x);
        vm |= ok ? (1u << e) : 0u;
    }
    return vm;
}

// c1 * (x . null_k[h]) of the lane's stationary query row (all four lane groups end with the full dot product)
template <int DH, bool F16>
__device__ __forceinline__ float null_dot(const bf16x8 (&xf)[DH / 32], const float* __restrict__ nvec, int h, int g4) {
    float d = 0.f;
#pragma unroll
    for (int ks = 0; ks < DH / 32; ++ks)
#pragma unroll
        for (int e = 0; e < 8; ++e) d = fmaf(el<F16>(xf[ks], e), nvec[h * DH + 32 * ks + 8 * g4 + e], d);
    d += __shfl_xor(d, 16, 64);
    d += __shfl_xor(d, 32, 64);
    return d;
}

// ---- forward (KEYSIDE = false: statistics pass, then o = A V) and the dv sweep (KEYSIDE = true: dv = A^T dO) ----------------------
template <int DH, bool F16, bool KEYSIDE, bool DROP = false>
__global__ __launch_bounds__(256, 1) void cattn_apply_kernel(CKArgs<DROP> a) {
    constexpr int KS = DH / 32, DB = DH / 16;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, g4 = lane >> 4;
    const int heads = a.heads, inner = heads * DH, pitch = inner * 2 + 16;
    char* rm = smem;
    char* tr = smem + YT * pitch;
    float* sst = reinterpret_cast<float*>(tr + inner * TP);           // key side: [2][8][32] statistics of the streamed queries
    uint32_t* svb = reinterpret_cast<uint32_t*>(sst + 2 * NHM * YT);
    const Item it = item_of<KEYSIDE>(a);
    const long rowb = it.rowx, rowy = it.rowy;
    const int xw = it.x0 + 16 * wave, x = xw + r16;
    const bool xin = x < it.nx;
    const bool xok = KEYSIDE ? (xin && (!a.mask || a.mask[rowb + (xin ? x : 0)] != 0)) : xin;
    const uint16_t* xsrc = KEYSIDE ? a.k : a.q;
    const int xld = KEYSIDE ? a.ldkv : a.ldq;
    const uint16_t* ysrc_rm = (KEYSIDE ? a.q : a.k) + rowy * (KEYSIDE ? a.ldq : a.ldkv);
    const int yld_rm = KEYSIDE ? a.ldq : a.ldkv;
    const uint16_t* ysrc_tr = (KEYSIDE ? a.dO : a.v) + rowy * (KEYSIDE ? a.lddo : a.ldkv);
    const int yld_tr = KEYSIDE ? a.lddo : a.ldkv;

    bf16x8 xf[NHM][KS];
#pragma unroll
    for (int h = 0; h < NHM; ++h)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) xf[h][ks] = ldfrag(xsrc + (rowb + x) * xld + h * DH + 32 * ks + 8 * g4, xin && h < heads);
    float w[NHM][NHM];
#pragma unroll
    for (int g = 0; g < NHM; ++g)
#pragma unroll
        for (int h = 0; h < NHM; ++h) w[g][h] = (g < heads && h < heads) ? a.wth[g * heads + h] : 0.f;

    float m[NHM], il[NHM], s0[NHM];
    if (!KEYSIDE) {
        // ---- pass 1: per (query, head) maximum and sum over the visible keys and the null key
        float l[NHM];
#pragma unroll
        for (int h = 0; h < NHM; ++h) {
            m[h] = NEG; l[h] = 0.f; s0[h] = 0.f;
            if (h < heads) s0[h] = a.c1 * null_dot<DH, F16>(xf[h], a.null_k, h, g4);
        }
        for (int yt = it.y_begin; yt < it.y_end; ++yt) {
            const int y0 = yt * YT;
            __syncthreads();
            stage_tile<true, false>(ysrc_rm, yld_rm, y0, it.ny, inner, rm, pitch, nullptr, tid);
            stage_vbits(a, rowy, y0, svb, tid);
            __syncthreads();
            if (a.causal && y0 > xw + 15) continue;
            const unsigned vm = valid_bits<false>(a, x, xok, y0, g4, *svb);
#pragma unroll
            for (int h = 0; h < NHM; ++h) {
                if (h < heads) {
                    float s[8];
                    score8<DH, F16>(rm, pitch, h, r16, g4, xf[h], s);
                    float tm = NEG;
#pragma unroll
                    for (int e = 0; e < 8; ++e) { s[e] = ((vm >> e) & 1u) ? a.c1 * s[e] : NEG; tm = fmaxf(tm, s[e]); }
                    const float mn = fmaxf(m[h], tm);
                    float sum = 0.f;
#pragma unroll
                    for (int e = 0; e < 8; ++e) sum += ((vm >> e) & 1u) ? __builtin_amdgcn_exp2f(s[e] - mn) : 0.f;
                    l[h] = l[h] * __builtin_amdgcn_exp2f(m[h] - mn) + sum;
                    m[h] = mn;
                    HEAD_FENCE();
                }
            }
        }
#pragma unroll
        for (int h = 0; h < NHM; ++h) {
            if (h < heads) {
                float mm = fmaxf(m[h], __shfl_xor(m[h], 16, 64));
                mm = fmaxf(mm, __shfl_xor(mm, 32, 64));
                float lh = l[h] * __builtin_amdgcn_exp2f(m[h] - mm);
                lh += __shfl_xor(lh, 16, 64);
                lh += __shfl_xor(lh, 32, 64);
                const float mf = fmaxf(mm, s0[h]);
                lh = lh * __builtin_amdgcn_exp2f(mm - mf) + __builtin_amdgcn_exp2f(s0[h] - mf);
                m[h] = mf;
                il[h] = 1.f / lh;
                if (g4 == 0 && xin) {
                    float* st = a.stats + (((long)it.b * heads + h) * a.n + x) * 2;
                    st[0] = mf; st[1] = il[h];
                }
            }
        }
    }

    // ---- pass 2 (forward) / the dv sweep: probabilities -> head mix -> the second product, per streamed tile
    f32x4 acc[NHM][DB];
#pragma unroll
    for (int g = 0; g < NHM; ++g)
#pragma unroll
        for (int db = 0; db < DB; ++db) acc[g][db] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int yt = it.y_begin; yt < it.y_end; ++yt) {
        const int y0 = yt * YT;
        __syncthreads();
        stage_tile<true, false>(ysrc_rm, yld_rm, y0, it.ny, inner, rm, pitch, nullptr, tid);
        stage_tile<false, true>(ysrc_tr, yld_tr, y0, it.ny, inner, nullptr, 0, tr, tid);
        if (KEYSIDE) {
            const int h = tid >> 5, r = tid & 31, qy = y0 + r;
            float mv = 0.f, iv = 0.f;
            if (h < heads && qy < a.n) { const float* st = a.stats + (((long)it.b * heads + h) * a.n + qy) * 2; mv = st[0]; iv = st[1]; }
            sst[h * YT + r] = mv; sst[NHM * YT + h * YT + r] = iv;
        } else {
            stage_vbits(a, rowy, y0, svb, tid);
        }
        __syncthreads();
        if (a.causal && (KEYSIDE ? (y0 + YT - 1 < xw) : (y0 > xw + 15))) continue;
        const unsigned vm = valid_bits<KEYSIDE>(a, x, xok, y0, g4, KEYSIDE ? 0u : *svb);
        uint2 kw = make_uint2(0u, 0u);                   // DROP: in flight under the probabilities, read by the mix
        if constexpr (DROP) kw = keep_words(KEYSIDE ? a.keep_t : a.keep, rowb + x, KEYSIDE ? a.NP : a.KP, xin, y0, g4);
        float p[NHM][8];
#pragma unroll
        for (int h = 0; h < NHM; ++h) {
#pragma unroll
            for (int e = 0; e < 8; ++e) p[h][e] = 0.f;
            if (h < heads) {
                float s[8];
                score8<DH, F16>(rm, pitch, h, r16, g4, xf[h], s);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float me = KEYSIDE ? sst[h * YT + yrow(g4, e)] : m[h];
                    const float ie = KEYSIDE ? sst[NHM * YT + h * YT + yrow(g4, e)] : il[h];
                    p[h][e] = ((vm >> e) & 1u) ? __builtin_amdgcn_exp2f(a.c1 * s[e] - me) * ie : 0.f;
                }
                HEAD_FENCE();
            }
        }
#pragma unroll
        for (int g = 0; g < NHM; ++g) {
            if (g < heads) {
                float am[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    float v = 0.f;
#pragma unroll
                    for (int h = 0; h < NHM; ++h) v = fmaf(w[g][h], p[h][e], v);
                    am[e] = v;
                    if constexpr (DROP) am[e] = keep_apply(kw, g, e, a.drop_s, v);
                }
                const bf16x8 bm = pack8<F16>(am);
#pragma unroll
                for (int db = 0; db < DB; ++db)
                    acc[g][db] = mfma16<F16>(lds16(tr + (g * DH + 16 * db + r16) * TP + 16 * g4), bm, acc[g][db]);
                HEAD_FENCE();
            }
        }
    }

    // ---- epilogue: acc[g][db][r] = result[x][g * DH + 16 db + 4 g4 + r]
    if (!KEYSIDE) {
        float p0[NHM], amax = 0.f;
#pragma unroll
        for (int h = 0; h < NHM; ++h) p0[h] = h < heads ? __builtin_amdgcn_exp2f(s0[h] - m[h]) * il[h] : 0.f;
        unsigned k0 = 0;                                 // DROP: the null slot's keep byte of the lane's query
        if constexpr (DROP) k0 = xin ? a.keep0[rowb + x] : 0u;
#pragma unroll
        for (int g = 0; g < NHM; ++g) {
            if (g < heads) {
                float a0 = 0.f;
#pragma unroll
                for (int h = 0; h < NHM; ++h) a0 = fmaf(w[g][h], p0[h], a0);
                if constexpr (DROP) a0 = ((k0 >> g) & 1u) ? a0 * a.drop_s : 0.f;
#pragma unroll
                for (int db = 0; db < DB; ++db) {
                    const int d = 16 * db + 4 * g4;
                    float v[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = fmaf(a0, a.null_v[g * DH + d + r], acc[g][db][r]);
                    if (xin) {
                        const long off = (rowb + x) * (long)a.ldo + g * DH + d;
                        const uint32_t h0 = pack2_rne(v[0], v[1]), h1 = pack2_rne(v[2], v[3]);
                        if (a.o) *reinterpret_cast<uint2*>(a.o + off) = make_uint2(h0, h1);
                        if (a.ol) {
                            uint2 lo;
                            if (a.ol_f16) { lo.x = pack2_f16_sat_n(v[0], v[1], amax); lo.y = pack2_f16_sat_n(v[2], v[3], amax); }
                            else { lo.x = pack2_rne(v[0] - lo_f(h0), v[1] - hi_f(h0)); lo.y = pack2_rne(v[2] - lo_f(h1), v[3] - hi_f(h1)); }
                            *reinterpret_cast<uint2*>(a.ol + off) = lo;
                        }
                    }
                }
            }
        }
        f16_sat_commit(amax);
    } else {
#pragma unroll
        for (int g = 0; g < NHM; ++g) {
            if (g < heads && xin) {
#pragma unroll
                for (int db = 0; db < DB; ++db) {
                    const long off = (rowb + x) * (long)a.lddkv + g * DH + 16 * db + 4 * g4;
                    *reinterpret_cast<uint2*>(a.dv + off) = make_uint2(pack2_rne(acc[g][db][0], acc[g][db][1]), pack2_rne(acc[g][db][2], acc[g][db][3]));
                }
            }
        }
    }
}

// ---- backward sweeps on bf16 operands.  MODE 0 (query side): delta, dW_th partials, the null key's terms.  MODE 1: dq (query side) / dk (key side)
template <int DH, bool KEYSIDE, int MODE, bool DROP = false>
__global__ __launch_bounds__(256, 1) void cattn_grad_kernel(CKArgs<DROP> a) {
    constexpr int KS = DH / 32, DB = DH / 16;
    static_assert(MODE == 1 || !KEYSIDE, "the delta sweep is query-stationary");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r16 = lane & 15, g4 = lane >> 4;
    const int heads = a.heads, inner = heads * DH, pitch = inner * 2 + 16;
    char* rm1 = smem;                                    // K rows (query side) / Q rows (key side)
    char* rm2 = rm1 + YT * pitch;                        // V rows / dO rows
    char* tr = rm2 + YT * pitch;                         // K^T / Q^T (MODE 1)
    float* sst = reinterpret_cast<float*>(tr + (MODE == 1 ? inner * TP : 0));      // key side: [3][8][32] m, 1 / l, delta of the streamed queries
    uint32_t* svb = reinterpret_cast<uint32_t*>(sst + 3 * NHM * YT);
    float* sred = reinterpret_cast<float*>(svb + 4);     // [4][64] dW_th of the four waves
    const Item it = item_of<KEYSIDE>(a);
    const long rowb = it.rowx, rowy = it.rowy;
    const int xw = it.x0 + 16 * wave, x = xw + r16;
    const bool xin = x < it.nx;
    const bool xok = KEYSIDE ? (xin && (!a.mask || a.mask[rowb + (xin ? x : 0)] != 0)) : xin;
    const uint16_t* ysrc1 = (KEYSIDE ? a.q : a.k) + rowy * (KEYSIDE ? a.ldq : a.ldkv);
    const int yld1 = KEYSIDE ? a.ldq : a.ldkv;
    const uint16_t* ysrc2 = (KEYSIDE ? a.dO : a.v) + rowy * (KEYSIDE ? a.lddo : a.ldkv);
    const int yld2 = KEYSIDE ? a.lddo : a.ldkv;

    bf16x8 xf1[NHM][KS], xf2[NHM][KS];
#pragma unroll
    for (int h = 0; h < NHM; ++h)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            const int c = h * DH + 32 * ks + 8 * g4;
            const bool ok = xin && h < heads;
            xf1[h][ks] = ldfrag((KEYSIDE ? a.k + (rowb + x) * a.ldkv : a.q + (rowb + x) * a.ldq) + c, ok);
            xf2[h][ks] = ldfrag((KEYSIDE ? a.v + (rowb + x) * a.ldkv : a.dO + (rowb + x) * a.lddo) + c, ok);
        }
    float w[NHM][NHM];
#pragma unroll
    for (int g = 0; g < NHM; ++g)
#pragma unroll
        for (int h = 0; h < NHM; ++h) w[g][h] = (g < heads && h < heads) ? a.wth[g * heads + h] : 0.f;

    float m[NHM], il[NHM], dl[NHM];
#pragma unroll
    for (int h = 0; h < NHM; ++h) {
        m[h] = 0.f; il[h] = 0.f; dl[h] = 0.f;
        if (!KEYSIDE && h < heads && xin) {
            const float* st = a.stats + (((long)it.b * heads + h) * a.n + x) * 2;
            m[h] = st[0]; il[h] = st[1];
            if (MODE == 1) dl[h] = a.delta[((long)it.b * heads + h) * a.n + x];
        }
    }
    float dw[MODE == 0 ? NHM * NHM : 1];
#pragma unroll
    for (int i = 0; i < (MODE == 0 ? NHM * NHM : 1); ++i) dw[i] = 0.f;
    f32x4 acc[MODE == 1 ? NHM : 1][DB];
#pragma unroll
    for (int h = 0; h < (MODE == 1 ? NHM : 1); ++h)
#pragma unroll
        for (int db = 0; db < DB; ++db) acc[h][db] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int yt = it.y_begin; yt < it.y_end; ++yt) {
        const int y0 = yt * YT;
        __syncthreads();
        stage_tile<true, MODE == 1>(ysrc1, yld1, y0, it.ny, inner, rm1, pitch, tr, tid);
        stage_tile<true, false>(ysrc2, yld2, y0, it.ny, inner, rm2, pitch, nullptr, tid);
        if (KEYSIDE) {
            const int h = tid >> 5, r = tid & 31, qy = y0 + r;
            float mv = 0.f, iv = 0.f, dv_ = 0.f;
            if (h < heads && qy < a.n) {
                const long si = ((long)it.b * heads + h) * a.n + qy;
                mv = a.stats[si * 2]; iv = a.stats[si * 2 + 1]; dv_ = a.delta[si];
            }
            sst[h * YT + r] = mv; sst[NHM * YT + h * YT + r] = iv; sst[2 * NHM * YT + h * YT + r] = dv_;
        } else {
            stage_vbits(a, rowy, y0, svb, tid);
        }
        __syncthreads();
        if (a.causal && (KEYSIDE ? (y0 + YT - 1 < xw) : (y0 > xw + 15))) continue;
        const unsigned vm = valid_bits<KEYSIDE>(a, x, xok, y0, g4, KEYSIDE ? 0u : *svb);
        uint2 kw = make_uint2(0u, 0u);                   // DROP: read by the dA loop only, dead before the probabilities
        if constexpr (DROP) kw = keep_words(KEYSIDE ? a.keep_t : a.keep, rowb + x, KEYSIDE ? a.NP : a.KP, xin, y0, g4);
        float dA[NHM][8];
#pragma unroll
        for (int g = 0; g < NHM; ++g) {
#pragma unroll
            for (int e = 0; e < 8; ++e) dA[g][e] = 0.f;
            if (g < heads) {
                score8<DH, false>(rm2, pitch, g, r16, g4, xf2[g], dA[g]);
                if constexpr (DROP) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) dA[g][e] = keep_apply(kw, g, e, a.drop_s, dA[g][e]);
                }
                HEAD_FENCE();
            }
        }
#pragma unroll
        for (int h = 0; h < NHM; ++h) {
            if (h < heads) {
                float s[8], p[8], dP[8];
                score8<DH, false>(rm1, pitch, h, r16, g4, xf1[h], s);
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float me = KEYSIDE ? sst[h * YT + yrow(g4, e)] : m[h];
                    const float ie = KEYSIDE ? sst[NHM * YT + h * YT + yrow(g4, e)] : il[h];
                    p[e] = ((vm >> e) & 1u) ? __builtin_amdgcn_exp2f(a.c1 * s[e] - me) * ie : 0.f;
                    float v = 0.f;
#pragma unroll
                    for (int g = 0; g < NHM; ++g) v = fmaf(w[g][h], dA[g][e], v);
                    dP[e] = v;
                }
                if constexpr (MODE == 0) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) dl[h] = fmaf(p[e], dP[e], dl[h]);
#pragma unroll
                    for (int g = 0; g < NHM; ++g)
#pragma unroll
                        for (int e = 0; e < 8; ++e) dw[(MODE == 0 ? g * NHM + h : 0)] = fmaf(p[e], dA[g][e], dw[(MODE == 0 ? g * NHM + h : 0)]);
                } else {
                    float ds[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float de = KEYSIDE ? sst[2 * NHM * YT + h * YT + yrow(g4, e)] : dl[h];
                        ds[e] = a.scale * (p[e] * (dP[e] - de));
                    }
                    const bf16x8 bm = pack8<false>(ds);
#pragma unroll
                    for (int db = 0; db < DB; ++db)
                        acc[MODE == 1 ? h : 0][db] = mfma16<false>(lds16(tr + (h * DH + 16 * db + r16) * TP + 16 * g4), bm, acc[MODE == 1 ? h : 0][db]);
                }
                HEAD_FENCE();
            }
        }
    }

    if constexpr (MODE == 0) {
        // the null key: dA0_g = dO_g . null_v_g, P0_h from the statistics; delta gets its term, then dS0 and the mixed A0 leave for the dq sweep
        // and for the null key / value gradients
        float p0[NHM], dA0[NHM];
        unsigned k0 = 0;                                 // DROP: the null slot's keep byte of the lane's query
        if constexpr (DROP) k0 = xin ? a.keep0[rowb + x] : 0u;
#pragma unroll
        for (int h = 0; h < NHM; ++h) {
            p0[h] = 0.f; dA0[h] = 0.f;
            if (h < heads) {
                const float s0 = a.c1 * null_dot<DH, false>(xf1[h], a.null_k, h, g4);
                p0[h] = xin ? __builtin_amdgcn_exp2f(s0 - m[h]) * il[h] : 0.f;
                dA0[h] = null_dot<DH, false>(xf2[h], a.null_v, h, g4);
                if constexpr (DROP) dA0[h] = ((k0 >> h) & 1u) ? dA0[h] * a.drop_s : 0.f;
                dl[h] += __shfl_xor(dl[h], 16, 64);
                dl[h] += __shfl_xor(dl[h], 32, 64);
            }
        }
#pragma unroll
        for (int h = 0; h < NHM; ++h) {
            if (h < heads) {
                float dP0 = 0.f, a0 = 0.f;
#pragma unroll
                for (int g = 0; g < NHM; ++g) { dP0 = fmaf(w[g][h], dA0[g], dP0); a0 = fmaf(w[h][g], p0[g], a0); }
                if constexpr (DROP) a0 = ((k0 >> h) & 1u) ? a0 * a.drop_s : 0.f;
                dl[h] = fmaf(p0[h], dP0, dl[h]);
                if (g4 == 0) {
#pragma unroll
                    for (int g = 0; g < NHM; ++g) dw[(MODE == 0 ? g * NHM + h : 0)] = fmaf(p0[h], dA0[g], dw[(MODE == 0 ? g * NHM + h : 0)]);
                    if (xin) {
                        a.delta[((long)it.b * heads + h) * a.n + x] = dl[h];
                        a.ds0[(rowb + x) * NHM + h] = a.scale * (p0[h] * (dP0 - dl[h]));
                        a.a0[(rowb + x) * NHM + h] = a0;
                    }
                }
            }
        }
        // dW_th: lanes -> wave -> workgroup through LDS, every sum in a fixed order
        float* red = sred + 4 * 64;                      // [256 threads][65]
#pragma unroll
        for (int i = 0; i < NHM * NHM; ++i) red[tid * 65 + i] = dw[MODE == 0 ? i : 0];
        __syncthreads();
        float sum = 0.f;
        for (int l = 0; l < 64; ++l) sum += red[(wave * 64 + l) * 65 + lane];
        sred[wave * 64 + lane] = sum;
        __syncthreads();
        if (wave == 0) a.part_th[(long)blockIdx.x * 64 + lane] = ((sred[lane] + sred[64 + lane]) + sred[128 + lane]) + sred[192 + lane];
    } else {
#pragma unroll
        for (int h = 0; h < NHM; ++h) {
            if (h < heads && xin) {
                const float d0 = KEYSIDE ? 0.f : a.ds0[(rowb + x) * NHM + h];
#pragma unroll
                for (int db = 0; db < DB; ++db) {
                    const int d = 16 * db + 4 * g4;
                    float v[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) v[r] = KEYSIDE ? acc[MODE == 1 ? h : 0][db][r] : fmaf(d0, a.null_k[h * DH + d + r], acc[MODE == 1 ? h : 0][db][r]);
                    uint16_t* dst = KEYSIDE ? a.dk + (rowb + x) * (long)a.lddkv : a.dq + (rowb + x) * (long)a.lddq;
                    *reinterpret_cast<uint2*>(dst + h * DH + d) = make_uint2(pack2_rne(v[0], v[1]), pack2_rne(v[2], v[3]));
                }
            }
        }
    }
}

// dnull_k[h][d] = sum_rows ds0[row][h] q[row][h DH + d], dnull_v[g][d] = sum_rows a0[row][g] dO[row][g DH + d]: per-chunk partials
// part[chunk][2 inner] (256 rows each, summed in row order), reduced in a fixed order afterwards
__global__ __launch_bounds__(256) void cattn_null_grads_kernel(const uint16_t* __restrict__ q, int ldq, const uint16_t* __restrict__ dO, int lddo,
                                                                const float* __restrict__ ds0, const float* __restrict__ a0, float* __restrict__ part,
                                                                long rows, int inner, int dh) {
    const long r0 = (long)blockIdx.x * 256, r1 = r0 + 256 < rows ? r0 + 256 : rows;
    for (int c = threadIdx.x; c < 2 * inner; c += 256) {
        const bool second = c >= inner;
        const int col = second ? c - inner : c, h = col / dh;
        const uint16_t* src = second ? dO : q;
        const int ld = second ? lddo : ldq;
        const float* coef = second ? a0 : ds0;
        float s = 0.f;
        for (long r = r0; r < r1; ++r) s = fmaf(coef[r * NHM + h], bf2f(src[r * ld + col]), s);
        part[(long)blockIdx.x * 2 * inner + c] = s;
    }
}

int keys_of(const amdnuwa_cattn_geom* g) { return g->n_keys ? g->n_keys : g->n; }      // 0 = self-attention
int check_c(const amdnuwa_cattn_geom* g) {
    if (!g) return AMDNUWA_ERR_ARG;
    if (g->heads < 1 || g->heads > NHM || (g->dim_head != 32 && g->dim_head != 64)) return AMDNUWA_ERR_UNSUPPORTED;
    if (g->B < 1 || g->n < 1 || g->n_keys < 0) return AMDNUWA_ERR_ARG;
    if (g->causal && keys_of(g) != g->n) return AMDNUWA_ERR_UNSUPPORTED;                   // the causal predicate is defined for queries == keys only
    if ((long long)g->B * g->n > 0x7fffffffLL / 1024 || (long long)g->B * keys_of(g) > 0x7fffffffLL / 1024)
        return AMDNUWA_ERR_UNSUPPORTED;                                                      // (row * ld stays far inside 63 bits; the grid inside 31)
    return AMDNUWA_OK;
}
size_t lds_apply(const amdnuwa_cattn_geom* g) {
    const size_t inner = (size_t)g->heads * g->dim_head;
    return YT * (inner * 2 + 16) + inner * TP + 2 * NHM * YT * 4 + 16;
}
size_t lds_grad(const amdnuwa_cattn_geom* g, int mode) {
    const size_t inner = (size_t)g->heads * g->dim_head;
    return 2 * YT * (inner * 2 + 16) + (mode ? inner * TP : 256 * 65 * 4) + 3 * NHM * YT * 4 + 16 + 4 * 64 * 4;
}
// workgroups of the query-stationary sweeps (the only ones that leave per-workgroup partials) and of the key-stationary sweeps
long long wgs(const amdnuwa_cattn_geom* g) { return (long long)g->B * ((g->n + XW - 1) / XW); }
long long wgs_k(const amdnuwa_cattn_geom* g) { return (long long)g->B * ((keys_of(g) + XW - 1) / XW); }
long long null_chunks(const amdnuwa_cattn_geom* g) { return ((long long)g->B * g->n + 255) / 256; }
size_t al(size_t v) { return (v + 255) / 256 * 256; }


// the mask arguments of a dropout entry: every array present and 4-byte aligned (the kernels read 32-bit words of keep / keep_t), s = 1 / (1 - p) >= 1
int check_mask(const CMask& mk, bool bwd) {
    if (!mk.keep || !mk.keep0 || (bwd && !mk.keep_t)) return AMDNUWA_ERR_ARG;
    if (((uintptr_t)mk.keep | (uintptr_t)mk.keep0 | (bwd ? (uintptr_t)mk.keep_t : 0)) & 3) return AMDNUWA_ERR_ARG;
    if (!(mk.s >= 1.f) || mk.s > 3.0e38f) return AMDNUWA_ERR_ARG;                           // (NaN fails the first comparison)
    return AMDNUWA_OK;
}

// The half of CArgs the forward and the backward run share: inputs, key mask, null key / value, W_th and the geometry.  Everything else
// stays zero; a run adds its own operands.
CArgs c_args(const amdnuwa_cattn_geom* g, const uint16_t* q, int ldq, const uint16_t* k, const uint16_t* v, int ldkv, const uint8_t* key_mask,
             const float* null_k, const float* null_v, const float* w_th, const float* stats) {
    CArgs a{};
    a.q = q; a.k = k; a.v = v; a.ldq = ldq; a.ldkv = ldkv; a.mask = key_mask;
    a.null_k = null_k; a.null_v = null_v; a.wth = w_th; a.stats = const_cast<float*>(stats);
    a.B = g->B; a.n = g->n; a.nk = keys_of(g); a.heads = g->heads; a.causal = g->causal ? 1 : 0; a.scale = g->scale; a.c1 = g->scale * 1.4426950408889634f;
    return a;
}

// one body of amdnuwa_cattn_fwd and amdnuwa_cattn_fwd_drop (mk == NULL: the unmasked kernels)
int cattn_fwd_run(const amdnuwa_cattn_geom* g, const uint16_t* q16, int ldq, const uint16_t* k16, const uint16_t* v16, int ldkv, const uint8_t* key_mask,
                  const float* null_k, const float* null_v, const float* w_th, uint16_t* o, uint16_t* o_lo, int ldo, int o_lo_f16, float* stats, int f16,
                  const CMask* mk, hipStream_t stream) {
    int rc = check_c(g);
    if (rc) return rc;
    if (!q16 || !k16 || !v16 || !null_k || !null_v || !w_th || !stats || ldq % 8 || ldkv % 8 || ldo % 4) return AMDNUWA_ERR_ARG;
    if (ldq < g->heads * g->dim_head || ldkv < g->heads * g->dim_head || ldo < g->heads * g->dim_head) return AMDNUWA_ERR_ARG;
    if (!o && !(o_lo && o_lo_f16)) return AMDNUWA_ERR_ARG;
    if (mk && (rc = check_mask(*mk, false))) return rc;
    CArgs a = c_args(g, q16, ldq, k16, v16, ldkv, key_mask, null_k, null_v, w_th, stats);
    a.o = o; a.ol = o_lo; a.ldo = ldo; a.ol_f16 = (o_lo && o_lo_f16) ? 1 : 0;
    const dim3 grid((unsigned)wgs(g));
    return launch_if(mk != nullptr, [&](auto drop) {
        const CKArgs<drop()> ka = c_kargs<drop()>(a, mk ? *mk : CMask{});
        return launch_pick<64, 32>(g->dim_head, [&](auto dh) { return launch_if(f16 != 0, [&](auto h) {
            return launch_kernel(cattn_apply_kernel<dh(), h(), false, drop()>, grid, dim3(256), lds_apply(g), true, stream, ka); }); });
    });
}

// one body of amdnuwa_cattn_bwd and amdnuwa_cattn_bwd_drop (mk == NULL: the unmasked kernels); the workspace is the same
int cattn_bwd_run(const amdnuwa_cattn_geom* g, const uint16_t* q, int ldq, const uint16_t* k, const uint16_t* v, int ldkv, const uint16_t* dO, int lddo,
                  const uint8_t* key_mask, const float* null_k, const float* null_v, const float* w_th, const float* stats, uint16_t* dq, int lddq,
                  uint16_t* dk, uint16_t* dv, int lddkv, float* dw_th, float* dnull_k, float* dnull_v, void* workspace, size_t workspace_bytes,
                  const CMask* mk, hipStream_t stream) {
    int rc = check_c(g);
    if (rc) return rc;
    if (!q || !k || !v || !dO || !null_k || !null_v || !w_th || !stats || !dq || !dk || !dv || !dw_th || !dnull_k || !dnull_v) return AMDNUWA_ERR_ARG;
    const int inner = g->heads * g->dim_head;
    if (ldq % 8 || ldkv % 8 || lddo % 8 || lddq % 4 || lddkv % 4 || ldq < inner || ldkv < inner || lddo < inner || lddq < inner || lddkv < inner) return AMDNUWA_ERR_ARG;
    if (mk && (rc = check_mask(*mk, true))) return rc;
    if (!workspace || workspace_bytes < amdnuwa_cattn_bwd_workspace_bytes(g)) return AMDNUWA_ERR_WORKSPACE;
    const size_t rows = (size_t)g->B * g->n;
    char* wp = (char*)workspace;
    auto take = [&](size_t bytes) { char* p = wp; wp += al(bytes); return p; };
    CArgs a = c_args(g, q, ldq, k, v, ldkv, key_mask, null_k, null_v, w_th, stats);
    a.dO = dO; a.lddo = lddo; a.dq = dq; a.dk = dk; a.dv = dv; a.lddq = lddq; a.lddkv = lddkv;
    a.delta = (float*)take(rows * g->heads * 4);
    a.ds0 = (float*)take(rows * NHM * 4);
    a.a0 = (float*)take(rows * NHM * 4);
    a.part_th = (float*)take((size_t)wgs(g) * 64 * 4);
    float* part_null = (float*)take((size_t)null_chunks(g) * 2 * inner * 4);
    float* dnull = (float*)take((size_t)2 * inner * 4);
    const size_t cs1 = amdnuwa_colsum_workspace_bytes(wgs(g), 64), cs2 = amdnuwa_colsum_workspace_bytes(null_chunks(g), 2 * inner);
    void* cws1 = take(cs1);
    void* cws2 = take(cs2);
    const dim3 grid((unsigned)wgs(g)), grid_k((unsigned)wgs_k(g)), block(256);
    // 1. delta, the talking-heads partials and the null key's dS / A per query;  2. dq (query-stationary), dk and dv (key-stationary)
    rc = launch_if(mk != nullptr, [&](auto drop) {
        const CKArgs<drop()> ka = c_kargs<drop()>(a, mk ? *mk : CMask{});
        return launch_pick<64, 32>(g->dim_head, [&](auto dh) {
            int r = launch_kernel(cattn_grad_kernel<dh(), false, 0, drop()>, grid, block, lds_grad(g, 0), true, stream, ka);
            if (!r) r = launch_kernel(cattn_grad_kernel<dh(), false, 1, drop()>, grid, block, lds_grad(g, 1), true, stream, ka);
            if (!r) r = launch_kernel(cattn_grad_kernel<dh(), true, 1, drop()>, grid_k, block, lds_grad(g, 1), true, stream, ka);
            if (!r) r = launch_kernel(cattn_apply_kernel<dh(), false, true, drop()>, grid_k, block, lds_apply(g), true, stream, ka);
            return r;
        });
    });
    if (rc) return rc;
    // 3. the small gradients: fixed-order reductions of the partials
    rc = launch_kernel(cattn_null_grads_kernel, dim3((unsigned)null_chunks(g)), block, 0, false, stream, q, ldq, dO, lddo, a.ds0, a.a0, part_null, (long)rows,
                       inner, g->dim_head);
    if (rc) return rc;
    rc = amdnuwa_colsum(a.part_th, dw_th, wgs(g), 64, 0, cws1, cs1, stream);
    if (rc) return rc;
    rc = amdnuwa_colsum(part_null, dnull, null_chunks(g), 2 * inner, 0, cws2, cs2, stream);
    if (rc) return rc;
    if (hipMemcpyAsync(dnull_k, dnull, (size_t)inner * 4, hipMemcpyDeviceToDevice, stream) != hipSuccess) return AMDNUWA_ERR_ARG;
    if (hipMemcpyAsync(dnull_v, dnull + inner, (size_t)inner * 4, hipMemcpyDeviceToDevice, stream) != hipSuccess) return AMDNUWA_ERR_ARG;
    return AMDNUWA_OK;
}

}  // namespace

extern "C" int amdnuwa_cattn_supported(const amdnuwa_cattn_geom* g) { return check_c(g) == AMDNUWA_OK; }
extern "C" int amdnuwa_cattn_drop_supported(const amdnuwa_cattn_geom* g) { return check_c(g) == AMDNUWA_OK; }

extern "C" size_t amdnuwa_cattn_bwd_workspace_bytes(const amdnuwa_cattn_geom* g) {
    if (check_c(g)) return 0;
    const size_t rows = (size_t)g->B * g->n, inner = (size_t)g->heads * g->dim_head;
    return al(rows * g->heads * 4) + 2 * al(rows * NHM * 4) + al((size_t)wgs(g) * 64 * 4) + al((size_t)null_chunks(g) * 2 * inner * 4) + al(2 * inner * 4) +
           al(amdnuwa_colsum_workspace_bytes(wgs(g), 64)) + al(amdnuwa_colsum_workspace_bytes(null_chunks(g), (int)(2 * inner)));
}

extern "C" int amdnuwa_cattn_fwd(const amdnuwa_cattn_geom* g, const uint16_t* q16, int ldq, const uint16_t* k16, const uint16_t* v16, int ldkv,
                                 const uint8_t* key_mask, const float* null_k, const float* null_v, const float* w_th, uint16_t* o, uint16_t* o_lo,
                                 int ldo, int o_lo_f16, float* stats, int f16, hipStream_t stream) {
    return cattn_fwd_run(g, q16, ldq, k16, v16, ldkv, key_mask, null_k, null_v, w_th, o, o_lo, ldo, o_lo_f16, stats, f16, nullptr, stream);
}

extern "C" int amdnuwa_cattn_fwd_drop(const amdnuwa_cattn_geom* g, const uint16_t* q16, int ldq, const uint16_t* k16, const uint16_t* v16, int ldkv,
                                      const uint8_t* key_mask, const float* null_k, const float* null_v, const float* w_th, uint16_t* o, uint16_t* o_lo,
                                      int ldo, int o_lo_f16, float* stats, int f16, const uint8_t* keep, const uint8_t* keep0, float drop_scale,
                                      hipStream_t stream) {
    const CMask mk{keep, nullptr, keep0, drop_scale};
    return cattn_fwd_run(g, q16, ldq, k16, v16, ldkv, key_mask, null_k, null_v, w_th, o, o_lo, ldo, o_lo_f16, stats, f16, &mk, stream);
}

extern "C" int amdnuwa_cattn_bwd(const amdnuwa_cattn_geom* g, const uint16_t* q, int ldq, const uint16_t* k, const uint16_t* v, int ldkv,
                                 const uint16_t* dO, int lddo, const uint8_t* key_mask, const float* null_k, const float* null_v, const float* w_th,
                                 const float* stats, uint16_t* dq, int lddq, uint16_t* dk, uint16_t* dv, int lddkv, float* dw_th, float* dnull_k,
                                 float* dnull_v, void* workspace, size_t workspace_bytes, hipStream_t stream) {
    return cattn_bwd_run(g, q, ldq, k, v, ldkv, dO, lddo, key_mask, null_k, null_v, w_th, stats, dq, lddq, dk, dv, lddkv, dw_th, dnull_k, dnull_v, workspace,
                         workspace_bytes, nullptr, stream);
}

extern "C" int amdnuwa_cattn_bwd_drop(const amdnuwa_cattn_geom* g, const uint16_t* q, int ldq, const uint16_t* k, const uint16_t* v, int ldkv,
                                      const uint16_t* dO, int lddo, const uint8_t* key_mask, const float* null_k, const float* null_v, const float* w_th,
                                      const float* stats, uint16_t* dq, int lddq, uint16_t* dk, uint16_t* dv, int lddkv, float* dw_th, float* dnull_k,
                                      float* dnull_v, void* workspace, size_t workspace_bytes, const uint8_t* keep, const uint8_t* keep_t,
                                      const uint8_t* keep0, float drop_scale, hipStream_t stream) {
    const CMask mk{keep, keep_t, keep0, drop_scale};
    return cattn_bwd_run(g, q, ldq, k, v, ldkv, dO, lddo, key_mask, null_k, null_v, w_th, stats, dq, lddq, dk, dv, lddkv, dw_th, dnull_k, dnull_v, workspace,
                         workspace_bytes, &mk, stream);
}

AMDNUWA_SAT_ACCESSOR(cattn)
