// Every index the many-head Sparse3DNA window kernels (sparse3dna_mh.hip, 9 .. 16 heads) form, and the host-side sizes their launches
// rest on, as small inline functions.  The kernels form addresses with these and nothing else; tools/s3mh_index_walk.cpp includes the same
// header in a plain host compile and walks every workgroup, thread, plane, tap and item of a case list through them under a sanitizer,
// checking each index against the extent the launcher allocates or the caller passes.  Plain C++: no HIP header is needed to read it.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/amdnuwa.h"

#if defined(__HIPCC__)
#define S3MH_HD __host__ __device__ __forceinline__
#else
#define S3MH_HD inline
#endif

constexpr int S3MH_MH = 16;          // compile-time head bound: the padded talking-heads matrix in LDS is [MH][MH]
constexpr int S3MH_MIN = 9;          // the kernels of sparse3dna.hip / sparse3dna_wide.hip serve 1 .. 8 heads
constexpr int S3MH_NG = 4;           // item groups of the dW_th partial reduction: RED is [NG][NH * NH], whatever the block size
constexpr size_t S3MH_LDS_MAX = 160 * 1024 - 2048;     // dynamic LDS of one launch (S3_LDS_MAX of sparse3dna.hip): the CU's 160 KiB less room for
                                                       // the kernels' static arrays (the [MH][MH] matrix: 1 KiB)

// ---- host-side sizes ---------------------------------------------------------------------------------------------------------
// Column tiles of a grid row: the arithmetic of s3_tile() (s3_args.h), which the workspace map s3_ws() counts its partials with.  A row
// of W * heads * 4 <= 512 threads is ONE tile that stages the whole row (sw = W, staged column 0 = grid column 0); a wider one is cut into
// nt balanced tiles of tw <= 128 / heads columns, each staging its own columns plus the (kw-1)*dw halo the taps reach.
struct S3mhTile { int tw, nt, sw; };
inline S3mhTile s3mh_tile(const amdnuwa_s3_geom* g) {
    if (g->W * g->heads * 4 <= 512) return {g->W, 1, g->W};
    const int twmax = 128 / g->heads, nt = (g->W + twmax - 1) / twmax, tw = (g->W + nt - 1) / nt;
    long long halo = (long long)(g->kw - 1) * g->dw;
    if (halo > 65536) halo = 65536;                       // (far beyond any LDS: the entry points refuse it, no kernel sees the clipped value)
    return {tw, nt, tw + (int)halo};
}
inline size_t s3mh_slots(const amdnuwa_s3_geom* g) { return (size_t)g->kf * g->kh * g->kw + 1; }
S3MH_HD int s3mh_threads(int tw, int nh) { return ((tw * nh * 4 + 63) / 64) * 64; }

// Dynamic LDS bytes of the forward, the query-side and the key-side backward (lo = hi + lo operand pairs).  Query side: the staged
// image, then SP and DP (the <bos> partial reduction reuses them as [tw][inner]: spdp = max(2 nsp, tw * inner) floats), then RED.
struct S3mhLds { size_t fwd, bq, bkv; };
inline S3mhLds s3mh_lds(const amdnuwa_s3_geom* g, bool lo) {
    const S3mhTile tl = s3mh_tile(g);
    const size_t J = s3mh_slots(g), inner = (size_t)g->heads * g->dim_head, tw = (size_t)tl.tw, sw = (size_t)tl.sw;
    const size_t stage = sw * inner * (lo ? 4 : 2), nsp = tw * J * g->heads;
    size_t spdp = 2 * nsp;
    if (spdp < tw * inner) spdp = tw * inner;
    return {stage + nsp * 4, stage + (spdp + (size_t)S3MH_NG * g->heads * g->heads) * 4, sw * inner * 8};
}
inline size_t s3mh_lds_need(const amdnuwa_s3_geom* g, bool lo) {
    const S3mhLds l = s3mh_lds(g, lo);
    const size_t m = l.fwd > l.bq ? l.fwd : l.bq;
    return m > l.bkv ? m : l.bkv;
}

// ---- LDS ---------------------------------------------------------------------------------------------------------------------
// Staged image of SW columns (bf16 elements from the start of its hi or lo region): 16-byte slot s = (sc*NH + h)*4 + c of staged column
// sc; half v8 of a chunk of CH = DH/4 elements sits v8 * HS further, HS = SW*NH*32, so a region holds (CH/8) * HS = SW*NH*DH elements.
S3MH_HD int s3mh_hs(int sw, int nh) { return sw * nh * 32; }
S3MH_HD int s3mh_stage_elems(int sw, int nh, int dh) { return sw * nh * dh; }
S3MH_HD int s3mh_st_write(int s, int v8, int hs) { return v8 * hs + s * 8; }
S3MH_HD int s3mh_st_read(int sc, int h, int c, int nh) { return ((sc * nh + h) * 4 + c) * 8; }      // half v8 at + v8 * hs
// grid column of staged column 0: `back` = halo columns that lie before the tile's own (query side: ow*dw, key side: (kw-1-ow)*dw)
S3MH_HD int s3mh_c0(int nt, int w0, int back) { return nt == 1 ? 0 : w0 - back; }
// score tables SP / DP [wt][j][h] (floats)
S3MH_HD int s3mh_tab(int wt, int j, int h, int J, int nh) { return (wt * J + j) * nh + h; }
S3MH_HD int s3mh_tab_item(int item, int h, int nh) { return item * nh + h; }                          // item = wt*J + j
// talking-heads matrix, zero-padded to [MH][MH] (static LDS), and its source [NH][NH]
S3MH_HD int s3mh_wsh(int g, int h) { return g * S3MH_MH + h; }
S3MH_HD int s3mh_wth(int g, int h, int nh) { return g * nh + h; }
// dW_th partials of item group grp (floats of RED)
S3MH_HD int s3mh_red(int grp, int pair, int nh) { return grp * nh * nh + pair; }
// <bos> partial of tile column wt (floats of the SP + DP space)
S3MH_HD int s3mh_rk(int wt, int e, int inner) { return wt * inner + e; }
S3MH_HD int s3mh_col(int h, int c, int dh) { return h * dh + c * (dh / 4); }                           // first column of chunk c of head h
// byte offsets of the regions of the dynamic LDS block (query side; the forward ends after SP)
S3MH_HD size_t s3mh_off_sp(int sw, int nh, int dh, bool lo) { return (size_t)s3mh_stage_elems(sw, nh, dh) * (lo ? 4 : 2); }
S3MH_HD int s3mh_nsp(int tw, int J, int nh) { return tw * J * nh; }
S3MH_HD int s3mh_spdp(int tw, int J, int nh, int dh) { const int a = 2 * s3mh_nsp(tw, J, nh), b = tw * nh * dh; return a > b ? a : b; }

// ---- global memory (element offsets) --------------------------------------------------------------------------------------------
// chunk (h, c) of row i of sample b in a tensor of `rows` rows per sample and `ld` elements per row: q, o, dO, dq (rows = ntok), dk, dv
S3MH_HD size_t s3mh_g_tok(int b, int rows, int i, int ld, int h, int c, int dh) { return ((size_t)b * rows + i) * ld + s3mh_col(h, c, dh); }
// element e of the <bos> row (row 0) of sample b
S3MH_HD size_t s3mh_g_bos(int b, int rows, int ld, int e) { return (size_t)b * rows * ld + e; }
// slot-0 key / value row: per-sample stride bs
S3MH_HD size_t s3mh_g_k0(int b, long long bs, int h, int c, int dh) { return (size_t)b * (size_t)bs + s3mh_col(h, c, dh); }
// 16-byte half v8 of staging slot r = h*4 + c of tensor row `row`
S3MH_HD size_t s3mh_g_stage(size_t row, int ld, int r, int ch, int v8) { return row * ld + r * ch + v8 * 8; }
// ds / P' workspace [B][nq][J][NH]; iq = 0-based query (token row - 1)
S3MH_HD size_t s3mh_g_ws(int b, int nq, int iq, int J, int j, int nh, int h) { return (((size_t)b * nq + iq) * J + j) * nh + h; }
// per-(row, tile) partials
S3MH_HD size_t s3mh_g_part(int bid, int n, int e) { return (size_t)bid * n + e; }
S3MH_HD int s3mh_g_bias(int j, int nh, int h) { return j * nh + h; }
