// CPU walk of every index the many-head Sparse3DNA window kernels (nuwa_pytorch_amd/csrc/sparse3dna_mh.hip) form.
//
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I nuwa_pytorch_amd/csrc tools/s3mh_index_walk.cpp -o walk
//     ./walk CASEFILE        (one case per line: B ntok F H W kf kh kw df dh dw heads dim_head lo bias)
//
// The kernels form addresses with the functions of s3mh_index.h and nothing else; this program includes the same header (a plain host
// compile: no HIP, no device) and, per case, replays the loop structure of the three kernels for every workgroup, thread, tap plane, tap and
// item.  Operands, outputs, the workspace and the LDS block are real host arrays of exactly the size the caller passes or the launcher
// allocates (s3mh_lds(), the s3_ws() map restated below), one byte per element, so an index outside its extent fails the explicit check
// AND trips the sanitizer.  It asserts that every index lies inside its extent -- for a 16-byte access, all 8 elements, inside the column
// range of its operand -- and that every output element and every partial is written exactly once: o and dq in all B * ntok rows, dk / dv
// in the rows 1 .. ntok - 1 (row 0 is s3_bwd_fin_kernel's, which is not walked: it is the 8-head kernels' own), ds and P' in every
// [b][query][slot][head], the dW_th and <bos> partials of every (row, tile) workgroup.  Prints `cases walked: N, indices checked: M`.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "s3mh_index.h"

static unsigned long long g_checked = 0;
static std::string g_case;

#define CHECK(cond, ...)                                                                       \
    do {                                                                                       \
        ++g_checked;                                                                           \
        if (!(cond)) {                                                                         \
            std::fprintf(stderr, "FAILED %s (line %d) in case %s: ", #cond, __LINE__, g_case.c_str()); \
            std::fprintf(stderr, __VA_ARGS__);                                                 \
            std::fprintf(stderr, "\n");                                                        \
            std::exit(1);                                                                      \
        }                                                                                      \
    } while (0)

// a flat array, one byte per element: reads touch it (the sanitizer sees the address), writes count
struct Buf {
    std::vector<unsigned char> n;
    const char* name;
    Buf(const char* nm, size_t elems) : n(elems, 0), name(nm) {}
    void rd(size_t i, size_t len = 1) const {
        CHECK(i + len <= n.size() && i + len >= i, "%s: read [%zu, +%zu) of %zu", name, i, len, n.size());
        volatile unsigned char sink = 0;
        for (size_t k = 0; k < len; ++k) sink = n.data()[i + k];
        (void)sink;
    }
    void wr(size_t i, size_t len = 1) {
        CHECK(i + len <= n.size() && i + len >= i, "%s: write [%zu, +%zu) of %zu", name, i, len, n.size());
        for (size_t k = 0; k < len; ++k) if (n.data()[i + k] < 255) ++n.data()[i + k];
    }
};
// an operand: `cols` columns from column `off` of a row-major [rows, ld] array (q | k | v share one, as the wrappers pass them)
struct Tensor {
    Buf* b; size_t off; int ld, cols; size_t rows;
    size_t at(size_t idx, size_t len) const {
        const size_t col = idx % ld;          // idx counts from the operand's own pointer
        CHECK(idx / ld < rows && col + len <= (size_t)cols, "%s: element %zu (+%zu) is row %zu column %zu of [%zu, %d]", b->name, idx, len, idx / ld, col, rows, cols);
        return off + idx;
    }
    void rd(size_t idx, size_t len = 1) const { b->rd(at(idx, len), len); }
    void wr(size_t idx, size_t len = 1) const { b->wr(at(idx, len), len); }
};

struct Args {      // the S3Args fields the kernels read, as the entry points fill them
    int B, ntok, F, H, W, kf, kh, kw, df, dh, dw, NH, DH, of, oh, ow, NT, TW, SW, J, lo, bias;
    long long k0_bs;
};
struct TilePos { int bid, b, ry, f, y, w0, tw; };

static int xcd_row_id(int id, int nb) {
    const int per = nb >> 3, rem = nb & 7, x = id & 7, k = id >> 3;
    return x * per + (x < rem ? x : rem) + k;
}
static TilePos tile_pos(const Args& a, int bid) {
    TilePos p;
    const int rows = a.F * a.H;
    p.bid = bid;
    const int rt = bid / a.NT, tl = bid - rt * a.NT;
    p.b = rt / rows; p.ry = rt % rows; p.f = p.ry / a.H; p.y = p.ry % a.H;
    p.w0 = tl * a.TW;
    p.tw = a.W - p.w0 < a.TW ? a.W - p.w0 : a.TW;
    CHECK(p.b >= 0 && p.b < a.B && p.tw >= 1 && p.tw <= a.TW, "workgroup %d: sample %d, %d columns", bid, p.b, p.tw);
    return p;
}

struct World {
    Args a;
    int nthreads;
    size_t lds_fwd, lds_bq, lds_bkv;
    // global memory, as kernels.sparse3dna_mh_fwd / _bwd allocate it
    Buf qkv, qkv_lo, o, o_lo, dO, dO_lo, dqkv, dqkv_lo, wth, biasb, ws;
    Tensor q, k, v, ql, kl, vl, to, tol, tdO, tdOl, dq, dk, dv, dql, dkl, dvl;
    size_t items, parts, off_pm, off_th, off_k0, off_v0, ws_floats;
    // LDS: the dynamic block (bytes) and the static talking-heads matrix (floats)
    Buf lds, wsh;
    World(const Args& a_, const amdnuwa_s3_geom& g)
        : a(a_), nthreads(s3mh_threads(a_.TW, a_.NH)),
          qkv("qkv", (size_t)a_.B * a_.ntok * 3 * a_.NH * a_.DH), qkv_lo("qkv_lo", qkv.n.size()),
          o("o", (size_t)a_.B * a_.ntok * a_.NH * a_.DH), o_lo("o_lo", o.n.size()), dO("dO", o.n.size()), dO_lo("dO_lo", o.n.size()),
          dqkv("dqkv", qkv.n.size()), dqkv_lo("dqkv_lo", qkv.n.size()), wth("w_th", (size_t)a_.NH * a_.NH), biasb("rel_bias", (size_t)a_.J * a_.NH),
          ws("workspace", 0), lds("dynamic LDS", 0), wsh("wsh", S3MH_MH * S3MH_MH) {
        const S3mhLds l = s3mh_lds(&g, a.lo != 0);
        lds_fwd = l.fwd; lds_bq = l.bq; lds_bkv = l.bkv;
        const int inner = a.NH * a.DH, ld3 = 3 * inner;
        const size_t R = (size_t)a.B * a.ntok;
        auto T = [&](Buf& b, int part, int ld) { return Tensor{&b, (size_t)part * inner, ld, inner, R}; };
        q = T(qkv, 0, ld3); k = T(qkv, 1, ld3); v = T(qkv, 2, ld3); ql = T(qkv_lo, 0, ld3); kl = T(qkv_lo, 1, ld3); vl = T(qkv_lo, 2, ld3);
        to = T(o, 0, inner); tol = T(o_lo, 0, inner); tdO = T(dO, 0, inner); tdOl = T(dO_lo, 0, inner);
        dq = T(dqkv, 0, ld3); dk = T(dqkv, 1, ld3); dv = T(dqkv, 2, ld3); dql = T(dqkv_lo, 0, ld3); dkl = T(dqkv_lo, 1, ld3); dvl = T(dqkv_lo, 2, ld3);
        // the workspace map s3_ws() of sparse3dna.hip, in floats (the column-sum scratch behind it belongs to amdnuwa_colsum)
        items = (size_t)a.B * (a.ntok - 1) * a.J * a.NH;
        parts = (size_t)a.B * a.F * a.H * a.NT;
        off_pm = items; off_th = 2 * items; off_k0 = off_th + parts * a.NH * a.NH; off_v0 = off_k0 + parts * inner; ws_floats = off_v0 + parts * inner;
        ws.n.assign(ws_floats, 0);
    }
    // ---- LDS accessors: element index inside a region + the region's place in the block of `total` bytes ----
    void lds_touch(size_t byte0, size_t bytes, size_t total) { CHECK(byte0 + bytes <= total, "LDS bytes [%zu, +%zu) of %zu", byte0, bytes, total); lds.rd(byte0, bytes); }
    // staged image region `reg` (0 = hi, 1 = lo; key side: 0 .. 3), 8 bf16 elements from element e
    void stage8(int reg, int e, size_t total) {
        const int se = s3mh_stage_elems(a.SW, a.NH, a.DH);
        CHECK(e >= 0 && e + 8 <= se && e % 8 == 0, "staged element %d (+8) of %d", e, se);
        lds_touch(((size_t)reg * se + e) * 2, 16, total);
    }
    size_t off_sp() const { return s3mh_off_sp(a.SW, a.NH, a.DH, a.lo != 0); }
    void sp(int idx, size_t total) { CHECK(idx >= 0 && idx < s3mh_nsp(a.TW, a.J, a.NH), "SP[%d]", idx); lds_touch(off_sp() + (size_t)idx * 4, 4, total); }
    void dp(int idx) { const int nsp = s3mh_nsp(a.TW, a.J, a.NH); CHECK(idx >= 0 && idx < nsp && 2 * nsp <= s3mh_spdp(a.TW, a.J, a.NH, a.DH), "DP[%d]", idx); lds_touch(off_sp() + ((size_t)nsp + idx) * 4, 4, lds_bq); }
    void red(int idx) { CHECK(idx >= 0 && idx < S3MH_NG * a.NH * a.NH, "RED[%d]", idx); lds_touch(off_sp() + ((size_t)s3mh_spdp(a.TW, a.J, a.NH, a.DH) + idx) * 4, 4, lds_bq); }
    void rk(int idx) { CHECK(idx >= 0 && idx < s3mh_spdp(a.TW, a.J, a.NH, a.DH), "RK[%d]", idx); lds_touch(off_sp() + (size_t)idx * 4, 4, lds_bq); }
    void wsh_at(int idx) { CHECK(idx >= 0 && idx < S3MH_MH * S3MH_MH, "wsh[%d]", idx); wsh.rd(idx); }
    size_t ws_item(size_t idx) { CHECK(idx < items, "ds / P' item %zu of %zu", idx, items); return idx; }
    size_t ws_part(size_t idx, size_t n) { CHECK(idx < parts * n, "partial %zu of %zu", idx, parts * n); return idx; }
};

// stage_cols of the kernels: slots s = t, t + nt, ... of one thread; the leading dimension is the operand's (q / k / v: 3 * inner, dO: inner)
static void stage_cols(World& w, const Tensor& src, const Tensor* srcl, size_t base_row, int pos0, int c0, int nrows_left, int reg_hi, int reg_lo, int t, size_t total) {
    const Args& a = w.a;
    const int CH = a.DH / 4, HS = s3mh_hs(a.SW, a.NH), nh4 = a.NH * 4, nslot = a.SW * nh4;
    for (int s = t; s < nslot; s += w.nthreads) {
        const int sc = s / nh4, r = s - sc * nh4, wc = c0 + sc;
        const bool ok = wc >= 0 && wc < a.W && pos0 + wc < nrows_left;
        for (int v8 = 0; v8 < CH / 8; ++v8) {
            const int li = s3mh_st_write(s, v8, HS);
            w.stage8(reg_hi, li, total);
            if (srcl) w.stage8(reg_lo, li, total);
            if (ok) {
                const size_t gi = s3mh_g_stage(base_row + pos0 + wc, src.ld, r, CH, v8);
                src.rd(gi, 8);
                if (srcl) srcl->rd(gi, 8);
            }
        }
    }
}

// sweep_taps of the kernels for one thread; tap(j) is called for every valid tap slot
template <class Fn>
static void sweep_taps(World& w, const Tensor& src, const Tensor* srcl, const TilePos& p, int t, size_t total, Fn&& tap) {
    const Args& a = w.a;
    const int c = t & 3, wh = t >> 2, h = wh % a.NH, wt = wh / a.NH, wq = p.w0 + wt;
    const bool qvalid = wt < p.tw && 1 + p.ry * a.W + wq < a.ntok;
    const int CH = a.DH / 4, HS = s3mh_hs(a.SW, a.NH);
    const int c0 = s3mh_c0(a.NT, p.w0, a.ow * a.dw);
    int fr = p.f - a.of * a.df;
    for (int ta = 0; ta < a.kf; ++ta, fr += a.df) {
        if (fr < 0 || fr >= a.F) continue;
        int yr = p.y - a.oh * a.dh;
        for (int tb = 0; tb < a.kh; ++tb, yr += a.dh) {
            if (yr < 0 || yr >= a.H) continue;
            const int pos0 = (fr * a.H + yr) * a.W;
            stage_cols(w, src, srcl, (size_t)p.b * a.ntok + 1, pos0, c0, a.ntok - 1, 0, 1, t, total);
            if (!qvalid) continue;
            const int jb = 1 + (ta * a.kh + tb) * a.kw;
            int wr = wq - a.ow * a.dw;
            for (int tc = 0; tc < a.kw; ++tc, wr += a.dw) {
                if (wr < 0 || wr >= a.W) continue;
                CHECK(wr - c0 >= 0 && wr - c0 < a.SW, "tap column %d is staged column %d of %d", wr, wr - c0, a.SW);
                // causal window: the key lies at or before the query, so inside the sequence -- its staged slot holds data, not the zero fill
                CHECK(pos0 + wr < a.ntok - 1, "tap position %d beyond the %d keys", pos0 + wr, a.ntok - 1);
                const int slot = s3mh_st_read(wr - c0, h, c, a.NH);
                for (int v8 = 0; v8 < CH / 8; ++v8) {
                    w.stage8(0, slot + v8 * HS, total);
                    if (srcl) w.stage8(1, slot + v8 * HS, total);
                }
                CHECK(jb + tc >= 1 && jb + tc < a.J, "slot %d of %d", jb + tc, a.J);
                tap(jb + tc);
            }
        }
    }
}

static void load_wsh(World& w, int t) {
    const Args& a = w.a;
    for (int e = t; e < S3MH_MH * S3MH_MH; e += w.nthreads) {
        const int g = e / S3MH_MH, h = e - g * S3MH_MH;
        w.wsh_at(s3mh_wsh(g, h));
        if (g < a.NH && h < a.NH) w.wth.rd(s3mh_wth(g, h, a.NH));
    }
}

static void scores_softmax(World& w, const TilePos& p, int t, size_t total) {
    const Args& a = w.a;
    const int c = t & 3, wh = t >> 2, h = wh % a.NH, wt = wh / a.NH, CH = a.DH / 4;
    const bool act = wt < p.tw, qvalid = act && 1 + p.ry * a.W + p.w0 + wt < a.ntok;
    for (int e = t; e < s3mh_nsp(a.TW, a.J, a.NH); e += w.nthreads) w.sp(e, total);
    if (qvalid) {
        const size_t g = s3mh_g_k0(p.b, a.k0_bs, h, c, a.DH);
        w.k.rd(g, CH);
        if (a.lo) w.kl.rd(g, CH);
        if (c == 0) { w.sp(s3mh_tab(wt, 0, h, a.J, a.NH), total); if (a.bias) w.biasb.rd(s3mh_g_bias(0, a.NH, h)); }
    }
    sweep_taps(w, w.k, a.lo ? &w.kl : nullptr, p, t, total, [&](int j) {
        if (c == 0) { w.sp(s3mh_tab(wt, j, h, a.J, a.NH), total); if (a.bias) w.biasb.rd(s3mh_g_bias(j, a.NH, h)); }
    });
    if (act) for (int j = c; j < a.J; j += 4) w.sp(s3mh_tab(wt, j, h, a.J, a.NH), total);
}

static void fwd_thread(World& w, const TilePos& p, int t) {
    const Args& a = w.a;
    const int c = t & 3, wh = t >> 2, h = wh % a.NH, wt = wh / a.NH, CH = a.DH / 4, inner = a.NH * a.DH;
    const int i = 1 + p.ry * a.W + p.w0 + wt;
    const bool act = wt < p.tw, qvalid = act && i < a.ntok;
    const size_t total = w.lds_fwd;
    load_wsh(w, t);
    if (p.ry == 0 && p.w0 == 0)
        for (int e = t; e < inner; e += w.nthreads) {
            w.v.rd(s3mh_g_bos(p.b, a.ntok, 3 * inner, e));
            if (a.lo) w.vl.rd(s3mh_g_bos(p.b, a.ntok, 3 * inner, e));
            w.to.wr(s3mh_g_bos(p.b, a.ntok, inner, e));
            if (a.lo) w.tol.wr(s3mh_g_bos(p.b, a.ntok, inner, e));
        }
    if (p.ry * a.W + p.w0 + 1 >= a.ntok) return;
    if (qvalid) { const size_t g = s3mh_g_tok(p.b, a.ntok, i, 3 * inner, h, c, a.DH); w.q.rd(g, CH); if (a.lo) w.ql.rd(g, CH); }
    scores_softmax(w, p, t, total);
    for (int item = t; item < p.tw * a.J; item += w.nthreads) {
        for (int hh = 0; hh < S3MH_MH; ++hh) if (hh < a.NH) w.sp(s3mh_tab_item(item, hh, a.NH), total);
        for (int g = 0; g < a.NH; ++g) {
            for (int hh = 0; hh < S3MH_MH; ++hh) w.wsh_at(s3mh_wsh(g, hh));
            w.sp(s3mh_tab_item(item, g, a.NH), total);
        }
    }
    if (qvalid) {
        const size_t g = s3mh_g_k0(p.b, a.k0_bs, h, c, a.DH);
        w.sp(s3mh_tab(wt, 0, h, a.J, a.NH), total);
        w.v.rd(g, CH);
        if (a.lo) w.vl.rd(g, CH);
    }
    sweep_taps(w, w.v, a.lo ? &w.vl : nullptr, p, t, total, [&](int j) { w.sp(s3mh_tab(wt, j, h, a.J, a.NH), total); });
    if (qvalid) {
        const size_t g = s3mh_g_tok(p.b, a.ntok, i, inner, h, c, a.DH);
        w.to.wr(g, CH);
        if (a.lo) w.tol.wr(g, CH);
    }
}

static void bwd_q_thread(World& w, const TilePos& p, int t) {
    const Args& a = w.a;
    const int c = t & 3, wh = t >> 2, h = wh % a.NH, wt = wh / a.NH, CH = a.DH / 4, inner = a.NH * a.DH, nn = a.NH * a.NH;
    const int i = 1 + p.ry * a.W + p.w0 + wt, nq = a.ntok - 1, nit = p.tw * a.J;
    const bool act = wt < p.tw, qvalid = act && i < a.ntok;
    const size_t total = w.lds_bq;
    load_wsh(w, t);
    if (p.ry == 0 && p.w0 == 0)
        for (int e = t; e < inner; e += w.nthreads) { w.dq.wr(s3mh_g_bos(p.b, a.ntok, 3 * inner, e)); if (a.lo) w.dql.wr(s3mh_g_bos(p.b, a.ntok, 3 * inner, e)); }
    if (p.ry * a.W + p.w0 + 1 >= a.ntok) {
        for (int e = t; e < nn; e += w.nthreads) w.ws.wr(w.off_th + w.ws_part(s3mh_g_part(p.bid, nn, e), nn));
        for (int e = t; e < inner; e += w.nthreads) {
            w.ws.wr(w.off_k0 + w.ws_part(s3mh_g_part(p.bid, inner, e), inner));
            w.ws.wr(w.off_v0 + w.ws_part(s3mh_g_part(p.bid, inner, e), inner));
        }
        return;
    }
    if (qvalid) {
        const size_t g = s3mh_g_tok(p.b, a.ntok, i, 3 * inner, h, c, a.DH), gd = s3mh_g_tok(p.b, a.ntok, i, inner, h, c, a.DH);
        w.q.rd(g, CH); w.tdO.rd(gd, CH);
        if (a.lo) { w.ql.rd(g, CH); w.tdOl.rd(gd, CH); }
    }
    scores_softmax(w, p, t, total);
    for (int item = t; item < nit; item += w.nthreads) {
        const int wq = item / a.J, j = item % a.J, iq = 1 + p.ry * a.W + p.w0 + wq;
        if (iq < a.ntok) {
            for (int hh = 0; hh < a.NH; ++hh) w.sp(s3mh_tab_item(item, hh, a.NH), total);
            for (int g = 0; g < a.NH; ++g) {
                for (int hh = 0; hh < S3MH_MH; ++hh) w.wsh_at(s3mh_wsh(g, hh));
                w.ws.wr(w.off_pm + w.ws_item(s3mh_g_ws(p.b, nq, iq - 1, a.J, j, a.NH, g)));
            }
        }
    }
    for (int e = t; e < s3mh_nsp(a.TW, a.J, a.NH); e += w.nthreads) w.dp(e);
    if (qvalid) {
        const size_t g = s3mh_g_k0(p.b, a.k0_bs, h, c, a.DH);
        w.v.rd(g, CH);
        if (a.lo) w.vl.rd(g, CH);
        if (c == 0) w.dp(s3mh_tab(wt, 0, h, a.J, a.NH));
    }
    sweep_taps(w, w.v, a.lo ? &w.vl : nullptr, p, t, total, [&](int j) { if (c == 0) w.dp(s3mh_tab(wt, j, h, a.J, a.NH)); });
    // dW_th partials
    for (int u = t; u < S3MH_NG * nn; u += w.nthreads) {
        const int grp = u / nn, pair = u - grp * nn, g = pair / a.NH, hh = pair - g * a.NH;
        CHECK(g < a.NH && hh < a.NH && grp < S3MH_NG, "unit %d", u);
        for (int item = grp; item < nit; item += S3MH_NG) { w.dp(s3mh_tab_item(item, g, a.NH)); w.sp(s3mh_tab_item(item, hh, a.NH), total); }
        w.red(s3mh_red(grp, pair, a.NH));
    }
    for (int pair = t; pair < nn; pair += w.nthreads) {
        for (int k = 0; k < S3MH_NG; ++k) w.red(s3mh_red(k, pair, a.NH));
        w.ws.wr(w.off_th + w.ws_part(s3mh_g_part(p.bid, nn, pair), nn));
    }
    for (int item = t; item < nit; item += w.nthreads) {
        for (int g = 0; g < a.NH; ++g) w.dp(s3mh_tab_item(item, g, a.NH));
        for (int hh = 0; hh < a.NH; ++hh) {
            for (int g = 0; g < S3MH_MH; ++g) w.wsh_at(s3mh_wsh(g, hh));
            w.dp(s3mh_tab_item(item, hh, a.NH));
        }
    }
    if (act)
        for (int j = c; j < a.J; j += 4) {
            const int idx = s3mh_tab(wt, j, h, a.J, a.NH);
            w.sp(idx, total); w.dp(idx);
            if (qvalid) w.ws.wr(w.ws_item(s3mh_g_ws(p.b, nq, i - 1, a.J, j, a.NH, h)));
        }
    if (qvalid) {
        const size_t g = s3mh_g_k0(p.b, a.k0_bs, h, c, a.DH);
        w.k.rd(g, CH);
        if (a.lo) w.kl.rd(g, CH);
        w.dp(s3mh_tab(wt, 0, h, a.J, a.NH));
        for (int hh = 0; hh < a.NH; ++hh) { w.wsh_at(s3mh_wsh(h, hh)); w.sp(s3mh_tab(wt, 0, hh, a.J, a.NH), total); }
    }
    sweep_taps(w, w.k, a.lo ? &w.kl : nullptr, p, t, total, [&](int j) { w.dp(s3mh_tab(wt, j, h, a.J, a.NH)); });
    if (qvalid) {
        const size_t g = s3mh_g_tok(p.b, a.ntok, i, 3 * inner, h, c, a.DH);
        w.dq.wr(g, CH);
        if (a.lo) w.dql.wr(g, CH);
    }
    for (int which = 0; which < 2; ++which) {
        if (act) for (int e = 0; e < CH; ++e) w.rk(s3mh_rk(wt, s3mh_col(h, c, a.DH) + e, inner));
        for (int e = t; e < inner; e += w.nthreads) {
            for (int ww = 0; ww < p.tw; ++ww) w.rk(s3mh_rk(ww, e, inner));
            w.ws.wr((which ? w.off_v0 : w.off_k0) + w.ws_part(s3mh_g_part(p.bid, inner, e), inner));
        }
    }
}

static void bwd_kv_thread(World& w, const TilePos& p, int t) {
    const Args& a = w.a;
    const int c = t & 3, wh = t >> 2, h = wh % a.NH, wt = wh / a.NH, CH = a.DH / 4, inner = a.NH * a.DH;
    const int wk = p.w0 + wt, ik = 1 + p.ry * a.W + wk, nq = a.ntok - 1;
    const bool act = wt < p.tw, kvalid = act && ik < a.ntok;
    const size_t total = w.lds_bkv;
    if (p.ry * a.W + p.w0 + 1 >= a.ntok) return;
    const int HS = s3mh_hs(a.SW, a.NH), c0 = s3mh_c0(a.NT, p.w0, (a.kw - 1 - a.ow) * a.dw);
    for (int tp = 0; tp < a.kf * a.kh; ++tp) {
        const int ta = tp / a.kh, tb = tp - ta * a.kh;
        const int fq = p.f + (a.of - ta) * a.df, yq = p.y + (a.oh - tb) * a.dh;
        if (!(fq >= 0 && yq >= 0 && fq < a.F && yq < a.H && (fq * a.H + yq) * a.W + 1 < a.ntok)) continue;
        const int pos0 = (fq * a.H + yq) * a.W;
        stage_cols(w, w.q, a.lo ? &w.ql : nullptr, (size_t)p.b * a.ntok + 1, pos0, c0, nq, 0, 1, t, total);
        stage_cols(w, w.tdO, a.lo ? &w.tdOl : nullptr, (size_t)p.b * a.ntok + 1, pos0, c0, nq, 2, 3, t, total);
        if (!kvalid) continue;
        for (int tc = 0; tc < a.kw; ++tc) {
            const int wq = wk + (a.ow - tc) * a.dw;
            if (wq < 0 || wq >= a.W) continue;
            const int pq = pos0 + wq;
            if (1 + pq >= a.ntok) continue;
            const int j = 1 + tp * a.kw + tc;
            CHECK(j >= 1 && j < a.J, "slot %d of %d", j, a.J);
            const size_t ci = w.ws_item(s3mh_g_ws(p.b, nq, pq, a.J, j, a.NH, h));
            w.ws.rd(ci); w.ws.rd(w.off_pm + ci);
            CHECK(wq - c0 >= 0 && wq - c0 < a.SW, "query column %d is staged column %d of %d", wq, wq - c0, a.SW);
            const int slot = s3mh_st_read(wq - c0, h, c, a.NH);
            for (int v8 = 0; v8 < CH / 8; ++v8) {
                w.stage8(0, slot + v8 * HS, total); w.stage8(2, slot + v8 * HS, total);
                if (a.lo) { w.stage8(1, slot + v8 * HS, total); w.stage8(3, slot + v8 * HS, total); }
            }
        }
    }
    if (kvalid) {
        const size_t g = s3mh_g_tok(p.b, a.ntok, ik, 3 * inner, h, c, a.DH);
        w.dk.wr(g, CH); w.dv.wr(g, CH);
        if (a.lo) { w.dkl.wr(g, CH); w.dvl.wr(g, CH); }
    }
}

static void expect_once(const Buf& b, const Tensor* t, size_t row0, size_t row_step, const char* what) {
    // every element of the tensor's columns in the rows row0, row0 + 1, ... of each block of row_step rows: written exactly once
    for (size_t r = 0; r < t->rows; ++r) {
        const bool want = (r % row_step) >= row0;
        for (int cidx = 0; cidx < t->cols; ++cidx) {
            const unsigned n = b.n[t->off + r * t->ld + cidx];
            CHECK(n == (want ? 1u : 0u), "%s: row %zu column %d written %u times", what, r, cidx, n);
        }
    }
}

static void walk_case(const int* f) {
    amdnuwa_s3_geom g;
    std::memset(&g, 0, sizeof g);
    g.B = f[0]; g.ntok = f[1]; g.F = f[2]; g.H = f[3]; g.W = f[4]; g.kf = f[5]; g.kh = f[6]; g.kw = f[7]; g.df = f[8]; g.dh = f[9]; g.dw = f[10];
    g.heads = f[11]; g.dim_head = f[12];
    const int lo = f[13], bias = f[14];
    CHECK(g.heads >= S3MH_MIN && g.heads <= S3MH_MH && (g.dim_head == 32 || g.dim_head == 64) && g.W >= 1 && g.W <= 64, "envelope");
    CHECK(g.ntok >= 1 && g.ntok - 1 <= g.F * g.H * g.W && g.B >= 1, "sequence");
    const S3mhTile tl = s3mh_tile(&g);
    Args a{};
    a.B = g.B; a.ntok = g.ntok; a.F = g.F; a.H = g.H; a.W = g.W; a.kf = g.kf; a.kh = g.kh; a.kw = g.kw; a.df = g.df; a.dh = g.dh; a.dw = g.dw;
    a.NH = g.heads; a.DH = g.dim_head; a.of = g.kf - 1; a.oh = g.kh - 1; a.ow = g.kw - 1;
    a.NT = tl.nt; a.TW = tl.tw; a.SW = tl.sw; a.J = (int)s3mh_slots(&g); a.lo = lo; a.bias = bias;
    a.k0_bs = (long long)g.ntok * 3 * g.heads * g.dim_head;
    World w(a, g);
    CHECK(w.nthreads >= 64 && w.nthreads <= 512 && w.nthreads % 64 == 0 && w.nthreads >= a.TW * a.NH * 4, "%d threads", w.nthreads);
    CHECK(a.NT * a.TW >= a.W && (a.NT - 1) * a.TW < a.W, "tiles %d x %d over %d columns", a.NT, a.TW, a.W);
    const size_t lds_max = 160 * 1024 - 2048, lds_need = s3mh_lds_need(&g, lo != 0);
    CHECK(lds_need <= lds_max, "LDS %zu", lds_need);
    w.lds.n.assign(lds_need, 0);
    const int nb = a.B * a.F * a.H * a.NT;
    std::vector<unsigned char> seen(nb, 0);
    for (int pass = 0; pass < 3; ++pass)
        for (int blk = 0; blk < nb; ++blk) {
            const int bid = xcd_row_id(blk, nb);
            CHECK(bid >= 0 && bid < nb, "workgroup id %d of %d", bid, nb);
            if (pass == 0) { CHECK(!seen[bid], "workgroup id %d twice", bid); seen[bid] = 1; }
            const TilePos p = tile_pos(a, bid);
            for (int t = 0; t < w.nthreads; ++t) {
                if (pass == 0) fwd_thread(w, p, t);
                else if (pass == 1) bwd_q_thread(w, p, t);
                else bwd_kv_thread(w, p, t);
            }
        }
    // written exactly once
    expect_once(w.o, &w.to, 0, 1, "o");
    expect_once(w.dqkv, &w.dq, 0, 1, "dq");
    expect_once(w.dqkv, &w.dk, 1, a.ntok, "dk");
    expect_once(w.dqkv, &w.dv, 1, a.ntok, "dv");
    if (lo) {
        expect_once(w.o_lo, &w.tol, 0, 1, "o_lo");
        expect_once(w.dqkv_lo, &w.dql, 0, 1, "dq_lo");
        expect_once(w.dqkv_lo, &w.dkl, 1, a.ntok, "dk_lo");
        expect_once(w.dqkv_lo, &w.dvl, 1, a.ntok, "dv_lo");
    }
    for (size_t e = 0; e < w.ws_floats; ++e) CHECK(w.ws.n[e] == 1, "workspace float %zu written %u times", e, (unsigned)w.ws.n[e]);
}

int main(int argc, char** argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s CASEFILE\n", argv[0]); return 2; }
    std::FILE* fp = std::fopen(argv[1], "r");
    if (!fp) { std::perror(argv[1]); return 2; }
    char line[512];
    int ncase = 0;
    while (std::fgets(line, sizeof line, fp)) {
        int f[15];
        if (std::sscanf(line, "%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", f, f + 1, f + 2, f + 3, f + 4, f + 5, f + 6, f + 7, f + 8, f + 9, f + 10, f + 11, f + 12,
                        f + 13, f + 14) != 15)
            continue;
        g_case = line;
        while (!g_case.empty() && (g_case.back() == '\n' || g_case.back() == ' ')) g_case.pop_back();
        walk_case(f);
        ++ncase;
    }
    std::fclose(fp);
    if (!ncase) { std::fprintf(stderr, "no case in %s\n", argv[1]); return 2; }
    std::printf("cases walked: %d, indices checked: %llu\n", ncase, g_checked);
    return 0;
}
