"""Case list of the many-head Sparse3DNA kernels (csrc/sparse3dna_mh.hip, 9 .. 16 heads) for tools/launch_log/run.py: the cases of
tests/test_gpu_s3_mh.py (tests/s3_mh_cases_util.py), forward and backward entry, with fake operand addresses.  The four host-side hooks the
entry points take from sparse3dna.hip (geometry fill, workspace bytes, <bos> slot / workspace binding, the tail of the backward) are stubs
here, so the unit compiles in seconds; the tail logs one `extern` line where the real one launches s3_bwd_fin_kernel and the column sums.

    python tools/launch_log/run.py --tree . --cases s3_mh -o LOG

prints, per kernel instantiation of the file, how many launches the case list makes, and `never launched: none`."""
import ctypes
import os
import sys

SOURCE = 'sparse3dna_mh.hip'

STUBS = r'''
#include "launch_log.h"
#include "common.h"
#include "s3_args.h"
int g_amdnuwa_tuning[32];
size_t s3_ws_bytes(const amdnuwa_s3_geom* g) {          // the s3_ws() map of sparse3dna.hip
    const size_t nq = g->ntok - 1, J = s3_slots(g), items = (size_t)g->B * nq * J * g->heads;
    const size_t parts = (size_t)g->B * g->F * g->H * s3_tile(g).nt, inner = (size_t)g->heads * g->dim_head;
    const long long R = (long long)g->B * nq;
    return (2 * items + parts * g->heads * g->heads + 2 * parts * inner) * sizeof(float) + 256 + (size_t)(R < 256 ? (R < 1 ? 1 : R) : 256) * J * g->heads * sizeof(float);
}
void s3_fill_causal(S3Args& a, const amdnuwa_s3_geom* g) {
    a.B = g->B; a.ntok = g->ntok; a.F = g->F; a.H = g->H; a.W = g->W; a.kf = g->kf; a.kh = g->kh; a.kw = g->kw;
    a.df = g->df; a.dh = g->dh; a.dw = g->dw; a.NH = g->heads; a.scale = g->scale; a.bias = g->rel_bias;
    a.of = g->kf - 1; a.oh = g->kh - 1; a.ow = g->kw - 1; a.FK = g->F; a.kvrows = g->ntok; a.kvoff = 1;
    const S3Tile tl = s3_tile(g);
    a.NT = tl.nt; a.TW = tl.tw; a.SW = tl.sw;
}
void s3_bind_self(S3Args&, const amdnuwa_s3_geom*, void*) {}
int s3_bwd_tail(const S3Args&, const amdnuwa_s3_geom* g, void*, hipStream_t) {
    char buf[96];
    snprintf(buf, sizeof buf, "extern s3_bwd_tail d_rel_bias %d\n", g->d_rel_bias ? 1 : 0);
    launch_log::lines() += buf;
    return 0;
}
'''

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
import s3_mh_cases_util as M                                 # noqa: E402

FAKE = 0x10000000
SG = None


def declare(L):
    from nuwa_pytorch_amd import _lib
    for name in ('amdnuwa_s3mh_supported', 'amdnuwa_sparse3dna_mh_bwd_workspace_bytes', 'amdnuwa_sparse3dna_mh_fwd', 'amdnuwa_sparse3dna_mh_bwd'):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return _lib.S3Geom


def call(L, S3Geom, c, entry):
    """one call of `entry` ('fwd' / 'bwd') with fake, distinct, 256-byte aligned operand addresses"""
    lo = c['form'] == 'hilo'
    inner = c['heads'] * c['dim_head']
    addr = iter(range(FAKE, FAKE + (1 << 20), 256))
    p = lambda: next(addr)
    plo = lambda: next(addr) if lo else None
    bias = p() if c['bias'] else None
    if entry == 'fwd':
        g = M.geom(S3Geom, c, rel_bias=bias)
        return L.amdnuwa_sparse3dna_mh_fwd(ctypes.byref(g), p(), p(), p(), plo(), plo(), plo(), 3 * inner, p(), p(), plo(), inner, None)
    g = M.geom(S3Geom, c, rel_bias=bias, d_rel_bias=p() if c['bias'] else None)
    nb = L.amdnuwa_sparse3dna_mh_bwd_workspace_bytes(ctypes.byref(g))
    return L.amdnuwa_sparse3dna_mh_bwd(ctypes.byref(g), p(), p(), p(), plo(), plo(), plo(), 3 * inner, p(), p(), plo(), inner,
                                       p(), p(), p(), plo(), plo(), plo(), 3 * inner, p(), 0, p(), nb, None)


def cases(L):
    """one item per (case, entry point): the launch log is taken after every call"""
    S3Geom = declare(L)
    for c in M.all_cases():
        for entry in ('fwd', 'bwd'):
            yield f"{c['name']} :: {entry}", {}, (lambda c=c, entry=entry: call(L, S3Geom, c, entry))
