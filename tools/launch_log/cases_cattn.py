"""Case list of the linear-memory attention entry points (cattn.hip) for tools/launch_log/run.py: amdnuwa_cattn_fwd / _fwd_drop and
amdnuwa_cattn_bwd / _bwd_drop, causal and not, on own and foreign keys, both head widths, fp16 and bf16 rows, every output form, with the
mask arguments of the dropout entries on both sides of each rule.  The column sums of elementwise.hip are stubs that log their call (operand
offsets inside the workspace included), so the log also pins the workspace layout."""
import ctypes as C

SOURCE = 'cattn.hip'

STUBS = r'''
#include "launch_log.h"
int g_amdnuwa_tuning[32];
extern "C" size_t amdnuwa_colsum_workspace_bytes(long long R, int D) {
    char buf[96];
    snprintf(buf, sizeof buf, "extern amdnuwa_colsum_workspace_bytes R %lld D %d\n", R, D);
    launch_log::lines() += buf;
    return (size_t)(R < 256 ? (R < 1 ? 1 : R) : 256) * D * sizeof(float);
}
extern "C" int amdnuwa_colsum(const float* x, float* out, long long R, int D, int accumulate, void* workspace, size_t workspace_bytes, hipStream_t) {
    char buf[192];
    snprintf(buf, sizeof buf, "extern amdnuwa_colsum x %p out %p R %lld D %d accumulate %d workspace %p bytes %zu\n", (const void*)x, (void*)out, R, D,
             accumulate, workspace, workspace_bytes);
    launch_log::lines() += buf;
    return 0;
}
'''

P, I, F, SZ = C.c_void_p, C.c_int, C.c_float, C.c_size_t


class CGeom(C.Structure):                   # amdnuwa_cattn_geom of include/amdnuwa.h
    _fields_ = [('B', I), ('n', I), ('heads', I), ('dim_head', I), ('scale', F), ('causal', I), ('n_keys', I)]


# fake operand addresses: fixed, distinct, 16-byte aligned, never dereferenced
(Q, K, V, MASK, NK, NV, WTH, O, OLO, STATS, DO, DQ, DK, DV, DWTH, DNK, DNV, WS, KEEP, KEEPT, KEEP0) = (0x10000000 + 0x01000000 * i for i in range(21))

BS, NS = (0, 1, 3), (0, 1, 31, 32, 33, 63, 64, 65, 2560)
INF, NAN = float('inf'), float('nan')
# (keep, keep_t, keep0, drop_scale): the accepted masks, then each rule of check_mask broken in turn
MASKS = ([(KEEP, KEEPT, KEEP0, s) for s in (1.0, 2.0, 0.5, INF, NAN, 3.0e38)] +
         [(KEEP + 1, KEEPT, KEEP0, 2.0), (KEEP, KEEPT + 2, KEEP0, 2.0), (KEEP, KEEPT, KEEP0 + 3, 2.0), (KEEP + 4, KEEPT + 8, KEEP0 + 12, 2.0),
          (None, KEEPT, KEEP0, 2.0), (KEEP, None, KEEP0, 2.0), (KEEP, KEEPT, None, 2.0)])


def cases(L):
    L.amdnuwa_cattn_bwd_workspace_bytes.restype, L.amdnuwa_cattn_bwd_workspace_bytes.argtypes = SZ, [P]
    fwd_t = [P, P, I, P, P, I, P, P, P, P, P, P, I, I, P, I]
    bwd_t = [P, P, I, P, P, I, P, I, P, P, P, P, P, P, I, P, P, I, P, P, P, P, SZ]
    L.amdnuwa_cattn_fwd.argtypes = fwd_t + [P]
    L.amdnuwa_cattn_fwd_drop.argtypes = fwd_t + [P, P, F, P]
    L.amdnuwa_cattn_bwd.argtypes = bwd_t + [P]
    L.amdnuwa_cattn_bwd_drop.argtypes = bwd_t + [P, P, P, F, P]
    for heads in (1, 5, 8):
        for dh in (32, 64):
            inner = heads * dh
            for B in BS:
                for n in NS:
                    for causal, nk in ((1, 0), (1, n), (1, 40), (0, 0), (0, n), (0, 40), (0, 2560), (0, -1)):
                        g = CGeom(B, n, heads, dh, dh ** -0.5, causal, nk)
                        tag = f'B {B} n {n} heads {heads} dh {dh} causal {causal} n_keys {nk}'
                        nb = L.amdnuwa_cattn_bwd_workspace_bytes(C.byref(g))
                        L.launch_log_take(None, 0)          # (the query's own stub lines belong to no case)
                        quick = not (B == 3 and n in (1, 33, 64, 2560))            # the full set of forms on a few shapes, a short one on the rest
                        for f16 in (0, 1):
                            for o, olo, of16 in ((O, OLO, 0),) if quick else ((O, None, 0), (O, OLO, 0), (O, OLO, 1), (None, OLO, 1), (None, OLO, 0)):
                                for mask in (None,) if quick else (None, MASK):
                                    a = (C.byref(g), Q, inner, K, V, 2 * inner, mask, NK, NV, WTH, o, olo, inner, of16, STATS, f16)
                                    yield (f'fwd f16 {f16} o {o is not None} o_lo {olo is not None} o_lo_f16 {of16} key mask {mask is not None} {tag}', {},
                                           lambda a=a: L.amdnuwa_cattn_fwd(*a, None))
                                    for kp, _, k0, s in MASKS[:1] if quick else MASKS:
                                        yield (f'fwd_drop keep {kp} keep0 {k0} s {s} f16 {f16} o {o is not None} o_lo {olo is not None} o_lo_f16 {of16} '
                                               f'key mask {mask is not None} {tag}', {}, lambda a=a, kp=kp, k0=k0, s=s: L.amdnuwa_cattn_fwd_drop(*a, kp, k0, s, None))
                        for mask in (None,) if quick else (None, MASK):
                            a = (C.byref(g), Q, inner, K, V, 2 * inner, DO, inner, mask, NK, NV, WTH, STATS, DQ, inner, DK, DV, 2 * inner, DWTH, DNK, DNV, WS)
                            yield f'bwd key mask {mask is not None} {tag}', {}, lambda a=a, nb=nb: L.amdnuwa_cattn_bwd(*a, nb, None)
                            for kp, kt, k0, s in MASKS[:1] if quick else MASKS:
                                yield (f'bwd_drop keep {kp} keep_t {kt} keep0 {k0} s {s} key mask {mask is not None} {tag}', {},
                                       lambda a=a, nb=nb, kp=kp, kt=kt, k0=k0, s=s: L.amdnuwa_cattn_bwd_drop(*a, nb, kp, kt, k0, s, None))
                        if nb and not quick:
                            yield f'bwd short workspace {tag}', {}, lambda a=a, nb=nb: L.amdnuwa_cattn_bwd(*a, nb - 1, None)
    # leading dimensions below the row width and off their alignment, unsupported head counts and widths
    g = CGeom(3, 64, 8, 64, 0.125, 1, 0)
    nb = L.amdnuwa_cattn_bwd_workspace_bytes(C.byref(g))
    L.launch_log_take(None, 0)
    for ldq, ldkv, ldo in ((504, 1024, 512), (512, 504, 512), (512, 1024, 508), (516, 1024, 512), (512, 1028, 512), (512, 1024, 514), (520, 1032, 516)):
        yield (f'fwd ldq {ldq} ldkv {ldkv} ldo {ldo}', {},
               lambda ldq=ldq, ldkv=ldkv, ldo=ldo: L.amdnuwa_cattn_fwd(C.byref(g), Q, ldq, K, V, ldkv, None, NK, NV, WTH, O, OLO, ldo, 0, STATS, 0, None))
        yield (f'bwd ldq {ldq} ldkv {ldkv} lddq {ldo}', {},
               lambda ldq=ldq, ldkv=ldkv, ldo=ldo: L.amdnuwa_cattn_bwd(C.byref(g), Q, ldq, K, V, ldkv, DO, ldq, None, NK, NV, WTH, STATS, DQ, ldo, DK, DV, ldkv,
                                                                        DWTH, DNK, DNV, WS, nb, None))
    for heads, dh in ((0, 64), (9, 64), (8, 48), (8, 128)):
        gb = CGeom(3, 64, heads, dh, 0.125, 1, 0)
        yield (f'fwd heads {heads} dh {dh}', {},
               lambda gb=gb: L.amdnuwa_cattn_fwd(C.byref(gb), Q, 512, K, V, 1024, None, NK, NV, WTH, O, OLO, 512, 0, STATS, 0, None))
