"""Case list of the third-design cross-attention entry points (xattn6.hip) for tools/launch_log/run.py: amdnuwa_xattn6_pack and _fwd in bf16 and
fp16 with every accepted (and rejected) output form, on work-item counts below, at and above the CU count the file falls back to without a
device (256: both grid branches); amdnuwa_xattn6_pack_bwd / _f16 and _bwd / _bwd_f16 with JP from amdnuwa_xattn_jp and with wrong ones."""
import ctypes as C

SOURCE = 'xattn6.hip'

STUBS = r'''
int g_amdnuwa_tuning[32];
'''

P, I, F, SZ = C.c_void_p, C.c_int, C.c_float, C.c_size_t


class XGeom(C.Structure):                   # amdnuwa_xattn_geom of include/amdnuwa.h
    _fields_ = [('B', I), ('n', I), ('T', I), ('JP', I), ('heads', I), ('dim_head', I), ('scale', F)]


class X6KV(C.Structure):                    # amdnuwa_xattn6_kv
    _fields_ = [('K6', P), ('V6', P), ('vbits', P)]


# fake operand addresses: fixed, distinct, 16-byte aligned, never dereferenced
(KV16, MASK, K6, V6, VBITS, Q16, NK, NV, WTH, O, OLO, STATS, DO, DS, PM, DQ, PART) = (0x10000000 + 0x01000000 * i for i in range(17))

# (B, n): the small batches over the query counts around the 64-row tile, then B x tiles = 255, 256, 257, 256 again and far above
BN = [(B, n) for B in (0, 1, 3) for n in (0, 1, 31, 32, 33, 63, 64, 65, 2560)] + [(255, 64), (256, 64), (257, 64), (128, 128), (128, 2560)]
TS = (1, 64, 65, 256, 2048, 2049)


def jp(T):
    return ((T + 1 + 31) // 32) * 32


def geom(B, n, T, JP=None, heads=8, dh=64):
    return XGeom(B, n, T, jp(T) if JP is None else JP, heads, dh, dh ** -0.5)


def cases(L):
    L.amdnuwa_xattn6_bwd_workspace_bytes.restype, L.amdnuwa_xattn6_bwd_workspace_bytes.argtypes = SZ, [P]
    L.amdnuwa_xattn6_pack.argtypes = [P, P, I, P, I, P, P]
    L.amdnuwa_xattn6_fwd.argtypes = [P, P, I, P, P, P, P, P, P, I, I, P, I, P]
    for fn in (L.amdnuwa_xattn6_pack_bwd, L.amdnuwa_xattn6_pack_bwd_f16):
        fn.argtypes = [P, P, I, P, P, P, P, P]
    for fn in (L.amdnuwa_xattn6_bwd, L.amdnuwa_xattn6_bwd_f16):
        fn.argtypes = [P, P, I, P, I, P, P, P, P, P, P, P, P, I, P, SZ, P]
    kv = X6KV(K6, V6, VBITS)
    shapes = [(B, n, T, None, 8, 64) for T in TS for B, n in BN] + [(3, 64, 256, None, 5, 64), (3, 64, 256, None, 8, 32)]
    for B, n, T, JP, heads, dh in shapes:
        g = geom(B, n, T, JP, heads, dh)
        tag = f'B {B} n {n} T {T} heads {heads} dh {dh}'
        for f16 in (0, 1):
            if n == 64 or B == 3:
                for mask in (None, MASK):
                    yield (f'pack f16 {f16} mask {mask is not None} {tag}', {},
                           lambda g=g, f16=f16, mask=mask: L.amdnuwa_xattn6_pack(C.byref(g), KV16, 1024, mask, f16, C.byref(kv), None))
            for o, olo, of16 in ((O, None, 0), (O, OLO, 0), (O, OLO, 1), (None, OLO, 1), (O, None, 1), (None, OLO, 0), (None, None, 0)):
                for stats in (STATS, None):
                    yield (f'fwd f16 {f16} o {o is not None} o_lo {olo is not None} o_lo_f16 {of16} stats {stats is not None} {tag}', {},
                           lambda g=g, f16=f16, o=o, olo=olo, of16=of16, stats=stats:
                           L.amdnuwa_xattn6_fwd(C.byref(g), Q16, 512, C.byref(kv), NK, NV, WTH, o, olo, 512, of16, stats, f16, None))
    # the backward: JP as amdnuwa_xattn_jp gives it, then one chunk more, one chunk short, not a multiple of 32
    for T in (1, 30, 31, 64, 65, 256, 2015, 2016):
        for JP in (jp(T), jp(T) + 32, jp(T) - 32, jp(T) + 8):
            for B, n in BN:
                if JP != jp(T) and not (B == 3 and n in (0, 64)):
                    continue
                g = geom(B, n, T, JP)
                tag = f'B {B} n {n} T {T} JP {JP}'
                nb = L.amdnuwa_xattn6_bwd_workspace_bytes(C.byref(g))
                for f16, pack, bwd in ((0, L.amdnuwa_xattn6_pack_bwd, L.amdnuwa_xattn6_bwd), (1, L.amdnuwa_xattn6_pack_bwd_f16, L.amdnuwa_xattn6_bwd_f16)):
                    if n == 64 or B == 3:
                        for mask in (None, MASK):
                            yield (f'pack_bwd f16 {f16} mask {mask is not None} {tag}', {},
                                   lambda g=g, pack=pack, mask=mask: pack(C.byref(g), KV16, 1024, NK, NV, mask, C.byref(kv), None))
                    yield (f'bwd f16 {f16} {tag}', {},
                           lambda g=g, bwd=bwd, nb=nb: bwd(C.byref(g), Q16, 512, DO, 512, C.byref(kv), NK, NV, WTH, STATS, DS, PM, DQ, 512, PART, nb, None))
                    if nb:
                        yield (f'bwd f16 {f16} short workspace {tag}', {},
                               lambda g=g, bwd=bwd, nb=nb: bwd(C.byref(g), Q16, 512, DO, 512, C.byref(kv), NK, NV, WTH, STATS, DS, PM, DQ, 512, PART, nb - 1, None))
