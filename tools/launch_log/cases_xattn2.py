"""Case list of the second-design cross-attention entry points (xattn2.hip) for tools/launch_log/run.py: amdnuwa_xattn2_fwd, _fwd_f16 in every
output form, _bwd / _bwd_ex with both dS / Pm layouts and the recomputing _bwd_rc, over batch sizes, query counts around the 32- and 64-row
tiles and text lengths up to (and past) the 288-key limit."""
import ctypes as C

SOURCE = 'xattn2.hip'

STUBS = r'''
int g_amdnuwa_tuning[32];
'''

P, I, F, SZ = C.c_void_p, C.c_int, C.c_float, C.c_size_t


class XGeom(C.Structure):                   # amdnuwa_xattn_geom of include/amdnuwa.h
    _fields_ = [('B', I), ('n', I), ('T', I), ('JP', I), ('heads', I), ('dim_head', I), ('scale', F)]


class XKV(C.Structure):                     # amdnuwa_xattn_kv
    _fields_ = [('Kp', P), ('Kp_lo', P), ('Kt', P), ('Kt_lo', P), ('Vp', P), ('Vp_lo', P), ('Vt', P), ('Vt_lo', P), ('valid', P)]


# fake operand addresses: fixed, distinct, 16-byte aligned, never dereferenced
(KP, KPL, KT, KTL, VP, VPL, VT, VTL, VALID, Q, Q16, WTH, O, OLO, STATS, DO, DS, PM, DQ, PART, NBD, DKP, DVP) = (0x10000000 + 0x01000000 * i for i in range(23))

BS, NS = (0, 1, 3), (0, 1, 31, 32, 33, 63, 64, 65, 2560)
TS = (1, 30, 31, 255, 256, 287, 288)


def geom(B, n, T, heads=8, dh=64, JP=None):
    return XGeom(B, n, T, ((T + 1 + 31) // 32) * 32 if JP is None else JP, heads, dh, dh ** -0.5)


def images(form):
    full = dict(Kp=KP, Kp_lo=KPL, Kt=KT, Kt_lo=KTL, Vp=VP, Vp_lo=VPL, Vt=VT, Vt_lo=VTL)
    pick = {'hi+lo': full, 'hi': {k: v for k, v in full.items() if not k.endswith('_lo')}, 'lean': dict(Kp=KP, Kp_lo=KPL, Vp=VP, Vt_lo=VTL),
            'lean bwd': dict(Kp=KP, Vp=VP)}[form]
    return XKV(valid=VALID, **pick)


def cases(L):
    for name in ('amdnuwa_xattn2_bwd_workspace_bytes', 'amdnuwa_xattn2_bwd_rc_stats_bytes'):
        getattr(L, name).restype, getattr(L, name).argtypes = SZ, [P]
    L.amdnuwa_xattn2_fwd.argtypes = [P, P, I, P, P, P, I, P, P]
    L.amdnuwa_xattn2_fwd_f16.argtypes = [P, P, I, P, P, P, P, I, I, P, P]
    L.amdnuwa_xattn2_bwd.argtypes = [P, P, I, P, I, P, P, P, P, P, P, I, P, SZ, P]
    L.amdnuwa_xattn2_bwd_ex.argtypes = [P, P, I, P, I, P, P, P, P, P, P, I, P, SZ, I, P]
    L.amdnuwa_xattn2_bwd_rc.argtypes = [P, P, I, P, I, P, P, P, P, I, P, SZ, P, SZ, P, P, P]
    shapes = [(B, n, T, 8, 64, None) for T in TS for B in BS for n in NS]
    shapes += [(3, 64, 256, 5, 64, None), (3, 64, 256, 8, 32, None), (3, 64, 40, 8, 64, 32), (3, 64, 40, 8, 64, 96), (3, 64, 40, 8, 64, 72)]
    for B, n, T, heads, dh, JP in shapes:
        g = geom(B, n, T, heads, dh, JP)
        tag = f'B {B} n {n} T {T} heads {heads} dh {dh} JP {g.JP}'
        for form in ('hi', 'hi+lo', 'lean bwd'):
            p = images(form)
            for stats in (None, STATS):
                yield (f'fwd images {form} stats {stats is not None} {tag}', {},
                       lambda g=g, p=p, stats=stats: L.amdnuwa_xattn2_fwd(C.byref(g), Q, 512, C.byref(p), WTH, O, 512, stats, None))
        for form in ('hi+lo', 'lean', 'hi'):
            p = images(form)
            for olo, of16 in ((OLO, 0), (OLO, 1), (None, 0), (None, 1)):
                yield (f'fwd_f16 images {form} o_lo {olo is not None} o_lo_f16 {of16} {tag}', {},
                       lambda g=g, p=p, olo=olo, of16=of16: L.amdnuwa_xattn2_fwd_f16(C.byref(g), Q16, 512, C.byref(p), WTH, O, olo, 512, of16, STATS, None))
        nb = L.amdnuwa_xattn2_bwd_workspace_bytes(C.byref(g))
        sb = L.amdnuwa_xattn2_bwd_rc_stats_bytes(C.byref(g))
        for form in ('hi', 'lean bwd'):
            p = images(form)
            yield (f'bwd images {form} {tag}', {},
                   lambda g=g, p=p, nb=nb: L.amdnuwa_xattn2_bwd(C.byref(g), Q, 512, DO, 512, C.byref(p), WTH, STATS, DS, PM, DQ, 512, PART, nb, None))
            for flags in (0, 1, 2, 3):
                yield (f'bwd_ex flags {flags} images {form} {tag}', {},
                       lambda g=g, p=p, nb=nb, flags=flags:
                       L.amdnuwa_xattn2_bwd_ex(C.byref(g), Q, 512, DO, 512, C.byref(p), WTH, STATS, DS, PM, DQ, 512, PART, nb, flags, None))
            yield (f'bwd_rc images {form} {tag}', {},
                   lambda g=g, p=p, nb=nb, sb=sb:
                   L.amdnuwa_xattn2_bwd_rc(C.byref(g), Q, 512, DO, 512, C.byref(p), WTH, STATS, DQ, 512, PART, nb, NBD, sb, DKP, DVP, None))
        if nb:
            p = images('hi')
            yield (f'bwd short workspace {tag}', {},
                   lambda g=g, p=p, nb=nb: L.amdnuwa_xattn2_bwd(C.byref(g), Q, 512, DO, 512, C.byref(p), WTH, STATS, DS, PM, DQ, 512, PART, nb - 1, None))
        if sb:
            p = images('hi')
            yield (f'bwd_rc short statistics {tag}', {},
                   lambda g=g, p=p, nb=nb, sb=sb:
                   L.amdnuwa_xattn2_bwd_rc(C.byref(g), Q, 512, DO, 512, C.byref(p), WTH, STATS, DQ, 512, PART, nb, NBD, sb - 1, DKP, DVP, None))
