"""Case list of the first-design cross-attention entry points (xattn.hip) for tools/launch_log/run.py: amdnuwa_xattn_pack / _pack_f16 over the
image sets the wrappers of kernels.py ask for, amdnuwa_xattn_fwd / _fwd_stats and amdnuwa_xattn_bwd in bf16 and hi + lo form with tuning key 5
both ways, amdnuwa_xattn_unpack in every accumulate form -- over head counts, both head widths and text lengths up to (and one past) the limit."""
import ctypes as C

SOURCE = 'xattn.hip'

STUBS = r'''
int g_amdnuwa_tuning[32];
'''

P, I, F = C.c_void_p, C.c_int, C.c_float


class XGeom(C.Structure):                   # amdnuwa_xattn_geom of include/amdnuwa.h
    _fields_ = [('B', I), ('n', I), ('T', I), ('JP', I), ('heads', I), ('dim_head', I), ('scale', F)]


class XKV(C.Structure):                     # amdnuwa_xattn_kv
    _fields_ = [('Kp', P), ('Kp_lo', P), ('Kt', P), ('Kt_lo', P), ('Vp', P), ('Vp_lo', P), ('Vt', P), ('Vt_lo', P), ('valid', P)]


# fake operand addresses: fixed, distinct, 16-byte aligned, never dereferenced
(KV, KVLO, NK, NV, MASK, KP, KPL, KT, KTL, VP, VPL, VT, VTL, VALID, Q, QLO, WTH, O, OLO, PP, PPL, PM, PML, STATS, DO, DOLO, DS, DSL, DQ, DQL,
 DWTH, WS, DKP, DVP, DKV, DKVLO, DNK, DNV) = (0x10000000 + 0x01000000 * i for i in range(38))

BS, NS = (0, 1, 3), (0, 1, 31, 32, 33, 63, 64, 65, 2560)
TS = (1, 30, 31, 255, 256, 287, 288)        # 287: the largest text check() takes (T + 1 <= 288)


def geom(B, n, T, heads, dh, JP=None):
    return XGeom(B, n, T, ((T + 1 + 31) // 32) * 32 if JP is None else JP, heads, dh, dh ** -0.5)


def images(form):
    """the image sets of PackedKV: all eight, the hi four, the lean sets of the fp16 forward and of the recomputing backward, none"""
    full = dict(Kp=KP, Kp_lo=KPL, Kt=KT, Kt_lo=KTL, Vp=VP, Vp_lo=VPL, Vt=VT, Vt_lo=VTL)
    pick = {'hi+lo': full, 'hi': {k: v for k, v in full.items() if not k.endswith('_lo')}, 'lean': dict(Kp=KP, Kp_lo=KPL, Vp=VP, Vt_lo=VTL),
            'lean bwd': dict(Kp=KP, Vp=VP), 'none': {}}[form]
    return XKV(valid=VALID, **pick)


def cases(L):
    L.amdnuwa_xattn_bwd_workspace_bytes.restype = C.c_size_t
    L.amdnuwa_xattn_bwd_workspace_bytes.argtypes = [P]
    for fn in (L.amdnuwa_xattn_pack, L.amdnuwa_xattn_pack_f16):
        fn.argtypes = [P, P, P, I, P, P, P, P, P]
    L.amdnuwa_xattn_fwd.argtypes = [P, P, P, I, P, P, P, P, I, P, P, P, P, P]
    L.amdnuwa_xattn_fwd_stats.argtypes = [P, P, P, I, P, P, P, P, I, P, P, P, P, P, P]
    L.amdnuwa_xattn_bwd.argtypes = [P, P, P, I, P, P, P, P, P, P, P, P, I, P, I, P, C.c_size_t, P]
    L.amdnuwa_xattn_unpack.argtypes = [P, P, P, P, P, I, P, P, I, P]
    for heads in (1, 5, 8):
        for dh in (32, 64):
            inner = heads * dh
            for T in TS:
                for B in BS:
                    g = geom(B, 64, T, heads, dh)
                    tag = f'B {B} T {T} heads {heads} dh {dh}'
                    for form, lo, mask in (('hi+lo', KVLO, MASK), ('hi', None, MASK), ('hi', None, None), ('lean bwd', None, MASK), ('hi+lo', None, MASK), ('none', None, MASK)):
                        p = images(form)
                        yield (f'pack {form} lo {lo is not None} mask {mask is not None} {tag}', {},
                               lambda g=g, p=p, lo=lo, mask=mask: L.amdnuwa_xattn_pack(C.byref(g), KV, lo, 2 * inner, NK, NV, mask, C.byref(p), None))
                    for form, f16 in (('hi+lo', KVLO), ('lean', KVLO), ('lean', None)):
                        p = images(form)
                        yield (f'pack_f16 {form} f16 {f16 is not None} {tag}', {},
                               lambda g=g, p=p, f16=f16: L.amdnuwa_xattn_pack_f16(C.byref(g), KV, f16, 2 * inner, NK, NV, MASK, C.byref(p), None))
                    for acc in range(8):
                        for lo in (None, DKVLO):
                            yield (f'unpack accumulate {acc} lo {lo is not None} {tag}', {},
                                   lambda g=g, acc=acc, lo=lo: L.amdnuwa_xattn_unpack(C.byref(g), DKP, DVP, DKV, lo, 2 * inner, DNK, DNV, acc, None))
                    for n in NS:
                        g = geom(B, n, T, heads, dh)
                        nb = L.amdnuwa_xattn_bwd_workspace_bytes(C.byref(g))
                        for x3 in (0, 1):
                            p = images('hi+lo' if x3 else 'hi')
                            ql, ol, pl, pml, dol, dsl, dql = (QLO, OLO, PPL, PML, DOLO, DSL, DQL) if x3 else (None,) * 7
                            for key5 in (0, 1):
                                keys = {5: 1} if key5 else {}
                                for stats in (None, STATS):
                                    yield (f"fwd_stats {'hi+lo' if x3 else 'bf16'} stats {stats is not None} n {n} {tag}", keys,
                                           lambda g=g, p=p, ql=ql, ol=ol, pl=pl, pml=pml, stats=stats:
                                           L.amdnuwa_xattn_fwd_stats(C.byref(g), Q, ql, inner, C.byref(p), WTH, O, ol, inner, PP, pl, PM, pml, stats, None))
                                yield (f"bwd {'hi+lo' if x3 else 'bf16'} n {n} {tag}", keys,
                                       lambda g=g, p=p, dol=dol, dsl=dsl, dql=dql, nb=nb:
                                       L.amdnuwa_xattn_bwd(C.byref(g), DO, dol, inner, C.byref(p), WTH, PP, PPL if dol else None, DS, dsl, DQ, dql, inner, DWTH, 1, WS, nb, None))
                            yield (f"fwd {'hi+lo' if x3 else 'bf16'} no saved P n {n} {tag}", {},
                                   lambda g=g, p=p, ql=ql, ol=ol: L.amdnuwa_xattn_fwd(C.byref(g), Q, ql, inner, C.byref(p), WTH, O, ol, inner, None, None, None, None, None))
    # a hi + lo call on images without the lo parts, a wrong JP, a short workspace
    g = geom(3, 64, 256, 8, 64)
    yield 'fwd_stats hi+lo on hi images', {}, lambda: L.amdnuwa_xattn_fwd_stats(C.byref(g), Q, QLO, 512, C.byref(images('hi')), WTH, O, OLO, 512, PP, PPL, PM, PML, None, None)
    gj = geom(3, 64, 256, 8, 64, JP=320)
    yield 'fwd_stats wrong JP', {}, lambda: L.amdnuwa_xattn_fwd_stats(C.byref(gj), Q, None, 512, C.byref(images('hi')), WTH, O, None, 512, PP, None, PM, None, None, None)
    nb = L.amdnuwa_xattn_bwd_workspace_bytes(C.byref(g))
    yield 'bwd short workspace', {}, lambda: L.amdnuwa_xattn_bwd(C.byref(g), DO, None, 512, C.byref(images('hi')), WTH, PP, None, DS, None, DQ, None, 512, DWTH, 0, WS, nb - 1, None)
