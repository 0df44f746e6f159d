"""What the dense-attention entry points of libamdnuwa (xattn.hip, xattn2.hip, xattn6.hip, cattn.hip) answer without launching anything,
pinned as literal tables.

Return codes: every case here returns before a launch -- it carries an error, or has B <= 0 (n <= 0 where the entry point has queries) --
so the tables run through ctypes without a device and the operand pointers are never dereferenced.  Per entry point: no geometry; the
geometries the family refuses (heads, dim_head, T, JP), each without rows (n = 0, or B = 0 where the entry point takes no n) so that an
accepted one returns OK instead of launching; every pointer argument and every image pointer NULL in turn, once at B = 3, n = 64 where the
required ones are errors, once without rows where the optional ones return OK; the leading-dimension rules; a short workspace; B <= 0 and
n <= 0 with and without a later error; the mask rules of the cattn _drop entries.  The order of the checks shows in the codes.

Queries: amdnuwa_xattn_jp, amdnuwa_xattn6_nch and every _supported, _image_bytes, _workspace_bytes and _stats_bytes query of the four files
over grids of geometries on both sides of each limit; one value per (query, geometry), runs of equal values written once.

The expected columns were recorded from the library of the commit BEFORE the host code of the four files was folded into one argument
builder and one launcher per family, and the tables passed there unchanged: they pin the behaviour that commit had."""
import ctypes

import pytest

OK, ARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
PTR = 4096                                        # a non-null, 16-byte aligned address that is never dereferenced
INF, NAN = float('inf'), float('nan')

INTS = {'accumulate': 0, 'flags': 1, 'f16': 1, 'o_lo_f16': 1}
SIZES = ('workspace_bytes', 'part_bytes', 'nbd_bytes')
# entry -> (parameters without the stream, the query of each size parameter, does a call with n <= 0 return before the launch?)
ENTRIES = {
    'amdnuwa_xattn_pack': ('xg kv kv_lo ldkv null_k null_v context_mask xkv', {}, False),
    'amdnuwa_xattn_pack_f16': ('xg kv kv_f16 ldkv null_k null_v context_mask xkv', {}, False),
    'amdnuwa_xattn_fwd': ('xg q q_lo ldq xkv w_th o o_lo ldo P P_lo Pm Pm_lo', {}, True),
    'amdnuwa_xattn_fwd_stats': ('xg q q_lo ldq xkv w_th o o_lo ldo P P_lo Pm Pm_lo stats', {}, True),
    'amdnuwa_xattn_bwd': ('xg dO dO_lo lddo xkv w_th P P_lo dS dS_lo dq dq_lo lddq dw_th accumulate workspace workspace_bytes',
                          {'workspace_bytes': 'amdnuwa_xattn_bwd_workspace_bytes'}, True),
    'amdnuwa_xattn_unpack': ('xg dKp dVp dkv dkv_lo ldkv dnull_k dnull_v accumulate', {}, False),
    'amdnuwa_xattn2_fwd': ('xg q ldq xkv w_th o ldo stats', {}, True),
    'amdnuwa_xattn2_fwd_f16': ('xg q_f16 ldq xkv w_th o o_lo ldo o_lo_f16 stats', {}, True),
    'amdnuwa_xattn2_bwd': ('xg q ldq dO lddo xkv w_th stats dS Pm dq lddq part_th part_bytes', {'part_bytes': 'amdnuwa_xattn2_bwd_workspace_bytes'}, True),
    'amdnuwa_xattn2_bwd_ex': ('xg q ldq dO lddo xkv w_th stats dS Pm dq lddq part_th part_bytes flags', {'part_bytes': 'amdnuwa_xattn2_bwd_workspace_bytes'}, True),
    'amdnuwa_xattn2_bwd_rc': ('xg q ldq dO lddo xkv w_th stats dq lddq part_th part_bytes nbd nbd_bytes dKp dVp',
                              {'part_bytes': 'amdnuwa_xattn2_bwd_workspace_bytes', 'nbd_bytes': 'amdnuwa_xattn2_bwd_rc_stats_bytes'}, True),
    'amdnuwa_xattn6_pack': ('xg kv16 ldkv context_mask f16 x6', {}, False),
    'amdnuwa_xattn6_fwd': ('xg q16 ldq x6 null_k null_v w_th o o_lo ldo o_lo_f16 stats f16', {}, True),
    'amdnuwa_xattn6_pack_bwd': ('xg kv ldkv null_k null_v context_mask x6', {}, False),
    'amdnuwa_xattn6_pack_bwd_f16': ('xg kv_f16 ldkv null_k null_v context_mask x6', {}, False),
    'amdnuwa_xattn6_bwd': ('xg q ldq dO lddo x6 null_k null_v w_th stats dS Pm dq lddq part_th part_bytes', {'part_bytes': 'amdnuwa_xattn6_bwd_workspace_bytes'}, True),
    'amdnuwa_xattn6_bwd_f16': ('xg q_f16 ldq dO_f16 lddo x6 null_k null_v w_th stats dS Pm dq lddq part_th part_bytes',
                               {'part_bytes': 'amdnuwa_xattn6_bwd_workspace_bytes'}, True),
    'amdnuwa_cattn_fwd': ('cg q16 ldq k16 v16 ldkv key_mask null_k null_v w_th o o_lo ldo o_lo_f16 stats f16', {}, False),
    'amdnuwa_cattn_fwd_drop': ('cg q16 ldq k16 v16 ldkv key_mask null_k null_v w_th o o_lo ldo o_lo_f16 stats f16 keep keep0 drop_scale', {}, False),
    'amdnuwa_cattn_bwd': ('cg q ldq k v ldkv dO lddo key_mask null_k null_v w_th stats dq lddq dk dv lddkv dw_th dnull_k dnull_v workspace workspace_bytes',
                          {'workspace_bytes': 'amdnuwa_cattn_bwd_workspace_bytes'}, False),
    'amdnuwa_cattn_bwd_drop': ('cg q ldq k v ldkv dO lddo key_mask null_k null_v w_th stats dq lddq dk dv lddkv dw_th dnull_k dnull_v workspace workspace_bytes '
                               'keep keep_t keep0 drop_scale', {'workspace_bytes': 'amdnuwa_cattn_bwd_workspace_bytes'}, False),
}
XKV_FIELDS = ('Kp', 'Kp_lo', 'Kt', 'Kt_lo', 'Vp', 'Vp_lo', 'Vt', 'Vt_lo', 'valid')
X6_FIELDS = ('K6', 'V6', 'vbits')


def jp(T):
    return ((T + 1 + 31) // 32) * 32


def ld_of(entry, name):
    """the tight leading dimension of a 16-bit operand: to_kv's [.., 2 inner] rows for the key / value side, inner = 512 elsewhere"""
    return 1024 if name in ('ldkv', 'lddkv') else 512


def cases_of(entry):
    """name -> overrides of the good call (B = 3, n = 64, T = 256, 8 heads of 64, every pointer PTR, tight leading dimensions, exact sizes).
    'g.X' / 'p.X': a field of the geometry / of the image set; 'g' / 'p': None = no geometry / no image set; 'short': bytes missing from each size"""
    params, sizes, _ = ENTRIES[entry]
    names = params.split()
    cattn, img = names[0] == 'cg', 'xkv' in names or 'x6' in names
    Z = {'g.n': 0} if ENTRIES[entry][2] else {'g.B': 0}              # no rows: returns OK before the launch wherever nothing is wrong
    ptrs = [n for n in names if n not in ('xg', 'cg', 'xkv', 'x6', 'drop_scale') and n not in INTS and n not in SIZES and not n.startswith('ld')]
    c = {'NULL geometry': {'g': None}, 'NULL geometry, pointers NULL': {'g': None, **{n: None for n in ptrs}}}
    if cattn:
        for k, v in (('heads', 0), ('heads', 9), ('dim_head', 48), ('dim_head', 128), ('B', 0), ('B', -2), ('n', 0), ('n', -1), ('n_keys', -1)):
            c[f'{k} {v}'] = {f'g.{k}': v}
        c['B 0, heads 9'] = {'g.B': 0, 'g.heads': 9}
        c['n 0, q NULL'] = {'g.n': 0, names[1]: None}
        c['causal, n_keys 40'] = {'g.causal': 1, 'g.n_keys': 40}
        c['rows past 2^31 / 1024'] = {'g.B': 1, 'g.n': 2097152}
        c['key rows past 2^31 / 1024'] = {'g.B': 1, 'g.n': 64, 'g.causal': 0, 'g.n_keys': 2097152}
        c['heads 9, q NULL'] = {'g.heads': 9, names[1]: None}
    else:
        for k, v in (('heads', 0), ('heads', 5), ('heads', 9), ('dim_head', 32), ('dim_head', 48), ('T', 0), ('T', 287), ('T', 288), ('T', 2016), ('T', 2048), ('T', 2049)):
            c[f'no rows, {k} {v}'] = {**Z, f'g.{k}': v, **({'g.JP': jp(v)} if k == 'T' else {})}
        for d in (32, -32, 8):
            c[f'no rows, JP {d:+d}'] = {**Z, 'g.JP': jp(256) + d}
        c['B 0'], c['B -1'] = {'g.B': 0}, {'g.B': -1}
        if img:
            c['heads 9, image set NULL'] = {'g.heads': 9, 'p': None}
        if ENTRIES[entry][2]:
            c['n 0'], c['n -5'], c['n 0, image set NULL'] = {'g.n': 0}, {'g.n': -5}, {'g.n': 0, 'p': None}
            c['n 0, T 2049'] = {'g.n': 0, 'g.T': 2049, 'g.JP': jp(2049)}
    # every pointer argument and image pointer NULL in turn: at the good geometry only those the entry point requires (the others would launch) ...
    for n in ptrs + (['p'] + ['p.' + f for f in (X6_FIELDS if 'x6' in names else XKV_FIELDS)] if img else []):
        if n in REQUIRED[entry]:
            c[f'{n} NULL'] = {n: None}
        # ... and all of them without rows (cattn has no such exit: a mask that fails later stands in for it in the _drop entries)
        if not cattn:
            c[f'no rows, {n} NULL'] = {**Z, n: None}
        elif 'drop_scale' in names and n not in REQUIRED[entry]:
            c[f'{n} NULL, drop_scale 0.5'] = {n: None, 'drop_scale': 0.5}
    # the leading-dimension rules, before an exit that launches nothing: B = 0, or for the cattn backward a short workspace (its forward has
    # no later exit: only values it refuses, in EXTRA)
    for n in (n for n in names if n.startswith('ld') and not (cattn and not sizes)):
        t = ld_of(entry, n)
        for v in (t + 4, t + 8, t - 8, t + 2, 504, 0):
            c[f'{n} {v}'] = {n: v, **({'short': {'workspace_bytes': 4}} if cattn else Z)}
    for s in sizes:
        c[f'{s} short'] = {'short': {s: 4}}
        c[f'{s} short, no rows'] = {'short': {s: 4}, **Z} if not cattn else {'short': {s: 4}, 'g.heads': 9}
        c[f'{s} 0 and NULL'] = {'short': {s: 1 << 62}, {'workspace_bytes': 'workspace', 'part_bytes': 'part_th', 'nbd_bytes': 'nbd'}[s]: None}
    c.update(EXTRA.get(entry, {}))
    return c


# the pointers (and image pointers) whose absence is an error at the good geometry, per entry point
X2B = {'q', 'dO', 'p', 'p.Kp', 'p.Vp', 'p.valid', 'w_th', 'stats', 'dq'}
X6B = {'p', 'p.K6', 'p.V6', 'p.vbits', 'null_k', 'null_v', 'w_th', 'stats', 'dS', 'Pm', 'dq', 'part_th'}
CF = {'q16', 'k16', 'v16', 'null_k', 'null_v', 'w_th', 'stats'}
CB = {'q', 'k', 'v', 'dO', 'null_k', 'null_v', 'w_th', 'stats', 'dq', 'dk', 'dv', 'dw_th', 'dnull_k', 'dnull_v', 'workspace'}
REQUIRED = {
    'amdnuwa_xattn_pack': {'kv', 'kv_lo', 'null_k', 'null_v', 'p', 'p.valid'}, 'amdnuwa_xattn_pack_f16': {'kv', 'kv_f16', 'null_k', 'null_v', 'p', 'p.valid'},
    'amdnuwa_xattn_fwd': {'q', 'p', 'w_th', 'o', 'p.Kp_lo', 'p.Vt_lo'}, 'amdnuwa_xattn_fwd_stats': {'q', 'p', 'w_th', 'o', 'p.Kp_lo', 'p.Vt_lo'},
    'amdnuwa_xattn_bwd': {'dO', 'p', 'w_th', 'P', 'dS', 'dq', 'dw_th', 'workspace', 'p.Vp_lo', 'p.Kt_lo'},
    'amdnuwa_xattn_unpack': {'dKp', 'dVp', 'dkv', 'dnull_k', 'dnull_v'},
    'amdnuwa_xattn2_fwd': {'q', 'p', 'p.Kp', 'p.Vt', 'p.valid', 'w_th', 'o'}, 'amdnuwa_xattn2_fwd_f16': {'q_f16', 'p', 'p.Kp_lo', 'p.Vt_lo', 'p.valid', 'w_th', 'o'},
    'amdnuwa_xattn2_bwd': X2B | {'dS', 'Pm', 'part_th'}, 'amdnuwa_xattn2_bwd_ex': X2B | {'dS', 'Pm', 'part_th'}, 'amdnuwa_xattn2_bwd_rc': X2B | {'dKp', 'dVp', 'part_th', 'nbd'},
    'amdnuwa_xattn6_pack': {'kv16', 'p', 'p.K6', 'p.V6', 'p.vbits'}, 'amdnuwa_xattn6_fwd': {'q16', 'p', 'p.K6', 'p.V6', 'p.vbits', 'null_k', 'null_v', 'w_th'},
    'amdnuwa_xattn6_pack_bwd': {'kv', 'null_k', 'null_v', 'p', 'p.K6', 'p.V6', 'p.vbits'}, 'amdnuwa_xattn6_pack_bwd_f16': {'kv_f16', 'null_k', 'null_v', 'p', 'p.K6', 'p.V6', 'p.vbits'},
    'amdnuwa_xattn6_bwd': X6B | {'q', 'dO'}, 'amdnuwa_xattn6_bwd_f16': X6B | {'q_f16', 'dO_f16'},
    'amdnuwa_cattn_fwd': CF, 'amdnuwa_cattn_fwd_drop': CF | {'keep', 'keep0'}, 'amdnuwa_cattn_bwd': CB, 'amdnuwa_cattn_bwd_drop': CB | {'keep', 'keep_t', 'keep0'},
}
BAD_MASKS = {'drop_scale 0.5': {'drop_scale': 0.5}, 'drop_scale 0': {'drop_scale': 0.0}, 'drop_scale -2': {'drop_scale': -2.0}, 'drop_scale inf': {'drop_scale': INF},
             'drop_scale NaN': {'drop_scale': NAN}, 'keep + 1': {'keep': PTR + 1}, 'keep + 2': {'keep': PTR + 2}, 'keep0 + 3': {'keep0': PTR + 3},
             'keep + 1, heads 9': {'keep': PTR + 1, 'g.heads': 9}, 'keep + 1, q NULL': {'keep': PTR + 1, 'q': None, 'q16': None},
             'keep + 1, o and o_lo NULL': {'keep': PTR + 1, 'o': None, 'o_lo': None}, 'keep + 1, ldq 8': {'keep': PTR + 1, 'ldq': 8}}
# leading dimensions the cattn forward refuses: off the 16-byte (inputs) / 8-byte (output) alignment, rows narrower than inner = 512
CF_LD = {f'{n} {v}': {n: v} for n, vs in (('ldq', (516, 514, 504, 0)), ('ldkv', (1028, 1026, 504, 0)), ('ldo', (514, 513, 508, 0))) for v in vs}
EXTRA = {
    'amdnuwa_xattn_pack': {'no image asked for': {**{'p.' + f: None for f in XKV_FIELDS[:8]}}, 'no image asked for, B 0': {'g.B': 0, **{'p.' + f: None for f in XKV_FIELDS[:8]}},
                           'lo image without kv_lo': {'kv_lo': None}, 'hi images without kv_lo, B 0': {'g.B': 0, 'kv_lo': None, **{'p.' + f: None for f in XKV_FIELDS[1:8:2]}}},
    'amdnuwa_xattn_fwd_stats': {'bf16 call on hi images, n 0': {'g.n': 0, 'q_lo': None, 'p.Kp_lo': None, 'p.Vt_lo': None}, 'T 288, q NULL': {'g.T': 288, 'g.JP': 320, 'q': None},
                                'JP + 32, q NULL': {'g.JP': 320, 'q': None}},
    'amdnuwa_xattn_bwd': {'short workspace, hi+lo call on hi images': {'short': {'workspace_bytes': 4}, 'p.Vp_lo': None}, 'short workspace, dO NULL': {'short': {'workspace_bytes': 4}, 'dO': None},
                          'bf16 call on hi images, n 0': {'g.n': 0, 'dO_lo': None, 'p.Vp_lo': None, 'p.Kt_lo': None}},
    'amdnuwa_xattn2_fwd_f16': {'o_lo NULL with o_lo_f16, n 0': {'g.n': 0, 'o_lo': None}},
    'amdnuwa_xattn2_bwd_rc': {'n 33': {'g.n': 33}, 'n 33, no geometry pointer': {'g': None, 'q': None}, 'n 32, q NULL': {'g.n': 32, 'q': None},
                              'both sizes short': {'short': {'part_bytes': 4, 'nbd_bytes': 4}}, 'part short, dKp NULL': {'short': {'part_bytes': 4}, 'dKp': None}},
    'amdnuwa_xattn6_fwd': {'o NULL, fp16 copy': {'g.n': 0, 'o': None}, 'o NULL, o_lo_f16 0': {'o': None, 'o_lo_f16': 0}, 'o and o_lo NULL': {'o': None, 'o_lo': None},
                           'o and o_lo NULL, n 0': {'g.n': 0, 'o': None, 'o_lo': None}, 'o NULL, o_lo_f16 0, q16 NULL': {'o': None, 'o_lo_f16': 0, 'q16': None}},
    'amdnuwa_xattn6_bwd': {'JP + 32, n 0': {'g.n': 0, 'g.JP': 320}, 'JP - 32': {'g.JP': 256}, 'T 2048': {'g.T': 2048, 'g.JP': jp(2048)}, 'T 2015, n 0': {'g.n': 0, 'g.T': 2015, 'g.JP': jp(2015)}},
    'amdnuwa_cattn_fwd': {**CF_LD, 'o NULL, o_lo_f16 0': {'o': None, 'o_lo_f16': 0}, 'o and o_lo NULL': {'o': None, 'o_lo': None}, 'o NULL, ldo 8': {'o': None, 'o_lo_f16': 0, 'ldo': 8}},
    'amdnuwa_cattn_fwd_drop': {**CF_LD, **BAD_MASKS, 'o NULL, o_lo_f16 0': {'o': None, 'o_lo_f16': 0}},
    'amdnuwa_cattn_bwd': {},
    'amdnuwa_cattn_bwd_drop': {**BAD_MASKS, 'keep_t + 2': {'keep_t': PTR + 2}, 'keep_t + 2, short workspace': {'keep_t': PTR + 2, 'short': {'workspace_bytes': 4}},
                               'drop_scale 0.5, no workspace': {'drop_scale': 0.5, 'workspace': None}},
}


def call(L, entry, over):
    from nuwa_pytorch_amd import _lib
    params, sizes, _ = ENTRIES[entry]
    names = params.split()
    over = dict(over)
    short = over.pop('short', {})
    if names[0] == 'cg':
        g = _lib.CGeom(3, 64, 8, 64, 0.125, 1, 0)
    else:
        g = _lib.XGeom(3, 64, 256, jp(256), 8, 64, 0.125)
    img = None
    if 'xkv' in names:
        img = _lib.XKV(*([PTR] * 9))
    elif 'x6' in names:
        img = _lib.X6KV(PTR, PTR, PTR)
    for k in [k for k in over if k.startswith('g.') or k.startswith('p.')]:
        setattr(g if k[0] == 'g' else img, k[2:], over.pop(k))
    gp = ctypes.byref(g) if over.pop('g', 1) is not None else None
    ip = ctypes.byref(img) if img is not None and over.pop('p', 1) is not None else None
    args = []
    for n in names:
        if n in ('xg', 'cg'):
            args.append(gp)
        elif n in ('xkv', 'x6'):
            args.append(ip)
        elif n in SIZES:
            nb = getattr(L, sizes[n])(gp) if gp is not None else 0
            args.append(ctypes.c_size_t(max(nb - short.get(n, 0), 0)))
        elif n.startswith('ld'):
            args.append(over.get(n, ld_of(entry, n)))
        elif n in INTS:
            args.append(over.get(n, INTS[n]))
        elif n == 'drop_scale':
            args.append(ctypes.c_float(over.get(n, 2.0)))
        else:
            v = over.get(n, PTR)
            args.append(None if v is None else ctypes.c_void_p(v))
    return getattr(L, entry)(*args, None), g


# ---------------------------------------------------------------------------------------------------
# recorded return codes, one letter per case in the order of cases_of(entry) (groups of ten): A = ARG, U = UNSUPPORTED, W = WORKSPACE, O = OK
# ---------------------------------------------------------------------------------------------------
WANT = {
    'amdnuwa_xattn_pack': 'AAUOUOUUOU UUUAAAOOUA AAAAAAAOAA OOOOOOOOAA AOOAOOAAAO',
    'amdnuwa_xattn_pack_f16': 'AAUOUOUUOU UUUAAAOOUA AAAAAAAOAA OOOOOOOOAA AOOAOO',
    'amdnuwa_xattn_fwd': 'AAUOUOUUOU UUUAAAOOUO OAUAAOAAAA OOOOOAAOAA OOOOOAAOAO OAOOOOAO',
    'amdnuwa_xattn_fwd_stats': 'AAUOUOUUOU UUUAAAOOUO OAUAAOAAAA OOOOOOAAOA AOOOOOAAOA OOAOOOOAOO UA',
    'amdnuwa_xattn_bwd': 'AAUOUOUUOU UUUAAAOOUO OAUAAOAAAA OAAOAAOAAW WAAOOOAAOA AOOOAOOAOO OOAOWOWWAO',
    'amdnuwa_xattn_unpack': 'AAUOUOUUOU UUUAAAOOAA AAAAOAAAAA OOAOO',
    'amdnuwa_xattn2_fwd': 'AAUUUUUOOU UUUUUUOOUO OAUAAAAAAO AAAAOOOOOA AOAAAOOAOO OOAO',
    'amdnuwa_xattn2_fwd_f16': 'AAUUUUUOOU UUUUUUOOUO OAUAAAAAAO OAAOAAOOOO OAAAAAOOAO OOOAOO',
    'amdnuwa_xattn2_bwd': 'AAUUUUUOOU UUUUUUOOUO OAUAAAAAAA AAAAAAAWWA AAAOOOAAOO OAAAOOAOAO OAOOOOAOWO W',
    'amdnuwa_xattn2_bwd_ex': 'AAUUUUUOOU UUUUUUOOUO OAUAAAAAAA AAAAAAAWWA AAAOOOAAOO OAAAOOAOAO OAOOOOAOWO W',
    'amdnuwa_xattn2_bwd_rc': 'AAUUUUUOOU UUUUUUOOUO UAUAAAAAAA AAAWWWWAAA AAAAAOOOAA OOOAAAOOAO AOOAOOOOAO WOWWOWUAAW A',
    'amdnuwa_xattn6_pack': 'AAUUUUUUOO OOUOOOOOUA AOAAAAAAAA AOAAAA',
    'amdnuwa_xattn6_fwd': 'AAUUUUUUOO OOUOOOOOUO OAUAAAAAAA AOOOAAAAAA AAAOOAOOOO AOOAAAA',
    'amdnuwa_xattn6_pack_bwd': 'AAUUUUUUUU UUUUUUUOUA UAUAUUAUAU AUAUUUUUUU',
    'amdnuwa_xattn6_pack_bwd_f16': 'AAUUUUUUUU UUUUUUUOUA UAUAUUAUAU AUAUUUUUUU',
    'amdnuwa_xattn6_bwd': 'AAUUUUUUOO OUUOUUUOUO OAUAAAAAAA AAAAAAAAAA AWWAAAAAAA AAOOAOAOOA OOOOAOWOWO UUO',
    'amdnuwa_xattn6_bwd_f16': 'AAUUUUUUOO OUUOUUUOUO OAUAAAAAAA AAAAAAAAAA AWWAAAAAAA AAOOAOAOOA OOOOAOWOW',
    'amdnuwa_cattn_fwd': 'AAUUUUAAAA AUAUUUUAAA AAAAAAAAAA AAAAAAAAA',
    'amdnuwa_cattn_fwd_drop': 'AAUUUUAAAA AUAUUUUAAA AAAAAAAAAA AAAAAAAAAA AAAAAAAAAU AAAA',
    'amdnuwa_cattn_bwd': 'AAUUUUAAAA AUAUUUUAAA AAAAAAAAAA AWAWAAAAWW AAAAWAAAWW AAAWWWAAAW UW',
    'amdnuwa_cattn_bwd_drop': 'AAUUUUAAAA AUAUUUUAAA AAAAAAAAAA AAWAAAAWAA AAWWAAAAWA AAWWAAAWWW AAAWUWAAAA AAAAUAAAAA A',
}


@pytest.mark.parametrize('entry', sorted(ENTRIES))
def test_return_codes_before_any_launch(entry):
    from nuwa_pytorch_amd import _lib
    L = _lib.lib()
    cases = cases_of(entry)
    want = [{'O': OK, 'A': ARG, 'U': UNSUPPORTED, 'W': WORKSPACE}[ch] for ch in WANT[entry].replace(' ', '')]
    assert len(want) == len(cases) >= 20
    cattn, needs_n = entry.startswith('amdnuwa_cattn'), ENTRIES[entry][2]
    got = []
    for (name, over), w in zip(cases.items(), want):
        B, n = over.get('g.B', 3), over.get('g.n', 64)
        assert w != OK or (not cattn and (B <= 0 or (needs_n and n <= 0))), f'{name}: a case may not reach a launch'
        got.append((name, call(L, entry, over)[0]))
    assert got == list(zip(cases, want))


# ---------------------------------------------------------------------------------------------------
# queries
# ---------------------------------------------------------------------------------------------------
X_QUERIES = ('amdnuwa_xattn2_supported', 'amdnuwa_xattn6_supported', 'amdnuwa_xattn2_bwd_rc_supported', 'amdnuwa_xattn6_image_bytes', 'amdnuwa_xattn6_bwd_image_bytes',
             'amdnuwa_xattn_bwd_workspace_bytes', 'amdnuwa_xattn2_bwd_workspace_bytes', 'amdnuwa_xattn6_bwd_workspace_bytes', 'amdnuwa_xattn2_bwd_rc_stats_bytes')
C_QUERIES = ('amdnuwa_cattn_supported', 'amdnuwa_cattn_drop_supported', 'amdnuwa_cattn_bwd_workspace_bytes')
T_VALUES = (-1, 0, 1, 30, 31, 32, 63, 64, 65, 255, 256, 287, 288, 2015, 2016, 2047, 2048, 2049)


def x_grid():
    """(B, n, T, JP, heads, dim_head): both sides of T = 287 | 288 (xattn, xattn2), 2016 (64 chunks of the xattn6 backward) and 2048 (xattn6),
    n around the 32- and 64-row tiles, JP as amdnuwa_xattn_jp gives it, one chunk more and not a multiple of 32; then the other head shapes"""
    out = [(B, n, T, jp(T) + d, 8, 64) for B in (0, 3) for n in (0, 1, 32, 33, 64, 65, 2560) for T in (0, 1, 31, 255, 256, 287, 288, 2015, 2016, 2048, 2049)
           for d in (0, 32, 8)]
    return out + [(3, 64, T, jp(T), h, dh) for T in (256, 2049) for h, dh in ((5, 64), (1, 32), (8, 32), (9, 64), (0, 64), (8, 48))]


def c_grid():
    """(B, n, heads, dim_head, causal, n_keys): the head shapes in and out of the envelope, B and n down to 0, own and foreign keys, and the
    row-count limit 2^31 / 1024 on either side"""
    out = [(B, n, h, dh, causal, nk) for B in (0, 1, 3) for n in (0, 1, 63, 64, 65, 2560) for h in (0, 1, 5, 8, 9) for dh in (32, 48, 64) for causal in (0, 1)
           for nk in (0, n, 40, -1)]
    return out + [(1, 2097151, 8, 64, 1, 0), (1, 2097152, 8, 64, 1, 0), (1, 64, 8, 64, 0, 2097151), (1, 64, 8, 64, 0, 2097152), (2047, 1024, 8, 64, 0, 1025), (2048, 1024, 8, 64, 0, 0)]


def rle(values):
    out = []
    for v in values:
        if out and out[-1][0] == v:
            out[-1][1] += 1
        else:
            out.append([v, 1])
    return ' '.join(str(v) if k == 1 else f'{v}x{k}' for v, k in out)


def unrle(text):
    out = []
    for tok in text.split():
        v, _, k = tok.partition('x')
        out += [int(v)] * int(k or 1)
    return out


def query_values(L):
    from nuwa_pytorch_amd import _lib
    got = {'amdnuwa_xattn_jp': [L.amdnuwa_xattn_jp(T) for T in T_VALUES], 'amdnuwa_xattn6_nch': [L.amdnuwa_xattn6_nch(T) for T in T_VALUES]}
    xs = [_lib.XGeom(B, n, T, JP, h, dh, dh ** -0.5 if dh else 0.0) for B, n, T, JP, h, dh in x_grid()]
    cs = [_lib.CGeom(B, n, h, dh, 0.125, causal, nk) for B, n, h, dh, causal, nk in c_grid()]
    for q in X_QUERIES:
        got[q] = [int(getattr(L, q)(ctypes.byref(g))) for g in xs] + [int(getattr(L, q)(None))]
    for q in C_QUERIES:
        got[q] = [int(getattr(L, q)(ctypes.byref(g))) for g in cs] + [int(getattr(L, q)(None))]
    return got


# recorded values, query -> one value per geometry of the grid (then the value for no geometry), 'VxK' = K times V
WANT_QUERIES = {
    'amdnuwa_xattn_jp':
        '0 32x4 64x2 96x2 256 288x2 320 2016 2048x2 2080x2',
    'amdnuwa_xattn6_nch':
        '0x2 2x6 4 8x2 10x2 64x4 66',
    'amdnuwa_xattn2_supported':
        '1x2 0 1x2 0 1x2 0 1x2 0 1 0x2 1 0x17 1x2 0 1x2 0 1x2 0 1x2 0 1 0x2 1 0x17 1x2 0 1x2 0 1x2 0 1x2 0 1 0x2 1 0x17 1x2 0 1x2 0 1x2 0 1x2 0 1 0x2 '
        '1 0x17 1x2 0 1x2 0 1x2 0 1x2 0 1 0x2 1 0x17 1x2 0 1x2 0 1x2 0 1x2 0 1 0x2 1 0x17 1x2 0 1x2 0 1x2 0 1x2 0 1 0x2 1 0x17 1x2 0 1x2 0 1x2 0 1x2 '
        '0 1 0x2 1 0x17 1x2 0 1x2 0 1x2 0 1x2 0 1 0x2 1 0x17 1x2 0 1x2 0 1x2 0 1x2 0 1 0x2 1 0x17 1x2 0 1x2 0 1x2 0 1x2 0 1 0x2 1 0x17 1x2 0 1x2 0 '
        '1x2 0 1x2 0 1 0x2 1 0x17 1x2 0 1x2 0 1x2 0 1x2 0 1 0x2 1 0x17 1x2 0 1x2 0 1x2 0 1x2 0 1 0x2 1 0x30',
    'amdnuwa_xattn6_supported':
        '0x3 1x27 0x6 1x27 0x6 1x27 0x6 1x27 0x6 1x27 0x6 1x27 0x6 1x27 0x6 1x27 0x6 1x27 0x6 1x27 0x6 1x27 0x6 1x27 0x6 1x27 0x6 1x27 0x16',
    'amdnuwa_xattn2_bwd_rc_supported':
        '1x2 0 1x2 0 1x2 0 1x2 0 1 0x2 1 0x50 1x2 0 1x2 0 1x2 0 1x2 0 1 0x2 1 0x50 1x2 0 1x2 0 1x2 0 1x2 0 1 0x2 1 0x50 1x2 0 1x2 0 1x2 0 1x2 0 1 0x2 '
        '1 0x17 1x2 0 1x2 0 1x2 0 1x2 0 1 0x2 1 0x50 1x2 0 1x2 0 1x2 0 1x2 0 1 0x2 1 0x50 1x2 0 1x2 0 1x2 0 1x2 0 1 0x2 1 0x50 1x2 0 1x2 0 1x2 0 1x2 '
        '0 1 0x2 1 0x30',
    'amdnuwa_xattn6_image_bytes':
        '0x234 196608x6 786432x6 983040x6 6291456x9 0x6 196608x6 786432x6 983040x6 6291456x9 0x6 196608x6 786432x6 983040x6 6291456x9 0x6 196608x6 '
        '786432x6 983040x6 6291456x9 0x6 196608x6 786432x6 983040x6 6291456x9 0x6 196608x6 786432x6 983040x6 6291456x9 0x6 196608x6 786432x6 983040x6 '
        '6291456x9 0x16',
    'amdnuwa_xattn6_bwd_image_bytes':
        '0x234 98304 196608 0 98304 196608 0 786432 884736 0 884736 983040 0 884736 983040 0 983040 1081344 0 6193152 6291456 0 6291456 0x11 98304 '
        '196608 0 98304 196608 0 786432 884736 0 884736 983040 0 884736 983040 0 983040 1081344 0 6193152 6291456 0 6291456 0x11 98304 196608 0 98304 '
        '196608 0 786432 884736 0 884736 983040 0 884736 983040 0 983040 1081344 0 6193152 6291456 0 6291456 0x11 98304 196608 0 98304 196608 0 '
        '786432 884736 0 884736 983040 0 884736 983040 0 983040 1081344 0 6193152 6291456 0 6291456 0x11 98304 196608 0 98304 196608 0 786432 884736 '
        '0 884736 983040 0 884736 983040 0 983040 1081344 0 6193152 6291456 0 6291456 0x11 98304 196608 0 98304 196608 0 786432 884736 0 884736 '
        '983040 0 884736 983040 0 983040 1081344 0 6193152 6291456 0 6291456 0x11 98304 196608 0 98304 196608 0 786432 884736 0 884736 983040 0 '
        '884736 983040 0 983040 1081344 0 6193152 6291456 0 6291456 0x21',
    'amdnuwa_xattn_bwd_workspace_bytes':
        '0x267 768 0x2 768 0x2 768 0x2 768 0x2 768 0x20 768 0x2 768 0x2 768 0x2 768 0x2 768 0x20 1536 0x2 1536 0x2 1536 0x2 1536 0x2 1536 0x20 1536 '
        '0x2 1536 0x2 1536 0x2 1536 0x2 1536 0x20 2304 0x2 2304 0x2 2304 0x2 2304 0x2 2304 0x20 61440 0x2 61440 0x2 61440 0x2 61440 0x2 61440 0x17 '
        '600 24 1536 0x10',
    'amdnuwa_xattn2_bwd_workspace_bytes':
        '0x264 768x2 0 768x2 0 768x2 0 768x2 0 768 0x2 768 0x17 768x2 0 768x2 0 768x2 0 768x2 0 768 0x2 768 0x17 768x2 0 768x2 0 768x2 0 768x2 0 768 '
        '0x2 768 0x17 768x2 0 768x2 0 768x2 0 768x2 0 768 0x2 768 0x17 1536x2 0 1536x2 0 1536x2 0 1536x2 0 1536 0x2 1536 0x17 30720x2 0 30720x2 0 '
        '30720x2 0 30720x2 0 30720 0x2 30720 0x30',
    'amdnuwa_xattn6_bwd_workspace_bytes':
        '0x267 768x2 0 768x2 0 768x2 0 768x2 0 768x2 0 768x2 0 768x2 0 768 0x11 768x2 0 768x2 0 768x2 0 768x2 0 768x2 0 768x2 0 768x2 0 768 0x11 '
        '768x2 0 768x2 0 768x2 0 768x2 0 768x2 0 768x2 0 768x2 0 768 0x11 768x2 0 768x2 0 768x2 0 768x2 0 768x2 0 768x2 0 768x2 0 768 0x11 1536x2 0 '
        '1536x2 0 1536x2 0 1536x2 0 1536x2 0 1536x2 0 1536x2 0 1536 0x11 30720x2 0 30720x2 0 30720x2 0 30720x2 0 30720x2 0 30720x2 0 30720x2 0 30720 '
        '0x21',
    'amdnuwa_xattn2_bwd_rc_stats_bytes':
        '0x297 6144x2 0 6144x2 0 6144x2 0 6144x2 0 6144 0x2 6144 0x50 12288x2 0 12288x2 0 12288x2 0 12288x2 0 12288 0x2 12288 0x50 491520x2 0 '
        '491520x2 0 491520x2 0 491520x2 0 491520 0x2 491520 0x30',
    'amdnuwa_cattn_supported':
        '0x864 1x3 0 1x2 0x10 1x3 0 1x2 0x2 1x3 0 1x2 0x10 1x3 0 1x2 0x2 1x3 0 1x2 0x10 1x3 0 1x2 0x50 1x3 0 1x2 0x10 1x3 0 1x2 0x2 1x3 0 1x2 0x10 '
        '1x3 0 1x2 0x2 1x3 0 1x2 0x10 1x3 0 1x2 0x50 1x3 0 1x2 0x10 1x3 0 1x2 0x2 1x3 0 1x2 0x10 1x3 0 1x2 0x2 1x3 0 1x2 0x10 1x3 0 1x2 0x50 1x3 0 '
        '1x2 0x10 1x3 0 1x2 0x2 1x3 0 1x2 0x10 1x3 0 1x2 0x2 1x3 0 1x2 0x10 1x3 0 1x2 0x50 1x3 0 1x2 0x10 1x3 0 1x2 0x2 1x3 0 1x2 0x10 1x3 0 1x2 0x2 '
        '1x3 0 1x2 0x10 1x3 0 1x2 0x170 1x3 0 1x2 0x10 1x3 0 1x2 0x2 1x3 0 1x2 0x10 1x3 0 1x2 0x2 1x3 0 1x2 0x10 1x3 0 1x2 0x50 1x3 0 1x2 0x10 1x3 0 '
        '1x2 0x2 1x3 0 1x2 0x10 1x3 0 1x2 0x2 1x3 0 1x2 0x10 1x3 0 1x2 0x50 1x3 0 1x2 0x10 1x3 0 1x2 0x2 1x3 0 1x2 0x10 1x3 0 1x2 0x2 1x3 0 1x2 0x10 '
        '1x3 0 1x2 0x50 1x3 0 1x2 0x10 1x3 0 1x2 0x2 1x3 0 1x2 0x10 1x3 0 1x2 0x2 1x3 0 1x2 0x10 1x3 0 1x2 0x50 1x3 0 1x2 0x10 1x3 0 1x2 0x2 1x3 0 '
        '1x2 0x10 1x3 0 1x2 0x2 1x3 0 1x2 0x10 1x3 0 1x2 0x26 1 0 1 0x4',
    'amdnuwa_cattn_drop_supported':
        '0x864 1x3 0 1x2 0x10 1x3 0 1x2 0x2 1x3 0 1x2 0x10 1x3 0 1x2 0x2 1x3 0 1x2 0x10 1x3 0 1x2 0x50 1x3 0 1x2 0x10 1x3 0 1x2 0x2 1x3 0 1x2 0x10 '
        '1x3 0 1x2 0x2 1x3 0 1x2 0x10 1x3 0 1x2 0x50 1x3 0 1x2 0x10 1x3 0 1x2 0x2 1x3 0 1x2 0x10 1x3 0 1x2 0x2 1x3 0 1x2 0x10 1x3 0 1x2 0x50 1x3 0 '
        '1x2 0x10 1x3 0 1x2 0x2 1x3 0 1x2 0x10 1x3 0 1x2 0x2 1x3 0 1x2 0x10 1x3 0 1x2 0x50 1x3 0 1x2 0x10 1x3 0 1x2 0x2 1x3 0 1x2 0x10 1x3 0 1x2 0x2 '
        '1x3 0 1x2 0x10 1x3 0 1x2 0x170 1x3 0 1x2 0x10 1x3 0 1x2 0x2 1x3 0 1x2 0x10 1x3 0 1x2 0x2 1x3 0 1x2 0x10 1x3 0 1x2 0x50 1x3 0 1x2 0x10 1x3 0 '
        '1x2 0x2 1x3 0 1x2 0x10 1x3 0 1x2 0x2 1x3 0 1x2 0x10 1x3 0 1x2 0x50 1x3 0 1x2 0x10 1x3 0 1x2 0x2 1x3 0 1x2 0x10 1x3 0 1x2 0x2 1x3 0 1x2 0x10 '
        '1x3 0 1x2 0x50 1x3 0 1x2 0x10 1x3 0 1x2 0x2 1x3 0 1x2 0x10 1x3 0 1x2 0x2 1x3 0 1x2 0x10 1x3 0 1x2 0x50 1x3 0 1x2 0x10 1x3 0 1x2 0x2 1x3 0 '
        '1x2 0x10 1x3 0 1x2 0x2 1x3 0 1x2 0x10 1x3 0 1x2 0x26 1 0 1 0x4',
    'amdnuwa_cattn_bwd_workspace_bytes':
        '0x864 2048x3 0 2048x2 0x10 2816x3 0 2816x2 0x2 5120x3 0 5120x2 0x10 8960x3 0 8960x2 0x2 7424x3 0 7424x2 0x10 13568x3 0 13568x2 0x50 5632x3 0 '
        '5632x2 0x10 6400x3 0 6400x2 0x2 9728x3 0 9728x2 0x10 13568x3 0 13568x2 0x2 12800x3 0 12800x2 0x10 18944x3 0 18944x2 0x50 5632x3 0 5632x2 '
        '0x10 6400x3 0 6400x2 0x2 9728x3 0 9728x2 0x10 13568x3 0 13568x2 0x2 12800x3 0 12800x2 0x10 18944x3 0 18944x2 0x50 6912x3 0 6912x2 0x10 '
        '7680x3 0 7680x2 0x2 11008x3 0 11008x2 0x10 14848x3 0 14848x2 0x2 14080x3 0 14080x2 0x10 20224x3 0 20224x2 0x50 199936x3 0 199936x2 0x10 '
        '205312x3 0 205312x2 0x2 262400x3 0 262400x2 0x10 289280x3 0 289280x2 0x2 309248x3 0 309248x2 0x10 352256x3 0 352256x2 0x170 3072x3 0 3072x2 '
        '0x10 3840x3 0 3840x2 0x2 6144x3 0 6144x2 0x10 9984x3 0 9984x2 0x2 8448x3 0 8448x2 0x10 14592x3 0 14592x2 0x50 15360x3 0 15360x2 0x10 16128x3 '
        '0 16128x2 0x2 21504x3 0 21504x2 0x10 25344x3 0 25344x2 0x2 26112x3 0 26112x2 0x10 32256x3 0 32256x2 0x50 15360x3 0 15360x2 0x10 16128x3 0 '
        '16128x2 0x2 21504x3 0 21504x2 0x10 25344x3 0 25344x2 0x2 26112x3 0 26112x2 0x10 32256x3 0 32256x2 0x50 17664x3 0 17664x2 0x10 18432x3 0 '
        '18432x2 0x2 23808x3 0 23808x2 0x10 27648x3 0 27648x2 0x2 28416x3 0 28416x2 0x10 34560x3 0 34560x2 0x50 599296x3 0 599296x2 0x10 614912x3 0 '
        '614912x2 0x2 784640x3 0 784640x2 0x10 862720x3 0 862720x2 0x2 923648x3 0 923648x2 0x10 1048576x3 0 1048576x2 0x26 244387840 0 18944 0x4',
}


def test_queries():
    from nuwa_pytorch_amd import _lib
    got = query_values(_lib.lib())
    assert sorted(got) == sorted(WANT_QUERIES)
    assert sum(len(v) for v in got.values()) == 2 * 18 + 9 * 475 + 3 * 2167
    bad = {q: [(i, a, b) for i, (a, b) in enumerate(zip(v, unrle(WANT_QUERIES[q]))) if a != b][:5] for q, v in got.items() if v != unrle(WANT_QUERIES[q])}
    assert not bad, bad
