"""The Sparse3DNA value-test cases (s3_cases_util.py) without a GPU: the case list is complete.  Walked through the launch log
(tools/launch_log: sparse3dna.hip + sparse3dna_wide.hip compiled with launch_log.h, fake operand addresses, nothing preloaded, nothing
launched) every case returns 0 and launches its kernels, every one of the 71 kernel instantiations of the two files is launched by at
least two cases, every route s3_route() can return is reached (with and without a mask where it admits one), and every kernel is reached
at the edges of its geometry (the rules below, read off the case geometry).  The inputs are shown not to be vacuous in float64: a window
slot moved one column changes the touched output rows by more than twice the bf16 forward tolerance; every keep mask has its special rows."""
import ctypes
import os
import re
import shutil
import sys

import pytest
import torch

import s3_cases_util as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, 'profiles', 's3_value_routes.txt')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
CASES = SC.all_cases()
BY_NAME = {c['name']: c for c in CASES}
ENTRIES = set(SC.PARAMS)


def test_case_list_shape():
    assert 150 <= len(CASES) <= 300
    for c in CASES:
        assert tuple(c) == SC.CASE_KEYS
        assert c['form'] in SC.FORMS and set(c['entries']) <= ENTRIES and 1 <= len(c['entries']) <= 2
        assert all(('_drop' in e) == (c['keep'] is not None) for e in c['entries'])
        F, H, W = c['grid']
        assert 1 <= c['B'] <= 3 and 2 <= c['ntok'] <= 1 + F * H * W
        tw, nt = SC.tile(c)
        if SC.is_band_geom(c):
            assert F * H * W <= 3 * 16 * 16
        elif nt > 1:
            assert F * H * W <= 2 * 4 * 64
        else:
            assert F * H * W <= 64
    # B = 2, and one B = 1 and one B = 3 in every kernel family
    for fam in ('valu.', 'wide.', 'band.'):
        assert {1, 2, 3} <= {c['B'] for c in CASES if c['group'].startswith(fam)}, fam


def test_call_shapes_name_every_parameter():
    from nuwa_pytorch_amd import _lib
    for e in ENTRIES:
        assert len(SC.PARAMS[e].split()) + 2 == len(_lib.SIGNATURES[e][1]), e          # + the geometry in front, the stream behind
    for c in CASES:
        for e in c['entries']:
            gs, args = SC.call_shape(c, e, 0)
            assert [n for n, _ in args] == SC.PARAMS[e].split()
            assert len(gs) == len(SC.GEOM_FIELDS) + 2


# ---------------------------------------------------------------------------------------------------
# the launch-log walk
# ---------------------------------------------------------------------------------------------------
def short(kernel):
    return re.sub(r'^void |\(.*$', '', kernel)


def walk(lib_path):
    """-> (kernels of the two files, rows): one row per case = (case, [(entry, return code, launched kernels, stub calls)])"""
    sys.path.insert(0, os.path.join(ROOT, 'tools', 'launch_log'))
    try:
        import run as LR
        import cases_s3_values as CS
    finally:
        sys.path.pop(0)
    names, kernels = LR.symbols(lib_path)
    L = ctypes.CDLL(lib_path)
    L.launch_log_take.restype = ctypes.c_size_t
    L.launch_log_take.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
    tuning = (ctypes.c_int * 32).in_dll(L, 'g_amdnuwa_tuning')
    buf = ctypes.create_string_buffer(1 << 16)
    rows = {}
    for name, keys, call in CS.cases(L):
        for k in range(32):
            tuning[k] = keys.get(k, 0)
        rc = call()
        n = L.launch_log_take(buf, len(buf))
        assert n < len(buf)
        body = re.sub(r'\+0x([0-9a-f]+)', lambda m: names.get(int(m.group(1), 16), m.group(0)), buf.value.decode())
        launched = [short(ln[len('launch '):ln.index(' grid ')]) for ln in body.splitlines() if ln.startswith('launch ')]
        extern = [ln.split(' ')[1] for ln in body.splitlines() if ln.startswith('extern ')]
        cname, entry = name.split(' :: ')
        rows.setdefault(cname, []).append((entry, rc, launched, extern))
    for k in range(32):
        tuning[k] = 0
    return {short(k) for k in kernels}, [(BY_NAME[n], calls) for n, calls in rows.items()]


def table_text(kernels, rows):
    seen = {}
    lines = ['# case -> kernels, written by tests/test_s3_cases_cpu.py::test_every_instantiation_is_reached (launch-log walk of sparse3dna.hip +',
             '# sparse3dna_wide.hip, no GPU).  columns: tuning keys | case | entry: return code, launches (+ column-sum stub) ; ...']
    for c, calls in rows:
        for _, _, launched, _ in calls:
            for kn in launched:
                seen[kn] = seen.get(kn, 0) + 1
        keys = ','.join(f'{k}={v}' for k, v in sorted(c['keys'].items()))
        cols = ' ; '.join(f'{e.replace("amdnuwa_", "")}: {rc}, {" > ".join(l)}{" + " + x[0] if x else ""}' for e, rc, l, x in calls)
        lines.append(f'{keys or "-"} | {c["name"]} | {cols}')
    lines.append(f'# {len(kernels)} kernel instantiations, launches per instantiation:')
    lines += [f'# {seen.get(kn, 0):5d}  {kn}' for kn in sorted(kernels)]
    never = sorted(kernels - set(seen))
    lines.append('# never launched: ' + (', '.join(never) if never else 'none'))
    return '\n'.join(lines) + '\n'


@pytest.fixture(scope='module')
def walked(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which('hipcc')):
        pytest.skip('hipcc is not installed')
    sys.path.insert(0, os.path.join(ROOT, 'tools', 'launch_log'))
    try:
        import run as LR
        import cases_s3_values as CS
    finally:
        sys.path.pop(0)
    return walk(LR.build(ROOT, CS.SOURCE, CS.STUBS, str(tmp_path_factory.mktemp('launch_log')), []))


def launched_of(calls):
    return [k for _, _, l, _ in calls for k in l]


def test_every_case_launches(walked):
    kernels, rows = walked
    assert len(rows) == len(CASES)
    for c, calls in rows:
        assert [e for e, *_ in calls] == list(c['entries']), c['name']
        for entry, rc, launched, extern in calls:
            assert rc == 0 and launched, (c['name'], entry, rc)
            if '_bwd' in entry:                               # query side, key side, final sums (+ the column sums of d(rel_bias))
                assert len(launched) == 3 and launched[2] == 's3_bwd_fin_kernel', (c['name'], launched)
                assert ('bwd_q' in launched[0]) and ('bwd_kv' in launched[1]), (c['name'], launched)
                assert (extern == ['amdnuwa_colsum']) == c['bias'], (c['name'], extern)
            else:
                assert len(launched) == 1 and 'fwd' in launched[0] and not extern, (c['name'], launched)
            masked = [k for k in launched if re.search(r', true>$', k) and ('fwd' in k or 'bwd_q' in k)]
            assert bool(masked) == (c['keep'] is not None), (c['name'], launched)


def reach(rows):
    r = {}
    for c, calls in rows:
        for kn in set(launched_of(calls)):
            r.setdefault(kn, []).append(c)
    return r


# ---- edges, per kernel: (rule name, predicate on a case).  A rule holds for a kernel when one of the cases that reach it satisfies it.
def _nq(c):
    return c['ntok'] - 1


def _absent_rows(c, rows):
    """rows of the last `rows`-row tile of the last frame that hold no query (dilation 1 on the row axis)"""
    F, H, W = c['grid']
    left = _nq(c) - (F - 1) * H * W
    present = -(-left // W)
    return (rows - present % rows) % rows if c['dilation'][1] == 1 and present < H else 0


VALU_RULES = [
    ('W * heads * 4 is no multiple of 64', lambda c: (c['grid'][2] * c['heads'] * 4) % 64 != 0),
    ('the sequence ends inside a grid row', lambda c: not c['cross'] and _nq(c) > 1 and _nq(c) % c['grid'][2] != 0),
    ('the sequence ends inside a frame', lambda c: not c['cross'] and _nq(c) > 1 and _nq(c) % (c['grid'][1] * c['grid'][2]) != 0),
    ('ntok = 2', lambda c: c['ntok'] == 2),
    ('a dilation at least the grid extent', lambda c: not c['cross'] and any(d >= e and k > 1 for d, e, k in zip(c['dilation'], c['grid'], c['window']))),
    ('a window extent of 1', lambda c: not c['cross'] and 1 in c['window']),
    ('cross form, every key of one sample hidden', lambda c: bool(c['cross']) and c['cross']['key_mask'] == 'sample1'),
    ('cross form, partial last query frame', lambda c: bool(c['cross']) and _nq(c) % (c['grid'][1] * c['grid'][2]) != 0),
]
VALU_UNMASKED = [('the non-causal window', lambda c: not c['causal'] and not c['cross'])]
WIDE_RULES = [
    ('two column tiles', lambda c: SC.tile(c)[1] == 2),
    ('at least three column tiles', lambda c: SC.tile(c)[1] >= 3),
    ('W no multiple of the tile width', lambda c: c['grid'][2] % SC.tile(c)[0] != 0),
    ('a column dilation whose halo crosses a tile border', lambda c: c['dilation'][2] > 1 and c['window'][2] > 1),
    ('the sequence ends inside a tile', lambda c: (_nq(c) % c['grid'][2]) % SC.tile(c)[0] != 0),
]
BAND_ROW = [                                                  # kernels that walk one query row per workgroup
    ('odd H', lambda c: c['grid'][1] % 2 == 1),
    ('kw below 3', lambda c: c['window'][2] < 3),
    ('different dilations per axis', lambda c: len(set(c['dilation'])) == 3),
    ('a partial last frame', lambda c: _nq(c) % (c['grid'][1] * 16) != 0),
]
BAND_TILE = [
    ('kw below 3', lambda c: c['window'][2] < 3),
    ('different dilations per axis', lambda c: len(set(c['dilation'])) == 3),
    ('a row dilation above 1', lambda c: c['dilation'][1] > 1),
    ('a partial last frame', lambda c: _nq(c) % (c['grid'][1] * 16) != 0),
]
BAND_TILE2 = BAND_TILE + [('H splits into two-row tiles', lambda c: c['grid'][1] % (2 * c['dilation'][1]) == 0),
                          ('the last row of a tile absent', lambda c: _absent_rows(c, 2) == 1)]
BAND_TILE4 = BAND_TILE + [('H splits into four-row tiles', lambda c: c['grid'][1] % (4 * c['dilation'][1]) == 0)] + \
    [(f'the last {n} row(s) of a tile absent', lambda c, n=n: _absent_rows(c, 4) == n) for n in (1, 2, 3)]
BIAS_BOTH = [('relative-position bias', lambda c: c['bias']), ('no bias', lambda c: not c['bias'])]


def rules_of(kn):
    drop = kn.endswith(', true>') and ('fwd' in kn or 'bwd_q' in kn)
    if kn.startswith('s3w_'):
        return WIDE_RULES
    if re.match(r's3_(fwd|bwd_q|bwd_kv)_kernel', kn):
        return VALU_RULES + ([] if drop else VALU_UNMASKED)
    if kn == 's3_bwd_fin_kernel':
        return VALU_RULES + VALU_UNMASKED + WIDE_RULES + BAND_ROW
    if kn.startswith('s3_fwd_mfma_kernel'):
        return BAND_ROW + BIAS_BOTH
    if kn.startswith('s3_fwd_tile_kernel<2'):
        return BAND_TILE2
    if kn.startswith('s3_fwd_tile_kernel<4'):
        return BAND_TILE4
    if kn.startswith('s3_bwd_kv_rc_mfma_kernel'):
        return []                                             # the opt-in recomputing key side: its route cases alone
    if kn.startswith('s3_bwd_kv_mfma_kernel<false'):
        return BAND_ROW                                       # the fp32 pair: bias cases (and tuning keys 19 / 24)
    if kn.startswith(('s3_bwd_q_mfma_kernel', 's3_bwd_kv_mfma_kernel')):
        return BAND_ROW
    raise AssertionError(f'no rules for {kn}')


def test_every_instantiation_is_reached(walked):
    kernels, rows = walked
    assert len(kernels) == 71
    assert sum(1 for k in kernels if k.startswith('s3w_')) == 20
    text = table_text(kernels, rows)
    try:
        with open(TABLE, 'w') as f:
            f.write(text)
    except OSError:
        pass
    assert text.endswith('# never launched: none\n'), text[text.rindex('# never launched'):]
    r = reach(rows)
    problems = []
    for kn in sorted(kernels):
        hits = r.get(kn, [])
        if len(hits) < 2:
            problems.append(f'{kn}: {len(hits)} case(s)')
        for rule, pred in rules_of(kn):
            if not any(pred(c) for c in hits):
                problems.append(f'{kn}: no case with {rule}')
    assert not problems, '\n'.join(problems)


def test_band_kernels_in_every_operand_form(walked):
    """every band group runs in the bf16 form, the fp16 forward and the fp16-gradient backward, masked and not"""
    kernels, rows = walked
    for group in SC.BAND:
        got = {(c['form'], c['keep'] is not None) for c, calls in rows if c['group'] == group and all('mfma' in k or 'tile' in k or 'fin' in k for k in launched_of(calls))}
        assert got == {(f, m) for f in ('bf16', 'f16fwd', 'f16grad') for m in (False, True)}, (group, got)
    # both head widths of the column-tiled kernels, masked and not, in both operand forms
    for dh in (32, 64):
        for lo in ('false', 'true'):
            for dr in ('false', 'true'):
                for k in ('s3w_fwd_kernel', 's3w_bwd_q_kernel'):
                    assert f'{k}<{dh}, {lo}, {dr}>' in kernels


# ---- routes: tuning keys (and bias) -> (forward kernel, query side, key side) as regular expressions; rc = the route admits no mask
BANDF, VALUF = r's3_fwd_tile_kernel<2, false, false, {m}>', r's3_fwd_kernel<64, false, {m}>'
QB, QV = r's3_bwd_q_mfma_kernel<false, false, {m}>', r's3_bwd_q_kernel<64, false, {m}>'
KV_PACKED, KV_F32, KV_RC, KV_VALU = r's3_bwd_kv_mfma_kernel<true, false>', r's3_bwd_kv_mfma_kernel<false, false>', 's3_bwd_kv_rc_mfma_kernel', r's3_bwd_kv_kernel<64, false>'
ROUTES = {                     # group: (forward, query side, key side unmasked, key side masked)
    'route.default': (BANDF, QB, KV_PACKED, KV_PACKED),
    'route.3=1': (VALUF, QB, KV_PACKED, KV_PACKED),
    'route.3=2': (BANDF, QB, KV_PACKED, KV_PACKED),
    'route.4=1': (BANDF, QV, KV_VALU, KV_VALU),
    'route.4=2': (BANDF, QB, KV_VALU, KV_VALU),
    'route.4=4': (BANDF, QB, KV_RC, KV_PACKED),
    'route.19=1': (BANDF, QB, KV_F32, KV_F32),
    'route.24=1': (BANDF, QB, KV_F32, KV_F32),
    'route.26=1': (BANDF, QB, KV_PACKED, None),               # masked: everything on the VALU kernels (below)
    'route.4=1,19=1': (BANDF, QV, KV_VALU, KV_VALU),
    'route.4=2,19=1': (BANDF, QB, KV_VALU, KV_VALU),
    'route.4=4,19=1': (BANDF, QB, KV_RC, KV_F32),
    'route.4=4,24=1': (BANDF, QB, KV_RC, KV_F32),
}


def test_every_route_is_reached(walked):
    kernels, rows = walked
    assert {SC.route_group(k) for k in SC.ROUTE_KEYS} == set(ROUTES)
    by = {(c['group'], c['keep'] is not None): launched_of(calls) for c, calls in rows if c['group'].startswith('route.')}
    for group, (fwd, q, kv0, kv1) in ROUTES.items():
        for masked in (False, True):
            assert (group, masked) in by, f'{group}: no {"masked" if masked else "unmasked"} case'
            m = 'true' if masked else 'false'
            want = [fwd.format(m=m), q.format(m=m), kv1 if masked else kv0, 's3_bwd_fin_kernel']
            if group == 'route.26=1' and masked:
                want = [VALUF.format(m=m), QV.format(m=m), KV_VALU, 's3_bwd_fin_kernel']
            assert by[(group, masked)] == want, (group, masked, by[(group, masked)])
    for masked in (False, True):
        m = 'true' if masked else 'false'
        assert ('route.hilo', masked) in by and ('route.bias24', masked) in by, 'route.hilo / route.bias24: a case is missing'
        assert by[('route.hilo', masked)] == [f's3_fwd_kernel<64, true, {m}>', f's3_bwd_q_kernel<64, true, {m}>', 's3_bwd_kv_kernel<64, true>', 's3_bwd_fin_kernel']
        assert by[('route.bias24', masked)] == [f's3_fwd_tile_kernel<2, false, true, {m}>', f's3_bwd_q_mfma_kernel<true, false, {m}>', KV_F32, 's3_bwd_fin_kernel']
    # tuning key 16 = 1, 2 (the default) and 4 each pick their forward kernel at a geometry that admits four-row tiles
    for group, want in (('band.kw2@1', 's3_fwd_mfma_kernel'), ('band.kw2@2', 's3_fwd_tile_kernel<2'), ('band.kw2@4', 's3_fwd_tile_kernel<4')):
        hit = [launched_of(calls)[0] for c, calls in rows if c['group'] == group and c['form'] != 'f16grad']
        assert hit and all(k.startswith(want) for k in hit), (group, hit)


def test_mask_keeps_route(walked):
    """a masked case launches the masked forms of its unmasked twin's kernels, except where s3_cases_util.mask_keeps_route says otherwise"""
    kernels, rows = walked
    by = {c['name']: launched_of(calls) for c, calls in rows}
    plain = lambda k: re.sub(r', true>$', ', false>', k) if ('fwd' in k or 'bwd_q' in k) else k
    n = 0
    for c, calls in rows:
        if c['keep'] is not None:
            twin = by[c['name'].replace(' masked', '')]
            assert ([plain(k) for k in launched_of(calls)] == twin) == SC.mask_keeps_route(c), (c['name'], launched_of(calls), twin)
            n += 1
    assert n == len(MASKED)


def test_every_group_is_needed():
    """deleting a case group leaves some rule above without its case: every group is named by a rule, a route or a band form check"""
    groups = {c['group'] for c in CASES}
    named = set(ROUTES) | set(SC.BAND) | {'route.hilo', 'route.bias24', 'valu.edge', 'valu.dil', 'valu.ntok2', 'valu.noncausal', 'valu.cross',
                                          'wide.two', 'wide.three'}
    assert groups == named
    only = {                       # the VALU / wide rule that one group alone satisfies
        'valu.edge': VALU_RULES[1], 'valu.dil': VALU_RULES[4], 'valu.ntok2': VALU_RULES[3], 'valu.noncausal': VALU_UNMASKED[0],
        'valu.cross': VALU_RULES[6], 'wide.two': WIDE_RULES[0], 'wide.three': WIDE_RULES[1],
    }
    for group, (rule, pred) in only.items():
        fam = group.split('.')[0]
        assert {c['group'] for c in CASES if c['group'].startswith(fam + '.') and pred(c)} == {group}, rule
    band_only = {'band.odd': BAND_ROW[0], 'band.t2': BAND_TILE2[-1], 'band.t4_1': BAND_TILE4[-3], 'band.t4_2': BAND_TILE4[-2],
                 'band.t4_3': BAND_TILE4[-1]}
    for group, (rule, pred) in band_only.items():               # (among the cases of the same tuning key 16, i.e. of the same forward kernel)
        k16 = SC.BAND[group][5].get(16, 0)
        assert {c['group'] for c in CASES if c['group'].startswith('band.') and c['keys'].get(16, 0) == k16 and pred(c)} == {group}, rule
    # band.kw2@1 / @2 / @4 and band.dil@2 / @4: kw below 3 and a row dilation above 1, once per forward kernel (tuning key 16)
    assert {c['group'] for c in CASES if c['group'].startswith('band.') and BAND_TILE[0][1](c)} == {'band.kw2@1', 'band.kw2@2', 'band.kw2@4'}
    assert {c['group'] for c in CASES if c['group'].startswith('band.') and BAND_TILE[2][1](c)} == {'band.dil@2', 'band.dil@4'}


# ---------------------------------------------------------------------------------------------------
# the inputs are not vacuous (float64, the reference alone)
# ---------------------------------------------------------------------------------------------------
def _geometries():
    seen = {}
    for c in CASES:
        key = (c['grid'], c['window'], c['dilation'], c['heads'], c['dim_head'], c['ntok'], c['B'], c['causal'], repr(c['cross']))
        if key not in seen and c['ntok'] > 2 and not c['bias'] and c['keep'] is None:
            seen[key] = c
    return list(seen.values())


GEOMS = _geometries()


@pytest.mark.parametrize('c', GEOMS, ids=[c['name'] for c in GEOMS])
def test_inputs_are_not_vacuous(c):
    """one window slot moved one column to the left in the neighbour table (the first slot that admits it, a middle one, the last): at least
    95 % of the query rows the change touches differ by more than twice the bf16 forward tolerance, measured as gpu_util.report does"""
    R = SC.reference(c)
    ref = R['o'].detach()
    W = c['grid'][2]
    if c['cross']:
        idx, valid = SC.cross_window(c)
        ok = valid & (idx % W > 0)
    else:
        idx = SC.table(c)
        ok = (idx >= 0) & (idx % W > 0)
        ok[c['ntok'] - 1:] = False
    cand = [t for t in range(idx.shape[1]) if bool(ok[:, t].any())]
    assert cand, c['name']
    for t in sorted({cand[0], cand[len(cand) // 2], cand[-1]}):
        idx2 = idx.clone()
        idx2[ok[:, t], t] -= 1
        with torch.no_grad():
            o2, _ = SC.forward64(c, R['I'], R['keep'], 1.0, idx=idx2)
        rows = torch.nonzero(ok[:, t][:c['ntok'] - 1]).flatten()
        a, b = (o2, ref) if c['cross'] else (o2[:, 1:], ref[:, 1:])
        if c['cross'] and c['cross']['key_mask'] == 'sample1':
            a, b = a[:1], b[:1]                                       # (sample 1 sees the null key alone: no slot to move)
        diff = (a - b)[:, rows].abs().amax(dim=(0, 2, 3)) / b.abs().max()
        frac = float((diff > 2 * 2 ** -7).double().mean())
        print(f'{c["name"]} slot {t}: {len(rows)} rows touched, {100 * frac:.0f} % differ, median {float(diff.median()):.3f}')
        assert frac >= 0.95, (c['name'], t, frac)


MASKED = [c for c in CASES if c['keep'] is not None]


def test_every_mask_has_its_special_rows():
    for c in MASKED:
        keep = SC.keep_mask(c)
        (r0, r1, r2), tail = SC.special_rows(c)
        assert len({r0, r1, r2}) == 3, c['name']
        assert not bool(keep[r0[0], r0[1]].any()), c['name']
        assert int(keep[r1[0], r1[1], :, 1].sum()) == 1 and bool(keep[r1[0], r1[1], 0, 1]), c['name']
        assert not bool(keep[r2[0], r2[1], 0].any()) and bool(keep[r2[0], r2[1], 1:].all()), c['name']
        F, H, W = c['grid']
        if (c['ntok'] - 1) % (H * W) and c['ntok'] > 7:
            assert tail == (0, c['ntok'] - 2) and not bool(keep[tail[0], tail[1]].any()), c['name']
        frac, count = SC.rest_fraction(c, keep)
        assert 0.60 <= frac <= 0.90, (c['name'], frac, count)
        assert bool(SC.keep_mask(c, ones=True).all())
