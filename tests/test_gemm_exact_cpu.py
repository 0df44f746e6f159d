"""The exact-sum GEMM cases (gemm_exact_util.py) without a GPU: every case's operands meet the exactness conditions, and the case list is
complete -- walked through the launch log (tools/launch_log: gemm.hip compiled with launch_log.h, fake operand addresses, nothing
preloaded, nothing launched) it reaches every kernel instantiation of gemm.hip at least twice, each NT / TN kernel at a shape with M and N
off its tile and at the shortest main loop its route admits.  The cross-entropy epilogues (inexact by nature) are reached by the fused
linear + cross-entropy entries at the smallest shape test_fused_linear_cross_entropy* value-tests."""
import ctypes
import os
import re
import shutil
import sys

import pytest
import torch

import gemm_exact_util as GX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, 'profiles', 'gemm_exact_routes.txt')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
CASES = GX.all_cases()
GROUPS = sorted({GX.group_of(c) for c in CASES})

# the kernels no exact-sum case can reach: the cross-entropy epilogues (EPI 2 / 3) and the two reductions behind them
CE_ONLY = re.compile(r'gemm_nt_256_kernel<false, [23],|gemm_nt_256x3_kernel<[23],|ce_combine_kernel|ce_mean_kernel')
# kernel -> (tile rows, tile columns, fewest K the route admits), read off nt_route_plain / nt_route_f16ops / nt_long_k / nt_persistent /
# tn_route of gemm.hip.  TN: K counts token rows; the shift forms take two samples of 1 + frames * 16 rows, so 34 at least.
RULES = [
    (r'gemm_nt_kernel<\w+, false', 128, 128, 8), (r'gemm_nt_kernel<\w+, true', 128, 128, 32), (r'gemm_nt_glds_kernel', 128, 128, 32),
    (r'gemm_nt_256_kernel<\w+, \d, 4, 4, 1', 256, 256, 32), (r'gemm_nt_256_kernel<\w+, \d, 1, 4, 4', 256, 256, 64),
    (r'gemm_nt_256p_kernel', 256, 256, 96), (r'gemm_nt_256x3_kernel', 256, 256, 32),
    (r'gemm_nt_w4k_kernel<\d, false', 256, 256, 64), (r'gemm_nt_w4k_kernel<\d, true', 256, 256, 96), (r'gemm_nt_rows_kernel', 8, 16, 8),
    (r'gemm_tn_kernel<\w+, false', 128, 128, 1), (r'gemm_tn_kernel<\w+, true', 128, 128, 34),
    (r'gemm_tn_glds_kernel<false', 128, 128, 1), (r'gemm_tn_glds_kernel<true', 128, 128, 34),
    (r'gemm_tn_256_kernel<false', 256, 256, 1), (r'gemm_tn_256_kernel<true', 256, 256, 34), (r'gemm_tn_w4k_kernel', 256, 256, 128),
    (r'gemm_tn_wm_kernel', 128, 64, 1), (r'gemm_tn_wmf_kernel', 128, 64, 32),
]
MAX_MN, MAX_K = 2200, 2752


def test_descriptor_is_the_librarys():
    from nuwa_pytorch_amd import _lib
    assert [(n, t) for n, t in GX.GemmDesc._fields_] == [(n, t) for n, t in _lib.GemmDesc._fields_]
    assert ctypes.sizeof(GX.GemmDesc) == ctypes.sizeof(_lib.GemmDesc)


def test_case_list_shape():
    assert len(CASES) >= 300 and len(GROUPS) >= 15
    for c in CASES:
        assert set(c) == set(GX.CASE_KEYS)
        assert c['alpha'] in (1.0, 0.5, 2.0) and c['beta'] in (0.0, 1.0) and c['adev'] in (None, 0.25)
        assert 1 <= c['hmax'] <= 4
        if c['frames']:
            assert (c['K'] if c['entry'] == GX.TN else c['M']) == 2 * GX.ntok_of(c)


@pytest.mark.parametrize('group', GROUPS)
def test_exactness_conditions(group):
    """S / lsb <= 2^22 after the bias and the old C, no lo x lo product, every operand value exact and normal in its 16-bit type, every
    expected value an fp32 number, every non-zero value of a 16-bit float output normal and finite in that type, and the product a gate
    reads back from its stored form exactly representable in it"""
    worst = 0.0
    for c in (c for c in CASES if GX.group_of(c) == group):
        o = GX.operands(c)
        e = GX.exactness(c, o)
        assert e['normal'], c['name']
        assert e['lolo'] == 0.0, c['name']
        assert e['span'] <= GX.SPAN_BITS, (c['name'], e['span'])
        worst = max(worst, e['span'])
        r = GX.result(c, o)
        assert bool((r.float().double() == r).all()), c['name']
        nz = r[r != 0].abs()
        if c['out'] != 'f32' and nz.numel():
            lo, hi = (2.0 ** -14, GX.F16_MAX) if c['out'] in ('f16', 'bf16+f16') else (2.0 ** -126, 3.0e38)
            assert float(nz.min()) >= lo and float(nz.max()) <= hi, (c['name'], float(nz.min()), float(nz.max()))
        if c['geglu'] and not c['acc_gate']:
            assert torch.equal(GX.stored_product(c, r), r), c['name']
        for name, t in GX.stored(c, o).items():
            rows, cols, ld, dt = GX.geometry(c)[name]
            assert tuple(t.shape) == (c['batch'] * rows if name in ('A', 'Alo', 'B', 'Blo') else rows, cols) and t.dtype == dt, (c['name'], name)
    print(f'{group}: worst span 2^{worst:.1f}')


# ---------------------------------------------------------------------------------------------------
# completeness: the launch-log walk
# ---------------------------------------------------------------------------------------------------
def walk(lib_path):
    """-> (kernels of gemm.hip, rows): one row per case = (name, case or None, return code, launched kernels, gate kernel calls, split-K slabs)"""
    sys.path.insert(0, os.path.join(ROOT, 'tools', 'launch_log'))
    try:
        import run as LR
        import cases_gemm_exact as CG
    finally:
        sys.path.pop(0)
    names, kernels = LR.symbols(lib_path)
    L = ctypes.CDLL(lib_path)
    L.launch_log_take.restype = ctypes.c_size_t
    L.launch_log_take.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
    tuning = (ctypes.c_int * 32).in_dll(L, 'g_amdnuwa_tuning')
    buf = ctypes.create_string_buffer(1 << 16)
    by_name = {c['name']: c for c in CASES}
    rows = []
    for name, keys, call in CG.cases(L):
        for k in range(32):
            tuning[k] = keys.get(k, 0)
        c = by_name.get(name)
        slabs = 0
        if c is not None and c['entry'] == GX.TN:
            d = GX.desc_of(c, GX.FAKE)
            slabs = L.amdnuwa_gemm_tn_workspace_bytes(ctypes.byref(d)) // (c['batch'] * c['M'] * c['N'] * 4)
        rc = call()
        n = L.launch_log_take(buf, len(buf))
        assert n < len(buf)
        body = re.sub(r'\+0x([0-9a-f]+)', lambda m: names.get(int(m.group(1), 16), m.group(0)), buf.value.decode())
        launched = [ln[len('launch '):ln.index(' grid ')] for ln in body.splitlines() if ln.startswith('launch ')]
        extern = [ln.split(' ')[1] for ln in body.splitlines() if ln.startswith('extern ')]
        rows.append((name, c, rc, launched, extern, slabs))
    for k in range(32):
        tuning[k] = 0
    return kernels, rows


def short(kernel):
    return re.sub(r'^void |\(.*$', '', kernel)


def table_text(kernels, rows):
    seen = {}
    lines = ['# case -> kernels, written by tests/test_gemm_exact_cpu.py::test_every_instantiation_is_reached (launch-log walk of gemm.hip, no GPU)',
             '# columns: return code | split-K slabs (TN) | tuning keys | case | launches (+ stand-alone gate kernel)']
    for name, c, rc, launched, extern, slabs in rows:
        for kn in launched:
            seen[kn] = seen.get(kn, 0) + 1
        keys = ','.join(f'{k}={v}' for k, v in sorted(c['keys'].items())) if c else ''
        lines.append(f'{rc} | {slabs or "-"} | {keys or "-"} | {name} | {" ; ".join(short(k) for k in launched)}{" + " + extern[0] if extern else ""}')
    lines.append(f'# {len(kernels)} kernel instantiations, launches per instantiation:')
    lines += [f'# {seen.get(kn, 0):5d}  {short(kn)}' for kn in sorted(kernels)]
    never = sorted(short(k) for k in kernels - set(seen))
    lines.append('# never launched: ' + (', '.join(never) if never else 'none'))
    return '\n'.join(lines) + '\n'


@pytest.fixture(scope='module')
def walked(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which('hipcc')):
        pytest.skip('hipcc is not installed')
    sys.path.insert(0, os.path.join(ROOT, 'tools', 'launch_log'))
    try:
        import run as LR
        import cases_gemm_exact as CG
    finally:
        sys.path.pop(0)
    return walk(LR.build(ROOT, CG.SOURCE, CG.STUBS, str(tmp_path_factory.mktemp('launch_log')), []))


def test_every_case_launches(walked):
    kernels, rows = walked
    assert len(rows) == len(CASES) + 3
    bad = [(name, rc) for name, c, rc, launched, extern, slabs in rows if rc != 0 or not launched]
    assert not bad, bad[:8]
    for name, c, rc, launched, extern, slabs in rows:
        if c is None:
            continue
        # a case that says its gate runs on the accumulators is inside one GEMM launch; a decomposed gate is one stand-alone kernel call
        if c['acc_gate']:
            assert len(launched) == 1 and not extern, name
        assert len(extern) <= 1 and (not extern or c['geglu']), name
        assert all(not CE_ONLY.search(k) for k in launched), name


def test_every_instantiation_is_reached(walked):
    kernels, rows = walked
    assert len(kernels) == 75
    text = table_text(kernels, rows)
    try:
        with open(TABLE, 'w') as f:
            f.write(text)
    except OSError:
        pass
    assert text.endswith('# never launched: none\n'), text[text.rindex('# never launched'):]
    reach = {kn: [] for kn in kernels}
    for name, c, rc, launched, extern, slabs in rows:
        for kn in launched:
            reach[kn].append((name, c, slabs))
    problems = []
    for kn, hits in sorted(reach.items()):
        if CE_ONLY.search(kn):
            if not any(c is None for _, c, _ in hits):
                problems.append(f'{short(kn)}: not reached by the linear + cross-entropy entries')
            continue
        cs = [c for _, c, _ in hits if c is not None]
        persistent = 'gemm_nt_256p_kernel' in kn
        small = [c for c in cs if c['K'] <= MAX_K and (persistent or max(c['M'], c['N']) <= MAX_MN)]
        if len(small) < 2:
            problems.append(f'{short(kn)}: {len(small)} case(s)')
        if 'splitk_reduce_kernel' in kn:
            if not any(s > 1 and c is not None and c['beta'] != 0 for _, c, s in hits):
                problems.append('splitk_reduce_kernel: no case with several splits and beta != 0')
            continue
        rule = [r for r in RULES if re.search(r[0], kn)]
        assert len(rule) == 1, kn
        _, tm, tn, kmin = rule[0]
        if not any(c['M'] % tm and c['N'] % tn for c in small):
            problems.append(f'{short(kn)}: no case with M and N off the {tm} x {tn} tile')
        if not any(c['K'] == kmin for c in small):
            problems.append(f'{short(kn)}: no case at K = {kmin}, the shortest main loop (has {sorted({c["K"] for c in small})})')
    assert not problems, '\n'.join(problems)


def test_persistent_ring_walks_a_second_round(walked):
    """one case of 257 to 300 ragged tiles with K = 96 per operand form: more tiles than workgroups, the last round partly filled"""
    kernels, rows = walked
    for f16 in ('false', 'true'):
        hit = [c for name, c, rc, launched, extern, slabs in rows if c is not None and any(f'gemm_nt_256p_kernel<' in k and f', {f16}>' in k for k in launched)
               and 257 <= -(-c['M'] // 256) * -(-c['N'] // 256) <= 300 and c['K'] == 96 and c['M'] % 256 and c['N'] % 256]
        assert hit, f16
