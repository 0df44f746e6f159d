"""GEMM kernels against float64 bit for bit: the exact-sum cases of gemm_exact_util.py on the device.

Every product and partial sum of a case is an fp32 number (test_gemm_exact_cpu.py asserts the condition per case), so each output must
EQUAL the float64-derived expectation: an fp32 output the value, a bf16 / fp16 output its round-to-nearest-even, a hi + lo pair
hi = RNE(v), lo = RNE(v - hi), a bf16 + fp16 pair both renderings of v.  GEGLU gate outputs are compared per element against float64
erfc-GELU with the bound of row_inputs_util.  Operands and outputs live in guard_util buffers (NaN prefill, bands, pitch padding checked
after every case; the old C of a beta = 0 case is NaN), every case runs twice and must give the same bits, and no fp16 store saturates.
The case list reaches every kernel instantiation of gemm.hip but the cross-entropy epilogues (test_gemm_exact_cpu.py proves it)."""
import ctypes

import pytest
import torch

import gemm_exact_util as GX
import guard_util as GU
import row_inputs_util as RU

pytestmark = pytest.mark.gpu
DEV = 'cuda'
PER_TEST = 24
CASES = GX.all_cases()


def _chunks():
    by = {}
    for c in CASES:
        by.setdefault(GX.group_of(c), []).append(c)
    out = []
    for g, cs in sorted(by.items()):
        for i in range(0, len(cs), PER_TEST):
            out.append(pytest.param(cs[i:i + PER_TEST], id=f'{g.replace(" ", "-")}-{i // PER_TEST}'))
    return out


@pytest.fixture(scope='module')
def L():
    from nuwa_pytorch_amd import _lib
    return _lib.lib()


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


def _mismatch(name, got, want):
    bad = (_bits(got) != _bits(want)) & ~((got == 0) & (want == 0))           # (+0 and -0 are the same value)
    n = int(bad.sum())
    if n == 0:
        return None
    idx = bad.nonzero()[:6].tolist()
    return f'{name}: {n} of {bad.numel()} elements differ; first (i, j, got, want): ' + ', '.join(
        f'({i}, {j}, {float(got[i, j])!r}, {float(want[i, j])!r})' for i, j in idx)


def run_case(L, c):
    from nuwa_pytorch_amd import _lib
    o = GX.operands(c)
    geo = GX.geometry(c)
    buf = {}
    for name, t in GX.stored(c, o).items():
        buf[name] = GU.guarded(t.to(DEV), ld=geo[name][2], label=f'{c["name"]}: {name}')
    cold = o['cold'].float().reshape(-1, c['N']).to(DEV) if c['beta'] else None
    for name in GX.OUTPUTS:
        if name in geo:
            rows, cols, ld, dt = geo[name]
            t = torch.full((c['batch'] * rows, cols), float('nan'), dtype=dt, device=DEV)
            buf[name] = GU.guarded(cold if (name == 'C' and cold is not None) else t, ld=ld, label=f'{c["name"]}: {name}')
    ptr = {n: t.data_ptr() for n, t in buf.items()}
    d = GX.desc_of(c, ptr, _lib.GemmDesc)
    old = {k: L.amdnuwa_get_tuning(k) for k in c['keys']}
    try:
        for k, v in c['keys'].items():
            L.amdnuwa_set_tuning(k, v)
        fused = bool(L.amdnuwa_gemm_nt_fused(ctypes.byref(d))) if c['entry'] == GX.NT else False
        ws = None
        if c['entry'] == GX.TN:
            nb = L.amdnuwa_gemm_tn_workspace_bytes(ctypes.byref(d))
            ws = GU.guarded_empty((max(nb, 16),), torch.uint8, DEV, label=f'{c["name"]}: workspace')
            ptr['ws'] = ws.data_ptr()
        L.amdnuwa_f16_sat_count(1)
        runs = []
        for _ in range(2):
            if cold is not None:
                buf['C'].copy_(cold)
            rc = GX.call(L, c, ptr, _lib.GemmDesc, ws_bytes=None if ws is None else ws.numel())
            assert rc == 0, f'{c["name"]}: return code {rc}'
            torch.cuda.synchronize()
            runs.append({n: buf[n].clone() for n in GX.OUTPUTS if n in buf})
        sat = L.amdnuwa_f16_sat_count(1)
    finally:
        for k, v in old.items():
            L.amdnuwa_set_tuning(k, v)
    bad = GU.check_registry()
    assert not bad, f'{c["name"]}: ' + '; '.join(bad)
    got = runs[0]
    problems = [f'{n}: the second call gave other bits' for n in got if not torch.equal(_bits(got[n]), _bits(runs[1][n]))]
    exact, gates = GX.expected(c, o, fused, DEV)
    assert exact or gates, c['name']
    for n in got:
        if n in exact:
            m = _mismatch(n, got[n], exact[n].to(DEV))
            if m:
                problems.append(m)
        elif not any(n in names for names, *_ in gates):
            if not bool(torch.isnan(got[n].float()).all()):                  # (the GEGLU backward inside an epilogue leaves C alone)
                problems.append(f'{n}: written, although this form does not write it')
    for names, ref, bound, ok, omax in gates:
        val = sum(got[n].double() for n in names)
        if c['geglu'] == 'bwd':
            val = GX.deinterleave(val, c['N'])
        worst, fine = RU.geglu_errors(val, ref, bound, ok, omax)
        if not (fine and worst <= 1.0):
            problems.append(f'{"+".join(names)}: gate output off its bound: worst err / bound {worst:.3f}, finite where representable: {fine}')
    if sat:
        problems.append(f'amdnuwa_f16_sat_count = {sat}')
    assert not problems, f'{c["name"]} keys {c["keys"]}:\n  ' + '\n  '.join(problems)


@pytest.mark.parametrize('cases', _chunks())
def test_gemm_exact(L, cases):
    assert all(L.amdnuwa_get_tuning(k) == 0 for k in range(32))
    for c in cases:
        run_case(L, c)
    assert all(L.amdnuwa_get_tuning(k) == 0 for k in range(32))
