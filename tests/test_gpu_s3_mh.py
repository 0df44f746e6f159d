"""The many-head Sparse3DNA window kernels (csrc/sparse3dna_mh.hip, 9 .. 16 heads) against float64 on the MI355X: the cases of
tests/s3_mh_cases_util.py -- the narrowest tiles (fewer threads than (g, h) pairs: 64 and 128 threads at 16 heads, idle lanes at 9), one full
tile, several tiles with a partial last one, sequences that end mid-row / at a row end / after one token (a tile wholly beyond the sequence
writes zero partials), dilation, flat and column-free windows, the relative-position bias -- each through kernels.sparse3dna_mh_fwd / _bwd
with its operands in guarded buffers and the calls inside guard(K), so every buffer the wrappers allocate (outputs, workspace) starts as NaN.

Reference: peaked_util.sparse3dna_core64 and its autograd gradients on the values the operands hold, computed once per (data, form) and
shared.  Metric: gpu_util.report (max-abs error over max-abs reference).  Tolerances, the project's for the form (s3_cases_util.tolerances)
with dW_th at 1e-4 in both forms:   bf16: o 2^-7, gradients 2^-6, dW_th 1e-4;   hi + lo: o 3e-5, gradients 5e-5, dW_th 1e-4.
Also per case: a second run repeats its bits; the <bos> row outputs its own value row and has dq = 0; results are finite and the guard bands
untouched.  tests/test_s3_mh_index_walk_cpu.py walks every index of exactly these cases on the CPU."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import peaked_util as PU  # noqa: E402
import s3_cases_util as SC  # noqa: E402
import s3_mh_cases_util as M  # noqa: E402
from gpu_util import report  # noqa: E402
from guard_util import guard, guarded  # noqa: E402

CASES = M.all_cases()
DEV = 'cuda'
NEW_SYMBOLS = ('amdnuwa_s3mh_supported', 'amdnuwa_sparse3dna_mh_bwd_workspace_bytes', 'amdnuwa_sparse3dna_mh_fwd', 'amdnuwa_sparse3dna_mh_bwd')


@pytest.fixture(scope='module')
def K():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import nuwa_pytorch_amd  # noqa: F401
    from nuwa_pytorch_amd import _lib, build, kernels
    # before the first launch: the loaded library is not older than any file under csrc/ (build.py's staleness rule) and has the new entries
    L = _lib.lib()
    path = getattr(L, '_name', None) or build.LIB
    deps = [os.path.join(build.CSRC, f) for f in os.listdir(build.CSRC)]
    assert not build._stale(path, deps), f'{path} is older than a file under {build.CSRC}: rebuild before launching'
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
    return kernels


def tolerances(c):
    t = SC.tolerances(c)
    t['dwth'] = 1e-4
    return t


_REF = {}


def reference(c, wth=None):
    """inputs (s3_cases_util.inputs: the values the operands of the form hold) and float64 results of a case, computed once and read-only"""
    key = (SC._seed(c), SC.value_form(c), c['bias'], None if wth is None else 'blockdiag')
    if key not in _REF:
        I = SC.inputs(c)
        if wth is not None:
            I['wth'] = wth
        leaf = lambda t: t.double().requires_grad_(True)
        Lf = dict(qkv=leaf(I['qkv']), wth=leaf(I['wth']))
        if I['rel'] is not None:
            Lf['rel'] = leaf(I['rel'])
        o = PU.sparse3dna_core64(Lf['qkv'][:, :, 0], Lf['qkv'][:, :, 1], Lf['qkv'][:, :, 2], Lf['wth'], SC.table(c), c['dim_head'] ** -0.5,
                                 rel=Lf.get('rel'))
        names = list(Lf)
        gr = dict(zip(names, torch.autograd.grad(o, [Lf[k] for k in names], I['do'].double())))
        E = dict(o=o.detach(), dq=gr['qkv'][:, :, 0], dk=gr['qkv'][:, :, 1], dv=gr['qkv'][:, :, 2], dwth=gr['wth'])
        if 'rel' in gr:
            E['drel'] = gr['rel']
        _REF[key] = dict(I=I, E=E)
    return _REF[key]


def _pair(K, t, hilo):
    hi = t.to(torch.bfloat16)
    lo = (t - hi.float()).to(torch.bfloat16) if hilo else None
    return K.BF(guarded(hi.contiguous(), device=DEV), guarded(lo.contiguous(), device=DEV) if hilo else None)


def run(K, c, I, heads=None, cols=None, mh=True):
    """one forward + backward through the kernels.py wrappers -> (values by name on the CPU, raw output arrays, the workspace as floats).
    heads / cols: run on a slice of the heads (the 8-head halves of the block-diagonal comparison, mh=False: the existing entry points)"""
    B, n, d = c['B'], c['ntok'], c['dim_head']
    h = c['heads'] if heads is None else heads
    inner, hilo = h * d, c['form'] == 'hilo'
    qkv_v, do_v, wth_v = I['qkv'], I['do'], I['wth']
    if cols is not None:
        qkv_v, do_v, wth_v = qkv_v[:, :, :, cols], do_v[:, :, cols], wth_v[cols][:, cols]
    wth = guarded(wth_v.contiguous(), device=DEV)
    rel = guarded(torch.cat((torch.zeros(1, h), I['rel'].t()), 0).contiguous(), device=DEV) if I['rel'] is not None else None
    g = K.s3_geom(B, n, c['grid'], c['window'], c['dilation'], h, d, causal=True)
    qkv, dO = _pair(K, qkv_v.reshape(B * n, 3 * inner), hilo), _pair(K, do_v.reshape(B * n, inner), hilo)
    fwd, bwd = (K.sparse3dna_mh_fwd, K.sparse3dna_mh_bwd) if mh else (K.sparse3dna_fwd, K.sparse3dna_bwd)
    made, real_ws = [], K.workspace

    def ws_spy(nbytes, device):
        made.append(real_ws(nbytes, device))
        return made[-1]
    K.workspace = ws_spy
    try:
        with guard(K) as gd:
            o = fwd(g, qkv, wth, rel_bias=rel)
            dqkv, dwth, drel = bwd(g, qkv, wth, dO, rel_bias=rel)
            assert gd.made() > 0
    finally:
        K.workspace = real_ws
    assert (o.lo is not None) == hilo and (dqkv.lo is not None) == hilo
    val = lambda p: (p.hi.float() + p.lo.float() if p.lo is not None else p.hi.float()).cpu()
    parts = lambda p: [t for t in (p.hi, p.lo) if t is not None]
    dv_ = val(dqkv).reshape(B, n, 3, h, d)
    out = dict(o=val(o).reshape(B, n, h, d), dq=dv_[:, :, 0], dk=dv_[:, :, 1], dv=dv_[:, :, 2], dwth=dwth.cpu())
    if drel is not None:
        out['drel'] = drel[1:].t().cpu()
    raw = [t.cpu() for t in parts(o) + parts(dqkv)] + [dwth.cpu()] + ([drel.cpu()] if drel is not None else [])
    ws = made[-1].cpu()
    return out, raw, ws[:ws.numel() // 4 * 4].view(torch.float32)


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _same_bits(xs, ys):
    return len(xs) == len(ys) >= 1 and all(a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b)) for a, b in zip(xs, ys))


@pytest.mark.parametrize('c', CASES, ids=[c['name'] for c in CASES])
def test_case_against_float64(K, c):
    g = K.s3_geom(c['B'], c['ntok'], c['grid'], c['window'], c['dilation'], c['heads'], c['dim_head'], causal=True)
    assert K.s3mh_supported(g, lo=c['form'] == 'hilo')
    R = reference(c)
    got, raw, ws = run(K, c, R['I'])
    _, raw2, _ = run(K, c, R['I'])
    want, tol = R['E'], tolerances(c)
    assert set(got) == set(want) == set(tol)
    for t in raw:
        assert bool(torch.isfinite(t.float()).all())
    errs = {}
    for nm in got:
        print(f'{c["name"]} {nm}: rel err {float((got[nm].double() - want[nm]).abs().max() / want[nm].abs().max().clamp(min=1e-30)):.3e} (tol {tol[nm]:.1e})')
    for nm in got:
        errs[nm] = report(f's3mh.{nm}[{c["name"]}]', got[nm], want[nm], tol[nm])
    # a second run repeats its bits
    assert _same_bits(raw, raw2)
    # the <bos> row outputs its own value row (the bits of the v operand) and has dq = 0
    v_held = R['I']['qkv'][:, 0, 2]
    assert torch.equal(got['o'][:, 0], v_held), 'the <bos> output row is not its own value row'
    assert bool((got['dq'][:, 0] == 0).all())
    # tiles wholly beyond the sequence: zero dW_th partials (the workspace started as NaN)
    F, H, W = c['grid']
    tw, nt, _ = M.tile(c)
    hh = c['heads'] * c['heads']
    pth = ws[M.part_th_offset(c):M.part_th_offset(c) + c['B'] * F * H * nt * hh].view(c['B'], F * H, nt, hh)
    assert bool(torch.isfinite(pth).all())
    beyond = 0
    for ry in range(F * H):
        for tl in range(nt):
            if ry * W + tl * tw + 1 >= c['ntok']:
                beyond += 1
                assert bool((pth[:, ry, tl] == 0).all()), (ry, tl)
    if c['ntok'] - 1 < F * H * W - W:
        assert beyond > 0


BLOCK_CASES = [c for c in CASES if c['heads'] == 16 and c['ntok'] == 1 + c['grid'][0] * c['grid'][1] * c['grid'][2] and not c['bias']
               and c['grid'] in ((2, 2, 2), (2, 3, 12)) and c['dilation'] == (1, 1, 1) and c['window'] == (3, 3, 3)]


@pytest.mark.parametrize('c', BLOCK_CASES, ids=[c['name'] for c in BLOCK_CASES])
def test_block_diagonal_mix_agrees_with_two_eight_head_calls(K, c):
    """16 heads whose talking-heads matrix is two 8 x 8 blocks are two independent 8-head attentions: the many-head kernels agree, within
    the form's tolerance, with the existing 8-head entry points on the head halves (and with float64)"""
    assert BLOCK_CASES
    gen = torch.Generator().manual_seed(5)
    wth = torch.zeros(16, 16)
    for s in (slice(0, 8), slice(8, 16)):
        wth[s, s] = torch.randn(8, 8, generator=gen) * 0.5 + torch.eye(8)
    R = reference(c, wth=wth)
    tol = tolerances(c)
    got, raw, _ = run(K, c, R['I'])
    for nm in ('o', 'dq', 'dk', 'dv'):
        report(f's3mh.block64.{nm}[{c["name"]}]', got[nm], R['E'][nm], tol[nm])
    for half, s in enumerate((slice(0, 8), slice(8, 16))):
        g8, raw8, _ = run(K, c, R['I'], heads=8, cols=s, mh=False)
        equal = True
        for nm in ('o', 'dq', 'dk', 'dv'):
            report(f's3mh.block8.{nm}[{c["name"]}, half {half}]', got[nm][:, :, s], g8[nm], tol[nm])
            equal = equal and torch.equal(got[nm][:, :, s], g8[nm])
        report(f's3mh.block8.dwth[{c["name"]}, half {half}]', got['dwth'][s, s], g8['dwth'], tol['dwth'])
        print(f'{c["name"]} half {half}: o / dq / dk / dv bits equal to the 8-head kernels: {equal}; '
              f'dW_th block bits equal: {torch.equal(got["dwth"][s, s], g8["dwth"])}')
