"""Every kernel instantiation of sparse3dna.hip and sparse3dna_wide.hip against float64 on the MI355X: the cases of tests/s3_cases_util.py
(tests/test_s3_cases_cpu.py shows without a GPU that they launch all 71 instantiations, every route of s3_route() and every edge of the
kernels' geometries), each through the kernels.py wrappers with its operands in guarded buffers and the calls inside guard(K).

Per case: the wrapper calls exactly the C entry points the case names, with the arguments the launch-log walk used (a recording proxy around
the library object reduces each call to s3_cases_util.call_shape); the results meet the tolerances the suite already applies to the form
(s3_cases_util.tolerances; metric gpu_util.report, max-abs error over max-abs reference); a second run repeats its bits; the <bos> row outputs
its own value row; under a mask the fully dropped queries output exactly 0 and have dq = 0, and an all-ones mask at drop_scale 1 gives the
bits of the unmasked call (under the two tuning keys that route a masked call to other kernels than the unmasked one, finite values)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import s3_cases_util as SC  # noqa: E402
from gpu_util import report  # noqa: E402

CASES = SC.all_cases()


@pytest.fixture(scope='module')
def K():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import nuwa_pytorch_amd  # noqa: F401
    from nuwa_pytorch_amd import kernels
    return kernels


@pytest.fixture
def spy(monkeypatch, K):
    """the library object behind kernels.py, wrapped: .calls lists the window entry points called, each as s3_cases_util.call_shape has it"""
    from nuwa_pytorch_amd import _lib
    rec = SC.Recorder(_lib.lib())
    monkeypatch.setattr(_lib, '_lib', rec)
    return rec


def _bits(t):
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _same_bits(xs, ys):
    assert len(xs) == len(ys) >= 1
    for a, b in zip(xs, ys):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize('c', CASES, ids=[c['name'] for c in CASES])
def test_case_against_float64(K, spy, c):
    L = spy._real
    masked = c['keep'] is not None
    R = SC.reference(c)
    keep, scale = (R['keep'], c['keep']) if masked else (None, 1.0)
    assert all(L.amdnuwa_get_tuning(k) == 0 for k in c['keys'])
    try:
        for k, v in c['keys'].items():
            L.amdnuwa_set_tuning(k, v)
        got, raw = SC.run(K, c, R, keep, scale)
        calls = list(spy.calls)
        _, raw2 = SC.run(K, c, R, keep, scale)
        if masked:
            R1 = SC.reference(c, masked=False)
            assert bool(R1['keep'].all())
            _, plain = SC.run(K, c, R1, None, 1.0)
            _, ones = SC.run(K, c, R1, R1['keep'], 1.0)
    finally:
        for k in c['keys']:
            L.amdnuwa_set_tuning(k, 0)
    # ---- the calls: the entry points the case names, with the arguments of the launch-log walk
    assert [n for n, _, _ in calls] == list(c['entries'])
    for name, gshape, args in calls:
        want_g, want_args = SC.call_shape(c, name, SC.workspace_bytes(L, c, name))
        assert gshape == want_g, (name, gshape, want_g)
        assert args == want_args, (name, [(a, b) for a, b in zip(args, want_args) if a != b])
    # ---- values
    want, tol = SC.expected(c, R), SC.tolerances(c)
    assert set(got) == set(want) == set(tol)
    errs = {nm: report(f's3every.{nm}[{c["name"]}]', got[nm], want[nm], tol[nm]) for nm in got}
    print(c['name'], {k: f'{v:.2e}' for k, v in errs.items()})
    # ---- a second run repeats its bits
    _same_bits(raw, raw2)
    assert all(bool(torch.isfinite(t.float()).all()) for t in raw)
    # ---- the <bos> row outputs its own value row
    if not c['cross'] and 'o' in got:
        assert torch.equal(got['o'][:, 0], R['I']['qkv'][:, 0, 2])
    if masked:
        # ---- the fully dropped queries output exactly 0 and have dq = 0
        (r0, _, _), tail = SC.special_rows(c)
        first = 0 if c['cross'] else 1                       # (the cross results start at query 1)
        for s, q in [r0] + ([tail] if tail else []):
            for nm in ('o', 'dq'):
                if nm in got:
                    assert float(got[nm][s, first + q].abs().max()) == 0.0, (nm, s, q)
        # ---- an all-ones mask at drop_scale 1 gives the bits of the unmasked call (where both take the same kernels: two tuning keys
        # route a masked call elsewhere, s3_cases_util.mask_keeps_route)
        if SC.mask_keeps_route(c):
            _same_bits(plain, ones)
        assert all(bool(torch.isfinite(t.float()).all()) for t in ones)
