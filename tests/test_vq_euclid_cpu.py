"""CPU side of the Euclidean VQ lookup (no GPU): the inputs of tests/test_gpu_vq_euclid.py are decidable by the float64 judge, the
shifted ones tell a centred fp32 lookup from the expanded form around the origin, and the two C-ABI entry points exist and check
their arguments before they touch a device."""
import ctypes

import pytest

import vq_euclid_util as U


@pytest.mark.parametrize('case', U.CASES, ids=U.case_id)
def test_inputs_are_decidable_in_float64(case):
    """the condition the GPU tests rest on: at least 99 % of the rows have a top-2 gap above twice the fp32 bound"""
    _, _, _, sure, _, _ = U.judged(case)
    share = float(sure.double().mean())
    print(f'{U.case_id(case)}: sure share {share:.4f}')
    assert share >= 0.99


@pytest.mark.parametrize('case', U.SHIFTED, ids=U.case_id)
def test_shifted_inputs_tell_centred_from_uncentred_fp32(case):
    """fp32 around the origin (torch.cdist's expansion) mispicks at least 10 % of the sure rows, the same arithmetic around the codebook
    mean none, and its distance stays inside the bound: the inputs discriminate, and the bound is not what the code under test gives"""
    x, cb, idx64, sure, tol, d2 = U.judged(case)
    wrong_u = int((U.uncentred_f32(x, cb)[sure] != idx64[sure]).sum())
    ic, dc = U.centred_f32(x, cb)
    wrong_c = int((ic[sure] != idx64[sure]).sum())
    err = float(((dc.double() - d2).abs() / tol).max())
    print(f'{U.case_id(case)}: sure {int(sure.sum())}, uncentred wrong {wrong_u}, centred wrong {wrong_c}, centred |d - d64| / tol {err:.3e}')
    assert wrong_u >= 0.1 * int(sure.sum())
    assert wrong_c == 0
    assert err <= 1.0


def test_library_exports_the_euclidean_lookup():
    from nuwa_pytorch_amd import _lib
    from nuwa_pytorch_amd import build as B
    so = ctypes.CDLL(B.build(verbose=False))
    for name in ('amdnuwa_vq_nearest_l2', 'amdnuwa_vq_nearest_l2_workspace_bytes'):
        assert hasattr(so, name), name
        assert name in _lib.SIGNATURES, name


def test_euclidean_lookup_argument_validation_without_gpu():
    """bad arguments are rejected before the device is touched (host memory stands in for the operands: nothing reads it)"""
    from nuwa_pytorch_amd import _lib
    L = _lib.lib()
    ARG, WORKSPACE = -1, -3
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    R, Cn, Dc = 7, 33, 256
    nb = L.amdnuwa_vq_nearest_l2_workspace_bytes(R, Cn, Dc)
    assert nb > 0
    assert L.amdnuwa_vq_nearest_l2_workspace_bytes(0, Cn, Dc) == 0
    assert L.amdnuwa_vq_nearest_l2_workspace_bytes(R, 0, Dc) == 0
    assert L.amdnuwa_vq_nearest_l2_workspace_bytes(R, Cn, -1) == 0
    assert L.amdnuwa_vq_nearest_l2(None, p, p, None, R, Cn, Dc, p, nb, None) == ARG
    assert L.amdnuwa_vq_nearest_l2(p, None, p, None, R, Cn, Dc, p, nb, None) == ARG
    assert L.amdnuwa_vq_nearest_l2(p, p, None, None, R, Cn, Dc, p, nb, None) == ARG
    assert L.amdnuwa_vq_nearest_l2(p, p, p, None, R, 0, Dc, p, nb, None) == ARG
    assert L.amdnuwa_vq_nearest_l2(p, p, p, None, R, Cn, 0, p, nb, None) == ARG
    assert L.amdnuwa_vq_nearest_l2(p, p, p, None, R, Cn, 33, p, nb, None) == ARG           # odd code_dim
    assert L.amdnuwa_vq_nearest_l2(p, p, p, None, 0, Cn, Dc, None, 0, None) == 0           # no rows: nothing to do
    assert L.amdnuwa_vq_nearest_l2(p, p, p, None, R, Cn, Dc, None, nb, None) == WORKSPACE
    assert L.amdnuwa_vq_nearest_l2(p, p, p, None, R, Cn, Dc, p, nb - 1, None) == WORKSPACE
    assert b'workspace' in L.amdnuwa_error_string(WORKSPACE)
    # every slice's partial pairs, the prep pass's sums and ||x - mu||^2 fit: the size grows with each argument
    assert L.amdnuwa_vq_nearest_l2_workspace_bytes(2 * R, Cn, Dc) > nb
    assert L.amdnuwa_vq_nearest_l2_workspace_bytes(R, 2 * Cn, Dc) > nb
    assert L.amdnuwa_vq_nearest_l2_workspace_bytes(R, Cn, 2 * Dc) > nb
