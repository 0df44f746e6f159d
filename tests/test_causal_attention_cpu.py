"""Plain causal self-attention (np.py:315-379 with causal=True, no context) without a GPU: the oracle against the reference module and
against the committed reference fixture g14, the product module's torch-op path against the oracle, and the argument checks of the
amdnuwa_cattn_* entry points."""
import ctypes

import pytest
import torch

from golden_util import load, rel_err
from oracle import nuwa_oracle as O

CASES = [(2, 32, 37), (8, 64, 130), (3, 32, 65)]


def _mask(b, n, seed):
    g = torch.Generator().manual_seed(seed)
    mask = torch.rand(b, n, generator=g) > 0.3
    mask[-1, :2] = False
    return mask


def _oracle_run(P0, heads, x0, mask, dy):
    P = {k: v.detach().clone().requires_grad_(True) for k, v in P0.items()}
    x = x0.detach().clone().requires_grad_(True)
    y = O.attention(x, P, heads, mask=mask, causal=True)
    y.backward(dy)
    return y.detach(), x.grad, {k: v.grad for k, v in P.items()}


@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('heads,dh,n', CASES)
def test_oracle_causal_attention_equals_the_reference(reference_pkg, heads, dh, n, masked):
    """O.attention(..., causal=True) against the reference's Attention(causal=True): output, dx and every parameter gradient, 1e-6 relative"""
    from nuwa_pytorch.nuwa_pytorch import Attention
    torch.manual_seed(0)
    dim = 48
    m = Attention(dim=dim, heads=heads, dim_head=dh, causal=True)
    torch.manual_seed(1)
    x = torch.randn(2, n, dim, requires_grad=True)
    mask = _mask(2, n, 2) if masked else None
    y_ref = m(x, mask=mask)
    dy = torch.randn_like(y_ref)
    y_ref.backward(dy)
    y, dx, G = _oracle_run(m.state_dict(), heads, x, mask, dy)
    assert rel_err(y, y_ref.detach()) <= 1e-6
    assert rel_err(dx, x.grad) <= 1e-6
    for k, p in m.named_parameters():
        assert rel_err(G[k], p.grad) <= 1e-6, k


@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('heads,dh,n', CASES)
def test_product_module_on_cpu_tensors_equals_the_oracle(heads, dh, n, masked):
    """off the GPU Attention(causal=True) keeps its torch-op formulation: same result as the oracle (fp32 summation order apart)"""
    import nuwa_pytorch_amd as A
    torch.manual_seed(0)
    dim = 48
    m = A.Attention(dim=dim, heads=heads, dim_head=dh, causal=True)
    torch.manual_seed(1)
    x = torch.randn(2, n, dim, requires_grad=True)
    mask = _mask(2, n, 2) if masked else None
    y = m(x, mask=mask)
    dy = torch.randn_like(y)
    y.backward(dy)
    y_ref, dx_ref, G = _oracle_run(m.state_dict(), heads, x, mask, dy)
    assert rel_err(y.detach(), y_ref) <= 1e-5
    assert rel_err(x.grad, dx_ref) <= 1e-5
    for k, p in m.named_parameters():
        assert rel_err(p.grad, G[k]) <= 1e-5, k


def test_oracle_reproduces_the_reference_fixture():
    """tests/golden/g14_causal_attention.npz (written from the reference by tests/golden/make_golden_causal.py)"""
    Ar, P, G = load('g14_causal_attention')
    assert tuple(Ar['x'].shape) == (2, 70, 32) and int(Ar['heads']) == 2
    y, dx, Gn = _oracle_run(P, 2, Ar['x'], Ar['mask'], Ar['dy'])
    assert rel_err(y, Ar['y']) <= 1e-6
    assert rel_err(dx, Ar['dx']) <= 1e-6
    assert set(G) == set(Gn)
    for k, g in G.items():
        assert rel_err(Gn[k], g) <= 1e-6, k


def test_cattn_argument_validation_without_gpu():
    """amdnuwa_cattn_supported / _fwd / _bwd reject bad descriptors before touching the device: a null geometry and null operands are
    AMDNUWA_ERR_ARG (-1), dim_head 48 and heads 9 AMDNUWA_ERR_UNSUPPORTED (-2), a short workspace AMDNUWA_ERR_WORKSPACE (-3)"""
    from nuwa_pytorch_amd import _lib
    L = _lib.lib()
    ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
    fwd_null = (None, 0, None, None, 0, None, None, None, None, None, None, 0, 0, None, 0, None)
    bwd_null = (None, 0, None, None, 0, None, 0, None, None, None, None, None, None, 0, None, None, 0, None, None, None, None, 0, None)
    assert L.amdnuwa_cattn_supported(None) == 0
    assert L.amdnuwa_cattn_fwd(None, *fwd_null) == ARG
    assert L.amdnuwa_cattn_bwd(None, *bwd_null) == ARG
    assert L.amdnuwa_cattn_bwd_workspace_bytes(None) == 0

    def geom(heads, dh, B=2, n=70):
        g = _lib.CGeom()
        g.B, g.n, g.heads, g.dim_head, g.scale, g.causal = B, n, heads, dh, dh ** -0.5, 1
        return g
    for g in (geom(8, 48), geom(9, 64), geom(0, 64)):
        assert L.amdnuwa_cattn_supported(ctypes.byref(g)) == 0
        assert L.amdnuwa_cattn_fwd(ctypes.byref(g), *fwd_null) == UNSUPPORTED
        assert L.amdnuwa_cattn_bwd(ctypes.byref(g), *bwd_null) == UNSUPPORTED
        assert L.amdnuwa_cattn_bwd_workspace_bytes(ctypes.byref(g)) == 0
    for g in (geom(8, 64, B=0), geom(8, 64, n=0)):          # an empty geometry
        assert L.amdnuwa_cattn_supported(ctypes.byref(g)) == 0
        assert L.amdnuwa_cattn_fwd(ctypes.byref(g), *fwd_null) == ARG
    for heads, dh, n in ((8, 64, 2561), (1, 32, 1), (5, 32, 129)):
        g = geom(heads, dh, n=n)
        assert L.amdnuwa_cattn_supported(ctypes.byref(g)) == 1
        assert L.amdnuwa_cattn_fwd(ctypes.byref(g), *fwd_null) == ARG             # null operands
        assert L.amdnuwa_cattn_bwd(ctypes.byref(g), *bwd_null) == ARG
        # linear in n: far below one fp32 score array
        assert 0 < L.amdnuwa_cattn_bwd_workspace_bytes(ctypes.byref(g)) < 2 * n * 8 * (8 + 8 + 8) * 4 + (1 << 20)
    # a workspace that is too small is reported as such (operands are only checked for NULL: nothing is dereferenced)
    g = geom(2, 32)
    one = ctypes.c_void_p(16)
    args = [one, 64, one, one, 128, one, 64, None, one, one, one, one, one, 64, one, one, 128, one, one, one, one, 8, None]
    assert L.amdnuwa_cattn_bwd(ctypes.byref(g), *args) == WORKSPACE
    args[4] = 60                                                                  # ldkv not a multiple of 8
    assert L.amdnuwa_cattn_bwd(ctypes.byref(g), *args) == ARG
