"""Non-causal attention over more than 287 keys (np.py:315-379, the keys a context's rows or the query rows themselves) without a GPU:
the oracle against the reference module and against the committed reference fixture g15, the product module's torch-op path against the
oracle, and the rectangular geometry (amdnuwa_cattn_geom.n_keys, ABI 21) in the argument checks of the amdnuwa_cattn_* entry points."""
import ctypes

import pytest
import torch

from golden_util import load, rel_err
from oracle import nuwa_oracle as O

T_LONG = 300


def _oracle_run(P0, heads, x0, dy, context=None, context_mask=None, mask=None):
    P = {k: v.detach().clone().requires_grad_(True) for k, v in P0.items()}
    x = x0.detach().clone().requires_grad_(True)
    c = None if context is None else context.detach().clone().requires_grad_(True)
    y = O.attention(x, P, heads, context=c, context_mask=context_mask, mask=mask, causal=False)
    y.backward(dy)
    return y.detach(), x.grad, (None if c is None else c.grad), {k: v.grad for k, v in P.items()}


def _context_case(seed, dim, n=23):
    torch.manual_seed(seed)
    x = torch.randn(2, n, dim, requires_grad=True)
    context = torch.randn(2, T_LONG, dim, requires_grad=True)
    cmask = torch.rand(2, T_LONG) > 0.3
    cmask[1] = False                         # a sample whose every context token is masked attends the null key alone
    return x, context, cmask


@pytest.mark.parametrize('heads,dh', [(2, 32), (8, 64)])
def test_oracle_attention_with_a_long_context_equals_the_reference(reference_pkg, heads, dh):
    """O.attention(context of 300 keys, context mask) against the reference's Attention: output, dx, dcontext and every parameter
    gradient, 1e-6 relative"""
    from nuwa_pytorch.nuwa_pytorch import Attention
    torch.manual_seed(0)
    dim = 48
    m = Attention(dim=dim, heads=heads, dim_head=dh)
    x, context, cmask = _context_case(1, dim)
    y_ref = m(x, context=context, context_mask=cmask)
    dy = torch.randn_like(y_ref)
    y_ref.backward(dy)
    y, dx, dc, G = _oracle_run(m.state_dict(), heads, x, dy, context=context, context_mask=cmask)
    assert rel_err(y, y_ref.detach()) <= 1e-6
    assert rel_err(dx, x.grad) <= 1e-6
    assert rel_err(dc, context.grad) <= 1e-6
    for k, p in m.named_parameters():
        assert rel_err(G[k], p.grad) <= 1e-6, k


@pytest.mark.parametrize('heads,dh', [(2, 32), (8, 64)])
def test_oracle_long_self_attention_equals_the_reference(reference_pkg, heads, dh):
    """O.attention as non-causal self-attention over 300 rows with a key mask against the reference's Attention: output, dx and every
    parameter gradient, 1e-6 relative.
    One sample on one CPU thread.  The talking-heads weight gradient is ONE sum over all b * n * (T + 1) probabilities -- 90 300 terms of
    either sign here -- which the reference (the backward of a 1 x 1 convolution) and the oracle (that of an einsum) split over threads and
    samples in different ways; fp32 sums that long and that cancelling agree to about 1e-6 of their result between two orders (measured
    3e-7 ... 2.8e-6 over 1 / 4 / 16 threads, b = 1 / 2, three seeds: either side is that far from a float64 evaluation), so on many threads
    the comparison would measure the summation order at the level of the bound.  On one thread and one sample both reduce in the same
    order, and the bound tests the formulas."""
    from nuwa_pytorch.nuwa_pytorch import Attention
    torch.manual_seed(0)
    dim = 48
    m = Attention(dim=dim, heads=heads, dim_head=dh)
    torch.manual_seed(1)
    x = torch.randn(1, T_LONG, dim, requires_grad=True)
    mask = torch.rand(1, T_LONG) > 0.3
    mask[0, :5] = False
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        y_ref = m(x, mask=mask)
        dy = torch.randn_like(y_ref)
        y_ref.backward(dy)
        y, dx, _, G = _oracle_run(m.state_dict(), heads, x, dy, mask=mask)
    finally:
        torch.set_num_threads(threads)
    errs = dict(y=rel_err(y, y_ref.detach()), dx=rel_err(dx, x.grad), **{k: rel_err(G[k], p.grad) for k, p in m.named_parameters()})
    print({k: f'{v:.2e}' for k, v in errs.items()})
    for k, v in errs.items():
        assert v <= 1e-6, k


def test_oracle_reproduces_the_reference_fixture():
    """tests/golden/g15_long_attention.npz (written from the reference by tests/golden/make_golden_long_attention.py)"""
    Ar, P, G = load('g15_long_attention')
    assert tuple(Ar['x'].shape) == (2, 20, 32) and tuple(Ar['context'].shape) == (2, T_LONG, 32) and int(Ar['heads']) == 2
    assert not bool(Ar['context_mask'][1].any()) and bool(Ar['context_mask'][0].any())      # one sample has every context token masked
    y, dx, dc, Gn = _oracle_run(P, 2, Ar['x'], Ar['dy'], context=Ar['context'], context_mask=Ar['context_mask'])
    assert rel_err(y, Ar['y']) <= 1e-6
    assert rel_err(dx, Ar['dx']) <= 1e-6
    assert rel_err(dc, Ar['dcontext']) <= 1e-6
    assert set(G) == set(Gn)
    for k, g in G.items():
        assert rel_err(Gn[k], g) <= 1e-6, k


def test_product_module_on_cpu_tensors_equals_the_oracle():
    """off the GPU the module keeps its torch-op formulation for long key counts too: same result as the oracle (fp32 summation order apart)"""
    import nuwa_pytorch_amd as A
    torch.manual_seed(0)
    dim = 48
    m = A.Attention(dim=dim, heads=2, dim_head=32)
    x, context, cmask = _context_case(1, dim)
    y = m(x, context=context, context_mask=cmask)
    dy = torch.randn_like(y)
    y.backward(dy)
    y_ref, dx_ref, dc_ref, G = _oracle_run(m.state_dict(), 2, x, dy, context=context, context_mask=cmask)
    assert rel_err(y.detach(), y_ref) <= 1e-5
    assert rel_err(x.grad, dx_ref) <= 1e-5
    assert rel_err(context.grad, dc_ref) <= 1e-5
    for k, p in m.named_parameters():
        assert rel_err(p.grad, G[k]) <= 1e-5, k


def test_long_key_predicate_without_gpu(monkeypatch):
    """Attention._long_hip_ok: non-causal, more than 287 keys, heads <= 8, dim_head 32 / 64, no attention dropout in training, not the
    parity mode -- disjoint from _hip_ok (at most 287 keys) at every key count -- and, the whole shape given, at least long_pairs_min
    (query, key) pairs and long_wgs_min workgroups of 64 rows on either side (the measured speed crossover)"""
    import nuwa_pytorch_amd as A
    from nuwa_pytorch_amd.nuwa_pytorch import Attention
    prev = A.get_precision()
    try:
        A.set_precision('bf16')
        m = A.Attention(dim=64, heads=2, dim_head=32)
        assert m._hip_ok(287) and not m._long_hip_ok(287) and not m._long_hip_ok(287, 4096, 64)
        assert m._long_hip_ok(288) and not m._hip_ok(288)
        assert m._long_hip_ok(4096)
        # as shipped: b = 8, 1024 x 1024 is routed; fewer pairs or fewer workgroups on one side are not
        assert m._long_hip_ok(1024, 1024, 8) and m._long_hip_ok(1024, 2561, 8)
        assert not m._long_hip_ok(1023, 1023, 8) and not m._long_hip_ok(1024, 1024, 2) and not m._long_hip_ok(512, 2561, 8)
        assert not m._long_hip_ok(1024, 8192, 1) and not m._long_hip_ok(300, 20, 2)
        monkeypatch.setattr(Attention, 'long_pairs_min', 0)
        monkeypatch.setattr(Attention, 'long_wgs_min', 0)
        assert m._long_hip_ok(288, 1, 1) and not m._long_hip_ok(287, 1, 1)
        assert not A.Attention(dim=64, heads=2, dim_head=32, causal=True)._long_hip_ok(300, 300, 2)
        assert not A.Attention(dim=64, heads=9, dim_head=32)._long_hip_ok(300, 300, 2)
        assert not A.Attention(dim=64, heads=2, dim_head=48)._long_hip_ok(300, 300, 2)
        d = A.Attention(dim=64, heads=2, dim_head=32, dropout=0.1)
        assert not d.train()._long_hip_ok(300, 300, 2) and d.eval()._long_hip_ok(300, 300, 2)
        A.set_precision('bf16x3')
        assert not m._long_hip_ok(300, 300, 2)          # the parity mode keeps the torch-op formulation
    finally:
        A.set_precision(prev)


def test_cattn_rectangular_geometry_without_gpu():
    """amdnuwa_cattn_geom.n_keys (ABI 21): n_keys != n is accepted with causal = 0 and rejected with causal = 1 (AMDNUWA_ERR_UNSUPPORTED,
    -2) by _supported / _fwd / _bwd; n_keys = 0 and n_keys = n are self-attention; a negative count is an argument error.  The backward's
    workspace holds per-QUERY-row arrays and the partials of the ceil(n / 64) query-stationary workgroups (the key-stationary sweeps leave
    none): it follows n, not n_keys, and a call with less is AMDNUWA_ERR_WORKSPACE (-3)"""
    from nuwa_pytorch_amd import _lib
    from nuwa_pytorch_amd import kernels as K
    L = _lib.lib()
    ARG, UNSUPPORTED, WORKSPACE = -1, -2, -3
    assert L.amdnuwa_abi_version() == 21
    fwd_null = (None, 0, None, None, 0, None, None, None, None, None, None, 0, 0, None, 0, None)
    bwd_null = (None, 0, None, None, 0, None, 0, None, None, None, None, None, None, 0, None, None, 0, None, None, None, None, 0, None)
    ws = lambda g: L.amdnuwa_cattn_bwd_workspace_bytes(ctypes.byref(g))

    for heads, dh, n, T in ((8, 64, 1, 300), (8, 64, 600, 289), (8, 64, 64, 1000), (2, 32, 70, 513), (5, 32, 129, 320)):
        g = K.cattn_geom(2, n, heads, dh, causal=False, n_keys=T)
        assert g.n_keys == T and K.cattn_keys(g) == T
        assert L.amdnuwa_cattn_supported(ctypes.byref(g)) == 1
        assert L.amdnuwa_cattn_fwd(ctypes.byref(g), *fwd_null) == ARG              # a valid geometry: the null operands are what is wrong
        assert L.amdnuwa_cattn_bwd(ctypes.byref(g), *bwd_null) == ARG
        # the same workspace as self-attention over n rows, whatever the key count; far below one fp32 score array
        assert ws(g) == ws(K.cattn_geom(2, n, heads, dh, causal=False)) > 0
        assert ws(g) < 2 * n * 8 * (8 + 8 + 8) * 4 + (1 << 20)
        c = K.cattn_geom(2, n, heads, dh, causal=True, n_keys=T)
        assert L.amdnuwa_cattn_supported(ctypes.byref(c)) == 0
        assert L.amdnuwa_cattn_fwd(ctypes.byref(c), *fwd_null) == UNSUPPORTED
        assert L.amdnuwa_cattn_bwd(ctypes.byref(c), *bwd_null) == UNSUPPORTED
        assert ws(c) == 0
    # the workspace grows with the query side: per-row arrays and one partial block per 64 query rows
    small, large = K.cattn_geom(2, 64, 8, 64, causal=False, n_keys=1000), K.cattn_geom(2, 1000, 8, 64, causal=False, n_keys=64)
    assert ws(large) > ws(small)
    assert ws(large) - ws(small) >= 2 * (1000 - 64) * (8 + 8 + 8) * 4
    # n_keys = 0 and n_keys = n mean self-attention, causal or not
    g = K.cattn_geom(2, 70, 2, 32, causal=True, n_keys=70)
    assert g.n_keys == 0 and L.amdnuwa_cattn_supported(ctypes.byref(g)) == 1
    raw = _lib.CGeom()
    raw.B, raw.n, raw.heads, raw.dim_head, raw.scale, raw.causal, raw.n_keys = 2, 70, 2, 32, 32 ** -0.5, 1, 70
    assert L.amdnuwa_cattn_supported(ctypes.byref(raw)) == 1
    raw.n_keys = -1
    assert L.amdnuwa_cattn_supported(ctypes.byref(raw)) == 0
    assert L.amdnuwa_cattn_fwd(ctypes.byref(raw), *fwd_null) == ARG
    # a workspace that is too small is reported as such for the rectangular form (operands are only checked for NULL)
    g = K.cattn_geom(2, 70, 2, 32, causal=False, n_keys=513)
    one = ctypes.c_void_p(16)
    args = [one, 64, one, one, 128, one, 64, None, one, one, one, one, one, 64, one, one, 128, one, one, one, one, 8, None]
    assert L.amdnuwa_cattn_bwd(ctypes.byref(g), *args) == WORKSPACE
