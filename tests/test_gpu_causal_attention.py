"""Causal (and plain non-causal) self-attention on the linear-memory cattn kernels (csrc/cattn.hip), on the MI355X: the kernels against
the oracle's attention_core, causality, determinism, the module against the reference fixture g14 and the oracle, the fused decoder blocks of
Transformer / ReversibleTransformer(causal=True) with plain attention, the routing guards, and the memory bound that separates the kernels
from the torch-op formulation.

Tolerances (max-abs error / max-abs reference, gpu_util.report): kernel level fp16 forward 1e-3 (as test_gpu_kernels.py's fp16 cores), bf16
forward 2e-2, bf16 backward 7e-2; module level the MODES of test_gpu_modules.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from golden_util import load  # noqa: E402
from gpu_util import report  # noqa: E402

DEV = 'cuda'
MODES = [('bf16x3', 1e-3, 2e-3), ('bf16x3-fwd', 1e-3, 7e-2), ('bf16', 2e-2, 7e-2)]
GEOMS = [(8, 64, 1), (8, 64, 33), (8, 64, 257), (8, 64, 600), (2, 32, 70), (5, 32, 129), (3, 64, 64)]


@pytest.fixture(scope='module')
def K():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from nuwa_pytorch_amd import kernels
    return kernels


@pytest.fixture(scope='module')
def A():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import nuwa_pytorch_amd
    return nuwa_pytorch_amd


@pytest.fixture(scope='module')
def O():
    from oracle import nuwa_oracle
    return nuwa_oracle


def _inputs(B, n, heads, dh, dt, masked, seed=17):
    torch.manual_seed(seed)
    inner = heads * dh
    q = torch.randn(B * n, inner).to(dt)
    kv = torch.randn(B * n, 2 * inner).to(dt)
    nk, nv = torch.randn(heads, dh), torch.randn(heads, dh)
    wth = torch.randn(heads, heads) * 0.5 + torch.eye(heads)
    mask = None
    if masked:
        mask = torch.rand(B, n) > 0.3
        mask[0] = False                    # a fully masked sample attends only the null key
    return q, kv, nk, nv, wth, mask


@pytest.mark.parametrize('heads,dh,n', GEOMS)
@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('f16', [True, False])
@pytest.mark.parametrize('causal', [1, 0])
def test_cattn_kernels_against_the_oracle(K, O, causal, f16, masked, heads, dh, n):
    """forward (fp16 and bf16 operands) and the bf16 backward against O.attention_core on inputs pre-rounded to the operand type"""
    B, inner = 2, heads * dh
    dt = torch.float16 if f16 else torch.bfloat16
    q, kv, nk, nv, wth, mask = _inputs(B, n, heads, dh, dt, masked)
    g = K.cattn_geom(B, n, heads, dh, causal=bool(causal))
    assert K.cattn_supported(g)
    qd, kvd = q.to(DEV), kv.to(DEV)
    md = mask.to(torch.uint8).to(DEV) if masked else None
    tag = f'[c={causal},f16={f16},m={masked},{heads},{dh},{n}]'

    qr = q.float().reshape(B, n, heads, dh).requires_grad_(True)
    kvr = kv.float().reshape(B, n, 2, heads, dh).requires_grad_(True)
    nkr, nvr, wr = nk.clone().requires_grad_(True), nv.clone().requires_grad_(True), wth.clone().requires_grad_(True)
    o_ref = O.attention_core(qr, kvr[:, :, 0], kvr[:, :, 1], nkr, nvr, wr, mask, dh ** -0.5, causal=bool(causal))

    o, stats = K.cattn_fwd(g, qd, kvd[:, :inner], kvd[:, inner:], nk.to(DEV), nv.to(DEV), wth.to(DEV), md)
    got = (o.hi.float() + o.lo.float()).reshape(B, n, heads, dh)
    report('cattn_fwd' + tag, got, o_ref, 1e-3 if f16 else 2e-2)
    assert stats.shape == (B, heads, n, 2)
    # the two other output forms carry the same values
    o2, _ = K.cattn_fwd(g, qd, kvd[:, :inner], kvd[:, inner:], nk.to(DEV), nv.to(DEV), wth.to(DEV), md, o_f16=True)
    assert torch.equal(o2.hi, o.hi)
    report('cattn_fwd.o_f16' + tag, o2.f16.float().reshape(B, n, heads, dh), o_ref, 1e-3 if f16 else 2e-2)
    o3, _ = K.cattn_fwd(g, qd, kvd[:, :inner], kvd[:, inner:], nk.to(DEV), nv.to(DEV), wth.to(DEV), md, lo=False)
    assert o3.lo is None and torch.equal(o3.hi, o.hi)
    if f16:
        return
    torch.manual_seed(5)
    dO = torch.randn(B * n, inner).to(torch.bfloat16)
    o_ref.backward(dO.float().reshape(B, n, heads, dh))
    dq, dkv, dwth, dnk, dnv = K.cattn_bwd(g, qd, kvd[:, :inner], kvd[:, inner:], dO.to(DEV), nk.to(DEV), nv.to(DEV), wth.to(DEV), stats, md)
    report('cattn_bwd.dq' + tag, dq.hi.float().reshape(B, n, heads, dh), qr.grad, 7e-2)
    dkvg = dkv.hi.float().reshape(B, n, 2, heads, dh)
    report('cattn_bwd.dk' + tag, dkvg[:, :, 0], kvr.grad[:, :, 0], 7e-2)
    report('cattn_bwd.dv' + tag, dkvg[:, :, 1], kvr.grad[:, :, 1], 7e-2)
    report('cattn_bwd.dW' + tag, dwth, wr.grad, 7e-2)
    report('cattn_bwd.dnull_k' + tag, dnk, nkr.grad, 7e-2)
    report('cattn_bwd.dnull_v' + tag, dnv, nvr.grad, 7e-2)


@pytest.mark.parametrize('p', [257, 1])
def test_causality_rows_before_a_change_are_bit_identical(A, p):
    """changing rows >= p of x leaves output rows < p bit-identical"""
    torch.manual_seed(3)
    n = 600
    m = A.Attention(dim=512, heads=8, dim_head=64, causal=True).to(DEV)
    for mode in ('bf16x3-fwd', 'bf16'):
        A.set_precision(mode)
        try:
            x = torch.randn(2, n, 512, device=DEV)
            x2 = x.clone()
            x2[:, p:] = torch.randn(2, n - p, 512, device=DEV) * 3.0
            with torch.no_grad():
                y, y2 = m(x), m(x2)
            assert torch.equal(y[:, :p], y2[:, :p]), mode
            assert not torch.equal(y[:, p:], y2[:, p:]), mode
        finally:
            A.set_precision('bf16')


def test_forward_and_backward_are_deterministic(A):
    """two runs of forward + backward bit-identical (no atomics on any gradient)"""
    torch.manual_seed(4)
    m = A.Attention(dim=512, heads=8, dim_head=64, causal=True).to(DEV)
    x0 = torch.randn(4, 600, 512, device=DEV)
    mask = torch.rand(4, 600, device=DEV) > 0.2
    dy = torch.randn(4, 600, 512, device=DEV)
    for mode in ('bf16x3-fwd', 'bf16'):
        A.set_precision(mode)
        try:
            runs = []
            for _ in range(2):
                m.zero_grad(set_to_none=True)
                x = x0.clone().requires_grad_(True)
                y = m(x, mask=mask)
                y.backward(dy)
                runs.append([y.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in m.parameters()])
            for a, b in zip(*runs):
                assert torch.equal(a, b), mode
        finally:
            A.set_precision('bf16')


def _oracle_module(O, m, x, mask, dy):
    """the oracle's attention(causal=True) on the module's parameters (CPU fp32): y, dx, parameter gradients by state-dict name"""
    P = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    xr = x.detach().cpu().clone().requires_grad_(True)
    y = O.attention(xr, P, m.heads, mask=None if mask is None else mask.cpu(), causal=True)
    y.backward(dy.cpu())
    return y.detach(), xr.grad, {k: v.grad for k, v in P.items()}


@pytest.mark.parametrize('mode,tol,gtol', MODES)
def test_module_against_the_reference_fixture(A, mode, tol, gtol):
    Ar, P, G = load('g14_causal_attention')
    m = A.Attention(dim=32, heads=int(Ar['heads']), dim_head=32, causal=True)
    m.load_state_dict(P)
    m = m.to(DEV)
    A.set_precision(mode)
    try:
        x = Ar['x'].to(DEV).requires_grad_(True)
        y = m(x, mask=Ar['mask'].to(DEV))
        report(f'g14[{mode}].y', y, Ar['y'], tol)
        y.backward(Ar['dy'].to(DEV))
        report(f'g14[{mode}].dx', x.grad, Ar['dx'], gtol)
        named = dict(m.named_parameters())
        for k, g in G.items():
            report(f'g14[{mode}].grad.{k}', named[k].grad, g, gtol)
    finally:
        A.set_precision('bf16')


@pytest.mark.parametrize('mode,tol,gtol', MODES)
def test_module_against_the_oracle_at_width_512(A, O, mode, tol, gtol):
    from nuwa_pytorch_amd import ops
    torch.manual_seed(9)
    m = A.Attention(dim=512, heads=8, dim_head=64, causal=True).to(DEV)
    x = torch.randn(2, 300, 512, device=DEV)
    mask = torch.rand(2, 300, device=DEV) > 0.25
    dy = torch.randn(2, 300, 512, device=DEV)
    y_ref, dx_ref, G = _oracle_module(O, m, x, mask, dy)
    calls = []
    orig = ops.CInner.fwd
    A.set_precision(mode)
    try:
        ops.CInner.fwd = staticmethod(lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
        xg = x.clone().requires_grad_(True)
        y = m(xg, mask=mask)
        report(f'cattn_module[{mode}].y', y, y_ref, tol)
        y.backward(dy)
        report(f'cattn_module[{mode}].dx', xg.grad, dx_ref, gtol)
        for k, p in m.named_parameters():
            report(f'cattn_module[{mode}].grad.{k}', p.grad, G[k], gtol)
        assert len(calls) == (0 if mode == 'bf16x3' else 1)      # the parity mode keeps the torch-op formulation
    finally:
        ops.CInner.fwd = orig
        A.set_precision('bf16')


@pytest.mark.parametrize('mode,tol,gtol', MODES[1:])
def test_module_with_rotary_embedding(A, O, mode, tol, gtol):
    """rotary position embedding on q, k and v (np.py:333-335) in front of the causal core, forward and backward"""
    from nuwa_pytorch_amd.nuwa_pytorch import RotaryEmbedding
    torch.manual_seed(12)
    m = A.Attention(dim=64, heads=2, dim_head=32, causal=True).to(DEV)
    x = torch.randn(2, 75, 64, device=DEV)
    mask = torch.rand(2, 75, device=DEV) > 0.25
    dy = torch.randn(2, 75, 64, device=DEV)
    rot = RotaryEmbedding(dim=32).to(DEV)(75, device=DEV)
    P = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    xr = x.cpu().clone().requires_grad_(True)
    y_ref = O.attention(xr, P, 2, mask=mask.cpu(), rotary=rot.cpu(), causal=True)
    y_ref.backward(dy.cpu())
    A.set_precision(mode)
    try:
        xg = x.clone().requires_grad_(True)
        y = m(xg, mask=mask, rotary_pos_emb=rot)
        report(f'cattn_rotary[{mode}].y', y, y_ref.detach(), tol)
        y.backward(dy)
        report(f'cattn_rotary[{mode}].dx', xg.grad, xr.grad, gtol)
        for k, p in m.named_parameters():
            report(f'cattn_rotary[{mode}].grad.{k}', p.grad, P[k].grad, gtol)
    finally:
        A.set_precision('bf16')


@pytest.mark.parametrize('mode,tol,gtol', MODES)
@pytest.mark.parametrize('reversible', [False, True])
def test_decoder_stack_with_plain_causal_attention(A, monkeypatch, reversible, mode, tol, gtol):
    """Transformer / ReversibleTransformer(causal=True) with plain attention: loss and every gradient against the torch-op formulation of
    the same modules, and the self-attention blocks run as fused SandwichBlockFn nodes of kind 'cattn'"""
    from nuwa_pytorch_amd import ops
    from nuwa_pytorch_amd.nuwa_pytorch import Attention
    torch.manual_seed(21)
    cls = A.ReversibleTransformer if reversible else A.Transformer
    net = cls(dim=64, depth=2, causal=True, heads=2, dim_head=32, cross_attend=True).to(DEV)
    x0 = torch.randn(2, 90, 64, device=DEV)
    ctx = torch.randn(2, 12, 64, device=DEV)
    cmask = torch.rand(2, 12, device=DEV) > 0.2
    mask = torch.rand(2, 90, device=DEV) > 0.15
    tgt = torch.randn(2, 90, 64, device=DEV)

    def run():
        net.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        loss = ((net(x, mask=mask, context=ctx, context_mask=cmask) - tgt) ** 2).mean()
        loss.backward()
        return loss.detach(), x.grad.clone(), {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}

    A.set_precision(mode)
    try:
        with monkeypatch.context() as mp:
            mp.setattr(Attention, '_causal_hip_ok', lambda self, n: False)
            loss_ref, dx_ref, G = run()
        kinds = []
        orig = ops.SandwichBlockFn.forward

        def spy(ctx_, x, resid, context, meta, *rest):
            kinds.append(meta['kind'])
            return orig(ctx_, x, resid, context, meta, *rest)
        with monkeypatch.context() as mp:
            mp.setattr(ops.SandwichBlockFn, 'forward', staticmethod(spy))
            loss, dx, Gn = run()
        tagm = f'cattn_stack[rev={reversible},{mode}]'
        report(tagm + '.loss', loss.reshape(1), loss_ref.reshape(1), tol)
        report(tagm + '.dx', dx, dx_ref, gtol)
        assert set(Gn) == set(G)
        for k in G:
            report(tagm + '.grad.' + k, Gn[k], G[k], gtol)
        if mode != 'bf16x3':
            assert kinds.count('cattn') >= 2, kinds            # one per layer (a reversible stack runs its blocks again in the backward)
        else:
            assert 'cattn' not in kinds
    finally:
        A.set_precision('bf16')


def test_routing_guards(A):
    from nuwa_pytorch_amd import ops
    from nuwa_pytorch_amd.decode import IncrementalDecoder
    kinds = []
    orig = ops.InnerFn.forward

    def spy(ctx_, x, context, meta, *p):
        kinds.append(meta['kind'])
        return orig(ctx_, x, context, meta, *p)
    x = torch.randn(2, 40, 64, device=DEV)
    ctx = torch.randn(2, 9, 64, device=DEV)
    try:
        ops.InnerFn.forward = staticmethod(spy)
        # attention dropout > 0 in training: the torch-op formulation
        m = A.Attention(dim=64, heads=2, dim_head=32, causal=True, dropout=0.1).to(DEV).train()
        m(x)
        assert kinds == []
        m.eval()
        m(x)
        assert kinds == ['cattn']
        del kinds[:]
        # non-causal self-attention and cross-attention: the cross-attention kernels, as before
        m2 = A.Attention(dim=64, heads=2, dim_head=32).to(DEV)
        m2(x)
        m2(x, context=ctx)
        assert kinds == ['xattn', 'xattn']
    finally:
        ops.InnerFn.forward = orig
    net = A.Transformer(dim=64, depth=1, causal=True, heads=2, dim_head=32, cross_attend=True).to(DEV).eval()
    with pytest.raises(NotImplementedError):
        IncrementalDecoder(net, 2, 40, ctx, None, torch.zeros(1, dtype=torch.int32, device=DEV))


def test_linear_memory_at_8192_rows(A):
    """b = 2, n = 8192, dim 512, 8 x 64, 'bf16x3-fwd', forward + backward of the bare module: the peak above what was allocated before the
    call stays below ONE fp32 score array b * heads * n * (n + 1) * 4 = 4.29 GB (the torch-op formulation holds several)"""
    b, n = 2, 8192
    torch.manual_seed(2)
    m = A.Attention(dim=512, heads=8, dim_head=64, causal=True).to(DEV)
    x = torch.randn(b, n, 512, device=DEV, requires_grad=True)
    dy = torch.randn(b, n, 512, device=DEV)
    A.set_precision('bf16x3-fwd')
    try:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        y = m(x)
        y.backward(dy)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
        bound = b * 8 * n * (n + 1) * 4
        print(f'cattn peak above the baseline: {peak / 1e6:.1f} MB (bound {bound / 1e9:.2f} GB)')
        assert torch.isfinite(y).all() and torch.isfinite(x.grad).all()
        assert peak < bound, (peak, bound)
    finally:
        A.set_precision('bf16')
