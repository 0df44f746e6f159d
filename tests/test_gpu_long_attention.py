"""Non-causal attention over any number of keys on the linear-memory cattn kernels' rectangular form (csrc/cattn.hip with
amdnuwa_cattn_geom.n_keys: n query rows, T key rows from another tensor), on the MI355X: the kernels against the oracle's attention_core
for n != T, determinism, the module against the reference fixture g15 and the oracle (cross-attention over a long context, long
self-attention with rotary embeddings), the fused blocks of encoder and decoder stacks, the routing guards and the memory bound.

The module ships with a shape gate on this route (Attention.long_pairs_min / long_wgs_min: the measured speed crossover against the torch-op
formulation); the tests that run the kernels at a few hundred keys lower it (fixture low_gate), the routing and memory tests
check it as shipped.

Tolerances (max-abs error / max-abs reference, gpu_util.report) are those of test_gpu_causal_attention.py: kernel level fp16 forward 1e-3,
bf16 forward 2e-2, bf16 backward 7e-2; module level the MODES of test_gpu_modules.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from golden_util import load  # noqa: E402
from gpu_util import report  # noqa: E402

DEV = 'cuda'
MODES = [('bf16x3', 1e-3, 2e-3), ('bf16x3-fwd', 1e-3, 7e-2), ('bf16', 2e-2, 7e-2)]
# (heads, dim_head, n query rows, T key rows)
GEOMS = [(8, 64, 1, 300), (8, 64, 257, 33), (8, 64, 600, 289), (8, 64, 64, 1000), (2, 32, 70, 513), (5, 32, 129, 320), (3, 64, 31, 64)]


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


@pytest.fixture
def low_gate(monkeypatch):
    """Attention.long_pairs_min / long_wgs_min ship at the measured speed crossover against the torch-op formulation; the
    kernels take every shape above the cross-attention kernels' 287 keys, and the tests below run them from there"""
    from nuwa_pytorch_amd.nuwa_pytorch import Attention
    monkeypatch.setattr(Attention, 'long_pairs_min', 0)
    monkeypatch.setattr(Attention, 'long_wgs_min', 0)


def _inputs(B, n, T, heads, dh, dt, masked, seed=17):
    torch.manual_seed(seed)
    inner = heads * dh
    q = torch.randn(B * n, inner).to(dt)
    kv = torch.randn(B * T, 2 * inner).to(dt)
    nk, nv = torch.randn(heads, dh), torch.randn(heads, dh)
    wth = torch.randn(heads, heads) * 0.5 + torch.eye(heads)
    mask = None
    if masked:
        mask = torch.rand(B, T) > 0.3
        mask[0] = False                    # a fully masked sample attends only the null key
    return q, kv, nk, nv, wth, mask


@pytest.mark.parametrize('heads,dh,n,T', GEOMS)
@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('f16', [True, False])
def test_rectangular_kernels_against_the_oracle(K, O, f16, masked, heads, dh, n, T):
    """n queries over T keys of another tensor: forward (fp16 and bf16 operands) and the bf16 backward against O.attention_core on inputs
    pre-rounded to the operand type"""
    B, inner = 2, heads * dh
    dt = torch.float16 if f16 else torch.bfloat16
    q, kv, nk, nv, wth, mask = _inputs(B, n, T, heads, dh, dt, masked)
    g = K.cattn_geom(B, n, heads, dh, causal=False, n_keys=T)
    assert K.cattn_supported(g) and not K.cattn_supported(K.cattn_geom(B, n, heads, dh, causal=True, n_keys=T))
    qd, kvd = q.to(DEV), kv.to(DEV)
    md = mask.to(torch.uint8).to(DEV) if masked else None
    tag = f'[f16={f16},m={masked},{heads},{dh},{n}x{T}]'

    qr = q.float().reshape(B, n, heads, dh).requires_grad_(True)
    kvr = kv.float().reshape(B, T, 2, heads, dh).requires_grad_(True)
    nkr, nvr, wr = nk.clone().requires_grad_(True), nv.clone().requires_grad_(True), wth.clone().requires_grad_(True)
    o_ref = O.attention_core(qr, kvr[:, :, 0], kvr[:, :, 1], nkr, nvr, wr, mask, dh ** -0.5, causal=False)

    o, stats = K.cattn_fwd(g, qd, kvd[:, :inner], kvd[:, inner:], nk.to(DEV), nv.to(DEV), wth.to(DEV), md)
    got = (o.hi.float() + o.lo.float()).reshape(B, n, heads, dh)
    report('cattn_kv_fwd' + tag, got, o_ref, 1e-3 if f16 else 2e-2)
    assert stats.shape == (B, heads, n, 2)
    o2, _ = K.cattn_fwd(g, qd, kvd[:, :inner], kvd[:, inner:], nk.to(DEV), nv.to(DEV), wth.to(DEV), md, o_f16=True)
    assert torch.equal(o2.hi, o.hi)
    report('cattn_kv_fwd.o_f16' + tag, o2.f16.float().reshape(B, n, heads, dh), o_ref, 1e-3 if f16 else 2e-2)
    if f16:
        return
    torch.manual_seed(5)
    dO = torch.randn(B * n, inner).to(torch.bfloat16)
    o_ref.backward(dO.float().reshape(B, n, heads, dh))
    args = (g, qd, kvd[:, :inner], kvd[:, inner:], dO.to(DEV), nk.to(DEV), nv.to(DEV), wth.to(DEV), stats, md)
    dq, dkv, dwth, dnk, dnv = K.cattn_bwd(*args)
    assert dq.hi.shape == (B * n, inner) and dkv.hi.shape == (B * T, 2 * inner)
    report('cattn_kv_bwd.dq' + tag, dq.hi.float().reshape(B, n, heads, dh), qr.grad, 7e-2)
    dkvg = dkv.hi.float().reshape(B, T, 2, heads, dh)
    report('cattn_kv_bwd.dk' + tag, dkvg[:, :, 0], kvr.grad[:, :, 0], 7e-2)
    report('cattn_kv_bwd.dv' + tag, dkvg[:, :, 1], kvr.grad[:, :, 1], 7e-2)
    report('cattn_kv_bwd.dW' + tag, dwth, wr.grad, 7e-2)
    report('cattn_kv_bwd.dnull_k' + tag, dnk, nkr.grad, 7e-2)
    report('cattn_kv_bwd.dnull_v' + tag, dnv, nvr.grad, 7e-2)
    # no atomics: a second run gives the same bits
    again = K.cattn_bwd(*args)
    for a, b in zip((dq.hi, dkv.hi, dwth, dnk, dnv), (again[0].hi, again[1].hi) + tuple(again[2:])):
        assert torch.equal(a, b)


def test_forward_and_backward_are_deterministic_with_a_context(A, low_gate):
    """two runs of forward + backward of the module over a long context bit-identical (no atomics on any gradient)"""
    torch.manual_seed(4)
    m = A.Attention(dim=512, heads=8, dim_head=64).to(DEV)
    x0 = torch.randn(3, 600, 512, device=DEV)
    c0 = torch.randn(3, 417, 512, device=DEV)
    cmask = torch.rand(3, 417, device=DEV) > 0.2
    dy = torch.randn(3, 600, 512, device=DEV)
    for mode in ('bf16x3-fwd', 'bf16'):
        A.set_precision(mode)
        try:
            runs = []
            for _ in range(2):
                m.zero_grad(set_to_none=True)
                x, c = x0.clone().requires_grad_(True), c0.clone().requires_grad_(True)
                y = m(x, context=c, context_mask=cmask)
                y.backward(dy)
                runs.append([y.detach().clone(), x.grad.clone(), c.grad.clone()] + [p.grad.clone() for p in m.parameters()])
            for a, b in zip(*runs):
                assert torch.equal(a, b), mode
        finally:
            A.set_precision('bf16')


def _oracle_module(O, m, x, dy, context=None, context_mask=None, mask=None, rotary=None):
    """the oracle's non-causal attention on the module's parameters (CPU fp32): y, dx, dcontext, parameter gradients by state-dict name"""
    cpu = lambda t: None if t is None else t.detach().cpu()
    P = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.state_dict().items()}
    xr = cpu(x).clone().requires_grad_(True)
    cr = None if context is None else cpu(context).clone().requires_grad_(True)
    y = O.attention(xr, P, m.heads, context=cr, context_mask=cpu(context_mask), mask=cpu(mask), rotary=cpu(rotary), causal=False)
    y.backward(dy.cpu())
    return y.detach(), xr.grad, (None if cr is None else cr.grad), {k: v.grad for k, v in P.items()}


class _Spy:
    """counts the calls of ops.CInner.fwd while active"""

    def __enter__(self):
        from nuwa_pytorch_amd import ops
        self.ops, self.orig, self.calls = ops, ops.CInner.fwd, []
        ops.CInner.fwd = staticmethod(lambda *a, **k: (self.calls.append(a[2].get('has_ctx')), self.orig(*a, **k))[1])
        return self

    def __exit__(self, *exc):
        self.ops.CInner.fwd = self.orig


@pytest.mark.parametrize('mode,tol,gtol', MODES)
def test_module_against_the_reference_fixture(A, low_gate, mode, tol, gtol):
    """fixture g15: 20 queries over a context of 300 keys, one sample with every context token masked"""
    Ar, P, G = load('g15_long_attention')
    m = A.Attention(dim=32, heads=int(Ar['heads']), dim_head=32)
    m.load_state_dict(P)
    m = m.to(DEV)
    A.set_precision(mode)
    try:
        with _Spy() as spy:
            x = Ar['x'].to(DEV).requires_grad_(True)
            c = Ar['context'].to(DEV).requires_grad_(True)
            y = m(x, context=c, context_mask=Ar['context_mask'].to(DEV))
            report(f'g15[{mode}].y', y, Ar['y'], tol)
            y.backward(Ar['dy'].to(DEV))
        report(f'g15[{mode}].dx', x.grad, Ar['dx'], gtol)
        report(f'g15[{mode}].dcontext', c.grad, Ar['dcontext'], gtol)
        named = dict(m.named_parameters())
        for k, g in G.items():
            report(f'g15[{mode}].grad.{k}', named[k].grad, g, gtol)
        assert spy.calls == ([] if mode == 'bf16x3' else [True])
    finally:
        A.set_precision('bf16')


@pytest.mark.parametrize('mode,tol,gtol', MODES)
def test_cross_attention_module_against_the_oracle_at_width_512(A, O, low_gate, mode, tol, gtol):
    """n = 300 queries over a context of T = 400 rows with a context mask: y, dx, dcontext and every parameter gradient; exactly one pass
    through ops.CInner.fwd in 'bf16' / 'bf16x3-fwd', none in the parity mode"""
    torch.manual_seed(9)
    m = A.Attention(dim=512, heads=8, dim_head=64).to(DEV)
    x = torch.randn(2, 300, 512, device=DEV)
    c = torch.randn(2, 400, 512, device=DEV)
    cmask = torch.rand(2, 400, device=DEV) > 0.25
    dy = torch.randn(2, 300, 512, device=DEV)
    y_ref, dx_ref, dc_ref, G = _oracle_module(O, m, x, dy, context=c, context_mask=cmask)
    A.set_precision(mode)
    try:
        with _Spy() as spy:
            xg, cg = x.clone().requires_grad_(True), c.clone().requires_grad_(True)
            y = m(xg, context=cg, context_mask=cmask)
            report(f'long_xattn_module[{mode}].y', y, y_ref, tol)
            y.backward(dy)
        report(f'long_xattn_module[{mode}].dx', xg.grad, dx_ref, gtol)
        report(f'long_xattn_module[{mode}].dcontext', cg.grad, dc_ref, gtol)
        for k, p in m.named_parameters():
            report(f'long_xattn_module[{mode}].grad.{k}', p.grad, G[k], gtol)
        assert spy.calls == ([] if mode == 'bf16x3' else [True])      # the parity mode keeps the torch-op formulation
    finally:
        A.set_precision('bf16')


@pytest.mark.parametrize('mode,tol,gtol', MODES)
def test_self_attention_module_with_rotary_against_the_oracle_at_width_512(A, O, low_gate, mode, tol, gtol):
    """non-causal self-attention over n = 512 rows (the text / sketch encoder's block) with a key mask and rotary embeddings on q, k, v"""
    from nuwa_pytorch_amd.nuwa_pytorch import RotaryEmbedding
    torch.manual_seed(10)
    m = A.Attention(dim=512, heads=8, dim_head=64).to(DEV)
    x = torch.randn(2, 512, 512, device=DEV)
    mask = torch.rand(2, 512, device=DEV) > 0.25
    dy = torch.randn(2, 512, 512, device=DEV)
    rot = RotaryEmbedding(dim=32).to(DEV)(512, device=DEV)
    y_ref, dx_ref, _, G = _oracle_module(O, m, x, dy, mask=mask, rotary=rot)
    A.set_precision(mode)
    try:
        with _Spy() as spy:
            xg = x.clone().requires_grad_(True)
            y = m(xg, mask=mask, rotary_pos_emb=rot)
            report(f'long_self_module[{mode}].y', y, y_ref, tol)
            y.backward(dy)
        report(f'long_self_module[{mode}].dx', xg.grad, dx_ref, gtol)
        for k, p in m.named_parameters():
            report(f'long_self_module[{mode}].grad.{k}', p.grad, G[k], gtol)
        assert spy.calls == ([] if mode == 'bf16x3' else [False])
    finally:
        A.set_precision('bf16')


def _stack_run(A, monkeypatch, net, fwd, mode, tol, gtol, tag):
    """loss and every gradient of `net` with the long-key predicate on against the same modules with it patched to False (the torch-op
    formulation); returns the kinds of the fused nodes the routed run went through"""
    from nuwa_pytorch_amd import ops
    from nuwa_pytorch_amd.nuwa_pytorch import Attention

    def run():
        net.zero_grad(set_to_none=True)
        loss, leaves = fwd()
        loss.backward()
        return loss.detach(), [t.grad.clone() for t in leaves], {k: p.grad.clone() for k, p in net.named_parameters() if p.grad is not None}

    A.set_precision(mode)
    try:
        with monkeypatch.context() as mp:
            mp.setattr(Attention, '_long_hip_ok', lambda self, *a, **k: False)
            loss_ref, leaves_ref, G = run()
        kinds = []
        orig = ops.SandwichBlockFn.forward

        def spy(ctx_, x, resid, context, meta, *rest):
            kinds.append((meta['kind'], bool(meta.get('has_ctx'))))
            return orig(ctx_, x, resid, context, meta, *rest)
        with monkeypatch.context() as mp:
            mp.setattr(ops.SandwichBlockFn, 'forward', staticmethod(spy))
            loss, leaves, Gn = run()
        report(tag + '.loss', loss.reshape(1), loss_ref.reshape(1), tol)
        for i, (a, b) in enumerate(zip(leaves, leaves_ref)):
            report(tag + f'.dinput{i}', a, b, gtol)
        assert set(Gn) == set(G)
        for k in G:
            report(tag + '.grad.' + k, Gn[k], G[k], gtol)
        return kinds
    finally:
        A.set_precision('bf16')


@pytest.mark.parametrize('mode,tol,gtol', MODES)
def test_six_layer_encoder_over_512_tokens(A, monkeypatch, low_gate, mode, tol, gtol):
    """the sketch encoder's shape: a 6-layer non-causal Transformer over 2 x 16 x 16 = 512 tokens with a key mask; every self-attention
    block runs as a fused SandwichBlockFn node of kind 'cattn'"""
    torch.manual_seed(22)
    net = A.Transformer(dim=512, depth=6, heads=8, dim_head=64).to(DEV)
    x0 = torch.randn(2, 512, 512, device=DEV)
    mask = torch.rand(2, 512, device=DEV) > 0.1
    tgt = torch.randn(2, 512, 512, device=DEV)

    def fwd():
        x = x0.clone().requires_grad_(True)
        return ((net(x, mask=mask) - tgt) ** 2).mean(), [x]
    kinds = _stack_run(A, monkeypatch, net, fwd, mode, tol, gtol, f'long_encoder[{mode}]')
    cattn = [k for k in kinds if k[0] == 'cattn']
    assert cattn == ([] if mode == 'bf16x3' else [('cattn', False)] * 6), kinds
    assert [k[0] for k in kinds].count('ff') == 6


@pytest.mark.parametrize('mode,tol,gtol', MODES)
@pytest.mark.parametrize('reversible', [False, True])
def test_decoder_stack_with_a_320_key_context(A, monkeypatch, low_gate, reversible, mode, tol, gtol):
    """Transformer / ReversibleTransformer(causal=True, cross_attend=True) over a context of 320 keys: the cross-attention blocks run as
    fused nodes of kind 'cattn' with the context; loss, dx, dcontext and every gradient against the torch-op formulation.
    At the models' width (dim 512, 8 x 64), not that of test_gpu_causal_attention.py's toy stack (dim 64, 2 x 32): the toy's 2 x 2
    talking-heads gradients are cancelling sums of magnitude 1e-3 that the bf16 modes resolve to 1e-2 ... 9e-2 depending on the seed, on
    the causal blocks of the parent's own routing just the same (seeds 21 ... 24: 2.3e-2, 9.0e-2, 4.1e-2, 5.9e-2 worst per seed), so the
    toy measures its seed; at width 512 the worst gradient of four seeds stays below 3e-2 on either routing."""
    torch.manual_seed(21)
    cls = A.ReversibleTransformer if reversible else A.Transformer
    depth, dim, n, T = 2, 512, 256, 320
    net = cls(dim=dim, depth=depth, causal=True, heads=8, dim_head=64, cross_attend=True).to(DEV)
    x0 = torch.randn(2, n, dim, device=DEV)
    c0 = torch.randn(2, T, dim, device=DEV)
    cmask = torch.rand(2, T, device=DEV) > 0.2
    mask = torch.rand(2, n, device=DEV) > 0.15
    tgt = torch.randn(2, n, dim, device=DEV)

    def fwd():
        x, c = x0.clone().requires_grad_(True), c0.clone().requires_grad_(True)
        return ((net(x, mask=mask, context=c, context_mask=cmask) - tgt) ** 2).mean(), [x, c]
    kinds = _stack_run(A, monkeypatch, net, fwd, mode, tol, gtol, f'long_ctx_stack[rev={reversible},{mode}]')
    cross = kinds.count(('cattn', True))
    if mode == 'bf16x3':
        assert cross == 0, kinds
    elif reversible:
        assert cross >= depth, kinds           # (a reversible stack runs its blocks again in the backward)
    else:
        assert cross == depth, kinds
    assert ('xattn', False) not in kinds


def test_routing_guards(A, monkeypatch):
    from nuwa_pytorch_amd import ops
    from nuwa_pytorch_amd.decode import IncrementalDecoder
    from nuwa_pytorch_amd.nuwa_pytorch import Attention
    kinds = []
    orig = ops.InnerFn.forward

    def spy(ctx_, x, context, meta, *p):
        kinds.append(meta['kind'])
        return orig(ctx_, x, context, meta, *p)
    x = torch.randn(2, 40, 64, device=DEV)
    try:
        ops.InnerFn.forward = staticmethod(spy)
        m = A.Attention(dim=64, heads=2, dim_head=32).to(DEV)
        # as shipped: up to 287 keys the cross-attention kernels, as before; beyond, the rectangular cattn form where it is the faster route
        # (batch * queries * keys >= long_pairs_min, long_wgs_min workgroups on either side), the torch-op formulation elsewhere
        m(x, context=torch.randn(2, 287, 64, device=DEV))
        m(torch.randn(2, 287, 64, device=DEV))
        assert kinds == ['xattn', 'xattn']
        del kinds[:]
        m(x, context=torch.randn(2, 288, 64, device=DEV))
        m(torch.randn(2, 288, 64, device=DEV))
        m(torch.randn(2, 1024, 64, device=DEV))                                                     # too few pairs, too few workgroups
        m(torch.randn(8, 1023, 64, device=DEV))                                                     # 8 x 1023 x 1023 pairs: just below
        assert kinds == []
        with torch.no_grad():
            m(torch.randn(8, 1024, 64, device=DEV))
            m(torch.randn(8, 1100, 64, device=DEV), context=torch.randn(8, 1024, 64, device=DEV))
        assert kinds == ['cattn', 'cattn']
        del kinds[:]
        # the kernels themselves start where the cross-attention kernels end: 288 keys with the gate lowered
        monkeypatch.setattr(Attention, 'long_pairs_min', 0)
        monkeypatch.setattr(Attention, 'long_wgs_min', 0)
        m(x, context=torch.randn(2, 287, 64, device=DEV))
        m(x, context=torch.randn(2, 288, 64, device=DEV))
        m(torch.randn(2, 287, 64, device=DEV))
        m(torch.randn(2, 288, 64, device=DEV))
        assert kinds == ['xattn', 'cattn', 'xattn', 'cattn']
        del kinds[:]
        ctx = torch.randn(2, 320, 64, device=DEV)
        # attention dropout > 0 in training: the torch-op formulation
        d = A.Attention(dim=64, heads=2, dim_head=32, dropout=0.1).to(DEV).train()
        d(x, context=ctx)
        assert kinds == []
        d.eval()
        d(x, context=ctx)
        assert kinds == ['cattn']
        del kinds[:]
        # causal attention with a context: the torch-op formulation
        A.Attention(dim=64, heads=2, dim_head=32, causal=True).to(DEV)(x, context=ctx)
        assert kinds == []
        # the parity mode keeps the torch-op formulation
        A.set_precision('bf16x3')
        m(x, context=ctx)
        assert kinds == []
    finally:
        A.set_precision('bf16')
        ops.InnerFn.forward = orig
    # cached decoding: no single-row path over a 320-key context (12 keys: the xattn_decode kernel, as before)
    net = A.Transformer(dim=64, depth=1, causal=True, heads=2, dim_head=32, cross_attend=True, sparse_3dna_attn=True,
                        sparse_3dna_video_shape=(2, 4, 4)).to(DEV).eval()
    pos = torch.zeros(1, dtype=torch.int32, device=DEV)
    IncrementalDecoder(net, 2, 33, torch.randn(2, 12, 64, device=DEV), None, pos)
    with pytest.raises(NotImplementedError):
        IncrementalDecoder(net, 2, 33, torch.randn(2, 320, 64, device=DEV), None, pos)


def test_generate_with_a_320_token_text(A, low_gate):
    """NUWA.generate with text_max_seq_len = 320: the cached decoder declines (no single-row kernel over that many keys) and the recompute
    loop returns frames, its text encoder and text cross-attention on the cattn kernels"""
    torch.manual_seed(5)
    vae = A.VQGanVAE(dim=32, image_size=16, num_layers=2, vq_codebook_size=64, vq_codebook_dim=32, use_vgg_and_gan=False)
    nuwa = A.NUWA(vae=vae, dim=64, text_num_tokens=50, text_max_seq_len=320, max_video_frames=2, text_enc_depth=1, dec_depth=1,
                  dec_heads=2, dec_dim_head=32, text_enc_heads=2, text_enc_dim_head=32, sparse_3dna_kernel_size=3).to(DEV).eval()
    text = torch.randint(1, 50, (1, 320), generator=torch.Generator().manual_seed(3)).to(DEV)
    A.set_precision('bf16x3-fwd')
    try:
        with _Spy() as spy:
            frames = nuwa.generate(text=text, filter_thres=0.99, num_frames=1, cond_scale=2.)
        assert frames.shape[0] == 1 and frames.shape[-1] == 16 and torch.isfinite(frames).all()
        assert nuwa.last_generated_ids.shape == (1, 16)
        assert False in spy.calls and True in spy.calls          # the text encoder's self-attention and the decoder's cross-attention
    finally:
        A.set_precision('bf16')


def test_linear_memory_with_4096_queries_and_4096_context_keys(A):
    """b = 2, n = 4096 queries, T = 4096 context keys, dim 512, 8 x 64, 'bf16x3-fwd', forward + backward of the bare module: the peak above
    what was allocated before the call stays below ONE fp32 score array b * heads * n * (T + 1) * 4 = 1.07 GB (the torch-op formulation
    holds several)"""
    b, n, T = 2, 4096, 4096
    torch.manual_seed(2)
    m = A.Attention(dim=512, heads=8, dim_head=64).to(DEV)
    x = torch.randn(b, n, 512, device=DEV, requires_grad=True)
    c = torch.randn(b, T, 512, device=DEV, requires_grad=True)
    dy = torch.randn(b, n, 512, device=DEV)
    A.set_precision('bf16x3-fwd')
    try:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        y = m(x, context=c)
        y.backward(dy)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
        bound = b * 8 * n * (T + 1) * 4
        print(f'cattn (context) peak above the baseline: {peak / 1e6:.1f} MB (bound {bound / 1e9:.2f} GB)')
        assert torch.isfinite(y).all() and torch.isfinite(x.grad).all() and torch.isfinite(c.grad).all()
        assert peak < bound, (peak, bound)
    finally:
        A.set_precision('bf16')
