"""Attention dropout inside the linear-memory cattn kernels (csrc/cattn.hip, the DROP forms; amdnuwa_cattn_fwd_drop / _bwd_drop) and the opt-in
module route on top of them (Attention.dropout_on_kernels), on the MI355X.

Shapes sit at the kernels' tile borders (64 stationary rows per workgroup, 16 per wave, 32 streamed rows per step): B = 2, n = 70 queries
(two query workgroups, the second ragged), T = 45 keys (a ragged second key tile, one ragged key-side workgroup) or 100 (two key-side
workgroups), causal n = 70; (heads, dim_head) = (2, 32), (3, 64) and (8, 64), the instantiation at the register ceiling; a key mask that
hides some keys of sample 0 and ALL keys of sample 1 (a null-only row); p = 0.2, one case at p = 0.5.

The reference is the fp64 restatement of np.py:339-378 with the same mask (tests/cattn_dropout_util.py), so the error metric
(max-abs / max-abs reference, gpu_util.report) and the bounds are those of the unmasked kernel tests (test_gpu_long_attention.py): forward
1e-3 on the fp16 core, 2e-2 on bf16, backward 7e-2; module level the MODES of the unmasked module tests."""
import copy
from functools import lru_cache

import pytest
import torch

pytestmark = pytest.mark.gpu

from attn_dropout_util import FixedMaskDropout  # noqa: E402
from cattn_dropout_util import attention_core_drop, fixed_keep, fixed_mask_fn  # noqa: E402
from gpu_util import report  # noqa: E402
from guard_util import guard, guarded  # noqa: E402

DEV = 'cuda'
B, N = 2, 70
MODES = [('bf16x3-fwd', 1e-3, 7e-2), ('bf16', 2e-2, 7e-2)]
HEADS = [(2, 32), (3, 64), (8, 64)]
# (T key rows or None = causal self-attention over the n rows, p)
SHAPES = [(45, 0.2), (100, 0.2), (None, 0.2)]
GEOMS = [(h, dh, T, p) for h, dh in HEADS for T, p in SHAPES] + [(8, 64, 45, 0.5)]


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


@lru_cache(maxsize=None)
def _case(heads, dh, T, p, f16):
    """inputs pre-rounded to the operand type, the fixed keep mask and the fp64 reference (forward; bf16 operands: the gradients too).
    Computed once per case and shared; nobody writes to it"""
    causal = T is None
    Tk = N if causal else T
    inner = heads * dh
    dt = torch.float16 if f16 else torch.bfloat16
    torch.manual_seed(17)
    q = torch.randn(B * N, inner).to(dt)
    kv = torch.randn(B * Tk, 2 * inner).to(dt)
    nk, nv = torch.randn(heads, dh), torch.randn(heads, dh)
    wth = torch.randn(heads, heads) * 0.5 + torch.eye(heads)
    mask = torch.rand(B, Tk) > 0.3
    mask[1] = False                        # a fully masked sample attends only the null key
    dO = torch.randn(B * N, inner).to(torch.bfloat16)
    keep = fixed_keep(B, heads, N, Tk, p, seed=heads + dh + Tk)
    s = 1.0 / (1.0 - p)
    qr = q.double().reshape(B, N, heads, dh).requires_grad_(True)
    kvr = kv.double().reshape(B, Tk, 2, heads, dh).requires_grad_(True)
    nkr, nvr, wr = (t.double().requires_grad_(True) for t in (nk, nv, wth))
    o_ref = attention_core_drop(qr, kvr[:, :, 0], kvr[:, :, 1], nkr, nvr, wr, mask, dh ** -0.5, keep, s, causal=causal)
    c = dict(causal=causal, Tk=Tk, inner=inner, q=q, kv=kv, nk=nk, nv=nv, wth=wth, mask=mask, dO=dO, keep=keep, s=s, o_ref=o_ref.detach())
    if not f16:
        o_ref.backward(dO.double().reshape(B, N, heads, dh))
        c.update(dq=qr.grad, dk=kvr.grad[:, :, 0], dv=kvr.grad[:, :, 1], dW=wr.grad, dnk=nkr.grad, dnv=nvr.grad)
    return c


def _dev(K, c, heads, dh, T):
    from nuwa_pytorch_amd import ops
    g = K.cattn_geom(B, N, heads, dh, causal=c['causal'], n_keys=T)
    assert K.cattn_supported(g) and K.cattn_drop_supported(g)
    qd, kvd = c['q'].to(DEV), c['kv'].to(DEV)
    small = (c['nk'].to(DEV), c['nv'].to(DEV), c['wth'].to(DEV))
    fargs = (g, qd, kvd[:, :c['inner']], kvd[:, c['inner']:]) + small + (c['mask'].to(torch.uint8).to(DEV),)
    return g, fargs, ops.cattn_pack_keep(c['keep'].to(DEV))


def _bargs(fargs, dO, stats):
    g, qd, kd, vd, nk, nv, wth, md = fargs
    return (g, qd, kd, vd, dO.to(DEV), nk, nv, wth, stats, md)


def _flat(o, stats=None):
    """every array a forward call leaves"""
    return [t for t in (o.hi, o.lo, o.f16, stats) if t is not None]


def _bflat(r):
    return [r[0].hi, r[1].hi] + list(r[2:])


@pytest.mark.parametrize('heads,dh,T,p', GEOMS)
@pytest.mark.parametrize('f16', [True, False])
def test_masked_kernels_against_the_fp64_restatement(K, f16, heads, dh, T, p):
    """o (both output forms on the fp16 core), dq, dk, dv, dW_th, dnull_k, dnull_v against the fp64 restatement with the same mask and s"""
    c = _case(heads, dh, T, p, f16)
    g, fargs, keep = _dev(K, c, heads, dh, T)
    kw = dict(keep=keep, drop_scale=c['s'])
    tag = f'[f16={f16},{heads},{dh},{N}x{c["Tk"]},c={c["causal"]},p={p}]'
    o, stats = K.cattn_fwd(*fargs, **kw)
    report('cattn_drop_fwd' + tag, (o.hi.float() + o.lo.float()).reshape(B, N, heads, dh), c['o_ref'], 1e-3 if f16 else 2e-2)
    o2, _ = K.cattn_fwd(*fargs, o_f16=True, **kw)
    assert torch.equal(o2.hi, o.hi)
    report('cattn_drop_fwd.o_f16' + tag, o2.f16.float().reshape(B, N, heads, dh), c['o_ref'], 1e-3 if f16 else 2e-2)
    if f16:
        return
    dq, dkv, dwth, dnk, dnv = K.cattn_bwd(*_bargs(fargs, c['dO'], stats), **kw)
    report('cattn_drop_bwd.dq' + tag, dq.hi.float().reshape(B, N, heads, dh), c['dq'], 7e-2)
    dkvg = dkv.hi.float().reshape(B, c['Tk'], 2, heads, dh)
    report('cattn_drop_bwd.dk' + tag, dkvg[:, :, 0], c['dk'], 7e-2)
    report('cattn_drop_bwd.dv' + tag, dkvg[:, :, 1], c['dv'], 7e-2)
    report('cattn_drop_bwd.dW' + tag, dwth, c['dW'], 7e-2)
    report('cattn_drop_bwd.dnull_k' + tag, dnk, c['dnk'], 7e-2)
    report('cattn_drop_bwd.dnull_v' + tag, dnv, c['dnv'], 7e-2)


@pytest.mark.parametrize('heads,dh,T,p', GEOMS[:-1])
def test_all_ones_mask_gives_the_bits_of_the_unmasked_calls(K, heads, dh, T, p):
    """keep = 1 everywhere, drop_scale = 1: forward (fp16 and bf16 operands, every output form, the statistics) and backward bit for bit"""
    from nuwa_pytorch_amd import ops
    for f16 in (True, False):
        c = _case(heads, dh, T, p, f16)
        g, fargs, _ = _dev(K, c, heads, dh, T)
        ones = ops.cattn_pack_keep(torch.ones_like(c['keep']).to(DEV))
        kw = dict(keep=ones, drop_scale=1.0)
        for okw in (dict(), dict(o_f16=True), dict(lo=False)):
            a, b = K.cattn_fwd(*fargs, **okw), K.cattn_fwd(*fargs, **okw, **kw)
            for x, y in zip(_flat(*a), _flat(*b)):
                assert torch.equal(x, y), (f16, okw)
        if not f16:
            stats = a[1]
            ra, rb = K.cattn_bwd(*_bargs(fargs, c['dO'], stats)), K.cattn_bwd(*_bargs(fargs, c['dO'], stats), **kw)
            for i, (x, y) in enumerate(zip(_bflat(ra), _bflat(rb))):
                assert torch.equal(x, y), i


@pytest.mark.parametrize('heads,dh,T,p', GEOMS[:-1])
def test_padding_high_bits_and_hidden_pairs_are_unobservable(K, heads, dh, T, p):
    """garbage in the padding bytes, in the bits at or above `heads`, and in the bytes of masked or causally hidden pairs: every output bit
    for bit that of the clean mask"""
    c = _case(heads, dh, T, p, False)
    g, fargs, clean = _dev(K, c, heads, dh, T)
    Tk = c['Tk']
    gen = torch.Generator().manual_seed(99)
    rnd = lambda t: torch.randint(0, 256, t.shape, generator=gen, dtype=torch.uint8).to(DEV)
    high = 0xFF & ~((1 << heads) - 1)                                               # the bits at or above `heads`
    hidden = ~c['mask'][:, None, :].expand(B, N, Tk).clone()                       # [B, n, T]: the key is masked
    if c['causal']:
        hidden |= torch.arange(Tk)[None, None, :] > torch.arange(N)[None, :, None]
    hidden = hidden.to(DEV)
    keep, keep_t, keep0 = (t.clone() for t in clean)
    for arr, hid, w in ((keep, hidden, Tk), (keep_t, hidden.transpose(1, 2), N)):
        r = rnd(arr)
        arr[:, :, w:] = r[:, :, w:]                                                   # padding bytes
        arr[:, :, :w] = torch.where(hid, r[:, :, :w], arr[:, :, :w] | (r[:, :, :w] & high))
    keep0 |= rnd(keep0) & high
    assert not torch.equal(keep, clean[0]) and not torch.equal(keep_t, clean[1])
    outs = []
    for kp in (clean, (keep, keep_t, keep0)):
        kw = dict(keep=kp, drop_scale=c['s'])
        o, stats = K.cattn_fwd(*fargs, **kw)
        o16, _ = K.cattn_fwd(*(fargs[:1] + (c['q'].half().to(DEV), c['kv'].half().to(DEV)[:, :c['inner']], c['kv'].half().to(DEV)[:, c['inner']:]) + fargs[4:]),
                             o_f16=True, **kw)
        outs.append(_flat(o, stats) + _flat(o16) + _bflat(K.cattn_bwd(*_bargs(fargs, c['dO'], stats), **kw)))
    for i, (x, y) in enumerate(zip(*outs)):
        assert torch.equal(x, y), i


@pytest.mark.parametrize('heads,dh', HEADS)
def test_the_null_slot_alone(K, heads, dh):
    """keep = 1 on every key: with keep0 = 0 the all-masked sample's output rows are exactly zero and dnull_v is exactly zero (no query hands
    it a term); with keep0 = 1 the null-only sample's output is the unmasked one times s"""
    from nuwa_pytorch_amd import ops
    T, p = 45, 0.2
    c = _case(heads, dh, T, p, False)
    g, fargs, _ = _dev(K, c, heads, dh, T)
    keep, keep_t, keep0 = ops.cattn_pack_keep(torch.ones_like(c['keep']).to(DEV))
    s = c['s']
    o, stats = K.cattn_fwd(*fargs, keep=(keep, keep_t, torch.zeros_like(keep0)), drop_scale=s)
    got = (o.hi.float() + o.lo.float()).reshape(B, N, -1)
    assert torch.count_nonzero(got[1]) == 0 and torch.count_nonzero(o.hi.reshape(B, N, -1)[1]) == 0
    assert torch.count_nonzero(got[0]) > 0
    dnv = K.cattn_bwd(*_bargs(fargs, c['dO'], stats), keep=(keep, keep_t, torch.zeros_like(keep0)), drop_scale=s)[4]
    assert torch.count_nonzero(dnv) == 0
    plain, _ = K.cattn_fwd(*fargs)
    o1, stats1 = K.cattn_fwd(*fargs, keep=(keep, keep_t, keep0), drop_scale=s)
    # one more fp32 rounding (s . a0) in front of a hi + lo pair of 16 significant bits: 1e-4 of the largest value
    want = (plain.hi.float() + plain.lo.float()).reshape(B, N, -1) * s
    report(f'cattn_drop_null[{heads},{dh}].o', (o1.hi.float() + o1.lo.float()).reshape(B, N, -1)[1], want[1], 1e-4)
    dnv0 = K.cattn_bwd(*_bargs(fargs, c['dO'], stats))[4]
    dnv1 = K.cattn_bwd(*_bargs(fargs, c['dO'], stats1), keep=(keep, keep_t, keep0), drop_scale=s)[4]
    report(f'cattn_drop_null[{heads},{dh}].dnull_v', dnv1, dnv0 * s, 1e-4)


@pytest.mark.parametrize('heads,dh,T,p', [(8, 64, 45, 0.2), (3, 64, None, 0.2), (2, 32, 100, 0.2)])
def test_two_runs_are_identical_inside_guard_bands(K, heads, dh, T, p):
    """outputs allocated NaN-prefilled between guard bands (guard_util): every element is written (finite), nothing outside is, and a
    second run gives the same bits.  The mask arrays sit in guarded buffers too: nothing writes them or next to them"""
    c = _case(heads, dh, T, p, False)
    g, fargs, keep = _dev(K, c, heads, dh, T)
    keep = tuple(guarded(t) for t in keep)
    kw = dict(keep=keep, drop_scale=c['s'])
    runs = []
    with guard(K) as gd:
        for _ in range(2):
            o, stats = K.cattn_fwd(*fargs, **kw)
            o16, _ = K.cattn_fwd(*fargs, o_f16=True, **kw)
            runs.append(_flat(o, stats) + _flat(o16) + _bflat(K.cattn_bwd(*_bargs(fargs, c['dO'], stats), **kw)))
        assert gd.made() > 0
    for i, (x, y) in enumerate(zip(*runs)):
        assert torch.isfinite(x.float()).all(), i
        assert torch.equal(x, y), i


# ---- module level ------------------------------------------------------------------------------------------------------------------------

class _Kinds:
    """records (kind, drop_p) of every ops.InnerFn.forward while active"""

    def __enter__(self):
        from nuwa_pytorch_amd import ops
        self.ops, self.orig, self.seen = ops, ops.InnerFn.forward, []

        def spy(ctx_, x, context, meta, *p):
            self.seen.append((meta['kind'], meta.get('drop_p')))
            return self.orig(ctx_, x, context, meta, *p)
        ops.InnerFn.forward = staticmethod(spy)
        return self

    def __exit__(self, *exc):
        self.ops.InnerFn.forward = self.orig


@pytest.fixture
def on_kernels(monkeypatch):
    from nuwa_pytorch_amd.nuwa_pytorch import Attention
    monkeypatch.setattr(Attention, 'dropout_on_kernels', True)


@pytest.mark.parametrize('form', ['context', 'causal', 'self+rotary'])
@pytest.mark.parametrize('mode,tol,gtol', MODES)
def test_module_against_the_torch_route_with_the_same_mask(A, monkeypatch, on_kernels, mode, tol, gtol, form):
    """Attention with a 45-key context (context mask, one sample wholly masked), causal self-attention, self-attention with rotary over 300
    rows: y, dx, dcontext and every parameter gradient against _forward_torch (fp32, CPU) with FixedMaskDropout of the same mask"""
    from nuwa_pytorch_amd import ops
    from nuwa_pytorch_amd.nuwa_pytorch import RotaryEmbedding
    p, heads = 0.2, 8
    s = 1.0 / (1.0 - p)
    torch.manual_seed(31)
    n = 300 if form == 'self+rotary' else N
    m = A.Attention(dim=512, heads=heads, dim_head=64, causal=form == 'causal', dropout=p).train()
    x = torch.randn(B, n, 512)
    dy = torch.randn(B, n, 512)
    kw, T = {}, n
    if form == 'context':
        T = 45
        cm = torch.rand(B, T) > 0.3
        cm[1] = False
        kw = dict(context=torch.randn(B, T, 512), context_mask=cm)
    else:
        kw = dict(mask=torch.rand(B, n) > 0.2)
        if form == 'self+rotary':
            kw['rotary_pos_emb'] = RotaryEmbedding(dim=32)(n, device='cpu')
    keep = fixed_keep(B, heads, n, T, p, seed=7)
    # the torch-op route of the same module with the same mask
    ref = copy.deepcopy(m)
    ref.dropout = FixedMaskDropout(keep, s)
    leaf = lambda t: t.clone().requires_grad_(True) if t.is_floating_point() and t.dim() == 3 else t
    rkw = {k: leaf(v) for k, v in kw.items()}
    xr = x.clone().requires_grad_(True)
    y_ref = ref._forward_torch(xr, **rkw)
    y_ref.backward(dy)
    assert ref.dropout.calls == 1
    # the kernel route
    md = m.to(DEV)
    md.dropout = FixedMaskDropout(keep, s)
    fn = fixed_mask_fn(keep)
    monkeypatch.setattr(ops, '_cattn_keep_mask', fn)
    A.set_precision(mode)
    try:
        dkw = {k: leaf(v.to(DEV)) for k, v in kw.items()}
        xg = x.to(DEV).requires_grad_(True)
        with _Kinds() as spy:
            y = md(xg, **dkw)
            y.backward(dy.to(DEV))
        tag = f'cattn_drop_module[{form},{mode}]'
        report(tag + '.y', y, y_ref, tol)
        report(tag + '.dx', xg.grad, xr.grad, gtol)
        if form == 'context':
            report(tag + '.dcontext', dkw['context'].grad, rkw['context'].grad, gtol)
        G = dict(ref.named_parameters())
        for k, prm in md.named_parameters():
            report(tag + '.grad.' + k, prm.grad, G[k].grad, gtol)
        assert len(spy.seen) == 1 and spy.seen[0][0] == 'cattn' and spy.seen[0][1] == pytest.approx(p)
        assert md.dropout.calls == 0 and fn.calls == 1
    finally:
        A.set_precision('bf16')


def test_routing(A, monkeypatch):
    from nuwa_pytorch_amd.nuwa_pytorch import Attention
    x = torch.randn(2, 40, 64, device=DEV)
    ctx = lambda T: torch.randn(2, T, 64, device=DEV)
    d = A.Attention(dim=64, heads=2, dim_head=32, dropout=0.1).to(DEV).train()
    dc = A.Attention(dim=64, heads=2, dim_head=32, causal=True, dropout=0.1).to(DEV).train()
    with _Kinds() as spy:
        # as shipped: a training module with live dropout launches no kernel node, as on the parent
        assert Attention.dropout_on_kernels is False
        d(x, context=ctx(45)), d(x, context=ctx(320)), d(x), dc(x)
        assert spy.seen == []
        monkeypatch.setattr(Attention, 'dropout_on_kernels', True)
        for T in (45, 287, 288):
            d(x, context=ctx(T))
            d(torch.randn(2, T, 64, device=DEV))
        dc(x)
        assert spy.seen == [('cattn', 0.1)] * 7
        del spy.seen[:]
        # eval mode and p = 0 take the unmasked routes
        d.eval(), dc.eval()
        d(x, context=ctx(45)), dc(x)
        assert spy.seen == [('xattn', None), ('cattn', None)]
        del spy.seen[:]
        d.train(), dc.train()
        z = A.Attention(dim=64, heads=2, dim_head=32, dropout=0.).to(DEV).train()
        z(x, context=ctx(45)), z(x, context=ctx(320))
        assert spy.seen == [('xattn', None)]                       # (320 keys at this size: below the long-key gate, torch ops)
        del spy.seen[:]
        # causal attention with a context keeps torch ops; so does the parity mode
        dc(x, context=ctx(45))
        assert spy.seen == []
        A.set_precision('bf16x3')
        try:
            d(x, context=ctx(45)), dc(x)
            assert spy.seen == []
        finally:
            A.set_precision('bf16')
        # an instance may opt in alone
        monkeypatch.setattr(Attention, 'dropout_on_kernels', False)
        d.dropout_on_kernels = True
        d(x, context=ctx(45)), dc(x)
        assert spy.seen == [('cattn', 0.1)]


# ---- stacks ------------------------------------------------------------------------------------------------------------------------------

def _stack(A, reversible):
    torch.manual_seed(21)
    cls = A.ReversibleTransformer if reversible else A.Transformer
    net = cls(dim=64, depth=2, causal=True, heads=2, dim_head=32, cross_attend=True, attn_dropout=0.2, sparse_3dna_attn=True,
              sparse_3dna_video_shape=(2, 4, 4), sparse_3dna_kernel_size=3).to(DEV).train()
    g = torch.Generator().manual_seed(4)
    x0 = torch.randn(2, 33, 64, generator=g).to(DEV)
    c0 = torch.randn(2, 12, 64, generator=g).to(DEV)
    cmask = (torch.rand(2, 12, generator=g) > 0.2).to(DEV)
    tgt = torch.randn(2, 33, 64, generator=g).to(DEV)

    def run(before_backward=None):
        net.zero_grad(set_to_none=True)
        x, c = x0.clone().requires_grad_(True), c0.clone().requires_grad_(True)
        loss = ((net(x, context=c, context_mask=cmask) - tgt) ** 2).mean()
        if before_backward is not None:
            before_backward()
        loss.backward()
        return loss.detach(), [x.grad.clone(), c.grad.clone()], {k: q.grad.clone() for k, q in net.named_parameters() if q.grad is not None}
    return net, run


def _kinds_of_blocks(monkeypatch, run):
    from nuwa_pytorch_amd import ops
    kinds, orig = [], ops.SandwichBlockFn.forward

    def spy(ctx_, x, resid, context, meta, *rest):
        kinds.append((meta['kind'], meta.get('drop_p')))
        return orig(ctx_, x, resid, context, meta, *rest)
    with monkeypatch.context() as mp:
        mp.setattr(ops.SandwichBlockFn, 'forward', staticmethod(spy))
        out = run()
    return kinds, out


@pytest.mark.parametrize('mode', ['bf16x3-fwd', 'bf16'])
def test_reversible_stack_replays_its_masks(A, monkeypatch, on_kernels, mode):
    """the masks drawn while the reversible backward recomputes its blocks are the forward's, block for block (last block first), and the
    main RNG stream leaves the backward where it entered; the same seed twice: the same bits; another seed: another loss"""
    from nuwa_pytorch_amd import ops
    net, run = _stack(A, True)
    drawn, orig = [], ops._cattn_keep_mask

    def spy(*a):
        out = orig(*a)
        drawn.append(tuple(t.clone() for t in out))
        return out
    monkeypatch.setattr(ops, '_cattn_keep_mask', spy)
    A.set_precision(mode)
    try:
        states = []
        torch.manual_seed(1234)
        kinds, first = _kinds_of_blocks(monkeypatch, lambda: run(lambda: states.append(torch.cuda.get_rng_state())))
        states.append(torch.cuda.get_rng_state())
        assert torch.equal(states[0], states[1])
        assert kinds.count(('cattn', 0.2)) == 4, kinds                      # two cross-attention blocks, forward and recomputation, fused
        assert len(drawn) == 4
        fwd, again = drawn[:2], drawn[2:]
        for a, b in zip(fwd, again[::-1]):
            assert all(torch.equal(x, y) for x, y in zip(a, b))
        assert not torch.equal(fwd[0][0], fwd[1][0])
        torch.manual_seed(1234)
        second = run()
        assert torch.equal(first[0], second[0])
        for a, b in zip(first[1], second[1]):
            assert torch.equal(a, b)
        assert set(first[2]) == set(second[2]) and all(torch.equal(first[2][k], second[2][k]) for k in first[2])
        torch.manual_seed(4321)
        assert not torch.equal(run()[0], first[0])
    finally:
        A.set_precision('bf16')


@pytest.mark.parametrize('mode,tol,gtol', MODES)
@pytest.mark.parametrize('reversible', [False, True])
def test_stacks_against_the_torch_route_with_the_same_mask(A, monkeypatch, reversible, mode, tol, gtol):
    """Transformer / ReversibleTransformer with the cross-attention dropout on the kernels against the same stack on the torch-op route, one
    fixed mask on either side: loss, dx, dcontext and every gradient"""
    from nuwa_pytorch_amd import ops
    from nuwa_pytorch_amd.nuwa_pytorch import Attention
    net, run = _stack(A, reversible)
    keep = fixed_keep(2, 2, 33, 12, 0.2, seed=8)
    for mod in net.modules():
        if isinstance(mod, Attention):
            mod.dropout = FixedMaskDropout(keep, 1.25)
    A.set_precision(mode)
    try:
        loss_ref, leaves_ref, G = run()                                    # as shipped: the torch-op route for live dropout
        assert all(mod.dropout.calls >= 1 for mod in net.modules() if isinstance(mod, Attention))
        calls = sum(mod.dropout.calls for mod in net.modules() if isinstance(mod, Attention))
        fn = fixed_mask_fn(keep)
        monkeypatch.setattr(ops, '_cattn_keep_mask', fn)
        monkeypatch.setattr(Attention, 'dropout_on_kernels', True)
        kinds, (loss, leaves, Gn) = _kinds_of_blocks(monkeypatch, run)
        dropped = [k for k, dp in kinds if k == 'cattn' and dp == pytest.approx(0.2)]
        assert len(dropped) == (4 if reversible else 2) and fn.calls == (4 if reversible else 2), kinds
        assert sum(mod.dropout.calls for mod in net.modules() if isinstance(mod, Attention)) == calls
        tag = f'cattn_drop_stack[rev={reversible},{mode}]'
        report(tag + '.loss', loss.reshape(1), loss_ref.reshape(1), tol)
        for i, (a, b) in enumerate(zip(leaves, leaves_ref)):
            report(tag + f'.dinput{i}', a, b, gtol)
        assert set(Gn) == set(G)
        for k in G:
            report(tag + '.grad.' + k, Gn[k], G[k], gtol)
    finally:
        A.set_precision('bf16')
