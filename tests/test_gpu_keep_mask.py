"""The dropout mask generator kernels (csrc/keepmask.hip) on the MI355X against the numpy restatement of their decision function
(tests/keep_mask_util.py), bit for bit, and the modules under ops.set_keep_mask_source('device').

Kernel level: every output sits NaN / 0xFF-prefilled between guard bands (tests/guard_util.py), so a byte the kernel skips and a byte it writes
outside are both seen.  Shapes: counts below, at and above the 16-byte pieces from bases at 0, 1 and 5 bytes past a 16-byte boundary; element
ranges that start inside a Philox group and one that crosses the counter's high word; cattn tiles (64 x 64) that are ragged, single and
several, 3 / 8 / 1 heads, one call whose element index crosses 2^34, one whose arrays are only 4-byte aligned.

Module level: a spy on the kernel wrappers records the seed words of every launch; the mask is restated on the CPU from them and handed to the
references the fixed-mask dropout tests use, at their bounds: test_gpu_cattn_dropout.py (MODES: 1e-3 / 2e-2 forward, 7e-2 gradients),
test_gpu_attn_dropout.py and test_gpu_modules.py (MODES: 1e-3 / 2e-3, 1e-3 / 7e-2, 2e-2 / 7e-2).  The masked kernels are the same, so are the bounds."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import keep_mask_util as KM  # noqa: E402
from attn_dropout_util import keep_to_bhij, sparse_causal_2dna_drop  # noqa: E402
from cattn_dropout_util import attention_drop  # noqa: E402
from gpu_util import report  # noqa: E402
from guard_util import FILL, guard, guarded_empty  # noqa: E402

DEV = 'cuda'
P_DROP = 0.25
S = 1.0 / (1.0 - P_DROP)
THR = KM.keep_threshold(P_DROP)
SEED = (0x243f6a88, 0x13198a2e)
CATTN_MODES = [('bf16x3-fwd', 1e-3, 7e-2), ('bf16', 2e-2, 7e-2)]
MODES = [('bf16x3', 1e-3, 2e-3), ('bf16x3-fwd', 1e-3, 7e-2), ('bf16', 2e-2, 7e-2)]


@pytest.fixture(scope='module')
def A():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import nuwa_pytorch_amd
    return nuwa_pytorch_amd


@pytest.fixture(scope='module')
def K(A):
    from nuwa_pytorch_amd import kernels
    return kernels


@pytest.fixture
def device_source(A):
    from nuwa_pytorch_amd import ops
    ops.set_keep_mask_source('device')
    yield ops
    ops.set_keep_mask_source('torch')


def _seed(words=SEED, high=0):
    """two int64 seed words on the device; `high` fills the upper halves, which the kernels ignore"""
    return torch.tensor([(high << 32) | words[0], (high << 32) | words[1]], dtype=torch.int64, device=DEV)


def _words(seed_t):
    return tuple(int(v) & 0xFFFFFFFF for v in seed_t.tolist())


class _Spy:
    """records (wrapper name, arguments, a device copy of the seed) of every generator launch while active"""

    def __init__(self, monkeypatch, K):
        self.calls = []
        lin0, cat0 = K.keep_mask_linear, K.keep_mask_cattn

        def lin(count, thr, seed, e0=0, out=None):
            self.calls.append(('linear', (count, thr, e0), seed.clone()))
            return lin0(count, thr, seed, e0=e0, out=out)

        def cat(B, n, T, heads, thr, seed, b_first=0, out=None):
            self.calls.append(('cattn', (B, n, T, heads, thr, b_first), seed.clone()))
            return cat0(B, n, T, heads, thr, seed, b_first=b_first, out=out)
        monkeypatch.setattr(K, 'keep_mask_linear', lin)
        monkeypatch.setattr(K, 'keep_mask_cattn', cat)

    def seeds(self):
        return [(name, _words(s)) for name, _, s in self.calls]


@pytest.fixture
def spy(monkeypatch, K):
    return _Spy(monkeypatch, K)


# ---------------------------------------------------------------------------------------------------
# 1. the linear kernel
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('e0', [0, 2, (1 << 34) - 32])
@pytest.mark.parametrize('off', [0, 1, 5])
def test_linear_is_the_restatement_bit_for_bit(K, e0, off):
    """count 1, 3, 70, 4099 from a base `off` bytes past a 16-byte boundary; (1 << 34) - 32 crosses the counter's high word after 32 elements"""
    seed = _seed(high=0x5a5a5a5a)
    bufs = []
    for count in (1, 3, 70, 4099):
        buf = guarded_empty((16 + off + count + 7,), torch.uint8, DEV)
        assert buf.data_ptr() % 16 == 0
        out = buf[16 + off:16 + off + count]
        assert K.keep_mask_linear(count, THR, seed, e0=e0, out=out) is out
        bufs.append((count, buf, out))
    with guard(K):                                                  # (checks the bands of the buffers above on exit)
        pass
    for count, buf, out in bufs:
        want = torch.from_numpy(KM.linear_keep(count, THR, SEED, e0=e0))
        assert torch.equal(out.cpu(), want), (count, off, e0)
        assert bool((buf[:16 + off] == FILL).all()) and bool((buf[16 + off + count:] == FILL).all()), (count, off, e0)
    if e0:
        assert 0 < int(want.sum()) < 4099


def test_the_two_linear_producers(K, device_source, spy):
    """ops._ff_keep_mask [R = 5, C = 70] and ops._attn_keep_mask [B = 2, nq = 7, J = 11, heads = 3] under 'device': bool tensors of today's shapes
    holding the restated decisions of e = r * C + c and of the storage index, from seed words drawn on the device"""
    ops = device_source
    torch.manual_seed(3)
    with guard(K) as gd:
        ff = ops._ff_keep_mask(5, 70, P_DROP, torch.device(DEV))
        at = ops._attn_keep_mask(2, 7, 11, 3, P_DROP, torch.device(DEV))
        assert gd.made() >= 2
    assert ff.dtype == torch.bool and tuple(ff.shape) == (5, 70) and at.dtype == torch.bool and tuple(at.shape) == (2, 7, 11, 3)
    assert ff.is_contiguous() and at.is_contiguous()
    (n0, a0, s0), (n1, a1, s1) = spy.calls
    assert (n0, a0) == ('linear', (350, THR, 0)) and (n1, a1) == ('linear', (2 * 7 * 11 * 3, THR, 0))
    assert _words(s0) != _words(s1)
    assert torch.equal(ff.cpu(), torch.from_numpy(KM.keep_of(KM.ff_elements(5, 70), THR, _words(s0))))
    assert torch.equal(at.cpu(), torch.from_numpy(KM.keep_of(KM.attn_elements(2, 7, 11, 3), THR, _words(s1))))
    assert torch.equal(ff.view(torch.uint8).cpu(), ff.cpu().to(torch.uint8))                # the bytes are 0 / 1


# ---------------------------------------------------------------------------------------------------
# 2. the cattn kernel
# ---------------------------------------------------------------------------------------------------

def _b_first_crossing(n, T, B, bit=34):
    """first logical sample of a B-sample call whose element index passes 2^bit inside the call"""
    per = n * (T + 1) * 8
    b_first = (1 << bit) // per - B // 2
    assert b_first * per < (1 << bit) < (b_first + B) * per
    return b_first


def _cattn_outputs(K, B, n, T, shift=0):
    """the three arrays, 0xFF-prefilled between guard bands; shift: bytes past the (16-byte aligned) start of the payload"""
    outs = []
    for shape in ((B, n, -(-T // 32) * 32), (B, T, -(-n // 32) * 32), (B, n)):
        buf = guarded_empty((shift + int(np.prod(shape)),), torch.uint8, DEV)
        outs.append((buf, buf[shift:].view(shape)))
    return outs


@pytest.mark.parametrize('B,heads,n,T,b_first,shift', [(2, 3, 37, 45, 0, 0), (2, 8, 37, 45, 0, 0), (1, 8, 33, 1, 0, 0), (3, 1, 1, 65, 0, 0),
                                                       (2, 8, 37, 45, 'cross', 0), (2, 3, 37, 45, 0, 4), (1, 5, 70, 130, 7, 0)])
def test_cattn_arrays_are_pack_keep_of_the_restated_mask(K, B, heads, n, T, b_first, shift):
    """keep, keep_t, keep0 equal ops.cattn_pack_keep of the restated boolean mask -- padding bytes and the bits at or above `heads` included
    (both zero).  'cross': the element index passes 2^34 between the two samples' ends; shift = 4: bases that are 4- but not 16-byte aligned;
    (70, 130): two query tiles and three key tiles, both ragged"""
    from nuwa_pytorch_amd import ops
    if b_first == 'cross':
        b_first = _b_first_crossing(n, T, B)
    outs = _cattn_outputs(K, B, n, T, shift)
    got = K.keep_mask_cattn(B, n, T, heads, THR, _seed(), b_first=b_first, out=tuple(v for _, v in outs))
    with guard(K):
        pass
    want = ops.cattn_pack_keep(torch.from_numpy(KM.cattn_keep(B, n, T, heads, THR, SEED, b_first=b_first)))
    for name, g, w, (buf, _) in zip(('keep', 'keep_t', 'keep0'), got, want, outs):
        assert torch.equal(g.cpu(), w), name
        assert bool((buf[:shift] == FILL).all()), name
    assert int(got[0].max()) < (1 << heads) and int(got[0].max()) > 0
    # three renderings of the same decisions
    assert torch.equal(got[0][:, :, :T].transpose(1, 2), got[1][:, :, :n])


def test_cattn_producer_returns_the_kernels_arrays(K, device_source, spy):
    ops = device_source
    torch.manual_seed(4)
    with guard(K) as gd:
        got = ops._cattn_keep_mask(2, 37, 45, 3, P_DROP, torch.device(DEV))
        assert gd.made() == 3
    (name, args, s), = spy.calls
    assert name == 'cattn' and args == (2, 37, 45, 3, THR, 0)
    g = K.cattn_geom(2, 37, 3, 64, causal=False, n_keys=45)
    assert [tuple(t.shape) for t in got] == [tuple(sh) for sh in K.cattn_keep_shapes(g)] and all(t.dtype == torch.uint8 for t in got)
    want = ops.cattn_pack_keep(torch.from_numpy(KM.cattn_keep(2, 37, 45, 3, THR, _words(s))))
    assert all(torch.equal(a.cpu(), b) for a, b in zip(got, want))


# ---------------------------------------------------------------------------------------------------
# 3. seeds
# ---------------------------------------------------------------------------------------------------

def test_seeds(K):
    """the same seed twice: identical bytes; another seed: other bytes; the upper halves of the seed words are ignored; a seed written on the
    device between two launches, with no host synchronisation in between, changes the output -- the kernel reads the seed when it runs"""
    run = lambda s: (K.keep_mask_linear(4099, THR, s),) + K.keep_mask_cattn(2, 37, 45, 8, THR, s)
    seed = _seed()
    a, b = run(seed), run(_seed(high=0x1234))
    other = run(_seed((SEED[0] + 1, SEED[1])))
    other2 = run(_seed((SEED[0], SEED[1] ^ 0x80000000)))
    for x, y, z, w in zip(a, b, other, other2):
        assert torch.equal(x, y) and not torch.equal(x, z) and not torch.equal(x, w) and not torch.equal(z, w)
    s = _seed()
    bump = torch.tensor([1, 0], dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    first = run(s)
    s.add_(bump)                                     # stream-ordered between the launches; nothing waits on the host
    second = run(s)
    for x, y, x0, y0 in zip(first, second, a, other):
        assert torch.equal(x, x0) and torch.equal(y, y0) and not torch.equal(x, y)


# ---------------------------------------------------------------------------------------------------
# 4. modules under 'device'
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('mode,tol,gtol', CATTN_MODES)
@pytest.mark.parametrize('form', ['context', 'causal'])
def test_attention_on_kernels_with_a_generated_mask(A, K, device_source, spy, monkeypatch, mode, tol, gtol, form):
    """Attention(dropout = 0.25, dropout_on_kernels) with a context of 45 keys / as causal self-attention of 37 rows: y and every gradient against
    the fp64 restatement (cattn_dropout_util.attention_drop) with the mask restated from the recorded seed"""
    from nuwa_pytorch_amd.nuwa_pytorch import Attention
    monkeypatch.setattr(Attention, 'dropout_on_kernels', True)
    B, n, dim, heads = 2, 37, 64, 2
    torch.manual_seed(41)
    m = A.Attention(dim=dim, heads=heads, dim_head=32, causal=form == 'causal', dropout=P_DROP).train()
    x, dy = torch.randn(B, n, dim), torch.randn(B, n, dim)
    T, ctx, cm = n, None, None
    if form == 'context':
        T = 45
        ctx = torch.randn(B, T, dim)
        cm = torch.rand(B, T) > 0.3
    P = {k: v.detach().double().requires_grad_(True) for k, v in m.state_dict().items()}
    md = m.to(DEV)
    A.set_precision(mode)
    try:
        xg = x.to(DEV).requires_grad_(True)
        cg = ctx.to(DEV).requires_grad_(True) if ctx is not None else None
        y = md(xg, context=cg, context_mask=cm.to(DEV)) if ctx is not None else md(xg)
        y.backward(dy.to(DEV))
    finally:
        A.set_precision('bf16')
    (name, args, s), = spy.calls
    assert name == 'cattn' and args == (B, n, T, heads, THR, 0)
    keep = torch.from_numpy(KM.cattn_keep(B, n, T, heads, THR, _words(s)))
    xr = x.double().requires_grad_(True)
    cr = ctx.double().requires_grad_(True) if ctx is not None else None
    yr = attention_drop(xr, P, heads, keep, S, None, context=cr, context_mask=cm, causal=form == 'causal')
    yr.backward(dy.double())
    tag = f'keep_mask_attention[{form},{mode}]'
    report(tag + '.y', y, yr.detach(), tol)
    report(tag + '.dx', xg.grad, xr.grad, gtol)
    if ctx is not None:
        report(tag + '.dcontext', cg.grad, cr.grad, gtol)
    got = {k: p.grad for k, p in md.named_parameters()}
    assert set(got) == set(P)
    for k, gr in got.items():
        report(tag + '.grad.' + k, gr, P[k].grad.reshape(gr.shape), gtol)


@pytest.mark.parametrize('mode,tol,gtol', MODES)
def test_sparse_causal_2dna_with_a_generated_mask(A, K, device_source, spy, mode, tol, gtol):
    """SparseCausal2DNA(dropout = 0.25) at the shape of test_gpu_attn_dropout.py: y and every gradient against the fp64 restatement
    (attn_dropout_util.sparse_causal_2dna_drop) with the mask restated from the recorded seed"""
    from nuwa_pytorch_amd import video_audio as VA
    torch.manual_seed(0)
    heads, ks, dil, b, n, dim = 2, 5, 2, 2, 34, 64
    m = VA.SparseCausal2DNA(dim=dim, heads=heads, dim_head=32, kernel_size=ks, dilation=dil, dropout=P_DROP).train()
    g = torch.Generator().manual_seed(7)
    x, dy = torch.randn(b, n, dim, generator=g), torch.randn(b, n, dim, generator=g)
    P = {k: v.detach().double().requires_grad_(True) for k, v in m.state_dict().items()}
    md = m.to(DEV)
    A.set_precision(mode)
    try:
        xd = x.to(DEV).requires_grad_(True)
        y = md(xd)
        y.backward(dy.to(DEV))
    finally:
        A.set_precision('bf16')
    (name, args, s), = spy.calls
    assert name == 'linear' and args == (b * (n - 1) * (ks + 1) * heads, THR, 0)
    keep = torch.from_numpy(KM.keep_of(KM.attn_elements(b, n - 1, ks + 1, heads), THR, _words(s)))
    xr = x.double().requires_grad_(True)
    yr = sparse_causal_2dna_drop(xr, P, heads, ks, dil, keep_to_bhij(keep), S)
    yr.backward(dy.double())
    tag = f'keep_mask_sc2dna[{mode}]'
    report(tag + '.y', y, yr.detach(), tol)
    report(tag + '.dx', xd.grad, xr.grad, gtol)
    got = {k: p.grad for k, p in md.named_parameters() if p.grad is not None}
    assert set(got) == set(P)
    for k, gr in got.items():
        report(tag + f'.grad.{k}', gr, P[k].grad, gtol)


@pytest.mark.parametrize('mode,tol,gtol', MODES)
@pytest.mark.parametrize('dim', [64, 512])
def test_feedforward_with_a_generated_mask(A, K, device_source, spy, dim, mode, tol, gtol):
    """FeedForward(dropout = 0.25) as test_gpu_modules.py::test_feedforward_dropout_runs_on_the_library checks it: forward and every gradient
    against the same arithmetic in torch fp32 with the mask restated from the recorded seed (e = r * C + c over the PADDED gate width)"""
    torch.manual_seed(11)
    m = A.FeedForward(dim=dim, dropout=P_DROP).to(DEV).train()
    w1, w2 = m.net[0].weight, m.net[3].weight
    FFI = w2.shape[1]
    FP = (FFI + 31) // 32 * 32
    x = torch.randn(2, 48, dim, device=DEV, requires_grad=True)
    dy = torch.randn(2, 48, dim, device=DEV)
    A.set_precision(mode)
    try:
        y = m(x)
        y.backward(dy)
    finally:
        A.set_precision('bf16')
    got = (y.detach().clone(), x.grad.clone(), w1.grad.clone(), w2.grad.clone())
    for t in (x, w1, w2):
        t.grad = None
    (name, args, s), = spy.calls
    assert name == 'linear' and args == (96 * FP, THR, 0)
    keep = torch.from_numpy(KM.keep_of(KM.ff_elements(96, FP), THR, _words(s))).to(DEV)
    assert 0.6 < float(keep.float().mean()) < 0.9
    u = x.reshape(96, dim) @ w1.t()
    a, g = u.chunk(2, dim=-1)
    gg = torch.where(keep[:, :FFI], a * F.gelu(g) * (1.0 / (1.0 - P_DROP)), torch.zeros((), device=DEV))
    yr = (gg @ w2.t()).reshape(2, 48, dim)
    yr.backward(dy)
    tag = f'keep_mask_ff[{dim},{mode}]'
    report(tag + '.y', got[0], yr.detach(), tol)
    report(tag + '.dx', got[1], x.grad, gtol)
    report(tag + '.dw1', got[2], w1.grad, gtol)
    report(tag + '.dw2', got[3], w2.grad, gtol)


# ---------------------------------------------------------------------------------------------------
# 5. a reversible stack
# ---------------------------------------------------------------------------------------------------

def test_reversible_stack_replays_its_seeds(A, K, device_source, spy, monkeypatch):
    """a reversible stack of depth 2 (window attention / FeedForward and cross attention / FeedForward blocks) with attn_dropout = ff_dropout =
    0.25: the seeds drawn while the backward recomputes its sub-blocks are the
    forward's, sub-block for sub-block (last first); the device generator leaves the backward where it entered; the same torch seed twice gives
    the same bits"""
    from nuwa_pytorch_amd.nuwa_pytorch import Attention
    monkeypatch.setattr(Attention, 'dropout_on_kernels', True)
    torch.manual_seed(21)
    net = A.ReversibleTransformer(dim=64, depth=2, causal=True, heads=2, dim_head=32, cross_attend=True, attn_dropout=P_DROP, ff_dropout=P_DROP,
                                  sparse_3dna_attn=True, sparse_3dna_video_shape=(2, 4, 4), sparse_3dna_kernel_size=3).to(DEV).train()
    g = torch.Generator().manual_seed(4)
    x0, c0 = torch.randn(2, 33, 64, generator=g).to(DEV), torch.randn(2, 12, 64, generator=g).to(DEV)
    cmask = (torch.rand(2, 12, generator=g) > 0.2).to(DEV)
    tgt = torch.randn(2, 33, 64, generator=g).to(DEV)
    marks = []

    def run():
        net.zero_grad(set_to_none=True)
        x, c = x0.clone().requires_grad_(True), c0.clone().requires_grad_(True)
        loss = ((net(x, context=c, context_mask=cmask) - tgt) ** 2).mean()
        marks.append((len(spy.calls), torch.cuda.get_rng_state()))
        loss.backward()
        marks.append((len(spy.calls), torch.cuda.get_rng_state()))
        return [loss.detach(), x.grad.clone(), c.grad.clone()] + [q.grad.clone() for q in net.parameters() if q.grad is not None]
    torch.manual_seed(1234)
    first = run()
    (nf, state_f), (nb, state_b) = marks
    assert torch.equal(state_f, state_b)
    seeds = spy.seeds()
    fwd, again = seeds[:nf], seeds[nf:nb]
    # per layer: FeedForward, cross attention, FeedForward (the Sparse3DNA of a reversible stack takes no dropout, as in the reference)
    assert [n for n, _ in fwd] == ['linear', 'cattn', 'linear'] * 2, fwd
    assert again == fwd[::-1]
    assert len(set(fwd)) == len(fwd)
    torch.manual_seed(1234)
    second = run()
    assert len(first) == len(second) > 10 and all(torch.equal(a, b) for a, b in zip(first, second))
    assert spy.seeds()[nb:] == seeds
    torch.manual_seed(4321)
    assert not torch.equal(run()[0], first[0])


# ---------------------------------------------------------------------------------------------------
# 6. the default route
# ---------------------------------------------------------------------------------------------------

def test_default_route_is_the_torch_draw(A, K, spy):
    from nuwa_pytorch_amd import ops
    assert ops.get_keep_mask_source() == 'torch'
    dev = torch.device(DEV)
    torch.manual_seed(77)
    ff = ops._ff_keep_mask(5, 70, .25, dev)
    at = ops._attn_keep_mask(2, 7, 11, 3, .25, dev)
    ca = ops._cattn_keep_mask(2, 37, 45, 3, .25, dev)
    torch.manual_seed(77)
    assert torch.equal(ff, torch.rand((5, 70), device=dev) >= .25)
    assert torch.equal(at, torch.rand((2, 7, 11, 3), device=dev) >= .25)
    want = ops.cattn_pack_keep(torch.rand((2, 3, 37, 46), device=dev) >= .25)
    assert all(torch.equal(a, b) for a, b in zip(ca, want))
    torch.manual_seed(11)
    m = A.FeedForward(dim=64, dropout=.25).to(DEV).train()
    m(torch.randn(2, 48, 64, device=DEV)).sum().backward()
    assert spy.calls == []
