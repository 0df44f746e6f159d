"""Whole models on trained-like weights, and the second call after the weights have changed.

C. Parity: the product on trained_like() weights (every norm gain and bias with values of its own: test_weight_updates_cpu.py shows that
   each of them moves the logits by five times the bound) against the fp32 oracle on the same weights -- loss, logits, every gradient --
   then one FusedAdamW step (lr 1e-2: every weight moves by about 1e-2), the product's weights read back into the oracle, and again.
   Comparing at the product's own current weights keeps AdamW's amplification of gradient noise out of the check; a kernel that read a
   stale copy of a weight still fails it.  Bounds: MODES of test_gpu_modules.py, as test_g5_g6_nuwa_loss_logits_grads uses them.
D. Warm caches equal cold caches, bit for bit: a model that has run before, its weights changed in one of the ways weights change, against
   a new instance with the same state dict.
E. Gradient buffers belong to the caller: no .grad is a view of a reused workspace, two backward passes accumulate exactly, a frozen
   text encoder changes nothing on the decoder side."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import trained_like_util as T  # noqa: E402
from gpu_util import record, rel_err, rel_l2  # noqa: E402
from test_gpu_modules import MODES  # noqa: E402

DEV = 'cuda'
LR, WD, CLIP = 1e-2, 0.1, 0.5


@pytest.fixture(scope='module')
def A():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import nuwa_pytorch_amd
    return nuwa_pytorch_amd


class Checks:
    """gpu_util.report without stopping at the first miss: every figure is logged (the parity log of gpu_util.record) and printed, all misses
    are asserted together at the end (tol None: logged only)"""

    def __init__(self, tag):
        self.tag, self.bad, self.worst = tag, [], {}

    def __call__(self, group, name, got, ref, tol):
        assert got.shape == ref.shape, f'{self.tag}.{name}: shape {tuple(got.shape)} vs {tuple(ref.shape)}'
        e, l2, finite = rel_err(got, ref), rel_l2(got, ref), bool(torch.isfinite(got).all())
        record(f'{self.tag}.{name}', e, l2, tol, finite)
        if e > self.worst.get(group, (-1.0, ''))[0]:
            self.worst[group] = (e, name)
        if tol is not None and (not finite or not e <= tol):
            self.bad.append(f'{name}: rel err {e:.3e} (l2 {l2:.3e}) > tol {tol:.1e}' + ('' if finite else ', non-finite'))

    def done(self):
        print(f'{self.tag}: ' + '; '.join(f'{g} {e:.2e} ({n})' for g, (e, n) in sorted(self.worst.items())))
        assert not self.bad, f'{self.tag}:\n  ' + '\n  '.join(self.bad)


def _model(A, name, state=None):
    """the product model of a fixture on the device, in training mode, with the trained-like weights (or `state`)"""
    Ar, _, Pt = T.fixture(name)
    m = T.build_product(A, name, Ar)
    if state is None:
        T.put_state(m, Pt)
    else:
        m.load_state_dict(state)
    return T.pin_sketch_ids(m.to(DEV).train(), name, Ar, DEV)


def _trainable(m):
    return [p for p in m.parameters() if p.requires_grad]


def _step(m, name, ids=None, zero=True):
    """one forward / backward: (loss, {name: clone of .grad})"""
    Ar = T.fixture(name)[0]
    if zero:
        m.zero_grad(set_to_none=True)
    loss = T.product_loss(m, name, Ar, DEV, video_ids=ids)
    loss.backward()
    return loss.detach().clone(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}


def _decoder_side(grads):
    """as test_training_step_is_bitwise_reproducible: the text encoder's own backward runs on torch ops, which fix no order"""
    return {n: g for n, g in grads.items() if not n.startswith('text_')}


def _assert_same(tag, a, b):
    (la, ga), (lb, gb) = a, b
    assert bool(torch.isfinite(la)), f'{tag}: loss {la}'
    assert torch.equal(la, lb), f'{tag}: loss {float(la)!r} (warm) vs {float(lb)!r} (cold)'
    ga, gb = _decoder_side(ga), _decoder_side(gb)
    assert set(ga) == set(gb) and len(ga) > 40
    diff = [n for n in ga if not torch.equal(ga[n], gb[n])]
    assert not diff, f'{tag}: {len(diff)} of {len(ga)} gradients differ between the warm model and its cold twin, e.g. {diff[:4]}'


# =================================================================================================
# C. parity on trained-like weights, and again after the optimiser has moved them
# =================================================================================================

@functools.lru_cache(maxsize=None)
def _oracle_at_start(name):
    """the oracle on the trained-like weights: computed once per model, shared by the three modes, left unchanged"""
    Ar, _, Pt = T.fixture(name)
    return T.oracle_step(name, Ar, Pt)


@pytest.mark.parametrize('mode,tol,gtol', MODES)
@pytest.mark.parametrize('name', list(T.MODELS))
def test_trained_like_parity_across_two_optimizer_steps(A, name, mode, tol, gtol):
    """Measured on the MI355X, largest error over the three comparisons (start, after step 1, after step 2) -- logits / loss / gradients:
    see DESIGN.md section 2.2 (table per model and mode)."""
    from nuwa_pytorch_amd.optimizer import FusedAdamW
    Ar = T.fixture(name)[0]
    m = _model(A, name)
    opt = FusedAdamW(_trainable(m), lr=LR, weight_decay=WD)
    tags = ('video_logits', 'audio_logits') if T.MODELS[name]['kind'] == 'va' else ('logits',)
    ck = Checks(f'trained_like.{name}[{mode}]')
    A.set_precision(mode)
    try:
        prev_logits = None
        for step in range(3):
            if step == 0:
                loss_ref, logits_ref, G = _oracle_at_start(name)
            else:
                loss_ref, logits_ref, G = T.oracle_step(name, Ar, T.read_state(m))
                # a condition on the step, from the oracle alone: the update is far above the bound, so logits computed from any
                # weight copy of before the step cannot pass
                moved = max(rel_err(a, b) for a, b in zip(logits_ref, prev_logits))
                print(f'{ck.tag}: step {step} moved the oracle logits by {moved:.2e}')
                assert moved > 5e-3, f'step {step} moved the oracle logits by {moved:.2e} only'
            prev_logits = logits_ref
            m.zero_grad(set_to_none=True)
            for t, got, ref in zip(tags, T.product_logits(m, name, Ar, DEV), logits_ref):
                ck('logits', f's{step}.{t}', got, ref, tol)
            loss = T.product_loss(m, name, Ar, DEV)
            ck('loss', f's{step}.loss', loss.reshape(1), loss_ref.reshape(1), tol)
            loss.backward()
            named, buffers = dict(m.named_parameters()), dict(m.named_buffers())
            n = 0
            for k, g in G.items():
                if k in buffers:                     # (the rotary frequencies: a float tensor to the oracle, a buffer to the model)
                    continue
                p = named[k]
                assert p.grad is not None, f'{ck.tag}: no grad for {k}'
                ck('grads', f's{step}.grad.{k}', p.grad, g, gtol * 2)        # (the text encoder's included, as test_g5_g6_nuwa_loss_logits_grads)
                n += 1
            assert n > 40
            if step < 2:
                before = {k: v.detach().clone() for k, v in named.items() if v.grad is not None}
                opt.step(max_grad_norm=CLIP)
                # AdamW's first update is lr * sign(g); the second is smaller where the two gradients disagree in sign
                dmin = min(float((named[k].detach() - v).abs().max()) for k, v in before.items())
                assert dmin > (0.5 * LR if step == 0 else 1e-3), f'step {step}: a parameter moved by {dmin:.2e} only'
    finally:
        A.set_precision('bf16')
    ck.done()


# =================================================================================================
# D. warm caches equal cold caches, bit for bit
# =================================================================================================

def _mut_none(A, m):
    pass


def _mut_fused_adamw(A, m):
    from nuwa_pytorch_amd.optimizer import FusedAdamW
    FusedAdamW(_trainable(m), lr=LR, weight_decay=WD).step()


def _mut_torch_adamw(A, m):
    opt = torch.optim.AdamW(_trainable(m), lr=LR, weight_decay=WD)
    assert opt.defaults.get('foreach') is None and not opt.defaults.get('fused')       # the default form: foreach on a device
    opt.step()


def _mut_load_state_dict(A, m):
    m.load_state_dict({k: v * 0.9 if v.is_floating_point() else v for k, v in m.state_dict().items()})


def _mut_mul_no_grad(A, m):
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(1.1)


def _mut_storage_swap(A, m):
    for p in m.parameters():
        p.data = p.data * 0.9


def _mut_storage_swap_old_address(A, m):
    """the fp32 storage is dropped first (an fp16 detour, as module.half().float() makes), so that the allocator may hand its block to
    the new fp32 storage"""
    reused = total = 0
    for p in m.parameters():
        old = p.data_ptr()
        half = p.data.to(torch.float16).mul_(0.9)
        p.data = half
        p.data = half.float()
        total += 1
        reused += int(p.data_ptr() == old)
    return reused, total


def _mut_cpu_round_trip(A, m):
    m.to('cpu')
    m.to(DEV)


def _mut_data_write_then_weights_changed(A, m):
    for p in m.parameters():
        p.data.mul_(0.9)
    A.weights_changed()


MUTATIONS = {'none': _mut_none, 'FusedAdamW.step': _mut_fused_adamw, 'torch.AdamW.step': _mut_torch_adamw,
             'load_state_dict': _mut_load_state_dict, 'no_grad p.mul_': _mut_mul_no_grad, 'p.data = new': _mut_storage_swap,
             'p.data = new at the old address': _mut_storage_swap_old_address, 'cpu and back': _mut_cpu_round_trip,
             'p.data.mul_ + weights_changed': _mut_data_write_then_weights_changed}
WARM_COLD = [('g5', m) for m, _, _ in MODES] + [('g9a', m) for m, _, _ in MODES] + [('g6', 'bf16')]


@pytest.mark.parametrize('mutation', list(MUTATIONS))
@pytest.mark.parametrize('short,mode', WARM_COLD)
def test_warm_model_equals_cold_twin_after_its_weights_changed(A, short, mode, mutation):
    name = T.SHORT[short]
    tag = f'warm_cold.{short}[{mode}] after {mutation}'
    A.set_precision(mode)
    try:
        warm = _model(A, name)
        first = _step(warm, name)                    # caches, verdicts, workspaces and gradients of the weights as they were
        info = MUTATIONS[mutation](A, warm)
        if mutation == 'p.data = new at the old address':
            reused, total = info
            print(f'{tag}: {reused} of {total} parameters got their old address back' +
                  ('' if reused else ' -- NONE did: this run says nothing about address reuse'))
        cold = _model(A, name, state=warm.state_dict())
        got = _step(warm, name)
        want = _step(cold, name)
        if mutation not in ('none', 'cpu and back'):       # (these two keep the values)
            assert not torch.equal(got[0], first[0]), f'{tag}: the mutation did not move the loss'
        _assert_same(tag, got, want)
    finally:
        A.set_precision('bf16')


def test_generate_after_an_optimizer_step_warm_equals_cold(A):
    """cached decoding reads the same WeightCache entries: after one FusedAdamW step, generate() of one frame (greedy: the top 1 % of
    64 logits is one candidate) gives the ids a new instance with the same weights gives"""
    from nuwa_pytorch_amd.optimizer import FusedAdamW
    name = T.SHORT['g5']
    text = T.fixture(name)[0]['text'].to(DEV)
    warm = _model(A, name)

    def gen(m):
        m.eval()
        with torch.no_grad():
            m.generate(text=text, filter_thres=0.99, num_frames=1, cond_scale=2.)
        m.train()
        return m.last_generated_ids.clone()

    before = gen(warm)
    _step(warm, name)
    opt = FusedAdamW(_trainable(warm), lr=LR, weight_decay=WD)
    for _ in range(3):                               # (three steps of 1e-2: enough for the greedy ids to change)
        _step(warm, name)
        opt.step()
    cold = _model(A, name, state=warm.state_dict())
    got, want = gen(warm), gen(cold)
    assert got.shape == (2, 16) and torch.equal(got, want), (got, want)
    print('generate: ids changed by the steps at', int((got != before).sum()), 'of', got.numel(), 'positions')


def test_fp16_range_guard_follows_a_weight_out_of_range_and_back(A, monkeypatch):
    """'bf16x3-fwd': a FeedForward w1 scaled by 1e6 (beyond ops.F16_WMAX) on a warm model -- the verdict of before must not stand: the
    block's plan drops a16, the loss is finite and the cold twin's; scaled back, the plan takes a16 again"""
    from nuwa_pytorch_amd import ops
    name = T.SHORT['g5']
    plans = []
    fwd = ops.FFInner.fwd
    monkeypatch.setattr(ops.FFInner, 'fwd', staticmethod(lambda h, p, meta: (plans.append((p[0], meta['plan'].a16)), fwd(h, p, meta))[1]))

    decoder_w1 = set()

    def a16_of(m, w):
        plans.clear()
        out = _step(m, name)
        seen = {id(p): a for p, a in plans if id(p) in decoder_w1}
        assert len(seen) == 3                        # the three FeedForward blocks of the decoder
        return out, seen[id(w)], [a for i, a in seen.items() if i != id(w)]

    A.set_precision('bf16x3-fwd')
    try:
        warm = _model(A, name)
        named = dict(warm.named_parameters())
        decoder_w1.update(id(named[f'video_transformer.layers.{i}.2.fn.fn.net.0.weight']) for i in range(3))
        w1 = named['video_transformer.layers.1.2.fn.fn.net.0.weight']
        _, mine, others = a16_of(warm, w1)
        assert mine is True and others == [True, True]
        with torch.no_grad():
            w1.mul_(1e6)
        assert float(w1.detach().abs().max()) > ops.F16_WMAX
        got, mine, others = a16_of(warm, w1)
        assert mine is False and others == [True, True]
        cold = _model(A, name, state=warm.state_dict())
        want = _step(cold, name)
        _assert_same('f16 guard, w1 * 1e6', got, want)
        with torch.no_grad():
            w1.mul_(1e-6)
        back, mine, others = a16_of(warm, w1)
        assert mine is True and others == [True, True]
        cold = _model(A, name, state=warm.state_dict())
        _assert_same('f16 guard, w1 back in range', back, _step(cold, name))
    finally:
        A.set_precision('bf16')


def test_context_written_through_data_is_recast_after_weights_changed(A):
    """the bf16 copy of the context (ops._ctx_to_bf) is kept per tensor object, storage and version: a write through `.data` is invisible
    to it, weights_changed() drops it -- the next call equals a call on a new tensor with the same values"""
    from golden_util import load
    Ar, P, _ = load('g2_cross_attention')
    m = A.Attention(dim=32, heads=int(Ar['heads']), dim_head=32)
    m.load_state_dict(P)
    m = m.to(DEV)
    x, ctx, mask = Ar['x'].to(DEV), Ar['ctx'].to(DEV), Ar['mask'].to(DEV)
    with torch.no_grad():
        y0 = m(x, context=ctx, context_mask=mask).clone()
        ctx.data.mul_(0.5)
        A.weights_changed()
        y1 = m(x, context=ctx, context_mask=mask).clone()
        want = m(x, context=ctx.clone(), context_mask=mask)
        assert torch.equal(y1, want) and not torch.equal(y1, y0)
        ctx.data = ctx.data * 0.5                    # a new storage needs no call
        y2 = m(x, context=ctx, context_mask=mask).clone()
        assert torch.equal(y2, m(x, context=ctx.clone(), context_mask=mask)) and not torch.equal(y2, y1)


# =================================================================================================
# E. gradient buffers belong to the caller
# =================================================================================================

def _other_ids(name):
    ids = T.fixture(name)[0]['video_ids']
    other = torch.randint(0, 64, ids.shape, generator=torch.Generator().manual_seed(17)).to(ids.dtype)
    assert not torch.equal(other, ids)
    return other


@pytest.mark.parametrize('mode', ['bf16', 'bf16x3-fwd'])
def test_gradients_are_not_views_of_reused_workspaces(A, mode):
    name = T.SHORT['g5']
    A.set_precision(mode)
    try:
        m = _model(A, name)
        _step(m, name)
        kept = {n: p.grad for n, p in m.named_parameters() if p.grad is not None}
        clones = {n: g.clone() for n, g in kept.items()}
        for p in m.parameters():
            p.grad = None
        loss2, g2 = _step(m, name, ids=_other_ids(name), zero=False)
        torch.cuda.synchronize()
        assert len(kept) > 40 and any(not torch.equal(g2[n], clones[n]) for n in clones)
        changed = [n for n in kept if not torch.equal(kept[n], clones[n])]
        assert not changed, f'gradient tensors of the first step were overwritten by the second: {changed[:6]}'
    finally:
        A.set_precision('bf16')


@pytest.mark.parametrize('mode', ['bf16', 'bf16x3-fwd'])
def test_two_backward_passes_accumulate_exactly(A, mode):
    name = T.SHORT['g5']
    A.set_precision(mode)
    try:
        m = _model(A, name)
        _, g1 = _step(m, name)
        _, g2 = _step(m, name, ids=_other_ids(name))
        _step(m, name)
        _, both = _step(m, name, ids=_other_ids(name), zero=False)
        g1, g2, both = _decoder_side(g1), _decoder_side(g2), _decoder_side(both)
        assert set(g1) == set(g2) == set(both) and len(both) > 40
        off = [n for n in both if not torch.equal(both[n], g1[n] + g2[n])]
        assert not off, f'accumulated gradients differ from the sum of the two: {off[:6]}'
    finally:
        A.set_precision('bf16')


@pytest.mark.parametrize('mode', ['bf16', 'bf16x3-fwd'])
def test_frozen_text_encoder_leaves_the_decoder_side_alone(A, mode):
    name = T.SHORT['g5']
    A.set_precision(mode)
    try:
        m = _model(A, name)
        loss, grads = _step(m, name)
        frozen = [p for n, p in m.named_parameters() if n.startswith('text_')]
        assert len(frozen) > 20 and any(n.startswith('text_') for n in grads)
        for p in frozen:
            p.requires_grad_(False)
        loss_f, grads_f = _step(m, name)
        assert torch.equal(loss, loss_f)
        assert all(p.grad is None for p in frozen) and not any(n.startswith('text_') for n in grads_f)
        a, b = _decoder_side(grads), _decoder_side(grads_f)
        assert set(a) == set(b) and len(a) > 40
        diff = [n for n in a if not torch.equal(a[n], b[n])]
        assert not diff, f'decoder-side gradients changed when the text encoder was frozen: {diff[:6]}'
    finally:
        A.set_precision('bf16')
