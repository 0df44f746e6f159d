"""The sampling tail of a generate() token on the MI355X (amdnuwa_sample_next_row, csrc/sample.hip; decode.GuidedStepper's sampler;
NUWA / NUWASketch.generate_device_sampler).  Pinned here:
  * the kernel samples the class the torch expression of nuwa_pytorch.sample_top_fraction samples from the same logits and the same
    uniforms, and its next input row is bit-equal to emb[id] + pos[idx]; operands and outputs in guarded buffers;
  * an out-of-range step or position index writes nothing, two launches are bit-identical, one captured launch follows the device-side
    step counter;
  * with the switch on, generate() -- eager and as a captured HIP graph -- samples the token ids of the reference's own generate()
    (fixtures g13a / g13b / g13e / g18a / g18b / g19a / g19b) without one call of sample_top_fraction or of the recompute loop, and
    with the prefills it had;
  * seeded Gumbel sampling (6 kept of 64) gives the ids of the torch tail."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from golden_util import load  # noqa: E402
from guard_util import FILL, guard, guarded, guarded_empty  # noqa: E402
from sketch_window_util import WINDOW_KW  # noqa: E402
from test_gpu_long_generate import _Spies  # noqa: E402
from test_gpu_long_generate import _fixture_model as _long_fixture_model  # noqa: E402
from test_gpu_long_generate import _generate as _generate_nuwa  # noqa: E402
from test_gpu_modules import SKETCH_KW, _tiny_nuwa  # noqa: E402
from test_gpu_sketch_window import _Spy  # noqa: E402
from test_gpu_sketch_window import _fixture_model as _sketch_fixture_model  # noqa: E402
from test_gpu_sketch_window import _generate as _generate_sketch  # noqa: E402

DEV = 'cuda'
P_ROWS, CAP, STEP = 48, 40, 7               # position rows, id columns, the step the single launches run at


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


# ---- the kernel ----------------------------------------------------------------------------------------------------------------

def torch_tail(logits, keep, temperature, u):
    """the expression tree of nuwa_pytorch.sample_top_fraction with the uniforms given: (ids [B], scores [B, keep] or None)"""
    vals, ids = logits.topk(keep, dim=-1)
    if keep == 1:
        return ids[..., 0], None
    gumbel = -torch.log((-torch.log(u.clamp(min=1e-20))).clamp(min=1e-20))
    scores = vals / temperature + gumbel
    return ids.gather(-1, scores.argmax(dim=-1, keepdim=True))[..., 0], scores


def assert_no_near_tie(logits, keep, scores):
    """the condition on the INPUTS under which two correct samplers must agree, judged on the torch side alone: no two of the top
    keep + 1 logits are equal (the kept set and its order are unique) and the two largest scores differ by at least 1e-4 (the
    arg-max survives the last bits of two logf implementations)"""
    top = logits.topk(min(keep + 1, logits.shape[-1]), dim=-1).values
    assert bool((top[:, 1:] != top[:, :-1]).all()), 'two of the top keep + 1 logits are equal'
    if scores is not None:
        s2 = scores.topk(2, dim=-1).values
        gap = float((s2[:, 0] - s2[:, 1]).min())
        assert gap >= 1e-4, f'the two largest scores differ by {gap:.3e}'


# Logits: a random permutation of C equally spaced values in [-6, 6) per row (pairwise distinct by construction); uniforms from the same
# seeded generator.  Seed 0, except where its two largest scores come closer than 1e-2 on the torch expression (margin to the 1e-4 above).
SEEDS = {(3, 1000, 100, 1.): 1}


def _inputs(B, C, keep, D, seed):
    g = torch.Generator().manual_seed(seed)
    logits = torch.stack([torch.randperm(C, generator=g).float() / C * 12 - 6 for _ in range(B)])
    u = torch.rand(B, keep, generator=g) if keep > 1 else None
    emb, pos = torch.randn(C, D, generator=g), torch.randn(P_ROWS, D, generator=g)
    pos_idx = torch.randint(0, P_ROWS, (CAP,), generator=g).to(torch.int32)
    return logits, u, emb, pos, pos_idx


def _operands(B, C, keep, D, seed, step=STEP):
    logits, u, emb, pos, pos_idx = _inputs(B, C, keep, D, seed)
    op = dict(logits=guarded(logits, device=DEV), u=guarded(u, device=DEV) if u is not None else None, emb=guarded(emb, device=DEV),
              pos=guarded(pos, device=DEV), pos_idx=guarded(pos_idx, device=DEV),
              step=guarded(torch.tensor([step], dtype=torch.int32), device=DEV),
              ids=guarded_empty((B, CAP), torch.int64, DEV), x_next=guarded_empty((B, D), torch.float32, DEV))
    return op


def _launch(K, op, keep, temperature):
    assert K.sample_next_row(op['logits'], keep, temperature, op['u'], op['emb'], op['pos'], op['pos_idx'], op['step'], op['ids'], op['x_next'])


def _untouched(t):
    return bool((t.contiguous().view(torch.uint8) == FILL).all())


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize('temperature', [1., 0.5])
@pytest.mark.parametrize('D', [32, 512])
@pytest.mark.parametrize('C,keep', [(64, 1), (64, 6), (1000, 100), (8192, 819), (16384, 1638), (16384, 16384)])
@pytest.mark.parametrize('B', [1, 3])
def test_kernel_samples_what_the_torch_expression_samples(K, B, C, keep, D, temperature):
    """same logits, same uniforms: the ids of every row are equal and x_next is bit-equal to emb[id] + pos[pos_idx[step]]; column `step` of
    ids alone is written; nothing outside the tensors (guard bands)"""
    op = _operands(B, C, keep, D, SEEDS.get((B, C, keep, temperature), 0))
    want, scores = torch_tail(op['logits'], keep, temperature, op['u'])
    assert_no_near_tie(op['logits'], keep, scores)
    with guard(K):
        _launch(K, op, keep, temperature)
    got = op['ids'][:, STEP]
    print(f'sample_next_row[B={B},C={C},keep={keep},D={D},T={temperature}]: ids {got.tolist()} (torch {want.tolist()})')
    assert torch.equal(got, want), (got, want)
    rest = torch.cat((op['ids'][:, :STEP], op['ids'][:, STEP + 1:]), dim=1)
    assert bool((rest == -1).all()), 'an id column other than the step was written'
    x_ref = op['emb'][want] + op['pos'][op['pos_idx'][STEP].long()]
    assert _same_bits(op['x_next'], x_ref)


def test_equal_logits_order_by_class_index(K):
    """equal values rank by lower class index first -- at the top of the row and across the cut between kept and dropped entries.  The
    reference is the torch expression over a STABLE descending sort (torch.topk leaves the order of equal values open)"""
    B, C, keep, D = 3, 64, 6, 32
    op = _operands(B, C, keep, D, 3)
    logits = op['logits']
    for b in range(B):
        order = logits[b].argsort(descending=True)
        logits[b, order[:3]] = logits[b, order[0]].clone()            # three equal maxima
        logits[b, order[5:9]] = logits[b, order[5]].clone()           # ranks 5 .. 8 equal: one of the four is kept
    vals, idx = logits.sort(dim=-1, descending=True, stable=True)
    vals, idx = vals[:, :keep], idx[:, :keep]
    scores = vals / 1. + -torch.log((-torch.log(op['u'].clamp(min=1e-20))).clamp(min=1e-20))
    s2 = scores.topk(2, dim=-1).values
    assert float((s2[:, 0] - s2[:, 1]).min()) >= 1e-4
    want = idx.gather(-1, scores.argmax(dim=-1, keepdim=True))[..., 0]
    with guard(K):
        _launch(K, op, keep, 1.)
    assert torch.equal(op['ids'][:, STEP], want), (op['ids'][:, STEP], want)
    # greedy: the lowest class among equal maxima
    op1 = _operands(B, C, 1, D, 3)
    op1['logits'].copy_(logits)
    with guard(K):
        _launch(K, op1, 1, 1.)
    assert torch.equal(op1['ids'][:, STEP], idx[:, 0]), (op1['ids'][:, STEP], idx[:, 0])


@pytest.mark.parametrize('what', ['step<0', 'step=cap', 'pos_idx<0', 'pos_idx=P'])
def test_invalid_step_or_position_writes_nothing(K, what):
    B, C, keep, D = 3, 1000, 100, 32
    op = _operands(B, C, keep, D, 0, step={'step<0': -1, 'step=cap': CAP}.get(what, STEP))
    if what.startswith('pos_idx'):
        op['pos_idx'][STEP] = -1 if what == 'pos_idx<0' else P_ROWS
    with guard(K):
        _launch(K, op, keep, 1.)
    assert _untouched(op['ids']) and _untouched(op['x_next'])


def test_two_launches_are_bit_identical(K):
    B, C, keep, D = 3, 8192, 819, 512
    outs = []
    for _ in range(2):
        op = _operands(B, C, keep, D, 0)
        with guard(K):
            _launch(K, op, keep, 1.)
        outs.append((op['ids'].clone(), op['x_next'].clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and _same_bits(outs[0][1], outs[1][1])
    assert int(outs[0][0][:, STEP].min()) >= 0


def test_captured_launch_follows_the_device_side_counter(K):
    """one launch (and the counter's increment) captured at step 0 and replayed three times with fresh uniforms: columns 0, 1 and 2 of ids
    hold what the torch expression samples from each draw, x_next the row of the last one"""
    B, C, keep, D = 3, 1000, 100, 32
    op = _operands(B, C, keep, D, 0, step=0)
    draws = [torch.rand(B, keep, generator=torch.Generator().manual_seed(40 + i)).to(DEV) for i in range(3)]
    want = []
    for u in draws:
        ids, scores = torch_tail(op['logits'], keep, 1., u)
        assert_no_near_tie(op['logits'], keep, scores)
        want.append(ids)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                  # warm-up outside the capture, then everything it wrote back to the fill
        _launch(K, op, keep, 1.)
    torch.cuda.current_stream().wait_stream(s)
    op['ids'].fill_(-1)
    op['x_next'].fill_(float('nan'))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _launch(K, op, keep, 1.)
        op['step'] += 1
    assert bool((op['ids'] == -1).all()) and int(op['step'][0]) == 0          # capture records, it does not run
    with guard(K):
        for u in draws:
            op['u'].copy_(u)
            graph.replay()
    assert int(op['step'][0]) == 3
    for t in range(3):
        assert torch.equal(op['ids'][:, t], want[t]), (t, op['ids'][:, t], want[t])
    assert bool((op['ids'][:, 3:] == -1).all())
    assert _same_bits(op['x_next'], op['emb'][want[2]] + op['pos'][op['pos_idx'][2].long()])


# ---- generate() ------------------------------------------------------------------------------------------------------------------

class _TailSpies:
    """call counters on the torch tail (nuwa_pytorch.sample_top_fraction) and on the kernel wrapper"""

    def __init__(self, monkeypatch, K):
        from nuwa_pytorch_amd import nuwa_pytorch as NP
        self.spy = _Spy(monkeypatch, NP, 'sample_top_fraction')
        self.kspy = _Spy(monkeypatch, K, 'sample_next_row')

    @property
    def torch_tail(self):
        return self.spy.n['sample_top_fraction']

    @property
    def kernel(self):
        return self.kspy.n['sample_next_row']


def _g13_model(A, name):
    Ar, P, _ = load(name)
    m = _tiny_nuwa(A, bool(Ar['reversible']))
    missing, unexpected = m.load_state_dict(P, strict=False)
    assert not unexpected, unexpected
    return Ar, m.to(DEV).eval()


@pytest.mark.parametrize('mode', ['cached+graph', 'cached'])
@pytest.mark.parametrize('name', ['g13a_generate_nuwa', 'g13b_generate_nuwa_reversible', 'g18a_generate_long_nuwa',
                                  'g18b_generate_long_nuwa_reversible'])
def test_nuwa_generate_reproduces_the_reference_ids_with_the_device_sampler(A, K, monkeypatch, name, mode):
    """fixtures g13a / g13b (2 frames inside the window) and g18a / g18b (5 frames on a 3-frame model: the window slides twice): greedy,
    guided.  With the switch on the token ids of the reference's own generate() come out of the id buffer, eager and as a captured graph;
    sample_top_fraction and the recompute loop are never called, and g18 keeps its two prefills of 33 rows (read from the id buffer)"""
    long = name.startswith('g18')
    Ar, m = _long_fixture_model(A, name) if long else _g13_model(A, name)
    monkeypatch.setattr(type(m), 'generate_device_sampler', True)
    spies, tail = _Spies(monkeypatch, A), _TailSpies(monkeypatch, K)
    frames = int(Ar['num_frames']) if long else 2
    ids = _generate_nuwa(A, m, Ar['text'].to(DEV), float(Ar['cond_scale']), frames, mode)
    assert torch.equal(ids, Ar['video_ids'].long()), (ids, Ar['video_ids'])
    assert tail.torch_tail == 0 and tail.kernel >= 1, (tail.torch_tail, tail.kernel)
    assert spies.recompute == 0
    assert (spies.prefill, spies.prefill_rows) == ((2, [33, 33]) if long else (0, []))
    if mode == 'cached':
        assert tail.kernel == 1 + 16 * frames                   # the envelope probe + one launch per token


@pytest.mark.parametrize('mode', ['cached+graph', 'cached'])
@pytest.mark.parametrize('name', ['g13e_generate_sketch', 'g19a_generate_sketch_window', 'g19b_generate_sketch_window_reversible'])
def test_sketch_generate_reproduces_the_reference_ids_with_the_device_sampler(A, K, monkeypatch, name, mode):
    """fixtures g13e (18-slot window) and g19a / g19b (300 slots, plain and reversible): NUWASketch.generate with the switch on; the <bos>
    row stays an eager first call, the graph serves rows >= 1"""
    Ar, m = _sketch_fixture_model(A, name, SKETCH_KW if name.startswith('g13') else WINDOW_KW)
    monkeypatch.setattr(type(m), 'generate_device_sampler', True)
    spy, tail = _Spy(monkeypatch, A.NUWASketch, '_guided_last_logits'), _TailSpies(monkeypatch, K)
    ids = _generate_sketch(A, m, Ar, mode)
    assert torch.equal(ids, Ar['video_ids'].long()), (ids, Ar['video_ids'])
    assert tail.torch_tail == 0 and tail.kernel >= 1, (tail.torch_tail, tail.kernel)
    assert spy.n['_guided_last_logits'] == 0
    if mode == 'cached':
        assert tail.kernel == 1 + 32


def test_switch_off_keeps_the_torch_tail(A, K, monkeypatch):
    Ar, m = _g13_model(A, 'g13a_generate_nuwa')
    monkeypatch.setattr(type(m), 'generate_device_sampler', False)
    tail = _TailSpies(monkeypatch, K)
    ids = _generate_nuwa(A, m, Ar['text'].to(DEV), float(Ar['cond_scale']), 2, 'cached+graph')
    assert torch.equal(ids, Ar['video_ids'].long())
    assert (tail.torch_tail, tail.kernel) == (32, 0)


def _seeded(A, m, text, seed, on):
    cls = type(m)
    A.set_precision('bf16x3')
    try:
        cls.generate_device_sampler = on
        torch.manual_seed(seed)
        m.generate(text=text, filter_thres=0.9, temperature=1., cond_scale=2., num_frames=2)
    finally:
        A.set_precision('bf16')
    return m.last_generated_ids.cpu()


def test_seeded_sampling_equals_the_torch_tail(A, K, monkeypatch):
    """tiny NUWA, filter_thres 0.9, temperature 1: 6 of 64 logits kept, 32 tokens, guided, as a captured graph.  The seed is the first of
    eight for which the TORCH tail's two best scores differ by at least 1e-4 at every step -- judged with the switch off, before the
    switch-on run, by re-evaluating sample_top_fraction's expression on the uniforms it drew (generator state rewound and replayed, so
    the call consumes what it would have).  The switch-on run must then sample the same ids from the same seed: the uniforms are drawn
    as torch.rand_like(vals) draws them"""
    from nuwa_pytorch_amd import nuwa_pytorch as NP
    Ar, m = _g13_model(A, 'g13a_generate_nuwa')
    monkeypatch.setattr(type(m), 'generate_device_sampler', False)          # (restored on exit)
    text = Ar['text'].to(DEV)
    gaps, orig = [], NP.sample_top_fraction

    def watched(logits, filter_thres=0.9, temperature=1.):
        state = torch.cuda.get_rng_state()
        token = orig(logits, filter_thres, temperature)
        after = torch.cuda.get_rng_state()
        torch.cuda.set_rng_state(state)
        keep = max(int((1 - filter_thres) * logits.shape[-1]), 1)
        mine, scores = torch_tail(logits, keep, temperature, torch.rand_like(logits.topk(keep, dim=-1).values))
        torch.cuda.set_rng_state(after)
        assert keep == 6 and torch.equal(mine, token)                       # the re-evaluation IS the call
        s2 = scores.topk(2, dim=-1).values
        gaps.append(float((s2[:, 0] - s2[:, 1]).min()))
        return token

    monkeypatch.setattr(NP, 'sample_top_fraction', watched)
    seed = want = None
    for cand in range(8):
        del gaps[:]
        ids = _seeded(A, m, text, cand, on=False)
        print(f'seeded sampling: seed {cand}: minimum gap of the two best scores {min(gaps):.3e} over {len(gaps)} steps')
        assert len(gaps) == 32
        if min(gaps) >= 1e-4:
            seed, want = cand, ids
            break
    assert seed is not None, 'no seed keeps the torch tail clear of near ties'
    assert len(set(want.flatten().tolist())) > 4                            # a sampled sequence, not a constant
    del gaps[:]
    kspy = _Spy(monkeypatch, K, 'sample_next_row')
    got = _seeded(A, m, text, seed, on=True)
    assert not gaps and kspy.n['sample_next_row'] >= 1                      # the torch tail did not run
    assert torch.equal(got, want), (got, want)
