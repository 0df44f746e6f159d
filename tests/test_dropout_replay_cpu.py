"""FeedForward dropout without a GPU (np.py:276; rev.py:20-50): the two mask entry points of csrc/dropout.hip are exported, declared and
registered at an unchanged ABI version, their argument checks answer before anything is launched, the RNG record / replay helper of
the reversible stacks replays the CPU generator and leaves the main stream undisturbed, and a FeedForward with live dropout is routed
into the fused block (SandwichNorm._inner, FeedForward._meta) -- in the reversible stacks too (no `_no_hip_dropout` mark any more)."""
import ctypes
import math
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ARG = 0, -1
PTR = ctypes.c_void_p(16)           # non-NULL, 16-byte aligned, never dereferenced on the host


@pytest.fixture(scope='module')
def L():
    from nuwa_pytorch_amd import _lib
    return _lib.lib()


def _fwd(L, **over):
    """amdnuwa_geglu_dropout_fwd in its bf16 form (b) with every pointer PTR; over: name -> value"""
    a = dict(inp=PTR, in_lo=None, ld_in=64, in_f16=0, keep=PTR, ld_keep=64, scale=1.25, out=PTR, out_lo=None, ld_out=64, out_f16=None,
             ld_f16=0, R=0, C=64, stream=None)
    a.update(over)
    return L.amdnuwa_geglu_dropout_fwd(*a.values())


def _bwd(L, **over):
    a = dict(u_hi=PTR, u_lo=None, d_hi=PTR, d_lo=None, keep=PTR, ld_keep=64, scale=1.25, du_hi=PTR, du_lo=None, R=0, FP=64, stream=None)
    a.update(over)
    return L.amdnuwa_geglu_il_bwd_dropout(*a.values())


def test_entry_points_are_exported_declared_and_registered(L):
    from nuwa_pytorch_amd import _lib
    from nuwa_pytorch_amd import kernels as K
    header = open(os.path.join(ROOT, 'include', 'amdnuwa.h')).read()
    for name in ('amdnuwa_geglu_dropout_fwd', 'amdnuwa_geglu_il_bwd_dropout'):
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES
        assert re.search(r'\b' + name + r'\s*\(', header), name
    assert 'np.py:276' in header
    assert callable(K.geglu_dropout_fwd) and callable(K.geglu_dropout_fwd_f16) and callable(K.geglu_il_bwd_dropout)
    assert callable(K.set_ff_drop_torch)
    assert L.amdnuwa_abi_version() == 21                      # purely additive


def test_forward_argument_checks_answer_before_any_launch(L):
    assert _fwd(L) == OK                                       # R = 0: nothing to do
    assert _fwd(L, R=-3) == OK
    assert _fwd(L, in_lo=PTR, out_lo=PTR) == OK
    assert _fwd(L, in_f16=1, out_f16=PTR, ld_f16=64) == OK
    for name in ('inp', 'keep', 'out'):
        assert _fwd(L, **{name: None}) == ARG, name
        assert _fwd(L, R=5, **{name: None}) == ARG, name
    assert _fwd(L, in_f16=1) == ARG                            # the fp16 form needs the fp16 output ...
    assert _fwd(L, in_f16=1, out_f16=PTR, ld_f16=64, in_lo=PTR) == ARG         # ... and takes no lo parts
    assert _fwd(L, in_f16=1, out_f16=PTR, ld_f16=64, out_lo=PTR) == ARG
    assert _fwd(L, out_f16=PTR, ld_f16=64) == ARG              # the bf16 form writes no fp16 copy
    for bad in (float('nan'), float('inf'), -float('inf'), 0.5, 0.0, -2.0):
        assert _fwd(L, scale=bad) == ARG, bad
    assert _fwd(L, scale=1.0) == OK
    for C in (0, -8, 4, 60, 63):
        assert _fwd(L, C=C, R=5) == ARG, C
    # row pitches: what the 16-byte accesses (8 mask bytes) need
    for name in ('ld_in', 'ld_out', 'ld_keep'):
        assert _fwd(L, **{name: 56}) == ARG, name              # shorter than the row
        assert _fwd(L, **{name: 68}) == ARG, name              # not a multiple of 8
        assert _fwd(L, **{name: 72}) == OK, name
    assert _fwd(L, in_f16=1, out_f16=PTR, ld_f16=68) == ARG
    assert _fwd(L, inp=ctypes.c_void_p(24)) == ARG             # base not 16-byte aligned
    assert _fwd(L, keep=ctypes.c_void_p(20)) == ARG            # mask base not 8-byte aligned
    assert _fwd(L, keep=ctypes.c_void_p(24)) == OK


def test_backward_argument_checks_answer_before_any_launch(L):
    assert _bwd(L) == OK and _bwd(L, R=-1) == OK
    assert _bwd(L, u_lo=PTR, d_lo=PTR, du_lo=PTR) == OK
    for name in ('u_hi', 'd_hi', 'keep', 'du_hi'):
        assert _bwd(L, **{name: None}) == ARG, name
        assert _bwd(L, R=5, **{name: None}) == ARG, name
    assert _bwd(L, u_lo=PTR) == ARG and _bwd(L, d_lo=PTR, du_lo=PTR) == ARG       # lo parts: all or none
    for bad in (float('nan'), float('inf'), 0.99, -1.0):
        assert _bwd(L, scale=bad) == ARG, bad
    for FP in (0, 4, 36, -8):
        assert _bwd(L, FP=FP, R=5) == ARG, FP
    assert _bwd(L, ld_keep=56) == ARG and _bwd(L, ld_keep=68) == ARG and _bwd(L, ld_keep=128) == OK
    assert _bwd(L, du_hi=ctypes.c_void_p(8)) == ARG


def test_rng_replay_on_the_cpu_generator():
    from nuwa_pytorch_amd.nuwa_pytorch import RngReplay, rng_record, rng_replay
    torch.manual_seed(11)
    undisturbed = [torch.rand(7), torch.rand(7)]
    torch.manual_seed(11)
    rec = RngReplay.record(torch.device('cpu'))
    first = torch.rand(7)
    with rec.replay():
        again = torch.rand(7)
        torch.rand(100)                                        # whatever else the recomputation draws stays inside the fork
    nxt = torch.rand(7)
    assert torch.equal(first, undisturbed[0]) and torch.equal(again, first)
    assert torch.equal(nxt, undisturbed[1])                    # the main stream comes out where it went in
    # two records in flight do not disturb each other
    torch.manual_seed(5)
    r1 = RngReplay.record()
    a = torch.rand(3)
    r2 = RngReplay.record()
    b = torch.rand(3)
    with r2.replay():
        assert torch.equal(torch.rand(3), b)
    with r1.replay():
        assert torch.equal(torch.rand(3), a)
    # nothing recorded -> nothing forked or set
    m = torch.nn.Dropout(0.0).train()
    assert rng_record(m, torch.zeros(1)) is None
    assert rng_record(torch.nn.Dropout(0.1).eval(), torch.zeros(1)) is None
    assert rng_record(torch.nn.Dropout(0.1).train(), torch.zeros(1), on=False) is None
    assert isinstance(rng_record(torch.nn.Sequential(torch.nn.Dropout(0.1)).train(), torch.zeros(1)), RngReplay)
    before = torch.get_rng_state()
    with rng_replay(None):
        pass
    assert torch.equal(before, torch.get_rng_state())


def test_dropout_feedforward_is_the_inner_stage_of_the_fused_block():
    from nuwa_pytorch_amd.nuwa_pytorch import SandwichNorm, FeedForward, ShiftVideoTokens
    block = SandwichNorm(dim=64, fn=FeedForward(dim=64, dropout=0.1)).train()
    inner = block._inner()
    assert inner is not None and inner[0] is block.fn and inner[1] is None
    meta = block.fn._meta(2, 33, torch.device('cpu'))
    assert meta['kind'] == 'ff' and math.isclose(meta['drop_p'], 0.1)
    block.eval()
    assert block._inner()[0] is block.fn
    assert 'drop_p' not in block.fn._meta(2, 33, torch.device('cpu'))
    plain = FeedForward(dim=64).train()
    assert 'drop_p' not in plain._meta(2, 33, torch.device('cpu'))
    shifted = SandwichNorm(dim=64, fn=ShiftVideoTokens(FeedForward(dim=64, dropout=0.1), image_size=4)).train()
    fn, fmap = shifted._inner()
    assert isinstance(fn, FeedForward) and fmap == 4 and fn._meta(2, 33, torch.device('cpu'))['drop_p'] > 0


def test_reversible_stacks_carry_no_torch_dropout_mark():
    from nuwa_pytorch_amd.nuwa_pytorch import ReversibleTransformer, FeedForward
    from nuwa_pytorch_amd.video_audio import ReversibleDualModalityDecoder
    rt = ReversibleTransformer(dim=64, depth=2, causal=True, heads=2, dim_head=32, cross_attend=True, sparse_3dna_attn=True,
                               sparse_3dna_video_shape=(2, 4, 4), shift_video_tokens=True, ff_dropout=0.1).train()
    dd = ReversibleDualModalityDecoder(dim=64, depth=1, num_audio_tokens_per_video_frame=4, num_video_tokens_per_frame=16,
                                       sparse_3dna_video_shape=(2, 4, 4), heads=2, dim_head=32, ff_dropout=0.1,
                                       cross_modality_attn_every=1).train()
    for model in (rt, dd):
        ffs = [m for m in model.modules() if isinstance(m, FeedForward)]
        assert ffs
        assert not any(hasattr(m, '_no_hip_dropout') for m in model.modules())
        assert all('drop_p' in m._meta(2, 33, torch.device('cpu')) for m in ffs)


def _toy(dim, p):
    return torch.nn.Sequential(torch.nn.Linear(dim, dim), torch.nn.Tanh(), torch.nn.Dropout(p))


def _grads(params, x):
    return [x.grad.clone()] + [q.grad.clone() for q in params]


@pytest.mark.parametrize('p', [0.3, 0.0])
def test_recomputing_stack_replays_the_masks_of_its_forward(p):
    """the recomputing backward of the reversible stack on toy sub-blocks with a live nn.Dropout (CPU generator): the gradients of the
    stored-graph forward under the same seed -- which draws the same masks in the same order and never recomputes -- and the main
    stream left where the stored-graph step leaves it.  Without the replay the recomputed halves draw fresh masks."""
    from nuwa_pytorch_amd.nuwa_pytorch import ReversibleSequence, _ReversibleStackFn, route_args
    torch.manual_seed(2)
    seq = ReversibleSequence([(_toy(8, p), _toy(8, p)) for _ in range(3)]).double().train()
    params = list(seq.parameters())
    x0 = torch.randn(2, 5, 8, dtype=torch.float64)
    args = route_args({}, {}, 3)
    out = []
    for efficient in (True, False):
        x = x0.clone().requires_grad_(True)
        for q in params:
            q.grad = None
        torch.manual_seed(9)
        y = _ReversibleStackFn.apply(x, None, seq, args) if efficient else seq(x)
        y.square().sum().backward()
        out.append((y.detach().clone(), _grads(params, x), torch.get_rng_state()))
    (ye, ge, se), (ys, gs, ss) = out
    assert torch.equal(ye, ys)
    for a, b in zip(ge, gs):
        assert float((a - b).abs().max()) <= 1e-9 * float(b.abs().max()), float((a - b).abs().max())
    assert torch.equal(se, ss)


def test_two_forwards_in_flight_keep_their_own_states():
    """the recorded states live on the autograd node: a second forward before the first backward does not overwrite them"""
    from nuwa_pytorch_amd.nuwa_pytorch import ReversibleSequence, _ReversibleStackFn, route_args
    torch.manual_seed(4)
    seq = ReversibleSequence([(_toy(8, 0.4), _toy(8, 0.4)) for _ in range(2)]).double().train()
    params = list(seq.parameters())
    args = route_args({}, {}, 2)
    xa, xb = (torch.randn(2, 3, 8, dtype=torch.float64) for _ in range(2))

    def ref(x0, seed):
        x = x0.clone().requires_grad_(True)
        for q in params:
            q.grad = None
        torch.manual_seed(seed)
        seq(x).square().sum().backward()
        return _grads(params, x)
    ra, rb = ref(xa, 1), ref(xb, 2)
    for q in params:
        q.grad = None
    x1, x2 = xa.clone().requires_grad_(True), xb.clone().requires_grad_(True)
    torch.manual_seed(1)
    y1 = _ReversibleStackFn.apply(x1, None, seq, args)
    torch.manual_seed(2)
    y2 = _ReversibleStackFn.apply(x2, None, seq, args)
    y1.square().sum().backward()
    g1 = _grads(params, x1)
    for q in params:
        q.grad = None
    y2.square().sum().backward()
    g2 = _grads(params, x2)
    for got, want in ((g1, ra), (g2, rb)):
        for a, b in zip(got, want):
            assert float((a - b).abs().max()) <= 1e-9 * float(b.abs().max())


def test_dual_recomputing_stack_replays_the_masks_of_its_forward():
    from nuwa_pytorch_amd.video_audio import DualModalityReversibleSequence, _DualReversibleStackFn
    torch.manual_seed(6)
    blocks = [[_toy(8, 0.3) for _ in range(4)] for _ in range(2)]
    seq = DualModalityReversibleSequence(blocks, ['intra_modality_self_attn'] * 2).double().train()
    params = list(seq.parameters())
    v0, a0 = torch.randn(2, 5, 8, dtype=torch.float64), torch.randn(2, 3, 8, dtype=torch.float64)
    out = []
    for efficient in (True, False):
        v, a = v0.clone().requires_grad_(True), a0.clone().requires_grad_(True)
        for q in params:
            q.grad = None
        torch.manual_seed(9)
        if efficient:
            yv, ya = _DualReversibleStackFn.apply(v, a, None, seq, dict(context_mask=None, video_mask=None, audio_mask=None))
        else:
            yv, ya = seq(v, a, context=None)
        (yv.square().sum() + ya.square().sum()).backward()
        out.append(([v.grad.clone(), a.grad.clone()] + [q.grad.clone() for q in params], torch.get_rng_state()))
    for x, y in zip(out[0][0], out[1][0]):
        assert float((x - y).abs().max()) <= 1e-9 * float(y.abs().max())
    assert torch.equal(out[0][1], out[1][1])
