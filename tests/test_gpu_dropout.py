"""Dropout in the fused and the reversible stacks on the MI355X (np.py:276; rev.py:20-50).

  * the two mask kernels of csrc/dropout.hip against the torch element-wise formulation they replace, written out here: bit for bit;
  * the A/B switch AMDNUWA_FF_DROP_TORCH (kernels.set_ff_drop_torch): both sides give the same bits through a FeedForward;
  * a FeedForward with live dropout runs as the inner stage of the fused block node, against torch fp32 with the same mask;
  * reversible stacks with dropout: the recomputing backward (RNG replay) gives the gradients of the stored-graph mode, rebuilds
    the stack's input, and leaves the HIP generator where the stored-graph mode leaves it; with dropout 0 nothing is recorded."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from gpu_util import report, rel_err  # noqa: E402
from test_gpu_modules import MODES  # noqa: E402

DEV = 'cuda'
SHAPES = [(1, 32), (96, 192), (97, 1376), (300, 64)]      # one row; the dim-64 FF (22 padding columns); the dim-512 width, odd rows; a short row
PS = [0.05, 0.25, 0.5]


@pytest.fixture(scope='module')
def A():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import nuwa_pytorch_amd
    return nuwa_pytorch_amd


def _drop(x_f32, keep, p):
    """the formulation the kernels replace: one fp32 multiply, a select"""
    return torch.where(keep, x_f32 * (1 / (1 - p)), torch.zeros((), dtype=torch.float32, device=x_f32.device))


def _masks(R, C, p, gen):
    wide = torch.zeros((R, C + 24), dtype=torch.bool, device=DEV)          # a keep mask with a row pitch larger than C
    wide[:, :C] = torch.rand((R, C), device=DEV, generator=gen) >= p
    return [('random', torch.rand((R, C), device=DEV, generator=gen) >= p), ('all-keep', torch.ones((R, C), dtype=torch.bool, device=DEV)),
            ('all-drop', torch.zeros((R, C), dtype=torch.bool, device=DEV)), ('pitched', wide[:, :C])]


def _pad0(C):
    return C - 22 if C >= 64 else C - 8          # first padding column of the test: the inputs are zero from here on (FFI ... FP)


@pytest.mark.parametrize('p', PS)
@pytest.mark.parametrize('R,C', SHAPES)
def test_forward_mask_kernel_is_bit_exact(A, R, C, p):
    from nuwa_pytorch_amd import kernels as K
    gen = torch.Generator(device=DEV).manual_seed(1000 * R + C)
    x = torch.randn((R, C), device=DEV, generator=gen) * 8.0             # well inside fp16's range, times 1 / (1 - p) too
    x[:, _pad0(C):] = 0
    scale = 1.0 / (1.0 - p)
    for name, keep in _masks(R, C, p, gen):
        assert name != 'pitched' or keep.stride(0) == C + 24
        # form (a): the fp16 gate copy -> dropped fp16 copy (out of place and in place) + dropped bf16 copy
        g16 = x.to(torch.float16)
        ref = _drop(g16.float(), keep, p)
        o16 = torch.full_like(g16, float('nan'))
        r16, rb = K.geglu_dropout_fwd_f16(g16, keep, scale, out16=o16)
        assert r16 is o16 and torch.equal(o16, ref.to(torch.float16)), (name, 'f16')
        assert torch.equal(rb, ref.to(torch.bfloat16)), (name, 'bf16 copy')
        assert torch.equal(g16, x.to(torch.float16))                      # the input is untouched out of place
        inpl = g16.clone()
        r16, rb2 = K.geglu_dropout_fwd_f16(inpl, keep, scale)
        assert r16 is inpl and torch.equal(inpl, o16) and torch.equal(rb2, rb), (name, 'in place')
        assert not bool(o16[:, _pad0(C):].any()) and not bool(rb[:, _pad0(C):].any())          # padding columns stay exactly zero
        # form (b): a bf16 hi or hi + lo pair in, a hi or hi + lo pair out
        for ilo in (False, True):
            hi = x.to(torch.bfloat16)
            g = K.BF(hi, (x - hi.float()).to(torch.bfloat16) if ilo else None)
            val = g.hi.float() + g.lo.float() if ilo else g.hi.float()
            for olo in (False, True):
                want = K.empty_bf((R, C), DEV, lo=olo)
                K.cast_pad(_drop(val, keep, p).contiguous(), want)
                got = K.geglu_dropout_fwd(g, keep, scale, lo=olo)
                assert torch.equal(got.hi, want.hi), (name, ilo, olo, 'hi')
                assert (got.lo is None) == (not olo)
                if olo:
                    assert torch.equal(got.lo, want.lo), (name, ilo, olo, 'lo')
                assert not bool(got.hi[:, _pad0(C):].any())


@pytest.mark.parametrize('p', PS)
@pytest.mark.parametrize('R,C', SHAPES)
def test_backward_mask_kernel_is_bit_exact(A, R, C, p):
    """amdnuwa_geglu_il_bwd_dropout on the undropped dgg == amdnuwa_geglu_il_bwd on the dropped, re-rounded dgd"""
    from nuwa_pytorch_amd import kernels as K
    gen = torch.Generator(device=DEV).manual_seed(7000 * R + C)
    FP = C
    uf = torch.randn((R, 2 * FP), device=DEV, generator=gen) * 1.5
    df = torch.randn((R, FP), device=DEV, generator=gen) * 4.0
    df[:, _pad0(C):] = 0
    scale = 1.0 / (1.0 - p)
    for name, keep in _masks(R, C, p, gen):
        for lo in (False, True):
            mk = lambda t: K.BF(t.to(torch.bfloat16), (t - t.to(torch.bfloat16).float()).to(torch.bfloat16) if lo else None)
            u, dgg = mk(uf), mk(df)
            val = dgg.hi.float() + dgg.lo.float() if lo else dgg.hi.float()
            dgd = K.empty_bf((R, FP), DEV, lo=lo)
            K.cast_pad(_drop(val, keep, p).contiguous(), dgd)
            want = K.geglu_bwd(u, dgd, FP, interleaved=True)
            got = K.geglu_il_bwd_dropout(u, dgg, keep, scale, FP)
            assert torch.equal(got.hi, want.hi), (name, lo, 'hi')
            if lo:
                assert torch.equal(got.lo, want.lo), (name, lo, 'lo')
            else:
                assert got.lo is None
            if name == 'all-drop':
                assert not bool(got.hi.any())


def test_fp16_store_saturates_and_keeps_nan(A):
    """form (a): a kept NaN stays NaN in both copies, a value beyond fp16's range (1e6 is inf as an fp16 input; 60000 / (1 - p) as a product)
    leaves as +-65504 in the fp16 copy, and a DROPPED NaN / inf is exactly 0 (a select, not a multiply by 0)"""
    from nuwa_pytorch_amd import kernels as K
    x = torch.zeros((4, 32), device=DEV)
    x[0, 0], x[0, 1], x[0, 2], x[0, 3], x[0, 4] = float('nan'), 1e6, -1e6, 60000.0, 3.0
    x[1, 0], x[1, 1] = float('nan'), 1e6
    keep = torch.ones((4, 32), dtype=torch.bool, device=DEV)
    keep[1] = False
    g16 = x.to(torch.float16)
    o16, ob = K.geglu_dropout_fwd_f16(g16.clone(), keep, 2.0)
    assert bool(torch.isnan(o16[0, 0])) and bool(torch.isnan(ob[0, 0]))
    assert float(o16[0, 1]) == 65504.0 and float(o16[0, 2]) == -65504.0 and float(o16[0, 3]) == 65504.0 and float(o16[0, 4]) == 6.0
    assert float(ob[0, 3]) == float(torch.tensor(120000.0).to(torch.bfloat16)) and float(ob[0, 4]) == 6.0
    assert not bool(o16[1].any()) and not bool(ob[1].any())
    assert not bool(o16[2:].any()) and not bool(ob[2:].any())


@pytest.mark.parametrize('mode,tol,gtol', MODES)
@pytest.mark.parametrize('dim', [64, 512])
def test_switch_sides_give_the_same_bits(A, monkeypatch, dim, mode, tol, gtol):
    from nuwa_pytorch_amd import ops, kernels as K
    torch.manual_seed(21)
    m = A.FeedForward(dim=dim, dropout=0.25).to(DEV).train()
    w1, w2 = m.net[0].weight, m.net[3].weight
    x = torch.randn(2, 48, dim, device=DEV, requires_grad=True)
    dy = torch.randn(2, 48, dim, device=DEV)
    keep_all = torch.rand(96, (w2.shape[1] + 31) // 32 * 32, device=DEV) >= 0.25
    monkeypatch.setattr(ops, '_ff_keep_mask', lambda R, C, pp, device: keep_all[:R, :C].clone())
    A.set_precision(mode)
    sides = []
    try:
        for torch_side in (False, True):
            K.set_ff_drop_torch(torch_side)
            for t in (x, w1, w2):
                t.grad = None
            y = m(x)
            y.backward(dy)
            sides.append((y.detach().clone(), x.grad.clone(), w1.grad.clone(), w2.grad.clone()))
    finally:
        K.set_ff_drop_torch(False)
        A.set_precision('bf16')
    for name, a, b in zip(('y', 'dx', 'dw1', 'dw2'), *sides):
        assert torch.equal(a, b), (name, rel_err(a, b))
    assert float(sides[0][0].abs().max()) > 0


@pytest.mark.parametrize('mode,tol,gtol', MODES)
def test_dropout_feedforward_runs_inside_the_fused_block(A, monkeypatch, mode, tol, gtol):
    """x + LN2(drop(geglu(LN1(x) W1^T)) W2^T): the FF block of a plain Transformer with ff_dropout > 0 in training is ONE fused node
    (kind 'ff' carrying drop_p), chained with its neighbours, and matches torch fp32 with the same mask"""
    import nuwa_pytorch_amd.nuwa_pytorch as M
    from nuwa_pytorch_amd import ops
    p = 0.25
    torch.manual_seed(5)
    tr = M.Transformer(dim=64, depth=1, heads=2, dim_head=32, causal=True, sparse_3dna_attn=True, sparse_3dna_video_shape=(2, 4, 4),
                       ff_dropout=p).to(DEV).train()
    block = tr.layers[0][2]
    ff = block.fn
    w1, w2 = ff.net[0].weight, ff.net[3].weight
    FFI = w2.shape[1]
    x = torch.randn(2, 33, 64, device=DEV, requires_grad=True)
    dy = torch.randn(2, 33, 64, device=DEV)
    stored = torch.rand(66, (FFI + 31) // 32 * 32, device=DEV) >= p
    monkeypatch.setattr(ops, '_ff_keep_mask', lambda R, C, pp, device: stored[:R, :C].clone())
    fused, alone = [], []
    fwd0, inner0 = ops.SandwichBlockFn.forward, ops.InnerFn.forward

    def spy_block(ctx, x_, resid, context, meta, *rest):
        fused.append((meta['kind'], meta.get('drop_p'), x_.detach().clone()))
        return fwd0(ctx, x_, resid, context, meta, *rest)

    def spy_inner(ctx, x_, context, meta, *rest):
        alone.append(meta['kind'])
        return inner0(ctx, x_, context, meta, *rest)
    monkeypatch.setattr(ops.SandwichBlockFn, 'forward', staticmethod(spy_block))
    monkeypatch.setattr(ops.InnerFn, 'forward', staticmethod(spy_inner))

    def reference(xin):
        xr = xin.detach().clone().requires_grad_(True)
        h = F.layer_norm(xr, (64,), block.prenorm.weight, block.prenorm.bias)
        a, g = (h.reshape(66, 64) @ w1.t()).chunk(2, dim=-1)
        gg = torch.where(stored[:, :FFI], a * F.gelu(g) * (1.0 / (1.0 - p)), torch.zeros((), device=DEV))
        yr = xr + F.layer_norm((gg @ w2.t()).reshape(2, 33, 64), (64,), block.postnorm.weight, block.postnorm.bias)
        return xr, yr
    params = dict(pre_w=block.prenorm.weight, pre_b=block.prenorm.bias, post_w=block.postnorm.weight, post_b=block.postnorm.bias, w1=w1, w2=w2)
    A.set_precision(mode)
    try:
        # inside the stack: routing, the block's output and its parameter gradients
        y = tr.forward_layers(x)
        y.backward(dy)
        kinds = [(k, d) for k, d, _ in fused]
        assert kinds == [('s3', None), ('ff', p)], kinds              # the FF ran as a fused block carrying drop_p ...
        assert 'ff' not in alone, alone                               # ... and not as a stand-alone node
        got = {k: v.grad.clone() for k, v in params.items()}
        for v in params.values():
            v.grad = None
        xr, yr = reference(fused[1][2])
        yr.backward(dy)
        report(f'fused_ff_dropout[{mode}].y', y.detach(), yr.detach(), tol)
        for k, v in params.items():
            report(f'fused_ff_dropout[{mode}].d{k}', got[k], v.grad, gtol)
            v.grad = None
        # the block on its own input: the input gradient too
        xin = torch.randn(2, 33, 64, device=DEV, requires_grad=True)
        yb = block.fused_residual(xin)
        yb.backward(dy)
        xr, yr = reference(xin)
        yr.backward(dy)
        report(f'fused_ff_dropout[{mode}].block.y', yb.detach(), yr.detach(), tol)
        report(f'fused_ff_dropout[{mode}].block.dx', xin.grad, xr.grad, gtol)
        assert float((yb.detach() - block.eval().fused_residual(xin).detach()).abs().max()) > 1e-3      # (the mask did something)
    finally:
        A.set_precision('bf16')


REV_KW = dict(dim=64, depth=3, causal=True, heads=2, dim_head=32, cross_attend=True, sparse_3dna_attn=True, sparse_3dna_video_shape=(2, 4, 4),
              shift_video_tokens=True)


def _rev_step(A, a, f, efficient, spy_block0=False, train=True):
    """one training step of the reversible stack in 'bf16x3': (dx, dctx, parameter grads, HIP generator state after the step, block-0
    reconstruction (x1, x2) when asked, the stack's input)"""
    import nuwa_pytorch_amd.nuwa_pytorch as M
    torch.manual_seed(0)
    tr = M.ReversibleTransformer(attn_dropout=a, ff_dropout=f, **REV_KW).to(DEV).train(train)
    tr.net.memory_efficient = efficient
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 33, 64, generator=g).to(DEV).requires_grad_(True)
    ctx = torch.randn(2, 6, 64, generator=g).to(DEV).requires_grad_(True)
    mask = torch.ones(2, 6, dtype=torch.bool, device=DEV)
    mask[1, 4:] = False
    seen = []
    if spy_block0:
        b0 = tr.net.blocks[0]
        orig = b0.backward_pass

        def spy(*args, **kw):
            out = orig(*args, **kw)
            seen.append((out[0].detach().clone(), out[1].detach().clone()))
            return out
        b0.backward_pass = spy
    y = tr(x, context=ctx, context_mask=mask)
    y.square().mean().backward()
    torch.cuda.synchronize()
    state = torch.cuda.get_rng_state()
    grads = {n: p.grad.clone() for n, p in tr.named_parameters() if p.grad is not None}
    return x.grad.clone(), ctx.grad.clone(), grads, state, (seen[0] if seen else None), x.detach()


@pytest.mark.parametrize('a,f', [(0.0, 0.25), (0.1, 0.0), (0.1, 0.25)])
def test_reversible_stack_with_dropout_recomputes_the_forward_it_ran(A, a, f):
    """gradients of the recomputing backward against the stored-graph mode, which draws the same masks in the same order and never
    recomputes (bound: the 2e-3 of the dropout-free comparison in test_gpu_modules).  Without RNG replay every case is off by order 1:
    the recomputed halves draw fresh masks, x2 = y2 - g(y1) is no longer the block's input."""
    A.set_precision('bf16x3')
    try:
        dx_e, dc_e, g_e, st_e, _, _ = _rev_step(A, a, f, True)
        dx_s, dc_s, g_s, st_s, _, _ = _rev_step(A, a, f, False)
    finally:
        A.set_precision('bf16')
    assert set(g_e) == set(g_s) and len(g_s) > 40
    worst = max([rel_err(dx_e, dx_s), rel_err(dc_e, dc_s)] + [rel_err(g_e[n], g_s[n]) for n in g_s])
    print(f'reversible dropout (attn {a}, ff {f}): worst relative error recomputing vs stored = {worst:.3e}')
    report(f'rev_dropout[{a},{f}].dx', dx_e, dx_s, 2e-3)
    report(f'rev_dropout[{a},{f}].dctx', dc_e, dc_s, 2e-3)
    for n in g_s:
        report(f'rev_dropout[{a},{f}].grad.{n}', g_e[n], g_s[n], 2e-3)
    assert torch.equal(st_e.cpu(), st_s.cpu())              # the main HIP stream leaves the backward where it went in


def test_reversible_reconstruction_returns_the_stack_input(A):
    """block 0's backward_pass rebuilds (x1, x2) = (x, x): with dropout the error stays at the rounding noise of the dropout-free
    stack (at most 4 x the figure measured here with both dropouts 0; a different mask gives order 1)"""
    A.set_precision('bf16x3')
    try:
        errs = {}
        for a, f in ((0.0, 0.0), (0.1, 0.25)):
            *_, rec, x = _rev_step(A, a, f, True, spy_block0=True)
            assert rec is not None
            errs[(a, f)] = max(rel_err(rec[0], x), rel_err(rec[1], x))
    finally:
        A.set_precision('bf16')
    print('reconstruction error of block 0 (relative to max |x|):', errs)
    assert errs[(0.0, 0.0)] > 0 or errs[(0.1, 0.25)] == 0
    assert errs[(0.1, 0.25)] <= 4 * errs[(0.0, 0.0)], errs


def test_reversible_dual_decoder_with_ff_dropout(A):
    import nuwa_pytorch_amd.video_audio as VA

    def run(efficient):
        torch.manual_seed(3)
        dec = VA.ReversibleDualModalityDecoder(dim=64, depth=4, heads=2, dim_head=32, num_audio_tokens_per_video_frame=8,
                                               num_video_tokens_per_frame=64, sparse_3dna_video_shape=(4, 8, 8),
                                               sparse_3dna_kernel_size=3, sparse_3dna_dilations=(1, 2), shift_video_tokens=True,
                                               shift_audio_tokens=True, cross_modality_attn_every=2, ff_dropout=0.25, attn_dropout=0.).to(DEV).train()
        g = torch.Generator().manual_seed(4)
        video = torch.randn(2, 1 + 4 * 64, 64, generator=g).to(DEV).requires_grad_(True)
        audio = torch.randn(2, 1 + 4 * 8, 64, generator=g).to(DEV).requires_grad_(True)
        ctx = torch.randn(2, 6, 64, generator=g).to(DEV).requires_grad_(True)
        cmask = torch.ones(2, 6, dtype=torch.bool, device=DEV)
        cmask[1, 4:] = False
        dec.net.memory_efficient = efficient
        v, a = dec(video, audio, context=ctx, context_mask=cmask)
        (v.square().mean() + a.square().mean()).backward()
        torch.cuda.synchronize()
        grads = {n: p.grad.clone() for n, p in dec.named_parameters() if p.grad is not None}
        return grads, video.grad.clone(), audio.grad.clone(), ctx.grad.clone(), torch.cuda.get_rng_state()
    A.set_precision('bf16x3')
    try:
        ge, dve, dae, dce, ste = run(True)
        gs, dvs, das, dcs, sts = run(False)
    finally:
        A.set_precision('bf16')
    assert set(ge) == set(gs) and len(ge) > 100
    worst = max([rel_err(dve, dvs), rel_err(dae, das), rel_err(dce, dcs)] + [rel_err(ge[n], gs[n]) for n in gs])
    print(f'dual reversible decoder, ff_dropout 0.25: worst relative error recomputing vs stored = {worst:.3e}')
    for n in ge:
        report(f'dual_rev_dropout.{n}', ge[n], gs[n], 2e-3)
    report('dual_rev_dropout.dvideo', dve, dvs, 2e-3)
    report('dual_rev_dropout.daudio', dae, das, 2e-3)
    report('dual_rev_dropout.dctx', dce, dcs, 2e-3)
    assert torch.equal(ste.cpu(), sts.cpu())


def test_dropout_zero_records_nothing_and_eval_is_dropout_free(A, monkeypatch):
    import nuwa_pytorch_amd.nuwa_pytorch as M
    calls = []
    record0 = M.RngReplay.record.__func__
    monkeypatch.setattr(M.RngReplay, 'record', classmethod(lambda cls, device=None: (calls.append(1), record0(cls, device))[1]))
    A.set_precision('bf16x3')
    try:
        _rev_step(A, 0.0, 0.0, True)
        assert not calls                                   # dropout 0: the parent's code path, nothing recorded, forked or set
        _rev_step(A, 0.1, 0.25, True)
        assert len(calls) == 3 * 3                         # (per depth: the FF of both blocks and the cross attention; the 3DNA block has no dropout)
        del calls[:]

        def eval_out(a, f):
            torch.manual_seed(0)
            tr = M.ReversibleTransformer(attn_dropout=a, ff_dropout=f, **REV_KW).to(DEV).eval()
            g = torch.Generator().manual_seed(1)
            x = torch.randn(2, 33, 64, generator=g).to(DEV)
            ctx = torch.randn(2, 6, 64, generator=g).to(DEV)
            with torch.no_grad():
                return tr(x, context=ctx, context_mask=torch.ones(2, 6, dtype=torch.bool, device=DEV))
        assert torch.equal(eval_out(0.1, 0.25), eval_out(0.0, 0.0))
        assert not calls
    finally:
        A.set_precision('bf16')
