"""Attention dropout inside the Sparse3DNA window kernels on the MI355X: the masked forms of the VALU kernels (row and column-tiled, bf16
and hi + lo operands) against the restatement of tests/attn_dropout_util.py, then SparseCausal2DNA / Sparse3DNA in training, the dual
decoders and a tiny NUWAVideoAudio with the README's switches.

Metric: gpu_util.report (max-abs error / max-abs reference).  Kernel bounds are those test_gpu_wide_grid.py::test_wide_sparse3dna_core
applies to the same kernels without a mask: forward 3e-5 as hi + lo pairs / 2^-7 in bf16, dq / dk / dv, dW_th and d(rel bias) 5e-5 /
2^-6 -- dW_th in bf16 at that test's own 1e-4, the tighter of the two.  The mask only scales entries by 0 or 1 / (1 - p); the reference
carries the same factor, so the relative bounds are unchanged.  Module bounds: the MODES of test_gpu_modules.py."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from attn_dropout_util import keep_to_bhij, sparse3dna_core_drop, sparse3dna_drop, sparse_causal_2dna_drop  # noqa: E402
from gpu_util import report, rel_err, bf_round, to_bf_pair, bf_value  # noqa: E402
from guard_util import guard, guarded  # noqa: E402

DEV = 'cuda'
MODES = [('bf16x3', 1e-3, 2e-3), ('bf16x3-fwd', 1e-3, 7e-2), ('bf16', 2e-2, 7e-2)]
P_DROP = 0.25
S = 1.0 / (1.0 - P_DROP)


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


@pytest.fixture(scope='module')
def O():
    from oracle import nuwa_oracle
    return nuwa_oracle


# ---------------------------------------------------------------------------------------------------
# 1. kernels
# ---------------------------------------------------------------------------------------------------

# name: (grid, kernel, dilation, heads, dim_head, ntok, rel_bias).  None is a band-kernel geometry (those need a 16-wide grid).
# A: the audio grid of cfg 5; A2: dilated, the sequence ends inside the grid; B / B2: a (2,4,4) video grid with the relative-position bias,
# full and ending inside a frame; C: 20 columns x 8 heads = 640 threads, two column tiles of 10 (sparse3dna_wide.hip)
CASES = {
    'A': ((33, 1, 1), (7, 1, 1), (1, 1, 1), 8, 64, 34, False),
    'A2': ((33, 1, 1), (5, 1, 1), (2, 1, 1), 2, 32, 20, False),
    'B': ((2, 4, 4), (3, 3, 3), (1, 1, 1), 2, 32, 33, True),
    'B2': ((2, 4, 4), (3, 3, 3), (1, 1, 1), 2, 32, 21, True),
    'C': ((1, 3, 20), (3, 3, 3), (1, 1, 1), 8, 32, 61, False),
}
B_ = 2


def _mask(case, ones=False):
    """kernel-order keep mask [B, nq, J, heads]: Bernoulli(0.75) from a fixed generator, query row nq // 3 of sample 0 fully dropped,
    (sample 1, query 2 nq // 3, head 1) with only the <bos> slot kept.  At C the two queries sit in different column tiles."""
    shape, kern, _, heads, _, n, _ = CASES[case]
    nq, J = n - 1, kern[0] * kern[1] * kern[2] + 1
    if ones:
        return torch.ones(B_, nq, J, heads, dtype=torch.bool), None, None
    g = torch.Generator().manual_seed(sum(map(ord, case)))
    keep = torch.rand(B_, nq, J, heads, generator=g) < 0.75
    r0, r1 = nq // 3, 2 * nq // 3
    keep[0, r0] = False
    keep[1, r1, :, 1] = False
    keep[1, r1, 0, 1] = True
    return keep, r0, r1


_REF = {}


def _reference(O, case, x3, masked):
    """inputs and the fp64 restatement's results for one case (computed once, read-only)"""
    key = (case, x3, masked)
    if key in _REF:
        return _REF[key]
    shape, kern, dil, heads, dh, n, rel_bias = CASES[case]
    J = kern[0] * kern[1] * kern[2] + 1
    torch.manual_seed(31 + sum(map(ord, case)))
    qkv = torch.randn(B_, n, 3, heads, dh)
    do = torch.randn(B_, n, heads, dh)
    if not x3:
        qkv, do = bf_round(qkv), bf_round(do)
    wth = torch.randn(heads, heads) * 0.5 + torch.eye(heads)
    rel = torch.randn(heads, J - 1) * 0.7 if rel_bias else None                 # oracle layout (h, K)
    keep, r0, r1 = _mask(case, ones=not masked)
    q64 = qkv.double().requires_grad_(True)
    w64 = wth.double().requires_grad_(True)
    rel64 = rel.double().requires_grad_(True) if rel_bias else None
    idx = O.neighbor_table(shape, kern, dil, causal=True)
    o = sparse3dna_core_drop(q64[:, :, 0], q64[:, :, 1], q64[:, :, 2], w64, idx, dh ** -0.5, keep_to_bhij(keep).double(),
                             S if masked else 1.0, rel_pos_bias=rel64)
    o.backward(do.double())
    _REF[key] = dict(qkv=qkv, do=do, wth=wth, rel=rel, keep=keep, r0=r0, r1=r1, o=o.detach(), dqkv=q64.grad, dwth=w64.grad,
                     drel=rel64.grad if rel_bias else None)
    return _REF[key]


def _operands(K, case, x3, R, do=None):
    """guarded device copies of one case's operands"""
    shape, kern, dil, heads, dh, n, _ = CASES[case]
    inner = heads * dh
    pair = lambda t: K.BF(*(guarded(p, device=DEV) if p is not None else None for p in to_bf_pair(t, x3)[:2]))
    qkv = pair(R['qkv'].reshape(B_ * n, 3 * inner))
    dO = pair((R['do'] if do is None else do).reshape(B_ * n, inner))
    wth = guarded(R['wth'], device=DEV)
    rel = guarded(torch.cat((torch.zeros(1, heads), R['rel'].t()), 0).contiguous(), device=DEV) if R['rel'] is not None else None
    return qkv, dO, wth, rel


def _run(K, case, x3, R, keep, scale, do=None):
    """forward + backward of one case under the guard -> (o, dqkv, dwth, drel) as fp32 values and the raw bf16 parts"""
    shape, kern, dil, heads, dh, n, _ = CASES[case]
    g = K.s3_geom(B_, n, shape, kern, dil, heads, dh)
    qkv, dO, wth, rel = _operands(K, case, x3, R, do)
    kw = {} if keep is None else dict(keep=guarded(keep.to(torch.uint8), device=DEV), drop_scale=scale)
    with guard(K) as gd:
        o = K.sparse3dna_fwd(g, qkv, wth, rel_bias=rel, **kw)
        dqkv, dwth, drel = K.sparse3dna_bwd(g, qkv, wth, dO, rel_bias=rel, **kw)
        assert gd.made() > 0
    raw = [t for t in (o.hi, o.lo, dqkv.hi, dqkv.lo, dwth, drel) if t is not None]
    val = lambda p: bf_value(p) if x3 else p.hi.float()
    return val(o), val(dqkv), dwth, drel, raw


@pytest.mark.parametrize('x3', [False, True])
@pytest.mark.parametrize('case', list(CASES))
def test_masked_window_kernels(K, O, case, x3):
    shape, kern, dil, heads, dh, n, rel_bias = CASES[case]
    inner = heads * dh
    g = K.s3_geom(B_, n, shape, kern, dil, heads, dh)
    assert K.s3_drop_supported(g, lo=x3) and not K.s3_f16_supported(g)
    assert (g.W * heads * 4 > 512) == (case == 'C')
    R = _reference(O, case, x3, True)
    o, dqkv, dwth, drel, raw = _run(K, case, x3, R, R['keep'], S)
    tag = f'[{case},x3={x3}]'
    tol_o, tol_g = (3e-5, 5e-5) if x3 else (2 ** -7, 2 ** -6)
    # ---- values
    report('s3drop_fwd' + tag, o.reshape(B_, n, heads, dh), R['o'], tol_o)
    gq = R['dqkv'].reshape(B_ * n, 3 * inner)
    for nm, sl in (('dq', slice(0, inner)), ('dk', slice(inner, 2 * inner)), ('dv', slice(2 * inner, 3 * inner))):
        report(f's3drop_bwd_{nm}' + tag, dqkv[:, sl], gq[:, sl], tol_g)
    report('s3drop_bwd_dwth' + tag, dwth, R['dwth'], 5e-5 if x3 else 1e-4)
    if rel_bias:
        report('s3drop_bwd_drel' + tag, drel[1:].t(), R['drel'], tol_g)
    # ---- exact zeros: the fully dropped query row (sample 0, query r0 = token row r0 + 1) outputs 0 and has dq = 0 ...
    row = 1 + R['r0']
    assert float(o.reshape(B_, n, inner)[0, row].abs().max()) == 0.0
    assert float(dqkv.reshape(B_, n, 3 * inner)[0, row, :inner].abs().max()) == 0.0
    # the <bos> query row outputs its own value row, whatever the mask says
    assert torch.equal(o.reshape(B_, n, inner)[:, 0].cpu(), bf_value(to_bf_pair(R['qkv'][:, 0, 2].reshape(B_, inner), x3)))
    # ... and contributes exactly 0 to dW_th: with another dO row there (no other query reads it), dW_th keeps its bits
    do2 = R['do'].clone()
    do2[0, row] = bf_round(torch.randn(heads, dh, generator=torch.Generator().manual_seed(1)) * 3)
    _, dqkv2, dwth2, drel2, raw2 = _run(K, case, x3, R, R['keep'], S, do=do2)
    assert torch.equal(dwth2, dwth)
    if rel_bias:
        assert torch.equal(drel2, drel)
    assert float(dqkv2.reshape(B_, n, 3 * inner)[0, row, :inner].abs().max()) == 0.0
    # ---- repeatability: a second run gives the same bits
    *_, raw3 = _run(K, case, x3, R, R['keep'], S)
    assert len(raw) == len(raw3) >= 3
    for a, b in zip(raw, raw3):
        assert torch.equal(a, b)


@pytest.mark.parametrize('x3', [False, True])
@pytest.mark.parametrize('case', list(CASES))
def test_full_mask_at_scale_one_is_the_unmasked_kernels_bit_for_bit(K, O, case, x3):
    R = _reference(O, case, x3, False)
    *_, plain = _run(K, case, x3, R, None, 1.0)
    *_, ones = _run(K, case, x3, R, R['keep'], 1.0)
    assert bool(R['keep'].all()) and len(plain) == len(ones) >= 3
    for a, b in zip(plain, ones):
        assert torch.equal(a.view(torch.int16 if a.dtype == torch.bfloat16 else torch.int32), b.view(torch.int16 if b.dtype == torch.bfloat16 else torch.int32))
    assert all(bool(torch.isfinite(t.float()).all()) for t in ones)


def test_wrapper_refuses_a_mask_of_the_wrong_shape_or_form(K):
    shape, kern, dil, heads, dh, n, _ = CASES['A2']
    g = K.s3_geom(B_, n, shape, kern, dil, heads, dh)
    qkv = to_bf_pair(torch.zeros(B_ * n, 3 * heads * dh, device=DEV), False)
    wth = torch.eye(heads, device=DEV)
    with pytest.raises(ValueError):
        K.sparse3dna_fwd(g, qkv, wth, keep=torch.ones(B_, n - 1, 6, heads + 1, dtype=torch.bool, device=DEV), drop_scale=S)
    with pytest.raises(RuntimeError, match='amdnuwa_sparse3dna_fwd_drop'):          # drop_scale < 1: AMDNUWA_ERR_ARG from the library
        K.sparse3dna_fwd(g, qkv, wth, keep=torch.ones(B_, n - 1, 6, heads, dtype=torch.bool, device=DEV), drop_scale=0.5)


# ---------------------------------------------------------------------------------------------------
# 2. modules in train() mode
# ---------------------------------------------------------------------------------------------------

@pytest.fixture
def spies(monkeypatch, K):
    """what ran: keep arguments of the kernel wrappers, (node, kind, drop_p) of the library nodes, calls of ops._attn_keep_mask"""
    from nuwa_pytorch_amd import ops
    seen = dict(fwd=[], bwd=[], nodes=[], draws=[])
    f0, b0, inner0, block0, draw0 = K.sparse3dna_fwd, K.sparse3dna_bwd, ops.InnerFn.forward, ops.SandwichBlockFn.forward, ops._attn_keep_mask
    monkeypatch.setattr(K, 'sparse3dna_fwd', lambda *a, **k: (seen['fwd'].append(k.get('keep') is not None), f0(*a, **k))[1])
    monkeypatch.setattr(K, 'sparse3dna_bwd', lambda *a, **k: (seen['bwd'].append(k.get('keep') is not None), b0(*a, **k))[1])
    monkeypatch.setattr(ops.InnerFn, 'forward', staticmethod(
        lambda ctx, x, context, meta, *p: (seen['nodes'].append(('inner', meta['kind'], meta.get('drop_p'))), inner0(ctx, x, context, meta, *p))[1]))
    monkeypatch.setattr(ops.SandwichBlockFn, 'forward', staticmethod(
        lambda ctx, x, resid, context, meta, *p: (seen['nodes'].append(('block', meta['kind'], meta.get('drop_p'))), block0(ctx, x, resid, context, meta, *p))[1]))
    seen['draw0'] = draw0
    return seen


def _fixed_mask(monkeypatch, seen, keep):
    from nuwa_pytorch_amd import ops

    def fixed(B, nq, J, heads, p, device):
        seen['draws'].append((B, nq, J, heads, p))
        assert tuple(keep.shape) == (B, nq, J, heads)
        return keep.to(device)
    monkeypatch.setattr(ops, '_attn_keep_mask', fixed)


def _count_calls(mod):
    calls = []
    mod.register_forward_hook(lambda *a: calls.append(1))
    return calls


def _grads_of(mod):
    return {n: p.grad.clone() for n, p in mod.named_parameters() if p.grad is not None}


@pytest.mark.parametrize('mode,tol,gtol', MODES)
@pytest.mark.parametrize('fused', [False, True])
def test_sparse_causal_2dna_trains_with_dropout_on_the_masked_kernels(A, O, spies, monkeypatch, fused, mode, tol, gtol):
    """stand-alone (ops.InnerFn) and as SandwichNorm(ShiftAudioTokens(.)) through _residual (the fused node); on the parent commit the
    module raises NotImplementedError"""
    from nuwa_pytorch_amd import video_audio as VA
    from nuwa_pytorch_amd.nuwa_pytorch import SandwichNorm
    torch.manual_seed(0)
    heads, ks, dil, b, n, dim = 2, 5, 2, 2, 34, 64
    attn = VA.SparseCausal2DNA(dim=dim, heads=heads, dim_head=32, kernel_size=ks, dilation=dil, dropout=P_DROP)
    m = SandwichNorm(dim=dim, fn=VA.ShiftAudioTokens(attn)) if fused else attn
    with torch.no_grad():
        for k, p in m.named_parameters():
            if 'norm' in k:
                p.add_(0.1 * torch.randn_like(p))
    g = torch.Generator().manual_seed(7)
    x, dy = torch.randn(b, n, dim, generator=g), torch.randn(b, n, dim, generator=g)
    keep = torch.rand(b, n - 1, ks + 1, heads, generator=g) >= P_DROP
    keep[0, 11] = False
    # fp32 restatement with the same mask
    P = {k: v.detach().clone().requires_grad_(True) for k, v in attn.state_dict().items()}
    xr = x.clone().requires_grad_(True)
    if fused:
        N = {k: v.detach().clone().requires_grad_(True) for k, v in m.state_dict().items() if 'norm' in k}
        h = O.shift_audio_tokens(F.layer_norm(xr, (dim,), N['prenorm.weight'], N['prenorm.bias']))
        yr = xr + F.layer_norm(sparse_causal_2dna_drop(h, P, heads, ks, dil, keep_to_bhij(keep), S), (dim,), N['postnorm.weight'], N['postnorm.bias'])
        want = {**{'fn.fn.' + k: v for k, v in P.items()}, **N}
    else:
        yr = sparse_causal_2dna_drop(xr, P, heads, ks, dil, keep_to_bhij(keep), S)
        want = P
    yr.backward(dy)
    m = m.to(DEV).train()
    torch_branch = _count_calls(attn.dropout)
    _fixed_mask(monkeypatch, spies, keep)
    A.set_precision(mode)
    try:
        xd = x.to(DEV).requires_grad_(True)
        y = VA._residual(m, xd) if fused else m(xd)
        tag = f'sc2dna_drop[fused={fused},{mode}]'
        report(tag + '.y', y, yr.detach(), tol)
        y.backward(dy.to(DEV))
        report(tag + '.dx', xd.grad, xr.grad, gtol)
        got = _grads_of(m)
        assert set(got) == set(want)
        for k, gr in got.items():
            report(tag + f'.grad.{k}', gr, want[k].grad, gtol)
    finally:
        A.set_precision('bf16')
    assert spies['nodes'] == [('block' if fused else 'inner', 's3', P_DROP)]
    assert spies['fwd'] == [True] and spies['bwd'] == [True] and len(spies['draws']) == 1
    assert not torch_branch                                  # the PyTorch-op branch (the only caller of the module's nn.Dropout) did not run


@pytest.mark.parametrize('mode,tol,gtol', MODES)
def test_sparse3dna_trains_with_dropout_on_the_masked_kernels(A, O, spies, monkeypatch, mode, tol, gtol):
    """causal Sparse3DNA with the relative-position bias; on the parent commit _meta raises NotImplementedError"""
    torch.manual_seed(0)
    heads, shape, b, n, dim = 2, (2, 4, 4), 2, 33, 64
    m = A.Sparse3DNA(dim=dim, video_shape=shape, heads=heads, dim_head=32, causal=True, rel_pos_bias=True, dropout=P_DROP)
    g = torch.Generator().manual_seed(8)
    x, dy = torch.randn(b, n, dim, generator=g), torch.randn(b, n, dim, generator=g)
    keep = torch.rand(b, n - 1, 28, heads, generator=g) >= P_DROP
    keep[1, 20] = False
    P = {k: v.detach().clone().requires_grad_(True) for k, v in m.state_dict().items() if v.is_floating_point()}
    xr = x.clone().requires_grad_(True)
    yr = sparse3dna_drop(xr, P, shape, 3, 1, heads, keep_to_bhij(keep), S, O)
    yr.backward(dy)
    m = m.to(DEV).train()
    torch_branch = _count_calls(m.dropout)
    _fixed_mask(monkeypatch, spies, keep)
    A.set_precision(mode)
    try:
        xd = x.to(DEV).requires_grad_(True)
        y = m(xd)
        tag = f's3_drop[{mode}]'
        report(tag + '.y', y, yr.detach(), tol)
        y.backward(dy.to(DEV))
        report(tag + '.dx', xd.grad, xr.grad, gtol)
        got = _grads_of(m)
        assert set(got) == {k for k in P if P[k].grad is not None} and len(got) >= 8
        for k, gr in got.items():
            report(tag + f'.grad.{k}', gr, P[k].grad, gtol)
    finally:
        A.set_precision('bf16')
    assert spies['nodes'] == [('inner', 's3', P_DROP)]
    assert spies['fwd'] == [True] and spies['bwd'] == [True] and len(spies['draws']) == 1 and not torch_branch


@pytest.mark.parametrize('mode', [m[0] for m in MODES])
def test_eval_takes_the_dropout_free_path(A, spies, monkeypatch, mode):
    """.eval(): bit-equal to a dropout = 0 twin, no mask drawn, the unmasked wrappers"""
    from nuwa_pytorch_amd import ops, video_audio as VA
    monkeypatch.setattr(ops, '_attn_keep_mask', lambda *a: (spies['draws'].append(a), spies['draw0'](*a))[1])
    g = torch.Generator().manual_seed(9)
    x = torch.randn(2, 34, 64, generator=g).to(DEV)
    A.set_precision(mode)
    try:
        outs = []
        for p in (P_DROP, 0.0):
            torch.manual_seed(0)
            a = VA.SparseCausal2DNA(dim=64, heads=2, dim_head=32, kernel_size=5, dilation=2, dropout=p).to(DEV).eval()
            torch.manual_seed(0)
            v = A.Sparse3DNA(dim=64, video_shape=(2, 4, 4), heads=2, dim_head=32, causal=True, rel_pos_bias=True, dropout=p).to(DEV).eval()
            with torch.no_grad():
                outs.append((a(x), v(x[:, :33])))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    finally:
        A.set_precision('bf16')
    assert not spies['draws'] and spies['fwd'] == [False] * 4
    assert all(n == ('inner', 's3', None) for n in spies['nodes']) and len(spies['nodes']) == 4


# ---------------------------------------------------------------------------------------------------
# 3. dual decoders: kwargs of test_gpu_dropout.py::test_reversible_dual_decoder_with_ff_dropout, attn_dropout = 0.1
# ---------------------------------------------------------------------------------------------------

DUAL_KW = dict(dim=64, depth=4, heads=2, dim_head=32, num_audio_tokens_per_video_frame=8, num_video_tokens_per_frame=64,
               sparse_3dna_video_shape=(4, 8, 8), sparse_3dna_kernel_size=3, sparse_3dna_dilations=(1, 2), shift_video_tokens=True,
               shift_audio_tokens=True, cross_modality_attn_every=2, ff_dropout=0.25, attn_dropout=0.1)


def _dual_step(VA, cls, efficient):
    torch.manual_seed(3)
    dec = cls(**DUAL_KW).to(DEV).train()
    g = torch.Generator().manual_seed(4)
    video = torch.randn(2, 1 + 4 * 64, 64, generator=g).to(DEV).requires_grad_(True)
    audio = torch.randn(2, 1 + 4 * 8, 64, generator=g).to(DEV).requires_grad_(True)
    ctx = torch.randn(2, 6, 64, generator=g).to(DEV).requires_grad_(True)
    cmask = torch.ones(2, 6, dtype=torch.bool, device=DEV)
    cmask[1, 4:] = False
    if efficient is not None:
        dec.net.memory_efficient = efficient
    v, a = dec(video, audio, context=ctx, context_mask=cmask)
    (v.square().mean() + a.square().mean()).backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.clone() for n, p in dec.named_parameters() if p.grad is not None}
    return grads, video.grad.clone(), audio.grad.clone(), ctx.grad.clone(), torch.cuda.get_rng_state()


@pytest.mark.parametrize('reversible', [False, True])
def test_dual_decoders_train_with_attn_dropout(A, spies, reversible):
    """the reversible decoder: gradients of the recomputing backward (masks replayed from the recorded RNG states) against the stored
    graph, 2e-3 as test_reversible_dual_decoder_with_ff_dropout; the plain decoder: two seeded steps.  The HIP generator ends in the same
    state either way.  On the parent commit both raise NotImplementedError in the audio tower."""
    import nuwa_pytorch_amd.video_audio as VA
    cls = VA.ReversibleDualModalityDecoder if reversible else VA.DualModalityDecoder
    A.set_precision('bf16x3')
    try:
        ge, dve, dae, dce, ste = _dual_step(VA, cls, True if reversible else None)
        first = list(spies['nodes'])
        gs, dvs, das, dcs, sts = _dual_step(VA, cls, False if reversible else None)
    finally:
        A.set_precision('bf16')
    # the audio tower's window attention ran as fused nodes with live dropout, on the masked wrappers, forward and backward
    audio = [nd for nd in first if nd[1] == 's3' and nd[2] is not None]
    assert len(audio) == (8 if reversible else 4) and all(nd == ('block', 's3', 0.1) for nd in audio), first     # (reversible: forward + recomputation)
    assert sum(spies['fwd']) >= 8 and sum(spies['bwd']) == 8
    assert set(ge) == set(gs) and len(ge) > 100
    tag = f'dual_attn_dropout[rev={reversible}]'
    for n in ge:
        report(f'{tag}.{n}', ge[n], gs[n], 2e-3)
    report(tag + '.dvideo', dve, dvs, 2e-3)
    report(tag + '.daudio', dae, das, 2e-3)
    report(tag + '.dctx', dce, dcs, 2e-3)
    assert all(bool(torch.isfinite(t).all()) for t in ge.values())
    assert torch.equal(ste.cpu(), sts.cpu())


# ---------------------------------------------------------------------------------------------------
# 4. whole model: the README example's switches
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('reversible', [False, True])
def test_video_audio_model_trains_with_the_readme_dropout(A, spies, reversible):
    """one forward(return_loss=True), backward and FusedAdamW step of a tiny NUWAVideoAudio with attn_dropout = ff_dropout = 0.05; on the
    parent commit the forward raises NotImplementedError"""
    from nuwa_pytorch_amd.optimizer import FusedAdamW
    from test_gpu_modules import VA_KW
    torch.manual_seed(0)
    vae = A.VQGanVAE(dim=32, image_size=16, num_layers=2, vq_codebook_size=64, vq_codebook_dim=32, use_vgg_and_gan=False)
    m = A.NUWAVideoAudio(vae=vae, attn_dropout=0.05, ff_dropout=0.05, **{**VA_KW, 'dec_reversible': reversible}).to(DEV).train()
    tpf, apf = m.num_video_tokens_per_frame, m.num_audio_tokens_per_video_frame
    g = torch.Generator().manual_seed(1)
    text = torch.randint(1, 50, (2, 8), generator=g).to(DEV)
    vid = torch.randint(0, 64, (2, 3 * tpf), generator=g).to(DEV)
    aud = torch.randint(0, 40, (2, 3 * apf), generator=g).to(DEV)
    params = [p for k, p in m.named_parameters() if not k.startswith('vae.')]
    opt = FusedAdamW(params, lr=1e-3)
    A.set_precision('bf16x3-fwd')
    try:
        loss = m(text=text, video=vid, audio=aud, return_loss=True)
        loss.backward()
        before = [p.detach().clone() for p in params[:4]]
        opt.step()
        torch.cuda.synchronize()
    finally:
        A.set_precision('bf16')
    assert bool(torch.isfinite(loss.detach()))
    with_grad = [p for p in params if p.grad is not None]
    assert len(with_grad) > 100 and all(bool(torch.isfinite(p.grad).all()) for p in with_grad)
    assert all(bool(torch.isfinite(p).all()) for p in params) and any(not torch.equal(a, p.detach()) for a, p in zip(before, params[:4]))
    assert any(nd[1] == 's3' and nd[2] == 0.05 for nd in spies['nodes']) and any(spies['fwd']) and any(spies['bwd'])
