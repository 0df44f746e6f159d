"""Token grids wider than 16 columns on the MI355X: the column-tiled window kernels (csrc/sparse3dna_wide.hip) against the oracle and
against a fixture captured from the reference, from the kernels up to a NUWA model on a 20 x 20 feature map.

Metric: gpu_util.report (max-abs error / max-abs reference).  Tolerances are the project's own: kernel level as
test_gpu_kernels.py::test_sparse3dna_core (forward 2^-7 in bf16 / 3e-5 as hi + lo pairs, dq / dk / dv 2^-6 / 5e-5, dW_th 1e-4), module
level the MODES of test_gpu_modules.py."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from golden_util import load, tup  # noqa: E402
from gpu_util import report, bf_round, to_bf_pair, bf_value  # noqa: E402

DEV = 'cuda'
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


@pytest.fixture(scope='module')
def O():
    from oracle import nuwa_oracle
    return nuwa_oracle


def _grads_of(mod):
    return {n: p.grad.clone() for n, p in mod.named_parameters() if p.grad is not None}


@pytest.fixture
def kinds(monkeypatch):
    """meta['kind'] of every ops.InnerFn.forward / ops.SandwichBlockFn.forward call: which library route a module took"""
    from nuwa_pytorch_amd import ops
    seen = []
    inner, block = ops.InnerFn.forward, ops.SandwichBlockFn.forward
    monkeypatch.setattr(ops.InnerFn, 'forward', staticmethod(lambda ctx, x, context, meta, *p: (seen.append(('inner', meta['kind'])), inner(ctx, x, context, meta, *p))[1]))
    monkeypatch.setattr(ops.SandwichBlockFn, 'forward',
                        staticmethod(lambda ctx, x, resid, context, meta, *p: (seen.append(('block', meta['kind'])), block(ctx, x, resid, context, meta, *p))[1]))
    return seen


# ---------------------------------------------------------------------------------------------------
# 1. kernels against O.sparse3dna_core
# ---------------------------------------------------------------------------------------------------

# (shape, kernel, dilation, heads, dh, n): 17 = one column past a 16-column row (2 tiles: 9 + 8); 20 with dilation 2 on every axis; 33 with
# kw 5 at dilation 4 (3 tiles of 11, halo 16 > the tile) and a sequence that ends mid-row; 40 x 4 heads (2 tiles of 20); 48 x 3 heads
# (2 tiles of 24); 64 x 8 heads (4 tiles of 16), the widest required, 5 rows + 7 tokens
WIDE_CASES = [((1, 17, 17), (3, 3, 3), (1, 1, 1), 8, 32, None), ((2, 20, 20), (3, 3, 3), (2, 2, 2), 8, 64, None),
              ((2, 33, 33), (3, 3, 5), (1, 1, 4), 8, 32, 1200), ((1, 40, 40), (3, 3, 3), (1, 1, 1), 4, 64, None),
              ((1, 48, 48), (3, 3, 3), (1, 1, 1), 3, 32, 500), ((1, 64, 64), (1, 3, 3), (1, 1, 2), 8, 64, 1 + 64 * 5 + 7)]


def _core_case(K, O, case, x3, rel_bias=False):
    shape, kern, dil, heads, dh, n = WIDE_CASES[case]
    N = shape[0] * shape[1] * shape[2]
    n = N if n is None else n
    B = 2
    inner = heads * dh
    J = kern[0] * kern[1] * kern[2] + 1
    torch.manual_seed(11 + case)
    qkv = torch.randn(B, n, 3, heads, dh)
    if not x3:
        qkv = bf_round(qkv)
    qkv.requires_grad_(True)
    wth = torch.randn(heads, heads) * 0.5 + torch.eye(heads)
    wth.requires_grad_(True)
    rel = (torch.randn(heads, J - 1) * 0.7).requires_grad_(True) if rel_bias else None      # oracle layout (h, K)
    idx = O.neighbor_table(shape, kern, dil, causal=True)
    o_ref = O.sparse3dna_core(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], wth, idx, dh ** -0.5, rel_pos_bias=rel)
    do = torch.randn_like(o_ref)
    if not x3:
        do = bf_round(do)
    o_ref.backward(do)
    g = K.s3_geom(B, n, shape, kern, dil, heads, dh)
    assert g.W * heads * 4 > 512 and K.s3_supported(shape, kern, dil, heads, dh, lo=x3)
    qkvp = to_bf_pair(qkv.detach().reshape(B * n, 3 * inner).to(DEV), x3)
    rel_dev = None
    if rel_bias:
        rel_dev = torch.cat((torch.zeros(1, heads), rel.detach().t()), 0).contiguous().to(DEV)   # kernel layout [J, heads], slot 0 = <bos>
    o = K.sparse3dna_fwd(g, qkvp, wth.detach().to(DEV), rel_bias=rel_dev)
    tol_o = 3e-5 if x3 else 2 ** -7
    tag = f'[{case},x3={x3},rel={rel_bias}]'
    report('s3w_fwd' + tag, (bf_value(o) if x3 else o.hi.float()).reshape(B, n, heads, dh), o_ref.detach(), tol_o)
    dqkv, dwth, drel = K.sparse3dna_bwd(g, qkvp, wth.detach().to(DEV), to_bf_pair(do.reshape(B * n, inner).to(DEV), x3), rel_bias=rel_dev)
    gq = qkv.grad.reshape(B * n, 3 * inner)
    got = bf_value(dqkv) if x3 else dqkv.hi.float()
    tol_g = 5e-5 if x3 else 2 ** -6
    for nm, sl in (('dq', slice(0, inner)), ('dk', slice(inner, 2 * inner)), ('dv', slice(2 * inner, 3 * inner))):
        report(f's3w_bwd_{nm}' + tag, got[:, sl], gq[:, sl], tol_g)
    report('s3w_bwd_dwth' + tag, dwth, wth.grad, 1e-4)
    if rel_bias:
        # d(bias) = column sums of ds, an fp32 workspace in both operand forms: the bound of dW_th's fp32 reduction in the hi + lo form,
        # the bf16 gradient bound in the bf16 form (as test_sparse3dna_core_rel_pos_bias_on_the_mfma_kernels)
        report('s3w_bwd_drel' + tag, drel[1:].t(), rel.grad, 1e-4 if x3 else 2 ** -6)


@pytest.mark.parametrize('case', range(len(WIDE_CASES)))
@pytest.mark.parametrize('x3', [False, True])
def test_wide_sparse3dna_core(K, O, case, x3):
    _core_case(K, O, case, x3)


@pytest.mark.parametrize('x3', [False, True])
def test_wide_sparse3dna_core_rel_pos_bias(K, O, x3):
    """(2,20,20), dilation 2, 8 x 64 with the relative-position bias: output, dq / dk / dv, dW_th and d(bias)"""
    _core_case(K, O, 1, x3, rel_bias=True)


# ---------------------------------------------------------------------------------------------------
# 2. determinism: several workgroups per CU, several rounds of them
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('x3', [False, True])
def test_wide_sparse3dna_is_bitwise_reproducible(K, x3):
    shape, kern, dil, heads, dh, B = (2, 20, 20), (3, 3, 3), (1, 1, 1), 8, 64, 16
    n = 1 + 800
    inner = heads * dh
    g = torch.Generator().manual_seed(3)
    qkv = to_bf_pair(torch.randn(B * n, 3 * inner, generator=g).to(DEV), x3)
    do = to_bf_pair(torch.randn(B * n, inner, generator=g).to(DEV), x3)
    wth = (torch.randn(heads, heads, generator=g) * 0.5 + torch.eye(heads)).to(DEV)
    geom = K.s3_geom(B, n, shape, kern, dil, heads, dh)
    runs = []
    for _ in range(2):
        o = K.sparse3dna_fwd(geom, qkv, wth)
        dqkv, dwth, _ = K.sparse3dna_bwd(geom, qkv, wth, do)
        torch.cuda.synchronize()
        runs.append([t.clone() for t in (o.hi, o.lo, dqkv.hi, dqkv.lo, dwth) if t is not None])
    assert len(runs[0]) >= 3
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    assert all(bool(torch.isfinite(t.float()).all()) for t in runs[0])


# ---------------------------------------------------------------------------------------------------
# 3. the module against the fixture captured from the reference
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('mode,tol,gtol', MODES)
def test_g15_sparse3dna_wide_module(A, kinds, mode, tol, gtol):
    """tests/golden/g15_sparse3dna_wide.npz (tests/golden/make_golden_wide_grid.py): the reference's Sparse3DNA on a (1, 17, 17) grid, 8 heads"""
    Ar, P, G = load('g15_sparse3dna_wide')
    m = A.Sparse3DNA(dim=32, video_shape=tup(Ar['video_shape']), kernel_size=tup(Ar['kernel_size']), heads=int(Ar['heads']), dim_head=32,
                     causal=True)
    m.load_state_dict(P)
    m = m.to(DEV)
    A.set_precision(mode)
    try:
        x = Ar['x'].to(DEV).requires_grad_(True)
        y = m(x)
        assert kinds == [('inner', 's3')]
        report(f'g15w[{mode}].y', y, Ar['y'], tol)
        y.backward(Ar['dy'].to(DEV))
        report(f'g15w[{mode}].dx', x.grad, Ar['dx'], gtol)
        named = dict(m.named_parameters())
        assert set(G) == set(named)
        for k, g in G.items():
            report(f'g15w[{mode}].grad.{k}', named[k].grad, g, gtol)
    finally:
        A.set_precision('bf16')


# ---------------------------------------------------------------------------------------------------
# 4. symmetric-window Sparse3DNA and SparseCross2DNA against the oracle
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('mode,tol,gtol', MODES)
@pytest.mark.parametrize('shape,kernel,dil,n,heads,dh,rel', [((2, 20, 20), 3, 1, 801, 8, 32, False), ((1, 24, 24), (3, 3, 5), (1, 1, 2), 400, 8, 64, True)])
def test_wide_noncausal_sparse3dna_hip_vs_oracle(A, O, kinds, shape, kernel, dil, n, heads, dh, rel, mode, tol, gtol):
    torch.manual_seed(0)
    dim = 64
    m = A.Sparse3DNA(dim=dim, video_shape=shape, kernel_size=kernel, dilation=dil, heads=heads, dim_head=dh, causal=False, rel_pos_bias=rel)
    P = {k: v.detach().cpu().clone().requires_grad_(v.is_floating_point()) for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(n)
    x, dy = torch.randn(2, n, dim, generator=g), torch.randn(2, n, dim, generator=g)
    xr = x.clone().requires_grad_(True)
    yr = O.sparse3dna(xr, P, shape, kernel, dil, heads, causal=False)
    yr.backward(dy)
    m = m.to(DEV)
    A.set_precision(mode)
    try:
        assert m._hip_ok() is True
        xd = x.to(DEV).requires_grad_(True)
        y = m(xd)
        assert kinds == [('inner', 's3')]
        tag = f'nc3dna_wide[{shape},{kernel},{dil},{n},{mode}]'
        report(tag + '.y', y, yr.detach(), tol)
        y.backward(dy.to(DEV))
        report(tag + '.dx', xd.grad, xr.grad, gtol)
        for k, gr in _grads_of(m).items():
            report(tag + f'.grad.{k}', gr, P[k].grad, gtol)
    finally:
        A.set_precision('bf16')


@pytest.mark.parametrize('mode,tol,gtol', MODES)
@pytest.mark.parametrize('fmap,heads,dh,kernel,dil,frames,n,masking', [(20, 8, 32, 3, 1, 2, 451, 'rand'), (24, 8, 64, 5, 2, 1, 301, 'frame')])
def test_wide_sparse_cross_2dna_hip_vs_oracle(A, O, kinds, fmap, heads, dh, kernel, dil, frames, n, masking, mode, tol, gtol):
    from nuwa_pytorch_amd.nuwa_pytorch import SparseCross2DNA
    torch.manual_seed(0)
    dim = 64
    m = SparseCross2DNA(dim=dim, image_size=fmap, heads=heads, dim_head=dh, kernel_size=kernel, dilation=dil)
    T = frames * fmap * fmap
    P = {k: v.detach().cpu().clone().requires_grad_(v.is_floating_point()) for k, v in m.state_dict().items()}
    g = torch.Generator().manual_seed(n + fmap)
    x, ctx, dy = torch.randn(2, n, dim, generator=g), torch.randn(2, T, dim, generator=g), torch.randn(2, n, dim, generator=g)
    if masking == 'frame':                           # sample 1 hides its last sketch frame
        mask = torch.ones(2, T, dtype=torch.bool)
        mask[1, (frames - 1) * fmap * fmap:] = False
    else:
        mask = torch.rand(2, T, generator=g) > 0.3
    xr, cr = x.clone().requires_grad_(True), ctx.clone().requires_grad_(True)
    yr = O.sparse_cross_2dna(xr, cr, P, heads, fmap, kernel, dil, context_mask=mask)
    yr.backward(dy)
    m = m.to(DEV)
    A.set_precision(mode)
    try:
        assert m._hip_ok(T) is True
        xd, cd = x.to(DEV).requires_grad_(True), ctx.to(DEV).requires_grad_(True)
        y = m(xd, context=cd, context_mask=mask.to(DEV))
        assert kinds == [('inner', 'xc2')]
        tag = f'xc2_wide[{fmap},{heads},{kernel},{dil},{n},{masking},{mode}]'
        report(tag + '.y', y, yr.detach(), tol)
        y.backward(dy.to(DEV))
        report(tag + '.dx', xd.grad, xr.grad, gtol)
        report(tag + '.dctx', cd.grad, cr.grad, gtol)
        for k, gr in _grads_of(m).items():
            report(tag + f'.grad.{k}', gr, P[k].grad, gtol)
    finally:
        A.set_precision('bf16')


# ---------------------------------------------------------------------------------------------------
# 5. decoder stacks: fused blocks, token shift, chained hand-off, reversible form
# ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def stack_case(O):
    """inputs + the oracle's results for both stack classes on a (2, 20, 20) grid (computed once, read-only)"""
    import nuwa_pytorch_amd.nuwa_pytorch as M
    vs, dim, n, T = (2, 20, 20), 64, 2 * 20 * 20, 6
    g = torch.Generator().manual_seed(7)
    x, ctx, dy = torch.randn(2, n, dim, generator=g), torch.randn(2, T, dim, generator=g), torch.randn(2, n, dim, generator=g)
    mask = torch.ones(2, T, dtype=torch.bool)
    mask[1, 4:] = False
    cfg = dict(video_shape=vs, kernel_size=3, dilations=(1, 2), heads=8, depth=2, shift=True)
    out = dict(x=x, ctx=ctx, dy=dy, mask=mask)
    for rev, cls, fn in ((False, M.Transformer, O.decoder_stack), (True, M.ReversibleTransformer, O.reversible_decoder_stack)):
        torch.manual_seed(0)
        tr = cls(dim=dim, depth=2, causal=True, heads=8, dim_head=32, cross_attend=True, sparse_3dna_attn=True,
                 sparse_3dna_video_shape=vs, sparse_3dna_dilations=(1, 2), shift_video_tokens=True)
        with torch.no_grad():                      # non-trivial norm parameters and biases
            for n_, p in tr.named_parameters():
                if 'norm' in n_ or n_.endswith('.bias'):
                    p.add_(0.1 * torch.randn_like(p))
        P = {k: v.detach().cpu().clone() for k, v in tr.state_dict().items() if not k.startswith('net.')}
        Pr = {k: (v.clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in P.items()}
        xr, cr = x.clone().requires_grad_(True), ctx.clone().requires_grad_(True)
        yr = fn(xr, Pr, cfg, cr, mask)
        yr.backward(dy)
        out[rev] = dict(module=tr, y=yr.detach(), dx=xr.grad, dctx=cr.grad, grads={k: v.grad for k, v in Pr.items() if torch.is_tensor(v) and v.grad is not None})
    return out


@pytest.mark.parametrize('mode,tol,gtol', MODES)
@pytest.mark.parametrize('reversible', [False, True])
def test_wide_decoder_stack_vs_oracle(A, stack_case, kinds, reversible, mode, tol, gtol):
    c, r = stack_case, stack_case[reversible]
    tr = r['module'].to(DEV).train()
    A.set_precision(mode)
    try:
        tr.zero_grad(set_to_none=True)
        xd, cd = c['x'].to(DEV).requires_grad_(True), c['ctx'].to(DEV).requires_grad_(True)
        y = tr(xd, context=cd, context_mask=c['mask'].to(DEV))
        # the self-attention blocks run as fused nodes of kind 's3' (one per depth), never as bare inner calls or torch ops
        s3 = [k for k in kinds if k[1] == 's3']
        assert len(s3) >= 2 and all(k[0] == 'block' for k in s3), kinds
        tag = f'wide_stack[rev={reversible},{mode}]'
        report(tag + '.y', y, r['y'], tol)
        y.backward(c['dy'].to(DEV))
        report(tag + '.dx', xd.grad, r['dx'], gtol)
        report(tag + '.dctx', cd.grad, r['dctx'], gtol)
        named = dict(tr.named_parameters())
        assert len(r['grads']) > 30
        for k, gr in r['grads'].items():
            report(tag + f'.grad.{k}', named[k].grad, gr, gtol)
    finally:
        A.set_precision('bf16')


# ---------------------------------------------------------------------------------------------------
# 6. a model on a 20 x 20 feature map: training step, cached decoding
# ---------------------------------------------------------------------------------------------------

def _nuwa20(A):
    torch.manual_seed(0)
    vae = A.VQGanVAE(dim=32, image_size=80, num_layers=2, vq_codebook_size=64, vq_codebook_dim=32, use_vgg_and_gan=False)
    return A.NUWA(vae=vae, dim=64, text_num_tokens=50, text_max_seq_len=8, max_video_frames=2, text_enc_depth=1, dec_depth=2,
                  enc_reversible=True, dec_heads=8, dec_dim_head=32, text_enc_heads=2, text_enc_dim_head=32, sparse_3dna_kernel_size=3,
                  sparse_3dna_dilation=(1, 2))


def test_wide_nuwa_training_step_is_finite(A):
    nuwa = _nuwa20(A).to(DEV).train()
    assert nuwa.video_fmap_size == 20
    g = torch.Generator().manual_seed(1)
    text = torch.randint(1, 50, (2, 8), generator=g).to(DEV)
    ids = torch.randint(0, 64, (2, 2 * 400), generator=g).to(DEV)
    A.set_precision('bf16x3-fwd')
    try:
        loss = nuwa(text=text, video=ids, return_loss=True, cond_dropout_prob=0.)
        loss.backward()
        torch.cuda.synchronize()
    finally:
        A.set_precision('bf16')
    assert bool(torch.isfinite(loss.detach())) and abs(float(loss.detach()) - 4.16) < 1.0, float(loss.detach())     # ~ln(64) at random init
    dec = [(k, p) for k, p in nuwa.named_parameters() if k.startswith('video_transformer.') or k.startswith('to_logits')]
    assert len(dec) > 30
    for k, p in dec:
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
        if 'to_q.weight' in k or 'to_kv.weight' in k:
            assert float(p.grad.abs().max()) > 0, k


@pytest.mark.parametrize('mode,tol', [('bf16x3', 1e-3), ('bf16', 1e-2)])
def test_wide_cached_rows_equal_the_full_forward(A, mode, tol):
    """teacher-forced rows 0..45 through the cached row program (the decoder of generate()) against the full-sequence forward of the same
    model: rows 21..45 have taps in the grid row above, left and right of a tile edge (bounds of
    test_gpu_decode.py::test_teacher_forced_cached_logits_match_reference_golden)"""
    from nuwa_pytorch_amd.decode import GuidedStepper
    nuwa = _nuwa20(A).to(DEV).eval()
    g = torch.Generator().manual_seed(2)
    text = torch.randint(1, 50, (2, 8), generator=g).to(DEV)
    ids = torch.randint(0, 64, (2, 45), generator=g).to(DEV)
    A.set_precision(mode)
    try:
        with torch.no_grad():
            mask = text != 0
            emb = nuwa.embed_text(text, mask=mask)
            rows = nuwa.embed_video(ids)                                          # [2, 46, dim]: <bos> + 45 tokens
            full = nuwa._final(nuwa.decode_hidden(rows, emb, mask))
            st = GuidedStepper(nuwa, emb, mask, rows.shape[1], 1., graph=False)
            got = torch.stack([st(rows[:, t].contiguous()).clone() for t in range(rows.shape[1])], 1)
        report(f'wide_cached_logits[{mode}]', got, full, tol)
    finally:
        A.set_precision('bf16')


# ---------------------------------------------------------------------------------------------------
# 7. narrow shapes: the same workspace as before the column tiles
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape,heads', [((4, 8, 8), 4), ((3, 4, 4), 3)])
def test_narrow_grid_workspace_is_unchanged(K, shape, heads):
    """one partial per query ROW: (2 B nq J heads + rows heads^2 + 2 rows inner) floats + 256 + the column-sum workspace"""
    from nuwa_pytorch_amd import _lib
    L = _lib.lib()
    B, dh, kern = 2, 64, (3, 3, 3)
    nq = shape[0] * shape[1] * shape[2]
    g = K.s3_geom(B, nq + 1, shape, kern, (1, 1, 1), heads, dh)
    J, rows, inner = 28, B * shape[0] * shape[1], heads * dh
    want = (2 * B * nq * J * heads + rows * heads * heads + 2 * rows * inner) * 4 + 256 + L.amdnuwa_colsum_workspace_bytes(B * nq, J * heads)
    assert L.amdnuwa_sparse3dna_bwd_workspace_bytes(ctypes.byref(g)) == want
