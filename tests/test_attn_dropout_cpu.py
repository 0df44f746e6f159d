"""Attention dropout inside the window attention, without a GPU: the restatements of tests/attn_dropout_util.py against the oracle, what the
amdnuwa_sparse3dna_*_drop entry points return before they touch the device (null operands: AMDNUWA_ERR_ARG = geometry accepted,
AMDNUWA_ERR_UNSUPPORTED = refused; the geometry check comes first), the mask helper, and the PyTorch-op branches of SparseCausal2DNA and
CrossModalityCrossAttention in training on CPU tensors.

Bounds of the module comparisons: module and restatement are two fp32 formulations of the same sums (gather vs padded slices, one
einsum vs a per-frame loop) of at most 65 products per output element on O(1) data: 1e-5 of the largest reference value (fp32 eps 6e-8 x
the few hundred roundings on the way, with room), max-abs error over max-abs reference as gpu_util.rel_err."""
import ctypes
import math

import pytest
import torch

from attn_dropout_util import (FixedMaskDropout, cross_modality_cross_attention_drop, keep_to_bhij, keep_to_kernel,
                               sparse3dna_core_drop, sparse_causal_2dna_drop)
from gpu_util import rel_err

ARG, UNSUPPORTED = -1, -2
TOL = 1e-5


@pytest.fixture(scope='module')
def O():
    from oracle import nuwa_oracle
    return nuwa_oracle


# ---------------------------------------------------------------------------------------------------
# 1. the restatement is the oracle when nothing is dropped
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('shape,kern,dil,heads,rel', [((2, 4, 4), (3, 3, 3), (1, 1, 1), 2, True), ((9, 1, 1), (5, 1, 1), (2, 1, 1), 4, False)])
def test_restatement_with_a_full_mask_is_the_oracle(O, shape, kern, dil, heads, rel):
    torch.manual_seed(0)
    b, d = 2, 8
    n = 1 + shape[0] * shape[1] * shape[2]
    J = kern[0] * kern[1] * kern[2] + 1
    q, k, v = (torch.randn(b, n, heads, d) for _ in range(3))
    wth = torch.randn(heads, heads)
    bias = torch.randn(heads, J - 1) if rel else None
    idx = O.neighbor_table(shape, kern, dil, causal=True)
    want = O.sparse3dna_core(q, k, v, wth, idx, d ** -0.5, rel_pos_bias=bias)
    got = sparse3dna_core_drop(q, k, v, wth, idx, d ** -0.5, torch.ones(b, heads, n - 1, J), 1.0, rel_pos_bias=bias)
    assert torch.equal(got, want)
    # ... and a mask does what nn.Dropout does to the mixed map: a fully dropped query row outputs 0
    keep = torch.ones(b, heads, n - 1, J)
    keep[1, :, 3] = 0
    got = sparse3dna_core_drop(q, k, v, wth, idx, d ** -0.5, keep, 2.0, rel_pos_bias=bias)
    assert bool((got[1, 4] == 0).all()) and torch.equal(got[:, 0], v[:, 0])


def test_mask_layout_conversions_are_inverse():
    keep = torch.rand(2, 5, 7, 3) > 0.5                       # kernel order [B, nq, J, heads]
    assert keep_to_bhij(keep).shape == (2, 3, 5, 7)
    assert torch.equal(keep_to_kernel(keep_to_bhij(keep)), keep) and keep_to_kernel(keep_to_bhij(keep)).is_contiguous()
    assert bool(keep_to_bhij(keep)[1, 2, 4, 6] == keep[1, 4, 6, 2])


# ---------------------------------------------------------------------------------------------------
# 2. the entry points' argument checks
# ---------------------------------------------------------------------------------------------------

def _geom(F, H, W, heads, dh=64, kernel=(3, 3, 3), dilation=(1, 1, 1), noncausal=0, B=2):
    from nuwa_pytorch_amd import _lib
    g = _lib.S3Geom()
    g.B, g.ntok = B, 1 + F * H * W
    g.F, g.H, g.W = F, H, W
    g.kf, g.kh, g.kw = kernel
    g.df, g.dh, g.dw = dilation
    g.heads, g.dim_head, g.scale = heads, dh, dh ** -0.5
    g.rel_bias, g.d_rel_bias, g.noncausal = None, None, noncausal
    return g


def _fwd(L, g, keep, scale):
    return L.amdnuwa_sparse3dna_fwd_drop(ctypes.byref(g), None, None, None, None, None, None, 512, None, None, None, 512, keep, scale, None)


def _bwd(L, g, keep, scale):
    return L.amdnuwa_sparse3dna_bwd_drop(ctypes.byref(g), None, None, None, None, None, None, 512, None, None, None, 512, None, None, None,
                                         None, None, None, 512, None, 0, None, 0, keep, scale, None)


# the audio grid, a small video grid, two column tiles, the decoder's 16 x 16 map (a band-kernel geometry when unmasked), the widest map
ACCEPTED = [(33, 1, 1, 8, 64, (7, 1, 1)), (2, 4, 4, 2, 32, (3, 3, 3)), (1, 3, 20, 8, 32, (3, 3, 3)), (2, 16, 16, 8, 64, (3, 3, 3)),
            (1, 64, 64, 8, 64, (3, 3, 3))]


@pytest.mark.parametrize('lo', [0, 1])
@pytest.mark.parametrize('F,H,W,heads,dh,kernel', ACCEPTED)
def test_drop_entry_points_with_null_operands(F, H, W, heads, dh, kernel, lo):
    from nuwa_pytorch_amd import _lib
    L = _lib.lib()
    g = _geom(F, H, W, heads, dh=dh, kernel=kernel)
    some = ctypes.create_string_buffer(16)                  # a non-null keep pointer: never dereferenced, the operand check fails first
    assert L.amdnuwa_s3_drop_supported(ctypes.byref(g), lo) == 1
    assert _fwd(L, g, some, 1.25) == ARG and _bwd(L, g, some, 1.25) == ARG           # accepted geometry, null operands
    assert _fwd(L, g, None, 1.25) == ARG and _bwd(L, g, None, 1.25) == ARG           # keep = NULL
    for bad in (0.5, math.inf, -math.inf, math.nan, 0.0, 0.999):
        assert _fwd(L, g, some, bad) == ARG and _bwd(L, g, some, bad) == ARG, bad


@pytest.mark.parametrize('lo', [0, 1])
def test_drop_entry_points_refuse_what_the_window_kernels_refuse(lo):
    from nuwa_pytorch_amd import _lib
    L = _lib.lib()
    some = ctypes.create_string_buffer(16)
    refused = [_geom(1, 20, 20, 9), _geom(1, 20, 20, 8, dh=48), _geom(2, 4, 4, 2, dh=32, noncausal=1), _geom(1, 65, 65, 8),
               _geom(2, 32, 32, 8, kernel=(3, 3, 3), dilation=(1, 1, 200))]
    for g in refused:
        assert L.amdnuwa_s3_drop_supported(ctypes.byref(g), lo) == 0
        for keep, scale in ((some, 1.25), (None, 1.25), (some, 0.5)):                # the geometry check comes before the argument checks
            assert _fwd(L, g, keep, scale) == UNSUPPORTED and _bwd(L, g, keep, scale) == UNSUPPORTED
    # the symmetric window itself is a geometry of the unmasked kernels
    assert L.amdnuwa_s3_supported(ctypes.byref(_geom(2, 4, 4, 2, dh=32, noncausal=1)), lo) == 1
    # the LDS limit is the unmasked kernels': (5,5,5) on a 32-wide map fits in bf16 only (test_wide_grid_cpu.py)
    g = _geom(2, 32, 32, 8, kernel=(5, 5, 5))
    assert L.amdnuwa_s3_drop_supported(ctypes.byref(g), lo) == L.amdnuwa_s3_supported(ctypes.byref(g), lo) == (0 if lo else 1)


def test_signatures_are_declared():
    from nuwa_pytorch_amd import _lib
    hdr = open(_lib.HERE + '/../include/amdnuwa.h').read()
    for name in ('amdnuwa_s3_drop_supported', 'amdnuwa_sparse3dna_fwd_drop', 'amdnuwa_sparse3dna_bwd_drop'):
        assert name in _lib.SIGNATURES and f'int {name}(' in hdr
    assert len(_lib.SIGNATURES['amdnuwa_sparse3dna_fwd_drop'][1]) == len(_lib.SIGNATURES['amdnuwa_sparse3dna_fwd'][1]) + 2
    assert len(_lib.SIGNATURES['amdnuwa_sparse3dna_bwd_drop'][1]) == len(_lib.SIGNATURES['amdnuwa_sparse3dna_bwd'][1]) + 2
    assert _lib.ABI_VERSION == 21 and _lib.lib().amdnuwa_abi_version() == 21         # additive entry points


# ---------------------------------------------------------------------------------------------------
# 3. the mask helper
# ---------------------------------------------------------------------------------------------------

def test_attn_keep_mask_draws_one_rand_from_torchs_stream():
    from nuwa_pytorch_amd import ops
    B, nq, J, heads, p = 2, 33, 8, 8, 0.25
    torch.manual_seed(5)
    keep = ops._attn_keep_mask(B, nq, J, heads, p, 'cpu')
    after = torch.get_rng_state()
    assert keep.shape == (B, nq, J, heads) and keep.dtype == torch.bool
    torch.manual_seed(5)
    twin = torch.rand((B, nq, J, heads)) >= p
    assert torch.equal(torch.get_rng_state(), after)        # exactly one rand of that shape was consumed
    assert torch.equal(keep, twin)
    torch.manual_seed(5)
    assert torch.equal(ops._attn_keep_mask(B, nq, J, heads, p, 'cpu'), keep)
    n = keep.numel()
    rate, sigma = float(keep.float().mean()), math.sqrt(0.75 * 0.25 / n)
    assert n == 2 * 33 * 8 * 8 and abs(rate - 0.75) <= 4 * sigma, (rate, sigma)


# ---------------------------------------------------------------------------------------------------
# 4. the PyTorch-op branches in training, CPU tensors, injected masks
# ---------------------------------------------------------------------------------------------------

def _P(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items()}


@pytest.mark.parametrize('full', [False, True])
def test_sparse_causal_2dna_torch_branch_with_dropout(O, full):
    """on the parent commit SparseCausal2DNA(dropout > 0).train() raises NotImplementedError"""
    from nuwa_pytorch_amd.video_audio import SparseCausal2DNA
    torch.manual_seed(1)
    heads, dh, ks, dil, b, n, dim = 2, 16, 5, 2, 2, 20, 32
    m = SparseCausal2DNA(dim=dim, heads=heads, dim_head=dh, kernel_size=ks, dilation=dil, dropout=.25).train()
    x = torch.randn(b, n, dim)
    y_live = m(x)                                             # the live nn.Dropout: runs, finite
    assert y_live.shape == (b, n, dim) and bool(torch.isfinite(y_live).all())
    g = torch.Generator().manual_seed(2)
    keep = torch.ones(b, heads, n - 1, ks + 1) if full else (torch.rand(b, heads, n - 1, ks + 1, generator=g) >= 0.25).float()
    s = 1.0 if full else 1.0 / 0.75
    if not full:
        keep[0, :, 5] = 0                                     # a fully dropped query row
        keep[1, 1, 7, 1:] = 0
        keep[1, 1, 7, 0] = 1                                  # only <bos> kept
    m.dropout = FixedMaskDropout(keep, s)
    P = _P(m)
    xg = x.clone().requires_grad_(True)
    y = m(xg)
    assert m.dropout.calls == 1
    xr = x.clone().requires_grad_(True)
    want = sparse_causal_2dna_drop(xr, P, heads, ks, dil, keep, s)
    assert rel_err(y, want) <= TOL
    dy = torch.randn(b, n, dim, generator=g)
    y.backward(dy)
    want.backward(dy)
    assert rel_err(xg.grad, xr.grad) <= TOL
    if full:
        assert rel_err(y, O.sparse_causal_2dna(x, P, heads, ks, dil)) <= TOL
    else:
        # the dropped row of sample 0 outputs to_out(0) = 0 (to_out has no bias)
        assert float(y.detach()[0, 6].abs().max()) == 0.0
    # eval: the dropout-free value
    m.eval()
    with torch.no_grad():
        assert rel_err(m(x), O.sparse_causal_2dna(x, P, heads, ks, dil)) <= TOL
    assert m.dropout.calls == 1


@pytest.mark.parametrize('full', [False, True])
def test_cross_modality_cross_attention_torch_branch_with_dropout(O, full):
    """on the parent commit CrossModalityCrossAttention(dropout > 0).train() raises NotImplementedError"""
    from nuwa_pytorch_amd.video_audio import CrossModalityCrossAttention
    torch.manual_seed(3)
    heads, dh, c, cc, b, dim, frames = 2, 16, 4, 3, 2, 32, 3
    m = CrossModalityCrossAttention(dim=dim, chunk_size=c, context_chunk_size=cc, heads=heads, dim_head=dh, dropout=.25).train()
    with torch.no_grad():
        m.talking_heads.bias.add_(0.1 * torch.randn(heads))
    seq, ctx = torch.randn(b, 1 + frames * c, dim), torch.randn(b, 1 + (frames - 1) * cc, dim)
    y_live = m(seq, ctx)
    assert y_live.shape == seq.shape and bool(torch.isfinite(y_live).all())
    g = torch.Generator().manual_seed(4)
    shape = (b, heads, frames, c, cc + 1)
    keep = torch.ones(shape) if full else (torch.rand(shape, generator=g) >= 0.25).float()
    s = 1.0 if full else 1.0 / 0.75
    if not full:
        keep[0, :, 1, 2] = 0                                  # a fully dropped query: only the Conv3d bias term is left
    m.dropout = FixedMaskDropout(keep, s)
    P = _P(m)
    sg, cg = seq.clone().requires_grad_(True), ctx.clone().requires_grad_(True)
    y = m(sg, cg)
    assert m.dropout.calls == 1
    sr, cr = seq.clone().requires_grad_(True), ctx.clone().requires_grad_(True)
    want = cross_modality_cross_attention_drop(sr, cr, P, heads, c, cc, keep, s)
    assert rel_err(y, want) <= TOL
    dy = torch.randn(seq.shape, generator=g)
    y.backward(dy)
    want.backward(dy)
    assert rel_err(sg.grad, sr.grad) <= TOL and rel_err(cg.grad, cr.grad) <= TOL
    if full:
        assert rel_err(y, O.cross_modality_cross_attention(seq, ctx, P, heads, c, cc)) <= TOL


def test_dropout_position_differs_between_the_two_modules():
    """SparseCausal2DNA drops AFTER the talking-heads mix (np.py:747-748), CrossModalityCrossAttention BEFORE it (np.py:1048-1051): with a
    mask that drops one head's weights and a mix that is not diagonal, dropping on the other side of the mix gives another result"""
    torch.manual_seed(6)
    b, h, i, j = 1, 2, 3, 4
    attn = torch.rand(b, h, i, j).softmax(-1)
    w = torch.tensor([[1.0, 0.5], [0.25, 1.0]])
    keep = torch.ones(b, h, i, j)
    keep[:, 0] = 0
    after = torch.einsum('gh,bhij->bgij', w, attn) * keep
    before = torch.einsum('gh,bhij->bgij', w, attn * keep)
    assert bool((after[:, 0] == 0).all()) and float(before[:, 0].abs().min()) > 0
