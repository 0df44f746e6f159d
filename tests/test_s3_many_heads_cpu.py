"""Sparse3DNA with more than 8 heads, everything that needs no device.  No kernel of the library takes such a geometry (the window, band
and single-row decode kernels stop at 8 heads): the entry points keep refusing it with AMDNUWA_ERR_UNSUPPORTED, and the modules say so by
name before anything is launched -- the causal window, which has no PyTorch-op formulation, with a NotImplementedError that names the limit
instead of an error code from the library; the symmetric window by staying on its PyTorch-op formulation; the cached decoder by declining
the block at construction."""
import ctypes

import pytest
import torch

import test_s3_entry_contract_cpu as T


@pytest.fixture(scope='module')
def L():
    from nuwa_pytorch_amd import _lib
    return _lib.lib()


def test_the_entries_still_refuse_nine_heads(L):
    g = T.geom('heads9', B=0)
    for entry in ('amdnuwa_sparse3dna_fwd', 'amdnuwa_sparse3dna_bwd', 'amdnuwa_cross2dna_fwd'):
        assert T.call(L, entry, g, {}) == T.UNSUPPORTED, entry
    assert L.amdnuwa_s3_supported(ctypes.byref(g), 0) == 0 and L.amdnuwa_s3_drop_supported(ctypes.byref(g), 0) == 0
    assert L.amdnuwa_sparse3dna_bwd_workspace_bytes(ctypes.byref(g)) == 0


def test_abi_version_is_unchanged(L):
    assert L.amdnuwa_abi_version() == 21


def _s3(heads, **kw):
    import nuwa_pytorch_amd as A
    return A.Sparse3DNA(dim=32, heads=heads, dim_head=32, **{'causal': True, 'video_shape': (2, 4, 4), 'kernel_size': 3, **kw})


@pytest.mark.parametrize('heads', [9, 12, 16, 17])
def test_causal_many_heads_name_the_limit(heads):
    m = _s3(heads)
    with pytest.raises(NotImplementedError, match=f'{heads} heads.*up to 8 heads'):
        m._meta(2, 33, torch.device('cpu'))
    with pytest.raises(NotImplementedError, match='up to 8 heads'):           # the bare module: before anything touches a device
        m(torch.zeros(2, 33, 32))


def test_eight_heads_plan_as_before():
    m = _s3(8)
    assert m._hip_ok()
    meta = m._meta(2, 33, torch.device('cpu'))
    assert meta['kind'] == 's3' and meta['geom'].heads == 8 and 'drop_p' not in meta
    assert _s3(8, dropout=.1).train()._meta(2, 33, torch.device('cpu'))['drop_p'] == pytest.approx(.1)


def test_symmetric_many_heads_stay_on_torch_ops():
    m = _s3(12, causal=False)
    assert not m._hip_ok()
    y = m(torch.randn(2, 33, 32, generator=torch.Generator().manual_seed(0)))      # _forward_noncausal, on the CPU
    assert y.shape == (2, 33, 32) and bool(torch.isfinite(y).all())


def test_incremental_decoder_declines_a_sixteen_head_block(monkeypatch):
    """at construction, while it walks the blocks and at the Sparse3DNA block itself (the cast of the text context, the one device call
    before that walk, is stubbed)"""
    import nuwa_pytorch_amd as A
    from nuwa_pytorch_amd import decode, ops
    monkeypatch.setattr(ops, '_ctx_to_bf', lambda context: None)
    m = A.Transformer(dim=32, depth=1, heads=16, dim_head=32, causal=True, cross_attend=True, sparse_3dna_attn=True,
                      sparse_3dna_video_shape=(2, 4, 4), sparse_3dna_kernel_size=3, shift_video_tokens=True)
    ctx = torch.zeros(2, 4, 32)
    with pytest.raises(NotImplementedError, match='16 heads'):
        decode.IncrementalDecoder(m, 2, 33, ctx, torch.ones(2, 4, dtype=torch.bool), torch.zeros(1, dtype=torch.int32))
