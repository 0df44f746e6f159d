"""VQGanAttention on feature maps of any size, the parts that need no GPU: the envelope the C-ABI entry points accept (argument checks
come before anything touches the device; N = 0 launches nothing), the new symbol, and ContinuousPositionBias.table -- the bias as a
function of the (dy, dx) offset -- against the [heads, P, P] bias of forward()."""
import ctypes
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from vae_wide_util import gather_table  # noqa: E402

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -2


@pytest.fixture(scope='module')
def L():
    from nuwa_pytorch_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize('dh,P', [(64, 324), (64, 400), (64, 1024), (64, 4096), (33, 361), (16, 1600)])
def test_vqattn_core_accepts_maps_past_the_lds_bound(L, dh, P):
    """2 dim_head P 4 B > 160 KiB: refused until the tiled kernel (18 x 18 was the first refused map at dim_head 64)"""
    p = ctypes.c_void_p(0x1000)
    assert L.amdnuwa_vqattn_core(p, p, p, p, 0, 8, dh, P, None) == OK


def test_vqattn_core_envelope_edges(L):
    p = ctypes.c_void_p(0x1000)
    for P in (1, 256, 289, 320, 400):
        assert L.amdnuwa_vqattn_core(p, p, p, p, 0, 8, 65, P, None) == ERR_UNSUPPORTED       # dim_head > 64
        assert L.amdnuwa_vqattn_core(p, p, p, p, 0, 8, 64, P, None) == OK
    assert L.amdnuwa_vqattn_core(p, p, p, p, 0, 8, 0, 400, None) == ERR_UNSUPPORTED
    assert L.amdnuwa_vqattn_core(p, p, p, p, 0, 8, 64, 0, None) == ERR_UNSUPPORTED
    for bad in range(4):
        args = [p, p, p, p]
        args[bad] = None
        assert L.amdnuwa_vqattn_core(*args, 0, 8, 64, 400, None) == ERR_ARG
        assert L.amdnuwa_vqattn_core_rel(*args, 0, 8, 64, 20, None) == ERR_ARG
    assert L.amdnuwa_vqattn_core(p, p, p, p, 0, 0, 64, 400, None) == ERR_ARG                  # heads
    for side in (1, 18, 20, 64):
        assert L.amdnuwa_vqattn_core_rel(p, p, p, p, 0, 8, 64, side, None) == OK
        assert L.amdnuwa_vqattn_core_rel(p, p, p, p, 0, 8, 1, side, None) == OK
        assert L.amdnuwa_vqattn_core_rel(p, p, p, p, 0, 8, 65, side, None) == ERR_UNSUPPORTED
    assert L.amdnuwa_vqattn_core_rel(p, p, p, p, 0, 8, 64, 65, None) == ERR_UNSUPPORTED      # the table form ends at the 3DNA envelope
    assert L.amdnuwa_vqattn_core_rel(p, p, p, p, 0, 8, 64, 0, None) == ERR_UNSUPPORTED


def test_new_symbol_is_declared_and_bound():
    import __graft_entry__ as G
    from nuwa_pytorch_amd import _lib
    assert 'amdnuwa_vqattn_core_rel' in G.declared_symbols()
    assert 'amdnuwa_vqattn_core_rel' in _lib.SIGNATURES
    assert _lib.SIGNATURES['amdnuwa_vqattn_core_rel'] == _lib.SIGNATURES['amdnuwa_vqattn_core']
    assert _lib.ABI_VERSION == 21                       # one added entry point, no version step


@pytest.mark.parametrize('side', [1, 2, 5, 20])
def test_position_bias_table_gathers_to_the_full_bias(side):
    from nuwa_pytorch_amd.vqgan_vae import ContinuousPositionBias
    torch.manual_seed(side)
    heads = 3
    m = ContinuousPositionBias(dim=16, heads=heads)
    P = side * side
    with torch.no_grad():
        m.net[-1].weight.mul_(4)
        full = m(torch.zeros(1, heads, P, P))[0]
        tab = m.table(side)
    assert tab.shape == (heads, 2 * side - 1, 2 * side - 1)
    got = gather_table(tab, side)
    assert got.shape == full.shape
    assert float(full.abs().max()) > 0.1
    assert float((got - full).abs().max()) <= 1e-6
