"""The dropout mask generator without a GPU: the numpy restatement of its decision function (tests/keep_mask_util.py) against the known
answers of Philox4x32-10 and its keep rate, the two C entry points (exported, declared, argument checks in front of any launch), the
package switch, and ops._cattn_keep_mask's use of the kernel wrapper."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import keep_mask_util as KM  # noqa: E402


def test_restatement_reproduces_the_known_answers():
    for counter, key, want in KM.KNOWN_ANSWERS:
        got = tuple(int(w) for w in KM.philox4x32_10(counter, key))
        assert got == want, ([hex(w) for w in got], [hex(w) for w in want])


def test_element_words_walk_the_counter():
    """element e reads word e mod 4 of group e // 4; the group's high half is counter word 1"""
    seed = (0xa4093822, 0x299f31d0)
    for grp in (0, 5, (1 << 32) - 1, 1 << 32, (7 << 32) + 3):
        want = KM.philox4x32_10((grp & 0xFFFFFFFF, grp >> 32, 0, 0), seed)
        got = KM.element_words(np.arange(4 * grp, 4 * grp + 4, dtype=np.uint64), seed)
        assert [int(w) for w in got] == [int(w) for w in want]


@pytest.mark.parametrize('p', [0.05, 0.25, 0.5])
def test_keep_rate_of_the_restatement(p):
    """seed (12345, 678), elements 0 .. 2^20 - 1: the keep rate within 5 sigma of 1 - thr / 2^32 (the issue's own run: 1.5 / 1.3 / 1.9)"""
    N = 1 << 20
    thr = KM.keep_threshold(p)
    q = 1.0 - thr / 4294967296.0
    rate = float(KM.keep_of(np.arange(N, dtype=np.uint64), thr, (12345, 678)).mean())
    sigma = math.sqrt(q * (1.0 - q) / N)
    print(f'p={p}: rate {rate:.6f}, expected {q:.6f}, {abs(rate - q) / sigma:.2f} sigma')
    assert abs(rate - q) <= 5.0 * sigma


def test_threshold():
    from nuwa_pytorch_amd import kernels as K
    for p, want in ((0.0, 0), (0.5, 1 << 31), (0.25, 1 << 30), (1.0 - 2.0 ** -40, 0xFFFFFFFF)):
        assert K.keep_threshold(p) == KM.keep_threshold(p) == want
    assert K.keep_threshold(0.05) == KM.keep_threshold(0.05) == int(math.floor(0.05 * 2.0 ** 32 + 0.5))


def test_both_symbols_are_exported_and_declared():
    import __graft_entry__ as G
    from nuwa_pytorch_amd import build as B, _lib
    so = ctypes.CDLL(B.build(verbose=False))
    for name in ('amdnuwa_keep_mask_linear', 'amdnuwa_keep_mask_cattn'):
        assert hasattr(so, name), name
        assert name in _lib.SIGNATURES and name in G.declared_symbols(), name


def test_argument_validation_without_gpu():
    """every refusal comes before the device is touched: the pointers below are never read"""
    from nuwa_pytorch_amd import _lib
    L = _lib.lib()
    ERR = -1                                     # AMDNUWA_ERR_ARG
    a, t, z, s = 0x10000, 0x20000, 0x30000, 0x40000
    lin, cat = L.amdnuwa_keep_mask_linear, L.amdnuwa_keep_mask_cattn
    assert lin(None, 16, 0, 1 << 30, s, None) == ERR
    assert lin(a, 16, 0, 1 << 30, None, None) == ERR
    assert lin(a, 0, 0, 1 << 30, s, None) == ERR and lin(a, -3, 0, 1 << 30, s, None) == ERR
    assert lin(a, 16, -1, 1 << 30, s, None) == ERR
    for args in ((None, t, z), (a, None, z), (a, t, None)):
        assert cat(*args, 2, 37, 45, 8, 0, 1 << 30, s, None) == ERR
    assert cat(a, t, z, 2, 37, 45, 8, 0, 1 << 30, None, None) == ERR
    for heads in (0, 9, -1):
        assert cat(a, t, z, 2, 37, 45, heads, 0, 1 << 30, s, None) == ERR
    for B, n, T in ((0, 37, 45), (2, 0, 45), (2, 37, 0), (-1, 37, 45)):
        assert cat(a, t, z, B, n, T, 8, 0, 1 << 30, s, None) == ERR
    for off in (1, 2, 3):
        assert cat(a + off, t, z, 2, 37, 45, 8, 0, 1 << 30, s, None) == ERR
        assert cat(a, t + off, z, 2, 37, 45, 8, 0, 1 << 30, s, None) == ERR
    assert cat(a, t, z, 2, 37, 45, 8, -1, 1 << 30, s, None) == ERR


def test_switch_defaults_to_torch_and_rejects_unknown_names():
    from nuwa_pytorch_amd import ops
    assert ops.KEEP_MASK_SOURCES == ('torch', 'device')
    assert ops.get_keep_mask_source() == os.environ.get('AMDNUWA_KEEP_MASK_SOURCE', 'torch') == 'torch'
    for name in ('philox', 'Device', '', None, True):
        with pytest.raises(ValueError):
            ops.set_keep_mask_source(name)
    assert ops.get_keep_mask_source() == 'torch'
    try:
        ops.set_keep_mask_source('device')
        assert ops.get_keep_mask_source() == 'device'
    finally:
        ops.set_keep_mask_source('torch')


@pytest.mark.parametrize('B,heads,n,T,p', [(2, 3, 37, 45, 0.25), (1, 8, 5, 1, 0.5)])
def test_cattn_producer_under_device_is_pack_keep_of_the_restated_mask(monkeypatch, B, heads, n, T, p):
    """the kernel wrapper replaced by the restatement: ops._cattn_keep_mask hands it the shape, ONE threshold and two seed words from torch's
    generator, and returns its three arrays -- equal to ops.cattn_pack_keep of the restated boolean mask"""
    from nuwa_pytorch_amd import kernels as K, ops
    calls = []

    def fake(B_, n_, T_, heads_, thr, seed, b_first=0, out=None):
        assert seed.dtype == torch.int64 and seed.numel() == 2
        calls.append((B_, n_, T_, heads_, thr, tuple(int(v) & 0xFFFFFFFF for v in seed.tolist()), b_first))
        return ops.cattn_pack_keep(torch.from_numpy(KM.cattn_keep(B_, n_, T_, heads_, thr, calls[-1][5], b_first)))
    monkeypatch.setattr(K, 'keep_mask_cattn', fake)
    ops.set_keep_mask_source('device')
    try:
        torch.manual_seed(5)
        got = ops._cattn_keep_mask(B, n, T, heads, p, torch.device('cpu'))
        torch.manual_seed(5)
        again = ops._cattn_keep_mask(B, n, T, heads, p, torch.device('cpu'))
        torch.manual_seed(6)
        other = ops._cattn_keep_mask(B, n, T, heads, p, torch.device('cpu'))
    finally:
        ops.set_keep_mask_source('torch')
    assert len(calls) == 3 and calls[0] == calls[1] and calls[2][5] != calls[0][5]
    assert calls[0][:5] == (B, n, T, heads, KM.keep_threshold(p)) and calls[0][6] == 0
    want = ops.cattn_pack_keep(torch.from_numpy(KM.cattn_keep(B, n, T, heads, KM.keep_threshold(p), calls[0][5])))
    assert [tuple(t.shape) for t in got] == [(B, n, -(-T // 32) * 32), (B, T, -(-n // 32) * 32), (B, n)]
    for g, a, w in zip(got, again, want):
        assert g.dtype == torch.uint8 and torch.equal(g, w) and torch.equal(a, w)
    assert not torch.equal(other[0], got[0])
    assert int(got[0].max()) < (1 << heads)
