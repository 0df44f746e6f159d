"""Single-query SparseCross2DNA over a window of any size (amdnuwa_cross2dna_decode, csrc/decode.hip; np.py:761-901) without a GPU: the
entry point and its workspace function are exported, declared and registered, their argument checks answer before anything is launched,
the ABI version is unchanged, the workspace follows the documented formula, and the slot table decode._Cross2DNARows hands the kernel
(decode.cross2dna_slot_rows) names the context rows SparseCross2DNA._forward_torch gathers, in its slot order."""
import ctypes
import os
import re

import pytest
import torch

from sketch_window_util import window_formula

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
SPLIT = 128


@pytest.fixture(scope='module')
def L():
    from nuwa_pytorch_amd import _lib
    return _lib.lib()


def _call(L, B=2, J=300, heads=8, dh=64, ptr=ctypes.c_void_p(16), ws=ctypes.c_void_p(16), ws_bytes=1 << 40, **over):
    """argument list of amdnuwa_cross2dna_decode with every pointer `ptr` (never dereferenced on the host); over: name -> value"""
    inner = heads * dh
    a = dict(B=B, J=J, heads=heads, dim_head=dh, scale=dh ** -0.5, q=ptr, q_lo=None, ldq=inner, kv=ptr, kv_lo=None, ctx_rows=192,
             slot_rows=ptr, n_pos=16, pos=ptr, key_mask=None, null_k=ptr, null_v=ptr, w_th=ptr, o=ptr, o_lo=None, ldo=inner, workspace=ws,
             workspace_bytes=ws_bytes, stream=None)
    assert not set(over) - set(a), over
    a.update(over)
    return L.amdnuwa_cross2dna_decode(*a.values())


def test_entry_points_are_exported_declared_and_registered(L):
    from nuwa_pytorch_amd import _lib
    from nuwa_pytorch_amd import kernels as K
    header = open(os.path.join(ROOT, 'include', 'amdnuwa.h')).read()
    for name in ('amdnuwa_cross2dna_decode', 'amdnuwa_cross2dna_decode_workspace_bytes'):
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES
        assert re.search(r'\b' + name + r'\s*\(', header), name
    assert callable(K.cross2dna_decode)
    assert L.amdnuwa_abi_version() == 21                      # purely additive


def test_argument_checks_answer_before_any_launch(L):
    assert _call(L, ptr=None) == ARG
    for name in ('q', 'kv', 'slot_rows', 'pos', 'null_k', 'null_v', 'w_th', 'o'):
        assert _call(L, **{name: None}) == ARG, name
    for name in ('B', 'J', 'n_pos', 'ctx_rows'):
        for v in (0, -3):
            assert _call(L, **{name: v}) == ARG, (name, v)
    lo = ctypes.c_void_p(32)
    for one_side in ('q_lo', 'kv_lo', 'o_lo'):                # the lo images come together or not at all
        assert _call(L, **{one_side: lo}) == ARG, one_side
    assert _call(L, q_lo=lo, o_lo=lo) == ARG and _call(L, kv_lo=lo, o_lo=lo) == ARG and _call(L, q_lo=lo, kv_lo=lo) == ARG
    assert _call(L, ldq=8) == ARG and _call(L, ldo=8) == ARG
    assert _call(L, heads=9) == UNSUPPORTED
    assert _call(L, dh=48) == UNSUPPORTED
    need = L.amdnuwa_cross2dna_decode_workspace_bytes(2, 300, 8, 64)
    assert _call(L, ws_bytes=need - 1) == WORKSPACE
    assert _call(L, ws=None) == WORKSPACE
    assert _call(L, ws_bytes=16) == WORKSPACE
    assert _call(L, q_lo=lo, kv_lo=lo, o_lo=lo, ws_bytes=16) == WORKSPACE      # all three lo images: past the argument checks
    # arguments first, the envelope second, the workspace last
    assert _call(L, heads=9, q=None) == ARG and _call(L, dh=48, n_pos=0) == ARG and _call(L, heads=9, dh=48, kv_lo=lo) == ARG
    assert _call(L, heads=9, ws=None, ws_bytes=0) == UNSUPPORTED


@pytest.mark.parametrize('heads,dh', [(8, 64), (3, 64), (1, 32), (5, 32)])
def test_workspace_follows_the_documented_formula(L, heads, dh):
    """4 * B * (heads * (J + 1) + splits * (2 * heads + heads * dim_head)) bytes, splits = ceil((J + 1) / 128): the sibling's formula
    (amdnuwa_attn_decode_rows) with T = J"""
    ws = lambda B, J: L.amdnuwa_cross2dna_decode_workspace_bytes(B, J, heads, dh)
    for B in (1, 3, 8):
        for J in (1, 9, 18, 125, 126, 127, 128, 255, 287, 288, 300, 1000):
            splits = -(-(J + 1) // SPLIT)
            assert ws(B, J) == 4 * B * (heads * (J + 1) + splits * (2 * heads + heads * dh)), (B, J)
            assert ws(B, J) == L.amdnuwa_attn_decode_rows_workspace_bytes(B, J, heads, dh)
    # one more slot past a split boundary opens one more split: one more statistics block and one more partial row per sample
    assert ws(1, 128) - ws(1, 127) == 4 * (heads + 2 * heads + heads * dh)
    assert ws(1, 127) - ws(1, 126) == 4 * heads
    assert ws(0, 10) == 0 and ws(2, 0) == 0


@pytest.mark.parametrize('kernel,dilation,frames', [(3, 2, 2), (5, 1, 12)])
def test_slot_table_names_the_rows_the_module_gathers(kernel, dilation, frames):
    """decode.cross2dna_slot_rows on a 4 x 4 map: random fp32 q / context / mask, the float64 gather formula evaluated THROUGH the table --
    null key, hidden slots (padding and masked rows), talking heads -- equals rows 1.. of SparseCross2DNA._forward_torch (the formulation
    tests/test_sketch_vs_reference.py pins to the reference) to 1e-5: slot order (frame, tap), padding and masking.  Padding entries stay
    -1, and NaN planted in every context row a position's table does not name never reaches that position's result."""
    from nuwa_pytorch_amd import decode
    from nuwa_pytorch_amd.nuwa_pytorch import SparseCross2DNA
    torch.manual_seed(3 + kernel)
    heads, dh, dim, fmap, B = 2, 32, 32, 4, 3
    tpf, T, n = fmap * fmap, frames * fmap * fmap, 1 + 24
    mod = SparseCross2DNA(dim=dim, image_size=fmap, heads=heads, dim_head=dh, kernel_size=kernel, dilation=dilation).eval()
    tab = decode.cross2dna_slot_rows(mod._nbr, frames)
    assert tab.dtype == torch.int32 and tuple(tab.shape) == (tpf, frames * kernel * kernel) and tab.is_contiguous()
    assert int(tab.min()) == -1 and int(tab.max()) < T
    # the same content as the (clamped index, validity) pair the packed path gathers with
    nbr = mod._nbr
    assert torch.equal(tab >= 0, (nbr >= 0).repeat(1, frames))
    assert torch.equal(tab.clamp(min=0).long(), torch.cat([torch.where(nbr >= 0, nbr + a * tpf, torch.zeros_like(nbr)) for a in range(frames)], 1))
    x, ctx = torch.randn(B, n, dim), torch.randn(B, T, dim)
    mask = torch.rand(B, T) > 0.3
    mask[1] = False                                            # a sample that sees the null key alone
    with torch.no_grad():
        ref = mod._forward_torch(x, context=ctx, context_mask=mask)[:, 1:]
        q = mod.to_q(x).double()
        kv = mod.to_kv(ctx).double()
        nk, nv = mod.null_k.double().reshape(heads, dh), mod.null_v.double().reshape(heads, dh)
        wth = mod.talking_heads.weight.double().reshape(heads, heads)
        rows = []
        for pos in range(1, n):
            i = (pos - 1) % tpf
            unnamed = torch.ones(T, dtype=torch.bool)
            unnamed[tab[i][tab[i] >= 0].long()] = False
            kv_p = kv.clone()
            kv_p[:, unnamed] = float('nan')
            rows.append(window_formula(q[:, pos], kv_p, tab[i], nk, nv, wth, mask, mod.scale))
        got = mod.to_out(torch.stack(rows, 1).float())
    assert bool(torch.isfinite(got).all())
    err = float((got - ref).abs().max() / ref.abs().max())
    assert err <= 1e-5, err
