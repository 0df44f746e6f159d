"""Attention dropout on the linear-memory cattn kernels, the part that needs no GPU: the three C-ABI symbols, what the masked entry points
return before they launch anything (through ctypes, operand pointers never dereferenced), the fp64 restatement the GPU tests compare
against (tests/cattn_dropout_util.py) against the module's torch-op route and the oracle, the mask packing, and the routing predicates
off the GPU and with the opt-in off."""
import ctypes
import os
import re

import pytest
import torch

from attn_dropout_util import FixedMaskDropout
from cattn_dropout_util import attention_drop, fixed_keep, unpack_keep
from gpu_util import rel_err

OK, ARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('amdnuwa_cattn_drop_supported', 'amdnuwa_cattn_fwd_drop', 'amdnuwa_cattn_bwd_drop')

_PTRS = ctypes.create_string_buffer(64)
PTR = (ctypes.addressof(_PTRS) + 15) & ~15                        # a non-null, 16-byte aligned address that is never dereferenced


@pytest.fixture(scope='module')
def O():
    from oracle import nuwa_oracle
    return nuwa_oracle


def _L():
    from nuwa_pytorch_amd import _lib
    return _lib.lib()


def test_symbols_exported_declared_and_bound():
    from nuwa_pytorch_amd import _lib
    from nuwa_pytorch_amd.build import LIB
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'amdnuwa.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(amdnuwa_[a-z0-9_]+)\s*\(', src))
    so = ctypes.CDLL(LIB)
    for s in SYMBOLS:
        assert s in declared, f'{s} is not declared in include/amdnuwa.h'
        assert hasattr(so, s), f'libamdnuwa.so does not export {s}'
        assert s in _lib.SIGNATURES, f'{s} has no ctypes signature'
    # the masked entries take the arguments of the unmasked ones plus (keep, keep0, scale) / (keep, keep_t, keep0, scale), the stream last
    S = _lib.SIGNATURES
    P, F = ctypes.c_void_p, ctypes.c_float
    assert S['amdnuwa_cattn_fwd_drop'][1] == S['amdnuwa_cattn_fwd'][1][:-1] + [P, P, F, P]
    assert S['amdnuwa_cattn_bwd_drop'][1] == S['amdnuwa_cattn_bwd'][1][:-1] + [P, P, P, F, P]
    assert S['amdnuwa_cattn_drop_supported'] == S['amdnuwa_cattn_supported']
    assert _L().amdnuwa_abi_version() == 21


# ---- entry contract ------------------------------------------------------------------------------------------------------------------

FWD = 'q16 ldq k16 v16 ldkv key_mask null_k null_v w_th o o_lo ldo o_lo_f16 stats f16 keep keep0 drop_scale'
BWD = ('q ldq k v ldkv dO lddo key_mask null_k null_v w_th stats dq lddq dk dv lddkv dw_th dnull_k dnull_v workspace workspace_bytes '
       'keep keep_t keep0 drop_scale')


def cgeom(B=2, n=70, heads=8, dh=64, causal=0, n_keys=45):
    from nuwa_pytorch_amd import _lib
    g = _lib.CGeom()
    g.B, g.n, g.heads, g.dim_head, g.scale, g.causal, g.n_keys = B, n, heads, dh, dh ** -0.5, causal, n_keys
    return g


def call(L, entry, g, over):
    """one call of the masked entry on geometry g: operand pointers PTR, leading dimensions 1024, key_mask / o_lo NULL, exactly the workspace
    bytes the library reports (minus ws_short), masks PTR, drop_scale 1.25 -- and the overrides `over`"""
    over = dict(over)
    short = over.pop('ws_short', 0)
    args = []
    for name in (FWD if entry == 'amdnuwa_cattn_fwd_drop' else BWD).split():
        if name in over:
            v = over[name]
        elif name == 'workspace_bytes':
            v = L.amdnuwa_cattn_bwd_workspace_bytes(ctypes.byref(g)) - short
        elif name.startswith('ld'):
            v = 1024
        elif name == 'drop_scale':
            v = 1.25
        elif name in ('o_lo_f16', 'f16'):
            v = 0
        elif name in ('key_mask', 'o_lo'):
            v = None
        else:
            v = PTR
        args.append(v)
    return getattr(L, entry)(ctypes.byref(g), *args, None)


# (case, geometry keywords, overrides, expected); every case returns before a launch
CASES = [
    ('keep NULL', {}, {'keep': None}, ARG),
    ('keep0 NULL', {}, {'keep0': None}, ARG),
    ('keep_t NULL', {}, {'keep_t': None}, ARG),
    ('keep misaligned', {}, {'keep': PTR + 1}, ARG),
    ('keep misaligned by 2', {}, {'keep': PTR + 2}, ARG),
    ('keep0 misaligned', {}, {'keep0': PTR + 3}, ARG),
    ('keep_t misaligned', {}, {'keep_t': PTR + 1}, ARG),
    ('drop_scale 0.5', {}, {'drop_scale': 0.5}, ARG),
    ('drop_scale inf', {}, {'drop_scale': float('inf')}, ARG),
    ('drop_scale nan', {}, {'drop_scale': float('nan')}, ARG),
    ('9 heads', {'heads': 9}, {}, UNSUPPORTED),
    ('dim_head 48', {'dh': 48}, {}, UNSUPPORTED),
    ('causal with other keys', {'causal': 1}, {}, UNSUPPORTED),
    # the order of the unmasked entries: geometry, then arguments, then the workspace
    ('9 heads and keep NULL', {'heads': 9}, {'keep': None}, UNSUPPORTED),
    ('q NULL', {}, {'q': None, 'q16': None}, ARG),
    ('short workspace', {}, {'ws_short': 1}, WORKSPACE),
    ('short workspace, causal', {'causal': 1, 'n_keys': 0}, {'ws_short': 1}, WORKSPACE),
    ('keep NULL and short workspace', {}, {'keep': None, 'ws_short': 1}, ARG),
    ('workspace NULL', {}, {'workspace': None}, WORKSPACE),
]


@pytest.mark.parametrize('entry', ['amdnuwa_cattn_fwd_drop', 'amdnuwa_cattn_bwd_drop'])
def test_return_codes_before_any_launch(entry):
    L = _L()
    names = set((FWD if 'fwd' in entry else BWD).split()) | ({'ws_short'} if 'bwd' in entry else set())
    # a case applies to an entry point that has one of the parameters it overrides (a geometry case: to both)
    mine = [(c, gkw, {k: v for k, v in over.items() if k in names}, want) for c, gkw, over, want in CASES if not over or any(k in names for k in over)]
    rows = [(c, want) for c, _, _, want in mine]
    got = [(c, call(L, entry, cgeom(**gkw), over)) for c, gkw, over, _ in mine]
    assert got == rows
    assert len(rows) >= (14 if 'fwd' in entry else 19)


def test_drop_supported_equals_supported():
    L = _L()
    table = [dict(), dict(heads=1, dh=32), dict(heads=9), dict(heads=0), dict(dh=48), dict(dh=128), dict(causal=1), dict(causal=1, n_keys=0),
             dict(causal=1, n_keys=70), dict(B=0), dict(n=0), dict(n_keys=-1), dict(n=1, n_keys=100000), dict(B=1 << 20, n=1 << 12)]
    got = []
    for kw in table:
        g = cgeom(**kw)
        a, b = L.amdnuwa_cattn_supported(ctypes.byref(g)), L.amdnuwa_cattn_drop_supported(ctypes.byref(g))
        assert a == b, kw
        got.append(a)
    assert got == [1, 1, 0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 1, 0]
    assert L.amdnuwa_cattn_drop_supported(None) == 0


# ---- the restatement the GPU tests compare against ---------------------------------------------------------------------------------------

def _module(A, causal, heads=3, dh=32, dim=48, p=0.2):
    torch.manual_seed(2)
    return A.Attention(dim=dim, heads=heads, dim_head=dh, causal=causal, dropout=p).train()


@pytest.mark.parametrize('form', ['causal', 'context+mask', 'self+rotary'])
def test_restatement_equals_the_torch_route_and_the_oracle(O, form):
    """attention_drop in fp64 with a fixed mask == Attention._forward_torch (fp32) with FixedMaskDropout of that mask, to fp32 rounding; with
    keep = 1 and s = 1 it is O.attention"""
    import nuwa_pytorch_amd as A
    from nuwa_pytorch_amd.nuwa_pytorch import RotaryEmbedding
    B, n, T, p = 2, 37, 21, 0.2
    causal = form == 'causal'
    m = _module(A, causal, p=p)
    torch.manual_seed(5)
    x = torch.randn(B, n, 48)
    kw, okw = {}, {}
    if form == 'context+mask':
        c = torch.randn(B, T, 48)
        cm = torch.rand(B, T) > 0.3
        cm[1] = False
        kw, okw = dict(context=c, context_mask=cm), dict(context=c, context_mask=cm)
    else:
        T = n
        mk = torch.rand(B, n) > 0.2
        kw, okw = dict(mask=mk), dict(mask=mk)
        if form == 'self+rotary':
            rot = RotaryEmbedding(dim=16)(n, device='cpu')
            kw['rotary_pos_emb'], okw['rotary'] = rot, rot
    P = {k: v.detach() for k, v in m.state_dict().items()}
    keep = fixed_keep(B, m.heads, n, T, p)
    s = 1.0 / (1.0 - p)
    m.dropout = FixedMaskDropout(keep, s)
    with torch.no_grad():
        y = m._forward_torch(x, **kw)
    assert m.dropout.calls == 1
    d = lambda t: t.double() if t.is_floating_point() else t
    P64, okw64 = {k: d(v) for k, v in P.items()}, {k: d(v) for k, v in okw.items()}
    ref = attention_drop(x.double(), P64, m.heads, keep, s, O, causal=causal, **okw64)
    assert ref.dtype == torch.float64 and rel_err(y, ref) < 1e-5
    plain = O.attention(x, P, m.heads, causal=causal, **okw)
    assert rel_err(plain, ref) > 1e-2                                                       # (the mask matters)
    # keep = 1, s = 1: the oracle's attention -- the same operations in fp32, its rounding against fp64
    assert torch.equal(attention_drop(x, P, m.heads, torch.ones_like(keep), 1.0, O, causal=causal, **okw), plain)
    assert rel_err(plain, attention_drop(x.double(), P64, m.heads, torch.ones_like(keep), 1.0, O, causal=causal, **okw64)) < 1e-5


# ---- packing ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('B,heads,n,T', [(2, 3, 70, 45), (1, 8, 33, 64), (3, 1, 1, 1), (2, 5, 64, 100)])
def test_pack_round_trip_transpose_and_padding(B, heads, n, T):
    from nuwa_pytorch_amd import ops
    mask = fixed_keep(B, heads, n, T, 0.4, seed=B + heads + n)
    keep, keep_t, keep0 = ops.cattn_pack_keep(mask)
    KP, NP = -(-T // 32) * 32, -(-n // 32) * 32
    assert keep.shape == (B, n, KP) and keep_t.shape == (B, T, NP) and keep0.shape == (B, n)
    assert all(t.dtype == torch.uint8 and t.is_contiguous() for t in (keep, keep_t, keep0))
    assert torch.equal(unpack_keep(keep, keep0, heads, T), mask)
    assert torch.equal(keep_t[:, :, :n], keep[:, :, :T].transpose(1, 2))
    assert int(keep[:, :, T:].sum()) == 0 and int(keep_t[:, :, n:].sum()) == 0
    assert int(keep.max()) < (1 << heads) and int(keep0.max()) < (1 << heads)


def test_drawn_mask_is_chunked_and_reproducible(monkeypatch):
    """_cattn_keep_mask: the same seed gives the same arrays; the keep rate is 1 - p; a draw limit below one sample's values still walks the
    batch sample by sample and consumes the RNG stream in the same order"""
    from nuwa_pytorch_amd import ops
    B, n, T, heads, p = 5, 40, 33, 3, 0.25
    torch.manual_seed(11)
    a = ops._cattn_keep_mask(B, n, T, heads, p, 'cpu')
    torch.manual_seed(11)
    b = ops._cattn_keep_mask(B, n, T, heads, p, 'cpu')
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    mask = unpack_keep(a[0], a[2], heads, T)
    assert abs(float(mask.float().mean()) - (1 - p)) < 0.02
    assert torch.equal(a[1][:, :, :n], a[0][:, :, :T].transpose(1, 2))
    monkeypatch.setattr(ops, '_CATTN_DRAW_MAX', 1)
    torch.manual_seed(11)
    c = ops._cattn_keep_mask(B, n, T, heads, p, 'cpu')
    assert all(torch.equal(x, y) for x, y in zip(a, c))


# ---- routing ----------------------------------------------------------------------------------------------------------------------------

def test_routing_predicates_off_the_gpu_and_with_the_opt_in_off():
    import nuwa_pytorch_amd as A
    from nuwa_pytorch_amd.nuwa_pytorch import Attention, SandwichNorm
    assert Attention.dropout_on_kernels is False
    x = torch.randn(2, 9, 64)
    c = torch.randn(2, 5, 64)
    for causal in (False, True):
        m = Attention(dim=64, heads=2, dim_head=32, causal=causal, dropout=0.2).train()
        # the parent's predicates: live dropout keeps every kernel route shut, and the opt-in predicate is shut by default
        assert not m._hip_ok(5) and not m._causal_hip_ok(9) and not m._long_hip_ok(300) and not m._long_hip_ok(300, 9, 2)
        assert not m._drop_hip_ok(False) and not m._drop_hip_ok(True)
        sn = SandwichNorm(dim=64, fn=m).train()
        assert sn._inner(None, seq_len=9, batch=2) is None and sn._inner(c, seq_len=9, batch=2) is None
        m.eval()
        assert m._hip_ok(5) == (not causal) and m._causal_hip_ok(9) == causal and not m._drop_hip_ok(False)
        m.train()
    # with the opt-in on: the predicate answers in training with p > 0 only, never for causal attention with a context, only in the two modes
    m = Attention(dim=64, heads=2, dim_head=32, dropout=0.2).train()
    m.dropout_on_kernels = True
    assert m._drop_hip_ok(False) and m._drop_hip_ok(True)
    assert not m._hip_ok(5) and not m._long_hip_ok(300)                                    # (the unmasked predicates stay those of the parent)
    A.set_precision('bf16x3')
    try:
        assert not m._drop_hip_ok(False)
    finally:
        A.set_precision('bf16')
    A.set_precision('bf16x3-fwd')
    try:
        assert m._drop_hip_ok(True)
    finally:
        A.set_precision('bf16')
    m.eval()
    assert not m._drop_hip_ok(False)
    m.train()
    m.dropout.p = 0.0
    assert not m._drop_hip_ok(False)
    mc = Attention(dim=64, heads=2, dim_head=32, causal=True, dropout=0.2).train()
    mc.dropout_on_kernels = True
    assert mc._drop_hip_ok(False) and not mc._drop_hip_ok(True)
    for bad in (dict(heads=9, dim_head=32), dict(heads=2, dim_head=48)):
        mb = Attention(dim=64, dropout=0.2, **bad).train()
        mb.dropout_on_kernels = True
        assert not mb._drop_hip_ok(False)
    # off the GPU the module runs its torch ops whatever the attribute says
    torch.manual_seed(0)
    y1 = m.eval()(x, context=c)
    assert y1.shape == x.shape
    m.train()
    m.dropout.p = 0.2
    assert m(x, context=c).shape == x.shape
