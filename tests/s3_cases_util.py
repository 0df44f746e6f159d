"""The value-test cases of the Sparse3DNA / SparseCross2DNA window kernels (plain helper, like gemm_exact_util.py; no GPU import at module
level).  One list, all_cases(), read by tests/test_gpu_s3_every_kernel.py (values on the GPU, through the kernels.py wrappers),
tests/test_s3_cases_cpu.py and tools/launch_log/cases_s3_values.py (which kernels each case launches, through the launch log of
sparse3dna.hip + sparse3dna_wide.hip with fake operand addresses).

Both sides make the same calls: call_shape(c, entry, workspace bytes) is the argument list of one C entry point for a case -- the geometry
block, every integer and float argument, and which pointer arguments are given.  call_fake() fills the pointers with fixed fake addresses;
the GPU test's recording proxy (Recorder) reduces what the wrapper really passed to the same form and the test compares the two.

References are the float64 restatements the suite already has: attn_dropout_util.sparse3dna_core_drop over oracle.neighbor_table and
xc2_dropout_util.cross2dna_core_drop64 over peaked_util.cross2dna_window.  Inputs are flat (torch.randn), rounded to the values the operand
form holds: a peaked softmax row hides a wrong window slot (test_s3_cases_cpu.py::test_inputs_are_not_vacuous measures that these do not)."""
import ctypes as C

import torch

import test_s3_entry_contract_cpu as T
import xc2_dropout_util as XU
from attn_dropout_util import keep_to_bhij, sparse3dna_core_drop

CASE_KEYS = ('name', 'group', 'entries', 'grid', 'window', 'dilation', 'heads', 'dim_head', 'ntok', 'B', 'causal', 'form', 'bias', 'cross',
             'keep', 'keys')
FORMS = ('bf16', 'hilo', 'f16fwd', 'f16grad')           # operand form: bf16, hi + lo pairs, fp16 forward, fp16-gradient backward
S_DROP = 1.0 / 0.75
PARAMS = {**T.PARAMS, **XU.drop_params(T)}              # parameter names of the twelve entries, in declaration order
LO_NAMES = {'q_lo', 'k_lo', 'v_lo', 'o_lo', 'dO_lo', 'dq_lo', 'dk_lo', 'dv_lo', 'null_k_lo', 'null_v_lo'}
INT_NAMES = {'ld', 'ldo', 'lddo', 'ldd', 'ldq', 'ldkv', 'lddq', 'lddkv', 'ctx_rows', 'accumulate', 'o_lo_f16', 'workspace_bytes'}
GEOM_FIELDS = ('B', 'ntok', 'F', 'H', 'W', 'kf', 'kh', 'kw', 'df', 'dh', 'dw', 'heads', 'dim_head', 'noncausal')


# ---------------------------------------------------------------------------------------------------
# the list
# ---------------------------------------------------------------------------------------------------
def _entries(form, masked, cross):
    d = '_drop' if masked else ''
    if cross:
        return ('amdnuwa_cross2dna_fwd' + d, 'amdnuwa_cross2dna_bwd' + d)
    if form == 'f16fwd':
        return ('amdnuwa_sparse3dna_fwd_f16' + d,)
    if form == 'f16grad':
        return ('amdnuwa_sparse3dna_bwd_f16' + d,)
    return ('amdnuwa_sparse3dna_fwd' + d, 'amdnuwa_sparse3dna_bwd' + d)


def _case(group, grid, window, dilation, heads, dim_head, ntok, B, form, masked, bias=False, keys=None, causal=True, cross=None):
    keys = dict(keys or {})
    name = (f'{group} {form} dh{dim_head}' + (' bias' if bias else '') + (' masked' if masked else '') +
            ''.join(f' k{k}={v}' for k, v in sorted(keys.items())))
    return dict(name=name, group=group, entries=_entries(form, masked, cross), grid=tuple(grid), window=tuple(window), dilation=tuple(dilation),
                heads=heads, dim_head=dim_head, ntok=ntok, B=B, causal=causal, form=form, bias=bias, cross=cross,
                keep=S_DROP if masked else None, keys=keys)


# band geometry (W = 16, 8 heads x 64, causal): group -> (grid, window, dilation, ntok, B, tuning keys)
BAND = {
    'band.odd': ((2, 3, 16), (3, 3, 3), (1, 1, 1), 1 + 48 + 21, 1, {}),          # odd H: the one-row kernel; the last frame is partial
    'band.t2': ((2, 2, 16), (3, 3, 3), (1, 1, 1), 1 + 32 + 8, 2, {}),            # two-row tiles, the last tile's second row absent
    'band.t4_1': ((2, 4, 16), (3, 3, 3), (1, 1, 1), 1 + 64 + 40, 2, {16: 4}),    # four-row tiles: the last row of the last tile absent,
    'band.t4_2': ((2, 4, 16), (3, 3, 3), (1, 1, 1), 1 + 64 + 24, 2, {16: 4}),    # ... the last two,
    'band.t4_3': ((2, 4, 16), (3, 3, 3), (1, 1, 1), 1 + 64 + 9, 2, {16: 4}),     # ... the last three
    'band.kw2@4': ((2, 4, 16), (2, 2, 2), (2, 1, 3), 1 + 128, 2, {16: 4}),       # kw = 2, another dilation on every axis
    'band.kw2@2': ((2, 4, 16), (2, 2, 2), (2, 1, 3), 1 + 128, 3, {}),
    'band.kw2@1': ((2, 4, 16), (2, 2, 2), (2, 1, 3), 1 + 128, 2, {16: 1}),
    'band.dil@4': ((1, 8, 16), (3, 3, 3), (1, 2, 2), 1 + 80 + 3, 2, {16: 4}),    # row dilation 2: a tile is every other row
    'band.dil@2': ((1, 8, 16), (3, 3, 3), (1, 2, 2), 1 + 80 + 3, 2, {}),
}
# the route keys of s3_route() at one band geometry in the bf16 form, each with and without a mask
ROUTE_GEOM = ((2, 2, 16), (3, 3, 3), (1, 1, 1), 1 + 64 - 5, 2)
ROUTE_KEYS = [{}, {3: 1}, {3: 2}, {4: 1}, {4: 2}, {4: 4}, {19: 1}, {24: 1}, {26: 1}, {4: 1, 19: 1}, {4: 2, 19: 1}, {4: 4, 19: 1}, {4: 4, 24: 1}]


def route_group(keys):
    return 'route.' + ('default' if not keys else ','.join(f'{k}={v}' for k, v in sorted(keys.items())))


def all_cases():
    out = []
    # ---- VALU row kernels: W * heads * 4 = 40 threads of work in a 64-thread workgroup
    for dh in (32, 64):
        for form in ('bf16', 'hilo'):
            small = dh == 64 and form == 'bf16'
            for masked in (False, True):
                kw = dict(heads=2, dim_head=dh, form=form, masked=masked)
                out.append(_case('valu.edge', (2, 3, 5), (3, 3, 3), (1, 1, 1), ntok=1 + 15 + 7, B=2, bias=dh == 32, **kw))
                out.append(_case('valu.dil', (2, 3, 5), (1, 3, 3), (1, 3, 2), ntok=31, B=1 if small else 2, **kw))
                out.append(_case('valu.ntok2', (2, 3, 5), (3, 3, 3), (1, 1, 1), ntok=2, B=3, **kw))
                if not masked:
                    out.append(_case('valu.noncausal', (2, 3, 5), (3, 3, 3), (1, 1, 2), ntok=31, B=2, causal=False, **kw))
                # SparseCross2DNA: 5 x 5 map, two sketch frames, the second query frame partial, sample 1's context fully hidden
                out.append(_case('valu.cross', (2, 5, 5), (2, 3, 3), (1, 1, 1), ntok=1 + 25 + 9, B=2, causal=False,
                                 cross=dict(frames=2, key_mask='sample1'), **kw))
    # ---- column-tiled kernels (8 heads: tiles of at most 16 columns)
    for dh in (32, 64):
        for form in ('bf16', 'hilo'):
            for masked in (False, True):
                kw = dict(heads=8, dim_head=dh, form=form, masked=masked)
                out.append(_case('wide.two', (2, 2, 20), (2, 3, 3), (1, 1, 2), ntok=1 + 40 + 20 + 7, B=2, **kw))
                out.append(_case('wide.three', (1, 2, 40), (1, 3, 3), (1, 1, 1), ntok=81, B=3 if masked else 1, **kw))
    # ---- MFMA band kernels
    for group, (grid, window, dil, ntok, B, keys) in BAND.items():
        for masked in (False, True):
            for bias in (False, True):
                out.append(_case(group, grid, window, dil, 8, 64, ntok, B, 'bf16', masked, bias=bias, keys=keys))
                out.append(_case(group, grid, window, dil, 8, 64, ntok, B, 'f16fwd', masked, bias=bias, keys=keys))
            out.append(_case(group, grid, window, dil, 8, 64, ntok, B, 'f16grad', masked, keys=keys))
    # ---- routes
    grid, window, dil, ntok, B = ROUTE_GEOM
    for keys in ROUTE_KEYS:
        for masked in (False, True):
            out.append(_case(route_group(keys), grid, window, dil, 8, 64, ntok, B, 'bf16', masked, keys=keys))
    for masked in (False, True):                          # hi + lo pairs at band geometry: the VALU kernels at 512 threads
        out.append(_case('route.hilo', grid, window, dil, 8, 64, ntok, B, 'hilo', masked))
        out.append(_case('route.bias24', grid, window, dil, 8, 64, ntok, B, 'bf16', masked, bias=True, keys={24: 1}))
    names = [c['name'] for c in out]
    assert len(set(names)) == len(names)
    return out


def mask_keeps_route(c):
    """does a masked call of this case run the masked forms of the kernels its unmasked call runs?  Not under tuning key 4 = 4 (the
    recomputing key side knows no mask: s3_route() gives a masked call the packed key side) nor under key 26 = 1 (a masked call alone moves
    to the VALU kernels).  tests/test_s3_cases_cpu.py checks this against the launch log."""
    return not (c['keys'].get(4) == 4 or c['keys'].get(26) == 1)


def slots(c):
    return c['window'][0] * c['window'][1] * c['window'][2] + 1


def ctx_rows(c):
    return c['window'][0] * c['grid'][1] * c['grid'][2]


def tile(c):
    """(queries per column tile, column tiles) as s3_tile() of s3_args.h has them"""
    W, heads = c['grid'][2], c['heads']
    if W * heads * 4 <= 512:
        return W, 1
    twmax = 128 // heads
    nt = -(-W // twmax)
    return -(-W // nt), nt


def is_band_geom(c):
    return c['causal'] and not c['cross'] and c['grid'][2] == 16 and c['heads'] == 8 and c['dim_head'] == 64 and c['window'][2] <= 3


# ---------------------------------------------------------------------------------------------------
# case -> calls
# ---------------------------------------------------------------------------------------------------
def geom_of(c, entry, rel_bias=None, d_rel_bias=None):
    from nuwa_pytorch_amd import _lib
    g = _lib.S3Geom()
    g.B, g.ntok = c['B'], c['ntok']
    g.F, g.H, g.W = c['grid']
    g.kf, g.kh, g.kw = c['window']
    g.df, g.dh, g.dw = c['dilation']
    g.heads, g.dim_head, g.scale = c['heads'], c['dim_head'], c['dim_head'] ** -0.5
    g.noncausal = 0 if c['causal'] else 1
    g.rel_bias = rel_bias if c['bias'] else None
    g.d_rel_bias = d_rel_bias if c['bias'] and '_bwd' in entry else None
    return g


def geom_shape(g):
    return tuple(int(getattr(g, f)) for f in GEOM_FIELDS) + (bool(g.rel_bias), bool(g.d_rel_bias))


def call_shape(c, entry, workspace_bytes):
    """the call of `entry` for case c: (geometry fields, [(parameter, value)]) -- pointers as True / False (given or NULL), integers and
    floats as they are.  The stream argument is left out."""
    inner = c['heads'] * c['dim_head']
    hilo, cross = c['form'] == 'hilo', bool(c['cross'])
    ints = dict(ld=3 * inner, ldo=inner, lddo=inner, ldd=3 * inner, ldq=inner, ldkv=2 * inner, lddq=inner, lddkv=2 * inner,
                ctx_rows=ctx_rows(c), accumulate=0, o_lo_f16=0, workspace_bytes=workspace_bytes)
    if cross:
        ints['ld'] = inner
    args = []
    for name in PARAMS[entry].split():
        if name in INT_NAMES:
            v = ints[name]
        elif name == 'drop_scale':
            v = float(c['keep'])
        elif name == 'key_mask':
            v = c['cross']['key_mask'] != 'none'
        elif name in LO_NAMES:
            v = hilo or (name == 'o_lo' and c['form'] == 'f16fwd')            # the fp16 forward writes a hi + lo output
        else:
            v = True
        args.append((name, v))
    g = geom_of(c, entry, 1, 1)
    return geom_shape(g), args


def declare(L):
    from nuwa_pytorch_amd import _lib
    for n, (res, argtypes) in _lib.SIGNATURES.items():
        if ('sparse3dna' in n or 'cross2dna' in n or n.startswith('amdnuwa_s3_')) and 'decode' not in n and hasattr(L, n):
            fn = getattr(L, n)
            fn.restype, fn.argtypes = res, argtypes


def workspace_bytes(L, c, entry):
    if '_bwd' not in entry:
        return 0
    fn = L.amdnuwa_cross2dna_bwd_workspace_bytes if c['cross'] else L.amdnuwa_sparse3dna_bwd_workspace_bytes
    return int(fn(C.byref(geom_of(c, entry, 1, 1))))


FAKE_BASE = 0x10000000


def call_fake(L, c, entry):
    """call_shape() with fixed fake operand addresses (distinct, 16-byte aligned, never dereferenced) -> the return code"""
    _, args = call_shape(c, entry, workspace_bytes(L, c, entry))
    vals = [(FAKE_BASE + 0x01000000 * (i + 1) if v else None) if isinstance(v, bool) else v for i, (_, v) in enumerate(args)]
    g = geom_of(c, entry, FAKE_BASE + 0x40000000, FAKE_BASE + 0x41000000)
    return getattr(L, entry)(C.byref(g), *vals, None)


class Recorder:
    """stands in for the loaded library: passes every attribute through and records the calls of the twelve window entry points in the form
    of call_shape()"""

    def __init__(self, real):
        from nuwa_pytorch_amd import _lib
        self._real, self._sig, self.calls = real, _lib.SIGNATURES, []

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name not in PARAMS:
            return fn

        def rec(gref, *args):
            names = PARAMS[name].split()
            assert len(args) == len(names) + 1, name
            shape = []
            for nm, typ, v in zip(names, self._sig[name][1][1:], args):
                if typ is C.c_void_p:
                    v = bool(v.value if isinstance(v, C.c_void_p) else v)
                elif typ is C.c_float:
                    v = float(v)
                else:
                    v = int(v)
                shape.append((nm, v))
            self.calls.append((name, geom_shape(gref._obj), shape))
            return fn(gref, *args)
        return rec


# ---------------------------------------------------------------------------------------------------
# operands, keep masks, float64 references
# ---------------------------------------------------------------------------------------------------
def _seed(c, salt=0):
    key = (c['grid'], c['window'], c['dilation'], c['heads'], c['dim_head'], c['ntok'], c['B'], c['causal'], salt)
    return sum((i + 1) * b for i, b in enumerate(repr(key).encode())) % (2 ** 31)


def held(t, form):
    """the values the operands of `form` hold of t: bf16-rounded (the fp16 forms: and exact in fp16), or what a hi + lo pair carries"""
    hi = t.to(torch.bfloat16).float()
    if form == 'hilo':
        return hi + (t - hi).to(torch.bfloat16).float()
    hi[hi.abs() < 2 ** -10] = 0
    return hi


def special_rows(c):
    """(sample, query) of: the fully dropped query; the one that keeps only slot 0 (head 1); the one with slot 0 alone dropped; and, where
    the sequence ends inside a frame (so inside a multi-row tile, where there is one), a further fully dropped query in the last present
    row -- the last query of sample 0.  Short sequences spread the three over three samples."""
    nq, B = c['ntok'] - 1, c['B']
    s1 = min(1, B - 1)
    if nq >= 6:
        rows = [(0, nq // 3), (s1, 2 * nq // 3), (s1, nq // 2)]
    else:
        assert B >= 3, c['name']
        rows = [(0, 0), (1, 0), (2, 0)]
    tail = None
    if nq % (c['grid'][1] * c['grid'][2]) and nq >= 6:
        tail = (0, nq - 1)
        assert tail not in rows
    return rows, tail


def keep_mask(c, ones=False):
    """kernel-order keep mask [B, nq, J, heads] of a case: Bernoulli(0.75) from a fixed generator, then the special rows"""
    nq, J, h = c['ntok'] - 1, slots(c), c['heads']
    if ones:
        return torch.ones(c['B'], nq, J, h, dtype=torch.bool)
    keep = torch.rand(c['B'], nq, J, h, generator=torch.Generator().manual_seed(_seed(c, 1))) < 0.75
    (r0, r1, r2), tail = special_rows(c)
    keep[r0[0], r0[1]] = False
    keep[r1[0], r1[1], :, 1] = False
    keep[r1[0], r1[1], 0, 1] = True
    keep[r2[0], r2[1]] = True
    keep[r2[0], r2[1], 0] = False
    if tail:
        keep[tail[0], tail[1]] = False
    return keep


def rest_fraction(c, keep):
    """the kept fraction of the mask outside the special rows"""
    (r0, r1, r2), tail = special_rows(c)
    rest = torch.ones_like(keep)
    for r in (r0, r2) + ((tail,) if tail else ()):
        rest[r[0], r[1]] = False
    rest[r1[0], r1[1], :, 1] = False
    return float(keep[rest].double().mean()), int(rest.sum())


def value_form(c):
    return 'hilo' if c['form'] == 'hilo' else 'bf16'


def table(c):
    """the neighbour table of a Sparse3DNA case (N, K), -1 = padding"""
    from oracle import nuwa_oracle as O
    return O.neighbor_table(c['grid'], c['window'], c['dilation'], causal=c['causal'])


def cross_window(c):
    import peaked_util as PU
    assert c['grid'][1] == c['grid'][2] and c['window'][1] == c['window'][2] and c['dilation'][1] == c['dilation'][2]
    return PU.cross2dna_window(c['grid'][1], c['window'][1], c['dilation'][1], c['window'][0], c['ntok'])


def inputs(c):
    g = torch.Generator().manual_seed(_seed(c))
    B, n, h, d, f = c['B'], c['ntok'], c['heads'], c['dim_head'], value_form(c)
    rn = lambda *s: held(torch.randn(*s, generator=g), f)
    I = dict(wth=torch.randn(h, h, generator=g) * 0.5 + torch.eye(h))
    if c['cross']:
        Tk = ctx_rows(c)
        I.update(q=rn(B, n, h, d), do=rn(B, n, h, d), k=rn(B, Tk, h, d), v=rn(B, Tk, h, d), nk=rn(h, d), nv=rn(h, d), kmask=None)
        if c['cross']['key_mask'] == 'sample1':
            I['kmask'] = torch.ones(B, Tk, dtype=torch.bool)
            I['kmask'][1] = False
        elif c['cross']['key_mask'] == 'rand':
            I['kmask'] = torch.rand(B, Tk, generator=g) > 0.3
    else:
        I.update(qkv=rn(B, n, 3, h, d), do=rn(B, n, h, d), rel=torch.randn(h, slots(c) - 1, generator=g) * 0.7 if c['bias'] else None)
    return I


def forward64(c, I, keep, s, idx=None):
    """the float64 restatement on the inputs I -> (output, leaves by name); idx replaces the window table (the vacuity check)"""
    leaf = lambda t: t.double().requires_grad_(True)
    if c['cross']:
        ix, valid = cross_window(c)
        ix = ix if idx is None else idx
        L = {k: leaf(I[k]) for k in ('q', 'k', 'v', 'nk', 'nv', 'wth')}
        o = XU.cross2dna_core_drop64(L['q'], L['k'], L['v'], L['nk'], L['nv'], L['wth'], I['kmask'], ix, valid, c['dim_head'] ** -0.5,
                                     keep_to_bhij(keep).double(), s)
        return o, L
    L = dict(qkv=leaf(I['qkv']), wth=leaf(I['wth']))
    if I['rel'] is not None:
        L['rel'] = leaf(I['rel'])
    o = sparse3dna_core_drop(L['qkv'][:, :, 0], L['qkv'][:, :, 1], L['qkv'][:, :, 2], L['wth'], table(c) if idx is None else idx,
                             c['dim_head'] ** -0.5, keep_to_bhij(keep).double(), s, rel_pos_bias=L.get('rel'))
    return o, L


_REF = {}


def reference(c, masked=None):
    """inputs and float64 results of a case, computed once per (data, mask) and read-only: shared by the cases that differ only in the
    kernels they take (tuning keys, and the three forms that read bf16-rounded values).  R['o'] keeps its graph for the fp16-gradient
    reference (grads64)."""
    masked = (c['keep'] is not None) if masked is None else masked
    key = (_seed(c), value_form(c), c['bias'], repr(c['cross']), masked)
    if key not in _REF:
        I = inputs(c)
        keep = keep_mask(c, ones=not masked)
        o, L = forward64(c, I, keep, c['keep'] if masked and c['keep'] else (S_DROP if masked else 1.0))
        do = I['do'][:, 1:] if c['cross'] else I['do']
        names = list(L)
        gr = torch.autograd.grad(o, [L[k] for k in names], do.double(), retain_graph=True)
        _REF[key] = dict(I=I, keep=keep, o=o, L=L, grads=dict(zip(names, gr)))
    return _REF[key]


def grads64(R, do):
    """gradients of the stored float64 graph for another dO (the fp16-gradient backward reads fp16(S dO) / S)"""
    names = list(R['L'])
    return dict(zip(names, torch.autograd.grad(R['o'], [R['L'][k] for k in names], do.double(), retain_graph=True)))


# ---------------------------------------------------------------------------------------------------
# tolerances (gpu_util.report: max-abs error over max-abs reference), those the suite already applies to each form
# ---------------------------------------------------------------------------------------------------
def tolerances(c):
    if c['cross']:                                       # test_gpu_xc2_dropout.py
        o, g = (1e-3, 2e-3) if c['form'] == 'hilo' else (2e-2, 7e-2)
        return dict(o=o, dq=g, dk=g, dv=g, dnk=g, dnv=g, dwth=g)
    if c['form'] in ('hilo', 'bf16'):                    # test_gpu_attn_dropout.py / test_gpu_wide_grid.py; d(rel_bias): the gradient tolerance
        t = dict(o=3e-5, dq=5e-5, dk=5e-5, dv=5e-5, dwth=5e-5, drel=5e-5) if c['form'] == 'hilo' else \
            dict(o=2 ** -7, dq=2 ** -6, dk=2 ** -6, dv=2 ** -6, dwth=1e-4, drel=2 ** -6)
        if not c['bias']:
            del t['drel']
        return t
    if c['form'] == 'f16fwd':                            # test_sparse3dna_fwd_f16_core
        return dict(o=6e-4)
    from test_gpu_attention_bwd16 import TOL_S3
    return dict(TOL_S3)


# ---------------------------------------------------------------------------------------------------
# the GPU side: one run of a case through the kernels.py wrappers, operands in guarded buffers, inside guard(K)
# ---------------------------------------------------------------------------------------------------
DEV = 'cuda'


def _pair(K, t, hilo):
    from guard_util import guarded
    hi = t.to(torch.bfloat16)
    lo = (t - hi.float()).to(torch.bfloat16) if hilo else None
    return K.BF(guarded(hi.contiguous(), device=DEV), guarded(lo.contiguous(), device=DEV) if hilo else None)


def grad_scale(c, R):
    """S of the production rule for this dO (ops._grad_scale), as tests/test_gpu_attention_bwd16.py takes it; once per reference"""
    if 'S16' not in R:
        from nuwa_pytorch_amd import ops
        R['S16'] = float(ops._grad_scale(R['I']['do'].reshape(-1, c['heads'] * c['dim_head']).to(DEV))[0])
    return R['S16']


def run(K, c, R, keep, scale):
    """-> (values by name as fp32 / fp64-comparable CPU tensors, the raw output arrays).  keep: kernel-order mask or None"""
    from guard_util import guard, guarded
    I = R['I']
    B, n, h, d = c['B'], c['ntok'], c['heads'], c['dim_head']
    inner, hilo = h * d, c['form'] == 'hilo'
    gd_ = lambda t: guarded(t, device=DEV) if t is not None else None
    kw = {} if keep is None else dict(keep=gd_(keep.to(torch.uint8)), drop_scale=scale)
    wth = gd_(I['wth'])
    g = K.s3_geom(B, n, c['grid'], c['window'], c['dilation'], h, d, causal=c['causal'])
    val = lambda p: (p.hi.float() + p.lo.float() if p.lo is not None else p.hi.float()).cpu()
    parts = lambda p: [t for t in (p.hi, p.lo, p.f16) if t is not None]
    out, raw = {}, []
    if c['cross']:
        Tk = ctx_rows(c)
        q, dO = _pair(K, I['q'].reshape(B * n, inner), hilo), _pair(K, I['do'].reshape(B * n, inner), hilo)
        kv = _pair(K, torch.cat((I['k'].reshape(B * Tk, inner), I['v'].reshape(B * Tk, inner)), 1), hilo)
        nk, nv = _pair(K, I['nk'].reshape(-1), hilo), _pair(K, I['nv'].reshape(-1), hilo)
        m8 = gd_(I['kmask'].to(torch.uint8)) if I['kmask'] is not None else None
        with guard(K) as gd:
            o = K.cross2dna_fwd(g, q, kv, nk, nv, m8, wth, Tk, **kw)
            dq, dkv, dnk, dnv, dwth = K.cross2dna_bwd(g, q, kv, nk, nv, m8, wth, dO, Tk, **kw)
            assert gd.made() > 0
        rows = lambda p: val(p).reshape(B, n, h, d)[:, 1:]            # row 0 (<bos>) is the caller's: not written, not compared
        dkvv = val(dkv)
        out = dict(o=rows(o), dq=rows(dq), dk=dkvv[:, :inner].reshape(B, Tk, h, d), dv=dkvv[:, inner:].reshape(B, Tk, h, d),
                   dnk=dnk.reshape(h, d).cpu(), dnv=dnv.reshape(h, d).cpu(), dwth=dwth.cpu())
        for p in (o, dq):
            raw += [t.reshape(B, n, inner)[:, 1:].cpu() for t in parts(p)]
        raw += [t.cpu() for t in parts(dkv)] + [dnk.cpu(), dnv.cpu(), dwth.cpu()]
        return out, raw
    rel = gd_(torch.cat((torch.zeros(1, h), I['rel'].t()), 0).contiguous()) if I['rel'] is not None else None
    flat = I['qkv'].reshape(B * n, 3 * inner)
    if c['form'] == 'f16fwd':
        qkv = K.BF(None, None, gd_(flat.half()))
        with guard(K) as gd:
            o = K.sparse3dna_fwd(g, qkv, wth, rel_bias=rel, **kw)
            assert gd.made() > 0
        assert o.hi is not None and o.lo is not None and o.f16 is None
        return dict(o=val(o).reshape(B, n, h, d)), [t.cpu() for t in parts(o)]
    if c['form'] == 'f16grad':
        assert K.s3_bwd16_supported(g)
        S16 = grad_scale(c, R)
        q16, dO16 = gd_(flat.half()), gd_((I['do'].reshape(B * n, inner) * S16).half())
        s2 = torch.tensor([S16, 1.0 / S16], dtype=torch.float32, device=DEV)
        K.f16_sat_count()
        with guard(K) as gd:
            dqkv, dwth = K.sparse3dna_bwd16(g, q16, wth, dO16, s2, **kw)
            assert gd.made() > 0
        assert K.f16_sat_count() == 0, 'fp16 stores saturated'
        dv_ = (dqkv.float() / S16).cpu().reshape(B, n, 3, h, d)
        return dict(dq=dv_[:, :, 0], dk=dv_[:, :, 1], dv=dv_[:, :, 2], dwth=dwth.cpu()), [dqkv.cpu(), dwth.cpu()]
    qkv, dO = _pair(K, flat, hilo), _pair(K, I['do'].reshape(B * n, inner), hilo)
    with guard(K) as gd:
        o = K.sparse3dna_fwd(g, qkv, wth, rel_bias=rel, **kw)
        dqkv, dwth, drel = K.sparse3dna_bwd(g, qkv, wth, dO, rel_bias=rel, **kw)
        assert gd.made() > 0
    assert (o.lo is not None) == hilo and (dqkv.lo is not None) == hilo
    dv_ = val(dqkv).reshape(B, n, 3, h, d)
    out = dict(o=val(o).reshape(B, n, h, d), dq=dv_[:, :, 0], dk=dv_[:, :, 1], dv=dv_[:, :, 2], dwth=dwth.cpu())
    if drel is not None:
        out['drel'] = drel[1:].t().cpu()
    raw = [t.cpu() for t in parts(o) + parts(dqkv)] + [dwth.cpu()] + ([drel.cpu()] if drel is not None else [])
    return out, raw


def expected(c, R):
    """the float64 results by the names run() uses"""
    G = R['grads']
    if c['cross']:
        return dict(o=R['o'].detach(), dq=G['q'][:, 1:], dk=G['k'], dv=G['v'], dnk=G['nk'], dnv=G['nv'], dwth=G['wth'])
    if c['form'] == 'f16fwd':
        return dict(o=R['o'].detach())
    if c['form'] == 'f16grad':
        S16 = R['S16']
        G = grads64(R, (R['I']['do'] * S16).half().float() / S16)
        return dict(dq=G['qkv'][:, :, 0], dk=G['qkv'][:, :, 1], dv=G['qkv'][:, :, 2], dwth=G['wth'])
    E = dict(o=R['o'].detach(), dq=G['qkv'][:, :, 0], dk=G['qkv'][:, :, 1], dv=G['qkv'][:, :, 2], dwth=G['wth'])
    if 'rel' in G:
        E['drel'] = G['rel']
    return E
