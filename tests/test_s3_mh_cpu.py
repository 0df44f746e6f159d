"""Sparse3DNA with 9 .. 16 heads (Sparse3DNA.many_heads, csrc/sparse3dna_mh.hip), everything that needs no device: the envelope and the
argument checks of the four new entry points (every case returns before a launch: B = 0, or an error that precedes it), the workspace
size against the s3_ws formula, the module switch through _meta / block_plan, and a launch-log walk of the GPU case list (which kernel
instantiation each case launches, with which grid, block and dynamic LDS)."""
import ctypes
import os
import re
import shutil
import sys

import pytest
import torch

import s3_mh_cases_util as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
_PTRS = ctypes.create_string_buffer(64)
PTR = (ctypes.addressof(_PTRS) + 15) & ~15                        # non-null, 16-byte aligned, never dereferenced

FWD = 'q k v q_lo k_lo v_lo ld w_th o o_lo ldo'.split()
BWD = 'q k v q_lo k_lo v_lo ld w_th dO dO_lo lddo dq dk dv dq_lo dk_lo dv_lo ldd dw_th accumulate workspace workspace_bytes'.split()


@pytest.fixture(scope='module')
def L():
    from nuwa_pytorch_amd import _lib
    return _lib.lib()


def geom(heads=12, dim_head=64, grid=(2, 4, 4), B=2, **over):
    from nuwa_pytorch_amd import _lib
    c = dict(B=B, ntok=1 + grid[0] * grid[1] * grid[2], grid=grid, window=(3, 3, 3), dilation=(1, 1, 1), heads=heads, dim_head=dim_head)
    return M.geom(_lib.S3Geom, c, **over)


def call(L, entry, g, **over):
    names = FWD if entry == 'fwd' else BWD
    short = over.pop('ws_short', 0)
    args = []
    for n in names:
        if n in over:
            v = over[n]
        elif n == 'workspace_bytes':
            v = (L.amdnuwa_sparse3dna_mh_bwd_workspace_bytes(ctypes.byref(g)) if g is not None else 0) - short
        elif n.startswith('ld'):
            v = 3072
        elif n == 'accumulate':
            v = 0
        elif n.endswith('_lo'):
            v = None
        else:
            v = PTR
        args.append(v)
    fn = L.amdnuwa_sparse3dna_mh_fwd if entry == 'fwd' else L.amdnuwa_sparse3dna_mh_bwd
    return fn(ctypes.byref(g) if g is not None else None, *args, None)


def test_abi_version_is_unchanged(L):
    assert L.amdnuwa_abi_version() == 21


@pytest.mark.parametrize('heads,want', [(8, UNSUPPORTED), (9, OK), (16, OK), (17, UNSUPPORTED)])
def test_head_envelope(L, heads, want):
    g = geom(heads=heads, B=0)
    assert call(L, 'fwd', g) == want and call(L, 'bwd', g) == want
    for lo in (0, 1):
        assert L.amdnuwa_s3mh_supported(ctypes.byref(g), lo) == (1 if want == OK else 0)
    assert (L.amdnuwa_sparse3dna_mh_bwd_workspace_bytes(ctypes.byref(g)) > 0) == (want == OK)


def test_the_existing_entries_and_the_new_ones_split_the_head_counts(L):
    """8 heads: the existing entries; 9: the new ones -- never both"""
    for heads in (8, 9):
        g = geom(heads=heads)
        assert bool(L.amdnuwa_s3_supported(ctypes.byref(g), 0)) == (heads == 8)
        assert bool(L.amdnuwa_s3mh_supported(ctypes.byref(g), 0)) == (heads == 9)


@pytest.mark.parametrize('entry', ['fwd', 'bwd'])
def test_envelope_and_argument_checks(L, entry):
    assert call(L, entry, None) == ARG                                                     # null geometry
    assert call(L, entry, geom(dim_head=48)) == UNSUPPORTED
    assert call(L, entry, geom(noncausal=1)) == UNSUPPORTED
    assert call(L, entry, geom(noncausal=1, B=0)) == UNSUPPORTED
    assert call(L, entry, geom(grid=(1, 2, 65))) == UNSUPPORTED                            # wider than 64 columns
    assert call(L, entry, geom(heads=16, grid=(1, 2, 16), dw=2000)) == UNSUPPORTED         # a halo beyond the LDS limit
    assert call(L, entry, geom(kf=0)) == ARG
    assert call(L, entry, geom(ntok=34)) == ARG                                            # beyond the 2 x 4 x 4 grid
    assert call(L, entry, geom(dim_head=48), q=None) == UNSUPPORTED                        # the geometry comes first
    for name in ('q', 'k', 'v', 'w_th') + (('o',) if entry == 'fwd' else ('dO', 'dq', 'dk', 'dv', 'dw_th')):
        assert call(L, entry, geom(), **{name: None}) == ARG, name
        assert call(L, entry, geom(B=0), **{name: None}) == ARG, name                      # checked before the B <= 0 return
    for name in ('ld', 'ldo') if entry == 'fwd' else ('ld', 'lddo', 'ldd'):
        assert call(L, entry, geom(), **{name: 3076}) == ARG, name
    assert call(L, entry, geom(), k_lo=PTR) == ARG                                         # a missing lo half: k_lo without q_lo / v_lo
    assert call(L, entry, geom(B=0), k_lo=PTR) == OK                                       # (checked after the B <= 0 return, as in the 8-head entries)
    assert call(L, entry, geom(B=0)) == OK and call(L, entry, geom(B=-1)) == OK
    if entry == 'bwd':
        assert call(L, entry, geom(), ws_short=1) == WORKSPACE
        assert call(L, entry, geom(), workspace=None) == WORKSPACE
        assert call(L, entry, geom(B=0), ws_short=1) == WORKSPACE
        assert call(L, entry, geom(), q_lo=PTR, k_lo=PTR, v_lo=PTR) == ARG                 # hi + lo q / k / v without dO_lo
        assert call(L, entry, geom(), dO_lo=PTR) == ARG


def test_supported_query_follows_the_lds_need(L):
    # 16 heads x 64 on 8-column tiles: stage of (8 + halo) columns x 1024 x 8 bytes on the key side
    for dw, want in ((1, 1), (4, 1), (8, 0)):
        g = geom(heads=16, grid=(1, 2, 16), dw=dw)
        c = dict(grid=(1, 2, 16), window=(3, 3, 3), dilation=(1, 1, dw), heads=16, dim_head=64)
        assert (max(M.lds(c, True)) <= M.S3_LDS_MAX) == bool(want), dw
        assert L.amdnuwa_s3mh_supported(ctypes.byref(g), 1) == want, dw


def test_workspace_bytes_follow_the_s3_ws_formula(L):
    from nuwa_pytorch_amd import _lib
    for c in M.all_cases():
        g = M.geom(_lib.S3Geom, c)
        assert L.amdnuwa_sparse3dna_mh_bwd_workspace_bytes(ctypes.byref(g)) == M.workspace_bytes(c), c['name']


def test_every_new_entry_is_declared(L):
    from nuwa_pytorch_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'amdnuwa.h')).read()
    for name in ('amdnuwa_s3mh_supported', 'amdnuwa_sparse3dna_mh_bwd_workspace_bytes', 'amdnuwa_sparse3dna_mh_fwd', 'amdnuwa_sparse3dna_mh_bwd'):
        assert name in _lib.SIGNATURES and re.search(rf'\b{name}\(', header) and hasattr(L, name), name


# ---------------------------------------------------------------------------------------------------
# the module switch
# ---------------------------------------------------------------------------------------------------
def _s3(heads, **kw):
    import nuwa_pytorch_amd as A
    return A.Sparse3DNA(dim=32, heads=heads, dim_head=32, **{'causal': True, 'video_shape': (2, 4, 4), 'kernel_size': 3, **kw})


CPU = torch.device('cpu')


def test_switch_off_is_todays_error_with_a_pointer_to_the_switch():
    import nuwa_pytorch_amd as A
    assert A.Sparse3DNA.many_heads is False
    with pytest.raises(NotImplementedError, match='12 heads.*up to 8 heads.*many_heads'):
        _s3(12)._meta(2, 33, CPU)


def test_switch_on_plans_the_plain_s3_block(monkeypatch):
    import nuwa_pytorch_amd as A
    from nuwa_pytorch_amd import ops
    monkeypatch.setattr(A.Sparse3DNA, 'many_heads', True)
    m = _s3(12)
    meta = m._meta(2, 33, CPU)
    assert meta['kind'] == 's3' and meta['geom'].heads == 12 and 'drop_p' not in meta
    pl = ops.block_plan('s3', 2 * 33, 32, m._plan_params(), meta)
    assert not pl.a16 and not pl.core16 and not pl.o16 and not pl.bwd16 and len(pl.guarded) == 3
    m8 = _s3(8)                                              # 8 heads plan as before, switch or not
    assert m8._meta(2, 33, CPU)['geom'].heads == 8


def test_switch_per_instance():
    m = _s3(16)
    m.many_heads = True
    assert m._meta(2, 33, CPU)['geom'].heads == 16
    with pytest.raises(NotImplementedError, match='up to 8 heads'):
        _s3(16)._meta(2, 33, CPU)


def test_switch_on_named_refusals(monkeypatch):
    import nuwa_pytorch_amd as A
    monkeypatch.setattr(A.Sparse3DNA, 'many_heads', True)
    with pytest.raises(NotImplementedError, match='17 heads.*up to 16 heads'):
        _s3(17)._meta(2, 33, CPU)
    with pytest.raises(NotImplementedError, match='12 heads and attention dropout'):
        _s3(12, dropout=0.1).train()._meta(2, 33, CPU)
    assert _s3(12, dropout=0.1).eval()._meta(2, 33, CPU)['geom'].heads == 12          # dropout that is not live: fine
    with pytest.raises(NotImplementedError, match='12 heads.*do not take this geometry'):
        A.Sparse3DNA(dim=32, heads=12, dim_head=48, causal=True, video_shape=(2, 4, 4), kernel_size=3)._meta(2, 33, CPU)
    m = _s3(12, causal=False)                                # the symmetric window stays on torch ops
    assert not m._hip_ok()


def test_incremental_decoder_still_declines(monkeypatch):
    import nuwa_pytorch_amd as A
    from nuwa_pytorch_amd import decode, ops
    monkeypatch.setattr(A.Sparse3DNA, 'many_heads', True)
    monkeypatch.setattr(ops, '_ctx_to_bf', lambda context: None)
    m = A.Transformer(dim=32, depth=1, heads=16, dim_head=32, causal=True, cross_attend=True, sparse_3dna_attn=True,
                      sparse_3dna_video_shape=(2, 4, 4), sparse_3dna_kernel_size=3, shift_video_tokens=True)
    with pytest.raises(NotImplementedError, match='16 heads'):
        decode.IncrementalDecoder(m, 2, 33, torch.zeros(2, 4, 32), torch.ones(2, 4, dtype=torch.bool), torch.zeros(1, dtype=torch.int32))


# ---------------------------------------------------------------------------------------------------
# the launch-log walk
# ---------------------------------------------------------------------------------------------------
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


@pytest.fixture(scope='module')
def walked(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which('hipcc')):
        pytest.skip('hipcc is not installed')
    sys.path.insert(0, os.path.join(ROOT, 'tools', 'launch_log'))
    try:
        import run as LR
        import cases_s3_mh as CS
    finally:
        sys.path.pop(0)
    lib_path = LR.build(ROOT, CS.SOURCE, CS.STUBS, str(tmp_path_factory.mktemp('launch_log_mh')), [])
    names, kernels = LR.symbols(lib_path)
    LL = ctypes.CDLL(lib_path)
    LL.launch_log_take.restype = ctypes.c_size_t
    LL.launch_log_take.argtypes = [ctypes.c_char_p, ctypes.c_size_t]
    buf = ctypes.create_string_buffer(1 << 16)
    rows = []
    for name, _, fn in CS.cases(LL):
        rc = fn()
        n = LL.launch_log_take(buf, len(buf))
        assert n < len(buf)
        body = re.sub(r'\+0x([0-9a-f]+)', lambda m: names.get(int(m.group(1), 16), m.group(0)), buf.value.decode())
        rows.append((name, rc, body.splitlines()))
    short = lambda k: re.sub(r'^void |\(.*$', '', k)
    return {short(k) for k in kernels}, rows, short


def _launches(lines, short):
    out = []
    for ln in lines:
        if ln.startswith('launch '):
            m = re.match(r'launch (.*) grid (\d+) (\d+) (\d+) block (\d+) (\d+) (\d+) lds (\d+) args', ln)
            out.append((short(m.group(1)),) + tuple(int(v) for v in m.groups()[1:]))
    return out


def test_launch_log_grid_block_and_lds(walked):
    kernels, rows, short = walked
    assert len(kernels) == 12, sorted(kernels)                       # 3 kernels x dim_head 32 / 64 x bf16 / hi + lo
    by_name = {c['name']: c for c in M.all_cases()}
    seen = {}
    for name, rc, lines in rows:
        cname, entry = name.split(' :: ')
        c = by_name[cname]
        lo = c['form'] == 'hilo'
        assert rc == 0, name
        la = _launches(lines, short)
        attrs = [ln for ln in lines if ln.startswith('attr ')]
        F, H, _ = c['grid']
        grid = c['B'] * F * H * M.tile(c)[1]                         # B * F * H * NT, query side and key side (FK = F) alike
        block = M.threads(c)
        assert block <= 512 and block % 64 == 0 and block >= M.tile(c)[0] * c['heads'] * 4
        fwd, bq, bkv = M.lds(c, lo)
        assert max(fwd, bq, bkv) <= M.S3_LDS_MAX
        tpl = f"<{c['dim_head']}, {'true' if lo else 'false'}>"
        want = [('s3mh_fwd_kernel' + tpl, fwd)] if entry == 'fwd' else [('s3mh_bwd_q_kernel' + tpl, bq), ('s3mh_bwd_kv_kernel' + tpl, bkv)]
        assert [(k, l) for k, *_, l in la] == want, (name, la)
        assert len(attrs) == len(la)                                 # the dynamic-LDS allowance is set on every launch
        for k, gx, gy, gz, bx, by, bz, _ in la:
            assert (gx, gy, gz) == (grid, 1, 1) and (bx, by, bz) == (block, 1, 1), (name, k)
            seen.setdefault(k, set()).add(cname)
        tail = [ln for ln in lines if ln.startswith('extern ')]
        assert tail == ([f"extern s3_bwd_tail d_rel_bias {1 if c['bias'] else 0}"] if entry == 'bwd' else []), name
    assert set(seen) == kernels
    for k in sorted(kernels):
        assert len(seen[k]) >= 2, (k, seen[k])                       # every instantiation by at least two cases
