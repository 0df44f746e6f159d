"""The block plan (ops.block_plan: Plan of one decoder block) is a pure function of the precision mode, the A/B switches, the kernels'
host-side support queries and the fp16 range verdict of the block's weights.  Needs the built library, no device.

TABLE pins the whole record for 144 inputs: dim 512; cross attention at (B, n, T, heads, dim_head), Sparse3DNA at (B, video shape) with a
3 x 3 x 3 window, FeedForward at (B, n); the three precision modes; one switch at a time around the defaults of 'bf16x3-fwd'; the weight
verdict True / False; a separate residual input ('resid': reversible stacks), no LayerNorm in front ('noln': the standalone modules),
rotary embeddings, keys from the query rows ('self_kv'), a bf16 null key, a relative-position bias ('rel'), live dropout ('drop').
The expected records were taken from the commit BEFORE the plan existed -- the block-level form (h16, bwd16) by calling that commit's own
predicates the way its SandwichBlockFn.forward did, the routes by walking its S3Inner / XInner / FFInner.fwd and XInner.bwd ladders -- and
confirmed on the device for the rows tools/launch_trace.py runs (profiles/block_plan_parity.txt).
Columns: (h16, bwd16, a16, core16, o16, core, pack, lean, bwd); see the comment above ops.Plan."""
import contextlib
import os

import pytest
import torch

from nuwa_pytorch_amd import kernels as K, nuwa_pytorch as NP, ops


DIM = 512
_SET = dict(cores_f16='set_cores_f16', xattn6='set_xattn6', xattn_rc='set_xattn_rc', bwd_f16='set_bwd_f16', proj_f16x2='set_proj_f16x2',
            qkv_f16='set_qkv_f16', ff_f16='set_ff_f16')
_STATE = ('_PRECISION', '_CORES_F16', '_XATTN6', '_XATTN_RC', '_BWD_F16', '_PROJ_F16X2', '_QKV_F16', '_FF_F16')


@contextlib.contextmanager
def apply_switch(mode, switch):
    """the precision mode and ONE switch away from the defaults; everything restored on exit"""
    saved, env = {k: getattr(K, k) for k in _STATE}, {k: os.environ.get(k) for k in ('AMDNUWA_XATTN6_BWD', 'AMDNUWA_XATTN_CM')}
    try:
        K.set_precision(mode)
        K.set_cores_f16(True), K.set_xattn6(True), K.set_xattn_rc(False), K.set_bwd_f16(K.DEFAULT_BWD_F16), K.set_proj_f16x2(K.DEFAULT_F16X2)
        K.set_qkv_f16(True), K.set_ff_f16(True)
        for k in env:
            os.environ.pop(k, None)
        if switch:
            name, val = switch.split('=')
            if name in _SET:
                getattr(K, _SET[name])({'0': False, '1': True}.get(val, val))
            else:
                os.environ[name] = val
        yield
    finally:
        for k, v in saved.items():
            setattr(K, k, v)
        for k, v in env.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


_MODULES = {}


def _module(key, make):
    if key not in _MODULES:
        _MODULES[key] = make()
    return _MODULES[key]


def build_case(case):
    """-> (R, D, params, meta as the block itself has it when it plans, meta as its predecessor in the chain builds it)"""
    kind, geom, mode, switch, wok, flags = case
    flags = flags.split()
    if kind == 'xattn':
        B, n, T, heads, dh = geom
        m = _module((kind, heads, dh), lambda: NP.Attention(dim=DIM, heads=heads, dim_head=dh))
        mask = torch.ones(B, T, dtype=torch.bool)
        if 'self_kv' in flags:
            kw = dict(mask=mask, rotary_pos_emb=torch.zeros(n, dh) if 'rotary' in flags else None)
        else:
            kw = dict(context=torch.empty(B, T, DIM), context_mask=mask)
        own = m._meta(B, n, 'cpu', **kw)
        pred = m._meta(B, n, 'cpu', **{k: v for k, v in kw.items() if 'mask' not in k})
        if 'rotary' in flags and 'self_kv' not in flags:
            own['rotary'] = pred['rotary'] = torch.zeros(n, dh)
        p = m._params()
        if 'nk_bf16' in flags:
            p = (p[0].bfloat16(),) + p[1:]
    elif kind == 's3':
        B, vs = geom
        n = vs[0] * vs[1] * vs[2]
        rel = 'rel' in flags
        m = _module((kind, vs, rel), lambda: NP.Sparse3DNA(dim=DIM, video_shape=vs, kernel_size=(3, 3, 3), dilation=1, heads=8, dim_head=64,
                                                               causal=True, rel_pos_bias=rel))
        own, pred, p = m._meta(B, n, 'cpu'), m._meta(B, n, 'cpu'), m._params()
        own['shift'] = (n, vs[2])
    else:
        B, n = geom
        drop = 'drop' in flags
        m = _module((kind, drop), lambda: NP.FeedForward(dim=DIM, mult=4, dropout=0.1 if drop else 0.).train())
        own, pred, p = m._meta(B, n, 'cpu'), m._meta(B, n, 'cpu'), m._params()
        own['shift'] = (n, 16)
    # what SandwichBlockFn.forward does to its meta before it plans: the shift rides in the pre-norm's store, the context's copy is there
    own = dict(own)
    if own.get('shift') is not None:
        own['shift'] = None
    if kind == 'xattn' and 'self_kv' not in flags:
        own['ctx_bf'] = object()
    return B * n, DIM, p, own, pred


TABLE = [
    (('xattn', (1, 2560, 256, 8, 64), 'bf16x3-fwd', '', True, ''), ('only', True, True, True, 'only', 'x6_f16_only', 'x6b16', False, 'x6_16')),
    (('xattn', (1, 2560, 256, 8, 64), 'bf16', '', True, ''), (False, False, False, False, False, 'x6_bf16', 'x6b', False, 'x6')),
    (('xattn', (1, 2560, 256, 8, 64), 'bf16x3', '', True, ''), (False, False, False, False, False, 'x1_p', 'x1', False, 'x1')),
    (('xattn', (1, 512, 128, 8, 64), 'bf16x3-fwd', '', True, ''), ('only', True, True, True, 'only', 'x6_f16_only', 'x6b16', False, 'x6_16')),
    (('xattn', (1, 512, 128, 8, 64), 'bf16', '', True, ''), (False, False, False, False, False, 'x6_bf16', 'x6b', False, 'x6')),
    (('xattn', (1, 512, 128, 8, 64), 'bf16x3', '', True, ''), (False, False, False, False, False, 'x1_p', 'x1', False, 'x1')),
    (('xattn', (1, 512, 64, 8, 64), 'bf16x3-fwd', '', True, ''), (True, False, True, True, True, 'x6_f16', 'x1', 'bwd', 'x2')),
    (('xattn', (1, 512, 64, 8, 64), 'bf16', '', True, ''), (False, False, False, False, False, 'x6_bf16', 'x1', 'bwd', 'x2')),
    (('xattn', (1, 512, 64, 8, 64), 'bf16x3', '', True, ''), (False, False, False, False, False, 'x1_p', 'x1', False, 'x1')),
    (('xattn', (2, 48, 128, 8, 64), 'bf16x3-fwd', '', True, ''), (True, False, True, True, True, 'x6_f16', 'x6b', False, 'x6')),
    (('xattn', (2, 48, 128, 8, 64), 'bf16', '', True, ''), (False, False, False, False, False, 'x6_bf16', 'x6b', False, 'x6')),
    (('xattn', (2, 48, 128, 8, 64), 'bf16x3', '', True, ''), (False, False, False, False, False, 'x1_p', 'x1', False, 'x1')),
    (('xattn', (1, 512, 128, 4, 64), 'bf16x3-fwd', '', True, ''), (False, False, False, False, False, 'x1_p', 'x1', False, 'x1')),
    (('xattn', (1, 512, 128, 4, 64), 'bf16', '', True, ''), (False, False, False, False, False, 'x1_p', 'x1', False, 'x1')),
    (('xattn', (1, 512, 128, 4, 64), 'bf16x3', '', True, ''), (False, False, False, False, False, 'x1_p', 'x1', False, 'x1')),
    (('xattn', (1, 512, 128, 8, 32), 'bf16x3-fwd', '', True, ''), (False, False, False, False, False, 'x1_p', 'x1', False, 'x1')),
    (('xattn', (1, 512, 128, 8, 32), 'bf16', '', True, ''), (False, False, False, False, False, 'x1_p', 'x1', False, 'x1')),
    (('xattn', (1, 512, 128, 8, 32), 'bf16x3', '', True, ''), (False, False, False, False, False, 'x1_p', 'x1', False, 'x1')),
    (('xattn', (1, 512, 128, 8, 64), 'bf16x3-fwd', 'cores_f16=0', True, ''), (False, False, False, False, False, 'x1_stats', 'x1', False, 'x2')),
    (('xattn', (1, 512, 128, 8, 64), 'bf16x3-fwd', 'xattn6=0', True, ''), (True, False, True, True, True, 'x2_f16', 'x1', True, 'x2')),
    (('xattn', (1, 512, 128, 8, 64), 'bf16x3-fwd', 'xattn_rc=1', True, ''), (True, False, True, True, True, 'x6_f16', 'x1', False, 'x2_rc')),
    (('xattn', (1, 512, 128, 8, 64), 'bf16x3-fwd', 'bwd_f16=', True, ''), (True, False, True, True, True, 'x6_f16', 'x6b', False, 'x6')),
    (('xattn', (1, 512, 128, 8, 64), 'bf16x3-fwd', 'bwd_f16=f', True, ''), (True, False, True, True, True, 'x6_f16', 'x6b', False, 'x6')),
    (('xattn', (1, 512, 128, 8, 64), 'bf16x3-fwd', 'bwd_f16=fs', True, ''), (True, False, True, True, True, 'x6_f16', 'x6b', False, 'x6')),
    (('xattn', (1, 512, 128, 8, 64), 'bf16x3-fwd', 'proj_f16x2=', True, ''), (False, False, False, True, False, 'x6_f16', 'x6b', False, 'x6')),
    (('xattn', (1, 512, 128, 8, 64), 'bf16x3-fwd', 'proj_f16x2=o', True, ''), (False, False, False, True, True, 'x6_f16', 'x6b', False, 'x6')),
    (('xattn', (1, 512, 128, 8, 64), 'bf16x3-fwd', 'proj_f16x2=q', True, ''), (True, False, True, True, False, 'x6_f16', 'x6b', False, 'x6')),
    (('xattn', (1, 512, 128, 8, 64), 'bf16x3-fwd', 'qkv_f16=0', True, ''), ('only', True, True, True, 'only', 'x6_f16_only', 'x6b16', False, 'x6_16')),
    (('xattn', (1, 512, 128, 8, 64), 'bf16x3-fwd', 'ff_f16=0', True, ''), ('only', True, True, True, 'only', 'x6_f16_only', 'x6b16', False, 'x6_16')),
    (('xattn', (1, 512, 128, 8, 64), 'bf16x3-fwd', 'AMDNUWA_XATTN6_BWD=0', True, ''), (True, False, True, True, True, 'x6_f16', 'x1', 'bwd', 'x2')),
    (('xattn', (1, 512, 128, 8, 64), 'bf16x3-fwd', 'AMDNUWA_XATTN_CM=0', True, ''), (True, False, True, True, True, 'x6_f16', 'x1', 'bwd', 'x2')),
    (('xattn', (1, 512, 64, 8, 64), 'bf16x3-fwd', 'cores_f16=0', True, ''), (False, False, False, False, False, 'x1_stats', 'x1', False, 'x2')),
    (('xattn', (1, 512, 64, 8, 64), 'bf16x3-fwd', 'xattn6=0', True, ''), (True, False, True, True, True, 'x2_f16', 'x1', True, 'x2')),
    (('xattn', (1, 512, 64, 8, 64), 'bf16x3-fwd', 'xattn_rc=1', True, ''), (True, False, True, True, True, 'x6_f16', 'x1', False, 'x2_rc')),
    (('xattn', (1, 512, 64, 8, 64), 'bf16x3-fwd', 'bwd_f16=', True, ''), (True, False, True, True, True, 'x6_f16', 'x1', 'bwd', 'x2')),
    (('xattn', (1, 512, 64, 8, 64), 'bf16x3-fwd', 'bwd_f16=f', True, ''), (True, False, True, True, True, 'x6_f16', 'x1', 'bwd', 'x2')),
    (('xattn', (1, 512, 64, 8, 64), 'bf16x3-fwd', 'bwd_f16=fs', True, ''), (True, False, True, True, True, 'x6_f16', 'x1', 'bwd', 'x2')),
    (('xattn', (1, 512, 64, 8, 64), 'bf16x3-fwd', 'proj_f16x2=', True, ''), (False, False, False, True, False, 'x6_f16', 'x1', 'bwd', 'x2')),
    (('xattn', (1, 512, 64, 8, 64), 'bf16x3-fwd', 'proj_f16x2=o', True, ''), (False, False, False, True, True, 'x6_f16', 'x1', 'bwd', 'x2')),
    (('xattn', (1, 512, 64, 8, 64), 'bf16x3-fwd', 'proj_f16x2=q', True, ''), (True, False, True, True, False, 'x6_f16', 'x1', 'bwd', 'x2')),
    (('xattn', (1, 512, 64, 8, 64), 'bf16x3-fwd', 'qkv_f16=0', True, ''), (True, False, True, True, True, 'x6_f16', 'x1', 'bwd', 'x2')),
    (('xattn', (1, 512, 64, 8, 64), 'bf16x3-fwd', 'ff_f16=0', True, ''), (True, False, True, True, True, 'x6_f16', 'x1', 'bwd', 'x2')),
    (('xattn', (1, 512, 64, 8, 64), 'bf16x3-fwd', 'AMDNUWA_XATTN6_BWD=0', True, ''), (True, False, True, True, True, 'x6_f16', 'x1', 'bwd', 'x2')),
    (('xattn', (1, 512, 64, 8, 64), 'bf16x3-fwd', 'AMDNUWA_XATTN_CM=0', True, ''), (True, False, True, True, True, 'x6_f16', 'x1', 'bwd', 'x2')),
    (('xattn', (1, 512, 128, 8, 64), 'bf16x3-fwd', '', False, ''), (False, False, False, True, False, 'x6_f16', 'x6b', False, 'x6')),
    (('xattn', (1, 512, 64, 8, 64), 'bf16x3-fwd', '', False, ''), (False, False, False, True, False, 'x6_f16', 'x1', 'bwd', 'x2')),
    (('xattn', (1, 512, 128, 8, 64), 'bf16x3-fwd', '', True, 'resid'), (True, False, True, True, True, 'x6_f16', 'x6b', False, 'x6')),
    (('xattn', (1, 512, 128, 8, 64), 'bf16x3-fwd', '', True, 'noln'), (False, False, True, True, True, 'x6_f16', 'x6b', False, 'x6')),
    (('xattn', (1, 512, 64, 8, 64), 'bf16x3-fwd', '', True, 'resid'), (True, False, True, True, True, 'x6_f16', 'x1', 'bwd', 'x2')),
    (('xattn', (1, 512, 64, 8, 64), 'bf16x3-fwd', '', True, 'noln'), (False, False, True, True, True, 'x6_f16', 'x1', 'bwd', 'x2')),
    (('s3', (1, (2, 16, 16)), 'bf16x3-fwd', '', True, ''), ('only', True, True, True, 'only', None, None, False, None)),
    (('s3', (1, (2, 16, 16)), 'bf16', '', True, ''), (False, False, False, False, False, None, None, False, None)),
    (('s3', (1, (2, 16, 16)), 'bf16x3', '', True, ''), (False, False, False, False, False, None, None, False, None)),
    (('s3', (1, (4, 8, 8)), 'bf16x3-fwd', '', True, ''), (False, False, False, False, False, None, None, False, None)),
    (('s3', (1, (4, 8, 8)), 'bf16', '', True, ''), (False, False, False, False, False, None, None, False, None)),
    (('s3', (1, (4, 8, 8)), 'bf16x3', '', True, ''), (False, False, False, False, False, None, None, False, None)),
    (('s3', (1, (2, 16, 16)), 'bf16x3-fwd', 'cores_f16=0', True, ''), (False, False, False, False, False, None, None, False, None)),
    (('s3', (1, (2, 16, 16)), 'bf16x3-fwd', 'xattn6=0', True, ''), ('only', True, True, True, 'only', None, None, False, None)),
    (('s3', (1, (2, 16, 16)), 'bf16x3-fwd', 'xattn_rc=1', True, ''), ('only', True, True, True, 'only', None, None, False, None)),
    (('s3', (1, (2, 16, 16)), 'bf16x3-fwd', 'bwd_f16=', True, ''), (True, False, True, True, True, None, None, False, None)),
    (('s3', (1, (2, 16, 16)), 'bf16x3-fwd', 'bwd_f16=f', True, ''), (True, False, True, True, True, None, None, False, None)),
    (('s3', (1, (2, 16, 16)), 'bf16x3-fwd', 'bwd_f16=fs', True, ''), ('only', True, True, True, 'only', None, None, False, None)),
    (('s3', (1, (2, 16, 16)), 'bf16x3-fwd', 'proj_f16x2=', True, ''), (True, False, True, True, False, None, None, False, None)),
    (('s3', (1, (2, 16, 16)), 'bf16x3-fwd', 'proj_f16x2=o', True, ''), ('only', True, True, True, 'only', None, None, False, None)),
    (('s3', (1, (2, 16, 16)), 'bf16x3-fwd', 'proj_f16x2=q', True, ''), (True, False, True, True, False, None, None, False, None)),
    (('s3', (1, (2, 16, 16)), 'bf16x3-fwd', 'qkv_f16=0', True, ''), (False, False, False, True, True, None, None, False, None)),
    (('s3', (1, (2, 16, 16)), 'bf16x3-fwd', 'ff_f16=0', True, ''), ('only', True, True, True, 'only', None, None, False, None)),
    (('s3', (1, (2, 16, 16)), 'bf16x3-fwd', 'AMDNUWA_XATTN6_BWD=0', True, ''), ('only', True, True, True, 'only', None, None, False, None)),
    (('s3', (1, (2, 16, 16)), 'bf16x3-fwd', 'AMDNUWA_XATTN_CM=0', True, ''), ('only', True, True, True, 'only', None, None, False, None)),
    (('s3', (1, (4, 8, 8)), 'bf16x3-fwd', 'cores_f16=0', True, ''), (False, False, False, False, False, None, None, False, None)),
    (('s3', (1, (4, 8, 8)), 'bf16x3-fwd', 'xattn6=0', True, ''), (False, False, False, False, False, None, None, False, None)),
    (('s3', (1, (4, 8, 8)), 'bf16x3-fwd', 'xattn_rc=1', True, ''), (False, False, False, False, False, None, None, False, None)),
    (('s3', (1, (4, 8, 8)), 'bf16x3-fwd', 'bwd_f16=', True, ''), (False, False, False, False, False, None, None, False, None)),
    (('s3', (1, (4, 8, 8)), 'bf16x3-fwd', 'bwd_f16=f', True, ''), (False, False, False, False, False, None, None, False, None)),
    (('s3', (1, (4, 8, 8)), 'bf16x3-fwd', 'bwd_f16=fs', True, ''), (False, False, False, False, False, None, None, False, None)),
    (('s3', (1, (4, 8, 8)), 'bf16x3-fwd', 'proj_f16x2=', True, ''), (False, False, False, False, False, None, None, False, None)),
    (('s3', (1, (4, 8, 8)), 'bf16x3-fwd', 'proj_f16x2=o', True, ''), (False, False, False, False, False, None, None, False, None)),
    (('s3', (1, (4, 8, 8)), 'bf16x3-fwd', 'proj_f16x2=q', True, ''), (False, False, False, False, False, None, None, False, None)),
    (('s3', (1, (4, 8, 8)), 'bf16x3-fwd', 'qkv_f16=0', True, ''), (False, False, False, False, False, None, None, False, None)),
    (('s3', (1, (4, 8, 8)), 'bf16x3-fwd', 'ff_f16=0', True, ''), (False, False, False, False, False, None, None, False, None)),
    (('s3', (1, (4, 8, 8)), 'bf16x3-fwd', 'AMDNUWA_XATTN6_BWD=0', True, ''), (False, False, False, False, False, None, None, False, None)),
    (('s3', (1, (4, 8, 8)), 'bf16x3-fwd', 'AMDNUWA_XATTN_CM=0', True, ''), (False, False, False, False, False, None, None, False, None)),
    (('s3', (1, (2, 16, 16)), 'bf16x3-fwd', '', False, ''), (False, False, False, True, False, None, None, False, None)),
    (('s3', (1, (4, 8, 8)), 'bf16x3-fwd', '', False, ''), (False, False, False, False, False, None, None, False, None)),
    (('s3', (1, (2, 16, 16)), 'bf16x3-fwd', '', True, 'resid'), (True, False, True, True, True, None, None, False, None)),
    (('s3', (1, (2, 16, 16)), 'bf16x3-fwd', '', True, 'noln'), (False, False, True, True, True, None, None, False, None)),
    (('s3', (1, (4, 8, 8)), 'bf16x3-fwd', '', True, 'resid'), (False, False, False, False, False, None, None, False, None)),
    (('s3', (1, (4, 8, 8)), 'bf16x3-fwd', '', True, 'noln'), (False, False, False, False, False, None, None, False, None)),
    (('ff', (1, 512), 'bf16x3-fwd', '', True, ''), ('only', True, True, False, False, None, None, False, None)),
    (('ff', (1, 512), 'bf16', '', True, ''), (False, False, False, False, False, None, None, False, None)),
    (('ff', (1, 512), 'bf16x3', '', True, ''), (False, False, False, False, False, None, None, False, None)),
    (('ff', (1, 256), 'bf16x3-fwd', '', True, ''), ('only', True, True, False, False, None, None, False, None)),
    (('ff', (1, 256), 'bf16', '', True, ''), (False, False, False, False, False, None, None, False, None)),
    (('ff', (1, 256), 'bf16x3', '', True, ''), (False, False, False, False, False, None, None, False, None)),
    (('ff', (1, 512), 'bf16x3-fwd', 'cores_f16=0', True, ''), ('only', True, True, False, False, None, None, False, None)),
    (('ff', (1, 512), 'bf16x3-fwd', 'xattn6=0', True, ''), ('only', True, True, False, False, None, None, False, None)),
    (('ff', (1, 512), 'bf16x3-fwd', 'xattn_rc=1', True, ''), ('only', True, True, False, False, None, None, False, None)),
    (('ff', (1, 512), 'bf16x3-fwd', 'bwd_f16=', True, ''), (True, False, True, False, False, None, None, False, None)),
    (('ff', (1, 512), 'bf16x3-fwd', 'bwd_f16=f', True, ''), ('only', True, True, False, False, None, None, False, None)),
    (('ff', (1, 512), 'bf16x3-fwd', 'bwd_f16=fs', True, ''), ('only', True, True, False, False, None, None, False, None)),
    (('ff', (1, 512), 'bf16x3-fwd', 'proj_f16x2=', True, ''), ('only', True, True, False, False, None, None, False, None)),
    (('ff', (1, 512), 'bf16x3-fwd', 'proj_f16x2=o', True, ''), ('only', True, True, False, False, None, None, False, None)),
    (('ff', (1, 512), 'bf16x3-fwd', 'proj_f16x2=q', True, ''), ('only', True, True, False, False, None, None, False, None)),
    (('ff', (1, 512), 'bf16x3-fwd', 'qkv_f16=0', True, ''), ('only', True, True, False, False, None, None, False, None)),
    (('ff', (1, 512), 'bf16x3-fwd', 'ff_f16=0', True, ''), (False, False, False, False, False, None, None, False, None)),
    (('ff', (1, 512), 'bf16x3-fwd', 'AMDNUWA_XATTN6_BWD=0', True, ''), ('only', True, True, False, False, None, None, False, None)),
    (('ff', (1, 512), 'bf16x3-fwd', 'AMDNUWA_XATTN_CM=0', True, ''), ('only', True, True, False, False, None, None, False, None)),
    (('ff', (1, 256), 'bf16x3-fwd', 'cores_f16=0', True, ''), ('only', True, True, False, False, None, None, False, None)),
    (('ff', (1, 256), 'bf16x3-fwd', 'xattn6=0', True, ''), ('only', True, True, False, False, None, None, False, None)),
    (('ff', (1, 256), 'bf16x3-fwd', 'xattn_rc=1', True, ''), ('only', True, True, False, False, None, None, False, None)),
    (('ff', (1, 256), 'bf16x3-fwd', 'bwd_f16=', True, ''), (True, False, True, False, False, None, None, False, None)),
    (('ff', (1, 256), 'bf16x3-fwd', 'bwd_f16=f', True, ''), ('only', True, True, False, False, None, None, False, None)),
    (('ff', (1, 256), 'bf16x3-fwd', 'bwd_f16=fs', True, ''), ('only', True, True, False, False, None, None, False, None)),
    (('ff', (1, 256), 'bf16x3-fwd', 'proj_f16x2=', True, ''), ('only', True, True, False, False, None, None, False, None)),
    (('ff', (1, 256), 'bf16x3-fwd', 'proj_f16x2=o', True, ''), ('only', True, True, False, False, None, None, False, None)),
    (('ff', (1, 256), 'bf16x3-fwd', 'proj_f16x2=q', True, ''), ('only', True, True, False, False, None, None, False, None)),
    (('ff', (1, 256), 'bf16x3-fwd', 'qkv_f16=0', True, ''), ('only', True, True, False, False, None, None, False, None)),
    (('ff', (1, 256), 'bf16x3-fwd', 'ff_f16=0', True, ''), (False, False, False, False, False, None, None, False, None)),
    (('ff', (1, 256), 'bf16x3-fwd', 'AMDNUWA_XATTN6_BWD=0', True, ''), ('only', True, True, False, False, None, None, False, None)),
    (('ff', (1, 256), 'bf16x3-fwd', 'AMDNUWA_XATTN_CM=0', True, ''), ('only', True, True, False, False, None, None, False, None)),
    (('ff', (1, 512), 'bf16x3-fwd', '', False, ''), (False, False, False, False, False, None, None, False, None)),
    (('ff', (1, 256), 'bf16x3-fwd', '', False, ''), (False, False, False, False, False, None, None, False, None)),
    (('ff', (1, 512), 'bf16x3-fwd', '', True, 'resid'), (True, False, True, False, False, None, None, False, None)),
    (('ff', (1, 512), 'bf16x3-fwd', '', True, 'noln'), (False, False, True, False, False, None, None, False, None)),
    (('ff', (1, 256), 'bf16x3-fwd', '', True, 'resid'), (True, False, True, False, False, None, None, False, None)),
    (('ff', (1, 256), 'bf16x3-fwd', '', True, 'noln'), (False, False, True, False, False, None, None, False, None)),
    (('xattn', (1, 512, 128, 8, 64), 'bf16', 'xattn6=0', True, ''), (False, False, False, False, False, 'x2_bf16', 'x1', False, 'x2')),
    (('xattn', (1, 512, 128, 8, 64), 'bf16x3', 'xattn6=0', True, ''), (False, False, False, False, False, 'x1_p', 'x1', False, 'x1')),
    (('xattn', (1, 512, 128, 8, 64), 'bf16', 'xattn_rc=1', True, ''), (False, False, False, False, False, 'x6_bf16', 'x1', False, 'x2_rc')),
    (('xattn', (1, 512, 128, 8, 64), 'bf16x3', 'xattn_rc=1', True, ''), (False, False, False, False, False, 'x1_p', 'x1', False, 'x1')),
    (('xattn', (1, 512, 128, 8, 64), 'bf16x3-fwd', '', True, 'rotary'), (False, False, False, False, False, 'x1_stats', 'x1', False, 'x2')),
    (('xattn', (1, 512, 128, 8, 64), 'bf16x3-fwd', '', True, 'nk_bf16'), (True, False, True, True, True, 'x2_f16', 'x1', True, 'x2')),
    (('xattn', (1, 512, 128, 8, 64), 'bf16', '', True, 'rotary'), (False, False, False, False, False, 'x6_bf16', 'x6b', False, 'x6')),
    (('xattn', (1, 512, 128, 8, 64), 'bf16', '', True, 'nk_bf16'), (False, False, False, False, False, 'x2_bf16', 'x1', False, 'x2')),
    (('xattn', (1, 512, 128, 8, 64), 'bf16x3', '', True, 'rotary'), (False, False, False, False, False, 'x1_p', 'x1', False, 'x1')),
    (('xattn', (1, 512, 128, 8, 64), 'bf16x3', '', True, 'nk_bf16'), (False, False, False, False, False, 'x1_p', 'x1', False, 'x1')),
    (('xattn', (2, 48, 48, 8, 64), 'bf16x3-fwd', '', True, 'self_kv'), (False, False, False, True, True, 'x6_f16', 'x1', 'bwd', 'x2')),
    (('xattn', (2, 48, 48, 8, 64), 'bf16x3-fwd', '', True, 'self_kv rotary'), (False, False, False, False, False, 'x1_stats', 'x1', False, 'x2')),
    (('xattn', (2, 48, 48, 8, 64), 'bf16', '', True, 'self_kv'), (False, False, False, False, False, 'x6_bf16', 'x1', 'bwd', 'x2')),
    (('xattn', (2, 48, 48, 8, 64), 'bf16', '', True, 'self_kv rotary'), (False, False, False, False, False, 'x6_bf16', 'x1', 'bwd', 'x2')),
    (('xattn', (2, 48, 48, 8, 64), 'bf16x3', '', True, 'self_kv'), (False, False, False, False, False, 'x1_p', 'x1', False, 'x1')),
    (('xattn', (2, 48, 48, 8, 64), 'bf16x3', '', True, 'self_kv rotary'), (False, False, False, False, False, 'x1_p', 'x1', False, 'x1')),
    (('s3', (1, (2, 16, 16)), 'bf16x3-fwd', '', True, 'rel'), (True, False, True, True, True, None, None, False, None)),
    (('ff', (1, 512), 'bf16x3-fwd', '', True, 'drop'), (True, False, True, False, False, None, None, False, None)),
]


@pytest.fixture(scope='module')
def lib():
    from nuwa_pytorch_amd import _lib
    return _lib.lib()


def _plans(case, monkeypatch):
    kind, geom, mode, switch, wok, flags = case
    monkeypatch.setattr(ops, 'f16_weights_ok', lambda *ws: wok)
    with apply_switch(mode, switch):
        R, D, p, own, pred = build_case(case)
        ln, resid = 'noln' not in flags, 'resid' in flags
        return (ops.block_plan(kind, R, D, p, own, resid, ln), ops.block_plan(kind, R, D, p, pred, resid, ln),
                ops.INNERS[kind].guarded(p))


@pytest.mark.parametrize('row', range(len(TABLE)), ids=lambda i: '-'.join(str(v) for v in TABLE[i][0]).replace(' ', ''))
def test_plan_matches_the_pinned_table(lib, monkeypatch, row):
    case, expected = TABLE[row]
    own, pred, guarded = _plans(case, monkeypatch)
    assert isinstance(own, ops.Plan) and own.guarded == guarded and len(guarded) in (2, 3)
    got = (own.h16, own.bwd16, own.a16, own.core16, own.o16, own.core, own.pack, own.lean, own.bwd)
    assert got == expected, f'{case}: plan {got}, pinned {expected}'
    assert all(type(v) is bool or v == 'only' for v in got[:5]) and (type(own.lean) is bool or own.lean == 'bwd')
    assert own.core is None or (own.core in ops.X_CORES and own.bwd in ops.X_BWDS and own.pack in ('x6b16', 'x6b', 'x1'))
    # ONE decision maker: the predecessor in the chain (next block's meta without its key mask, shift and context copy) gets the same record
    assert pred == own, f'{case}: the predecessor plans {pred}, the block itself {own}'


def test_table_covers_every_route():
    cores = {e[5] for _, e in TABLE if e[5] is not None}
    bwds = {e[8] for _, e in TABLE if e[8] is not None}
    assert cores == set(ops.X_CORES) and bwds == set(ops.X_BWDS)
    assert {e[0] for _, e in TABLE} == {False, True, 'only'}


def test_plan_is_not_cached_across_calls(lib, monkeypatch):
    """modes and switches flip between calls inside one process: the same inputs plan anew every time"""
    case = ('xattn', (1, 512, 128, 8, 64), 'bf16x3-fwd', '', True, '')
    first = _plans(case, monkeypatch)[0]
    other = _plans(case[:3] + ('xattn6=0',) + case[4:], monkeypatch)[0]
    again = _plans(case, monkeypatch)[0]
    assert first == again and first.core == 'x6_f16_only' and other.core == 'x2_f16' and other.bwd == 'x2'


def test_plan_makes_no_transfer_of_its_own(lib, monkeypatch):
    """outside 'bf16x3-fwd' no plan asks for a weight verdict (a verdict costs a device -> host transfer unless prefetched)"""
    asked = []
    case = ('s3', (1, (2, 16, 16)), 'bf16', '', True, '')
    with apply_switch('bf16', ''):
        monkeypatch.setattr(ops, 'f16_weights_ok', lambda *ws: asked.append(ws) or True)
        for kind, geom in (('s3', (1, (2, 16, 16))), ('ff', (1, 512)), ('xattn', (1, 512, 128, 8, 64))):
            R, D, p, own, _ = build_case((kind, geom, 'bf16', '', True, ''))
            ops.block_plan(kind, R, D, p, own)
    assert asked == []


def test_the_chain_hands_over_what_the_block_plans_for_itself(lib, monkeypatch):
    """through SandwichNorm.fused_residual, as Transformer.forward_layers chains it (SandwichBlockFn.apply stubbed): what every block hands
    over about its successor -- (kind, _plan_params(), meta, has_resid) -- plans to the record the successor computes from its own arguments,
    and planning for a Sparse3DNA with a relative-position bias evaluates no bias (no launch, no autograd graph outside the block itself)"""
    torch.manual_seed(0)
    tr = NP.Transformer(dim=DIM, depth=2, causal=True, heads=8, dim_head=64, cross_attend=True, sparse_3dna_attn=True,
                        sparse_3dna_video_shape=(2, 16, 16), sparse_3dna_kernel_size=(3, 3, 3), sparse_3dna_dilations=(1, 2),
                        sparse_3dna_rel_pos_bias=True, shift_video_tokens=True)
    x, ctx = torch.zeros(1, 512, DIM), torch.zeros(1, 128, DIM)
    mask = torch.ones(1, 128, dtype=torch.bool)
    blocks = [(b, kw, b._inner(kw.get('context'), seq_len=512, batch=1)) for attn, cross, ff in tr.layers
              for b, kw in ((attn, {}), (cross, dict(context=ctx, context_mask=mask)), (ff, {}))]
    seen, bias_calls = [], []
    monkeypatch.setattr(ops.SandwichBlockFn, 'apply', staticmethod(lambda x, resid, context, meta, *rest: (seen.append((meta, rest[4:])), x)[1]))
    monkeypatch.setattr(ops, 'f16_weights_ok', lambda *ws: True)
    for s3 in (tr.layers[0][0].fn.fn, tr.layers[1][0].fn.fn):
        monkeypatch.setattr(s3.rel_pos_bias, 'forward', (lambda f: lambda *a, **k: (bias_calls.append(len(seen)), f(*a, **k))[1])(s3.rel_pos_bias.forward))
    with apply_switch('bf16x3-fwd', ''):
        for i, (b, kw, _) in enumerate(blocks):
            nxt = blocks[i + 1] if i + 1 < len(blocks) else None
            b.fused_residual(x, chain=(None, nxt[0] if nxt else None, nxt[2][1] if nxt else None, {}, nxt[1] if nxt else {}), **kw)
        assert bias_calls == [0, 3], bias_calls           # each 3DNA block's own _params(), nobody else's
        kinds = []
        for (meta, _), (own, p) in zip(seen, seen[1:]):
            handed = meta['next_pre'][3]
            assert handed is not None and handed[3] is False
            own = dict(own, shift=None)                   # (SandwichBlockFn.forward: the shift rides in the pre-norm's store)
            mine = ops.block_plan(own['kind'], 512, DIM, p, {k: v for k, v in own.items() if k not in ('handoff_in', 'next_pre', 'handoff_out')})
            assert ops.block_plan(handed[0], 512, DIM, *handed[1:]) == mine, (handed[0], mine)
            kinds.append((handed[0], mine.h16, mine.bwd16))
    assert kinds == [('xattn', 'only', True), ('ff', 'only', True), ('s3', True, False), ('xattn', 'only', True), ('ff', 'only', True)], kinds
