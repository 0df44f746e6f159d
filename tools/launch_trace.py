"""Which kernels.py wrappers does a training step call, in which order, on which operand forms -- and what does it compute?

    python tools/launch_trace.py run --out DIR [--root CHECKOUT] [--models a,b,...] [--hash]
    python tools/launch_trace.py compare DIR_A DIR_B

`run` wraps every public function defined in nuwa_pytorch_amd/kernels.py and records, in call order, each call that receives a tensor: the wrapper's
name, dtype and shape of every tensor argument (for a BF which of hi / lo / f16 it carries), the scalar arguments.  The host-side queries
(`*_ok`, `*_supported`, `bf_rows_cols`) launch nothing and are left out.  It then runs a matrix of small seeded models forward and backward -- every model under
the three precision modes and, around the defaults, one A/B switch at a time -- and writes DIR/trace.json plus every output, input gradient and
parameter gradient (DIR/<key>.pt; --hash: the SHA-256 of their bytes in DIR/tensors.json instead, for runs whose tensors need not be kept).
--root names the checkout whose package is imported (default: the one this file is in), so ONE copy of this file serves two commits: it
touches only names both have.  `compare` wants equal key sets, equal traces and bit-identical tensors, and lists what differs.
Run it once per commit, each in a fresh process."""
import argparse
import contextlib
import hashlib
import inspect
import json
import os
import re
import sys

import torch

MODES = ('bf16x3-fwd', 'bf16', 'bf16x3')
SWITCHES = ('cores_f16=0', 'xattn6=0', 'xattn_rc=1', 'bwd_f16=', 'bwd_f16=f', 'bwd_f16=fs', 'proj_f16x2=', 'proj_f16x2=o', 'proj_f16x2=q',
            'qkv_f16=0', 'ff_f16=0', 'AMDNUWA_XATTN6_BWD=0', 'AMDNUWA_XATTN_CM=0')
X_SWITCHES = ('xattn6=0', 'xattn_rc=1', 'AMDNUWA_XATTN6_BWD=0', 'AMDNUWA_XATTN_CM=0')        # the ones 'bf16' listens to as well
CONFIGS = [(m, '') for m in MODES] + [(MODES[0], s) for s in SWITCHES] + [('bf16', s) for s in X_SWITCHES]
_SET = dict(cores_f16='set_cores_f16', xattn6='set_xattn6', xattn_rc='set_xattn_rc', bwd_f16='set_bwd_f16', proj_f16x2='set_proj_f16x2',
            qkv_f16='set_qkv_f16', ff_f16='set_ff_f16')
_STATE = ('_PRECISION', '_CORES_F16', '_XATTN6', '_XATTN_RC', '_BWD_F16', '_PROJ_F16X2', '_QKV_F16', '_FF_F16')
_ENV = ('AMDNUWA_XATTN6_BWD', 'AMDNUWA_XATTN_CM')
QUERY = re.compile(r'(_ok|_supported)$|^bf_rows_cols$')          # host-side queries: they launch nothing
DEV = 'cuda'


@contextlib.contextmanager
def config(K, mode, switch):
    """the precision mode and ONE switch away from the defaults; everything restored on exit"""
    saved, env = {k: getattr(K, k) for k in _STATE}, {k: os.environ.get(k) for k in _ENV}
    try:
        K.set_precision(mode)
        K.set_cores_f16(True), K.set_xattn6(True), K.set_xattn_rc(False), K.set_bwd_f16(K.DEFAULT_BWD_F16), K.set_proj_f16x2(K.DEFAULT_F16X2)
        K.set_qkv_f16(True), K.set_ff_f16(True)
        for k in _ENV:
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


# ---- the recorder -------------------------------------------------------------------------------------

class Recorder:
    def __init__(self, K, ops):
        self.K, self.on, self.calls, self.handed = K, False, [], None
        # the disagreement guards of SandwichBlockFn.forward, recorded directly: while a block runs that was offered a hand-off, a pre-norm
        # ln_fwd of its own ('guard:recomputed') or an fp16 conversion OF the handed tensor ('guard:converted') is marked in the trace
        fwd = ops.SandwichBlockFn.forward

        def forward(ctx, x, resid, context, meta, *rest):
            hin = meta.get('handoff_in')
            self.handed = hin.get('h') if hin else None
            try:
                return fwd(ctx, x, resid, context, meta, *rest)
            finally:
                self.handed = None
        ops.SandwichBlockFn.forward = staticmethod(forward)
        for name, fn in list(vars(K).items()):
            if inspect.isfunction(fn) and fn.__module__ == K.__name__ and not name.startswith('_') and not QUERY.search(name):
                setattr(K, name, self._wrap(name, fn))

    def describe(self, v):
        """(description, does it hold a tensor)"""
        K = self.K
        if isinstance(v, torch.Tensor):
            return f'{str(v.dtype)[6:]}{list(v.shape)}', True
        if isinstance(v, K.BF):
            return {'BF': {k: self.describe(t)[0] for k, t in zip(('hi', 'lo', 'f16'), v) if t is not None}}, True
        if isinstance(v, K.G16):
            return {'G16': self.describe(v.t)[0]}, True
        if isinstance(v, (tuple, list)):
            d = [self.describe(t) for t in v]
            return [t[0] for t in d], any(t[1] for t in d)
        if v is None or isinstance(v, (bool, int, float, str)):
            return v, False
        f16 = getattr(v, 'f16', None)
        return type(v).__name__ + ('.f16' if f16 is True else ''), False

    def _wrap(self, name, fn):
        def wrapped(*a, **k):
            if self.on and self.handed is not None and ((name == 'ln_fwd' and 'shift' in k) or (name == 'hilo_to_f16' and a[0] is self.handed)):
                self.calls.append(['guard:recomputed' if name == 'ln_fwd' else 'guard:converted', [], {}])
            if self.on:
                da, dk = [self.describe(v) for v in a], {n: self.describe(v) for n, v in k.items()}
                if any(t[1] for t in da) or any(t[1] for t in dk.values()):
                    self.calls.append([name, [t[0] for t in da], {n: t[0] for n, t in dk.items()}])
            return fn(*a, **k)
        wrapped.__wrapped__ = fn
        return wrapped

    @contextlib.contextmanager
    def record(self):
        self.on, self.calls = True, []
        try:
            yield self.calls
        finally:
            self.on = False


# ---- the models -----------------------------------------------------------------------------------------

def _stack(M, cls='Transformer', heads=8, T=128, **kw):
    """-> step(): (dict of named tensors).  Models (a) ... (g): a depth-2 decoder stack at dim 512 on a 2 x 16 x 16 token grid, batch 1"""
    torch.manual_seed(0)
    chain = kw.pop('chain_blocks', True)
    scale_ff = kw.pop('scale_ff', None)
    tr = getattr(M, cls)(dim=512, depth=2, causal=True, heads=heads, dim_head=64, cross_attend=True, sparse_3dna_attn=True,
                         sparse_3dna_video_shape=(2, 16, 16), sparse_3dna_kernel_size=(3, 3, 3), sparse_3dna_dilations=(1, 2),
                         shift_video_tokens=True, **kw).to(DEV).train()
    if not chain:
        tr.chain_blocks = False
    if scale_ff is not None:            # layer 0's FeedForward weights outside the fp16 range: that block runs the hi + lo products
        ff = tr.layers[0][2].fn.fn
        with torch.no_grad():
            ff.net[0].weight.mul_(scale_ff / float(ff.net[0].weight.abs().max()))
            ff.net[3].weight.mul_(1.0 / scale_ff)
    g = torch.Generator().manual_seed(1)
    x0, c0 = torch.randn(1, 512, 512, generator=g).to(DEV), torch.randn(1, T, 512, generator=g).to(DEV)
    mask = (torch.rand(1, T, generator=g) > 0.25).to(DEV)
    wout = torch.randn(1, 512, 512, generator=g).to(DEV)

    def step():
        x, c = x0.clone().requires_grad_(True), c0.clone().requires_grad_(True)
        out = tr(x, context=c, context_mask=mask)
        (out * wout).sum().backward()
        return tr, dict(out=out, dx=x.grad, dcontext=c.grad)
    return step


def _tiny_nuwa(A, reversible):
    """model (h): the tiny NUWA of tests/test_gpu_modules.py -- dim 32 (every block on the hi + lo forms), text encoder with rotary self-attention"""
    torch.manual_seed(0)
    vae = A.VQGanVAE(dim=32, image_size=16, num_layers=2, vq_codebook_size=64, vq_codebook_dim=32, use_vgg_and_gan=False)
    nuwa = A.NUWA(vae=vae, dim=32, text_num_tokens=50, text_max_seq_len=8, max_video_frames=3, text_enc_depth=2,
                  dec_depth=3, enc_reversible=True, dec_reversible=reversible, dec_heads=2, dec_dim_head=32,
                  text_enc_heads=2, text_enc_dim_head=16, sparse_3dna_kernel_size=3, sparse_3dna_dilation=(1, 2)).to(DEV).train()
    g = torch.Generator().manual_seed(10)
    text, vid = torch.randint(1, 50, (2, 8), generator=g).to(DEV), torch.randint(0, 64, (2, 3, 4, 4), generator=g).to(DEV)

    def step():
        loss = nuwa(text=text, video=vid, return_loss=True, cond_dropout_prob=0.)
        loss.backward()
        return nuwa, dict(loss=loss)
    return step


def _alone(M, which):
    """model (i): one module on its own (ops.InnerFn) at the shapes of model (a)"""
    torch.manual_seed(0)
    if which == 's3':
        mod = M.Sparse3DNA(dim=512, video_shape=(2, 16, 16), kernel_size=(3, 3, 3), dilation=1, heads=8, dim_head=64, causal=True)
    else:
        mod = M.Attention(dim=512, heads=8, dim_head=64) if which == 'xattn' else M.FeedForward(dim=512, mult=4)
    mod = mod.to(DEV).train()
    g = torch.Generator().manual_seed(1)
    x0, c0 = torch.randn(1, 512, 512, generator=g).to(DEV), torch.randn(1, 128, 512, generator=g).to(DEV)
    mask = (torch.rand(1, 128, generator=g) > 0.25).to(DEV)
    wout = torch.randn(1, 512, 512, generator=g).to(DEV)

    def step():
        x, c = x0.clone().requires_grad_(True), c0.clone().requires_grad_(True)
        out = mod(x, context=c, context_mask=mask) if which == 'xattn' else mod(x)
        (out * wout).sum().backward()
        return mod, dict(out=out, dx=x.grad, **(dict(dcontext=c.grad) if which == 'xattn' else {}))
    return step


def models(A, M):
    return {
        'a': lambda: _stack(M),
        'a_rel': lambda: _stack(M, sparse_3dna_rel_pos_bias=True),
        'b': lambda: _stack(M, T=64),
        'c': lambda: _stack(M, heads=4),
        'd': lambda: _stack(M, ff_dropout=0.1),
        'e': lambda: _stack(M, scale_ff=2.0e5),
        'f': lambda: _stack(M, chain_blocks=False),
        'g': lambda: _stack(M, cls='ReversibleTransformer'),
        'h_plain': lambda: _tiny_nuwa(A, False),
        'h_reversible': lambda: _tiny_nuwa(A, True),
        'i_s3': lambda: _alone(M, 's3'),
        'i_xattn': lambda: _alone(M, 'xattn'),
        'i_ff': lambda: _alone(M, 'ff'),
    }


# ---- run / compare ---------------------------------------------------------------------------------------

def _sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()


def run(args):
    sys.path.insert(0, os.path.abspath(args.root))
    import nuwa_pytorch_amd as A
    from nuwa_pytorch_amd import kernels as K, nuwa_pytorch as M, ops
    assert os.path.abspath(A.__file__).startswith(os.path.abspath(args.root) + os.sep), f'imported {A.__file__}, not the checkout {args.root}'
    os.makedirs(args.out, exist_ok=True)
    rec = Recorder(K, ops)
    traces, hashes = {}, {}
    todo = models(A, M)
    for name in (args.models.split(',') if args.models else todo):
        step = todo[name]()
        for mode, switch in CONFIGS:
            key = f'{name}|{mode}|{switch}'
            with config(K, mode, switch):
                torch.manual_seed(1234)              # (FeedForward dropout draws its masks from torch's stream)
                with rec.record() as calls:
                    mod, outs = step()
                torch.cuda.synchronize()
            outs = {k: v.detach() for k, v in outs.items()}
            outs.update({'grad.' + n: p.grad.detach() for n, p in mod.named_parameters() if p.grad is not None})
            traces[key] = calls
            if args.hash:
                hashes[key] = {k: _sha(v) for k, v in outs.items()}
            else:
                torch.save({k: v.cpu() for k, v in outs.items()}, os.path.join(args.out, key.replace('|', '__') + '.pt'))
            mod.zero_grad(set_to_none=True)
            print(f'{key}: {len(calls)} calls, {len(outs)} tensors', flush=True)
        del step
        torch.cuda.empty_cache()
    json.dump(traces, open(os.path.join(args.out, 'trace.json'), 'w'))
    if args.hash:
        json.dump(hashes, open(os.path.join(args.out, 'tensors.json'), 'w'))


def _tensors(d, key):
    f = os.path.join(d, 'tensors.json')
    if os.path.exists(f):
        return json.load(open(f))[key], (lambda a, b: a == b)
    return torch.load(os.path.join(d, key.replace('|', '__') + '.pt')), torch.equal


def guards(calls):
    """(pre-norms recomputed although a hand-off was offered, hi + lo hand-offs converted to fp16) of one run: the Recorder's own marks"""
    return sum(1 for c in calls if c[0] == 'guard:recomputed'), sum(1 for c in calls if c[0] == 'guard:converted')


def compare(args):
    ta, tb = ({k: [c for c in v if not QUERY.search(c[0])] for k, v in json.load(open(os.path.join(d, 'trace.json'))).items()} for d in (args.a, args.b))
    print(f'keys: {len(ta)} / {len(tb)}; only in A: {sorted(set(ta) - set(tb))}; only in B: {sorted(set(tb) - set(ta))}')
    for side, t in (('A', ta), ('B', tb)):
        took = {k: guards(c) for k, c in t.items() if any(guards(c))}
        print(f'{side}: runs that took a hand-off guard (pre-norms recomputed, hi + lo hand-offs converted to fp16): {took if took else "none"}')
    bad_trace = bad_tensor = ncalls = ntensors = 0
    for key in sorted(set(ta) & set(tb)):
        ca, cb = ta[key], tb[key]
        ncalls += len(ca)
        diff = [i for i in range(max(len(ca), len(cb))) if i >= len(ca) or i >= len(cb) or ca[i] != cb[i]]
        if diff:
            bad_trace += len(diff)
            i = diff[0]
            print(f'TRACE {key}: {len(ca)} / {len(cb)} calls, {len(diff)} differ; first at {i}:\n   A {ca[i] if i < len(ca) else None}\n   B {cb[i] if i < len(cb) else None}')
        (xa, eq), (xb, _) = _tensors(args.a, key), _tensors(args.b, key)
        ntensors += len(xa)
        if set(xa) != set(xb):
            print(f'TENSORS {key}: names differ: {sorted(set(xa) ^ set(xb))}')
            bad_tensor += len(set(xa) ^ set(xb))
        wrong = [n for n in sorted(set(xa) & set(xb)) if not eq(xa[n], xb[n])]
        if wrong:
            bad_tensor += len(wrong)
            print(f'TENSORS {key}: {len(wrong)} of {len(xa)} differ: {wrong[:6]}')
    print(f'{len(set(ta) & set(tb))} runs, {ncalls} trace entries, {ntensors} tensors: {bad_trace} differing trace entries, {bad_tensor} differing tensors')
    return 1 if bad_trace or bad_tensor or set(ta) != set(tb) else 0


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    sub = ap.add_subparsers(dest='cmd', required=True)
    r = sub.add_parser('run')
    r.add_argument('--out', required=True)
    r.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    r.add_argument('--models', default='')
    r.add_argument('--hash', action='store_true')
    c = sub.add_parser('compare')
    c.add_argument('a')
    c.add_argument('b')
    a = ap.parse_args()
    sys.exit(run(a) if a.cmd == 'run' else compare(a))
