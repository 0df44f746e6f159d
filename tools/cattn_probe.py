#!/usr/bin/env python
"""Plain attention on the linear-memory cattn kernels against the torch-op formulation, in one process.

Times forward + backward of ONE `Attention(dim=512, heads=8, dim_head=64)` through the module's kernel path and through
`Attention._forward_torch` (the PyTorch-ROCm formulation the module ran before the cattn kernels took the shape), alternating, after
warm-up, device-synchronised (one HIP-event pair per iteration), and prints the peak memory of each above the baseline.  Causal
self-attention by default; --no-causal: non-causal self-attention over the n rows; --keys T (implies --no-causal): n queries over a
context of T rows, with its gradient.  --layers L times a whole non-causal `Transformer(dim=512, depth=L)` over n tokens instead (the
sketch encoder's stack), its long-key blocks as fused cattn nodes against the same stack on torch ops.  --xm C (with --keys CC, --frames F)
times `CrossModalityCrossAttention(dim=512, chunk_size=C, context_chunk_size=CC)` over F frames instead: batch * F samples of C queries
x CC keys on the cattn kernels against the module with use_hip=False (the torch-op path).

    python tools/cattn_probe.py [--batch 8] [--n 2561] [--keys T] [--no-causal] [--layers L] [--xm C --frames F] [--iters 20] [--warmup 3]
                                [--mode bf16x3-fwd] [--kernels-only] [--json PATH]

--kernels-only runs just the kernel path (e.g. under `rocprofv3 --kernel-trace --stats`).  The MFMA roof fraction quoted is the algorithmic
FLOP count of the visible (query, key) pairs (kernels._c_work: 2 products forward, 5 backward) over 2.5 PFLOP/s dense bf16 / fp16."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nuwa_pytorch_amd as A  # noqa: E402
from nuwa_pytorch_amd import kernels as K  # noqa: E402

MFMA_ROOF = 2.5e15


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--n', type=int, default=2561)
    ap.add_argument('--keys', type=int, default=None, help='rows of a context the n queries attend (non-causal)')
    ap.add_argument('--no-causal', action='store_true')
    ap.add_argument('--layers', type=int, default=0, help='time a non-causal Transformer of this depth instead of one module')
    ap.add_argument('--xm', type=int, default=0, help='chunk_size of a CrossModalityCrossAttention (context_chunk_size = --keys)')
    ap.add_argument('--frames', type=int, default=10)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--mode', default='bf16x3-fwd')
    ap.add_argument('--kernels-only', action='store_true')
    ap.add_argument('--json', default=None)
    args = ap.parse_args()
    dev = 'cuda'
    torch.manual_seed(0)
    A.set_precision(args.mode)
    causal = not (args.no_causal or args.keys is not None or args.layers)
    if args.xm:                                              # F frames of C queries; the context: its start token + F - 1 frames of CC rows
        assert args.keys is not None, '--xm needs --keys (the context_chunk_size)'
        args.n, n_ctx = 1 + args.frames * args.xm, 1 + (args.frames - 1) * args.keys
    else:
        n_ctx = args.keys
    x = torch.randn(args.batch, args.n, 512, device=dev, requires_grad=True)
    dy = torch.randn(args.batch, args.n, 512, device=dev)
    ctx = torch.randn(args.batch, n_ctx, 512, device=dev, requires_grad=True) if args.keys is not None else None
    T = args.keys if args.keys is not None else args.n
    from nuwa_pytorch_amd.nuwa_pytorch import Attention
    shipped = (Attention.long_pairs_min, Attention.long_wgs_min)
    Attention.long_pairs_min = Attention.long_wgs_min = 0        # the probe times the kernels at any shape; the shipped gate's verdict is printed
    if args.xm:
        from nuwa_pytorch_amd.video_audio import CrossModalityCrossAttention as XM
        shipped = (XM.long_pairs_min, XM.long_wgs_min)
        XM.long_pairs_min = XM.long_wgs_min = 0
        m = XM(dim=512, chunk_size=args.xm, context_chunk_size=T, heads=8, dim_head=64).to(dev)
        with torch.no_grad():
            m.talking_heads.bias.normal_(0, 0.3)
        assert m._long_hip_ok(args.batch * args.frames, args.xm, T), 'the module would not take the kernel path at this shape / in this mode'

        def xm_path(hip):
            def fn(t):
                m.use_hip = hip
                return m(t, ctx)
            return fn
        kernel_fn, torch_fn = xm_path(True), xm_path(False)
    elif args.layers:
        assert ctx is None, '--layers times a self-attention stack'
        m = A.Transformer(dim=512, depth=args.layers, heads=8, dim_head=64).to(dev)
        routed = Attention._long_hip_ok

        def torch_stack(t):
            Attention._long_hip_ok = lambda self, *a, **k: False
            try:
                return m(t)
            finally:
                Attention._long_hip_ok = routed
        kernel_fn, torch_fn = m, torch_stack
        assert m.layers[0][0].fn._long_hip_ok(T), 'the stack would not take the kernel path at this length / in this mode'
    else:
        m = A.Attention(dim=512, heads=8, dim_head=64, causal=causal).to(dev)
        assert m._causal_hip_ok(args.n) if causal else m._long_hip_ok(T), 'the module would not take the kernel path at this shape / in this mode'
        kw = {} if ctx is None else dict(context=ctx)
        kernel_fn, torch_fn = (lambda t: m(t, **kw)), (lambda t: m._forward_torch(t, **kw))

    def step(fn):
        m.zero_grad(set_to_none=True)
        x.grad = None
        if ctx is not None:
            ctx.grad = None
        y = fn(x)
        y.backward(dy)

    paths = [('cattn', kernel_fn)] + ([] if args.kernels_only else [('torch', torch_fn)])
    times, peaks = {k: [] for k, _ in paths}, {}
    for name, fn in paths:                                   # warm-up + peak memory, one path at a time
        for _ in range(args.warmup):
            step(fn)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        step(fn)
        torch.cuda.synchronize()
        peaks[name] = torch.cuda.max_memory_allocated() - base
    for _ in range(args.iters):                              # alternate the two paths
        for name, fn in paths:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            step(fn)
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1))
    if args.xm:                                              # the kernels' view: batch * frames samples of C queries x CC keys
        args.batch, args.n = args.batch * args.frames, args.xm
    g = K.cattn_geom(args.batch, args.n, 8, 64, causal=causal, n_keys=args.keys)
    flops = (K._c_work('fwd')((g,), {}, None)[0] + K._c_work('bwd')((g,), {}, None)[0]) * max(args.layers, 1)
    if not causal:
        takes = args.batch * args.n * T >= shipped[0] and args.batch * min(-(-args.n // 64), -(-T // 64)) >= shipped[1]
        print(f'the shipped gate (pairs >= {shipped[0]}, workgroups per side >= {shipped[1]}) routes this shape to: ' + ('the kernels' if takes else 'torch ops'))
    res = dict(batch=args.batch, n=args.n, keys=T, xm=bool(args.xm), causal=causal, layers=args.layers, mode=args.mode, iters=args.iters, core_flops=flops)
    for name, _ in paths:
        t = times[name]
        res[name] = dict(ms_median=statistics.median(t), ms_min=min(t), ms_max=max(t), peak_bytes=peaks[name])
        print(f'{name:6s} forward + backward: median {statistics.median(t):9.3f} ms  (min {min(t):.3f}, max {max(t):.3f}, {len(t)} iterations)   '
              f'peak above the baseline {peaks[name] / 1e6:10.1f} MB')
    if 'torch' in res:
        res['ratio'] = res['torch']['ms_median'] / res['cattn']['ms_median']
        print(f"torch / cattn = {res['ratio']:.2f} x")
    # the module time includes the three projections and their gradients (a stack's: the feed-forward blocks and the norms too); the per-kernel split comes from a profiler run (--kernels-only)
    res['roof_fraction_whole_module'] = flops / (res['cattn']['ms_median'] * 1e-3) / MFMA_ROOF
    print(f"core FLOPs (visible pairs) {flops / 1e9:.1f} G  ->  {res['roof_fraction_whole_module'] * 100:.2f} % of the MFMA roof over the WHOLE time")
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, 'w') as f:
            json.dump(res, f, indent=1)
    A.set_precision('bf16')


if __name__ == '__main__':
    main()
