#!/usr/bin/env python
"""Dropout keep masks from torch's RNG draw ('torch') against the Philox generator kernels of csrc/keepmask.hip ('device'):
ops.set_keep_mask_source, one call on one MI355X.

The three producers alone, at the shapes of BASELINE cfg 3 at b = 128 (--batch), p = 0.05:
  ff      ops._ff_keep_mask      the FeedForward gate: 128 x 2560 rows x the padded gate width of a dim-512 FeedForward
  window  ops._attn_keep_mask    the video window mask: [128, 2560, 46, 8] (window (5, 3, 3) + <bos>, 8 heads)
  cattn   ops._cattn_keep_mask   the text cross-attention: 2561 queries x 256 keys (+ the null slot), 8 heads: keep, keep_t, keep0
then the fused SandwichNorm(Attention) block of tools/cattn_dropout_probe.py (dim 512, 8 x 64, 2561 x 256, dropout_on_kernels, forward +
backward) with its mask from either source.  The two sides are alternated round by round; medians and the spread (max - min) between rounds
of HIP-event times around `--iters` calls; peak memory above the resident tensors of one call per side.

    python tools/keep_mask_probe.py [--batch 128] [--rounds 7] [--iters 5] [--p 0.05] [--precision bf16x3-fwd|bf16]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nuwa_pytorch_amd as A  # noqa: E402
from nuwa_pytorch_amd import ops  # noqa: E402
from cattn_dropout_probe import block, residual  # noqa: E402

SIDES = ('torch', 'device')


def measure(name, what, run, rounds, iters):
    """run(): one call under the current source.  Prints one line per side and the ratio"""
    peak, times = {}, {s: [] for s in SIDES}
    for s in SIDES:
        ops.set_keep_mask_source(s)
        for _ in range(2):
            run()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        run()
        torch.cuda.synchronize()
        peak[s] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    for _ in range(rounds):
        for s in SIDES:
            ops.set_keep_mask_source(s)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                run()
            e1.record()
            torch.cuda.synchronize()
            times[s].append(e0.elapsed_time(e1) / iters * 1e3)
    ops.set_keep_mask_source('torch')
    med = {s: statistics.median(t) for s, t in times.items()}
    print(f'{name}: {what}')
    for s in SIDES:
        t = times[s]
        print(f'  {s:<6}: median {med[s]:10.1f} us, spread {max(t) - min(t):8.1f} us, peak {peak[s]:9.1f} MiB   (rounds: {" ".join(f"{v:.1f}" for v in t)})')
    print(f'  device / torch = {med["device"] / med["torch"]:.3f} in time, {peak["device"] / peak["torch"]:.3f} in peak memory; '
          f'torch - device = {med["torch"] - med["device"]:.1f} us')
    return med, peak


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--p', type=float, default=0.05)
    ap.add_argument('--precision', default='bf16x3-fwd', choices=['bf16x3-fwd', 'bf16'])
    args = ap.parse_args()
    dev = torch.device('cuda')
    A.set_precision(args.precision)
    b, p = args.batch, args.p
    FFI = A.FeedForward(dim=512).net[3].weight.shape[1]
    FP = (FFI + 31) // 32 * 32
    R = b * 2560
    measure('ff', f'_ff_keep_mask({R}, {FP})  [{R * FP / 1e6:.0f} M entries]', lambda: ops._ff_keep_mask(R, FP, p, dev), args.rounds, args.iters)
    measure('window', f'_attn_keep_mask({b}, 2560, 46, 8)  [{b * 2560 * 46 * 8 / 1e6:.0f} M entries]',
            lambda: ops._attn_keep_mask(b, 2560, 46, 8, p, dev), args.rounds, args.iters)
    n, T = 2561, 256
    draw, _ = measure('cattn', f'_cattn_keep_mask({b}, {n}, {T}, 8)  [{b * n * (T + 1) * 8 / 1e6:.0f} M decisions, 2 x {b * n * T / 1e6:.0f} MB of mask]',
                      lambda: ops._cattn_keep_mask(b, n, T, 8, p, dev), args.rounds, args.iters)
    m = block(p, False, True, dev)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(b, n, 512, generator=g).to(dev).requires_grad_(True)
    dy = torch.randn(b, n, 512, generator=g).to(dev)
    ctx = torch.randn(b, T, 512, generator=g).to(dev).requires_grad_(True)
    cm = (torch.rand(b, T, generator=g) > 0.1).to(dev)

    def step():
        m.zero_grad(set_to_none=True)
        x.grad = ctx.grad = None
        residual(m, x, context=ctx, context_mask=cm).backward(dy)
    blk, _ = measure('block', f'SandwichNorm(Attention) b = {b}, {n} x {T}, dropout = {p}, {args.precision}, forward + backward on the masked cattn kernels',
                     step, args.rounds, args.iters)
    print(f'block: torch - device = {blk["torch"] - blk["device"]:.1f} us; the producer alone: {draw["torch"] - draw["device"]:.1f} us')


if __name__ == '__main__':
    main()
