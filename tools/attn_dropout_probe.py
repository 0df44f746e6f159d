#!/usr/bin/env python
"""The audio block of BASELINE cfg 5 with and without attention dropout: SandwichNorm(ShiftAudioTokens(SparseCausal2DNA)) as the fused
residual node (dim 512, 8 heads x 64, window 7, 1 + 320 audio tokens), forward + backward, p = 0 against p = 0.05 (the README's value).
With p > 0 the block draws a [b, 320, 8, 8] keep mask from torch's RNG stream and runs the masked window kernels
(amdnuwa_sparse3dna_fwd_drop / _bwd_drop); with p = 0 it runs the code of the dropout-free path.  The two sides are alternated round by
round; the figure is the median round of each side (HIP events around `--iters` forward + backward calls).

    python tools/attn_dropout_probe.py [--batch 64] [--rounds 7] [--iters 20] [--precision bf16x3-fwd]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nuwa_pytorch_amd as A  # noqa: E402
from nuwa_pytorch_amd import video_audio as VA  # noqa: E402
from nuwa_pytorch_amd.nuwa_pytorch import SandwichNorm  # noqa: E402


def block(p, dev):
    torch.manual_seed(0)
    attn = VA.SparseCausal2DNA(dim=512, heads=8, dim_head=64, kernel_size=7, dilation=1, dropout=p)
    return SandwichNorm(dim=512, fn=VA.ShiftAudioTokens(attn)).to(dev).train()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--precision', default='bf16x3-fwd', choices=['bf16x3-fwd', 'bf16', 'bf16x3'])
    args = ap.parse_args()
    dev = 'cuda'
    A.set_precision(args.precision)
    sides = {0.0: block(0.0, dev), 0.05: block(0.05, dev)}
    g = torch.Generator().manual_seed(1)
    x = torch.randn(args.batch, 321, 512, generator=g).to(dev).requires_grad_(True)
    dy = torch.randn(args.batch, 321, 512, generator=g).to(dev)

    def run(m):
        m.zero_grad(set_to_none=True)
        x.grad = None
        VA._residual(m, x).backward(dy)

    times = {p: [] for p in sides}
    for m in sides.values():                      # warm-up: weight casts, allocator
        for _ in range(3):
            run(m)
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for p, m in sides.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                run(m)
            e1.record()
            torch.cuda.synchronize()
            times[p].append(e0.elapsed_time(e1) / args.iters * 1e3)
    med = {p: statistics.median(t) for p, t in times.items()}
    for p, t in times.items():
        print(f'p = {p:<4}: median {med[p]:8.1f} us per forward + backward   (rounds: {" ".join(f"{v:.1f}" for v in t)})')
    print(f'audio block b = {args.batch}, {args.precision}: dropout 0.05 / dropout 0 = {med[0.05] / med[0.0]:.3f}')


if __name__ == '__main__':
    main()
