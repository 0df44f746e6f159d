#!/usr/bin/env python
"""The audio block of BASELINE cfg 5 with and without attention dropout: SandwichNorm(ShiftAudioTokens(SparseCausal2DNA)) as the fused
residual node (dim 512, 8 heads x 64, window 7, 1 + 320 audio tokens), forward + backward, p = 0 against p = 0.05 (the README's value).
With p > 0 the block draws a [b, 320, 8, 8] keep mask from torch's RNG stream and runs the masked window kernels
(amdnuwa_sparse3dna_fwd_drop / _bwd_drop); with p = 0 it runs the code of the dropout-free path.  The two sides are alternated round by
round; the figure is the median round of each side (HIP events around `--iters` forward + backward calls).

    python tools/attn_dropout_probe.py [--batch 64] [--rounds 7] [--iters 20] [--precision bf16x3-fwd]

--block video: the video block of cfg 3 at its own shape, SandwichNorm(ShiftVideoTokens(Sparse3DNA)) on 1 + 10 x 16 x 16 tokens (dim 512, 8 heads
x 64, window (5, 3, 3), --dilation 1 / 2 / 4) -- a geometry of the MFMA band kernels.  Three sides, alternated round by round: dropout 0 (the
floor), p = 0.05 on the masked VALU window kernels (tuning key 26 = 1: the block then also gets the bare plan, as before the band kernels
had masked forms) and p = 0.05 on the masked band kernels (the plan of the dropout-free block).  Medians and the spread between rounds.

    python tools/attn_dropout_probe.py --block video [--batch 32] [--dilation 1] [--precision bf16x3-fwd | bf16]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nuwa_pytorch_amd as A  # noqa: E402
from nuwa_pytorch_amd import video_audio as VA  # noqa: E402
from nuwa_pytorch_amd import _lib, kernels as K, ops  # noqa: E402
from nuwa_pytorch_amd.nuwa_pytorch import SandwichNorm, ShiftVideoTokens, Sparse3DNA  # noqa: E402


def block(p, dev):
    torch.manual_seed(0)
    attn = VA.SparseCausal2DNA(dim=512, heads=8, dim_head=64, kernel_size=7, dilation=1, dropout=p)
    return SandwichNorm(dim=512, fn=VA.ShiftAudioTokens(attn)).to(dev).train()


def video_block(p, dev, dilation):
    torch.manual_seed(0)
    attn = Sparse3DNA(dim=512, video_shape=(10, 16, 16), kernel_size=(5, 3, 3), dilation=dilation, heads=8, dim_head=64, causal=True, dropout=p)
    return SandwichNorm(dim=512, fn=ShiftVideoTokens(attn, image_size=16)).to(dev).train()


def video(args):
    """floor / VALU route / band route of the cfg-3 video block"""
    dev, L = 'cuda', _lib.lib()
    blocks = {'floor': video_block(0.0, dev, args.dilation), 'drop': video_block(0.05, dev, args.dilation)}
    g = torch.Generator().manual_seed(1)
    n = 1 + 10 * 16 * 16
    x = torch.randn(args.batch, n, 512, generator=g).to(dev).requires_grad_(True)
    dy = torch.randn(args.batch, n, 512, generator=g).to(dev)
    plan0, s3f16 = ops.S3Inner.plan, K.s3_f16_supported

    def run(side):
        m = blocks['floor' if side == 'floor' else 'drop']
        m.zero_grad(set_to_none=True)
        x.grad = None
        if side == 'valu':      # the route before the band kernels had masked forms: key 26 in the library, the bare plan in the block
            L.amdnuwa_set_tuning(26, 1)
            ops.S3Inner.plan = staticmethod(lambda R, D, p, meta, has_resid=False, ln=True: ops.Plan(guarded=ops.S3Inner.guarded(p)))
        try:
            VA._residual(m, x).backward(dy)
        finally:
            L.amdnuwa_set_tuning(26, 0)
            ops.S3Inner.plan = staticmethod(plan0)

    sides = ('floor', 'valu', 'band')
    times = {s: [] for s in sides}
    for s in sides:
        for _ in range(3):
            run(s)
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for s in sides:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                run(s)
            e1.record()
            torch.cuda.synchronize()
            times[s].append(e0.elapsed_time(e1) / args.iters * 1e3)
    med = {s: statistics.median(t) for s, t in times.items()}
    spread = {s: max(t) - min(t) for s, t in times.items()}
    for s, t in times.items():
        print(f'{s:<5}: median {med[s]:9.1f} us per forward + backward, spread {spread[s]:7.1f} us   (rounds: {" ".join(f"{v:.1f}" for v in t)})')
    print(f'video block b = {args.batch}, dilation {args.dilation}, {args.precision}: band / floor = {med["band"] / med["floor"]:.3f}, '
          f'valu / floor = {med["valu"] / med["floor"]:.3f}, valu - band = {med["valu"] - med["band"]:.1f} us '
          f'(largest spread between rounds {max(spread.values()):.1f} us)')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--block', default='audio', choices=['audio', 'video'])
    ap.add_argument('--dilation', type=int, default=1)
    ap.add_argument('--batch', type=int, default=None)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--precision', default='bf16x3-fwd', choices=['bf16x3-fwd', 'bf16', 'bf16x3'])
    args = ap.parse_args()
    dev = 'cuda'
    A.set_precision(args.precision)
    if args.batch is None:
        args.batch = 64 if args.block == 'audio' else 32
    if args.block == 'video':
        return video(args)
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
