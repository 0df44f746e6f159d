#!/usr/bin/env python
"""Attention dropout on the SparseCross2DNA kernels (SparseCross2DNA.dropout_on_kernels) against the torch-op route and the dropout-free block.

One block: the fused residual node SandwichNorm(SparseCross2DNA) of the NUWASketch decoder -- 16 x 16 map, 5 video frames (1281 rows),
2 sketch frames (512 context rows, J = 19 slots), dim 512, 8 heads x 64, kernel 3 -- forward + backward, dropout 0.05, at the largest batch
of 128, 64, 32, ... whose torch-op route fits the device (--batch fixes it).
Three sides, alternated round by round (medians and the spread between rounds of HIP-event times around `--iters` calls), peak memory
above the resident tensors of one forward + backward per side:
  torch   dropout_on_kernels = False: SparseCross2DNA._forward_torch, the gathered fp32 keys / values (what the parent commit runs)
  kernel  the default: mask drawn by ops._attn_keep_mask, amdnuwa_cross2dna_fwd_drop / _bwd_drop
  floor   the same block with dropout 0 (amdnuwa_cross2dna_fwd / _bwd)
and `draw`, ops._attn_keep_mask alone at the block's shape: its share of the gap between `kernel` and `floor`.

    python tools/xc2_dropout_probe.py [--batch N] [--rounds 7] [--iters 3] [--precision bf16x3-fwd|bf16]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nuwa_pytorch_amd as A  # noqa: E402
from nuwa_pytorch_amd import ops  # noqa: E402
from nuwa_pytorch_amd.nuwa_pytorch import SandwichNorm, SparseCross2DNA  # noqa: E402

FMAP, FRAMES, SKETCH_FRAMES, DIM, HEADS, DH, KERNEL = 16, 5, 2, 512, 8, 64, 3


def block(p, on_kernels, dev):
    torch.manual_seed(0)
    attn = SparseCross2DNA(dim=DIM, image_size=FMAP, heads=HEADS, dim_head=DH, dropout=p, kernel_size=KERNEL)
    attn.dropout_on_kernels = on_kernels
    return SandwichNorm(dim=DIM, fn=attn).to(dev).train()


def residual(m, x, **kw):
    if m._inner(kw.get('context'), seq_len=x.shape[1], batch=x.shape[0]) is not None:
        return m.fused_residual(x, **kw)
    return x + m(x, **kw)


def measure(args, b, dev):
    n, T, J = 1 + FRAMES * FMAP * FMAP, SKETCH_FRAMES * FMAP * FMAP, SKETCH_FRAMES * KERNEL * KERNEL + 1
    blocks = {'torch': block(args.p, False, dev), 'kernel': block(args.p, True, dev), 'floor': block(0.0, True, dev)}
    assert blocks['torch']._inner(torch.empty(b, T, DIM, device=dev), seq_len=n) is None          # the torch-op route
    assert blocks['kernel']._inner(torch.empty(b, T, DIM, device=dev), seq_len=n) is not None     # the fused node on the masked kernels
    g = torch.Generator().manual_seed(1)
    x = torch.randn(b, n, DIM, generator=g).to(dev).requires_grad_(True)
    dy = torch.randn(b, n, DIM, generator=g).to(dev)
    kw = dict(context=torch.randn(b, T, DIM, generator=g).to(dev).requires_grad_(True), context_mask=(torch.rand(b, T, generator=g) > 0.1).to(dev))

    def run(side):
        if side == 'draw':
            ops._attn_keep_mask(b, n - 1, J, HEADS, args.p, dev)
            return
        m = blocks[side]
        m.zero_grad(set_to_none=True)
        x.grad = None
        kw['context'].grad = None
        residual(m, x, **kw).backward(dy)

    sides = ('torch', 'kernel', 'floor', 'draw')
    peak = {}
    for s in sides:
        for _ in range(2):
            run(s)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        run(s)
        torch.cuda.synchronize()
        peak[s] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    times = {s: [] for s in sides}
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
        print(f'{s:<6}: median {med[s]:10.1f} us, spread {spread[s]:8.1f} us, peak {peak[s]:9.1f} MiB   (rounds: {" ".join(f"{v:.1f}" for v in t)})')
    gap = med['kernel'] - med['floor']
    print(f'xc2 block b = {b}, {n} rows x {T} context rows (J = {J}), p = {args.p}, {args.precision}: kernel / torch = {med["kernel"] / med["torch"]:.3f}, '
          f'kernel / floor = {med["kernel"] / med["floor"]:.3f}, kernel - floor = {gap:.1f} us of which the mask draw {med["draw"]:.1f} us '
          f'({100 * med["draw"] / gap if gap > 0 else float("nan"):.0f} %); peak memory kernel / torch = {peak["kernel"] / peak["torch"]:.3f}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=None)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--p', type=float, default=0.05)
    ap.add_argument('--precision', default='bf16x3-fwd', choices=['bf16x3-fwd', 'bf16'])
    args = ap.parse_args()
    dev = 'cuda'
    A.set_precision(args.precision)
    b = args.batch or 128
    while True:
        try:
            measure(args, b, dev)
            return
        except torch.cuda.OutOfMemoryError:
            if args.batch or b == 1:
                raise
            print(f'b = {b}: the torch-op route does not fit, halving')
            b //= 2
            torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
