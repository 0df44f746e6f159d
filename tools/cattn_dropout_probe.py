#!/usr/bin/env python
"""Attention dropout on the linear-memory cattn kernels (Attention.dropout_on_kernels) against the torch-op route and the dropout-free block.

Two blocks, each the fused residual node SandwichNorm(Attention) at dim 512, 8 heads x 64, forward + backward, dropout 0.05:
  cross   the text cross-attention block of BASELINE cfg 3: 2561 rows over a 256-key context, b = 128 (--batch)
  causal  the plain causal self-attention block: 1024 rows, b = 8
Three sides, alternated round by round (medians and the spread between rounds of HIP-event times around `--iters` calls), peak memory
above the resident tensors of one forward + backward per side:
  torch   live dropout as shipped: Attention._forward_torch (what the parent commit runs)
  kernel  dropout_on_kernels = True: mask drawn by ops._cattn_keep_mask, the masked cattn kernels
  floor   the same block with dropout 0 (cross: the xattn6 kernels, causal: the unmasked cattn kernels)
and `draw`, ops._cattn_keep_mask alone at the block's shape: its share of the gap between `kernel` and `floor`.

    python tools/cattn_dropout_probe.py [--block cross|causal] [--batch N] [--rounds 7] [--iters 5] [--precision bf16x3-fwd|bf16]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nuwa_pytorch_amd as A  # noqa: E402
from nuwa_pytorch_amd import ops  # noqa: E402
from nuwa_pytorch_amd.nuwa_pytorch import Attention, SandwichNorm  # noqa: E402


def block(p, causal, on_kernels, dev):
    torch.manual_seed(0)
    attn = Attention(dim=512, heads=8, dim_head=64, causal=causal, dropout=p)
    attn.dropout_on_kernels = on_kernels
    return SandwichNorm(dim=512, fn=attn).to(dev).train()


def residual(m, x, **kw):
    if m._inner(kw.get('context'), seq_len=x.shape[1], batch=x.shape[0]) is not None:
        return m.fused_residual(x, **kw)
    return x + m(x, **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--block', default='cross', choices=['cross', 'causal'])
    ap.add_argument('--batch', type=int, default=None)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--p', type=float, default=0.05)
    ap.add_argument('--precision', default='bf16x3-fwd', choices=['bf16x3-fwd', 'bf16'])
    args = ap.parse_args()
    dev = 'cuda'
    A.set_precision(args.precision)
    causal = args.block == 'causal'
    b = args.batch or (8 if causal else 128)
    n, T = (1024, 1024) if causal else (2561, 256)
    blocks = {'torch': block(args.p, causal, False, dev), 'kernel': block(args.p, causal, True, dev), 'floor': block(0.0, causal, False, dev)}
    g = torch.Generator().manual_seed(1)
    x = torch.randn(b, n, 512, generator=g).to(dev).requires_grad_(True)
    dy = torch.randn(b, n, 512, generator=g).to(dev)
    kw = {}
    if not causal:
        kw['context'] = torch.randn(b, T, 512, generator=g).to(dev).requires_grad_(True)
        kw['context_mask'] = (torch.rand(b, T, generator=g) > 0.1).to(dev)

    def run(side):
        if side == 'draw':
            ops._cattn_keep_mask(b, n, T, 8, args.p, dev)
            return
        m = blocks[side]
        m.zero_grad(set_to_none=True)
        x.grad = None
        if not causal:
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
    print(f'{args.block} block b = {b}, {n} x {T}, p = {args.p}, {args.precision}: kernel / torch = {med["kernel"] / med["torch"]:.3f}, '
          f'kernel / floor = {med["kernel"] / med["floor"]:.3f}, kernel - floor = {gap:.1f} us of which the mask draw {med["draw"]:.1f} us '
          f'({100 * med["draw"] / gap if gap > 0 else float("nan"):.0f} %); peak memory kernel / torch = {peak["kernel"] / peak["torch"]:.3f}')


if __name__ == '__main__':
    main()
