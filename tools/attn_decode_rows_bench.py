#!/usr/bin/env python
"""The single-query attention kernel over cached rows (amdnuwa_attn_decode_rows, csrc/decode.hip) alone: 8 heads x 64, one query per
sample over T rows of a [B, T, 1024] key | value cache, with the talking-heads bias, hi-only and hi + lo operands.

    python tools/attn_decode_rows_bench.py [--iters 50] [--warmup 5]
        runs every (T, B, form) of CONFIGS in order, warmup + iters launches each, and prints the time per launch between two HIP events
        around the iters launches (back to back: launch overhead included where the kernels are shorter than it)
    rocprofv3 --kernel-trace --stats -d DIR -o rows --output-format csv -- python tools/attn_decode_rows_bench.py
    python tools/attn_decode_rows_bench.py --summarize DIR/.../rows_kernel_trace.csv
        the kernel time proper: the three kernels of a launch (statistics, apply, reduce) summed, median over the iters launches of each
        configuration (taken from the trace in launch order), against the bytes the launch must read -- 2 * T * inner * 2 B per sample,
        twice with lo -- as GB/s, with the split count."""
import argparse
import csv
import os
import statistics
import sys

CONFIGS = [(T, B, lo) for T in (400, 1024, 4096) for B in (2, 8) for lo in (False, True)]
HEADS, DH = 8, 64
KERNELS = ('rows_stats_kernel', 'rows_apply_kernel', 'rows_reduce_kernel')


def bytes_read(T, B, lo):
    return B * 2 * T * HEADS * DH * 2 * (2 if lo else 1)


def splits(T):
    return -(-(T + 1) // 128)


def summarize(path, iters, warmup):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            name = r['Kernel_Name']
            if any(k in name for k in KERNELS):
                rows.append((int(r['Start_Timestamp']), int(r['End_Timestamp']) - int(r['Start_Timestamp'])))
    rows.sort()
    per = 3 * (iters + warmup)
    assert len(rows) == per * len(CONFIGS), f'{len(rows)} kernel records, expected {per * len(CONFIGS)}'
    print('T      B  form    splits  us/launch (median; stats + apply + reduce)   MB read   GB/s')
    for i, (T, B, lo) in enumerate(CONFIGS):
        d = [x[1] for x in rows[i * per:(i + 1) * per]]
        launches = [sum(d[3 * j:3 * j + 3]) for j in range(warmup, warmup + iters)]
        parts = [statistics.median(d[3 * j + k] for j in range(warmup, warmup + iters)) / 1e3 for k in range(3)]
        us = statistics.median(launches) / 1e3
        nb = bytes_read(T, B, lo)
        print(f'{T:5d} {B:2d}  {"hi+lo" if lo else "hi   "}  {splits(T):6d}  {us:8.2f}  ({parts[0]:.2f} + {parts[1]:.2f} + {parts[2]:.2f})'
              f'   {nb / 1e6:8.2f}  {nb / us / 1e3:7.1f}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--summarize', default=None, help='a rocprofv3 kernel-trace csv of a run of this tool with the same --iters / --warmup')
    args = ap.parse_args()
    if args.summarize:
        return summarize(args.summarize, args.iters, args.warmup)
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from nuwa_pytorch_amd import kernels as K
    dev, inner = 'cuda', HEADS * DH
    torch.manual_seed(0)
    nk, nv = torch.randn(HEADS, DH, device=dev), torch.randn(HEADS, DH, device=dev)
    wth = torch.randn(HEADS, HEADS, device=dev) * 0.5 + torch.eye(HEADS, device=dev)
    bias = torch.randn(HEADS, device=dev) * 0.3
    first = torch.zeros(1, dtype=torch.int32, device=dev)
    for T, B, lo in CONFIGS:
        mk = lambda *s: K.BF(torch.randn(*s, device=dev).bfloat16(), torch.randn(*s, device=dev).bfloat16() * 2 ** -9 if lo else None)
        q, kv = mk(B, inner), mk(B, T, 2 * inner)
        run = lambda: K.attn_decode_rows(q, kv, first, T, HEADS, DH, nk, nv, wth, th_bias=bias)
        for _ in range(args.warmup):
            run()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            run()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / args.iters
        print(f'T={T} B={B} {"hi+lo" if lo else "hi"}: {splits(T)} splits, {us:.1f} us per launch between events (3 kernels back to back), '
              f'{bytes_read(T, B, lo) / 1e6:.2f} MB to read')


if __name__ == '__main__':
    main()
