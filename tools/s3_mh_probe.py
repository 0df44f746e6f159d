#!/usr/bin/env python
"""What a head costs on the many-head Sparse3DNA window kernels (csrc/sparse3dna_mh.hip): forward and backward time of the core alone
(kernels.sparse3dna_mh_fwd / _bwd) at the decoder grid (10, 16, 16), window (5, 3, 3), batch 8, with 16 x 64 and 12 x 64 heads, in both
operand forms (bf16, hi + lo pairs) -- next to the existing 8-head VALU window kernels on the same grid run TWICE (2 x 8 heads = the
arithmetic of 16 heads; tuning keys 3 = 1 and 4 = 1 keep the bf16 form off the MFMA band kernels, so VALU stands against VALU).

Method: every side is warmed up, then the sides are alternated round by round; a round times `--iters` calls between two HIP events; the
figure is the median round of each side, with the spread between rounds next to it.  Inputs are fixed random operands; nothing is
compared here (tests/test_gpu_s3_mh.py holds the values).

    python tools/s3_mh_probe.py [--batch 8] [--rounds 7] [--iters 10] [--out profiles/s3_mh_probe.txt]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nuwa_pytorch_amd import _lib, kernels as K  # noqa: E402

GRID, WINDOW, DIL = (10, 16, 16), (5, 3, 3), (1, 1, 1)
DEV = 'cuda'


def pair(t, hilo):
    hi = t.to(torch.bfloat16)
    return K.BF(hi.contiguous(), (t - hi.float()).to(torch.bfloat16).contiguous() if hilo else None)


def side(heads, hilo, B, mh, calls):
    """-> (forward(), backward()) closures of one side: `calls` core calls of `heads` heads each"""
    n, d = 1 + GRID[0] * GRID[1] * GRID[2], 64
    inner = heads * d
    gen = torch.Generator().manual_seed(heads)
    qkv = pair(torch.randn(B * n, 3 * inner, generator=gen).to(DEV), hilo)
    dO = pair(torch.randn(B * n, inner, generator=gen).to(DEV), hilo)
    wth = (torch.randn(heads, heads, generator=gen) * 0.5 + torch.eye(heads)).to(DEV)
    g = K.s3_geom(B, n, GRID, WINDOW, DIL, heads, d, causal=True)
    fwd, bwd = (K.sparse3dna_mh_fwd, K.sparse3dna_mh_bwd) if mh else (K.sparse3dna_fwd, K.sparse3dna_bwd)

    def f():
        for _ in range(calls):
            fwd(g, qkv, wth)

    def b():
        for _ in range(calls):
            bwd(g, qkv, wth, dO)
    return f, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    L = _lib.lib()
    lines = [f'Sparse3DNA core, grid {GRID}, window {WINDOW}, batch {a.batch}, dim_head 64; median of {a.rounds} rounds x {a.iters} calls, '
             f'microseconds per call (min .. max over the rounds); {torch.cuda.get_device_name(0)}']
    for hilo in (False, True):
        sides = {'mh 16 heads': side(16, hilo, a.batch, True, 1), 'mh 12 heads': side(12, hilo, a.batch, True, 1),
                 '8-head VALU x 2': side(8, hilo, a.batch, False, 2), '8-head VALU x 1': side(8, hilo, a.batch, False, 1)}
        L.amdnuwa_set_tuning(3, 1)
        L.amdnuwa_set_tuning(4, 1)
        try:
            times = {(s, k): [] for s in sides for k in (0, 1)}
            for s, fb in sides.items():
                for k in (0, 1):
                    for _ in range(2):
                        fb[k]()
            torch.cuda.synchronize()
            for _ in range(a.rounds):
                for s, fb in sides.items():
                    for k in (0, 1):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(a.iters):
                            fb[k]()
                        e1.record()
                        torch.cuda.synchronize()
                        times[(s, k)].append(e0.elapsed_time(e1) / a.iters * 1e3)
        finally:
            L.amdnuwa_set_tuning(3, 0)
            L.amdnuwa_set_tuning(4, 0)
        lines.append(f'--- operands: {"hi + lo pairs" if hilo else "bf16"}')
        for s in sides:
            f, b = times[(s, 0)], times[(s, 1)]
            lines.append(f'{s:18s} forward {statistics.median(f):9.1f} ({min(f):.1f} .. {max(f):.1f})   backward {statistics.median(b):9.1f} ({min(b):.1f} .. {max(b):.1f})')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(text)


if __name__ == '__main__':
    main()
