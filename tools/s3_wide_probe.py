#!/usr/bin/env python
"""Sparse3DNA window kernels on a grid wider than one workgroup row (the column-tiled kernels of csrc/sparse3dna_wide.hip) beside the row
kernels of csrc/sparse3dna.hip on the 16-wide grid, same window, same batch: forward and backward microseconds per query token.

    python tools/s3_wide_probe.py [--batch 8] [--iters 10] [--fmaps 16,32] [--kernels-only]

(10, 32, 32) and (10, 16, 16), 8 heads x 64, kernel (5, 3, 3), dilation 2; the 16-wide runs keep the MFMA band kernels off (tuning keys 3 = 1 and
4 = 1) so that both sides run the VALU window kernels.  Per token the tiled form stages (TW + halo) / TW of the row form's columns: 20 / 16 here.
--kernels-only: a few launches of each, for `rocprofv3 --kernel-trace --stats -- python tools/s3_wide_probe.py --kernels-only`."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nuwa_pytorch_amd import kernels as K, _lib  # noqa: E402
from attn_bench import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--fmaps', default='16,32', help='grid widths to time (16 alone runs on a library without the tiled kernels)')
    ap.add_argument('--kernels-only', action='store_true')
    a = ap.parse_args()
    L = _lib.lib()
    heads, dh, kern, dil, b = 8, 64, (5, 3, 3), (2, 2, 2), a.batch
    inner = heads * dh
    torch.manual_seed(0)
    wth = (torch.randn(heads, heads, device='cuda') * 0.3 + torch.eye(heads, device='cuda')).contiguous()
    L.amdnuwa_set_tuning(3, 1)
    L.amdnuwa_set_tuning(4, 1)
    res = {}
    fmaps = [int(v) for v in a.fmaps.split(',')]
    for fmap in fmaps:
        shape = (10, fmap, fmap)
        nq = shape[0] * fmap * fmap
        n = nq + 1
        g = K.s3_geom(b, n, shape, kern, dil, heads, dh)
        for lo in (False, True):
            hi = torch.randn(b * n, 3 * inner, device='cuda')
            qkv = K.BF(hi.to(torch.bfloat16), (hi * 2 ** -9).to(torch.bfloat16) if lo else None)
            d = torch.randn(b * n, inner, device='cuda')
            do = K.BF(d.to(torch.bfloat16), (d * 2 ** -9).to(torch.bfloat16) if lo else None)
            if a.kernels_only:
                for _ in range(3):
                    K.sparse3dna_fwd(g, qkv, wth)
                    K.sparse3dna_bwd(g, qkv, wth, do)
                torch.cuda.synchronize()
                continue
            tf = bench(lambda: K.sparse3dna_fwd(g, qkv, wth), a.iters)
            tb = bench(lambda: K.sparse3dna_bwd(g, qkv, wth, do), a.iters)
            res[(fmap, lo)] = (tf * 1e6 / (b * nq) * 1e3, tb * 1e6 / (b * nq) * 1e3)
            print(f'(10,{fmap},{fmap}) b={b} {"hi+lo" if lo else "bf16 "}: fwd {tf * 1e6:8.1f} us = {res[(fmap, lo)][0]:6.2f} ns/token   '
                  f'bwd {tb * 1e6:8.1f} us = {res[(fmap, lo)][1]:6.2f} ns/token', flush=True)
            del qkv, do, hi, d
    L.amdnuwa_set_tuning(3, 0)
    L.amdnuwa_set_tuning(4, 0)
    if not a.kernels_only and fmaps == [16, 32]:
        for lo in (False, True):
            f = res[(32, lo)][0] / res[(16, lo)][0]
            bw = res[(32, lo)][1] / res[(16, lo)][1]
            print(f'{"hi+lo" if lo else "bf16 "}: per token, 32-wide / 16-wide = fwd {f:.2f}x  bwd {bw:.2f}x   (staged columns: 20 / 16 = 1.25x)')


if __name__ == '__main__':
    main()
