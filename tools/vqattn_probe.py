#!/usr/bin/env python
"""The VQGanAttention core alone (amdnuwa_vqattn_core / amdnuwa_vqattn_core_rel, csrc/vae.hip) on N = 80 images, 8 heads x 64, and
the whole block (VQGanVAE._hip_module) against the torch-op VQGanAttention.forward on the same GPU.

    python tools/vqattn_probe.py [--iters 50] [--warmup 5]
        runs every configuration of CONFIGS in order, warmup + iters launches each, and prints the time per launch between two HIP
        events (launch overhead included where the kernel is shorter than it)
    rocprofv3 --kernel-trace --stats -d DIR -o vq --output-format csv -- python tools/vqattn_probe.py
    python tools/vqattn_probe.py --summarize DIR/.../vq_kernel_trace.csv
        the kernel time proper: median over the iters launches of each configuration (taken from the trace in launch order), and the
        rate 4 N heads P^2 c FLOP / time against the 157 TF fp32 matrix peak
    python tools/vqattn_probe.py --block [--iters 10]
        whole-block time at dim 512, S = 20 and 32, N = 8: _hip_module(attn) (conv, l2norm, core, conv, LayerNormChan) against
        VQGanAttention.forward in torch ops -- the only route on those shapes before the tiled kernel (HIP events, mean per call)"""
import argparse
import csv
import os
import statistics
import sys

N, HEADS, DH = 80, 8, 64
PEAK_TF = 157.0
# (side, bias form, tuning key 15)
CONFIGS = [(17, 'bias', 0), (17, 'bias', 2), (20, 'table', 0), (32, 'table', 0), (32, 'bias', 0), (64, 'table', 0)]
KERNELS = ('vqattn_core_kernel', 'vqattn_mfma_kernel', 'vqattn_tiled_kernel')


def flop(S):
    return 4.0 * N * HEADS * (S * S) ** 2 * DH


def label(S, form, key):
    P = S * S
    kernel = 'tiled' if key == 2 or 2 * DH * P * 4 > 160 * 1024 or form == 'table' else ('mfma' if P == 256 else 'VALU')
    return f'{S:2d} x {S:<2d} (P = {P:4d})  {form:5s}  {kernel:5s}'


def summarize(path, iters, warmup):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            if any(k in r['Kernel_Name'] for k in KERNELS):
                rows.append((int(r['Start_Timestamp']), int(r['End_Timestamp']) - int(r['Start_Timestamp']), r['Kernel_Name']))
    rows.sort()
    per = iters + warmup
    assert len(rows) == per * len(CONFIGS), f'{len(rows)} kernel records, expected {per * len(CONFIGS)}'
    print(f'N = {N} images, {HEADS} x {DH}; median of {iters} launches (rocprofv3 kernel trace)')
    print('map                   bias   kernel    us/launch    TF/s   of 157 TF peak')
    for i, (S, form, key) in enumerate(CONFIGS):
        us = statistics.median(x[1] for x in rows[i * per + warmup:(i + 1) * per]) / 1e3
        tf = flop(S) / us / 1e6
        print(f'{label(S, form, key)}  {us:10.1f}  {tf:6.1f}   {100 * tf / PEAK_TF:5.1f} %')


def block(iters, warmup):
    import torch
    import nuwa_pytorch_amd as A
    from nuwa_pytorch_amd.vqgan_vae import VQGanAttention
    dev = 'cuda'
    vae = A.VQGanVAE(dim=32, image_size=32, num_layers=2, vq_codebook_size=64, vq_codebook_dim=16, use_vgg_and_gan=False)
    print('whole block, dim 512, 8 x 64, N = 8 images: ms per call (HIP events, mean)')
    for S in (20, 32):
        torch.manual_seed(S)
        m = VQGanAttention(dim=512, dim_head=DH, heads=HEADS).eval().to(dev)
        x = torch.randn(8, 512, S, S, device=dev)
        res = {}
        with torch.no_grad():
            for name, fn in (('hip', lambda: vae._hip_module(m, x)), ('torch ops', lambda: m(x))):
                for _ in range(warmup):
                    fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                res[name] = e0.elapsed_time(e1) / iters
        print(f'S = {S}: _hip_module {res["hip"]:.3f} ms, torch ops {res["torch ops"]:.3f} ms ({res["torch ops"] / res["hip"]:.2f} x)')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--summarize', default=None, help='a rocprofv3 kernel-trace csv of a run of this tool with the same --iters / --warmup')
    ap.add_argument('--block', action='store_true')
    args = ap.parse_args()
    if args.summarize:
        return summarize(args.summarize, args.iters, args.warmup)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if args.block:
        return block(args.iters, args.warmup)
    import torch
    import torch.nn.functional as F
    from nuwa_pytorch_amd import _lib, kernels as K
    dev = 'cuda'
    L = _lib.lib()
    for S, form, key in CONFIGS:
        P = S * S
        torch.manual_seed(S)
        qkv = torch.randn(N, 3, HEADS * DH, P, device=dev)
        qkv[:, :2] = F.normalize(qkv[:, :2], dim=-1)
        qkv = qkv.reshape(N, 3 * HEADS * DH, P).contiguous()
        scale = torch.full((HEADS,), 5.0, device=dev)
        kw = dict(bias=torch.randn(HEADS, P, P, device=dev)) if form == 'bias' else dict(rel_table=torch.randn(HEADS, 2 * S - 1, 2 * S - 1, device=dev))
        run = lambda: K.vqattn_core(qkv, scale, HEADS, **kw)
        L.amdnuwa_set_tuning(15, key)
        try:
            for _ in range(args.warmup):
                run()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                run()
            e1.record()
            torch.cuda.synchronize()
        finally:
            L.amdnuwa_set_tuning(15, 0)
        us = e0.elapsed_time(e1) * 1e3 / args.iters
        print(f'{label(S, form, key)}: {us:.1f} us per launch between events, {flop(S) / us / 1e6:.1f} TF/s')


if __name__ == '__main__':
    main()
