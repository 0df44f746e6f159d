#!/usr/bin/env python
"""The two VQ code lookups side by side (csrc/vae.hip): cosine (amdnuwa_vq_argmax_ws) and Euclidean (amdnuwa_vq_nearest_l2), one device,
R = 20480 rows (80 frames x 16 x 16), codebook 8192 x 256 -- the cfg-3 tokenizer's lookup.

    python tools/vq_lookup_probe.py [--rounds 7] [--window 0.5] [--warmup 20]
        after a warm-up the two lookups run ALTERNATELY, `rounds` times each, every run a window of back-to-back calls of at least
        `window` seconds between two HIP events (the call count is fixed from a calibration run, the same for every window of a
        lookup).  Prints ms per call of every window, the medians, and the spread (max - min) / median of the repeated cosine windows:
        the yardstick the Euclidean lookup is read against is the cosine kernel of the same process, not itself.  Both issue the same
        MFMAs; the Euclidean one adds a subtraction per staged element and the prep pass (column mean + centred code norms, two reads
        of the 8 MB codebook).
    rocprofv3 --kernel-trace --stats -d DIR -o vq --output-format csv -- python tools/vq_lookup_probe.py --trace
        a short run (warm-up + 20 calls of each) for the kernel trace: the per-kernel statistics give the prep pass's own time
        (vq_l2_colsum_kernel + vq_l2_mean_kernel + vq_l2_half_kernel) next to vq_inv_norm_kernel of the cosine lookup"""
import argparse
import os
import statistics
import sys

R, CN, DC = 20480, 8192, 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--window', type=float, default=0.5, help='seconds per timed window, at least')
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--trace', action='store_true', help='warm-up + 20 calls of each lookup, no timing windows')
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import torch.nn.functional as F
    from nuwa_pytorch_amd import kernels as K
    dev = 'cuda'
    g = torch.Generator().manual_seed(0)
    cb = torch.randn(CN, DC, generator=g)
    x = (cb[torch.randint(0, CN, (R,), generator=g)] + 0.5 * torch.randn(R, DC, generator=g)).to(dev)
    cb = cb.to(dev)
    cbn = F.normalize(cb, dim=-1)
    lookups = {'cosine': lambda: K.vq_argmax(x, cbn), 'euclidean': lambda: K.vq_nearest_l2(x, cb)}

    def window(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / calls

    for fn in lookups.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    if args.trace:
        for fn in lookups.values():
            window(fn, 20)
        return
    calls = {name: max(20, int(args.window * 1e3 / window(fn, 20)) + 1) for name, fn in lookups.items()}
    ms = {name: [] for name in lookups}
    for _ in range(args.rounds):
        for name, fn in lookups.items():
            ms[name].append(window(fn, calls[name]))
    print(f'R = {R}, codebook {CN} x {DC}; {args.rounds} alternating windows of >= {args.window} s each')
    for name in lookups:
        print(f'{name:9s} ({calls[name]} calls per window) ms per call: ' + ' '.join(f'{v:.4f}' for v in ms[name]))
    med = {name: statistics.median(v) for name, v in ms.items()}
    spread = (max(ms['cosine']) - min(ms['cosine'])) / med['cosine']
    print(f'median: cosine {med["cosine"]:.4f} ms, euclidean {med["euclidean"]:.4f} ms, difference {1e3 * (med["euclidean"] - med["cosine"]):+.1f} us '
          f'({100 * (med["euclidean"] / med["cosine"] - 1):+.2f} %); spread of the cosine windows {100 * spread:.2f} % = {1e3 * spread * med["cosine"]:.1f} us')


if __name__ == '__main__':
    main()
