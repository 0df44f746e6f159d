#!/usr/bin/env python
"""NUWA.generate past max_video_frames at BASELINE cfg 3 on one MI355X: the whole call with the cache prefill at every slide of the frame
window (generate_slide_cache = True: cached row steps, one full-sequence prefill per extra frame) against the whole call on the
reference's recompute loop (generate_slide_cache = False: what ran before the prefill existed), alternated inside ONE process.
One warm-up call per path (weight caches, workspaces, graph capture), then --alternations rounds of (slide, recompute); every call is timed
between two synchronisations; the table gives every sample, the median and the spread (max - min) per path.
  python tools/gen_long_bench.py [--batch 4] [--extra-frames 2] [--alternations 3] [--out profiles/gen_long_bench.txt]"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nuwa_pytorch_amd as A  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--extra-frames', type=int, default=2)
    ap.add_argument('--alternations', type=int, default=3)
    ap.add_argument('--cond-scale', type=float, default=2.)
    ap.add_argument('--max-frames', type=int, default=10)
    ap.add_argument('--depth', type=int, default=24)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = 'cuda'
    torch.manual_seed(0)
    vae = A.VQGanVAE(dim=64, image_size=256, num_layers=4, vq_codebook_size=8192, use_vgg_and_gan=False)
    nuwa = A.NUWA(vae=vae, dim=512, max_video_frames=args.max_frames, text_max_seq_len=256, text_enc_depth=6, enc_reversible=True,
                  dec_depth=args.depth, dec_heads=8, dec_dim_head=64, sparse_3dna_kernel_size=(5, 3, 3), sparse_3dna_dilation=(1, 2, 4),
                  shift_video_tokens=True).to(dev).eval()
    b, frames = args.batch, args.max_frames + args.extra_frames
    tpf = nuwa.video_fmap_size ** 2
    text = torch.randint(1, 49408, (b, 256), generator=torch.Generator().manual_seed(1)).to(dev)

    def run(slide):
        type(nuwa).generate_slide_cache = slide
        try:
            torch.manual_seed(0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            nuwa.generate(text=text, num_frames=frames, cond_scale=args.cond_scale)
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        finally:
            type(nuwa).generate_slide_cache = True

    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)

    say(f'NUWA.generate(num_frames={frames}) at cfg 3 shape (dim 512, depth {args.depth}, {args.max_frames} x 16 x 16), b = {b}, '
             f"cond_scale = {args.cond_scale}, precision '{A.get_precision()}', {frames * tpf} tokens per sample; seconds per call "
             f'(incl. text encoder, sampling and the VAE decode), {torch.cuda.get_device_name(0)}')
    warm = {s: run(s) for s in (True, False)}
    say(f'warm-up calls (not counted): slide {warm[True]:.2f} s, recompute {warm[False]:.2f} s')
    samples = {True: [], False: []}
    for i in range(args.alternations):
        for s in (True, False):
            samples[s].append(run(s))
        say(f'alternation {i + 1}: slide {samples[True][-1]:.2f} s | recompute {samples[False][-1]:.2f} s')
    med = {s: statistics.median(v) for s, v in samples.items()}
    spread = {s: max(v) - min(v) for s, v in samples.items()}
    say('| path | median s | spread (max - min) s | ms per token |')
    say('|---|---|---|---|')
    for s, name in ((True, 'generate_slide_cache = True (prefill at each slide + row steps)'), (False, 'generate_slide_cache = False (recompute loop)')):
        say(f'| {name} | {med[s]:.2f} | {spread[s]:.2f} | {med[s] / (frames * tpf) * 1e3:.2f} |')
    gain = med[False] - med[True]
    say(f'recompute / slide = {med[False] / med[True]:.2f}x; difference of the medians {gain:.2f} s against a spread of '
                 f'{max(spread.values()):.2f} s: the sliding path {"beats" if gain > max(spread.values()) else "does NOT beat"} the recompute loop by more than the spread')
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
