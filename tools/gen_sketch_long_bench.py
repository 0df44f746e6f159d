#!/usr/bin/env python
"""NUWASketch.generate past max_video_frames on one MI355X, at the configuration of tools/gen_sketch_bench.py (dim 512, 12 decoder layers,
5 x 16 x 16 video tokens, 2 sketch frames, SparseCross2DNA kernel 3): the whole call with the cache prefill at every slide of the frame
window (generate_slide_cache = True: cached row steps, one full-sequence prefill per extra frame, SparseCross2DNA by
amdnuwa_cross2dna_rows) against the whole call on the reference's recompute loop (generate_slide_cache = False: what ran before the rows
form existed), alternated inside ONE process.  One warm-up call per path (weight caches, workspaces, graph capture), then --alternations
rounds of (slide, recompute); every call is timed between two synchronisations; the table gives every sample, the median and the spread
(max - min) per path.  Then ONE prefill on its own: GuidedStepper.prefill over the rows a slide keeps (<bos> + max_frames - 1 frames),
both guidance passes, median of three after a warm-up.
  python tools/gen_sketch_long_bench.py [--batch 4] [--extra-frames 2] [--alternations 3] [--out profiles/gen_sketch_long_bench.txt]"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nuwa_pytorch_amd as A  # noqa: E402
from nuwa_pytorch_amd.decode import GuidedStepper  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--extra-frames', type=int, default=2)
    ap.add_argument('--alternations', type=int, default=3)
    ap.add_argument('--cond-scale', type=float, default=2.)
    ap.add_argument('--max-frames', type=int, default=5)
    ap.add_argument('--depth', type=int, default=12)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = 'cuda'
    torch.manual_seed(0)
    vae = A.VQGanVAE(dim=64, image_size=256, num_layers=4, vq_codebook_size=8192, use_vgg_and_gan=False)
    svae = A.VQGanVAE(dim=64, image_size=256, num_layers=4, vq_codebook_size=1024, use_vgg_and_gan=False)
    m = A.NUWASketch(vae=vae, sketch_vae=svae, dim=512, image_size=256, max_video_frames=args.max_frames, sketch_max_video_frames=2,
                     sketch_enc_depth=2, dec_depth=args.depth, dec_heads=8, dec_dim_head=64, cross_2dna_kernel_size=3, cross_2dna_dilation=2,
                     sparse_3dna_kernel_size=(5, 3, 3), sparse_3dna_dilation=(1, 2, 4)).to(dev).eval()
    b, frames = args.batch, args.max_frames + args.extra_frames
    tpf = m.video_fmap_size ** 2
    g = torch.Generator().manual_seed(1)
    sketch = torch.rand(b, 2, 3, 256, 256, generator=g).to(dev)

    def run(slide):
        type(m).generate_slide_cache = slide
        try:
            torch.manual_seed(0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.generate(sketch=sketch, num_frames=frames, cond_scale=args.cond_scale)
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        finally:
            type(m).generate_slide_cache = True

    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)

    say(f'NUWASketch.generate(num_frames={frames}) at the gen_sketch_bench shape (dim 512, depth {args.depth}, {args.max_frames} x 16 x 16, 2 sketch '
        f"frames), b = {b}, cond_scale = {args.cond_scale}, precision '{A.get_precision()}', {frames * tpf} tokens per sample; seconds per call "
        f'(incl. sketch encoder, sampling and the VAE decode), {torch.cuda.get_device_name(0)}')
    warm = {s: run(s) for s in (True, False)}
    say(f'warm-up calls (not counted): slide {warm[True]:.2f} s, recompute {warm[False]:.2f} s')
    samples = {True: [], False: []}
    for i in range(args.alternations):
        for s in (True, False):
            samples[s].append(run(s))
        say(f'alternation {i + 1}: slide {samples[True][-1]:.2f} s | recompute {samples[False][-1]:.2f} s')
    med = {s: statistics.median(v) for s, v in samples.items()}
    spread = {s: max(v) - min(v) for s, v in samples.items()}
    say('| path | median s | spread (max - min) s | ms per token | spread, ms per token |')
    say('|---|---|---|---|---|')
    per = 1e3 / (frames * tpf)
    for s, name in ((True, 'generate_slide_cache = True (prefill at each slide + row steps)'), (False, 'generate_slide_cache = False (recompute loop)')):
        say(f'| {name} | {med[s]:.2f} | {spread[s]:.2f} | {med[s] * per:.2f} | {spread[s] * per:.2f} |')
    gain = med[False] - med[True]
    say(f'recompute / slide = {med[False] / med[True]:.2f}x; difference of the medians {gain:.2f} s against a spread of '
        f'{max(spread.values()):.2f} s: the sliding path {"beats" if gain > max(spread.values()) else "does NOT beat"} the recompute loop by more than the spread')
    with torch.no_grad():
        ctx, cmask = m.embed_sketch(sketch)
        R = tpf * (args.max_frames - 1) + 1
        ids = torch.randint(0, 8192, (b, R - 1), generator=g).to(dev)
        rows = m.embed_video(ids)
        st = GuidedStepper(m, ctx, cmask, tpf * args.max_frames + 1, args.cond_scale)
        times = []
        for i in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st.prefill(rows)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
    say(f'one prefill (GuidedStepper.prefill, {R} rows per sample, {"both passes" if args.cond_scale != 1 else "one pass"}): '
        f'median {statistics.median(times[1:]) * 1e3:.1f} ms, spread {(max(times[1:]) - min(times[1:])) * 1e3:.1f} ms (first call {times[0] * 1e3:.1f} ms, not counted)')
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
