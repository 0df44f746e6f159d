#!/usr/bin/env python
"""NUWA.generate under a text of more than 287 tokens on one MI355X: the BASELINE cfg-3 decoder (dim 512, depth 24, 8 heads x 64, 3DNA
kernel (5, 3, 3), 16 x 16 tokens per frame) with text_max_seq_len = 512, b = 4.  generate_long_context_cache = True (the cached row
program, the text keys / values attended in place: amdnuwa_attn_decode_rows per token, amdnuwa_attn_rows in the cache prefill of a window
slide) against generate_long_context_cache = False (the default: such a call runs the reference's recompute loop for every token),
alternated inside ONE process, for a call INSIDE the frame window (num_frames = max_video_frames) and for a call that SLIDES it twice
(num_frames = max_video_frames + 2: 7 frames at the default --max-frames 5).  One warm-up call per (path, call) -- the whole call, because the
recompute loop runs a new shape at every prefix length (a warm-up of one frame left the first timed call at 97 s against 43.5 s for the
next two) -- then --alternations rounds; every call is timed between two synchronisations; the table gives every sample, the median and
the spread (max - min) per path.  Every line is appended to --out as it is printed.  Then ONE prefill on its own: GuidedStepper.prefill over the rows a slide keeps
(<bos> + max_frames - 1 frames), both guidance passes, median of three after a warm-up, next to the key / value bytes the rows form of the
cross-attention re-reads through L2 (every query reads its sample's T rows: B * R * T * 2 * inner elements per image and layer).
  python tools/gen_long_text_bench.py [--batch 4] [--text-len 512] [--max-frames 5] [--alternations 3] [--out profiles/gen_long_text_bench.txt]"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nuwa_pytorch_amd as A  # noqa: E402
from nuwa_pytorch_amd import kernels as K  # noqa: E402
from nuwa_pytorch_amd.decode import GuidedStepper  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--text-len', type=int, default=512)
    ap.add_argument('--extra-frames', type=int, default=2)
    ap.add_argument('--alternations', type=int, default=3)
    ap.add_argument('--cond-scale', type=float, default=2.)
    ap.add_argument('--max-frames', type=int, default=5)
    ap.add_argument('--depth', type=int, default=24)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = 'cuda'
    torch.manual_seed(0)
    vae = A.VQGanVAE(dim=64, image_size=256, num_layers=4, vq_codebook_size=8192, use_vgg_and_gan=False)
    nuwa = A.NUWA(vae=vae, dim=512, max_video_frames=args.max_frames, text_max_seq_len=args.text_len, text_enc_depth=6, enc_reversible=True,
                  dec_depth=args.depth, dec_heads=8, dec_dim_head=64, sparse_3dna_kernel_size=(5, 3, 3), sparse_3dna_dilation=(1, 2, 4),
                  shift_video_tokens=True).to(dev).eval()
    b, T = args.batch, args.text_len
    tpf = nuwa.video_fmap_size ** 2
    calls = (('inside the window', args.max_frames), ('sliding', args.max_frames + args.extra_frames))
    text = torch.randint(1, 49408, (b, T), generator=torch.Generator().manual_seed(1)).to(dev)

    def run(cached, frames):
        type(nuwa).generate_long_context_cache = cached
        try:
            torch.manual_seed(0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            nuwa.generate(text=text, num_frames=frames, cond_scale=args.cond_scale)
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        finally:
            type(nuwa).generate_long_context_cache = False

    if args.out:
        open(args.out, 'w').close()

    def say(line):
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(line + '\n')

    say(f'NUWA.generate under a text of {T} tokens at the cfg 3 decoder shape (dim 512, depth {args.depth}, {args.max_frames} x 16 x 16), b = {b}, '
        f"cond_scale = {args.cond_scale}, precision '{A.get_precision()}'; seconds per call (incl. text encoder, sampling and the VAE decode), "
        f'{torch.cuda.get_device_name(0)}')
    med, spread = {}, {}
    for what, frames in calls:
        warm = {c: run(c, frames) for c in (True, False)}
        say(f'{what} (num_frames = {frames}, {frames * tpf} tokens per sample): warm-up calls (not counted): cached {warm[True]:.2f} s, '
            f'recompute {warm[False]:.2f} s')
        samples = {True: [], False: []}
        for i in range(args.alternations):
            for c in (True, False):
                samples[c].append(run(c, frames))
            say(f'  alternation {i + 1}: cached {samples[True][-1]:.2f} s | recompute {samples[False][-1]:.2f} s')
        for c in (True, False):
            med[what, c], spread[what, c] = statistics.median(samples[c]), max(samples[c]) - min(samples[c])
    say('| call | path | median s | spread (max - min) s | ms per token | spread, ms per token |')
    say('|---|---|---|---|---|---|')
    for what, frames in calls:
        per = 1e3 / (frames * tpf)
        for c, name in ((True, 'generate_long_context_cache = True (cached rows)'), (False, 'generate_long_context_cache = False (recompute loop, the default)')):
            say(f'| {what}, {frames} frames | {name} | {med[what, c]:.2f} | {spread[what, c]:.2f} | {med[what, c] * per:.2f} | {spread[what, c] * per:.2f} |')
    for what, frames in calls:
        gain, worst = med[what, False] - med[what, True], max(spread[what, True], spread[what, False])
        say(f'{what}: recompute / cached = {med[what, False] / med[what, True]:.2f}x; difference of the medians {gain:.2f} s against a spread of '
            f'{worst:.2f} s: the cached path {"beats" if gain > worst else "does NOT beat"} the recompute loop by more than the spread')
    with torch.no_grad():
        mask = text != 0
        ctx = nuwa.embed_text(text, mask=mask)
        R = tpf * (args.max_frames - 1) + 1
        ids = torch.randint(0, 8192, (b, R - 1), generator=torch.Generator().manual_seed(2)).to(dev)
        rows = nuwa.embed_video(ids)
        st = GuidedStepper(nuwa, ctx, mask, tpf * args.max_frames + 1, args.cond_scale, long_context=True)
        times = []
        for i in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st.prefill(rows)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
    images = 2 if K.want_lo() else 1
    # the conditioned pass alone re-reads keys: on the text-masked pass the output row is a constant and nothing is launched
    gbytes = b * R * T * 2 * 512 * 2 * images * args.depth / 1e9
    pre = statistics.median(times[1:])
    say(f'one prefill (GuidedStepper.prefill, {R} rows per sample, {"both passes" if args.cond_scale != 1 else "one pass"}): median '
        f'{pre * 1e3:.1f} ms, spread {(max(times[1:]) - min(times[1:])) * 1e3:.1f} ms (first call {times[0] * 1e3:.1f} ms, not counted)')
    say(f'  key / value bytes its {args.depth} amdnuwa_attn_rows calls re-read through L2 (b * R * T * 2 * inner elements, {images} image(s) of 2 bytes, '
        f'per layer): {gbytes:.1f} GB in all = {gbytes / pre / 1e3:.2f} TB/s if the prefill did nothing else')
    slide = med['sliding', True]
    say(f'  {args.extra_frames} prefills = {args.extra_frames * pre:.3f} s of the sliding call\'s {slide:.2f} s ({100 * args.extra_frames * pre / slide:.1f} %)')


if __name__ == '__main__':
    main()
