#!/usr/bin/env python
"""SparseCross2DNA rows of the cached NUWASketch.generate: the in-place kernel (amdnuwa_cross2dna_decode, one launch per row and layer)
against the gather + pack + amdnuwa_xattn_decode path it replaces (AMDNUWA_XC2_DECODE_PACKED=1), on one MI355X.

Time per guided token of the cached + graph path (decode.GuidedStepper, graph=True: what NUWASketch.generate runs per token; rows >= 2
are graph replays) of a dim-512 model, 12 decoder layers of 8 heads x 64, 16 x 16 token maps, b = 4, for two windows:
  * 2 sketch frames x 3 x 3 = 18 slots (the default window),
  * 5 sketch frames x 5 x 5 = 125 slots.
Per window ONE process builds the model once and alternates the two sides of the switch, `--rounds` repeats interleaved; each repeat
builds a fresh stepper (the switch is read there), runs rows 0 and 1 untimed (row 1 captures the graph) and times `--tokens` further rows
with the host clock around device-synchronised work.  The spread between the repeats of one side is the noise of the comparison.

    python tools/sketch_decode_probe.py [--rounds 5] [--tokens 400] [--batch 4] [--step-timeout 240] [--out FILE]

Without --window the tool is the driver: it starts one child process per window, each under its own `timeout`, stops at the first child
that fails, and writes the table (and the rule's verdict for the default of windows the packed path can hold) to --out."""
import argparse
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WINDOWS = {18: dict(frames=2, kernel=3, dilation=2), 125: dict(frames=5, kernel=5, dilation=1)}
SIDES = (('in place', '0'), ('packed', '1'))


def measure(slots, batch, tokens, rounds):
    import torch
    import nuwa_pytorch_amd as A
    from nuwa_pytorch_amd.decode import GuidedStepper
    assert torch.cuda.is_available(), 'the probe measures on the GPU'
    w, dev = WINDOWS[slots], 'cuda'
    torch.manual_seed(0)
    vae = A.VQGanVAE(dim=64, image_size=256, num_layers=4, vq_codebook_size=8192, use_vgg_and_gan=False)
    svae = A.VQGanVAE(dim=64, image_size=256, num_layers=4, vq_codebook_size=1024, use_vgg_and_gan=False)
    m = A.NUWASketch(vae=vae, sketch_vae=svae, dim=512, image_size=256, max_video_frames=5, sketch_max_video_frames=w['frames'],
                     sketch_enc_depth=2, dec_depth=12, dec_heads=8, dec_dim_head=64, cross_2dna_kernel_size=w['kernel'],
                     cross_2dna_dilation=w['dilation'], sparse_3dna_kernel_size=(5, 3, 3), sparse_3dna_dilation=(1, 2, 4)).to(dev).eval()
    g = torch.Generator().manual_seed(1)
    sids = torch.randint(0, 1024, (batch, w['frames'] * 256), generator=g).to(dev)
    m.sketch_vae.get_video_indices = lambda frames: sids          # the tokenizer is not what is measured
    N = 5 * 256
    ids = torch.randint(0, 8192, (batch, N), generator=g).to(dev)
    res = {name: [] for name, _ in SIDES}
    with torch.no_grad():
        ctx, cmask = m.embed_sketch(torch.zeros(batch, w['frames'], 3, 256, 256, device=dev))
        rows = m.embed_video(ids[:, :tokens + 2])
        last = {}
        for _ in range(rounds + 1):                               # the first round warms both sides up and is dropped
            for name, flag in SIDES:
                os.environ['AMDNUWA_XC2_DECODE_PACKED'] = flag
                st = GuidedStepper(m, ctx, cmask, N, 2., graph=True)
                assert all(b.c2.packed == (flag == '1') and b.c2.slot_rows.shape[1] == slots for b in st.cond.blocks if b.c2 is not None)
                st(rows[:, 0])
                st(rows[:, 1])
                torch.cuda.synchronize()
                assert st.graph is not None, 'the step was not captured'
                t0 = time.perf_counter()
                for t in range(2, tokens + 2):
                    out = st(rows[:, t])
                torch.cuda.synchronize()
                res[name].append((time.perf_counter() - t0) / tokens * 1e3)
                last[name] = out.clone()
                del st
    os.environ.pop('AMDNUWA_XC2_DECODE_PACKED', None)
    diff = float((last['in place'] - last['packed']).abs().max() / last['packed'].abs().max())
    for name, _ in SIDES:
        v = res[name][1:]
        print(f'RESULT {slots} {name}: ' + ' '.join(f'{t:.4f}' for t in v) + f' | min {min(v):.4f} spread {max(v) - min(v):.4f}', flush=True)
    print(f'RESULT {slots} logits: in place vs packed, last timed row, max-abs / max-abs {diff:.2e}', flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--window', type=int, choices=sorted(WINDOWS), default=None)
    ap.add_argument('--batch', type=int, default=4)
    ap.add_argument('--tokens', type=int, default=400)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--step-timeout', type=int, default=240)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if args.window is not None:
        return measure(args.window, args.batch, args.tokens, args.rounds)
    lines = [f'tools/sketch_decode_probe.py: ms per guided token of the cached + graph NUWASketch row step (dim 512, 12 layers of 8 x 64, b = {args.batch}, '
             f"precision mode '{os.environ.get('AMDNUWA_PRECISION', 'bf16x3-fwd')}'), {args.tokens} graph replays per repeat, {args.rounds} repeats per side, "
             'sides interleaved in one process per window; host clock around device-synchronised work']
    stats = {}
    for slots in sorted(WINDOWS):
        cmd = ['timeout', '-k', '10', str(args.step_timeout), sys.executable, os.path.abspath(__file__), '--window', str(slots), '--batch', str(args.batch),
               '--tokens', str(args.tokens), '--rounds', str(args.rounds)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        got = [ln[len('RESULT '):] for ln in r.stdout.splitlines() if ln.startswith('RESULT ')]
        if r.returncode != 0:
            lines.append(f'window of {slots} slots: not measured (the child process ended with status {r.returncode})')
            print('\n'.join(lines))
            print(r.stdout[-2000:], r.stderr[-4000:], sep='\n')
            return r.returncode                                   # nothing more is started on the GPU
        w = WINDOWS[slots]
        lines.append(f'window of {slots} slots ({w["frames"]} sketch frames x {w["kernel"]} x {w["kernel"]}):')
        for ln in got:
            lines.append('  ' + ln.split(' ', 1)[1])
            if '| min' in ln:
                side = ln.split(' ', 1)[1].split(':')[0]
                stats[slots, side] = (float(ln.split('min ')[1].split()[0]), float(ln.split('spread ')[1]))
    (ti, si), (tp, sp) = stats[18, 'in place'], stats[18, 'packed']
    faster = tp - ti > max(si, sp)
    lines.append(f'rule (18 slots): packed min {tp:.4f} - in place min {ti:.4f} = {tp - ti:+.4f} ms against a spread of {max(si, sp):.4f} ms between repeats: '
                 + ('in place is faster by more than the spread -- it stays the default for every window' if faster else
                    'in place is NOT faster by more than the spread -- windows of at most 287 slots default to the packed path'))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
