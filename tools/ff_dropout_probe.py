#!/usr/bin/env python
"""FeedForward dropout (np.py:276) on the mask kernels of csrc/dropout.hip against the torch element-wise formulation they replace
(AMDNUWA_FF_DROP_TORCH = 1, kernels.set_ff_drop_torch), one process:

  * forward + backward of ONE dim-512 FeedForward (stand-alone node) at rows = batch x 2560, p = 0.05, 'bf16x3-fwd': the two sides
    alternately, `--rounds` rounds each after warm-up, every round `--iters` device-synchronised iterations; the same FF without
    dropout as the floor.  The spread between the rounds of one setting is the noise of the comparison.
  * with --cfg4: one training step of the cfg-4 decoder (dec_reversible, bench.py CFGS) with ff_dropout = 0.05 on both sides, and with
    dropout 0.

    python tools/ff_dropout_probe.py [--batch 128] [--rounds 3] [--iters 10] [--cfg4 --cfg4-batch 64 --cfg4-depth 64] [--out FILE]"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nuwa_pytorch_amd as A  # noqa: E402
from nuwa_pytorch_amd import kernels as K  # noqa: E402

DEV = 'cuda'


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def alternate(settings, rounds, iters, warm=2):
    """settings: name -> (prepare(), run()).  Warm every setting, then time them alternately: {name: [ms per round]}"""
    for prep, run in settings.values():
        prep()
        for _ in range(warm):
            run()
    out = {k: [] for k in settings}
    for _ in range(rounds):
        for k, (prep, run) in settings.items():
            prep()
            out[k].append(timed(run, iters))
    return out


def table(title, res, lines):
    lines.append(title)
    for k, v in res.items():
        lines.append(f'  {k:34s} ' + ' '.join(f'{t:9.3f}' for t in v) + f'   ms   (min {min(v):.3f}, spread {max(v) - min(v):.3f})')


def ff_layer(batch, rounds, iters, lines):
    rows = batch * 2560
    torch.manual_seed(0)
    ffd = A.FeedForward(dim=512, dropout=0.05).to(DEV).train()
    ff0 = A.FeedForward(dim=512, dropout=0.).to(DEV).train()
    ff0.load_state_dict(ffd.state_dict())
    x = torch.randn(batch, 2560, 512, device=DEV, requires_grad=True)
    dy = torch.randn(batch, 2560, 512, device=DEV)

    def run(m):
        def f():
            x.grad = None
            for p in m.parameters():
                p.grad = None
            m(x).backward(dy)
        return f
    res = alternate({'dropout 0.05, torch passes': (lambda: K.set_ff_drop_torch(True), run(ffd)),
                     'dropout 0.05, mask kernels': (lambda: K.set_ff_drop_torch(False), run(ffd)),
                     'no dropout (floor)': (lambda: K.set_ff_drop_torch(False), run(ff0))}, rounds, iters)
    K.set_ff_drop_torch(False)
    table(f'FeedForward dim 512 forward + backward, rows = {batch} x 2560 = {rows}, p = 0.05, bf16x3-fwd, {iters} iterations per round:', res, lines)
    return res


def cfg4_step(batch, depth, rounds, lines):
    import bench
    c = dict(bench.CFGS['cfg4'], dec_depth=depth)

    def build(p):
        torch.manual_seed(0)
        vae = A.VQGanVAE(dim=c['vae']['dim'], image_size=c['vae']['image_size'], num_layers=c['vae']['num_layers'],
                         vq_codebook_size=c['codebook'], use_vgg_and_gan=False)
        m = A.NUWA(vae=vae, dim=c['dim'], max_video_frames=c['frames'], text_max_seq_len=c['text_len'], text_enc_depth=1, enc_reversible=True,
                   dec_reversible=True, dec_depth=depth, dec_heads=c['heads'], dec_dim_head=c['dim_head'], sparse_3dna_kernel_size=c['kernel'],
                   sparse_3dna_dilation=c['dilation'], shift_video_tokens=True, ff_dropout=p).to(DEV).train()
        params = bench.decoder_params(m)
        for q in m.parameters():
            q.requires_grad_(False)
        for q in params:
            q.requires_grad_(True)
        return m, params
    ids, ctx, mask = bench.synthetic_batch(c, batch, 0, DEV)
    md, pd = build(0.05)
    m0, p0 = build(0.)

    def run(m, params):
        def f():
            for q in params:
                q.grad = None
            bench.decoder_step(m, ids, ctx, mask)
        return f
    res = alternate({'ff_dropout 0.05, torch passes': (lambda: K.set_ff_drop_torch(True), run(md, pd)),
                     'ff_dropout 0.05, mask kernels': (lambda: K.set_ff_drop_torch(False), run(md, pd)),
                     'ff_dropout 0 (floor)': (lambda: K.set_ff_drop_torch(False), run(m0, p0))}, rounds, 1, warm=1)
    K.set_ff_drop_torch(False)
    table(f'cfg-4 decoder step (reversible, depth {depth}), b = {batch}, bf16x3-fwd, one step per round; peak memory {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB:', res, lines)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--cfg4', action='store_true')
    ap.add_argument('--cfg4-batch', type=int, default=64)
    ap.add_argument('--cfg4-depth', type=int, default=64)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'the probe measures on the GPU'
    A.set_precision('bf16x3-fwd')
    lines = [f'tools/ff_dropout_probe.py on {torch.cuda.get_device_name(0)}: host clock around device-synchronised work, settings alternated, ms per iteration per round']
    ff_layer(args.batch, args.rounds, args.iters, lines)
    if args.cfg4:
        try:
            cfg4_step(args.cfg4_batch, args.cfg4_depth, args.rounds, lines)
        except torch.cuda.OutOfMemoryError as e:
            lines.append(f'cfg-4 step at b = {args.cfg4_batch}: not measured (out of memory: {str(e).splitlines()[0]})')
    text = '\n'.join(lines)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
