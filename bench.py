#!/usr/bin/env python
"""Benchmark of the hot path BASELINE.json names: video-tokens/sec, NUWA 3DNA decoder forward+backward
at 10x16x16 video tokens (BASELINE cfg 3: dim 512, depth 24, 8 heads, 3DNA kernel (5,3,3), dilation
cycle (1,2,4), 256 text tokens of context), bf16 MFMA operands, synthetic data, random-init weights.

The HEADLINE (`value`) is the precision mode that meets BOTH halves of the north star's sentence: 'bf16x3-fwd' = the cheapest
forward arithmetic that keeps the full-depth logits within 1e-3 of the fp32 reference (measured live below in `parity`):
bf16 hi + lo operand pairs (3 MFMAs per product) on the cross-attention kv projection and to_logits; TWO fp16 MFMAs (fp16 activation x
the weight as an fp16 hi + lo pair) on to_out x2 and the cross-attention q projection; SINGLE fp16 MFMAs (fp16 operands, fp32
accumulate) on the Sparse3DNA q / k / v projection, FF1 (+ GEGLU gate), FF2 and both attention cores;
the backward runs single bf16 MFMAs.  The all-bf16 mode (faster, logits ~8e-3) is timed in a `--full` run as `fast_mode`.

    python bench.py --gpus 1 --steps 20 --warmup 5
    python bench.py --gpus 1 --steps 20 --warmup 5 --full  (+ every side measurement and check below)
    python bench.py --gpus 1 --steps 20 --warmup 5 --dump-outputs DIR
    python bench.py --gpus N --steps K --warmup W          (N > 1 without a launcher: starts itself under torch.distributed.run)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

One "step" = embedding assemble -> 24 decoder layers -> StableLayerNorm -> to_logits -> cross entropy ->
backward to all decoder parameter gradients (+ the RCCL gradient all-reduce for N > 1), on `--batch`
samples per GPU (weak scaling).  Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times the K steps, writes --dump-outputs if given and prints the line; everything else it
can measure or check (`roofline.families`, `parity`, `fast_mode`, `vae_tokenizer`, `cpu_baseline`) runs only with --full.

--dump-outputs DIR: after the timed steps, rank 0 writes what the last timed step returned to its caller -- the loss (DIR/loss.npy,
float64) and the gradient of every decoder parameter (DIR/grad.<parameter name>.npy, float32) -- so that two builds can be compared
output for output on identical inputs.  Gradients of at most 65536 elements are written whole; of the larger ones a fixed, seeded,
sorted sample of flat positions (the same for the same shape and name), sized to keep the directory under 64 MB.

What the line carries (rank 0):
  value / ms_per_step   EXACTLY K steps between barrier + synchronize on both sides, wall clock, max over ranks; the per-launch
                        HIP-event timer of the library is OFF in this region.  `ms_per_step_median` = median of the K per-step
                        HIP-event intervals recorded on the compute stream in the same region.
  roofline              SURVEY 8(d): the WHOLE decoder step -- algorithmic FLOPs of forward + backward / ms_per_step against the dense bf16
                        MFMA peak (`frac` == `step_mfma_frac`); `families` (--full) = the same object per kernel family (gemm_nt, xattn: MFMA-bound;
                        s3, ln: HBM-bound, algorithmic bytes / time against 8 TB/s) from a SECOND pass of a few steps with the library's
                        per-launch HIP-event timer armed (events on the launch stream, inside libamdnuwa).
  parity (--full)       the same 24-layer decoder, one sample, logits against the oracle's (fp32 CPU restatement of the
                        reference) in every precision mode, measured in this run; `worst_of_8` = the committed sweep over 8 samples / 3
                        models (tools/parity_sweep.py -> profiles/parity_sweep.json); `grad_rel_max` = worst gradient error of ONE cfg-3
                        decoder layer (dx, dcontext, every parameter) against the oracle, live, in the headline mode and in 'bf16'.
  fast_mode (--full)    throughput of the all-bf16 mode (no lo parts anywhere; logits error in `parity.bf16`) in the same run.
  cpu_baseline (--full) the oracle's full step (24 layers forward + backward through the CE loss), b = 1, on the host cores.
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time
import zlib

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

CFGS = {
    'cfg3': dict(dim=512, dec_depth=24, heads=8, dim_head=64, frames=10, fmap=16, kernel=(5, 3, 3), dilation=(1, 2, 4),
                 text_len=256, codebook=8192, vae=dict(dim=64, image_size=256, num_layers=4)),
    'cfg4': dict(dim=512, dec_depth=64, heads=8, dim_head=64, frames=10, fmap=16, kernel=(5, 3, 3), dilation=(1, 2, 4),
                 text_len=256, codebook=8192, vae=dict(dim=64, image_size=256, num_layers=4), reversible=True),
    'cfg2': dict(dim=256, dec_depth=6, heads=8, dim_head=64, frames=4, fmap=16, kernel=(3, 3, 3), dilation=(1,),
                 text_len=256, codebook=512, vae=dict(dim=64, image_size=64, num_layers=2)),
}
PEAK_BF16_TFLOPS = 2500.0      # dense bf16 MFMA peak, MI355X_MICROARCH.md
PEAK_HBM_GBS = 8000.0          # HBM3E peak, MI355X_MICROARCH.md
ROOFLINE_SOURCES = ('nuwa_pytorch_amd/csrc/gemm.hip',)      # kernels the committed PMC traffic figure belongs to


def fwd_flops_per_sample(c):
    """ALGORITHMIC forward FLOPs per sample: GEMMs + attention cores (valid 3DNA taps only).
    Reversible stacks (cfg 4, np.py:1246-1277) carry a FeedForward after the 3DNA block AND after the cross-attention block."""
    D, h, d, T, C = c['dim'], c['heads'], c['dim_head'], c['text_len'], c['codebook']
    n = c['frames'] * c['fmap'] ** 2
    inner = h * d
    ffi = (D * 4 * 2) // 3
    proj3 = 2 * n * D * inner + 2 * (n + 1) * D * 2 * inner + 2 * n * inner * D
    projx = 2 * n * D * inner + 2 * T * D * 2 * inner + 2 * n * inner * D
    corex = 4 * h * n * (T + 1) * d + 2 * h * h * n * (T + 1)
    ff = 2 * n * D * 2 * ffi + 2 * n * ffi * D
    from nuwa_pytorch_amd.nuwa_pytorch import causal_neighbor_mask
    tot = 0
    for l in range(c['dec_depth']):
        dl = c['dilation'][l % len(c['dilation'])]
        m = causal_neighbor_mask((c['frames'], c['fmap'], c['fmap']), c['kernel'], (dl, dl, dl))
        valid = int((~m[:n - 1]).sum())
        tot += proj3 + (4 * h * d + 2 * h * h) * valid + projx + corex + ff * (2 if c.get('reversible') else 1)
    return tot + 2 * n * D * C


def build_model(c, device, seed=0):
    import nuwa_pytorch_amd as A
    torch.manual_seed(seed)
    vae = A.VQGanVAE(dim=c['vae']['dim'], image_size=c['vae']['image_size'], num_layers=c['vae']['num_layers'],
                     vq_codebook_size=c['codebook'], use_vgg_and_gan=False)
    nuwa = A.NUWA(vae=vae, dim=c['dim'], max_video_frames=c['frames'], text_max_seq_len=c['text_len'], text_enc_depth=1,
                  enc_reversible=True, dec_reversible=bool(c.get('reversible')), dec_depth=c['dec_depth'], dec_heads=c['heads'], dec_dim_head=c['dim_head'],
                  sparse_3dna_kernel_size=c['kernel'], sparse_3dna_dilation=c['dilation'], shift_video_tokens=True)
    return nuwa.to(device).train()


def decoder_params(nuwa):
    ps = list(nuwa.video_transformer.parameters()) + [nuwa.to_logits.weight, nuwa.video_bos] + \
        list(nuwa.image_embedding.parameters()) + list(nuwa.video_pos_emb.parameters())
    seen, out = set(), []
    for p in ps:
        if id(p) not in seen:
            seen.add(id(p)); out.append(p)
    return out


def decoder_step(nuwa, ids, ctx, mask):
    x = nuwa.embed_video(ids[:, :-1])
    h = nuwa.decode_hidden(x, ctx, mask)
    loss = nuwa._final(h, ids)
    loss.backward()
    return loss


def synthetic_batch(c, b, rank, dev):
    N = c['frames'] * c['fmap'] ** 2
    g = torch.Generator(device='cpu').manual_seed(1234 + rank)
    ids = torch.randint(0, c['codebook'], (b, N), generator=g)
    ctx = torch.randn(b, c['text_len'], c['dim'], generator=g)
    mask = torch.ones(b, c['text_len'], dtype=torch.bool)
    mask[:, -64:] = torch.rand(b, 64, generator=g) > 0.5        # exercise the key mask
    return ids.to(dev), ctx.to(dev), mask.to(dev)


def cpu_baseline(c, nuwa, ids, ctx, mask, max_runs=3, budget_s=75.0, threads=None):
    """the oracle (fp32 CPU restatement of the reference algorithm) on the host cores: ONE sample of the same workload, the FULL
    step -- embed -> every decoder layer -> StableLayerNorm -> logits -> cross entropy -> backward -- with the benchmarked
    model's own weights; repeated up to `max_runs` times while the total stays within `budget_s`, median reported.
    Returns (json object, oracle logits of that sample)."""
    from oracle import nuwa_oracle as O
    host = os.cpu_count() or 1
    # default 32 threads: beyond that the fp32 oracle gets slower, not faster (profiles/r03_cpu_baseline_threads.txt holds the
    # os.cpu_count() run that shows it; --cpu-threads N re-takes it)
    torch.set_num_threads(min(host, threads or 32))
    threads = torch.get_num_threads()
    N = c['frames'] * c['fmap'] ** 2
    keep = lambda k: not (k.startswith('vae.') or k.startswith('text_'))
    P = {k: v.detach().float().cpu().clone() for k, v in nuwa.state_dict().items() if keep(k)}
    Pg = {k: (v.requires_grad_(True) if v.is_floating_point() else v) for k, v in P.items()}
    cfg = dict(video_shape=(c['frames'], c['fmap'], c['fmap']), kernel_size=c['kernel'], dilations=c['dilation'], heads=c['heads'],
               depth=c['dec_depth'], shift=True, reversible=bool(c.get('reversible')))
    i1, c1, m1 = ids[:1].cpu(), ctx[:1].float().cpu(), mask[:1].cpu()
    times, logits = [], None
    t_all = time.perf_counter()
    while len(times) < max_runs and (not times or time.perf_counter() - t_all + times[-1] <= budget_s):
        for v in Pg.values():
            if v.is_floating_point():
                v.grad = None
        t0 = time.perf_counter()
        loss, lg = O.decoder_loss(Pg, cfg, i1, c1, m1, training=True, return_logits=True)
        loss.backward()
        times.append(time.perf_counter() - t0)
        logits = lg.detach()
    t_step = statistics.median(times)
    return dict(value=N / t_step, unit='video-tokens/s', cores=threads, host_cores=host, kind='port', runs=len(times),
                seconds_per_step=t_step,
                sample=f'oracle fp32, b=1, the full step ({c["dec_depth"]} decoder layers + embed/norm/logits/CE, forward + backward), '
                       f'median of {len(times)} run(s): {", ".join(f"{t:.1f}" for t in times)} s'), logits


def gpu_logits(nuwa, ids, ctx, mask, mode):
    import nuwa_pytorch_amd as A
    prev = A.get_precision()
    A.set_precision(mode)
    try:
        with torch.no_grad():
            x = nuwa.embed_video(ids[:1, :-1])
            h = nuwa.decode_hidden(x, ctx[:1].contiguous(), mask[:1].contiguous())
            return nuwa._final(h).float().cpu()
    finally:
        A.set_precision(prev)


def layer_grad_parity(A, c, modes=('bf16x3-fwd', 'bf16')):
    """worst max-abs / max-abs gradient error of ONE decoder layer (3DNA dilation 1 + text cross attention + FeedForward) at the named
    size against the oracle on the same inputs, per precision mode -- the number that says what the benchmarked backward computes
    (tests/test_gpu_named_size.py asserts the same quantity for every dilation)"""
    import nuwa_pytorch_amd.nuwa_pytorch as M
    from oracle import nuwa_oracle as O
    vs, T = (c['frames'], c['fmap'], c['fmap']), c['text_len']
    torch.manual_seed(0)
    tr = M.Transformer(dim=c['dim'], depth=1, causal=True, heads=c['heads'], dim_head=c['dim_head'], cross_attend=True, sparse_3dna_attn=True,
                       sparse_3dna_kernel_size=c['kernel'], sparse_3dna_video_shape=vs, sparse_3dna_dilations=(c['dilation'][0],),
                       shift_video_tokens=True)
    with torch.no_grad():
        for n_, p in tr.named_parameters():
            if 'norm' in n_ or n_.endswith('.bias'):
                p.add_(0.1 * torch.randn_like(p))
    P = {k: v.detach().cpu().clone() for k, v in tr.state_dict().items()}
    Pr = {k: (v.clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in P.items()}
    n = vs[0] * vs[1] * vs[2]
    g = torch.Generator().manual_seed(7)
    x, ctx = torch.randn(1, n, c['dim'], generator=g), torch.randn(1, T, c['dim'], generator=g)
    mask = torch.ones(1, T, dtype=torch.bool)
    mask[:, -T // 4:] = torch.rand(1, T // 4, generator=g) > 0.5
    dy = torch.randn(1, n, c['dim'], generator=g)
    cfg = dict(video_shape=vs, kernel_size=c['kernel'], dilations=(c['dilation'][0],), heads=c['heads'], depth=1, shift=True)
    xr, cr = x.clone().requires_grad_(True), ctx.clone().requires_grad_(True)
    O.decoder_layer(xr, O.sub(Pr, 'layers.0'), cfg, 0, cr, mask).backward(dy)
    tr = tr.to('cuda')
    rel = lambda a, b: float((a.detach().double().cpu() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30))
    out = {}
    for mode in modes:
        A.set_precision(mode)
        tr.zero_grad(set_to_none=True)
        xd, cd = x.cuda().requires_grad_(True), ctx.cuda().requires_grad_(True)
        tr.forward_layers(xd, context=cd, context_mask=mask.cuda()).backward(dy.cuda())
        worst = max(rel(xd.grad, xr.grad), rel(cd.grad, cr.grad))
        for k, p in tr.named_parameters():
            if Pr[k].grad is not None:
                worst = max(worst, rel(p.grad, Pr[k].grad))
        out[mode] = worst
    return out


def file_sha16(paths):
    h = hashlib.sha256()
    for p in paths:
        with open(os.path.join(ROOT, p), 'rb') as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def traffic_from_profiles(config, b, mode='bf16'):
    """HBM bytes per NT-GEMM launch from the committed PMC passes (profiles/traffic.json, written by tools/pmc_summary.py from
    separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE runs of this same command).  The entry records the hash of the kernel
    sources it was measured on; a figure taken on other sources is REFUSED (None + the reason), not reported stale."""
    try:
        with open(os.path.join(ROOT, 'profiles', 'traffic.json')) as f:
            t = json.load(f)
    except (OSError, ValueError):
        return None, 'profiles/traffic.json missing'
    e = t.get(f'{config}_b{b}_{mode}') or (t.get(f'{config}_b{b}') if mode == 'bf16' else None)
    if not e or 'bytes_per_launch' not in e:
        return None, f'no PMC pass committed for {config} at b={b} in {mode}'
    now = file_sha16(ROOFLINE_SOURCES)
    if e.get('src_sha16') != now:
        return None, f'stale: PMC pass taken on kernel sources {e.get("src_sha16")}, this tree has {now}'
    return e, e.get('source', '')


def tokenizer_rate(nuwa, c, b, dev):
    """frozen VQGanVAE tokenizer (get_video_indices, exact-fp32 HIP kernels) on b videos of raw frames; reported beside the
    decoder metric, never inside its timed region (the decoder bench feeds token ids, as a cached-token trainer would)."""
    v = c['vae']
    video = torch.rand(b, c['frames'], 3, v['image_size'], v['image_size'], device=dev)
    nuwa.vae.get_video_indices(video)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(3):
        ids = nuwa.vae.get_video_indices(video)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / 3
    return {'frames_per_s': b * c['frames'] / dt, 'video_tokens_per_s': ids.numel() / dt, 'ms': dt * 1e3, 'videos': b, 'dtype': 'f32'}


DUMP_BYTES = 60 * 2 ** 20      # --dump-outputs stays under 64 MB
DUMP_WHOLE = 65536             # gradients up to this many elements are written whole


def dump_outputs(out_dir, nuwa, params, loss):
    """writes the loss and every decoder parameter gradient of the last step (module docstring: --dump-outputs)"""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    names = {id(p): k for k, p in nuwa.named_parameters()}
    grads = [(names[id(p)], p.grad) for p in params if p.grad is not None]
    whole = sum(g.numel() for _, g in grads if g.numel() <= DUMP_WHOLE)
    large = sum(g.numel() for _, g in grads if g.numel() > DUMP_WHOLE)
    frac = min(1.0, (DUMP_BYTES // 4 - whole) / max(large, 1))
    np.save(os.path.join(out_dir, 'loss.npy'), np.asarray(float(loss.detach()), dtype=np.float64))
    for name, g in grads:
        flat = g.detach().reshape(-1)
        if flat.numel() > DUMP_WHOLE:
            gen = torch.Generator(device='cpu').manual_seed(zlib.crc32(name.encode()))
            keep = max(1, int(flat.numel() * frac))
            idx = torch.randperm(flat.numel(), generator=gen)[:keep].sort().values
            flat = flat[idx.to(flat.device)]
        np.save(os.path.join(out_dir, f'grad.{name}.npy'), flat.float().cpu().numpy())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=None,
                    help="samples per GPU (weak scaling); default for cfg3: 128 in 'bf16x3-fwd' (243 GB of the 288 GB; +2.2 %% tokens/s over 96) and in 'bf16', 16 in 'bf16x3'; 64 for the other configs")
    ap.add_argument('--config', default='cfg3', choices=list(CFGS))
    ap.add_argument('--precision', default='bf16x3-fwd', choices=['bf16x3-fwd', 'bf16', 'bf16x3'],
                    help="mode of the HEADLINE value; the default is the mode that meets the 1e-3 logits bound")
    ap.add_argument('--side-batch', type=int, default=None, help="samples per GPU of the 'bf16' side measurement (default: the headline batch)")
    ap.add_argument('--no-parity', action='store_true', help="skip the 'bf16' side pass and the logits-vs-oracle measurement")
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--cpu-threads', type=int, default=None, help='host threads of the cpu_baseline leg (default 32; 0 = os.cpu_count())')
    ap.add_argument('--backend', default='nccl', choices=['nccl', 'gloo'], help='nccl = RCCL over xGMI (default); gloo only for functional checks')
    ap.add_argument('--collective', default='allreduce', choices=['allreduce', 'rs_ag', 'native', 'native_rs_ag'],
                    help="gradient exchange per bucket: torch.distributed collectives, or libamdnuwa's own RCCL communicator (native*)")
    ap.add_argument('--single-device', action='store_true', help='functional check only: every rank uses cuda:0 (with --backend gloo)')
    ap.add_argument('--graph', action='store_true',
                    help='replay the timed steps as ONE HIP graph (forward + backward, ~2700 launches) instead of launching kernel by kernel; '
                         'single GPU only.  Measured neutral (DESIGN.md 5m): off by default')
    ap.add_argument('--no-tokenizer', action='store_true', help='skip the (untimed, separately reported) frozen-VAE tokenizer rate')
    ap.add_argument('--full', action='store_true',
                    help='after the headline: the per-family roofline pass, the all-bf16 side pass, the tokenizer rate, the CPU baseline and the '
                         'parity checks (the --no-* options above leave parts of it out); a plain run times the headline only')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help='write the loss and the decoder parameter gradients of the last timed step to DIR/*.npy (rank 0)')
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        raise SystemExit('bench.py: --steps must be >= 1 and --warmup >= 0')

    if not torch.cuda.is_available():
        raise SystemExit('bench.py needs a HIP device (the decoder path has no CPU fallback)')
    if 'WORLD_SIZE' not in os.environ and args.gpus > 1:
        # `python bench.py --gpus N` without a launcher: start the launcher (one rank per GPU, RCCL) as a child, so that the line says n_gpus: N
        # and measures N devices -- or fail loudly when the box does not have them.  A child, not exec: this process has already opened the
        # device (device_count), and replacing a process that holds the device with another program is not safe on every driver
        have = torch.cuda.device_count()
        if have < args.gpus and not args.single_device:
            raise SystemExit(f'bench.py --gpus {args.gpus}: this box exposes {have} HIP device(s)')
        import socket
        with socket.socket() as sk:
            sk.bind(('127.0.0.1', 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={args.gpus}', '--master-addr', '127.0.0.1',
               '--master-port', str(port), os.path.abspath(__file__)] + sys.argv[1:]
        sys.stdout.flush()
        raise SystemExit(subprocess.call(cmd))
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local = int(os.environ.get('LOCAL_RANK', '0'))
    if world != args.gpus:
        raise SystemExit(f'bench.py --gpus {args.gpus} was launched with WORLD_SIZE={world}: the two must agree')
    if not args.single_device and torch.cuda.device_count() < world:
        raise SystemExit(f'bench.py: {world} ranks but only {torch.cuda.device_count()} HIP device(s) on this node')
    if args.single_device:
        local = 0
    torch.cuda.set_device(local)
    dev = torch.device('cuda', local)
    if world > 1:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        dist.init_process_group(args.backend, rank=rank, world_size=world)
    import nuwa_pytorch_amd as A
    from nuwa_pytorch_amd import kernels as K
    from nuwa_pytorch_amd.distributed import GradReducer, broadcast_parameters
    A.set_precision(args.precision)
    c = CFGS[args.config]
    nuwa = build_model(c, dev)
    if world > 1:
        broadcast_parameters(nuwa, src=0)                 # one flat collective per dtype, not one per tensor
    params = decoder_params(nuwa)
    for p in nuwa.parameters():
        p.requires_grad_(False)
    for p in params:
        p.requires_grad_(True)
    reducer = GradReducer(nuwa, collective=args.collective) if world > 1 else None

    default_b = {'bf16x3-fwd': 128, 'bf16': 128, 'bf16x3': 16}[args.precision] if args.config == 'cfg3' else (16 if args.precision == 'bf16x3' else 64)
    b = args.batch if args.batch else default_b
    N = c['frames'] * c['fmap'] ** 2
    ids, ctx, mask = synthetic_batch(c, b, rank, dev)

    def step(batch=(ids, ctx, mask)):
        if reducer is not None:
            reducer.zero_grad()
        else:
            for p in params:
                p.grad = None
        loss = decoder_step(nuwa, *batch)
        if reducer is not None:
            reducer.finish()
        return loss

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    # ---- --graph: the step as ONE HIP graph (single GPU): forward + backward are ~2700 launches with static shapes.  Captured after one
    # eager step (weight operand copies, workspaces, lazy module state); any capture failure falls back to eager launches.  Measured:
    # the capture works, the step time does not change (the 3.3 % of idle time in the kernel trace sits between DEPENDENT kernels and
    # stays there under graph launch), so it is opt-in.  With N > 1 the bucket collectives run on a side stream from autograd hooks:
    # those steps stay eager.
    graph, graph_note = None, None
    timed_step = step
    if args.graph and world == 1:
        try:
            step()
            torch.cuda.synchronize()
            for p in params:
                p.grad = None
            torch.cuda.empty_cache()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                static_loss = step()

            def timed_step():
                graph.replay()
                return static_loss
        except Exception as e:      # noqa: BLE001  (capture is an optimisation, never a requirement)
            graph, graph_note = None, f'capture failed, eager launches: {type(e).__name__}: {str(e)[:200]}'
            timed_step = step
            torch.cuda.synchronize()
            for p in params:
                p.grad = None
            torch.cuda.empty_cache()

    # ---- headline: K steps, wall clock between fences; per-step HIP events on the compute stream for the median
    for _ in range(args.warmup):
        timed_step()
    fence()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    t0 = time.perf_counter()
    marks[0].record()
    for i in range(args.steps):
        loss = timed_step()
        marks[i + 1].record()
    fence()
    dt = time.perf_counter() - t0
    per_step_ms = [marks[i].elapsed_time(marks[i + 1]) for i in range(args.steps)]
    tmax = torch.tensor([dt], device=dev, dtype=torch.float64)
    if world > 1:
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    dt = float(tmax.item())
    peak_gb = torch.cuda.max_memory_allocated(dev) / 2 ** 30
    loss_val = float(loss.detach())
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, nuwa, params, loss)
    graph_used = graph is not None
    if graph is not None:                        # the graph's private pool holds a whole step's tensors: release it before the side passes
        del timed_step, static_loss, loss
        graph.reset()
        for p in params:
            p.grad = None
        torch.cuda.empty_cache()

    # ---- second pass (--full, rank 0's numbers): the library's per-launch HIP-event timer armed around every amdnuwa_gemm_nt launch
    probe_steps = max(1, min(args.steps, 5))
    gemm_ms, gemm_launches, gemm_flops, gemm_bytes, gemm_issued = (0.0, 0, 0.0, 0.0, 0.0)
    families = {}
    if args.full:
        if rank == 0:
            K.timer_arm(True)
        t1 = time.perf_counter()
        for _ in range(probe_steps):
            step()
        fence()
        dt_probe = time.perf_counter() - t1
        if rank == 0:
            gemm_ms, gemm_launches, gemm_flops, gemm_bytes = K.timer_collect()
            gemm_issued = K.timer_issued_flops()
            families = K.timer_families()
            K.timer_arm(False)

    # ---- the all-bf16 mode beside the headline (--full; same batch unless --side-batch), a few steps
    fast_mode = None
    loss = None
    if args.full and not args.no_parity and args.precision != 'bf16':
        torch.cuda.empty_cache()      # the side pass allocates differently sized activations: hand the cached blocks back first
        pb = max(1, args.side_batch or b)
        pbatch = (ids, ctx, mask) if pb == b else synthetic_batch(c, pb, rank, dev)
        A.set_precision('bf16')
        try:
            step(pbatch)
            step(pbatch)
            fence()
            ps = max(2, min(args.steps, 5))
            t2 = time.perf_counter()
            for _ in range(ps):
                step(pbatch)
            fence()
            d2 = torch.tensor([time.perf_counter() - t2], device=dev, dtype=torch.float64)
            if world > 1:
                dist.all_reduce(d2, op=dist.ReduceOp.MAX)
            d2 = float(d2.item())
            fast_mode = {'dtype': 'bf16', 'value': world * pb * N * ps / d2, 'unit': 'video-tokens/s', 'ms_per_step': d2 / ps * 1e3,
                         'per_gpu_batch': pb, 'steps': ps,
                         'step_mfma_frac': 3.0 * fwd_flops_per_sample(c) * pb / (d2 / ps) / 1e12 / PEAK_BF16_TFLOPS,
                         'note': 'single bf16 MFMA per product in forward and backward; does NOT meet the 1e-3 logits bound (see parity.bf16)'}
        finally:
            A.set_precision(args.precision)
            for p in params:
                p.grad = None
        torch.cuda.empty_cache()

    if rank == 0:
        tokens = world * b * N * args.steps
        value = tokens / dt
        # which parts of the 'bf16x3-fwd' forward run single fp16 MFMAs in THIS run (AMDNUWA_F16_CORES / _FF / _QKV switches)
        x2 = K._PROJ_F16X2 if K._CORES_F16 else (K._PROJ_F16X2 & frozenset('l'))      # (to_out / q take the fp16 cores' operands)
        f16_parts = {'cores': bool(K._CORES_F16), 'ff': bool(K._FF_F16), 'qkv': bool(K._QKV_F16 and K._CORES_F16),
                     'two_mfma_products': ''.join(sorted(x2))}
        three = [nm for nm, cls in (('to_out x2', 'o'), ('cross-attention q projection', 'q'), ('cross-attention kv projection', None), ('to_logits', 'l'))
                 if cls is None or cls not in x2]
        three += ([] if f16_parts['cores'] else ['both attention cores']) + ([] if f16_parts['ff'] else ['FF1', 'FF2']) + \
            ([] if f16_parts['qkv'] else ['3DNA q/k/v projection'])
        two = [nm for nm, cls in (('to_out x2', 'o'), ('cross-attention q projection', 'q'), ('to_logits', 'l')) if cls in x2]
        fl = fwd_flops_per_sample(c)
        step_flops = 3.0 * fl * b
        ach = gemm_flops / (gemm_ms * 1e-3) / 1e12 if gemm_ms > 0 else 0.0
        out = {
            'metric': 'video-tokens/sec, 3DNA decoder fwd+bwd @ 10x16x16' if args.config == 'cfg3' else 'video-tokens/sec, 3DNA decoder fwd+bwd',
            'value': value, 'unit': 'video-tokens/s', 'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup,
            'ms_per_step': dt / args.steps * 1e3, 'ms_per_step_median': statistics.median(per_step_ms),
            'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None,
            'dtype': {'bf16': 'bf16 operands, fp32 accumulate (single bf16 MFMA per product, forward and backward)',
                      'bf16x3': 'bf16 hi+lo operand pairs, fp32 accumulate (3 bf16 MFMAs per product, forward and backward)',
                      'bf16x3-fwd': 'bf16/fp16 operands, fp32 accumulate -- forward: 3-MFMA bf16 hi+lo pairs on ' + ', '.join(three) +
                                    ('; 2 fp16 MFMAs (fp16 activation x fp16 hi+lo weight) on ' + ', '.join(two) if two else '') +
                                    '; single fp16 MFMA on ' + (', '.join(nm for nm, on in (('3DNA q/k/v projection', f16_parts['qkv']), ('FF1 + gate', f16_parts['ff']),
                                                                                          ('FF2', f16_parts['ff']), ('Sparse3DNA core', f16_parts['cores']),
                                                                                          ('cross-attention core', f16_parts['cores'])) if on) or 'nothing') +
                                    '; backward: single bf16 MFMAs' + ('' if not K._BWD_F16 else ' except ' + ', '.join(nm for nm, cl in (('FeedForward', 'f'), ('Sparse3DNA', 's'), ('cross attention', 'x')) if cl in K._BWD_F16) +
                                                                        ' (single fp16 MFMAs on fp16(S x gradient), device-side power-of-two S, one fp16 copy per activation)')}[args.precision],
            'precision_mode': args.precision, 'fp16_forward_parts': f16_parts if args.precision == 'bf16x3-fwd' else None,
            'fp16_gradient_blocks': (''.join(sorted(K._BWD_F16)) if args.precision == 'bf16x3-fwd' else None), 'data': 'synthetic',
            'config': {'workload': f'BASELINE {args.config}: NUWA decoder dim={c["dim"]} depth={c["dec_depth"]} heads={c["heads"]}, '
                                   f'{c["frames"]}x{c["fmap"]}x{c["fmap"]} video tokens, 3DNA kernel {c["kernel"]} dilation {c["dilation"]}, '
                                   f'{c["text_len"]} text tokens, codebook {c["codebook"]}',
                       'per_gpu_batch': b, 'global_batch': b * world, 'tokens_per_sample': N, 'parallelism': f'dp{world}',
                       'loss': loss_val, 'collective': args.collective if world > 1 else None},
            'per_gpu_value': value / world,
            'launch': ('hip graph replay (one graph per step, captured after one eager step)' if graph_used else 'eager') +
                      (f' [{graph_note}]' if graph_note else ''),
            'peak_hbm_gb': peak_gb,
            'step_tflops_per_gpu': step_flops / (dt / args.steps) / 1e12,
            'step_mfma_frac': step_flops / (dt / args.steps) / 1e12 / PEAK_BF16_TFLOPS,
            'timing': 'value: wall clock over exactly `steps` steps between barrier+synchronize fences, max over ranks, library timer off; '
                      'ms_per_step_median: median of the per-step HIP-event intervals on the compute stream in the same region',
            'roofline': {'bound': 'mfma', 'kernel': 'the whole decoder step (SURVEY 8(d)): algorithmic FLOPs of forward + backward (3 x the forward products) / ms_per_step '
                                                     'against the dense bf16 MFMA peak; `traffic` = HBM bytes per step from the committed FETCH / WRITE counter passes',
                         'achieved': step_flops / (dt / args.steps) / 1e12, 'peak': PEAK_BF16_TFLOPS, 'unit': 'TFLOP/s',
                         'frac': step_flops / (dt / args.steps) / 1e12 / PEAK_BF16_TFLOPS, 'traffic': None,
                         'flops_per_step': step_flops, 'families': {}},
        }
        gemm_fam = {} if not args.full else {'bound': 'mfma', 'kernel': 'gemm_nt_* (bf16 / fp16 MFMA NT GEMM family; `achieved` counts the ALGORITHMIC 2MNK per product, `mfma_issued_tflops` what the hi+lo forward GEMMs really issue; every amdnuwa_gemm_nt launch of a separate pass of '
                              f'{probe_steps} step(s) with the per-launch HIP-event timer armed, events on the launch stream)',
                    'achieved': ach, 'peak': PEAK_BF16_TFLOPS, 'unit': 'TFLOP/s', 'frac': ach / PEAK_BF16_TFLOPS,
                    'traffic': None, 'algorithmic_bytes_per_launch': gemm_bytes / max(gemm_launches, 1),
                    'flops_per_launch': gemm_flops / max(gemm_launches, 1),
                    'mfma_issued_tflops': gemm_issued / (gemm_ms * 1e-3) / 1e12 if gemm_ms > 0 else 0.0,
                    'launches': gemm_launches, 'avg_launch_us': gemm_ms * 1e3 / max(gemm_launches, 1),
                    'ms_per_step': gemm_ms / probe_steps, 'share_of_step': gemm_ms * 1e-3 / dt_probe}
        if args.full:
            out['roofline']['families']['gemm_nt'] = gemm_fam
        for nm, bound, what in (('xattn', 'mfma', 'cross-attention cores: forward, backward query side, batched dK / dV products (algorithmic QK^T / P\'V / head-mix FLOPs)'),
                                ('s3', 'hbm', 'Sparse3DNA cores: forward (reads q, k, v, writes o) and backward (reads q, k, v, dO, writes dq, dk, dv)'),
                                ('ln', 'hbm', 'LayerNorm kernels: every large operand read once, every result written once')):
            f = families.get(nm)
            if not f or f['ms'] <= 0:
                continue
            if bound == 'mfma':
                a_, pk_, un_ = f['flops'] / (f['ms'] * 1e-3) / 1e12, PEAK_BF16_TFLOPS, 'TFLOP/s'
            else:
                a_, pk_, un_ = f['bytes'] / (f['ms'] * 1e-3) / 1e9, PEAK_HBM_GBS, 'GB/s'
            out['roofline']['families'][nm] = {'bound': bound, 'kernel': what, 'achieved': a_, 'peak': pk_, 'unit': un_, 'frac': a_ / pk_, 'traffic': None,
                                               'launches': f['launches'], 'avg_launch_us': f['ms'] * 1e3 / max(f['launches'], 1),
                                               'ms_per_step': f['ms'] / probe_steps, 'share_of_step': f['ms'] * 1e-3 / dt_probe}
        tr, why = traffic_from_profiles(args.config, b, args.precision)
        if tr is not None:
            gemm_fam['traffic'] = tr['bytes_per_launch']
            out['roofline']['traffic'] = tr.get('step_bytes')
        out['roofline']['traffic_source'] = why
        if fast_mode is not None:
            out['fast_mode'] = fast_mode
        if args.full and not args.no_tokenizer and world == 1:          # (side measurement, single-GPU runs only: keeps the ranks in step)
            out['vae_tokenizer'] = tokenizer_rate(nuwa, c, min(b, 8), dev)
        oracle_logits = None
        if args.full and world == 1 and not args.no_cpu_baseline:
            try:
                out['cpu_baseline'], oracle_logits = cpu_baseline(c, nuwa, ids, ctx, mask, threads=(os.cpu_count() if args.cpu_threads == 0 else args.cpu_threads))
            except Exception as e:      # the baseline is a report, never a reason to lose the GPU number
                out['cpu_baseline'] = {'value': None, 'unit': 'video-tokens/s', 'cores': os.cpu_count(), 'kind': 'port',
                                       'sample': f'failed: {type(e).__name__}: {e}'}
        if oracle_logits is not None and not args.no_parity:
            # the checker: this run's GPU logits of the baseline's sample (full depth) against the oracle's, both modes
            par = {'sample': f'logits [1, {N}, {c["codebook"]}] of sample 0 after all {c["dec_depth"]} layers vs the oracle (fp32 CPU), '
                             'max-abs error / max-abs reference; the north-star bound is 1e-3',
                   'bound': {'bf16x3-fwd': 1e-3, 'bf16x3': 1e-3, 'bf16': 1.2e-2}}
            ref = oracle_logits.double()
            for mode in ('bf16x3-fwd', 'bf16', 'bf16x3'):
                try:
                    got = gpu_logits(nuwa, ids, ctx, mask, mode).double()
                    par[mode] = {'logits_rel_max': float((got - ref).abs().max() / ref.abs().max()),
                                 'logits_rel_l2': float((got - ref).norm() / ref.norm())}
                except Exception as e:
                    par[mode] = {'error': f'{type(e).__name__}: {e}'}
            try:
                with open(os.path.join(ROOT, 'profiles', 'parity_sweep.json')) as f:
                    sweep = json.load(f)
                # the committed sweep (tools/parity_sweep.py on the round's evidence box): the 8 samples the 1e-3 bound is asserted on -- two
                # random initialisations x 3 samples + the mild trained-like model x 2 -- in the shipped two-MFMA class set; the harsh
                # trained-like model (recorded, not asserted: DESIGN.md section 2) beside it
                x2 = ''.join(sorted(K._PROJ_F16X2)) if hasattr(K, '_PROJ_F16X2') else 'oq'
                rows = [r for r in sweep if r.get('mode') == 'bf16x3-fwd' and ''.join(sorted(r.get('two_mfma') or '')) == x2]
                harsh = [r for r in rows if 'tails x4' in r['model']]
                eight = [r for r in rows if 'tails x4' not in r['model']]
                par['worst_of_8'] = {'source': 'profiles/parity_sweep.json', 'samples': len(eight),
                                     'logits_rel_max': max(r['rel_max'] for r in eight), 'logits_rel_l2': max(r['rel_l2'] for r in eight),
                                     'worst_sample': max(eight, key=lambda r: r['rel_max'])['model'],
                                     'harsh_trained_like_rel_max_not_asserted': max((r['rel_max'] for r in harsh), default=None)}
            except (OSError, ValueError, KeyError):
                par['worst_of_8'] = None
            try:
                gr = layer_grad_parity(A, c)
                par['grad_rel_max'] = {'sample': 'one cfg-3 decoder layer (dilation 1) forward + backward vs the oracle: worst of dx, dcontext and every parameter gradient, '
                                                 'max-abs error / max-abs reference', **gr}
            except Exception as e:
                par['grad_rel_max'] = {'error': f'{type(e).__name__}: {e}'}
            finally:
                A.set_precision(args.precision)
            out['parity'] = par
        # fp16 saturation monitor over everything this process ran (timed steps included): the COUNTED stores (LayerNorm fp16 copies, cross-attention
        # output copy, fp16-gradient epilogues; include/amdnuwa.h says which clamp without counting): 0 in a healthy run
        if args.full:
            try:
                out.setdefault('parity', {})['f16_saturations'] = K.f16_sat_count(reset=False)
            except Exception as e:
                out.setdefault('parity', {})['f16_saturations'] = f'{type(e).__name__}: {e}'
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
