"""bench.py's command line: the plain run prints the headline line only (every side measurement behind --full), and
--dump-outputs writes the last timed step's loss and decoder gradients -- the same sample on every run, under 64 MB."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _cfg3_with_seeded_grads():
    import bench
    nuwa = bench.build_model(bench.CFGS['cfg3'], 'cpu')
    params = bench.decoder_params(nuwa)
    g = torch.Generator().manual_seed(3)
    for p in params:
        p.grad = torch.randn(p.shape, generator=g)
    return bench, nuwa, params


def test_dump_outputs_is_a_fixed_sample_under_64_mb(tmp_path):
    bench, nuwa, params = _cfg3_with_seeded_grads()
    loss = torch.tensor(9.25)
    bench.dump_outputs(str(tmp_path / 'a'), nuwa, params, loss)
    bench.dump_outputs(str(tmp_path / 'b'), nuwa, params, loss)
    files = sorted(os.path.basename(f) for f in glob.glob(str(tmp_path / 'a' / '*.npy')))
    assert files == sorted(os.path.basename(f) for f in glob.glob(str(tmp_path / 'b' / '*.npy')))
    assert 'loss.npy' in files and len(files) == 1 + len(params)
    assert sum(os.path.getsize(tmp_path / 'a' / f) for f in files) < 64 * 2 ** 20
    names = {id(p): k for k, p in nuwa.named_parameters()}
    for p in params:
        a = np.load(tmp_path / 'a' / f'grad.{names[id(p)]}.npy')
        assert a.dtype == np.float32 and np.array_equal(a, np.load(tmp_path / 'b' / f'grad.{names[id(p)]}.npy'))
        flat = p.grad.reshape(-1).numpy()
        if p.numel() <= bench.DUMP_WHOLE:
            assert np.array_equal(a, flat)
        else:                                   # a sample of the gradient's own values, in flat-position order
            assert 0 < a.size < p.numel() and np.isin(a, flat).all()
    lo = np.load(tmp_path / 'a' / 'loss.npy')
    assert lo.dtype == np.float64 and float(lo) == 9.25


def test_bench_rejects_zero_steps():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '0'], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode != 0 and '--steps' in r.stderr


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only_and_dumps_the_last_step(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    out_dir = tmp_path / 'dump'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1', '--batch', '2',
                        '--dump-outputs', str(out_dir)], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out['steps'] == 2 and out['higher_is_better'] is True and out['unit'] == 'video-tokens/s' and 'single fp16 MFMA on' in out['dtype']
    assert abs(out['value'] - 2 * 2560 * 2 / (out['ms_per_step'] * 2e-3)) < 1e-3 * out['value']
    assert out['roofline']['families'] == {} and not {'parity', 'fast_mode', 'cpu_baseline', 'vae_tokenizer'} & set(out)
    lo = np.load(out_dir / 'loss.npy')
    assert abs(float(lo) - out['config']['loss']) < 1e-6 * abs(out['config']['loss'])
    grads = glob.glob(str(out_dir / 'grad.*.npy'))
    assert len(grads) > 500 and all(np.isfinite(np.load(f)).all() for f in grads)
    assert sum(os.path.getsize(f) for f in grads) < 64 * 2 ** 20
