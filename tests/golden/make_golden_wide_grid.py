"""Generates tests/golden/g15_sparse3dna_wide.npz from the READ-ONLY reference checkout (imported through oracle/ref_shims.py, as
make_golden.py does): the reference's causal Sparse3DNA on a token grid WIDER than 16 columns -- (1, 17, 17) with 8 heads, one column
past what one workgroup row of the window kernels holds -- seeded input, state dict, output, input gradient and every parameter
gradient.  fp32 CPU, dropout 0.

    python tests/golden/make_golden_wide_grid.py

Seeds: torch.manual_seed(0) for parameters, torch.manual_seed(1) for data (make_golden.py's convention).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import ref_shims  # noqa: E402

ref_shims.install()
from nuwa_pytorch.nuwa_pytorch import Sparse3DNA  # noqa: E402


def g15_sparse3dna_wide():
    video_shape, kernel, heads, n = (1, 17, 17), 3, 8, 290
    torch.manual_seed(0)
    m = Sparse3DNA(dim=32, video_shape=video_shape, kernel_size=kernel, heads=heads, dim_head=32, causal=True)
    torch.manual_seed(1)
    x = torch.randn(2, n, 32, requires_grad=True)
    y = m(x)
    g = torch.randn_like(y)
    y.backward(g)
    arrs = dict(x=x, y=y, dy=g, dx=x.grad, heads=heads, video_shape=np.asarray(video_shape), kernel_size=np.asarray((kernel,) * 3))
    arrs.update({'p.' + k: v for k, v in m.state_dict().items()})
    arrs.update({'g.' + k: p.grad for k, p in m.named_parameters() if p.grad is not None})
    path = os.path.join(HERE, 'g15_sparse3dna_wide.npz')
    np.savez_compressed(path, **{k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrs.items()})
    print(f'g15_sparse3dna_wide: {os.path.getsize(path) / 1024:.1f} KiB')


if __name__ == '__main__':
    g15_sparse3dna_wide()
