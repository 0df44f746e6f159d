"""Generates tests/golden/g14_causal_attention.npz from the READ-ONLY reference checkout (imported through oracle/ref_shims.py, as
make_golden.py does): the reference's Attention(causal=True) as plain self-attention with a key mask -- seeded input, state dict,
output, input gradient and every parameter gradient.  fp32 CPU, dropout 0.

    python tests/golden/make_golden_causal.py

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
from nuwa_pytorch.nuwa_pytorch import Attention  # noqa: E402


def g14_causal_attention():
    torch.manual_seed(0)
    m = Attention(dim=32, heads=2, dim_head=32, causal=True)
    torch.manual_seed(1)
    x = torch.randn(2, 70, 32, requires_grad=True)
    mask = torch.rand(2, 70) > 0.25
    mask[1, :3] = False                      # the first queries of sample 1 see the null key alone
    y = m(x, mask=mask)
    g = torch.randn_like(y)
    y.backward(g)
    arrs = dict(x=x, mask=mask, y=y, dy=g, dx=x.grad, heads=2)
    arrs.update({'p.' + k: v for k, v in m.state_dict().items()})
    arrs.update({'g.' + k: p.grad for k, p in m.named_parameters() if p.grad is not None})
    path = os.path.join(HERE, 'g14_causal_attention.npz')
    np.savez_compressed(path, **{k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrs.items()})
    print(f'g14_causal_attention: {os.path.getsize(path) / 1024:.1f} KiB')


if __name__ == '__main__':
    g14_causal_attention()
