"""Generates tests/golden/g15_long_attention.npz from the READ-ONLY reference checkout (imported through oracle/ref_shims.py, as
make_golden.py does): the reference's non-causal Attention as cross-attention of a few query rows over a context of 300 keys (more than
the 287 the cross-attention kernels take) with a context mask -- seeded input, context, state dict, output, input and context gradients
and every parameter gradient.  fp32 CPU, dropout 0.

    python tests/golden/make_golden_long_attention.py

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


def g15_long_attention():
    torch.manual_seed(0)
    m = Attention(dim=32, heads=2, dim_head=32)
    torch.manual_seed(1)
    x = torch.randn(2, 20, 32, requires_grad=True)
    context = torch.randn(2, 300, 32, requires_grad=True)
    # sample 0 sees about a quarter of the context, sample 1 none of it (its queries attend the null key alone, so its exact null_k gradient
    # is zero).  Why so few visible keys: the null key's gradient scales with its probability, about 1 / (visible keys), while the
    # 'bf16x3-fwd' mode recomputes the probabilities of its bf16 backward against the statistics of its fp16 forward, which leaves a
    # null-only row a spurious term of some 2^-9 of the row's dP: with most of 300 keys visible the fixture's null_k gradient would sit at
    # that noise floor and test nothing
    context_mask = torch.rand(2, 300) > 0.75
    context_mask[1] = False
    y = m(x, context=context, context_mask=context_mask)
    g = torch.randn_like(y)
    y.backward(g)
    arrs = dict(x=x, context=context, context_mask=context_mask, y=y, dy=g, dx=x.grad, dcontext=context.grad, heads=2)
    arrs.update({'p.' + k: v for k, v in m.state_dict().items()})
    arrs.update({'g.' + k: p.grad for k, p in m.named_parameters() if p.grad is not None})
    path = os.path.join(HERE, 'g15_long_attention.npz')
    np.savez_compressed(path, **{k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrs.items()})
    print(f'g15_long_attention: {os.path.getsize(path) / 1024:.1f} KiB')


if __name__ == '__main__':
    g15_long_attention()
