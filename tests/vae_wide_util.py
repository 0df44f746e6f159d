"""Shared by the wide-map VAE tests and tests/golden/make_golden_vae_wide.py: the recipe that keeps the VQGanAttention softmax from
being flat (a flat one hides key-indexing errors) and the float64 reference of the attention core."""
import math

import torch


def sharp_scale(heads, P, c, gen):
    """q and k are l2-normalised over the SPATIAL axis (quirk Q9): raw scores are of order sqrt(c) / P, so the learned log-scale
    is set to log(2 P / sqrt(c)) + 0.3 N(0, 1) per head: scores of order 1"""
    return math.log(2 * P / math.sqrt(c)) + 0.3 * torch.randn(heads, generator=gen)


def sharpen_attention(module, P, seed=0, cpb_gain=None):
    """every VQGanAttention under `module` (anything with .cpb, .scale and .heads; the reference's class has the same fields):
    scale by sharp_scale, drawn per module in named_modules() order; optionally the last CPB layer's weight times cpb_gain"""
    gen = torch.Generator().manual_seed(1000 + seed)
    with torch.no_grad():
        for _, m in module.named_modules():
            if hasattr(m, 'cpb') and hasattr(m, 'scale') and hasattr(m, 'heads'):
                c = m.to_qkv.out_channels // (3 * m.heads)
                m.scale.copy_(sharp_scale(m.heads, P, c, gen).reshape(m.scale.shape).to(m.scale))
                if cpb_gain is not None:
                    m.cpb.net[-1].weight.mul_(cpb_gain)
    return module


def core_ref64(qkv, bias, scale, heads):
    """softmax(q^T k e^scale + bias) v in float64 on the CPU: qkv [N, 3 heads c, P] (q, k already normalised), bias [heads, P, P]"""
    N, _, P = qkv.shape
    q, k, v = (t.reshape(N, heads, -1, P).double() for t in qkv.cpu().chunk(3, dim=1))
    sim = torch.matmul(q.transpose(-1, -2), k) * scale.cpu().double().reshape(1, heads, 1, 1).exp() + bias.cpu().double()[None]
    attn = sim.softmax(dim=-1)
    return torch.matmul(v, attn.transpose(-1, -2)).reshape(N, -1, P), attn


def gather_table(table, side):
    """[heads, 2S-1, 2S-1] -> [heads, P, P]: bias(i, j) = table[h, y_i - y_j + S-1, x_i - x_j + S-1]"""
    ax = torch.arange(side, device=table.device)
    yx = torch.cartesian_prod(ax, ax).reshape(-1, 2)
    d = yx[:, None] - yx[None] + side - 1
    return table[:, d[..., 0], d[..., 1]]
