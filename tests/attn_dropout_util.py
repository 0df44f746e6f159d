"""Attention dropout inside the window attention (plain helper, like gpu_util.py).

Restatements of the oracle's Sparse3DNA core, SparseCausal2DNA and CrossModalityCrossAttention with the dropout mask of the reference at
the reference's position: `attn = attn * keep * s` after the talking-heads mix in the two window modules (np.py:554-564, 746-752), between
the softmax and the talking-heads Conv3d in the cross-modality attention (np.py:1048-1051).  With keep = 1 and s = 1 every one of them
is its oracle function, operation for operation.  They run in the dtype of their inputs (fp32 or fp64).

Mask layouts: the kernels read keep as [B, nq, J, heads] (the index order of their ds / P' workspace); the restatements take the
attention-map order (b, heads, i, j)."""
import torch
import torch.nn.functional as F


def keep_to_bhij(keep):
    """kernel order [B, nq, J, heads] -> attention-map order (b, heads, i, j)"""
    return keep.permute(0, 3, 1, 2)


def keep_to_kernel(keep):
    """attention-map order (b, heads, i, j) -> kernel order [B, nq, J, heads], contiguous"""
    return keep.permute(0, 2, 3, 1).contiguous()


def sparse3dna_core_drop(q, k, v, w_th, idx, scale, keep, s, rel_pos_bias=None):
    """oracle.nuwa_oracle.sparse3dna_core with `attn = attn * keep * s` between the mix and the V product.
    keep: (b, h, nq, J) of 0 / 1 (any dtype), s = 1 / (1 - p)"""
    b, n, h, d = q.shape
    if n == 1:
        return v.clone()
    nq = n - 1
    K = idx.shape[1]
    tab = idx[:nq]
    valid = tab >= 0
    gidx = tab.clamp(min=0) + 1
    need = int(gidx.max()) + 1
    if k.shape[1] < need:
        k = F.pad(k, (0, 0, 0, 0, 0, need - k.shape[1]))
        v = F.pad(v, (0, 0, 0, 0, 0, need - v.shape[1]))
    qs = q[:, 1:] * scale
    kg = k[:, gidx.reshape(-1)].reshape(b, nq, K, h, d)
    vg = v[:, gidx.reshape(-1)].reshape(b, nq, K, h, d)
    vmask = valid[None, :, :, None, None].to(q.dtype)
    kg = kg * vmask
    vg = vg * vmask
    kb = k[:, :1, None].expand(b, nq, 1, h, d)
    vb = v[:, :1, None].expand(b, nq, 1, h, d)
    kk = torch.cat((kb, kg), dim=2)
    vv = torch.cat((vb, vg), dim=2)
    sim = torch.einsum('bihd,bijhd->bhij', qs, kk)
    if rel_pos_bias is not None:
        sim = sim + F.pad(rel_pos_bias, (1, 0))[None, :, None, :]
    mask = F.pad(~valid, (1, 0), value=False)
    sim = sim.masked_fill(mask[None, None], -torch.finfo(torch.float32).max)
    attn = sim.softmax(dim=-1, dtype=torch.float32 if sim.dtype == torch.float32 else sim.dtype)
    attn = torch.einsum('gh,bhij->bgij', w_th, attn)
    attn = attn * keep.to(attn.dtype) * s                     # nn.Dropout in training: the one added line
    out = torch.einsum('bgij,bijgd->bigd', attn, vv)
    return torch.cat((v[:, :1], out), dim=1)


def sparse3dna_drop(x, P, video_shape, kernel_size, dilation, heads, keep, s, O):
    """oracle.nuwa_oracle.sparse3dna (causal) around sparse3dna_core_drop.  O = the oracle module (neighbour table, axial bias)"""
    b, n, D = x.shape
    inner = P['to_q.weight'].shape[0]
    d = inner // heads
    idx = O.neighbor_table(video_shape, kernel_size, dilation, causal=True)
    q = x @ P['to_q.weight'].t()
    kv = x @ P['to_kv.weight'].t()
    k, v = kv[..., :inner], kv[..., inner:]
    rpb = None
    if 'rel_pos_bias.axial1' in P:
        ks = O._tup3(kernel_size)
        axes = [P[f'rel_pos_bias.axial{i + 1}'] for i in range(sum(1 for t in ks if t > 1))]
        pos = axes[0]
        for ax in axes[1:]:
            pos = pos.unsqueeze(-2) + ax
        rpb = pos.reshape(-1, heads).t()
    sh = lambda t: t.reshape(b, n, heads, d)
    o = sparse3dna_core_drop(sh(q), sh(k), sh(v), P['talking_heads.weight'].reshape(heads, heads), idx, d ** -0.5, keep, s, rpb)
    return o.reshape(b, n, inner) @ P['to_out.weight'].t() + P['to_out.bias']


def sparse_causal_2dna_drop(x, P, heads, kernel_size, dilation, keep, s):
    """oracle.nuwa_oracle.sparse_causal_2dna with `attn = attn * keep * s` after the talking-heads mix (np.py:747-748).
    keep: (b, h, n - 1, kernel_size + 1)"""
    b, n, _ = x.shape
    q, k, v = (x @ P['to_qkv.weight'].t()).chunk(3, dim=-1)
    if n == 1:
        return v @ P['to_out.weight'].t()
    hd = lambda t: t.reshape(b, n, heads, -1).permute(0, 2, 1, 3)
    q, k, v = hd(q), hd(k), hd(v)
    q = q * q.shape[-1] ** -0.5
    m, pad = n - 1, (kernel_size - 1) * dilation
    kp, vp = F.pad(k[:, :, 1:], (0, 0, pad, 0)), F.pad(v[:, :, 1:], (0, 0, pad, 0))
    t = torch.arange(m)
    sims, vals = [(q[:, :, 1:] * k[:, :, :1]).sum(-1)], [v[:, :, :1].expand(-1, -1, m, -1)]
    bias = P['rel_pos_bias.axial1']
    for a in range(kernel_size):
        ka, va = kp[:, :, a * dilation:a * dilation + m], vp[:, :, a * dilation:a * dilation + m]
        s_a = (q[:, :, 1:] * ka).sum(-1) + bias[a][None, :, None]
        valid = (t - (kernel_size - 1 - a) * dilation) >= 0
        sims.append(s_a.masked_fill(~valid[None, None], -torch.finfo(x.dtype).max))
        vals.append(va)
    attn = torch.stack(sims, dim=-1).softmax(dim=-1, dtype=torch.float32 if x.dtype == torch.float32 else x.dtype)
    attn = torch.einsum('gh,bhij->bgij', P['talking_heads.weight'].reshape(heads, heads), attn)
    attn = attn * keep.to(attn.dtype) * s
    out = (attn[..., None] * torch.stack(vals, dim=-2)).sum(-2)
    out = torch.cat((v[:, :, :1], out), dim=2)
    return out.permute(0, 2, 1, 3).reshape(b, n, -1) @ P['to_out.weight'].t()


def cross_modality_cross_attention_drop(seq, context, P, heads, chunk, ctx_chunk, keep, s):
    """oracle.nuwa_oracle.cross_modality_cross_attention with `attn = attn * keep * s` between the softmax and the talking-heads
    Conv3d (np.py:1048-1051).  keep: (b, h, frames, chunk, ctx_chunk + 1)"""
    b, n, d = seq.shape
    body = seq[:, 1:]
    ctx = F.pad(context, (0, 0, ctx_chunk - 1, 0))
    ctx = F.pad(ctx, (0, 0, 0, (-ctx.shape[1]) % ctx_chunk))
    nf = min(-(-body.shape[1] // chunk), ctx.shape[1] // ctx_chunk)
    w_th, b_th = P['talking_heads.weight'].reshape(heads, heads), P['talking_heads.bias']
    outs = []
    for f in range(nf):
        qf = body[:, f * chunk:(f + 1) * chunk]
        qf = F.pad(qf, (0, 0, 0, chunk - qf.shape[1]))
        cf = ctx[:, f * ctx_chunk:(f + 1) * ctx_chunk]
        hd = lambda t: t.reshape(b, t.shape[1], heads, -1).permute(0, 2, 1, 3)
        q = hd(qf @ P['to_q.weight'].t())
        k, v = (hd(t) for t in (cf @ P['to_kv.weight'].t()).chunk(2, dim=-1))
        q = q * q.shape[-1] ** -0.5
        k = torch.cat((P['null_k'][None, :, None].expand(b, -1, -1, -1), k), dim=2)
        v = torch.cat((P['null_v'][None, :, None].expand(b, -1, -1, -1), v), dim=2)
        attn = (q @ k.transpose(-1, -2)).softmax(dim=-1, dtype=torch.float32 if seq.dtype == torch.float32 else seq.dtype)
        attn = attn * keep[:, :, f].to(attn.dtype) * s
        attn = torch.einsum('gh,bhij->bgij', w_th, attn) + b_th[None, :, None, None]
        outs.append((attn @ v).permute(0, 2, 1, 3).reshape(b, chunk, -1) @ P['to_out.weight'].t())
    out = torch.cat(outs, dim=1) if outs else seq.new_zeros(b, 0, d)
    out = F.pad(out, (0, 0, 0, max(0, body.shape[1] - out.shape[1])))[:, :body.shape[1]]
    return F.pad(out, (0, 0, 1, 0))


class FixedMaskDropout(torch.nn.Module):
    """stands in for a module's nn.Dropout: in training it multiplies by a fixed keep mask (broadcastable to the input) and by s"""

    def __init__(self, keep, s):
        super().__init__()
        self.keep, self.s, self.p = keep, s, 1.0 - 1.0 / s
        self.calls = 0

    def forward(self, x):
        if not self.training:
            return x
        self.calls += 1
        return x * self.keep.to(x.dtype).to(x.device) * self.s
