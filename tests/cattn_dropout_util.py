"""Attention dropout inside the plain attention (plain helper, like attn_dropout_util.py).

A restatement of the oracle's Attention (np.py:339-378, oracle.nuwa_oracle.attention / attention_core) with the dropout mask of the
reference at the reference's position: `attn = attn * keep * s` after the talking-heads mix (np.py:370-374,
`self.dropout(self.talking_heads(attn))`).  With keep = 1 and s = 1 it is the oracle function, operation for operation.  It runs in
the dtype of its inputs (fp32 or fp64).

Mask layouts: the restatement takes the attention-map order (b, heads, i, j) with j = 0 the null key; the masked cattn kernels read one
byte per (query, key) pair, bit g = output head g kept: keep [B, n, KP], the same bytes transposed keep_t [B, T, NP] (KP / NP = T / n
rounded up to 32) and keep0 [B, n] for the null slot (ops.cattn_pack_keep)."""
import torch
import torch.nn.functional as F


def attention_core_drop(q, k, v, null_k, null_v, w_th, key_mask, scale, keep, s, causal=False):
    """oracle.nuwa_oracle.attention_core with `attn = attn * keep * s` between the mix and the V product.
    q (b,n,h,d); k, v (b,m,h,d); keep: (b, h, n, m + 1) of 0 / 1 (any dtype), s = 1 / (1 - p)"""
    b, n, h, d = q.shape
    kk = torch.cat((null_k[None, None].expand(b, 1, h, d), k), dim=1)
    vv = torch.cat((null_v[None, None].expand(b, 1, h, d), v), dim=1)
    sim = torch.einsum('bihd,bjhd->bhij', q * scale, kk)
    neg = -torch.finfo(torch.float32).max
    if key_mask is not None:
        km = F.pad(key_mask, (1, 0), value=True)
        sim = sim.masked_fill(~km[:, None, None, :], neg)
    if causal:
        i, j = sim.shape[-2:]
        sim = sim.masked_fill(torch.ones(i, j, dtype=torch.bool).triu_(j - i + 1), neg)
    attn = sim.softmax(dim=-1, dtype=torch.float32 if sim.dtype == torch.float32 else sim.dtype)
    attn = torch.einsum('gh,bhij->bgij', w_th, attn)
    attn = attn * keep.to(attn.dtype) * s                     # nn.Dropout in training: the one added line
    return torch.einsum('bgij,bjgd->bigd', attn, vv)


def attention_drop(x, P, heads, keep, s, O, context=None, context_mask=None, mask=None, rotary=None, causal=False):
    """oracle.nuwa_oracle.attention around attention_core_drop.  O = the oracle module (rotary)"""
    b, n, _ = x.shape
    inner = P['to_q.weight'].shape[0]
    d = inner // heads
    src = context if context is not None else x
    q = (x @ P['to_q.weight'].t()).reshape(b, n, heads, d)
    kv = src @ P['to_kv.weight'].t()
    m = src.shape[1]
    k = kv[..., :inner].reshape(b, m, heads, d)
    v = kv[..., inner:].reshape(b, m, heads, d)
    if context is None and rotary is not None:
        fr = rotary[None, :, None, :]
        q, k, v = (O.apply_rotary(fr, t) for t in (q, k, v))
    km = context_mask if context is not None else mask
    o = attention_core_drop(q, k, v, P['null_k'].reshape(heads, d), P['null_v'].reshape(heads, d),
                            P['talking_heads.weight'].reshape(heads, heads), km, d ** -0.5, keep, s, causal)
    return o.reshape(b, n, inner) @ P['to_out.weight'].t()


def fixed_keep(B, heads, n, T, p, seed=3):
    """a reproducible boolean keep mask (b, heads, i, j) over the T + 1 key slots"""
    gen = torch.Generator().manual_seed(seed)
    return torch.rand((B, heads, n, T + 1), generator=gen) >= p


def unpack_keep(keep, keep0, heads, T):
    """the kernels' mask arrays -> the boolean mask (b, heads, i, j): reads keep [B, n, KP] and keep0 [B, n] only"""
    packed = torch.cat((keep0[:, :, None], keep[:, :, :T]), dim=2)
    return torch.stack([(packed >> g) & 1 for g in range(heads)], dim=1).bool()


def fixed_mask_fn(keep_bhij):
    """a stand-in for ops._cattn_keep_mask that hands out the mask arrays of one fixed boolean mask (b, heads, i, j); .calls counts"""
    from nuwa_pytorch_amd import ops

    def fn(B, n, T, heads, p, device):
        assert tuple(keep_bhij.shape) == (B, heads, n, T + 1), (tuple(keep_bhij.shape), (B, heads, n, T + 1))
        fn.calls += 1
        return ops.cattn_pack_keep(keep_bhij.to(device))
    fn.calls = 0
    return fn
