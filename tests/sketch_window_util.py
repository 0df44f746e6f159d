"""Shared by tests/test_sketch_window_cpu.py and tests/test_gpu_sketch_window.py (plain helper, like gpu_util.py): the gather formula of
one SparseCross2DNA query through a slot table, and the NUWASketch configuration whose window has 300 slots."""
import torch
import torch.nn.functional as F

# SKETCH_KW of tests/test_gpu_modules.py with 12 sketch frames and a 5 x 5 window: 12 * 25 = 300 slots per query
WINDOW_KW = dict(dim=32, image_size=16, max_video_frames=3, sketch_max_video_frames=12, sketch_enc_depth=2, sketch_enc_dim_head=16,
                 sketch_enc_heads=2, dec_depth=3, dec_dim_head=32, dec_heads=2, cross_2dna_kernel_size=5, cross_2dna_dilation=1,
                 sparse_3dna_kernel_size=3, sparse_3dna_dilation=(1, 2))
SKETCH_FRAMES = 12
SKETCH_ID_SEED = 5                 # the stubbed sketch tokenizer: seeded random ids in [0, 48)


def sketch_ids(batch=2, frames=SKETCH_FRAMES, tpf=16):
    return torch.randint(0, 48, (batch, frames * tpf), generator=torch.Generator().manual_seed(SKETCH_ID_SEED))


def sketch_mask(batch=2, frames=SKETCH_FRAMES):
    """hides sketch frames 7.. of sample 1"""
    m = torch.ones(batch, frames, dtype=torch.bool)
    m[1, 7:] = False
    return m


def window_formula(q, kv, rows, nk, nv, wth, mask, scale):
    """one query per sample through one row of a slot table, in the dtype of q: q [B, inner]; kv [B, T, 2 * inner] (k | v); rows int [J],
    the context row of every slot, negative = padding; nk / nv [heads, dh]; wth [heads, heads]; mask bool [B, T] or None.  Null key at
    slot 0 (always visible), scores q . k * scale, hidden slots (padding, masked rows) filled with -max, softmax over the J + 1 slots,
    talking-heads mix without bias, . V.  Values of padding slots never enter the arithmetic (they may be NaN)."""
    B, (heads, dh) = q.shape[0], nk.shape
    inner = heads * dh
    named = rows >= 0
    idx = rows.clamp(min=0).long()
    win = torch.where(named[None, :, None], kv[:, idx], torch.zeros((), dtype=kv.dtype, device=kv.device))
    J = rows.shape[0]
    k, v = win[..., :inner].reshape(B, J, heads, dh), win[..., inner:].reshape(B, J, heads, dh)
    kk = torch.cat((nk[None, None].expand(B, 1, heads, dh), k), 1)
    vv = torch.cat((nv[None, None].expand(B, 1, heads, dh), v), 1)
    sim = torch.einsum('bhd,bjhd->bhj', q.reshape(B, heads, dh) * scale, kk)
    vis = named[None].expand(B, J) if mask is None else named[None] & mask[:, idx]
    sim = sim.masked_fill(~F.pad(vis, (1, 0), value=True)[:, None], -torch.finfo(q.dtype).max)
    attn = torch.einsum('gh,bhj->bgj', wth, sim.softmax(dim=-1))
    return torch.einsum('bgj,bjgd->bgd', attn, vv).reshape(B, inner)
