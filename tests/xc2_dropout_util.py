"""Attention dropout inside SparseCross2DNA (plain helper, like attn_dropout_util.py).

`sparse_cross_2dna_drop` restates oracle.nuwa_oracle.sparse_cross_2dna with the dropout mask of the reference at the reference's position:
the one added line `attn = attn * keep * s` behind the talking-heads mix of the windowed queries (np.py:888-892).  The <bos> query has no
dropout and no talking heads (np.py:826-844).  With keep = 1 and s = 1 it is the oracle function, operation for operation.  It runs in the
dtype of its inputs (fp32 or fp64).  `cross2dna_core_drop64` is the same line inside peaked_util.cross2dna_core64, the float64 statement of
what the kernels themselves compute (rows 1 .. n - 1).

Mask layouts: the kernels read keep as [B, nq, J, heads] (the index order of their ds / P' workspace, J = frames * kernel^2 + 1, slot 0 = the
null key); the module restatement takes the attention-map order (b, heads, query frame, position, slot) of the reference's `attn`, the core
restatement (b, heads, i, j).

The entry-contract helpers run the `_drop` entry points of amdnuwa_cross2dna_fwd / _bwd through the machinery of
tests/test_s3_entry_contract_cpu.py (its geometries, cases and default arguments) without touching that file."""
import torch
import torch.nn.functional as F

FP32_NEG_MAX = -torch.finfo(torch.float32).max


def keep_to_bgfij(keep, tpf):
    """kernel order [B, nq, J, heads] -> the order of the reference's attention map (b, heads, query frame, position in the frame, slot);
    the rows that pad the last query frame are ones (their outputs are cut off)"""
    B, nq, J, heads = keep.shape
    pad = (-nq) % tpf
    k = torch.cat((keep, torch.ones(B, pad, J, heads, dtype=keep.dtype)), 1) if pad else keep
    return k.reshape(B, -1, tpf, J, heads).permute(0, 4, 1, 2, 3)


def sparse_cross_2dna_drop(x, context, P, heads, image_size, kernel_size, dilation, keep, s, context_mask=None):
    """oracle.nuwa_oracle.sparse_cross_2dna with `attn = attn * keep * s` between the mix and the V product.
    keep: (b, h, F, tpf, J) of 0 / 1 (any dtype; keep_to_bgfij), s = 1 / (1 - p)"""
    from oracle.nuwa_oracle import neighbor_table
    b, n, _ = x.shape
    h = heads
    tpf, kn = image_size ** 2, kernel_size ** 2
    if context_mask is None:
        context_mask = torch.ones(b, context.shape[1], dtype=torch.bool)
    inner = P['to_q.weight'].shape[0]
    q = (x @ P['to_q.weight'].t()).reshape(b, n, h, -1).transpose(1, 2) * (inner // h) ** -0.5
    kv = context @ P['to_kv.weight'].t()
    k, v = (t.reshape(b, -1, h, inner // h).transpose(1, 2) for t in kv.chunk(2, dim=-1))      # b h m d
    nk, nv = P['null_k'][None].expand(b, -1, -1, -1), P['null_v'][None].expand(b, -1, -1, -1)
    sm = lambda t: t.softmax(dim=-1, dtype=torch.float32 if t.dtype == torch.float32 else t.dtype)
    sim_bos = torch.einsum('bhd,bhjd->bhj', q[:, :, 0], torch.cat((nk, k), dim=-2))
    sim_bos = sim_bos.masked_fill(~F.pad(context_mask[:, None], (1, 0), value=True), FP32_NEG_MAX)
    out_bos = torch.einsum('bhj,bhjd->bhd', sm(sim_bos), torch.cat((nv, v), dim=-2)).reshape(b, 1, -1)
    if n == 1:
        return out_bos @ P['to_out.weight'].t()
    f = context.shape[1] // tpf
    tab = neighbor_table((1, image_size, image_size), (1, kernel_size, kernel_size), (1, dilation, dilation), causal=False)  # (tpf, kn)
    valid = tab >= 0
    idx = tab.clamp(min=0).reshape(-1)
    gather = lambda t: t.reshape(b, h, f, tpf, -1)[:, :, :, idx].reshape(b, h, f, tpf, kn, -1).permute(0, 1, 3, 2, 4, 5).reshape(b, h, tpf, f * kn, -1)
    kf, vf = gather(k), gather(v)                                                         # slot order (frame, tap), np.py:855
    kf = torch.cat((nk[:, :, None].expand(-1, -1, tpf, -1, -1), kf), dim=-2)
    vf = torch.cat((nv[:, :, None].expand(-1, -1, tpf, -1, -1), vf), dim=-2)
    qr = q[:, :, 1:]
    qr = F.pad(qr, (0, 0, 0, (-qr.shape[2]) % tpf)).reshape(b, h, -1, tpf, qr.shape[-1])
    sim = torch.einsum('bhfid,bhijd->bhfij', qr, kf)
    cm = context_mask.reshape(b, f, tpf)[:, :, idx].reshape(b, f, tpf, kn) & valid[None, None]
    cm = F.pad(cm.permute(0, 2, 1, 3).reshape(b, 1, 1, tpf, f * kn), (1, 0), value=True)
    attn = sm(sim.masked_fill(~cm, FP32_NEG_MAX))
    attn = torch.einsum('gh,bhfij->bgfij', P['talking_heads.weight'].reshape(h, h), attn)
    attn = attn * keep.to(attn.dtype) * s                       # nn.Dropout in training: the one added line
    out = torch.einsum('bhfij,bhijd->bhfid', attn, vf).permute(0, 2, 3, 1, 4).reshape(b, -1, inner)
    return torch.cat((out_bos, out), dim=1)[:, :n] @ P['to_out.weight'].t()


def cross2dna_core_drop64(q, k, v, nk, nv, wth, mask, idx, valid, scale, keep, s):
    """peaked_util.cross2dna_core64 (the windowed queries in float64, rows 1 .. n - 1 -> (B, n - 1, h, d)) with the same added line.
    keep: (b, h, n - 1, J) of 0 / 1, s = 1 / (1 - p)"""
    import peaked_util as PU
    assert q.dtype == torch.float64
    B, n, h, d = q.shape
    sc = PU.cross2dna_scores(q, k, nk, mask, idx, valid, scale)
    attn = torch.einsum('gh,bhij->bgij', wth, sc.softmax(-1))
    attn = attn * keep.to(attn.dtype) * s                       # the one added line
    vg = v[:, idx.reshape(-1)].reshape(B, n - 1, -1, h, d)
    vv = torch.cat((nv[None, None, None].expand(B, n - 1, 1, h, d), vg), 2)
    return torch.einsum('bgij,bijgd->bigd', attn, vv)


# ---------------------------------------------------------------------------------------------------
# entry contract of amdnuwa_cross2dna_fwd_drop / _bwd_drop (tests/test_s3_entry_contract_cpu.py's machinery)
# ---------------------------------------------------------------------------------------------------
DROP_OF = {'amdnuwa_cross2dna_fwd_drop': 'amdnuwa_cross2dna_fwd', 'amdnuwa_cross2dna_bwd_drop': 'amdnuwa_cross2dna_bwd'}


def drop_params(T):
    """parameter names of the two masked entries in declaration order: the unmasked entry's, then keep and drop_scale"""
    return {e: T.PARAMS[u] + ' keep drop_scale' for e, u in DROP_OF.items()}


def call_drop(T, L, entry, g, over):
    """T.call() for a masked cross entry: the defaults of that file (keep = its PTR, drop_scale 1.25) and the overrides `over`"""
    params, lo_of = drop_params(T), T.LO_OF[DROP_OF[entry]]
    over = dict(over)
    if over.pop('all_lo', False):
        over = {**{n: T.PTR for n in lo_of.split()}, **over}
    short = over.pop('ws_short', 0)
    args = []
    for name in params[entry].split():
        if name in over:
            v = T.PTR + 1 if over[name] == 'PTR+1' else over[name]
        elif name == 'workspace_bytes':
            v = (L.amdnuwa_cross2dna_bwd_workspace_bytes(T.ctypes.byref(g)) if g is not None else 0) - short
        elif name == 'ctx_rows':
            v = g.kf * g.H * g.W if g is not None else 0
        elif name.startswith('ld'):
            v = 512
        elif name == 'drop_scale':
            v = 1.25
        elif name.endswith('_lo') or name == 'key_mask':
            v = None
        else:
            v = T.PTR
        args.append(v)
    return getattr(L, entry)(T.ctypes.byref(g) if g is not None else None, *args, None)


# the mask cases the two masked entries add to the cross cases of the table: (name, geometry name, geometry keywords, overrides, expected)
OK, ARG, UNSUPPORTED, WORKSPACE = 0, -1, -2, -3
MASK_CASES = [
    ('keep NULL', 'narrow', {}, {'keep': None}, ARG),
    ('keep NULL, B = 0', 'narrow', {'B': 0}, {'keep': None}, ARG),
    ('drop_scale 0.5', 'narrow', {}, {'drop_scale': 0.5}, ARG),
    ('drop_scale 0.5, B = 0', 'narrow', {'B': 0}, {'drop_scale': 0.5}, ARG),
    ('drop_scale NaN', 'narrow', {}, {'drop_scale': float('nan')}, ARG),
    ('drop_scale inf', 'narrow', {}, {'drop_scale': float('inf')}, ARG),
    ('drop_scale inf, B = 0', 'narrow', {'B': 0}, {'drop_scale': float('inf')}, ARG),
    ('wide2, keep NULL', 'wide2', {}, {'keep': None}, ARG),
    ('workspace NULL, keep NULL', 'narrow', {}, {'workspace': None, 'keep': None}, ARG),        # (backward only: the forward has no workspace)
    ('workspace one byte short, keep NULL, B = 0', 'narrow', {'B': 0}, {'ws_short': 1, 'keep': None}, ARG),
    ('LDS need over the limit, keep NULL', 'lds', {}, {'keep': None}, UNSUPPORTED),
    ('dim_head 48, keep NULL, drop_scale 0.5', 'dh48', {}, {'keep': None, 'drop_scale': 0.5}, UNSUPPORTED),
    ('drop_scale 1, B = 0', 'narrow', {'B': 0}, {'drop_scale': 1.0}, OK),
    ('keep misaligned by one byte, B = 0', 'narrow', {'B': 0}, {'keep': 'PTR+1'}, OK),           # no alignment rule: never a band kernel
    ('band geometry, keep misaligned by one byte, hi + lo operands, B = 0', 'band', {'B': 0}, {'keep': 'PTR+1', 'all_lo': True}, OK),
]
