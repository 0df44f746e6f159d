"""The case list of the many-head Sparse3DNA window kernels (9 .. 16 heads, csrc/sparse3dna_mh.hip) and the Python restatements of the
host-side sizes their launches rest on.  One list, three readers: tests/test_gpu_s3_mh.py runs every case on the GPU against float64,
tests/test_s3_mh_index_walk_cpu.py hands the same geometries to tools/s3mh_index_walk.cpp, tools/launch_log/cases_s3_mh.py to the launch log.
Cases are dicts in the form of s3_cases_util (its inputs() / held() / tolerances() read them)."""
MH, MH_MIN, NG = 16, 9, 4
S3_LDS_MAX = 160 * 1024 - 2048
FORMS = ('bf16', 'hilo')


def _case(name, grid, heads, dim_head, form, window=(3, 3, 3), dilation=(1, 1, 1), ntok=None, bias=False, B=2):
    full = 1 + grid[0] * grid[1] * grid[2]
    return dict(name=f'{name}-h{heads}x{dim_head}-{form}', group='mh', grid=grid, window=window, dilation=dilation, heads=heads, dim_head=dim_head,
                ntok=full if ntok is None else ntok, B=B, causal=True, form=form, bias=bias, cross=None, keep=None, keys={})


def all_cases():
    c = []
    # narrowest tiles: fewer threads than (g, h) pairs
    c += [_case('g221', (2, 2, 1), 16, 64, 'hilo'), _case('g221', (2, 2, 1), 16, 32, 'bf16')]                       # 64 threads
    c += [_case('g222', (2, 2, 2), 16, d, f) for d in (64, 32) for f in FORMS]                                     # 128 threads, all four
    c += [_case('g233', (2, 3, 3), 9, 64, 'hilo'), _case('g233', (2, 3, 3), 9, 32, 'bf16')]                         # 108 -> 128 threads, idle lanes
    # one full tile
    c += [_case('g248', (2, 4, 8), 16, 64, 'bf16'), _case('g248', (2, 4, 8), 16, 32, 'hilo'), _case('g244', (2, 4, 4), 12, 64, 'hilo')]
    # several tiles: 6 + 6, 7 + 6 (a partial last tile), 10 + 10
    c += [_case('g2312', (2, 3, 12), 16, 64, 'hilo'), _case('g2312', (2, 3, 12), 16, 32, 'bf16')]
    c += [_case('g2313', (2, 3, 13), 16, 64, 'bf16'), _case('g2313', (2, 3, 13), 16, 32, 'hilo')]
    c += [_case('g2220', (2, 2, 20), 9, 64, 'hilo')]
    # sequence ends, one-tile grid (2, 4, 4): mid-row (and mid-frame), at a row end inside the second frame, ntok = 2
    c += [_case('g244-nq22', (2, 4, 4), 12, 64, 'bf16', ntok=23), _case('g244-nq24', (2, 4, 4), 12, 32, 'hilo', ntok=25),
          _case('g244-nq1', (2, 4, 4), 12, 64, 'hilo', ntok=2)]
    # sequence ends, two-tile grid (2, 3, 12): mid-row inside the first tile (the second tile of that row lies wholly beyond the sequence), at a
    # row end inside the second frame, ntok = 2
    c += [_case('g2312-nq51', (2, 3, 12), 16, 64, 'hilo', ntok=52), _case('g2312-nq48', (2, 3, 12), 16, 32, 'bf16', ntok=49),
          _case('g2312-nq1', (2, 3, 12), 16, 64, 'bf16', ntok=2)]
    # window variations
    c += [_case('g2312-dil', (2, 3, 12), 16, 64, 'hilo', dilation=(1, 2, 2)),
          _case('g244-k133', (2, 4, 4), 12, 32, 'hilo', window=(1, 3, 3)),
          _case('g2312-k311', (2, 3, 12), 16, 64, 'bf16', window=(3, 1, 1)),
          _case('g233-bias', (2, 3, 3), 9, 64, 'hilo', bias=True)]
    return c


def slots(c):
    return c['window'][0] * c['window'][1] * c['window'][2] + 1


def tile(c):
    """s3mh_tile() of csrc/s3mh_index.h: (tw, nt, sw)"""
    W, h = c['grid'][2], c['heads']
    if W * h * 4 <= 512:
        return W, 1, W
    twmax = 128 // h
    nt = -(-W // twmax)
    tw = -(-W // nt)
    return tw, nt, tw + (c['window'][2] - 1) * c['dilation'][2]


def threads(c):
    return -(-(tile(c)[0] * c['heads'] * 4) // 64) * 64


def lds(c, lo):
    """s3mh_lds() of csrc/s3mh_index.h: dynamic LDS bytes of (forward, query-side backward, key-side backward)"""
    tw, _, sw = tile(c)
    J, h, inner = slots(c), c['heads'], c['heads'] * c['dim_head']
    stage, nsp = sw * inner * (4 if lo else 2), tw * J * h
    spdp = max(2 * nsp, tw * inner)
    return stage + nsp * 4, stage + (spdp + NG * h * h) * 4, sw * inner * 8


def workspace_bytes(c):
    """s3_ws() of csrc/sparse3dna.hip"""
    B, nq, J, h = c['B'], c['ntok'] - 1, slots(c), c['heads']
    F, H, _ = c['grid']
    items, parts, inner = B * nq * J * h, B * F * H * tile(c)[1], h * c['dim_head']
    floats = 2 * items + parts * h * h + 2 * parts * inner
    R, D = B * nq, J * h
    return floats * 4 + 256 + (R if 1 <= R < 256 else (1 if R < 1 else 256)) * D * 4


def part_th_offset(c):
    """float offset of the dW_th partials [B * F * H * NT][heads * heads] in the workspace"""
    return 2 * c['B'] * (c['ntok'] - 1) * slots(c) * c['heads']


def walk_line(c):
    """one line of the case file of tools/s3mh_index_walk.cpp"""
    F, H, W = c['grid']
    return ' '.join(str(v) for v in (c['B'], c['ntok'], F, H, W, *c['window'], *c['dilation'], c['heads'], c['dim_head'],
                                     1 if c['form'] == 'hilo' else 0, 1 if c['bias'] else 0))


def geom(S3Geom, c, B=None, rel_bias=None, d_rel_bias=None, **over):
    g = S3Geom()
    g.B, g.ntok = c['B'] if B is None else B, c['ntok']
    g.F, g.H, g.W = c['grid']
    g.kf, g.kh, g.kw = c['window']
    g.df, g.dh, g.dw = c['dilation']
    g.heads, g.dim_head, g.scale = c['heads'], c['dim_head'], c['dim_head'] ** -0.5
    g.noncausal = 0
    g.rel_bias, g.d_rel_bias = rel_bias, d_rel_bias          # (addresses or None)
    for k, v in over.items():
        setattr(g, k, v)
    return g
