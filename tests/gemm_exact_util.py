"""Exact-sum cases of the GEMM entry points (gemm.hip): one case list, one descriptor builder, operands whose product has no rounding.

A case names the entry (amdnuwa_gemm_nt / amdnuwa_gemm_tn), the shape, the descriptor fields and the tuning keys.  desc_of() builds the
amdnuwa_gemm_desc of a case from a table of addresses: the GPU test passes the addresses of guarded buffers, the CPU walk (launch log)
passes fake ones, and both call the C entry through ctypes -- the descriptor that is value-tested is the descriptor that was walked.

Operands (operands()): C = A B^T with A [M, K], B [N, K] ("NT form"; the TN entry stores both transposed).
  * hi parts are integers in [-hmax, hmax] (hmax = 4, smaller where a case says so),
  * lo parts of the hi + lo forms are multiples of 2^-4 with |lo| <= 1/4, non-zero in A only on even k and in B only on odd k: every
    lo x lo product is zero, so the three-MFMA and two-MFMA forms (which drop that term) are exact, and both cross terms are exercised,
  * row i of A is scaled by 2^p_i and row j of B by 2^q_j (random integer exponents in the case's ranges ea / eb), bias_j is an integer
    times 2^(q_j + mid(ea)), the old C of a beta = 1 case an integer times 2^(p_i + q_j); alpha, beta and the device factor are powers of 2.
Every product and every partial sum is then a multiple of lsb_ij = (2^-4 with lo parts) 2^(p_i + q_j); with S = |A| |B|^T the sum of the
magnitudes, S_ij / lsb_ij <= 2^22 (exactness(), asserted for every case by the CPU test) makes every partial sum of every order an
integer multiple of lsb_ij below 2^24 lsb_ij: exact in fp32.  Any accumulation order, any split-K and the MFMA's adder must return the
same bits, so the comparison has no tolerance (expected()).  The widest case of the list spans 2^21.1 (the bound is 2^22); on the MI355X
every route returned the expected bits at that span, so the generator was not narrowed -- see DESIGN.md section 2.3.

GEGLU epilogues: the product (u, or dgg) is exact as above and -- where the gate reads it back from its stored form (the plain rings, the
decomposed paths) -- chosen to be exactly representable in that form (hmax^2 K <= 256 for one bf16), so "the exact u" and "the stored u"
are the same number; the gate outputs are compared per element against float64 erfc-GELU with the bound of row_inputs_util."""
import ctypes as C
import zlib

import torch

P, I, LL, F = C.c_void_p, C.c_int, C.c_longlong, C.c_float
FMAP = 4
BF_EPS, PAIR_EPS, F16_EPS = 2.0 ** -8, 2.0 ** -16, 2.0 ** -11
F16_MAX = 65504.0
SPAN_BITS = 22
NT, TN = 'amdnuwa_gemm_nt', 'amdnuwa_gemm_tn'


class GemmDesc(C.Structure):                # amdnuwa_gemm_desc of include/amdnuwa.h; the CPU test compares it with _lib.GemmDesc
    _fields_ = [('A', P), ('Alo', P), ('strideA', LL), ('lda', I), ('B', P), ('Blo', P), ('strideB', LL), ('ldb', I),
                ('C', P), ('Clo', P), ('strideC', LL), ('ldc', I), ('c_is_bf16', I), ('bias', P), ('alpha', F), ('beta', F),
                ('M', I), ('N', I), ('K', I), ('batch', I), ('shift_ntok', I), ('shift_fmap', I),
                ('batch_inner', I), ('strideA_inner', LL), ('strideB_inner', LL), ('strideC_inner', LL),
                ('C2', P), ('C2lo', P), ('ldc2', I), ('geglu_u', P), ('geglu_u_lo', P), ('ld_u', I), ('c_lo_f16', I), ('ab_f16', I), ('c_f16', I),
                ('alpha_dev', P), ('a_chunk32', I)]


DEFAULTS = dict(ops='bf16',          # operand form: 'bf16', 'x3' (bf16 hi + lo), 'f16', 'f16x2' (fp16 A x fp16 hi + lo B)
                out='f32',           # output form: 'f32', 'bf16', 'bf16x2' (hi + lo), 'bf16+f16' (bf16 and its fp16 copy), 'f16' (ONE fp16 output)
                bias=False, alpha=1.0, beta=0.0, adev=None,
                frames=0,            # > 0: token shift, ntok = 1 + frames * FMAP^2 rows per sample, two samples
                batch=1, inner=0, chunk=False,
                pad=(0, 0, 0),       # extra elements of lda, ldb, ldc over the tight pitch
                geglu=None,          # 'fwd': C = u [M, N] interleaved, C2 = a gelu(gate) [M, N / 2]; 'bwd': product = dgg [M, N], C2 = du [M, 2 N]
                c2lo=False, ulo=False, pad2=0,
                acc_gate=False,      # the gate is computed on the fp32 accumulators (hi + lo ring, fp16 rings), not on the stored u
                hmax=4, ea=(-12, 12), eb=(-12, 12), keys=None)
CASE_KEYS = ('name', 'entry', 'M', 'N', 'K') + tuple(DEFAULTS)


def case(name, entry, M, N, K, keys=None, **kw):
    assert not set(kw) - set(DEFAULTS), set(kw) - set(DEFAULTS)
    c = dict(DEFAULTS, name=name, entry=entry, M=M, N=N, K=K, **kw)
    c['keys'] = dict(keys or {})
    return c


def ntok_of(c):
    return 1 + c['frames'] * FMAP * FMAP


def _r8(n):
    return (n + 7) // 8 * 8


def op_dtype(c):
    return torch.float16 if c['ops'] in ('f16', 'f16x2') else torch.bfloat16


def geometry(c):
    """name -> (rows per batch element, columns, pitch, dtype) of every buffer of the case; 'bias' and 'adev' are 1-row buffers"""
    M, N, K, tn = c['M'], c['N'], c['K'], c['entry'] == TN
    od = op_dtype(c)
    g = {}
    if tn:
        g['A'] = ((M + 31) // 32 * K, 32, 32, od) if c['chunk'] else (K, M, _r8(M) + c['pad'][0], od)
        g['B'] = (K, N, _r8(N) + c['pad'][1], od)
        g['C'] = (M, N, N + c['pad'][2], torch.float32)
    else:
        g['A'] = (M, K, K + c['pad'][0], od)
        g['B'] = (N, K, K + c['pad'][1], od)
        cd = {'f32': torch.float32, 'f16': torch.float16}.get(c['out'], torch.bfloat16)
        g['C'] = (M, N, N + c['pad'][2], cd)
        if c['out'] == 'bf16x2':
            g['Clo'] = (M, N, N + c['pad'][2], torch.bfloat16)
        if c['out'] == 'bf16+f16':
            g['Clo'] = (M, N, N + c['pad'][2], torch.float16)
        gd = torch.float16 if c['ops'] == 'f16' else torch.bfloat16
        if c['geglu'] == 'fwd':
            g['C2'] = (M, N // 2, N // 2 + c['pad2'], gd)
            if c['c2lo']:
                g['C2lo'] = (M, N // 2, N // 2 + c['pad2'], torch.bfloat16)
        if c['geglu'] == 'bwd':
            g['U'] = (M, 2 * N, 2 * N + c['pad2'], torch.bfloat16)
            if c['ulo']:
                g['Ulo'] = g['U']
            g['C2'] = (M, 2 * N, 2 * N + c['pad2'], torch.float16 if c['out'] == 'f16' else torch.bfloat16)
            if c['c2lo']:
                g['C2lo'] = (M, 2 * N, 2 * N + c['pad2'], torch.bfloat16)
        if c['bias']:
            g['bias'] = (1, N, N, torch.float32)
    if c['ops'] == 'x3':
        g['Alo'] = g['A']
    if c['ops'] in ('x3', 'f16x2'):
        g['Blo'] = g['B']
    if c['adev'] is not None:
        g['adev'] = (1, 1, 1, torch.float32)
    return g


INPUTS = ('A', 'Alo', 'B', 'Blo', 'bias', 'adev', 'U', 'Ulo')
OUTPUTS = ('C', 'Clo', 'C2', 'C2lo')


def desc_of(c, ptr, Desc=GemmDesc):
    """the amdnuwa_gemm_desc of case c over the addresses ptr[name] (the names of geometry(c))"""
    g = geometry(c)
    d = Desc()
    for f, n in (('A', 'A'), ('Alo', 'Alo'), ('B', 'B'), ('Blo', 'Blo'), ('C', 'C'), ('Clo', 'Clo'), ('C2', 'C2'), ('C2lo', 'C2lo'),
                 ('geglu_u', 'U'), ('geglu_u_lo', 'Ulo'), ('bias', 'bias'), ('alpha_dev', 'adev')):
        if n in g:
            setattr(d, f, ptr[n])
    d.lda, d.ldb, d.ldc = g['A'][2], g['B'][2], g['C'][2]
    d.M, d.N, d.K, d.batch = c['M'], c['N'], c['K'], c['batch']
    d.alpha, d.beta = c['alpha'], c['beta']
    d.c_is_bf16 = int(c['out'] != 'f32')
    d.c_f16 = int(c['out'] == 'f16')
    d.c_lo_f16 = int(c['out'] == 'bf16+f16' and c['ops'] == 'x3')
    d.ab_f16 = int(c['ops'] in ('f16', 'f16x2'))
    d.a_chunk32 = int(c['chunk'])
    if c['frames']:
        d.shift_ntok, d.shift_fmap = ntok_of(c), FMAP
    per = {n: g[n][0] * g[n][2] for n in 'ABC'}
    if c['inner']:
        d.batch_inner = c['inner']
        d.strideA, d.strideB, d.strideC = (c['inner'] * per[n] for n in 'ABC')
        d.strideA_inner, d.strideB_inner, d.strideC_inner = (per[n] for n in 'ABC')
    elif c['batch'] > 1:
        d.strideA, d.strideB, d.strideC = (per[n] for n in 'ABC')
    if 'C2' in g:
        d.ldc2 = g['C2'][2]
    if 'U' in g:
        d.ld_u = g['U'][2]
    return d


FAKE = {n: 0x10000000 + 0x01000000 * i for i, n in enumerate(INPUTS + OUTPUTS + ('ws',))}      # never dereferenced


def call(L, c, ptr, Desc=GemmDesc, ws=None, ws_bytes=None):
    """runs case c on library L (argtypes are set by the caller or left open) -> return code"""
    d = desc_of(c, ptr, Desc)
    if c['entry'] == NT:
        return L.amdnuwa_gemm_nt(C.byref(d), None)
    nb = L.amdnuwa_gemm_tn_workspace_bytes(C.byref(d)) if ws_bytes is None else ws_bytes
    return L.amdnuwa_gemm_tn(C.byref(d), C.c_void_p(ptr['ws'] if ws is None else ws), C.c_size_t(nb), None)


# ---------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------
def interleave(t, FP):
    """[a (FP) | gate (FP)] columns -> the interleaved-by-8 order (kernels.geglu_interleave, dim 1)"""
    return t.reshape(t.shape[0], 2, FP // 8, 8).transpose(1, 2).reshape(t.shape[0], 2 * FP)


def deinterleave(t, FP):
    return t.reshape(t.shape[0], FP // 8, 2, 8).transpose(1, 2).reshape(t.shape[0], 2 * FP)


def _shift(x, c):
    """token shift of x [b, rows, D] (rows = two samples of ntok tokens)"""
    from oracle.nuwa_oracle import shift_video_tokens
    b, rows, D = x.shape
    nt = ntok_of(c)
    assert rows == 2 * nt
    return shift_video_tokens(x.reshape(b * 2, nt, D), FMAP).reshape(b, rows, D)


def _pow2(e):
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e.double())


def operands(c):
    """float64 CPU tensors of the case: the stored operands Ahi / Alo / Bhi / Blo [batch, M | N, K] (before the token shift), the effective
    ones A_hi / A_lo / B_hi / B_lo (after it), the exponents, bias [N], cold [batch, M, N], u [M, 2 N] (GEGLU backward, [a | gate] order)"""
    gen = torch.Generator().manual_seed(zlib.crc32(c['name'].encode()))
    M, N, K, b, tn, h = c['M'], c['N'], c['K'], c['batch'], c['entry'] == TN, c['hmax']

    def ri(lo, hi, shape):
        return torch.randint(lo, hi + 1, shape, generator=gen).double()
    o = {}
    p, q = ri(*c['ea'], (b, M, 1)), ri(*c['eb'], (b, N, 1))
    sa, sb = _pow2(p), _pow2(q)
    o['Ahi'], o['Bhi'] = ri(-h, h, (b, M, K)) * sa, ri(-h, h, (b, N, K)) * sb
    k = torch.arange(K)
    zero = torch.zeros(())
    o['Alo'] = ri(-4, 4, (b, M, K)) / 16 * sa * (k % 2 == 0) if c['ops'] == 'x3' else zero * o['Ahi']
    if c['ops'] in ('x3', 'f16x2'):
        par = k[None, :].expand(N, K)
        if tn and c['frames']:       # the shift moves the second quarter of B's columns down one token row: keep the lo parts on odd k AFTER it
            cq = -(-N // 4)
            moved = ((torch.arange(N) >= cq) & (torch.arange(N) < 2 * cq))[:, None] & (k % ntok_of(c) != 0)[None, :]      # (<bos> rows stay)
            par = par + moved.long()
        o['Blo'] = ri(-4, 4, (b, N, K)) / 16 * sb * (par % 2 == 1)
    else:
        o['Blo'] = zero * o['Bhi']
    if c['frames'] and not tn:       # NT: A rows are tokens
        o['A_hi'], o['A_lo'] = _shift(o['Ahi'], c), _shift(o['Alo'], c)
        o['B_hi'], o['B_lo'] = o['Bhi'], o['Blo']
    elif c['frames']:                # TN: B [token rows, N]
        o['B_hi'], o['B_lo'] = (_shift(t.transpose(1, 2).contiguous(), c).transpose(1, 2) for t in (o['Bhi'], o['Blo']))
        o['A_hi'], o['A_lo'] = o['Ahi'], o['Alo']
    else:
        o['A_hi'], o['A_lo'], o['B_hi'], o['B_lo'] = o['Ahi'], o['Alo'], o['Bhi'], o['Blo']
    o['p'], o['q'] = p, q
    if c['bias']:
        assert b == 1
        o['bias'] = ri(-4, 4, (N,)) * sb[0, :, 0] * 2.0 ** ((c['ea'][0] + c['ea'][1]) // 2)
    if c['beta']:
        o['cold'] = ri(-4, 4, (b, M, N)) * sa * sb.transpose(1, 2)
    if c['geglu'] == 'bwd':
        u = torch.randn((M, 2 * N), generator=gen) * 2
        uh = u.to(torch.bfloat16).float()
        o['Uhi'] = uh.double()
        o['Ulo'] = ((u - uh).to(torch.bfloat16).double() if c['ulo'] else 0 * uh.double())
    return o


def lsb(x):
    """the largest power of two that divides each element of the float64 tensor x (inf for 0)"""
    m, e = torch.frexp(x.abs())
    mi = (m * 2.0 ** 53).long()
    low = (mi & -mi).double()
    out = low * _pow2(e - 53)
    return torch.where(x == 0, torch.full_like(out, float('inf')), out)


def product(o, dev='cpu'):
    """float64 A B^T [batch, M, N] of the effective operands"""
    a, b = (o['A_hi'] + o['A_lo']).to(dev), (o['B_hi'] + o['B_lo']).to(dev)
    return a @ b.transpose(1, 2)


def result(c, o, dev='cpu'):
    """float64 value of every element of C: alpha (device factor) A B^T + bias + beta C_old"""
    r = product(o, dev) * (c['alpha'] * (c['adev'] if c['adev'] is not None else 1.0))
    if c['bias']:
        r = r + o['bias'].to(dev)
    if c['beta']:
        r = r + c['beta'] * o['cold'].to(dev)
    return r


def exactness(c, o):
    """-> dict(span = max over the elements of log2(S_ij / lsb_ij), S and lsb after the bias and the old C; lolo = the largest lo x lo
    product magnitude sum (must be 0); normal = every stored operand value is exact and normal in its 16-bit type)"""
    dt = op_dtype(c)
    tiny = float(torch.finfo(dt).tiny)
    normal = True
    for n in ('Ahi', 'Alo', 'Bhi', 'Blo'):
        v = o[n]
        normal &= bool((v.to(dt).double() == v).all()) and bool(((v == 0) | (v.abs() >= tiny)).all()) and bool(torch.isfinite(v.to(dt).float()).all())
    aa, ba = o['A_hi'].abs() + o['A_lo'].abs(), o['B_hi'].abs() + o['B_lo'].abs()
    f = abs(c['alpha'] * (c['adev'] if c['adev'] is not None else 1.0))
    S = f * (aa @ ba.transpose(1, 2))
    ra = torch.minimum(lsb(o['A_hi']), lsb(o['A_lo'])).amin(2, keepdim=True)       # [b, M, 1]
    rb = torch.minimum(lsb(o['B_hi']), lsb(o['B_lo'])).amin(2, keepdim=True)       # [b, N, 1]
    low = f * ra * rb.transpose(1, 2)
    if c['bias']:
        S, low = S + o['bias'].abs(), torch.minimum(low, lsb(o['bias']).expand_as(low))
    if c['beta']:
        S, low = S + abs(c['beta']) * o['cold'].abs(), torch.minimum(low, abs(c['beta']) * lsb(o['cold']))
    ok = torch.isfinite(low)
    span = float(torch.log2((S[ok] / low[ok]).clamp(min=1.0)).max()) if bool(ok.any()) else 0.0
    lolo = float((o['A_lo'].abs() @ o['B_lo'].abs().transpose(1, 2)).max())
    return dict(span=span, lolo=lolo, normal=normal)


def _hilo(v32):
    hi = v32.to(torch.bfloat16)
    return hi, (v32 - hi.float()).to(torch.bfloat16)


def c_written(c, fused):
    """False where the entry does not write C: the GEGLU backward inside an epilogue (amdnuwa_gemm_nt_fused, or the fp16 rings)"""
    return not (c['geglu'] == 'bwd' and (fused or c['ops'] == 'f16'))


def stored_product(c, r):
    """what the stored form of C holds of the float64 values r, as float64: the case's gate reads this back unless acc_gate"""
    v = r.float()
    if c['out'] == 'f32':
        return v.double()
    if c['out'] == 'f16':
        return v.half().double()
    if c['out'] == 'bf16x2':
        hi, lo = _hilo(v)
        return hi.double() + lo.double()
    return v.to(torch.bfloat16).double()


def expected(c, o, fused, dev='cpu'):
    """-> (exact, gates).  exact: name -> tensor [batch * rows, columns] the output buffer must equal bit for bit.  gates: list of
    (names whose float values are summed, float64 reference, bound, ok mask, largest finite value of the type), all in [a | gate] order
    for the GEGLU backward ([da | dg], the kernel's interleaved du de-interleaved)."""
    import row_inputs_util as RU
    r = result(c, o, dev)
    assert bool((r.float().double() == r).all()), 'the expected values are not fp32 numbers'
    b, M, N = r.shape
    v = r.float().reshape(b * M, N)
    exact, gates = {}, []
    if c_written(c, fused):
        if c['out'] == 'f32':
            exact['C'] = v
        elif c['out'] == 'f16':
            exact['C'] = v.half()
        elif c['out'] == 'bf16x2':
            exact['C'], exact['Clo'] = _hilo(v)
        else:
            exact['C'] = v.to(torch.bfloat16)
            if c['out'] == 'bf16+f16':
                exact['Clo'] = v.half()
    if c['geglu']:
        f16 = c['ops'] == 'f16'
        src = r[0] if c['acc_gate'] else stored_product(c, r[0])
        if c['geglu'] == 'fwd':
            FP = N // 2
            g = RU.geglu64(deinterleave(src, FP), torch.zeros((M, FP), dtype=torch.float64, device=src.device), FP)
            keys, outs = ('y',), [(('C2', 'C2lo') if c['c2lo'] and not f16 else ('C2',))]
            if f16 and c['c2lo']:
                outs.append(('C2lo',))            # fp16 rings: C2 = the fp16 copy, C2lo = the bf16 copy
        else:
            FP = N
            g = RU.geglu64((o['Uhi'] + o['Ulo']).to(src.device), src, FP)
            keys, outs = ('da', 'dg'), [(('C2', 'C2lo') if c['c2lo'] else ('C2',))]
        for names in outs:
            kind = torch.float16 if (f16 and names == ('C2',) and (c['geglu'] == 'fwd' or c['out'] == 'f16')) else torch.bfloat16
            eps = F16_EPS if kind == torch.float16 else (PAIR_EPS if len(names) == 2 else BF_EPS)
            omax = F16_MAX if kind == torch.float16 else RU.BF16_MAX
            bd = RU.geglu_bounds(g, eps, omax, floor=2.0 ** -25 if kind == torch.float16 else 2.0 ** -126)
            gates.append((names, torch.cat([g[k] for k in keys], 1), torch.cat([bd[k] for k in keys], 1), torch.cat([bd['ok'][k] for k in keys], 1), omax))
    return exact, gates


def stored(c, o):
    """name -> 2-D tensor [batch * rows, columns] of every INPUT buffer of the case in its own type (the layout of geometry(c))"""
    dt, tn, b = op_dtype(c), c['entry'] == TN, c['batch']
    s = {}

    def lay(t, name):                 # [b, rows, K] in NT form -> the stored layout
        if not tn:
            return t.reshape(-1, t.shape[2]).to(dt)
        t = t.transpose(1, 2)          # [b, K, M | N]
        if name == 'A' and c['chunk']:
            K, M = t.shape[1], t.shape[2]
            pl = (M + 31) // 32
            full = torch.full((b, K, pl * 32), float('nan'), dtype=torch.float64)
            full[:, :, :M] = t
            return full.reshape(b, K, pl, 32).permute(0, 2, 1, 3).reshape(-1, 32).to(dt)
        return t.reshape(-1, t.shape[2]).to(dt)
    s['A'], s['B'] = lay(o['Ahi'], 'A'), lay(o['Bhi'], 'B')
    if c['ops'] == 'x3':
        s['Alo'] = lay(o['Alo'], 'A')
    if c['ops'] in ('x3', 'f16x2'):
        s['Blo'] = lay(o['Blo'], 'B')
    if c['bias']:
        s['bias'] = o['bias'].float().reshape(1, -1)
    if c['adev'] is not None:
        s['adev'] = torch.tensor([[c['adev']]], dtype=torch.float32)
    if c['geglu'] == 'bwd':
        s['U'] = interleave(o['Uhi'], c['N']).to(torch.bfloat16)
        if c['ulo']:
            s['Ulo'] = interleave(o['Ulo'], c['N']).to(torch.bfloat16)
    return s


# ---------------------------------------------------------------------------------------------------
# the case list.  Tuning keys (gemm.hip, "Host side"): 0 NT family (5 = 128 register-staged, 2 = 128 direct-to-LDS, 7 = 256 x 256 family,
# 11 = K-step 64 ring, 12 = four-wave kernel for K % 64 == 0), 13 hi + lo off its ring, 20 persistent ring (1 off, 2 forced), 22 four-wave
# kernel (2 = every K % 32 == 0 from 96 up); TN: 6 family (1 register-staged, 2 direct-to-LDS), 8 = 2 staggered wave rows, 23 = 1 no
# four-wave kernel, 25 whole-M kernel (1 off, 2 never direct, 3 general form), 1 / 2 split-K slots / least token rows per split.
# ---------------------------------------------------------------------------------------------------
S256 = ((255, 257), (257, 255), (549, 513))          # (M, N): tile - 1, tile + 1, two tiles and a ragged rest
S128 = ((127, 129), (129, 127), (293, 257))
RING_K = (32, 64, 96, 128, 160)                      # a 4-stage ring of 32: fewer k-steps than stages, as many, one more
K64_K = (64, 128, 192, 96, 160)                      # 96 and 160: the K % 64 == 32 half iteration
NARROW = dict(ea=(-6, 6), eb=(-6, 6))                # cases with a bias or an old C: fewer bits of span for the exponents
F16E = dict(ea=(-6, 6), eb=(-6, 6))                  # fp16 operands: every value normal in fp16
F16O = dict(ea=(-3, 2), eb=(-3, 2), hmax=2)          # an fp16 output: every non-zero expected value normal and finite in fp16
GATE = dict(ea=(-3, 3), eb=(-3, 3))


def _n(n, mult):
    """n rounded down to a multiple of mult, never a multiple of 128"""
    n = n // mult * mult
    return n - mult if n % 128 == 0 else n


def _hm(K, stored_bits=8):
    """largest hmax in (4, 2, 1) whose integer sums over K stay exactly representable in stored_bits significand bits"""
    for h in (4, 2, 1):
        if h * h * K <= 2 ** stored_bits:
            return h
    return 1


def _epi_forms(ops, K, gates, shift=False):
    """the output forms that share the fp32 and the 16-bit epilogue of a bf16 / hi + lo NT kernel: (tag, N multiple, fields)"""
    f = [('f32', 1, {}), ('f32 bias alpha 0.5 ldc+4', 1, dict(bias=True, alpha=0.5, pad=(0, 0, 4), **NARROW)),
         ('bf16', 1, dict(out='bf16')), ('bf16 bias alpha 2 ldc+8', 2, dict(out='bf16', bias=True, alpha=2.0, pad=(8, 8, 8), **NARROW)),
         ('bf16x2', 1, dict(out='bf16x2'))]
    if gates and not shift:
        x3 = ops == 'x3'
        hm = _hm(K)
        if x3:
            f += [('gate fwd u hi+lo', 16, dict(out='bf16x2', geglu='fwd', c2lo=True, hmax=2, **GATE)),
                  ('gate bwd u hi+lo', 8, dict(out='bf16x2', geglu='bwd', c2lo=True, ulo=True, hmax=2, **GATE))]
        else:
            f += [('gate fwd', 16, dict(out='bf16', geglu='fwd', hmax=hm, **GATE)), ('gate bwd', 16, dict(out='bf16', geglu='bwd', hmax=hm, **GATE))]
    return f


def nt_cases():
    out = []

    def add(tag, fam, keys, shapes, Ks, ops, forms, **kw):
        for i, K in enumerate(Ks):
            for j, (ftag, mult, fields) in enumerate(forms(K) if callable(forms) else forms):
                M, N = shapes[(i + j) % len(shapes)]
                f = {**fields, **kw}
                if f.get('frames'):
                    M = 2 * (1 + f['frames'] * FMAP * FMAP)
                if f.get('geglu') == 'bwd':
                    N = N // 2               # (the gate's u and du are [M, 2 N])
                out.append(case(f'nt {fam} {ops} {tag}{ftag} M{M} N{_n(N, mult) if mult > 1 else N} K{K}', NT, M, _n(N, mult) if mult > 1 else N, K, keys, ops=ops, **f))

    # ---- 128 x 128 register-staged (key 0 = 5): any K % 8 == 0; the token shift needs K % 32 == 0
    for ops in ('bf16', 'x3'):
        add('', '128reg', {0: 5}, S128, (8, 40, 72), ops, lambda K, ops=ops: _epi_forms(ops, K, True))
        add('shift ', '128reg', {0: 5}, S128, (32, 64, 96), ops, lambda K, ops=ops: _epi_forms(ops, K, False, True)[:4], frames=4, ea=(-2, 2))
    # ---- 128 x 128 direct-to-LDS (key 0 = 2, and what `auto` takes below 512 tiles)
    add('', '128glds', {0: 2}, S128, RING_K, 'bf16', lambda K: _epi_forms('bf16', K, True))
    add('auto ', '128glds', {}, S128, (32, 96), 'bf16', lambda K: _epi_forms('bf16', K, False)[:3])
    add('shift ', '128glds', {0: 2}, S128, (32, 96, 160), 'bf16', lambda K: _epi_forms('bf16', K, False, True)[:4], frames=9, ea=(-2, 2))
    add('batch3 ', '128glds', {0: 2}, S128[:2], (64,), 'bf16', [('f32', 1, dict(batch=3)), ('bf16 inner2', 1, dict(out='bf16', batch=4, inner=2))])
    # ---- the 256 x 256 ring (key 0 = 7; key 20 = 1 keeps it off the persistent form)
    ring = {0: 7, 20: 1}
    add('', 'ring', ring, S256, RING_K, 'bf16', lambda K: _epi_forms('bf16', K, True))
    add('pitched gate ', 'ring', ring, S256, (64,), 'bf16', [('fwd', 16, dict(out='bf16', geglu='fwd', hmax=2, pad=(8, 8, 8), pad2=8, **GATE)),
                                                             ('bwd', 16, dict(out='bf16', geglu='bwd', hmax=2, pad=(8, 8, 8), pad2=8, **GATE))])
    add('shift ', 'ring', ring, S256, RING_K, 'bf16', lambda K: _epi_forms('bf16', K, False, True)[:4], frames=8, ea=(-2, 2))
    add('shift ', 'ring', ring, S256, (96,), 'bf16', lambda K: _epi_forms('bf16', K, False, True)[:4], frames=17, ea=(-2, 2))
    add('batch2 ', 'ring', ring, S256[:2], (96,), 'bf16', [('f32', 1, dict(batch=2)), ('bf16 inner2', 1, dict(out='bf16', batch=4, inner=2))])
    # ---- its K-step 64 form (key 0 = 11); K = 1376 is what `auto` sends there at training sizes
    add('', 'k64', {0: 11}, S256, K64_K + (1376,), 'bf16', lambda K: _epi_forms('bf16', K, False)[:5] if K < 1000 else
        [('f32', 1, dict(hmax=2, **NARROW)), ('bf16 bias', 1, dict(out='bf16', bias=True, hmax=2, **NARROW))])
    # ---- the persistent ring (key 20 = 2): a handful of tiles, so most workgroups own none, and one walk with a second, partly filled round
    pers = {0: 7, 20: 2}
    add('', 'persistent', pers, S256, (96, 128, 160), 'bf16', lambda K: _epi_forms('bf16', K, True))
    add('two rounds ', 'persistent', pers, ((4349, 4101),), (96,), 'bf16', [('f32 bias', 1, dict(bias=True, **NARROW)), ('bf16', 1, dict(out='bf16'))])
    # ---- the four-wave K-step 64 kernel: key 0 = 12 (K % 64 == 0), key 22 = 2 (every K % 32 == 0 from 96 up)
    w4 = [('f32', 1, {}), ('f32 bias alpha 0.5 ldc+4', 1, dict(bias=True, alpha=0.5, pad=(0, 0, 4), **NARROW)), ('bf16', 1, dict(out='bf16')),
          ('bf16 ldc+8', 2, dict(out='bf16', alpha=2.0, pad=(8, 8, 8)))]
    add('', 'w4k', {0: 12}, S256, (64, 128, 192), 'bf16', w4)
    add('key22 ', 'w4k', {0: 7, 22: 2}, S256, (96, 160, 192), 'bf16', w4 + [('bf16 bias', 1, dict(out='bf16', bias=True, **NARROW)), ('bf16x2', 1, dict(out='bf16x2'))])
    add('batch2 ', 'w4k', {0: 12}, S256[:1], (128,), 'bf16', [('f32', 1, dict(batch=2))])
    # ---- the hi + lo ring (three MFMAs per product; key 0 = 7)
    x3f = lambda K: (_epi_forms('x3', K, False) + [
        ('bf16+f16 bias', 8, dict(out='bf16+f16', bias=True, ea=(-3, 2), eb=(-3, 2), hmax=2)),
        ('gate fwd u hi+lo', 16, dict(out='bf16x2', geglu='fwd', c2lo=True, acc_gate=True, **GATE)),
        ('gate fwd u hi', 16, dict(out='bf16', geglu='fwd', c2lo=True, acc_gate=True, **GATE)),
        ('gate bwd decomposed', 8, dict(out='bf16x2', geglu='bwd', c2lo=True, ulo=True, hmax=2, **GATE))])
    add('', 'x3ring', {0: 7}, S256, RING_K, 'x3', x3f)
    add('batch2 ', 'x3ring', {0: 7}, S256[:1], (96,), 'x3', [('bf16x2', 1, dict(out='bf16x2', batch=2))])
    # ---- fp16 operands: the rings with one MFMA per product (auto: K < 1024 -> the ring; key 20 = 2 its persistent form; key 11 / K = 1376 the
    # K-step 64 ring; key 22 = 2 the four-wave kernel)
    def f16f(K, epi5=True, copy=True, gate=True):
        f = [('f32', 4, dict(**F16E)), ('f32 bias', 4, dict(bias=True, ea=(-4, 4), eb=(-4, 4))), ('bf16', 16, dict(out='bf16', **F16E)),
             ('bf16 bias ldc+8', 16, dict(out='bf16', bias=True, pad=(8, 8, 8), ea=(-4, 4), eb=(-4, 4))),
             ('f16', 16, dict(out='f16', **F16O))]
        if copy:
            f.append(('bf16+f16', 16, dict(out='bf16+f16', **F16O)))
        if gate:
            f += [('gate fwd f16+bf16', 16, dict(out='bf16', geglu='fwd', c2lo=True, acc_gate=True, ea=(-3, 1), eb=(-3, 1))),
                  ('gate fwd f16', 16, dict(out='bf16', geglu='fwd', acc_gate=True, ea=(-3, 1), eb=(-3, 1)))]
        if epi5:
            f.append(('gate bwd f16', 16, dict(out='f16', geglu='bwd', acc_gate=True, ea=(-3, 0), eb=(-3, 0), hmax=2)))
        return f
    add('', 'ring', {}, S256, RING_K, 'f16', f16f)
    add('', 'persistent', {20: 2}, S256, (96, 128, 160), 'f16', f16f)
    add('two rounds ', 'persistent', {20: 2}, ((4349, 4112),), (96,), 'f16', [('f16', 16, dict(out='f16', **F16O)), ('gate bwd f16 full tiles', 16, dict(out='f16', geglu='bwd', acc_gate=True, ea=(-3, 0), eb=(-3, 0), hmax=2))])
    add('full tiles ', 'persistent', {20: 2}, ((512, 512),), (96,), 'f16', [('gate bwd f16', 16, dict(out='f16', geglu='bwd', acc_gate=True, ea=(-3, 0), eb=(-3, 0), hmax=2)),
                                                                           ('gate fwd f16+bf16', 16, dict(out='bf16', geglu='fwd', c2lo=True, acc_gate=True, ea=(-3, 1), eb=(-3, 1)))])
    add('full tiles ', 'ring', {}, ((512, 512),), (96,), 'f16', [('gate bwd f16', 16, dict(out='f16', geglu='bwd', acc_gate=True, ea=(-3, 0), eb=(-3, 0), hmax=2))])
    add('', 'k64', {0: 11}, S256, K64_K, 'f16', lambda K: f16f(K, epi5=False, gate=False))
    add('auto ', 'k64', {}, S256, (1376,), 'f16', [('f32', 4, dict(hmax=2, **F16E)), ('bf16', 16, dict(out='bf16', hmax=2, **F16E)), ('f16', 16, dict(out='f16', ea=(-3, 0), eb=(-3, 0), hmax=1))])
    add('', 'w4k', {22: 2}, S256, (96, 128, 160), 'f16', lambda K: f16f(K, epi5=False, gate=False))
    # ---- fp16 A x fp16 hi + lo B: the two-MFMA form of the hi + lo ring
    x2 = [('f32', 1, dict(**F16E)), ('f32 bias', 1, dict(bias=True, ea=(-4, 4), eb=(-4, 4))), ('bf16', 8, dict(out='bf16', **F16E)),
          ('bf16 bias ldc+8', 8, dict(out='bf16', bias=True, pad=(8, 8, 8), ea=(-4, 4), eb=(-4, 4))), ('bf16+f16', 8, dict(out='bf16+f16', **F16O)),
          ('f16', 8, dict(out='f16', **F16O))]
    add('', 'x2ring', {}, S256, RING_K, 'f16x2', x2)
    # ---- the few-row kernel (auto, M <= 32, plain fp32 FMAs)
    rows = lambda ops: [('f32', 1, {}), ('f32 bias alpha 0.5', 1, dict(bias=True, alpha=0.5, **NARROW)), ('bf16', 1, dict(out='bf16')), ('bf16x2 bias', 1, dict(out='bf16x2', bias=True, **NARROW))]
    for ops in ('bf16', 'x3'):
        add('', 'rows', {}, ((1, 15), (8, 16), (9, 17), (32, 133)), (8, 72, 512, 1032), ops, rows(ops))
    return out


def tn_cases():
    out = []

    def add(tag, fam, keys, shapes, Ks, ops, forms, **kw):
        for i, K in enumerate(Ks):
            for j, (ftag, fields) in enumerate(forms):
                M, N = shapes[(i + j) % len(shapes)]
                f = {**fields, **kw}
                if f.get('frames'):
                    K = 2 * (1 + f['frames'] * FMAP * FMAP)
                out.append(case(f'tn {fam} {ops} {tag}{ftag} M{M} N{N} K{K}', TN, M, N, K, {**keys, **f.pop('morekeys', {})}, ops=ops, **f))
    base = [('beta 0', {}), ('beta 1 alpha 0.5', dict(beta=1.0, alpha=0.5, **NARROW)), ('3 splits', dict(morekeys={1: 1024, 2: 32})),
            ('3 splits beta 1 adev', dict(beta=1.0, adev=0.25, morekeys={1: 1024, 2: 32}, **NARROW)), ('ldc+4 lda+8', dict(pad=(8, 8, 4)))]
    TOK = (1, 31, 33, 65, 96)                              # token rows: one, a step - 1, a step + 1, 64 + 1, three whole steps
    # ---- 128 x 128 register-staged (key 6 = 1; hi + lo operands always)
    add('', '128reg', {6: 1}, S128, TOK, 'bf16', base)
    add('', '128reg', {}, S128, TOK, 'x3', base)
    sh128 = ((127, 128), (129, 96), (293, 160))            # the shift needs N % 32 == 0
    for ops in ('bf16', 'x3'):
        add('shift ', '128reg', {6: 1}, sh128, (0, 0), ops, base[:4], frames=1, eb=(-2, 2))
        add('shift ', '128reg', {6: 1}, sh128, (0,), ops, base[:2], frames=4, eb=(-2, 2))
    # ---- 128 x 128 direct-to-LDS (key 6 = 2): the wide form, the narrow form (N <= 64), the shift form
    add('', '128glds', {6: 2}, S128, TOK, 'bf16', base)
    add('auto ', '128glds', {}, ((255, 300), (300, 129)), (33, 96), 'bf16', base[:2])
    add('narrow ', '128glds', {6: 2}, ((127, 8), (129, 33), (293, 64)), TOK, 'bf16', base)
    add('narrow batch3 ', '128glds', {6: 2, 25: 1}, ((129, 8), (293, 64)), (33, 96), 'bf16', [('beta 0', dict(batch=3)), ('inner2 beta 1', dict(batch=4, inner=2, beta=1.0, **NARROW))])
    add('shift ', '128glds', {6: 2}, sh128, (0, 0), 'bf16', base[:4], frames=1, eb=(-2, 2))
    add('shift ', '128glds', {6: 2}, sh128, (0,), 'bf16', base[:2], frames=4, eb=(-2, 2))
    # ---- the 256 x 256 8-wave ring (key 23 = 1 keeps the products off the four-wave kernel), lock-step and staggered (key 8 = 2)
    s256 = ((257, 259), (300, 257), (549, 513))            # both output dimensions >= 256
    sh256 = ((257, 288), (300, 256), (549, 544))
    for tag, k8 in (('', {}), ('staggered ', {8: 2})):
        add(tag, 'ring', {23: 1, **k8}, s256, TOK + (128, 160), 'bf16', base)
        add(tag + 'shift ', 'ring', k8, sh256, (0, 0), 'bf16', base[:4], frames=1, eb=(-2, 2))
        add(tag + 'shift ', 'ring', k8, sh256, (0,), 'bf16', base[:2], frames=4, eb=(-2, 2))
    add('batch2 ', 'ring', {23: 1}, s256[:1], (65,), 'bf16', [('beta 0', dict(batch=2))])
    # ---- the four-wave kernel: token rows a multiple of 64 from 128 up
    for ops, e in (('bf16', {}), ('f16', F16E)):
        add('', 'w4k', {}, s256, (128, 192, 64 * 37), ops, [(t, {**f, **e} if 'ea' not in f else {**f, 'ea': (-4, 4), 'eb': (-4, 4)}) for t, f in base], hmax=2)
    # ---- the whole-M kernels: batched, N <= 64, 128 < M <= 384; lean form (whole steps of 32 token rows) and general form (key 25 = 3)
    wm = [('beta 0', {}), ('beta 1 alpha 0.5', dict(beta=1.0, alpha=0.5, **NARROW)), ('adev', dict(adev=0.25)), ('2 splits', dict(morekeys={2: 32})),
          ('2 splits beta 1 adev', dict(beta=1.0, adev=0.25, morekeys={2: 32}, **NARROW)), ('chunked A', dict(chunk=True)), ('inner2 chunked A', dict(batch=4, inner=2, chunk=True)),
          ('never direct', dict(morekeys={25: 2}))]
    wms = ((129, 8), (200, 32), (264, 64), (383, 8), (256, 33), (320, 40), (384, 64))
    for ops, e in (('bf16', {}), ('f16', F16E)):
        fs = [(t, {**f, **e} if 'ea' not in f else {**f, 'ea': (-4, 4), 'eb': (-4, 4)}) for t, f in wm]
        add('lean ', 'wholeM', {}, wms, (32, 64, 96, 160, 192, 224), ops, fs, batch=2)
        add('general ', 'wholeM', {25: 3}, wms, (32, 65, 96, 31, 1, 160), ops, fs, batch=2)
        add('odd rows ', 'wholeM', {}, wms, (33, 65), ops, fs[:6], batch=3)
    return out


def all_cases():
    cs = nt_cases() + tn_cases()
    names = [c['name'] for c in cs]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)[:4]
    return cs


def group_of(c):
    """cases of one parametrised GPU test: entry, kernel family, operand form"""
    w = c['name'].split(' ')
    return ' '.join(w[:3])
