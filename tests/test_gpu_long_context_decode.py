"""Cached generate() over text contexts of more than 287 tokens on the MI355X: the rows form of the single-query attention kernel
(amdnuwa_attn_rows, csrc/decode.hip), the long form of the row program's text cross-attention block built on it and on
amdnuwa_attn_decode_rows (decode.IncrementalDecoder(long_context=True)), and the two generate() calls behind their class switch.
Pinned here:
  * every row of the rows form is BIT-identical to the single-row kernel (amdnuwa_attn_decode_rows) on that row alone, hi only and
    hi + lo, with and without a key mask / the talking-heads bias, on a window that starts inside a longer cache;
  * the rows form against a float64 restatement of the formula, with the single-row kernel's own bound;
  * a call of more queries than one chunk of launches takes, on the workspace of one chunk;
  * guarded operands: nothing outside the operands is written, every output row is, a window that leaves the cache writes nothing,
    two launches are bit-identical;
  * the row program over a 320-key context: refused by default, built with long_context=True, its rows equal to the full sequence;
  * teacher-forced cached logits against the REFERENCE's logits (fixtures g21a / g21b: a text of 300 tokens), eager and as a graph;
  * prefill-then-step against all-steps and the full forward, with NaN in every cache row the prefill did not write;
  * NUWA.generate samples the token ids the reference's own generate() sampled, on the cached path with the switch on and on the
    recompute loop with it off; NUWAVideoAudio's dual decoder and generate() likewise."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from golden_util import load  # noqa: E402
from gpu_util import bf_value, report, to_bf_pair  # noqa: E402
from guard_util import guard, guarded  # noqa: E402
from test_gpu_long_generate import TF_CASES, _poison_rows_from, _rows_in, _same, _Spies  # noqa: E402

DEV = 'cuda'
R_MAX = 5
SENTINEL = 123.0                  # exact in bf16
GEOMS = [(2, 32), (3, 32), (8, 64)]
FIXTURES = ['g21a_generate_long_context', 'g21b_generate_long_context_reversible']
MODE_TOL = [('bf16x3', 1e-3), ('bf16x3-fwd', 1e-3), ('bf16', 1e-2)]          # the table of test_gpu_long_generate.TF_CASES


@pytest.fixture(scope='module')
def A():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import nuwa_pytorch_amd
    return nuwa_pytorch_amd


@pytest.fixture(scope='module')
def K(A):
    from nuwa_pytorch_amd import kernels
    return kernels


# ---- 1-4: the kernel ---------------------------------------------------------------------------------------------------------------

def _case(K, B, T, heads, dh, x3, first, seed, R=R_MAX, guard_them=False):
    """Q [B, R, inner]: the query of decoder row r of sample b.  kv [B, cache_rows, 2 * inner] with cache_rows = T + 7 when the window
    starts at first = 3 (T when it starts at 0); every cache row outside the window holds NaN in both images."""
    g = torch.Generator().manual_seed(seed)
    inner = heads * dh
    cache_rows = T + 7 if first else T
    Q = torch.randn(B, R, inner, generator=g)
    kvf = torch.randn(B, cache_rows, 2 * inner, generator=g)
    outside = torch.ones(cache_rows, dtype=torch.bool)
    outside[first:first + T] = False
    kvf[:, outside] = float('nan')
    kv = to_bf_pair(kvf, x3)
    put = (lambda t: None if t is None else guarded(t, device=DEV)) if guard_them else (lambda t: None if t is None else t.to(DEV))
    return dict(Q=Q, kv=K.BF(put(kv.hi), put(kv.lo)), nk=put(torch.randn(heads, dh, generator=g)), nv=put(torch.randn(heads, dh, generator=g)),
                wth=put(torch.randn(heads, heads, generator=g) * 0.5 + torch.eye(heads)), bias=put(torch.randn(heads, generator=g) * 0.3),
                fd=put(torch.full((1,), first, dtype=torch.int32)), first=first, heads=heads, dh=dh, T=T, B=B, R=R, x3=x3, inner=inner,
                put=put, gen=g)


def _masks(c):
    """name -> bool [B, T] or None: no mask; every key hidden; at three splits one whole split (slots 128 .. 255 = window rows 127 ..
    254) hidden for every sample, and 30 % of the other keys of the last sample"""
    B, T = c['B'], c['T']
    out = {'none': None, 'all_hidden': torch.zeros(B, T, dtype=torch.bool)}
    if T >= 256:
        m = torch.ones(B, T, dtype=torch.bool)
        m[B - 1] = torch.rand(T, generator=c['gen']) > 0.3
        m[:, 127:255] = False
        out['split_hidden'] = m
    return out


def _q(K, c, rows):
    """BF [len(rows) or B * R, inner] on the device: Q[:, r] for a single row r, Q[:, :R] sample-major for R rows"""
    q = to_bf_pair(rows.contiguous(), c['x3'])
    return K.BF(c['put'](q.hi), c['put'](q.lo))


def _single(K, c, r, mask_u8, bias):
    return K.attn_decode_rows(_q(K, c, c['Q'][:, r]), c['kv'], c['fd'], c['T'], c['heads'], c['dh'], c['nk'], c['nv'], c['wth'],
                              th_bias=bias, mask_u8=mask_u8)


def _rows(K, c, R, mask_u8, bias, out=None):
    """the rows form on Q[:, :R] -> BF [B, R, inner]"""
    o = K.attn_rows(_q(K, c, c['Q'][:, :R].reshape(c['B'] * R, c['inner'])), c['kv'], c['fd'], c['T'], R, c['heads'], c['dh'], c['nk'],
                    c['nv'], c['wth'], th_bias=bias, mask_u8=mask_u8, out=out)
    shape = (c['B'], R, c['inner'])
    return K.BF(o.hi.reshape(shape), None if o.lo is None else o.lo.reshape(shape))


def _parts(o):
    return [t for t in (o.hi, o.lo) if t is not None]


@pytest.mark.parametrize('x3', [False, True])
@pytest.mark.parametrize('heads,dh', GEOMS)
@pytest.mark.parametrize('T', [1, 127, 128, 300])
def test_rows_are_bit_identical_to_the_single_row_kernel(K, T, heads, dh, x3):
    """T + 1 slots = one key, exactly one split, a second split holding a single slot, three splits.  Row (b, r) of the rows form equals
    amdnuwa_attn_decode_rows on Q[b, r] alone in every bit of both images, for B in {1, 3}, R in {1, 2, 5}, every mask case, with and
    without the talking-heads bias, on the whole cache (first row 0) and on a window at first row 3 of a cache of T + 7 rows"""
    for B in (1, 3):
        for first in (0, 3):
            c = _case(K, B, T, heads, dh, x3, first, seed=7 * T + heads + B + first)
            for mname, mask in _masks(c).items():
                mask_u8 = None if mask is None else mask.to(torch.uint8).to(DEV)
                for bias in (None, c['bias']):
                    ref = [_single(K, c, r, mask_u8, bias) for r in range(R_MAX)]
                    for R in (1, 2, 5):
                        o = _rows(K, c, R, mask_u8, bias)
                        assert (o.lo is not None) == x3
                        tag = f'attn_rows[T={T},{heads}x{dh},x3={x3},B={B},first={first},mask={mname},bias={bias is not None},R={R}]'
                        for part, pick in zip(_parts(o), (lambda t: t.hi, lambda t: t.lo)):
                            _same(tag, part, torch.stack([pick(ref[r]) for r in range(R)], 1))
                            assert bool(torch.isfinite(part.float()).all()), tag


def _formula64(q, kv, first, T, nk, nv, wth, bias, mask, scale):
    """float64 on the values the kernel reads: q [B, R, inner]; null key at slot 0, scores q . k * scale, key mask, softmax over the
    T + 1 slots, talking-heads mix, + bias on every slot, . V -> [B, R, inner]"""
    B, R, _ = q.shape
    heads, dh = nk.shape
    inner = heads * dh
    d = lambda t: t.double().cpu()
    q, kv, nk, nv, wth = d(q), d(kv), d(nk), d(nv), d(wth)
    win = kv[:, first:first + T]
    k, v = win[..., :inner].reshape(B, T, heads, dh), win[..., inner:].reshape(B, T, heads, dh)
    kk = torch.cat((nk[None, None].expand(B, 1, heads, dh), k), 1)
    vv = torch.cat((nv[None, None].expand(B, 1, heads, dh), v), 1)
    sim = torch.einsum('brhd,bjhd->brhj', q.reshape(B, R, heads, dh) * scale, kk)
    if mask is not None:
        sim = sim.masked_fill(~F.pad(mask.cpu(), (1, 0), value=True)[:, None, None], float('-inf'))
    attn = torch.einsum('gh,brhj->brgj', wth, sim.softmax(dim=-1))
    if bias is not None:
        attn = attn + d(bias)[None, None, :, None]
    return torch.einsum('brgj,bjgd->brgd', attn, vv).reshape(B, R, inner)


@pytest.mark.parametrize('x3', [False, True])
@pytest.mark.parametrize('heads,dh', GEOMS)
def test_rows_against_the_float64_formula(K, heads, dh, x3):
    """three splits, B = 3, R = 5, the split-hiding mask and the bias, the window at first row 3; the bound is
    test_gpu_xm_long.test_kernel_against_the_fp32_formula's for the single-row kernel -- the same arithmetic and rounding"""
    c = _case(K, 3, 300, heads, dh, x3, 3, seed=31 + heads)
    mask = _masks(c)['split_hidden']
    o = bf_value(_rows(K, c, R_MAX, mask.to(torch.uint8).to(DEV), c['bias']))
    qv = bf_value(to_bf_pair(c['Q'], x3))
    want = _formula64(qv, bf_value(c['kv']), 3, 300, c['nk'], c['nv'], c['wth'], c['bias'], mask, dh ** -0.5)
    report(f'attn_rows.formula[{heads}x{dh},x3={x3}]', o.double().cpu(), want, 3e-5 if x3 else 2 ** -7)


def test_more_queries_than_one_chunk(K, monkeypatch):
    """B = 2, R = 1025: 2050 queries, two sets of launches (2048 + 2) on the workspace of 2048 queries.  The rows on either side of the
    chunk border (2047, 2048), the last row (2049), the rows around the border between the two samples and row 0 are bit-identical to
    single-row calls on that sample's keys"""
    B, R, T, heads, dh = 2, 1025, 130, 2, 32
    from nuwa_pytorch_amd import _lib
    c = _case(K, B, T, heads, dh, True, 0, seed=5, R=R)
    mask = torch.rand(B, T, generator=c['gen']) > 0.3
    mask_u8 = mask.to(torch.uint8).to(DEV)
    asked = []
    orig_ws = K.workspace
    monkeypatch.setattr(K, 'workspace', lambda nbytes, device: (asked.append(int(nbytes)), orig_ws(nbytes, device))[1])
    out = K.BF(*(torch.full((B * R, c['inner']), SENTINEL, dtype=torch.bfloat16, device=DEV) for _ in range(2)))
    o = _rows(K, c, R, mask_u8, c['bias'], out=out)
    assert asked == [_lib.lib().amdnuwa_attn_decode_rows_workspace_bytes(2048, T, heads, dh)], asked
    for part in _parts(o):
        assert not bool((part.float() == SENTINEL).all(-1).any()), 'a query row was not written'
        assert bool(torch.isfinite(part.float()).all())
    for u in (0, 1024, 1025, 2047, 2048, 2049):
        b, r = divmod(u, R)
        one = dict(c, B=1, kv=K.BF(c['kv'].hi[b:b + 1], c['kv'].lo[b:b + 1]), Q=c['Q'][b:b + 1])
        ref = _single(K, one, r, mask_u8[b:b + 1].contiguous(), c['bias'])
        _same(f'attn_rows.chunks[u={u}].hi', o.hi[b, r], ref.hi[0])
        _same(f'attn_rows.chunks[u={u}].lo', o.lo[b, r], ref.lo[0])


@pytest.mark.parametrize('x3', [False, True])
def test_guarded_operands_invalid_windows_and_repeatability(K, x3):
    """q, kv, the mask, the parameters, o and the workspace between guard bands, o and the workspace NaN-prefilled: nothing outside them
    is written, every o row is written (finite), two launches are bit-identical; a window that leaves [0, cache_rows) on either side
    leaves o as it was"""
    B, T, heads, dh = 3, 300, 8, 64
    c = _case(K, B, T, heads, dh, x3, 3, seed=9, guard_them=True)
    mask_u8 = guarded(_masks(c)['split_hidden'].to(torch.uint8), device=DEV)
    with guard(K) as gd:
        a, b = _rows(K, c, R_MAX, mask_u8, c['bias']), _rows(K, c, R_MAX, mask_u8, c['bias'])
        assert gd.made() >= 4                                   # o and the workspace of either launch at least
        for ta, tb in zip(_parts(a), _parts(b)):
            _same(f'attn_rows.twice[x3={x3}]', ta, tb)
            assert bool(torch.isfinite(ta.float()).all()), 'an output element was not written'
    assert (a.lo is not None) == x3
    full = lambda: guarded(torch.full((B * R_MAX, c['inner']), SENTINEL, dtype=torch.bfloat16), device=DEV)
    for first in (T + 7 - T + 1, -1, 1 << 30):                  # one row too far, before the cache, far behind it
        c['fd'].fill_(first)
        with guard(K):
            o = _rows(K, c, R_MAX, mask_u8, c['bias'], out=K.BF(full(), full() if x3 else None))
        assert all(bool((t.float() == SENTINEL).all()) for t in _parts(o)), f'first row {first}: the window leaves the cache, yet o was written'
    c['fd'].fill_(3)
    with guard(K):
        o = _rows(K, c, R_MAX, mask_u8, c['bias'], out=K.BF(full(), full() if x3 else None))
    for t, ta in zip(_parts(o), _parts(a)):
        _same(f'attn_rows.after_invalid[x3={x3}]', t, ta)


# ---- 5: the row program over a 320-key context -----------------------------------------------------------------------------------------

@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('mode,tol', MODE_TOL)
def test_row_program_over_a_320_key_context(A, mode, tol, masked):
    """the network test_gpu_long_attention.test_routing_guards pins: by default a 320-key context is refused; with long_context=True the
    row program builds -- in every precision mode, the training route's speed thresholds at their defaults -- and its 33 stepped rows
    equal the full-sequence forward_layers of the same mode; the mask hides one whole split (slots 128 .. 255) of sample 1"""
    from nuwa_pytorch_amd.decode import IncrementalDecoder
    torch.manual_seed(13)
    net = A.Transformer(dim=64, depth=1, causal=True, heads=2, dim_head=32, cross_attend=True, sparse_3dna_attn=True,
                        sparse_3dna_video_shape=(2, 4, 4)).to(DEV).eval()
    ctx = torch.randn(2, 320, 64, device=DEV)
    x = torch.randn(2, 33, 64, device=DEV)
    mask = None
    if masked:
        mask = torch.ones(2, 320, dtype=torch.bool, device=DEV)
        mask[1, 127:255] = False
        mask[1, 300:] = False
    pos = torch.zeros(1, dtype=torch.int32, device=DEV)
    A.set_precision(mode)
    try:
        with torch.no_grad():
            with pytest.raises(NotImplementedError):
                IncrementalDecoder(net, 2, 33, ctx, mask, pos)
            dec = IncrementalDecoder(net, 2, 33, ctx, mask, pos, long_context=True)
            cross = [b for b in dec.blocks if b.kind == 'x']
            assert len(cross) == 1 and cross[0].long and cross[0].pk is None and tuple(cross[0].ctx_kv.hi.shape) == (2, 320, 128)
            want = net.forward_layers(x, context=ctx, context_mask=mask)
            got = []
            for t in range(33):
                pos.fill_(t)
                got.append(dec.step(x[:, t].contiguous()))
        report(f'long_context_rows[{mode},masked={masked}]', torch.stack(got, 1), want, tol)
    finally:
        A.set_precision('bf16')


def test_short_contexts_keep_the_packed_images_whatever_the_switch_says(A):
    from nuwa_pytorch_amd.decode import IncrementalDecoder
    net = A.Transformer(dim=64, depth=1, causal=True, heads=2, dim_head=32, cross_attend=True, sparse_3dna_attn=True,
                        sparse_3dna_video_shape=(2, 4, 4)).to(DEV).eval()
    pos = torch.zeros(1, dtype=torch.int32, device=DEV)
    for T in (12, 287):
        dec = IncrementalDecoder(net, 2, 33, torch.randn(2, T, 64, device=DEV), None, pos, long_context=True)
        blk, = [b for b in dec.blocks if b.kind == 'x']
        assert not blk.long and blk.pk is not None and blk.ctx_kv is None


# ---- 6-8: the g21 models -----------------------------------------------------------------------------------------------------------------

def _g21(A, name):
    Ar, P, _ = load(name)
    vae = A.VQGanVAE(dim=32, image_size=16, num_layers=2, vq_codebook_size=64, vq_codebook_dim=32, use_vgg_and_gan=False)
    m = A.NUWA(vae=vae, dim=32, text_num_tokens=50, text_max_seq_len=300, max_video_frames=3, text_enc_depth=2, dec_depth=3,
               enc_reversible=True, dec_reversible=bool(Ar['reversible']), dec_heads=2, dec_dim_head=32, text_enc_heads=2,
               text_enc_dim_head=16, sparse_3dna_kernel_size=3, sparse_3dna_dilation=(1, 2))
    missing, unexpected = m.load_state_dict(P, strict=False)
    assert not unexpected, unexpected
    assert float(Ar['min_gap']) >= 3e-3                  # the fixture's condition on its inputs: no near tie under greedy sampling
    return Ar, m.to(DEV).eval()


def _teacher_inputs(nuwa, Ar):
    text = Ar['text'].to(DEV)
    mask = text != 0
    return nuwa.embed_text(text, mask=mask), mask, _rows_in(nuwa, Ar['video_ids'].long().to(DEV)[:, :47])


@pytest.mark.parametrize('graph', [False, True])
@pytest.mark.parametrize('mode,tol', MODE_TOL)
@pytest.mark.parametrize('name', FIXTURES)
def test_teacher_forced_cached_logits_match_the_reference(A, name, mode, tol, graph):
    """the REFERENCE's conditioned logits on its own first 48 ids under a text of 300 tokens (sample 1: 120 tokens + padding, the second
    split of its context wholly hidden): the cached decoder, fed the same rows one at a time, must reproduce every row"""
    from nuwa_pytorch_amd.decode import GuidedStepper
    Ar, nuwa = _g21(A, name)
    A.set_precision(mode)
    try:
        with torch.no_grad():
            emb, mask, rows = _teacher_inputs(nuwa, Ar)
            with pytest.raises(NotImplementedError):
                GuidedStepper(nuwa, emb, mask, 48, 1., graph=graph)
            st = GuidedStepper(nuwa, emb, mask, 48, 1., graph=graph, long_context=True)
            assert all(b.long for b in st.cond.blocks if b.kind == 'x')
            got = torch.stack([st(rows[:, t]).clone() for t in range(48)], 1)
            assert (st.graph is not None) == graph
        report(f'long_context_cached_logits[{name},{mode},graph={graph}]', got, Ar['cond_logits'], tol)
    finally:
        A.set_precision('bf16')


@pytest.mark.parametrize('mode,tol,cond_scale,graph,reversible', TF_CASES)
def test_prefill_then_step_matches_all_steps_and_the_full_forward(A, mode, tol, cond_scale, graph, reversible):
    """test_gpu_long_generate's test of the same name on the g21 models: the cross-attention of the prefill is amdnuwa_attn_rows over the
    300 context rows (the text-masked pass: its constant row replicated).  After the prefill every cache row >= R is NaN: all logits
    must stay finite"""
    from nuwa_pytorch_amd.decode import GuidedStepper
    Ar, nuwa = _g21(A, FIXTURES[int(reversible)])
    A.set_precision(mode)
    try:
        with torch.no_grad():
            emb, mask, rows = _teacher_inputs(nuwa, Ar)
            n = rows.shape[1]
            hidden = nuwa.decode_hidden(rows, emb, mask)
            cond_ref = ref = nuwa._final(hidden)
            if cond_scale != 1:
                un = nuwa._final(nuwa.decode_hidden(nuwa.video_transformer.norm(hidden), emb, torch.zeros_like(mask)))
                ref = un + (cond_ref - un) * cond_scale
            st_all = GuidedStepper(nuwa, emb, mask, n, cond_scale, graph=graph, long_context=True)
            stepped = torch.stack([st_all(rows[:, t]).clone() for t in range(n)], 1)
            tag = f'[{mode},cs={cond_scale},graph={graph},rev={reversible}]'
            report('long_context_prefill.all_steps_vs_full' + tag, stepped, ref, tol)
            if cond_scale == 1:
                report('long_context_prefill.all_steps_vs_reference' + tag, stepped, Ar['cond_logits'], tol)
            for R in (1, 17, 40):
                st = GuidedStepper(nuwa, emb, mask, n, cond_scale, graph=graph, long_context=True)
                h = st.prefill(rows[:, :R].contiguous())
                assert int(st.pos_dev) == R
                _poison_rows_from(st, R)
                got = torch.stack([st(rows[:, t]).clone() for t in range(R, n)], 1)
                assert bool(torch.isfinite(got).all()), f'{tag}[R={R}]: a step read a cache row nothing had written'
                report(f'long_context_prefill.hidden_vs_full{tag}[R={R}]', nuwa._final(h), cond_ref[:, :R], tol)
                report(f'long_context_prefill.then_step_vs_all_steps{tag}[R={R}]', got, stepped[:, R:], tol)
                report(f'long_context_prefill.then_step_vs_full{tag}[R={R}]', got, ref[:, R:], tol)
    finally:
        A.set_precision('bf16')


def _generate(A, m, text, cond_scale, num_frames, graph, long_cache):
    cls = type(m)
    A.set_precision('bf16x3')
    try:
        cls.generate_use_graph, cls.generate_long_context_cache = graph, long_cache
        torch.manual_seed(0)
        m.generate(text=text, filter_thres=0.99, cond_scale=cond_scale, num_frames=num_frames)
    finally:
        cls.generate_use_graph, cls.generate_long_context_cache = True, False
        A.set_precision('bf16')
    return m.last_generated_ids.cpu()


@pytest.mark.parametrize('mode', ['cached+graph', 'cached', 'switch off'])
@pytest.mark.parametrize('name', FIXTURES)
def test_generate_reproduces_the_reference_token_ids(A, monkeypatch, name, mode):
    """fixtures g21: the token ids the REFERENCE's own generate() sampled under a text of 300 tokens for num_frames = 5 on a model of
    max_video_frames = 3 (80 tokens, the window slides at tokens 49 and 65; greedy, guided).  With generate_long_context_cache on, the
    cached row program -- eager and as a captured HIP graph -- samples exactly those ids with TWO prefills and NO recomputed prefix; with
    the switch at its default the same call recomputes the prefix for each of the 80 tokens and samples them too"""
    Ar, m = _g21(A, name)
    assert type(m).generate_long_context_cache is False
    spies = _Spies(monkeypatch, A)
    ids = _generate(A, m, Ar['text'].to(DEV), float(Ar['cond_scale']), int(Ar['num_frames']), mode == 'cached+graph', mode != 'switch off')
    if mode == 'switch off':
        assert (spies.recompute, spies.prefill) == (80, 0), (spies.recompute, spies.prefill)
    else:
        assert (spies.recompute, spies.prefill) == (0, 2), (spies.recompute, spies.prefill)
        assert spies.prefill_rows == [33, 33]            # <bos> + two kept frames
    assert torch.equal(ids, Ar['video_ids'].long()), (ids, Ar['video_ids'])


# ---- 9: NUWAVideoAudio --------------------------------------------------------------------------------------------------------------------

def _va_long(A, reversible):
    from test_gpu_modules import VA_KW
    torch.manual_seed(21)
    vae = A.VQGanVAE(dim=32, image_size=16, num_layers=2, vq_codebook_size=64, vq_codebook_dim=32, use_vgg_and_gan=False)
    m = A.NUWAVideoAudio(vae=vae, sparse_3dna_rel_pos_bias=True, **{**VA_KW, 'text_max_seq_len': 300, 'dec_reversible': reversible})
    m = m.to(DEV).eval()
    with torch.no_grad():                                  # (fresh modules start with a zero Conv3d bias / tap bias: make them count)
        for mod in m.modules():
            if isinstance(mod, torch.nn.Conv3d) and mod.bias is not None:
                mod.bias.normal_(0, 0.3)
    text = torch.randint(1, 50, (2, 300), generator=torch.Generator().manual_seed(4)).to(DEV)
    text[1, 120:] = 0
    return m, text


@pytest.mark.parametrize('reversible', [False, True])
def test_dual_decoder_cached_rows_match_full_sequences_under_a_300_token_text(A, reversible):
    """test_gpu_decode.test_dual_decoder_cached_rows_match_full_sequences with a text of 300 tokens: the text cross-attention of both
    streams attends the context rows in place; refused without long_context"""
    from nuwa_pytorch_amd.decode import DualIncrementalDecoder
    m, text = _va_long(A, reversible)
    gen = torch.Generator().manual_seed(4)
    tpf, apf, F_ = m.num_video_tokens_per_frame, m.num_audio_tokens_per_video_frame, 3
    vids = torch.randint(0, 64, (2, F_ * tpf), generator=gen).to(DEV)
    aids = torch.randint(0, 40, (2, F_ * apf), generator=gen).to(DEV)
    A.set_precision('bf16x3')
    try:
        with torch.no_grad():
            mask = text != 0
            emb = m.embed_text(text, mask=mask)
            v_in, a_in = m.embed_video(vids), m.embed_audio(aids).contiguous()
            dec = m.video_audio_transformer
            v_ref, a_ref = dec.forward_layers(v_in, a_in, context=emb, context_mask=mask)
            with pytest.raises(NotImplementedError):
                DualIncrementalDecoder(dec, 2, v_in.shape[1], a_in.shape[1], emb, mask)
            d = DualIncrementalDecoder(dec, 2, v_in.shape[1], a_in.shape[1], emb, mask, long_context=True)
            for key in 'va':
                cross = [b for b in d.streams[key].blocks if b.kind == 'x']
                assert cross and all(b.long for b in cross)
            v_got, a_got = [d.step('v', v_in[:, 0])], [d.step('a', a_in[:, 0])]
            for f in range(F_):
                for t in range(f * tpf, (f + 1) * tpf):
                    v_got.append(d.step('v', v_in[:, 1 + t]))
                for t in range(f * apf, (f + 1) * apf):
                    a_got.append(d.step('a', a_in[:, 1 + t]))
        report(f'long_context_dual_cached_video_rows[rev={reversible}]', torch.stack(v_got, 1), v_ref, 1e-4)
        report(f'long_context_dual_cached_audio_rows[rev={reversible}]', torch.stack(a_got, 1), a_ref, 1e-4)
    finally:
        A.set_precision('bf16')


@pytest.mark.parametrize('reversible', [False, True])
def test_video_audio_generate_takes_the_cached_path_with_the_switch_on(A, monkeypatch, reversible):
    """NUWAVideoAudio.generate under a text of 300 tokens: with generate_long_context_cache on it runs _generate_cached and returns the
    same ids with and without the HIP graph; with the switch at its default it does not"""
    m, text = _va_long(A, reversible)
    cls = type(m)
    assert cls.generate_long_context_cache is False
    cached_runs = []
    orig_cached = cls._generate_cached
    monkeypatch.setattr(cls, '_generate_cached', lambda self, *a, **k: (cached_runs.append(1), orig_cached(self, *a, **k))[1])
    A.set_precision('bf16x3')
    outs = []
    try:
        for graph in (True, False):
            cls.generate_use_graph, cls.generate_long_context_cache = graph, True
            torch.manual_seed(0)
            outs.append(m.generate(text=text, filter_thres=0.99, cond_scale=2., num_frames=2))
        assert len(cached_runs) == 2
        cls.generate_long_context_cache = False
        torch.manual_seed(0)
        off = m.generate(text=text, filter_thres=0.99, cond_scale=2., num_frames=1)
        assert len(cached_runs) == 2                        # the recompute loop, as before the switch existed
    finally:
        cls.generate_use_graph, cls.generate_long_context_cache = True, False
        A.set_precision('bf16')
    (vg, ag), (v0, a0) = outs
    assert v0.shape == (2, 2, 3, 16, 16) and a0.shape == (2, 2 * m.num_audio_tokens_per_video_frame)
    assert torch.equal(ag, a0) and torch.equal(vg, v0)
    assert off[0].shape == (2, 1, 3, 16, 16) and bool(torch.isfinite(off[0]).all())
