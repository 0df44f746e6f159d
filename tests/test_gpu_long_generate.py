"""Cached generate() past max_video_frames (NUWA.generate, decode.GuidedStepper.prefill, csrc/decode.hip) on the MI355X.

Past the window the reference slides over the last frames (np.py:1873-1881): every kept token moves one frame earlier, so every cached
row changes.  At a slide the caches are rebuilt by one full-sequence pass (the prefill) and the new frame's tokens are single-row steps
again.  Pinned here:
  * the two prefill kernels are BIT-identical to the single-row kernels called R times (guard bands, rows >= R untouched);
  * prefill-then-step reproduces the all-steps decoder and the full forward, teacher-forced, with NaN in every cache row the prefill
    did not write;
  * generate() samples the token ids the REFERENCE's own generate() sampled for 5 frames on a 3-frame model (fixtures g18a / g18b),
    on the cached path with two prefills and no recomputed prefix."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from golden_util import load  # noqa: E402
from gpu_util import report, to_bf_pair  # noqa: E402
from guard_util import guard, guarded  # noqa: E402
from test_gpu_modules import _tiny_nuwa  # noqa: E402

DEV = 'cuda'
ROWS = 33                                   # cache rows: <bos> + two 4 x 4 frames
R_SET = (1, 2, 17, 20, 33)                  # <bos> only, first token, frame border, partial frame, full cache
SENTINEL = 123.0                            # exact in bf16


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


def _bits(t):
    return t.contiguous().view(torch.int16)


def _same(name, got, ref):
    """bit equality of two bf16 / fp32 tensors (NaN patterns included)"""
    g, r = (_bits(got), _bits(ref)) if got.dtype == torch.bfloat16 else (got.contiguous().view(torch.int32), ref.contiguous().view(torch.int32))
    bad = int((g != r).sum())
    assert bad == 0, f'{name}: {bad} of {g.numel()} elements differ bitwise'


def _cache(K, B, cols, x3):
    c = K.BF(guarded(torch.full((B, ROWS, cols), SENTINEL, dtype=torch.bfloat16), device=DEV),
             guarded(torch.full((B, ROWS, cols), SENTINEL, dtype=torch.bfloat16), device=DEV) if x3 else None)
    return c


def _check_cache(name, cache, ref, R):
    for part, rpart in ((cache.hi, ref.hi), (cache.lo, ref.lo)):
        if part is None:
            continue
        _same(f'{name}.cache rows < {R}', part[:, :R], rpart[:, :R])
        assert bool((part[:, R:].float() == SENTINEL).all()), f'{name}: a cache row >= {R} was written'


# what runs around the norms: (fp32 or bf16 y, residual + post-norm, next pre-norm, cache of the next block, fmap)
LN_VARIANTS = [('full', False, True, True, True, 4), ('full.ybf', True, True, True, True, 4), ('no_cache', False, True, True, False, 0),
               ('post_only', False, True, False, False, 0), ('pre_only', False, False, True, True, 4), ('audio', False, True, True, True, -1)]


@pytest.mark.parametrize('x3', [False, True])
@pytest.mark.parametrize('D', [32, 64])
def test_prefill_ln_is_bit_identical_to_decode_ln_row_by_row(K, D, x3):
    """amdnuwa_prefill_ln over R rows per sample against R calls of amdnuwa_decode_ln at pos = 0 .. R-1: x_new, the cache rows and the
    (shifted) operand rows, bit for bit; operands and caches in guarded buffers, cache rows >= R hold a sentinel that must survive"""
    torch.manual_seed(11 + D)
    B = 3
    y, resid = torch.randn(B, ROWS, D) * 1.2, torch.randn(B, ROWS, D)
    w, b, w2, b2 = (guarded(torch.randn(D), device=DEV) for _ in range(4))
    pos = torch.zeros(1, dtype=torch.int32, device=DEV)
    K.set_precision('bf16x3' if x3 else 'bf16')
    try:
        for name, ybf, use_resid, use_next, use_cache, fmap in LN_VARIANTS:
            if name == 'audio' and D != 64:
                continue                                                     # ShiftAudioTokens: once per operand form
            yv = y.bfloat16().float() if ybf else y
            src = yv if use_resid else resid                                 # without a post-norm, y IS the fp32 stream row
            post, nxt = ((w, b) if use_resid else None), ((w2, b2) if use_next else None)
            # the reference: ROWS single-row calls, once; the first R of them are what an R-row prefill must leave
            ref_cache = _cache(K, B, D, x3) if use_cache else None
            xs, hs = [], []
            for t in range(ROWS):
                pos.fill_(t)
                yt = src[:, t].contiguous().to(DEV)
                xn, h = K.decode_ln(K.BF(yt.bfloat16(), None) if ybf else yt, resid[:, t].contiguous().to(DEV) if use_resid else None,
                                    post, nxt, cache=ref_cache, pos_dev=pos if use_cache else None, fmap=fmap)
                xs.append(xn)
                hs.append(h)
            for R in R_SET:
                tag = f'prefill_ln[{name},D={D},x3={x3},R={R}]'
                yr = guarded(src[:, :R].reshape(B * R, D).contiguous(), device=DEV)
                rr = guarded(resid[:, :R].reshape(B * R, D).contiguous(), device=DEV) if use_resid else None
                cache = _cache(K, B, D, x3) if use_cache else None
                with guard(K) as gd:
                    xn, h = K.prefill_ln(K.BF(guarded(yr.bfloat16()), None) if ybf else yr, rr, post, nxt, R, cache=cache, fmap=fmap)
                    assert gd.made() > 0
                if use_resid:
                    _same(tag + '.x_new', xn.reshape(B, R, D), torch.stack(xs[:R], 1))
                else:
                    assert xn is None
                if use_next:
                    _same(tag + '.out.hi', h.hi.reshape(B, R, D), torch.stack([t.hi for t in hs[:R]], 1))
                    assert (h.lo is not None) == x3
                    if x3:
                        _same(tag + '.out.lo', h.lo.reshape(B, R, D), torch.stack([t.lo for t in hs[:R]], 1))
                else:
                    assert h is None
                if use_cache:
                    _check_cache(tag, cache, ref_cache, R)
    finally:
        K.set_precision('bf16')


@pytest.mark.parametrize('x3', [False, True])
@pytest.mark.parametrize('heads,dh', [(2, 32), (8, 64)])
def test_prefill_kv_leaves_the_cache_of_s3_decode_row_by_row(K, heads, dh, x3):
    """amdnuwa_prefill_kv against the key / value cache R calls of amdnuwa_s3_decode leave (the assertion
    test_s3_decode_rows_equal_full_attention makes on it), bit for bit; rows >= R and the guard bands untouched"""
    torch.manual_seed(7 + heads)
    B, inner = 3, heads * dh
    shape, kern, dil = (2, 4, 4), (3, 3, 3), (1, 1, 1)
    qkv = torch.randn(B, ROWS, 3 * inner)
    if not x3:
        qkv = qkv.bfloat16().float()
    wth = (torch.randn(heads, heads) * 0.5 + torch.eye(heads)).to(DEV)
    g = K.s3_geom(B, ROWS, shape, kern, dil, heads, dh)
    ref = K.zeros_bf((B, ROWS, 2 * inner), DEV, lo=x3)
    pos = torch.zeros(1, dtype=torch.int32, device=DEV)
    flat = qkv.to(DEV)
    for t in range(ROWS):
        pos.fill_(t)
        K.s3_decode(g, to_bf_pair(flat[:, t].contiguous(), x3), ref, pos, wth)
    want = to_bf_pair(flat[:, :, inner:].contiguous(), x3)
    _same('s3_decode cache', ref.hi, want.hi)                                 # (the sibling test's assertion: the reference is what it says)
    for R in R_SET:
        rows = to_bf_pair(flat[:, :R].reshape(B * R, 3 * inner).contiguous(), x3)
        rows = K.BF(guarded(rows.hi), guarded(rows.lo) if x3 else None)
        cache = _cache(K, B, 2 * inner, x3)
        with guard(K):
            K.prefill_kv(rows, cache, R)
        _check_cache(f'prefill_kv[{heads}x{dh},x3={x3},R={R}]', cache, ref, R)


# ---- prefill then step, teacher-forced -------------------------------------------------------------------------------------

def _load_g5(A, reversible=False):
    Ar, P, _ = load('g6_nuwa_tiny_reversible' if reversible else 'g5_nuwa_tiny')
    nuwa = _tiny_nuwa(A, reversible)
    nuwa.load_state_dict(P, strict=False)
    return Ar, nuwa.to(DEV).eval()


def _rows_in(nuwa, ids):
    """decoder input rows for token ids [B, m]: <bos>, then embedding + position"""
    with torch.no_grad():
        pos = nuwa.video_pos_emb()
        emb = nuwa.image_embedding(ids) + pos[:ids.shape[1]]
        return torch.cat((nuwa.video_bos[None, None].expand(ids.shape[0], 1, -1), emb), 1)


def _poison_rows_from(stepper, R):
    """NaN in every cache row >= R of every block of both passes: a step that read a row before the step that writes it would show"""
    for dec in (stepper.cond, stepper.uncond):
        if dec is None:
            continue
        for blk in dec.blocks:
            for c in (blk.hcache, blk.kvcache):
                if c is not None:
                    c.hi[:, R:] = float('nan')
                    if c.lo is not None:
                        c.lo[:, R:] = float('nan')


# the tolerance table of test_gpu_decode.test_teacher_forced_cached_logits_match_reference_golden; 'bf16x3' over the whole matrix, the
# other two modes on the guided graph path (the one generate() runs)
TF_CASES = [('bf16x3', 1e-3, cs, graph, rev) for cs in (1., 2.5) for graph in (False, True) for rev in (False, True)] + \
           [(mode, tol, 2.5, True, rev) for mode, tol in (('bf16x3-fwd', 1e-3), ('bf16', 1e-2)) for rev in (False, True)]


@pytest.mark.parametrize('mode,tol,cond_scale,graph,reversible', TF_CASES)
def test_prefill_then_step_matches_all_steps_and_the_full_forward(A, mode, tol, cond_scale, graph, reversible):
    """GuidedStepper.prefill(rows[:, :R]) followed by single-row steps for the remaining rows, against (a) the stepper fed every row one by
    one and (b) the full-sequence forward (decode_hidden, guided as np.py:1894-1898); R = <bos> alone, one frame + <bos>, 2.5 frames.
    The first block's pre-norm cache is the same LayerNorm of the same input on both paths: bit-identical.  After the prefill every cache
    row >= R is NaN: all logits must stay finite."""
    from nuwa_pytorch_amd.decode import GuidedStepper
    Ar, nuwa = _load_g5(A, reversible)
    A.set_precision(mode)
    try:
        with torch.no_grad():
            text = Ar['text'].to(DEV)
            ids = Ar['video_ids'].to(DEV).reshape(2, -1)[:, :-1]
            mask = text != 0
            emb = nuwa.embed_text(text, mask=mask)
            rows = _rows_in(nuwa, ids)
            n = rows.shape[1]
            hidden = nuwa.decode_hidden(rows, emb, mask)
            cond_ref = ref = nuwa._final(hidden)
            if cond_scale != 1:
                un = nuwa._final(nuwa.decode_hidden(nuwa.video_transformer.norm(hidden), emb, torch.zeros_like(mask)))
                ref = un + (cond_ref - un) * cond_scale
            st_all = GuidedStepper(nuwa, emb, mask, n, cond_scale, graph=graph)
            stepped = torch.stack([st_all(rows[:, t]).clone() for t in range(n)], 1)
            first_all = st_all.cond.blocks[0].hcache
            assert first_all is not None
            tag = f'[{mode},cs={cond_scale},graph={graph},rev={reversible}]'
            report('prefill.all_steps_vs_full' + tag, stepped, ref, tol)
            for R in (1, 17, 40):
                st = GuidedStepper(nuwa, emb, mask, n, cond_scale, graph=graph)
                assert st.max_rows == n
                h = st.prefill(rows[:, :R].contiguous())
                assert int(st.pos_dev) == R
                first = st.cond.blocks[0].hcache
                _same(f'prefill.first_hcache.hi{tag}[R={R}]', first.hi[:, :R], first_all.hi[:, :R])
                if first.lo is not None:
                    _same(f'prefill.first_hcache.lo{tag}[R={R}]', first.lo[:, :R], first_all.lo[:, :R])
                _poison_rows_from(st, R)
                got = torch.stack([st(rows[:, t]).clone() for t in range(R, n)], 1)
                assert bool(torch.isfinite(got).all()), f'{tag}[R={R}]: a step read a cache row nothing had written'
                report(f'prefill.hidden_vs_full{tag}[R={R}]', nuwa._final(h), cond_ref[:, :R], tol)
                report(f'prefill.then_step_vs_all_steps{tag}[R={R}]', got, stepped[:, R:], tol)
                report(f'prefill.then_step_vs_full{tag}[R={R}]', got, ref[:, R:], tol)
    finally:
        A.set_precision('bf16')


# ---- generate() --------------------------------------------------------------------------------------------------------------

class _Spies:
    """call counters on NUWA._guided_last_logits (one recomputed prefix) and GuidedStepper.prefill (one cache rebuild)"""

    def __init__(self, monkeypatch, A):
        from nuwa_pytorch_amd.decode import GuidedStepper
        self.recompute = self.prefill = 0
        self.prefill_rows = []
        orig_r, orig_p = A.NUWA._guided_last_logits, GuidedStepper.prefill

        def spy_r(m, *a, **kw):
            self.recompute += 1
            return orig_r(m, *a, **kw)

        def spy_p(st, rows):
            self.prefill += 1
            self.prefill_rows.append(rows.shape[1])
            return orig_p(st, rows)

        monkeypatch.setattr(A.NUWA, '_guided_last_logits', spy_r)
        monkeypatch.setattr(GuidedStepper, 'prefill', spy_p)


def _generate(A, m, text, cond_scale, num_frames, mode, slide=True):
    """mode: 'cached+graph' | 'cached' | 'recompute'"""
    cls = type(m)
    A.set_precision('bf16x3')
    try:
        cls.generate_use_cache, cls.generate_use_graph, cls.generate_slide_cache = mode != 'recompute', mode == 'cached+graph', slide
        torch.manual_seed(0)
        m.generate(text=text, filter_thres=0.99, cond_scale=cond_scale, num_frames=num_frames)
    finally:
        cls.generate_use_cache = cls.generate_use_graph = cls.generate_slide_cache = True
        A.set_precision('bf16')
    return m.last_generated_ids.cpu()


def _fixture_model(A, name):
    Ar, P, _ = load(name)
    m = _tiny_nuwa(A, bool(Ar['reversible']))
    missing, unexpected = m.load_state_dict(P, strict=False)
    assert not unexpected, unexpected
    assert float(Ar['min_gap']) >= 3e-3                  # the fixture's condition on its inputs: no near tie under greedy sampling
    return Ar, m.to(DEV).eval()


@pytest.mark.parametrize('mode', ['cached+graph', 'cached', 'recompute'])
@pytest.mark.parametrize('name', ['g18a_generate_long_nuwa', 'g18b_generate_long_nuwa_reversible'])
def test_long_generate_reproduces_the_reference_token_ids(A, monkeypatch, name, mode):
    """fixtures g18: the token ids the REFERENCE's own generate() sampled for num_frames = 5 on a model of max_video_frames = 3 (80
    tokens, the window slides at tokens 49 and 65; greedy, guided).  The cached row program -- eager and as a captured HIP graph -- must
    sample exactly those ids with TWO prefills and NO recomputed prefix; the recompute loop must sample them too"""
    Ar, m = _fixture_model(A, name)
    spies = _Spies(monkeypatch, A)
    ids = _generate(A, m, Ar['text'].to(DEV), float(Ar['cond_scale']), int(Ar['num_frames']), mode)
    assert torch.equal(ids, Ar['video_ids'].long()), (ids, Ar['video_ids'])
    if mode == 'recompute':
        assert (spies.recompute, spies.prefill) == (80, 0)
    else:
        assert (spies.recompute, spies.prefill) == (0, 2), (spies.recompute, spies.prefill)
        assert spies.prefill_rows == [33, 33]            # <bos> + two kept frames


def test_slide_cache_switch_restores_the_recompute_path(A, monkeypatch):
    """generate_slide_cache = False: past the window the whole call runs the recompute loop, every token of it, as before the prefill existed"""
    Ar, m = _fixture_model(A, 'g18a_generate_long_nuwa')
    spies = _Spies(monkeypatch, A)
    ids = _generate(A, m, Ar['text'].to(DEV), float(Ar['cond_scale']), int(Ar['num_frames']), 'cached+graph', slide=False)
    assert (spies.recompute, spies.prefill) == (80, 0)
    assert torch.equal(ids, Ar['video_ids'].long())


def test_inside_the_window_nothing_changes(A, monkeypatch):
    """num_frames <= max_video_frames: no prefill, no recomputed prefix, and the ids of generate_slide_cache = False"""
    Ar, m = _fixture_model(A, 'g18a_generate_long_nuwa')
    spies = _Spies(monkeypatch, A)
    text = Ar['text'].to(DEV)
    a = _generate(A, m, text, 2., 2, 'cached+graph')
    b = _generate(A, m, text, 2., 2, 'cached+graph', slide=False)
    assert (spies.recompute, spies.prefill) == (0, 0)
    assert a.shape == (2, 32) and torch.equal(a, b)
    assert torch.equal(a, Ar['video_ids'].long()[:, :32])           # the first two frames of the long call: the same steps


@pytest.mark.parametrize('reversible', [False, True])
def test_single_frame_window_prefills_the_start_row_alone(A, monkeypatch, reversible):
    """max_video_frames = 1, num_frames = 3: at every slide the window keeps <bos> and the newest token, so the prefill has R = 1 row.
    Cached ids equal the recompute loop's under greedy sampling.  Greedy sampling reproduces only while the arg-max is no near tie, so
    the text is the first of eight seeded candidates for which the RECOMPUTE loop's guided logits keep a top-2 gap of at least the
    fixtures' 3e-3 at every step -- a condition on the inputs, judged on the recompute loop alone, before the cached path runs."""
    from nuwa_pytorch_amd import nuwa_pytorch as NP
    torch.manual_seed(12)
    vae = A.VQGanVAE(dim=32, image_size=16, num_layers=2, vq_codebook_size=64, vq_codebook_dim=32, use_vgg_and_gan=False)
    m = A.NUWA(vae=vae, dim=32, text_num_tokens=50, text_max_seq_len=8, max_video_frames=1, text_enc_depth=2, dec_depth=3,
               enc_reversible=True, dec_reversible=reversible, dec_heads=2, dec_dim_head=32, text_enc_heads=2, text_enc_dim_head=16,
               sparse_3dna_kernel_size=3, sparse_3dna_dilation=(1, 2)).to(DEV).eval()
    gaps = []
    orig = NP.sample_top_fraction

    def sampler(logits, *a, **kw):
        top2 = logits.topk(2, dim=-1).values
        gaps.append(top2[:, 0] - top2[:, 1])
        return orig(logits, *a, **kw)

    monkeypatch.setattr(NP, 'sample_top_fraction', sampler)
    spies = _Spies(monkeypatch, A)
    text = want = None
    for seed in range(1, 9):
        cand = torch.randint(1, 50, (2, 8), generator=torch.Generator().manual_seed(seed)).to(DEV)
        del gaps[:]
        spies.recompute = 0
        ids = _generate(A, m, cand, 2., 3, 'recompute')
        min_gap = float(torch.stack(gaps).min())
        print(f'single_frame_window[rev={reversible}]: text seed {seed}: minimum top-2 gap {min_gap:.3e}')
        assert spies.recompute == 48
        if min_gap >= 3e-3:
            text, want = cand, ids
            break
    assert text is not None, 'no candidate text keeps the recompute loop clear of near ties'
    for mode in ('cached', 'cached+graph'):
        spies.recompute = spies.prefill = 0
        del spies.prefill_rows[:]
        got = _generate(A, m, text, 2., 3, mode)
        assert (spies.recompute, spies.prefill) == (0, 2) and spies.prefill_rows == [1, 1]
        assert got.shape == (2, 48) and torch.equal(got, want), (mode, got, want)
