"""NUWASketch.generate past max_video_frames on the MI355X: the rows form of the single-query SparseCross2DNA kernel
(amdnuwa_cross2dna_rows, csrc/decode.hip), the rows program built on it (decode._Cross2DNARows.attend_rows -> IncrementalDecoder.prefill)
and the long call itself.  Pinned here:
  * every row of the rows form is BIT-identical to the single-row kernel (amdnuwa_cross2dna_decode) at that row's position, hi only and
    hi + lo, on tables with padding and a key mask; the <bos> rows are neither read nor written;
  * the rows form against the fp32 gather formula, with the single-row kernel's own bound;
  * more than 65 535 query rows in one call;
  * guarded operands: nothing outside the named rows is read into a result or written, two launches are bit-identical, R = 1 writes
    nothing, an out-of-range table entry leaves exactly the query rows that use it unwritten;
  * prefill-then-step reproduces the all-steps decoder and the recomputed prefix, teacher-forced, with NaN in every cache row the prefill
    did not write;
  * generate() samples the token ids the REFERENCE's own NUWASketch.generate sampled for 5 frames on a 3-frame model (fixtures g20a /
    g20b), on the cached path with two prefills and no recomputed prefix."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import bf_value, report, to_bf_pair  # noqa: E402
from guard_util import guard, guarded  # noqa: E402
from sketch_window_util import SKETCH_FRAMES, WINDOW_KW, window_formula  # noqa: E402
from test_gpu_long_generate import TF_CASES, _poison_rows_from, _same  # noqa: E402
from test_gpu_sketch_window import _fixture_model  # noqa: E402

DEV = 'cuda'
N_POS = 16
R_MAX = 40                        # rows of the kernel cases: the table is walked more than twice
R_SET = (2, 17, 40)               # the first query alone, one frame + <bos>, 2.5 frames
HIDDEN_POS = 3                    # the feature-map position whose every table entry is -1
SENTINEL = 123.0                  # exact in bf16


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

def _case(K, J, heads, dh, x3, B=2, seed=0):
    """operands in guarded buffers.  Q [B, R_MAX, inner]: the query of decoder row r of sample b, row 0 (<bos>) NaN.  The table names
    EVEN context rows only, about 20 % of its entries are -1 and position HIDDEN_POS is all -1; every odd context row -- named by no
    slot of any position -- holds NaN in both images.  The key mask hides about 30 % of the context rows of sample 1."""
    g = torch.Generator().manual_seed(seed)
    inner, T = heads * dh, 2 * J + 7
    tab = (torch.randint(0, (T + 1) // 2, (N_POS, J), generator=g) * 2).to(torch.int32)
    tab[torch.rand(N_POS, J, generator=g) < 0.2] = -1
    tab[HIDDEN_POS] = -1
    tab[0, 0] = T - 1 if (T - 1) % 2 == 0 else T - 2             # the last even context row and row 0 are named
    tab[1, J - 1] = 0
    Q = torch.randn(B, R_MAX, inner, generator=g)
    Q[:, 0] = float('nan')
    kvf = torch.randn(B, T, 2 * inner, generator=g)
    kvf[:, 1::2] = float('nan')
    kv = to_bf_pair(kvf, x3)
    mask = torch.ones(B, T, dtype=torch.bool)
    mask[B - 1] = torch.rand(T, generator=g) > 0.3
    gd = lambda t: None if t is None else guarded(t, device=DEV)
    return dict(Q=Q, kv=K.BF(gd(kv.hi), gd(kv.lo)), tab=gd(tab), mask=gd(mask), mask_u8=gd(mask.to(torch.uint8)),
                nk=gd(torch.randn(heads, dh, generator=g)), nv=gd(torch.randn(heads, dh, generator=g)),
                wth=gd(torch.randn(heads, heads, generator=g) * 0.5 + torch.eye(heads)), pos=gd(torch.ones(1, dtype=torch.int32)),
                heads=heads, dh=dh, T=T, J=J, B=B, x3=x3, inner=inner)


def _q_rows(K, c, R):
    """q BF [B * R, inner], sample-major, guarded"""
    q = to_bf_pair(c['Q'][:, :R].reshape(c['B'] * R, c['inner']).contiguous(), c['x3'])
    return K.BF(guarded(q.hi, device=DEV), None if q.lo is None else guarded(q.lo, device=DEV))


def _sentinels(K, c, R):
    full = lambda: guarded(torch.full((c['B'] * R, c['inner']), SENTINEL, dtype=torch.bfloat16), device=DEV)
    return K.BF(full(), full() if c['x3'] else None)


def _rows(K, c, R, q=None):
    """the rows form into an output of sentinels -> BF [B, R, inner]"""
    o = K.cross2dna_rows(_q_rows(K, c, R) if q is None else q, c['kv'], c['tab'], R, c['heads'], c['dh'], c['nk'], c['nv'], c['wth'],
                         mask_u8=c['mask_u8'], out=_sentinels(K, c, R))
    shape = (c['B'], R, c['inner'])
    return K.BF(o.hi.reshape(shape), None if o.lo is None else o.lo.reshape(shape))


def _single_rows(K, c, rows=range(1, R_MAX)):
    """the single-row kernel at pos = r on Q[:, r] for every r -> {r: BF [B, inner]}"""
    out = {}
    for r in rows:
        c['pos'].fill_(r)
        q = to_bf_pair(c['Q'][:, r].contiguous(), c['x3'])
        q = K.BF(q.hi.to(DEV), None if q.lo is None else q.lo.to(DEV))
        out[r] = K.cross2dna_decode(q, c['kv'], c['tab'], c['pos'], c['heads'], c['dh'], c['nk'], c['nv'], c['wth'], mask_u8=c['mask_u8'])
    return out


def _is_sentinel(t):
    return bool((t.float() == SENTINEL).all())


@pytest.mark.parametrize('x3', [False, True])
@pytest.mark.parametrize('heads,dh', [(2, 32), (8, 64)])
@pytest.mark.parametrize('J', [24, 127, 128, 300])
def test_rows_are_bit_identical_to_the_single_row_kernel(K, J, heads, dh, x3):
    """J + 1 slots = one split, exactly one full split, a second split of one slot, three splits.  Row (b, r) of the rows form equals
    amdnuwa_cross2dna_decode on Q[b, r] at pos = r in every bit of both images; row 0 of every sample keeps its sentinel (and its NaN
    query reaches nothing)"""
    c = _case(K, J, heads, dh, x3, seed=J + heads)
    ref = _single_rows(K, c)
    for R in R_SET:
        with guard(K) as gd:
            o = _rows(K, c, R)
            assert gd.made() >= 1                              # the workspace at least
        assert (o.lo is not None) == x3
        for part, pick in ((o.hi, lambda t: t.hi), (o.lo, lambda t: t.lo)):
            if part is None:
                continue
            assert _is_sentinel(part[:, 0]), f'R={R}: a <bos> row was written'
            _same(f'cross2dna_rows[J={J},{heads}x{dh},x3={x3},R={R}]', part[:, 1:], torch.stack([pick(ref[r]) for r in range(1, R)], 1))
            assert bool(torch.isfinite(part[:, 1:].float()).all())


@pytest.mark.parametrize('x3', [False, True])
@pytest.mark.parametrize('J,heads,dh', [(24, 2, 32), (300, 8, 64), (128, 3, 64)])
def test_rows_against_the_fp32_formula(K, J, heads, dh, x3):
    """the rows form against sketch_window_util.window_formula through every row's table row, on the values the kernel reads; the bound
    is test_gpu_sketch_window.test_kernel_against_the_fp32_formula's for the single-row kernel (the same arithmetic and rounding)"""
    c = _case(K, J, heads, dh, x3, B=3, seed=5 * J + heads)
    R = R_MAX
    q = _q_rows(K, c, R)
    with guard(K):
        o = bf_value(_rows(K, c, R, q=q))
    qv = bf_value(q).reshape(c['B'], R, c['inner'])
    kvv = bf_value(c['kv'])                                    # (the NaN rows are named by no slot: the formula never gathers them)
    want = torch.stack([window_formula(qv[:, r], kvv, c['tab'][(r - 1) % N_POS], c['nk'], c['nv'], c['wth'], c['mask'], dh ** -0.5)
                        for r in range(1, R)], 1)
    report(f'cross2dna_rows.formula[J={J},{heads}x{dh},x3={x3}]', o[:, 1:], want, 3e-5 if x3 else 2 ** -7)


@pytest.mark.parametrize('B,R', [(2, 32801), (16400, 5)])
def test_more_query_rows_than_a_grid_dimension_holds(K, B, R):
    """B * (R - 1) = 65 600 query rows in one call (heads 1, dim_head 32, one slot, one feature-map position): every row equals the
    single-row result -- the case a grid that counts query rows on y or z gets wrong or refuses.  Two samples with the same query on all
    their rows against ONE single-row launch; 16 400 samples with four queries each against four."""
    assert B * (R - 1) == 65600
    g = torch.Generator().manual_seed(B)
    inner, T = 32, 3
    uniq = 1 if B == 2 else R - 1                              # distinct queries per sample
    Qu = torch.randn(B, uniq, inner, generator=g)
    Q = torch.cat((torch.full((B, 1, inner), float('nan')), Qu.expand(B, R - 1, inner) if uniq == 1 else Qu), 1)
    kv = to_bf_pair(torch.randn(B, T, 2 * inner, generator=g).to(DEV), True)
    tab = torch.tensor([[1]], dtype=torch.int32, device=DEV)
    nk, nv = torch.randn(1, 32, generator=g).to(DEV), torch.randn(1, 32, generator=g).to(DEV)
    wth = torch.tensor([[0.75]], device=DEV)
    pos = torch.ones(1, dtype=torch.int32, device=DEV)
    q = to_bf_pair(Q.reshape(B * R, inner).to(DEV), True)
    out = K.BF(*(torch.full((B * R, inner), SENTINEL, dtype=torch.bfloat16, device=DEV) for _ in range(2)))
    o = K.cross2dna_rows(q, kv, tab, R, 1, 32, nk, nv, wth, out=out)
    for u in range(uniq):
        ref = K.cross2dna_decode(to_bf_pair(Qu[:, u].contiguous().to(DEV), True), kv, tab, pos, 1, 32, nk, nv, wth)
        for got, want in ((o.hi, ref.hi), (o.lo, ref.lo)):
            got = got.reshape(B, R, inner)
            assert _is_sentinel(got[:, 0])
            rows = got[:, 1:] if uniq == 1 else got[:, 1 + u:2 + u]
            _same(f'cross2dna_rows.many[B={B},R={R},u={u}]', rows, want[:, None].expand_as(rows))
    assert bool(torch.isfinite(bf_value(o).reshape(B, R, inner)[:, 1:]).all())


@pytest.mark.parametrize('x3', [False, True])
def test_guarded_operands_invalid_rows_and_repeatability(K, x3):
    """q, kv, o, the table and the workspace between guard bands; NaN in every context row no slot names and in q row 0 reaches no output
    (the case's inputs); two launches are bit-identical; R = 1 writes nothing; a table row with an entry >= ctx_rows leaves exactly the
    query rows that use it unwritten and every other row as it was"""
    c = _case(K, 300, 8, 64, x3, B=3, seed=9)
    R = R_MAX
    with guard(K) as gd:
        a, b = _rows(K, c, R), _rows(K, c, R)
        assert gd.made() >= 2
    parts = lambda o: [t for t in (o.hi, o.lo) if t is not None]
    for ta, tb in zip(parts(a), parts(b)):
        _same(f'cross2dna_rows.twice[x3={x3}]', ta, tb)
        assert _is_sentinel(ta[:, 0]) and bool(torch.isfinite(ta.float()).all())
        assert not bool((ta[:, 1:].float() == SENTINEL).all(-1).any())          # every query row was written
    with guard(K):
        one = _rows(K, c, 1)
    assert all(_is_sentinel(t) for t in parts(one))
    bad_pos = 5
    c['tab'][bad_pos, 299] = c['T']                             # in the LAST split: every workgroup of the three launches must agree
    with guard(K):
        o = _rows(K, c, R)
    uses = torch.tensor([r >= 1 and (r - 1) % N_POS == bad_pos for r in range(R)], device=DEV)
    assert int(uses.sum()) == 3
    for t, ta in zip(parts(o), parts(a)):
        assert _is_sentinel(t[:, uses]), 'a query row whose table row leaves the context was written'
        assert _is_sentinel(t[:, 0])
        _same(f'cross2dna_rows.after_invalid[x3={x3}]', t[:, ~uses], ta[:, ~uses])


# ---- 5: prefill then step, teacher-forced ----------------------------------------------------------------------------------------------

def _context(m, Ar):
    ids = Ar['sketch_ids']
    sketch = torch.zeros(ids.shape[0], ids.shape[1] // 16, 3, 16, 16, device=DEV)       # only its shape is read: the tokenizer is stubbed
    return m.embed_sketch(sketch, mask=Ar['sketch_mask'].to(DEV) if 'sketch_mask' in Ar else None)


def _rows_in(m, ids):
    """decoder input rows for token ids [B, n]: <bos>, then embedding + position"""
    pos = m.video_pos_emb()
    return torch.cat((m.video_bos[None, None].expand(ids.shape[0], 1, -1), m.image_embedding(ids) + pos[:ids.shape[1]]), 1)


class _Calls:
    """call counters on attributes of a class or module"""

    def __init__(self, monkeypatch, owner, *names):
        self.n = {name: 0 for name in names}
        for name in names:
            monkeypatch.setattr(owner, name, self._wrap(getattr(owner, name), name))

    def _wrap(self, orig, name):
        def spy(*a, **kw):
            self.n[name] += 1
            return orig(*a, **kw)
        return spy


def _prefill_then_step(A, K, monkeypatch, m, Ar, mode, tol, cond_scale, graph, tag, n=44, packed=False):
    from nuwa_pytorch_amd.decode import GuidedStepper
    B = Ar['sketch_ids'].shape[0]
    ids = torch.randint(0, 64, (B, n - 1), generator=torch.Generator().manual_seed(3)).to(DEV)
    A.set_precision(mode)
    try:
        with torch.no_grad():
            ctx, cmask = _context(m, Ar)
            rows = _rows_in(m, ids)
            hidden = m.decode_hidden(rows, ctx, cmask)
            cond_ref = ref = m._final(hidden)
            if cond_scale != 1:
                un = m._final(m.decode_hidden(m.video_transformer.norm(hidden), ctx, torch.zeros_like(cmask)))
                ref = un + (cond_ref - un) * cond_scale
            st_all = GuidedStepper(m, ctx, cmask, n, cond_scale, graph=graph)
            xc2 = [b for b in st_all.cond.blocks if b.kind == 'xc2']
            assert xc2 and all(b.c2.packed == packed and b.c2.kv is not None for b in xc2)
            stepped = torch.stack([st_all(rows[:, t]).clone() for t in range(n)], 1)
            first_all = st_all.cond.blocks[0].hcache
            report('sketch_prefill.all_steps_vs_full' + tag, stepped, ref, tol)
            spy = _Calls(monkeypatch, K, 'cross2dna_rows', 'cross2dna_decode', 'xattn_pack')
            for R in (1, 17, 40):
                st = GuidedStepper(m, ctx, cmask, n, cond_scale, graph=graph)
                for k in spy.n:
                    spy.n[k] = 0
                h = st.prefill(rows[:, :R].contiguous())
                assert int(st.pos_dev) == R
                # the rows form reads the window in place on both routes; the text-masked pass launches nothing
                assert spy.n == dict(cross2dna_rows=len(xc2), cross2dna_decode=0, xattn_pack=0), spy.n
                first = st.cond.blocks[0].hcache
                _same(f'sketch_prefill.first_hcache.hi{tag}[R={R}]', first.hi[:, :R], first_all.hi[:, :R])
                if first.lo is not None:
                    _same(f'sketch_prefill.first_hcache.lo{tag}[R={R}]', first.lo[:, :R], first_all.lo[:, :R])
                _poison_rows_from(st, R)
                got = torch.stack([st(rows[:, t]).clone() for t in range(R, n)], 1)
                assert bool(torch.isfinite(got).all()), f'{tag}[R={R}]: a step read a cache row nothing had written'
                report(f'sketch_prefill.hidden_vs_full{tag}[R={R}]', m._final(h), cond_ref[:, :R], tol)
                report(f'sketch_prefill.then_step_vs_all_steps{tag}[R={R}]', got, stepped[:, R:], tol)
                report(f'sketch_prefill.then_step_vs_full{tag}[R={R}]', got, ref[:, R:], tol)
    finally:
        A.set_precision('bf16')


@pytest.mark.parametrize('mode,tol,cond_scale,graph,reversible', TF_CASES)
def test_prefill_then_step_matches_all_steps_and_the_recomputed_prefix(A, K, monkeypatch, mode, tol, cond_scale, graph, reversible):
    """the 300-slot model with the parameters of fixtures g19a / g19b, 44 teacher-forced rows: GuidedStepper.prefill(rows[:, :R]) followed by
    single-row steps, against (a) the stepper fed every row one by one and (b) the recomputed prefix (decode_hidden, guided as
    np.py:1894-1898); R = <bos> alone, one frame + <bos>, 2.5 frames; mode / tolerance table of test_gpu_long_generate.TF_CASES.  After the
    prefill every cache row >= R is NaN: all later logits must stay finite."""
    Ar, m = _fixture_model(A, 'g19b_generate_sketch_window_reversible' if reversible else 'g19a_generate_sketch_window', WINDOW_KW)
    assert Ar['sketch_ids'].shape[1] == SKETCH_FRAMES * 16
    _prefill_then_step(A, K, monkeypatch, m, Ar, mode, tol, cond_scale, graph, f'[{mode},cs={cond_scale},graph={graph},rev={reversible}]')


def test_prefill_reads_the_window_in_place_when_the_rows_take_the_packed_route(A, K, monkeypatch):
    """AMDNUWA_XC2_DECODE_PACKED=1 on a window the packed images hold (SKETCH_KW, 18 slots; the parameters of fixture g13e): the single rows
    gather and pack, the prefill still runs amdnuwa_cross2dna_rows over self.kv -- and the two agree as above"""
    from test_gpu_modules import SKETCH_KW
    monkeypatch.setenv('AMDNUWA_XC2_DECODE_PACKED', '1')
    Ar, m = _fixture_model(A, 'g13e_generate_sketch', SKETCH_KW)
    _prefill_then_step(A, K, monkeypatch, m, Ar, 'bf16x3', 1e-3, 2.5, True, '[packed]', packed=True)


# ---- 6: generate() -------------------------------------------------------------------------------------------------------------------------

class _Spies:
    """call counters on NUWASketch._guided_last_logits (one recomputed prefix) and GuidedStepper.prefill (one cache rebuild)"""

    def __init__(self, monkeypatch, A):
        from nuwa_pytorch_amd.decode import GuidedStepper
        self.recompute = self.prefill = 0
        self.prefill_rows = []
        orig_r, orig_p = A.NUWASketch._guided_last_logits, GuidedStepper.prefill

        def spy_r(m, *a, **kw):
            self.recompute += 1
            return orig_r(m, *a, **kw)

        def spy_p(st, rows):
            self.prefill += 1
            self.prefill_rows.append(rows.shape[1])
            return orig_p(st, rows)

        monkeypatch.setattr(A.NUWASketch, '_guided_last_logits', spy_r)
        monkeypatch.setattr(GuidedStepper, 'prefill', spy_p)


def _generate(A, m, Ar, mode, num_frames=None, slide=True, device_sampler=True):
    """mode: 'cached+graph' | 'cached' | 'recompute'"""
    cls = type(m)
    A.set_precision('bf16x3')
    try:
        cls.generate_use_cache, cls.generate_use_graph, cls.generate_slide_cache = mode != 'recompute', mode == 'cached+graph', slide
        cls.generate_device_sampler = device_sampler
        torch.manual_seed(2)
        ids = Ar['sketch_ids']
        sketch = torch.zeros(ids.shape[0], ids.shape[1] // 16, 3, 16, 16, device=DEV)
        m.generate(sketch=sketch, sketch_mask=Ar['sketch_mask'].to(DEV), filter_thres=0.99, cond_scale=float(Ar['cond_scale']),
                   num_frames=int(Ar['num_frames']) if num_frames is None else num_frames)
    finally:
        cls.generate_use_cache = cls.generate_use_graph = cls.generate_slide_cache = cls.generate_device_sampler = True
        A.set_precision('bf16')
    return m.last_generated_ids.cpu()


def _long_fixture(A, name):
    Ar, m = _fixture_model(A, name, WINDOW_KW)
    assert float(Ar['min_gap']) >= 3e-3                  # the fixture's condition on its inputs: no near tie under greedy sampling
    assert float(Ar['gaps'].min()) == float(Ar['min_gap']) and Ar['gaps'].numel() == 80 and int(Ar['num_frames']) == 5
    return Ar, m


@pytest.mark.parametrize('mode,device_sampler', [('cached+graph', True), ('cached+graph', False), ('cached', True), ('cached', False),
                                                 ('recompute', True)])
@pytest.mark.parametrize('name', ['g20a_generate_sketch_long', 'g20b_generate_sketch_long_reversible'])
def test_long_generate_reproduces_the_reference_token_ids(A, monkeypatch, name, mode, device_sampler):
    """fixtures g20: the token ids the REFERENCE's own NUWASketch.generate sampled for num_frames = 5 on the 300-slot model of
    max_video_frames = 3 (80 tokens, the window slides at tokens 49 and 65; greedy, guided), plain and reversible decoder.  The cached row
    program -- eager and as a captured HIP graph, with the device sampler and with the torch tail -- must sample exactly those ids with TWO
    prefills of 33 rows and NO recomputed prefix; the recompute loop must sample them too"""
    Ar, m = _long_fixture(A, name)
    spies = _Spies(monkeypatch, A)
    ids = _generate(A, m, Ar, mode, device_sampler=device_sampler)
    assert torch.equal(ids, Ar['video_ids'].long()), (ids, Ar['video_ids'])
    if mode == 'recompute':
        assert (spies.recompute, spies.prefill) == (80, 0)
    else:
        assert (spies.recompute, spies.prefill) == (0, 2), (spies.recompute, spies.prefill)
        assert spies.prefill_rows == [33, 33]            # <bos> + two kept frames


def test_slide_cache_switch_restores_the_recompute_path(A, monkeypatch):
    """generate_slide_cache = False: past the window the whole call runs the recompute loop, every token of it, as before the rows form"""
    Ar, m = _long_fixture(A, 'g20a_generate_sketch_long')
    spies = _Spies(monkeypatch, A)
    ids = _generate(A, m, Ar, 'cached+graph', slide=False)
    assert (spies.recompute, spies.prefill) == (80, 0)
    assert torch.equal(ids, Ar['video_ids'].long())


def test_inside_the_window_nothing_changes(A, monkeypatch):
    """num_frames <= max_video_frames: no prefill, no recomputed prefix, and the ids of generate_slide_cache = False"""
    Ar, m = _long_fixture(A, 'g20a_generate_sketch_long')
    spies = _Spies(monkeypatch, A)
    a = _generate(A, m, Ar, 'cached+graph', num_frames=2)
    b = _generate(A, m, Ar, 'cached+graph', num_frames=2, slide=False)
    assert (spies.recompute, spies.prefill) == (0, 0)
    assert a.shape == (2, 32) and torch.equal(a, b)
    assert torch.equal(a, Ar['video_ids'].long()[:, :32])           # the first two frames of the long call: the same steps
