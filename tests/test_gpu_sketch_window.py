"""NUWASketch cached decoding over any sketch window on the MI355X: the single-query SparseCross2DNA kernel that reads its window in place
through a slot table (amdnuwa_cross2dna_decode, csrc/decode.hip; np.py:761-901), the row program built on it (decode._Cross2DNARows) on a
model whose window has 300 slots -- more than the packed key images of amdnuwa_xattn_decode hold --, NUWASketch.generate against the
token ids of the reference's own generate() on that model (fixtures g19a / g19b), and the A/B switch AMDNUWA_XC2_DECODE_PACKED."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from golden_util import load  # noqa: E402
from gpu_util import bf_value, record, report, to_bf_pair  # noqa: E402
from guard_util import guard, guarded  # noqa: E402
from sketch_window_util import SKETCH_FRAMES, WINDOW_KW, sketch_ids, sketch_mask, window_formula  # noqa: E402

DEV = 'cuda'
SPLIT = 128                       # slots (null key + window slots) per workgroup: kernels.ATTN_DECODE_ROWS_SPLIT
N_POS = 16
HIDDEN_POS = 3                    # the feature-map position whose every table entry is -1
POSITIONS = (1, 16, 17, 40)       # decoder rows: the first position, the last, the wrap into the next frame, the middle
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
    assert kernels.ATTN_DECODE_ROWS_SPLIT == SPLIT
    return kernels


# ---- 1-4: the kernel ---------------------------------------------------------------------------------------------------------------

def _case(K, B, J, heads, dh, x3, seed=0):
    """operands in guarded buffers: a synthetic table of random context rows, about 20 % of its entries -1, position HIDDEN_POS all -1;
    more context rows than a table row names, so that every position leaves rows unnamed"""
    g = torch.Generator().manual_seed(seed)
    inner, T = heads * dh, 2 * J + 7
    tab = torch.randint(0, T, (N_POS, J), generator=g, dtype=torch.int32)
    tab[torch.rand(N_POS, J, generator=g) < 0.2] = -1
    tab[HIDDEN_POS] = -1
    tab[0, 0] = T - 1                                           # the last context row is named (and row 0 by position 1 below)
    tab[1, J - 1] = 0
    q = to_bf_pair(torch.randn(B, inner, generator=g), x3)
    kv = to_bf_pair(torch.randn(B, T, 2 * inner, generator=g), x3)
    mask = torch.rand(B, T, generator=g) > 0.3
    if B > 1:
        mask[0] = False                                        # a sample with every context row masked: the null key alone
    gd = lambda t: None if t is None else guarded(t, device=DEV)
    return dict(q=K.BF(gd(q.hi), gd(q.lo)), kv=K.BF(gd(kv.hi), gd(kv.lo)), tab=gd(tab), mask=gd(mask), mask_u8=gd(mask.to(torch.uint8)),
                nk=gd(torch.randn(heads, dh, generator=g)), nv=gd(torch.randn(heads, dh, generator=g)),
                wth=gd(torch.randn(heads, heads, generator=g) * 0.5 + torch.eye(heads)), pos=gd(torch.ones(1, dtype=torch.int32)),
                heads=heads, dh=dh, T=T, J=J)


def _launch(K, c, use_mask=True, kv=None):
    return K.cross2dna_decode(c['q'], c['kv'] if kv is None else kv, c['tab'], c['pos'], c['heads'], c['dh'], c['nk'], c['nv'], c['wth'],
                              mask_u8=c['mask_u8'] if use_mask else None)


def _formula(c, pos, use_mask=True, kv=None):
    """fp32, on the values the kernel reads, through row (pos - 1) mod N_POS of the table"""
    return window_formula(bf_value(c['q']), bf_value(c['kv'] if kv is None else kv), c['tab'][(pos - 1) % N_POS], c['nk'], c['nv'], c['wth'],
                          c['mask'] if use_mask else None, c['dh'] ** -0.5)


@pytest.mark.parametrize('x3', [False, True])
@pytest.mark.parametrize('heads,dh', [(8, 64), (3, 64), (1, 32), (5, 32)])
@pytest.mark.parametrize('J', [1, 9, SPLIT - 2, SPLIT - 1, SPLIT, 255, 300])
def test_kernel_against_the_fp32_formula(K, J, heads, dh, x3):
    """J + 1 slots around every place the code changes path: one slot, less than one split, the three counts straddling one split (J + 1
    = 127, 128, 129), two full splits, three splits with a partial last one.  Tolerances of test_gpu_xm_long.py's kernel test (the same
    arithmetic, the same output rounding).  Outputs and the workspace are guarded buffers too (the guard on kernels)."""
    for B in (1, 3):
        c = _case(K, B, J, heads, dh, x3, seed=J + B)
        for use_mask in (False, True):
            for pos in POSITIONS + (HIDDEN_POS + 1,):
                c['pos'].fill_(pos)
                with guard(K) as gd:
                    o = _launch(K, c, use_mask)
                    assert gd.made() >= 2                      # the output and the workspace at least
                assert (o.lo is not None) == x3
                report(f'cross2dna_decode[J={J},{heads}x{dh},B={B},x3={x3},mask={use_mask},pos={pos}]', bf_value(o),
                       _formula(c, pos, use_mask), 3e-5 if x3 else 2 ** -7)


@pytest.mark.parametrize('x3', [False, True])
@pytest.mark.parametrize('J,heads,dh', [(300, 8, 64), (SPLIT - 1, 3, 64), (1, 5, 32)])
def test_kernel_reads_the_rows_its_table_names_and_no_others(K, J, heads, dh, x3):
    """every context row the selected position's table does not name holds NaN in both images: the output is finite and bit-equal to the
    launch with zeros there (a -1 slot forms no address; with every entry -1 EVERY row is NaN).  Rows a mask hides may be read: they
    stay finite."""
    c = _case(K, 2, J, heads, dh, x3, seed=3)
    for pos in POSITIONS + (HIDDEN_POS + 1,):
        row = c['tab'][(pos - 1) % N_POS]
        unnamed = torch.ones(c['T'], dtype=torch.bool, device=DEV)
        unnamed[row[row >= 0].long()] = False
        assert bool(unnamed.any())
        c['pos'].fill_(pos)

        def run(fill):
            kv = K.BF(*(None if t is None else guarded(t.clone()) for t in (c['kv'].hi, c['kv'].lo)))
            for t in (kv.hi, kv.lo):
                if t is not None:
                    t[:, unnamed] = fill
            with guard(K):
                return bf_value(_launch(K, c, kv=kv)), kv
        (o_nan, _), (o_zero, kv_zero) = run(float('nan')), run(0.)
        assert bool(torch.isfinite(o_nan).all()), pos
        assert torch.equal(o_nan, o_zero), pos
        report(f'cross2dna_decode.named_rows[J={J},x3={x3},pos={pos}]', o_zero, _formula(c, pos, kv=kv_zero), 3e-5 if x3 else 2 ** -7)


@pytest.mark.parametrize('x3', [False, True])
def test_two_launches_are_bit_identical_and_an_invalid_launch_writes_nothing(K, monkeypatch, x3):
    c = _case(K, 3, 300, 8, 64, x3, seed=5)
    c['pos'].fill_(17)
    with guard(K):
        a, b = _launch(K, c), _launch(K, c)
    assert torch.equal(a.hi, b.hi) and (not x3 or torch.equal(a.lo, b.lo))
    # pos = 0 (the <bos> row is the caller's) and a table entry >= ctx_rows in the LAST split: every workgroup of the three launches
    # agrees that nothing is written -- an output buffer of sentinels stays as it is
    full = lambda shape, dev, lo=None: K.BF(*(guarded(torch.full(shape, SENTINEL, dtype=torch.bfloat16), device=dev) if want else None
                                              for want in (True, x3)))
    monkeypatch.setattr(K, 'empty_bf', full)
    untouched = lambda o: all(t is None or bool((t.float() == SENTINEL).all()) for t in (o.hi, o.lo))
    assert not untouched(_launch(K, c))                        # (the patched buffer is the one the kernel writes)
    c['pos'].fill_(0)
    with guard(K):
        assert untouched(_launch(K, c))
    c['pos'].fill_(1 + 5)
    c['tab'][5, 299] = c['T']
    with guard(K):
        assert untouched(_launch(K, c))
    c['pos'].fill_(1 + 6)                                      # another position of the same table is served as before
    with guard(K):
        o = _launch(K, c)
    report(f'cross2dna_decode.after_invalid[x3={x3}]', bf_value(o), _formula(c, 7), 3e-5 if x3 else 2 ** -7)


def test_captured_launch_follows_the_device_side_position(K):
    """one launch captured in a HIP graph at pos = 1, replayed after the position changed IN PLACE: each replay is that position's formula"""
    c = _case(K, 2, 300, 2, 32, True, seed=7)
    c['pos'].fill_(1)
    run = lambda: _launch(K, c)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        o_g = run()
    for pos in (7, 23):
        c['pos'].fill_(pos)
        g.replay()
        o_e = run()
        torch.cuda.synchronize()
        assert torch.equal(o_g.hi, o_e.hi) and torch.equal(o_g.lo, o_e.lo)
        report(f'cross2dna_decode.graph[pos={pos}]', bf_value(o_g), _formula(c, pos), 3e-5)


# ---- 5-7: the 300-slot model ---------------------------------------------------------------------------------------------------------

def _vaes(A):
    vae = A.VQGanVAE(dim=32, image_size=16, num_layers=2, vq_codebook_size=64, vq_codebook_dim=32, use_vgg_and_gan=False)
    sketch_vae = A.VQGanVAE(dim=32, image_size=16, num_layers=2, vq_codebook_size=48, vq_codebook_dim=32, use_vgg_and_gan=False)
    return vae, sketch_vae


def _window_model(A, seed=21, **over):
    torch.manual_seed(seed)
    vae, sketch_vae = _vaes(A)
    m = A.NUWASketch(vae=vae, sketch_vae=sketch_vae, **{**WINDOW_KW, **over}).to(DEV).eval()
    ids = sketch_ids().to(DEV)
    m.sketch_vae.get_video_indices = lambda frames: ids        # an untrained sketch VAE gives every image one single id
    return m


def _context(m):
    sketch = torch.zeros(2, SKETCH_FRAMES, 3, 16, 16, device=DEV)       # only its shape is read: the tokenizer is stubbed
    return m.embed_sketch(sketch, mask=sketch_mask().to(DEV))


@pytest.mark.parametrize('cond_scale', [1., 2.5])
def test_sketch_cached_rows_match_the_recomputed_prefix_on_a_300_slot_window(A, cond_scale):
    """test_gpu_decode.py::test_sketch_cached_rows_match_the_recomputed_prefix with 12 sketch frames and a 5 x 5 window (300 slots; a
    sketch mask hides frames 7.. of sample 1): GuidedStepper builds -- it used to raise NotImplementedError -- and its logits stay within
    1e-3 of the whole recomputed prefix (`_guided_last_logits`) at every position of 1.5 frames"""
    from nuwa_pytorch_amd.decode import GuidedStepper
    m = _window_model(A)
    tpf, total = 16, 24
    ids = torch.randint(0, 64, (2, total), generator=torch.Generator().manual_seed(3)).to(DEV)
    A.set_precision('bf16x3')
    try:
        with torch.no_grad():
            ctx, cmask = _context(m)
            assert ctx.shape[1] == SKETCH_FRAMES * tpf and not bool(cmask[1, 7 * tpf:].any()) and bool(cmask[1, :7 * tpf].all())
            st = GuidedStepper(m, ctx, cmask, total, cond_scale, graph=False)
            xc2 = [b for b in st.cond.blocks if b.c2 is not None]
            assert len(xc2) == WINDOW_KW['dec_depth'] and all(b.kind == 'xc2' for b in xc2) and st.cond.bos_row_differs
            assert all(tuple(b.c2.slot_rows.shape) == (tpf, 300) and not b.c2.packed for b in xc2)
            pos_table = m.video_pos_emb()
            row = m.video_bos[None].expand(2, -1)
            worst = 0.
            for t in range(total):
                got = st(row)
                ref = m._guided_last_logits(ids[:, :t], ctx, cmask, cond_scale)
                worst = max(worst, float((got - ref).abs().max() / ref.abs().max()))
                row = m.image_embedding(ids[:, t]) + pos_table[t]
    finally:
        A.set_precision('bf16')
    record(f'sketch_window_cached_rows[cond_scale={cond_scale}].logits', worst, worst, 1e-3)
    assert worst < 1e-3, worst


class _Spy:
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


def _generate(A, m, Ar, mode):
    """mode: 'cached+graph' | 'cached' | 'recompute'"""
    cls = type(m)
    A.set_precision('bf16x3')
    try:
        cls.generate_use_cache, cls.generate_use_graph = mode != 'recompute', mode == 'cached+graph'
        torch.manual_seed(0)
        sketch = torch.zeros(Ar['sketch_ids'].shape[0], Ar['sketch_ids'].shape[1] // 16, 3, 16, 16, device=DEV)
        smask = Ar['sketch_mask'].to(DEV) if 'sketch_mask' in Ar else None
        m.generate(sketch=sketch, sketch_mask=smask, filter_thres=0.99, cond_scale=float(Ar['cond_scale']), num_frames=2)
    finally:
        cls.generate_use_cache = cls.generate_use_graph = True
        A.set_precision('bf16')
    return m.last_generated_ids.cpu()


def _fixture_model(A, name, kw):
    Ar, P, _ = load(name)
    vae, sketch_vae = _vaes(A)
    m = A.NUWASketch(vae=vae, sketch_vae=sketch_vae, **{**kw, 'dec_reversible': bool(Ar.get('reversible', False))})
    missing, unexpected = m.load_state_dict(P, strict=False)
    assert not unexpected, unexpected
    m = m.to(DEV).eval()
    ids = Ar['sketch_ids'].reshape(Ar['sketch_ids'].shape[0], -1).to(DEV)
    Ar['sketch_ids'] = ids
    m.sketch_vae.get_video_indices = lambda frames: ids
    return Ar, m


@pytest.mark.parametrize('mode', ['cached+graph', 'cached', 'recompute'])
@pytest.mark.parametrize('name', ['g19a_generate_sketch_window', 'g19b_generate_sketch_window_reversible'])
def test_window_generate_reproduces_the_reference_token_ids(A, monkeypatch, name, mode):
    """fixtures g19: the token ids the REFERENCE's own NUWASketch.generate sampled (greedy, guided, 32 tokens) on the 300-slot model, plain
    and reversible decoder; sketch token ids and sketch mask are part of the fixture.  The cached row program -- eager and as a captured
    HIP graph -- samples exactly those ids WITHOUT one recomputed prefix (it used to fall back to 32 of them); so does the recompute loop"""
    Ar, m = _fixture_model(A, name, WINDOW_KW)
    assert float(Ar['min_gap']) >= 3e-3                  # the fixture's condition on its inputs: no near tie under greedy sampling
    assert float(Ar['gaps'].min()) == float(Ar['min_gap']) and Ar['gaps'].numel() == 32
    spy = _Spy(monkeypatch, A.NUWASketch, '_guided_last_logits')
    ids = _generate(A, m, Ar, mode)
    assert torch.equal(ids, Ar['video_ids'].long()), (ids, Ar['video_ids'])
    assert spy.n['_guided_last_logits'] == (32 if mode == 'recompute' else 0)


@pytest.mark.parametrize('packed', [True, False])
def test_switch_selects_the_packed_path_for_windows_it_can_hold(A, K, monkeypatch, packed):
    """AMDNUWA_XC2_DECODE_PACKED=1: the default-window model (SKETCH_KW, 18 slots) gathers, packs and attends with amdnuwa_xattn_decode;
    without the switch it takes the side decode.XC2_DECODE_PACKED_DEFAULT names.  Both reproduce fixture g13e's ids.  The 300-slot model
    takes the in-place kernel under either setting."""
    from nuwa_pytorch_amd import decode
    from test_gpu_modules import SKETCH_KW
    if packed:
        monkeypatch.setenv('AMDNUWA_XC2_DECODE_PACKED', '1')
    else:
        monkeypatch.delenv('AMDNUWA_XC2_DECODE_PACKED', raising=False)
    assert decode.xc2_decode_packed() == (packed or decode.XC2_DECODE_PACKED_DEFAULT)
    takes_packed = decode.xc2_decode_packed()
    Ar, m = _fixture_model(A, 'g13e_generate_sketch', SKETCH_KW)
    spy = _Spy(monkeypatch, K, 'xattn_pack', 'xattn_decode', 'cross2dna_decode')
    ids = _generate(A, m, Ar, 'cached')
    assert torch.equal(ids, Ar['video_ids'].long()), (ids, Ar['video_ids'])
    rows = 3 * 31                                        # cross-2DNA layers x rows after <bos>, in the conditioned pass
    if takes_packed:
        assert spy.n['cross2dna_decode'] == 0 and spy.n['xattn_decode'] >= rows and spy.n['xattn_pack'] >= rows, spy.n
    else:
        assert spy.n['xattn_decode'] == 0 and spy.n['xattn_pack'] == 0 and spy.n['cross2dna_decode'] >= rows, spy.n
    for k in spy.n:
        spy.n[k] = 0
    Aw, mw = _fixture_model(A, 'g19a_generate_sketch_window', WINDOW_KW)
    ids = _generate(A, mw, Aw, 'cached')
    assert torch.equal(ids, Aw['video_ids'].long())
    assert spy.n['xattn_decode'] == 0 and spy.n['xattn_pack'] == 0 and spy.n['cross2dna_decode'] >= rows, spy.n
