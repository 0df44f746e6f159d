"""Cached generate() past max_video_frames without a GPU: the per-step window plan (slide_plan) agrees with the reference's look-back
window (lookback_window, np.py:1876-1881) at every length, and the two cache-prefill entry points (amdnuwa_prefill_ln,
amdnuwa_prefill_kv, csrc/decode.hip) are exported, declared and registered and check their arguments before anything is launched."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ARG, UNSUPPORTED = 0, -1, -2
PTR = ctypes.c_void_p(16)                  # never dereferenced on the host


@pytest.fixture(scope='module')
def L():
    from nuwa_pytorch_amd import _lib
    return _lib.lib()


@pytest.mark.parametrize('tpf', [1, 4, 16])
@pytest.mark.parametrize('max_frames', [1, 2, 3])
def test_slide_plan_agrees_with_lookback_window(tpf, max_frames):
    """keep is the window's length at every n; slid is exactly 'the window starts later than at n - 1'; in between the window grows by one
    token at its end (the cached rows stay valid); and the rows a step feeds (keep + 1 with <bos>) never exceed window + 1"""
    from nuwa_pytorch_amd.nuwa_pytorch import lookback_window, slide_plan
    window = tpf * max_frames
    ids = torch.arange(6 * tpf)[None]
    start_prev = 0
    for n in range(6 * tpf + 1):
        win = lookback_window(ids[:, :n], tpf, max_frames)
        keep, slid = slide_plan(n, tpf, max_frames)
        assert keep == win.shape[1], (n, keep, win.shape)
        start = n - keep
        assert slid == (start != start_prev), (n, start, start_prev, slid)
        assert keep + 1 <= window + 1
        if n <= window:
            assert (keep, slid) == (n, False)
        else:
            assert slid == (n % tpf == 1 or tpf == 1)
            assert start % tpf == 0                       # whole frames leave
            assert keep >= 1                              # the newest token is always inside: the prefill has R = keep >= 1 rows
        if keep:
            assert torch.equal(win, ids[:, start:n])
        start_prev = start


def test_entry_points_are_exported_declared_and_registered(L):
    from nuwa_pytorch_amd import _lib
    from nuwa_pytorch_amd import kernels as K
    header = open(os.path.join(ROOT, 'include', 'amdnuwa.h')).read()
    for name in ('amdnuwa_prefill_ln', 'amdnuwa_prefill_kv'):
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES
        assert re.search(r'\b' + name + r'\s*\(', header), name
    assert callable(K.prefill_ln) and callable(K.prefill_kv)
    assert L.amdnuwa_abi_version() == 21                      # purely additive


def _ln(L, **over):
    a = dict(y=PTR, y_is_bf16=0, resid=PTR, w=PTR, b=PTR, next_w=PTR, next_b=PTR, x_new=PTR, cache_hi=PTR, cache_lo=PTR, out_hi=PTR,
             out_lo=PTR, B=2, R=17, cache_rows=33, D=64, fmap=4, eps=1e-5, stream=None)
    a.update(over)
    return L.amdnuwa_prefill_ln(*a.values())


def _kv(L, **over):
    a = dict(qkv=PTR, qkv_lo=PTR, kv_cache=PTR, kv_cache_lo=PTR, B=2, R=17, cache_rows=33, inner=64, stream=None)
    a.update(over)
    return L.amdnuwa_prefill_kv(*a.values())


def test_prefill_ln_checks_arguments_before_any_launch(L):
    assert _ln(L, y=None) == ARG
    assert _ln(L, w=None) == ARG and _ln(L, b=None) == ARG and _ln(L, x_new=None) == ARG         # a residual needs the post-norm
    assert _ln(L, next_b=None) == ARG and _ln(L, out_hi=None) == ARG                              # a next norm needs its bias and out
    assert _ln(L, resid=None, next_w=None) == ARG                                                 # nothing to do
    assert _ln(L, resid=None, y_is_bf16=1) == ARG
    assert _ln(L, next_w=None) == ARG                                                             # a cache without the norm that fills it
    assert _ln(L, cache_lo=None) == ARG and _ln(L, out_lo=None) == ARG                            # lo on both sides or on neither
    for name in ('B', 'R', 'D', 'cache_rows'):
        assert _ln(L, **{name: 0}) == ARG and _ln(L, **{name: -3}) == ARG, name
    assert _ln(L, fmap=0) == ARG and _ln(L, fmap=-2) == ARG
    assert _ln(L, R=34) == ARG                                                                    # R > cache_rows
    assert _ln(L, D=24) == UNSUPPORTED and _ln(L, D=4112) == UNSUPPORTED
    assert _ln(L, D=24, R=34) == ARG                                                              # arguments first, the envelope second


def test_prefill_kv_checks_arguments_before_any_launch(L):
    assert _kv(L, qkv=None) == ARG and _kv(L, kv_cache=None) == ARG
    assert _kv(L, qkv_lo=None) == ARG and _kv(L, kv_cache_lo=None) == ARG                         # lo on both sides or on neither
    for name in ('B', 'R', 'cache_rows', 'inner'):
        assert _kv(L, **{name: 0}) == ARG and _kv(L, **{name: -1}) == ARG, name
    assert _kv(L, R=34) == ARG                                                                    # R > cache_rows
    assert _kv(L, inner=60) == UNSUPPORTED                                                        # 16-byte vectors


def test_prefill_refuses_blocks_without_a_full_sequence_form():
    """kinds 'xm' and 'xc2' (NUWAVideoAudio, NUWASketch) keep the recompute loop past their window: prefill raises before any launch"""
    from nuwa_pytorch_amd import decode
    d = decode.IncrementalDecoder.__new__(decode.IncrementalDecoder)
    d.B, d.rows, d.halves = 2, 8, 1
    for kind in ('xm', 'xc2'):
        blk = decode._Block()
        blk.kind, blk.store_before, blk.store_after = kind, (), ()
        d.blocks = [blk]
        with pytest.raises(NotImplementedError):
            d.prefill(torch.zeros(2, 3, 32))
    with pytest.raises(ValueError):
        d.prefill(torch.zeros(2, 9, 32))                      # more rows than the caches hold


class _StubStepper:
    """what the token loop drives of decode.GuidedStepper, recording every call into model.log; `t` = steps taken so far"""

    def __init__(self, model, context, context_mask, max_rows, cond_scale, graph=True, sampler=None):
        self.log, self.t = model.log, 0
        self.log['built'].append(max_rows)
        self.device_sampler = sampler is not None
        self.batch = context.shape[0]
        if sampler is not None:
            self.ids = torch.zeros((self.batch, sampler['total']), dtype=torch.long)

    def prefill(self, rows):
        self.log['prefill'].append((self.t, rows.clone()))

    def __call__(self, row):
        self.log['rows'].append(row.clone())
        self.t += 1
        return torch.zeros(self.batch, 8)

    def advance(self, x_row=None):
        assert (x_row is not None) == (self.t == 0)               # the <bos> row once; afterwards the step leaves the next row in place
        self.t += 1


def _loop_model(fmap, max_frames, slide_cache, device_sampler):
    """the attributes NUWA._sample_video reads, on a stand-in: <bos> = -1, token embedding 0, position row i = i + 1 in every channel"""
    import types
    m = types.SimpleNamespace(video_fmap_size=fmap, max_video_frames=max_frames, generate_use_cache=True, generate_use_graph=True,
                              generate_slide_cache=slide_cache, generate_device_sampler=device_sampler,
                              log=dict(built=[], prefill=[], rows=[], recompute=[]))
    window = fmap * fmap * max_frames
    m.video_bos = torch.full((4,), -1.)
    m.image_embedding = lambda ids: torch.zeros(*ids.shape, 4)
    m.video_pos_emb = lambda: (torch.arange(window, dtype=torch.float32) + 1)[:, None].expand(window, 4)
    m._ids_to_frames = lambda ids, chunks: ids

    def recompute(ids, context, context_mask, cond_scale):
        m.log['recompute'].append(ids.shape[1])
        return torch.zeros(ids.shape[0], 8)
    m._guided_last_logits = recompute
    return m


@pytest.mark.parametrize('fmap', [1, 2])
@pytest.mark.parametrize('max_frames', [1, 2, 3])
def test_token_loop_prefills_at_slides_and_follows_the_position_schedule(monkeypatch, fmap, max_frames):
    """NUWA._sample_video (the loop NUWA.generate and NUWASketch.generate share) on a stub stepper, total = 1 .. three frames past the
    window, both cached tails: prefill exactly at the steps slide_plan marks, with `keep` rows (<bos>, then the window's position rows from 0);
    the torch tail feeds step t + 1 the position row position_schedule(...)[t]; the caches hold total or window + 1 rows; with the slide
    switch off (NUWASketch's setting) a call past the window never builds a stepper and recomputes the look-back window at every step"""
    import types
    from nuwa_pytorch_amd import decode
    from nuwa_pytorch_amd.nuwa_pytorch import NUWA, slide_plan
    monkeypatch.setattr(decode, 'GuidedStepper', _StubStepper)
    tpf = fmap * fmap
    window = tpf * max_frames
    ctx = types.SimpleNamespace(shape=(2, 3, 4), is_cuda=True, device='cpu')
    for total in range(1, window + 3 * tpf + 1):
        slides = [t for t in range(total) if slide_plan(t, tpf, max_frames)[1]]
        schedule = decode.position_schedule(tpf, max_frames, total)
        for device_sampler in (False, True):
            m = _loop_model(fmap, max_frames, True, device_sampler)
            ids = NUWA._sample_video(m, ctx, None, total, 0.9, 1., 2., 10)
            assert ids is m.last_generated_ids and tuple(ids.shape) == (2, total)
            assert m.log['built'] == [total if total <= window else window + 1] and not m.log['recompute']
            assert [t for t, _ in m.log['prefill']] == slides, (total, device_sampler)
            for t, rows in m.log['prefill']:
                keep = slide_plan(t, tpf, max_frames)[0]
                assert tuple(rows.shape) == (2, keep, 4)
                assert torch.equal(rows[0, :, 0], torch.cat((torch.tensor([-1.]), torch.arange(keep - 1) + 1.)))
            if not device_sampler:
                fed = torch.stack(m.log['rows'])[:, 0, 0]
                assert fed[0] == -1 and torch.equal(fed[1:], schedule[:total - 1] + 1.)
        m = _loop_model(fmap, max_frames, False, True)
        NUWA._sample_video(m, ctx, None, total, 0.9, 1., 2., 10)
        assert tuple(m.last_generated_ids.shape) == (2, total)
        if total > window:
            assert not m.log['built'] and m.log['recompute'] == [slide_plan(t, tpf, max_frames)[0] for t in range(total)]
        else:
            assert m.log['built'] == [total] and not m.log['recompute']
