"""No GPU needed.  Two things the GPU tests of test_gpu_weight_updates.py stand on:

1. The trained-like weights of trained_like_util.py make wiring visible.  With every LayerNorm gain at 1 and every bias at 0 -- the
   state of all whole-model fixtures -- two such vectors can trade places unnoticed.  After trained_like() each perturbed vector, put back
   to its fixture value ALONE, moves the fp32 oracle's logits by at least 5e-3 (max-abs difference over max-abs logits, the measure of
   gpu_util.report): five times the 1e-3 bound the product is held to on these weights, so a product that read the wrong vector anywhere
   cannot pass.  This is a condition on the inputs, computed from the oracle alone; no vector is exempt.

   Least visible vector per model at the (seed, bias amplitude) of trained_like_util.MODELS, measured with this test:
       g5   seed 5, 0.3   8.8e-3  video_transformer.layers.2.1.prenorm.bias
       g6   seed 5, 0.3   1.3e-2  video_transformer.layers.5.0.prenorm.bias
       g9a  seed 2, 0.3   1.2e-2  video_audio_transformer.layers.3.0.0.prenorm.bias
       g9c  seed 5, 0.3   1.1e-2  video_audio_transformer.layers.5.2.prenorm.bias
       g11a seed 5, 0.3   7.3e-3  video_transformer.layers.1.1.prenorm.bias
   g9a takes seed 2: with seed 5 the pre-norm of its audio-side cross-modality block (layers.3.1.0) drew a bias that moves the logits by
   2.2e-3 and a gain that moves them by 3.9e-3; a larger bias amplitude does not help a gain, another draw does (seeds 1 .. 10 were
   scanned on that block: 2, 3 and 10 clear 5e-3 at amplitude 0.3; 2 has the widest margin).

2. The keys of the caches that hold derivatives of the weights (ops.WeightCache, the fp16 range verdicts) see every change torch can
   see -- also a new storage at the OLD address -- and ops.weights_changed() covers the writes torch cannot see."""
import gc

import pytest
import torch

import trained_like_util as T
from gpu_util import rel_err

VISIBLE = 5e-3


# ------------------------------------------------------------------------------------------------------------------------------
# trained_like()
# ------------------------------------------------------------------------------------------------------------------------------

def test_trained_like_perturbs_the_vectors_and_nothing_else():
    _, P, _ = T.fixture('g9a_video_audio')
    a, b, c = T.trained_like(P, 5), T.trained_like(P, 5), T.trained_like(P, 6)
    assert set(a) == set(P)
    nvec = 0
    for k, v in P.items():
        assert a[k].shape == v.shape and a[k].dtype == v.dtype
        assert torch.equal(a[k], b[k]), k                       # one seeded generator: the same draw every time
        if T.is_vector(k, v):
            nvec += 1
            assert not torch.equal(a[k], c[k]), k
            if k.endswith('.weight'):
                assert float(a[k].min()) >= 0.5 and float(a[k].max()) <= 2.0 and float(a[k].max() / a[k].min()) > 1.5, k
            else:
                d = a[k] - v
                assert 0.03 < float(d.abs().max()) < 0.3 * 6, k
        else:
            assert torch.equal(a[k], v), k
    assert nvec == 115
    # gains are log-uniform: about half of them below 1
    gains = torch.cat([a[k] for k in P if k.endswith('.weight') and P[k].dim() == 1])
    assert 0.4 < float((gains < 1).float().mean()) < 0.6
    narrow = T.trained_like(P, 5, gain_span=(0.7, 1.4), bias_amp=0.)
    for k, v in P.items():
        if T.is_vector(k, v) and k.endswith('.weight'):
            assert 0.7 <= float(narrow[k].min()) and float(narrow[k].max()) <= 1.4
        elif T.is_vector(k, v):
            assert torch.equal(narrow[k], v)


@pytest.mark.parametrize('name', list(T.MODELS))
def test_every_perturbed_vector_moves_the_oracle_logits(name):
    Ar, P, Pt = T.fixture(name)
    keys = T.vector_keys(P)
    assert len(keys) >= 59
    with torch.no_grad():
        _, base = T.oracle_forward(name, Ar, Pt)
        assert len(base) == (2 if T.MODELS[name]['kind'] == 'va' else 1)
        moved = {}
        for k in keys:
            assert not torch.equal(Pt[k], P[k]), k
            Q = dict(Pt)
            Q[k] = P[k]
            _, lg = T.oracle_forward(name, Ar, Q)
            moved[k] = max(rel_err(a, b) for a, b in zip(lg, base))
    least = min(moved, key=moved.get)
    print(f'{name}: {len(keys)} vectors, least visible {least} moves the logits by {moved[least]:.2e}')
    hidden = {k: v for k, v in moved.items() if not v >= VISIBLE}
    assert not hidden, f'{name}: vectors whose fixture value the oracle logits do not tell from the perturbed one: {hidden}'


def test_state_dict_round_trip_through_a_product_model():
    """put_state / read_state: what goes into a product model comes back out, key for key, as the oracle's P"""
    import nuwa_pytorch_amd as A
    for name in ('g6_nuwa_tiny_reversible', 'g11a_sketch'):
        Ar, P, Pt = T.fixture(name)
        m = T.put_state(T.build_product(A, name, Ar), Pt)
        back = T.read_state(m)
        assert set(back) >= set(k for k in Pt if T.kept(k))
        for k, v in Pt.items():
            assert torch.equal(back[k], v), k


# ------------------------------------------------------------------------------------------------------------------------------
# cache keys
# ------------------------------------------------------------------------------------------------------------------------------

class StandIn:
    """What the caches ask of a parameter, over a tensor that can be exchanged: data_ptr() and _version keep answering what they
    answered first -- the allocator handed the old block to the new storage, whose version counter starts where the old one stood."""

    def __init__(self, t):
        self.t, self._ptr, self._version = t, t.data_ptr(), t._version
        self.is_cuda = False

    def data_ptr(self):
        return self._ptr

    def untyped_storage(self):
        return self.t.untyped_storage()


@pytest.fixture
def ops():
    from nuwa_pytorch_amd import ops
    saved = dict(ops._F16_RANGE)
    yield ops
    ops._F16_RANGE.clear()
    ops._F16_RANGE.update(saved)


def _get(ops, cache, params):
    return cache.get('k', params, lambda: [float(p.t.sum() if isinstance(p, StandIn) else p.detach().sum()) for p in params])


def test_weight_cache_sees_a_new_storage_at_the_old_address(ops):
    cache = ops.WeightCache()
    w = StandIn(torch.ones(8))
    assert _get(ops, cache, (w,)) == [8.0]
    assert _get(ops, cache, (w,)) == [8.0]
    w.t = torch.full((8,), 2.0)                          # new storage; data_ptr() and _version unchanged
    assert _get(ops, cache, (w,)) == [16.0]


def test_weight_cache_entry_holds_the_storages_it_was_built_from(ops):
    """while an entry lives, the storage it was built from lives: its address cannot be given to the storage that replaces it"""
    cache = ops.WeightCache()
    p = torch.nn.Parameter(torch.ones(1 << 16))
    _get(ops, cache, (p,))
    held = cache._store['k'][2]
    assert len(held) == 1 and held[0].data_ptr() == p.data_ptr()
    old = p.data_ptr()
    half = p.data.to(torch.float16)
    p.data = half                                        # (what module.half() does: the fp32 storage is dropped here ...
    gc.collect()
    p.data = half.float() * 0.5                          #  ... and module.float() allocates one of the same size)
    assert p.data_ptr() != old
    assert _get(ops, cache, (p,)) == [float(1 << 15)]


def test_weight_cache_sees_every_write_torch_sees_and_weights_changed_covers_the_rest(ops):
    import nuwa_pytorch_amd as A
    cache = ops.WeightCache()
    p = torch.nn.Parameter(torch.ones(8))
    assert _get(ops, cache, (p,)) == [8.0]
    with torch.no_grad():
        p.mul_(2.0)
    assert _get(ops, cache, (p,)) == [16.0]              # in place under no_grad: the version counter
    p.data = p.data * 2.0
    assert _get(ops, cache, (p,)) == [32.0]              # a new storage
    opt = torch.optim.AdamW([p], lr=1.0, weight_decay=0.)
    p.grad = torch.ones(8)
    opt.step()
    assert _get(ops, cache, (p,)) == [float(p.detach().sum())] and float(p.detach().sum()) < 32.0 - 7.9
    before = float(p.detach().sum())
    p.data.mul_(0.5)                                     # `.data` has a version counter of its own: torch hides this write
    assert _get(ops, cache, (p,)) == [before]            # (the documented blind spot ...
    A.weights_changed()
    assert _get(ops, cache, (p,)) == [before * 0.5]      #  ... and its remedy)


def test_f16_verdict_is_tied_to_the_storage_and_dropped_by_weights_changed(ops):
    w = StandIn(torch.ones(8))
    assert ops._f16_known(w) is None
    ops._f16_record(w, True)
    assert ops._f16_known(w) is True
    w.t = torch.full((8,), 1e6)                          # new storage behind the same data_ptr() / _version / object
    assert ops._f16_known(w) is None
    ops._f16_record(w, False)
    assert ops._f16_known(w) is False
    assert len([e for e in ops._F16_RANGE.values() if e[0]() is w]) == 1        # one verdict per object: the old one (and its storage) is gone

    p = torch.nn.Parameter(torch.ones(8))
    ops._f16_record(p, True)
    assert ops._f16_known(p) is True
    with torch.no_grad():
        p.mul_(2.0)
    assert ops._f16_known(p) is None
    ops._f16_record(p, True)
    p.data = p.data * 2.0
    assert ops._f16_known(p) is None
    ops._f16_record(p, True)
    p.data.mul_(2.0)
    assert ops._f16_known(p) is True                     # invisible to torch ...
    ops.weights_changed()
    assert ops._f16_known(p) is None                     # ... hence weights_changed()

    n = len(ops._F16_RANGE)
    q = torch.ones(8)
    ops._f16_record(q, True)
    assert len(ops._F16_RANGE) == n + 1
    del q
    gc.collect()
    assert len(ops._F16_RANGE) == n                      # a verdict (and the storage it holds) goes with its tensor


def test_weights_changed_is_exported_and_moves_the_epoch(ops):
    import nuwa_pytorch_amd as A
    assert 'weights_changed' in A.__all__ and A.weights_changed is ops.weights_changed
    e = ops.WeightCache.EPOCH
    A.weights_changed()
    assert ops.WeightCache.EPOCH == e + 1
