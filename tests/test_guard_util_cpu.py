"""Self-test of tests/guard_util.py on CPU tensors (no GPU needed): the harness the guarded GPU tests stand on must itself notice a byte
written outside a tensor, hand out NaN-prefilled interiors of the requested form and leave the guarded module as it found it."""
import types

import pytest
import torch

import guard_util as G
from guard_util import FILL, guard, guarded, guarded_empty


def _module():
    """a stand-in for kernels.py: a module whose functions allocate through its global `torch`"""
    m = types.ModuleType('fake_kernels')
    m.torch = torch
    exec('def alloc(shape, dtype, kind="empty", **kw):\n'
         '    if kind == "full":\n'
         '        return torch.full(shape, 3, dtype=dtype, **kw)\n'
         '    return getattr(torch, kind)(shape, dtype=dtype, **kw)\n'
         'def like(t, kind):\n'
         '    return getattr(torch, kind)(t)\n'
         'def unrelated():\n'
         '    return torch.float32, torch.autograd.Function, torch.arange(3)\n', m.__dict__)
    return m


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16, torch.bfloat16, torch.int64, torch.uint8])
@pytest.mark.parametrize('shape', [(7, 33), (5,), (2, 3, 130), (300, 700)])
def test_interior_has_the_requested_form_and_reads_as_fill(shape, dtype):
    m = _module()
    with guard(m, cpu=True):
        t = m.alloc(shape, dtype)
        ref = torch.empty(shape, dtype=dtype)
        assert t.shape == ref.shape and t.dtype == dtype and t.stride() == ref.stride() and t.is_contiguous()
        e = G._REGISTRY[-1]
        nbytes = ref.numel() * ref.element_size()
        assert e['nbytes'] == nbytes and e['buf'].numel() == 2 * e['band'] + nbytes
        assert e['band'] % 4096 == 0 and 64 << 10 <= e['band'] <= 8 << 20 and e['band'] >= min(nbytes, 8 << 20)
        assert (t.data_ptr() - e['buf'].data_ptr()) == e['band']          # interior = allocation start + a multiple of 4 KiB
        assert 'alloc' in e['label']
        if dtype.is_floating_point:
            assert bool(torch.isnan(t).all())
        elif dtype == torch.uint8:
            assert bool((t == 255).all())
        else:
            assert bool((t == -1).all())
        z = m.alloc(shape, dtype, kind='zeros')
        assert z.shape == ref.shape and bool((z == 0).all())
        f = m.alloc(shape, dtype, kind='full')
        assert f.dtype == dtype and bool((f == 3).all())
        for kind in ('empty_like', 'zeros_like'):
            l = m.like(ref, kind)
            assert l.shape == ref.shape and l.dtype == dtype and l.stride() == ref.stride()
            assert bool((l == 0).all()) if kind == 'zeros_like' else bool((l.view(torch.uint8) == FILL).all())
        assert len(G._REGISTRY) == 5
    assert G._REGISTRY == []


def test_band_size_limits():
    assert G.band_bytes(0) == 64 << 10 and G.band_bytes(1) == 64 << 10
    assert G.band_bytes((64 << 10) + 1) == (64 << 10) + 4096
    assert G.band_bytes(1 << 30) == 8 << 20


def test_untouched_run_passes_and_cpu_is_left_alone_unless_asked():
    m = _module()
    with guard(m, cpu=True):
        t = m.alloc((4, 4), torch.float32)
        t.fill_(1.0)                                    # the whole interior, nothing else
    with guard(m):                                      # as the GPU tests use it: CPU allocations are plain torch ones
        t = m.alloc((4, 4), torch.float32)
        assert t._base is None and G._REGISTRY == []


@pytest.mark.parametrize('side', ['front', 'back'])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16])
def test_a_write_one_element_outside_fails_naming_side_and_offset(side, dtype):
    m = _module()
    with pytest.raises(AssertionError) as ei:
        with guard(m, cpu=True):
            t = m.alloc((3, 5), dtype)
            e = G._REGISTRY[-1]
            flat = e['buf'].view(dtype)
            first = e['band'] // t.element_size()
            if side == 'front':
                flat[first - 1] = 1.0                   # the element just before the tensor
            else:
                flat[first + t.numel()] = 1.0           # the element just behind it
            band, esz = e['band'], t.element_size()
    msg = str(ei.value)
    assert 'alloc' in msg and f'{side} band' in msg and ('back band' if side == 'front' else 'front band') not in msg
    lo = band - esz if side == 'front' else 0
    # 1.0 has zero low bytes in both formats: at least its top byte differs from 0xFF, all inside the one element
    assert 'first at offset ' in msg and 'last at offset ' in msg
    first_off = int(msg.split('first at offset ')[1].split(',')[0])
    last_off = int(msg.split('last at offset ')[1].split()[0])
    n = int(msg.split('damaged: ')[1].split(' bytes')[0])
    assert lo <= first_off <= last_off < lo + esz and 1 <= n <= esz
    assert G._REGISTRY == []


def test_both_sides_are_listed_in_one_error():
    m = _module()
    with pytest.raises(AssertionError) as ei:
        with guard(m, cpu=True):
            m.alloc((8,), torch.uint8)
            m.alloc((8,), torch.uint8)
            G._REGISTRY[0]['buf'][G._REGISTRY[0]['band'] - 1] = 0
            G._REGISTRY[1]['buf'][G._REGISTRY[1]['band'] + 8] = 0
    assert '2 guard region(s)' in str(ei.value) and 'front band' in str(ei.value) and 'back band' in str(ei.value)


def test_proxy_forwards_everything_else():
    m = _module()
    with guard(m, cpu=True):
        f32, fn, ar = m.unrelated()
        assert f32 is torch.float32 and fn is torch.autograd.Function and torch.equal(ar, torch.arange(3))
        assert m.torch is not torch and m.torch.nn is torch.nn and isinstance(ar, m.torch.Tensor)


def test_module_torch_is_restored_after_an_exception():
    m = _module()
    with pytest.raises(ValueError):
        with guard(m, cpu=True):
            assert m.torch is not torch
            raise ValueError('inside')
    assert m.torch is torch and G._REGISTRY == []
    with pytest.raises(AssertionError, match='inside'):
        with guard(m, cpu=True):
            assert False, 'inside'
    assert m.torch is torch


def test_a_failing_block_with_damaged_bands_reports_both():
    m = _module()
    with pytest.raises(AssertionError) as ei:
        with guard(m, cpu=True):
            m.alloc((8,), torch.uint8)
            G._REGISTRY[0]['buf'][G._REGISTRY[0]['band'] + 8] = 0
            assert False, 'values differ'
    assert 'back band' in str(ei.value) and 'values differ' in str(ei.value)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.int64, torch.uint8])
def test_guarded_operand_round_trips_inside_fill(dtype):
    torch.manual_seed(0)
    src = (torch.randn(5, 13) * 10).to(dtype)
    m = _module()
    with guard(m, cpu=True):
        v = guarded(src, ld=24, rows_after=3)
        assert v.shape == src.shape and v.stride() == (24, 1) and torch.equal(v, src)
        e = G._REGISTRY[-1]
        esz = src.element_size()
        assert e['nbytes'] == 8 * 24 * esz and v.data_ptr() - e['buf'].data_ptr() == e['band']
        raw = e['buf'].clone()
        grid = raw[e['band']:e['band'] + e['nbytes']].view(8, 24 * esz)
        assert bool((raw[:e['band']] == FILL).all()) and bool((raw[e['band'] + e['nbytes']:] == FILL).all())
        assert bool((grid[:5, 13 * esz:] == FILL).all()) and bool((grid[5:] == FILL).all())
        assert torch.equal(grid[:5, :13 * esz].contiguous().view(dtype), src)
        c = guarded(src)                                 # plain contiguous copy
        assert c.is_contiguous() and torch.equal(c, src)
        d3 = guarded(torch.arange(24.).reshape(2, 3, 4))
        assert d3.shape == (2, 3, 4) and torch.equal(d3, torch.arange(24.).reshape(2, 3, 4))


@pytest.mark.parametrize('where', ['row pitch', 'rows behind'])
def test_a_write_into_the_pitch_or_the_rows_behind_fails(where):
    m = _module()
    with pytest.raises(AssertionError, match=where):
        with guard(m, cpu=True):
            v = guarded(torch.zeros(4, 6), ld=8, rows_after=2)
            full = torch.as_strided(v, (6, 8), (8, 1))
            if where == 'row pitch':
                full[3, 6] = 0.0
            else:
                full[4, 0] = 0.0


def test_guarded_empty_called_directly():
    """the function the proxy stands on: FILL interior (zero=True: a zero interior), both bands FILL, the caller named in the label"""
    G._REGISTRY.clear()
    a = guarded_empty((3, 4), torch.float16, 'cpu')
    z = guarded_empty(5, torch.int64, 'cpu', zero=True)
    assert bool(torch.isnan(a).all()) and bool((z == 0).all()) and z.shape == (5,)
    for e in G._REGISTRY:
        assert 'test_guarded_empty_called_directly' in e['label']
        assert bool((e['buf'][:e['band']] == FILL).all()) and bool((e['buf'][e['band'] + e['nbytes']:] == FILL).all())
    assert G.check_registry() == [] and G._REGISTRY == []


def test_operands_made_before_the_block_are_checked_and_made_counts_the_block():
    m = _module()
    G._REGISTRY.clear()
    v = guarded(torch.zeros(4, 6), ld=8)
    with pytest.raises(AssertionError, match='row pitch'):
        with guard(m, cpu=True) as gd:
            assert gd.made() == 0
            m.alloc((2, 2), torch.float32)
            assert gd.made() == 1
            torch.as_strided(v, (4, 8), (8, 1))[0, 7] = 0.0
    assert gd.made() == 1 and G._REGISTRY == []
