"""Guard bands and NaN prefill for the buffers the kernels write and read (plain helper, like gpu_util.py).

Every guarded tensor is the interior view of ONE flat uint8 buffer `band | payload | band` that is filled with FILL = 0xFF before
use: a byte pattern that reads as NaN in fp32 / fp16 / bf16, -1 in the signed integers and 255 in uint8.  So
  * an output element a kernel never writes stays NaN and fails the value comparison of the test that owns it,
  * an operand byte outside the logical tensor (pitch padding, rows behind the last, both bands) is NaN: a loader that lets it reach
    the arithmetic -- even multiplied by zero -- gives NaN,
  * a store outside the payload lands in a band (physically inside the test's own buffer) and is found byte for byte on exit.
Limit: a write further than one band from its buffer is not seen.  The band is the payload size rounded up to 4 KiB (64 KiB at
least, 8 MiB at most), so at the test shapes every write within one tensor size of the buffer is."""
import math
import sys

import torch as _torch

FILL = 0xFF
PAGE = 4096                        # a multiple of the caching allocator's 512-byte (and the CPU allocator's 64-byte) alignment
BAND_MIN, BAND_MAX = 64 << 10, 8 << 20

_REGISTRY = []                     # dicts: buf, band, nbytes, label, pitch (None or (rows, cols, ld, total rows, element size))


def band_bytes(nbytes):
    return min(max((nbytes + PAGE - 1) // PAGE * PAGE, BAND_MIN), BAND_MAX)


def _caller():
    """name of the nearest calling function outside this file"""
    f = sys._getframe(1)
    while f is not None and f.f_code.co_filename == __file__:
        f = f.f_back
    return f.f_code.co_name if f is not None else '?'


def _shape(shape):
    if isinstance(shape, (int, _torch.SymInt)):
        return (int(shape),)
    return tuple(int(s) for s in shape)


def _raw(nbytes, device, label, pitch=None):
    band = band_bytes(nbytes)
    buf = _torch.full((band + nbytes + band,), FILL, dtype=_torch.uint8, device=device)
    _REGISTRY.append(dict(buf=buf, band=band, nbytes=nbytes, label=label, pitch=pitch))
    return buf, band


def guarded_empty(shape, dtype, device, zero=False, label=None):
    """what torch.empty(shape, dtype=dtype, device=device) returns, inside a FILL-ed buffer with a band on either side"""
    shape = _shape(shape)
    esz = _torch.empty((), dtype=dtype).element_size()
    nbytes = math.prod(shape) * esz
    buf, band = _raw(nbytes, device, f'{label or _caller()}: {str(dtype).replace("torch.", "")}{list(shape)}')
    inner = buf[band:band + nbytes]
    if zero:
        inner.zero_()
    return inner.view(dtype).view(shape)


def guarded(t, ld=None, rows_after=0, device=None, label=None):
    """device copy of `t` inside a guarded buffer.  2-D tensors: ld (elements) > columns adds a FILL pitch behind every row, rows_after
    FILL rows behind the last one; the returned view has stride (ld, 1), the form kernels._ld() accepts.  The pitch and the rows
    behind are checked on exit like the bands (nothing may write them)."""
    device = t.device if device is None else device
    t = t.detach()
    esz = t.element_size()
    if ld is None and rows_after == 0:
        out = guarded_empty(t.shape, t.dtype, device, label=label or _caller())
        out.copy_(t)
        return out
    assert t.dim() == 2, 'ld / rows_after describe a 2-D operand'
    rows, cols = t.shape
    ld = cols if ld is None else int(ld)
    assert ld >= cols
    total = rows + int(rows_after)
    nbytes = total * ld * esz
    buf, band = _raw(nbytes, device, f'{label or _caller()}: {str(t.dtype).replace("torch.", "")}[{rows}+{rows_after}, {cols} of {ld}]',
                     pitch=(rows, cols, ld, total, esz))
    inner = buf[band:band + nbytes].view(t.dtype).view(total, ld)
    out = inner[:rows, :cols]
    out.copy_(t)
    return out


def _damage(region):
    """(count, first, last) of the bytes of a flat uint8 region that are no longer FILL"""
    idx = (region != FILL).nonzero()
    return int(idx.numel()), (int(idx[0]) if idx.numel() else -1), (int(idx[-1]) if idx.numel() else -1)


def _regions(e):
    buf, band, nb = e['buf'], e['band'], e['nbytes']
    yield 'front band', buf[:band]
    yield 'back band', buf[band + nb:]
    if e['pitch'] is not None:
        rows, cols, ld, total, esz = e['pitch']
        grid = buf[band:band + nb].view(total, ld * esz)
        if ld > cols:
            yield 'row pitch', grid[:rows, cols * esz:]
        if total > rows:
            yield 'rows behind', grid[rows:]


def check_registry(clear=True):
    """-> list of damage lines (empty: every band, pitch and trailing row still holds FILL).  Offsets count bytes from the start of the
    damaged region (front band: offset band - 1 is the byte just before the tensor; back band: offset 0 the byte just behind it)."""
    entries = list(_REGISTRY)
    if clear:
        _REGISTRY.clear()
    if not entries:
        return []
    # one device round trip for the common (clean) case: the damaged-byte counts of all regions of one device together
    flags, where = {}, []
    for e in entries:
        for side, region in _regions(e):
            flags.setdefault(region.device, []).append((region != FILL).sum())
            where.append((e, side, region))
    counts = {}
    for dev, fl in flags.items():
        counts[dev] = iter(_torch.stack(fl).cpu().tolist())
    bad = []
    for e, side, region in where:
        if next(counts[region.device]):
            n, first, last = _damage(region.reshape(-1) if region.is_contiguous() else region.contiguous().view(-1))
            bad.append(f'{e["label"]}: {side} ({region.numel()} bytes) damaged: {n} bytes, first at offset {first}, last at offset {last}')
    return bad


class _TorchProxy:
    """stands in for a module's global `torch`: every attribute is the real one, except that the five allocating constructors return
    guarded tensors (CUDA allocations; CPU ones only when the guard asks for them, for the self-test; nothing during a graph capture,
    where the fill would become part of the graph)"""

    def __init__(self, cpu=False):
        object.__setattr__(self, '_cpu', cpu)

    def __getattr__(self, name):
        return getattr(_torch, name)

    def __setattr__(self, name, value):
        setattr(_torch, name, value)

    def _wanted(self, device, kw):
        if any(k in kw for k in ('out', 'layout', 'pin_memory', 'memory_format', 'names')):
            return False
        if device.type == 'cuda':
            return not _torch.cuda.is_current_stream_capturing()
        return device.type == 'cpu' and self._cpu

    @staticmethod
    def _device(kw):
        d = kw.get('device')
        if d is None:
            return _torch.get_default_device() if hasattr(_torch, 'get_default_device') else _torch.device('cpu')
        return _torch.device(d) if not isinstance(d, int) else _torch.device('cuda', d)

    @staticmethod
    def _size(args):
        return _shape(args[0]) if len(args) == 1 else _shape(args)

    def _finish(self, t, kw):
        return t.requires_grad_() if kw.get('requires_grad') else t

    def empty(self, *size, **kw):
        dev = self._device(kw)
        if 'size' in kw or not self._wanted(dev, kw):
            return _torch.empty(*size, **kw)
        return self._finish(guarded_empty(self._size(size), kw.get('dtype') or _torch.get_default_dtype(), dev), kw)

    def zeros(self, *size, **kw):
        dev = self._device(kw)
        if 'size' in kw or not self._wanted(dev, kw):
            return _torch.zeros(*size, **kw)
        return self._finish(guarded_empty(self._size(size), kw.get('dtype') or _torch.get_default_dtype(), dev, zero=True), kw)

    def full(self, size, fill_value, *more, **kw):
        dev = self._device(kw)
        if more or not self._wanted(dev, kw):          # (positional dtype / layout / ...: rare forms, left to torch)
            return _torch.full(size, fill_value, *more, **kw)
        dtype = kw.get('dtype') or _torch.full((), fill_value).dtype
        out = guarded_empty(size, dtype, dev)
        out.fill_(fill_value)
        return self._finish(out, kw)

    def _like(self, t, kw, zero):
        real = _torch.zeros_like if zero else _torch.empty_like
        dev = _torch.device(kw['device']) if kw.get('device') is not None else t.device
        fmt = {k: v for k, v in kw.items() if k != 'memory_format'}      # contiguous source: every dense format gives the same tensor
        if kw.get('memory_format', _torch.preserve_format) not in (_torch.preserve_format, _torch.contiguous_format) or \
                not self._wanted(dev, fmt) or not t.is_contiguous() or t.layout != _torch.strided:
            return real(t, **kw)              # a strided source keeps its strides: left to torch
        return self._finish(guarded_empty(t.shape, kw.get('dtype') or t.dtype, dev, zero=zero), kw)

    def empty_like(self, t, **kw):
        return self._like(t, kw, False)

    def zeros_like(self, t, **kw):
        return self._like(t, kw, True)


class guard:
    """with guard(kernels, ops, ...): every torch.empty / zeros / empty_like / zeros_like / full those modules make on the GPU is a guarded
    buffer; on exit: synchronise, check every band (and the pitch of every guarded() operand in the registry, made inside the block or
    before it) byte for byte, raise ONE AssertionError that lists each damaged region, clear the registry.  made() = the number of
    guarded buffers created since entry: a test asserts it is not zero, so that a block whose allocations all slipped past the proxy
    cannot pass as clean.  Guards may nest: the inner exit checks (and releases) the outer one's buffers as well, early but not less.
    The modules' `torch` is restored whatever happens inside."""

    def __init__(self, *modules, cpu=False):
        self.modules = modules
        self.proxy = _TorchProxy(cpu=cpu)

    def __enter__(self):
        self.made_total = 0
        self._mark = len(_REGISTRY)           # entries made before the block (guarded() operands) stay and are checked on exit
        self.saved = [(m, m.__dict__['torch']) for m in self.modules]
        for m, _ in self.saved:
            m.torch = self.proxy
        return self

    def made(self):
        return self.made_total + max(len(_REGISTRY) - self._mark, 0)

    def __exit__(self, et, ev, tb):
        for m, real in self.saved:
            m.torch = real
        self.made_total, self._mark = self.made(), 0
        if et is not None and not issubclass(et, AssertionError):
            # any other exception leaves the bands unchecked: after a HIP error the device may be unusable and touching it again
            # could hang, and the price is that an ordinary Python error (a wrapper's shape check, say) hides band damage done before
            # it -- the test fails either way, with the original exception
            _REGISTRY.clear()
            return False
        if _torch.cuda.is_available():
            _torch.cuda.synchronize()
        bad = check_registry()
        if bad:
            msg = f'{len(bad)} guard region(s) written outside their tensor:\n  ' + '\n  '.join(bad)
            if ev is not None:
                msg += f'\n(the block also failed with: {ev})'
            raise AssertionError(msg)
        return False
