"""The sampling tail of a generate() token on the device (amdnuwa_sample_next_row, csrc/sample.hip; decode.GuidedStepper's sampler)
without a GPU: the entry point is exported, declared and registered and the ABI version is unchanged, its argument and envelope checks
answer before anything is launched, and the device schedule of position rows equals slide_plan step by step."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ARG, UNSUPPORTED = 0, -1, -2


@pytest.fixture(scope='module')
def L():
    from nuwa_pytorch_amd import _lib
    return _lib.lib()


def _call(L, ptr=ctypes.c_void_p(16), **over):
    """argument list of amdnuwa_sample_next_row with every pointer `ptr` (never dereferenced on the host); over: name -> value"""
    a = dict(B=2, C=64, keep=6, temperature=1., logits=ptr, ld=64, u=ptr, emb=ptr, D=32, pos=ptr, P=48, pos_idx=ptr, cap=32, step=ptr,
             ids=ptr, x_next=ptr, stream=None)
    assert not set(over) - set(a), over
    a.update(over)
    return L.amdnuwa_sample_next_row(*a.values())


def test_entry_point_is_exported_declared_and_registered(L):
    from nuwa_pytorch_amd import _lib
    from nuwa_pytorch_amd import kernels as K
    header = open(os.path.join(ROOT, 'include', 'amdnuwa.h')).read()
    name = 'amdnuwa_sample_next_row'
    assert hasattr(L, name)
    assert name in _lib.SIGNATURES
    assert re.search(r'\b' + name + r'\s*\(', header)
    assert callable(K.sample_next_row)
    assert L.amdnuwa_abi_version() == 21 and _lib.ABI_VERSION == 21          # purely additive
    assert 'sample.hip' in __import__('nuwa_pytorch_amd.build', fromlist=['SOURCES']).SOURCES


def test_argument_checks_answer_before_any_launch(L):
    assert _call(L, ptr=None) == ARG
    for name in ('logits', 'emb', 'pos', 'pos_idx', 'step', 'ids', 'x_next'):
        assert _call(L, **{name: None}) == ARG, name
    for name in ('B', 'C', 'D', 'P', 'cap'):
        for v in (0, -3):
            assert _call(L, **{name: v}) == ARG, (name, v)
    assert _call(L, keep=0) == ARG and _call(L, keep=-1) == ARG and _call(L, keep=65) == ARG
    assert _call(L, ld=63) == ARG
    # the uniforms: NULL exactly when one logit is kept
    assert _call(L, u=None) == ARG and _call(L, keep=1) == ARG
    for t in (0., -1., float('nan'), float('inf')):
        assert _call(L, temperature=t) == ARG, t


def test_envelope_checks_come_second_and_answer_unsupported(L):
    assert _call(L, C=16385, ld=16385, keep=100) == UNSUPPORTED
    for D in (30, 33, 2):
        assert _call(L, D=D) == UNSUPPORTED, D
    odd = ctypes.c_void_p(20)                                   # the row pointers travel as 16-byte vectors
    for name in ('emb', 'pos', 'x_next'):
        assert _call(L, **{name: odd}) == UNSUPPORTED, name
    # arguments first, the envelope second
    assert _call(L, C=16385, ld=16385, keep=100, step=None) == ARG
    assert _call(L, D=30, keep=65) == ARG
    assert _call(L, C=20000, ld=100) == ARG


@pytest.mark.parametrize('tpf,frames,total', [(16, 3, 80), (1, 1, 3), (16, 3, 32)])
def test_position_schedule_equals_slide_plan(tpf, frames, total):
    """entry t of the device schedule is the position-embedding row generate() gives the token step t samples: slide_plan(t + 1)[0] - 1,
    always a row of the (frames * tpf)-row table; inside the window it is t itself"""
    from nuwa_pytorch_amd.decode import position_schedule
    from nuwa_pytorch_amd.nuwa_pytorch import slide_plan
    sched = position_schedule(tpf, frames, total)
    assert sched.dtype == torch.int32 and tuple(sched.shape) == (total,)
    assert sched.tolist() == [slide_plan(t + 1, tpf, frames)[0] - 1 for t in range(total)]
    assert int(sched.min()) >= 0 and int(sched.max()) < tpf * frames
    inside = min(total, tpf * frames)
    assert sched[:inside].tolist() == list(range(inside))


def test_kept_logits_is_sample_top_fraction_s_count():
    from nuwa_pytorch_amd.decode import kept_logits
    assert kept_logits(0.9, 64) == 6 and kept_logits(0.99, 64) == 1 and kept_logits(0.9, 8192) == 819 and kept_logits(0., 64) == 64


def test_both_models_carry_the_switch():
    import nuwa_pytorch_amd as A
    assert isinstance(A.NUWA.generate_device_sampler, bool) and isinstance(A.NUWASketch.generate_device_sampler, bool)
