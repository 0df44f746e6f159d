"""Where the kernels touch memory (tests/guard_util.py): every buffer kernels.py hands to libamdnuwa -- outputs and workspaces -- and
every operand of the new input-side cases below sits between two 0xFF (NaN) bands inside a buffer the test owns.

1. The existing kernel tests, called as they are inside `with guard(...)`: each carries its own float64 / oracle reference and its
   own tolerance.  With NaN-prefilled outputs its comparison proves that every element was written, report() that nothing is
   non-finite, and the band check on exit that no output and no *_workspace_bytes formula is a tile short.
2. One training step and one generate() with the proxy in every module that allocates (buffer sizing outside kernels.py).
3. New bodies that place the OPERANDS in guarded buffers (NaN row pitch, NaN rows behind the last, NaN bands): a loader that lets a
   byte outside an operand reach the arithmetic gives NaN.  Every tolerance is the constant of the existing test of that kernel, named
   beside it; the error is max-abs / max-abs of the reference, as gpu_util.report() computes it.
Masked keys are never NaN: the reference's 0 * NaN is NaN too, so that is no contract."""
import importlib
import inspect

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from gpu_util import report, bf_round, bf_value  # noqa: E402
from guard_util import FILL, guard, guarded, guarded_empty  # noqa: E402

DEV = 'cuda'
PKG_MODULES = ('kernels', 'ops', 'nuwa_pytorch', 'video_audio', 'decode', 'vqgan_vae', 'optimizer')


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')


def _pkg(*names):
    return [importlib.import_module('nuwa_pytorch_amd.' + n) for n in names]


# ---------------------------------------------------------------------------------------------------
# 1. the existing kernel tests under guard
# ---------------------------------------------------------------------------------------------------

RERUN = []


def _add(mod, fn, *cases):
    for c in (cases or [()]):
        RERUN.append((mod, fn, c))


def _x(*cases):
    """every case with x3 False and True appended"""
    return [c + (x3,) for c in cases for x3 in (False, True)]


k = 'test_gpu_kernels'
_add(k, 'test_gemm_nt', *_x((1, 8, 8), (200, 72, 96), (257, 513, 40), (300, 100, 1376)))
_add(k, 'test_gemm_nt_shift_loader', (2, 17, 4, 32, 24), (3, 48, 4, 64, 130))
_add(k, 'test_gemm_tn', *_x((33, 8, 8), (300, 72, 40), (5000, 85, 32)))
_add(k, 'test_gemm_tn_shift_loader', (2, 17, 4, 32, 24), (2, 129, 8, 128, 200))
_add(k, 'test_gemm_tn_four_wave_kernel', (128, 256, 256))
_add(k, 'test_gemm_nt_long_k_kernel_equals_the_ring', (300, 264, 64))
_add(k, 'test_gemm_nt_two_mfma_form', (300, 520, 96))
_add(k, 'test_batched_tn_whole_m_kernel_equals_the_tiled_one', (3, 4, 100, 200, 32), (1, 2, 71, 300, 64))
_add(k, 'test_gemm_nt_with_geglu_epilogue', (300, 96, 64, False), (300, 96, 64, True), (8, 2752, 512, False))
_add(k, 'test_gemm_nt_with_geglu_backward_epilogue', (300, 48, 64, False), (300, 48, 64, True), (8, 1376, 512, False))
_add(k, 'test_layernorm_fwd_bwd', (7, 32), (33, 48))
_add(k, 'test_layernorm_bwd_chain', (2, 23, 4, 32, False), (1, 5, None, 64, False), (2, 23, 4, 32, 'dh'))
_add(k, 'test_layernorm_post_pre_chain', (2, 23, 4, 32, False), (1, 5, None, 64, False))
_add(k, 'test_stable_layernorm')
_add(k, 'test_geglu')
_add(k, 'test_casts')
_add(k, 'test_embed_fwd_bwd')
_add(k, 'test_embed_bwd_long_runs', ('one code',), ('few codes',), ('uniform',), ('alternating blocks',))
_add(k, 'test_cross_entropy', (5, 64), (17, 1000))
_add(k, 'test_fused_linear_cross_entropy', (300, 192, 64))
_add(k, 'test_fused_linear_cross_entropy_hi_lo', (300, 192, 64))
_add(k, 'test_layernorm_backward_with_fp16_gradients', (1.0,))
_add(k, 'test_fp16_gradient_gemms')
# S3_CASES whose grid is at most 16 x 16 with at most 3 frames
_add(k, 'test_sparse3dna_core', *[(c, x3) for c in (0, 1, 5, 6, 7, 8, 9) for x3 in (False, True)])
_S3_TWO = (((2, 16, 16), (5, 3, 3), (1, 1, 1), None), ((3, 16, 16), (3, 3, 3), (4, 4, 4), 300))
_add(k, 'test_sparse3dna_bwd_recomputing_key_side', *_S3_TWO)
_add(k, 'test_sparse3dna_fwd_f16_core', *_S3_TWO)
_add(k, 'test_sparse3dna_fwd_multi_row_tiles', *[(rows,) + c + (False,) for rows in (2, 4) for c in _S3_TWO])
_add(k, 'test_sparse3dna_bwd_packed_workspace_equals_the_fp32_workspace', (1,), (2,), (4,))
_add(k, 'test_cross_attention_core', *[(c, x3) for c in range(5) for x3 in (False, True)])          # every X_CASES entry has n <= 300
_add(k, 'test_cross_attention_bwd_recomputing_key_side', (2, 96, 33), (2, 32, 287))
_add(k, 'test_cross_attention_xattn6_fwd', *[c + (f16,) for c in ((3, 70, 1), (2, 130, 64), (2, 100, 33), (1, 200, 300)) for f16 in (True, False)])
_add(k, 'test_cross_attention_xattn6_bwd', (3, 70, 1), (2, 130, 64), (2, 100, 33), (4, 300, 200))

# the other kernel-level modules: every case with at most about 300 query rows and 600 keys, tests that take the kernels module,
# the library handle and the oracle only, nothing that captures a graph
k = 'test_gpu_causal_attention'
_add(k, 'test_cattn_kernels_against_the_oracle', *[(causal, f16, masked) + g for causal in (1, 0) for f16 in (True, False) for masked in (False, True)
                                                    for g in ((8, 64, 1), (8, 64, 33), (8, 64, 257), (2, 32, 70), (5, 32, 129), (3, 64, 64))])
k = 'test_gpu_long_attention'
_add(k, 'test_rectangular_kernels_against_the_oracle', *[(f16, masked) + g for f16 in (True, False) for masked in (False, True)
                                                          for g in ((8, 64, 1, 300), (8, 64, 257, 33), (2, 32, 70, 513), (5, 32, 129, 320), (3, 64, 31, 64))])
k = 'test_gpu_xm_long'
_add(k, 'test_kernel_against_the_fp32_formula', *[(T, h, dh, x3) for T in (1, 31, 126, 127, 128, 288, 289) for h, dh in ((8, 64), (3, 64), (1, 32), (5, 32))
                                                   for x3 in (False, True)])
_add(k, 'test_kernel_reads_its_window_only', *_x((300, 8, 64), (127, 3, 64), (1, 5, 32)))
k = 'test_gpu_wide_grid'
_add(k, 'test_wide_sparse3dna_core', *_x((0,), (5,)))               # 17 x 17 = 289 rows; 64 wide, 5 rows + 7 tokens = 328 rows
k = 'test_gpu_vae_wide'
_add(k, 'test_tiled_core_against_float64', (2, 2, 64, 18, 'bias'), (2, 2, 64, 18, 'table'))            # 18 x 18 = 324 positions
_add(k, 'test_tiled_core_on_tiny_maps', (1, 1, 1, 1), (2, 2, 7, 2), (1, 3, 64, 5), (3, 2, 31, 9))
_add(k, 'test_running_maximum_moves_at_every_key_tile')
_add(k, 'test_tiled_core_against_the_resident_kernels', (16,), (17,))
k = 'test_gpu_attention_bwd16'
_add(k, 'test_sparse3dna_bwd16_vs_oracle', (0,), (1,), (2,))                                          # 16 x 16 grids, at most 3 frames
_add(k, 'test_cross_attention_bwd16_vs_oracle', (0,), (1,), (2,), (3,), (4,), (6,))
_add(k, 'test_cross_attention_bwd16_unrounded_null_key')
k = 'test_gpu_decode'
_add(k, 'test_s3_decode_rows_equal_full_attention', *[(c, x3) for c in range(4) for x3 in (False, True)])
_add(k, 'test_decode_shift_rows_equal_shift_video_tokens', (False,), (True,))
_add(k, 'test_xattn_decode_equals_cross_attention_core', *[(c, x3) for c in range(4) for x3 in (False, True)])
_add(k, 'test_few_row_gemm', *_x((1, 512, 512), (4, 1536, 512), (8, 2752, 512), (9, 512, 1376), (32, 100, 64), (3, 77, 2752)))
_add(k, 'test_decode_ln_fuses_post_norm_pre_norm_and_shift', *[(D, ybf, x3) for D, ybf in ((64, False), (512, True), (1024, False)) for x3 in (False, True)])
k = 'test_gpu_vae'
_add(k, 'test_conv2d', (2, 3, 32, 32, 32, 5, 1, 2, False), (2, 32, 32, 32, 64, 4, 2, 1, True), (3, 64, 8, 8, 64, 3, 1, 1, False),
     (3, 64, 8, 8, 192, 1, 1, 0, False), (1, 5, 7, 9, 130, 3, 1, 1, True), (1, 128, 16, 16, 256, 4, 2, 1, True), (2, 6, 9, 11, 70, 2, 1, 0, False),
     (1, 4, 12, 12, 8, 7, 1, 3, True), (1, 3, 10, 10, 20, 3, 2, 1, False))
_add(k, 'test_groupnorm', (2, 64, 8, 16, True), (3, 32, 5, 16, False), (1, 512, 16, 16, True))
_add(k, 'test_vq_argmax', (100, 64, 16), (1, 5, 2), (64, 130, 32), (131, 1000, 256), (7, 33, 256))
del k


def _fixture_values():
    from nuwa_pytorch_amd import kernels, _lib
    from oracle import nuwa_oracle
    return {'K': kernels, 'O': nuwa_oracle, 'O_': nuwa_oracle, 'L': _lib.lib()}


@pytest.mark.parametrize('mod,fn,case', RERUN, ids=[f'{m[9:]}.{f[5:]}{list(c)}'.replace(' ', '') for m, f, c in RERUN])
def test_existing_kernel_test_under_guard(mod, fn, case):
    _gpu()
    m = importlib.import_module(mod)
    f = getattr(m, fn)
    fx = _fixture_values()
    names = list(inspect.signature(f).parameters)
    given = {n: fx[n] for n in names if n in fx}
    params = [n for n in names if n not in fx]
    assert len(params) == len(case), (params, case)                 # a parameter list that changed must be followed here
    from nuwa_pytorch_amd import kernels, ops
    with guard(kernels, ops, m) as gd:                              # the test module too: the outputs it allocates itself are guarded
        f(**given, **dict(zip(params, case)))
        assert gd.made() > 0, 'no allocation of this test went through the proxy: nothing was guarded'


# ---------------------------------------------------------------------------------------------------
# 2. one training step and one generate() with every allocating module under guard
# ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('mode', ['bf16', 'bf16x3-fwd'])
@pytest.mark.parametrize('name', ['g5_nuwa_tiny', 'g6_nuwa_tiny_reversible'])
def test_training_step_under_guard(name, mode):
    """test_gpu_modules.py::test_g5_g6_nuwa_loss_logits_grads restated with its constants (logits and loss at the mode's `tol`, gradients
    at 2 * `gtol` of test_gpu_modules.MODES), plus one FusedAdamW.step(max_grad_norm=1.0), all inside the guard"""
    _gpu()
    import nuwa_pytorch_amd as A
    import test_gpu_modules as tm
    from golden_util import load
    from nuwa_pytorch_amd.optimizer import get_optimizer
    _, tol, gtol = next(t for t in tm.MODES if t[0] == mode)
    Ar, P, G = load(name)
    with guard(*_pkg(*PKG_MODULES)):
        nuwa = tm._tiny_nuwa(A, bool(Ar['reversible']))
        missing, unexpected = nuwa.load_state_dict(P, strict=False)
        assert not unexpected, unexpected
        nuwa = nuwa.to(DEV).train()
        opt = get_optimizer(nuwa.parameters(), lr=3e-4, wd=0.01, filter_by_requires_grad=True)
        A.set_precision(mode)
        try:
            text, vid = Ar['text'].to(DEV), Ar['video_ids'].to(DEV)
            logits = nuwa(text=text, video=vid.reshape(2, -1)[:, :-1], return_loss=False, cond_dropout_prob=0.)
            report(f'guarded {name}[{mode}].logits', logits, Ar['logits'], tol)
            loss = nuwa(text=text, video=vid, return_loss=True, cond_dropout_prob=0.)
            report(f'guarded {name}[{mode}].loss', loss.reshape(1), Ar['loss'].reshape(1), tol)
            loss.backward()
            assert tm.check_grads(nuwa, G, gtol * 2, f'guarded {name}[{mode}]', skip=('.net.blocks.',)) > 40
            before = {k: p.detach().clone() for k, p in nuwa.named_parameters() if p.grad is not None}
            opt.step(max_grad_norm=1.0)
            torch.cuda.synchronize()
            moved = 0
            for k, p in nuwa.named_parameters():
                assert bool(torch.isfinite(p).all()), f'{k} is not finite after the step'
                if k in before:
                    step = (p.detach() - before[k]).abs().max()
                    assert float(step) <= 3e-4 * 1.01 + 0.01 * 3e-4 * float(before[k].abs().max()), f'{k}: a step of {float(step):.3e} at lr 3e-4'
                    moved += int(step > 0)
            assert moved > 40
        finally:
            A.set_precision('bf16')


@pytest.mark.parametrize('name', ['g13a_generate_nuwa', 'g13c_generate_video_audio'])
def test_generate_under_guard(name):
    """test_gpu_decode.py::test_generate_reproduces_the_reference_token_ids in its 'eager' form (cached rows, no HIP graph: the proxy is
    off during a capture anyway): the reference's token ids, from guarded buffers"""
    _gpu()
    import nuwa_pytorch_amd as A
    import test_gpu_decode as td
    with guard(*_pkg(*PKG_MODULES), td):
        td.test_generate_reproduces_the_reference_token_ids(A, name, 'eager')


# ---------------------------------------------------------------------------------------------------
# 3. operands in guarded buffers
# ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def K():
    _gpu()
    from nuwa_pytorch_amd import kernels
    return kernels


def _g(t, ld=None, rows_after=0):
    """CPU (or device) tensor -> guarded device copy"""
    return guarded(t, ld=ld, rows_after=rows_after, device=DEV)


def _gpair(K, t, x3, pad=8, rows_after=3):
    """fp32 values -> BF pair (hi, lo when x3) of guarded 2-D operands: a NaN pitch of `pad` columns, NaN rows behind the last"""
    hi = t.to(torch.bfloat16)
    lo = (t - hi.float()).to(torch.bfloat16) if x3 else None
    ld = t.shape[1] + pad
    return K.BF(_g(hi, ld, rows_after), None if lo is None else _g(lo, ld, rows_after))


def _pair64(p):
    v = p.hi.double().cpu()
    return v + p.lo.double().cpu() if p.lo is not None else v


SKIPPED_FORMS = []            # (form, shape, why): filled by the tests that consult a *_supported query; the list is in DESIGN.md 2.1


def _skipped(form, shape, why):
    SKIPPED_FORMS.append((form, shape, why))
    print('SKIPPED FORM', SKIPPED_FORMS[-1])


@pytest.mark.parametrize('M,N,Kd', [(1, 8, 8), (257, 513, 40), (200, 72, 96), (300, 264, 1088)])
@pytest.mark.parametrize('form', ['bf16', 'hi+lo', 'f16ops', 'f16x2'])
def test_gemm_nt_operands_in_guarded_buffers(K, M, N, Kd, form):
    """A [M, K] and B [N, K] with ld = K + 8 and 3 rows behind, bias guarded.  Tolerances: test_gemm_nt (fp32 output 2e-6 bf16 /
    2e-5 hi + lo; bf16 output 2 ** -8; hi + lo output 3e-5), test_gemm_nt_fp16_operands_and_ln_fp16_copy (y_f32 2e-6, u 2 ** -8),
    test_gemm_nt_two_mfma_form (f32 3e-6, bf16 2 ** -8)"""
    torch.manual_seed(0)
    a = torch.randn(M, Kd) * (1 + torch.arange(Kd) % 3)
    b = torch.randn(N, Kd) + 0.25
    bias = torch.randn(N)
    tag = f'guarded gemm_nt[{form},{M},{N},{Kd}]'
    with guard(K):
        if form in ('bf16', 'hi+lo'):
            x3 = form == 'hi+lo'
            A, Bm = _gpair(K, a, x3), _gpair(K, b, x3)
            ref = _pair64(A) @ _pair64(Bm).t()
            out = K.gemm_nt(A, Bm, bias=_g(bias), alpha=0.5)
            report(tag + '.f32', out, (0.5 * ref + bias.double()).float(), 2e-5 if x3 else 2e-6)
            outb = K.gemm_nt(A, Bm, out_bf16=True)
            report(tag + '.bf16', outb.hi.float(), ref.float(), 2 ** -8)
            if x3:
                report(tag + '.hilo', bf_value(outb), ref.float(), 3e-5)
            return
        a16, b16 = (a * 0.7).half(), (b * 0.2).half()
        A16 = _g(a16, Kd + 8, 3)
        said_yes = 0
        if form == 'f16ops':
            B16 = _g(b16, Kd + 8, 3)
            ref = a16.double() @ b16.double().t()
            for out_bf16, tol in ((False, 2e-6), (True, 2 ** -8)):
                if not K.gemm_nt_f16ops_ok(M, N, Kd, out_bf16=out_bf16):
                    _skipped(form, (M, N, Kd, f'out_bf16={out_bf16}'), 'amdnuwa_gemm_nt_f16ops_supported says no')
                    continue
                said_yes += 1
                report(tag + f'.out_bf16={out_bf16}', K.gemm_nt_f16ops(A16, B16, out_bf16=out_bf16).float(), ref.float(), tol)
        else:
            wh, wl = K.f16_pair(b * 0.05)
            ref = a16.double() @ (wh.double() + wl.double()).t()
            wp = (_g(wh, Kd + 8, 3), _g(wl, Kd + 8, 3))
            if K.gemm_nt_f16x2_ok(M, N, Kd, out_bf16=False):
                said_yes += 1
                report(tag + '.f32', K.gemm_nt_f16x2(A16, wp, bias=_g(bias)), (ref + bias.double()).float(), 3e-6)
            else:
                _skipped(form, (M, N, Kd, 'out_bf16=False'), 'amdnuwa_gemm_nt_f16x2_supported says no')
            if K.gemm_nt_f16x2_ok(M, N, Kd, out_bf16=True):
                said_yes += 1
                report(tag + '.bf16', K.gemm_nt_f16x2(A16, wp, out_bf16=True).hi.float(), ref.float(), 2 ** -8)
            else:
                _skipped(form, (M, N, Kd, 'out_bf16=True'), 'amdnuwa_gemm_nt_f16x2_supported says no')
        # the queries are host arithmetic on the shape: what they answer for these four shapes is pinned, so that a form cannot drop
        # out of this test unnoticed (DESIGN.md 2.1 lists the same)
        want = {('f16ops', 200): 1, ('f16ops', 300): 1, ('f16x2', 200): 2, ('f16x2', 300): 2}.get((form, M), 0)
        assert said_yes == want, (form, M, N, Kd, said_yes, want)


def test_gemm_nt_shift_loader_reads_nothing_before_the_first_row(K):
    """test_gemm_nt_shift_loader's (2, 17, 4, 32, 24) at its 2e-6: the rows the shifted loader would take from before sample 0's row 0
    are the front band"""
    import test_gpu_kernels as tk
    B, ntok, fmap, D, N = 2, 17, 4, 32, 24
    torch.manual_seed(1)
    a = bf_round(torch.randn(B * ntok, D))
    w = bf_round(torch.randn(N, D))
    ref = tk.shift_ref(a, ntok, fmap).double() @ w.double().t()
    with guard(K):
        out = K.gemm_nt(_gpair(K, a, False), _gpair(K, w, False), shift=(ntok, fmap))
        report('guarded gemm_nt_shift', out, ref.float(), 2e-6)


@pytest.mark.parametrize('N', [513, 72])
@pytest.mark.parametrize('x3', [False, True])
def test_gemm_nt_into_a_pitched_output(K, N, x3):
    """out= a guarded view with ldc = N + 8, fp32 and the bf16 pair: test_gemm_nt's tolerances; the pad columns stay FILL (checked on exit)"""
    M, Kd = 257, 40
    torch.manual_seed(0)
    a, b = torch.randn(M, Kd) * (1 + torch.arange(Kd) % 3), torch.randn(N, Kd) + 0.25
    with guard(K):
        A, Bm = _gpair(K, a, x3), _gpair(K, b, x3)
        ref = _pair64(A) @ _pair64(Bm).t()
        out = _g(torch.full((M, N), float('nan')), N + 8, 2)
        K.gemm_nt(A, Bm, out=out)
        report(f'guarded gemm_nt_ldc.f32[{N},x3={x3}]', out, ref.float(), 2e-5 if x3 else 2e-6)
        nanb = torch.full((M, N), float('nan'), dtype=torch.bfloat16)
        ob = K.BF(_g(nanb, N + 8, 2), _g(nanb, N + 8, 2) if x3 else None)
        K.gemm_nt(A, Bm, out=ob, out_bf16=True)
        report(f'guarded gemm_nt_ldc.bf16[{N},x3={x3}]', ob.hi.float(), ref.float(), 2 ** -8)
        if x3:
            report(f'guarded gemm_nt_ldc.hilo[{N}]', bf_value(ob), ref.float(), 3e-5)


@pytest.mark.parametrize('R', [33, 300, 2560 + 37])
@pytest.mark.parametrize('x3', [False, True])
def test_gemm_tn_operands_in_guarded_buffers(K, R, x3):
    """N1 = 85, N2 = 30: the columns up to the next multiple of 8 (readable by contract, content irrelevant) are NaN, so are 3 rows behind
    row R; out a NaN-filled view with ldc > N2: beta = 0 must not read it.  test_gemm_tn's 3e-6 (bf16) / 3e-5 (hi + lo)"""
    N1, N2 = 85, 30
    torch.manual_seed(2)
    a = torch.randn(R, N1) * (1 + torch.arange(N1) % 5)
    b = torch.randn(R, N2) - 0.3
    tol = 3e-5 if x3 else 3e-6
    with guard(K):
        A, Bm = _gpair(K, a, x3, pad=88 - N1), _gpair(K, b, x3, pad=40 - N2)
        ref = 2.0 * (_pair64(A).t() @ _pair64(Bm))
        out = _g(torch.full((N1, N2), float('nan')), 40, 2)
        K.gemm_tn(A, Bm, out, alpha=2.0, beta=0.0, N1=N1, N2=N2)
        report(f'guarded gemm_tn[{R},x3={x3}]', out, ref.float(), tol)
        out2 = _g(torch.ones(N1, N2), 40, 2)
        K.gemm_tn(A, Bm, out2, alpha=1.0, beta=1.0, N1=N1, N2=N2)
        report(f'guarded gemm_tn_beta[{R},x3={x3}]', out2, (ref / 2 + 1).float(), tol)


def test_batched_tn_operands_in_guarded_buffers(K):
    """the batched whole-M TN product (xattn_kv_grads: dK = dS^T q * scale, dV = P'^T dO per sample and head) at
    test_batched_tn_whole_m_kernel_equals_the_tiled_one's (3, 4, 100, 200, 32) and its 2e-3: dS / P' as [.., :mx] views of guarded
    [B, heads, n, JP] arrays whose columns past mx are NaN, q and dO pitched by 8 NaN columns with 3 NaN rows behind"""
    Bq, heads, n, T, dh = 3, 4, 100, 200, 32
    torch.manual_seed(5 + n)
    g = K.x_geom(Bq, n, T, heads, dh)
    inner = heads * dh
    mx = (T + 1 + 7) // 8 * 8
    full = lambda t: torch.cat((t, torch.full((Bq, heads, n, g.JP - mx), float('nan'))), -1).to(torch.bfloat16)
    dS, Pm = full(bf_round(torch.randn(Bq, heads, n, mx))), full(bf_round(torch.rand(Bq, heads, n, mx)))
    q, do = bf_round(torch.randn(Bq * n, inner)), bf_round(torch.randn(Bq * n, inner))
    with guard(K):
        dKp, dVp = K.xattn_kv_grads(g, K.BF(_g(dS)[..., :mx], None), K.BF(_g(Pm)[..., :mx], None), _gpair(K, q, False), _gpair(K, do, False))
        want_k = torch.einsum('bhnj,bnhd->bhjd', dS[..., :mx].double(), q.double().reshape(Bq, n, heads, dh)) * g.scale
        want_v = torch.einsum('bhnj,bnhd->bhjd', Pm[..., :mx].double(), do.double().reshape(Bq, n, heads, dh))
        report('guarded tn_whole_m.dK', dKp[:, :, :mx], want_k.float(), 2e-3)
        report('guarded tn_whole_m.dV', dVp[:, :, :mx], want_v.float(), 2e-3)


@pytest.mark.parametrize('R,D,shift', [(7, 32, None), (33, 48, None), (33, 48, (11, 2)), (130, 512, None)])
def test_layernorm_operands_in_guarded_buffers(K, R, D, shift):
    """ln_fwd (pre, post), ln_bwd (pair and accumulating forms), ln_post_pre_fwd and ln_bwd_chain with x, resid, dy, w, b, mean and rstd in
    guarded buffers.  Tolerances: test_layernorm_fwd_bwd (pre 2e-5, post 2e-6, dx pair 3e-5, dw / db 1e-5, dsum 1e-4, dx acc 1e-5),
    test_layernorm_post_pre_chain (x 2e-5, h 8e-3), test_layernorm_bwd_chain (dx 2e-5, dy_prev 3e-5, dw / dw_prev / db_prev 2e-5)"""
    from oracle import nuwa_oracle as O
    torch.manual_seed(4)
    B = R // shift[0] if shift else 1

    def sh(t):                                              # shift(LN(.)) of the [R, D] rows
        return O.shift_video_tokens(t.reshape(B, R // B, D), shift[1]).reshape(R, D) if shift else t

    x = (torch.randn(R, D) * 2 + 0.5).double().requires_grad_(True)
    res = torch.randn(R, D).double().requires_grad_(True)
    w, b = torch.randn(D).double().requires_grad_(True), torch.randn(D).double().requires_grad_(True)
    w2, b2 = torch.randn(D), torch.randn(D)
    g = torch.randn(R, D)
    ln = F.layer_norm(x, (D,), w, b)
    tag = f'[{R},{D},{shift}]'
    f32 = lambda t: t.detach().float()
    K.set_precision('bf16x3')
    try:
        with guard(K):
            xd, rd, wd, bd, gd = (_g(f32(t)) for t in (x, res, w, b, g))
            out, m, r, _ = K.ln_fwd(xd, wd, bd, shift=shift)
            report('guarded ln_fwd_pre' + tag, bf_value(out), f32(sh(ln)), 2e-5)
            yo, m2, r2 = K.ln_fwd(xd, wd, bd, resid=rd)
            report('guarded ln_fwd_post' + tag, yo, f32(ln + res), 2e-6)
            # backward of h = shift(LN(x)) for the gradient g
            (sh(ln) * g.double()).sum().backward()
            m2, r2 = _g(m2), _g(r2)
            dx, dw, db, ds = K.ln_bwd(gd, xd, m2, r2, wd, to_bf=True, want_dsum=True, shift=shift)
            report('guarded ln_bwd_dx_bf' + tag, bf_value(dx), f32(x.grad), 3e-5)
            report('guarded ln_bwd_dw' + tag, dw, f32(w.grad), 1e-5)
            report('guarded ln_bwd_db' + tag, db, f32(b.grad), 1e-5)
            report('guarded ln_bwd_dsum' + tag, ds, f32(x.grad.sum(0)), 1e-4)
            dres = torch.randn(R, D)
            dx2, _, _, _ = K.ln_bwd(gd, xd, m2, r2, wd, dres=_g(dres), shift=shift)
            report('guarded ln_bwd_dx_acc' + tag, dx2, f32(x.grad + dres.double()), 1e-5)
            # post-norm + residual, then the next block's pre-norm (+ shift)
            xo, _, _, h, m1, r1 = K.ln_post_pre_fwd(xd, rd, wd, bd, _g(w2), _g(b2), next_shift=shift)
            x_ref = (ln + res).detach()
            report('guarded ln_post_pre.x' + tag, xo, f32(x_ref), 2e-5)
            report('guarded ln_post_pre.h' + tag, bf_value(h), f32(sh(F.layer_norm(x_ref, (D,), w2.double(), b2.double()))), 8e-3)
            # chain: stream row xs, h = shift(LN(xs; w2)) receives dh, the row also receives g; the block before it is LN(yprev; wp)
            xs = x_ref.clone().requires_grad_(True)
            w2r = w2.double().requires_grad_(True)
            dh = torch.randn(R, D)
            (sh(F.layer_norm(xs, (D,), w2r, torch.zeros(D).double())) * dh.double()).sum().backward()
            dx_ref = g.double() + xs.grad
            yprev = torch.randn(R, D).double().requires_grad_(True)
            wp, bp = torch.randn(D).double().requires_grad_(True), torch.zeros(D).double().requires_grad_(True)
            (F.layer_norm(yprev, (D,), wp, bp) * dx_ref).sum().backward()
            xsd, ypd = _g(f32(xs)), _g(f32(yprev))
            zeros = _g(torch.zeros(D))
            _, mc, rc, _ = K.ln_fwd(xsd, _g(w2), zeros)
            _, mp, rp = K.ln_fwd(ypd, _g(f32(wp)), zeros, resid=_g(torch.zeros(R, D)))
            cdx, cdw, cdb, cdy, cdwp, cdbp, _ = K.ln_bwd_chain(_g(dh), xsd, _g(mc), _g(rc), _g(w2), gd, ypd, _g(mp), _g(rp), _g(f32(wp)),
                                                              shift=shift, want_dsum=True)
            report('guarded ln_bwd_chain.dx' + tag, cdx, f32(dx_ref), 2e-5)
            report('guarded ln_bwd_chain.dy_prev' + tag, bf_value(cdy), f32(yprev.grad), 3e-5)
            report('guarded ln_bwd_chain.dw' + tag, cdw, f32(w2r.grad), 2e-5)
            report('guarded ln_bwd_chain.dw_prev' + tag, cdwp, f32(wp.grad), 2e-5)
            report('guarded ln_bwd_chain.db_prev' + tag, cdbp, f32(bp.grad), 2e-5)
    finally:
        K.set_precision('bf16')


@pytest.mark.parametrize('R,C', [(5, 64), (17, 1000)])
def test_cross_entropy_operands_in_guarded_buffers(K, R, C):
    """test_cross_entropy's 1e-6 (loss) and 3e-5 (dlogits); targets include 0 and C - 1"""
    torch.manual_seed(10)
    logits = (torch.randn(R, C) * 3).double().requires_grad_(True)
    t = torch.randint(0, C, (R,))
    t[0], t[-1] = 0, C - 1
    loss = F.cross_entropy(logits, t)
    loss.backward()
    K.set_precision('bf16x3')
    try:
        with guard(K):
            lk, dl = K.ce_fwd(_g(logits.detach().float()), _g(t), 1.0 / R)
            report(f'guarded ce_loss[{R},{C}]', lk.reshape(1), loss.detach().float().reshape(1), 1e-6)
            report(f'guarded ce_dlogits[{R},{C}]', bf_value(dl), logits.grad.float(), 3e-5)
    finally:
        K.set_precision('bf16')


@pytest.mark.parametrize('x3', [False, True])
def test_linear_ce_operands_in_guarded_buffers(K, x3):
    """(R, C, K) = (300, 192, 64), h and w pitched by 8 NaN columns with 3 NaN rows behind, targets guarded: loss 2e-6 and dlogits 2 ** -8
    as test_fused_linear_cross_entropy (bf16) and test_fused_linear_cross_entropy_hi_lo (pairs, 'bf16x3-fwd')"""
    R, C, Kd = 300, 192, 64
    gen = torch.Generator().manual_seed(R + C + x3)
    h = torch.randn(R, Kd, generator=gen) * 0.8
    w = torch.randn(C, Kd, generator=gen) * (3.0 / Kd ** 0.5)
    t = torch.randint(0, C, (R,), generator=gen)
    t[0], t[1], t[-1] = 0, C - 1, C - 1
    K.set_precision('bf16x3-fwd' if x3 else 'bf16')
    try:
        with guard(K):
            hb, wb = _gpair(K, h, x3), _gpair(K, w, x3)
            logits = _pair64(hb) @ _pair64(wb).t()
            ref_loss = F.cross_entropy(logits, t).float()
            ref_dl = ((logits.softmax(-1) - F.one_hot(t, C).double()) / R).float()
            out = K.linear_ce(hb, wb, _g(t), 1.0 / R)
            assert out is not None
            report(f'guarded linear_ce[x3={x3}].loss', out[0].reshape(1), ref_loss.reshape(1), 2e-6)
            report(f'guarded linear_ce[x3={x3}].dlogits', out[1].hi.float(), ref_dl, 2 ** -8)
    finally:
        K.set_precision('bf16')


def test_embed_operands_in_guarded_buffers(K):
    """test_embed_fwd_bwd (1e-6 forward, 1e-5 gradients) with every table guarded and ids that hold 0 and the last code at the first and
    the last position of the last frame, row and column"""
    from oracle import nuwa_oracle as O
    torch.manual_seed(9)
    B, Fr, H, W, D, C = 2, 3, 4, 4, 32, 20
    n1 = Fr * H * W - 1
    names = ('image_embedding.embed.weight', 'video_bos', 'video_pos_emb.axial1', 'video_pos_emb.axial2', 'video_pos_emb.axial3')
    P = {k: torch.randn(*s, requires_grad=True) for k, s in zip(names, ((C, D), (D,), (Fr, D), (H, D), (W, D)))}
    ids = torch.randint(0, C, (B, n1))
    ids[0, 0], ids[0, -1], ids[1, 0], ids[1, -1] = 0, C - 1, C - 1, 0
    x = O.embed_assemble(ids, P, training=True, frac=0.2)
    g = torch.randn_like(x)
    x.backward(g)
    with guard(K):
        d = {k: _g(v) for k, v in P.items()}
        idd = _g(ids)
        xk = K.embed_fwd(idd, d[names[0]], d[names[2]], d[names[3]], d[names[4]], d[names[1]], B, n1 + 1, H, W, 0.2)
        report('guarded embed_fwd', xk.reshape(B, n1 + 1, D), x.detach(), 1e-6)
        dW, db, d1, d2, d3 = (_g(torch.zeros_like(P[k])) for k in names)
        K.embed_bwd(idd, _g(g.reshape(B * (n1 + 1), D)), dW, d1, d2, d3, db, B, n1 + 1, Fr, H, W, 0.2)
        for nm, got, k in (('dW', dW, names[0]), ('ax1', d1, names[2]), ('ax2', d2, names[3]), ('ax3', d3, names[4]), ('bos', db, names[1])):
            report(f'guarded embed_bwd_{nm}', got, P[k].grad, 1e-5)


# ----- VAE -----

@pytest.mark.parametrize('H,W', [(5, 7), (16, 16)])
@pytest.mark.parametrize('k,stride,pad', [(3, 1, 1), (4, 2, 1)])
def test_conv2d_operands_in_guarded_buffers(K, H, W, k, stride, pad):
    """the zero border must not come from memory: x, w and bias between NaN bands, test_conv2d's 1e-5"""
    torch.manual_seed(0)
    N, Cin, Cout = 2, 5, 70
    x, w, b = torch.randn(N, Cin, H, W), torch.randn(Cout, Cin, k, k) / (Cin * k * k) ** 0.5, torch.randn(Cout)
    with guard(K):
        y = K.conv2d_fwd(_g(x), _g(w), _g(b), stride, pad, leaky=True)
        report(f'guarded conv2d[{H}x{W},k{k},s{stride}]', y, F.leaky_relu(F.conv2d(x.double(), w.double(), b.double(), stride=stride, padding=pad), 0.1).float(), 1e-5)
        y2 = K.conv2d_fwd(_g(x), _g(w), None, stride, pad)
        report(f'guarded conv2d_nobias[{H}x{W},k{k},s{stride}]', y2, F.conv2d(x.double(), w.double(), None, stride=stride, padding=pad).float(), 1e-5)


def test_groupnorm_operands_in_guarded_buffers(K):
    """(3, 32, 5, 16) at test_groupnorm's 1e-5"""
    torch.manual_seed(1)
    x, w, b = torch.randn(3, 32, 5, 5) * 2 + 0.5, torch.randn(32), torch.randn(32)
    with guard(K):
        report('guarded groupnorm', K.groupnorm_fwd(_g(x), _g(w), _g(b), 16, 1e-5), F.group_norm(x.double(), 16, w.double(), b.double(), 1e-5).float(), 1e-5)


@pytest.mark.parametrize('R,Cn,Dc', [(7, 33, 256), (131, 1000, 256)])
def test_vq_argmax_operands_in_guarded_buffers(K, R, Cn, Dc):
    """test_vq_argmax's checks (ids equal wherever the top-2 gap exceeds 1e-5, similarity at 1e-5) with rows and codebook between NaN bands"""
    from oracle import nuwa_oracle as O
    torch.manual_seed(2)
    x, cb = torch.randn(R, Dc), torch.randn(Cn, Dc)
    idx_ref, gap = (t.reshape(-1) for t in O.vq_eval_lookup(x.t()[None, :, :, None], cb))
    with guard(K):
        idx, sim = K.vq_argmax(_g(x), _g(cb), want_sim=True)
        sure = gap > 1e-5
        assert torch.equal(idx.cpu()[sure], idx_ref[sure]) and float(sure.float().mean()) > 0.99
        report(f'guarded vq_sim[{R}x{Cn}x{Dc}]', sim, (F.normalize(x, dim=-1) * F.normalize(cb, dim=-1)[idx_ref]).sum(-1), 1e-5)


# ----- optimizer -----

def test_fused_adamw_on_guarded_parameters(K):
    """test_fused_clip_adamw_matches_torch at max_grad_norm = 0.5, one step, rtol 2e-5 / atol 3e-5 and the norm at rtol 1e-5 / atol 1e-7:
    parameters and gradients live in guarded buffers before the optimizer is built, the moments and the chunk table are guarded by the proxy"""
    import test_gpu_optimizer as to
    from nuwa_pytorch_amd import optimizer as opt_mod
    a, b = to._model(), to._model()
    with guard(K, opt_mod):
        for p in a.parameters():
            p.data = _g(p.data)
        wd_p, no_wd_p = opt_mod.separate_weight_decayable_params(list(b.parameters()))
        ref = torch.optim.AdamW([{'params': wd_p}, {'params': no_wd_p, 'weight_decay': 0}], lr=3e-3, weight_decay=0.1)
        opt = opt_mod.get_optimizer(a.parameters(), lr=3e-3, wd=0.1, filter_by_requires_grad=True)
        x = torch.randn(16, 37, generator=torch.Generator().manual_seed(1)).to(DEV)
        for m in (a, b):
            (m(x).square().mean() * 50).backward()
        for p in a.parameters():
            p.grad = _g(p.grad)
        n_ref = torch.nn.utils.clip_grad_norm_(b.parameters(), 0.5)
        ref.step()
        opt.step(max_grad_norm=0.5)
        torch.testing.assert_close(opt._norm[0], n_ref, rtol=1e-5, atol=1e-7)
        for (n, pa), pb in zip(a.named_parameters(), b.parameters()):
            torch.testing.assert_close(pa, pb, rtol=2e-5, atol=3e-5, msg=lambda s, n=n: f'{n}: {s}')


# ----- attention -----

@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('causal,n,T', [(True, 1, None), (True, 65, None), (True, 300, None), (False, 70, 1), (False, 33, 513)])
def test_cattn_operands_in_guarded_buffers(K, causal, n, T, masked):
    """q | k | v as column slices of ONE guarded [rows, 3 inner + 8] buffer (the production packed form; rectangular: q and k | v in two
    buffers) with 3 NaN rows behind; null key / value, W_th, the key-mask bytes, dO and the statistics guarded.  Forward fp16 and bf16,
    bf16 backward: 1e-3 / 2e-2 and 7e-2 of test_cattn_kernels_against_the_oracle and test_rectangular_kernels_against_the_oracle"""
    from oracle import nuwa_oracle as O
    B, heads, dh = 2, 3, 64
    inner = heads * dh
    Tk = n if T is None else T
    torch.manual_seed(17)
    q32, kv32 = torch.randn(B * n, inner), torch.randn(B * Tk, 2 * inner)
    nk, nv = torch.randn(heads, dh), torch.randn(heads, dh)
    wth = torch.randn(heads, heads) * 0.5 + torch.eye(heads)
    mask = None
    if masked:
        mask = torch.rand(B, Tk) > 0.3
        mask[0] = False
    dO = torch.randn(B * n, inner).to(torch.bfloat16)
    g = K.cattn_geom(B, n, heads, dh, causal=causal, n_keys=T)
    assert K.cattn_supported(g)
    tag = f'[c={causal},{n}x{Tk},m={masked}]'
    for dt in (torch.float16, torch.bfloat16):
        f16 = dt == torch.float16
        q, kv = q32.to(dt), kv32.to(dt)
        qr = q.float().reshape(B, n, heads, dh).requires_grad_(True)
        kvr = kv.float().reshape(B, Tk, 2, heads, dh).requires_grad_(True)
        nkr, nvr, wr = nk.clone().requires_grad_(True), nv.clone().requires_grad_(True), wth.clone().requires_grad_(True)
        o_ref = O.attention_core(qr, kvr[:, :, 0], kvr[:, :, 1], nkr, nvr, wr, mask, dh ** -0.5, causal=causal)
        with guard(K):
            if T is None:
                packed = _g(torch.cat((q, kv), 1), 3 * inner + 8, 3)
                qd, kd, vd = packed[:, :inner], packed[:, inner:2 * inner], packed[:, 2 * inner:]
            else:
                qd = _g(q, inner + 8, 3)
                kvd = _g(kv, 2 * inner + 8, 3)
                kd, vd = kvd[:, :inner], kvd[:, inner:]
            md = _g(mask.to(torch.uint8)) if masked else None
            nkd, nvd, wd = _g(nk), _g(nv), _g(wth)
            o, stats = K.cattn_fwd(g, qd, kd, vd, nkd, nvd, wd, md)
            report(f'guarded cattn_fwd[f16={f16}]' + tag, (o.hi.float() + o.lo.float()).reshape(B, n, heads, dh), o_ref, 1e-3 if f16 else 2e-2)
            if f16:
                continue
            o_ref.backward(dO.float().reshape(B, n, heads, dh))
            dq, dkv, dwth, dnk, dnv = K.cattn_bwd(g, qd, kd, vd, _g(dO, inner + 8, 3), nkd, nvd, wd, _g(stats), md)
            report('guarded cattn_bwd.dq' + tag, dq.hi.float().reshape(B, n, heads, dh), qr.grad, 7e-2)
            dkvg = dkv.hi.float().reshape(B, Tk, 2, heads, dh)
            report('guarded cattn_bwd.dk' + tag, dkvg[:, :, 0], kvr.grad[:, :, 0], 7e-2)
            report('guarded cattn_bwd.dv' + tag, dkvg[:, :, 1], kvr.grad[:, :, 1], 7e-2)
            report('guarded cattn_bwd.dW' + tag, dwth, wr.grad, 7e-2)
            report('guarded cattn_bwd.dnull_k' + tag, dnk, nkr.grad, 7e-2)
            report('guarded cattn_bwd.dnull_v' + tag, dnv, nvr.grad, 7e-2)


@pytest.mark.parametrize('x3', [False, True])
@pytest.mark.parametrize('shape,kern,dil,n,heads,dh', [((2, 16, 16), (3, 3, 3), (1, 1, 1), None, 8, 64), ((3, 16, 16), (5, 3, 3), (2, 1, 4), None, 8, 64),
                                                      ((3, 16, 16), (5, 3, 3), (2, 1, 4), 530, 8, 64), ((1, 17, 17), (3, 3, 3), (1, 1, 1), None, 8, 32)])
def test_sparse3dna_operands_in_guarded_buffers(K, shape, kern, dil, n, heads, dh, x3):
    """q | k | v in one guarded [rows, 3 inner + 8] buffer with 3 NaN rows behind (the window taps in the padding and the rows past a
    partial last frame must come from nowhere), W_th, the relative-position bias and dO guarded; the last case is test_gpu_wide_grid's
    smallest wide grid.  Tolerances of test_sparse3dna_core (hi + lo: 3e-5 forward, 5e-5 gradients, 1e-4 dW_th), of
    test_sparse3dna_core_rel_pos_bias_on_the_mfma_kernels (bf16: 2 ** -7 forward, 2 ** -6 every gradient) and, for d(bias) in the hi + lo
    form, test_gpu_wide_grid's 1e-4"""
    from oracle import nuwa_oracle as O
    B, inner = 2, heads * dh
    n = shape[0] * shape[1] * shape[2] if n is None else n
    J = kern[0] * kern[1] * kern[2] + 1
    assert K.s3_supported(shape, kern, dil, heads, dh, lo=x3)
    torch.manual_seed(23)
    qkv = torch.randn(B, n, 3, heads, dh)
    do = torch.randn(B, n, heads, dh)
    if not x3:
        qkv, do = bf_round(qkv), bf_round(do)
    qkv.requires_grad_(True)
    wth = (torch.randn(heads, heads) * 0.5 + torch.eye(heads)).requires_grad_(True)
    rel = (torch.randn(heads, J - 1) * 0.7).requires_grad_(True)
    idx = O.neighbor_table(shape, kern, dil, causal=True)
    o_ref = O.sparse3dna_core(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], wth, idx, dh ** -0.5, rel_pos_bias=rel)
    o_ref.backward(do)
    g = K.s3_geom(B, n, shape, kern, dil, heads, dh)
    tag = f'[{shape},{kern},{dil},n={n},x3={x3}]'
    val = bf_value if x3 else (lambda p: p.hi.float())
    with guard(K):
        qkvp = _gpair(K, qkv.detach().reshape(B * n, 3 * inner), x3)
        wd = _g(wth.detach())
        rel_dev = _g(torch.cat((torch.zeros(1, heads), rel.detach().t()), 0).contiguous())
        o = K.sparse3dna_fwd(g, qkvp, wd, rel_bias=rel_dev)
        report('guarded s3_fwd' + tag, val(o).reshape(B, n, heads, dh), o_ref.detach(), 3e-5 if x3 else 2 ** -7)
        dqkv, dwth, drel = K.sparse3dna_bwd(g, qkvp, wd, _gpair(K, do.reshape(B * n, inner), x3), rel_bias=rel_dev)
        gq = qkv.grad.reshape(B * n, 3 * inner)
        for nm, sl in (('dq', slice(0, inner)), ('dk', slice(inner, 2 * inner)), ('dv', slice(2 * inner, 3 * inner))):
            report(f'guarded s3_bwd_{nm}' + tag, val(dqkv)[:, sl], gq[:, sl], 5e-5 if x3 else 2 ** -6)
        wide = shape[2] > 16                     # test_gpu_wide_grid holds dW_th to 1e-4 in both operand forms
        report('guarded s3_bwd_dwth' + tag, dwth, wth.grad, 1e-4 if (x3 or wide) else 2 ** -6)
        report('guarded s3_bwd_drel' + tag, drel[1:].t(), rel.grad, 1e-4 if x3 else 2 ** -6)


@pytest.mark.parametrize('x3', [False, True])
def test_attn_decode_rows_operands_in_guarded_buffers(K, x3):
    """the smallest key count that takes more than one split, every operand (query row, cache, first-row index, null key / value, W_th,
    bias, mask bytes) between NaN bands: test_kernel_against_the_fp32_formula's 3e-5 (hi + lo) / 2 ** -7 (bf16) against its formula"""
    import test_gpu_xm_long as tx
    T = next(t for t in range(1, 1000) if K.attn_decode_rows_splits(t) > 1)
    B, heads, dh = 3, 3, 64
    q, kv, nk, nv, wth, bias, mask, fd = tx._case(B, T, heads, dh, x3, seed=T + B)
    ref = tx._formula(bf_value(q), bf_value(kv), 0, T, nk, nv, wth, bias, mask)
    with guard(K):
        gp = lambda p: K.BF(_g(p.hi), None if p.lo is None else _g(p.lo))
        o = K.attn_decode_rows(gp(q), gp(kv), _g(fd), T, heads, dh, _g(nk), _g(nv), _g(wth), th_bias=_g(bias), mask_u8=_g(mask.to(torch.uint8)))
        report(f'guarded attn_decode_rows[T={T},x3={x3}]', bf_value(o), ref, 3e-5 if x3 else 2 ** -7)


@pytest.mark.parametrize('form', ['bias', 'table'])
@pytest.mark.parametrize('N,heads,c,S', [(1, 3, 64, 5), (2, 8, 64, 20)])
def test_vqattn_core_operands_in_guarded_buffers(K, N, heads, c, S, form):
    """both bias forms of the VQGanVAE attention core on a ragged 5 x 5 map and on 20 x 20, the bias form on the tiled kernel (tuning key
    15 = 2), qkv, scale and bias / table between NaN bands: test_gpu_vae_wide's TOL = 2e-5 against its float64 reference"""
    import test_gpu_vae_wide as tw
    from nuwa_pytorch_amd import _lib
    if S == 20:
        qkv, bias, table, scale, ref = tw._case(N, heads, c, S)
    else:
        gen = torch.Generator().manual_seed(S)
        qkv, scale = tw._qkv(N, heads, c, S * S, gen), tw.sharp_scale(heads, S * S, c, gen)
        table = torch.randn(heads, 2 * S - 1, 2 * S - 1, generator=gen)
        bias = tw.gather_table(table, S).contiguous()
        ref, _ = tw.core_ref64(qkv, bias, scale, heads)
    with guard(K):
        if form == 'bias':
            with tw.tuning15(_lib.lib(), 2):
                out = K.vqattn_core(_g(qkv), _g(scale), heads, bias=_g(bias))
        else:
            out = K.vqattn_core(_g(qkv), _g(scale), heads, rel_table=_g(table))
        report(f'guarded vqattn[{form},S{S}]', out, ref, tw.TOL)


@pytest.mark.parametrize('B,n,T', [(3, 70, 1), (2, 130, 64), (4, 300, 200)])      # (the last: the one shape of the list whose xattn6 backward runs)
def test_xattn6_and_xattn2_operands_in_guarded_buffers(K, B, n, T):
    """xattn6 pack + forward (fp16 and bf16 rows) + backward, and xattn_pack + xattn2 forward / backward on the same bf16 rows: q and
    k | v pitched by 8 NaN columns with 3 NaN rows behind, null key / value, W_th, mask bytes, dO and the statistics between NaN bands.
    Tolerances of test_cross_attention_xattn6_fwd (1e-3 fp16, 2 ** -7 bf16), test_cross_attention_xattn6_bwd (2 ** -6) and
    test_cross_attention_core's xattn2 checks (2 ** -7 forward, 2 ** -6 gradients)"""
    from oracle import nuwa_oracle as O
    heads, dh = 8, 64
    inner = heads * dh
    torch.manual_seed(13)
    q = bf_round(torch.randn(B, n, heads, dh)).requires_grad_(True)
    kv = bf_round(torch.randn(B, T, 2, heads, dh)).requires_grad_(True)
    nk, nv = bf_round(torch.randn(heads, dh)).requires_grad_(True), bf_round(torch.randn(heads, dh)).requires_grad_(True)
    wth = (torch.randn(heads, heads) * 0.5 + torch.eye(heads)).requires_grad_(True)
    mask = torch.rand(B, T) > 0.3
    mask[0] = False
    o_ref = O.attention_core(q, kv[:, :, 0], kv[:, :, 1], nk, nv, wth, mask, dh ** -0.5)
    do = bf_round(torch.randn(B, n, heads, dh))
    o_ref.backward(do)
    q2, kv2 = q.detach().reshape(B * n, inner), kv.detach().reshape(B * T, 2 * inner)
    g = K.x_geom(B, n, T, heads, dh)
    assert K.xattn6_supported(g)
    tag = f'[{B},{n},{T}]'
    with guard(K):
        m8, w = _g(mask.to(torch.uint8)), _g(wth.detach())
        nkd, nvd = _g(nk.detach()), _g(nv.detach())
        # fp16 rows: the same values (bf16-rounded randn is not exact in fp16 -- the reference for this form is taken on the fp16 values)
        q16, kv16 = q2.half(), kv2.half()
        kv4 = kv16.float().reshape(B, T, 2, heads, dh)
        ref16 = O.attention_core(q16.float().reshape(B, n, heads, dh), kv4[:, :, 0], kv4[:, :, 1], nk.detach(), nv.detach(), wth.detach(), mask, dh ** -0.5)
        pk16 = K.xattn6_pack(g, _g(kv16, 2 * inner + 8, 3), m8)
        o16, _ = K.xattn6_fwd(g, _g(q16, inner + 8, 3), pk16, nkd, nvd, w)
        report('guarded xattn6_fwd.f16' + tag, bf_value(o16).reshape(B, n, heads, dh), ref16, 1e-3)
        qp = K.BF(_g(q2.to(torch.bfloat16), inner + 8, 3), None)
        kvp = K.BF(_g(kv2.to(torch.bfloat16), 2 * inner + 8, 3), None)
        dop = K.BF(_g(do.reshape(B * n, inner).to(torch.bfloat16), inner + 8, 3), None)
        pk6 = K.xattn6_pack(g, kvp.hi, m8)
        o, stats = K.xattn6_fwd(g, qp.hi, pk6, nkd, nvd, w, lo=False)
        report('guarded xattn6_fwd.bf16' + tag, o.hi.float().reshape(B, n, heads, dh), o_ref.detach(), 2 ** -7)
        stats = _g(stats)
        pko = K.xattn_pack(g, kvp, nkd, nvd, m8)
        if K.xattn6_bwd_ok(g):
            pkb = K.xattn6_pack_bwd(g, kvp.hi, nkd, nvd, m8)
            dq, dS, Pm, dwth = K.xattn6_bwd(g, qp, dop, pkb, w, stats)
            report('guarded xattn6_bwd.dq' + tag, dq.hi.float().reshape(B, n, heads, dh), q.grad, 2 ** -6)
            report('guarded xattn6_bwd.dwth' + tag, dwth, wth.grad, 2 ** -6)
            dKp, dVp = K.xattn_kv_grads(g, dS, Pm, qp, dop)
            dkv, dnk, dnv = K.xattn_unpack(g, dKp, dVp, lo=False, permuted=True, null_last=True)
            report('guarded xattn6_bwd.dkv' + tag, dkv.hi.float().reshape(B, T, 2, heads, dh), kv.grad, 2 ** -6)
            report('guarded xattn6_bwd.dnull_k' + tag, dnk, nk.grad, 2 ** -6)
            report('guarded xattn6_bwd.dnull_v' + tag, dnv, nv.grad, 2 ** -6)
        else:
            _skipped('xattn6_bwd', (B, n, T), 'xattn6_bwd_ok says no')
        assert K.xattn6_bwd_ok(g) == (T == 200)                    # pinned like the GEMM forms above
        if K.xattn2_supported(g, qp):
            o2, stats2 = K.xattn2_fwd(g, qp, pko, w)
            report('guarded xattn2_fwd' + tag, o2.hi.float().reshape(B, n, heads, dh), o_ref.detach(), 2 ** -7)
            dq2, dS2, Pm2, dwth2 = K.xattn2_bwd(g, qp, dop, pko, w, _g(stats2))
            report('guarded xattn2_dq' + tag, dq2.hi.float().reshape(B, n, heads, dh), q.grad, 2 ** -6)
            report('guarded xattn2_dwth' + tag, dwth2, wth.grad, 2 ** -6)
            dKp2, dVp2 = K.xattn_kv_grads(g, dS2, Pm2, qp, dop)
            dkv2, dnk2, dnv2 = K.xattn_unpack(g, dKp2, dVp2, lo=False, permuted=True)
            report('guarded xattn2_dkv' + tag, dkv2.hi.float().reshape(B, T, 2, heads, dh), kv.grad, 2 ** -6)
            report('guarded xattn2_dnull_k' + tag, dnk2, nk.grad, 2 ** -6)
            report('guarded xattn2_dnull_v' + tag, dnv2, nv.grad, 2 ** -6)
        else:
            _skipped('xattn2', (B, n, T), 'xattn2_supported says no')
        assert K.xattn2_supported(g, qp)


def test_cross2dna_operands_in_guarded_buffers(K):
    """cross2dna_fwd / cross2dna_bwd at test_gpu_peaked_softmax.py::test_cross2dna_kernels' smallest shape (a 4 x 4 map, 2 sketch frames,
    30 % of the keys masked, recipe 'sharp'), with that test's float64 reference, comparison rule (Checks + peaked_util.floors) and
    tolerances (2e-2 / 7e-2 bf16, 1e-3 / 2e-3 hi + lo): q, k | v and dO pitched by 8 NaN columns with 3 NaN rows behind, null key / value,
    mask bytes and W_th between NaN bands.  Row 0 of every sample (<bos>) is left to the caller by the kernels: not compared"""
    import peaked_util as PU
    import test_gpu_peaked_softmax as tp
    fmap, kern, dil, frames, heads, dh, n = PU.XC2_SHAPES[0]
    c = PU.Cross2DNACase('sharp', fmap, kern, dil, frames, heads, dh, n, seed=20)
    B, T, inner = c.B, c.T, heads * dh
    chk = tp.Checks('[guarded]', c.scores, 'sharp')
    g = K.s3_geom(B, n, (-(-(n - 1) // (fmap * fmap)), fmap, fmap), (frames, kern, kern), (1, dil, dil), heads, dh, causal=False)
    for x3 in (False, True):
        rnd = PU.exact if x3 else PU.bf_round
        ref, fl = c.reference(rnd), PU.floors(c, rnd)
        m = 'x3' if x3 else 'bf16'
        tol, gtol = (1e-3, 2e-3) if x3 else (2e-2, 7e-2)
        assert K.s3_supported((1, fmap, fmap), (frames, kern, kern), (1, dil, dil), heads, dh, causal=False, lo=x3)
        with guard(K):
            m8, w = _g(c.mask.to(torch.uint8)), _g(c.wth)
            qp = _gpair(K, c.q.reshape(B * n, -1), x3)
            kvp = _gpair(K, torch.cat((c.k.reshape(B * T, -1), rnd(c.v).reshape(B * T, -1)), 1), x3)
            dop = _gpair(K, rnd(c.dO).reshape(B * n, -1), x3)
            vec = lambda t: K.BF(_g(t.reshape(-1).to(torch.bfloat16)), _g((t.reshape(-1) - t.reshape(-1).to(torch.bfloat16).float()).to(torch.bfloat16)) if x3 else None)
            nk, nv = vec(c.nk), vec(rnd(c.nv))
            rows = lambda p: bf_value(p).reshape(B, n, heads, dh)[:, 1:]
            o = K.cross2dna_fwd(g, qp, kvp, nk, nv, m8, w, T)
            chk(f'cross2dna_fwd.{m}', rows(o), ref['o'], tol, x3)
            dq, dkv, dnk, dnv, dwth = K.cross2dna_bwd(g, qp, kvp, nk, nv, m8, w, dop, T)
            chk(f'cross2dna_bwd.dq.{m}', rows(dq), ref['dq'], gtol, x3, floor=fl['dq'])
            dkv = bf_value(dkv)
            chk(f'cross2dna_bwd.dk.{m}', dkv[:, :inner].reshape(B, T, heads, dh), ref['dk'], gtol, x3, floor=fl['dk'])
            chk(f'cross2dna_bwd.dv.{m}', dkv[:, inner:].reshape(B, T, heads, dh), ref['dv'], gtol, x3, floor=fl['dv'])
            chk(f'cross2dna_bwd.dnull_k.{m}', dnk.reshape(heads, dh), ref['dnk'], gtol, x3, floor=fl['dnk'])
            chk(f'cross2dna_bwd.dnull_v.{m}', dnv.reshape(heads, dh), ref['dnv'], gtol, x3, floor=fl['dnv'])
            chk(f'cross2dna_bwd.dwth.{m}', dwth, ref['dwth'], gtol, x3)
    chk.done()


def test_vae_block_operands_in_guarded_buffers(K):
    """a VQGanAttention block (1 x 1 convolutions, rows_l2norm, vqattn_core, chan_layernorm) on a 5 x 5 map (the module's continuous
    position bias is defined on square maps only) with its parameters and x between NaN bands, against the torch module on the CPU at
    test_vqgan_attention_mfma_form_at_cfg3_shape's 2e-5; glu_chan and upsample_bilinear2x on a 5 x 7 map at
    test_g7_vae_decoder_on_hip's 1e-6"""
    import nuwa_pytorch_amd as A
    from nuwa_pytorch_amd import vqgan_vae
    torch.manual_seed(5)
    m = vqgan_vae.VQGanAttention(dim=64, dim_head=32, heads=2).eval()
    with torch.no_grad():
        m.scale.add_(torch.randn_like(m.scale) * 0.3 + 3.0)
        m.post_norm.g.mul_(torch.rand_like(m.post_norm.g) + 0.5)
        x = torch.randn(2, 64, 5, 5)
        ref = m(x)
        vae = A.VQGanVAE(dim=32, image_size=32, num_layers=2, vq_codebook_size=64, vq_codebook_dim=16, use_vgg_and_gan=False)
        md = m.to(DEV)
        with guard(K, vqgan_vae):
            for p in md.parameters():
                p.data = _g(p.data)
            report('guarded vqgan_attention[5x5]', vae._hip_module(md, _g(x)), ref, 2e-5)
            x6 = torch.randn(2, 6, 5, 7)
            report('guarded upsample2x', K.upsample_bilinear2x(_g(x6)), F.interpolate(x6, scale_factor=2, mode='bilinear', align_corners=False), 1e-6)
            report('guarded glu', K.glu_chan(_g(x6)), F.glu(x6, dim=1), 1e-6)
