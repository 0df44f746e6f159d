"""The peaked / shifted softmax inputs of tests/peaked_util.py, without a GPU: at every shape test_gpu_peaked_softmax.py uses, the float64
reference on each recipe must show what the recipe is for (a sharp row, a running maximum that moves at every key tile, scores that
overflow exp without the maximum subtracted, gradients that do not vanish) -- otherwise a GPU comparison on it says nothing.  The
float64 restatements are pinned to the project's oracle (oracle/nuwa_oracle.py, which casts its softmax to fp32) and to the fp32
formula of the single-query kernel's test."""
import pytest
import torch

import peaked_util as PU
from oracle import nuwa_oracle as O


def _x_cases():
    for n, T in PU.X_SHAPES:
        yield dict(B=2, n=n, T=T, heads=8, dh=64, masked=True, causal=False)
    yield dict(B=2, n=70, T=33, heads=4, dh=32, masked=True, causal=False)
    yield dict(B=2, n=130, T=287, heads=4, dh=32, masked=True, causal=False)
    for T in PU.XDEC_T + PU.ROWS_T:
        yield dict(B=3, n=1, T=T, heads=8, dh=64, masked=True, causal=False)


def _c_cases():
    for heads, dh, n, T, causal in PU.CATTN_CASES:
        for masked in (False, True):
            yield dict(B=2, n=n, T=T, heads=heads, dh=dh, masked=masked, causal=causal)


CASES = list(_x_cases()) + list(_c_cases())


@pytest.mark.parametrize('recipe', PU.RECIPES)
@pytest.mark.parametrize('case', range(len(CASES)), ids=lambda i: '{n}x{T},{heads}x{dh},m={masked},c={causal}'.format(**CASES[i]))
def test_attention_recipes_meet_their_conditions(recipe, case):
    kw = CASES[case]
    if recipe == 'masked_peak' and not kw['masked']:
        return                                           # no key is hidden: the recipe is ramp_up there
    c = PU.AttentionCase(recipe, seed=case, **kw)
    figures = c.check()
    print(recipe, kw, figures)
    # exactness: q, k and the null key survive a trip through bf16 and through fp16
    for t in (c.q, c.k, c.nk):
        assert torch.equal(t.to(torch.bfloat16).float(), t) and torch.equal(t.half().float(), t)


@pytest.mark.parametrize('recipe', PU.S3_RECIPES)
@pytest.mark.parametrize('shape', range(len(PU.S3_SHAPES)))
def test_sparse3dna_recipes_meet_their_conditions(recipe, shape):
    c = PU.S3Case(recipe, *PU.S3_SHAPES[shape], seed=shape)
    print(recipe, PU.S3_SHAPES[shape], c.check())
    for t in (c.q, c.k):
        assert torch.equal(t.to(torch.bfloat16).float(), t) and torch.equal(t.half().float(), t)


@pytest.mark.parametrize('recipe', PU.RECIPES)
@pytest.mark.parametrize('shape', range(len(PU.XC2_SHAPES)))
def test_cross2dna_recipes_meet_their_conditions(recipe, shape):
    c = PU.Cross2DNACase(recipe, *PU.XC2_SHAPES[shape], seed=shape)
    print(recipe, PU.XC2_SHAPES[shape], c.check())
    for t in (c.q, c.k, c.nk):
        assert torch.equal(t.to(torch.bfloat16).float(), t) and torch.equal(t.half().float(), t)


def test_flat_inputs_are_flat():
    """what the existing tests feed: randn q, k with scale dim_head^-0.5 -- a mean row maximum far below the sharp recipe's 0.4 and no
    score that would overflow exp without the maximum"""
    c = PU.AttentionCase('flat', 2, 130, 256, 8, 64, seed=0, masked=False)
    mean_max, _ = PU.row_max_stats(c.scores)
    assert mean_max < 0.2 and float(c.scores.max()) < 8.0, (mean_max, float(c.scores.max()))


@pytest.mark.parametrize('recipe', ['flat', 'sharp', 'ramp_up', 'masked_peak'])
@pytest.mark.parametrize('causal', [False, True])
def test_float64_attention_restatement_equals_the_oracle(recipe, causal):
    """attention_core64 against O.attention_core (fp32) on the same values: fp32 rounding of the oracle is all that separates them"""
    c = PU.AttentionCase(recipe, 2, 70, 70 if causal else 130, 4, 32, seed=3, causal=causal)
    ref = c.reference(PU.bf_round)
    f = lambda t: t.clone().requires_grad_(True)
    q, k, v, nk, nv, w = f(c.q), f(c.k), f(PU.bf_round(c.v)), f(c.nk), f(PU.bf_round(c.nv)), f(c.wth)
    o = O.attention_core(q, k, v, nk, nv, w, c.mask, c.scale, causal=causal)
    o.backward(PU.bf_round(c.dO))
    for name, got in (('o', o.detach()), ('dq', q.grad), ('dk', k.grad), ('dv', v.grad), ('dnk', nk.grad), ('dnv', nv.grad), ('dwth', w.grad)):
        err = float((got.double() - ref[name]).abs().max() / ref[name].abs().max().clamp(min=1e-30))
        assert err < 2e-5, (name, err)


@pytest.mark.parametrize('recipe', ['flat', 'sharp', 'ramp_up', 'big_bias'])
def test_float64_sparse3dna_restatement_equals_the_oracle(recipe):
    c = PU.S3Case(recipe, (3, 4, 4), (3, 3, 3), (1, 2, 1), 2, 32, 41, seed=5)
    ref = c.reference(PU.bf_round)
    f = lambda t: t.clone().requires_grad_(True)
    q, k, v, w = f(c.q), f(c.k), f(PU.bf_round(c.v)), f(c.wth)
    rel = f(c.rel) if c.rel is not None else None
    o = O.sparse3dna_core(q, k, v, w, c.table(), c.scale, rel_pos_bias=rel)
    o.backward(PU.bf_round(c.dO))
    pairs = [('o', o.detach()), ('dq', q.grad), ('dk', k.grad), ('dv', v.grad), ('dwth', w.grad)] + ([('drel', rel.grad)] if rel is not None else [])
    for name, got in pairs:
        err = float((got.double() - ref[name]).abs().max() / ref[name].abs().max().clamp(min=1e-30))
        assert err < 2e-5, (name, err)


@pytest.mark.parametrize('recipe', ['flat', 'sharp', 'ramp_up', 'masked_peak'])
@pytest.mark.parametrize('fmap,kern,dil,frames,n', [(4, 3, 1, 2, 1 + 2 * 16), (5, 3, 2, 3, 1 + 40)])
def test_float64_cross2dna_restatement_equals_the_oracle(recipe, fmap, kern, dil, frames, n):
    """cross2dna_core64 against O.sparse_cross_2dna (fp32) with identity projections: x = (q | 0), context = (k | v), to_q = (I 0),
    to_kv = I, to_out = (I 0)^T; the gradient arriving at the <bos> row is zero, so that row (which the module computes outside the
    kernels) contributes to no gradient"""
    heads, dh = 2, 32
    inner = heads * dh
    c = PU.Cross2DNACase(recipe, fmap, kern, dil, frames, heads, dh, n, seed=7)
    ref = c.reference(PU.bf_round)
    B, T = c.B, c.T
    f = lambda t: t.clone().requires_grad_(True)
    eye = torch.eye(inner)
    P = {'to_q.weight': torch.cat((eye, torch.zeros(inner, inner)), 1), 'to_kv.weight': torch.eye(2 * inner),
         'to_out.weight': torch.cat((eye, torch.zeros(inner, inner)), 0), 'null_k': f(c.nk[:, None]), 'null_v': f(PU.bf_round(c.nv)[:, None]),
         'talking_heads.weight': f(c.wth.reshape(heads, heads, 1, 1, 1))}
    x = f(torch.cat((c.q.reshape(B, n, inner), torch.zeros(B, n, inner)), -1))
    ctx = f(torch.cat((c.k.reshape(B, T, inner), PU.bf_round(c.v).reshape(B, T, inner)), -1))
    y = O.sparse_cross_2dna(x, ctx, P, heads, fmap, kern, dil, context_mask=c.mask)
    dy = torch.zeros(B, n, 2 * inner)
    dy[:, 1:, :inner] = PU.bf_round(c.dO).reshape(B, n, inner)[:, 1:]
    y.backward(dy)
    sh = lambda t, rows: t.reshape(B, rows, heads, dh)
    pairs = [('o', sh(y.detach()[:, 1:, :inner], n - 1)), ('dq', sh(x.grad[:, 1:, :inner], n - 1)), ('dk', sh(ctx.grad[..., :inner], T)),
             ('dv', sh(ctx.grad[..., inner:], T)), ('dnk', P['null_k'].grad[:, 0]), ('dnv', P['null_v'].grad[:, 0]),
             ('dwth', P['talking_heads.weight'].grad.reshape(heads, heads))]
    for name, got in pairs:
        err = float((got.double() - ref[name]).abs().max() / ref[name].abs().max().clamp(min=1e-30))
        assert err < 2e-5, (name, err)


def test_float64_single_query_restatement_equals_the_fp32_formula():
    """attention_core64 with the talking-heads bias against test_gpu_xm_long._formula, the reference of the single-query kernel's test"""
    from test_gpu_xm_long import _formula
    c = PU.AttentionCase('ramp_up', 3, 1, 300, 8, 64, seed=9)
    bias = torch.randn(8) * 0.3
    ref = c.reference(PU.exact, th_bias=bias.double())['o']
    kv = torch.cat((c.k.reshape(3, 300, -1), c.v.reshape(3, 300, -1)), -1)
    got = _formula(c.q.reshape(3, -1), kv, 0, 300, c.nk, c.nv, c.wth, bias, c.mask)
    err = float((got.double() - ref.reshape(3, -1)).abs().max() / ref.abs().max())
    assert err < 2e-5, err
