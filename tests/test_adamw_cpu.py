"""The clip + AdamW value cases of tests/adamw_util.py without a GPU: the chunk layout covers every element once, numpy fp32 models of the
kernels stay inside the derived bounds against the float64 reference on every case (so the bounds admit a correct fp32 implementation
before a GPU is involved), the inputs are not vacuous (a reference with a plausible mistake in it fails the same bounds), and bias
corrections taken from the double betas -- what FusedAdamW._upload did before -- fail them at t = 1.  Writes
profiles/adamw_value_bounds.txt."""
import os

import numpy as np
import pytest

import adamw_util as AU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, 'profiles', 'adamw_value_bounds.txt')
_ROWS = {}


# ---- chunk layout --------------------------------------------------------------------------------------------------------------------------

def _check_layout(numels):
    from nuwa_pytorch_amd.optimizer import CHUNK, chunk_layout
    owner, off, n = chunk_layout(numels)
    assert len(owner) == len(off) == len(n) == sum(-(-x // CHUNK) for x in numels)
    assert bool((off % 16 == 0).all()) and bool((n > 0).all()) and bool((n <= CHUNK).all())
    # in order: owners never decrease, and inside one tensor chunk k starts where chunk k - 1 ended
    assert bool((np.diff(owner) >= 0).all())
    pos = 0
    for i, numel in enumerate(numels):
        sel = owner == i
        start = (off[sel] // 4).astype(np.int64)
        assert start.size and start[0] == 0, i
        assert bool((start[1:] == start[:-1] + n[sel][:-1]).all()), i
        assert int(start[-1] + n[sel][-1]) == numel, i
        pos += numel
    assert int(n.sum()) == pos
    assert AU.chunk_ns(numels) == [int(x) for x in n]


def test_chunk_layout_covers_every_element_once_in_order():
    _check_layout(list(AU.NUMELS) * 2)
    for many in AU.MANY:
        _check_layout([AU.MANY_N] * many)
    rng = np.random.default_rng(7)
    _check_layout([int(x) for x in rng.integers(1, 400000, 60)] + [65536 * 3, 65536 * 3 + 1, 1])


# ---- models inside the bounds, inputs not vacuous --------------------------------------------------------------------------------------------

def _model_step(d, bc_betas=None):
    """adamw_model32 + norm_model32 over the tensors of a case -> lists p, m, v, and (norm, coefficient).  bc_betas: the doubles whose
    powers give the bias corrections (default: the fp32-rounded betas)"""
    h = d['hyper']
    norm32, k32 = AU.norm_model32(d['g'], d['max_norm'])
    if d['max_norm'] is None:
        k32 = np.float32(1.0)
    b1d, b2d = bc_betas or (h['b1'], h['b2'])
    out = []
    for p, g, m, v, wd, t in zip(d['p'], d['g'], d['m'], d['v'], d['wds'], d['steps']):
        bc1, bc2 = AU.bias_corrections32(b1d, b2d, t)
        out.append(AU.adamw_model32(p, g, m, v, h['lr'], h['b1'], h['b2'], h['eps'], wd, bc1, bc2, k32))
    return out, (float(norm32), float(k32))


def _reference(d, dt=0, variant=None):
    return [AU.adamw64(p, g, m, v, d['hyper'], t + dt, d['clip'], wd=wd, variant=variant)
            for p, g, m, v, wd, t in zip(d['p'], d['g'], d['m'], d['v'], d['wds'], d['steps'])]


def _ratios(d, got, refs, e_g):
    w = dict(p=0.0, m=0.0, v=0.0)
    for (p, m, v), r in zip(got, refs):
        b = AU.adamw_bounds(r, d['hyper'], e_g)
        for k, x in (('p', p), ('m', m), ('v', v)):
            w[k] = max(w[k], AU.worst(x, r[k], b[k]))
    return w


@pytest.mark.parametrize('case', AU.CASES, ids=lambda c: c['name'])
def test_models_meet_the_bounds_and_mistakes_do_not(case):
    d = AU.case_data(case)
    h = d['hyper']
    e_g = AU.clip_rel_bound(d['numels'], d['clip'])
    refs = _reference(d)
    got, (norm32, k32) = _model_step(d)
    w = _ratios(d, got, refs, e_g)
    nb = AU.norm_bound(d['numels'])
    wn = abs(norm32 - d['norm']) / (nb * d['norm']) if d['norm'] else float(norm32 != 0.0)
    wk = abs(k32 - d['clip']) / ((nb + 3 * AU.U) * d['clip']) if d['clip'] != 1.0 else float(k32 != 1.0)
    _ROWS[case['name']] = dict(w, norm=wn, coef=wk)
    assert max(w.values()) <= 1.0 and wn <= 1.0 and wk <= 1.0, (case['name'], w, wn, wk)
    if case['recipe'] == 'zeros':
        return
    # the update moves p by more than 100 x its bound on at least 90 % of the elements with a nonzero gradient
    moved = np.concatenate([(np.abs(r['p'] - r['p0']) > 100 * AU.adamw_bounds(r, h, e_g)['p'])[g != 0] for r, g in zip(refs, d['g'])])
    assert moved.mean() >= 0.9, (case['name'], float(moved.mean()))
    # a reference with a mistake in it is more than twice the bound away somewhere: a kernel that computed it would fail
    def far(alt):
        return max(AU.worst(a['p'], r['p'], AU.adamw_bounds(r, h, e_g)['p']) for a, r in zip(alt, refs))
    if all(AU.t_observable(h, t) for t in d['steps']):
        assert far(_reference(d, dt=1)) > 2.0, case['name']
    else:
        assert max(d['steps']) >= 100000 and 1 - h['b2'] ** 100000 == 1.0          # saturated corrections: nothing to observe
    if case['wd'] != 0:
        assert far(_reference(d, variant='decay_after')) > 2.0, case['name']
    assert far(_reference(d, variant='eps_inside')) > 2.0, case['name']


def test_mixed_case_holds_five_different_counts():
    d = AU.case_data(next(c for c in AU.CASES if c['t'] == 'mixed'))
    assert set(d['steps']) == set(AU.STEPS)
    for k in ('lr', 'wd', 'eps', 'betas', 'clip', 'recipe'):
        want = dict(lr={3e-4, 1e-2}, wd={0.0, 0.01, 0.1}, eps={1e-8, 1e-3}, betas={(0.9, 0.999), (0.5, 0.9), (0.0, 0.999)},
                    clip=set(AU.CLIPS), recipe=set(AU.RECIPES))[k]
        assert {c[k] for c in AU.CASES} == want, k
    assert {c['t'] for c in AU.CASES} >= set(AU.STEPS) and any(c['wd_edit'] for c in AU.CASES)


@pytest.mark.parametrize('many', AU.MANY)
@pytest.mark.parametrize('recipe', AU.RECIPES)
def test_norm_model_meets_the_bound_on_many_tensors(many, recipe):
    numels = [AU.MANY_N] * many
    g = AU.make_grads(recipe, numels)
    ref = AU.norm64(g)
    norm32, _ = AU.norm_model32(g)
    nb = AU.norm_bound(numels)
    wn = abs(float(norm32) - ref) / (nb * ref) if ref else float(norm32 != 0.0)
    key = f'norm_many_{recipe}'
    _ROWS[key] = dict(norm=max(wn, _ROWS.get(key, {}).get('norm', 0.0)))
    assert wn <= 1.0, (many, recipe, wn)
    if ref:
        # a finalize loop that stopped after its first 1024 partials, or one dropped chunk of average size, is far outside
        sq = [float(np.sum(x.astype(np.float64) ** 2)) for x in g]
        j = max(i for i in range(many) if sq[i] >= sum(sq) / many)
        assert abs(AU.norm64(g[:j] + g[j + 1:]) - ref) > 2 * nb * ref
        # (at 1025 tensors the one partial behind the first 1024 is, with the per-tensor scales, a tensor of scale 1 among scale 1e4 ones)
        if many > 1024 and (recipe != 'scales' or many >= 2049):
            assert abs(AU.norm64(g[:1024]) - ref) > 2 * nb * ref


# ---- the bias-correction mismatch ----------------------------------------------------------------------------------------------------------------

def test_bias_corrections_from_the_double_betas_fail_at_t1():
    """1 - 0.999 in double is 1e-3; the kernel forms 1.f - float(0.999) = 9.99987e-4.  A step whose corrections come from the double betas is
    an AdamW for no pair of betas: at t = 1 its v-hat is 1.3e-5 off and its update 6.4e-6 of a step, against a bound of a few u"""
    case = next(c for c in AU.CASES if c['name'] == 'randn_t1')
    d = AU.case_data(case)
    refs = _reference(d)
    good, _ = _model_step(d)
    bad, _ = _model_step(d, bc_betas=case['betas'])
    wg, wb = _ratios(d, good, refs, 0.0), _ratios(d, bad, refs, 0.0)
    _ROWS['bias_corrections_double_betas_t1'] = dict(p=wb['p'])
    assert wg['p'] <= 1.0 and wb['p'] > 2.0, (wg, wb)


@pytest.fixture(scope='module', autouse=True)
def _write_profile():
    """after the file's tests: the worst model / bound ratio of each case group and the margin it leaves (1 / ratio); written only by a run
    of the whole file"""
    yield
    if len(_ROWS) < len(AU.CASES) + len(AU.RECIPES) + 1:
        return
    lines = ['# worst (numpy fp32 model - float64 reference) / derived bound per case group, and the margin 1 / ratio it leaves.',
             '# Written by tests/test_adamw_cpu.py; bounds and models: tests/adamw_util.py.  A ratio above 1 fails the test.',
             '# The p bound is two or three roundings of p itself wherever the weight is larger than its update, and a worst-case bound of so few',
             '# terms is nearly attained by some element of a million: a margin below 2 there is the bound being tight, not the model being close to wrong.',
             f'# {"group":34s} {"p":>9s} {"m":>9s} {"v":>9s} {"norm":>9s} {"coef":>9s} {"margin":>8s}']
    for name, r in _ROWS.items():
        cells = ' '.join(f'{r[k]:9.3f}' if k in r else f'{"-":>9s}' for k in ('p', 'm', 'v', 'norm', 'coef'))
        top = max(r.values())
        lines.append(f'  {name:34s} {cells} {(1 / top if top else float("inf")):8.2f}')
    try:
        os.makedirs(os.path.dirname(PROFILE), exist_ok=True)
        with open(PROFILE, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    except OSError:
        pass
