"""The clip + AdamW kernels (csrc/optim.hip through nuwa_pytorch_amd/optimizer.py) against the float64 reference of tests/adamw_util.py at
the bounds derived there: chunk edges, step counts up to 100 000, mixed counts in one launch, every clip kind, skipped parameters, all-zero
and non-finite gradients, the [norm, coefficient] pair over more than 1024 and more than 4096 chunks, and the data-parallel recipe of
INTEGRATION.md whose gradients are views at odd element offsets of one flat bucket.  Parameters, gradients and moments live in guarded,
NaN-prefilled buffers (guard_util); the error / bound ratios go to the parity log (gpu_util.record, tol 1 = the bound)."""
import numpy as np
import pytest
import torch
from torch import nn

import adamw_util as AU
import gpu_util
import guard_util as GU

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SMALL = [(1, 5), (1, 65537), (3, 341), (1025,), (3,), (65536,)]          # a short list for the behavioural tests


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from nuwa_pytorch_amd import optimizer
    return optimizer


def _np(t):
    return t.detach().cpu().numpy().reshape(-1)


def _params(d):
    """guarded parameters with guarded gradients (None where the case holds no gradient)"""
    ps = []
    for i, (shape, p, g) in enumerate(zip(d['shapes'], d['p'], d['g'])):
        q = nn.Parameter(GU.guarded(torch.from_numpy(p).reshape(shape), device=DEV, label=f'p{i}'))
        if g is not None:
            q.grad = GU.guarded(torch.from_numpy(g).reshape(shape), device=DEV, label=f'g{i}')
        ps.append(q)
    return ps


def _optimizer(O, case, d, ps):
    """FusedAdamW over guarded moments (the caller holds guard(O)), seeded through load_state_dict with the case's counts and moments"""
    wd0 = 0.5 if case['wd_edit'] else case['wd']
    opt = O.FusedAdamW(ps, lr=case['lr'], betas=case['betas'], eps=case['eps'], weight_decay=wd0)
    assert [tuple(p.shape) for p in opt.params] == [tuple(s) for s in d['shapes']]
    if case['wd_edit']:
        opt.param_groups[0]['weight_decay'] = case['wd']               # edited after construction, as a schedule would
    sd = opt.state_dict()
    for i, (shape, m, v, t) in enumerate(zip(d['shapes'], d['m'], d['v'], d['steps'])):
        sd['state'][i] = dict(step=torch.tensor(float(t - 1)), exp_avg=torch.from_numpy(m).reshape(shape),
                              exp_avg_sq=torch.from_numpy(v).reshape(shape))
    opt.load_state_dict(sd)
    assert opt.param_steps == [t - 1 for t in d['steps']]
    return opt


def _before(opt):
    return [(_np(p), _np(m), _np(v)) for p, m, v in zip(opt.params, opt.state_m, opt.state_v)]


def _compare(name, opt, d, before, clip, e_g, steps=None, grads=None):
    """p, m, v of every parameter with a gradient against adamw64 from the device's own values before the step -> worst ratios"""
    w = dict(p=0.0, m=0.0, v=0.0)
    steps = d['steps'] if steps is None else steps
    grads = d['g'] if grads is None else grads
    for i, (p, m, v) in enumerate(zip(opt.params, opt.state_m, opt.state_v)):
        if grads[i] is None:
            continue
        r = AU.adamw64(before[i][0], grads[i], before[i][1], before[i][2], d['hyper'], steps[i], clip, wd=d['wds'][i])
        b = AU.adamw_bounds(r, d['hyper'], e_g)
        for k, x in (('p', p), ('m', m), ('v', v)):
            got = _np(x).astype(np.float64)
            assert np.isfinite(got).all(), f'{name}: {k}[{i}] holds non-finite values'
            w[k] = max(w[k], AU.worst(got, r[k], b[k]))
    for k in w:
        gpu_util.record(f'adamw/{name}/{k}', w[k], 0.0, 1.0)
    print(f'adamw/{name}: error / bound  p {w["p"]:.3f}  m {w["m"]:.3f}  v {w["v"]:.3f}')
    return w


def _check_norm(name, out2, d, numels):
    """the device's [norm, coefficient] against norm64 / clip64"""
    norm, coef = (float(x) for x in out2.cpu())
    nb = AU.norm_bound(numels)
    wn = abs(norm - d['norm']) / (nb * d['norm']) if d['norm'] else float(norm != 0.0)
    wk = abs(coef - d['clip']) / ((nb + 3 * AU.U) * d['clip']) if d['clip'] != 1.0 else float(coef != 1.0)
    gpu_util.record(f'adamw/{name}/norm', wn, 0.0, 1.0)
    gpu_util.record(f'adamw/{name}/coef', wk, 0.0, 1.0)
    print(f'adamw/{name}: error / bound  norm {wn:.3f}  coef {wk:.3f}')
    assert wn <= 1.0 and wk <= 1.0, (name, norm, d['norm'], coef, d['clip'], wn, wk)


def _check_steps(opt):
    for i, p in enumerate(opt.params):
        assert float(opt.state[p]['step']) == float(opt.param_steps[i]), i


# ---- one step per case -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', AU.CASES, ids=lambda c: c['name'])
def test_one_step_against_float64(case):
    O = _gpu()
    d = AU.case_data(case)
    e_g = AU.clip_rel_bound(d['numels'], d['clip'])
    with GU.guard(O) as G:
        ps = _params(d)
        opt = _optimizer(O, case, d, ps)
        before = _before(opt)
        opt.step(max_grad_norm=d['max_norm'])
        torch.cuda.synchronize()
        w = _compare(case['name'], opt, d, before, d['clip'], e_g)
        if d['max_norm'] is not None:
            _check_norm(case['name'], opt._norm, d, d['numels'])
        assert max(w.values()) <= 1.0, (case['name'], w)
        assert opt.param_steps == d['steps']
        _check_steps(opt)
        for p, g in zip(ps, d['g']):                                    # the step reads the gradients and never writes them
            assert np.array_equal(_np(p.grad).view(np.uint32), g.view(np.uint32))
        if case['recipe'] == 'zeros':
            # m == 0, v == 0, and p == p * (1 - lr wd) in ONE rounding of the product, bit for bit.  The fp32 decay itself is 1 - lr wd
            # rounded once (a fused multiply-add) or twice (product, then difference): either is the kernel's expression
            lr, F = np.float32(case['lr']), np.float32
            for i, (p, m, v) in enumerate(zip(opt.params, opt.state_m, opt.state_v)):
                assert not _np(m).any() and not _np(v).any()
                wd = F(d['wds'][i])
                decays = {float(F(1.0) - lr * wd), float(F(1.0 - float(lr) * float(wd)))}
                assert any(np.array_equal(_np(p).view(np.uint32), (before[i][0] * F(D)).view(np.uint32)) for D in decays), i
    assert G.made() >= 2 * len(ps)                                       # the moments were guarded too


# ---- clip_grad_norm_ + step() ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['scales_t2_clip0.9', 'const_t2_clip0.01', 'randn_t10_far', 'randn_t100000_zero'])
def test_clip_grad_norm_then_step(name):
    """clip_grad_norm_ scales the gradients in place (bands around g intact: the guard checks them), a coefficient of exactly 1 leaves them
    bit-identical, and the plain step() that follows gives the p of step(max_grad_norm=...) at the bound"""
    O = _gpu()
    case = next(c for c in AU.CASES if c['name'] == name)
    d = AU.case_data(case)
    e_g = AU.clip_rel_bound(d['numels'], d['clip'])
    with GU.guard(O):
        ps = _params(d)
        opt = _optimizer(O, case, d, ps)
        before = _before(opt)
        nrm = O.clip_grad_norm_(opt, d['max_norm'])
        torch.cuda.synchronize()
        _check_norm(name + '/clip_grad_norm_', opt._norm, d, d['numels'])
        assert float(nrm) == float(opt._norm[0])
        k = float(opt._norm[1])
        for p, g in zip(ps, d['g']):
            got = _np(p.grad)
            if d['clip'] == 1.0:
                assert np.array_equal(got.view(np.uint32), g.view(np.uint32))
            else:
                assert np.array_equal(got.view(np.uint32), (g * np.float32(k)).view(np.uint32))      # one product by the device's coefficient
        opt.step()
        torch.cuda.synchronize()
        w = _compare(name + '/clip_then_step', opt, d, before, d['clip'], e_g)
        assert max(w.values()) <= 1.0, (name, w)
        _check_steps(opt)


# ---- skipped parameters ----------------------------------------------------------------------------------------------------------------------

def test_parameters_without_gradient_are_skipped_and_lag():
    O = _gpu()
    case = next(c for c in AU.CASES if c['name'] == 'scales_t2_clip0.9')
    d = AU.case_data(case, shapes=SMALL)
    skipped = (1, 3)
    with GU.guard(O):
        ps = _params(d)
        opt = _optimizer(O, case, d, ps)
        held = {i: ps[i].grad for i in skipped}
        for i in skipped:
            ps[i].grad = None
        before = _before(opt)
        g1 = [None if i in skipped else g for i, g in enumerate(d['g'])]
        norm = AU.norm64([g for g in g1 if g is not None])
        clip = AU.clip64(norm, d['max_norm'])
        e_g = AU.clip_rel_bound(d['numels'], clip)
        opt.step(max_grad_norm=d['max_norm'])
        torch.cuda.synchronize()
        for i in skipped:
            for x, b in zip((opt.params[i], opt.state_m[i], opt.state_v[i]), before[i]):
                assert np.array_equal(_np(x).view(np.uint32), b.view(np.uint32)), i
            assert opt.param_steps[i] == d['steps'][i] - 1
        w = _compare('skipped/first', opt, d, before, clip, e_g, grads=g1)
        assert max(w.values()) <= 1.0, w
        _check_steps(opt)
        # the next step: everyone has a gradient, the skipped ones use their lagging count
        for i in skipped:
            ps[i].grad = held[i]
        before = _before(opt)
        steps2 = [t if i in skipped else t + 1 for i, t in enumerate(d['steps'])]
        opt.step(max_grad_norm=d['max_norm'])
        torch.cuda.synchronize()
        assert opt.param_steps == steps2
        w = _compare('skipped/second', opt, d, before, d['clip'], AU.clip_rel_bound(d['numels'], d['clip']), steps=steps2)
        assert max(w.values()) <= 1.0, w
        # (a count off by one on a lagging parameter is outside the bound: the CPU test shows it for this case)
        _check_steps(opt)


# ---- norm and coefficient ----------------------------------------------------------------------------------------------------------------------

def _gapped(n_tensors, numel, stride=8):
    """n_tensors views of `numel` floats, `stride` floats apart, inside ONE guarded NaN-filled buffer: the floats between two tensors are
    bands of their own, at a few kilobytes for thousands of tensors.  stride 8 keeps every tensor on a 32-byte border"""
    flat = GU.guarded_empty((n_tensors * stride,), torch.float32, DEV)
    grid = flat.view(n_tensors, stride)
    return flat, grid, [grid[i, :numel] for i in range(n_tensors)]


def _gaps_intact(grid, numel):
    return bool((grid[:, numel:].contiguous().view(torch.uint8) == GU.FILL).all())


@pytest.mark.parametrize('many', AU.MANY)
def test_norm_over_many_tensors(many):
    """nchunks on both sides of 1024 (the finalize stride loop) and of 4096, every recipe: [norm, coefficient] at the bound, bit-identical on a
    second call, and clip_grad_norm_ writes nothing between the tensors"""
    O = _gpu()
    numels = [AU.MANY_N] * many
    with GU.guard():
        _, pgrid, pv = _gapped(many, AU.MANY_N)
        _, ggrid, gv = _gapped(many, AU.MANY_N)
        pgrid[:, :AU.MANY_N] = 0.01
        ps = [nn.Parameter(v) for v in pv]
        for p, g in zip(ps, gv):
            p.grad = g
        opt = O.FusedAdamW(ps, lr=3e-4)
        assert opt.nchunks == many
        for recipe in AU.RECIPES:
            g = AU.make_grads(recipe, numels)
            ggrid[:, :AU.MANY_N] = torch.from_numpy(np.stack(g)).to(DEV)
            norm = AU.norm64(g)
            for kind in (0.9, None):
                max_norm = AU.max_norm_of(kind, norm)
                d = dict(norm=norm, clip=AU.clip64(norm, max_norm))
                a = opt.grad_norm(0. if max_norm is None else max_norm).clone()
                b = opt.grad_norm(0. if max_norm is None else max_norm).clone()
                assert torch.equal(a.view(torch.int32), b.view(torch.int32))
                _check_norm(f'many{many}/{recipe}/{kind}', a, d, numels)
            O.clip_grad_norm_(opt, AU.max_norm_of(0.9, norm))
            k = np.float32(float(opt._norm[1]))
            got = ggrid[:, :AU.MANY_N].cpu().numpy()
            assert np.array_equal(got.view(np.uint32), (np.stack(g) * k).view(np.uint32)), recipe
            assert _gaps_intact(ggrid, AU.MANY_N) and _gaps_intact(pgrid, AU.MANY_N), recipe


@pytest.mark.parametrize('recipe', AU.RECIPES)
def test_norm_over_the_value_shapes(recipe):
    O = _gpu()
    case = dict(AU.CASES[0], recipe=recipe, name=f'norm_{recipe}')
    for kind in AU.CLIPS:
        d = AU.case_data(dict(case, clip=kind))
        with GU.guard(O):
            ps = _params(d)
            opt = O.FusedAdamW(ps, lr=3e-4)
            mn = 0. if d['max_norm'] is None else d['max_norm']
            a = opt.grad_norm(mn).clone()
            b = opt.grad_norm(mn).clone()
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
            _check_norm(f'values/{recipe}/{kind}', a, d, d['numels'])


# ---- non-finite gradients ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('max_norm', [None, 1.0])
@pytest.mark.parametrize('bad', [float('inf'), float('nan')])
def test_non_finite_gradient_behaves_as_torch(bad, max_norm):
    """a behavioural pin, not a precision test: one inf / NaN gradient element gives the p, m, v that torch.nn.utils.clip_grad_norm_ +
    torch.optim.AdamW(foreach=False) give on the same device tensors"""
    O = _gpu()
    case = AU.CASES[0]
    d = AU.case_data(case, shapes=SMALL)
    d['g'][1][65536] = bad                                          # the one element of a second, ragged chunk
    with GU.guard(O):
        ps = _params(d)
        twins = [nn.Parameter(p.detach().clone()) for p in ps]
        for t, p in zip(twins, ps):
            t.grad = p.grad.clone()
        opt = O.FusedAdamW(ps, lr=case['lr'], betas=case['betas'], eps=case['eps'], weight_decay=case['wd'])
        wd_p, no_wd_p = O.separate_weight_decayable_params(twins)
        ref = torch.optim.AdamW([{'params': wd_p}, {'params': no_wd_p, 'weight_decay': 0.}], lr=case['lr'], betas=case['betas'],
                                eps=case['eps'], weight_decay=case['wd'], foreach=False)
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_(twins, max_norm)
        ref.step()
        opt.step(max_grad_norm=max_norm)
        torch.cuda.synchronize()
        for i, (p, t) in enumerate(zip(ps, twins)):
            torch.testing.assert_close(p.detach(), t.detach(), equal_nan=True, msg=lambda s, i=i: f'p[{i}]: {s}')
            torch.testing.assert_close(opt.state_m[i], ref.state[t]['exp_avg'], equal_nan=True, msg=lambda s, i=i: f'm[{i}]: {s}')
            torch.testing.assert_close(opt.state_v[i], ref.state[t]['exp_avg_sq'], equal_nan=True, msg=lambda s, i=i: f'v[{i}]: {s}')
        assert not bool(torch.isfinite(ps[1].detach()).all())         # the element did arrive
        _check_steps(opt)


# ---- the data-parallel recipe of INTEGRATION.md ----------------------------------------------------------------------------------------------

class _Odd(nn.Module):
    """parameter sizes 35, 7, 64, 513 and 70 001: a talking-heads matrix, a bias, a square matrix, an odd width and an odd table"""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(11)
        for name, shape in (('heads', (5, 7)), ('bias', (7,)), ('proj', (8, 8)), ('gain', (513,)), ('table', (1, 70001))):
            p = 0.02 * torch.randn(shape, generator=g)
            p.view(-1)[::7] *= 2.0 ** -10
            setattr(self, name, nn.Parameter(p))


def test_integration_recipe_gradients_at_odd_offsets():
    """GradReducer(module) then get_optimizer(...): every p.grad is a view into one flat bucket at the sum of the earlier numels, so most are
    4-byte aligned only.  The step must be bit-identical to the same step on fresh, aligned gradient copies, and both within the bound"""
    O = _gpu()
    from nuwa_pytorch_amd.distributed import GradReducer
    torch.manual_seed(5)
    mods = [_Odd().to(DEV), _Odd().to(DEV)]
    coefs = [torch.randn(p.shape, generator=torch.Generator().manual_seed(20 + i)).to(DEV) for i, p in enumerate(mods[0].parameters())]
    reducer = GradReducer(mods[0])
    with GU.guard(O):
        opts = [O.get_optimizer(m.parameters(), lr=3e-4, wd=0.01, filter_by_requires_grad=True) for m in mods]
        reducer.zero_grad()
        for m in mods:
            sum((p * c).sum() for p, c in zip(m.parameters(), coefs)).backward()
        reducer.finish()
        for p in mods[1].parameters():
            p.grad = p.grad.clone()                                     # fresh allocations
        assert any(p.grad.data_ptr() % 16 for p in opts[0].params) and all(p.grad.data_ptr() % 4 == 0 for p in opts[0].params)
        assert all(p.grad.data_ptr() % 16 == 0 for p in opts[1].params)
        assert all(p.grad.data_ptr() == reducer.buckets[0]['flat'].data_ptr() + 4 * off for p, off in
                   zip(mods[0].parameters(), (0, 35, 42, 106, 619)))
        grads = [_np(p.grad).copy() for p in opts[0].params]
        assert all(np.array_equal(g, _np(p.grad)) for g, p in zip(grads, opts[1].params))
        norm = AU.norm64(grads)
        max_norm = AU.max_norm_of(0.9, norm)
        clip = AU.clip64(norm, max_norm)
        before = _before(opts[0])
        for o in opts:
            o.step(max_grad_norm=max_norm)
        torch.cuda.synchronize()
        assert torch.equal(opts[0]._norm.view(torch.int32), opts[1]._norm.view(torch.int32))
        for i in range(len(grads)):
            for a, b in ((opts[0].params[i], opts[1].params[i]), (opts[0].state_m[i], opts[1].state_m[i]), (opts[0].state_v[i], opts[1].state_v[i])):
                assert torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32)), i
        numels = [g.size for g in grads]
        d = dict(hyper=AU.hyper32(3e-4, (0.9, 0.999), 1e-8), steps=[1] * len(grads), g=grads, norm=norm, clip=clip,
                 wds=[0.01 if p.ndim >= 2 else 0.0 for p in opts[0].params])
        e_g = AU.clip_rel_bound(numels, clip)
        for tag, o in (('bucket_views', opts[0]), ('aligned_copies', opts[1])):
            _check_norm(f'recipe/{tag}', o._norm, d, numels)
            w = _compare(f'recipe/{tag}', o, d, before, clip, e_g)
            assert max(w.values()) <= 1.0, (tag, w)
            _check_steps(o)
    reducer.remove()
