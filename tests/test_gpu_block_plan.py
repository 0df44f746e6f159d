"""Which cross-attention kernel generation does a shape reach?  The block's plan (ops.XInner.plan) names the forward core, the packed images
and the backward; a decoder stack runs forward and backward with the kernels.py wrappers of the cross attention recorded, and the wrappers
seen must be exactly those the plan names -- and the plan the one pinned here (rows of tests/test_block_plan_cpu.py)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
# what each route launches (kernels.py wrappers)
CORE = {'x6_f16_only': {'xattn6_pack', 'xattn6_fwd'}, 'x6_f16': {'xattn6_pack', 'xattn6_fwd'}, 'x6_bf16': {'xattn6_pack', 'xattn6_fwd'},
        'x2_f16': {'xattn2_fwd_f16'}, 'x2_bf16': {'xattn2_fwd'}, 'x1_stats': {'xattn_fwd'}, 'x1_p': {'xattn_fwd'}}
PACK = {'x6b16': {'xattn6_pack_bwd'}, 'x6b': {'xattn6_pack_bwd'}, 'x1': {'xattn_pack'}}
BWD = {'x6_16': {'xattn6_bwd16', 'xattn_kv_grads16', 'xattn_unpack'}, 'x6': {'xattn6_bwd', 'xattn_kv_grads', 'xattn_unpack'},
       'x2': {'xattn2_bwd', 'xattn_kv_grads', 'xattn_unpack'}, 'x2_rc': {'xattn2_bwd_rc', 'xattn_unpack'},
       'x1': {'xattn_bwd', 'xattn_kv_grads', 'xattn_unpack'}}
WRAPPERS = set().union(*CORE.values(), *PACK.values(), *BWD.values())
# (context length, precision mode, switch) -> (core, pack, bwd)
PINNED = {
    (128, 'bf16x3-fwd', None): ('x6_f16_only', 'x6b16', 'x6_16'),
    (128, 'bf16x3-fwd', 'xattn6'): ('x2_f16', 'x1', 'x2'),
    (128, 'bf16x3-fwd', 'xattn_rc'): ('x6_f16', 'x1', 'x2_rc'),
    (128, 'bf16', None): ('x6_bf16', 'x6b', 'x6'),
    (64, 'bf16x3-fwd', None): ('x6_f16', 'x1', 'x2'),
    (64, 'bf16x3-fwd', 'xattn6'): ('x2_f16', 'x1', 'x2'),
    (64, 'bf16x3-fwd', 'xattn_rc'): ('x6_f16', 'x1', 'x2_rc'),
    (64, 'bf16', None): ('x6_bf16', 'x1', 'x2'),
}


@pytest.fixture(scope='module')
def stack():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import nuwa_pytorch_amd.nuwa_pytorch as M
    torch.manual_seed(0)
    return M.Transformer(dim=512, depth=2, causal=True, heads=8, dim_head=64, cross_attend=True, sparse_3dna_attn=True,
                         sparse_3dna_video_shape=(2, 16, 16), sparse_3dna_kernel_size=(3, 3, 3), sparse_3dna_dilations=(1, 2),
                         shift_video_tokens=True).to(DEV).train()


@pytest.mark.parametrize('T,mode,switch', sorted(PINNED, key=str))
def test_cross_attention_runs_the_generation_its_plan_names(stack, monkeypatch, T, mode, switch):
    from nuwa_pytorch_amd import kernels as K, ops
    seen, plans = [], []
    for name in WRAPPERS:
        monkeypatch.setattr(K, name, (lambda n, f: lambda *a, **k: (seen.append(n), f(*a, **k))[1])(name, getattr(K, name)))
    fwd = ops.XInner.fwd
    monkeypatch.setattr(ops.XInner, 'fwd', staticmethod(lambda h, p, meta: (plans.append(meta['plan']), fwd(h, p, meta))[1]))
    g = torch.Generator().manual_seed(1)
    x = torch.randn(1, 512, 512, generator=g).to(DEV).requires_grad_(True)
    ctx = torch.randn(1, T, 512, generator=g).to(DEV).requires_grad_(True)
    mask = (torch.rand(1, T, generator=g) > 0.25).to(DEV)
    was, x6 = K.get_precision(), K.xattn6_on()
    rc = K.xattn2_bwd_rc_ok(K.x_geom(1, 512, 128, 8, 64))        # (the switch as found: a geometry the recomputing kernel takes)
    try:
        K.set_precision(mode)
        K.set_xattn6(switch != 'xattn6')
        K.set_xattn_rc(switch == 'xattn_rc')
        stack.zero_grad(set_to_none=True)
        out = stack(x, context=ctx, context_mask=mask)
        forward, seen[:] = set(seen), []
        out.square().mean().backward()
        torch.cuda.synchronize()
        backward = set(seen)
    finally:
        K.set_precision(was)
        K.set_xattn6(x6)
        K.set_xattn_rc(rc)
    plan = plans[0]._replace(guarded=())            # (the two layers guard their own weights: everything else agrees)
    assert len(plans) == 2 and plans[1]._replace(guarded=()) == plan, plans
    assert (plan.core, plan.pack, plan.bwd) == PINNED[(T, mode, switch)]
    assert forward == CORE[plan.core] | PACK[plan.pack], f'forward ran {sorted(forward)}, the plan names {plan.core} + {plan.pack}'
    assert backward == BWD[plan.bwd], f'backward ran {sorted(backward)}, the plan names {plan.bwd}'
    assert bool(torch.isfinite(x.grad).all()) and bool(torch.isfinite(ctx.grad).all())
