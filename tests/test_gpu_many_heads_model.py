"""Sparse3DNA with 9 .. 16 heads at module and model level on the MI355X, with Sparse3DNA.many_heads switched on: the bare module (12 heads;
16 heads with the relative-position bias) and a tiny NUWA with dec_heads = 12 in the plain and the reversible decoder (depth 2, shifted
tokens), forward and gradients against the float32 oracle on the model's own state dict, within the bounds the existing 8-head module tests
(tests/test_gpu_modules.py: MODES) and full-model parity tests (gradients at twice the mode's bound) use; generate() on the recompute loop;
and the same model with the switch off still raises."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from gpu_util import report  # noqa: E402
from test_gpu_modules import MODES  # noqa: E402

DEV = 'cuda'
SHAPE = (2, 4, 4)


@pytest.fixture(scope='module')
def A():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import nuwa_pytorch_amd
    return nuwa_pytorch_amd


@pytest.fixture(scope='module')
def O_mod():
    from oracle import nuwa_oracle
    return nuwa_oracle


@pytest.fixture
def many(A, monkeypatch):
    monkeypatch.setattr(A.Sparse3DNA, 'many_heads', True)


def _state(m):
    return {k: v.detach().cpu().clone().requires_grad_(v.is_floating_point()) for k, v in m.state_dict().items()}


@pytest.mark.parametrize('mode,tol,gtol', MODES)
@pytest.mark.parametrize('heads,rel', [(12, False), (16, True)])
def test_bare_module_against_the_oracle(A, O_mod, many, heads, rel, mode, tol, gtol):
    torch.manual_seed(0)
    dim, n = 64, 1 + SHAPE[0] * SHAPE[1] * SHAPE[2]
    m = A.Sparse3DNA(dim=dim, heads=heads, dim_head=32, video_shape=SHAPE, causal=True, rel_pos_bias=rel)
    P = _state(m)
    g = torch.Generator().manual_seed(heads)
    x, dy = torch.randn(2, n, dim, generator=g), torch.randn(2, n, dim, generator=g)
    xr = x.clone().requires_grad_(True)
    yr = O_mod.sparse3dna(xr, P, SHAPE, 3, 1, heads, causal=True)
    yr.backward(dy)
    m = m.to(DEV)
    A.set_precision(mode)
    try:
        xd = x.to(DEV).requires_grad_(True)
        y = m(xd)
        tag = f'mh_module[{heads},{mode}]'
        report(tag + '.y', y, yr.detach(), tol)
        y.backward(dy.to(DEV))
        report(tag + '.dx', xd.grad, xr.grad, gtol)
        n_checked = 0
        for k, p in m.named_parameters():
            assert p.grad is not None and P[k].grad is not None, k
            report(tag + f'.grad.{k}', p.grad, P[k].grad, gtol)
            n_checked += 1
        assert n_checked >= (8 if rel else 5)
    finally:
        A.set_precision('bf16')


def _tiny_nuwa(A, reversible, heads=12):
    vae = A.VQGanVAE(dim=32, image_size=16, num_layers=2, vq_codebook_size=64, vq_codebook_dim=32, use_vgg_and_gan=False)
    return A.NUWA(vae=vae, dim=64, text_num_tokens=50, text_max_seq_len=8, max_video_frames=SHAPE[0], text_enc_depth=1,
                  dec_depth=2, enc_reversible=True, dec_reversible=reversible, dec_heads=heads, dec_dim_head=32,
                  text_enc_heads=2, text_enc_dim_head=16, sparse_3dna_kernel_size=3, sparse_3dna_dilation=1)


def _cfg(reversible, heads=12):
    return dict(video_shape=SHAPE, kernel_size=3, dilations=(1,), heads=heads, depth=2, shift=True, text_depth=1, text_heads=2, reversible=reversible)


def _inputs():
    g = torch.Generator().manual_seed(11)
    text = torch.randint(1, 50, (2, 8), generator=g)
    text[1, 6:] = 0                                          # a padded text row
    ids = torch.randint(0, 64, (2, SHAPE[0] * SHAPE[1] * SHAPE[2]), generator=g)
    return text, ids


@pytest.mark.parametrize('mode,tol,gtol', MODES)
@pytest.mark.parametrize('reversible', [False, True], ids=['plain', 'reversible'])
def test_tiny_nuwa_with_twelve_heads_against_the_oracle(A, O_mod, many, reversible, mode, tol, gtol):
    torch.manual_seed(3)
    nuwa = _tiny_nuwa(A, reversible)
    P = _state(nuwa)
    text, ids = _inputs()
    cfg = _cfg(reversible)
    ctx, mask = O_mod.text_encoder(text, P, cfg)
    loss_ref = O_mod.decoder_loss(P, cfg, ids, ctx, mask)
    loss_ref.backward()
    nuwa = nuwa.to(DEV).train()
    A.set_precision(mode)
    try:
        loss = nuwa(text=text.to(DEV), video=ids.to(DEV), return_loss=True, cond_dropout_prob=0.)
        tag = f'mh_nuwa[{"rev" if reversible else "plain"},{mode}]'
        report(tag + '.loss', loss.reshape(1), loss_ref.detach().reshape(1), tol)
        loss.backward()
        named = dict(nuwa.named_parameters())
        layer = [k for k in named if k.startswith('video_transformer.layers.0.') and '.net.blocks.' not in k]
        assert len(layer) >= 10 and any('talking_heads' in k for k in layer), layer
        for k in layer:
            assert named[k].grad is not None and P[k].grad is not None, k
            report(tag + f'.grad.{k}', named[k].grad, P[k].grad, gtol * 2)
    finally:
        A.set_precision('bf16')


@pytest.mark.parametrize('reversible', [False, True], ids=['plain', 'reversible'])
def test_generate_runs_the_recompute_loop(A, many, reversible):
    torch.manual_seed(4)
    nuwa = _tiny_nuwa(A, reversible, heads=16).to(DEV).eval()
    text, _ = _inputs()
    frames = nuwa.generate(text=text.to(DEV), num_frames=1, filter_thres=0.9, cond_scale=2.)
    ids = nuwa.last_generated_ids
    assert ids.shape == (2, SHAPE[1] * SHAPE[2]) and ids.dtype == torch.long
    assert int(ids.min()) >= 0 and int(ids.max()) < 64
    assert frames.shape == (2, 1, 3, 16, 16) and bool(torch.isfinite(frames).all())


def test_one_training_step_with_sixteen_heads(A, many):
    torch.manual_seed(6)
    nuwa = _tiny_nuwa(A, False, heads=16).to(DEV).train()
    text, ids = _inputs()
    opt = torch.optim.SGD(nuwa.parameters(), lr=1e-2)
    loss = nuwa(text=text.to(DEV), video=ids.to(DEV), return_loss=True, cond_dropout_prob=0.)
    loss.backward()
    w = [p for k, p in nuwa.named_parameters() if k.startswith('video_transformer.layers.0.') and k.endswith('talking_heads.weight')][0]
    assert tuple(w.shape[:2]) == (16, 16) and bool(torch.isfinite(loss))
    assert all(p.grad is None or bool(torch.isfinite(p.grad).all()) for p in nuwa.parameters())
    opt.step()
    loss2 = nuwa(text=text.to(DEV), video=ids.to(DEV), return_loss=True, cond_dropout_prob=0.)
    assert bool(torch.isfinite(loss2)) and float(loss2.detach()) != float(loss.detach())
    assert w.grad is not None and float(w.grad.abs().max()) > 0


def test_switch_off_still_raises(A):
    assert A.Sparse3DNA.many_heads is False
    nuwa = _tiny_nuwa(A, False).to(DEV).train()
    text, ids = _inputs()
    with pytest.raises(NotImplementedError, match='12 heads.*up to 8 heads'):
        nuwa(text=text.to(DEV), video=ids.to(DEV), return_loss=True, cond_dropout_prob=0.)
