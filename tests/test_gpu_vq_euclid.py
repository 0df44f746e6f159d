"""Euclidean VQ codebooks on the device tokenizer: kernels.vq_nearest_l2 (amdnuwa_vq_nearest_l2) against the float64 judge of
tests/vq_euclid_util.py, and the module paths it opens -- VQGanVAE.get_video_indices with vq_use_cosine_sim=False, NUWA from raw
frames, NUWASketch.forward / generate.  The bound and the `sure` rule are derived in vq_euclid_util.py; test_vq_euclid_cpu.py shows
that the shifted inputs defeat the fp32 expansion around the origin."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import vq_euclid_util as U  # noqa: E402
from guard_util import guard, guarded  # noqa: E402

DEV = 'cuda'


@pytest.fixture(scope='module')
def A():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    import nuwa_pytorch_amd
    return nuwa_pytorch_amd


@pytest.fixture(scope='module')
def K(A):
    from nuwa_pytorch_amd import kernels
    return kernels


def _first_form(fn):
    """fn() with tuning key 15 = 1 (the general kernel for every code_dim), restored afterwards"""
    from nuwa_pytorch_amd import _lib
    L = _lib.lib()
    L.amdnuwa_set_tuning(15, 1)
    try:
        return fn()
    finally:
        L.amdnuwa_set_tuning(15, 0)


# ----- 1. the lookup against float64 -----

@pytest.mark.parametrize('case', U.CASES, ids=U.case_id)
def test_lookup_matches_float64_on_sure_rows(K, case):
    ref = U.judged(case)
    x, cb = ref[0].to(DEV), ref[1].to(DEV)
    idx, dist = K.vq_nearest_l2(x, cb, want_dist=True)
    U.check_lookup(idx, dist, ref, f'vq_nearest_l2[{U.case_id(case)}]')
    assert torch.equal(K.vq_nearest_l2(x, cb), idx)                  # best_dist is optional


# ----- 2. exact ties -----

def _tie_case(Cn, Dc, copies, R, seed):
    g = torch.Generator().manual_seed(seed)
    cb = torch.randn(Cn, Dc, generator=g)
    for c in copies:
        cb[c] = cb[5]
    x = cb[5] + 0.5 * torch.randn(R, Dc, generator=g)
    return x, cb


def test_exact_ties_return_the_lowest_index(K):
    """duplicates of code 5 in another lane of its tile (31), the next tile (32, and 37: the lane of 5 again) and in other slices (700,
    4097, 8191 of the 64 slices of 128 codes): bit-equal scores everywhere, so the strict '>' in scan and combine order must keep 5"""
    x, cb = _tie_case(8192, 256, (31, 32, 37, 700, 4097, 8191), 40, 31)
    idx64, _, _, _ = U.judge64(x, cb)
    assert set(idx64.tolist()) <= {5, 31, 32, 37, 700, 4097, 8191}     # the rows do sit next to the duplicated code
    idx = K.vq_nearest_l2(x.to(DEV), cb.to(DEV)).cpu()
    assert idx.tolist() == [5] * 40, idx.tolist()
    idx1 = _first_form(lambda: K.vq_nearest_l2(x.to(DEV), cb.to(DEV))).cpu()
    assert idx1.tolist() == [5] * 40, idx1.tolist()


def test_exact_ties_general_form(K):
    """70 codes x 32 dims (two code tiles, the second ragged): copies of code 5 in the other 32-column half (37), at the tile's end (63)
    and in the ragged tile (69)"""
    x, cb = _tie_case(70, 32, (37, 63, 69), 40, 32)
    idx64, _, _, _ = U.judge64(x, cb)
    assert set(idx64.tolist()) <= {5, 37, 63, 69}
    idx = K.vq_nearest_l2(x.to(DEV), cb.to(DEV)).cpu()
    assert idx.tolist() == [5] * 40, idx.tolist()


# ----- 3. both forms agree -----

@pytest.mark.parametrize('case', [c for c in U.CASES if c[:3] == (300, 8192, 256)], ids=U.case_id)
def test_sliced_and_general_form_agree(K, case):
    ref = U.judged(case)
    x, cb, tol = ref[0].to(DEV), ref[1].to(DEV), ref[4]
    idx, dist = K.vq_nearest_l2(x, cb, want_dist=True)
    idx1, dist1 = _first_form(lambda: K.vq_nearest_l2(x, cb, want_dist=True))
    err = float(((dist.cpu().double() - dist1.cpu().double()).abs() / tol).max())
    print(f'{U.case_id(case)}: differing ids {int((idx != idx1).sum())}, |best_dist difference| / tol {err:.3e}')
    assert torch.equal(idx, idx1)
    assert err <= 1.0
    U.check_lookup(idx1, dist1, ref, f'vq_nearest_l2[general form, {U.case_id(case)}]')


# ----- 4. determinism -----

@pytest.mark.parametrize('case', [U.CASES[4], U.SHIFTED[3], U.SHIFTED[2]], ids=U.case_id)
def test_two_calls_agree_bit_for_bit(K, case):
    ref = U.judged(case)
    x, cb = ref[0].to(DEV), ref[1].to(DEV)
    idx, dist = K.vq_nearest_l2(x, cb, want_dist=True)
    K.vq_argmax(x, cb)                                                # another user of the shared allocator in between
    idx2, dist2 = K.vq_nearest_l2(x, cb, want_dist=True)
    assert torch.equal(idx, idx2)
    assert torch.equal(dist.view(torch.int32), dist2.view(torch.int32))


# ----- 5. guarded operands -----

@pytest.mark.parametrize('case', U.GUARDED, ids=U.case_id)
def test_operands_and_outputs_in_guarded_buffers(K, case):
    """rows and codebook between NaN bands, outputs and workspace NaN-prefilled with bands of their own: test 1's checks must hold (no
    byte from outside an operand reaches the arithmetic, every output element is written), and every band must come back intact"""
    ref = U.judged(case)
    with guard(K) as g:
        idx, dist = K.vq_nearest_l2(guarded(ref[0], device=DEV), guarded(ref[1], device=DEV), want_dist=True)
        assert g.made() >= 5                                          # two operands, two outputs, the workspace
        assert not bool(torch.isnan(dist).any())
        assert bool(((idx >= 0) & (idx < case[1])).all())
        U.check_lookup(idx, dist, ref, f'guarded vq_nearest_l2[{U.case_id(case)}]')


def test_slices_never_start_behind_the_codebook(K):
    """8256 codes under the cap of 64 slices: 129 codes per slice round up to 160, so only 52 slices start inside the codebook.  Both
    lookups must launch those alone (a slice behind the end would form code addresses past the operand) and still see every code:
    rows next to the LAST codes, operands between NaN bands"""
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(51)
    cb = torch.randn(8256, 256, generator=g)
    pick = torch.cat([torch.arange(8256 - 20, 8256), torch.randint(0, 8256, (20,), generator=g)])
    x = cb[pick] + 0.5 * torch.randn(40, 256, generator=g)
    idx64, gap, tol, d2 = U.judge64(x, cb)
    sim64 = F.normalize(x.double(), dim=-1) @ F.normalize(cb.double(), dim=-1).t()
    top = sim64.topk(2, dim=-1)
    with guard(K) as g_:
        xg, cg = guarded(x, device=DEV), guarded(cb, device=DEV)
        idx, dist = K.vq_nearest_l2(xg, cg, want_dist=True)
        U.check_lookup(idx, dist, (x, cb, idx64, gap > 2 * tol, tol, d2), 'vq_nearest_l2[40x8256x256]')
        cidx, sim = K.vq_argmax(xg, cg, want_sim=True)
        assert g_.made() >= 8
        assert bool((top.values[:, 0] - top.values[:, 1] > 1e-5).all())           # the bound of test_gpu_vae.py::test_vq_argmax
        assert torch.equal(cidx.cpu(), top.indices[:, 0])
        assert float((sim.cpu().double() - top.values[:, 0]).abs().max()) <= 1e-5
    assert idx.cpu()[:20].tolist() == list(range(8256 - 20, 8256))


# ----- 6. the module -----

def _euclid_vae(A, size, dim, seed):
    """a Euclidean VAE on the device whose codebook is a tight cloud around rows the device encoder itself produces"""
    torch.manual_seed(seed)
    vae = A.VQGanVAE(dim=32, image_size=32, num_layers=2, vq_codebook_size=size, vq_codebook_dim=dim, use_vgg_and_gan=False,
                     attn_dim_head=16, attn_heads=4, vq_use_cosine_sim=False).eval().to(DEV)
    return vae


def _encoder_rows(vae, video):
    """the rows the tokenizer looks up, from the device stages (tested on their own) plus project_in, on the CPU"""
    from nuwa_pytorch_amd import kernels as K
    fmap = video.reshape(-1, *video.shape[2:]).float()
    for enc in vae.encoders:
        fmap = vae._hip_module(enc, fmap)
    pin = vae.vq.project_in
    fmap = K.conv2d_fwd(fmap, pin.weight[:, :, None, None], pin.bias, 1, 0)
    return fmap.permute(0, 2, 3, 1).reshape(-1, fmap.shape[1]).cpu()


@pytest.mark.parametrize('size,dim', [(64, 16), (512, 256)])
def test_euclidean_vae_tokenizes_on_the_device(A, monkeypatch, size, dim):
    vae = _euclid_vae(A, size, dim, 41)
    assert not vae.vq.use_cosine_sim
    g = torch.Generator().manual_seed(42)
    video = torch.rand(2, 3, 3, 32, 32, generator=g).to(DEV)
    rows = _encoder_rows(vae, video)
    pick = torch.randint(0, rows.shape[0], (size,), generator=g)
    with torch.no_grad():
        vae.vq._codebook.embed.copy_((rows[pick] + 0.05 * torch.randn(size, dim, generator=g)).to(DEV))
    monkeypatch.setenv('AMDNUWA_TOKENIZER_CHUNK', '0')
    ids = vae.get_video_indices(video)
    assert ids.shape == (2, 3, 8, 8) and ids.dtype == torch.int64
    idx64, gap, tol, _ = U.judge64(rows, vae.vq.embed)
    sure = gap > 2 * tol
    share = float(sure.double().mean())
    wrong = int((ids.reshape(-1).cpu()[sure] != idx64[sure]).sum())
    print(f'euclidean vae {size} x {dim}: sure share {share:.4f}, wrong on sure rows {wrong}, codebook mean norm {float(vae.vq.embed.mean(0).norm()):.3f}')
    assert share >= 0.99
    assert wrong == 0
    monkeypatch.setenv('AMDNUWA_TOKENIZER_CHUNK', '4')
    assert torch.equal(vae.get_video_indices(video), ids)


# ----- 7. end to end -----

def test_nuwa_trains_from_raw_frames_with_a_euclidean_vae(A):
    torch.manual_seed(7)
    vae = A.VQGanVAE(dim=32, image_size=16, num_layers=2, vq_codebook_size=64, vq_codebook_dim=32, use_vgg_and_gan=False,
                     vq_use_cosine_sim=False)
    nuwa = A.NUWA(vae=vae, dim=32, text_num_tokens=50, text_max_seq_len=8, max_video_frames=3, text_enc_depth=2,
                  dec_depth=3, enc_reversible=True, dec_reversible=False, dec_heads=2, dec_dim_head=32,
                  text_enc_heads=2, text_enc_dim_head=16, sparse_3dna_kernel_size=3, sparse_3dna_dilation=(1, 2)).to(DEV).train()
    g = torch.Generator().manual_seed(8)
    text = torch.randint(1, 50, (2, 8), generator=g).to(DEV)
    frames = torch.rand(2, 3, 3, 16, 16, generator=g).to(DEV)
    loss = nuwa(text=text, video=frames, return_loss=True, cond_dropout_prob=0.)
    ids = nuwa.vae.get_video_indices(frames)
    assert ids.dtype == torch.int64 and int(ids.min()) >= 0 and int(ids.max()) < 64
    loss_ids = nuwa(text=text, video=ids, return_loss=True, cond_dropout_prob=0.)
    assert bool(torch.isfinite(loss).all())
    assert torch.equal(loss, loss_ids), (float(loss), float(loss_ids))


def test_sketch_forward_and_generate_with_a_euclidean_sketch_vae(A):
    from test_gpu_modules import SKETCH_KW
    torch.manual_seed(5)
    vae = A.VQGanVAE(dim=32, image_size=16, num_layers=2, vq_codebook_size=64, vq_codebook_dim=32, use_vgg_and_gan=False)
    sketch_vae = A.VQGanVAE(dim=32, image_size=16, num_layers=2, vq_codebook_size=48, vq_codebook_dim=32, use_vgg_and_gan=False,
                            vq_use_cosine_sim=False)
    m = A.NUWASketch(vae=vae, sketch_vae=sketch_vae, **SKETCH_KW).to(DEV).train()
    g = torch.Generator().manual_seed(1)
    sketch = torch.rand(1, 2, 3, 16, 16, generator=g).to(DEV)
    video = torch.rand(1, 3, 3, 16, 16, generator=g).to(DEV)
    loss = m(sketch=sketch, video=video, return_loss=True, cond_dropout_prob=0.)
    assert bool(torch.isfinite(loss).all())
    m.eval()
    A.set_precision('bf16x3')
    try:
        torch.manual_seed(9)
        a = m.generate(sketch=sketch, filter_thres=0.9, num_frames=1, cond_scale=2.)
        torch.manual_seed(9)
        b = m.generate(sketch=sketch, filter_thres=0.9, num_frames=1, cond_scale=2.)
    finally:
        A.set_precision('bf16')
    assert a.shape == (1, 1, 3, 16, 16) and bool(torch.isfinite(a).all()) and torch.equal(a, b)
