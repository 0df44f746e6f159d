"""VQGanAttention on feature maps past the LDS-resident kernels (18 x 18 and wider at 8 x 64): the query-tiled, key-streaming f32 MFMA
core (vqattn_tiled_kernel) with both bias sources -- [heads, P, P] from memory and the relative-offset table [heads, 2S-1, 2S-1] in
LDS -- against float64 on the CPU, against the resident kernels on shapes all of them take, and through the block, the tokenizer,
the decoder and NUWA.generate on a 20 x 20 map.

Bound of every fp32 feature map: 2e-5 max-abs over max-ref (test_gpu_vae.py's figure; the CPU's own fp32 evaluation of the same
recipe sits at 0.7 ... 1.4e-6 from float64), reconstructions 5e-5 (g7.recon).  The softmax is kept from being flat
(vae_wide_util.sharp_scale, last CPB layer times 4): the reference must show a mean row maximum of >= 10 / P."""
import copy
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from golden_util import fill_params, load  # noqa: E402
from gpu_util import report  # noqa: E402
from vae_wide_util import core_ref64, gather_table, sharp_scale, sharpen_attention  # noqa: E402

DEV = 'cuda'
TOL = 2e-5
VAE20_KW = dict(dim=32, image_size=80, num_layers=2, vq_codebook_size=64, vq_codebook_dim=32, use_vgg_and_gan=False)


@pytest.fixture(scope='module')
def K():
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    from nuwa_pytorch_amd import kernels
    return kernels


@pytest.fixture(scope='module')
def L():
    from nuwa_pytorch_amd import _lib
    return _lib.lib()


class tuning15:
    def __init__(self, L, v):
        self.L, self.v = L, v

    def __enter__(self):
        self.L.amdnuwa_set_tuning(15, self.v)

    def __exit__(self, *a):
        self.L.amdnuwa_set_tuning(15, 0)


def _qkv(N, heads, c, P, gen):
    qkv = torch.randn(N, 3, heads, c, P, generator=gen)
    qkv[:, :2] = F.normalize(qkv[:, :2], dim=-1)              # q and k over the SPATIAL axis (quirk Q9)
    return qkv.reshape(N, 3 * heads * c, P).contiguous()


_CASES = {}


def _case(N, heads, c, S):
    """inputs and the float64 reference of one core shape: computed once, shared by both bias forms, never modified"""
    key = (N, heads, c, S)
    if key not in _CASES:
        from nuwa_pytorch_amd.vqgan_vae import ContinuousPositionBias
        P = S * S
        gen = torch.Generator().manual_seed(100 * S + c)
        torch.manual_seed(S)
        cpb = ContinuousPositionBias(dim=32, heads=heads)
        with torch.no_grad():
            cpb.net[-1].weight.mul_(4)
            table = cpb.table(S)
        bias = gather_table(table, S).contiguous()
        qkv, scale = _qkv(N, heads, c, P, gen), sharp_scale(heads, P, c, gen)
        ref, attn = core_ref64(qkv, bias, scale, heads)
        rowmax = float(attn.amax(dim=-1).mean())
        uniform = qkv.reshape(N, 3, heads * c, P)[:, 2].double().mean(dim=-1, keepdim=True)
        print(f'vqattn case {key}: mean row-max {rowmax * P:.1f}/P, |ref - uniform| / |ref| = {float((ref - uniform).norm() / ref.norm()):.3f}')
        assert rowmax >= 10 / P, f'reference softmax too flat to show key-indexing errors: mean row-max {rowmax * P:.2f}/P'
        _CASES[key] = (qkv, bias, table.contiguous(), scale, ref)
    return _CASES[key]


CORE_SHAPES = [(2, 2, 64, 18),      # the first refused size: ragged in queries and keys
               (2, 8, 64, 20), (2, 3, 40, 23), (1, 2, 33, 19),
               (2, 2, 64, 32),      # exact tiles, several key tiles
               (1, 4, 16, 32), (1, 1, 64, 48),
               (1, 1, 64, 64)]      # the far corner of the table form


@pytest.mark.parametrize('form', ['bias', 'table'])
@pytest.mark.parametrize('N,heads,c,S', CORE_SHAPES)
def test_tiled_core_against_float64(K, L, N, heads, c, S, form):
    """(the bias form with tuning key 15 = 2: at dim_head 33 and 16 these maps still fit the resident VALU kernel, which is not the
    kernel under test; the table form always runs the tiled kernel)"""
    qkv, bias, table, scale, ref = _case(N, heads, c, S)
    if form == 'bias':
        with tuning15(L, 2):
            out = K.vqattn_core(qkv.to(DEV), scale.to(DEV), heads, bias=bias.to(DEV))
    else:
        out = K.vqattn_core(qkv.to(DEV), scale.to(DEV), heads, rel_table=table.to(DEV))
    report(f'vqattn_tiled[{form},N{N},h{heads},c{c},S{S}]', out, ref, TOL)


@pytest.mark.parametrize('N,heads,c,S', [(1, 1, 1, 1), (2, 2, 7, 2), (1, 3, 64, 5), (3, 2, 31, 9)])
def test_tiled_core_on_tiny_maps(K, L, N, heads, c, S):
    """one position, fewer keys than a tile, fewer queries than a wave, a single channel: everything padding (no row-maximum
    precondition: with P keys the maximum cannot be 10 / P)"""
    P = S * S
    gen = torch.Generator().manual_seed(S)
    qkv, scale = _qkv(N, heads, c, P, gen), sharp_scale(heads, P, c, gen)
    table = torch.randn(heads, 2 * S - 1, 2 * S - 1, generator=gen)
    bias = gather_table(table, S).contiguous()
    ref, _ = core_ref64(qkv, bias, scale, heads)
    with tuning15(L, 2):
        out = K.vqattn_core(qkv.to(DEV), scale.to(DEV), heads, bias=bias.to(DEV))
    report(f'vqattn_tiled[bias,tiny,c{c},S{S}]', out, ref, TOL)
    report(f'vqattn_tiled[table,tiny,c{c},S{S}]', K.vqattn_core(qkv.to(DEV), scale.to(DEV), heads, rel_table=table.to(DEV)), ref, TOL)


def test_running_maximum_moves_at_every_key_tile(K):
    """bias rising with the key index: the running maximum changes at every key tile and everything accumulated so far is rescaled;
    falling: the first tile holds it and every later tile is small against it"""
    N, heads, c, S = 1, 2, 64, 32
    P = S * S
    gen = torch.Generator().manual_seed(7)
    qkv, scale = _qkv(N, heads, c, P, gen), sharp_scale(heads, P, c, gen)
    ramp = (20.0 * torch.arange(P, dtype=torch.float32) / P)[None, :].expand(P, P)
    bias = torch.stack([ramp, -ramp]).contiguous()
    ref, _ = core_ref64(qkv, bias, scale, heads)
    out = K.vqattn_core(qkv.to(DEV), scale.to(DEV), heads, bias=bias.to(DEV))
    hc = heads * c // 2
    report('vqattn_tiled[bias +20 j/P]', out[:, :hc], ref[:, :hc], TOL)
    report('vqattn_tiled[bias -20 j/P]', out[:, hc:], ref[:, hc:], TOL)


@pytest.mark.parametrize('S', [16, 17])
def test_tiled_core_against_the_resident_kernels(K, L, S):
    """P = 256 (vqattn_mfma_kernel) and P = 289 (the VALU kernel) at dim_head 64: tuning key 15 = 2 sends them to the tiled kernel.
    Without it they launch what they launched before: the same bits call after call, and at P = 289 the bits of the forced VALU form"""
    N, heads, c = 2, 4, 64
    qkv, bias, table, scale, ref = _case(N, heads, c, S)
    a = (qkv.to(DEV), scale.to(DEV), heads)
    y0 = K.vqattn_core(*a, bias=bias.to(DEV))
    y0b = K.vqattn_core(*a, bias=bias.to(DEV))
    with tuning15(L, 1):
        y1 = K.vqattn_core(*a, bias=bias.to(DEV))
    with tuning15(L, 2):
        y2 = K.vqattn_core(*a, bias=bias.to(DEV))
    y2t = K.vqattn_core(*a, rel_table=table.to(DEV))
    assert torch.equal(y0, y0b)
    if S == 17:
        assert torch.equal(y0, y1)                       # the VALU kernel either way
    else:
        assert not torch.equal(y0, y1)                   # MFMA against VALU: another summation order
        report('vqattn[mfma vs valu]', y0, y1.cpu(), TOL)
    assert not torch.equal(y0, y2), 'tuning key 15 = 2 did not change the kernel'
    report(f'vqattn[tiled vs resident,S{S}]', y2, y0.cpu(), TOL)
    report(f'vqattn[tiled table vs resident,S{S}]', y2t, y0.cpu(), TOL)
    report(f'vqattn[resident vs f64,S{S}]', y0, ref, TOL)
    report(f'vqattn[tiled vs f64,S{S}]', y2, ref, TOL)


def test_tiled_core_is_reproducible_and_independent_of_the_batch(K):
    heads = 8
    qkv, bias, table, scale, _ = _case(2, heads, 64, 20)
    gen = torch.Generator().manual_seed(11)
    q3 = torch.cat([qkv, _qkv(1, heads, 64, 400, gen)]).to(DEV)
    for kw in (dict(bias=bias.to(DEV)), dict(rel_table=table.to(DEV))):
        y = K.vqattn_core(qkv.to(DEV), scale.to(DEV), heads, **kw)
        assert torch.equal(y, K.vqattn_core(qkv.to(DEV), scale.to(DEV), heads, **kw))
        y3 = K.vqattn_core(q3, scale.to(DEV), heads, **kw)
        y1 = K.vqattn_core(q3[:1].contiguous(), scale.to(DEV), heads, **kw)
        assert torch.equal(y3[:1], y1) and torch.equal(y3[:2], y)


@pytest.mark.parametrize('S', [20, 32])
def test_attention_block_on_wide_maps(S):
    """VQGanVAE._hip_module(VQGanAttention) -- 1x1 conv, l2norm, core with the offset table, 1x1 conv, LayerNormChan + residual --
    against the torch module on the CPU"""
    import nuwa_pytorch_amd as A
    from nuwa_pytorch_amd.vqgan_vae import VQGanAttention
    torch.manual_seed(S)
    m = VQGanAttention(dim=128, dim_head=64, heads=8).eval()
    sharpen_attention(m, S * S, seed=S, cpb_gain=4.)
    with torch.no_grad():
        m.post_norm.g.mul_(torch.rand_like(m.post_norm.g) + 0.5)
        x = torch.randn(2, 128, S, S)
        ref = m(x)
        vae = A.VQGanVAE(dim=32, image_size=32, num_layers=2, vq_codebook_size=64, vq_codebook_dim=16, use_vgg_and_gan=False)
        y = vae._hip_module(copy.deepcopy(m).to(DEV), x.to(DEV))
    report(f'vqgan_attention[wide,S{S}]', y, ref, TOL)


@pytest.fixture(scope='module')
def vae20():
    import nuwa_pytorch_amd as A
    torch.manual_seed(0)
    vae = A.VQGanVAE(**VAE20_KW).eval()
    return sharpen_attention(vae, 400, seed=3)


def test_tokenizer_on_a_20x20_map_matches_oracle(vae20, monkeypatch):
    """the conditions of test_cfg3_vae_tokenizer_matches_oracle; the parent's library refuses the shape"""
    from oracle import nuwa_oracle as O
    torch.manual_seed(1)
    video = torch.rand(2, 2, 3, 80, 80)
    P = {k: v.detach() for k, v in vae20.state_dict().items()}
    fm = O.vae_encode_fmap(video.reshape(4, 3, 80, 80), P, num_layers=2, heads=8)
    idx_ref, gap = (t.reshape(-1) for t in O.vq_eval_lookup(fm, P['vq._codebook.embed'], P.get('vq.project_in.weight'), P.get('vq.project_in.bias')))
    dvae = copy.deepcopy(vae20).to(DEV)
    monkeypatch.setenv('AMDNUWA_TOKENIZER_CHUNK', '0')
    whole = dvae.get_video_indices(video.to(DEV))
    assert whole.shape == (2, 2, 20, 20)
    idx = whole.reshape(-1).cpu()
    sure = gap > 1e-5
    assert float(sure.float().mean()) > 0.98
    assert torch.equal(idx[sure], idx_ref[sure])
    for chunk in ('1', '3'):
        monkeypatch.setenv('AMDNUWA_TOKENIZER_CHUNK', chunk)
        assert torch.equal(dvae.get_video_indices(video.to(DEV)), whole), chunk


def test_decoder_on_a_20x20_map(vae20):
    torch.manual_seed(2)
    ids = torch.randint(0, 64, (1, 2 * 400))
    ref = vae20.codebook_indices_to_video(ids)                           # CPU: vae.decode
    got = copy.deepcopy(vae20).to(DEV).codebook_indices_to_video(ids.to(DEV))
    assert got.shape == (1, 2, 3, 80, 80)
    report('vae20.decode', got, ref, 5e-5)


def test_g17_wide_vae_against_reference_fixture():
    """the reference's VQGanVAE (8 x 64 attention) on one 80 x 80 frame: tests/golden/make_golden_vae_wide.py"""
    import nuwa_pytorch_amd as A
    Ar, _, _ = load('g17_vae_wide')
    seed = int(Ar['param_seed'])
    vae = A.VQGanVAE(**VAE20_KW).eval()
    fill_params(vae, seed=seed)
    sharpen_attention(vae, 400, seed=seed)
    vae = vae.to(DEV)
    with torch.no_grad():
        fm = Ar['img'].to(DEV)
        for enc in vae.encoders:
            fm = vae._hip_module(enc, fm)
        report('g17.fmap', fm, Ar['fmap'], TOL)
        idx = vae.get_video_indices(Ar['img'].to(DEV)[None])[0].cpu()
        sure = Ar['top2_gap'].reshape(idx.shape) > 1e-5
        assert bool(sure.all()), 'fixture has near-ties'
        assert torch.equal(idx, Ar['indices'].reshape(idx.shape))
        ind = Ar['indices'].to(DEV)
        quant = vae.vq.project_out(vae.vq.embed[ind]).permute(0, 3, 1, 2).contiguous()
        report('g17.recon', vae._hip_decode(quant), Ar['recon'], 5e-5)


def test_nuwa_generate_and_raw_frames_on_a_20x20_map():
    """NUWA.generate returns frames (the parent raises: its library refuses the VAE's attention shape), and forward() takes raw frames"""
    import nuwa_pytorch_amd as A
    from test_gpu_wide_grid import _nuwa20
    nuwa = _nuwa20(A)
    sharpen_attention(nuwa.vae, 400, seed=5)
    cpu_vae = copy.deepcopy(nuwa.vae).eval()
    nuwa = nuwa.to(DEV).eval()
    g = torch.Generator().manual_seed(1)
    text = torch.randint(1, 50, (2, 8), generator=g).to(DEV)
    with torch.no_grad():
        frames = nuwa.generate(text=text, num_frames=1, cond_scale=2.)
    assert frames.shape == (2, 1, 3, 80, 80) and bool(torch.isfinite(frames).all())
    ids = nuwa.last_generated_ids
    assert ids.shape == (2, 400)
    report('nuwa20.generate frames', frames, cpu_vae.codebook_indices_to_video(ids.cpu()), 5e-5)
    video = torch.rand(2, 2, 3, 80, 80, generator=g).to(DEV)
    with torch.no_grad():
        tok = nuwa.vae.get_video_indices(video)
        a = nuwa(text=text, video=video, return_loss=True, cond_dropout_prob=0.)
        b = nuwa(text=text, video=tok, return_loss=True, cond_dropout_prob=0.)
    assert bool(torch.isfinite(a)) and torch.equal(a, b), (float(a), float(b))
