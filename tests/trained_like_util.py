"""Trained-like weights for the full-model fixtures, and the plumbing between a fixture, the oracle and a product model.

Every whole-model fixture (tests/golden/make_golden.py) holds the state dict of a freshly constructed reference model: each
LayerNorm gain is exactly 1, each LayerNorm bias and (almost) every other bias exactly 0.  Vectors that are all equal can be swapped
-- pre-norm for post-norm, this block for the next, video stream for audio stream -- without the forward noticing.  trained_like()
gives every such vector its own values; test_weight_updates_cpu.py proves, from the oracle alone, that each of them then moves
the logits, and test_gpu_weight_updates.py compares the product with the oracle on those weights.

The constructors and oracle configurations are the ones that sit beside the fixtures in test_gpu_modules.py and
test_oracle_golden.py (imported, not copied)."""
import functools
import math

import torch

from golden_util import load
from test_gpu_modules import SKETCH_KW, VA_KW, _tiny_nuwa
from test_oracle_golden import NUWA_CFG, SKETCH_CFG, VA_CFG

GAIN_SPAN = (0.5, 2.0)       # log-uniform LayerNorm / StableLayerNorm gains
BIAS_AMP = 0.3               # bias = fixture value + BIAS_AMP * N(0, 1)

# fixture name -> model family, and the (seed, bias amplitude) of its trained-like weights: chosen so that the least visible vector of every
# model moves the oracle's logits by more than the 5e-3 test_weight_updates_cpu.py asks for (figures, and why g9a draws with seed 2, there).
MODELS = {
    'g5_nuwa_tiny': dict(kind='nuwa', seed=5, bias_amp=BIAS_AMP),
    'g6_nuwa_tiny_reversible': dict(kind='nuwa', seed=5, bias_amp=BIAS_AMP),
    'g9a_video_audio': dict(kind='va', seed=2, bias_amp=BIAS_AMP),
    'g9c_video_audio_reversible': dict(kind='va', seed=5, bias_amp=BIAS_AMP),
    'g11a_sketch': dict(kind='sketch', seed=5, bias_amp=BIAS_AMP),
}
SHORT = {'g5': 'g5_nuwa_tiny', 'g6': 'g6_nuwa_tiny_reversible', 'g9a': 'g9a_video_audio', 'g9c': 'g9c_video_audio_reversible',
         'g11a': 'g11a_sketch'}


def is_vector(k, v):
    """the state-dict entries trained_like() perturbs: 1-D `*.weight` (norm gains) and every `*.bias`"""
    return (k.endswith('.weight') and v.dim() == 1) or k.endswith('.bias')


def kept(k):
    """the key filter of test_gpu_modules.py / test_oracle_golden.py: no tokenizer, no second registration of a reversible stack's blocks"""
    return not k.startswith(('vae.', 'sketch_vae.')) and '.net.blocks.' not in k


def trained_like(P, seed, gain_span=GAIN_SPAN, bias_amp=BIAS_AMP):
    """a perturbed copy of the fixture state dict P: every 1-D `*.weight` drawn log-uniformly from gain_span, every `*.bias` its value
    + bias_amp * N(0, 1), everything else untouched (cloned).  One seeded CPU generator, keys walked in sorted order."""
    g = torch.Generator().manual_seed(seed)
    lo, hi = math.log(gain_span[0]), math.log(gain_span[1])
    out = {k: v.clone() for k, v in P.items()}
    for k in sorted(P):
        v = P[k]
        if not kept(k) or not is_vector(k, v):
            continue
        if k.endswith('.weight'):
            out[k] = torch.exp(lo + (hi - lo) * torch.rand(v.shape, generator=g)).to(v.dtype)
        else:
            out[k] = v + bias_amp * torch.randn(v.shape, generator=g).to(v.dtype)
    return out


def vector_keys(P):
    return [k for k in sorted(P) if kept(k) and is_vector(k, P[k])]


@functools.lru_cache(maxsize=None)
def fixture(name):
    """(arrays, fixture state dict, trained-like state dict) of a fixture; loaded once and shared -- callers leave them unchanged"""
    Ar, P, _ = load(name)
    spec = MODELS[name]
    return Ar, P, trained_like(P, spec['seed'], bias_amp=spec['bias_amp'])


# ------------------------------------------------------------------------------------------------------------------------------
# the oracle on a state dict
# ------------------------------------------------------------------------------------------------------------------------------

def oracle_cfg(name, Ar):
    kind = MODELS[name]['kind']
    rev = bool(Ar['reversible']) if 'reversible' in Ar else False
    if kind == 'nuwa':
        return dict(NUWA_CFG, reversible=rev)
    if kind == 'va':
        return dict(VA_CFG, reversible=rev)
    return dict(SKETCH_CFG, enc_reversible=rev, dec_reversible=rev, enc_3dna=rev)


def oracle_forward(name, Ar, P):
    """(loss, [logits tensors]) of the fp32 oracle in training mode on the fixture's own inputs: NUWA and NUWASketch give one logits
    tensor (sketch_loss exposes them), NUWAVideoAudio the video and the audio logits"""
    from oracle import nuwa_oracle as O
    kind, cfg = MODELS[name]['kind'], oracle_cfg(name, Ar)
    b = Ar['video_ids'].shape[0]
    if kind == 'sketch':
        smask = Ar['sketch_mask'] if bool(Ar['has_mask']) else None
        loss, logits, _ = O.sketch_loss(P, cfg, Ar['sketch_ids'], Ar['video_ids'], smask)
        return loss, [logits]
    ctx, mask = O.text_encoder(Ar['text'], P, cfg)
    if kind == 'nuwa':
        loss, logits = O.decoder_loss(P, cfg, Ar['video_ids'].reshape(b, -1), ctx, mask, return_logits=True)
        return loss, [logits]
    loss, vl, al = O.video_audio_loss(P, cfg, Ar['video_ids'].reshape(b, -1), Ar['audio_ids'], ctx, mask, return_logits=True)
    return loss, [vl, al]


def oracle_step(name, Ar, P):
    """loss, logits and every gradient of the oracle at the weights P: (loss, [logits], {key: grad})"""
    Pr = {k: v.detach().clone().requires_grad_(v.is_floating_point()) for k, v in P.items()}
    loss, logits = oracle_forward(name, Ar, Pr)
    loss.backward()
    return loss.detach(), [l.detach() for l in logits], {k: v.grad for k, v in Pr.items() if v.grad is not None}


# ------------------------------------------------------------------------------------------------------------------------------
# the product model on a state dict
# ------------------------------------------------------------------------------------------------------------------------------

def build_product(A, name, Ar):
    """a new product model of the fixture's configuration (CPU, default initialisation)"""
    kind = MODELS[name]['kind']
    rev = bool(Ar['reversible']) if 'reversible' in Ar else False
    if kind == 'nuwa':
        return _tiny_nuwa(A, rev)
    vae = A.VQGanVAE(dim=32, image_size=16, num_layers=2, vq_codebook_size=64, vq_codebook_dim=32, use_vgg_and_gan=False)
    if kind == 'va':
        return A.NUWAVideoAudio(vae=vae, sparse_3dna_rel_pos_bias=bool(Ar['rel_pos_bias']), **{**VA_KW, 'dec_reversible': rev})
    assert not rev, 'the sketch fixture used here is the plain one (g11a)'
    sketch_vae = A.VQGanVAE(dim=32, image_size=16, num_layers=2, vq_codebook_size=48, vq_codebook_dim=32, use_vgg_and_gan=False)
    return A.NUWASketch(vae=vae, sketch_vae=sketch_vae, **SKETCH_KW)


def put_state(model, P):
    """a fixture-style state dict into a product model: nothing unexpected, nothing missing but the tokenizers and the second
    registration of reversible blocks"""
    missing, unexpected = model.load_state_dict(P, strict=False)
    assert not unexpected, unexpected
    assert all(not kept(k) for k in missing), missing
    return model


def read_state(model):
    """the product model's current weights as the oracle's P dict (CPU clones, same key filter)"""
    return {k: v.detach().cpu().clone() for k, v in model.state_dict().items() if kept(k)}


def product_inputs(name, Ar, dev):
    """keyword arguments of the product model's forward for the fixture's inputs, without `video=` / `audio=` (see product_step)"""
    kind = MODELS[name]['kind']
    if kind == 'sketch':
        b, f = Ar['sketch_ids'].shape[:2]
        return dict(sketch=torch.zeros(b, f, 3, 16, 16, device=dev), sketch_mask=Ar['sketch_mask'].to(dev) if bool(Ar['has_mask']) else None)
    return dict(text=Ar['text'].to(dev))


def pin_sketch_ids(model, name, Ar, dev):
    """the sketch fixture carries the token ids of the reference's tokenizer (as test_g11_sketch_loss_logits_grads does)"""
    if MODELS[name]['kind'] == 'sketch':
        ids = Ar['sketch_ids'].to(dev)
        model.sketch_vae.get_video_indices = lambda frames: ids
    return model


def product_logits(model, name, Ar, dev):
    kw = product_inputs(name, Ar, dev)
    vid = Ar['video_ids'].to(dev)
    b = vid.shape[0]
    if MODELS[name]['kind'] == 'va':
        return list(model(video=vid.reshape(b, -1)[:, :-1], audio=Ar['audio_ids'].to(dev)[:, :-1], return_loss=False, cond_dropout_prob=0., **kw))
    return [model(video=vid.reshape(b, -1)[:, :-1], return_loss=False, cond_dropout_prob=0., **kw)]


def product_loss(model, name, Ar, dev, video_ids=None):
    """the training loss (a graph: call .backward() on it).  video_ids: other ids of the fixture's shape (default the fixture's)"""
    kw = product_inputs(name, Ar, dev)
    vid = (Ar['video_ids'] if video_ids is None else video_ids).to(dev)
    if MODELS[name]['kind'] == 'va':
        kw['audio'] = Ar['audio_ids'].to(dev)
    return model(video=vid, return_loss=True, cond_dropout_prob=0., **kw)
