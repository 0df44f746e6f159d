"""Generates tests/golden/g16_video_audio_wide.npz from the READ-ONLY reference checkout (imported through oracle/ref_shims.py, as
make_golden.py does): the reference's NUWAVideoAudio on a 17 x 17 token map -- 289 video tokens per frame, so that every audio row of
its CrossModalityCrossAttention attends 289 + 1 slots, two past what the packed single-query kernel holds -- and a bare reference
CrossModalityCrossAttention(chunk_size=4, context_chunk_size=289) with its outputs and all gradients.  fp32 CPU, dropout 0.

    python tests/golden/make_golden_video_audio_wide.py

Contents: text / video / audio token ids (b = 1, 2 frames), the loss and the video and audio logits of forward(); for the bare module
`xm.p.*` (state dict), `xm.x`, `xm.context`, `xm.y`, `xm.dy`, `xm.dx`, `xm.dcontext`, `xm.g.*`.
The MODEL's state dict is not stored: at 1.0 MB it alone is twice the size this fixture may have.  Its entries are the values
tests/golden_util.fill_params(module, seed=PARAM_SEED) draws per state-dict NAME, on the reference module here and on the product module
in the test (the g12 fixture's way; the decoder's boolean mask buffers keep their values).  The reversible text encoder is the exception: the reference's state dict names each of its tensors
twice (`layers.*` and `net.blocks.*`, the latter drawn last), so its entries are stored as `p.text_transformer.layers.*`.
Seeds: torch.manual_seed(0) for the bare module's parameters, torch.manual_seed(1) for data (make_golden.py's convention).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from golden_util import fill_params  # noqa: E402
from oracle import ref_shims  # noqa: E402

ref_shims.install()
from nuwa_pytorch import NUWAVideoAudio, VQGanVAE  # noqa: E402
from nuwa_pytorch.nuwa_pytorch import CrossModalityCrossAttention  # noqa: E402

WIDE_KW = dict(dim=32, image_size=68, num_audio_tokens=40, num_audio_tokens_per_video_frame=4, max_video_frames=2, text_num_tokens=50,
               text_max_seq_len=8, text_enc_depth=2, text_enc_dim_head=16, text_enc_heads=2, enc_reversible=True, dec_reversible=False,
               dec_depth=3, dec_dim_head=32, dec_heads=2, sparse_3dna_kernel_size=3, sparse_3dna_dilation=2, sparse_2dna_kernel_size=7,
               sparse_2dna_dilation=2, cross_modality_attn_every=3, audio_loss_weight=0.7, sparse_3dna_rel_pos_bias=False)
PARAM_SEED = 16


def g16_video_audio_wide():
    torch.manual_seed(0)
    vae = VQGanVAE(dim=32, image_size=68, num_layers=2, vq_codebook_size=64, vq_codebook_dim=32, use_vgg_and_gan=False)
    m = NUWAVideoAudio(vae=vae, **WIDE_KW)
    masks = {k: v.clone() for k, v in m.state_dict().items() if v.dtype == torch.bool}
    fill_params(m, seed=PARAM_SEED)                        # (Conv3d biases of the talking heads included: non-zero)
    with torch.no_grad():                                  # (fill_params sets every bool buffer: the attention masks are not its to set)
        for k, v in m.state_dict().items():
            if k in masks and not k.startswith('vae.'):
                v.copy_(masks[k])
    torch.manual_seed(1)
    text = torch.randint(1, 50, (1, 8))
    text[-1, 6:] = 0
    vid = torch.randint(0, 64, (1, 2, 17, 17))
    aud = torch.randint(0, 40, (1, 8))
    cap = {}
    hooks = [m.to_video_logits.register_forward_hook(lambda mod, i, o: cap.__setitem__('vl', o.detach())),
             m.to_audio_logits.register_forward_hook(lambda mod, i, o: cap.__setitem__('al', o.detach()))]
    with torch.no_grad():
        loss = m(text=text, video=vid, audio=aud, return_loss=True, cond_dropout_prob=0.)
    for h in hooks:
        h.remove()
    arrs = dict(text=text, video_ids=vid, audio_ids=aud, loss=loss, video_logits=cap['vl'], audio_logits=cap['al'], param_seed=PARAM_SEED)
    arrs.update({'p.' + k: v for k, v in m.state_dict().items() if k.startswith('text_transformer.layers.')})

    torch.manual_seed(0)
    xm = CrossModalityCrossAttention(dim=32, chunk_size=4, context_chunk_size=289, heads=2, dim_head=32)
    torch.manual_seed(1)
    x = torch.randn(1, 1 + 2 * 4, 32, requires_grad=True)
    context = torch.randn(1, 1 + 289, 32, requires_grad=True)
    y = xm(x, context)
    dy = torch.randn_like(y)
    y.backward(dy)
    arrs.update({'xm.x': x, 'xm.context': context, 'xm.y': y, 'xm.dy': dy, 'xm.dx': x.grad, 'xm.dcontext': context.grad})
    arrs.update({'xm.p.' + k: v for k, v in xm.state_dict().items()})
    arrs.update({'xm.g.' + k: p.grad for k, p in xm.named_parameters() if p.grad is not None})
    path = os.path.join(HERE, 'g16_video_audio_wide.npz')
    np.savez_compressed(path, **{k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrs.items()})
    print(f'g16_video_audio_wide: {os.path.getsize(path) / 1024:.1f} KiB')


if __name__ == '__main__':
    g16_video_audio_wide()
