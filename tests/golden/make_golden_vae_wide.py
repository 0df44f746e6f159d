"""Generates tests/golden/g17_vae_wide.npz from the READ-ONLY reference checkout (imported through oracle/ref_shims.py, as
make_golden.py does): the reference's VQGanVAE with default attention (8 heads x 64) on one 80 x 80 frame, i.e. a 20 x 20 feature
map -- 400 positions, past what the LDS-resident attention kernels hold.  fp32 CPU.

    python tests/golden/make_golden_vae_wide.py

Contents: the image, the last encoder feature map, the code ids, the top-2 similarity gap and the reconstruction (decode of the
quantised map).  No parameters: they are the values tests/golden_util.fill_params(module, seed=PARAM_SEED) draws per state-dict NAME,
and the attention log-scales are then set by tests/vae_wide_util.sharpen_attention(module, 400, seed=PARAM_SEED) -- on the reference
module here and on the product module in the test.
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
from vae_wide_util import sharpen_attention  # noqa: E402
from oracle import ref_shims  # noqa: E402

ref_shims.install()
from nuwa_pytorch import VQGanVAE  # noqa: E402

PARAM_SEED = 17
VAE_KW = dict(dim=32, image_size=80, num_layers=2, vq_codebook_size=64, vq_codebook_dim=32, use_vgg_and_gan=False)


def g17_vae_wide():
    torch.manual_seed(0)
    vae = VQGanVAE(**VAE_KW).eval()
    fill_params(vae, seed=PARAM_SEED)
    sharpen_attention(vae, 400, seed=PARAM_SEED)
    torch.manual_seed(1)
    img = torch.rand(1, 3, 80, 80)
    with torch.no_grad():
        fm = img
        for enc in vae.encoders:
            fm = enc(fm)
        quant, ind, _ = vae.vq(fm)          # VQ = shimmed restatement: PARITY UNPINNED
        xn = torch.nn.functional.normalize(vae.vq.project_in(fm.permute(0, 2, 3, 1)), dim=-1)
        top2 = (xn @ torch.nn.functional.normalize(vae.vq.embed, dim=-1).t()).topk(2, dim=-1).values
        recon = vae.decode(quant)
    arrs = dict(img=img, fmap=fm, indices=ind, top2_gap=top2[..., 0] - top2[..., 1], recon=recon, param_seed=PARAM_SEED)
    path = os.path.join(HERE, 'g17_vae_wide.npz')
    np.savez_compressed(path, **{k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrs.items()})
    print(f'g17_vae_wide: {os.path.getsize(path) / 1024:.1f} KiB; fmap {tuple(fm.shape)}, min top-2 gap {float(arrs["top2_gap"].min()):.3e}')


if __name__ == '__main__':
    g17_vae_wide()
