"""Generates the long-text fixtures g21a / g21b: the reference's OWN NUWA.generate() under a text of 300 tokens -- more context keys
than the packed key images of the single-query cross-attention kernel hold (287) -- recorded the way make_golden_long_generate records
g18.

    python tests/golden/make_golden_long_context.py

Tiny model of make_golden.tiny_nuwa with text_max_seq_len = 300 (token map 4 x 4 -> 16 tokens per frame, max_video_frames 3), parameter
seed 0, text = randint(1, 50, (2, 300)) with tokens 120: of sample 1 set to 0 (padding): its context slots 121 .. 300 are hidden, so the
SECOND 128-slot split of the rows kernel (slots 128 .. 255) is wholly masked for that sample and the third holds hidden slots only.
torch.manual_seed(2) before generate, greedy sampling (filter_thres 0.99 keeps one logit), cond_scale 2, num_frames 5: 80 tokens, the
window slides at token 49 and at token 65.

Besides the sampled ids every fixture carries the reference's CONDITIONED full-sequence logits on its own first 48 ids (one forward,
return_loss=True with the to_logits output hooked: 48 rows, row t scores token t) for teacher-forced comparisons.

Greedy sampling reproduces only while the arg-max is not a near tie: the gap between the two largest guided logits is recorded at every
step, the minimum goes into the fixture (`min_gap`) and the script ASSERTS min_gap >= 3e-3, trying text seeds in order until one meets
it.  That is a condition on the inputs, as in g18, not a tolerance of any test.
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402  (installs the reference shims)
from nuwa_pytorch import nuwa_pytorch as ref_np  # noqa: E402

MIN_GAP = 3e-3
TEXT_LEN = 300
CASES = (('g21a_generate_long_context', False), ('g21b_generate_long_context_reversible', True))       # name, reversible
SEEDS = range(1, 17)


def tiny_nuwa_long_text(reversible):
    """make_golden.tiny_nuwa with a text of up to TEXT_LEN tokens"""
    torch.manual_seed(0)
    vae = MG.VQGanVAE(dim=32, image_size=16, num_layers=2, vq_codebook_size=64, vq_codebook_dim=32, use_vgg_and_gan=False)
    return MG.NUWA(vae=vae, dim=32, text_num_tokens=50, text_max_seq_len=TEXT_LEN, max_video_frames=3, text_enc_depth=2, dec_depth=3,
                   enc_reversible=True, dec_reversible=reversible, dec_heads=2, dec_dim_head=32, text_enc_heads=2, text_enc_dim_head=16,
                   sparse_3dna_kernel_size=3, sparse_3dna_dilation=(1, 2))


def sample(m, text, num_frames, cond_scale):
    """-> (ids [2, num_frames * 16], minimum top-2 gap of the guided logits over all steps)"""
    seen, gaps = [], []
    keep_decode = m.vae.decode
    m.vae.decode = lambda codes: (seen.append(codes.detach().clone()), torch.zeros(codes.shape[0], 3, 16, 16))[1]
    orig_top_k = ref_np.top_k

    def top_k(logits, thres=0.5):
        top2 = logits.topk(2, dim=-1).values
        gaps.append(float((top2[:, 0] - top2[:, 1]).min()))
        return orig_top_k(logits, thres=thres)

    ref_np.top_k = top_k
    try:
        torch.manual_seed(2)
        m.generate(text=text, filter_thres=0.99, cond_scale=cond_scale, num_frames=num_frames)
    finally:
        ref_np.top_k = orig_top_k
        m.vae.decode = keep_decode
    ids = MG._codes_to_ids(torch.cat(seen, 0), m.vae.codebook).reshape(2, -1)
    assert ids.shape[1] == num_frames * 16 and len(gaps) == ids.shape[1]
    return ids, min(gaps)


def generate_long_context(name, reversible, num_frames=5, cond_scale=2.):
    m = tiny_nuwa_long_text(reversible).eval()
    for seed in SEEDS:
        torch.manual_seed(seed)
        text = torch.randint(1, 50, (2, TEXT_LEN))
        text[1, 120:] = 0
        with torch.no_grad():
            ids, min_gap = sample(m, text, num_frames, cond_scale)
        print(f'{name}: text seed {seed}: minimum top-2 gap {min_gap:.2e}')
        if min_gap >= MIN_GAP:
            break
    assert min_gap >= MIN_GAP, f'{name}: a near tie ({min_gap:.2e} < {MIN_GAP}) under every text seed'
    cap = {}
    hook = m.to_logits.register_forward_hook(lambda mod, i, o: cap.__setitem__('logits', o.detach()))
    with torch.no_grad():
        m(text=text, video=ids[:, :48].reshape(2, 3, 4, 4), return_loss=True, cond_dropout_prob=0.)
    hook.remove()
    assert tuple(cap['logits'].shape) == (2, 48, 64)
    P = {k: v for k, v in MG.params(m).items() if not k.startswith('p.vae.') and '.net.blocks.' not in k}
    MG.save(name, text=text, text_seed=seed, video_ids=ids, cond_scale=cond_scale, reversible=reversible, num_frames=num_frames,
            min_gap=min_gap, cond_logits=cap['logits'], **P)


if __name__ == '__main__':
    for case in CASES:
        generate_long_context(*case)
