"""Plain-torch restatement of the VQ-VAE tokenizer's TRAINING step for ANY topology the constructors build (helper, no tests):
a functional walk over a block list -- Conv2d 4x4 stride 2 / 3x3 / 1x1, ConvTranspose2d 4x4 stride 2 / 1x1, ReLU, and
ResBlock as branch(relu(x)) + relu(x) (the block's leading ReLU is in place, so the skip connection carries relu(x)) -- with
the weights read from a state dict by the module's keys, then the loss, the EMA update and autograd as in
tests/vqvae_train_cases.py, whose pieces (distances, ema_update, ids_acceptable, rel, random_state) are reused."""
import os

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from tests import vqvae_train_cases as T

BUFFERS = T.BUFFERS
CONFIG_I = dict(channel=8, n_res_block=2, n_res_channel=8, embed_dim=8, n_embed=32, stride=6)          # fixture "i"
CONFIG_III = dict(channel=8, n_res_block=0, embed_dim=8, n_embed=32, stride=4)                         # fixture "iii"


def block_spec(blocks):
    """The structure of an nn.Sequential of the block vocabulary, without its weights: a list of ("relu",), ("res",),
    ("conv", stride, padding) and ("convT", stride, padding).  Works on the reference's modules and on cogview_amd's alike
    (a ResBlock is recognised by its `conv` member)."""
    spec = []
    for m in blocks:
        if isinstance(m, nn.ReLU):
            spec.append(("relu",))
        elif isinstance(m, nn.ConvTranspose2d):
            spec.append(("convT", m.stride, m.padding))
        elif isinstance(m, nn.Conv2d):
            spec.append(("conv", m.stride, m.padding))
        else:
            assert isinstance(m.conv, nn.Sequential) and len(m.conv) == 4
            spec.append(("res",))
    return spec


def run_blocks(p, prefix, spec, x):
    """The block list `spec` on the NCHW tensor x with the parameters p[prefix + ".blocks.<i>..."]."""
    for i, s in enumerate(spec):
        key = f"{prefix}.blocks.{i}"
        if s[0] == "relu":
            x = F.relu(x)
        elif s[0] == "conv":
            x = F.conv2d(x, p[key + ".weight"], p[key + ".bias"], stride=s[1], padding=s[2])
        elif s[0] == "convT":
            x = F.conv_transpose2d(x, p[key + ".weight"], p[key + ".bias"], stride=s[1], padding=s[2])
        else:
            r = F.relu(x)
            t = F.relu(F.conv2d(r, p[key + ".conv.1.weight"], p[key + ".conv.1.bias"], padding=1))
            x = F.conv2d(t, p[key + ".conv.3.weight"], p[key + ".conv.3.bias"]) + r
    return x


def model_spec(model):
    return block_spec(model.enc_b.blocks), block_spec(model.dec.blocks)


def train_forward_backward(spec, state, img, dtype=torch.float32, ids=None, train_codebook=True, latent_loss_weight=0.25,
                           trainable=lambda name: True):
    """tests/vqvae_train_cases.train_forward_backward for the topology spec = model_spec(model): same arguments otherwise,
    same result dict."""
    enc, dec_spec = spec
    p = {k: v.detach().to(dtype).clone() for k, v in state.items()}
    for k, v in p.items():
        if k not in BUFFERS and trainable(k):
            v.requires_grad_(True)
    img = img.to(dtype)
    logits = run_blocks(p, "enc_b", enc, img).permute(0, 2, 3, 1)
    flat = logits.reshape(-1, logits.shape[-1])
    embed = p["quantize_t.embed"]
    dist = T.distances(flat.detach(), embed)
    own_ids = (-dist).max(1)[1]
    use = own_ids if ids is None else ids.reshape(-1).cpu()
    q = F.embedding(use, embed.t()).view_as(logits)
    buffers = {k: p[k] for k in BUFFERS}
    if train_codebook:
        e, cs, avg = T.ema_update(embed, p["quantize_t.cluster_size"], p["quantize_t.embed_avg"], use, flat.detach())
        buffers = {"quantize_t.embed": e, "quantize_t.cluster_size": cs, "quantize_t.embed_avg": avg}
    diff = (q.detach() - logits).pow(2).mean()
    quantize = logits + (q - logits).detach()
    dec = run_blocks(p, "dec", dec_spec, quantize.permute(0, 3, 1, 2))
    recon = F.mse_loss(dec, img)
    loss = recon + latent_loss_weight * diff
    loss.backward()
    return dict(dec=dec.detach(), diff=diff.detach(), ids=use.view(logits.shape[:-1]), own_ids=own_ids.view(logits.shape[:-1]),
                dist=dist, flat=flat.detach(), loss=loss.detach(), recon_loss=recon.detach(),
                grads={k: v.grad for k, v in p.items() if k not in BUFFERS}, buffers=buffers)


def fixture(golden_dir, name):
    """(everything stored for configuration `name` of tests/golden/vqvae_train_res.npz, its initial state dict)"""
    z = np.load(os.path.join(golden_dir, "vqvae_train_res.npz"), allow_pickle=False)
    g = {k[len(name) + 1:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(name + ".")}
    return g, {k[6:]: v for k, v in g.items() if k.startswith("param.")}


def fixture_reference(g):
    """The reference's own results of a fixture configuration, in train_forward_backward's shape."""
    return dict(dec=g["dec"], diff=g["diff"], loss=g["loss"], grads={k[5:]: v for k, v in g.items() if k.startswith("grad.")},
                buffers={k[6:]: v for k, v in g.items() if k.startswith("after.")})
