"""Plain-torch restatement of the VQ-VAE tokenizer's TRAINING step (helper, no tests): forward of the stride-6, simple,
n_res_block=0 topology (three 4x4 stride-2 convolutions + 1x1, nearest code, three 4x4 stride-2 transposed convolutions +
1x1), the loss mse(dec, img) + w * diff, the EMA codebook update and the parameter gradients through autograd, on the CPU in
any dtype.  State dict keys as the module's: enc_b.blocks.{0,2,4,6}.*, quantize_t.{embed,cluster_size,embed_avg},
dec.blocks.{0,2,4,6}.*.
"""
import torch
import torch.nn.functional as F

BUFFERS = ("quantize_t.embed", "quantize_t.cluster_size", "quantize_t.embed_avg")
# two distances closer than this fraction of (|x|^2 + |E_j|^2) count as tied: 16 units of fp32 rounding (2^-24 each) of the
# largest term of |x|^2 - 2 x.E + |E|^2 -- what two correct fp32 summation orders of that expression can differ by
TIE_ULPS = 16 * 2.0 ** -24


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def encoder(p, img):
    x = F.relu(F.conv2d(img, p["enc_b.blocks.0.weight"], p["enc_b.blocks.0.bias"], stride=2, padding=1))
    x = F.relu(F.conv2d(x, p["enc_b.blocks.2.weight"], p["enc_b.blocks.2.bias"], stride=2, padding=1))
    x = F.relu(F.conv2d(x, p["enc_b.blocks.4.weight"], p["enc_b.blocks.4.bias"], stride=2, padding=1))
    return F.conv2d(x, p["enc_b.blocks.6.weight"], p["enc_b.blocks.6.bias"]).permute(0, 2, 3, 1)


def decoder(p, q_nhwc):
    x = q_nhwc.permute(0, 3, 1, 2)
    x = F.relu(F.conv_transpose2d(x, p["dec.blocks.0.weight"], p["dec.blocks.0.bias"], stride=2, padding=1))
    x = F.relu(F.conv_transpose2d(x, p["dec.blocks.2.weight"], p["dec.blocks.2.bias"], stride=2, padding=1))
    x = F.relu(F.conv_transpose2d(x, p["dec.blocks.4.weight"], p["dec.blocks.4.bias"], stride=2, padding=1))
    return F.conv2d(x, p["dec.blocks.6.weight"], p["dec.blocks.6.bias"])


def distances(flat, embed):
    return flat.pow(2).sum(1, keepdim=True) - 2 * flat @ embed + embed.pow(2).sum(0, keepdim=True)


def near_ties(dist, flat, embed):
    """bool [M]: pixels whose two smallest distances are tied in the sense of TIE_ULPS."""
    two = dist.double().topk(2, dim=1, largest=False)
    scale = flat.double().pow(2).sum(1) + embed.double().pow(2).sum(0)[two.indices[:, 0]]
    return (two.values[:, 1] - two.values[:, 0]) <= TIE_ULPS * scale


def ids_acceptable(ids_dev, dist, flat, embed):
    """(share of near-tie pixels, ok): the device's ids equal the restatement's argmin except at near-tie pixels, and even
    there the code they chose is within the tie tolerance of the smallest distance."""
    ids_dev = ids_dev.reshape(-1).cpu()
    d = dist.double()
    best = d.min(1)
    scale = flat.double().pow(2).sum(1) + embed.double().pow(2).sum(0)[best.indices]
    ties = near_ties(dist, flat, embed)
    differ = ids_dev != (-dist).max(1)[1]
    chosen = d.gather(1, ids_dev.view(-1, 1)).squeeze(1)
    ok = bool((~differ | ties).all()) and bool(((chosen - best.values) <= TIE_ULPS * scale).all())
    return ties.double().mean().item(), ok


def ema_update(embed, cluster_size, embed_avg, ids, flat, decay=0.99, eps=1e-5):
    """vqvae/vqvae_zc.py:68-83 without the one-hot matrix: (embed, cluster_size, embed_avg) after the update."""
    n_embed = embed.shape[1]
    count = torch.bincount(ids.reshape(-1), minlength=n_embed).to(flat.dtype)
    total = torch.zeros_like(embed).index_add_(1, ids.reshape(-1), flat.t())
    cluster_size = cluster_size * decay + (1 - decay) * count
    embed_avg = embed_avg * decay + (1 - decay) * total
    n = cluster_size.sum()
    smoothed = (cluster_size + eps) / (n + n_embed * eps) * n
    return embed_avg / smoothed.unsqueeze(0), cluster_size, embed_avg


def train_forward_backward(state, img, dtype=torch.float32, ids=None, train_codebook=True, latent_loss_weight=0.25,
                           trainable=lambda name: True):
    """One forward / backward of the training step on `state` (a state dict; not modified).  ids: use these instead of the
    restatement's own argmin (the device's ids, so that a legitimate near-tie cannot cascade into everything downstream).
    Returns dict(dec, diff, ids, own_ids, dist, flat, loss, recon_loss, grads {name: grad or None}, buffers {name: after the
    update}).  The lookup uses the codebook from BEFORE the update."""
    p = {k: v.detach().to(dtype).clone() for k, v in state.items()}
    for k, v in p.items():
        if k not in BUFFERS and trainable(k):
            v.requires_grad_(True)
    img = img.to(dtype)
    logits = encoder(p, img)
    flat = logits.reshape(-1, logits.shape[-1])
    embed = p["quantize_t.embed"]
    dist = distances(flat.detach(), embed)
    own_ids = (-dist).max(1)[1]
    use = own_ids if ids is None else ids.reshape(-1).cpu()
    q = F.embedding(use, embed.t()).view_as(logits)
    buffers = {k: p[k] for k in BUFFERS}
    if train_codebook:
        e, cs, avg = ema_update(embed, p["quantize_t.cluster_size"], p["quantize_t.embed_avg"], use, flat.detach())
        buffers = {"quantize_t.embed": e, "quantize_t.cluster_size": cs, "quantize_t.embed_avg": avg}
    diff = (q.detach() - logits).pow(2).mean()
    quantize = logits + (q - logits).detach()
    dec = decoder(p, quantize)
    recon = F.mse_loss(dec, img)
    loss = recon + latent_loss_weight * diff
    loss.backward()
    return dict(dec=dec.detach(), diff=diff.detach(), ids=use.view(logits.shape[:-1]), own_ids=own_ids.view(logits.shape[:-1]),
                dist=dist, flat=flat.detach(), loss=loss.detach(), recon_loss=recon.detach(),
                grads={k: v.grad for k, v in p.items() if k not in BUFFERS}, buffers=buffers)


def sgd_step(state, out, lr):
    """state after one plain SGD step on out's gradients, with out's updated buffers."""
    new = {k: v.detach().clone() for k, v in state.items()}
    for k, g in out["grads"].items():
        if g is not None:
            new[k] = new[k].to(g.dtype) - lr * g
    for k, v in out["buffers"].items():
        new[k] = v.detach().clone()
    return new


def random_state(model_state, seed, weight_scale=1.0):
    """A state dict with the shapes of model_state and seeded values (biases included, so that no gradient is trivially zero)."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, v in model_state.items():
        if k == "quantize_t.cluster_size":
            out[k] = torch.rand(v.shape, generator=g) * 3
        elif k.endswith(".bias"):
            out[k] = torch.randn(v.shape, generator=g) * 0.1
        else:
            fan = v[0].numel() if v.dim() > 1 else 1
            out[k] = torch.randn(v.shape, generator=g) * weight_scale / max(fan, 1) ** 0.5
    out["quantize_t.embed_avg"] = out["quantize_t.embed"] * out["quantize_t.cluster_size"].clamp_min(0.5)
    return out
