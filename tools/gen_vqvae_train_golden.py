"""Write tests/golden/vqvae_train.npz: one training forward / backward of the REFERENCE's own VQVAE
(vqvae/vqvae_zc.py: VQVAE(channel=16, n_res_block=0, embed_dim=8, n_embed=32, stride=6).train()) on a [2, 3, 32, 48] input
with the loss mse(dec, img) + 0.25 * diff -- the initial state dict and the input, dec, diff and the ids, every parameter
gradient, and the three Quantize buffers after the EMA update.  Data only.  Runs on the CPU; needs torch, numpy and a
checkout of the reference:

    python tools/gen_vqvae_train_golden.py /path/to/reference
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 20261


def main(ref_root):
    spec = importlib.util.spec_from_file_location("ref_vqvae_zc", os.path.join(ref_root, "vqvae", "vqvae_zc.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    torch.manual_seed(SEED)
    model = ref.VQVAE(channel=16, n_res_block=0, embed_dim=8, n_embed=32, stride=6).train()
    g = torch.Generator().manual_seed(SEED)
    with torch.no_grad():
        # the default initialisation leaves the encoder's output far smaller than the codebook (every pixel on one code):
        # scale the last encoder layer so that the 48 pixels spread over the codes, and give the EMA state a history
        model.enc_b.blocks[6].weight.mul_(8.0)
        model.enc_b.blocks[6].bias.copy_(torch.randn(8, generator=g) * 0.2)
        model.quantize_t.cluster_size.copy_(torch.rand(32, generator=g) * 3)
        model.quantize_t.embed_avg.copy_(model.quantize_t.embed * model.quantize_t.cluster_size.clamp_min(0.5))
    out = {"param." + k: v.detach().clone().numpy() for k, v in model.state_dict().items()}
    img = torch.randn(2, 3, 32, 48, generator=g)
    dec, diff = model(img)
    loss = torch.nn.functional.mse_loss(dec, img) + 0.25 * diff.mean()
    loss.backward()
    # the ids of that forward: the lookup used the codebook from BEFORE the update, which the saved initial state holds
    with torch.no_grad():
        model.eval()
        before = ref.VQVAE(channel=16, n_res_block=0, embed_dim=8, n_embed=32, stride=6).eval()
        before.load_state_dict({k[6:]: torch.from_numpy(v) for k, v in out.items()})
        ids = before.encode(img)[2]
    out.update({"img": img.numpy(), "dec": dec.detach().numpy(), "diff": diff.detach().numpy(), "ids": ids.numpy(),
                "loss": loss.detach().numpy()})
    for k, p in model.named_parameters():
        out["grad." + k] = p.grad.numpy()
    for k in ("embed", "cluster_size", "embed_avg"):
        out["after.quantize_t." + k] = getattr(model.quantize_t, k).detach().numpy()
    path = os.path.join(ROOT, "tests", "golden", "vqvae_train.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(set(ids.reshape(-1).tolist())), "codes in use")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
