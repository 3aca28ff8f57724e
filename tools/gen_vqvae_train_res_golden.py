"""Write tests/golden/vqvae_train_res.npz: one training forward / backward of the REFERENCE's own VQVAE (vqvae/vqvae_zc.py,
.train()) with the loss mse(dec, img) + 0.25 * diff, for two topologies outside the production one:

    i    VQVAE(channel=8, n_res_block=2, n_res_channel=8, embed_dim=8, n_embed=32, stride=6) on a [2, 3, 32, 48] input
         (ResBlocks in both stacks, the ReLU behind a ResBlock chain in front of a 1x1 and of a transposed convolution)
    iii  VQVAE(channel=8, n_res_block=0, embed_dim=8, n_embed=32, stride=4) on a [2, 3, 16, 24] input
         (the stride-4 encoder, which ends in a 3x3 convolution)

Per configuration, under the prefix "<name>.": the initial state dict (seeded as tests/vqvae_train_cases.random_state with
weight_scale=1.0 -- the reference's default initialisation puts every pixel on one code), the input, dec, diff, the ids, the
loss, every parameter gradient, and the three Quantize buffers after the EMA update.  Data only, float32 and int64.  The
generator refuses a state under which fewer than 8 codes are in use or more than 1 % of the pixels are near-ties
(tests/vqvae_train_cases.near_ties).  Runs on the CPU; needs torch, numpy and a checkout of the reference:

    python tools/gen_vqvae_train_res_golden.py /path/to/reference
"""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (constructor arguments, input shape, seed: the first from 20262 on under which the state passes the generator's checks)
CONFIGS = {
    "i": (dict(channel=8, n_res_block=2, n_res_channel=8, embed_dim=8, n_embed=32, stride=6), (2, 3, 32, 48), 20269),
    "iii": (dict(channel=8, n_res_block=0, embed_dim=8, n_embed=32, stride=4), (2, 3, 16, 24), 20262),
}


def one(ref, T, name, kwargs, shape, seed):
    model = ref.VQVAE(**kwargs).train()
    state = T.random_state(model.state_dict(), seed, weight_scale=1.0)
    model.load_state_dict(state)
    out = {f"{name}.param.{k}": v.detach().clone().numpy() for k, v in model.state_dict().items()}
    img = torch.randn(*shape, generator=torch.Generator().manual_seed(seed + 1))
    with torch.no_grad():                                # the ids and their margins, from the codebook BEFORE the update
        before = ref.VQVAE(**kwargs).eval()
        before.load_state_dict(state)
        logits = before.enc_b(img)
        ids = before.encode(img)[2]
        flat = logits.reshape(-1, logits.shape[-1])
        ties = T.near_ties(T.distances(flat, state["quantize_t.embed"]), flat, state["quantize_t.embed"]).double().mean().item()
    codes = len(set(ids.reshape(-1).tolist()))
    assert codes >= 8 and ties <= 0.01, (name, codes, ties)
    dec, diff = model(img)
    loss = torch.nn.functional.mse_loss(dec, img) + 0.25 * diff.mean()
    loss.backward()
    out.update({f"{name}.img": img.numpy(), f"{name}.dec": dec.detach().numpy(), f"{name}.diff": diff.detach().numpy(),
                f"{name}.ids": ids.numpy(), f"{name}.loss": loss.detach().numpy()})
    for k, p in model.named_parameters():
        out[f"{name}.grad.{k}"] = p.grad.numpy()
    for k in ("embed", "cluster_size", "embed_avg"):
        out[f"{name}.after.quantize_t.{k}"] = getattr(model.quantize_t, k).detach().numpy()
    print(f"{name}: {codes} codes in use over {ids.numel()} pixels, near-tie share {ties:.4f}, loss {loss.item():.6f}")
    return out


def main(ref_root):
    from tests import vqvae_train_cases as T
    spec = importlib.util.spec_from_file_location("ref_vqvae_zc", os.path.join(ref_root, "vqvae", "vqvae_zc.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)
    out = {}
    for name, (kwargs, shape, seed) in CONFIGS.items():
        out.update(one(ref, T, name, kwargs, shape, seed))
    assert all(v.dtype in (np.float32, np.int64) for v in out.values())
    path = os.path.join(ROOT, "tests", "golden", "vqvae_train_res.npz")
    np.savez(path, **out)
    assert os.path.getsize(path) < 256 * 1024
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
