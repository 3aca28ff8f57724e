"""Images per second of vqvae.train_step on the production tokenizer (vqvae.new_model(), 256 x 256 images) or, with
--topology default, on VQVAE() with its own default arguments (stride 4, two ResBlocks of 32 channels per stack, 1024 codes;
trained under set_train_topologies("all")), with a yardstick
in the same process: the same step written with plain torch.nn modules in fp32 (F.conv2d / F.conv_transpose2d and their
autograd, distances by one matmul, the EMA sums by index_add_ -- not the reference's one-hot product, which needs
batch x 1024 x 8192 floats).  Both use SGD.  Per batch: a warm-up, then the two routes alternate and the median of 7 steps of
each is reported; then one step with every launch bracketed by events (ops.timed_launch) for the per-kernel table and the
weight-gradient family's share of the 157.3 TFLOP/s fp32-MFMA peak; then the peak memory of a step.

Batches: 32, and the largest power of two up to --max-batch at which train_step fits (the yardstick is left out of a batch
it does not fit).  Progress goes to stderr, one JSON line per batch to stdout.

    python tools/mb_vqvae_train.py [--topology production|default] [--batch 32] [--max-batch 256] [--reps 7] [--size 256] [--no-torch]
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FP32_MFMA_PEAK_TFLOPS = 157.3


class TorchResBlock(nn.Module):
    """vqvae/vqvae_zc.py:99-114 without the in-place ReLU: branch(relu(x)) + relu(x), which is what that block computes."""

    def __init__(self, in_channel, channel):
        super().__init__()
        self.conv = nn.Sequential(nn.Conv2d(in_channel, channel, 3, padding=1), nn.ReLU(), nn.Conv2d(channel, in_channel, 1))

    def forward(self, x):
        r = F.relu(x)
        return self.conv(r) + r


class TorchVQVAE(nn.Module):
    """The production topology (default arguments) or, with topology="default", VQVAE()'s own default topology, in plain
    torch.nn, channels-first, fp32."""

    def __init__(self, channel=512, embed_dim=256, n_embed=8192, decay=0.99, eps=1e-5, topology="production"):
        super().__init__()
        c = channel
        if topology == "production":
            self.enc = nn.Sequential(nn.Conv2d(3, c, 4, 2, 1), nn.ReLU(), nn.Conv2d(c, c, 4, 2, 1), nn.ReLU(), nn.Conv2d(c, c, 4, 2, 1), nn.ReLU(),
                                     nn.Conv2d(c, embed_dim, 1))
            self.dec = nn.Sequential(nn.ConvTranspose2d(embed_dim, c, 4, 2, 1), nn.ReLU(), nn.ConvTranspose2d(c, c, 4, 2, 1), nn.ReLU(),
                                     nn.ConvTranspose2d(c, c, 4, 2, 1), nn.ReLU(), nn.Conv2d(c, 3, 1))
        else:
            self.enc = nn.Sequential(nn.Conv2d(3, c // 2, 4, 2, 1), nn.ReLU(), nn.Conv2d(c // 2, c, 4, 2, 1), nn.ReLU(), nn.Conv2d(c, c, 3, padding=1),
                                     TorchResBlock(c, 32), TorchResBlock(c, 32), nn.ReLU(), nn.Conv2d(c, embed_dim, 1))
            self.dec = nn.Sequential(nn.ConvTranspose2d(embed_dim, c, 4, 2, 1), TorchResBlock(c, 32), TorchResBlock(c, 32), nn.ReLU(),
                                     nn.ConvTranspose2d(c, 3, 4, 2, 1))
        self.decay, self.eps, self.n_embed = decay, eps, n_embed
        embed = torch.randn(embed_dim, n_embed)
        self.register_buffer("embed", embed)
        self.register_buffer("cluster_size", torch.zeros(n_embed))
        self.register_buffer("embed_avg", embed.clone())

    def forward(self, img):
        x = self.enc(img).permute(0, 2, 3, 1)
        flat = x.reshape(-1, x.shape[-1])
        with torch.no_grad():
            dist = flat.pow(2).sum(1, keepdim=True) - 2 * flat @ self.embed + self.embed.pow(2).sum(0, keepdim=True)
            ids = (-dist).max(1)[1]
            del dist
            q = F.embedding(ids, self.embed.t()).view_as(x)
            count = torch.bincount(ids, minlength=self.n_embed).float()
            total = torch.zeros_like(self.embed).index_add_(1, ids, flat.t())
            self.cluster_size.mul_(self.decay).add_(count, alpha=1 - self.decay)
            self.embed_avg.mul_(self.decay).add_(total, alpha=1 - self.decay)
            n = self.cluster_size.sum()
            smoothed = (self.cluster_size + self.eps) / (n + self.n_embed * self.eps) * n
            self.embed.copy_(self.embed_avg / smoothed.unsqueeze(0))
        diff = (q - x).pow(2).mean()
        return self.dec((x + (q - x).detach()).permute(0, 3, 1, 2)), diff


def torch_step(model, opt, img, w=0.25):
    opt.zero_grad(set_to_none=True)
    dec, diff = model(img)
    loss = F.mse_loss(dec, img) + w * diff
    loss.backward()
    opt.step()
    return loss.detach()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def say(msg):
    print(msg, file=sys.stderr, flush=True)


def measure(batch, size, reps, routes, topology):
    from cogview_amd import ops
    img = torch.randn(batch, 3, size, size, device="cuda", generator=torch.Generator("cuda").manual_seed(batch))
    for k in list(routes):                             # warm-up: code objects, library algorithm choices, allocator
        try:
            t = [timed(lambda: routes[k](img)) for _ in range(2)]
            say(f"batch {batch}: {k} warmed up ({t[0]:.1f} s, {t[1]:.2f} s)")
        except torch.cuda.OutOfMemoryError:
            say(f"batch {batch}: {k} does not fit, left out")
            routes = {r: f for r, f in routes.items() if r != k}
            torch.cuda.empty_cache()
    times = {k: [] for k in routes}
    for i in range(reps):
        for k, f in routes.items():
            times[k].append(timed(lambda: f(img)))
        say(f"batch {batch}: repetition {i + 1} of {reps}")
    res = {"batch": batch, "topology": topology}
    for k, ts in times.items():
        med = sorted(ts)[len(ts) // 2]
        res[k] = {"images_per_s_median": round(batch / med, 2), "step_ms_median": round(med * 1e3, 2),
                  "step_ms_all": [round(t * 1e3, 1) for t in ts]}
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    routes["hip"](img)
    torch.cuda.synchronize()
    res["hip"]["peak_step_mbytes_per_image"] = round((torch.cuda.max_memory_allocated() - base) / batch / 2 ** 20, 1)
    ops.enable_gemm_timing()
    routes["hip"](img)
    stats = ops.collect_gemm_timing()
    res["hip"]["kernels"] = {k: {"ms": round(v["total_ms"], 3), "launches": v["launches"], "tflops": round(v["tflops"], 2)}
                             for k, v in sorted(stats["by_variant"].items(), key=lambda kv: -kv[1]["total_ms"])}
    res["hip"]["kernel_ms_total"] = round(stats["total_ms"], 2)
    wg = stats["by_variant"].get("conv_wgrad")
    if wg:
        res["hip"]["wgrad_share_of_fp32_mfma_peak"] = round(wg["tflops"] / FP32_MFMA_PEAK_TFLOPS, 4)
        res["hip"]["wgrad_by_shape"] = {k: v for k, v in stats["by_shape"].items() if k.startswith("conv_wgrad")}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--topology", choices=("production", "default"), default="production",
                    help="production: vqvae.new_model(); default: VQVAE() under set_train_topologies('all')")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--max-batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch.nn yardstick")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X: nothing here is measured on a CPU"
    from cogview_amd import vqvae
    torch.manual_seed(0)
    if args.topology == "production":
        model = vqvae.new_model().cuda().train()
    else:
        model = vqvae.set_train_topologies(vqvae.VQVAE(), "all").cuda().train()
    opt = torch.optim.SGD(model.parameters(), lr=1e-4)
    routes = {"hip": lambda img: vqvae.train_step(model, opt, img)}
    if not args.no_torch:
        ref = (TorchVQVAE() if args.topology == "production" else
               TorchVQVAE(channel=128, embed_dim=64, n_embed=1024, topology="default")).cuda().train()
        ropt = torch.optim.SGD(ref.parameters(), lr=1e-4)
        routes["torch_nn_fp32"] = lambda img: torch_step(ref, ropt, img)
    out = [measure(args.batch, args.size, args.reps, routes, args.topology)]
    print(json.dumps(out[-1]), flush=True)
    fits, b = args.batch, args.batch * 2
    while b <= args.max_batch:                          # the largest power of two at which train_step fits: one step each
        try:
            img = torch.randn(b, 3, args.size, args.size, device="cuda")
            routes["hip"](img)
            torch.cuda.synchronize()
            fits = b
            say(f"batch {b}: train_step fits")
        except torch.cuda.OutOfMemoryError:
            break
        finally:
            img = None
            model.zero_grad(set_to_none=True)
            torch.cuda.empty_cache()
        b *= 2
    if fits != args.batch:
        out.append(measure(fits, args.size, args.reps, routes, args.topology))
        print(json.dumps(out[-1]), flush=True)
    print(json.dumps({"largest_batch_tried_that_fits": fits, "max_batch": args.max_batch}))


if __name__ == "__main__":
    main()
