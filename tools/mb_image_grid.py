"""Time from VQ-VAE codes to the uint8 image-grid bytes on the host, two routes in one process on the production tokenizer:

  device : vqvae.code2img_u8 -- the decoder, ops.image_grid on its output, one device-to-host copy of 3 bytes per pixel
  host   : what torchvision.utils.save_image does -- vqvae.code2img, .cpu() (12 bytes per pixel), then make_grid and the
           byte conversion as torch operations on 16 threads (tests/image_grid_cases.py: torchvision is not needed)

for 256 code maps of 32 x 32 (decoded in batches of 32) without normalisation, and for the 8-image normalize=True page of
generate_images_once (generate_samples.py:175-199).  The bytes of the two routes are asserted equal.  The decoder is the
same work in both routes; ops.image_grid alone is also timed with device events on the decoder's output.

    python tools/mb_image_grid.py [--images 256] [--batch 32] [--reps 7]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(routes, reps):
    """Alternate the routes `reps` times after one warm-up each; seconds per route, every repetition."""
    out = {k: f() for k, f in routes.items()}
    ts = {k: [] for k in routes}
    for _ in range(reps):
        for k, f in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ts[k].append(time.perf_counter() - t0)
    return out, ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X: nothing here is measured on a CPU"
    from cogview_amd import ops, vqvae
    from tests import image_grid_cases as GC
    torch.set_num_threads(16)
    torch.manual_seed(0)
    model = vqvae.new_model().cuda().eval()
    codes = torch.randint(0, 8192, (args.images, 32, 32), device="cuda")
    res = {"images": args.images}
    for name, code, kw in (("page", list(codes.split(args.batch)), dict(nrow=16)),
                           ("normalize8", [codes[:8]], dict(normalize=True))):
        routes = {"device": lambda: vqvae.code2img_u8(model, code, **kw).cpu(),
                  "host": lambda: GC.grid_bytes(torch.cat([vqvae.code2img(model, c).cpu() for c in code]), **kw)}
        out, ts = timed(routes, args.reps)
        same = bool(torch.equal(out["device"], out["host"]))
        res[name + "_bytes_equal"] = same
        res[name + "_grid"] = list(out["device"].shape)
        for k, t in ts.items():
            res[f"{name}_{k}_ms_median"] = round(1e3 * sorted(t)[len(t) // 2], 2)
            res[f"{name}_{k}_ms_best"] = round(1e3 * min(t), 2)
            print(f"{name:>10} {k:>6}: {1e3 * sorted(t)[len(t) // 2]:9.2f} ms median, {1e3 * min(t):9.2f} ms best of {len(t)}")
        assert same, f"{name}: the two routes gave different bytes"
        # the egress launches alone, on the decoder's output
        imgs = [vqvae.code2img(model, c) for c in code]
        grid = ops.image_grid(imgs, **kw)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
        for a, b in ev:
            a.record()
            ops.image_grid(imgs, out=grid, **kw)
            b.record()
        torch.cuda.synchronize()
        ms = sorted(a.elapsed_time(b) for a, b in ev)[len(ev) // 2]
        nbytes = 4 * sum(i.numel() for i in imgs) * (2 if kw.get("normalize") else 1) + grid.numel()
        res[name + "_image_grid_ms_median"] = round(ms, 4)
        res[name + "_image_grid_gbytes_per_s"] = round(nbytes / ms / 1e6, 1)
        print(f"{name:>10} ops.image_grid alone: {ms:.4f} ms median of {len(ev)}, {nbytes / ms / 1e6:.1f} GB/s of algorithmic bytes")
        del imgs, grid
    print(json.dumps(res))


if __name__ == "__main__":
    main()
