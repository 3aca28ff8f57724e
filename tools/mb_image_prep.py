"""Images per second from decoded uint8 images to VQ-VAE codes, two routes in one process on the production tokenizer:

  device : vqvae.img2code_raw -- one host-to-device copy of the raw bytes, ops.image_prep, the encoder on its NHWC4 output
  host   : what a user had to do before -- Pillow resize + centre crop + ToTensor + Normalize on 16 threads,
           torch.stack, .cuda(), vqvae.img2code

on 256 random-byte images of mixed sizes.  Both routes give the same codes (checked).  Needs Pillow for the host route.

    python tools/mb_image_prep.py [--images 256] [--reps 5] [--size 256]
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = [(480, 640), (375, 500), (768, 1024), (1200, 800), (256, 256), (500, 333), (1080, 1920), (300, 300)]      # H x W


def host_route(model, imgs, S, pool, mean, std):
    from PIL import Image
    from cogview_amd.vqvae import img2code
    m, sd = torch.tensor(mean).view(3, 1, 1), torch.tensor(std).view(3, 1, 1)

    def one(a):
        H, W = a.shape[:2]
        short, long = (W, H) if W <= H else (H, W)
        nl = int(S * long / short)
        nw, nh = (S, nl) if W <= H else (nl, S)
        img = Image.fromarray(a, "RGB")
        if (nw, nh) != (W, H):
            img = img.resize((nw, nh), Image.BILINEAR)
        top, left = int(round((nh - S) / 2.0)), int(round((nw - S) / 2.0))
        t = torch.from_numpy(np.asarray(img.crop((left, top, left + S, top + S))).copy()).permute(2, 0, 1)
        return t.to(torch.float32).div(255).sub_(m).div_(sd)

    x = torch.stack(list(pool.map(one, imgs))).cuda()
    return img2code(model, x)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", type=int, default=256)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X: nothing here is measured on a CPU"
    from cogview_amd import vqvae
    from cogview_amd.vqvae.api import _MEAN, _STD
    torch.manual_seed(0)
    model = vqvae.new_model().cuda().eval()
    rs = np.random.RandomState(0)
    imgs = [rs.randint(0, 256, size=SIZES[i % len(SIZES)] + (3,)).astype(np.uint8) for i in range(args.images)]
    raw_mb = sum(a.size for a in imgs) / 1e6
    pool = ThreadPoolExecutor(16)
    routes = {"device": lambda: vqvae.img2code_raw(model, imgs, args.size),
              "host": lambda: host_route(model, imgs, args.size, pool, _MEAN, _STD)}
    ids = {k: f() for k, f in routes.items()}                     # warm-up, and the two routes agree
    same = bool(torch.equal(ids["device"], ids["host"]))
    best = {}
    for _ in range(args.reps):                                    # alternate the routes; keep each one's best and all its times
        for k, f in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            best.setdefault(k, []).append(time.perf_counter() - t0)
    res = {"images": args.images, "size": args.size, "raw_megabytes": round(raw_mb, 1), "codes_equal": same}
    for k, ts in best.items():
        res[k + "_images_per_s"] = round(args.images / min(ts), 1)
        res[k + "_images_per_s_median"] = round(args.images / sorted(ts)[len(ts) // 2], 1)
        print(f"{k:>6}: {args.images / min(ts):8.1f} images/s best, {args.images / sorted(ts)[len(ts) // 2]:8.1f} median of {len(ts)}")
    print(json.dumps(res))
    assert same, "the two routes gave different codes"


if __name__ == "__main__":
    main()
