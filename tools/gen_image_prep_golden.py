"""Write tests/golden/image_prep.npz: random-byte RGB images and what Pillow makes of them under
transforms.Resize(16) + CenterCrop(16) (Image.resize((nw, nh), Image.BILINEAR), then the crop), the fixture that pins
ops.image_prep's uint8 stage to Pillow byte for byte.  Needs Pillow and numpy only.

    python tools/gen_image_prep_golden.py
"""
import os

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 16
SHAPES = [(37, 53), (53, 37), (16, 16), (9, 40), (17, 16), (20, 20), (13, 29), (100, 64), (150, 259), (511, 33)]      # H x W


def resize_crop(arr, S):
    """torchvision's Resize(S) and CenterCrop(S) on a PIL image, spelled out."""
    H, W = arr.shape[:2]
    short, long = (W, H) if W <= H else (H, W)
    new_long = int(S * long / short)
    nw, nh = (S, new_long) if W <= H else (new_long, S)
    img = Image.fromarray(arr, "RGB")
    if (nw, nh) != (W, H):
        img = img.resize((nw, nh), Image.BILINEAR)
    top, left = int(round((nh - S) / 2.0)), int(round((nw - S) / 2.0))
    return np.asarray(img.crop((left, top, left + S, top + S)))


def main():
    rs = np.random.RandomState(20260)
    out = {}
    for i, (H, W) in enumerate(SHAPES):
        src = rs.randint(0, 256, size=(H, W, 3)).astype(np.uint8)
        out["src%d" % i] = src
        out["out%d" % i] = resize_crop(src, S)
    path = os.path.join(ROOT, "tests", "golden", "image_prep.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
