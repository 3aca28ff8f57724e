"""Shared by the CPU and GPU tests of the tokenizer ingest (ops.image_prep, ops.sr_patches): a numpy restatement of what
transforms.Resize(S) + CenterCrop(S) do to a PIL image (Pillow's Image.resize(BILINEAR), then the crop), the stored
Pillow results it is checked against, and torch restatements of the float stage and of the super-resolution crops.
Test infrastructure: the package does not import it."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_prep.npz")
GOLDEN_S = 16
# H x W of the stored images (tools/gen_image_prep_golden.py): downscale, upscale, one axis unchanged, nothing to do,
# half-even crop offsets on either axis, extreme aspect
GOLDEN_SHAPES = [(37, 53), (53, 37), (16, 16), (9, 40), (17, 16), (20, 20), (13, 29), (100, 64), (150, 259), (511, 33)]
PRECISION_BITS = 22


def target_size(H, W, S):
    """(new H, new W) of transforms.Resize(S): short side S, long side int(S * long / short)."""
    short, long = (W, H) if W <= H else (H, W)
    new_long = int(S * long / short)
    return (new_long, S) if W <= H else (S, new_long)


def crop_offset(n, S):
    """transforms.CenterCrop: round((n - S) / 2.0), Python's round (half to even)."""
    return int(round((n - S) / 2.0))


def axis_coeffs(n_in, n_out):
    """[(xmin, int weights)] per output index of one axis, or None where the axis keeps its size (a copy)."""
    if n_in == n_out:
        return None
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = fs
    out = []
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in)
        w = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) / fs)) for x in range(xmax - xmin)]
        ww = 0.0
        for v in w:
            ww += v
        out.append((xmin, np.array([int(v / ww * (1 << PRECISION_BITS) + 0.5) for v in w], dtype=np.int64)))
    return out


def apply_axis(img, coeffs, axis, first=0, n=None):
    """One pass along `axis` (0: vertical, 1: horizontal) of a uint8 [H, W, 3] image with integer tables [(xmin, k)],
    outputs first .. first + n only; rounded to uint8 as Pillow rounds each pass."""
    n = len(coeffs) - first if n is None else n
    src = np.moveaxis(img.astype(np.int64), axis, 0)
    out = np.empty((n,) + src.shape[1:], dtype=np.uint8)
    for i in range(n):
        xmin, k = coeffs[first + i]
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(k, src[xmin:xmin + len(k)], axes=(0, 0))
        out[i] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def pil_bilinear_u8(img, S):
    """uint8 [H, W, 3] -> uint8 [S, S, 3]: Resize(S) then CenterCrop(S) as torchvision does them on a PIL image.  Horizontal
    pass first, rounded to uint8, then the vertical pass; only the crop's rows and columns are computed."""
    img = np.asarray(img)
    H, W = img.shape[:2]
    nh, nw = target_size(H, W, S)
    top, left = crop_offset(nh, S), crop_offset(nw, S)
    ch, cv = axis_coeffs(W, nw), axis_coeffs(H, nh)
    img = img[:, left:left + S] if ch is None else apply_axis(img, ch, 1, left, S)
    return img[top:top + S] if cv is None else apply_axis(img, cv, 0, top, S)


def tables_from_library(xmin, count, k):
    """cogv_resample_coeffs' arrays in axis_coeffs' form."""
    return [(int(xmin[i]), k[i, :count[i]].astype(np.int64)) for i in range(len(xmin))]


def golden():
    """[(source uint8 [H, W, 3], Pillow's uint8 [16, 16, 3])] in GOLDEN_SHAPES order."""
    z = np.load(GOLDEN)
    return [(z["src%d" % i], z["out%d" % i]) for i in range(len(GOLDEN_SHAPES))]


def lut_reference(u8, mean, std):
    """ToTensor + Normalize of uint8 [..., 3] in torch fp32, channel last: ((u / 255) - mean) / std."""
    import torch
    x = torch.as_tensor(np.ascontiguousarray(u8)).to(torch.float32).div(255)
    return x.sub(torch.tensor(mean, dtype=torch.float32)).div(torch.tensor(std, dtype=torch.float32))


def sr_patches_reference(x4, positions):
    """torch restatement of ops.sr_patches on [b, S, S, 4] (preprocess/pretokenized_data.py:100-124)."""
    import torch
    b, S = x4.shape[0], x4.shape[1]
    t0, t1 = S // 4, S // 2
    pw, ph = [0, t0, t1] * 3, [0, 0, 0, t0, t0, t0, t1, t1, t1]
    patches = torch.stack([x4[i, ph[p]:ph[p] + t1, pw[p]:pw[p] + t1] for i in range(b) for p in positions])
    overview = torch.nn.functional.interpolate(x4.permute(0, 3, 1, 2), size=(t1, t1), mode='bilinear').permute(0, 2, 3, 1)
    return patches.contiguous(), overview.contiguous()
