"""Shared by the CPU and GPU tests of the image egress (ops.image_grid, vqvae.code2img_u8 / save_image): torchvision's
make_grid and save_image's byte conversion restated as the literal sequence of torch operations they run, on CPU tensors
(the CPU is the oracle: its div_ is a true division), the case list and the inputs.
Test infrastructure: the package does not import it."""
import itertools
import math

import torch

SHAPES = [(8, 8), (9, 10), (24, 40)]      # W % 4 == 0 (16-byte loads), odd rows with W % 4 != 0, several workgroups
BATCHES = [1, 2, 5, 9]
NROWS = [8, 3]
PADDINGS = [0, 2, 3]
PAD_VALUES = [0.0, 0.5, 1.0]
# keywords of each normalisation; (0, 1) clamps and otherwise leaves the values as they are
MODES = {
    "none": dict(),
    "normalize": dict(normalize=True),
    "range01": dict(normalize=True, value_range=(0.0, 1.0)),
    "range": dict(normalize=True, value_range=(-0.3, 1.7)),
    "range_each": dict(normalize=True, value_range=(0.1, 0.9), scale_each=True),
    "scale_each": dict(normalize=True, scale_each=True),
}


def grid_cases():
    """(B, nrow, padding, pad_value) of every geometry run per shape and mode."""
    return list(itertools.product(BATCHES, NROWS, PADDINGS, PAD_VALUES))


def make_grid(tensor, nrow=8, padding=2, normalize=False, value_range=None, scale_each=False, pad_value=0.0):
    """torchvision.utils.make_grid for a CPU fp32 tensor [B, 3, H, W] (or [3, H, W]), operation by operation."""
    if tensor.dim() == 3:
        tensor = tensor.unsqueeze(0)
    if normalize is True:
        tensor = tensor.clone()

        def norm_ip(img, low, high):
            img.clamp_(min=low, max=high)
            img.sub_(low).div_(max(high - low, 1e-5))

        def norm_range(t, value_range):
            if value_range is not None:
                norm_ip(t, value_range[0], value_range[1])
            else:
                norm_ip(t, float(t.min()), float(t.max()))

        if scale_each is True:
            for t in tensor:
                norm_range(t, value_range)
        else:
            norm_range(tensor, value_range)
    if tensor.size(0) == 1:
        return tensor.squeeze(0)
    nmaps = tensor.size(0)
    xmaps = min(nrow, nmaps)
    ymaps = int(math.ceil(float(nmaps) / xmaps))
    height, width = int(tensor.size(2) + padding), int(tensor.size(3) + padding)
    grid = tensor.new_full((3, height * ymaps + padding, width * xmaps + padding), pad_value)
    k = 0
    for y in range(ymaps):
        for x in range(xmaps):
            if k >= nmaps:
                break
            grid.narrow(1, y * height + padding, height - padding).narrow(2, x * width + padding, width - padding).copy_(tensor[k])
            k = k + 1
    return grid


def grid_bytes(tensor, **kwargs):
    """save_image's array: make_grid, then mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(uint8) -> [GH, GW, 3]."""
    grid = make_grid(tensor, **kwargs)
    return grid.mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8).contiguous()


def replicate(sources, size):
    """A list of CPU sources [n, 3, h, w] brought to `size` as the reference's callers do: F.interpolate in its default
    nearest mode, then one batch."""
    return torch.cat([torch.nn.functional.interpolate(s, size=size) for s in sources])


def images(B, H, W, seed=0):
    """[B, 3, H, W] fp32 on the CPU: normal around 0.5 (so there are values below 0 and above 1), the extremes planted in the
    first and the last element, values (m + 0.5) / 255 in image 0 (x * 255 + 0.5 lands next to an integer, where the order of the roundings shows), and, from
    three images on, image 1 constant (its own range is empty: d = 1e-5)."""
    g = torch.Generator().manual_seed(1000 * seed + 100 * B + H + W)
    x = torch.randn(B, 3, H, W, generator=g) * 0.5 + 0.5
    n = min(255, H * W)
    x[0, 1].view(-1)[:n] = (torch.arange(n, dtype=torch.float32) + 0.5) / 255
    x[0, 2].view(-1)[:n] = (torch.arange(255 - n, 255, dtype=torch.float32) + 0.5) / 255
    if B >= 3:
        x[1] = 0.25
    x.view(-1)[0] = -3.0
    x.view(-1)[-1] = 4.0
    return x
