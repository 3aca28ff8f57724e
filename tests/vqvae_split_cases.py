"""Helper (no tests) for the tokenizer's split-bf16 precision mode: the plain-torch restatement of the three-limb split, the
kernel cells with their fp64 references, and the fp32 / fp64 restatement of the one ResBlock topology the whole-model
tests run.  Used by tests/test_vqvae_split_cpu.py and tests/test_vqvae_split_gpu.py."""
import torch
import torch.nn.functional as F

CONV, CONVT, ONE, C3 = "conv", "convT", "1x1", "3x3"
# (kind, B, H, W, Cin, Cout): per kind the smallest shapes at which the kernel takes another path -- Cin = 4 (the image
# layer, k-tiles that straddle taps, K < 32), Cin % 32 == 0 (whole k-tiles inside one tap), channel counts across the 128
# tile edge, pixel counts that are no multiple of 128, several pixel tiles, and the production width (K = 8192).
CELLS = [
    (CONV, 1, 4, 4, 4, 8), (CONV, 2, 6, 10, 8, 40), (CONV, 1, 8, 8, 136, 24), (CONV, 2, 16, 24, 32, 136), (CONV, 1, 16, 16, 512, 512),
    (CONVT, 2, 5, 7, 8, 8), (CONVT, 1, 8, 8, 136, 40), (CONVT, 2, 12, 20, 24, 136),
    (ONE, 1, 4, 4, 16, 8), (ONE, 2, 9, 11, 136, 264),
    (C3, 1, 5, 7, 8, 8), (C3, 2, 9, 11, 40, 136),
]
EPILOGUE_CELLS = [(CONV, 2, 6, 10, 8, 40), (CONVT, 2, 5, 7, 8, 8)]
EPILOGUES = ["relu", "relu_in", "residual", "relu_residual", "no_bias"]
RGB_CELL = (CONVT, 1, 4, 6, 8, 128)
# the second fused-RGB cell: 162 pixels per parity = two pixel tiles, the last one partial (the epilogue's m < M guard), and two
# channel tiles (the partial sums' tile index n0 / 128 = 1)
RGB_CELLS = [RGB_CELL, (CONVT, 2, 9, 9, 8, 256)]
RANGE_CELL = (CONV, 2, 6, 10, 8, 40)
# Relative Frobenius error against fp64 a cell must stay under.  One missing small product (x2y0, x1y1 or x0y2), a
# two-limb kernel or a limb read from the wrong plane reads 2.4e-6 or more; a correct kernel emulated on the CPU at most 1.3e-7.
BOUND = 1e-6


def split3(x):
    """The truncating three-limb split of an fp32 tensor: limbs [3, *x.shape] fp32, each a bf16 value (low 16 bits zero);
    limb 0 = the top 16 bits of x, limb 1 = the top 16 bits of x - limb 0, limb 2 = the top 16 bits of what then remains."""
    assert x.dtype == torch.float32
    out, r = [], x.clone()
    for _ in range(3):
        h = (r.view(torch.int32) & -65536).view(torch.float32)
        out.append(h)
        r = r - h
    return torch.stack(out)


def limb_bits(x):
    """split3 as the int16 planes cogv_conv_split_weights writes."""
    return (split3(x).view(torch.int32) >> 16).to(torch.int16)


def special_values():
    """fp32 values the split must survive: both zeros, 1e-30, 3e38, FLT_MAX, low mantissa bits all ones at several exponents
    and ordinary random numbers.  (Below about 2^-110 the third limb leaves bf16's exponent range and the split stops being
    exact -- bf16 has fp32's exponents but 16 fewer bits under them; such values are not in the list.)"""
    bits = torch.tensor([0x3fffffff, 0x3f80ffff, 0x7f7fffff, 0x0d7fffff, 0x0affffff, 0x4b7fffff, 0x3f7fff01], dtype=torch.int32)
    named = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 3e38, -3e38, 1.0, -1.0, 1.0 / 3.0], dtype=torch.float32)
    g = torch.Generator().manual_seed(0)
    rnd = torch.randn(997, generator=g) * torch.logspace(-20, 20, 997)
    v = torch.cat([named, bits.view(torch.float32), -bits.view(torch.float32), rnd])
    return torch.cat([v, torch.zeros((-v.numel()) % 4)])              # a multiple of 4 elements


def make_cell(kind, B, H, W, Cin, Cout, scale=1.0, seed_extra=0):
    """dict(x NCHW, w (torch layout), bias, res (output-shaped), w_rgb [3, Cout], b_rgb [3]) of fp32 CPU tensors.  Inputs are
    signed; weights ~ 1 / sqrt(K), so outputs are O(1) * scale."""
    g = torch.Generator().manual_seed(B * 1000 + H * 100 + Cin * 10 + Cout + seed_extra)
    x = torch.randn(B, Cin, H, W, generator=g) * scale
    if Cin == 4:
        x[:, 3] = 0                                           # the image layer: channel 3 is padding
    taps = {CONV: 16, CONVT: 4, ONE: 1, C3: 9}[kind]
    ks = {CONV: 4, CONVT: 4, ONE: 1, C3: 3}[kind]
    shape = (Cin, Cout, ks, ks) if kind == CONVT else (Cout, Cin, ks, ks)
    w = torch.randn(shape, generator=g) / (taps * Cin) ** 0.5
    bias = torch.randn(Cout, generator=g) * 0.1 * scale
    c = dict(kind=kind, x=x, w=w, bias=bias)
    c["res"] = torch.randn(conv64(c, x.double(), bias=None).shape, generator=g) * scale
    c["w_rgb"] = torch.randn(3, Cout, generator=g) / Cout ** 0.5
    c["b_rgb"] = torch.randn(3, generator=g) * 0.1
    return c


def conv64(c, x64, bias="own"):
    """The cell's convolution in fp64 on the CPU: F.conv2d / F.conv_transpose2d, NCHW."""
    w = c["w"].double()
    b = c["bias"].double() if bias == "own" else None
    if c["kind"] == CONV:
        return F.conv2d(x64, w, b, stride=2, padding=1)
    if c["kind"] == CONVT:
        return F.conv_transpose2d(x64, w, b, stride=2, padding=1)
    if c["kind"] == C3:
        return F.conv2d(x64, w, b, padding=1)
    return F.conv2d(x64, w, b)


def reference(c, epilogue=None):
    """fp64 NCHW result of the cell with one of EPILOGUES (None: bias only)."""
    x = c["x"].double()
    if epilogue == "relu_in":
        x = F.relu(x)
    y = conv64(c, x, bias=None if epilogue == "no_bias" else "own")
    if epilogue == "relu":
        y = F.relu(y)
    if epilogue == "residual":
        y = y + c["res"].double()
    if epilogue == "relu_residual":
        y = y + F.relu(c["res"].double())
    return y


def reference_rgb(c, scale, shift):
    """fp64: ReLU(cell) -> 1x1 to RGB -> * scale + shift (the decoder's last two layers and api.code2img's de-normalisation)."""
    y = F.relu(conv64(c, c["x"].double()))
    img = F.conv2d(y, c["w_rgb"].double().view(3, -1, 1, 1), c["b_rgb"].double())
    return img * torch.tensor(scale, dtype=torch.float64).view(1, 3, 1, 1) + torch.tensor(shift, dtype=torch.float64).view(1, 3, 1, 1)


def kernel_kind(kind):
    from cogview_amd import _lib as L
    return {CONV: L.CONV_4X4_S2, CONVT: L.CONVT_4X4_S2, ONE: L.CONV_1X1, C3: L.CONV_3X3_S1}[kind]


def packed_weight(c):
    from cogview_amd.vqvae.vqvae_zc import pack_conv_weight, pack_convt_weight
    return (pack_convt_weight if c["kind"] == CONVT else pack_conv_weight)(c["w"])


def run_cell(c, dev, precision, epilogue=None, rgb=None):
    """The cell on the device through vqvae_zc._conv -> NCHW on the CPU.  dev: dict of the cell's device tensors (device_cell)."""
    from cogview_amd.vqvae.vqvae_zc import _conv
    cout = c["bias"].numel()
    kw = dict(precision=precision, w_limbs=dev["limbs"] if precision == "bf16x3" else None)
    bias = None if epilogue == "no_bias" else dev["bias"]
    if rgb is not None:
        return _conv(kernel_kind(c["kind"]), dev["x"], dev["w"], bias, cout, True, rgb=(dev["w_rgb"], dev["b_rgb"]) + tuple(rgb), **kw).cpu()
    if epilogue in ("residual", "relu_residual"):
        kw.update(residual=dev["res"], relu_residual=epilogue == "relu_residual")
    y = _conv(kernel_kind(c["kind"]), dev["x"], dev["w"], bias, cout, epilogue == "relu", relu_in=epilogue == "relu_in", **kw)
    return y.permute(0, 3, 1, 2).cpu()


def device_cell(c):
    from cogview_amd.vqvae.vqvae_zc import split_weight_limbs
    wp = packed_weight(c).cuda()
    return dict(x=c["x"].permute(0, 2, 3, 1).contiguous().cuda(), w=wp, limbs=split_weight_limbs(wp), bias=c["bias"].cuda(),
                res=c["res"].permute(0, 2, 3, 1).contiguous().cuda(), w_rgb=c["w_rgb"].contiguous().cuda(), b_rgb=c["b_rgb"].cuda())


# ---- the ResBlock topology of the whole-model tests: VQVAE(channel=32, n_res_block=2, n_res_channel=16, embed_dim=16,
# n_embed=64, stride=4), restated in plain torch in the dtype of `p` (state-dict keys as the module's)
RES_CONFIG = dict(channel=32, n_res_block=2, n_res_channel=16, embed_dim=16, n_embed=64, stride=4)


def _res_block(p, prefix, x):
    """vqvae/vqvae_zc.py:99-114: the leading in-place ReLU overwrites the input, so the block adds back relu(input)."""
    r = F.relu(x)
    t = F.relu(F.conv2d(r, p[prefix + ".conv.1.weight"], p[prefix + ".conv.1.bias"], padding=1))
    return F.conv2d(t, p[prefix + ".conv.3.weight"], p[prefix + ".conv.3.bias"]) + r


def res_encoder(p, img):
    """Encoder(stride=4, n_res_block=2): conv4x4s2, ReLU, conv4x4s2, ReLU, conv3x3, ResBlock x 2, ReLU, conv1x1 -> NHWC."""
    x = F.relu(F.conv2d(img, p["enc_b.blocks.0.weight"], p["enc_b.blocks.0.bias"], stride=2, padding=1))
    x = F.relu(F.conv2d(x, p["enc_b.blocks.2.weight"], p["enc_b.blocks.2.bias"], stride=2, padding=1))
    x = F.conv2d(x, p["enc_b.blocks.4.weight"], p["enc_b.blocks.4.bias"], padding=1)
    x = _res_block(p, "enc_b.blocks.5", x)
    x = _res_block(p, "enc_b.blocks.6", x)
    return F.conv2d(F.relu(x), p["enc_b.blocks.8.weight"], p["enc_b.blocks.8.bias"]).permute(0, 2, 3, 1)


def res_decoder(p, q_nhwc):
    """Decoder(stride=2, n_res_block=2): convT4x4s2, ResBlock x 2, ReLU, convT4x4s2 -> NCHW image."""
    x = F.conv_transpose2d(q_nhwc.permute(0, 3, 1, 2), p["dec.blocks.0.weight"], p["dec.blocks.0.bias"], stride=2, padding=1)
    x = _res_block(p, "dec.blocks.1", x)
    x = _res_block(p, "dec.blocks.2", x)
    return F.conv_transpose2d(F.relu(x), p["dec.blocks.4.weight"], p["dec.blocks.4.bias"], stride=2, padding=1)
