"""VQ-VAE image tokenizer: module surface of vqvae/vqvae_zc.py (class names, constructor arguments,
state_dict keys: enc_b.blocks.{0,2,4,6}.*, quantize_t.{embed,cluster_size,embed_avg}, dec.blocks.{0,2,4,6}.*),
inference arithmetic in the HIP library (cogview_amd/csrc/conv.hip).

Scope: the frozen tokenizer as CogView uses it (vqvae/api.py: img2code / code2img, eval mode).  The production topology
-- stride=6, simple=True, n_res_block=0: three 4x4 stride-2 convolutions + 1x1, nearest-code search, three 4x4 stride-2
transposed convolutions + 1x1 -- runs the fused fast path (final 1x1 -> RGB in the last transposed convolution's epilogue).
Every OTHER topology the reference's constructors can build (vqvae/vqvae_zc.py:116-214: stride 6 / 4 / 2, simple or not,
any number of ResBlocks) runs through a generic interpreter of the same block list on the same kernels (round 4: 3x3
convolution, input ReLU and residual add in the convolution kernel) -- channel counts a multiple of 8.

Precision (eval mode only): VQVAE.set_precision("bf16x3") runs every convolution of both stacks -- fast path and interpreter --
on the split-bf16 kernel (cogview_amd/csrc/conv_split.hip: three bf16 limbs per fp32 operand, six products, fp32 accumulation);
the default "fp32" is the exact-fp32 kernel.  The nearest-code search, the embedding lookup and every training launch are the
same exact-fp32 code in both modes.

Training (module.train(), vqvae/vqvae_zc.py:67-86): the default, non-relaxed path of every topology made of 4x4 stride-2
convolutions, 4x4 stride-2 transposed convolutions, 1x1 convolutions and ReLU (new_model() and every n_res_block=0 stride-6
configuration).  The stacks run layer by layer, each layer a torch.autograd.Function on the kernels of
cogview_amd/csrc/conv.hip (forward, data gradient) and conv_bwd.hip (weight gradient, ReLU mask + bias gradient, codebook
statistics, EMA update, straight-through gradient).

Every other topology trains after an opt-in, VQVAE.set_train_topologies("all") (a later change makes it the default): VQVAE()
with its own default arguments, the stride-4 and stride-2 encoders (they end in a 3x3 convolution) and any n_res_block > 0.
A 3x3 convolution is a layer like the others (weight gradient: conv_bwd.hip with topologies=1; data gradient: the 3x3
forward kernel on the weight with in / out swapped and both tap axes flipped).  A ResBlock is ONE autograd.Function
(_ResBlockLayer): the two launches of run_block_list forward, and backward the 1x1 pair, the ReLU mask, the 3x3 weight
gradient against max(x, 0) (relu_x=1), the 3x3 data gradient with the skip connection's gradient added in its residual
epilogue, and the gate of the block's leading in-place ReLU.  A convolution behind the ReLU that closes a ResBlock chain runs
with relu_in, keeps its pre-ReLU input, and gates its data gradient the same way.  What still raises NotImplementedError in
training mode: without the opt-in, ResBlock topologies and 3x3 convolutions, exactly as before; with or without it,
continuous_relax=True (the Gumbel-softmax branch), in any mode.
"""
import ctypes as C

import torch
from torch import nn

from .. import _lib as L
from .. import ops


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


PRECISIONS = ("fp32", "bf16x3")
TRAIN_TOPOLOGIES = ("plain", "all")


def split_weight_limbs(wp):
    """The three bf16 limb planes of a packed fp32 weight (cogv_conv_split_weights): int16 [3, *wp.shape], plane 0 the most
    significant; the planes sum back to wp bit for bit.  What _conv(precision="bf16x3") reads instead of wp."""
    if not wp.is_cuda:
        raise L.CogviewHipError("cogview_amd.vqvae runs only on an MI355X (HIP) device; there is no CPU fallback")
    wp = wp.contiguous()
    limbs = torch.empty((3,) + tuple(wp.shape), dtype=torch.int16, device=wp.device)
    L.check(L.lib().cogv_conv_split_weights(_p(wp), _p(limbs), wp.numel(), _stream()), "cogv_conv_split_weights")
    return limbs


def _conv(kind, x, w, bias, cout, relu, rgb=None, relu_in=False, residual=None, relu_residual=False, precision="fp32",
          w_limbs=None):
    """x NHWC fp32 contiguous -> NHWC fp32.  rgb = (w_rgb [3, cout], bias_rgb [3], scale, shift): the decoder's final
    1x1 convolution (and the de-normalisation of api.code2img) fused into this layer's epilogue -- the layer's own
    output tensor is never written; returns the NCHW image [b, 3, oh, ow].
    precision: "fp32" (the exact-fp32 kernel; w_limbs ignored) or "bf16x3" (the split-bf16 kernel on w_limbs =
    split_weight_limbs(w): fp32-class accuracy, not the exact path's bits).  The fused RGB projection's own arithmetic and
    rgb_finalize are the same fp32 code in both."""
    if precision not in PRECISIONS:
        raise ValueError(f"precision must be one of {PRECISIONS}, not {precision!r}")
    if precision == "bf16x3" and w_limbs is None:
        raise ValueError('precision="bf16x3" needs w_limbs (split_weight_limbs of the packed weight)')
    if not x.is_cuda:
        raise L.CogviewHipError("cogview_amd.vqvae runs only on an MI355X (HIP) device; there is no CPU fallback")
    b, ih, iw, cin = x.shape
    if kind == L.CONV_4X4_S2:
        oh, ow = ih // 2, iw // 2
    elif kind == L.CONVT_4X4_S2:
        oh, ow = ih * 2, iw * 2
    else:
        oh, ow = ih, iw
    d = L.ConvDesc()
    d.kind, d.B, d.IH, d.IW, d.Cin, d.Cout, d.relu = kind, b, ih, iw, cin, cout, int(relu)
    d.relu_in, d.relu_residual = int(relu_in), int(relu_residual)
    if residual is not None:
        assert residual.shape == (b, oh, ow, cout) and residual.is_contiguous() and rgb is None
        d.residual = residual.data_ptr()
    setattr(d, "in", x.data_ptr())
    d.w, d.bias = w.data_ptr(), (None if bias is None else bias.data_ptr())      # no bias: the data gradient of a layer
    if precision == "bf16x3":
        assert w_limbs.shape == (3,) + tuple(w.shape) and w_limbs.dtype == torch.int16 and w_limbs.is_contiguous()
        d.precision, d.w_limbs = L.CONV_BF16X3, w_limbs.data_ptr()
    if rgb is None:
        out = torch.empty((b, oh, ow, cout), dtype=torch.float32, device=x.device)
        d.out = out.data_ptr()
    else:
        ntiles = cout // 128
        out = torch.empty((ntiles, b * oh * ow, 4), dtype=torch.float32, device=x.device)
        d.rgb_w, d.rgb_partial = rgb[0].data_ptr(), out.data_ptr()
    par = 4 if kind == L.CONVT_4X4_S2 else 1
    taps = {L.CONV_4X4_S2: 16, L.CONV_1X1: 1, L.CONVT_4X4_S2: 4, L.CONV_3X3_S1: 9}[kind]
    npix_out = b * oh * ow
    with ops.timed_launch("conv", 2.0 * npix_out * cout * taps * cin, 4.0 * (x.numel() + w.numel() + out.numel()),
                          f"kind{kind} {b}x{ih}x{iw}x{cin}->{cout}" + (" bf16x3" if precision == "bf16x3" else "")):
        L.check(L.lib().cogv_conv2d_nhwc_f32(C.byref(d), _stream()), "cogv_conv2d_nhwc_f32")
    if rgb is not None:
        img = torch.empty((b, 3, oh, ow), dtype=torch.float32, device=x.device)
        sc = (C.c_float * 3)(*rgb[2]) if rgb[2] is not None else None
        sh = (C.c_float * 3)(*rgb[3]) if rgb[3] is not None else None
        with ops.timed_launch("rgb_finalize", 0.0, 4.0 * (out.numel() + img.numel()), f"{b}x{oh}x{ow}"):
            L.check(L.lib().cogv_rgb_finalize_f32(_p(out), cout // 128, _p(rgb[1]), _p(img), b, oh, ow, sc, sh, _stream()),
                    "cogv_rgb_finalize_f32")
        return img
    return out


def pack_conv_weight(w):
    """Conv2d weight [Cout, Cin, kh, kw] -> [Cout, kh*kw, Cin4] (Cin padded to a multiple of 4)."""
    co, ci, kh, kw = w.shape
    ci4 = (ci + 3) // 4 * 4
    out = torch.zeros((co, kh * kw, ci4), dtype=torch.float32, device=w.device)
    out[:, :, :ci] = w.detach().float().permute(0, 2, 3, 1).reshape(co, kh * kw, ci)
    return out.contiguous()


def pack_convt_weight(w):
    """ConvTranspose2d weight [Cin, Cout, 4, 4] (stride 2, pad 1) -> [4 parities][Cout][4 taps][Cin]:
    output pixel (2y+py, 2x+px) = sum over taps (ty,tx) of in[y+offy, x+offx] with ky = 2*ty (py=1) or 1+2*ty (py=0)."""
    ci, co, kh, kw = w.shape
    assert kh == 4 and kw == 4
    wf = w.detach().float()
    out = torch.empty((4, co, 4, ci), dtype=torch.float32, device=w.device)
    for py in range(2):
        for px in range(2):
            for ty in range(2):
                for tx in range(2):
                    ky = 2 * ty if py else 1 + 2 * ty
                    kx = 2 * tx if px else 1 + 2 * tx
                    out[py * 2 + px, :, ty * 2 + tx, :] = wf[:, :, ky, kx].t()
    return out.contiguous()


def _convt_taps():
    """(parity, tap, ky, kx) of pack_convt_weight's layout: every (ky, kx) of the 4x4 kernel occurs exactly once."""
    for py in range(2):
        for px in range(2):
            for ty in range(2):
                for tx in range(2):
                    yield py * 2 + px, ty * 2 + tx, (2 * ty if py else 1 + 2 * ty), (2 * tx if px else 1 + 2 * tx)


def unpack_conv_weight_grad(dwp, shape):
    """Inverse of pack_conv_weight for a weight gradient: packed [Cout', kh*kw, Cin'] (channels possibly padded) -> the
    Conv2d parameter's layout `shape` = [Cout, Cin, kh, kw]; the padding is dropped."""
    co, ci, kh, kw = shape
    return dwp[:co, :, :ci].reshape(co, kh, kw, ci).permute(0, 3, 1, 2).contiguous()


def unpack_convt_weight_grad(dwp, shape):
    """Inverse of pack_convt_weight for a weight gradient: packed [4, Cout', 4, Cin'] -> the ConvTranspose2d parameter's
    layout `shape` = [Cin, Cout, 4, 4]; the padding is dropped."""
    ci, co, kh, kw = shape
    assert kh == 4 and kw == 4
    out = torch.empty(tuple(shape), dtype=dwp.dtype, device=dwp.device)
    for z, t, ky, kx in _convt_taps():
        out[:, :, ky, kx] = dwp[z, :co, t, :ci].t()
    return out


class _StraightThrough(torch.autograd.Function):
    """(quantize, diff) of vqvae/vqvae_zc.py:85-86 with their graph: diff = (q - x)^2 .mean(), and the straight-through
    output, whose VALUE is the lookup q itself (the reference's x + (q - x) is q up to one rounding; returning q keeps the
    decoder's input bit-identical to the frozen-codebook path).  Backward: one launch, g_q + g_diff * 2 (x - q) / numel."""

    @staticmethod
    def forward(ctx, x, q):
        ctx.save_for_backward(x, q)
        return q.view_as(q), (q - x).pow(2).mean()

    @staticmethod
    def backward(ctx, g_q, g_diff):
        x, q = ctx.saved_tensors
        return ops.vq_ste_bwd(g_q, None if g_diff is None else g_diff.reshape(1).contiguous(), x, q), None


class Quantize(nn.Module):
    """Codebook holder (vqvae/vqvae_zc.py:26-96).  `embed` is [dim, n_embed] as in the reference."""

    def __init__(self, dim, n_embed, decay=0.99, eps=1e-5):
        super().__init__()
        self.dim, self.n_embed, self.decay, self.eps = dim, n_embed, decay, eps
        embed = torch.randn(dim, n_embed)
        torch.nn.init.xavier_uniform_(embed, gain=torch.nn.init.calculate_gain('tanh'))
        self.register_buffer("embed", embed)
        self.register_buffer("cluster_size", torch.zeros(n_embed))
        self.register_buffer("embed_avg", embed.clone())
        self._cache = None

    def _tables(self):
        """E^T [n_embed, dim] and |E_j|^2, rebuilt when the buffer changes (one-time set-up, not the hot path)."""
        key = (self.embed.data_ptr(), self.embed._version)
        if self._cache is None or self._cache[0] != key:
            et = self.embed.detach().float().t().contiguous()
            e2 = self.embed.detach().float().pow(2).sum(0).contiguous()       # vqvae_zc.py:46 `embed.pow(2).sum(0)`
            self._cache = (key, et, e2)
        return self._cache[1], self._cache[2]

    def nearest_code(self, x_nhwc):
        """x [b, h, w, dim] fp32 -> ids [b, h, w] int64 (argmax of -dist, first maximum)."""
        et, e2 = self._tables()
        flat = x_nhwc.reshape(-1, self.dim)
        ids = torch.empty(flat.shape[0], dtype=torch.int64, device=flat.device)
        with ops.timed_launch("vq_argmin", 2.0 * flat.shape[0] * self.dim * self.n_embed,
                              4.0 * (flat.numel() + et.numel()) + 8.0 * flat.shape[0], f"{flat.shape[0]}x{self.dim}x{self.n_embed}"):
            L.check(L.lib().cogv_vq_argmin_f32(_p(flat), _p(et), _p(e2), _p(ids), flat.shape[0], self.dim, self.n_embed,
                                               _stream()), "cogv_vq_argmin_f32")
        return ids.view(*x_nhwc.shape[:-1])

    def embed_code(self, embed_id):
        """F.embedding(ids, embed^T) -> [..., dim] (vqvae/vqvae_zc.py:95-96)."""
        et, _ = self._tables()
        ids = embed_id.contiguous()
        out = torch.empty(tuple(ids.shape) + (self.dim,), dtype=torch.float32, device=et.device)
        L.check(L.lib().cogv_embed_code_f32(_p(ids), _p(et), _p(out), ids.numel(), self.dim, self.n_embed, _stream()),
                "cogv_embed_code_f32")
        return out

    def forward_(self, input, continuous_relax=False, temperature=1., hard=False):
        if continuous_relax:
            raise NotImplementedError("continuous_relax=True: the Gumbel-softmax branch of Quantize.forward_ (vqvae/vqvae_zc.py:55-65, "
                                      ":88-92) is not implemented; only argmax + lookup is")
        x = input.contiguous()
        ids = self.nearest_code(x.detach())
        quantize = self.embed_code(ids)                  # from the codebook BEFORE the update, as in the reference
        if self.training:
            self.ema_update(x.detach(), ids)
        if torch.is_grad_enabled() and x.requires_grad:
            quantize, diff = _StraightThrough.apply(x, quantize)
        else:
            diff = (quantize - input).pow(2).mean()
        return quantize, diff, ids

    def invalidate_cache(self):
        """Forget E^T / |E|^2: they are keyed on embed._version, which a write through the buffer's storage (the EMA kernels,
        the reference-style embed.data.copy_) does not advance."""
        self._cache = None

    def ema_update(self, x_nhwc, ids):
        """The training branch of vqvae/vqvae_zc.py:67-83 on the device: per-code pixel count and vector sum (inverted index,
        no one-hot product), then cluster_size / embed_avg decay, Laplace smoothing and the new embed, in place."""
        with torch.no_grad():
            flat = x_nhwc.reshape(-1, self.dim)
            count, total = ops.vq_code_stats(ids.reshape(-1), flat, self.n_embed)
            ops.vq_ema_update(count, total, self.cluster_size, self.embed_avg, self.embed, self.decay, self.eps)
        self.invalidate_cache()


class _ConvStack(nn.Module):
    def __init__(self, blocks):
        super().__init__()
        self.blocks = nn.Sequential(*blocks)
        self._packed = None
        self._precision = "fp32"          # VQVAE.set_precision; eval-mode launches only
        self._train_topologies = "plain"  # VQVAE.set_train_topologies; training-mode launches only

    def _weights(self, packers):
        key = tuple((m.weight.data_ptr(), m.weight._version) for m in self.blocks if hasattr(m, "weight"))
        if self._packed is None or self._packed[0] != key:
            mods = [m for m in self.blocks if hasattr(m, "weight")]
            self._packed = (key, [(pk(m.weight), m.bias.detach().float().contiguous()) for pk, m in zip(packers, mods)], None)
        return self._packed[1]

    def _limbs(self, packers, n):
        """split_weight_limbs of the first n packed weights of _weights(packers) (None in "fp32" mode).  They live in the
        same cache entry under the same key: a weight update drops both."""
        packed = self._weights(packers)
        if self._precision != "bf16x3":
            return [None] * n
        if self._packed[2] is None:
            self._packed = self._packed[:2] + ([split_weight_limbs(w) for w, _ in packed[:n]],)
        return self._packed[2]


class ResBlock(nn.Module):
    """vqvae/vqvae_zc.py:99-114: ReLU(inplace), conv3x3, ReLU(inplace), conv1x1, `out += input`.  The leading in-place ReLU
    overwrites the block's input before it is added back, so the block computes conv(...) + relu(input)."""

    def __init__(self, in_channel, channel):
        super().__init__()
        self.conv = nn.Sequential(nn.ReLU(inplace=True), nn.Conv2d(in_channel, channel, 3, padding=1), nn.ReLU(inplace=True),
                                  nn.Conv2d(channel, in_channel, 1))


def _pad8(n):
    return (n + 7) // 8 * 8


def _pack_generic(m):
    """(kind, packed weight [.., Cout8, taps, Cin4], bias [Cout8], Cout) of one convolution module; output channels are padded
    to a multiple of 8 with zero filters (the kernel's 8-wide output vectors), input channels to a multiple of 4."""
    w = m.weight.detach().float()
    if isinstance(m, nn.ConvTranspose2d):
        if m.kernel_size == (1, 1):                       # a 1x1 transposed convolution is a 1x1 convolution with W^T
            kind, wp = L.CONV_1X1, pack_conv_weight(w.permute(1, 0, 2, 3))
        else:
            assert m.kernel_size == (4, 4) and m.stride == (2, 2) and m.padding == (1, 1)
            kind, wp = L.CONVT_4X4_S2, pack_convt_weight(w)
            if wp.shape[3] % 4:
                wp = torch.nn.functional.pad(wp, (0, 4 - wp.shape[3] % 4))
    else:
        ks, st, pd = m.kernel_size, m.stride, m.padding
        if ks == (4, 4) and st == (2, 2) and pd == (1, 1):
            kind = L.CONV_4X4_S2
        elif ks == (3, 3) and st == (1, 1) and pd == (1, 1):
            kind = L.CONV_3X3_S1
        elif ks == (1, 1) and st == (1, 1) and pd == (0, 0):
            kind = L.CONV_1X1
        else:
            raise NotImplementedError(f"convolution {ks} stride {st} padding {pd} does not occur in vqvae/vqvae_zc.py")
        wp = pack_conv_weight(w)
    cout = m.out_channels
    cdim = 1 if kind == L.CONVT_4X4_S2 else 0
    if cout % 8:
        pad = [0, 0] * (wp.dim() - 1 - cdim) + [0, _pad8(cout) - cout]
        wp = torch.nn.functional.pad(wp, pad)
    bias = torch.zeros(_pad8(cout), dtype=torch.float32, device=w.device)
    bias[:cout] = m.bias.detach().float()
    return kind, wp.contiguous(), bias, cout


def run_block_list(blocks, x, cache, precision="fp32"):
    """Interpret an nn.Sequential of the reference's block vocabulary (Conv2d 4x4s2 / 3x3 / 1x1, ConvTranspose2d 4x4s2 / 1x1,
    ReLU, ResBlock) on NHWC fp32 activations.  A ReLU that follows a convolution rides in that convolution's epilogue; a
    ReLU that follows a ResBlock (or opens one) is applied to the input of the next convolution inside the kernel.  Padded
    output channels (zero filters) are carried as zeros and ignored by the next layer's zero-padded input channels.
    precision="bf16x3" runs every convolution on the split-bf16 kernel; the limb planes are made on first use and kept in
    the cache entry of the packed weight they were made from."""
    mods = list(blocks)
    relu_pending = False
    i = 0

    def conv(m, x, relu_out, relu_in, residual=None, relu_residual=False):
        key = (id(m), x.shape[-1])
        ver = (m.weight.data_ptr(), m.weight._version, m.bias._version)
        if key not in cache or cache[key][0] != ver:
            kind, wp, bias, _ = _pack_generic(m)
            if x.shape[-1] > wp.shape[-1]:               # the previous layer's zero-padded output channels: zero weights for them
                wp = torch.nn.functional.pad(wp, (0, x.shape[-1] - wp.shape[-1])).contiguous()
            cache[key] = (ver, (kind, wp, bias), None)
        kind, wp, bias = cache[key][1]
        limbs = None
        if precision == "bf16x3":
            if cache[key][2] is None:
                cache[key] = cache[key][:2] + (split_weight_limbs(wp),)
            limbs = cache[key][2]
        if x.shape[-1] < wp.shape[-1]:
            x = torch.nn.functional.pad(x, (0, wp.shape[-1] - x.shape[-1]))
        return _conv(kind, x, wp, bias, bias.numel(), relu_out, relu_in=relu_in, residual=residual, relu_residual=relu_residual,
                     precision=precision, w_limbs=limbs)

    while i < len(mods):
        m = mods[i]
        if isinstance(m, nn.ReLU):
            relu_pending = True
            i += 1
        elif isinstance(m, ResBlock):
            c3, c1 = m.conv[1], m.conv[3]
            t = conv(c3, x, True, True)                  # leading ReLU on the input, second ReLU in the epilogue
            x = conv(c1, t, False, False, residual=x, relu_residual=True)      # + relu(input): the in-place ReLU's doing
            relu_pending = False                         # (a ReLU pending from before the block is subsumed by the block's own)
            i += 1
        else:
            fuse = i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU)
            x = conv(m, x, fuse, relu_pending)
            relu_pending = False
            i += 2 if fuse else 1
    if relu_pending:
        x = torch.relu(x)
    return x


def _dgrad_weight(m, kind, cin_x, cout_p):
    """(kind, packed weight) of the layer that computes the DATA gradient of convolution module m (forward kind `kind`): it
    reads the cout_p channels of the output gradient and writes the cin_x channels of the input gradient.
      Conv2d k4 s2 p1, W [Cout, Cin, 4, 4]          -> transposed convolution whose [in, out, 4, 4] weight is W itself
      ConvTranspose2d k4 s2 p1, W [Cin, Cout, 4, 4] -> convolution whose [out, in, 4, 4] weight is W itself
      1x1                                            -> 1x1 with the transposed matrix
      Conv2d k3 s1 p1, W [Cout, Cin, 3, 3]          -> 3x3 convolution whose [out, in, 3, 3] weight is W with in and out
                                                        swapped and both tap axes flipped"""
    w = m.weight.detach().float()
    if kind == L.CONV_4X4_S2:
        k2, wp = L.CONVT_4X4_S2, pack_convt_weight(w)
    elif kind == L.CONVT_4X4_S2:
        k2, wp = L.CONV_4X4_S2, pack_conv_weight(w)
    elif kind == L.CONV_3X3_S1:
        k2, wp = L.CONV_3X3_S1, pack_conv_weight(w.permute(1, 0, 2, 3).flip(2, 3))
    else:
        k2, wp = L.CONV_1X1, pack_conv_weight(w if isinstance(m, nn.ConvTranspose2d) else w.permute(1, 0, 2, 3))
    wp = torch.nn.functional.pad(wp, (0, cout_p - wp.shape[-1], 0, 0, 0, cin_x - wp.shape[-3]))
    return k2, wp.contiguous()


def _unpack_weight_grad(m, kind, dwp):
    """The packed weight gradient of convolution module m (forward kind `kind`) in the parameter's own layout."""
    if kind == L.CONVT_4X4_S2:
        return unpack_convt_weight_grad(dwp, m.weight.shape)
    if isinstance(m, nn.ConvTranspose2d):                 # 1x1 transposed: the parameter is the transposed matrix
        return dwp[:m.out_channels, 0, :m.in_channels].t().reshape(m.weight.shape).contiguous()
    return unpack_conv_weight_grad(dwp, m.weight.shape)


def _packed_for(m, x):
    """_pack_generic(m) with the weight's input channels padded up to x's (the previous layer's zero-padded output channels
    meet zero weights)."""
    kind, wp, bp, _ = _pack_generic(m)
    if x.shape[-1] > wp.shape[-1]:
        wp = torch.nn.functional.pad(wp, (0, x.shape[-1] - wp.shape[-1])).contiguous()
    return kind, wp, bp


class _ConvLayer(torch.autograd.Function):
    """One convolution layer (+ the ReLU that follows it) of a training-mode stack.  Saves its input and, with a ReLU, its
    post-ReLU output; backward launches the ReLU mask + bias gradient, the data gradient (the forward kernel on repacked
    weights) and the weight gradient -- each only when something needs it.

    relu_in (topologies "all"): the layer reads max(x, 0) -- a ReLU that follows a ResBlock is applied inside the kernel.
    x is saved as it is, PRE-ReLU: the weight gradient runs with relu_x=1 and the data gradient is gated by x > 0
    (relu_bias_bwd, whose mask only tests act > 0).

    Column-sum carriers (topologies "all").  That gate's column sum IS the bias gradient of the layer that produced x, when
    that layer has no ReLU of its own.  To hand it back through autograd, such a producer (emit=True) returns a second
    output, an uninitialised [C] tensor nobody reads; the gating consumer takes it as its input `carrier` and returns the
    column sum as that input's gradient; the producer finds it as the gradient of its second output and launches no bias
    sum of its own.  Without a carrier gradient the producer sums for itself."""

    @staticmethod
    def forward(ctx, x, weight, bias, carrier, m, relu, relu_in, emit, topo):
        kind, wp, bp = _packed_for(m, x)
        y = _conv(kind, x, wp, bp, bp.numel(), relu, relu_in=relu_in)
        ctx.m, ctx.kind, ctx.relu, ctx.relu_in, ctx.topo = m, kind, relu, relu_in, topo
        ctx.save_for_backward(x, y if relu else None)
        ctx.set_materialize_grads(False)
        assert not (emit and relu)
        return (y, y.new_empty(y.shape[-1])) if emit else y

    @staticmethod
    def backward(ctx, g, g_carrier=None):
        if g is None:
            return (None,) * 9
        x, y = ctx.saved_tensors
        m, kind = ctx.m, ctx.kind
        need_x, need_w, need_b, need_c = ctx.needs_input_grad[:4]
        g = g.contiguous()
        db = g_carrier
        if ctx.relu or (need_b and db is None):
            g, db = ops.relu_bias_bwd(g, y if ctx.relu else None)
        dx = dw = dc = None
        if need_x:
            k2, wp = _dgrad_weight(m, kind, x.shape[-1], g.shape[-1])
            dx = _conv(k2, g, wp, None, x.shape[-1], False)
            if ctx.relu_in:
                dx, dc = ops.relu_bias_bwd(dx, x)
        if need_w:
            dw = _unpack_weight_grad(m, kind, ops.conv_wgrad(kind, x, g, relu_x=int(ctx.relu_in), topologies=ctx.topo))
        if need_b:
            db = db[:m.out_channels].contiguous()
        return dx, dw, (db if need_b else None), (dc if need_c else None), None, None, None, None, None


class _ResBlockLayer(torch.autograd.Function):
    """One ResBlock of a training-mode stack (topologies "all").  Forward, the two launches of run_block_list:
        t = relu(conv3x3(relu(x)))            relu_in, ReLU epilogue
        y = conv1x1(t) + relu(x)              residual epilogue with relu_residual
    saving x (PRE-ReLU) and t.  Backward from g:
        db1 = column sum of g                 (the carrier's gradient when a gating consumer handed it back, see _ConvLayer)
        dW1 = wgrad 1x1 (t, g)
        d_t = dgrad 1x1 (g), masked by t > 0, with db3 out of the same launch
        dW3 = wgrad 3x3 (x, d_t, relu_x=1)
        d_r = dgrad 3x3 (d_t) + g             the add rides the forward kernel's residual epilogue
        dx  = d_r gated by x > 0              its column sum goes to the carrier: the bias gradient of what produced x"""

    @staticmethod
    def forward(ctx, x, w3, b3, w1, b1, carrier, block, emit):
        c3, c1 = block.conv[1], block.conv[3]
        k3, wp3, bp3 = _packed_for(c3, x)
        t = _conv(k3, x, wp3, bp3, bp3.numel(), True, relu_in=True)
        k1, wp1, bp1 = _packed_for(c1, t)
        if bp1.numel() != x.shape[-1]:
            raise NotImplementedError(f"training a ResBlock whose input has {x.shape[-1]} channels for {c1.out_channels} of its own")
        y = _conv(k1, t, wp1, bp1, bp1.numel(), False, residual=x, relu_residual=True)
        ctx.c3, ctx.c1 = c3, c1
        ctx.save_for_backward(x, t)
        ctx.set_materialize_grads(False)
        return (y, y.new_empty(y.shape[-1])) if emit else y

    @staticmethod
    def backward(ctx, g, g_carrier=None):
        if g is None:
            return (None,) * 8
        x, t = ctx.saved_tensors
        c3, c1 = ctx.c3, ctx.c1
        need_x, need_w3, need_b3, need_w1, need_b1, need_c = ctx.needs_input_grad[:6]
        g = g.contiguous()
        dx = dw3 = db3 = dw1 = db1 = dc = None
        if need_b1:
            db1 = g_carrier if g_carrier is not None else ops.relu_bias_bwd(g, None)[1]
            db1 = db1[:c1.out_channels].contiguous()
        if need_w1:
            dw1 = unpack_conv_weight_grad(ops.conv_wgrad(L.CONV_1X1, t, g, topologies=1), c1.weight.shape)
        if need_x or need_w3 or need_b3:
            _, wp = _dgrad_weight(c1, L.CONV_1X1, t.shape[-1], g.shape[-1])
            d_t, db3 = ops.relu_bias_bwd(_conv(L.CONV_1X1, g, wp, None, t.shape[-1], False), t)
            db3 = db3[:c3.out_channels].contiguous() if need_b3 else None
            if need_w3:
                dw3 = unpack_conv_weight_grad(ops.conv_wgrad(L.CONV_3X3_S1, x, d_t, relu_x=1, topologies=1), c3.weight.shape)
            if need_x:
                _, wp = _dgrad_weight(c3, L.CONV_3X3_S1, x.shape[-1], d_t.shape[-1])
                dx, dc = ops.relu_bias_bwd(_conv(L.CONV_3X3_S1, d_t, wp, None, x.shape[-1], False, residual=g), x)
        return dx, dw3, db3, dw1, db1, (dc if need_c else None), None, None


def _training_kind(m, topologies="plain"):
    """The kernel kind of a module the training path supports; NotImplementedError naming what is missing otherwise."""
    everything = topologies == "all"
    if isinstance(m, ResBlock):
        if everything:
            return
        raise NotImplementedError("training a ResBlock topology is not implemented: the ResBlock backward (3x3 weight gradient, "
                                  "residual branch) is missing; n_res_block=0 topologies train")
    if isinstance(m, nn.ConvTranspose2d):
        if m.kernel_size == (1, 1) or (m.kernel_size == (4, 4) and m.stride == (2, 2) and m.padding == (1, 1)):
            return
    elif isinstance(m, nn.Conv2d):
        ks, st, pd = m.kernel_size, m.stride, m.padding
        if (ks == (4, 4) and st == (2, 2) and pd == (1, 1)) or (ks == (1, 1) and st == (1, 1) and pd == (0, 0)):
            return
        if everything and ks == (3, 3) and st == (1, 1) and pd == (1, 1):
            return
        if ks == (3, 3):
            raise NotImplementedError("training a topology with a 3x3 convolution is not implemented: the 3x3 weight gradient is "
                                      "missing (stride 6 encoders and their decoders train)")
    raise NotImplementedError(f"training through {m} is not implemented")


def _gated_next(mods, i):
    """Is the first convolution or ResBlock from mods[i] on one that gates its data gradient by its input's sign -- a ResBlock,
    or a convolution behind a ReLU?  (Then its gate's column sum is the bias gradient of the module in front of mods[i].)"""
    relu = False
    while i < len(mods) and isinstance(mods[i], nn.ReLU):
        relu, i = True, i + 1
    return i < len(mods) and (relu or isinstance(mods[i], ResBlock))


def train_block_list(blocks, x, topologies="plain"):
    """run_block_list for training mode: the same blocks on the same forward kernels, one _ConvLayer per convolution so that
    autograd reaches the weights.  topologies="plain" (default): the topologies of 4x4 stride-2, transposed 4x4 stride-2 and
    1x1 convolutions, where every ReLU follows a convolution and rides in its epilogue; everything else raises.
    topologies="all": 3x3 convolutions and ResBlocks (_ResBlockLayer) too, a ReLU behind a ResBlock applied to the input of
    the next convolution inside the kernel, as run_block_list does."""
    if topologies not in TRAIN_TOPOLOGIES:
        raise ValueError(f"topologies must be one of {TRAIN_TOPOLOGIES}, not {topologies!r}")
    mods = list(blocks)
    for m in mods:
        if not isinstance(m, nn.ReLU):
            _training_kind(m, topologies)
    everything = topologies == "all"
    relu_pending, carrier = False, None
    i = 0
    while i < len(mods):
        m = mods[i]
        if isinstance(m, nn.ReLU):
            if not everything:
                raise NotImplementedError("training: a ReLU that does not follow a convolution (ResBlock topologies) is not implemented")
            relu_pending = True
            i += 1
            continue
        if isinstance(m, ResBlock):
            emit = _gated_next(mods, i + 1)
            c3, c1 = m.conv[1], m.conv[3]
            out = _ResBlockLayer.apply(x, c3.weight, c3.bias, c1.weight, c1.bias, carrier, m, emit)
            i += 1                                       # (a ReLU pending from before the block is subsumed by the block's own)
        else:
            fuse = i + 1 < len(mods) and isinstance(mods[i + 1], nn.ReLU)
            emit = everything and not fuse and _gated_next(mods, i + 1)
            cin_p = (m.in_channels + 3) // 4 * 4
            if x.shape[-1] < cin_p:
                x, carrier = torch.nn.functional.pad(x, (0, cin_p - x.shape[-1])), None
            out = _ConvLayer.apply(x, m.weight, m.bias, carrier if relu_pending else None, m, fuse, relu_pending, emit, int(everything))
            i += 2 if fuse else 1
        relu_pending = False
        x, carrier = out if emit else (out, None)
    if relu_pending:                                     # a stack that ENDS in a ReLU behind a ResBlock (decoder stride 0), as run_block_list
        x = torch.relu(x)
    return x


class Encoder(_ConvStack):
    """vqvae/vqvae_zc.py:116-164.  Production (stride 6, simple, no ResBlocks): conv4x4s2+ReLU, conv4x4s2+ReLU, conv4x4s2, ReLU,
    conv1x1 on the fused fast path; every other topology through run_block_list."""

    def __init__(self, in_channel, channel, n_res_block, n_res_channel, stride, embed_dim, n_embed, simple):
        if stride == 6:
            c1, c2 = (channel, channel) if simple else (channel // 4, channel // 2)
            blocks = [nn.Conv2d(in_channel, c1, 4, stride=2, padding=1), nn.ReLU(inplace=True),
                      nn.Conv2d(c1, c2, 4, stride=2, padding=1), nn.ReLU(inplace=True),
                      nn.Conv2d(c2, channel, 4, stride=2, padding=1)]
        elif stride == 4:
            blocks = [nn.Conv2d(in_channel, channel // 2, 4, stride=2, padding=1), nn.ReLU(inplace=True),
                      nn.Conv2d(channel // 2, channel, 4, stride=2, padding=1), nn.ReLU(inplace=True),
                      nn.Conv2d(channel, channel, 3, padding=1)]
        elif stride == 2:
            blocks = [nn.Conv2d(in_channel, channel // 2, 4, stride=2, padding=1), nn.ReLU(inplace=True),
                      nn.Conv2d(channel // 2, channel, 3, padding=1)]
        else:
            raise ValueError("stride must be 6, 4 or 2 (vqvae/vqvae_zc.py:120-155)")
        blocks += [ResBlock(channel, n_res_channel) for _ in range(n_res_block)]
        blocks += [nn.ReLU(inplace=True), nn.Conv2d(channel, embed_dim, 1)]
        super().__init__(blocks)
        self.channel, self.embed_dim = channel, embed_dim
        self._fast = stride == 6 and simple and n_res_block == 0 and channel % 8 == 0 and embed_dim % 8 == 0
        self._generic_cache = {}

    def forward(self, input):
        """NCHW image -> [b, h/8, w/8, embed_dim] (the reference returns the NHWC permutation too, :164)."""
        return self.forward_nhwc4(ops.nchw3_to_nhwc4(input))

    def forward_nhwc4(self, x4):
        """[b, h, w, 4] fp32 image, channel 3 zero (what the layout launch of forward or ops.image_prep writes) ->
        [b, h/8, w/8, embed_dim]."""
        assert x4.dim() == 4 and x4.shape[3] == 4 and x4.dtype == torch.float32, "encoder expects NHWC4 fp32 input"
        x4 = x4.contiguous()
        if self.training:
            y = train_block_list(self.blocks, x4, self._train_topologies)
            return y[..., :self.embed_dim].contiguous() if y.shape[-1] != self.embed_dim else y
        if not self._fast:
            y = run_block_list(self.blocks, x4, self._generic_cache, self._precision)
            return y[..., :self.embed_dim].contiguous() if y.shape[-1] != self.embed_dim else y
        (w1, b1), (w2, b2), (w3, b3), (w4, b4) = self._weights([pack_conv_weight] * 4)
        l1, l2, l3, l4 = self._limbs([pack_conv_weight] * 4, 4)
        pr = self._precision
        y = _conv(L.CONV_4X4_S2, x4, w1, b1, self.channel, True, precision=pr, w_limbs=l1)
        y = _conv(L.CONV_4X4_S2, y, w2, b2, self.channel, True, precision=pr, w_limbs=l2)
        y = _conv(L.CONV_4X4_S2, y, w3, b3, self.channel, True, precision=pr, w_limbs=l3)     # ReLU of blocks[5] folded into this epilogue
        return _conv(L.CONV_1X1, y, w4, b4, self.embed_dim, False, precision=pr, w_limbs=l4)


class Decoder(_ConvStack):
    """vqvae/vqvae_zc.py:167-214.  Production (stride 4, simple, no ResBlocks): convT+ReLU x3, conv1x1 -> RGB on the fused fast
    path; every other topology through run_block_list."""

    def __init__(self, in_channel, out_channel, channel, n_res_block, n_res_channel, stride, simple):
        blocks = [nn.ConvTranspose2d(in_channel, channel, 4, stride=2, padding=1)]
        blocks += [ResBlock(channel, n_res_channel) for _ in range(n_res_block)]
        blocks.append(nn.ReLU(inplace=True))
        if stride == 4 and simple:
            blocks += [nn.ConvTranspose2d(channel, channel, 4, stride=2, padding=1), nn.ReLU(inplace=True),
                       nn.ConvTranspose2d(channel, channel, 4, stride=2, padding=1), nn.ReLU(inplace=True),
                       nn.Conv2d(channel, out_channel, 1)]
        elif stride == 4:
            blocks += [nn.ConvTranspose2d(channel, channel, 4, stride=2, padding=1), nn.ReLU(inplace=True),
                       nn.ConvTranspose2d(channel, channel // 2, 1), nn.ReLU(inplace=True),
                       nn.ConvTranspose2d(channel // 2, out_channel, 4, stride=2, padding=1)]
        elif stride == 2:
            blocks.append(nn.ConvTranspose2d(channel, out_channel, 4, stride=2, padding=1))
        # (any other stride: the reference appends nothing -- vqvae/vqvae_zc.py:178-208)
        super().__init__(blocks)
        # (a decoder stride other than 4 / 2 ends with the ReLU: its output has `channel` channels)
        self.channel, self.out_channel = channel, (out_channel if stride in (4, 2) else channel)
        self._fast = stride == 4 and simple and n_res_block == 0 and out_channel == 3 and channel % 8 == 0 and in_channel % 4 == 0
        self._generic_cache = {}

    def forward_nhwc(self, q_nhwc, scale=None, shift=None):
        if self.training or not self._fast:
            run = ((lambda b, x: train_block_list(b, x, self._train_topologies)) if self.training else
                   (lambda b, x: run_block_list(b, x, self._generic_cache, self._precision)))
            y = run(self.blocks, q_nhwc.contiguous().float())
            img = y[..., :self.out_channel].permute(0, 3, 1, 2).contiguous()
            if scale is not None:
                img = img * torch.tensor(scale, device=img.device, dtype=img.dtype).view(1, -1, 1, 1)
            if shift is not None:
                img = img + torch.tensor(shift, device=img.device, dtype=img.dtype).view(1, -1, 1, 1)
            return img
        packers = [pack_convt_weight] * 3 + [lambda w: w.detach().float().reshape(3, -1).contiguous()]
        (w1, b1), (w2, b2), (w3, b3), (w4, b4) = self._weights(packers)
        l1, l2, l3 = self._limbs(packers, 3)             # the final 1x1 -> RGB stays fp32 arithmetic in both modes
        pr = self._precision
        y = _conv(L.CONVT_4X4_S2, q_nhwc.contiguous(), w1, b1, self.channel, True, precision=pr, w_limbs=l1)
        y = _conv(L.CONVT_4X4_S2, y, w2, b2, self.channel, True, precision=pr, w_limbs=l2)
        if self.channel % 128 == 0:
            # production width: the last transposed convolution projects straight to RGB in its epilogue
            return _conv(L.CONVT_4X4_S2, y, w3, b3, self.channel, True, rgb=(w4, b4, scale, shift), precision=pr, w_limbs=l3)
        y = _conv(L.CONVT_4X4_S2, y, w3, b3, self.channel, True, precision=pr, w_limbs=l3)
        b, h, w, c = y.shape
        out = torch.empty((b, 3, h, w), dtype=torch.float32, device=y.device)
        sc = (C.c_float * 3)(*scale) if scale is not None else None
        sh = (C.c_float * 3)(*shift) if shift is not None else None
        with ops.timed_launch("conv1x1_rgb", 2.0 * b * h * w * c * 3, 4.0 * (y.numel() + out.numel()), f"{b}x{h}x{w}x{c}->3"):
            L.check(L.lib().cogv_conv1x1_to_rgb_f32(_p(y), _p(w4), _p(b4), _p(out), b, h, w, c, sc, sh, _stream()),
                    "cogv_conv1x1_to_rgb_f32")
        return out

    def forward(self, input):
        """NCHW quantised map -> NCHW image."""
        return self.forward_nhwc(input.permute(0, 2, 3, 1))


class VQVAE(nn.Module):
    def __init__(self, in_channel=3, channel=128, n_res_block=2, n_res_channel=32, embed_dim=64, n_embed=1024,
                 stride=4, simple=True, decay=0.99):
        super().__init__()
        if channel == 2048:
            n_res_block = 0
        self.enc_b = Encoder(in_channel, channel, n_res_block, n_res_channel, stride, embed_dim, n_embed, simple)
        self.quantize_t = Quantize(embed_dim, n_embed)
        self.dec = Decoder(in_channel=embed_dim, out_channel=in_channel, channel=channel, n_res_block=n_res_block,
                           n_res_channel=n_res_channel, stride=stride - 2, simple=simple)

    @property
    def precision(self):
        """"fp32" or "bf16x3": what the eval-mode convolutions run on (set_precision)."""
        return self.enc_b._precision

    def set_precision(self, precision):
        """"fp32" (default): every convolution on the exact-fp32 MFMA kernel.  "bf16x3": the eval-mode convolutions of the
        encoder and the decoder (fast path and run_block_list alike) on the split-bf16 kernel -- three bf16 limbs per operand,
        six products, fp32 accumulation: fp32-class accuracy at a higher matrix rate, but not the exact path's bits, so an id
        whose two nearest codes are a near-tie may differ.  Deliberately unchanged by the mode: vq_argmin (the distance
        product that decides an id stays exact fp32), embed_code, rgb_finalize, image_prep and image_grid; and every
        training-mode launch -- train_block_list, _ConvLayer, the data gradient and conv_wgrad stay exact fp32, a model in
        .train() ignores the mode.  Returns self."""
        if precision not in PRECISIONS:
            raise ValueError(f"precision must be one of {PRECISIONS}, not {precision!r}")
        self.enc_b._precision = self.dec._precision = precision
        return self

    @property
    def train_topologies(self):
        """"plain" or "all": what module.train() covers (set_train_topologies)."""
        return self.enc_b._train_topologies

    def set_train_topologies(self, which):
        """"plain" (default): training covers the topologies made of 4x4 stride-2, transposed 4x4 stride-2 and 1x1
        convolutions with a ReLU behind a convolution (new_model(), every n_res_block=0 stride-6 configuration); ResBlocks
        and 3x3 convolutions raise NotImplementedError, as they always did.  "all" (opt-in; a later change makes it the
        default): every topology the constructors build trains -- VQVAE() itself, the stride-4 and stride-2 encoders, any
        n_res_block.  continuous_relax=True raises in both.  Eval-mode results do not depend on it.  Returns self."""
        if which not in TRAIN_TOPOLOGIES:
            raise ValueError(f"which must be one of {TRAIN_TOPOLOGIES}, not {which!r}")
        self.enc_b._train_topologies = self.dec._train_topologies = which
        return self

    def encode(self, input, continuous_relax=False, temperature=1., hard=False, KL=False):
        """-> (quantised NCHW, diff [1], ids [b, h/8, w/8]) as vqvae/vqvae_zc.py:251-259."""
        logits = self.enc_b(input)
        quant_t, diff_t, id_t = self.quantize_t.forward_(logits, continuous_relax, temperature, hard)
        return quant_t.permute(0, 3, 1, 2), diff_t.unsqueeze(0), id_t

    def encode_ids(self, input):
        """ids only: skips the embedding lookup / diff that img2code discards."""
        return self.quantize_t.nearest_code(self.enc_b(input))

    def encode_ids_nhwc4(self, x4):
        """encode_ids of an image that is NHWC4 already (ops.image_prep): no layout launch."""
        return self.quantize_t.nearest_code(self.enc_b.forward_nhwc4(x4))

    def invalidate_caches(self):
        """Forget every table derived from a parameter or buffer (packed weights, E^T, |E|^2).  They are keyed on the tensors'
        version counters, which in-place operators advance but writes through `.data` or the storage do not; api.train_step
        calls this after optimizer.step()."""
        self.quantize_t.invalidate_cache()
        for stack in (self.enc_b, self.dec):
            stack._packed = None
            stack._generic_cache.clear()

    def decode(self, code):
        return self.dec(code)

    def decode_code(self, code_t, scale=None, shift=None):
        return self.dec.forward_nhwc(self.quantize_t.embed_code(code_t), scale, shift)

    def forward(self, input, continuous_relax=False, temperature=1., hard=False, KL=False):
        quant_t, diff, _ = self.encode(input, continuous_relax, temperature, hard, KL)
        return self.dec(quant_t), diff
