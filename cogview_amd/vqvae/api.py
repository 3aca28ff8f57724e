"""Production tokenizer API (vqvae/api.py:12-44): new_model / img2code / code2img, and the ingest of raw images
(data_utils/vqvae_tokenizer.py:72-82) in front of it: read_images / img2code_raw; behind it the image grid bytes of
torchvision.utils.save_image (generate_samples.py:175-199, :236-244): code2img_u8 / save_image."""
import math

import torch

from .vqvae_zc import VQVAE

_STD = (0.30379, 0.32279, 0.32800)
_MEAN = (0.79093, 0.76271, 0.75340)


def new_model(precision="fp32"):
    """The pretrained tokenizer's architecture (vqvae/api.py:12-20).  precision: see set_precision."""
    return VQVAE(channel=512, n_res_block=0, n_res_channel=32, embed_dim=256, n_embed=8192, stride=6).set_precision(precision)


def set_precision(model, precision):
    """"fp32" (default, the exact-fp32 convolutions) or "bf16x3" (VQVAE.set_precision: the eval-mode convolutions on the
    split-bf16 kernel).  img2code, img2code_raw, code2img, code2img_u8 and save_image of a model's images honour it; the
    nearest-code search, the embedding lookup, ingest, egress and train_step do not change with it.  Returns the model."""
    return model.set_precision(precision)


def set_train_topologies(model, which):
    """"plain" (default): train_step covers new_model() and the other n_res_block=0 stride-6 configurations; ResBlocks and 3x3
    convolutions raise NotImplementedError in training mode.  "all" (opt-in, VQVAE.set_train_topologies; a later change makes
    it the default): every topology VQVAE's constructor builds trains, VQVAE() with its default arguments among them.  The
    Gumbel-softmax branch (continuous_relax=True) raises in both.  Returns the model."""
    return model.set_train_topologies(which)


def img2code(model, img):
    """[b, 3, H, W] normalised image -> LongTensor [b, (H/8)*(W/8)]."""
    with torch.no_grad():
        ids = model.encode_ids(img)
    return ids.view(img.shape[0], -1)


def read_images(images, img_size=256, device=None):
    """read_img (data_utils/vqvae_tokenizer.py:72-82) for a list of decoded uint8 HWC RGB images of any sizes: Resize,
    CenterCrop, ToTensor and Normalize in one launch -> [b, img_size, img_size, 4] fp32 NHWC, channel 3 zero."""
    from .. import ops
    images = [torch.as_tensor(im) for im in images]
    return ops.image_prep(images, img_size, _MEAN, _STD, device=device)


def img2code_raw(model, images, img_size=256):
    """raw uint8 HWC images -> LongTensor [b, (img_size/8)**2]: read_images, then the encoder on its NHWC4 output."""
    dev = next(model.parameters()).device
    with torch.no_grad():
        x4 = read_images(images, img_size, device=dev)
        ids = model.encode_ids_nhwc4(x4)
    return ids.view(x4.shape[0], -1)


def code2img(model, code):
    """[b, h, w] codes (or [1, h*w]: the reference takes the square root of the TOTAL element count, so flat
    codes are only valid for batch 1 -- vqvae/api.py:38-40) -> de-normalised image [b, 3, 8h, 8w]; the
    per-channel `* std + mean` of api.py:43 is fused into the last kernel."""
    if len(code.shape) == 2:
        s = int(math.sqrt(len(code.view(-1))) + 1e-5)
        code = code.view(code.shape[0], s, s)
    with torch.no_grad():
        return model.decode_code(code, scale=_STD, shift=_MEAN)


def train_step(model, optimizer, img, latent_loss_weight=0.25):
    """One training step of the tokenizer (model.train(); the default, non-relaxed path of vqvae/vqvae_zc.py:67-86 and
    :261-268): forward, loss = mse(dec, img) + latent_loss_weight * diff, backward, optimizer.step() -- any torch.optim
    optimizer over the fp32 parameters.  The EMA codebook update happens inside the forward, as in the reference.
    Which topologies train: set_train_topologies.
    Returns dict(loss, recon_loss, latent_loss) as device scalars (no host read)."""
    optimizer.zero_grad(set_to_none=True)
    dec, diff = model(img)
    recon_loss = torch.nn.functional.mse_loss(dec, img)
    latent_loss = diff.mean()
    loss = recon_loss + latent_loss_weight * latent_loss
    loss.backward()
    optimizer.step()
    model.invalidate_caches()
    return dict(loss=loss.detach(), recon_loss=recon_loss.detach(), latent_loss=latent_loss.detach())


def code2img_u8(model, code, **grid_kwargs):
    """code2img, then ops.image_grid on its output: codes -> the uint8 [GH, GW, 3] image grid torchvision.utils.save_image
    would write (generate_samples.py:175-199, :236-244), on the device.  code: as for code2img, or a list of code maps of
    different sizes (32 x 32 and 64 x 64: the smaller images are replicated to the larger, as F.interpolate does there);
    grid_kwargs: nrow, padding, normalize, value_range, scale_each, pad_value, size, out."""
    from .. import ops
    codes = code if isinstance(code, (list, tuple)) else [code]
    return ops.image_grid([code2img(model, c) for c in codes], **grid_kwargs)


def save_image(tensor, fp, format=None, **grid_kwargs):
    """torchvision.utils.save_image for CUDA fp32 images [B, 3, H, W] (or a list, as ops.image_grid takes it): the grid and
    the bytes are made on the device, one device-to-host copy of 3 bytes per pixel, then Pillow writes the file."""
    from PIL import Image
    from .. import ops
    grid = ops.image_grid(tensor, **grid_kwargs)
    Image.fromarray(grid.cpu().numpy()).save(fp, format=format)
