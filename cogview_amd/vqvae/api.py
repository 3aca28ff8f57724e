"""Production tokenizer API (vqvae/api.py:12-44): new_model / img2code / code2img, and the ingest of raw images
(data_utils/vqvae_tokenizer.py:72-82) in front of it: read_images / img2code_raw."""
import math

import torch

from .vqvae_zc import VQVAE

_STD = (0.30379, 0.32279, 0.32800)
_MEAN = (0.79093, 0.76271, 0.75340)


def new_model():
    """The pretrained tokenizer's architecture (vqvae/api.py:12-20)."""
    return VQVAE(channel=512, n_res_block=0, n_res_channel=32, embed_dim=256, n_embed=8192, stride=6)


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
