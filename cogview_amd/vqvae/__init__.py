from .api import code2img, img2code, img2code_raw, new_model, read_images  # noqa: F401
from .vqvae_zc import VQVAE  # noqa: F401
