from .api import code2img, code2img_u8, img2code, img2code_raw, new_model, read_images, save_image, set_precision, set_train_topologies, train_step  # noqa: F401
from .vqvae_zc import VQVAE  # noqa: F401
