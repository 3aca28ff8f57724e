"""The img2code stage of the reference's preprocessing (preprocess/preprocess_text_image_data.py:28-64: images in batches
of 128 through the VQ-VAE encoder, one row of text ids + 1024 codes per image), writing the CompactBinaryDataset file the
trainer reads instead of LMDB pickles (no lmdb module in this image).  The encoder is the HIP VQ-VAE path."""
import random

import numpy as np
import torch

from .. import ops
from ..generation.id_space import IdSpace
from .datasets import write_compact_binary

SR_CODES = 1024                      # codes of the 256 x 256 overview and of each 256 x 256 patch of a 512 x 512 image
SR_ROW_CODES = 2 * SR_CODES + 1      # a compact super-resolution row: overview codes, position, patch codes


@torch.no_grad()
def images_to_compact_binary(model, images, text_ids, path, batch_size=128, img2code=None):
    """images: tensor [n, 3, 256, 256] (normalised as vqvae/api.py expects) or an iterable of such batches;
    text_ids: n id lists.  Returns the number of rows written."""
    if img2code is None:
        from ..vqvae import img2code as _img2code
        img2code = _img2code
    if isinstance(images, torch.Tensor):
        images = [images[i:i + batch_size] for i in range(0, images.shape[0], batch_size)]
    done = 0
    for chunk in images:
        codes = img2code(model, chunk)
        codes = codes.reshape(codes.shape[0], -1).cpu().numpy()
        write_compact_binary(path, text_ids[done:done + codes.shape[0]], codes, append=done > 0)
        done += codes.shape[0]
    assert done == len(text_ids)
    return done


@torch.no_grad()
def raw_images_to_compact_binary(model, images, text_ids, path, img_size=256, batch_size=128):
    """images_to_compact_binary for raw images: an iterable of decoded uint8 HWC RGB arrays or tensors of any sizes, resized,
    cropped and normalised on the device (vqvae.read_images: preprocess_entry.py:87-106) in batches of batch_size.  Writes
    the same file; returns the number of rows written."""
    from ..vqvae import img2code_raw
    done, chunk = 0, []

    def flush():
        nonlocal done, chunk
        codes = img2code_raw(model, chunk, img_size).cpu().numpy()
        write_compact_binary(path, text_ids[done:done + codes.shape[0]], codes, append=done > 0)
        done += codes.shape[0]
        chunk = []

    for im in images:
        chunk.append(im)
        if len(chunk) == batch_size:
            flush()
    if chunk:
        flush()
    assert done == len(text_ids)
    return done


@torch.no_grad()
def make_super_resolution_rows(model, tokenizer, text_ids, images, img_size=512, sampling_num=4, positions=None):
    """make_super_resolution_batch (preprocess/pretokenized_data.py:89-140) on the device: for each image, sampling_num
    rows  [ROI1] text [BASE] [BOI1] overview codes [EOI1] [ROI2] [POSp] [BASE] [BOI2] patch codes [EOI2]  (the query layout of
    generate_samples.py:208 with the answer appended), image-major, the crop positions p shared by all images.
    images: raw uint8 HWC images of any sizes, or a normalised tensor [b, 3, 512, 512]; text_ids: one id list per image;
    tokenizer: an IdSpace or the reference's tokenizer; positions: sampling_num values of 0..8 (default: drawn as the
    reference draws them).  Returns b * sampling_num int64 numpy arrays."""
    if img_size != 512:
        raise NotImplementedError("super-resolution rows are built from 512 x 512 images ([BASE] overview and patches)")
    tokenizer = tokenizer if tokenizer is not None else IdSpace()
    if positions is None:
        positions = random.choices(range(9), weights=[1] * 9, k=sampling_num)
    positions = [int(p) for p in positions]
    assert len(positions) == sampling_num
    if isinstance(images, torch.Tensor):
        assert images.dim() == 4 and tuple(images.shape[1:]) == (3, img_size, img_size)
        x4 = ops.nchw3_to_nhwc4(images)
    else:
        from ..vqvae import read_images
        x4 = read_images(images, img_size, device=next(model.parameters()).device)
    b = x4.shape[0]
    assert len(text_ids) == b
    patches, overview = ops.sr_patches(x4, positions)
    codes_patches = model.encode_ids_nhwc4(patches).reshape(b * sampling_num, -1).cpu().numpy()
    codes_overviews = model.encode_ids_nhwc4(overview).reshape(b, -1).cpu().numpy()
    size_tk = tokenizer['[BASE]']
    rows = []
    for i in range(b):
        head = np.array([tokenizer['[ROI1]']] + [int(t) for t in text_ids[i]] + [size_tk, tokenizer['[BOI1]']], dtype=np.int64)
        for j, p in enumerate(positions):
            mid = np.array([tokenizer['[EOI1]'], tokenizer['[ROI2]'], tokenizer['[POS%d]' % p], size_tk, tokenizer['[BOI2]']], dtype=np.int64)
            rows.append(np.concatenate((head, codes_overviews[i].astype(np.int64), mid,
                                        codes_patches[i * sampling_num + j].astype(np.int64), np.array([tokenizer['[EOI2]']], dtype=np.int64))))
    return rows


def compact_super_resolution_row(row, tokenizer=None):
    """One row of super_resolution_to_compact_binary's file -> the token row make_super_resolution_rows built."""
    tokenizer = tokenizer if tokenizer is not None else IdSpace()
    row = np.asarray(row).astype(np.int64)
    text, ov, p, patch = row[:64], row[64:64 + SR_CODES], int(row[64 + SR_CODES]), row[64 + SR_CODES + 1:]
    size_tk = tokenizer['[BASE]']
    return np.concatenate((np.array([tokenizer['[ROI1]']]), text[text > -1], np.array([size_tk, tokenizer['[BOI1]']]), ov,
                           np.array([tokenizer['[EOI1]'], tokenizer['[ROI2]'], tokenizer['[POS%d]' % p], size_tk, tokenizer['[BOI2]']]),
                           patch, np.array([tokenizer['[EOI2]']])))


def super_resolution_to_compact_binary(model, text_ids, images, path, img_size=512, sampling_num=4, positions=None, append=False):
    """The rows of make_super_resolution_rows in a flat int32 file, written with write_compact_binary: per row 64 text ids
    padded with -1, then SR_ROW_CODES values: 1024 overview codes, the position p, 1024 patch codes (the command tokens
    are the tokenizer's to add: compact_super_resolution_row, e.g. as the process_fn of a BinaryDataset with
    length_per_sample=64 + SR_ROW_CODES).  Returns the number of rows written."""
    ids = IdSpace()
    rows = make_super_resolution_rows(model, ids, text_ids, images, img_size, sampling_num, positions)
    pos0 = ids['[POS0]']
    texts, codes = [], np.zeros((len(rows), SR_ROW_CODES), dtype=np.int64)
    for n, row in enumerate(rows):
        t = len(row) - (2 * SR_CODES + 9)                    # ids between [ROI1] and [BASE]
        texts.append(row[1:1 + t])
        codes[n, :SR_CODES] = row[t + 3:t + 3 + SR_CODES]
        codes[n, SR_CODES] = row[t + 5 + SR_CODES] - pos0
        codes[n, SR_CODES + 1:] = row[t + 8 + SR_CODES:-1]
    return write_compact_binary(path, texts, codes, append=append, code_len=SR_ROW_CODES)
