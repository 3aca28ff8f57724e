"""GPU: the tokenizer ingest kernels.  ops.image_prep's output equals the value table indexed by Pillow's bytes
(tests/golden/image_prep.npz) and by the numpy restatement on live shapes -- equality, no tolerance; ops.sr_patches'
crops are copies and its overview is F.interpolate's; img2code_raw runs the same encoder as img2code; the raw-image
dataset writer writes the same file; refused calls write nothing."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from cogview_amd import _lib as L
from cogview_amd import ops
from tests import image_prep_cases as IC

pytestmark = pytest.mark.gpu

MEAN, STD = (0.79093, 0.76271, 0.75340), (0.30379, 0.32279, 0.32800)


def _check(out, want_u8):
    """out [B, S, S, 4] against uint8 [B, S, S, 3]: channels 0-2 the value table of the bytes, channel 3 zero."""
    out = out.cpu()
    assert torch.equal(out[..., :3], IC.lut_reference(np.stack(want_u8), MEAN, STD))
    assert torch.equal(out[..., 3], torch.zeros_like(out[..., 3]))


def _random_images(shapes, seed):
    rs = np.random.RandomState(seed)
    return [rs.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in shapes]


def test_fixture_in_one_launch():
    gold = IC.golden()
    out = ops.image_prep([torch.from_numpy(src) for src, _ in gold], IC.GOLDEN_S, MEAN, STD)
    assert out.shape == (len(gold), 16, 16, 4) and out.dtype == torch.float32
    _check(out, [o for _, o in gold])


@pytest.mark.parametrize("shapes,S", [
    ([(512, 520)], 16),                     # 65 taps across, 64 down: the cap; one output row per run of source rows
    ([(16, 4096)], 16),                     # a long crop axis, nothing resampled
    ([(20, 20)], 32),                       # an upscale with two taps
    ([(16, 16), (16, 23), (40, 16)], 16),   # a batch whose images are only cropped
    ([(300, 407), (150, 150), (160, 331)], 152),   # two column segments (128 + 24), bands in several runs, mixed scales
], ids=["cap65", "long_crop", "upscale", "copies", "two_segments"])
def test_live_shapes_against_the_restatement(shapes, S):
    imgs = _random_images(shapes, 7)
    out = ops.image_prep([torch.from_numpy(a) for a in imgs], S, MEAN, STD)
    _check(out, [IC.pil_bilinear_u8(a, S) for a in imgs])


def test_device_images_and_given_output():
    imgs = _random_images([(37, 53), (53, 37)], 3)
    out = torch.full((2, 16, 16, 4), 7.0, device="cuda")
    got = ops.image_prep([torch.from_numpy(a).cuda() for a in imgs], 16, MEAN, STD, out=out)
    assert got is out
    _check(out, [IC.pil_bilinear_u8(a, 16) for a in imgs])


def test_sr_patches():
    b, S, positions = 2, 32, [0, 4, 8, 5]
    x4 = torch.randn(b, S, S, 4, generator=torch.Generator().manual_seed(5)).clamp_(-3.9, 3.9)
    x4[..., 3] = 0
    patches, overview = ops.sr_patches(x4.cuda(), positions)
    ref_p, ref_o = IC.sr_patches_reference(x4, positions)
    assert patches.shape == (b * 4, 16, 16, 4) and overview.shape == (b, 16, 16, 4)
    assert torch.equal(patches.cpu(), ref_p)
    # |x| < 4: one ulp is 2.4e-7; three rounded additions keep either summation order within 1.5 ulp of the exact mean,
    # so two orders differ by at most 7.2e-7
    err = (overview.cpu() - ref_o).abs().max().item()
    print(f"overview max abs error {err:.3e}")
    assert err <= 1e-6
    p2, o2 = ops.sr_patches(x4.cuda(), torch.tensor(positions, device="cuda"))
    assert torch.equal(p2, patches) and torch.equal(o2, overview)
    with pytest.raises(ValueError):
        ops.sr_patches(x4.cuda(), [9])
    sent = torch.full((1,), 3.0, device="cuda")
    pos = torch.zeros(1, dtype=torch.int32, device="cuda")
    x24 = torch.zeros(1, 24, 24, 4, device="cuda")                                # S % 16 != 0
    rc = L.lib().cogv_sr_patches_nhwc4_f32(x24.data_ptr(), pos.data_ptr(), sent.data_ptr(), sent.data_ptr(), 1, 24, 1, None)
    assert rc == L.ERR_ARG and sent.item() == 3.0


def _small_vqvae():
    from cogview_amd.vqvae.vqvae_zc import VQVAE
    torch.manual_seed(11)
    return VQVAE(channel=32, n_res_block=0, n_res_channel=32, embed_dim=16, n_embed=64, stride=6).cuda().eval()


def test_img2code_raw_is_the_same_encoder():
    from cogview_amd.vqvae import img2code, img2code_raw, read_images
    m = _small_vqvae()
    imgs = _random_images([(70, 91), (64, 64), (130, 66)], 9)
    x4 = read_images(imgs, 64)
    assert x4.shape == (3, 64, 64, 4)
    ids = img2code_raw(m, imgs, 64)
    assert ids.shape == (3, 64) and ids.dtype == torch.int64
    assert torch.equal(ids, img2code(m, x4[..., :3].permute(0, 3, 1, 2).contiguous()))


def test_raw_dataset_writer_writes_the_same_file(tmp_path):
    from cogview_amd.data_utils import BinaryDataset, images_to_compact_binary, raw_images_to_compact_binary
    from cogview_amd.vqvae import read_images
    m = _small_vqvae()
    imgs = _random_images([(300, 256), (256, 256), (260, 400), (512, 512), (256, 257)], 13)
    texts = [[8192 + i, 8300 + i] for i in range(5)]
    a, b = str(tmp_path / "raw.bin"), str(tmp_path / "pre.bin")
    assert raw_images_to_compact_binary(m, iter(imgs), texts, a, img_size=256, batch_size=2) == 5
    x = read_images(imgs, 256)[..., :3].permute(0, 3, 1, 2).contiguous()
    assert images_to_compact_binary(m, x, texts, b, batch_size=2) == 5
    da, db = BinaryDataset(a, lambda r: np.array(r)), BinaryDataset(b, lambda r: np.array(r))
    assert len(da) == len(db) == 5
    for i in range(5):
        assert np.array_equal(da[i], db[i]) and da[i][:2].tolist() == texts[i]


def test_refused_calls_write_nothing():
    out = torch.full((1, 16, 16, 4), 7.0, device="cuda")
    for img, S, o, what in ((torch.zeros(528, 528, 3, dtype=torch.uint8), 16, out, "unsupported"),
                            (torch.zeros(20, 20, 3, dtype=torch.uint8), 12, torch.full((1, 12, 12, 4), 7.0, device="cuda"), "bad argument"),
                            (torch.zeros(0, 20, 3, dtype=torch.uint8), 16, out, "bad argument")):
        with pytest.raises(L.CogviewHipError, match=what):
            ops.image_prep([img], S, MEAN, STD, out=o)
        assert (o == 7.0).all()
    # the entry point itself, on a table that names such images: its code, and nothing launched
    good = torch.from_numpy(_random_images([(20, 20)], 1)[0])
    table, coeffs, nbytes = ops.image_prep_pack([good], 16)
    pack = torch.zeros(1216, dtype=torch.uint8, device="cuda")
    lut = ops.image_prep_lut(MEAN, STD, torch.device("cuda"))
    dcoef = torch.from_numpy(coeffs).cuda()

    def call(tab, S=16, pack_ptr=None, B=1):
        dtab = torch.from_numpy(np.ascontiguousarray(tab)).cuda()
        rc = L.lib().cogv_image_prep_u8(pack.data_ptr() if pack_ptr is None else pack_ptr, pack.numel(), dtab.data_ptr(), tab.ctypes.data,
                                        dcoef.data_ptr(), coeffs.size, B, S, lut.data_ptr(), out.data_ptr(), None)
        torch.cuda.synchronize()
        return rc

    def edited(**kw):
        t = table.copy()
        for name, v in kw.items():
            t[0, {"H": 2, "W": 3, "htab": 4, "off": 0}[name]] = v
        return t

    assert call(edited(H=528, W=528)) == L.ERR_UNSUPPORTED                        # 66 taps
    assert call(table, S=12) == L.ERR_ARG                                         # S % 8 != 0
    assert call(edited(H=0)) == L.ERR_ARG                                         # an empty image
    assert call(table, pack_ptr=pack.data_ptr() + 4) == L.ERR_ARG                 # a misaligned pointer
    assert call(edited(off=64)) == L.ERR_ARG                                      # the image ends beyond the pack
    assert call(edited(htab=coeffs.size)) == L.ERR_ARG                            # a table beyond the coefficients
    assert call(table, B=0) == L.ERR_ARG and call(table, B=65536) == L.ERR_ARG
    assert (out == 7.0).all()
    assert call(table) == L.OK and not (out == 7.0).any()                         # the same call, unedited, is taken
