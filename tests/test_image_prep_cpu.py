"""CPU: the host half of the tokenizer ingest.  The numpy restatement of Pillow's bilinear resize equals the stored Pillow
results (and live Pillow where it is installed); the library's coefficient tables (cogv_resample_coeffs), pushed through
the integer formula, reproduce them byte for byte, and so do the tables ops.image_prep_pack lays out for the kernel; the
plan query refuses what the kernel refuses; make_super_resolution_rows builds the reference's row layout."""
import numpy as np
import pytest
import torch

from cogview_amd import _lib as L
from cogview_amd import ops
from tests import image_prep_cases as IC

S = IC.GOLDEN_S


@pytest.fixture(scope="module")
def golden():
    return IC.golden()


def test_restatement_equals_stored_pillow_results(golden):
    assert [g[0].shape[:2] for g in golden] == IC.GOLDEN_SHAPES
    for src, out in golden:
        assert out.shape == (S, S, 3) and out.dtype == np.uint8
        assert np.array_equal(IC.pil_bilinear_u8(src, S), out), src.shape


def test_restatement_equals_live_pillow(golden):
    Image = pytest.importorskip("PIL.Image")
    for src, _ in golden:
        H, W = src.shape[:2]
        nh, nw = IC.target_size(H, W, S)
        img = Image.fromarray(src, "RGB")
        if (nw, nh) != (W, H):
            img = img.resize((nw, nh), Image.BILINEAR)
        top, left = IC.crop_offset(nh, S), IC.crop_offset(nw, S)
        ref = np.asarray(img.crop((left, top, left + S, top + S)))
        assert np.array_equal(IC.pil_bilinear_u8(src, S), ref), src.shape


def test_library_coefficients_reproduce_the_fixture(golden):
    for src, out in golden:
        H, W = src.shape[:2]
        rc, plan = L.image_prep_plan(H, W, S)
        assert rc == L.OK
        assert (plan["nh"], plan["nw"]) == IC.target_size(H, W, S)
        img = src
        for n_in, n_out, first, axis, taps in ((W, plan["nw"], plan["left"], 1, plan["taps_h"]), (H, plan["nh"], plan["top"], 0, plan["taps_v"])):
            rc, xmin, count, k = L.resample_coeffs(n_in, n_out, taps)
            assert rc == L.OK and int(count.max()) == taps
            assert not k[np.arange(taps)[None, :] >= count[:, None]].any()        # zero beyond count
            if n_in == n_out:                                                      # a copy: one tap of weight one
                assert np.array_equal(xmin, np.arange(n_out)) and (count == 1).all() and (k[:, 0] == 1 << 22).all()
            img = IC.apply_axis(img, IC.tables_from_library(xmin, count, k), axis, first, S)
        assert np.array_equal(img, out), src.shape


def test_library_coefficients_equal_the_restatement():
    for n_in, n_out in ((53, 22), (37, 16), (9, 16), (40, 71), (511, 247), (259, 27), (520, 16)):
        rc, xmin, count, k = L.resample_coeffs(n_in, n_out)
        assert rc == L.OK
        for (rx, rk), lx, lc, lk in zip(IC.axis_coeffs(n_in, n_out), xmin, count, k):
            assert (rx, len(rk)) == (lx, lc) and np.array_equal(rk, lk[:lc]), (n_in, n_out)


def test_packed_tables_reproduce_the_fixture(golden):
    """What ops.image_prep hands the kernel (records, crop-cut transposed tables, byte offsets), walked as the kernel walks it."""
    images = [torch.from_numpy(src) for src, _ in golden]
    table, coeffs, nbytes = ops.image_prep_pack(images, S)
    assert table.shape == (len(golden), 8) and table.dtype == np.int32 and coeffs.dtype == np.int32
    assert nbytes == sum(src.size for src, _ in golden)
    pack = np.concatenate([src.reshape(-1) for src, _ in golden])
    for rec, (_, out) in zip(table, golden):
        off, H, W, htab, vtab, th, tv = int(rec[0]), *[int(v) for v in rec[2:]]
        img = pack[off:off + H * W * 3].reshape(H, W, 3)
        for tab, taps, axis in ((htab, th, 1), (vtab, tv, 0)):
            xmin, count = coeffs[tab:tab + S], coeffs[tab + S:tab + 2 * S]
            k = coeffs[tab + 2 * S:tab + (2 + taps) * S].reshape(taps, S).T
            assert count.max() <= taps
            img = IC.apply_axis(img, IC.tables_from_library(xmin, count, k), axis)
        assert np.array_equal(img, out), (H, W)
    # images of one size share their tables
    t2, c2, _ = ops.image_prep_pack([images[0], images[1], images[0]], S)
    assert tuple(t2[0, 2:]) == tuple(t2[2, 2:]) and t2[2, 0] == images[0].numel() + images[1].numel()
    assert c2.size == sum((2 + taps) * S for taps in t2[0, 6:].tolist())             # 53 -> 22 and 37 -> 16, each stored once


def test_crop_offsets_round_half_to_even():
    assert IC.crop_offset(17, 16) == 0 and IC.crop_offset(19, 16) == 2 and IC.crop_offset(18, 16) == 1
    for H, W, top, left in ((17, 16, 0, 0), (19, 16, 2, 0), (16, 17, 0, 0), (16, 19, 0, 2), (16, 21, 0, 2), (16, 23, 0, 4)):
        rc, plan = L.image_prep_plan(H, W, 16)
        assert rc == L.OK and (plan["nh"], plan["nw"]) == (H, W) and (plan["top"], plan["left"]) == (top, left), (H, W)


def test_size_rule_truncates_the_long_side():
    assert IC.target_size(511, 33, 16) == (int(16 * 511 / 33), 16) == (247, 16)
    rc, plan = L.image_prep_plan(511, 33, 16)
    assert rc == L.OK and (plan["nh"], plan["nw"]) == (247, 16) and plan["top"] == IC.crop_offset(247, 16) == 116
    rc, plan = L.image_prep_plan(33, 511, 16)
    assert rc == L.OK and (plan["nh"], plan["nw"], plan["left"]) == (16, 247, 116)


def test_plan_refuses_what_the_kernel_refuses():
    # 528 -> 16 (scale 33): output 1 reads source pixels 17 .. 82, 66 of them; 520 -> 16 reads 65 at most and is taken
    assert max(len(k) for _, k in IC.axis_coeffs(528, 16)) == 66
    assert L.image_prep_plan(528, 528, 16)[0] == L.ERR_UNSUPPORTED
    assert L.image_prep_plan(600, 528, 16)[0] == L.ERR_UNSUPPORTED
    assert L.resample_coeffs(528, 16)[0] == L.ERR_UNSUPPORTED
    rc, plan = L.image_prep_plan(512, 520, 16)
    assert rc == L.OK and (plan["taps_h"], plan["taps_v"]) == (65, 64)
    assert plan["lds_bytes"] <= 65536 and plan["lds_rows"] >= plan["taps_v"]
    # at the largest tap count of both axes and the widest segment the tile still fits
    rc, plan = L.image_prep_plan(8192, 8200, 256)                                 # W / 256 just above 32, H / 256 = 32
    assert rc == L.OK and plan["taps_h"] == 65 and plan["lds_bytes"] <= 65536 and plan["lds_rows"] >= plan["taps_v"]
    assert L.image_prep_plan(20, 20, 12)[0] == L.ERR_ARG                          # S % 8 != 0
    assert L.image_prep_plan(20, 20, 0)[0] == L.ERR_ARG and L.image_prep_plan(20, 20, -8)[0] == L.ERR_ARG
    assert L.image_prep_plan(0, 20, 16)[0] == L.ERR_ARG and L.image_prep_plan(20, 0, 16)[0] == L.ERR_ARG      # an empty image
    assert L.resample_coeffs(0, 16)[0] == L.ERR_ARG
    # the Python entry raises with the same verdicts before anything is copied or launched
    with pytest.raises(L.CogviewHipError, match="unsupported"):
        ops.image_prep_pack([torch.zeros(528, 528, 3, dtype=torch.uint8)], 16)
    with pytest.raises(L.CogviewHipError, match="bad argument"):
        ops.image_prep_pack([torch.zeros(20, 20, 3, dtype=torch.uint8)], 12)
    with pytest.raises(L.CogviewHipError, match="bad argument"):
        ops.image_prep_pack([torch.zeros(0, 20, 3, dtype=torch.uint8)], 16)


def test_value_table_is_totensor_and_normalize():
    mean, std = (0.79093, 0.76271, 0.75340), (0.30379, 0.32279, 0.32800)
    lut = ops.image_prep_lut(mean, std)
    assert lut.shape == (3, 256) and lut.dtype == torch.float32
    u8 = np.stack([np.arange(256, dtype=np.uint8)] * 3, axis=-1)                  # [256, 3]
    assert torch.equal(lut.t(), IC.lut_reference(u8, mean, std))


class _StubModel:
    """encode_ids_nhwc4 returns codes that name the input's batch index and size."""

    def __init__(self):
        self.calls = []

    def encode_ids_nhwc4(self, x4):
        self.calls.append(tuple(x4.shape))
        n = x4.shape[0]
        base = 1000 if x4.shape[0] == self.b else 5000            # overview call has b rows, patch call b * k
        return (torch.arange(n).view(n, 1, 1) * 10 + base + torch.arange(32).view(1, 32, 1) % 7 + torch.zeros(n, 32, 32, dtype=torch.long))


def test_super_resolution_rows_follow_the_reference_layout(monkeypatch):
    from cogview_amd.data_utils import compact_super_resolution_row, make_super_resolution_rows
    from cogview_amd.generation.id_space import IdSpace
    seen = {}

    def fake_sr_patches(x4, positions):
        seen["positions"] = list(positions)
        return IC.sr_patches_reference(x4, positions)

    monkeypatch.setattr(ops, "sr_patches", fake_sr_patches)
    monkeypatch.setattr(ops, "nchw3_to_nhwc4", lambda x: torch.nn.functional.pad(x.permute(0, 2, 3, 1), (0, 1)).contiguous())
    tok, model = IdSpace(), _StubModel()
    b, k, positions = 2, 3, [4, 0, 8]
    model.b = b
    imgs = torch.zeros(b, 3, 512, 512)
    texts = [[8200, 8201, 8202], [9000]]
    rows = make_super_resolution_rows(model, tok, texts, imgs, img_size=512, sampling_num=k, positions=positions)
    assert seen["positions"] == positions
    assert model.calls == [(b * k, 256, 256, 4), (b, 256, 256, 4)]               # one patch call, one overview call
    assert len(rows) == b * k
    codes_p = model.encode_ids_nhwc4(torch.zeros(b * k, 256, 256, 4)).reshape(b * k, -1).numpy()
    codes_o = model.encode_ids_nhwc4(torch.zeros(b, 256, 256, 4)).reshape(b, -1).numpy()
    base = 8192 + 50000                                                          # command ids, written out by hand
    ROI1, ROI2, BOI1, BOI2, EOI1, EOI2, BASE, POS0 = base + 7, base + 8, base + 1, base + 2, base + 4, base + 5, base + 16, base + 18
    for i in range(b):
        for j, p in enumerate(positions):                                        # image-major; the positions repeat per image
            want = [ROI1] + texts[i] + [BASE, BOI1] + codes_o[i].tolist() + [EOI1, ROI2, POS0 + p, BASE, BOI2] + \
                codes_p[i * k + j].tolist() + [EOI2]
            row = rows[i * k + j]
            assert len(row) == len(texts[i]) + 2 * 1024 + 9 and row.dtype == np.int64
            assert row.tolist() == want, (i, j)
    # default positions: sampling_num draws from 0..8, shared across the images
    rows = make_super_resolution_rows(model, tok, texts, imgs, sampling_num=4)
    assert len(rows) == 8 and len(seen["positions"]) == 4 and all(0 <= p <= 8 for p in seen["positions"])
    t0, t1 = len(texts[0]), len(texts[1])
    assert [int(rows[j][t0 + 5 + 1024]) for j in range(4)] == [int(rows[4 + j][t1 + 5 + 1024]) for j in range(4)] == [POS0 + p for p in seen["positions"]]
    with pytest.raises(NotImplementedError):
        make_super_resolution_rows(model, tok, texts, imgs, img_size=256)


def test_super_resolution_file_round_trip(tmp_path, monkeypatch):
    from cogview_amd.data_utils import BinaryDataset, compact_super_resolution_row, make_super_resolution_rows, super_resolution_to_compact_binary
    from cogview_amd.data_utils.preprocess import SR_ROW_CODES
    monkeypatch.setattr(ops, "sr_patches", IC.sr_patches_reference)
    monkeypatch.setattr(ops, "nchw3_to_nhwc4", lambda x: torch.nn.functional.pad(x.permute(0, 2, 3, 1), (0, 1)).contiguous())
    model = _StubModel()
    model.b = 2
    imgs, texts, positions = torch.zeros(2, 3, 512, 512), [[8200, 8201], [9000, 9001, 9002]], [7, 2]
    path = str(tmp_path / "sr.bin")
    assert super_resolution_to_compact_binary(model, texts, imgs, path, sampling_num=2, positions=positions) == 4
    ds = BinaryDataset(path, compact_super_resolution_row, length_per_sample=64 + SR_ROW_CODES)
    rows = make_super_resolution_rows(model, None, texts, imgs, sampling_num=2, positions=positions)
    assert len(ds) == 4
    for i in range(4):
        assert np.array_equal(ds[i], rows[i])
