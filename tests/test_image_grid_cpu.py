"""CPU: the host side of the image egress.  cogv_image_grid_plan's geometry is make_grid's for the whole case list, one
image comes back without padding, and every refusal is answered from the host copy of the source table before anything
could be launched (no call here passes the checks: there is no device).  The inputs of the GPU test hold the
edge values its cases need."""
import ctypes as C

import numpy as np
import pytest
import torch

from cogview_amd import _lib as L
from cogview_amd import ops
from tests import image_grid_cases as GC


def _table(*sources, ptr=0x10000):
    """int32 [K, 8] source table of (n, h, w, factor) batches at made-up, 16-byte aligned addresses that nothing reads."""
    t = np.zeros((len(sources), 8), dtype=np.uint32)
    first = 0
    for k, (n, h, w, f) in enumerate(sources):
        t[k] = (ptr & 0xffffffff, ptr >> 32, n, h, w, f, first, 0)
        first += n
        ptr += 0x100000
    return t.view(np.int32)


@pytest.mark.parametrize("H,W", GC.SHAPES)
def test_plan_is_make_grid_geometry(H, W):
    for B, nrow, padding, _ in GC.grid_cases():
        want = GC.make_grid(torch.zeros(B, 3, H, W), nrow=nrow, padding=padding)
        for each in (False, True):
            rc, plan = L.image_grid_plan(B, H, W, nrow, padding, each, _table((B, H, W, 1)))
            assert rc == L.OK, (B, nrow, padding)
            assert (plan["grid_h"], plan["grid_w"]) == tuple(want.shape[1:]), (B, nrow, padding)
            assert plan["out_bytes"] == want.numel()
            assert plan["range_bytes"] == 8 * (B if each else 1)
            if B > 1:
                assert plan["xmaps"] == min(nrow, B) and plan["ymaps"] == -(-B // plan["xmaps"])


def test_one_image_has_no_padding():
    rc, plan = L.image_grid_plan(1, 9, 10, 8, 5)
    assert rc == L.OK and (plan["xmaps"], plan["ymaps"], plan["grid_h"], plan["grid_w"], plan["out_bytes"]) == (1, 1, 9, 10, 270)
    assert tuple(GC.grid_bytes(torch.zeros(1, 3, 9, 10), padding=5).shape) == (9, 10, 3)


def test_two_sizes_in_one_grid_plan():
    # 24 images of 256 x 256 and 8 of 512 x 512 at 512: the super-resolution page of generate_samples.py:236-244
    rc, plan = L.image_grid_plan(32, 512, 512, 8, 2, False, _table((24, 256, 256, 2), (8, 512, 512, 1)))
    assert rc == L.OK and (plan["grid_h"], plan["grid_w"]) == (514 * 4 + 2, 514 * 8 + 2)


def _codes(which, table, B, H, W, nrow=8, padding=2, norm=L.GRID_NORM_NONE, low=0.0, high=1.0, out=0x20000, out_bytes=1 << 40,
           rng=0x30000, K=None):
    """The codes of the entry points named in `which` (p: the plan, r: the range launch, g: the grid launch) for one set of
    arguments.  The device pointers are made up, so an entry point is only named where it refuses the arguments."""
    K = table.shape[0] if K is None else K
    th = C.c_void_p(table.ctypes.data)
    plan = (C.c_int64 * L.IMAGE_GRID_PLAN_INTS)()
    lib = L.lib()
    calls = {"p": lambda: lib.cogv_image_grid_plan(th, K, B, H, W, nrow, padding, 0, plan),
             "r": lambda: lib.cogv_image_range_f32(C.c_void_p(0x40000), th, K, B, H, W, 0, C.c_void_p(rng), 1 << 20, None),
             "g": lambda: lib.cogv_image_grid_u8(C.c_void_p(0x40000), th, K, B, H, W, nrow, padding, 0.0, norm, C.c_void_p(rng), low,
                                                 high, C.c_void_p(out), out_bytes, None)}
    return tuple(calls[c]() for c in which)


def test_refusals_of_sources_and_replication():
    A, U = L.ERR_ARG, L.ERR_UNSUPPORTED
    ok = _table((2, 8, 8, 1))
    # other factors, or a source that does not reach H x W with its factor
    assert _codes("prg", _table((2, 8, 8, 3)), 2, 24, 24) == (U, U, U)
    assert _codes("prg", _table((2, 8, 8, 16)), 2, 128, 128) == (U, U, U)
    assert _codes("prg", _table((2, 5, 8, 2)), 2, 9, 16) == (U, U, U)
    assert _codes("prg", _table((2, 8, 5, 2)), 2, 16, 9) == (U, U, U)
    assert _codes("prg", _table((1, 8, 8, 1), (1, 4, 4, 1)), 2, 8, 8) == (U, U, U)
    # B == 0, B > 65535; nrow and padding are the grid's alone
    assert _codes("prg", _table((1, 8, 8, 1)), 0, 8, 8) == (A, A, A)
    assert _codes("prg", _table((65536, 8, 8, 1)), 65536, 8, 8) == (A, A, A)
    assert _codes("pg", ok, 2, 8, 8, nrow=0) == (A, A)
    assert _codes("pg", ok, 2, 8, 8, nrow=-1) == (A, A)
    assert _codes("pg", ok, 2, 8, 8, padding=-1) == (A, A)
    # a null or misaligned source; batches that do not add up to B; no batch at all
    assert _codes("prg", _table((2, 8, 8, 1), ptr=0), 2, 8, 8) == (A, A, A)
    assert _codes("prg", _table((2, 8, 8, 1), ptr=0x10008), 2, 8, 8) == (A, A, A)
    assert _codes("prg", ok, 3, 8, 8) == (A, A, A)
    assert _codes("prg", ok, 2, 8, 8, K=0) == (A, A, A)
    # value_range upside down; an out smaller than the grid or misaligned; a range pointer missing where one is read
    assert _codes("g", ok, 2, 8, 8, norm=L.GRID_NORM_FIXED, low=1.0, high=0.5) == (A,)
    assert _codes("g", ok, 2, 8, 8, out_bytes=12 * 22 * 3 - 1) == (A,)
    assert _codes("g", ok, 2, 8, 8, out=0x20004) == (A,)
    assert _codes("rg", ok, 2, 8, 8, norm=L.GRID_NORM_RANGE, rng=0) == (A, A)
    assert _codes("g", ok, 2, 8, 8, norm=7) == (A,)
    # a range workspace smaller than the plan's
    th = C.c_void_p(ok.ctypes.data)
    assert L.lib().cogv_image_range_f32(C.c_void_p(0x40000), th, 1, 2, 8, 8, 1, C.c_void_p(0x30000), 15, None) == A
    # sizes beyond the limits
    assert L.image_grid_plan(2, 32769, 8)[0] == U and L.image_grid_plan(2, 8, 8, padding=32769)[0] == U
    assert L.image_grid_plan(65535, 32768, 32768, nrow=1)[0] == U


def test_wrapper_refuses_before_the_library():
    with pytest.raises(L.CogviewHipError):
        ops.image_grid(torch.zeros(2, 3, 8, 8))                       # CPU tensors: no fallback
    with pytest.raises(L.CogviewHipError):
        ops.image_grid([torch.zeros(3, 8, 8)])
    with pytest.raises(ValueError):
        ops.image_grid([])


def test_inputs_hold_what_the_cases_need():
    """Extremes in the first and the last element, a constant image, values outside [0, 1], the (m + 0.5) / 255 values."""
    for H, W in GC.SHAPES:
        x = GC.images(5, H, W)
        assert x.view(-1)[0].item() == x.min().item() == -3.0 and x.view(-1)[-1].item() == x.max().item() == 4.0
        assert (x[1] == 0.25).all() and (x[2:] < 0).any() and (x[2:] > 1).any()
        t = x[0, 1].view(-1)[1:min(255, H * W)].mul(255).add_(0.5)
        assert (t - t.round()).abs().max().item() <= 2.0 ** -16           # within an ulp or two of an integer
        assert GC.images(1, H, W).max().item() == 4.0


def test_restatement_against_torchvision():
    tv = pytest.importorskip("torchvision.utils")
    for (H, W), B in zip(GC.SHAPES, (2, 5, 9)):
        x = GC.images(B, H, W)
        for kw in GC.MODES.values():
            for nrow, padding, pad_value in ((8, 2, 0.0), (3, 3, 0.5)):
                kw = dict(kw, nrow=nrow, padding=padding, pad_value=pad_value)
                want = tv.make_grid(x, **kw).mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to("cpu", torch.uint8)
                assert torch.equal(GC.grid_bytes(x, **kw), want)
