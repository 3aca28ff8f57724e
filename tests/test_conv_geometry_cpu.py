"""CPU: the forward convolution (cogv_conv2d_nhwc_f32) and its weight gradient (cogv_conv_wgrad_nhwc_f32) take a layer's
geometry from one helper (csrc/conv_args.cuh conv_geometry), so both refuse the same bad geometry with the same code, before
any launch (no device here).  Pointer fields are non-null, 16-byte-aligned dummy integers that are never dereferenced."""
import ctypes as C

import pytest

from cogview_amd import _lib as L

FIELDS = ("kind", "B", "IH", "IW", "Cin", "Cout")
GOOD = dict(kind=L.CONV_1X1, B=1, IH=4, IW=4, Cin=8, Cout=8)


def _forward(**kw):
    d = L.ConvDesc()
    for k, v in {**GOOD, **kw}.items():
        setattr(d, k, v)
    setattr(d, "in", 0x1000)
    d.w, d.bias, d.out = 0x2000, 0x3000, 0x4000
    return d


def _wgrad(**kw):
    d = L.ConvWgradDesc()
    for k, v in {**GOOD, **kw}.items():
        setattr(d, k, v)
    d.x, d.dy, d.dw = 0x1000, 0x2000, 0x3000
    return d


REFUSALS = [
    ("odd IH, 4x4 stride 2", dict(kind=L.CONV_4X4_S2, IH=5, IW=4), L.ERR_ARG),
    ("odd IW, 4x4 stride 2", dict(kind=L.CONV_4X4_S2, IH=4, IW=7), L.ERR_ARG),
    ("unknown kind", dict(kind=97), L.ERR_UNSUPPORTED),
    ("Cin % 4", dict(Cin=6), L.ERR_ARG),
    ("Cout % 8", dict(Cout=12), L.ERR_ARG),
    ("B * IH * IW = 2^31", dict(B=32768, IH=256, IW=256), L.ERR_ARG),
]


@pytest.mark.parametrize("name,kw,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_forward_and_weight_gradient_refuse_the_same_geometry_with_the_same_code(name, kw, code):
    lib = L.lib()
    assert lib.cogv_conv2d_nhwc_f32(C.byref(_forward(**kw)), None) == code
    assert lib.cogv_conv_wgrad_nhwc_f32(C.byref(_wgrad(**kw)), None) == code
    assert lib.cogv_conv_wgrad_plan(C.byref(_wgrad(**kw)), None) == code
    d = _forward(**kw)                                        # the split-bf16 form refuses through the same check
    d.precision, d.w_limbs = L.CONV_BF16X3, 0x5000
    assert lib.cogv_conv2d_nhwc_f32(C.byref(d), None) == code


def test_half_the_overflowing_batch_is_not_refused_for_its_geometry():
    """B * IH * IW = 2^30 fits.  Only the weight gradient has a launch-free path for a valid descriptor (its plan query), and
    it reads the geometry the forward path reads; the forward entry point itself would launch, so it is not called."""
    kw = dict(B=16384, IH=256, IW=256)
    plan = (C.c_int * 6)()
    assert L.lib().cogv_conv_wgrad_plan(C.byref(_wgrad(**kw)), plan) == L.OK
    assert plan[0] >= 1 and plan[5] == 1
    rc, fields = L.conv_wgrad_plan(L.CONV_1X1, 16384, 256, 256, 8, 8)
    assert rc == L.OK and fields


def test_weight_gradient_still_has_no_3x3():
    assert L.lib().cogv_conv_wgrad_plan(C.byref(_wgrad(kind=L.CONV_3X3_S1)), None) == L.ERR_UNSUPPORTED
    assert L.lib().cogv_conv_wgrad_nhwc_f32(C.byref(_wgrad(kind=L.CONV_3X3_S1)), None) == L.ERR_UNSUPPORTED
