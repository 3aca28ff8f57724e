"""CPU: the ABI and the arithmetic restatement of the tokenizer's split-bf16 precision mode (no GPU needed): header mirror,
refusals before any launch, the three-limb split summing back to its input, the ResBlock restatement's shapes."""
import ctypes as C
import os
import re

import pytest
import torch

from cogview_amd import _lib as L
from tests import vqvae_split_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "cogview_hip.h")).read()


def test_conv_desc_ends_with_precision_and_w_limbs_in_header_order():
    body = re.search(r"typedef struct cogv_conv_desc \{(.*?)\} cogv_conv_desc;", _header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", part)[-1] for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    fields = [f[0] for f in L.ConvDesc._fields_]
    assert names == fields
    assert fields[-2:] == ["precision", "w_limbs"]
    assert dict(L.ConvDesc._fields_)["precision"] is C.c_int and dict(L.ConvDesc._fields_)["w_limbs"] is C.c_void_p
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"#define COGV_CONV_FP32 0\b", src) and re.search(r"#define COGV_CONV_BF16X3 1\b", src)
    assert (L.CONV_FP32, L.CONV_BF16X3) == (0, 1)


def test_split_weights_symbol_is_declared_bound_and_exported():
    src = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"int cogv_conv_split_weights\(const float\* w, void\* limbs, size_t n, void\* stream\);", src)
    assert "cogv_conv_split_weights" in L.SIGNATURES
    assert hasattr(L.lib(), "cogv_conv_split_weights")


def _null_desc():
    d = L.ConvDesc()
    d.kind, d.B, d.IH, d.IW, d.Cin, d.Cout = L.CONV_1X1, 1, 4, 4, 8, 8
    return d


def test_bad_precision_and_missing_limbs_are_refused_before_any_launch():
    assert "precision" in dict(L.ConvDesc._fields_) and "w_limbs" in dict(L.ConvDesc._fields_)
    lib = L.lib()
    d = _null_desc()
    d.precision = 7
    assert lib.cogv_conv2d_nhwc_f32(C.byref(d), None) == L.ERR_ARG
    d = _null_desc()
    d.precision = L.CONV_BF16X3
    assert lib.cogv_conv2d_nhwc_f32(C.byref(d), None) == L.ERR_ARG
    d.w_limbs = 0x1008                                       # misaligned (never dereferenced: the data pointers are null)
    assert lib.cogv_conv2d_nhwc_f32(C.byref(d), None) == L.ERR_ARG
    assert lib.cogv_conv_split_weights(None, None, 16, None) == L.ERR_ARG


def test_python_surface_refuses_unknown_modes_and_defaults_to_fp32():
    from cogview_amd import vqvae
    from cogview_amd.vqvae.vqvae_zc import VQVAE
    m = VQVAE(channel=16, n_res_block=0, embed_dim=8, n_embed=32, stride=6)
    assert m.precision == "fp32"
    assert m.set_precision("bf16x3") is m and m.precision == "bf16x3"
    assert vqvae.set_precision(m, "fp32") is m and m.precision == "fp32"
    with pytest.raises(ValueError):
        m.set_precision("bf16")
    with pytest.raises(AttributeError):
        m.precision = "bf16x3"                               # read-only
    assert m.precision == "fp32"


def test_three_limbs_sum_back_to_the_value():
    """Every limb is a bf16 value, limb 0 is the top 16 bits of x (so it carries the sign, of a zero too), and the limbs
    sum back to x exactly: (l0 + l1) + l2 == x in fp32 and l0 + l1 + l2 == x in fp64."""
    x = S.special_values()
    l = S.split3(x)
    assert (l.view(torch.int32) & 0xffff).eq(0).all()
    assert torch.equal(l[0].view(torch.int32), x.view(torch.int32) & -65536)
    back = (l[0] + l[1]) + l[2]
    assert torch.equal(back, x) and torch.isfinite(l).all()
    nz = x != 0
    assert torch.equal(back.view(torch.int32)[nz], x.view(torch.int32)[nz])          # bit for bit
    assert torch.equal(l.double().sum(0), x.double())
    assert torch.equal(torch.signbit(l[0]), torch.signbit(x))
    # a truncated bf16 leaves less than one unit of its 8-bit significand: limb 1 < 2^-7 |limb 0|, limb 2 < 2^-15 |limb 0|
    assert (l[1].abs() <= l[0].abs() * 2.0 ** -7).all() and (l[2].abs() <= l[0].abs() * 2.0 ** -15).all()
    b = S.limb_bits(x)
    assert b.dtype == torch.int16 and torch.equal((b.to(torch.int32) << 16).view(torch.float32), l)


def test_resblock_restatement_matches_the_module_structure():
    """The helper's restatement of the ResBlock topology reads every parameter of the module and produces its shapes."""
    from cogview_amd.vqvae.vqvae_zc import VQVAE
    m = VQVAE(**S.RES_CONFIG)
    state = m.state_dict()

    class Recording(dict):
        def __init__(self, d):
            super().__init__(d)
            self.used = set()

        def __getitem__(self, k):
            self.used.add(k)
            return super().__getitem__(k)

    p = Recording(state)
    logits = S.res_encoder(p, torch.randn(2, 3, 32, 32))
    assert logits.shape == (2, 8, 8, 16)
    img = S.res_decoder(p, logits)
    assert img.shape == (2, 3, 32, 32)
    assert p.used == {k for k in state if not k.startswith("quantize_t.")}
    assert m.precision == "fp32"
