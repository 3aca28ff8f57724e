"""CPU: the pieces of the VQ-VAE tokenizer's training path that need no device -- the plain-torch restatement
(tests/vqvae_train_cases.py) against the reference's own training step (tests/golden/vqvae_train.npz, written by
tools/gen_vqvae_train_golden.py), the inverse weight packings, the host-side plan of the weight-gradient kernel and the
refusals of what the training path does not cover."""
import os

import numpy as np
import pytest
import torch

from cogview_amd import _lib as L
from tests import vqvae_train_cases as T


def _fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "vqvae_train.npz"))
    g = {k: torch.from_numpy(z[k]) for k in z.files}
    return g, {k[6:]: v for k, v in g.items() if k.startswith("param.")}


def test_fixture_is_small_and_data_only(golden_dir):
    path = os.path.join(golden_dir, "vqvae_train.npz")
    assert os.path.getsize(path) < 256 * 1024
    z = np.load(path, allow_pickle=False)
    assert all(z[k].dtype in (np.float32, np.int64) for k in z.files)


def test_restatement_reproduces_the_reference_training_step(golden_dir):
    g, state = _fixture(golden_dir)
    out = T.train_forward_backward(state, g["img"])
    assert torch.equal(out["ids"], g["ids"])
    assert T.near_ties(out["dist"], out["flat"], state["quantize_t.embed"]).double().mean().item() <= 0.01
    assert torch.allclose(out["dec"], g["dec"], rtol=1e-5, atol=1e-6)
    assert torch.allclose(out["diff"], g["diff"].reshape(()), rtol=1e-5, atol=0)
    assert torch.allclose(out["loss"], g["loss"], rtol=1e-5, atol=0)
    for k, grad in out["grads"].items():
        ref = g["grad." + k]
        assert torch.allclose(grad, ref, rtol=1e-4, atol=1e-6 * ref.abs().max().item()), k
    for k, v in out["buffers"].items():
        assert torch.allclose(v, g["after." + k], rtol=1e-5, atol=1e-7), k
    # fed the ids explicitly, the restatement computes the same
    again = T.train_forward_backward(state, g["img"], ids=g["ids"])
    assert torch.equal(again["dec"], out["dec"])


@pytest.mark.parametrize("co,ci", [(8, 4), (16, 3), (3, 16), (24, 136), (40, 8)])
def test_pack_then_unpack_is_the_identity(co, ci):
    """Both packed layouts, with channel counts that the forward packing pads (Cin to 4, Cout to 8): unpacking the packed
    weight -- padded the way the layer's weight gradient arrives -- gives the parameter back, bit for bit."""
    from torch import nn
    from cogview_amd.vqvae.vqvae_zc import (_pack_generic, pack_conv_weight, pack_convt_weight, unpack_conv_weight_grad,
                                            unpack_convt_weight_grad)
    g = torch.Generator().manual_seed(co * 100 + ci)
    w = torch.randn(co, ci, 4, 4, generator=g)
    assert torch.equal(unpack_conv_weight_grad(pack_conv_weight(w), w.shape), w)
    w1 = torch.randn(co, ci, 1, 1, generator=g)
    assert torch.equal(unpack_conv_weight_grad(pack_conv_weight(w1), w1.shape), w1)
    wt = torch.randn(ci, co, 4, 4, generator=g)
    assert torch.equal(unpack_convt_weight_grad(pack_convt_weight(wt), wt.shape), wt)
    # as the modules pack them: output channels padded to 8, input channels to 4, zero filters in the padding
    conv = nn.Conv2d(ci, co, 4, stride=2, padding=1)
    kind, wp, bias, cout = _pack_generic(conv)
    assert kind == L.CONV_4X4_S2 and wp.shape[0] % 8 == 0 and wp.shape[2] % 4 == 0 and cout == co
    assert torch.equal(unpack_conv_weight_grad(wp, conv.weight.shape), conv.weight.detach())
    convt = nn.ConvTranspose2d(ci, co, 4, stride=2, padding=1)
    kind, wp, bias, cout = _pack_generic(convt)
    assert kind == L.CONVT_4X4_S2 and wp.shape[1] % 8 == 0 and wp.shape[3] % 4 == 0
    assert torch.equal(unpack_convt_weight_grad(wp, convt.weight.shape), convt.weight.detach())


def test_weight_gradient_plan_and_argument_checks():
    """Host only: splits where (tiles x parities) does not fill the chip, one split where they do; the refusals."""
    rc, first = L.conv_wgrad_plan(L.CONV_4X4_S2, 32, 256, 256, 4, 512)       # the image layer: 64 columns, 4 channel tiles
    assert rc == L.OK and first["splits"] > 1 and first["k_tiles"] == 1 and first["cout_tiles"] == 4
    assert first["span"] % 32 == 0 and first["span"] * first["splits"] >= 32 * 128 * 128 > first["span"] * (first["splits"] - 1)
    rc, mid = L.conv_wgrad_plan(L.CONV_4X4_S2, 32, 128, 128, 512, 512)
    assert rc == L.OK and mid["splits"] == 4 and mid["k_tiles"] == 64 and mid["workgroups"] == 1024
    rc, t = L.conv_wgrad_plan(L.CONVT_4X4_S2, 2, 8, 8, 24, 136)
    assert rc == L.OK and t["parities"] == 4 and t["cout_tiles"] == 2 and t["k_tiles"] == 1
    rc, forced = L.conv_wgrad_plan(L.CONV_1X1, 2, 8, 8, 32, 8, splits=4)
    assert rc == L.OK and forced["splits"] == 4 and forced["span"] == 32
    d = L.ConvWgradDesc()
    d.kind, d.B, d.IH, d.IW, d.Cin, d.Cout = L.CONV_1X1, 2, 8, 8, 32, 8
    assert L.lib().cogv_conv_wgrad_workspace_bytes(d) == 0
    d.splits = 4
    assert L.lib().cogv_conv_wgrad_workspace_bytes(d) == 4 * 8 * 32 * 4
    assert L.conv_wgrad_plan(L.CONV_3X3_S1, 1, 8, 8, 8, 8)[0] == L.ERR_UNSUPPORTED
    assert L.conv_wgrad_plan(L.CONV_1X1, 1, 8, 8, 6, 8)[0] == L.ERR_ARG           # Cin % 4
    assert L.conv_wgrad_plan(L.CONV_1X1, 1, 8, 8, 8, 12)[0] == L.ERR_ARG          # Cout % 8
    assert L.conv_wgrad_plan(L.CONV_4X4_S2, 1, 7, 8, 8, 8)[0] == L.ERR_ARG        # odd height
    # null and misaligned pointers are refused before any launch
    d = L.ConvWgradDesc()
    d.kind, d.B, d.IH, d.IW, d.Cin, d.Cout = L.CONV_1X1, 1, 4, 4, 8, 8
    assert L.lib().cogv_conv_wgrad_nhwc_f32(d, None) == L.ERR_ARG
    d.x, d.dy, d.dw = 0x1000, 0x2000, 0x3004
    assert L.lib().cogv_conv_wgrad_nhwc_f32(d, None) == L.ERR_ARG
    assert L.lib().cogv_relu_bias_bwd_f32(None, None, None, None, None, 0, 16, 8, None) == L.ERR_ARG
    assert L.lib().cogv_relu_bias_bwd_f32(0x1000, None, None, 0x2000, 0x3000, 1 << 20, 16, 6, None) == L.ERR_ARG     # C % 4
    assert L.lib().cogv_vq_code_stats_f32(None, None, None, None, None, 0, 16, 8, 4, None) == L.ERR_ARG
    assert L.lib().cogv_vq_ste_bwd_f32(None, None, 0x1000, 0x2000, 0x3000, 6, None) == L.ERR_ARG                    # n % 4
    assert L.lib().cogv_relu_bias_bwd_workspace_bytes(1000, 24) >= 24 * 4
    assert L.lib().cogv_vq_code_stats_workspace_bytes(1000, 24, 50) > 1000 * 4


def test_weight_gradient_descriptor_mirrors_the_header():
    """Field order of cogv_conv_wgrad_desc in include/cogview_hip.h == _lib.ConvWgradDesc (as tests/test_abi.py checks the
    other descriptors)."""
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "cogview_hip.h")).read()
    body = re.search(r"typedef struct cogv_conv_wgrad_desc \{(.*?)\} cogv_conv_wgrad_desc;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.findall(r"[A-Za-z_][A-Za-z0-9_]*", part)[-1] for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    assert names == [f[0] for f in L.ConvWgradDesc._fields_]


def test_training_mode_refusals_name_what_is_missing():
    """ResBlock topologies, 3x3 encoders and continuous_relax=True raise in training mode before any kernel runs, and say
    which piece is missing."""
    from cogview_amd.vqvae.vqvae_zc import VQVAE, Quantize, train_block_list
    x = torch.zeros(1, 8, 8, 4)
    m = VQVAE(channel=16, n_res_block=1, n_res_channel=8, embed_dim=8, n_embed=16, stride=6).train()
    with pytest.raises(NotImplementedError, match="ResBlock"):
        train_block_list(m.enc_b.blocks, x)
    with pytest.raises(NotImplementedError, match="ResBlock"):
        m.enc_b.forward_nhwc4(x)
    with pytest.raises(NotImplementedError, match="ResBlock"):
        m.dec.forward_nhwc(torch.zeros(1, 1, 1, 8))
    m = VQVAE(channel=16, n_res_block=0, embed_dim=8, n_embed=16, stride=4).train()
    with pytest.raises(NotImplementedError, match="3x3"):
        m.enc_b.forward_nhwc4(x)
    q = Quantize(8, 16).train()
    with pytest.raises(NotImplementedError, match="Gumbel-softmax"):
        q.forward_(torch.zeros(1, 2, 2, 8), continuous_relax=True)
    with pytest.raises(NotImplementedError, match="Gumbel-softmax"):
        q.eval().forward_(torch.zeros(1, 2, 2, 8), continuous_relax=True)
