"""CPU: the pieces of tokenizer training for ResBlock and 3x3 topologies (opt-in, VQVAE.set_train_topologies("all")) that need
no device -- the restatement of any block list (tests/vqvae_res_train_cases.py) against the reference's own training steps
(tests/golden/vqvae_train_res.npz, written by tools/gen_vqvae_train_res_golden.py), the repack of a 3x3 weight for its data
gradient, the weight-gradient plan under topologies=1, and the switch itself."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from cogview_amd import _lib as L
from tests import vqvae_res_train_cases as R
from tests import vqvae_train_cases as T


def test_fixture_is_small_and_data_only(golden_dir):
    path = os.path.join(golden_dir, "vqvae_train_res.npz")
    assert os.path.getsize(path) < 256 * 1024
    z = np.load(path, allow_pickle=False)
    assert all(z[k].dtype in (np.float32, np.int64) for k in z.files)
    assert {k.split(".")[0] for k in z.files} == {"i", "iii"}


@pytest.mark.parametrize("name,config", [("i", R.CONFIG_I), ("iii", R.CONFIG_III)])
def test_restatement_reproduces_the_reference_training_steps(golden_dir, name, config):
    """Tolerances as tests/test_vqvae_train_cpu.py::test_restatement_reproduces_the_reference_training_step."""
    from cogview_amd.vqvae.vqvae_zc import VQVAE
    g, state = R.fixture(golden_dir, name)
    spec = R.model_spec(VQVAE(**config))
    out = R.train_forward_backward(spec, state, g["img"])
    assert torch.equal(out["ids"], g["ids"])
    assert len(set(out["ids"].reshape(-1).tolist())) >= 8
    assert T.near_ties(out["dist"], out["flat"], state["quantize_t.embed"]).double().mean().item() <= 0.01
    assert torch.allclose(out["dec"], g["dec"], rtol=1e-5, atol=1e-6)
    assert torch.allclose(out["diff"], g["diff"].reshape(()), rtol=1e-5, atol=0)
    assert torch.allclose(out["loss"], g["loss"], rtol=1e-5, atol=0)
    assert set(out["grads"]) == {k[5:] for k in g if k.startswith("grad.")}
    for k, grad in out["grads"].items():
        ref = g["grad." + k]
        assert torch.allclose(grad, ref, rtol=1e-4, atol=1e-6 * ref.abs().max().item()), k
    for k, v in out["buffers"].items():
        assert torch.allclose(v, g["after." + k], rtol=1e-5, atol=1e-7), k
    again = R.train_forward_backward(spec, state, g["img"], ids=g["ids"])
    assert torch.equal(again["dec"], out["dec"])


@pytest.mark.parametrize("cin,cout,cin_x,cout_p", [(8, 8, 8, 8), (6, 10, 8, 16), (136, 24, 136, 24), (3, 40, 4, 40)])
def test_3x3_data_gradient_repack(cin, cout, cin_x, cout_p):
    """_dgrad_weight of a 3x3 layer: a 3x3 convolution of the output gradient with the repacked weight -- in and out
    swapped, both tap axes flipped -- is autograd's input gradient; the channel padding is zeros."""
    from cogview_amd.vqvae.vqvae_zc import _dgrad_weight, unpack_conv_weight_grad
    gen = torch.Generator().manual_seed(cin * 100 + cout)
    m = nn.Conv2d(cin, cout, 3, padding=1)
    with torch.no_grad():
        m.weight.copy_(torch.randn(m.weight.shape, generator=gen))
    x = torch.randn(2, cin, 5, 7, generator=gen, requires_grad=True)
    g = torch.randn(2, cout, 5, 7, generator=gen)
    F.conv2d(x, m.weight, m.bias, padding=1).backward(g)
    kind, packed = _dgrad_weight(m, L.CONV_3X3_S1, cin_x, cout_p)
    assert kind == L.CONV_3X3_S1 and tuple(packed.shape) == (cin_x, 9, cout_p) and packed.is_contiguous()
    w2 = unpack_conv_weight_grad(packed, (cin, cout, 3, 3))
    assert torch.equal(w2, m.weight.detach().permute(1, 0, 2, 3).flip(2, 3))
    assert T.rel(F.conv2d(g, w2, padding=1), x.grad) < 1e-6
    assert packed[cin:].abs().sum().item() == 0 and packed[:, :, cout:].abs().sum().item() == 0


def test_weight_gradient_plan_under_topologies():
    """Host only: topologies=1 lifts the 3x3 refusal (K = 9 Cin) and tiles Cout <= 32 in 32-wide tiles; topologies=0 plans
    what it always did; the two new fields take 0 / 1 only; relu_x changes no plan."""
    rc, p = L.conv_wgrad_plan(L.CONV_3X3_S1, 1, 8, 8, 8, 8, topologies=1)
    assert rc == L.OK and p["k_tiles"] == 1 and p["parities"] == 1
    assert L.conv_wgrad_plan(L.CONV_3X3_S1, 1, 8, 8, 8, 8, topologies=0)[0] == L.ERR_UNSUPPORTED
    assert L.conv_wgrad_plan(L.CONV_3X3_S1, 1, 8, 8, 8, 8, relu_x=1)[0] == L.ERR_UNSUPPORTED
    rc, p = L.conv_wgrad_plan(L.CONV_3X3_S1, 2, 5, 7, 136, 24, topologies=1)
    assert rc == L.OK and p["k_tiles"] == (9 * 136 + 127) // 128 == 10
    for kind in (L.CONV_3X3_S1, L.CONV_1X1, L.CONV_4X4_S2, L.CONVT_4X4_S2):
        for cout in (8, 24, 32, 40, 128, 136, 264):
            rc, wide = L.conv_wgrad_plan(kind, 2, 8, 8, 8, cout, topologies=1)
            assert rc == L.OK and wide["cout_tiles"] == ((cout + 31) // 32 if cout <= 32 else (cout + 127) // 128), (kind, cout)
            if kind != L.CONV_3X3_S1:
                rc, plain = L.conv_wgrad_plan(kind, 2, 8, 8, 8, cout)
                assert rc == L.OK and plain["cout_tiles"] == (cout + 127) // 128
                assert L.conv_wgrad_plan(kind, 2, 8, 8, 8, cout, relu_x=1) == (rc, plain)
    assert L.conv_wgrad_plan(L.CONV_1X1, 2, 8, 8, 8, 8, topologies=2)[0] == L.ERR_ARG
    assert L.conv_wgrad_plan(L.CONV_1X1, 2, 8, 8, 8, 8, relu_x=2)[0] == L.ERR_ARG
    assert L.conv_wgrad_plan(L.CONV_1X1, 2, 8, 8, 8, 8, topologies=-1)[0] == L.ERR_ARG
    # the workspace follows the plan, and a launch without pointers is refused before anything runs
    d = L.ConvWgradDesc()
    d.kind, d.B, d.IH, d.IW, d.Cin, d.Cout, d.splits, d.topologies = L.CONV_3X3_S1, 2, 8, 8, 8, 8, 4, 1
    assert L.lib().cogv_conv_wgrad_workspace_bytes(d) == 4 * 8 * 72 * 4
    assert L.lib().cogv_conv_wgrad_nhwc_f32(d, None) == L.ERR_ARG
    d.topologies = 0
    assert L.lib().cogv_conv_wgrad_workspace_bytes(d) == 0
    assert L.lib().cogv_conv_wgrad_nhwc_f32(d, None) == L.ERR_UNSUPPORTED


def test_the_switch():
    """set_train_topologies: "plain" by default, stored on both stacks, returns the model, refuses an unknown value; under
    "all" the Gumbel-softmax branch still raises; train_block_list refuses an unknown setting."""
    from cogview_amd import vqvae
    from cogview_amd.vqvae.vqvae_zc import VQVAE, train_block_list
    m = VQVAE(channel=16, n_res_block=1, n_res_channel=8, embed_dim=8, n_embed=16, stride=6)
    assert m.train_topologies == "plain" and m.enc_b._train_topologies == "plain" and m.dec._train_topologies == "plain"
    assert vqvae.set_train_topologies(m, "all") is m
    assert m.train_topologies == "all" and m.enc_b._train_topologies == "all" and m.dec._train_topologies == "all"
    with pytest.raises(ValueError, match="plain"):
        m.set_train_topologies("everything")
    assert m.train_topologies == "all"
    m.train()
    with pytest.raises(NotImplementedError, match="Gumbel-softmax"):
        m.quantize_t.forward_(torch.zeros(1, 2, 2, 8), continuous_relax=True)
    with pytest.raises(ValueError, match="plain"):
        train_block_list(m.enc_b.blocks, torch.zeros(1, 8, 8, 4), topologies="some")
    assert m.set_train_topologies("plain") is m
    with pytest.raises(NotImplementedError, match="ResBlock"):
        m.enc_b.forward_nhwc4(torch.zeros(1, 8, 8, 4))


def test_restatement_block_specs():
    """The helper reads the structure of every topology: ResBlocks, 3x3, the 1x1 transposed layer."""
    from cogview_amd.vqvae.vqvae_zc import VQVAE
    enc, dec = R.model_spec(VQVAE())
    assert [s[0] for s in enc] == ["conv", "relu", "conv", "relu", "conv", "res", "res", "relu", "conv"] and enc[4][1:] == ((1, 1), (1, 1))
    assert [s[0] for s in dec] == ["convT", "res", "res", "relu", "convT"]
    enc, dec = R.model_spec(VQVAE(stride=6, simple=False, channel=16, n_res_block=1, n_res_channel=8))
    assert [s[0] for s in dec] == ["convT", "res", "relu", "convT", "relu", "convT", "relu", "convT"] and dec[5][1:] == ((1, 1), (0, 0))
