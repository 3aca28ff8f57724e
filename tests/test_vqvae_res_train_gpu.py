"""GPU: tokenizer training for ResBlock and 3x3 topologies (opt-in, VQVAE.set_train_topologies("all")) -- the 3x3 weight
gradient, the weight gradient against max(x, 0) (relu_x) for every kind, the 32-wide output-channel tile, and whole models
against the plain-torch restatement (tests/vqvae_res_train_cases.py) and the reference's own training steps
(tests/golden/vqvae_train_res.npz); train_step, decoder-only fine-tuning, eval after training; the refusals without the opt-in.

Bars as in tests/test_vqvae_train_gpu.py: tensors within relative L2 1e-5 of CPU torch in fp32, every kernel comparison twice
and the two runs bitwise equal; ids equal to the restatement's except at near-ties (at most 1 % of the pixels, asserted), and
everything downstream of the ids compared with the restatement FED the device's ids.
"""
import pytest
import torch
import torch.nn.functional as F

from tests import vqvae_res_train_cases as R
from tests import vqvae_train_cases as T

pytestmark = pytest.mark.gpu
rel = T.rel

CONV, CONVT, ONE, C3 = "conv", "convT", "1x1", "3x3"
# (B, H, W, Cin, Cout) of the 3x3 layer: only the centre tap inside the image; one contraction step; odd sizes and K = 1224
# ending in a ragged k-tile; Cout across a 128 tile edge; several splits; the two narrow-tile shapes
C3_CELLS = [(1, 1, 1, 8, 8), (1, 4, 4, 8, 8), (2, 5, 7, 136, 24), (1, 3, 3, 8, 136), (3, 32, 48, 16, 40), (2, 8, 8, 32, 8), (2, 8, 8, 8, 32)]
RELU_X_CELLS = [(C3, 2, 5, 7, 136, 24, 1), (ONE, 2, 9, 11, 136, 264, 0), (CONV, 2, 6, 10, 8, 40, 0), (CONVT, 2, 5, 7, 8, 8, 0),
                (ONE, 2, 9, 11, 136, 24, 1), (CONV, 2, 6, 10, 8, 32, 1), (CONVT, 2, 5, 7, 8, 8, 1)]


def _case(kind, B, H, W, Cin, Cout, relu_x=False):
    """(x NCHW, dy NCHW, weight gradient by CPU autograd -- against relu(x) with relu_x --, kernel kind, unpack).  With relu_x
    a tenth of x is +0.0 and a tenth -0.0."""
    from cogview_amd import _lib as L
    from cogview_amd.vqvae.vqvae_zc import unpack_conv_weight_grad, unpack_convt_weight_grad
    g = torch.Generator().manual_seed(B * 1000 + H * 100 + Cin * 10 + Cout)
    x = torch.randn(B, Cin, H, W, generator=g)
    if relu_x:
        u = torch.rand(x.shape, generator=g)
        x = torch.where(u < 0.1, torch.zeros_like(x), torch.where(u < 0.2, torch.full_like(x, -0.0), x))
        assert bool((x == 0).any()) and bool(torch.signbit(x[x == 0]).any()) and bool((~torch.signbit(x[x == 0])).any())
    xin = F.relu(x) if relu_x else x
    if kind == CONV:
        w = torch.zeros(Cout, Cin, 4, 4, requires_grad=True)
        y, k, unpack = F.conv2d(xin, w, stride=2, padding=1), L.CONV_4X4_S2, unpack_conv_weight_grad
    elif kind == CONVT:
        w = torch.zeros(Cin, Cout, 4, 4, requires_grad=True)
        y, k, unpack = F.conv_transpose2d(xin, w, stride=2, padding=1), L.CONVT_4X4_S2, unpack_convt_weight_grad
    elif kind == C3:
        w = torch.zeros(Cout, Cin, 3, 3, requires_grad=True)
        y, k, unpack = F.conv2d(xin, w, padding=1), L.CONV_3X3_S1, unpack_conv_weight_grad
    else:
        w = torch.zeros(Cout, Cin, 1, 1, requires_grad=True)
        y, k, unpack = F.conv2d(xin, w), L.CONV_1X1, unpack_conv_weight_grad
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy)
    return x, dy, w.grad, k, unpack


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().cuda()


@pytest.mark.parametrize("B,H,W,Cin,Cout", C3_CELLS)
def test_3x3_weight_gradient_cells(B, H, W, Cin, Cout):
    """cogv_conv_wgrad_nhwc_f32 on COGV_CONV_3X3_S1 (topologies=1) against CPU autograd, twice, bitwise equal."""
    from cogview_amd import ops
    x, dy, ref, k, unpack = _case(C3, B, H, W, Cin, Cout)
    xh, dyh = _nhwc(x), _nhwc(dy)
    runs = [unpack(ops.conv_wgrad(k, xh, dyh, topologies=1), ref.shape) for _ in range(2)]
    for r in runs:
        e = rel(r, ref)
        print(f"wgrad 3x3 {(B, H, W, Cin, Cout)}: rel {e:.2e}")
        assert e < 1e-5
    assert torch.equal(runs[0], runs[1]), "two runs differ bitwise"


def test_3x3_cells_cover_the_plans():
    """The cells above do run several splits, one contraction step, a ragged last k-tile, two Cout tiles and the narrow tile
    (host-side plan query); without the opt-in the launch itself is refused."""
    from cogview_amd import _lib as L
    from cogview_amd import ops
    rc, p = L.conv_wgrad_plan(L.CONV_3X3_S1, 3, 32, 48, 16, 40, topologies=1)
    assert rc == L.OK and p["splits"] > 1 and p["k_tiles"] == 2 and p["cout_tiles"] == 1
    rc, p = L.conv_wgrad_plan(L.CONV_3X3_S1, 1, 4, 4, 8, 8, topologies=1)
    assert rc == L.OK and p["splits"] == 1 and p["span"] == 32 and p["k_tiles"] == 1
    rc, p = L.conv_wgrad_plan(L.CONV_3X3_S1, 2, 5, 7, 136, 24, topologies=1)
    assert rc == L.OK and p["k_tiles"] == 10 and 9 * 136 % 128 != 0
    rc, p = L.conv_wgrad_plan(L.CONV_3X3_S1, 1, 3, 3, 8, 136, topologies=1)
    assert rc == L.OK and p["cout_tiles"] == 2
    for cin, cout in ((32, 8), (8, 32)):
        rc, p = L.conv_wgrad_plan(L.CONV_3X3_S1, 2, 8, 8, cin, cout, topologies=1)
        assert rc == L.OK and p["cout_tiles"] == 1
    assert L.conv_wgrad_plan(L.CONV_3X3_S1, 2, 8, 8, 8, 40, topologies=1)[1]["cout_tiles"] == 1       # 40 > 32: one 128-wide tile
    xh = torch.zeros(1, 4, 4, 8, device="cuda")
    with pytest.raises(L.CogviewHipError):
        ops.conv_wgrad(L.CONV_3X3_S1, xh, xh)


@pytest.mark.parametrize("kind,B,H,W,Cin,Cout,topologies", RELU_X_CELLS)
def test_weight_gradient_against_relu_of_x(kind, B, H, W, Cin, Cout, topologies):
    """relu_x=1 on every kind (and on both tile widths): x holds exact zeros of both signs; the result is autograd's weight
    gradient on F.relu(x), twice, bitwise equal; the same call without the flag is a different tensor."""
    from cogview_amd import ops
    x, dy, ref, k, unpack = _case(kind, B, H, W, Cin, Cout, relu_x=True)
    xh, dyh = _nhwc(x), _nhwc(dy)
    runs = [unpack(ops.conv_wgrad(k, xh, dyh, relu_x=1, topologies=topologies), ref.shape) for _ in range(2)]
    for r in runs:
        e = rel(r, ref)
        print(f"wgrad relu_x {kind} {(B, H, W, Cin, Cout)} topologies {topologies}: rel {e:.2e}")
        assert e < 1e-5
    assert torch.equal(runs[0], runs[1]), "two runs differ bitwise"
    plain = unpack(ops.conv_wgrad(k, xh, dyh, topologies=topologies), ref.shape)
    assert rel(plain, ref) > 1e-3
    # the kernel's ReLU is the forward kernel's: feeding relu(x) without the flag gives the same bits
    assert torch.equal(unpack(ops.conv_wgrad(k, torch.relu(xh), dyh, topologies=topologies), ref.shape), runs[0])


@pytest.mark.parametrize("kind,B,H,W,Cin,Cout", [(ONE, 2, 8, 8, 32, 8), (ONE, 3, 32, 48, 16, 32), (CONV, 2, 6, 10, 8, 24), (CONVT, 2, 5, 7, 8, 8)])
def test_narrow_tile_adds_in_the_wide_tile_order(kind, B, H, W, Cin, Cout):
    """Cout <= 32: the 32-wide tile (topologies=1) and the 128-wide tile (topologies=0) plan the same splits and add every
    element's pixels in the same order -- the same bits."""
    from cogview_amd import _lib as L
    from cogview_amd import ops
    x, dy, ref, k, unpack = _case(kind, B, H, W, Cin, Cout)
    xh, dyh = _nhwc(x), _nhwc(dy)
    assert L.conv_wgrad_plan(k, B, H, W, Cin, Cout, topologies=1) == L.conv_wgrad_plan(k, B, H, W, Cin, Cout)
    narrow, wide = ops.conv_wgrad(k, xh, dyh, topologies=1), ops.conv_wgrad(k, xh, dyh)
    assert rel(unpack(narrow, ref.shape), ref) < 1e-5
    assert torch.equal(narrow, wide)


# ---- whole models
CONFIG_1X1T = dict(stride=6, simple=False, channel=16, n_res_block=1, n_res_channel=8, embed_dim=8, n_embed=32)
CONFIG_OFF_TILE = dict(channel=136, n_res_block=1, n_res_channel=40, embed_dim=24, n_embed=50, stride=6, simple=False)


def _model(config, state, opt_in=True):
    from cogview_amd.vqvae.vqvae_zc import VQVAE
    m = VQVAE(**config)
    m.load_state_dict(state)
    return m.set_train_topologies("all" if opt_in else "plain").cuda().train()


def _forward_backward(model, img, w=0.25):
    quant, diff, ids = model.encode(img)
    dec = model.dec(quant)
    loss = F.mse_loss(dec, img) + w * diff.mean()
    loss.backward()
    return dec.detach(), diff.detach(), ids, loss.detach()


def _check_against(model, dec, diff, ids, loss, ref):
    e = {"dec": rel(dec, ref["dec"]), "diff": rel(diff.reshape(()), ref["diff"].reshape(())), "loss": rel(loss, ref["loss"])}
    for k, p in model.named_parameters():
        assert p.grad is not None, k
        e["grad " + k] = rel(p.grad, ref["grads"][k])
    for k, v in ref["buffers"].items():
        e["after " + k] = rel(model.state_dict()[k], v)
    for k, v in e.items():
        print(f"  {k}: rel {v:.2e}")
    bad = {k: v for k, v in e.items() if not v < 1e-5}
    assert not bad, bad


def _whole_model(config, state, img):
    model = _model(config, state)
    dec, diff, ids, loss = _forward_backward(model, img.cuda())
    oracle = R.train_forward_backward(R.model_spec(model), state, img, ids=ids)
    assert dec.shape == oracle["dec"].shape and diff.shape == (1,)
    share, ok = T.ids_acceptable(ids, oracle["dist"], oracle["flat"], state["quantize_t.embed"])
    assert share <= 0.01 and ok, share
    _check_against(model, dec, diff, ids, loss, oracle)
    return model, dec, diff, ids, loss


@pytest.mark.parametrize("name,config", [("i", R.CONFIG_I), ("iii", R.CONFIG_III)])
def test_whole_model_against_the_reference_training_steps(golden_dir, name, config):
    """The fixture's two configurations on the fixture's inputs: against the restatement fed the device's ids, and -- the ids
    being the reference's -- against the reference's own dec / diff / loss / gradients / buffers."""
    g, state = R.fixture(golden_dir, name)
    model, dec, diff, ids, loss = _whole_model(config, state, g["img"])
    assert ids.shape == g["ids"].shape
    if torch.equal(ids.cpu(), g["ids"]):          # (always, unless a near-tie was resolved the other way)
        _check_against(model, dec, diff, ids, loss, R.fixture_reference(g))


@pytest.mark.parametrize("config,shape,seed", [(CONFIG_1X1T, (2, 3, 16, 24), 5), (CONFIG_OFF_TILE, (1, 3, 16, 24), 3), ({}, (1, 3, 16, 16), 7)],
                         ids=["1x1-transposed", "off-tile", "default-arguments"])
def test_whole_model_against_the_restatement(config, shape, seed):
    """simple=False with one ResBlock (the 1x1 transposed layer); channel 136 / n_res_channel 40 / embed_dim 24 / 50 codes
    (nothing a multiple of a tile); VQVAE() with its own default arguments."""
    from cogview_amd.vqvae.vqvae_zc import VQVAE
    state = T.random_state(VQVAE(**config).state_dict(), seed)
    _whole_model(config, state, torch.randn(*shape, generator=torch.Generator().manual_seed(seed + 1)))


def test_stride_2_encoder_against_the_restatement():
    """The stride-2 encoder alone (its VQVAE cannot form a loss: the stride-0 decoder's output has `channel` channels), with a
    seeded output gradient: conv4x4 + ReLU, conv3x3, ResBlock, ReLU, conv1x1."""
    from cogview_amd.vqvae.vqvae_zc import VQVAE
    model = VQVAE(channel=16, n_res_block=1, n_res_channel=8, embed_dim=8, n_embed=32, stride=2)
    state = T.random_state(model.state_dict(), 9)
    model.load_state_dict(state)
    enc = model.set_train_topologies("all").cuda().train().enc_b
    g = torch.Generator().manual_seed(10)
    img, gy = torch.randn(2, 3, 12, 20, generator=g), torch.randn(2, 6, 10, 8, generator=g)
    y = enc(img.cuda())
    y.backward(gy.cuda())
    p = {k: v.clone().requires_grad_(True) for k, v in state.items() if k.startswith("enc_b.")}
    want = R.run_blocks(p, "enc_b", R.block_spec(enc.blocks), img).permute(0, 2, 3, 1)
    want.backward(gy)
    e = {"out": rel(y, want)}
    e.update({k: rel(q.grad, p["enc_b." + k].grad) for k, q in enc.named_parameters()})
    print(e)
    assert all(v < 1e-5 for v in e.values()), e


def test_two_train_steps_see_updated_weights_and_codebook(golden_dir):
    """Two vqvae.train_step calls on configuration i with SGD(lr=0.1) against two restatement steps, judged by the SECOND
    step, as tests/test_vqvae_train_gpu.py does for the production topology."""
    from cogview_amd import vqvae
    g, state = R.fixture(golden_dir, "i")
    model = _model(R.CONFIG_I, state)
    spec = R.model_spec(model)
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    seen = {"ids": [], "dec": []}
    inner = model.quantize_t.forward_

    def spy(*a, **k):
        out = inner(*a, **k)
        seen["ids"].append(out[2].detach().clone())
        return out
    model.quantize_t.forward_ = spy
    model.dec.register_forward_hook(lambda mod, inp, out: seen["dec"].append(out.detach().clone()))
    imgs = [g["img"], torch.randn(2, 3, 32, 48, generator=torch.Generator().manual_seed(11))]
    losses = [vqvae.train_step(model, opt, im.cuda()) for im in imgs]
    st = state
    for step, im in enumerate(imgs):
        oracle = R.train_forward_backward(spec, st, im, ids=seen["ids"][step])
        share, ok = T.ids_acceptable(seen["ids"][step], oracle["dist"], oracle["flat"], st["quantize_t.embed"])
        assert share <= 0.01 and ok, step
        st = T.sgd_step(st, oracle, 0.1)
    e_loss, e_dec = rel(losses[1]["loss"], oracle["loss"]), rel(seen["dec"][1], oracle["dec"])
    print(f"second step: loss rel {e_loss:.2e}, dec rel {e_dec:.2e}; losses {losses[0]['loss'].item():.6f} -> {losses[1]['loss'].item():.6f}")
    assert e_loss < 1e-5 and e_dec < 1e-5
    assert rel(losses[1]["recon_loss"], oracle["recon_loss"]) < 1e-5 and rel(losses[1]["latent_loss"], oracle["diff"]) < 1e-5
    first = R.train_forward_backward(spec, state, imgs[1], ids=seen["ids"][1])
    assert rel(first["dec"], oracle["dec"]) > 1e-4           # the step did change what the second forward used


def test_decoder_only_fine_tuning(golden_dir):
    """Configuration i with enc_b frozen and quantize_t in eval mode: ids and buffers untouched, no encoder gradient, decoder
    gradients bitwise equal to the full run's."""
    g, state = R.fixture(golden_dir, "i")
    img = g["img"].cuda()
    full = _model(R.CONFIG_I, state)
    _, _, ids_full, _ = _forward_backward(full, img)
    part = _model(R.CONFIG_I, state)
    part.enc_b.requires_grad_(False)
    part.quantize_t.eval()
    _, _, ids, _ = _forward_backward(part, img)
    assert torch.equal(ids, ids_full)
    for k in T.BUFFERS:
        assert torch.equal(part.state_dict()[k].cpu(), state[k]), k
        assert not torch.equal(full.state_dict()[k].cpu(), state[k]), k
    assert all(p.grad is None for p in part.enc_b.parameters())
    for (k, a), (_, b) in zip(part.dec.named_parameters(), full.dec.named_parameters()):
        assert a.grad is not None and torch.equal(a.grad, b.grad), k


def test_eval_after_training_matches_a_fresh_model(golden_dir):
    """Configuration i: img2code / code2img after a training step equal those of a fresh eval model loaded from the trained
    state dict (no stale packed weights or codebook tables)."""
    from cogview_amd import vqvae
    from cogview_amd.vqvae.vqvae_zc import VQVAE
    g, state = R.fixture(golden_dir, "i")
    img = g["img"].cuda()
    model = _model(R.CONFIG_I, state).eval()
    ids0 = vqvae.img2code(model, img)                     # fills the eval-mode caches before training
    model.train()
    vqvae.train_step(model, torch.optim.SGD(model.parameters(), lr=0.1), img)
    model.eval()
    ids1 = vqvae.img2code(model, img)
    fresh = VQVAE(**R.CONFIG_I)
    fresh.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    fresh = fresh.cuda().eval()
    assert torch.equal(ids1, vqvae.img2code(fresh, img))
    assert torch.equal(vqvae.code2img(model, ids1.view(2, 4, 6)), vqvae.code2img(fresh, ids1.view(2, 4, 6)))
    untrained = VQVAE(**R.CONFIG_I)
    untrained.load_state_dict(state)
    assert torch.equal(ids0, vqvae.img2code(untrained.cuda().eval(), img))


@pytest.mark.parametrize("config,shape", [(R.CONFIG_I, (2, 3, 32, 48)), (R.CONFIG_III, (2, 3, 16, 24)), ({}, (1, 3, 16, 16))],
                         ids=["i", "iii", "default-arguments"])
def test_without_the_opt_in_training_still_raises(config, shape):
    from cogview_amd.vqvae.vqvae_zc import VQVAE
    model = _model(config, VQVAE(**config).state_dict(), opt_in=False)
    assert model.train_topologies == "plain"
    with pytest.raises(NotImplementedError, match="ResBlock|3x3"):
        model(torch.zeros(*shape, device="cuda"))
