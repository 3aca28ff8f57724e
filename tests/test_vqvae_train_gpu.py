"""GPU: the VQ-VAE tokenizer's training path -- weight gradient, ReLU mask + bias gradient, codebook statistics + EMA update,
the whole model's forward / backward against the reference's own training step (tests/golden/vqvae_train.npz) and the
plain-torch restatement (tests/vqvae_train_cases.py), train_step, decoder-only fine-tuning, eval after training.

Bars as in tests/test_vqvae_gpu.py: tensors within relative L2 1e-5 of CPU torch in fp32, every kernel comparison twice (and
the two runs bitwise equal: no sum here depends on timing); ids equal to the restatement's except at near-ties (at most 1 % of
the pixels, asserted), and everything downstream of the ids compared with the restatement FED the device's ids.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import vqvae_train_cases as T

pytestmark = pytest.mark.gpu
rel = T.rel

CONV, CONVT, ONE = "conv", "convT", "1x1"
WGRAD_CELLS = [
    (CONV, 1, 4, 4, 4, 8), (CONV, 2, 6, 10, 8, 40), (CONV, 1, 8, 8, 136, 24), (CONV, 2, 16, 24, 32, 136), (CONV, 3, 32, 48, 16, 16),
    (CONVT, 2, 5, 7, 8, 8), (CONVT, 1, 8, 8, 136, 40), (CONVT, 2, 12, 20, 24, 136),
    (ONE, 1, 4, 4, 16, 8), (ONE, 2, 9, 11, 136, 264), (ONE, 2, 8, 8, 32, 8),
]


def _wgrad_case(kind, B, H, W, Cin, Cout):
    """(x NCHW, dy NCHW, reference weight gradient by CPU autograd, kernel kind, unpack)"""
    from cogview_amd import _lib as L
    from cogview_amd.vqvae.vqvae_zc import unpack_conv_weight_grad, unpack_convt_weight_grad
    g = torch.Generator().manual_seed(B * 1000 + H * 100 + Cin * 10 + Cout)
    x = torch.randn(B, Cin, H, W, generator=g)
    if Cin == 4:
        x[:, 3] = 0                                           # the image layer: channel 3 is padding
    if kind == CONV:
        w = torch.zeros(Cout, Cin, 4, 4, requires_grad=True)
        y = F.conv2d(x, w, stride=2, padding=1)
        k, unpack = L.CONV_4X4_S2, unpack_conv_weight_grad
    elif kind == CONVT:
        w = torch.zeros(Cin, Cout, 4, 4, requires_grad=True)
        y = F.conv_transpose2d(x, w, stride=2, padding=1)
        k, unpack = L.CONVT_4X4_S2, unpack_convt_weight_grad
    else:
        w = torch.zeros(Cout, Cin, 1, 1, requires_grad=True)
        y = F.conv2d(x, w)
        k, unpack = L.CONV_1X1, unpack_conv_weight_grad
    dy = torch.randn(y.shape, generator=g)
    y.backward(dy)
    return x, dy, w.grad, k, unpack


@pytest.mark.parametrize("kind,B,H,W,Cin,Cout", WGRAD_CELLS)
def test_weight_gradient_cells(kind, B, H, W, Cin, Cout):
    """cogv_conv_wgrad_nhwc_f32 against CPU autograd: odd and non-square sizes (border taps), channel counts across the
    128-tile edge, Cin = 4 and Cout = 8, a pixel count above one split (slabs + reduce), one contraction step only."""
    from cogview_amd import ops
    x, dy, ref, k, unpack = _wgrad_case(kind, B, H, W, Cin, Cout)
    xh, dyh = x.permute(0, 2, 3, 1).contiguous().cuda(), dy.permute(0, 2, 3, 1).contiguous().cuda()
    runs = [unpack(ops.conv_wgrad(k, xh, dyh), ref.shape) for _ in range(2)]
    for r in runs:
        e = rel(r, ref)
        print(f"wgrad {kind} {(B, H, W, Cin, Cout)}: rel {e:.2e}")
        assert e < 1e-5
    assert torch.equal(runs[0], runs[1]), "two runs differ bitwise"


def test_weight_gradient_cells_cover_both_plans():
    """The cells above do run the split path and the single-step path (host-side plan query)."""
    from cogview_amd import _lib as L
    rc, p = L.conv_wgrad_plan(L.CONV_4X4_S2, 3, 32, 48, 16, 16)
    assert rc == L.OK and p["splits"] > 1
    rc, p = L.conv_wgrad_plan(L.CONV_4X4_S2, 1, 4, 4, 4, 8)
    assert rc == L.OK and p["splits"] == 1 and p["span"] == 32 and p["k_tiles"] == 1


def test_weight_gradient_split_counts_agree():
    """One cell with two forced split counts: different summation orders, same sum."""
    from cogview_amd import _lib as L
    from cogview_amd import ops
    x, dy, ref, k, unpack = _wgrad_case(CONV, 2, 16, 24, 32, 136)
    xh, dyh = x.permute(0, 2, 3, 1).contiguous().cuda(), dy.permute(0, 2, 3, 1).contiguous().cuda()
    assert L.conv_wgrad_plan(k, 2, 16, 24, 32, 136, splits=2)[1]["splits"] == 2
    assert L.conv_wgrad_plan(k, 2, 16, 24, 32, 136, splits=3)[1]["splits"] == 3
    a, b = ops.conv_wgrad(k, xh, dyh, splits=2), ops.conv_wgrad(k, xh, dyh, splits=3)
    one = ops.conv_wgrad(k, xh, dyh, splits=1)
    e = rel(a, b)
    print(f"splits 2 vs 3: rel {e:.2e}; vs 1: {rel(a, one):.2e}")
    assert e < 1e-5 and rel(a, one) < 1e-5
    assert rel(unpack(a, ref.shape), ref) < 1e-5 and rel(unpack(b, ref.shape), ref) < 1e-5


@pytest.mark.parametrize("M,C", [(777, 136), (5000, 8), (70, 1032), (3, 24)])
def test_relu_mask_and_bias_gradient(M, C):
    """dx = dy * (A > 0) exactly (both zeros of A mask), db = the column sums of dx within 1e-5 of fp64, run to run bitwise."""
    from cogview_amd import ops
    g = torch.Generator().manual_seed(M + C)
    dy = torch.randn(M, C, generator=g)
    a = torch.relu(torch.randn(M, C, generator=g))
    a[::3] = torch.where(a[::3] == 0, torch.full_like(a[::3], -0.0), a[::3])       # a third of the rows: zeros become -0.0
    assert bool((a == 0).any()) and bool(torch.signbit(a).any())
    want = torch.where(a > 0, dy, torch.zeros_like(dy))
    outs = [ops.relu_bias_bwd(dy.cuda(), a.cuda()) for _ in range(2)]
    for dx, db in outs:
        assert torch.equal(dx.cpu(), want)
        e = rel(db, want.double().sum(0))
        print(f"relu/bias {M}x{C}: db rel {e:.2e}")
        assert e < 1e-5
    assert torch.equal(outs[0][1], outs[1][1])
    # without a ReLU: the bias gradient alone, dx is dy
    dyc = dy.cuda()
    dx, db = ops.relu_bias_bwd(dyc, None)
    assert dx.data_ptr() == dyc.data_ptr() and rel(db, dy.double().sum(0)) < 1e-5
    assert torch.equal(db, ops.relu_bias_bwd(dyc, None)[1])


def _stats_case(M, D, NE, skew):
    g = torch.Generator().manual_seed(M + D + NE)
    x = torch.randn(M, D, generator=g)
    if skew:
        used = torch.tensor([1, 2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47])      # the other codes own no pixel
        ids = used[torch.randint(0, len(used), (M,), generator=g)]
        ids[torch.randperm(M, generator=g)[:600]] = 7                                          # one code owns 600 pixels
    else:
        ids = torch.randint(0, NE, (M,), generator=g)
    return x, ids


@pytest.mark.parametrize("M,D,NE,skew", [(1000, 24, 50, True), (4096, 256, 8192, False)])
def test_codebook_statistics_and_ema_update(M, D, NE, skew):
    """count / sum through the inverted index: counts exact, sums within 1e-5 of fp64, two runs bitwise equal; a list longer
    than one sum chunk (600 > 256) and codes without pixels; then the EMA update against the restatement, empty codes
    keeping embed_avg * decay."""
    from cogview_amd import ops
    x, ids = _stats_case(M, D, NE, skew)
    count_ref = torch.bincount(ids, minlength=NE)
    if skew:
        assert count_ref.max() >= 600 and (count_ref == 0).sum() >= 30
    sum_ref = torch.zeros(NE, D, dtype=torch.float64).index_add_(0, ids, x.double())
    runs = [ops.vq_code_stats(ids.cuda(), x.cuda(), NE) for _ in range(2)]
    for count, total in runs:
        assert torch.equal(count.cpu().long(), count_ref)
        e = rel(total, sum_ref)
        print(f"code stats {M}x{D}x{NE}: sum rel {e:.2e}")
        assert e < 1e-5
        assert bool((total.cpu()[count_ref == 0] == 0).all())
    assert torch.equal(runs[0][1], runs[1][1])
    g = torch.Generator().manual_seed(7)
    embed = torch.randn(D, NE, generator=g)
    cs = torch.rand(NE, generator=g) * 3
    avg = embed * cs.clamp_min(0.5)
    e_ref, cs_ref, avg_ref = T.ema_update(embed, cs, avg, ids, x)
    for _ in range(2):
        e_d, cs_d, avg_d = embed.clone().cuda(), cs.clone().cuda(), avg.clone().cuda()
        n = ops.vq_ema_update(runs[0][0], runs[0][1], cs_d, avg_d, e_d, 0.99, 1e-5)
        assert rel(cs_d, cs_ref) < 1e-5 and rel(avg_d, avg_ref) < 1e-5 and rel(e_d, e_ref) < 1e-5 and rel(n, cs_ref.sum()) < 1e-5
        empty = count_ref == 0
        assert torch.equal(avg_d.cpu()[:, empty], (avg * 0.99)[:, empty])


def _fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "vqvae_train.npz"))
    g = {k: torch.from_numpy(z[k]) for k in z.files}
    return g, {k[6:]: v for k, v in g.items() if k.startswith("param.")}


def _small_model(state):
    from cogview_amd.vqvae.vqvae_zc import VQVAE
    m = VQVAE(channel=16, n_res_block=0, embed_dim=8, n_embed=32, stride=6)
    m.load_state_dict(state)
    return m.cuda().train()


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


def test_whole_model_against_the_reference_training_step(golden_dir):
    """The fixture's configuration on the fixture's input: ids by the audit rule against the reference's, dec / diff / every
    parameter gradient / the three buffers after the EMA update within 1e-5 of the reference's own."""
    g, state = _fixture(golden_dir)
    model = _small_model(state)
    dec, diff, ids, loss = _forward_backward(model, g["img"].cuda())
    assert dec.shape == g["dec"].shape and diff.shape == (1,) and ids.shape == g["ids"].shape
    oracle = T.train_forward_backward(state, g["img"], ids=ids)
    share, ok = T.ids_acceptable(ids, oracle["dist"], oracle["flat"], state["quantize_t.embed"])
    assert share <= 0.01 and ok, (share, (ids.cpu() != g["ids"]).sum().item())
    _check_against(model, dec, diff, ids, loss, oracle)
    if torch.equal(ids.cpu(), g["ids"]):          # (always, unless a near-tie was resolved the other way)
        ref = dict(dec=g["dec"], diff=g["diff"], loss=g["loss"], grads={k[5:]: v for k, v in g.items() if k.startswith("grad.")},
                   buffers={k[6:]: v for k, v in g.items() if k.startswith("after.")})
        _check_against(model, dec, diff, ids, loss, ref)


def test_whole_model_off_tile_widths_against_the_restatement():
    """channel 136 (one more than a 128 tile plus padding), embed_dim 24, 50 codes, a [1, 3, 16, 24] image."""
    from cogview_amd.vqvae.vqvae_zc import VQVAE
    model = VQVAE(channel=136, n_res_block=0, embed_dim=24, n_embed=50, stride=6)
    state = T.random_state(model.state_dict(), 3)
    model.load_state_dict(state)
    model = model.cuda().train()
    img = torch.randn(1, 3, 16, 24, generator=torch.Generator().manual_seed(4))
    dec, diff, ids, loss = _forward_backward(model, img.cuda())
    oracle = T.train_forward_backward(state, img, ids=ids)
    share, ok = T.ids_acceptable(ids, oracle["dist"], oracle["flat"], state["quantize_t.embed"])
    assert share <= 0.01 and ok
    _check_against(model, dec, diff, ids, loss, oracle)


def test_two_train_steps_see_updated_weights_and_codebook(golden_dir):
    """Two vqvae.train_step calls with SGD(lr=0.1) against two restatement steps, judged by the loss and dec of the SECOND
    step: it is right only if the packed-weight caches saw the optimizer's update and the lookup saw the EMA's codebook."""
    from cogview_amd import vqvae
    g, state = _fixture(golden_dir)
    model = _small_model(state)
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
    assert all(v.is_cuda and v.dim() == 0 for v in losses[1].values()) and set(losses[1]) == {"loss", "recon_loss", "latent_loss"}
    st = state
    for step, im in enumerate(imgs):
        oracle = T.train_forward_backward(st, im, ids=seen["ids"][step])
        share, ok = T.ids_acceptable(seen["ids"][step], oracle["dist"], oracle["flat"], st["quantize_t.embed"])
        assert share <= 0.01 and ok, step
        st = T.sgd_step(st, oracle, 0.1)
    e_loss, e_dec = rel(losses[1]["loss"], oracle["loss"]), rel(seen["dec"][1], oracle["dec"])
    print(f"second step: loss rel {e_loss:.2e}, dec rel {e_dec:.2e}; losses {losses[0]['loss'].item():.6f} -> {losses[1]['loss'].item():.6f}")
    assert e_loss < 1e-5 and e_dec < 1e-5
    assert rel(losses[1]["recon_loss"], oracle["recon_loss"]) < 1e-5 and rel(losses[1]["latent_loss"], oracle["diff"]) < 1e-5
    # the step did change what the second forward used
    first = T.train_forward_backward(state, imgs[1], ids=seen["ids"][1])
    assert rel(first["dec"], oracle["dec"]) > 1e-4


def test_decoder_only_fine_tuning(golden_dir):
    """enc_b frozen and quantize_t in eval mode: ids and the three buffers bit-identical before and after, encoder gradients
    None, decoder gradients bitwise equal to the full run's (the decoder's input is the pre-update lookup in both)."""
    g, state = _fixture(golden_dir)
    img = g["img"].cuda()
    full = _small_model(state)
    _, _, ids_full, _ = _forward_backward(full, img)
    part = _small_model(state)
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
    _, _, ids_again = part.encode(img)
    assert torch.equal(ids_again, ids)


def test_eval_after_training_matches_a_fresh_model(golden_dir):
    """img2code after a training step equals img2code of a fresh eval model loaded from the trained state dict (no stale
    packed weights or codebook tables), and training left eval-mode results of an untrained copy alone."""
    from cogview_amd import vqvae
    from cogview_amd.vqvae.vqvae_zc import VQVAE
    g, state = _fixture(golden_dir)
    img = g["img"].cuda()
    model = _small_model(state).eval()
    ids0 = vqvae.img2code(model, img)                     # fills the eval-mode caches before training
    model.train()
    vqvae.train_step(model, torch.optim.SGD(model.parameters(), lr=0.1), img)
    model.eval()
    ids1 = vqvae.img2code(model, img)
    fresh = VQVAE(channel=16, n_res_block=0, embed_dim=8, n_embed=32, stride=6)
    fresh.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
    fresh = fresh.cuda().eval()
    assert torch.equal(ids1, vqvae.img2code(fresh, img))
    assert torch.equal(vqvae.code2img(model, ids1.view(2, 4, 6)), vqvae.code2img(fresh, ids1.view(2, 4, 6)))
    untrained = VQVAE(channel=16, n_res_block=0, embed_dim=8, n_embed=32, stride=6)
    untrained.load_state_dict(state)
    assert torch.equal(ids0, vqvae.img2code(untrained.cuda().eval(), img))
