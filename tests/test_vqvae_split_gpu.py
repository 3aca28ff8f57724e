"""GPU: the tokenizer's split-bf16 precision mode ("bf16x3": three bf16 limbs per fp32 operand, six products, fp32
accumulation on v_mfma_f32_32x32x16_bf16).

Kernel cells: every kind, epilogue and the fused RGB partials against F.conv2d / F.conv_transpose2d in fp64 on the CPU;
relative Frobenius error < 1e-6 per cell (tests/vqvae_split_cases.py BOUND: one missing small product reads 2.4e-6), printed
next to the exact-fp32 kernel's error on the same cell; two runs bitwise equal.  Limb planes bitwise against the restatement.
Whole model, three configurations in both modes: ids by the audit rule of tests/test_vqvae_train_gpu.py, decoded images
against the fp64 restatement fed the device's ids, bytes of code2img_u8, mode switches, training ignoring the mode."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import image_grid_cases as GC
from tests import vqvae_split_cases as S
from tests import vqvae_train_cases as T

pytestmark = pytest.mark.gpu
rel = T.rel


def _check_cell(c, dev, name, ref, **run):
    split = [S.run_cell(c, dev, "bf16x3", **run) for _ in range(2)]
    exact = [S.run_cell(c, dev, "fp32", **run) for _ in range(2)]
    e_split, e_exact = rel(split[0], ref), rel(exact[0], ref)
    print(f"{name}: rel to fp64 bf16x3 {e_split:.2e}  exact fp32 {e_exact:.2e}")
    assert split[0].shape == ref.shape and torch.isfinite(split[0]).all()
    assert torch.equal(split[0], split[1]), "two bf16x3 runs differ bitwise"
    assert torch.equal(exact[0], exact[1]), "two fp32 runs differ bitwise"
    assert e_exact < 1e-5                  # the exact path's own bar (tests/test_vqvae_gpu.py); printed for comparison
    assert e_split < S.BOUND
    return split[0], exact[0]


@pytest.mark.parametrize("kind,B,H,W,Cin,Cout", S.CELLS)
def test_kernel_cells_against_fp64(kind, B, H, W, Cin, Cout):
    c = S.make_cell(kind, B, H, W, Cin, Cout)
    _check_cell(c, S.device_cell(c), f"{kind} {(B, H, W, Cin, Cout)}", S.reference(c))


@pytest.mark.parametrize("epilogue", S.EPILOGUES)
@pytest.mark.parametrize("kind,B,H,W,Cin,Cout", S.EPILOGUE_CELLS)
def test_epilogues_against_fp64(kind, B, H, W, Cin, Cout, epilogue):
    c = S.make_cell(kind, B, H, W, Cin, Cout)
    if epilogue == "relu_in":
        assert (c["x"] < 0).any()
    _check_cell(c, S.device_cell(c), f"{kind} {(B, H, W, Cin, Cout)} {epilogue}", S.reference(c, epilogue), epilogue=epilogue)


@pytest.mark.parametrize("cell", S.RGB_CELLS, ids=lambda cell: "-".join(map(str, cell)))
def test_fused_rgb_partials_against_fp64(cell):
    """The last decoder layer's form: ReLU(convT) projected to RGB in the epilogue, cogv_rgb_finalize_f32 with scale and shift."""
    c = S.make_cell(*cell)
    scale, shift = (0.30379, 0.32279, 0.32800), (0.79093, 0.76271, 0.75340)
    _check_cell(c, S.device_cell(c), f"rgb {cell}", S.reference_rgb(c, scale, shift), rgb=(scale, shift))


@pytest.mark.parametrize("scale", [1e30, 1e-30])
def test_inputs_with_range(scale):
    c = S.make_cell(*S.RANGE_CELL, scale=scale)
    _check_cell(c, S.device_cell(c), f"{S.RANGE_CELL} x {scale:g}", S.reference(c))


def test_default_descriptor_is_the_exact_path():
    """precision left at zero, precision="fp32" and a set-but-unused w_limbs all give the exact kernel's bits."""
    from cogview_amd.vqvae.vqvae_zc import _conv
    c = S.make_cell(*S.CELLS[3])
    dev = S.device_cell(c)
    k, cout = S.kernel_kind(c["kind"]), c["bias"].numel()
    plain = _conv(k, dev["x"], dev["w"], dev["bias"], cout, False)
    assert torch.equal(plain, _conv(k, dev["x"], dev["w"], dev["bias"], cout, False, precision="fp32"))
    assert torch.equal(plain, _conv(k, dev["x"], dev["w"], dev["bias"], cout, False, precision="fp32", w_limbs=dev["limbs"]))
    assert not torch.equal(plain, _conv(k, dev["x"], dev["w"], dev["bias"], cout, False, precision="bf16x3", w_limbs=dev["limbs"]))
    with pytest.raises(ValueError):
        _conv(k, dev["x"], dev["w"], dev["bias"], cout, False, precision="bf16x3")


def test_limb_planes_equal_the_restatement_bitwise():
    from cogview_amd.vqvae.vqvae_zc import split_weight_limbs
    x = S.special_values()
    assert torch.equal(split_weight_limbs(x.cuda()).cpu(), S.limb_bits(x))
    w = S.packed_weight(S.make_cell(*S.CELLS[6]))
    got = split_weight_limbs(w.cuda()).cpu()
    assert got.shape == (3,) + tuple(w.shape) and torch.equal(got, S.limb_bits(w))


# ---------------------------------------------------------------------------------------------- whole model
def _fixture(golden_dir):
    z = np.load(os.path.join(golden_dir, "vqvae_train.npz"))
    g = {k: torch.from_numpy(z[k]) for k in z.files}
    return g, {k[6:]: v for k, v in g.items() if k.startswith("param.")}


def _model(config, state, precision="fp32"):
    from cogview_amd.vqvae.vqvae_zc import VQVAE
    m = VQVAE(**config)
    m.load_state_dict(state)
    return m.cuda().eval().set_precision(precision)


FIXTURE_CONFIG = dict(channel=16, n_res_block=0, embed_dim=8, n_embed=32, stride=6)
OFF_TILE_CONFIG = dict(channel=136, n_res_block=0, embed_dim=24, n_embed=50, stride=6)


def _configuration(name, golden_dir):
    """(config, state, image, encoder restatement, decoder restatement)"""
    from cogview_amd.vqvae.vqvae_zc import VQVAE
    if name == "fixture":
        g, state = _fixture(golden_dir)
        return FIXTURE_CONFIG, state, g["img"], T.encoder, T.decoder
    if name == "off_tile":
        state = T.random_state(VQVAE(**OFF_TILE_CONFIG).state_dict(), 3)
        return OFF_TILE_CONFIG, state, torch.randn(1, 3, 16, 24, generator=torch.Generator().manual_seed(4)), T.encoder, T.decoder
    state = T.random_state(VQVAE(**S.RES_CONFIG).state_dict(), 5)
    return S.RES_CONFIG, state, torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(6)), S.res_encoder, S.res_decoder


@pytest.mark.parametrize("name", ["fixture", "off_tile", "resblocks"])
def test_whole_model_ids_and_images_in_both_modes(name, golden_dir):
    config, state, img, enc, dec = _configuration(name, golden_dir)
    model = _model(config, state)
    with torch.no_grad():
        ids_exact = model.encode_ids(img.cuda())
        model.set_precision("bf16x3")
        ids_split = model.encode_ids(img.cuda())
        dec_split = model.decode_code(ids_split)
        model.set_precision("fp32")
        dec_exact = model.decode_code(ids_split)
    embed = state["quantize_t.embed"]
    logits = enc(state, img)
    flat = logits.reshape(-1, logits.shape[-1])
    dist = T.distances(flat, embed)
    share, ok = T.ids_acceptable(ids_split, dist, flat, embed)
    share_exact, ok_exact = T.ids_acceptable(ids_exact, dist, flat, embed)
    differ = ids_split.reshape(-1).cpu() != ids_exact.reshape(-1).cpu()
    print(f"{name}: near-tie share {share:.4f}, ids differing between the modes {int(differ.sum())} of {differ.numel()}")
    assert share <= 0.01 and ok
    assert share_exact <= 0.01 and ok_exact
    assert bool((~differ | T.near_ties(dist, flat, embed)).all())
    p64 = {k: v.double() for k, v in state.items()}
    q64 = F.embedding(ids_split.cpu(), p64["quantize_t.embed"].t())
    dec64 = dec(p64, q64)
    e_split, e_exact = rel(dec_split, dec64), rel(dec_exact, dec64)
    print(f"{name}: decoded image rel to fp64 bf16x3 {e_split:.2e}  exact fp32 {e_exact:.2e}")
    assert dec_split.shape == dec64.shape
    assert e_split <= max(1e-6, 2 * e_exact)


def test_code2img_u8_bytes_in_split_mode():
    """Split mode's bytes are what torch's CPU operations make of split mode's own float images (the egress contract), and
    they differ from exact mode's bytes by at most one count on at most 0.1 % of the bytes.  channel = 128: the decoder's
    last layer runs the fused RGB partials."""
    from cogview_amd.vqvae import code2img, code2img_u8, set_precision
    from cogview_amd.vqvae.vqvae_zc import VQVAE
    torch.manual_seed(11)
    m = VQVAE(channel=128, n_res_block=0, n_res_channel=32, embed_dim=16, n_embed=64, stride=6).cuda().eval()
    code = torch.randint(0, 64, (2, 16, 16), generator=torch.Generator().manual_seed(3)).cuda()
    kw = dict(nrow=2, padding=2)
    exact = code2img_u8(m, code, **kw).cpu()
    set_precision(m, "bf16x3")
    got = code2img_u8(m, code, **kw).cpu()
    imgs = code2img(m, code).cpu()
    assert torch.equal(got, GC.grid_bytes(imgs, **kw))
    diff = (got.int() - exact.int()).abs()
    print(f"bytes differing between the modes: {int((diff > 0).sum())} of {diff.numel()}, largest {int(diff.max())}")
    assert int(diff.max()) <= 1 and (diff > 0).double().mean().item() <= 1e-3
    set_precision(m, "fp32")
    assert not torch.equal(imgs, code2img(m, code).cpu()), "the mode did not reach the decoder"


def test_switching_back_gives_the_never_switched_results(golden_dir):
    g, state = _fixture(golden_dir)
    img = g["img"].cuda()
    never, switched = _model(FIXTURE_CONFIG, state), _model(FIXTURE_CONFIG, state, "bf16x3")
    with torch.no_grad():
        ids = never.encode_ids(img)
        dec = never.decode_code(ids)
        dec_split = switched.decode_code(ids)
        switched.encode_ids(img)
        switched.set_precision("fp32")
        assert switched.precision == "fp32"
        assert torch.equal(switched.encode_ids(img), ids) and torch.equal(switched.decode_code(ids), dec)
    assert not torch.equal(dec_split, dec)


def test_split_mode_sees_new_weights_after_load_state_dict(golden_dir):
    from cogview_amd.vqvae.vqvae_zc import VQVAE
    g, state = _fixture(golden_dir)
    other = T.random_state(VQVAE(**FIXTURE_CONFIG).state_dict(), 21)
    img = g["img"].cuda()
    model, fresh = _model(FIXTURE_CONFIG, state, "bf16x3"), _model(FIXTURE_CONFIG, other, "bf16x3")
    with torch.no_grad():
        ids = fresh.encode_ids(img)
        before = model.decode_code(ids)                   # fills the caches with the first weights' limb planes
        model.encode_ids(img)
        model.load_state_dict(other)
        assert model.precision == "bf16x3"
        assert torch.equal(model.encode_ids(img), ids)
        after = model.decode_code(ids)
    assert torch.equal(after, fresh.decode_code(ids)) and not torch.equal(after, before)


def test_training_ignores_the_mode(golden_dir):
    """A model in .train() launches the exact-fp32 kernels whatever the mode: outputs and gradients of the fixture's step are
    bitwise equal in both settings."""
    g, state = _fixture(golden_dir)
    img = g["img"].cuda()
    out = {}
    for mode in ("fp32", "bf16x3"):
        m = _model(FIXTURE_CONFIG, state, mode).train()
        quant, diff, ids = m.encode(img)
        dec = m.dec(quant)
        (F.mse_loss(dec, img) + 0.25 * diff.mean()).backward()
        out[mode] = [dec.detach(), diff.detach(), ids] + [p.grad for _, p in sorted(m.named_parameters())] + \
                    [m.state_dict()[k] for k in T.BUFFERS]
        assert all(t is not None for t in out[mode])
    for a, b in zip(out["fp32"], out["bf16x3"]):
        assert torch.equal(a, b)
