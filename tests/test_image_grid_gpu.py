"""GPU: the image egress kernels.  ops.image_grid's bytes equal make_grid + save_image's conversion as torch runs them on
CPU tensors (tests/image_grid_cases.py) -- equality, no tolerance -- for every geometry, normalisation and replication
factor; a given `out` is written inside its bounds only; two runs agree; code2img_u8 and save_image are that on the
decoder's own output."""
import io

import pytest
import torch

from cogview_amd import _lib as L
from cogview_amd import ops
from tests import image_grid_cases as GC

pytestmark = pytest.mark.gpu

_INPUTS = {}


def _inputs(B, H, W):
    """(CPU images, the same on the device), made once per shape and shared."""
    key = (B, H, W)
    if key not in _INPUTS:
        x = GC.images(B, H, W)
        _INPUTS[key] = (x, x.cuda())
    return _INPUTS[key]


@pytest.mark.parametrize("mode", list(GC.MODES))
@pytest.mark.parametrize("H,W", GC.SHAPES)
def test_bytes_equal_the_restatement(H, W, mode):
    kw = GC.MODES[mode]
    for B, nrow, padding, pad_value in GC.grid_cases():
        x, xd = _inputs(B, H, W)
        args = dict(kw, nrow=nrow, padding=padding, pad_value=pad_value)
        want = GC.grid_bytes(x, **args)
        got = ops.image_grid(xd, **args)
        assert got.dtype == torch.uint8 and got.shape == want.shape, (B, nrow, padding, pad_value)
        assert torch.equal(got.cpu(), want), (B, nrow, padding, pad_value)


def test_one_image_without_batch_dimension():
    x, xd = _inputs(1, 9, 10)
    got = ops.image_grid(xd[0], padding=3, pad_value=1.0)
    assert got.shape == (9, 10, 3) and torch.equal(got.cpu(), GC.grid_bytes(x[0], padding=3, pad_value=1.0))


@pytest.mark.parametrize("mode", ["none", "normalize", "scale_each"])
def test_factors_1_2_4_8_in_one_grid(mode):
    g = torch.Generator().manual_seed(21)
    srcs = [torch.randn(n, 3, h, w, generator=g) * 0.5 + 0.5 for n, h, w in ((1, 32, 40), (2, 16, 20), (3, 8, 10), (1, 4, 5))]
    srcs[1].view(-1)[0], srcs[2].view(-1)[-1] = -2.5, 3.5          # the extremes are in replicated sources
    kw = dict(GC.MODES[mode], nrow=4, padding=3, pad_value=0.5)
    want = GC.grid_bytes(GC.replicate(srcs, (32, 40)), **kw)
    got = ops.image_grid([s.cuda() for s in srcs], **kw)
    assert torch.equal(got.cpu(), want)
    # size= names the target: the same sources at twice the size (factors 2, 4, 8 and one the kernel does not take)
    want = GC.grid_bytes(GC.replicate(srcs[:3], (64, 80)), **kw)
    assert torch.equal(ops.image_grid([s.cuda() for s in srcs[:3]], size=(64, 80), **kw).cpu(), want)
    with pytest.raises(L.CogviewHipError, match="unsupported"):
        ops.image_grid([s.cuda() for s in srcs], size=(64, 80), **kw)
    with pytest.raises(L.CogviewHipError, match="unsupported"):
        ops.image_grid([srcs[0].cuda(), torch.zeros(1, 3, 16, 16).cuda()])


def test_given_out_is_written_inside_its_bounds():
    x, xd = _inputs(5, 9, 10)
    kw = dict(nrow=3, padding=3, normalize=True)
    want = GC.grid_bytes(x, **kw)
    n = want.numel()
    assert n % 16 != 0                                             # the grid ends inside a 16-byte store
    buf = torch.full((16 + n + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    got = ops.image_grid(xd, out=buf[16:16 + n], **kw)
    assert got.data_ptr() == buf.data_ptr() + 16 and got.shape == want.shape
    assert torch.equal(got.cpu(), want)
    assert (buf[:16] == 0xA5).all() and (buf[16 + n:] == 0xA5).all()
    buf.fill_(0xA5)
    with pytest.raises(ValueError):
        ops.image_grid(xd, out=buf[16:16 + n - 1], **kw)           # smaller than the grid
    with pytest.raises(L.CogviewHipError, match="bad argument"):
        ops.image_grid(xd, out=buf[4:4 + n], **kw)                 # not 16-byte aligned
    with pytest.raises(L.CogviewHipError, match="bad argument"):
        ops.image_grid(xd, out=buf[16:16 + n], **dict(kw, value_range=(1.0, 0.0)))
    assert (buf == 0xA5).all()


def test_two_runs_give_the_same_bytes():
    x, xd = _inputs(9, 24, 40)
    for kw in (dict(normalize=True), dict(normalize=True, scale_each=True)):
        a = ops.image_grid(xd, nrow=3, **kw).clone()
        b = ops.image_grid(xd, nrow=3, **kw)
        assert torch.equal(a, b)


def test_both_launches_are_captured_and_replayed():
    """Nothing is read back between the range and the grid launch, so the pair goes into a graph; replayed on new values in
    the same tensors it gives their bytes."""
    x = GC.images(5, 24, 40)
    xd = x.cuda()
    kw = dict(nrow=3, normalize=True, scale_each=True)
    out = torch.zeros(GC.grid_bytes(x, **kw).numel(), dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.image_grid(xd, out=out, **kw)                          # the source table is on the device from here on
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.image_grid(xd, out=out, **kw)
    x2 = GC.images(5, 24, 40, seed=1)
    xd.copy_(x2)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu().view(-1), GC.grid_bytes(x2, **kw).view(-1))


def _small_vqvae():
    from cogview_amd.vqvae.vqvae_zc import VQVAE
    torch.manual_seed(11)
    return VQVAE(channel=128, n_res_block=0, n_res_channel=32, embed_dim=16, n_embed=64, stride=6).cuda().eval()


def test_code2img_u8_is_the_restatement_of_code2img():
    from cogview_amd.vqvae import code2img, code2img_u8
    m = _small_vqvae()
    g = torch.Generator().manual_seed(3)
    c16 = torch.randint(0, 64, (2, 16, 16), generator=g).cuda()
    c32 = torch.randint(0, 64, (1, 32, 32), generator=g).cuda()
    kw = dict(nrow=2, padding=2, normalize=True)
    got = code2img_u8(m, [c16, c32], **kw)
    imgs = [code2img(m, c16).cpu(), code2img(m, c32).cpu()]
    assert imgs[0].shape == (2, 3, 128, 128) and imgs[1].shape == (1, 3, 256, 256)
    want = GC.grid_bytes(GC.replicate(imgs, (256, 256)), **kw)
    assert got.shape == (2 * 258 + 2, 2 * 258 + 2, 3) and torch.equal(got.cpu(), want)
    one = code2img_u8(m, c32)
    assert torch.equal(one.cpu(), GC.grid_bytes(imgs[1]))


def test_save_image_png_reads_back_equal():
    Image = pytest.importorskip("PIL.Image")
    import numpy as np
    from cogview_amd.vqvae import save_image
    x, xd = _inputs(5, 24, 40)
    fp = io.BytesIO()
    save_image(xd, fp, format="png", nrow=3, normalize=True)
    fp.seek(0)
    back = torch.from_numpy(np.array(Image.open(fp)))
    assert torch.equal(back, GC.grid_bytes(x, nrow=3, normalize=True))
