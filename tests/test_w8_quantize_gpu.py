"""GPU: the row-wise E4M3 weight quantizer (cogv_quantize_rows_e4m3 through ops.quantize_rows_e4m3) against the same two
operations on the CPU, bit for bit: scale = row abs-max / 448 in fp32 (1.0 for a zero row), q = torch's float8_e4m3fn
conversion (round to nearest even, 460 -> 448) of w.float() / scale."""
import pytest
import torch

pytestmark = pytest.mark.gpu

E4M3 = torch.float8_e4m3fn


def _codes():
    """every finite non-negative E4M3 value, ascending (bytes 0x00 .. 0x7e)"""
    return torch.arange(0x7f, dtype=torch.uint8).view(E4M3).float()


def _weights(N, K, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    big = (torch.randn(N, K + 64, generator=g) * 0.05).to(dtype)          # rows K + 64 apart: a non-contiguous row stride
    w = big[:, :K]
    w[0] = 0                                                              # an all-zero row
    w[1] = 0
    w[1, K - 3] = -0.37                                                   # a single nonzero
    # quotients exactly on E4M3 ties: midpoints of neighbouring codes, times a power-of-two scale (row maximum 448 / 16,
    # so scale = 1 / 16 and the division is exact); every midpoint has 4 significant bits: exact in fp16 and bf16
    c = _codes()
    mid = (c[:-1] + c[1:]) / 2
    row = torch.cat([mid, -mid, torch.tensor([448.0])]) / 16
    assert row.numel() <= K
    w[2] = 0
    w[2, :row.numel()] = row.to(dtype)
    assert torch.equal(w[2, :row.numel()].float(), row)
    w[3, 5], w[3, 6] = -0.0, 0.0                                          # a row containing -0.0
    return w


def _cpu_reference(w):
    amax = w.float().abs().amax(dim=1)
    scale = torch.where(amax == 0, torch.ones_like(amax), amax / 448.0)
    q = (w.float() / scale[:, None]).to(E4M3).view(torch.uint8)
    return q, scale


def test_cpu_conversion_is_what_the_docstring_says():
    x = torch.tensor([460.0, 17.0, 19.0, -0.0])         # 460 -> 448; 17 and 19 are ties of the 16 / 18 / 20 grid: to even
    assert (x.to(E4M3).float() == torch.tensor([448.0, 16.0, 20.0, 0.0])).all()
    assert x.to(E4M3).view(torch.uint8)[3] == 0x80


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("N,K", [(24, 512), (8, 2560)])
def test_quantizer_matches_the_cpu_bit_for_bit(dtype, N, K):
    from cogview_amd import ops
    w = _weights(N, K, dtype, seed=N + K)
    assert not w.is_contiguous()
    q_ref, s_ref = _cpu_reference(w)
    wd = torch.empty_strided(w.shape, w.stride(), dtype=dtype, device="cuda").copy_(w)
    assert wd.stride() == w.stride()
    q, s = ops.quantize_rows_e4m3(wd)
    assert q.dtype == torch.uint8 and q.shape == (N, K) and s.dtype == torch.float32 and s.shape == (N,)
    assert torch.equal(s.cpu().view(torch.int32), s_ref.view(torch.int32)), "scales must be bit-equal"
    bad = (q.cpu() != q_ref).nonzero()
    assert bad.numel() == 0, (bad[:8].tolist(), q.cpu()[q.cpu() != q_ref][:8].tolist(), q_ref[q.cpu() != q_ref][:8].tolist())
    qc = q.cpu()
    assert s_ref[0] == 1.0 and bool(((qc[0] == 0) | (qc[0] == 0x80)).all())                  # the zero row
    assert int((qc[1] & 0x7f != 0).sum()) == 1 and qc[1, K - 3] == 0xfe                       # -448: the row's maximum
    assert s_ref[2] == 1.0 / 16 and qc[2].max() <= 0xfe and int((qc[2] & 0x7f).max()) == 0x7e
    assert qc[3, 5] == 0x80 and qc[3, 6] == 0x00                                              # the sign of zero survives
    assert int((qc & 0x7f).max()) <= 0x7e, "no NaN byte: nothing leaves the representable range"
    again_q, again_s = ops.quantize_rows_e4m3(wd)
    assert torch.equal(again_q, q) and torch.equal(again_s, s)
