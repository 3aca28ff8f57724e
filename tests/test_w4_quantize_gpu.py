"""GPU: the MXFP4 weight quantizer (cogv_quantize_rows_mxfp4) against the rule on the CPU (tests/w4_cases.py: quantize), bytes and
scale bytes equal with the sign of zero codes masked.  Rows ldw = K + 8 elements apart in; the outputs lie inside sentinel-filled
buffers with rows ldq = K / 2 + 16 and lds = K / 32 + 3 bytes apart."""
import ctypes as C

import pytest
import torch

from tests import gemv_cells as GC
from tests import w4_cases as W4

pytestmark = pytest.mark.gpu
SENTINEL = 0xEE


def _device_quantize(w_strided_cpu, pad_q=16, pad_s=3):
    """the device quantizer on a copy with the same row stride, into sentinel buffers -> (q, s, intact: the sentinels stand)"""
    from cogview_amd import _lib as L
    from cogview_amd import ops
    w = w_strided_cpu
    N, K = w.shape
    wd = torch.empty_strided(w.shape, w.stride(), dtype=w.dtype, device="cuda").copy_(w)
    assert wd.stride() == w.stride()
    ldq, lds = K // 2 + pad_q, K // 32 + pad_s
    qbuf = torch.full((N + 2, ldq), SENTINEL, dtype=torch.uint8, device="cuda")
    sbuf = torch.full((N + 2, lds), SENTINEL, dtype=torch.uint8, device="cuda")
    q, s = qbuf[1:N + 1, :K // 2], sbuf[1:N + 1, :K // 32]
    L.check(L.lib().cogv_quantize_rows_mxfp4(ops.dt_code(wd), wd.data_ptr(), wd.stride(0), N, K, q.data_ptr(), ldq, s.data_ptr(), lds, None),
            "cogv_quantize_rows_mxfp4")
    torch.cuda.synchronize()
    qc, sc = qbuf.cpu(), sbuf.cpu()
    intact = bool((qc[0] == SENTINEL).all() and (qc[-1] == SENTINEL).all() and (qc[:, K // 2:] == SENTINEL).all()
                  and (sc[0] == SENTINEL).all() and (sc[-1] == SENTINEL).all() and (sc[:, K // 32:] == SENTINEL).all())
    return qc[1:N + 1, :K // 2].contiguous(), sc[1:N + 1, :K // 32].contiguous(), intact


def _strided(w, pad=8):
    big = torch.zeros((w.shape[0], w.shape[1] + pad), dtype=w.dtype)
    big[:, :w.shape[1]] = w
    return big[:, :w.shape[1]]


@pytest.mark.parametrize("dtype", W4.DTYPES, ids=GC.DT_NAME.get)
@pytest.mark.parametrize("N,K", [(24, 512), (8, 2560)])
def test_quantizer_matches_the_cpu_rule(dtype, N, K):
    from cogview_amd import ops
    g = torch.Generator().manual_seed(N + K)
    w = (torch.randn((N, K), generator=g) * 0.02).to(dtype)
    w[0] = 0                                                              # an all-zero row
    w[1] = 0
    w[1, K - 3] = -0.37                                                   # a single nonzero
    w[2] = (torch.randn(K, generator=g) * torch.exp2(torch.randint(-14, 10, (K // 32,), generator=g).float()).repeat_interleave(32)).to(dtype)
    w[3, 5], w[3, 6] = -0.0, 0.0
    w = _strided(w)
    assert not w.is_contiguous() and w.stride(0) == K + 8
    q_ref, s_ref = W4.quantize(w)
    q, s, intact = _device_quantize(w)
    assert intact, "the quantizer wrote outside its rows"
    assert torch.equal(s, s_ref), (s != s_ref).nonzero()[:8].tolist()
    assert W4.same_codes(q, q_ref), (W4.unpack(q) != W4.unpack(q_ref)).nonzero()[:8].tolist()
    assert int(s.min()) >= 1 and int(s.max()) <= 254 and bool((s[0] == 127).all())
    assert int((W4.unpack(q)[1] & 7 != 0).sum()) == 1
    # through ops: contiguous outputs, the same bytes, twice
    wd = torch.empty_strided(w.shape, w.stride(), dtype=dtype, device="cuda").copy_(w)
    q2, s2 = ops.quantize_rows_mxfp4(wd)
    assert q2.shape == (N, K // 2) and s2.shape == (N, K // 32) and q2.dtype == s2.dtype == torch.uint8
    assert torch.equal(q2.cpu(), q) and torch.equal(s2.cpu(), s)
    again = ops.quantize_rows_mxfp4(wd)
    assert torch.equal(again[0], q2) and torch.equal(again[1], s2)
    # and the torch dequantizer on the device reads back what the CPU rule holds
    assert torch.equal(ops.dequantize_rows_mxfp4(q2, s2).double().cpu(), W4.dequantize(q_ref, s_ref))


@pytest.mark.parametrize("dtype", W4.DTYPES, ids=GC.DT_NAME.get)
def test_crafted_rows_through_the_device_quantizer(dtype):
    """every tie, both signs, saturation, a zero block, a block at the exponent clamp (tests/w4_cases.py: crafted_rows)"""
    w, codes, scales = W4.crafted_rows(dtype)
    q, s, intact = _device_quantize(_strided(w.repeat(3, 1)))
    assert intact
    for row in range(3):
        assert torch.equal(s[row], scales), s[row].tolist()
        assert W4.same_codes(q[row:row + 1], W4.pack(codes.view(1, -1))), (W4.unpack(q[row:row + 1])[0] != codes).nonzero().flatten().tolist()


def test_bad_arguments_are_refused():
    from cogview_amd import _lib as L
    w = torch.zeros((2, 64), dtype=torch.float16, device="cuda")
    q = torch.zeros((2, 32), dtype=torch.uint8, device="cuda")
    s = torch.zeros((2, 2), dtype=torch.uint8, device="cuda")
    call = L.lib().cogv_quantize_rows_mxfp4
    assert call(L.F16, w.data_ptr(), 64, 2, 64, q.data_ptr(), 32, s.data_ptr(), 2, None) == L.OK
    assert call(L.F16, w.data_ptr(), 64, 2, 48, q.data_ptr(), 32, s.data_ptr(), 2, None) == L.ERR_ARG        # K % 32
    assert call(L.F16, w.data_ptr(), 64, 2, 64, q.data_ptr(), 28, s.data_ptr(), 2, None) == L.ERR_ARG        # ldq < K / 2
    assert call(L.F16, w.data_ptr(), 64, 2, 64, q.data_ptr(), 32, s.data_ptr(), 1, None) == L.ERR_ARG        # lds < K / 32
    assert call(2, w.data_ptr(), 64, 2, 64, q.data_ptr(), 32, s.data_ptr(), 2, None) == L.ERR_UNSUPPORTED    # fp32
    torch.cuda.synchronize()
