"""GPU: the kernels of the 8-bit key/value cache -- cogv_kv_quantize_e4m3 and cogv_attention_decode_kv8 (fp16 and bf16).
Cache layout: q [b, 2, H, capacity, 64] uint8 (OCP E4M3 bytes; plane 0 keys, plane 1 values), scale [b, 2, H, capacity] fp32."""
import pytest
import torch

from oracle import cogview_oracle as O
from tests.test_kernels_gpu import TOL, rel

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
E4M3 = torch.float8_e4m3fn


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X; run with -m 'not gpu' elsewhere"
    from cogview_amd import ops as _ops
    return _ops


def rnd(shape, dtype, gen, scale=1.0):
    return (torch.randn(shape, generator=gen) * scale).to(dtype)


def cpu_quantize(x):
    """x [..., 64] (16-bit, CPU) -> (bytes uint8 [..., 64], scale fp32 [...]): fp32 absmax / 448, fp32 division, RNE to E4M3"""
    f = x.float()
    amax = f.abs().amax(dim=-1)
    scale = torch.where(amax == 0, torch.ones_like(amax), amax / 448.0)
    return (f / scale.unsqueeze(-1)).to(E4M3).view(torch.uint8), scale


def heads_of(rows, H):
    """[b, n, 2 * H * 64] keys | values -> [b, 2, H, n, 64]: the cache's order"""
    b, n, _ = rows.shape
    return rows.view(b, n, 2, H, 64).permute(0, 2, 3, 1, 4)


def dequantize(q, scale):
    """-> [b, capacity, 2 * H * 64] fp32, keys | values"""
    b, _, H, cap, _ = q.shape
    x = q.view(E4M3).float() * scale.unsqueeze(-1)
    return x.permute(0, 3, 1, 2, 4).reshape(b, cap, 2 * H * 64)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("slot0", [0, 5])
def test_kv_quantizer_bits(ops, dtype, slot0):
    B, n, H, cap = 2, 37, 3, 192
    g = torch.Generator().manual_seed(11 + slot0)
    wide = rnd((B, n + 3, 2 * H * 64 + 64), dtype, g)
    wide[1, 4, 8 + 64:8 + 128] = 0                                # one all-zero head: row 3 of the slice, keys of head 1
    kv = wide[:, 1:1 + n, 8:8 + 2 * H * 64]                       # strided in batch and row, 16-byte aligned
    assert not kv.is_contiguous()
    kv_d = wide.cuda()[:, 1:1 + n, 8:8 + 2 * H * 64]
    q0 = torch.randint(0, 256, (B, 2, H, cap, 64), dtype=torch.uint8, generator=g)
    s0 = torch.randn((B, 2, H, cap), generator=g)
    q_d, s_d = q0.cuda(), s0.cuda()
    ops.kv_quantize_e4m3(kv_d, q_d, s_d, slot0)
    q, s = q_d.cpu(), s_d.cpu()
    want_q, want_s = cpu_quantize(heads_of(kv.contiguous(), H))
    sl = slice(slot0, slot0 + n)
    assert torch.equal(s[:, :, :, sl], want_s), "scales: fp32 absmax / 448 (1.0 for a zero head)"
    assert torch.equal(q[:, :, :, sl], want_q), "bytes: rne_e4m3(x / scale)"
    assert s[1, 0, 1, slot0 + 3] == 1.0 and not q[1, 0, 1, slot0 + 3].any()
    # the weight quantizer on the [rows, 64] view gives the same bits
    rows = heads_of(kv_d, H).reshape(-1, 64).contiguous()
    rq, rs = ops.quantize_rows_e4m3(rows)
    assert torch.equal(rq.cpu().view(B, 2, H, n, 64), q[:, :, :, sl]) and torch.equal(rs.cpu().view(B, 2, H, n), s[:, :, :, sl])
    # slots outside [slot0, slot0 + n) are untouched
    keep = torch.ones(cap, dtype=torch.bool)
    keep[sl] = False
    assert torch.equal(q[:, :, :, keep], q0[:, :, :, keep]) and torch.equal(s[:, :, :, keep], s0[:, :, :, keep])


def _cache(b, H, cap, pos, dtype, g):
    """an 8-bit cache whose slots < pos hold quantized random keys / values and whose slots >= pos hold NaN bytes and NaN scales"""
    q, s = cpu_quantize(heads_of(rnd((b, cap, 2 * H * 64), dtype, g), H))
    q, s = q.contiguous(), s.contiguous()
    q[:, :, :, pos:] = 0x7F
    s[:, :, :, pos:] = float("nan")
    return q, s


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("b,H,cap,pos", [(1, 2, 128, 0), (2, 3, 300, 127), (2, 3, 300, 128), (3, 2, 256, 255), (2, 3, 192, 150)])
def test_attention_decode_kv8_step(ops, dtype, b, H, cap, pos):
    """own slot only | last slot of a split | first slot of the next | last slot of the cache | a capacity that ends inside a split"""
    g = torch.Generator().manual_seed(cap + pos)
    hp = H * 64
    q0, s0 = _cache(b, H, cap, pos, dtype, g)
    qkv = rnd((b, 1, 3 * hp), dtype, g)
    q_d, s_d, qkv_d = q0.cuda(), s0.cuda(), qkv.cuda()
    pos_d = torch.tensor([pos], dtype=torch.int64, device="cuda")
    out = ops.attention_decode_kv8(qkv_d, (q_d, s_d), pos_d, H)
    q1, s1 = q_d.cpu(), s_d.cpu()
    # slot pos: the CPU quantization of the k | v in qkv; slots < pos unchanged; slots > pos untouched
    want_q, want_s = cpu_quantize(heads_of(qkv[:, :, hp:], H))
    assert torch.equal(q1[:, :, :, pos:pos + 1], want_q) and torch.equal(s1[:, :, :, pos:pos + 1], want_s)
    assert torch.equal(q1[:, :, :, :pos], q0[:, :, :, :pos]) and torch.equal(s1[:, :, :, :pos], s0[:, :, :, :pos])
    assert torch.equal(q1[:, :, :, pos + 1:], q0[:, :, :, pos + 1:]) and bool(torch.isnan(s1[:, :, :, pos + 1:]).all())
    # fp64 softmax attention over the dequantized slots [0, pos] as the kernel left them
    kv = dequantize(q1, s1)[:, :pos + 1].double()
    assert bool(torch.isfinite(kv).all())
    qq = qkv[:, :, :hp].double().view(b, 1, H, 64).permute(0, 2, 1, 3)
    k = kv[:, :, :hp].reshape(b, pos + 1, H, 64).permute(0, 2, 1, 3)
    v = kv[:, :, hp:].reshape(b, pos + 1, H, 64).permute(0, 2, 1, 3)
    ref = O.standard_attention(qq, k, v, torch.ones(1, 1, 1, pos + 1, dtype=torch.float64)).permute(0, 2, 1, 3).reshape(b, 1, hp)
    assert bool(torch.isfinite(out.float()).all()), "slots past pos (NaN bytes, NaN scales) reached the output"
    e = rel(out, ref)
    print(f"[{dtype}] b={b} H={H} cap={cap} pos={pos}: rel-L2 {e:.2e}")
    assert e < TOL[dtype]
    again = ops.attention_decode_kv8(qkv_d, (q_d, s_d), pos_d, H)
    assert torch.equal(out, again)
    assert torch.equal(q_d.cpu(), q1) and torch.equal(s_d.cpu()[:, :, :, :pos + 1], s1[:, :, :, :pos + 1])


@pytest.mark.parametrize("dtype", DTYPES)
def test_kv8_partials_feed_the_combine_prologues(ops, dtype):
    """combine=False leaves the partials cogv_gemv_attn / cogv_gemv_attn_w8 combine: bit-identical to the combine launch followed
    by the plain product."""
    b, H, cap, pos, N = 2, 8, 256, 130, 512
    g = torch.Generator().manual_seed(77)
    hp = H * 64
    q0, s0 = _cache(b, H, cap, pos, dtype, g)
    qkv = rnd((b, 1, 3 * hp), dtype, g).cuda()
    w, bias = rnd((N, hp), dtype, g, 0.05).cuda(), rnd((N,), dtype, g).cuda()
    pos_d = torch.tensor([pos], dtype=torch.int64, device="cuda")
    att = ops.attention_decode_kv8(qkv, (q0.cuda(), s0.cuda()), pos_d, H)
    two = ops.gemm(att.view(b, hp), w, bias=bias)
    two8 = ops.gemm_w8(att.view(b, hp), ops.quantize_rows_e4m3(w), bias=bias)
    parts = ops.attention_decode_kv8(qkv, (q0.cuda(), s0.cuda()), pos_d, H, combine=False)
    one = ops.gemv_attn(parts, b, H, cap, w, bias=bias)
    assert bool(torch.isfinite(one.float()).all()) and torch.equal(one, two)
    one8 = ops.gemv_attn_w8(parts, b, H, cap, ops.quantize_rows_e4m3(w), dtype, bias=bias)
    assert torch.equal(one8, two8)


def test_kv8_argument_checks(ops):
    """bad arguments come back as errors, never as launches: misaligned bytes, a short cache, fp32 input"""
    from cogview_amd._lib import CogviewHipError
    b, H, cap = 1, 2, 128
    q = torch.zeros((b, 2, H, cap, 64), dtype=torch.uint8, device="cuda")
    s = torch.ones((b, 2, H, cap), dtype=torch.float32, device="cuda")
    pos = torch.zeros(1, dtype=torch.int64, device="cuda")
    with pytest.raises((CogviewHipError, AssertionError)):
        ops.attention_decode_kv8(torch.zeros((b, 1, 3 * H * 64), dtype=torch.float32, device="cuda"), (q, s), pos, H)
    big = torch.zeros(q.numel() + 16, dtype=torch.uint8, device="cuda")
    with pytest.raises(CogviewHipError, match="argument"):
        ops.attention_decode_kv8(torch.zeros((b, 1, 3 * H * 64), dtype=torch.float16, device="cuda"), (big[8:8 + q.numel()].view(q.shape), s), pos, H)
    with pytest.raises((CogviewHipError, AssertionError)):
        ops.kv_quantize_e4m3(torch.zeros((b, 4, 2 * H * 64), dtype=torch.float16, device="cuda"), q, s, cap - 3)
