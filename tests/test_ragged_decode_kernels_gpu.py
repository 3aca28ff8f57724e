"""GPU: the ragged form of the decode attentions -- cogv_attn_decode_desc.first / cogv_attn_decode_kv8_desc.first (fp16 and bf16).
Row b of one launch attends slots [first[b], pos]: the slots below first[b] are padding and hold NaN here (16-bit cache: NaN
elements; 8-bit cache: NaN scales), so any product that touches them shows in the output."""
import ctypes as C

import pytest
import torch

from oracle import cogview_oracle as O
from tests.test_kernels_gpu import TOL, dev, rel, rnd
from tests.test_kv8_kernels_gpu import cpu_quantize, dequantize, heads_of

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
# own slot only | same split, split 0 fully masked, rows differing in one launch | masked split boundary | last slot of the
# cache | the model's own head count
CASES = [(1, 2, 128, 5, [5]), (3, 3, 300, 140, [0, 5, 130]), (2, 3, 300, 128, [127, 128]), (2, 2, 256, 255, [129, 0]),
         (1, 40, 1152, 1024, [37])]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X; run with -m 'not gpu' elsewhere"
    from cogview_amd import ops as _ops
    return _ops


def _first(first):
    return torch.tensor(first, dtype=torch.int32, device="cuda")


def _reference(qkv, kv, H, pos, first):
    """the oracle's standard_attention per row over slots [first_b, pos] of kv [b, cap, 2 * hp] (the new token's in slot pos)"""
    b, hp = qkv.shape[0], H * 64
    rows = []
    for r in range(b):
        n = pos + 1 - first[r]
        q = qkv[r:r + 1, :, :hp].to(kv.dtype).view(1, 1, H, 64).permute(0, 2, 1, 3)
        k = kv[r:r + 1, first[r]:pos + 1, :hp].reshape(1, n, H, 64).permute(0, 2, 1, 3)
        v = kv[r:r + 1, first[r]:pos + 1, hp:].reshape(1, n, H, 64).permute(0, 2, 1, 3)
        rows.append(O.standard_attention(q, k, v, torch.ones(1, 1, 1, n, dtype=kv.dtype)).permute(0, 2, 1, 3).reshape(1, 1, hp))
    return torch.cat(rows, 0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("b,H,cap,pos,first", CASES)
def test_attention_decode_ragged(ops, dtype, b, H, cap, pos, first):
    g = torch.Generator().manual_seed(cap + pos)
    hp = H * 64
    clean = rnd((b, cap, 2 * hp), dtype, g)
    qkv = rnd((b, 1, 3 * hp), dtype, g)
    cache = clean.clone()
    for r in range(b):
        cache[r, :first[r]] = float("nan")
    cache_d, qkv_d = dev(cache.clone()), dev(qkv)
    pos_d = torch.tensor([pos], dtype=torch.int64, device="cuda")
    out = ops.attention_decode(qkv_d, cache_d, pos_d, H, first=_first(first))
    assert bool(torch.isfinite(out.float()).all()), "a padding slot (NaN) reached the output"
    want = cache.clone()
    want[:, pos, :hp] = qkv[:, 0, hp:2 * hp]
    want[:, pos, hp:] = qkv[:, 0, 2 * hp:]
    got = cache_d.cpu()
    for r in range(b):                                        # only slot pos is written; the NaNs are still there
        assert torch.equal(got[r, first[r]:], want[r, first[r]:])
        assert bool(torch.isnan(got[r, :first[r]]).all())
    e = rel(out, _reference(qkv, want.float(), H, pos, first))
    print(f"[{dtype}] b={b} H={H} cap={cap} pos={pos} first={first}: rel-L2 {e:.2e}")
    assert e < TOL[dtype]
    again = ops.attention_decode(qkv_d, cache_d, pos_d, H, first=_first(first))
    assert torch.equal(out, again)
    # first all zeros: the bits of the call without `first`
    c0, c1 = dev(clean.clone()), dev(clean.clone())
    plain = ops.attention_decode(qkv_d, c0, pos_d, H)
    zeros = ops.attention_decode(qkv_d, c1, pos_d, H, first=_first([0] * b))
    assert torch.equal(plain, zeros) and torch.equal(c0, c1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_first_outside_the_context(ops, dtype):
    """first[b] < 0 counts as 0; first[b] > pos attends the new token's own slot only"""
    b, H, cap, pos = 2, 2, 256, 130
    g = torch.Generator().manual_seed(5)
    hp = H * 64
    cache, qkv = rnd((b, cap, 2 * hp), dtype, g), rnd((b, 1, 3 * hp), dtype, g)
    pos_d = torch.tensor([pos], dtype=torch.int64, device="cuda")
    plain = ops.attention_decode(dev(qkv), dev(cache.clone()), pos_d, H)
    out = ops.attention_decode(dev(qkv), dev(cache.clone()), pos_d, H, first=_first([-3, 200]))
    assert torch.equal(out[0], plain[0])
    assert torch.equal(out[1].cpu(), qkv[1, :, 2 * hp:])      # softmax over one slot: the new value itself


def _cache8(b, H, cap, first, dtype, g):
    """an 8-bit cache of quantized random keys / values whose padding slots [0, first_b) hold NaN scales"""
    q, s = cpu_quantize(heads_of(rnd((b, cap, 2 * H * 64), dtype, g), H))
    q, s = q.contiguous(), s.contiguous()
    for r in range(b):
        s[r, :, :, :first[r]] = float("nan")
    return q, s


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("b,H,cap,pos,first", CASES)
def test_attention_decode_kv8_ragged(ops, dtype, b, H, cap, pos, first):
    g = torch.Generator().manual_seed(cap + pos + 1)
    hp = H * 64
    q0, s0 = _cache8(b, H, cap, first, dtype, g)
    qkv = rnd((b, 1, 3 * hp), dtype, g)
    q_d, s_d, qkv_d = q0.cuda(), s0.cuda(), qkv.cuda()
    pos_d = torch.tensor([pos], dtype=torch.int64, device="cuda")
    out = ops.attention_decode_kv8(qkv_d, (q_d, s_d), pos_d, H, first=_first(first))
    assert bool(torch.isfinite(out.float()).all()), "a padding slot (NaN scale) reached the output"
    q1, s1 = q_d.cpu(), s_d.cpu()
    want_q, want_s = cpu_quantize(heads_of(qkv[:, :, hp:], H))
    assert torch.equal(q1[:, :, :, pos:pos + 1], want_q) and torch.equal(s1[:, :, :, pos:pos + 1], want_s)
    keep = torch.ones(cap, dtype=torch.bool)
    keep[pos] = False
    assert torch.equal(q1[:, :, :, keep], q0[:, :, :, keep])                       # bytes and scales unchanged outside slot pos
    assert torch.equal(s1[:, :, :, keep].view(torch.int32), s0[:, :, :, keep].view(torch.int32))
    # fp64 softmax attention over the dequantized slots [first_b, pos] as the kernel left them (test_attention_decode_kv8_step's bar)
    e = rel(out, _reference(qkv, dequantize(q1, s1).double(), H, pos, first))
    print(f"[{dtype}] b={b} H={H} cap={cap} pos={pos} first={first}: rel-L2 {e:.2e}")
    assert e < TOL[dtype]
    again = ops.attention_decode_kv8(qkv_d, (q_d, s_d), pos_d, H, first=_first(first))
    assert torch.equal(out, again)
    assert torch.equal(q_d.cpu(), q1) and torch.equal(s_d.cpu().view(torch.int32), s1.view(torch.int32))
    # first all zeros: the bits of the call without `first`
    qc, sc = cpu_quantize(heads_of(rnd((b, cap, 2 * hp), dtype, g), H))
    qc, sc = qc.contiguous(), sc.contiguous()
    a, c = (qc.cuda(), sc.cuda()), (qc.cuda(), sc.cuda())
    plain = ops.attention_decode_kv8(qkv_d, a, pos_d, H)
    zeros = ops.attention_decode_kv8(qkv_d, c, pos_d, H, first=_first([0] * b))
    assert torch.equal(plain, zeros) and torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kv8", [False, True])
def test_ragged_partials_feed_the_combine_prologues(ops, dtype, kv8):
    """combine=False with `first` leaves the partials cogv_gemv_attn / cogv_gemv_attn_w8 combine -- splits wholly in the padding
    included: bit-identical to the combine launch followed by the plain product."""
    b, H, cap, pos, N, first = 4, 8, 256, 200, 512, [0, 64, 128, 199]
    g = torch.Generator().manual_seed(78)
    hp = H * 64
    qkv = rnd((b, 1, 3 * hp), dtype, g).cuda()
    w, bias = rnd((N, hp), dtype, g, 0.05).cuda(), rnd((N,), dtype, g).cuda()
    pos_d = torch.tensor([pos], dtype=torch.int64, device="cuda")
    if kv8:
        q0, s0 = _cache8(b, H, cap, first, dtype, g)
        run = lambda **kw: ops.attention_decode_kv8(qkv, (q0.cuda(), s0.cuda()), pos_d, H, first=_first(first), **kw)
    else:
        cache = rnd((b, cap, 2 * hp), dtype, g)
        for r in range(b):
            cache[r, :first[r]] = float("nan")
        run = lambda **kw: ops.attention_decode(qkv, cache.cuda(), pos_d, H, first=_first(first), **kw)
    att = run()
    two = ops.gemm(att.view(b, hp), w, bias=bias)
    two8 = ops.gemm_w8(att.view(b, hp), ops.quantize_rows_e4m3(w), bias=bias)
    parts = run(combine=False)
    one = ops.gemv_attn(parts, b, H, cap, w, bias=bias)
    assert bool(torch.isfinite(one.float()).all()) and torch.equal(one, two)
    one8 = ops.gemv_attn_w8(parts, b, H, cap, ops.quantize_rows_e4m3(w), dtype, bias=bias)
    assert torch.equal(one8, two8)


def test_misaligned_first_is_a_bad_argument(ops):
    """a `first` pointer that is not 4-byte aligned comes back as code 1 (bad argument), never as a launch"""
    from cogview_amd import _lib
    b, H, cap, hp = 2, 2, 128, 128
    lib = _lib.lib()
    qkv = torch.zeros((b, 1, 3 * hp), dtype=torch.float16, device="cuda")
    pos = torch.zeros(1, dtype=torch.int64, device="cuda")
    ws = torch.zeros(lib.cogv_attention_decode_workspace_bytes(b, H, cap), dtype=torch.uint8, device="cuda")
    out = torch.zeros((b, 1, hp), dtype=torch.float16, device="cuda")
    first = torch.zeros(b + 1, dtype=torch.int32, device="cuda")
    cache = torch.zeros((b, cap, 2 * hp), dtype=torch.float16, device="cuda")
    d = _lib.AttnDecodeDesc()
    d.dtype, d.B, d.H, d.capacity, d.head_dim, d.scale = 0, b, H, cap, 64, 0.125
    d.qkv, d.qkv_bs, d.cache, d.cache_bs, d.cache_rs = qkv.data_ptr(), 3 * hp, cache.data_ptr(), cap * 2 * hp, 2 * hp
    d.out, d.out_bs, d.pos, d.workspace, d.workspace_bytes = out.data_ptr(), hp, pos.data_ptr(), ws.data_ptr(), ws.numel()
    q = torch.zeros((b, 2, H, cap, 64), dtype=torch.uint8, device="cuda")
    s = torch.ones((b, 2, H, cap), dtype=torch.float32, device="cuda")
    d8 = _lib.AttnDecodeKv8Desc()
    d8.dtype, d8.B, d8.H, d8.capacity, d8.head_dim, d8.scale = 0, b, H, cap, 64, 0.125
    d8.qkv, d8.qkv_bs, d8.kv_q, d8.kv_q_bs, d8.kv_scale, d8.kv_scale_bs = qkv.data_ptr(), 3 * hp, q.data_ptr(), q.stride(0), s.data_ptr(), s.stride(0)
    d8.out, d8.out_bs, d8.pos, d8.workspace, d8.workspace_bytes = out.data_ptr(), hp, pos.data_ptr(), ws.data_ptr(), ws.numel()
    for off, code in ((2, 1), (1, 1), (4, 0)):
        d.first = d8.first = first.data_ptr() + off
        assert lib.cogv_attention_decode(C.byref(d), None) == code
        assert lib.cogv_attention_decode_kv8(C.byref(d8), None) == code
    torch.cuda.synchronize()
