"""GPU: cogv_attention_decode_chunk (ops.attention_decode_chunk), fp16 and bf16 -- the decode attention of m tokens per cache
row.  Its contract is bit identity with m successive ops.attention_decode calls at pos, pos + 1, ...: outputs, split partials
and the cache afterwards.  Every slot from pos on (and every padding slot below `first`) holds NaN before the call, and the
cache is a view inside a buffer of sentinels, so a product with a slot that is not attended, or a store outside [pos, pos + m)
or past the capacity, shows."""
import ctypes as C

import pytest
import torch

from oracle import cogview_oracle as O
from tests.test_kernels_gpu import TOL, dev, rel, rnd

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
MS = [1, 2, 3, 5, 8]
# one split, from an empty cache | the chunk straddles a split boundary | ends in the last slot | 32 splits, most past the chunk
CASES = [(1, 2, 128, 0), (2, 3, 300, 125), (1, 8, 384, 376), (1, 2, 4096, 2000)]
SENTINEL, TAIL = 77.0, 8


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X; run with -m 'not gpu' elsewhere"
    from cogview_amd import ops as _ops
    return _ops


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


class Case:
    """Inputs of one comparison: a buffer [B, cap + TAIL, 2 hp] of sentinels whose leading cap slots are the cache -- random in
    [first_b, pos), NaN elsewhere -- and qkv [B, m, 3 hp]."""

    def __init__(self, dtype, B, H, cap, pos, m, first=None, seed=0):
        g = torch.Generator().manual_seed(1000 * seed + cap + pos + m)
        self.dtype, self.B, self.H, self.cap, self.pos, self.m, self.first = dtype, B, H, cap, pos, m, first
        self.hp = hp = H * 64
        buf = torch.full((B, cap + TAIL, 2 * hp), SENTINEL, dtype=dtype)
        buf[:, :cap] = rnd((B, cap, 2 * hp), dtype, g)
        buf[:, min(pos, cap):cap] = float("nan")
        for b in range(B):
            buf[b, :self.lo(b, 0)] = float("nan")
        self.buf, self.qkv = buf, rnd((B, m, 3 * hp), dtype, g)
        self.first_d = None if first is None else torch.tensor(first, dtype=torch.int32, device="cuda")
        self.nsplit = (cap + 127) // 128

    def lo(self, b, j):
        """first attended slot of row (b, j): first_b clamped to [0, pos + j]"""
        return 0 if self.first is None else min(max(self.first[b], 0), self.pos + j)

    def _pos(self, j=0):
        return torch.tensor([self.pos + j], dtype=torch.int64, device="cuda")

    def sequential(self, ops, combine=True):
        """m one-token calls -> (out [B, m, hp] or partials [B * m, H, nsplit, 66], buffer afterwards)"""
        buf, qkv = dev(self.buf.clone()), dev(self.qkv)
        res = []
        for j in range(self.m):
            r = ops.attention_decode(qkv[:, j:j + 1].contiguous(), buf[:, :self.cap], self._pos(j), self.H, combine=combine, first=self.first_d)
            res.append(r.clone() if combine else r.view(torch.float32)[:self.B * self.H * self.nsplit * 66].view(self.B, 1, self.H, self.nsplit, 66).clone())
        res = torch.cat(res, 1)
        return (res if combine else res.view(self.B * self.m, self.H, self.nsplit, 66)), buf

    def chunk(self, ops, combine=True):
        buf = dev(self.buf.clone())
        r = ops.attention_decode_chunk(dev(self.qkv), buf[:, :self.cap], self._pos(), self.H, combine=combine, first=self.first_d)
        if not combine:
            r = r.view(torch.float32)[:self.B * self.m * self.H * self.nsplit * 66].view(self.B * self.m, self.H, self.nsplit, 66).clone()
        return r, buf

    def want_buffer(self):
        want = self.buf.clone()
        n = max(0, min(self.m, self.cap - self.pos))
        want[:, self.pos:self.pos + n] = self.qkv[:, :n, self.hp:]
        return want

    def reference(self):
        """the oracle's standard_attention of row (b, j) over slots [lo, pos + j], the chunk's own rows in slots pos ..."""
        kv = self.want_buffer()[:, :self.cap].float()
        H, hp, rows = self.H, self.hp, []
        for b in range(self.B):
            for j in range(self.m):
                lo, hi = self.lo(b, j), min(self.pos + j, self.cap - 1) + 1
                n = hi - lo
                q = self.qkv[b:b + 1, j:j + 1, :hp].float().view(1, 1, H, 64).permute(0, 2, 1, 3)
                k = kv[b:b + 1, lo:hi, :hp].reshape(1, n, H, 64).permute(0, 2, 1, 3)
                v = kv[b:b + 1, lo:hi, hp:].reshape(1, n, H, 64).permute(0, 2, 1, 3)
                rows.append(O.standard_attention(q, k, v, torch.ones(1, 1, 1, n)).permute(0, 2, 1, 3).reshape(1, hp))
        return torch.cat(rows, 0).view(self.B, self.m, hp)


def _check_against_sequential(ops, case):
    out, buf = case.chunk(ops)
    seq, seq_buf = case.sequential(ops)
    assert tuple(out.shape) == (case.B, case.m, case.hp)
    assert bool(torch.isfinite(out.float()).all()), "a slot that is not attended (NaN) reached the output"
    assert _same(out, seq), "outputs differ from m one-token calls"
    assert _same(buf, seq_buf), "the cache differs from the one m one-token calls leave"
    # only slots [pos, pos + m) below the capacity change; the sentinels behind the view stay
    assert _same(buf.cpu(), case.want_buffer())
    parts, buf2 = case.chunk(ops, combine=False)
    seq_parts, _ = case.sequential(ops, combine=False)
    assert _same(parts, seq_parts), "partials differ from m one-token calls"
    assert _same(buf2, seq_buf)
    return out


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("B,H,cap,pos", CASES)
def test_chunk_is_m_one_token_calls_to_the_bit(ops, dtype, B, H, cap, pos, m):
    _check_against_sequential(ops, Case(dtype, B, H, cap, pos, m))


@pytest.mark.parametrize("dtype", DTYPES)
def test_m1_is_the_one_token_call(ops, dtype):
    case = Case(dtype, 2, 3, 300, 127, 1)
    out, buf = case.chunk(ops)
    one_buf = dev(case.buf.clone())
    one = ops.attention_decode(dev(case.qkv), one_buf[:, :case.cap], case._pos(), case.H)
    assert _same(out, one) and _same(buf, one_buf)


@pytest.mark.parametrize("dtype", DTYPES)
def test_nothing_written_or_attended_at_or_past_the_capacity(ops, dtype):
    """pos = cap - 2, m = 4: rows 2 and 3 have no slot; they attend [0, cap) and write nothing"""
    case = Case(dtype, 2, 2, 256, 254, 4)
    _check_against_sequential(ops, case)
    _, buf = case.chunk(ops)
    assert bool((buf[:, case.cap:].float() == SENTINEL).all())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,H,cap,pos,m,first", [(2, 3, 300, 125, 5, [100, 0]),       # below pos
                                                 (2, 3, 300, 125, 5, [127, 126]),     # inside the chunk: rows before it keep their own slot
                                                 (2, 2, 256, 130, 3, [-3, 500]),      # negative: 0; beyond every slot: own slot only
                                                 (1, 2, 384, 200, 8, [129])])         # split 0 wholly in the padding
def test_first(ops, dtype, B, H, cap, pos, m, first):
    case = Case(dtype, B, H, cap, pos, m, first=first, seed=1)
    out = _check_against_sequential(ops, case)
    e = rel(out, case.reference())
    print(f"[{dtype}] first={first}: rel-L2 {e:.2e}")
    assert e < TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,H,cap,pos,m", [(1, 2, 128, 0, 3), (2, 3, 300, 125, 8), (1, 8, 384, 376, 8), (2, 2, 256, 254, 4)])
def test_against_standard_attention_under_the_causal_mask(ops, dtype, B, H, cap, pos, m):
    case = Case(dtype, B, H, cap, pos, m, seed=2)
    out, _ = case.chunk(ops)
    e = rel(out, case.reference())
    print(f"[{dtype}] B={B} H={H} cap={cap} pos={pos} m={m}: rel-L2 {e:.2e}")
    assert e < TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,m", [(1, 8), (2, 4)])
def test_chunk_partials_feed_the_combine_prologue(ops, dtype, B, m):
    """ops.gemv_attn with B * m = 8 rows on the chunk's partials == on the partials of the m one-token calls"""
    H, cap, pos, N = 8, 384, 250, 512
    case = Case(dtype, B, H, cap, pos, m, seed=3)
    g = torch.Generator().manual_seed(9)
    w, bias = dev(rnd((N, H * 64), dtype, g, 0.05)), dev(rnd((N,), dtype, g))
    parts, _ = case.chunk(ops, combine=False)
    seq_parts, _ = case.sequential(ops, combine=False)
    one = ops.gemv_attn(parts, B * m, H, cap, w, bias=bias)
    two = ops.gemv_attn(seq_parts, B * m, H, cap, w, bias=bias)
    assert bool(torch.isfinite(one.float()).all()) and _same(one, two)
    out, _ = case.chunk(ops)
    assert _same(one, ops.gemm(out.view(B * m, H * 64), w, bias=bias))


def test_error_codes(ops):
    from cogview_amd import _lib
    B, H, cap, m, hp = 2, 2, 128, 4, 128
    lib = _lib.lib()
    qkv = torch.zeros((B * m + 1, 3 * hp), dtype=torch.float16, device="cuda")
    pos = torch.zeros(1, dtype=torch.int64, device="cuda")
    need = lib.cogv_attention_decode_workspace_bytes(B * m, H, cap)
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    out = torch.zeros((B * m, hp), dtype=torch.float16, device="cuda")
    first = torch.zeros(B + 1, dtype=torch.int32, device="cuda")
    cache = torch.zeros((B, cap, 2 * hp), dtype=torch.float16, device="cuda")

    def desc(**kw):
        d = _lib.AttnDecodeChunkDesc()
        d.dtype, d.B, d.H, d.capacity, d.head_dim, d.m, d.scale = _lib.F16, B, H, cap, 64, m, 0.125
        d.qkv, d.qkv_rs, d.cache, d.cache_bs, d.cache_rs = qkv.data_ptr(), 3 * hp, cache.data_ptr(), cap * 2 * hp, 2 * hp
        d.out, d.out_rs, d.pos, d.workspace, d.workspace_bytes = out.data_ptr(), hp, pos.data_ptr(), ws.data_ptr(), ws.numel()
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    call = lambda **kw: lib.cogv_attention_decode_chunk(C.byref(desc(**kw)), None)
    assert call() == 0
    assert call(m=0) == 1 and call(m=9) == 1 and call(m=-1) == 1
    assert call(qkv=qkv.data_ptr() + 2) == 1 and call(cache=cache.data_ptr() + 8) == 1 and call(qkv_rs=3 * hp + 4) == 1
    assert call(first=first.data_ptr() + 2) == 1 and call(first=first.data_ptr() + 4) == 0
    assert call(workspace_bytes=need - 1) == 1
    assert call(workspace_bytes=lib.cogv_attention_decode_workspace_bytes(B, H, cap)) == 1          # sized for B rows, not B * m
    assert call(out=None) == 1 and call(out=None, skip_combine=1) == 0
    assert call(dtype=_lib.F32) == 3 and call(head_dim=128) == 3
    torch.cuda.synchronize()
