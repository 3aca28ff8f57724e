"""GPU: cogv_attention_decode_chunk_kv8 (ops.attention_decode_chunk_kv8), fp16 and bf16 -- the decode attention of m tokens per
cache row on the 8-bit key/value cache.  Its contract is bit identity with m successive ops.attention_decode_kv8 calls at pos,
pos + 1, ...: outputs, split partials, and the cache's bytes and scales afterwards.  Every slot outside [first_b, pos) holds NaN
bytes (0x7F) and NaN scales before the call, and the byte and scale planes are views inside buffers of sentinels, so a product
with a slot that is not attended, or a store outside [pos, pos + m) or past the capacity, shows."""
import ctypes as C

import pytest
import torch

from oracle import cogview_oracle as O
from tests.test_kernels_gpu import TOL, dev, rel, rnd
from tests.test_kv8_kernels_gpu import cpu_quantize, dequantize, heads_of

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
MS = [1, 2, 3, 5, 8]
# one split, from an empty cache | the chunk straddles a split boundary and the capacity ends inside a split | straddles the
# 64-key pass boundary inside a split | ends in the last slot | 32 splits, most past the chunk
CASES = [(1, 2, 128, 0), (2, 3, 300, 125), (1, 2, 256, 60), (1, 8, 384, 376), (1, 2, 4096, 2000)]
Q_SENTINEL, S_SENTINEL, Q_TAIL, S_TAIL = 0x55, 77.0, 64, 8


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X; run with -m 'not gpu' elsewhere"
    from cogview_amd import ops as _ops
    return _ops


def _bits(t):
    t = t.contiguous()
    return t if t.dtype == torch.uint8 else t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


class Case:
    """Inputs of one comparison: byte buffer [B, 2 * H * cap * 64 + Q_TAIL] and scale buffer [B, 2 * H * cap + S_TAIL] of
    sentinels whose leading parts are the cache planes -- quantized random data in slots [first_b, pos), 0x7F bytes and NaN scales
    elsewhere -- and qkv [B, m, 3 hp]."""

    def __init__(self, dtype, B, H, cap, pos, m, first=None, seed=0, qkv=None):
        g = torch.Generator().manual_seed(1000 * seed + cap + pos + m)
        self.dtype, self.B, self.H, self.cap, self.pos, self.m, self.first = dtype, B, H, cap, pos, m, first
        self.hp = hp = H * 64
        self.nq, self.nsc = 2 * H * cap * 64, 2 * H * cap
        q, s = cpu_quantize(heads_of(rnd((B, cap, 2 * hp), dtype, g), H))
        q, s = q.contiguous(), s.contiguous()
        q[:, :, :, min(pos, cap):] = 0x7F
        s[:, :, :, min(pos, cap):] = float("nan")
        for b in range(B):
            q[b, :, :, :self.lo(b, 0)] = 0x7F
            s[b, :, :, :self.lo(b, 0)] = float("nan")
        self.qbuf = torch.full((B, self.nq + Q_TAIL), Q_SENTINEL, dtype=torch.uint8)
        self.sbuf = torch.full((B, self.nsc + S_TAIL), S_SENTINEL, dtype=torch.float32)
        self.qbuf[:, :self.nq] = q.view(B, -1)
        self.sbuf[:, :self.nsc] = s.view(B, -1)
        self.qkv = rnd((B, m, 3 * hp), dtype, g) if qkv is None else qkv
        self.first_d = None if first is None else torch.tensor(first, dtype=torch.int32, device="cuda")
        self.nsplit = (cap + 127) // 128

    def lo(self, b, j):
        """first attended slot of row (b, j): first_b clamped to [0, pos + j]"""
        return 0 if self.first is None else min(max(self.first[b], 0), self.pos + j)

    def _pos(self, j=0):
        return torch.tensor([self.pos + j], dtype=torch.int64, device="cuda")

    def planes(self, qbuf, sbuf):
        """the cache views (q [B, 2, H, cap, 64], scale [B, 2, H, cap]) inside the buffers"""
        return qbuf[:, :self.nq].view(self.B, 2, self.H, self.cap, 64), sbuf[:, :self.nsc].view(self.B, 2, self.H, self.cap)

    def _parts(self, ws, rows):
        return ws.view(torch.float32)[:rows * self.H * self.nsplit * 66].clone()

    def sequential(self, ops, combine=True):
        """m one-token calls -> (out [B, m, hp] or partials [B * m, H, nsplit, 66], byte buffer, scale buffer afterwards)"""
        qbuf, sbuf, qkv = dev(self.qbuf.clone()), dev(self.sbuf.clone()), dev(self.qkv)
        res = []
        for j in range(self.m):
            r = ops.attention_decode_kv8(qkv[:, j:j + 1].contiguous(), self.planes(qbuf, sbuf), self._pos(j), self.H, combine=combine, first=self.first_d)
            res.append(r.clone() if combine else self._parts(r, self.B).view(self.B, 1, self.H, self.nsplit, 66))
        res = torch.cat(res, 1)
        return (res if combine else res.view(self.B * self.m, self.H, self.nsplit, 66)), qbuf, sbuf

    def chunk(self, ops, combine=True):
        qbuf, sbuf = dev(self.qbuf.clone()), dev(self.sbuf.clone())
        r = ops.attention_decode_chunk_kv8(dev(self.qkv), self.planes(qbuf, sbuf), self._pos(), self.H, combine=combine, first=self.first_d)
        if not combine:
            r = self._parts(r, self.B * self.m).view(self.B * self.m, self.H, self.nsplit, 66)
        return r, qbuf, sbuf

    def written(self):
        """slots the step writes: [pos, pos + m) below the capacity"""
        return slice(min(self.pos, self.cap), min(self.pos + self.m, self.cap))

    def want_buffers(self):
        """the buffers after the step: the chunk's k | v by cpu_quantize in the written slots, everything else as it was"""
        qbuf, sbuf = self.qbuf.clone(), self.sbuf.clone()
        q, s = self.planes(qbuf, sbuf)
        w = self.written()
        n = w.stop - w.start
        if n:
            wq, wsc = cpu_quantize(heads_of(self.qkv[:, :n, self.hp:].contiguous(), self.H))
            q[:, :, :, w], s[:, :, :, w] = wq, wsc
        return qbuf, sbuf

    def reference(self, qbuf, sbuf):
        """the oracle's standard_attention in fp64 of row (b, j) over the dequantized slots [lo, pos + j] of the cache as the
        kernel left it (qbuf, sbuf: CPU)"""
        q8, s8 = self.planes(qbuf, sbuf)
        H, hp, rows = self.H, self.hp, []
        for b in range(self.B):
            for j in range(self.m):
                lo, hi = self.lo(b, j), min(self.pos + j, self.cap - 1) + 1
                n = hi - lo
                kv = dequantize(q8[b:b + 1, :, :, lo:hi], s8[b:b + 1, :, :, lo:hi]).double()
                assert bool(torch.isfinite(kv).all())
                q = self.qkv[b:b + 1, j:j + 1, :hp].double().view(1, 1, H, 64).permute(0, 2, 1, 3)
                k = kv[:, :, :hp].reshape(1, n, H, 64).permute(0, 2, 1, 3)
                v = kv[:, :, hp:].reshape(1, n, H, 64).permute(0, 2, 1, 3)
                rows.append(O.standard_attention(q, k, v, torch.ones(1, 1, 1, n, dtype=torch.float64)).permute(0, 2, 1, 3).reshape(1, hp))
        return torch.cat(rows, 0).view(self.B, self.m, hp)


def _check_against_sequential(ops, case):
    out, qbuf, sbuf = case.chunk(ops)
    seq, seq_q, seq_s = case.sequential(ops)
    assert tuple(out.shape) == (case.B, case.m, case.hp)
    assert bool(torch.isfinite(out.float()).all()), "a slot that is not attended (NaN bytes, NaN scale) reached the output"
    assert _same(out, seq), "outputs differ from m one-token calls"
    assert _same(qbuf, seq_q), "the cache's bytes differ from those m one-token calls leave"
    hi = min(case.pos + case.m, case.cap)
    assert _same(case.planes(qbuf, sbuf)[1][:, :, :, :hi], case.planes(seq_q, seq_s)[1][:, :, :, :hi]), "scales of slots [0, pos + m)"
    assert _same(sbuf, seq_s), "the scale buffer differs from the one m one-token calls leave"
    # the written slots hold cpu_quantize of the chunk's k | v; every other slot and the sentinels behind the views stay
    want_q, want_s = case.want_buffers()
    assert _same(qbuf.cpu(), want_q), "bytes: only slots [pos, pos + m) below the capacity change, to rne_e4m3(x / scale)"
    assert _same(sbuf.cpu(), want_s), "scales: only slots [pos, pos + m) below the capacity change, to fp32 absmax / 448"
    parts, qbuf2, sbuf2 = case.chunk(ops, combine=False)
    seq_parts, _, _ = case.sequential(ops, combine=False)
    assert _same(parts, seq_parts), "partials differ from m one-token calls"
    assert _same(qbuf2, seq_q) and _same(sbuf2, seq_s)
    return out, qbuf.cpu(), sbuf.cpu()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("B,H,cap,pos", CASES)
def test_chunk_is_m_one_token_calls_to_the_bit(ops, dtype, B, H, cap, pos, m):
    _check_against_sequential(ops, Case(dtype, B, H, cap, pos, m))


@pytest.mark.parametrize("dtype", DTYPES)
def test_m1_is_the_one_token_call(ops, dtype):
    case = Case(dtype, 2, 3, 300, 127, 1)
    out, qbuf, sbuf = case.chunk(ops)
    one_q, one_s = dev(case.qbuf.clone()), dev(case.sbuf.clone())
    one = ops.attention_decode_kv8(dev(case.qkv), case.planes(one_q, one_s), case._pos(), case.H)
    assert _same(out, one) and _same(qbuf, one_q) and _same(sbuf, one_s)


@pytest.mark.parametrize("dtype", DTYPES)
def test_nothing_written_or_attended_at_or_past_the_capacity(ops, dtype):
    """pos = cap - 2, m = 4: rows 2 and 3 have no slot; they attend [0, cap) and write nothing"""
    case = Case(dtype, 2, 2, 256, 254, 4)
    out, qbuf, sbuf = _check_against_sequential(ops, case)
    assert bool((qbuf[:, case.nq:] == Q_SENTINEL).all()) and bool((sbuf[:, case.nsc:] == S_SENTINEL).all())
    e = rel(out, case.reference(qbuf, sbuf))
    print(f"[{dtype}] rows without a slot: rel-L2 {e:.2e}")
    assert e < TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,H,cap,pos,m,first", [(2, 3, 300, 125, 5, [100, 0]),       # below pos
                                                 (2, 3, 300, 125, 5, [127, 126]),     # inside the chunk: rows before it keep their own slot
                                                 (2, 2, 256, 130, 3, [-3, 500]),      # negative: 0; beyond every slot: own slot only
                                                 (1, 2, 384, 200, 8, [129])])         # split 0 wholly in the padding
def test_first(ops, dtype, B, H, cap, pos, m, first):
    case = Case(dtype, B, H, cap, pos, m, first=first, seed=1)
    out, qbuf, sbuf = _check_against_sequential(ops, case)
    e = rel(out, case.reference(qbuf, sbuf))
    print(f"[{dtype}] first={first}: rel-L2 {e:.2e}")
    assert e < TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
def test_an_all_zero_key_head_takes_scale_one_and_zero_bytes(ops, dtype):
    B, H, cap, pos, m = 1, 2, 256, 60, 5
    case = Case(dtype, B, H, cap, pos, m, seed=4)
    case.qkv[0, 2, case.hp + 64:case.hp + 128] = 0               # row 2, keys of head 1
    _, qbuf, sbuf = _check_against_sequential(ops, case)
    q, s = case.planes(qbuf, sbuf)
    assert s[0, 0, 1, pos + 2] == 1.0 and not q[0, 0, 1, pos + 2].any()
    assert s[0, 1, 1, pos + 2] != 1.0 and q[0, 1, 1, pos + 2].any()          # its value head is an ordinary one


@pytest.mark.parametrize("dtype", DTYPES)
def test_rows_of_different_magnitudes_take_separate_scales(ops, dtype):
    B, H, cap, pos, m = 1, 2, 256, 126, 4
    case = Case(dtype, B, H, cap, pos, m, seed=5)
    case.qkv[0, 1, case.hp:] *= 1e-3
    case.qkv[0, 2, case.hp:] *= 1e2
    out, qbuf, sbuf = _check_against_sequential(ops, case)
    _, s = case.planes(qbuf, sbuf)
    small, large = s[0, :, :, pos + 1], s[0, :, :, pos + 2]
    want = cpu_quantize(heads_of(case.qkv[:, 1:3, case.hp:].contiguous(), H))[1]
    assert torch.equal(small, want[0, :, :, 0]) and torch.equal(large, want[0, :, :, 1])
    assert bool((large > 1e4 * small).all())
    e = rel(out, case.reference(qbuf, sbuf))
    print(f"[{dtype}] magnitudes 1e-3 | 1e2: rel-L2 {e:.2e}")
    assert e < TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,H,cap,pos,m", [(1, 2, 128, 0, 3), (2, 3, 300, 125, 8), (1, 2, 256, 60, 8), (1, 8, 384, 376, 8), (2, 2, 256, 254, 4)])
def test_against_standard_attention_under_the_causal_rule(ops, dtype, B, H, cap, pos, m):
    case = Case(dtype, B, H, cap, pos, m, seed=2)
    out, qbuf, sbuf = case.chunk(ops)
    e = rel(out, case.reference(qbuf.cpu(), sbuf.cpu()))
    print(f"[{dtype}] B={B} H={H} cap={cap} pos={pos} m={m}: rel-L2 {e:.2e}")
    assert e < TOL[dtype]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B,m", [(1, 8), (2, 4)])
def test_chunk_partials_feed_the_combine_prologues(ops, dtype, B, m):
    """ops.gemv_attn / ops.gemv_attn_w8 with B * m = 8 rows on the chunk's partials == on the partials of the m one-token calls"""
    H, cap, pos, N = 8, 384, 250, 512
    case = Case(dtype, B, H, cap, pos, m, seed=3)
    g = torch.Generator().manual_seed(9)
    w, bias = dev(rnd((N, H * 64), dtype, g, 0.05)), dev(rnd((N,), dtype, g))
    w8 = ops.quantize_rows_e4m3(w)
    parts, _, _ = case.chunk(ops, combine=False)
    seq_parts, _, _ = case.sequential(ops, combine=False)
    one = ops.gemv_attn(parts, B * m, H, cap, w, bias=bias)
    two = ops.gemv_attn(seq_parts, B * m, H, cap, w, bias=bias)
    assert bool(torch.isfinite(one.float()).all()) and _same(one, two)
    one8 = ops.gemv_attn_w8(parts, B * m, H, cap, w8, dtype, bias=bias)
    two8 = ops.gemv_attn_w8(seq_parts, B * m, H, cap, w8, dtype, bias=bias)
    assert bool(torch.isfinite(one8.float()).all()) and _same(one8, two8)
    out, _, _ = case.chunk(ops)
    assert _same(one, ops.gemm(out.view(B * m, H * 64), w, bias=bias))
    assert _same(one8, ops.gemm_w8(out.view(B * m, H * 64), w8, bias=bias))


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
    q = torch.zeros((B, 2, H, cap, 64), dtype=torch.uint8, device="cuda")
    s = torch.ones((B, 2, H, cap + 1), dtype=torch.float32, device="cuda")

    def desc(**kw):
        d = _lib.AttnDecodeChunkKv8Desc()
        d.dtype, d.B, d.H, d.capacity, d.head_dim, d.m, d.scale = _lib.F16, B, H, cap, 64, m, 0.125
        d.qkv, d.qkv_rs = qkv.data_ptr(), 3 * hp
        d.kv_q, d.kv_q_bs, d.kv_scale, d.kv_scale_bs = q.data_ptr(), 2 * H * cap * 64, s.data_ptr(), 2 * H * cap
        d.out, d.out_rs, d.pos, d.workspace, d.workspace_bytes = out.data_ptr(), hp, pos.data_ptr(), ws.data_ptr(), ws.numel()
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    call = lambda **kw: lib.cogv_attention_decode_chunk_kv8(C.byref(desc(**kw)), None)
    assert call() == 0
    assert call(m=0) == 1 and call(m=9) == 1 and call(m=-1) == 1
    assert call(qkv=qkv.data_ptr() + 2) == 1 and call(qkv_rs=3 * hp + 4) == 1
    assert call(kv_q=q.data_ptr() + 8) == 1 and call(kv_scale=s.data_ptr() + 2) == 1 and call(kv_q=None) == 1 and call(kv_scale=None) == 1
    assert call(kv_q_bs=2 * H * cap * 64 - 16) == 1 and call(kv_q_bs=2 * H * cap * 64 + 8) == 1 and call(kv_scale_bs=2 * H * cap - 1) == 1
    assert call(first=first.data_ptr() + 2) == 1 and call(first=first.data_ptr() + 4) == 0
    assert call(workspace_bytes=need - 1) == 1
    assert call(workspace_bytes=lib.cogv_attention_decode_workspace_bytes(B, H, cap)) == 1          # sized for B rows, not B * m
    assert call(out=None) == 1 and call(out=None, skip_combine=1) == 0
    assert call(dtype=_lib.F32) == 3 and call(head_dim=128) == 3
    torch.cuda.synchronize()
