"""Shared by the tests of the 4-bit (OCP MXFP4) decode weights: the CPU quantizer and dequantizer of the rule in
include/cogview_hip.h, the code comparison that masks the sign of zero codes, and the grid the GPU sweep of the 4-bit launch
plans runs (tests/test_w4_cpu.py proves that it reaches every plan of GV_CLASSES_4).

THE RULE on bit patterns.  A block is 32 consecutive elements of a row; amax = max |x|:
    e = clamp(floor(log2(amax)) - 2, -126, 127), s = e + 127 (127 for a zero block);  code = E2M1 nearest to float(x) / 2^e,
    ties to the even code, above 6 -> 6.
With |x| = M * 2^(E - 150) (E: biased fp32 exponent, at least 1; M: significand with its hidden bit), 4 |x| / 2^e = M / 2^r with
r = s + 21 - E >= 19, and the code boundaries 0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5 are the integers 1, 3, 5, 7, 10, 14, 20: only
integer shifts and compares -- no division, no rounding.  quantize_float is the same rule in floating point (torch.frexp, a
power-of-two division in fp64, nearest by distance): the two are held against each other in tests/test_w4_cpu.py."""
import torch

from cogview_amd import _lib
from tests import gemv_cells as GC

E2M1 = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
BOUNDS = ((1, False), (3, True), (5, False), (7, True), (10, False), (14, True), (20, False))      # (4 * boundary, belongs to the code above)

KINDS, DTYPES, MS, NS = GC.KINDS, GC.DTYPES, GC.MS, GC.NS
# the issue's K, and what the class boundaries of GV_CLASSES_4 add: 2048 (a one-row column that ends with a whole 2048-element slot),
# 5632 and 9728 (one row: the guarded class up to 10240; more rows: above the guarded classes, refused)
KS = (512, 1024, 1536, 2048, 2560, 3072, 4096, 5120, 5632, 9728, 10240)
LN_MAX_K = 4096
M_MAX, N_MAX = max(MS), max(NS)
CAPS = GC.CAPS
# exact-integer product: x in {-1, 0, 1} with density 1/4, codes in {-1, 0, 1} with density 1/8, block scales in {1, 2, 1/2}, integer
# |bias| <= 4: a sum is a multiple of 1/2 of standard deviation sqrt(K / 32 * 1.75) = 24 at K = 10240; 6 sigma + 4 = 146 -- fp16
# holds multiples of 1/2 up to 1024, bf16 up to 128: asserted per K before any launch (the seeds are fixed)
X_DENSITY, W_DENSITY, BIAS_MAX = 0.25, 0.125, 4
EXACT_MAX = {torch.float16: 1024, torch.bfloat16: 128}


def ks(kind):
    return tuple(K for K in KS if kind != "ln" or K <= LN_MAX_K)


def plan(kind, dtype, M, N, K, nsplit=1):
    return _lib.gemv_w4_plan(GC.KIND_CODE[kind], GC.DT_CODE[dtype], M, N, K, nsplit=nsplit)


# ------------------------------------------------------------------------------------------------ the rule on the CPU
def pack(codes):
    """nibbles [N, K] (int) -> bytes [N, K / 2]: element 2i in the low nibble of byte i"""
    c = codes.to(torch.int64)
    return (c[:, 0::2] | (c[:, 1::2] << 4)).to(torch.uint8)


def unpack(q):
    """bytes [N, K / 2] -> nibbles [N, K] int64"""
    q = q.to(torch.int64)
    return torch.stack((q & 15, q >> 4), dim=-1).reshape(q.shape[0], -1)


def quantize(w):
    """w [N, K] fp16 / bf16 / fp32 (K % 32 == 0) -> (q [N, K / 2] uint8, s [N, K / 32] uint8), integer operations only"""
    N, K = w.shape
    bits = w.detach().cpu().float().contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    mag = bits & 0x7FFFFFFF
    amax = mag.view(N, K // 32, 32).amax(-1)
    s = torch.where(amax == 0, torch.full_like(amax, 127), ((amax >> 23) - 2).clamp(min=1))
    E = mag >> 23
    M = torch.where(E > 0, (mag & 0x7FFFFF) | 0x800000, mag)
    r = (s.repeat_interleave(32, dim=1) + 21 - E.clamp(min=1)).clamp(0, 26)
    code = torch.zeros_like(M)
    for b4, above in BOUNDS:
        code += (M >= (b4 << r)) if above else (M > (b4 << r))
    return pack(((bits >> 28) & 8) | code), s.to(torch.uint8)


def quantize_float(w):
    """the same rule in floating point: frexp for the exponent, an exact power-of-two division in fp64, the nearest E2M1 value by
    distance with ties to the even code"""
    N, K = w.shape
    x = w.detach().cpu().double().view(N, K // 32, 32)
    amax = x.abs().amax(-1)
    _, ex = torch.frexp(amax)                                   # amax = m * 2^ex, 0.5 <= m < 1: floor(log2) = ex - 1
    e = torch.where(amax > 0, (ex - 1 - 2).clamp(-126, 127), torch.zeros_like(ex))
    y = torch.ldexp(x.abs(), -e.unsqueeze(-1)).clamp(max=6.0)
    grid = torch.tensor(E2M1, dtype=torch.float64)
    d = (y.unsqueeze(-1) - grid).abs()
    lo = d.argmin(-1)                                           # the first of two equally near codes: the lower one
    tie = torch.gather(d, -1, (lo + 1).clamp(max=7).unsqueeze(-1)).squeeze(-1) == torch.gather(d, -1, lo.unsqueeze(-1)).squeeze(-1)
    code = torch.where(tie & (lo % 2 == 1) & (lo < 7), lo + 1, lo)
    nib = (code | torch.where(torch.signbit(x), 8, 0)).view(N, K)
    return pack(nib), (e + 127).to(torch.uint8)


def dequantize(q, s):
    """(q, s) -> the values [N, K] in fp64: sign * E2M1[code] * 2^(s - 127)"""
    nib = unpack(q.cpu())
    mag = torch.tensor(E2M1, dtype=torch.float64)[nib & 7]
    return torch.ldexp(torch.where((nib & 8) != 0, -mag, mag), (s.cpu().to(torch.int64) - 127).repeat_interleave(32, dim=1))


def same_codes(q_a, q_b):
    """byte tensors equal up to the sign bit of codes of magnitude zero"""
    a, b = unpack(q_a.cpu()), unpack(q_b.cpu())
    a = torch.where((a & 7) == 0, torch.zeros_like(a), a)
    b = torch.where((b & 7) == 0, torch.zeros_like(b), b)
    return torch.equal(a, b)


def crafted_rows(dtype):
    """One row of five blocks, each with one element of 4 * 2^e that fixes its scale at e (= 0, 3, -7, 0, and the clamp), and what
    the rule makes of them: ties, saturation, a zero block, a block at the exponent clamp.  -> (w [1, 160], nibbles [160], s [5])"""
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 7.0]
    tie_codes = [0, 2, 2, 4, 4, 6, 6, 7]
    near = [0.28125, 0.71875, 1.28125, 1.71875, 2.625, 3.375, 5.125, 0.21875]           # just off the ties, exact in 8 significant bits
    near_codes = [1, 1, 3, 3, 5, 5, 7, 0]
    blocks, codes, scales = [], [], []

    def block(vals, cds, e, top=4.0, top_code=6):
        v = torch.zeros(32, dtype=torch.float64)
        c = torch.zeros(32, dtype=torch.int64)
        n = len(vals)
        v[:n] = torch.tensor(vals, dtype=torch.float64)
        c[:n] = torch.tensor(cds)
        v[n:2 * n] = -v[:n]
        c[n:2 * n] = c[:n] | 8
        v[31], c[31] = top, top_code
        blocks.append(torch.ldexp(v, torch.tensor(e)))
        codes.append(c)
        scales.append(e + 127)

    block(ties, tie_codes, 0)
    block(near, near_codes, 3)
    # saturation: amax in (6, 8) * 2^e keeps e (floor(log2) = e + 2) and saturates to 6
    block([6.5, 7.5, 7.0, 6.0, 5.5, 0.0, 3.0, 1.0], [7, 7, 7, 7, 7, 0, 5, 2], -7, top=7.75, top_code=7)
    blocks.append(torch.zeros(32, dtype=torch.float64)); codes.append(torch.zeros(32, dtype=torch.int64)); scales.append(127)
    if dtype == torch.bfloat16:
        # below 2^-126 * 4: amax = 2^-125: e would be -127, clamps to -126 (s = 1); 2^-128 = 0.25 * 2^-126 is the tie that goes to 0
        v = torch.zeros(32, dtype=torch.float64)
        c = torch.zeros(32, dtype=torch.int64)
        for i, (m, cd) in enumerate(((2.0 ** -128, 0), (2.0 ** -127, 1), (2.0 ** -126, 2), (-(2.0 ** -126) * 1.5, 8 | 3), (2.0 ** -125, 4),
                                     (2.0 ** -127 * 1.5, 2), (-(2.0 ** -130), 8))):
            v[i], c[i] = m, cd
        blocks.append(v); codes.append(c); scales.append(1)
    else:
        # fp16's smallest values are far above the clamp: its smallest subnormal 2^-24 alone in a block: e = -26
        v = torch.zeros(32, dtype=torch.float64)
        c = torch.zeros(32, dtype=torch.int64)
        v[3], c[3] = -(2.0 ** -24), 8 | 6
        blocks.append(v); codes.append(c); scales.append(-26 + 127)
    w = torch.cat(blocks).view(1, -1)
    assert torch.equal(w.to(dtype).double(), w), "the crafted values are exact in the storage type"
    return w.to(dtype), torch.cat(codes), torch.tensor(scales, dtype=torch.uint8)


# ------------------------------------------------------------------------------------------------ operands of the GPU sweep
def exact_operands(K, dtype):
    """x [8, K] in {-1, 0, 1}; W = code * scale with codes in {-1, 0, 1} and a block scale of {1, 2, 1/2}, as (q, s) and in fp64;
    integer bias; ref = x W^T + bias in fp64, exact in `dtype`"""
    g = torch.Generator().manual_seed(4 * K + 1)
    x, c = GC.ternary((M_MAX, K), X_DENSITY, g), GC.ternary((N_MAX, K), W_DENSITY, g)
    e = torch.randint(-1, 2, (N_MAX, K // 32), generator=g)
    nib = torch.where(c > 0, 2, torch.where(c < 0, 10, 0))
    q, s = pack(nib), (e + 127).to(torch.uint8)
    w = dequantize(q, s)
    assert torch.equal(w, torch.ldexp(c, e.repeat_interleave(32, dim=1)))
    bias = torch.randint(-BIAS_MAX, BIAS_MAX + 1, (N_MAX,), generator=g).double()
    dot = x @ w.t()
    assert float((dot + bias).abs().max()) <= EXACT_MAX[dtype], (K, float((dot + bias).abs().max()))
    return x, (q, s), w, bias, dot


class Product:
    """One (kind, dtype, K) on the 4-bit weight qs: the device operands of the largest cell, launched at any (M, N) by leading
    rows (tests/gemv_cells.py: Product, whose operands for the three kinds these are)."""

    def __init__(self, ops, kind, dtype, K, x, qs, bias, z=None):
        self.ops, self.kind, self.dtype, self.K = ops, kind, dtype, K
        dev = "cuda"
        self.q, self.s = (t.to(dev) for t in qs)
        self.bias = bias.to(dtype).to(dev)
        if kind == "plain":
            self.x = x.to(dtype).to(dev)
        elif kind == "attn":
            self.parts = {cap: GC.partials(x.to(dev), (cap + 127) // 128) for cap in CAPS}
        else:
            self.z = z.to(dtype).to(dev)
            self.zero, self.zeros = torch.zeros(K, dtype=dtype, device=dev), torch.zeros((M_MAX, K), dtype=dtype, device=dev)
            self.beta = x[0].to(dtype).to(dev)

    def weight(self, N):
        return self.q[:N], self.s[:N]

    def __call__(self, M, N, bias=True, gelu=False, cap=128, post=False):
        ops, b, w = self.ops, (self.bias[:N] if bias else None), self.weight(N)
        if self.kind == "plain":
            return ops.gemm_w4(self.x[:M], w, bias=b, gelu=gelu)
        if self.kind == "attn":
            return ops.gemv_attn_w4(self.parts[cap][:M], M, self.K // 64, cap, w, self.dtype, bias=b)
        kw = dict(post=(self.zero, self.beta), residual=self.zeros[:M], want_t=True) if post else {}
        out, t = ops.gemv_ln_w4(self.z[:M], w, b, self.zero, self.beta, GC.EPS, gelu=gelu, **kw)
        if post and not torch.equal(t, self.beta.expand(M, self.K)):
            return None
        return out
