"""Shared by tests/test_gemm_rows_q_plan.py (CPU) and tests/test_gemm_rows_q_gpu.py: the grid of the cell sweep of the wide
product on quantized weights (cogv_gemm_rows_w8 / cogv_gemm_rows_w4, GWQ_CLASSES of csrc/gemv_wide_plan.h), the operands of its
exact-integer products and their fp64 references.

The exact-integer product is tests/gemm_rows_cells.py's -- x in {-1, 0, 1} with density 1/2, weight codes in {-1, 0, 1} with
density 1/8 (the densities of tests/gemv_cells.py), an integer bias, 64 rows and up to 4104 columns -- with the formats' scales
on top, all powers of two, so that every partial sum is a multiple of 1/2 far below 2^23 and an fp32 sum in any association is
exact:

  e4m3   the bytes 0xB8 / 0x00 / 0x38 and a row scale of {1, 2, 1/2}, column n taking SCALES[n % 3].  The unscaled sums are those of
         tests/gemm_rows_cells.py (same seeds: at most 121 + 4 in magnitude), so a scaled one plus its bias stays below 256 -- an
         integer bf16 holds -- and a halved one is a multiple of 1/2 below 128.
  mxfp4  the nibbles 0xA / 0x0 / 0x2 and one block-scale byte per 32 elements of {127, 128, 126} = {1, 2, 1/2} (the convention of
         tests/w4_cases.py).  bf16 holds multiples of 1/2 only below 128 and integers below 256, and a sum over blocks of all three
         scales has a standard deviation of 33 at K = 10240: 5.2 sigma is neither.  So a column draws its blocks from TWO of the
         three bytes: an even column from {127, 126} (multiples of 1/2, sigma = sqrt(K / 16 * 0.625) = 20: 5.2 sigma + 4 = 108 <
         128), an odd one from {127, 128} (integers, sigma = 40: 212 < 256).  Every column still changes its scale from block to
         block, and all three bytes are used.

Both references are asserted representable in fp16 and in bf16 on the host, before anything is launched."""
import functools

import torch

from cogview_amd import _lib
from tests import gemm_rows_cells as RC
from tests import gemv_cells as GC
from tests import w4_cases as W4

FORMATS = ("e4m3", "mxfp4")
PK = {"e4m3": 1, "mxfp4": 2}                   # contraction elements per byte of the codes
DTYPES, DT_CODE, DT_NAME = GC.DTYPES, GC.DT_CODE, GC.DT_NAME
MS = (1, 9, 16, 17, 33, 48, 64)
N_BIG = 4104
NS = (8, 40, 136, N_BIG)
KS = (512, 1024, 1536, 2560, 4096, 5632, 10240)
M_MAX, N_MAX = max(MS), max(NS)
SCALES = (1.0, 2.0, 0.5)
SCALE_BYTES = (127, 128, 126)


def plan(fmt, dtype, M, N, K, **kw):
    """(code, the integers of cogv_gemm_rows_w8_plan / cogv_gemm_rows_w4_plan) of a contiguous product"""
    fn = _lib.gemm_rows_w8_plan if fmt == "e4m3" else _lib.gemm_rows_w4_plan
    return fn(DT_CODE[dtype], M, N, K, **kw)


plan_id = RC.plan_id


def _representable(ref):
    for dtype in DTYPES:
        assert torch.equal(ref.to(dtype).double(), ref), f"the reference is not exact in {DT_NAME[dtype]}"


@functools.lru_cache(maxsize=2)
def exact_operands(fmt, K):
    """x [64, K] fp32 in {-1, 0, 1}, the weight operand of [N_BIG] rows as the format's (codes, scales), bias [N_BIG] fp32 integers
    and ref [64, N_BIG] = x dequantized(W)^T + bias in fp64, exact in both storage types"""
    if fmt == "e4m3":
        x, w, bias, _ = RC.exact_operands(K)
        scale = torch.tensor(SCALES)[torch.arange(N_MAX) % 3]
        ref = (x.double() @ w.double().t()) * scale.double() + bias.double()
        _representable(ref)
        return x, (GC.e4m3_bytes(w), scale), bias, ref
    g = torch.Generator().manual_seed(4 * K + 3)
    x, c = GC.ternary((M_MAX, K), GC.X_DENSITY, g).float(), GC.ternary((N_MAX, K), GC.W_DENSITY, g)
    bias = torch.randint(-GC.BIAS_MAX, GC.BIAS_MAX + 1, (N_MAX,), generator=g).float()
    pick = torch.randint(0, 2, (N_MAX, K // 32), generator=g)                       # 0: scale 1; 1: the column's other scale
    other = torch.where(torch.arange(N_MAX) % 2 == 0, 126, 128).view(-1, 1)
    s = torch.where(pick == 0, torch.full_like(pick, 127), other.expand_as(pick)).to(torch.uint8)
    assert set(s.unique().tolist()) == set(SCALE_BYTES)
    q = W4.pack(torch.where(c > 0, 2, torch.where(c < 0, 10, 0)))
    ref = x.double() @ W4.dequantize(q, s).t() + bias.double()
    _representable(ref)
    return x, (q, s), bias, ref
