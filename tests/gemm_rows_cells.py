"""Shared by tests/test_gemm_rows_plan.py (CPU) and tests/test_gemm_rows_gpu.py: the grid of the wide product's cell sweep
(cogv_gemm_rows, csrc/gemv_wide_plan.h), the operands of its exact-integer product and their fp64 reference.

The exact-integer product is tests/gemv_cells.py's with 64 rows and up to N_BIG columns: x, W in {-1, 0, 1}, an integer bias;
every partial sum is an integer far below 2^24, so an fp32 sum in any association is exact and the result equals the fp64 one to
the bit.  Densities as there: K / 16 non-zero products of +-1, a sum of standard deviation 25.3 at K = 10240; the 64 x 4104 sums of
a K stay below 5.2 sigma + 4 = 136 < 256 (asserted per K on the host before any launch; with these seeds the largest |ref| over
the grid's seven K is 121, at K = 10240, on the leading 136 columns as on all 4104)."""
import functools

import torch

from cogview_amd import _lib
from tests import gemv_cells as GC

DTYPES, DT_CODE, DT_NAME = GC.DTYPES, GC.DT_CODE, GC.DT_NAME
MS = (1, 9, 16, 17, 33, 48, 64)
N_BIG = 4104              # 129 workgroups of two column tiles from 17 rows on (the last one ends inside its first tile), 257 of one tile below
NS = (8, 40, 136, N_BIG)
KS = (512, 1024, 1536, 2560, 4096, 5632, 10240)
M_MAX, N_MAX = max(MS), max(NS)


def plan(dtype, M, N, K):
    """(code, the integers of cogv_gemm_rows_plan) of a contiguous product"""
    return _lib.gemm_rows_plan(DT_CODE[dtype], M, N, K)


def plan_id(out):
    """what identifies a plan besides its grid: everything but the workgroup count"""
    return tuple(out[:7]) + tuple(out[8:])


@functools.lru_cache(maxsize=1)
def exact_operands(K):
    """x [64, K], W [N_BIG, K], bias [N_BIG] as fp32 integers and ref [64, N_BIG] = x W^T + bias in fp64 (the fp32 product of
    these integers is exact, and is checked against fp64 on the leading 136 columns)"""
    g = torch.Generator().manual_seed(K)
    x, w = GC.ternary((M_MAX, K), GC.X_DENSITY, g).float(), GC.ternary((N_MAX, K), GC.W_DENSITY, g).float()
    bias = torch.randint(-GC.BIAS_MAX, GC.BIAS_MAX + 1, (N_MAX,), generator=g).float()
    ref = (x @ w.t() + bias).double()
    assert torch.equal(ref[:, :136], x.double() @ w[:136].double().t() + bias[:136].double())
    assert float(ref.abs().max()) <= min(GC.EXACT_MAX.values()), (K, float(ref.abs().max()))
    return x, w, bias, ref
