"""GPU: every cell of the wide product's launch plan (cogv_gemm_rows, csrc/gemv_wide_plan.h) executed on the grid of
tests/gemm_rows_cells.py -- tests/test_gemm_rows_plan.py proves on the CPU that the grid reaches every plan entry in both dtypes.
Operands with lda = K + 8 and ldb = K + 16, A followed by rows of NaN, C inside a buffer of sentinels.  Per cell: (a) the
exact-integer product, bit-equal to fp64; (b) a second call gives the same bits; (c) a `randn` product held element by element to
gemv_cells.bound with factor 1; (d) the GeLU epilogue against the fp64 tanh form; (e) the published abs-max == max|C|; per (dtype,
K) also (f) a permutation of A's rows permutes C's rows to the bit.  The launch returns the plan test's refusal codes."""
import ctypes as C

import pytest
import torch

from cogview_amd import _lib
from tests import gemm_rows_cells as RC
from tests import gemv_cells as GC
from tests.test_gemm_rows_plan import REFUSALS, _desc
from tests.test_kernels_gpu import TOL, rel

pytestmark = pytest.mark.gpu

SENTINEL = -77.0
CASES = [(dtype, K) for K in RC.KS for dtype in RC.DTYPES]
IDS = [f"{RC.DT_NAME[dtype]}-K{K}" for dtype, K in CASES]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X; run with -m 'not gpu' elsewhere"
    from cogview_amd import ops as _ops
    return _ops


def _a_with_nan_rows(x, M, K):
    """rows 0 .. M - 1 of x in a [M + 3, K + 8] buffer whose other elements are NaN: the view [M, K] with lda = K + 8"""
    buf = torch.full((M + 3, K + 8), float("nan"), dtype=x.dtype, device=x.device)
    buf[:M, :K] = x[:M]
    return buf[:M, :K]


def _padded_rows(w, K, pad):
    buf = torch.full((w.shape[0], K + pad), float("nan"), dtype=w.dtype, device=w.device)
    buf[:, :K] = w
    return buf[:, :K]


def _c_in_sentinels(M, N, dtype):
    buf = torch.full((M + 2, N + 16), SENTINEL, dtype=dtype, device="cuda")
    return buf, buf[1:M + 1, 8:8 + N]


def _intact(buf, M, N):
    b = buf.clone()
    b[1:M + 1, 8:8 + N] = SENTINEL
    return bool((b == SENTINEL).all())


def _gelu64(x):
    return 0.5 * x * (1.0 + torch.tanh(0.7978845608028654 * x * (1.0 + 0.044715 * x * x)))


@pytest.mark.parametrize("dtype,K", CASES, ids=IDS)
def test_exact_integer_product(ops, dtype, K):
    """(a), (b), (e), (f): x, W in {-1, 0, 1} and an integer bias == fp64, to the bit, on every (M, N) of the grid"""
    x, w, bias, ref = RC.exact_operands(K)              # |ref| <= 256 asserted there, on the host, before any launch
    xd, bd = x.to(dtype).cuda(), bias.to(dtype).cuda()
    wd = _padded_rows(w.to(dtype).cuda(), K, 16)
    ref_d = ref.to(dtype).cuda()
    assert torch.equal(ref_d.double().cpu(), ref)
    fails = []
    for M in RC.MS:
        a = _a_with_nan_rows(xd, M, K)
        for N in RC.NS:
            rc, pl = RC.plan(dtype, M, N, K)
            assert rc == _lib.OK
            where = f"{RC.DT_NAME[dtype]} M={M} N={N} K={K} {pl}"
            buf, out = _c_in_sentinels(M, N, dtype)
            slot = torch.zeros(1, dtype=torch.float32, device="cuda")
            got = ops.gemm_rows(a, wd[:N], bias=bd[:N], absmax=slot, out=out)
            if not torch.equal(got, ref_d[:M, :N]):
                fails.append(f"{where}: {int((got != ref_d[:M, :N]).sum())} wrong elements")
            if not _intact(buf, M, N):
                fails.append(f"{where}: a sentinel around C was overwritten")
            if float(slot) != float(ref[:M, :N].abs().max()):
                fails.append(f"{where}: abs-max {float(slot)} != {float(ref[:M, :N].abs().max())}")
            if not torch.equal(ops.gemm_rows(a, wd[:N], bias=bd[:N]), got):
                fails.append(f"{where}: the second call gives other bits")
    assert not fails, "\n".join(fails[:40])


@pytest.mark.parametrize("dtype,K", CASES, ids=IDS)
def test_randn_product_gelu_and_row_permutation(ops, dtype, K):
    """(c), (d), (e), (f) on every (M, N): the fp64 reference is taken once per (dtype, K), on the device"""
    g = torch.Generator().manual_seed(7 * K + 1)
    x = torch.randn((RC.M_MAX, K), generator=g).to(dtype).cuda()
    w = _padded_rows((torch.randn((RC.N_MAX, K), generator=g) * 0.05).to(dtype).cuda(), K, 16)
    bias = torch.randn(RC.N_MAX, generator=g).to(dtype).cuda()
    x64, w64, b64 = x.double(), w.double(), bias.double()
    ref = x64 @ w64.t() + b64
    bnd = GC.bound(ref, x64.abs() @ w64.abs().t(), b64, K, dtype)
    gelu_ref = _gelu64(ref)
    fails, worst = [], 0.0
    for M in RC.MS:
        a = _a_with_nan_rows(x, M, K)
        for N in RC.NS:
            where = f"{RC.DT_NAME[dtype]} M={M} N={N} K={K}"
            buf, out = _c_in_sentinels(M, N, dtype)
            slot = torch.zeros(1, dtype=torch.float32, device="cuda")
            got = ops.gemm_rows(a, w[:N], bias=bias[:N], absmax=slot, out=out)
            ratio = float(((got.double() - ref[:M, :N]).abs() / bnd[:M, :N]).max())
            worst = max(worst, ratio)
            if not ratio <= 1.0:
                fails.append(f"{where}: err / bound = {ratio:.3f}")
            if not _intact(buf, M, N):
                fails.append(f"{where}: a sentinel around C was overwritten")
            if float(slot) != float(got.float().abs().max()):
                fails.append(f"{where}: abs-max {float(slot)} != max|C| {float(got.float().abs().max())}")
            e = rel(ops.gemm_rows(a, w[:N], bias=bias[:N], gelu=True), gelu_ref[:M, :N])
            if not e < TOL[dtype]:
                fails.append(f"{where}: GeLU output rel-L2 {e:.2e}")
            if M > 1 and N in (136, RC.N_BIG):
                perm = torch.randperm(M, generator=g).cuda()
                if not torch.equal(ops.gemm_rows(_a_with_nan_rows(x[:M][perm], M, K), w[:N], bias=bias[:N]), got[perm]):
                    fails.append(f"{where}: permuted rows of A do not give the permuted rows of C")
    print(f"RATIO rows {RC.DT_NAME[dtype]} K={K}: worst err / bound = {worst:.4f}")
    assert not fails, "\n".join(fails[:40])


def test_a_row_does_not_depend_on_the_rows_next_to_it(ops):
    """row 0 of a 64-row call, of a 17-row call and of a 1-row call: the same bits (the class follows K alone)"""
    for dtype in RC.DTYPES:
        for K in (2560, 5632):
            g = torch.Generator().manual_seed(K)
            x = torch.randn((64, K), generator=g).to(dtype).cuda()
            w = (torch.randn((RC.N_BIG, K), generator=g) * 0.05).to(dtype).cuda()
            full = ops.gemm_rows(x, w)
            for M in (1, 17, 48):
                assert torch.equal(ops.gemm_rows(x[:M], w), full[:M]), (dtype, K, M)


def test_launch_returns_the_refusal_codes_of_the_plan(ops):
    lib = _lib.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for kw, code in REFUSALS:
        assert lib.cogv_gemm_rows(C.byref(_desc(**kw)), stream) == code, kw
    with pytest.raises(_lib.CogviewHipError):
        ops.gemm_rows(torch.zeros(65, 512, dtype=torch.float16, device="cuda"), torch.zeros(8, 512, dtype=torch.float16, device="cuda"))
    torch.cuda.synchronize()
