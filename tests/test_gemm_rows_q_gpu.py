"""GPU: every cell of the launch plans of the wide product on quantized weights (cogv_gemm_rows_w8 / cogv_gemm_rows_w4, GWQ_CLASSES
of csrc/gemv_wide_plan.h) executed on the grid of tests/gemm_rows_q_cells.py -- tests/test_gemm_rows_q_plan.py proves on the CPU
that the grid reaches every plan entry of both formats in both dtypes.  tests/test_gemm_rows_gpu.py's sweep per (format, dtype, K):
A with lda = K + 8 followed by rows of NaN, C inside a buffer of sentinels, the codes in a buffer with ldq = K / PK + 16 and the
padding filled with poison that must never be read -- 0x7F bytes (an E4M3 NaN) and NaN row scales behind the N the call names for
e4m3, 0x77 bytes (two codes of 6) and the scale byte 254 (2^127) in strided block scales for mxfp4.  Per cell: (a) the exact-integer
product, bit-equal to fp64; (b) a second call gives the same bits; (c) a `randn` product (weights of sigma 0.05 through the device
quantizer) held element by element to gemv_cells.bound with factor 1 against fp64 on the dequantized weights; (d) the GeLU epilogue
against the fp64 tanh form; (e) the published abs-max == max|C|; (f) a permutation of A's rows permutes C's rows to the bit.  Row 0
of a 64-, 17- and 1-row call has the same bits, and the launch returns the plan test's refusal codes."""
import ctypes as C

import pytest
import torch

from cogview_amd import _lib
from tests import gemm_rows_q_cells as QC
from tests import gemv_cells as GC
from tests import w4_cases as W4
from tests.test_gemm_rows_gpu import _a_with_nan_rows, _c_in_sentinels, _gelu64, _intact
from tests.test_gemm_rows_q_plan import _refusals
from tests.test_kernels_gpu import TOL, rel

pytestmark = pytest.mark.gpu

CASES = [(fmt, dtype, K) for fmt in QC.FORMATS for K in QC.KS for dtype in QC.DTYPES]
IDS = [f"{fmt}-{QC.DT_NAME[dtype]}-K{K}" for fmt, dtype, K in CASES]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X; run with -m 'not gpu' elsewhere"
    from cogview_amd import ops as _ops
    return _ops


class Operand:
    """The weight of one (format, K) on the device, in poisoned buffers: .take(N) is the operand of the leading N rows."""

    def __init__(self, fmt, qs):
        q, s = (t.cuda() for t in qs)
        self.fmt = fmt
        nq = q.shape[1]
        buf = torch.full((q.shape[0], nq + 16), 0x7F if fmt == "e4m3" else 0x77, dtype=torch.uint8, device="cuda")
        buf[:, :nq] = q
        self.q = buf[:, :nq]
        if fmt == "e4m3":
            self.s = s.float()
        else:
            sb = torch.full((s.shape[0], s.shape[1] + 8), 254, dtype=torch.uint8, device="cuda")
            sb[:, :s.shape[1]] = s
            self.s = sb[:, :s.shape[1]]

    def take(self, N):
        if self.fmt == "mxfp4":
            return self.q[:N], self.s[:N]
        s = torch.full((N + 8,), float("nan"), dtype=torch.float32, device="cuda")         # NaN right behind the N row scales
        s[:N] = self.s[:N]
        return self.q[:N], s[:N]


def _product(ops, fmt):
    return ops.gemm_rows_w8 if fmt == "e4m3" else ops.gemm_rows_w4


@pytest.mark.parametrize("fmt,dtype,K", CASES, ids=IDS)
def test_exact_integer_product(ops, fmt, dtype, K):
    """(a), (b), (e): x, codes in {-1, 0, 1}, power-of-two scales and an integer bias == fp64, to the bit, on every (M, N)"""
    x, qs, bias, ref = QC.exact_operands(fmt, K)        # representable in both storage types: asserted there, on the host, before any launch
    xd, bd = x.to(dtype).cuda(), bias.to(dtype).cuda()
    w, fn = Operand(fmt, qs), _product(ops, fmt)
    ref_d = ref.to(dtype).cuda()
    assert torch.equal(ref_d.double().cpu(), ref)
    fails = []
    for M in QC.MS:
        a = _a_with_nan_rows(xd, M, K)
        for N in QC.NS:
            rc, pl = QC.plan(fmt, dtype, M, N, K)
            assert rc == _lib.OK
            where = f"{fmt} {QC.DT_NAME[dtype]} M={M} N={N} K={K} {pl}"
            buf, out = _c_in_sentinels(M, N, dtype)
            slot = torch.zeros(1, dtype=torch.float32, device="cuda")
            wn = w.take(N)
            got = fn(a, wn, bias=bd[:N], absmax=slot, out=out)
            if not torch.equal(got, ref_d[:M, :N]):
                fails.append(f"{where}: {int((got != ref_d[:M, :N]).sum())} wrong elements")
            if not _intact(buf, M, N):
                fails.append(f"{where}: a sentinel around C was overwritten")
            if float(slot) != float(ref[:M, :N].abs().max()):
                fails.append(f"{where}: abs-max {float(slot)} != {float(ref[:M, :N].abs().max())}")
            if not torch.equal(fn(a, wn, bias=bd[:N]), got):
                fails.append(f"{where}: the second call gives other bits")
    assert not fails, "\n".join(fails[:40])


def _dequantized(fmt, qs):
    """the values the quantized pair holds, fp64 on the device"""
    q, s = qs
    if fmt == "e4m3":
        return q.view(torch.float8_e4m3fn).float().double() * s.double().unsqueeze(1)
    return W4.dequantize(q, s).cuda()


@pytest.mark.parametrize("fmt,dtype,K", CASES, ids=IDS)
def test_randn_product_gelu_and_row_permutation(ops, fmt, dtype, K):
    """(c), (d), (e), (f) on every (M, N): the fp64 reference is taken once per (format, dtype, K)"""
    g = torch.Generator().manual_seed(7 * K + 1)
    x = torch.randn((QC.M_MAX, K), generator=g).to(dtype).cuda()
    w16 = (torch.randn((QC.N_MAX, K), generator=g) * 0.05).to(dtype).cuda()
    bias = torch.randn(QC.N_MAX, generator=g).to(dtype).cuda()
    qs = (ops.quantize_rows_e4m3 if fmt == "e4m3" else ops.quantize_rows_mxfp4)(w16)
    w, fn = Operand(fmt, qs), _product(ops, fmt)
    x64, w64, b64 = x.double(), _dequantized(fmt, qs), bias.double()
    ref = x64 @ w64.t() + b64
    bnd = GC.bound(ref, x64.abs() @ w64.abs().t(), b64, K, dtype)
    gelu_ref = _gelu64(ref)
    fails, worst = [], 0.0
    for M in QC.MS:
        a = _a_with_nan_rows(x, M, K)
        for N in QC.NS:
            where = f"{fmt} {QC.DT_NAME[dtype]} M={M} N={N} K={K}"
            buf, out = _c_in_sentinels(M, N, dtype)
            slot = torch.zeros(1, dtype=torch.float32, device="cuda")
            wn = w.take(N)
            got = fn(a, wn, bias=bias[:N], absmax=slot, out=out)
            ratio = float(((got.double() - ref[:M, :N]).abs() / bnd[:M, :N]).max())
            worst = max(worst, ratio)
            if not ratio <= 1.0:
                fails.append(f"{where}: err / bound = {ratio:.3f}")
            if not _intact(buf, M, N):
                fails.append(f"{where}: a sentinel around C was overwritten")
            if float(slot) != float(got.float().abs().max()):
                fails.append(f"{where}: abs-max {float(slot)} != max|C| {float(got.float().abs().max())}")
            e = rel(fn(a, wn, bias=bias[:N], gelu=True), gelu_ref[:M, :N])
            if not e < TOL[dtype]:
                fails.append(f"{where}: GeLU output rel-L2 {e:.2e}")
            if M > 1 and N in (136, QC.N_BIG):
                perm = torch.randperm(M, generator=g).cuda()
                if not torch.equal(fn(_a_with_nan_rows(x[:M][perm], M, K), wn, bias=bias[:N]), got[perm]):
                    fails.append(f"{where}: permuted rows of A do not give the permuted rows of C")
    print(f"RATIO rows {fmt} {QC.DT_NAME[dtype]} K={K}: worst err / bound = {worst:.4f}")
    assert not fails, "\n".join(fails[:40])


@pytest.mark.parametrize("fmt", QC.FORMATS)
def test_a_row_does_not_depend_on_the_rows_next_to_it(ops, fmt):
    """row 0 of a 64-row call, of a 17-row call and of a 1-row call: the same bits (the class follows K alone)"""
    fn = _product(ops, fmt)
    for dtype in QC.DTYPES:
        for K in (2560, 5632):
            g = torch.Generator().manual_seed(K)
            x = torch.randn((64, K), generator=g).to(dtype).cuda()
            w16 = (torch.randn((QC.N_BIG, K), generator=g) * 0.05).to(dtype).cuda()
            qs = (ops.quantize_rows_e4m3 if fmt == "e4m3" else ops.quantize_rows_mxfp4)(w16)
            full = fn(x, qs)
            for M in (1, 17, 48):
                assert torch.equal(fn(x[:M], qs), full[:M]), (fmt, dtype, K, M)


@pytest.mark.parametrize("fmt", QC.FORMATS)
def test_launch_returns_the_refusal_codes_of_the_plan(ops, fmt):
    lib = _lib.lib()
    launch = lib.cogv_gemm_rows_w8 if fmt == "e4m3" else lib.cogv_gemm_rows_w4
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for d, w, code, kw in _refusals(fmt):
        assert launch(C.byref(d), C.byref(w), stream) == code, kw
    a = torch.zeros(65, 512, dtype=torch.float16, device="cuda")
    qs = (torch.zeros(8, 512, dtype=torch.uint8, device="cuda"), torch.ones(8, device="cuda")) if fmt == "e4m3" else \
        (torch.zeros(8, 256, dtype=torch.uint8, device="cuda"), torch.full((8, 16), 127, dtype=torch.uint8, device="cuda"))
    with pytest.raises(_lib.CogviewHipError):
        _product(ops, fmt)(a, qs)
    # the skinny entry points keep their 8 rows
    with pytest.raises(_lib.CogviewHipError):
        (ops.gemm_w8 if fmt == "e4m3" else ops.gemm_w4)(a[:9], qs)
    torch.cuda.synchronize()
