"""GPU: cogv_gemm launches what its plan names.  For the smallest shapes at which each path of the dispatch (csrc/gemm_plan.h) can
go wrong -- each kernel generation, edge tiles, split-K with its reduce pass, the fourth operand layout -- the auto-dispatched
product and the product with the kernel_variant of the planned generation are the same launch, so they agree bit for bit (output
and abs-max: the split-K reduce sums in a fixed order, the abs-max is an order-free maximum), and the result is within the
single-kernel tolerance of the fp32 product.  tests/test_gemm_plan.py pins the plans themselves; the exact-prefetch path, which
needs more tiles than CUs, is tests/test_gemm_bench_scale_gpu.py's."""
import pytest
import torch

from tests.test_gemm_plan import NT, TA, TN, desc, plan
from tests.test_kernels_gpu import DTYPES, TOL, dev, rel, rnd

pytestmark = pytest.mark.gpu

VARIANT = {1: 1, 2: 3, 3: 9, 4: 10}               # generation -> kernel_variant
CODE = {torch.float16: 0, torch.bfloat16: 1}


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X; run with -m 'not gpu' elsewhere"
    from cogview_amd import ops as _ops
    return _ops


CASES = [
    # (M, N, K), layout, splitk, kernel_variant asked for, generation planned
    ((56, 64, 64), NT, 1, 0, 1), ((64, 64, 72), NT, 1, 0, 1),
    ((64, 64, 64), NT, 1, 0, 2), ((255, 256, 64), NT, 1, 0, 2), ((256, 128, 64), NT, 1, 0, 2),
    ((256, 256, 64), NT, 1, 0, 4), ((264, 520, 256), NT, 1, 0, 4),
    ((256, 256, 64), NT, 1, 9, 3),
    ((56, 64, 256), NT, 2, 0, 1), ((64, 64, 256), NT, 2, 0, 2), ((256, 256, 256), NT, 2, 9, 3), ((256, 256, 256), NT, 2, 0, 4),
    ((264, 136, 128), TA, 1, 0, 2), ((256, 256, 64), TA, 1, 0, 4),
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape,layout,splitk,ask,generation", CASES)
def test_auto_dispatch_is_the_planned_kernel(ops, dtype, shape, layout, splitk, ask, generation):
    M, N, K = shape
    rc, out = plan(desc(M, N, K, layout, CODE[dtype], splitk=splitk, kernel_variant=ask), cus=0)
    assert (rc, out[0], out[1], out[6]) == (0, 0, generation, splitk)
    g = torch.Generator().manual_seed(M * 7 + N + K)
    a, b = rnd((K, M) if layout == TA else (M, K), dtype, g), rnd((N, K), dtype, g, 0.1)
    ref = (a.float().t() if layout == TA else a.float()) @ b.float().t()
    got = []
    for variant in (ask, VARIANT[generation]):
        amax = torch.zeros(1, dtype=torch.float32, device="cuda")
        got.append((ops.gemm(dev(a), dev(b), trans_a=layout == TA, splitk=splitk, variant=variant, absmax=amax), amax))
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
    assert rel(got[0][0], ref) < TOL[dtype]
    assert got[0][1].item() == got[0][0].float().abs().max().item()


@pytest.mark.parametrize("dtype", DTYPES)
def test_grouped_falls_back_where_the_library_refuses(ops, dtype):
    """A weight gradient whose dY rows are 2^25 elements apart (64 rows: a span of 4 GiB, past the persistent kernel's 32-bit
    offsets) passed the Python predicate ops.gemm_grouped used to have and made cogv_gemm_grouped raise; it is now one cogv_gemm,
    which generation 2 takes.  (M = 260 under trans_a, the other such case, is a bad argument to cogv_gemm as well.)"""
    M, N, K = 264, 256, 64
    g = torch.Generator().manual_seed(5)
    dy, x, prev = rnd((K, M), dtype, g), rnd((K, N), dtype, g), rnd((M, N), dtype, g, 3.0)
    wide = torch.empty((K, 1 << 25), dtype=dtype, device="cuda")[:, :M]
    wide.copy_(dy)
    assert plan(desc(M, N, K, TN, CODE[dtype], lda=1 << 25), cus=0)[1][1] == 2 and not ops._persistent_takes(desc(M, N, K, TN, CODE[dtype], lda=1 << 25))
    out = dev(prev.clone())
    ops.gemm_grouped([(wide, dev(x), out)], trans_a=True, trans_b=True, accumulate=True)
    assert rel(out, dy.float().t() @ x.float() + prev.float()) < TOL[dtype]
    # ... and next to a problem the grouped kernel takes, both come out right
    out2, out3 = dev(prev.clone()), dev(prev.clone())
    ops.gemm_grouped([(dev(dy), dev(x), out2), (wide, dev(x), out3)], trans_a=True, trans_b=True, accumulate=True)
    for o in (out2, out3):
        assert rel(o, dy.float().t() @ x.float() + prev.float()) < TOL[dtype]
