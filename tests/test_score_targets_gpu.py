"""GPU: the candidate scorer (cogv_score_targets through ops.score_targets) against a float64 torch computation made on the
CPU from the SAME logits tensor: log_softmax over the allowed slice, gather, group sums.

The bound is derived, not tuned: widening 16-bit logits to fp32 is exact; fp32 expf / logf and a per-thread sum of at most
64 sequential terms followed by a short fixed tree give at most ~1e-5 absolute error per log-probability for |logits| <= 30;
the tests draw 3 * randn and assert |logp - ref| <= 1e-4 per row (a tenfold margin) and |score - ref| <= 1e-4 * group."""
import pytest
import torch

from cogview_amd import ops
from cogview_amd._lib import CogviewHipError

pytestmark = pytest.mark.gpu

TOL = 1e-4
NEG_INF = -float("inf")


def _logits(shape, dtype, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (3.0 * torch.randn(*shape, generator=g)).to(dtype).cuda()


def _targets(rows, lo, hi, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi, (rows,), generator=g)


def _reference(x, targets, allow, group):
    """float64 on the CPU from the device tensor's own values; a target outside `allow` scores -inf."""
    v = x.shape[-1]
    lo, hi = (0, v) if allow is None else allow
    x2 = x.detach().cpu().reshape(-1, v).double()
    t = targets.cpu().reshape(-1)
    lp = torch.log_softmax(x2[:, lo:hi], dim=-1).gather(1, (t - lo).clamp(0, hi - lo - 1).unsqueeze(1)).squeeze(1)
    lp[(t < lo) | (t >= hi)] = NEG_INF
    return lp, lp.view(-1, group).sum(dim=1)


def _check(x, targets, allow, group, what):
    assert torch.cuda.is_available(), "GPU tests need an MI355X; run with -m 'not gpu' elsewhere"
    logp, scores = ops.score_targets(x, targets.cuda(), allow=allow, group=group)
    ref_lp, ref_sc = _reference(x, targets, allow, group)
    rows = ref_lp.numel()
    assert logp.dtype == scores.dtype == torch.float32 and tuple(logp.shape) == (rows,) and tuple(scores.shape) == (rows // group,)
    lp, sc = logp.cpu().double(), scores.cpu().double()
    fin_lp, fin_sc = torch.isfinite(ref_lp), torch.isfinite(ref_sc)
    assert torch.equal(lp[~fin_lp], ref_lp[~fin_lp]) and torch.equal(sc[~fin_sc], ref_sc[~fin_sc])     # -inf where the reference has it
    e_lp = float((lp[fin_lp] - ref_lp[fin_lp]).abs().max()) if fin_lp.any() else 0.0
    e_sc = float((sc[fin_sc] - ref_sc[fin_sc]).abs().max()) if fin_sc.any() else 0.0
    print(f"{what}: max |logp - ref| = {e_lp:.3e} (bound {TOL:.0e}), max |score - ref| = {e_sc:.3e} (bound {TOL * group:.0e})")
    assert torch.isfinite(lp[fin_lp]).all() and torch.isfinite(sc[fin_sc]).all()
    assert e_lp <= TOL and e_sc <= TOL * group
    return logp, scores


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_aligned_vector_path_production_layout(dtype):
    """58 240 ids, the 8192 image codes excluded, two candidates of nine text positions: 16-byte loads, no ragged ends."""
    x = _logits((18, 58240), dtype)
    assert x.data_ptr() % 16 == 0
    _check(x, _targets(18, 8192, 58240), (8192, 58240), 9, f"vector {dtype}")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_scalar_path_nothing_a_multiple_of_eight(dtype):
    """vocab 1003 in rows 1011 elements apart: neither the rows nor the range are 16-byte aligned."""
    big = _logits((6, 1011), dtype, seed=2)
    x = big[:, :1003]
    assert x.stride(0) == 1011 and (x.stride(0) * x.element_size()) % 16 != 0
    _check(x, _targets(6, 37, 990), (37, 990), 3, f"scalar {dtype}")


def test_strided_vector_path_slice_of_a_larger_tensor():
    """big[:, 5:9, :] of [3, 16, 4096]: rows strided and aligned, scored where they lie; the range's ragged ends (100 and 4001
    are no multiples of 8) go through the vector path's end ids."""
    big = _logits((3, 16, 4096), torch.float16, seed=3)
    x = big[:, 5:9, :]
    assert not x.is_contiguous()
    _check(x, _targets(12, 0, 4096).view(3, 4), None, 4, "strided vector, whole vocabulary")
    _check(x, _targets(12, 100, 4001).view(3, 4), (100, 4001), 4, "strided vector, ragged range")


def test_vector_path_with_rows_really_strided():
    """big[:, :4096] of [6, 4104] fp16: ONE launch on the 16-byte-load kernel with row_stride (4104) > vocab (4096)."""
    big = _logits((6, 4104), torch.float16, seed=13)
    x = big[:, :4096]
    assert x.stride(0) == 4104 and x.data_ptr() % 16 == 0 and (x.stride(0) * x.element_size()) % 16 == 0
    _check(x, _targets(6, 100, 4001), (100, 4001), 3, "vector, row stride 4104")


def test_fp32_vector_path():
    """fp32 rows of 1000 ids: 16-byte loads of four, a range that starts and ends inside a load."""
    x = _logits((6, 1000), torch.float32, seed=4)
    _check(x, _targets(6, 3, 998), (3, 998), 2, "vector fp32")


def test_targets_at_the_edges_and_outside():
    lo, hi = 1000, 3000
    x = _logits((8, 4096), torch.float16, seed=5)
    t = torch.tensor([lo, hi - 1, lo - 1, 1500, hi, 1500, 1200, 1300])
    logp, scores = _check(x, t, (lo, hi), 2, "edges")
    assert torch.isfinite(logp).tolist() == [True, True, False, True, False, True, True, True]
    assert logp[2].item() == NEG_INF and logp[4].item() == NEG_INF
    assert torch.isfinite(scores).tolist() == [True, False, False, True]
    assert scores[1].item() == NEG_INF and scores[2].item() == NEG_INF
    # the same on the scalar path, with ids outside the vocabulary too
    xs = _logits((4, 1011), torch.float16, seed=6)[:, :1003]
    logp, _ = _check(xs, torch.tensor([37, 989, 36, 990]), (37, 990), 1, "edges, scalar")
    assert torch.isfinite(logp).tolist() == [True, True, False, False]
    logp, _ = ops.score_targets(xs, torch.tensor([-1, 1003, 1 << 40, 500]).cuda())
    assert torch.isfinite(logp).tolist() == [False, False, False, True]


def test_small_limits():
    x = _logits((4, 4096), torch.float16, seed=7)
    for xx, what in ((x, "vector"), (x[:, 1:1000], "scalar")):
        logp, scores = _check(xx, torch.full((4,), 77), (77, 78), 2, f"one allowed id, {what}")
        assert logp.tolist() == [0.0] * 4 and scores.tolist() == [0.0] * 2           # exactly: x - max = 0, log(1) = 0
    _check(x[2:3], _targets(1, 0, 4096), None, 1, "one row, one group")
    _check(x[1:2, 5:6], torch.zeros(1, dtype=torch.int64), None, 1, "vocabulary of one id")
    x33 = _logits((33, 257), torch.float32, seed=8)
    _check(x33, _targets(33, 0, 257), None, 33, "group of 33")


def test_same_bits_run_after_run():
    x = _logits((18, 58240), torch.float16, seed=9)
    t = _targets(18, 8192, 58240).cuda()
    a = ops.score_targets(x, t, allow=(8192, 58240), group=9)
    b = ops.score_targets(x, t, allow=(8192, 58240), group=9)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    xs = _logits((6, 1011), torch.float32, seed=10)[:, :1003]
    ts = _targets(6, 37, 990).cuda()
    a = ops.score_targets(xs, ts, allow=(37, 990), group=3)
    b = ops.score_targets(xs, ts, allow=(37, 990), group=3)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_outputs_given_by_the_caller_are_filled_in_place():
    x = _logits((6, 4096), torch.float16, seed=11)
    t = _targets(6, 0, 4096).cuda()
    logp = torch.full((6,), 7.0, device="cuda")
    scores = torch.full((8,), 7.0, device="cuda")
    got = ops.score_targets(x, t, group=3, logp=logp, scores=scores[2:4])
    want = ops.score_targets(x, t, group=3)
    assert got[0].data_ptr() == logp.data_ptr() and torch.equal(logp, want[0]) and torch.equal(scores[2:4], want[1])
    assert scores[:2].tolist() == [7.0, 7.0] and scores[4:].tolist() == [7.0] * 4


def test_argument_errors():
    x = _logits((6, 1024), torch.float16, seed=12)
    t = _targets(6, 0, 1024).cuda()
    with pytest.raises(CogviewHipError):
        ops.score_targets(x, t, group=4)                               # rows % group != 0
    with pytest.raises(CogviewHipError):
        ops.score_targets(x, t, group=0)
    with pytest.raises(CogviewHipError):
        ops.score_targets(x, t, allow=(100, 100))                      # empty range
    with pytest.raises(CogviewHipError):
        ops.score_targets(x, t, allow=(0, 1025))                       # past the vocabulary
    with pytest.raises(CogviewHipError):
        ops.score_targets(x.as_strided((6, 1024), (1000, 1)), t)       # row_stride < vocab
    with pytest.raises(CogviewHipError):
        ops.score_targets(x.cpu(), t.cpu())
