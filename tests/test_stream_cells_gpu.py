"""GPU: the trainer's memory-bound kernels (cogview_amd/csrc/elementwise.hip, cogview_amd/csrc/ce_optim.hip) on every cell of
tests/stream_cells.py -- the smallest shapes that reach each path (tests/test_stream_cells_cpu.py proves that on the CPU): the capped
grid's second pass of every flat kernel, the scalar tails, every embedding mode, the column sum's slabs and its finalize kernel's
unrolled and tail loops, the cross entropy around a thread's second vector and at the shard's edges, chunk tables past the workgroup
caps of the gradient statistics and of AdamW.  Operands lie inside guarded allocations and are passed through the C ABI.  add, scale,
add_stream, the casts, dropout, embedding forward, every absmax, rowmax, predicted, params == round_T(master) and the `exact` cells are
judged to the bit; GELU, sumexp, loss, dlogits, the `randn` column sums and embedding gradients, the sum of squares and AdamW's state
element by element against fp64 within bounds derived from the kernels' own roundings.  Sentinels around every output and workspace
intact; a second call, in-place outputs restored, bit-equal.

Worst err / bound as measured: MEASURED in tests/stream_cells.py."""
import pytest
import torch

from tests import stream_cells as SC

pytestmark = pytest.mark.gpu

IDS = [SC.NAME[d] for d in SC.DTYPES]
IDS3 = [SC.NAME[d] for d in SC.CE_DTYPES]


@pytest.fixture(scope="module")
def backend():
    assert torch.cuda.is_available(), "GPU tests need an MI355X; run with -m 'not gpu' elsewhere"
    from cogview_amd import ops
    return SC.Launched(ops)


def report(tag, fails, cells, worst=None):
    print(f"{tag}: {cells} cells, {len(fails)} failures")
    for (op, name), r in sorted((worst or {}).items()):
        print(f"RATIO {tag} {op} {name}: worst err / bound = {r:.4f}")
    assert not fails, "\n".join(fails[:40])


@pytest.mark.parametrize("dtype", SC.DTYPES, ids=IDS)
@pytest.mark.parametrize("op", SC.FLAT_OPS)
def test_flat_cells(backend, op, dtype):
    """one flat kernel on one lane, 255 lanes, a full workgroup, a second workgroup with one lane and the capped grid's second pass
    (the casts: and the three tail sizes)"""
    fails, cells, worst = SC.flat_sweep(backend, op, dtype)
    report(f"{op} {SC.NAME[dtype]}", fails, cells, worst)
    assert cells == 5 + 3 * (op in SC.TAILED) and (op not in ("gelu_fwd", "gelu_bwd") or len(worst) == 1)


@pytest.mark.parametrize("dtype", SC.CE_DTYPES, ids=IDS3)
def test_absmax_cells(backend, dtype):
    """cogv_absmax: the maximum in the first element, the last vector and the scalar tail, a NaN, a negative largest magnitude"""
    fails, cells = SC.absmax_sweep(backend, dtype)
    report(f"absmax {SC.NAME[dtype]}", fails, cells)
    assert cells >= 28


@pytest.mark.parametrize("dtype", SC.DTYPES, ids=IDS)
def test_embedding_forward_cells(backend, dtype):
    """{T, fp32 out} x {ids, x_in} x {pos} x {dropout} x {absmax slot}, ids on both edges of the shard, clamped position ids: to the bit"""
    fails, cells = SC.emb_fwd_sweep(backend, dtype)
    report(f"embedding_fwd {SC.NAME[dtype]}", fails, cells)
    assert cells == 27


@pytest.mark.parametrize("dtype", SC.DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", SC.EMB_BWD_SHAPES, ids=str)
def test_embedding_backward_cells(backend, shape, dtype):
    """dtable, dpos, dx for unique keys, a key across scan windows, one key on every token and keys outside the shard"""
    fails, cells, worst = SC.emb_bwd_sweep(backend, shape, dtype)
    report(f"embedding_bwd {shape} {SC.NAME[dtype]}", fails, cells, worst)
    assert cells == 16 and {n for _, n in worst} == {"dtable", "dpos", "dx"}


@pytest.mark.parametrize("dtype", SC.DTYPES, ids=IDS)
def test_column_sum_cells(backend, dtype):
    fails, cells, worst = SC.colsum_sweep(backend, dtype)
    report(f"colsum {SC.NAME[dtype]}", fails, cells, worst)
    assert cells == 24 and len(worst) == 1


@pytest.mark.parametrize("dtype", SC.DTYPES, ids=IDS)
def test_column_sum_finalize_cells(backend, dtype):
    """cogv_colsum_finalize called directly: 1 .. 100 partial rows, the unrolled loop and the tail of every row slice"""
    fails, cells, worst = SC.finalize_sweep(backend, dtype)
    report(f"colsum_finalize {SC.NAME[dtype]}", fails, cells, worst)
    assert cells == 32 and len(worst) == 1


@pytest.mark.parametrize("ldt", SC.CE_DTYPES, ids=IDS3)
def test_cross_entropy_cells(backend, ldt):
    """forward and backward on every shape x target cell, loss == NULL, the maximum in the last column, equal logits, a first vector of
    -inf, and two shards combined against the whole-vocabulary loss"""
    fails, cells, worst = SC.ce_sweep(backend, ldt)
    report(f"cross entropy {SC.NAME[ldt]}", fails, cells, worst)
    assert cells == 59 and {n for _, n in worst} == {"sumexp", "loss", "loss2", "dlogits"}


@pytest.mark.parametrize("gdt", SC.CE_DTYPES, ids=IDS3)
def test_grad_stats_cells(backend, gdt):
    """the eight chunk lengths, 2051 chunks on 2048 workgroups, inf and NaN in a scalar tail"""
    fails, cells, worst = SC.grad_stats_sweep(backend, gdt)
    report(f"grad_stats {SC.NAME[gdt]}", fails, cells, worst)
    assert cells == 4 and len(worst) == 1


@pytest.mark.parametrize("dtype", SC.DTYPES, ids=IDS)
def test_adamw_cells(backend, dtype):
    """decoupled and L2 decay, clipping inactive and active, no bias correction, the norm override, a loss scale, steps 1 and 2, 4100
    chunks on 4096 workgroups, and the skipped step after an overflow"""
    fails, cells, worst = SC.adam_sweep(backend, dtype)
    report(f"adamw {SC.NAME[dtype]}", fails, cells, worst)
    assert cells == 18 and {n for _, n in worst} == {"master", "exp_avg", "exp_avg_sq"}
