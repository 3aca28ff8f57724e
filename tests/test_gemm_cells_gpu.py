"""GPU: every cell of the tile-GEMM launch plan (csrc/gemm_plan.h) and every fused epilogue executed -- tests/gemm_cells.py holds the
grid, the epilogue cells, the guarded operands and the fp64 references; tests/test_gemm_plan.py proves on the CPU that the grid
reaches every generation's edge tiles, k-tile counts, uneven splits and the item hand-over of the persistent kernels.
Per (generation, layout, dtype): (a) exact-integer cells, bit-equal to fp64 rounded once -- values, zero signs under dropout,
abs-max, fused column sums -- with every sentinel around every output intact; (b) GeLU / dGeLU cells within 1 ulp of fp64 at exact
integer arguments; (c) the refusals, with the plan's code and nothing written; (d) a second call gives the same bits; (e) a
`randn` product against fp64 element by element.  Beside the sweep: cogv_gemm_grouped across problem and split boundaries.

Worst err / bound of (e) as measured: DESIGN.md 4.1.6."""
import pytest
import torch

from tests import gemm_cells as GC

pytestmark = pytest.mark.gpu

PARAMS = [(gen, layout, dtype) for gen in GC.GENERATIONS for layout in GC.LAYOUTS for dtype in GC.DTYPES]
IDS = [f"gen{gen}-{GC.LAYOUT_NAME[layout]}-{GC.DT_NAME[dtype]}" for gen, layout, dtype in PARAMS]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X; run with -m 'not gpu' elsewhere"
    from cogview_amd import ops as _ops
    return _ops


@pytest.mark.parametrize("gen,layout,dtype", PARAMS, ids=IDS)
def test_cells(ops, gen, layout, dtype):
    """(a) - (e) on every shape of the generation's row, in one layout and dtype"""
    fails, ran, refused, cells = GC.sweep(ops, gen, layout, dtype)
    more, worst = GC.randn_ratios(ops, gen, layout, dtype)
    print(f"gen {gen} {GC.LAYOUT_NAME[layout]} {GC.DT_NAME[dtype]}: {ran} cells launched, {refused} refused, {len(fails) + len(more)} failures")
    for tag, r in worst.items():
        print(f"RATIO gen {gen} {GC.LAYOUT_NAME[layout]} {GC.DT_NAME[dtype]} {tag}: worst err / bound = {r:.4f}")
    fails += more
    assert not fails, "\n".join(fails[:40])
    assert ran + refused == cells == sum(len(GC.cells_of(shape[3])) for shape, _ in GC.GRID[gen]) and refused > 0
    assert len(worst) == len(GC.RANDN_SHAPES)


def test_grouped(ops):
    """three problems in one persistent launch, per-problem flags and split-K, on the full grid and on 8 workgroups (items chain
    across problem and split boundaries): exact, canaries intact, each problem bit-equal to its launch alone"""
    fails, runs = [], 0
    for layout in GC.LAYOUTS:
        for dtype in GC.DTYPES:
            for wg8 in (False, True):
                fails += GC.grouped_sweep(ops, layout, dtype, wg8)
                runs += 1
    print(f"grouped: {runs} launches of {len(GC.GROUP)} problems, {len(fails)} failures")
    assert not fails, "\n".join(fails[:40])
