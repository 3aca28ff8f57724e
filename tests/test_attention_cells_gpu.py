"""GPU: the attention training kernels (cogview_amd/csrc/attention.hip) on every cell of tests/attention_cells.py -- the smallest
shapes that reach each path (tests/test_attention_cells_cpu.py proves that on the CPU), every form, operands inside guarded
allocations.  Per (form, dtype): (a) selector cells, exact to the bit; (b) decoy cells aimed at the first key a query must not
see; (c) `randn` cells element by element against fp64, lse row by row; (d) every stored keep bit against the oracle's mask;
(e) the fused bias gradient against the stored gradients; sentinels around every output intact and a second call bit-equal.
Beside the sweep: (f) the gathered inference form and the sparse training form in slot space with cogv_sparse_slot_reduce; (g) the
refusals through the launching entry points.

Worst err / bound as measured: DESIGN.md 4.2.1."""
import pytest
import torch

from tests import attention_cells as AC

pytestmark = pytest.mark.gpu

PARAMS = [(form, dtype) for form in AC.FORMS for dtype in AC.DTYPES]
IDS = [f"{form}-{AC.DT_NAME[dtype]}" for form, dtype in PARAMS]
DT_IDS = [AC.DT_NAME[d] for d in AC.DTYPES]


@pytest.fixture(scope="module")
def backend():
    assert torch.cuda.is_available(), "GPU tests need an MI355X; run with -m 'not gpu' elsewhere"
    from cogview_amd import ops
    return AC.Launched(ops)


def report(tag, worst):
    for name, r in sorted(worst.items()):
        print(f"RATIO {tag} {name}: worst err / bound = {r:.4f}")


@pytest.mark.parametrize("form,dtype", PARAMS, ids=IDS)
def test_cells(backend, form, dtype):
    """(a) - (e) on every shape of the grid, in one form and dtype"""
    fails, ran, refused, cells, worst = AC.sweep(backend, form, dtype)
    print(f"{form} {AC.DT_NAME[dtype]}: {ran} cells launched, {refused} refused, {len(fails)} failures")
    report(f"{form} {AC.DT_NAME[dtype]}", worst)
    assert not fails, "\n".join(fails[:40])
    assert ran + refused == cells == AC.cells_of(form) and refused == 0
    assert set(AC.OUTPUTS) <= set(worst) and all(f"{name} / randn" in worst for name in AC.OUTPUTS)


@pytest.mark.parametrize("dtype", AC.DTYPES, ids=DT_IDS)
def test_gathered_inference_form(backend, dtype):
    """(f) kv_index, forward only: an identity table and a sorted random table with flagged slots"""
    fails, ran, worst = AC.gather_sweep(backend, dtype)
    print(f"GATHER {AC.DT_NAME[dtype]}: {ran} cells launched, {len(fails)} failures")
    report(f"GATHER {AC.DT_NAME[dtype]}", worst)
    assert not fails, "\n".join(fails[:40])
    assert ran == len(AC.GATHER_CELLS) and set(worst) == {"o", "lse"}


@pytest.mark.parametrize("dtype", AC.DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("form", ("SPARSE", "SPARSE_DROP"))
def test_sparse_training_form(backend, form, dtype):
    """(f) forward, dQ and the slot-space dK / dV before the fold, dropout off and on"""
    fails, worst = AC.sparse_cell(backend, form, dtype)
    report(f"{form} {AC.DT_NAME[dtype]}", worst)
    assert not fails, "\n".join(fails[:40])
    assert set(worst) == set(AC.OUTPUTS)


@pytest.mark.parametrize("dtype", AC.DTYPES, ids=DT_IDS)
def test_sparse_slot_reduce(backend, dtype):
    """(f) cogv_sparse_slot_reduce alone on integer slot gradients: bit-equal to the fold it documents"""
    fails = AC.slot_reduce_cell(backend, dtype)
    assert not fails, "\n".join(fails[:40])


@pytest.mark.parametrize("dtype", AC.DTYPES, ids=DT_IDS)
def test_refusals(backend, dtype):
    """(g) the launching entry points answer the plan's code and write nothing"""
    fails, n = AC.refusal_sweep(backend, dtype)
    print(f"refusals {AC.DT_NAME[dtype]}: {n} descriptors, {len(fails)} failures")
    assert not fails, "\n".join(fails)
    assert n == len(AC.REFUSALS) >= 12
