"""GPU: the Sandwich-LN kernels (cogview_amd/csrc/layernorm.hip) on every cell of tests/layernorm_cells.py -- the smallest shapes
that reach each path (tests/test_layernorm_cells_cpu.py proves that on the CPU), every forward instantiation (NV 1..8 x 3 stream
modes), all twelve forms of ln_bwd_kernel, the pair kernel and the reduce kernel, operands inside guarded allocations, the backward
with statistics that do not come from the GPU forward.  `randn` and `lowvar` cells are judged element by element against fp64 (mean
and rstd included, absmax_out exactly), `exact` cells to the bit; sentinels around every output and the workspace intact and a
second call bit-equal.  Beside the sweeps: the refusals through the launching entry points.

Worst err / bound as measured: MEASURED in tests/layernorm_cells.py."""
import pytest
import torch

from tests import layernorm_cells as LC

pytestmark = pytest.mark.gpu

DT_IDS = [LC.DT_NAME[d] for d in LC.DTYPES]


def params(forms):
    p = [(form, dtype) for form in forms for dtype in LC.DTYPES]
    return dict(argnames="form,dtype", argvalues=p, ids=[f"{form}-{LC.DT_NAME[dtype]}" for form, dtype in p])


@pytest.fixture(scope="module")
def backend():
    assert torch.cuda.is_available(), "GPU tests need an MI355X; run with -m 'not gpu' elsewhere"
    from cogview_amd import ops
    return LC.Launched(ops)


def report(tag, fails, cells, worst):
    print(f"{tag}: {cells} cells, {len(fails)} failures")
    for name, r in sorted(worst.items()):
        print(f"RATIO {tag} {name}: worst err / bound = {r:.4f}")


@pytest.mark.parametrize(**params(LC.FWD_FORMS))
def test_forward_cells(backend, form, dtype):
    """every shape of the forward grid (randn) and the lowvar cells in one stream mode and dtype: y, mean, rstd, absmax_out"""
    fails, cells, worst = LC.fwd_sweep(backend, form, dtype)
    report(f"{form} {LC.DT_NAME[dtype]}", fails, cells, worst)
    assert not fails, "\n".join(fails[:40])
    assert cells == len(LC.fwd_cells(form)) >= 10 and set(LC.FWD_OUTPUTS) <= set(worst) and "y / lowvar" in worst


@pytest.mark.parametrize(**params(LC.BWD_FORMS))
def test_backward_cells(backend, form, dtype, monkeypatch):
    """every shape x (exact, randn) of one backward form under its per-launch switches: dx, dgamma, dbeta, colsum"""
    LC.with_switches(monkeypatch, LC.BWD_FORMS[form][4])
    fails, cells, worst = LC.bwd_sweep(backend, form, dtype)
    report(f"{form} {LC.DT_NAME[dtype]}", fails, cells, worst)
    assert not fails, "\n".join(fails[:40])
    assert cells == len(LC.BWD_SHAPES) * 2 and set(LC.BWD_OUTPUTS) <= set(worst)


@pytest.mark.parametrize(**params(LC.PAIR_FORMS))
def test_pair_cells(backend, form, dtype):
    """LN2' + LN3' in one pass: dy (fp32), d_ao and the five column reductions against fp64 and, in the exact kind, to the bit"""
    fails, cells, worst = LC.pair_sweep(backend, form, dtype)
    report(f"{form} {LC.DT_NAME[dtype]}", fails, cells, worst)
    assert not fails, "\n".join(fails[:40])
    assert cells == len(LC.PAIR_SHAPES) * 2 and set(LC.PAIR_OUTPUTS) <= set(worst)


@pytest.mark.parametrize("dtype", LC.DTYPES, ids=DT_IDS)
def test_refusals(backend, dtype):
    """the launching entry points answer the plan's code and write nothing"""
    fails, n = LC.refusal_sweep(backend, dtype)
    print(f"refusals {LC.DT_NAME[dtype]}: {n} calls, {len(fails)} failures")
    assert not fails, "\n".join(fails)
    assert n == len(LC.REFUSALS) >= 20
