"""CPU: what the Sandwich-LN cell sweep (tests/layernorm_cells.py, run on the GPU by tests/test_layernorm_cells_gpu.py) rests on.
1. every row of the shape grids reaches what its comment names (cogv_ln_bwd_plan, cogv_ln_bwd_pair_plan and the grid arithmetic
   restated in Python): all 8 NV values, all twelve LN_FORM instantiations per dtype, both loop depths, the reduce kernel's unrolled
   path and its tail; 2. the fp64 references are the oracle's; 3. the preconditions of the lowvar and of the exact cells; 4. the
   checks check: an fp32 emulation of the kernels' arithmetic passes them on the whole grid with every ratio below 1, and each
   seeded mutant of it is rejected on the shape named for it."""
import pytest
import torch

from cogview_amd import _lib
from oracle import cogview_oracle as O
from tests import layernorm_cells as LC

DTYPES = LC.DTYPES
IDS = [LC.DT_NAME[d] for d in DTYPES]


# ---------------------------------------------------------------------------------------------------------------- 1. the grids
@pytest.mark.parametrize("shape,want", LC.FWD_GRID, ids=[str(s) for s in LC.FWD_SHAPES])
def test_forward_grid_row_reaches_what_it_names(shape, want):
    assert LC.fwd_geometry(*shape) == want


def test_forward_grid_covers_every_instantiation_and_both_loop_depths():
    assert {LC.fwd_geometry(*s)[0] for s in LC.FWD_SHAPES} == set(range(1, 9))
    assert {m for m, _ in LC.FWD_FORMS.values()} == {LC.ALL_T, LC.IN, LC.OUT}
    assert [LC.fwd_geometry(*s)[3] for s in LC.FWD_SHAPES].count(True) == 1
    # the grid cap is min(4096, resident workgroups): at most 4 x 4096 waves, whatever the occupancy query answers
    assert 16389 > LC.FWD_MAX_WAVES == 16384
    # partial last vectors: one lane, 63 lanes; full ones
    assert {LC.fwd_geometry(*s)[1] for s in LC.FWD_SHAPES} >= {1, 63, 64}
    # absmax_out and save_stats both ways, and the all-T form with and without a residual
    cells = [LC.fwd_problem("F_T", s, "randn", torch.float16) for s in LC.FWD_SHAPES]
    assert {c.save_stats for c in cells} == {c.want_absmax for c in cells} == {True, False}
    assert cells[-1].save_stats and cells[-1].want_absmax
    assert (LC.FWD_FORMS["F_T"], LC.FWD_FORMS["F_T_RES"]) == ((LC.ALL_T, False), (LC.ALL_T, True))
    assert sum(not absmax for f in LC.FWD_FORMS for _, _, absmax in LC.fwd_cells(f)) == 1


@pytest.mark.parametrize("shape,want", LC.BWD_GRID, ids=[str(s) for s in LC.BWD_SHAPES])
def test_backward_grid_row_reaches_what_it_names(shape, want, monkeypatch):
    rows, h = shape
    nw, wide = want
    assert ((h + 511) // 512, (h + 511) // 512 >= 4) == want
    for form, (mode, drop, marked, add, env) in LC.BWD_FORMS.items():
        LC.with_switches(monkeypatch, env)
        rc, (R, lean, mark, blocks, threads) = LC.bwd_plan(mode, rows, h, 0.5 if drop else 0.0, marked, add)
        assert rc == _lib.OK and threads == 64 * nw and mark == marked and (mode, R, lean, mark) in LC.LN_FORMS
        assert blocks <= _lib.lib().cogv_ln_bwd_num_blocks(rows) and blocks * 3 * h * 4 <= _lib.lib().cogv_ln_bwd_workspace_bytes(rows, h)
        if not wide:
            assert (R, lean) == (4, 0)
        n = LC.passes(rows, R, blocks)
        if shape == (4101, 64):          # 1024 workgroups at the workspace bound; a second pass of 5 rows: workgroup 0 a full group of
            assert (blocks, n) == (1024, 2) and rows - 4 * blocks == 5      # four, workgroup 1 one row and three past the end
        elif shape == (1029, 1544):      # every form loops; the reduce runs its unrolled path (b + 7 * 16 < nblk) and its tail
            assert n >= 2 and blocks in (256, 258) and blocks > 7 * 16 + 15
            if R == 4:
                assert (blocks, n) == (256, 2) and rows - 4 * blocks == 5
            if blocks == 258:
                assert blocks % 128 == 2                                    # two of the sixteen slices run the reduce's tail loop
        else:
            assert blocks == (rows + 3) // 4 and n == (1 if R == 4 or rows <= 2 * blocks else 2)   # a two-row form: a workgroup per 4 rows
        if shape == (7, 1544):
            assert rows % R != 0                                            # a row tail in the only pass


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_backward_grid_plans_all_twelve_forms(dtype, monkeypatch):
    seen = {}
    for form, (mode, drop, marked, add, env) in LC.BWD_FORMS.items():
        LC.with_switches(monkeypatch, env)
        for shape in LC.BWD_SHAPES:
            for p in (LC.P_EXACT, LC.P_RANDN) if drop else (0.0,):
                rc, plan = LC.bwd_plan(mode, shape[0], shape[1], p, marked, add)
                assert rc == _lib.OK
                seen.setdefault((mode, *plan[:3]), set()).add((shape, LC.passes(shape[0], plan[0], plan[3])))
    assert LC.bwd_problem("OUT_LEAN", (1, 8), "randn", dtype).p == LC.P_RANDN and LC.bwd_problem("OUT_LEAN", (1, 8), "exact", dtype).p == LC.P_EXACT
    assert set(seen) == LC.LN_FORMS and len(LC.LN_FORMS) == 12
    # every instantiation loops somewhere (prefetch of a later group, the other half of the LDS double buffer); the four-row forms
    # make a single pass somewhere too (the two-row forms get a workgroup per FOUR rows: one pass only up to two rows)
    for f, where in seen.items():
        assert {min(n, 2) for _, n in where} == ({1, 2} if f[1] == 4 else {2}), f
    # both per-launch switches are flipped by some form, the once-per-process ones by none
    used = set().union(*[set(v[4]) for v in LC.BWD_FORMS.values()])
    assert used == set(LC.SWITCHES) and not used & {"COGV_LN_BWD_ROWS", "COGV_LN_BWD_PAIR_BLOCKS"}
    # `accumulate` both ways and each output pointer NULL, on every form
    for form in LC.BWD_FORMS:
        v = {LC.bwd_variant(form, s, k) for s in LC.BWD_SHAPES for k in LC.BWD_KINDS}
        assert {a for a, _ in v} == {0, 1} and {n for _, n in v} == {None, "dgamma", "dbeta", "colsum"}, form


def test_pair_grid():
    for rows, h in LC.PAIR_SHAPES:
        for p in (0.0, 0.5):
            rc, (R, lean, mark, blocks, threads) = LC.pair_plan(rows, h, p)
            assert rc == _lib.OK and (R, lean, mark, threads) == (2, 0, int(p > 0), 64 * ((h + 511) // 512))
            assert 2 * blocks * 3 * h * 4 <= _lib.lib().cogv_ln_bwd_pair_workspace_bytes(rows, h)
            assert blocks == min((rows + 3) // 4, 512) and LC.passes(rows, R, blocks) == (2 if rows > 2 else 1)    # a workgroup per 4 rows
    assert LC.pair_plan(1029, 1544, 0.5)[1][3] == 258
    assert {c.accumulate for c in (LC.pair_problem("PAIR", s, k, torch.float16) for s in LC.PAIR_SHAPES for k in LC.BWD_KINDS)} == {0, 1}


def test_factors_and_bookkeeping():
    assert all(1.0 <= f <= 2.0 for f in LC.FACTOR.values())
    assert set(LC.MEASURED) <= set(LC.FACTOR) and all(r <= 1.0 for r in LC.MEASURED.values())
    for name, (entry, form, shape, kind) in LC.MUTANTS.items():
        assert shape in {"fwd": LC.FWD_SHAPES + (LC.LOWVAR_SHAPE,), "bwd": LC.BWD_SHAPES, "pair": LC.PAIR_SHAPES}[entry], name
    for name in ("accumulate ignored", "accumulate applied twice"):
        assert LC.mutant_cell(name, torch.float16)[1].accumulate == 1
    assert LC.mutant_cell("colsum of the unrounded values", torch.float16)[1].null != "colsum"
    # every tensor of the sweep is under 7 MB
    assert max(r * h * 4 for r, h in LC.FWD_SHAPES + LC.BWD_SHAPES + LC.PAIR_SHAPES) < 7e6


# ---------------------------------------------------------------------------------------------------------------- 2. reference pins
@pytest.mark.parametrize("form,shape", [("T", (7, 1544)), ("T_DROP_ADD", (5, 520)), ("IN_ADD", (6, 2560)), ("OUT_LEAN", (7, 1544))])
def test_backward_reference_is_the_oracles(form, shape):
    """LN' of the cells module against autograd through the oracle's Sandwich-LN in fp64 (the saved statistics: the oracle's own)"""
    c = LC.bwd_problem(form, shape, "randn", torch.float16)
    x = c.x.clone().requires_grad_(True)
    g = c.gamma.clone().requires_grad_(True)
    b = torch.zeros(c.h, dtype=torch.float64, requires_grad=True)
    mean, rstd, _ = LC.oracle_stats(c.x)
    exact = LC.SimpleNamespace(**{**vars(c), "mean": mean, "rstd": rstd, "add": None, "keep": None, "init": None})
    ref, _ = LC.bwd_reference(exact)
    cc = c.x.abs().max() / 8                                             # detached, as in the reference
    y = torch.nn.functional.layer_norm(x / cc, (c.h,), g, b, LC.EPS)
    y.backward(c.dy)
    # the kernel's dx is the gradient with the scalar c held fixed
    for name, a, want in (("dx", ref["dx"], x.grad), ("dgamma", ref["dgamma"], g.grad), ("dbeta", ref["dbeta"], b.grad)):
        assert float((a - want).abs().max()) <= 1e-11 * max(1.0, float(want.abs().max())), name
    # dropout and add_in: dx_out = add_in + keep scale LN'(dy); the statistics as rounded to fp32 move dx by less than 1e-6
    full, _ = LC.bwd_reference(c)
    keep = torch.from_numpy(O.dropout_keep_mask(c.rows * c.h, c.p, LC.SEED, LC.STREAM)).view(c.rows, c.h).double() if c.p else 1.0
    want = x.grad * keep + (c.add if c.add is not None else 0.0)
    assert float((full["dx"] - want).abs().max()) <= 1e-5 * float(want.abs().max())


@pytest.mark.parametrize("form", tuple(LC.FWD_FORMS))
def test_forward_reference_is_the_oracles(form):
    c = LC.fwd_problem(form, (5, 520), "randn", torch.bfloat16)
    ref, bound, var, eps_eff = LC.fwd_reference(c)
    want = O.sandwich_layernorm(c.x, c.gamma, c.beta, LC.EPS) + (c.res if c.res is not None else 0.0)
    assert torch.equal(ref["y"], want)
    # mean and rstd in the units of the undivided x reproduce the oracle's output
    again = (c.x - ref["mean"][:, None]) * ref["rstd"][:, None] * c.gamma + c.beta + (c.res if c.res is not None else 0.0)
    assert float((again - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert all(bool((b > 0).all()) for b in bound.values())


# ---------------------------------------------------------------------------------------------------------------- 3. preconditions
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_lowvar_preconditions(dtype):
    """the epsilon fold decides y: the judged rows' variance is below eps c^2, and each wrong fold moves y by more than 100 x the bound"""
    for form in LC.FWD_FORMS:
        c = LC.fwd_problem(form, LC.LOWVAR_SHAPE, "lowvar", dtype)
        ref, bound, var, eps_eff = LC.fwd_reference(c)
        cc = float(c.x.abs().max()) / 8
        assert cc == 10.0 and abs(float(eps_eff) - 1e-3) < 1e-12
        assert float(var[:-1].max()) < float(eps_eff) and float(var[:-1].min()) > 0.02 * float(eps_eff)
        for fold in ("none", "c", "absmax^2", "1/c^2"):
            wrong, _, _, _ = LC.fwd_reference(c, fold)
            moved = ((wrong["y"] - ref["y"]).abs() / bound["y"])[:-1]
            assert float(moved.max()) > 100.0, (form, fold, float(moved.max()))
            assert float(((wrong["rstd"] - ref["rstd"]).abs() / bound["rstd"])[:-1].min()) > 100.0
    plain = LC.fwd_problem("F_T", LC.LOWVAR_SHAPE, "lowvar", dtype, False)
    assert plain.absmax is None and torch.equal(plain.x, LC.fwd_problem("F_T", LC.LOWVAR_SHAPE, "lowvar", dtype).x)


def _distinct(t, h):
    """no two rows and no two 8-column groups of t hold the same values"""
    rows = t.shape[0]
    groups = t.view(rows, h // 8, 8).transpose(0, 1).reshape(h // 8, -1)
    return torch.unique(t, dim=0).shape[0] == rows and torch.unique(groups, dim=0).shape[0] == h // 8


def _exact_stage(c, limit):
    """the preconditions of one exact LN' cell"""
    rows, h = c.rows, c.h
    isint = lambda t: bool((t == t.round()).all())
    assert isint(c.mean) and isint(c.dy) and (c.add is None or isint(c.add)) and isint(c.xh)
    assert set(c.rstd.tolist()) <= {0.5, 1.0, 2.0} and set(c.gamma.abs().tolist()) <= {0.5, 1.0, 2.0}
    assert float(c.dy.abs().min()) >= 1 and float(c.xh.abs().min()) >= 1 and float(c.xh.abs().max()) <= 8
    # x = mean + x-hat / rstd, and the kernel's fused multiply-add gives x-hat back exactly
    assert torch.equal(c.x * c.rstd[:, None] - (c.mean * c.rstd)[:, None], c.xh)
    assert torch.equal(c.x.to(c.dtype).double(), c.x) and torch.equal(c.dy.to(c.dtype).double(), c.dy)
    gy = c.dy * c.gamma
    assert isint(gy) and bool((gy.view(rows, -1, 2).sum(-1) == 0).all()) and bool(((gy * c.xh).view(rows, -1, 2).sum(-1) == 0).all())
    if h % 4 == 0:                                                       # groups of four: two pairs
        assert bool((gy.view(rows, -1, 4).sum(-1) == 0).all())
    assert float(gy.abs().sum(1).max()) * 8 < 2 ** 24                    # every fp32 partial sum of a row is an exact integer
    dx, sums = LC.exact_expected(c)
    assert torch.equal(dx.to(c.dtype).double(), dx) and float(dx.abs().max()) <= limit
    raw = [(c.dy * c.xh), c.dy, dx]
    for s, t, i in zip(sums, raw, c.init or [None] * 3):
        assert isint(s) and float(s.abs().max()) <= limit, float(s.abs().max())       # the final sum, with the initial value
        assert float(t.sum(0).abs().max()) <= limit and float(t.abs().sum(0).max()) < 2 ** 24          # every partial sum
        assert i is None or (isint(i) and float(i.abs().max()) <= 8)
    if c.keep is not None:
        assert c.p == 0.5 and LC.keep_scale(c.p) == 2.0
        if rows * h >= 64:
            assert bool(c.keep.any()) and not bool(c.keep.all())
    return dx


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("form", tuple(LC.BWD_FORMS))
def test_exact_preconditions(form, dtype):
    limit = LC.EXACT_MAX[dtype]
    mode, drop, marked, add, _ = LC.BWD_FORMS[form]
    for shape in LC.BWD_SHAPES:
        c = LC.bwd_problem(form, shape, "exact", dtype)
        dx = _exact_stage(c, limit)
        rows, h = shape
        if rows * h >= 4096:
            # swapping two rows or two 8-column groups changes the expected bits; a lost workgroup changes the column sums
            assert _distinct(dx, h)
        if marked and rows * h >= 2048:
            bits = LC.BwdStaged(c, "cpu").x.bits
            dropped, zero = bits == -32768, bits == 0
            assert torch.equal(dropped, ~c.keep) and bool((zero & c.keep).any())             # kept elements equal to +0.0
            assert bool(dropped[:, 0::2].any()) and bool(dropped[:, 1::2].any())             # both halves of a 32-bit word
            assert bool((dropped[:, 0::2] & ~dropped[:, 1::2]).any()) and bool((~dropped[:, 0::2] & dropped[:, 1::2]).any())
    if marked:
        c = LC.bwd_problem(form, (1029, 1544), "randn", dtype)
        bits = LC.BwdStaged(c, "cpu").x.bits
        assert torch.equal(bits == -32768, ~c.keep) and bool(((bits == 0) & c.keep).any()) and c.p == LC.P_RANDN


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_pair_exact_preconditions(dtype):
    for form in LC.PAIR_FORMS:
        for shape in LC.PAIR_SHAPES:
            c = LC.pair_problem(form, shape, "exact", dtype)
            s2, s3 = LC.pair_stages(c, c.dy_want)
            s2.xh, s3.xh = c.xh2, c.xh3
            assert torch.equal(_exact_stage(s2, 2 ** 20), c.dy_want)       # dy is an fp32 output: any integer below 2^24
            _exact_stage(s3, LC.EXACT_MAX[dtype])
            assert torch.equal(c.dout.float().double(), c.dout)


# ---------------------------------------------------------------------------------------------------------------- 4. the checker checks
def report(tag, worst):
    for name, r in sorted(worst.items()):
        print(f"RATIO emulation {tag} {name}: worst err / bound = {r:.4f}")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("form", tuple(LC.FWD_FORMS))
def test_emulation_passes_the_forward_checks(form, dtype):
    fails, cells, worst = LC.fwd_sweep(LC.Emulated(), form, dtype)
    report(f"{form} {LC.DT_NAME[dtype]}", worst)
    assert not fails, "\n".join(fails[:20])
    assert cells == len(LC.FWD_SHAPES) + 1 + (form == "F_T") and set(LC.FWD_OUTPUTS) <= set(worst)
    assert all(r < 1.0 for r in worst.values()), worst


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("form", tuple(LC.BWD_FORMS))
def test_emulation_passes_the_backward_checks(form, dtype, monkeypatch):
    LC.with_switches(monkeypatch, LC.BWD_FORMS[form][4])
    fails, cells, worst = LC.bwd_sweep(LC.Emulated(), form, dtype)
    report(f"{form} {LC.DT_NAME[dtype]}", worst)
    assert not fails, "\n".join(fails[:20])
    assert cells == 14 and set(LC.BWD_OUTPUTS) <= set(worst)
    assert all(r < 1.0 for r in worst.values()), worst


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("form", tuple(LC.PAIR_FORMS))
def test_emulation_passes_the_pair_checks(form, dtype):
    fails, cells, worst = LC.pair_sweep(LC.Emulated(), form, dtype)
    report(f"{form} {LC.DT_NAME[dtype]}", worst)
    assert not fails, "\n".join(fails[:20])
    assert cells == 8 and set(LC.PAIR_OUTPUTS) <= set(worst)
    assert all(r < 1.0 for r in worst.values()), worst


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("mutant", tuple(LC.MUTANTS))
def test_mutant_is_rejected(mutant, dtype, monkeypatch):
    entry, c = LC.mutant_cell(mutant, dtype)
    if entry == "bwd":
        LC.with_switches(monkeypatch, c.env)
    run = {"fwd": LC.run_fwd, "bwd": LC.run_bwd, "pair": LC.run_pair}[entry]
    fails, _ = run(LC.Emulated(mutant), c)
    assert fails, mutant
    clean, _ = run(LC.Emulated(), c)
    assert not clean, clean
    print(f"{mutant} on {c.form} {LC.DT_NAME[dtype]} {c.shape} {c.kind}: " + "; ".join(fails[:3]))


def test_refusal_descriptors_are_refused_by_the_plan():
    """the plan's code for every shape or dropout argument the GPU test hands to the launching entry points"""
    class PlanOnly:
        device = "cpu"

        def _code(self, entry, S, kw):
            a = S.args(**kw)
            if any(k not in ("h", "rows", "p", "marked", "mode") for k in kw) or entry == "fwd":
                return _lib.ERR_ARG                                         # pointers, the workspace, the forward: no plan query
            if entry == "bwd":
                return LC.bwd_plan(a["mode"], a["rows"], a["h"], a["p"], a["marked"], 0)[0]
            return LC.pair_plan(a["rows"], a["h"], a["p"])[0]

        def fwd(self, S, **kw):
            return self._code("fwd", S, kw)

        def bwd(self, S, **kw):
            return self._code("bwd", S, kw)

        def pair(self, S, **kw):
            return self._code("pair", S, kw)
    fails, n = LC.refusal_sweep(PlanOnly(), torch.float16)
    assert not fails and n == len(LC.REFUSALS) >= 20, fails
    planned = [(e, kw) for e, kw, _ in LC.REFUSALS if e != "fwd" and all(k in ("h", "rows", "p", "marked", "mode") for k in kw)]
    assert len(planned) >= 12
