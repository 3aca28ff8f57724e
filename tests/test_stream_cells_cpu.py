"""CPU: what the cell sweep of the trainer's memory-bound kernels (tests/stream_cells.py, run on the GPU by
tests/test_stream_cells_gpu.py) rests on.
1. every row of the grids reaches what its comment names (the launch arithmetic of cogview_amd/csrc/elementwise.hip and ce_optim.hip
   restated in Python, the workspace queries of the real library); 2. the preconditions of the bitwise and of the `exact` cells;
3. the fp64 references are the oracle's; 4. the checks check: the stand-ins of tests/cpu_ops.py pass the whole sweep with every ratio
   below 1 and each seeded mutant is rejected on the cell named for it; 5. every argument check of these entry points refuses with the
   code the source gives -- against the real library, with aligned dummy pointers that nothing reads, before any launch."""
import math

import pytest
import torch

from cogview_amd import _lib
from oracle import cogview_oracle as O
from tests import stream_cells as SC

DTYPES = SC.DTYPES
IDS = [SC.NAME[d] for d in DTYPES]
IDS3 = [SC.NAME[d] for d in SC.CE_DTYPES]


# ---------------------------------------------------------------------------------------------------------------- 1. the grids
@pytest.mark.parametrize("n,want", SC.FLAT_GRID + SC.TAIL_GRID, ids=[str(n) for n in SC.FLAT_N + SC.TAIL_N])
def test_flat_grid_row_reaches_what_it_names(n, want):
    assert SC.flat_geometry(n) == want


def test_flat_grid_covers_the_cap_the_lanes_and_the_tails():
    geo = [SC.flat_geometry(n) for n in SC.FLAT_N]
    assert {g[1] for g in geo} == {1, 2} and max(g[0] for g in geo) == 2048         # one pass and the capped grid's second pass
    assert {g[2] for g in geo} >= {1, 255, 256} and all(g[3] == 0 for g in geo)     # every flat entry point refuses n % 8
    assert SC.BIG - 2048 * 256 * 8 == 264 * 8                                       # second pass: workgroup 0 full, workgroup 1 with 8 lanes
    tails = [SC.flat_geometry(n) for n in SC.TAIL_N]
    assert [g[1] > 0 for g in tails] == [False, True, True] and all(g[3] for g in tails) and tails[2][0] == 2048
    # the fp32 absmax takes 4 elements per lane: the same sizes loop too, and its own two sizes are one lane and a second workgroup
    assert SC.flat_geometry(SC.BIG, 4)[:2] == (2048, 3) and SC.flat_geometry(4, 4) == (1, 1, 1, 0) and SC.flat_geometry(2052, 4) == (3, 1, 1, 0)
    assert all(n % 4 == 0 for n in SC.ABSMAX32_N)
    # absmax: every placement on every size that has the place
    for n in SC.FLAT_N + SC.TAIL_N:
        names = [c[0] for c in SC.absmax_cells(n, False)]
        assert {"first", "nan", "neg"} <= set(names) and ("tail" in names) == (n % 8 != 0) and ("lastvec" in names) == (n >= 8)
        assert all(0 <= i < n for _, i, _ in SC.absmax_cells(n, False))
    assert [i for v, i, _ in SC.absmax_cells(13, False) if v in ("lastvec", "tail")] == [7, 12]
    # every op runs every size; the casts run the tails; the absmax slot is both present and NULL on the ops that have one
    for op in ("dropout", "add", "add_stream"):
        assert {SC.flat_operands(op, n, torch.float16).slot for n in SC.FLAT_N[:4]} == {True, False}
    assert set(SC.TAILED) == {"cast_flat", "cast_flat_back"} and len(SC.FLAT_OPS) == 8
    # the largest operand: 16-bit 8 MB (its fp32 counterparts of the same element count 16 MB)
    assert SC.BIG_TAIL * 2 < 8.5e6 and SC.BIG * 2 < 8.5e6


@pytest.mark.parametrize("shape,want", SC.EMB_FWD_GRID, ids=[str(s) for s in SC.EMB_FWD_SHAPES])
def test_embedding_forward_grid_row_reaches_what_it_names(shape, want):
    assert SC.emb_fwd_geometry(*shape) == want


def test_embedding_forward_cells_cover_every_factor_and_every_pair():
    cells = SC.EMB_FWD_CELLS
    for f in range(5):
        assert {bool(c[f]) for c in cells} == {True, False}
        assert {bool(c[f]) for c in SC.EMB_FWD_BIG_CELLS} == {True, False}
    assert {(bool(c[0]), c[2], c[3]) for c in cells} == {(a, b, c) for a in (False, True) for b in (False, True) for c in (False, True)}
    assert SC.emb_fwd_geometry(4099, 1032)[1] == 2 and len(SC.emb_fwd_cells()) == 27
    # the ids on both edges of the shard and one outside on either side, the position ids -1 and n_pos: on every shape with four tokens,
    # and over the smaller shapes together
    seen_ids, seen_pos = set(), set()
    for shape in SC.EMB_FWD_SHAPES:
        c = SC.emb_fwd_problem(shape, (0, True, True, False, True), torch.float16)
        ids, pos = set(c.ids.tolist()), set(c.pos_ids.tolist())
        if shape[0] >= 4:
            assert set(SC.EDGE_IDS) <= ids and {-1, SC.EMB_NPOS} <= pos
        seen_ids |= ids
        seen_pos |= pos
    assert set(SC.EDGE_IDS) <= seen_ids and {-1, SC.EMB_NPOS} <= seen_pos
    assert SC.EDGE_IDS == (SC.EMB_START - 1, SC.EMB_START, SC.EMB_START + SC.EMB_ROWS - 1, SC.EMB_START + SC.EMB_ROWS)


@pytest.mark.parametrize("shape,want", SC.EMB_BWD_GRID, ids=[str(s) for s in SC.EMB_BWD_SHAPES])
def test_embedding_backward_grid_row_reaches_what_it_names(shape, want):
    assert SC.emb_bwd_geometry(*shape) == want
    cells = SC.emb_bwd_cells(shape)
    assert {(p, k, d) for p, k, d, _, _ in cells} == {(p, k, d) for p in SC.EMB_PATTERNS for k in SC.KINDS for d in (0, 1)}
    assert {w for _, _, _, w, _ in cells} == set(SC.EMB_WHICH) and {dr for *_, dr in cells} == {True, False}
    assert {(d, w) for _, _, d, w, _ in cells} >= {(d, w) for d in (0, 1) for w in ("dtable", "both")}
    assert all(w != "dpos" for p, _, _, w, _ in cells if p == "outside")


def test_embedding_backward_key_patterns():
    g = SC._gen(1)
    n_tok, rows = 600, 605
    keys = SC.emb_keys("window", n_tok, rows, g)
    shared = [t for t in range(n_tok) if keys[t] == keys[0]]
    assert tuple(shared) == SC.WINDOW_TOKENS
    # the first token's workgroup scans [1, 257), [257, 513), [513, 769): occurrences on both sides of the first window's end, one in the last
    assert SC.scan_windows(shared, n_tok) == [[255, 256], [257], [599]]
    assert len(set(SC.emb_keys("unique", n_tok, rows, g).tolist())) == n_tok
    assert len(SC.scan_windows(list(range(n_tok)), n_tok)) == 3 and set(SC.emb_keys("every", n_tok, rows, g).tolist()) == {3}
    assert set(SC.emb_keys("outside", n_tok, rows, g).tolist()) == {-1, rows}
    c = SC.emb_bwd_problem((300, 520), "outside", "exact", 0, "both", False, torch.float16)
    assert float(c.count["dtable"].sum()) == 0 and set(c.ids.tolist()) == {SC.EMB_START - 1, SC.EMB_START + c.rows}
    assert c.count["dpos"][0] == 150 and c.count["dpos"][-1] == 150         # the position ids -1 and n_pos, clamped


@pytest.mark.parametrize("shape,want", SC.COLSUM_GRID, ids=[str(s) for s in SC.COLSUM_SHAPES])
def test_column_sum_grid_row_reaches_what_it_names(shape, want):
    M, N, ld = shape
    assert SC.colsum_geometry(M, N, ld) == want
    nslab, rows_per, first = SC.colsum_plan(M)
    # the workspace query sizes the partials by the first estimate; the recomputed slab count never exceeds it
    assert _lib.lib().cogv_colsum_workspace_bytes(M, N) == first * N * 4 and nslab <= first and (nslab - 1) * rows_per < M <= nslab * rows_per


def test_column_sum_grid_covers_the_slabs_and_both_loops():
    geo = {s: SC.colsum_geometry(*s) for s in SC.COLSUM_SHAPES}
    assert geo[(257, 136, 136)][1:3] == (2, 129) and geo[(9472, 8, 8)][1] == 37 and geo[(16400, 8, 8)][1:3] == (64, 257)
    assert 16400 / 64 > 256                                                  # rows_per rounds up past 256 under the 64-slab cap
    assert any(s[2] > s[1] for s in SC.COLSUM_SHAPES) and any(s[1] % 64 for s in SC.COLSUM_SHAPES) and any(s[1] % 512 == 8 for s in SC.COLSUM_SHAPES)
    # colsum_final_kernel through cogv_colsum: the unrolled loop together with its tail (37 slabs), the unrolled loop twice (64)
    assert [SC.final_iterations(37, p) for p in range(4)] == [(1, 2), (1, 1), (1, 1), (1, 1)]
    assert [SC.final_iterations(64, p) for p in range(4)] == [(2, 0)] * 4
    # called directly: no unrolled iteration (1 .. 5 rows: some slices idle), the unrolled loop in slice 0 only (29), in all four with a
    # tail in slice 0 (33), twice (64), three times with a tail in every slice (100)
    it = {r: [SC.final_iterations(r, p) for p in range(4)] for r in SC.FINALIZE_ROWS}
    assert it[1] == [(0, 1), (0, 0), (0, 0), (0, 0)] and it[5] == [(0, 2), (0, 1), (0, 1), (0, 1)]
    assert it[29] == [(1, 0), (0, 7), (0, 7), (0, 7)] and it[33] == [(1, 1), (1, 0), (1, 0), (1, 0)]
    assert it[64] == [(2, 0)] * 4 and it[100] == [(3, 1)] * 4
    assert SC.FINALIZE_N == (8, 72) and {SC.finalize_problem(r, n, "randn", torch.float16).accumulate for r in SC.FINALIZE_ROWS for n in SC.FINALIZE_N} == {0, 1}


@pytest.mark.parametrize("shape,want", SC.CE_GRID, ids=[str(s) for s in SC.CE_SHAPES])
def test_cross_entropy_grid_row_reaches_what_it_names(shape, want):
    assert SC.ce_geometry(shape[1]) == want


def test_cross_entropy_cells():
    # thread 0 owns vectors 0 and 256 from v_local = 2056 on: columns 0..7 and 2048..2055
    assert [i for i in range(SC.ce_geometry(2056)[0]) if i % 256 == 0] == [0, 256] and SC.ce_geometry(2048)[2] == 1
    assert SC.NEGINF_SHAPE == (1, 2056)
    l = SC.ce_logits(SC.NEGINF_SHAPE, "neginf", torch.float16)
    t = SC.ce_targets(SC.NEGINF_SHAPE, "neginf") - SC.VOCAB_START
    assert bool(torch.isinf(l[:, :8]).all()) and bool(torch.isfinite(l[:, 8:]).all()) and int(t[0]) >= 8
    ref, bound = SC.ce_reference(l, t + SC.VOCAB_START, SC.VOCAB_START)
    assert all(bool(torch.isfinite(v).all()) for v in list(ref.values()) + list(bound.values()))
    assert SC.VOCAB_START == 29184
    for shape in SC.CE_SHAPES:
        v = shape[1]
        got = {tag: set((SC.ce_targets(shape, tag) - SC.VOCAB_START).tolist()) for tag in SC.CE_TARGETS}
        assert got == {"first": {0}, "last": {v - 1}, "below": {-1}, "above": {v}}
        assert all((s, tag) in SC.ce_cells() for s in [shape] for tag in SC.CE_TARGETS)
    tags = [t for _, t in SC.ce_cells()]
    assert {"noloss", "maxlast", "equal", "neginf"} <= set(tags)
    l = SC.ce_logits((2, 4104), "maxlast", torch.bfloat16)
    assert bool((l.argmax(1) == 4103).all()) and len(set(SC.ce_logits((3, 2056), "equal", torch.float16).flatten().tolist())) == 1


def test_chunk_tables():
    starts, lens, groups, counted, total = SC.chunk_table("lens")
    assert tuple(lens.tolist()) == SC.TABLE_LENS == (1, 7, 8, 9, 2047, 2048, 2056, 32768)
    for name, cap, want in (("lens", 2048, (8, 1)), ("stats", 2048, (2048, 2)), ("adam", 4096, (4096, 2))):
        s, n, g, c, tot = SC.chunk_table(name)
        assert SC.chunk_passes(len(n), cap) == want
        assert bool((s % 8 == 0).all()) and bool((s[1:] >= s[:-1] + n[:-1]).all()) and int(s[-1] + n[-1]) <= tot
        assert set(g.tolist()) == {0, 7} and c.tolist().count(0) == 1
        assert not bool(SC.chunk_mask(SC.chunk_table(name)).all())              # gaps that belong to no chunk
    assert len(SC.chunk_table("stats")[1]) == 2051 and len(SC.chunk_table("adam")[1]) == 4100
    assert int(SC.chunk_table("adam")[1].min()) >= 8 and int(SC.chunk_table("adam")[1].max()) <= 40
    # AdamW's cells: both decay modes, clipping inactive and active, no bias correction, the override, a loss scale; steps 1 and 2
    cells = SC.adam_cells()
    assert {c for c, *_ in cells} == set(SC.ADAM_CELLS) == {"plain", "clip_inactive", "clip", "l2", "nobc", "override", "scaled"}
    assert {(c, s) for c, s, t, p in cells if t == "lens" and not p} == {(c, s) for c in SC.ADAM_CELLS for s in (1, 2)}
    assert any(t == "adam" for _, _, t, _ in cells) and [p for *_, p in cells if p] == list(SC.OVERFLOWS) and SC.WD == {0: 0.0, 7: 0.1}
    for name, o in ((n, SC.adam_args(n, 1, "lens", torch.float16)) for n in SC.ADAM_CELLS):
        coef = o["max_grad_norm"] / (math.sqrt(o["sumsq"]) * o["inv_loss_scale"] + 1e-6) if o["max_grad_norm"] else None
        assert (coef is None) == (name in ("plain", "l2", "nobc")) and (coef is None or (coef < 1) == (name != "clip_inactive")), name
    assert SC.adam_args("scaled", 1, "lens", torch.float16)["inv_loss_scale"] == 1 / 64
    # the overflow cells poison a scalar tail
    assert [(SC.TABLE_LENS[c] % 8, v == v) for c, v in SC.OVERFLOWS] == [(1, True), (7, False)]


def test_factors_and_bookkeeping():
    assert all(1.0 <= f <= 2.0 for f in SC.FACTOR.values()) and set(SC.FACTOR) == set(SC.BOUNDED)
    assert set(SC.MEASURED) <= set(SC.FACTOR) and all(r <= 1.0 for r in SC.MEASURED.values())
    assert len(SC.MUTANTS) >= 12


# ---------------------------------------------------------------------------------------------------------------- 2. preconditions
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_bitwise_cells_are_exact_in_fp32(dtype):
    """the single fp32 operation of each bitwise kernel is exact on its operands, so the output is the fp64 result rounded once"""
    assert SC.keep_scale(0.5) == 2.0
    for s in SC.SCALES:
        m, _ = math.frexp(s)
        assert (m * 256).is_integer()                                        # at most 8 significant bits
    for op in ("dropout", "add", "scale", "add_stream", "cast_flat", "cast_flat_back"):
        for n in SC.FLAT_N + (SC.TAIL_N if op in SC.TAILED else ()):
            c = SC.flat_operands(op, n, dtype)
            assert c.bitwise and all(torch.equal(t.to(dt).double(), t) for t, dt in c.ins)          # the operands as stored
            f = [t.float() for t, _ in c.ins]
            if op == "add" or op == "add_stream":
                got = f[0] + f[1]
                if op == "add":
                    _, e = torch.frexp(torch.stack([t for t, _ in c.ins]).abs())
                    assert int(e.max() - e.min()) < 13                                              # exponent spread under 13 bits
                else:                                                                               # a fixed-point grid: 18 bits below 64
                    assert all(bool((t * 2 ** 12 == (t * 2 ** 12).round()).all()) and float(t.abs().max()) <= 32 for t, _ in c.ins)
                    assert float((c.ins[0][0].to(dtype).double() != c.ins[0][0]).double().mean()) > 0.5 or n < 64   # more than T holds
            elif op == "scale":
                got = f[0] * torch.tensor(c.scale, dtype=torch.float32)
            elif op == "dropout":
                got = torch.where(SC.keep_bool(n, 0.5), f[0] * 2.0, torch.zeros_like(f[0]))
                assert n < 64 or 0.4 < float(SC.keep_bool(n, 0.5).double().mean()) < 0.6
            else:
                got = f[0]
            assert torch.equal(got.double(), c.ref) and SC.exact_in_fp32(c.ref)
            if op != "cast_flat_back" and c.out_dt != torch.float32:
                assert float(c.ref.abs().max()) < 128
    # the down cast rounds: most values are not representable in the 16-bit type
    c = SC.flat_operands("cast_flat_back", 2056, dtype)
    assert float((c.ref.to(dtype).double() != c.ref).double().mean()) > 0.9


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_embedding_forward_sums_are_exact(dtype):
    for shape, combo in SC.emb_fwd_cells():
        if shape[0] > 100 and combo != SC.EMB_FWD_BIG_CELLS[0]:
            continue
        c = SC.emb_fwd_problem(shape, combo, dtype)
        assert c.sum_exact and SC.exact_in_fp32(c.ref) and float(c.ref.abs().max()) <= 128


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_exact_cells_hold_integers_the_storage_type_holds(dtype):
    limit = SC.EXACT_MAX[dtype]
    isint = lambda t: bool((t == t.round()).all())
    for shape in SC.COLSUM_SHAPES:
        for acc in (0, 1):
            c = SC.colsum_problem(shape, "exact", acc, dtype)
            assert isint(c.x) and isint(c.ref) and float(c.ref.abs().max()) <= 10 <= limit and float(c.x.abs().sum(0).max()) < 2 ** 24
            assert float(c.x.cumsum(0).abs().max()) <= 2
    nslab, rows_per, _ = SC.colsum_plan(9472)
    x = SC.colsum_problem((9472, 8, 8), "exact", 0, dtype).x                 # a slab left out would show: no slab sums to zero in every column
    assert all(bool(x[b * rows_per:(b + 1) * rows_per].sum(0).abs().sum() > 0) for b in range(nslab))
    for rows in SC.FINALIZE_ROWS:
        c = SC.finalize_problem(rows, 72, "exact", dtype)
        assert isint(c.partial) and float(c.ref.abs().max()) <= 10
    for shape in SC.EMB_BWD_SHAPES:
        for pattern, kind, d32, which, drop in SC.emb_bwd_cells(shape):
            if kind != "exact":
                continue
            c = SC.emb_bwd_problem(shape, pattern, kind, d32, which, drop, dtype)
            assert c.p in (0.0, 0.5) and isint(c.masked) and float(c.masked.abs().max()) <= 2
            for n in ("dtable", "dpos"):
                assert isint(c.ref[n]) and float(c.ref[n].abs().max()) <= limit, (shape, pattern, n, float(c.ref[n].abs().max()))


# ---------------------------------------------------------------------------------------------------------------- 3. reference pins
def test_gelu_references_are_the_oracles():
    x = torch.linspace(-12, 12, 4001, dtype=torch.float64)
    s, ds, u2 = SC.gelu_terms(x)
    xr = x.clone().requires_grad_(True)
    O.gelu(xr).sum().backward()
    assert float((x * s - O.gelu(x)).abs().max()) < 1e-14                    # 0.5 (1 + tanh u) = sigmoid(2 u)
    assert float((s + x * s * (1 - s) * u2 - xr.grad).abs().max()) < 1e-13
    c = SC.flat_operands("gelu_fwd", 2056, torch.float16)
    assert torch.equal(c.ref, O.gelu(c.ins[0][0])) and bool((c.bound > 0).all())


@pytest.mark.parametrize("ldt", SC.CE_DTYPES, ids=IDS3)
def test_cross_entropy_reference_is_the_oracles(ldt):
    shape = (3, 2056)
    l, target = SC.ce_logits(shape, "last", ldt), SC.ce_targets(shape, "last")
    ref, bound = SC.ce_reference(l, target, SC.VOCAB_START)
    want = O.vocab_parallel_cross_entropy(l, target - SC.VOCAB_START)        # (the oracle computes in fp32)
    assert float((ref["loss"] - want.double()).abs().max()) < 2e-5
    assert all(bool((b > 0).all()) for b in bound.values())
    # two shards: rowmax, sumexp and predicted of each combine to the oracle's sharded loss and to the whole-vocabulary loss
    l2 = torch.cat((l, SC.ce_logits(shape, "first", ldt) + 1.0), 1)
    tgt = SC.VOCAB_START + torch.tensor([5, 2055, 2056 + 9])
    parts = [SC.ce_reference(l2[:, i * 2056:(i + 1) * 2056], tgt, SC.VOCAB_START + i * 2056)[0] for i in range(2)]
    gmax = torch.maximum(parts[0]["rowmax"], parts[1]["rowmax"])
    gsum = sum(p["sumexp"] * (p["rowmax"] - gmax).exp() for p in parts)
    loss = gsum.log() - (parts[0]["predicted"] + parts[1]["predicted"] - gmax)
    sharded = O.vocab_parallel_cross_entropy_sharded([l2[:, :2056], l2[:, 2056:]], tgt - SC.VOCAB_START)
    assert float((loss - sharded.double()).abs().max()) < 2e-5
    assert float((loss - SC.ce_reference(l2, tgt, SC.VOCAB_START)[0]["loss"]).abs().max()) < 1e-12
    # the backward reference is autograd of the loss
    lr = l.clone().requires_grad_(True)
    lw = lr - lr.max(1, keepdim=True).values.detach()
    grad = torch.tensor([0.0, 1.0, -0.375], dtype=torch.float64)
    ((lw.exp().sum(1).log() - lw.gather(1, (target - SC.VOCAB_START)[:, None])[:, 0]) * grad).sum().backward()
    back, _ = SC.ce_bwd_reference(l, target, SC.VOCAB_START, ref["rowmax"], ref["sumexp"], grad, ldt)
    assert float((back - lr.grad).abs().max()) < 1e-14


@pytest.mark.parametrize("step", SC.ADAM_STEPS)
def test_adamw_reference_is_the_oracles(step):
    table = SC.chunk_table("lens")
    starts, lens, groups, _, total = table
    g, mask = SC.grads_of("lens", torch.float16)
    w, m, v = SC.adam_state("lens", step, torch.float16)
    o = SC.adam_args("plain", step, "lens", torch.float16)
    ref = SC.adam_reference(g, w, m, v, table, o)
    for s, n, grp in zip(starts.tolist(), lens.tolist(), groups.tolist()):
        sl = slice(s, s + n)
        p_, m_, v_ = w[sl].clone(), m[sl].clone(), v[sl].clone()
        lr, wd = float(torch.tensor(SC.LR[grp], dtype=torch.float32)), float(torch.tensor(SC.WD[grp], dtype=torch.float32))
        O.adamw_step(p_, g[sl].clone(), m_, v_, step, lr, SC.BETA1, SC.BETA2, SC.ADAM_EPS, wd)
        for name, want in (("master", p_), ("exp_avg", m_), ("exp_avg_sq", v_)):
            assert float((ref[name][0][sl] - want).abs().max()) < 1e-14, name
    assert all(bool((b[mask] > 0).all()) and bool((b[~mask] == 0).all()) for _, b in ref.values())
    # clipping is the oracle's clip_grad_norm on the counted chunks' norm
    o = SC.adam_args("clip", step, "lens", torch.float16)
    counted = [g[s:s + n].clone() for s, n, c in zip(starts.tolist(), lens.tolist(), table[3].tolist()) if c]
    assert abs(O.clip_grad_norm(counted, o["max_grad_norm"]) - math.sqrt(o["sumsq"])) < 1e-9 * math.sqrt(o["sumsq"])
    sl = slice(int(starts[0]), int(starts[0]) + int(lens[0]))
    clipped = SC.adam_reference(g, w, m, v, table, o)["exp_avg"][0][sl]
    assert float((clipped - (SC.BETA1 * m[sl] + (1 - SC.BETA1) * counted[0])).abs().max()) < 1e-9


def test_sum_of_squares_and_embedding_references():
    starts, lens, _, counted, _ = SC.chunk_table("lens")
    g, _ = SC.grads_of("lens", torch.float32)
    tot, bound = SC.sumsq_reference("lens", torch.float32)
    want = sum(float(g[s:s + n].norm() ** 2) for s, n, c in zip(starts.tolist(), lens.tolist(), counted.tolist()) if c)
    assert abs(tot - want) < 1e-9 * want and 0 < bound < 1e-4 * tot
    c = SC.emb_bwd_problem((300, 520), "window", "randn", 0, "both", True, torch.float16)
    keep = torch.from_numpy(O.dropout_keep_mask(300 * 520, c.p, SC.SEED, SC.STREAM)).view(300, 520).double()
    assert c.p == 0.1 and torch.equal(c.masked != 0, (c.dout * keep) != 0)           # (the oracle's scale is an fp32 number)
    assert float((c.masked - c.dout * keep).abs().max()) < 1e-6
    want = c.init["dtable"].clone().index_add_(0, c.ids - SC.EMB_START, c.masked)
    assert float((c.ref["dtable"] - want).abs().max()) < 1e-12


# ---------------------------------------------------------------------------------------------------------------- 4. the checker checks
def _below_one(tag, fails, worst):
    for k, r in sorted(worst.items()):
        print(f"RATIO stand-in {tag} {k[0]} {k[1]}: worst err / bound = {r:.6f}")
    assert not fails, "\n".join(fails[:20])
    assert all(r < 1.0 for r in worst.values()), worst


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_stand_ins_pass_the_flat_and_embedding_checks(dtype):
    B = SC.StandIn()
    for op in SC.FLAT_OPS:
        fails, cells, worst = SC.flat_sweep(B, op, dtype)
        _below_one(f"{op} {SC.NAME[dtype]}", fails, worst)
    fails, cells = SC.emb_fwd_sweep(B, dtype)
    assert not fails and cells == 27, fails[:10]
    seen = set()
    for shape in SC.EMB_BWD_SHAPES:
        fails, cells, worst = SC.emb_bwd_sweep(B, shape, dtype)
        _below_one(f"embedding_bwd {shape} {SC.NAME[dtype]}", fails, worst)
        seen |= set(worst)
    assert seen == {("embedding_bwd", n) for n in ("dtable", "dpos", "dx")}


@pytest.mark.parametrize("dtype", SC.CE_DTYPES, ids=IDS3)
def test_stand_ins_pass_the_absmax_cross_entropy_and_statistics_checks(dtype):
    B = SC.StandIn()
    fails, cells = SC.absmax_sweep(B, dtype)
    assert not fails and cells >= 28, fails[:10]
    fails, cells, worst = SC.ce_sweep(B, dtype)
    _below_one(f"cross entropy {SC.NAME[dtype]}", fails, worst)
    assert cells == 59 and {n for _, n in worst} == {"sumexp", "loss", "loss2", "dlogits"}
    fails, cells, worst = SC.grad_stats_sweep(B, dtype)
    _below_one(f"grad_stats {SC.NAME[dtype]}", fails, worst)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_stand_ins_pass_the_column_sum_and_adamw_checks(dtype):
    B = SC.StandIn()
    for sweep, cells_want in ((SC.colsum_sweep, 24), (SC.finalize_sweep, 32), (SC.adam_sweep, 18)):
        fails, cells, worst = sweep(B, dtype)
        _below_one(f"{sweep.__name__} {SC.NAME[dtype]}", fails, worst)
        assert cells == cells_want and worst


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("mutant", tuple(SC.MUTANTS))
def test_mutant_is_rejected(mutant, dtype):
    fails = SC.run_mutant_cell(SC.StandIn(mutant), mutant, dtype)
    assert fails, mutant
    clean = SC.run_mutant_cell(SC.StandIn(), mutant, dtype)
    assert not clean, clean
    print(f"{mutant} on {SC.MUTANTS[mutant]} {SC.NAME[dtype]}: " + "; ".join(fails[:3]))


# ---------------------------------------------------------------------------------------------------------------- 5. the refusals
def _refusal_id(r):
    return f"{r[0]}-" + ",".join(f"{k}={'misaligned' if isinstance(v, int) and v > 0xFFFF and v % 16 else v}" for k, v in r[1].items())


@pytest.mark.parametrize("entry,kw,code", SC.REFUSALS, ids=[_refusal_id(r) for r in SC.REFUSALS])
def test_refusal(entry, kw, code):
    assert SC.refuse(entry, kw) == code


def test_refusal_table_covers_every_entry_point_and_condition():
    assert {e for e, _, _ in SC.REFUSALS} == set(SC.REFUSAL_BASE) and len(SC.REFUSAL_BASE) == 17
    assert _lib.lib().cogv_adamw_step(None, None) == _lib.ERR_ARG
    by = {e: [kw for x, kw, _ in SC.REFUSALS if x == e] for e in SC.REFUSAL_BASE}
    has = lambda e, **kw: kw in by[e]
    for e in ("gelu_fwd", "gelu_bwd", "dropout", "add", "scale", "add_stream"):
        assert has(e, n=60) and has(e, dtype=_lib.F32)                          # n % 8, an unsupported dtype
    assert has("absmax", n=0) and has("cast_flat", n=0) and has("cast_flat_back", n=0)
    assert has("colsum", N=12) and has("colsum", ld=20) and has("colsum", workspace_bytes=2 * 16 * 4 - 1)
    assert has("embedding_fwd", h=12) and has("embedding_bwd", h=12) and has("embedding_bwd", n_tok=2 ** 31 - 1)
    assert has("dropout", p=1.0) and has("dropout", p=-0.25) and has("embedding_fwd", dropout_p=1.0) and has("embedding_bwd", dropout_p=-0.5)
    assert has("grad_stats", nchunks=0) and has("adamw_step", nchunks=0) and has("adamw_step", step=0)
    assert has("grad_stats", workspace_bytes=2048 * 8 - 1) and _lib.lib().cogv_grad_stats_workspace_bytes() == 2048 * 8
    assert _lib.lib().cogv_embedding_bwd_workspace_bytes(16, 4) == (16 + 4) * 8 and _lib.lib().cogv_colsum_workspace_bytes(300, 16) == 2 * 16 * 4
    # every pointer of every base is aligned and non-null where required: each refusal changes exactly what it names
    for e, base in SC.REFUSAL_BASE.items():
        assert all(v % 16 == 0 for k, v in base.items() if isinstance(v, int) and v > 0xFFFF), e
    assert {c for _, _, c in SC.REFUSALS} == {_lib.ERR_ARG, _lib.ERR_UNSUPPORTED}
