"""Shared body of the tile-GEMM cell sweep (csrc/gemm_plan.h, csrc/gemm_gen1 .. 4.cuh): the grid of shapes every generation
runs (tests/test_gemm_plan.py proves on the CPU that it reaches the paths named below), the epilogue cells, the operands inside
guarded allocations, the fp64 references and the sweeps tests/test_gemm_cells_gpu.py runs.  Imports without a GPU.

Exact cells: A, B in {-1, 0, 1}, integer bias / previous C / aux, dropout at p = 0.5 (keep scale exactly 2).  Every partial sum
is an integer far below 2^24, so an fp32 sum in ANY order, in any split and through the reduce pass is exact and the output
equals the fp64 reference rounded once -- to the bit, zero signs included.  The reference follows the epilogue order of
include/cogview_hip.h (+bias -> [store pre-activation or gelu'] -> GeLU | x gelu'(aux) | x aux -> dropout -> +C -> round ->
abs-max) and is written here, not taken from tests/cpu_ops.py.

Operands: A, B, C, aux and the bias each live inside a larger allocation (leading dimension = width + 8 or + 24, 4 guard rows
before and after; vectors: 8 guard elements each side).  Padding and guards of inputs are NaN -- the kernels clamp edge rows and
columns to the last valid one, so no legitimate path reads them -- and those of every output hold a sentinel bit pattern that
must be intact after the call."""
import ctypes as C
import functools
from collections import namedtuple
from contextlib import contextmanager

import torch

from cogview_amd import _lib
from oracle import cogview_oracle as O
from tests.gemv_cells import DT_CODE, DT_NAME, DTYPES, EXACT_MAX, U, bound, ternary

BIAS, GELU, DGELU, DROPOUT, ABSMAX, ACCUM, COLSUM, GELU_DAUX, MULAUX = 1, 2, 4, 8, 16, 32, 64, 128, 256
FLAG_NAMES = ((BIAS, "BIAS"), (GELU, "GELU"), (DGELU, "DGELU"), (DROPOUT, "DROPOUT"), (ABSMAX, "ABSMAX"), (ACCUM, "ACCUM"),
              (COLSUM, "COLSUM"), (GELU_DAUX, "GELU_DAUX"), (MULAUX, "MULAUX"))
NT, NN, TN, TA = 0, 1, 2, 3                                      # layout index: -, trans_b, both, trans_a only
LAYOUTS = (NT, NN, TN, TA)
LAYOUT_NAME = {NT: "NT", NN: "NN", TN: "TN", TA: "TA"}
GENERATIONS = (1, 2, 3, 4)
VARIANT = {1: 1, 2: 3, 3: 9, 4: 10}                              # generation -> kernel_variant
TILE = {1: (128, 128), 2: (256, 128), 3: (256, 256), 4: (256, 256)}

# The grid: the smallest shapes at which each path can still go wrong.  (M, N, K, splitk asked for, grid shrunk to 8 workgroups)
# -> what the plan must say: (tiles M, tiles N, effective splitk, k-tiles of 64 per split).
#   tile edges: one full tile, 8-row and 8-column edge tiles, a ragged K (72, 200, 328: tails of 8) for generation 1
#   k-tiles: one, two and three (prologue and drain of the 2- and 3-stage pipelines)
#   split-K: 192 = 3 k-tiles in 2 splits -> 2 + 1
# Generation 1's row of ragged Ks has neither a one-k-tile cell nor a split of unequal k-tile counts (328 -> 3 + 3, the second
# with a tail of 8): the last two cells of its row add them (64 -> 1; 264 -> 5 k-tiles -> 3 + 2).
_PERSISTENT = (((256, 256, 64, 1, False), (1, 1, 1, 1)), ((264, 520, 128, 1, False), (2, 3, 1, 2)), ((520, 264, 192, 2, False), (3, 2, 2, 2)),
               ((520, 520, 192, 1, True), (3, 3, 1, 3)), ((520, 520, 192, 2, True), (3, 3, 2, 2)))
GRID = {
    1: (((56, 64, 72, 1, False), (1, 1, 1, 2)), ((200, 136, 200, 1, False), (2, 2, 1, 4)), ((136, 264, 328, 2, False), (2, 3, 2, 3)),
        ((56, 64, 64, 1, False), (1, 1, 1, 1)), ((136, 264, 264, 2, False), (2, 3, 2, 3))),
    2: (((64, 64, 64, 1, False), (1, 1, 1, 1)), ((264, 136, 128, 1, False), (2, 2, 1, 2)), ((520, 264, 192, 2, False), (3, 3, 2, 2))),
    3: _PERSISTENT,
    4: _PERSISTENT,
}
RANDN_SHAPES = (1, 2)                                            # of a generation's row: its middle shape and its split-K shape

# one epilogue cell: flag set, fp32 output, GELU: the pre-activation is stored (aux set), dropout_row0
Cell = namedtuple("Cell", "flags out_f32 aux row0", defaults=(False, False, 0))
# the flag sets generations 3 and 4 compile an epilogue instance for; every other set runs the run-time-flag instance (F == -1)
COMPILED = (0, BIAS, ACCUM, BIAS | DROPOUT | ABSMAX, BIAS | GELU, DGELU | COLSUM, DGELU, BIAS | GELU | GELU_DAUX, MULAUX | COLSUM)
RUNTIME_ONLY = (ABSMAX, BIAS | ACCUM, MULAUX, DROPOUT | ACCUM, DROPOUT, COLSUM | ACCUM)
CELLS = tuple(Cell(f) for f in COMPILED) + (
    Cell(ABSMAX), Cell(BIAS | ACCUM), Cell(MULAUX), Cell(DROPOUT | ACCUM, row0=16), Cell(DROPOUT), Cell(BIAS | GELU, aux=True),
    Cell(COLSUM | ACCUM),                                        # the column sums of the run-time-flag instance, of an accumulated C
    Cell(0, out_f32=True), Cell(BIAS | ACCUM, out_f32=True), Cell(BIAS | DROPOUT | ABSMAX, out_f32=True),
    Cell(MULAUX | COLSUM, out_f32=True))                         # (refused: the column sums are those of a 16-bit output)
SPLIT_CELLS = (Cell(0), Cell(BIAS), Cell(ACCUM), Cell(BIAS | DROPOUT | ABSMAX), Cell(BIAS | GELU), Cell(ACCUM, out_f32=True),
               Cell(MULAUX | COLSUM))                            # (refused: no column sums through the reduce pass)
# cogv_gemm_grouped (generation 4): (M, N, K, flags, splitk) of the three problems of one launch
GROUP = ((256, 264, 128, ACCUM, 1), (520, 256, 192, 0, 2), (264, 520, 64, ACCUM, 1))
GROUP_ITEMS = 1 * 2 + 3 * 1 * 2 + 2 * 3

A_DENSITY, GELU_DENSITY = 0.5, 0.125
SEED, STREAM = 20240, 7                                          # of the dropout mask
SENT16, SENT32, NAN16 = 0x7BCD, 0x7BCD7BCD, 0x7FFF               # finite in fp16, bf16 and fp32; no output here equals them


def cells_of(splitk):
    return SPLIT_CELLS if splitk > 1 else CELLS


def refusal(gen, splitk, cell):
    """the code cogv_gemm and cogv_gemm_plan must answer for a cell (0: it runs): the column sums with split-K or an fp32 output
    are a bad argument (checked first), in generations 1 and 2 an unsupported combination"""
    if cell.flags & COLSUM:
        if splitk > 1 or cell.out_f32:
            return _lib.ERR_ARG
        if gen <= 2:
            return _lib.ERR_UNSUPPORTED
    return _lib.OK


def flags_name(flags):
    return "|".join(n for f, n in FLAG_NAMES if flags & f) or "0"


def cell_name(cell):
    return "flags=" + flags_name(cell.flags) + (" out_f32" if cell.out_f32 else "") + (" aux" if cell.aux else "") + \
        (f" row0={cell.row0}" if cell.row0 else "")


# ------------------------------------------------------------------------------------------------------------ references (fp64)
def gelu_grad(x):
    """d/dx of O.gelu (the tanh form of mpu/sparse_transformer.py:172-176)"""
    c, a = 0.7978845608028654, 0.044715
    t = torch.tanh(c * x * (1.0 + a * x * x))
    return 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * c * (1.0 + 3.0 * a * x * x)


@functools.lru_cache(maxsize=None)
def operands(M, N, K, density):
    """CPU, fp64, shared and never written: A [M, K], B [N, K] in {-1, 0, 1}, dot = A B^T, integer bias / previous C / aux"""
    g = torch.Generator().manual_seed(1000003 * M + 1009 * N + K + int(64 * density))
    a, b = ternary((M, K), density, g), ternary((N, K), density, g)
    rnd = lambda lim, shape: torch.randint(-lim, lim + 1, shape, generator=g).double()
    return dict(a=a, b=b, dot=a @ b.t() + 0.0, bias=rnd(4, (N,)), prev=rnd(4, (M, N)), mul=rnd(2, (M, N)), dg=rnd(3, (M, N)),
                csprev=rnd(4, (N,)))


@functools.lru_cache(maxsize=None)
def keep_mask(M, N, row0):
    """bool [M, N]: the elements dropout(p = 0.5, SEED, STREAM) keeps of rows [row0, row0 + M) of a tensor N wide"""
    m = O.dropout_keep_mask((row0 + M) * N, 0.5, SEED, STREAM)
    return torch.from_numpy(m > 0).view(row0 + M, N)[row0:].clone()


def reference(cell, dot, bias, aux, keep, prev):
    """the epilogue of include/cogview_hip.h in fp64, before the one rounding: (output, what aux receives or None)"""
    f, x, stored = cell.flags, dot, None
    if f & BIAS:
        x = x + bias
    if f & GELU:
        if f & GELU_DAUX:
            stored = gelu_grad(x)
        elif cell.aux:
            stored = x                                           # rounded to the storage type: exact for these integers
        x = O.gelu(x)
    if f & DGELU:
        x = x * gelu_grad(aux)
    if f & MULAUX:
        x = x * aux
    if f & DROPOUT:                                              # dropped: -0.0; a kept element is never -0.0
        x = torch.where(keep, x * 2.0 + 0.0, torch.full_like(x, -0.0))
    if f & ACCUM:
        x = x + prev
    return x, stored


def ulp(ref, dtype):
    """one unit in the last place of the 16-bit type at |ref| (fp16: subnormal spacing below 2^-14), at least 2^-24"""
    _, e = torch.frexp(ref.abs())                                # |ref| = m 2^e, m in [0.5, 1)
    e = torch.where(ref == 0, -1000.0, (e - 1).double())
    if dtype == torch.float16:
        e = e.clamp_min(-14.0)
    return torch.exp2(e - (10.0 if dtype == torch.float16 else 7.0)).clamp_min(2.0 ** -24)


# ------------------------------------------------------------------------------------------------------------ guarded allocations
class Guarded:
    """[rows, cols] of `dtype` inside a larger device allocation: rows `cols + pad` apart, 4 guard rows before and after -- or
    (rows None) a vector of `cols` with 8 guard elements each side.  Everything outside `view` holds NaN (an input) or the
    sentinel (an output)."""

    def __init__(self, rows, cols, dtype, pad=0, nan=False):
        wide = dtype == torch.float32
        assert not (nan and wide)
        self.fill = NAN16 if nan else SENT32 if wide else SENT16
        bits = torch.int32 if wide else torch.int16
        if rows is None:
            self.buf = torch.full((cols + 16,), self.fill, dtype=bits, device="cuda")
            self.region = (slice(8, 8 + cols),)
        else:
            self.buf = torch.full((rows + 8, cols + pad), self.fill, dtype=bits, device="cuda")
            self.region = (slice(4, 4 + rows), slice(0, cols))
        self.view = self.buf.view(dtype)[self.region]
        self.bits = self.buf[self.region]
        assert self.view.data_ptr() % 16 == 0

    def set(self, values):
        self.view.copy_(values)
        return self

    def reset(self):
        self.buf.fill_(self.fill)

    def intact(self):
        t = self.buf.clone()
        t[self.region] = self.fill
        return bool((t == self.fill).all())


def make_desc(dtype, layout, M, N, K, a, b, c, flags=0, bias=None, aux=None, absmax=None, dropout=False, row0=0, splitk=1, variant=0,
              ws=None, partial=None):
    """cogv_gemm_desc from tensors and their strides (ops.gemm cannot express ldaux, per-problem flags or per-problem split-K)"""
    d = _lib.GemmDesc()
    d.dtype, d.M, d.N, d.K = DT_CODE[dtype], M, N, K
    d.trans_a, d.trans_b = int(layout in (TN, TA)), int(layout in (NN, TN))
    d.A, d.lda, d.B, d.ldb, d.C, d.ldc = a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), c.data_ptr(), c.stride(0)
    d.out_f32, d.flags, d.splitk, d.kernel_variant = int(c.dtype == torch.float32), flags, splitk, variant
    if bias is not None:
        d.bias = bias.data_ptr()
    if aux is not None:
        d.aux, d.ldaux = aux.data_ptr(), aux.stride(0)
    if absmax is not None:
        d.absmax = absmax.data_ptr()
    if dropout:
        d.dropout_p, d.seed, d.stream_id, d.dropout_row0 = 0.5, SEED, STREAM, row0
    if ws is not None:
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    if partial is not None:
        d.colsum_partial = partial.data_ptr()
    return d


class Staged:
    """One (shape, layout, dtype): A and B (fp64 values the 16-bit type holds) and the bias on the device with NaN around them,
    the outputs with sentinels around them.  `call` launches one epilogue cell through cogv_gemm."""

    def __init__(self, ops, M, N, K, layout, dtype, a, b, bias, splitk=1):
        self.ops, self.M, self.N, self.K, self.layout, self.dtype, self.splitk = ops, M, N, K, layout, dtype, splitk
        ta, tb = layout in (TN, TA), layout in (NN, TN)
        self.A = Guarded(K if ta else M, M if ta else K, dtype, 8, nan=True).set(a.t() if ta else a)
        self.B = Guarded(K if tb else N, N if tb else K, dtype, 24, nan=True).set(b.t() if tb else b)
        self.bias = Guarded(None, N, dtype, nan=True).set(bias)
        self.C16, self.C32 = Guarded(M, N, dtype, 24), Guarded(M, N, torch.float32, 8)
        self.aux_in, self.aux_out = Guarded(M, N, dtype, 8, nan=True), Guarded(M, N, dtype, 8)
        self.absmax = torch.zeros(1, dtype=torch.float32, device="cuda")
        self.rows = 2 * ((M + 255) // 256)                       # cogv_gemm_colsum_rows(M), by the header
        self.partial = Guarded(None, self.rows * N, torch.float32)
        self.cs, self.cs_acc = Guarded(None, N, dtype), Guarded(None, N, dtype)
        self.ws = Guarded(None, splitk * M * N, torch.float32) if splitk > 1 else None
        self.outputs = [o for o in (self.C16, self.C32, self.aux_out, self.partial, self.ws) if o is not None]

    def out(self, cell):
        return self.C32 if cell.out_f32 else self.C16

    def desc(self, cell, variant, splitk=None):
        f = cell.flags
        aux = self.aux_in if f & (DGELU | MULAUX) else self.aux_out if (f & GELU_DAUX) or cell.aux else None
        return make_desc(self.dtype, self.layout, self.M, self.N, self.K, self.A.view, self.B.view, self.out(cell).view, f,
                         bias=self.bias.view if f & BIAS else None, aux=None if aux is None else aux.view,
                         absmax=self.absmax if f & ABSMAX else None, dropout=bool(f & DROPOUT), row0=cell.row0,
                         splitk=self.splitk if splitk is None else splitk, variant=variant,
                         ws=None if self.ws is None else self.ws.view, partial=self.partial.view if f & COLSUM else None)

    def arm(self, cell, prev=None):
        """every output back to sentinels, the previous C in place, the abs-max slot zeroed"""
        for o in self.outputs:
            o.reset()
        if cell.flags & ACCUM:
            self.out(cell).view.copy_(prev)
        self.absmax.zero_()

    def call(self, d):
        rc = _lib.lib().cogv_gemm(C.byref(d), self.ops._stream())
        torch.cuda.synchronize()
        return rc

    def stray(self, cell):
        """names of the outputs whose sentinels changed"""
        names = ((self.C16, "C"), (self.C32, "C (fp32)"), (self.aux_out, "aux"), (self.partial, "colsum partials"), (self.ws, "split-K slabs"))
        written = [self.out(cell), self.ws] + ([self.aux_out] if (cell.flags & GELU_DAUX) or cell.aux else []) + \
            ([self.partial] if cell.flags & COLSUM else [])
        bad = []
        for o, name in names:
            if o is None:
                continue
            if any(o is w for w in written):
                if not o.intact():
                    bad.append("guards of " + name)
            elif not bool((o.buf == o.fill).all()):
                bad.append(name + " (not an output of this cell)")
        return bad


def _wrong(got, want):
    """'' or 'n wrong elements, first at (r, c)'"""
    bad = got != want
    n = int(bad.sum())
    if not n:
        return ""
    r, c = bad.nonzero()[0].tolist()
    return f"{n} wrong elements, first at ({r}, {c})"


def _finalize(S, out, accumulate):
    rc = _lib.lib().cogv_colsum_finalize(DT_CODE[S.dtype], S.partial.view.data_ptr(), S.rows, S.N, out.view.data_ptr(), int(accumulate), S.ops._stream())
    torch.cuda.synchronize()
    return rc


@contextmanager
def eight_workgroups(ops, on=True):
    """cogv_gemm_reserve_cus such that max(CUs - reserved, 8) == 8; the previous value comes back"""
    if not on:
        yield
        return
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    prev = ops.gemm_reserve_cus(cus - 8)
    try:
        yield
    finally:
        ops.gemm_reserve_cus(prev)


def run_cell(S, ref, cell, gen):
    """One cell on staged operands: [] or the failures ('refused' is the caller's to know from `refusal`).
    ref: dict on the device, fp64 -- dot, bias, prev, mul, dg, csprev; keep masks come from keep_mask."""
    f, dtype, M, N = cell.flags, S.dtype, S.M, S.N
    odt = torch.float32 if cell.out_f32 else dtype
    out, d = S.out(cell), S.desc(cell, VARIANT[gen])
    want_rc = refusal(gen, S.splitk, cell)
    prc, plan = _lib.gemm_plan(d)
    fails = []
    aux = ref["dg"] if f & DGELU else ref["mul"] if f & MULAUX else None
    if aux is not None:
        S.aux_in.view.copy_(aux)
    prev = ref["prev"].to(odt) if f & ACCUM else None
    S.arm(cell, prev)
    if want_rc != _lib.OK:
        before = out.buf.clone()
        rc = S.call(d)
        if (prc, rc) != (want_rc, want_rc):
            fails.append(f"the plan answers {prc} and the call {rc} where both must refuse with {want_rc}")
        if not torch.equal(out.buf, before) or not all(bool((o.buf == o.fill).all()) for o in S.outputs if o is not out):
            fails.append("a refused call wrote C, its guards or another output")
        return fails
    if prc != _lib.OK or plan[0]["generation"] != gen:
        return [f"planned {prc}, generation {plan[0]['generation'] if plan else None}"]
    rc = S.call(d)
    if rc != _lib.OK:
        return [f"the call answers {rc}"]
    first = {id(o): o.buf.clone() for o in S.outputs}
    got = out.view
    fails += S.stray(cell)
    if bool(torch.isnan(got).any()) or ((f & GELU_DAUX or cell.aux) and bool(torch.isnan(S.aux_out.view).any())):
        fails.append("an out-of-range operand element was used (NaN in an output)")
    keep = keep_mask(M, N, cell.row0).cuda() if f & DROPOUT else None
    x, stored = reference(cell, ref["dot"], ref["bias"], aux, keep, ref["prev"])
    if f & (GELU | DGELU):
        # transcendental outputs: the correctly rounded value or its neighbour (1 ulp of the 16-bit type, floor 2^-24)
        for name, g, w in (("C", got, x),) + ((("stored gelu'", S.aux_out.view, stored),) if f & GELU_DAUX else ()):
            bad = (g.double() - w).abs() > ulp(w, dtype)
            if bool(bad.any()):
                r, c = bad.nonzero()[0].tolist()
                fails.append(f"{name}: {int(bad.sum())} elements beyond 1 ulp, first at ({r}, {c}): {float(g[r, c])} against {float(w[r, c]):.9g}")
        if cell.aux:
            w = _wrong(S.aux_out.view, stored.to(dtype))
            if w:
                fails.append("stored pre-activation: " + w)
        if f & COLSUM:
            if not bool((S.partial.bits != SENT32).all()):
                fails.append(f"the {S.rows} x {N} column-sum partials are not fully written")
            S.cs.reset()
            if _finalize(S, S.cs, False) != _lib.OK or not S.cs.intact():
                fails.append("cogv_colsum_finalize failed or wrote outside the vector")
            own = got.double()
            sums = own.sum(0)
            lim = M * 2.0 ** -24 * own.abs().sum(0) + U[dtype] * sums.abs()
            bad = (S.cs.view.double() - sums).abs() > lim
            if bool(bad.any()):
                fails.append(f"column sums: {int(bad.sum())} beyond the bound, first at column {int(bad.nonzero()[0])}")
    else:
        assert float(x.abs().max()) <= EXACT_MAX[dtype], (cell, float(x.abs().max()))
        want = x.to(odt)
        w = _wrong(got, want)
        if w:
            fails.append(w)
        if (f & DROPOUT) and not (f & ACCUM):                    # marked zeros: the raw patterns
            zero = -0x80000000 if cell.out_f32 else -0x8000      # (the sign bit alone, as the signed integer the buffer holds)
            marked = out.bits == zero
            if not torch.equal(marked, ~keep):
                fails.append(f"marked zeros: {int((marked & keep).sum())} kept elements are -0.0, {int((~marked & ~keep).sum())} dropped ones are not")
        if f & ABSMAX:
            amax = float(want.to(dtype).abs().max())             # fp32 output: the max of the 16-bit roundings
            if float(S.absmax) != amax:
                fails.append(f"abs-max {float(S.absmax)} against {amax}")
        if f & COLSUM:
            if S.rows != _lib.lib().cogv_gemm_colsum_rows(M):
                fails.append(f"cogv_gemm_colsum_rows({M}) is not {S.rows}")
            if not bool((S.partial.bits != SENT32).all()):
                fails.append(f"the {S.rows} x {N} column-sum partials are not fully written")
            sums = want.double().sum(0)
            S.cs.reset()
            S.cs_acc.reset()
            S.cs_acc.view.copy_(ref["csprev"])
            if _finalize(S, S.cs, False) != _lib.OK or _finalize(S, S.cs_acc, True) != _lib.OK or not (S.cs.intact() and S.cs_acc.intact()):
                fails.append("cogv_colsum_finalize failed or wrote outside the vector")
            if not torch.equal(S.cs.view, sums.to(dtype)):
                fails.append(f"column sums: {int((S.cs.view != sums.to(dtype)).sum())} wrong")
            if not torch.equal(S.cs_acc.view, (sums + ref["csprev"]).to(dtype)):
                fails.append(f"accumulated column sums: {int((S.cs_acc.view != (sums + ref['csprev']).to(dtype)).sum())} wrong")
    # a second call gives the same bits, in every output and around it
    S.arm(cell, prev)
    if S.call(d) != _lib.OK or not all(torch.equal(o.buf, first[id(o)]) for o in S.outputs):
        fails.append("the second call gives other bits")
    return fails


def _device_ref(M, N, K, density):
    return {k: v.cuda() for k, v in operands(M, N, K, density).items() if k not in ("a", "b")}


def sweep(ops, gen, layout, dtype):
    """every shape of the generation's row x every epilogue cell: -> (failures: one line each, launched, refused, cells)"""
    fails, ran, refused, cells = [], 0, 0, 0
    for (M, N, K, splitk, wg8), _ in GRID[gen]:
        tag = f"gen {gen} {LAYOUT_NAME[layout]} {DT_NAME[dtype]} M={M} N={N} K={K}" + (f" splitk={splitk}" if splitk > 1 else "") + (" 8 workgroups" if wg8 else "")
        with eight_workgroups(ops, wg8):
            staged = {}
            for density in (A_DENSITY, GELU_DENSITY):
                o = operands(M, N, K, density)
                staged[density] = (Staged(ops, M, N, K, layout, dtype, o["a"], o["b"], o["bias"], splitk), _device_ref(M, N, K, density))
            pre = operands(M, N, K, GELU_DENSITY)
            pre = pre["dot"] + pre["bias"]
            assert float((pre.abs() <= 4).double().mean()) >= 0.5, (M, N, K)
            if wg8:
                S = staged[A_DENSITY][0]
                rc, plan = _lib.gemm_plan(S.desc(Cell(0), VARIANT[gen]), num_cus=0)
                assert rc == _lib.OK and plan[0]["grid_x"] == 8 and plan[0]["items"] in (9, 18), (tag, rc, plan)
            for cell in cells_of(splitk):
                cells += 1
                S, ref = staged[GELU_DENSITY if cell.flags & (GELU | DGELU) else A_DENSITY]
                bad = run_cell(S, ref, cell, gen)
                if refusal(gen, splitk, cell) != _lib.OK:
                    refused += 1
                else:
                    ran += 1
                fails += [f"{tag} {cell_name(cell)}: {b}" for b in bad]
    return fails, ran, refused, cells


def randn_ratios(ops, gen, layout, dtype):
    """flag set BIAS on `randn` operands (integers do not exercise operand mantissas): |got - ref| <= gemv_cells.bound element by
    element -> (failures, {shape tag: worst err / bound})"""
    fails, worst = [], {}
    for i in RANDN_SHAPES:
        (M, N, K, splitk, wg8), _ = GRID[gen][i]
        g = torch.Generator().manual_seed(7 * K + M + N)
        a, b = torch.randn((M, K), generator=g).to(dtype).double(), (torch.randn((N, K), generator=g) * 0.05).to(dtype).double()
        bias = torch.randn(N, generator=g).to(dtype).double()
        ref, absdot = a @ b.t() + bias, a.abs() @ b.abs().t()
        S = Staged(ops, M, N, K, layout, dtype, a, b, bias, splitk)
        cell = Cell(BIAS)
        S.arm(cell)
        rc = S.call(S.desc(cell, VARIANT[gen]))
        tag = f"M={M} N={N} K={K} splitk={splitk}"
        if rc != _lib.OK:
            fails.append(f"{tag}: the call answers {rc}")
            continue
        ratio = float(((S.C16.view.double().cpu() - ref).abs() / bound(ref, absdot, bias, K, dtype)).max())
        worst[tag] = ratio
        if not ratio <= 1.0:
            fails.append(f"{tag}: err / bound = {ratio:.3f}")
        fails += [f"{tag}: {b}" for b in S.stray(cell)]
    return fails, worst


def grouped_sweep(ops, layout, dtype, wg8):
    """the three problems of GROUP in one cogv_gemm_grouped launch (per-problem ACCUM / 0 / ACCUM, split-K 1 / 2 / 1): exact,
    canaries intact, and each problem bit-equal to the same problem launched alone with kernel_variant 10 -> failures"""
    fails, cell_of = [], {}
    tag = f"grouped {LAYOUT_NAME[layout]} {DT_NAME[dtype]}" + (" 8 workgroups" if wg8 else "")
    with eight_workgroups(ops, wg8):
        probs = []
        for M, N, K, flags, splitk in GROUP:
            o = operands(M, N, K, A_DENSITY)
            S = Staged(ops, M, N, K, layout, dtype, o["a"], o["b"], o["bias"], splitk)
            cell = Cell(flags)
            prev = o["prev"].to(dtype).cuda()
            S.arm(cell, prev)
            want = reference(cell, o["dot"], None, None, None, o["prev"])[0]
            assert float(want.abs().max()) <= EXACT_MAX[dtype]
            probs.append((S, cell, prev, want.to(dtype).cuda()))
        descs = (_lib.GemmDesc * len(probs))(*[S.desc(cell, 0) for S, cell, _, _ in probs])
        rc, plan = _lib.gemm_plan(descs, len(probs))
        if rc != _lib.OK or any(p["generation"] != 4 or p["items"] != GROUP_ITEMS for p in plan):
            return [f"{tag}: planned {rc} {plan}"]
        if wg8:
            assert plan[0]["grid_x"] == 8 < plan[0]["items"], plan[0]
        rc = _lib.lib().cogv_gemm_grouped(descs, len(probs), ops._stream())
        torch.cuda.synchronize()
        if rc != _lib.OK:
            return [f"{tag}: the call answers {rc}"]
        for i, (S, cell, prev, want) in enumerate(probs):
            where = f"{tag} problem {i} M={S.M} N={S.N} K={S.K} flags={flags_name(cell.flags)} splitk={S.splitk}"
            w = _wrong(S.C16.view, want)
            if w:
                fails.append(f"{where}: {w}")
            if bool(torch.isnan(S.C16.view).any()):
                fails.append(f"{where}: an out-of-range operand element was used (NaN in an output)")
            fails += [f"{where}: {b}" for b in S.stray(cell)]
            together = S.C16.buf.clone()
            S.arm(cell, prev)
            rc = S.call(S.desc(cell, VARIANT[4]))
            if rc != _lib.OK or not torch.equal(S.C16.buf, together):
                fails.append(f"{where}: launched alone (kernel_variant 10, answer {rc}) it gives other bits")
    return fails
