"""Shared body of the cell sweep of the trainer's memory-bound kernels (cogview_amd/csrc/elementwise.hip: ew_kernel, absmax_kernel,
absmax_f32_kernel, add_stream_kernel, embedding_fwd_kernel, embedding_dx_kernel, emb_key_stats_kernel, emb_segsum_kernel,
colsum_partial_kernel, colsum_final_kernel; cogview_amd/csrc/ce_optim.hip: ce_fwd_kernel, ce_bwd_kernel, grad_stats_kernel,
grad_stats_final_kernel, adamw_kernel, cast_up_kernel, cast_down_kernel): the grids (tests/test_stream_cells_cpu.py proves on the CPU
that they reach the paths named below), the operands inside guarded allocations, the fp64 references, the element-wise bounds and the
sweeps tests/test_stream_cells_gpu.py runs.  Imports without a GPU.

BITWISE (the output must equal the fp64 result rounded once; only the sign of a zero is free): add, scale, add_stream, both casts, dropout
(p = 0.5: keep scale exactly 2), embedding forward, every absmax (the flat ones and every absmax_out slot: max |stored output|),
rowmax and predicted of the cross entropy, params == round_T(master) of AdamW, and the `exact` kind of column sum and embedding
backward.  Each of these kernels is one IEEE fp32 operation and one rounding; the operands are chosen so that the fp32 operation is
exact (exponent spread under 13 bits, a scale of at most 8 significant bits, small integers), which the CPU test asserts.
BOUNDED (|got - ref64| <= FACTOR x bound, element by element): GELU forward and backward, sumexp, loss and dlogits of the cross
entropy, the `randn` kind of column sum, column-sum finalize and embedding backward, the gradient statistics and the three fp32 state
tensors of AdamW.  A bound is half a unit in the last place of a 16-bit output at the reference (nothing for an fp32 output) plus the
fp32 error terms of the kernel's own operations, each named where it is added; none comes from what a kernel produced.

The backward of the cross entropy is judged in isolation: gmax and gsum are the fp64 reference rounded to fp32, never the GPU forward.
AdamW gets the sum of squares from the fp64 reference too.

Operands: inputs lie inside NaN guards (`ld > N` pads of the column sum included), outputs and workspaces between sentinels, workspaces
sized exactly to their `*_workspace_bytes` query.  After every call all sentinels must be intact, and a second call -- after in-place
outputs (accumulated column sums, embedding tables, AdamW state, the statistics) are restored -- gives the same bits.

`StandIn` drives the stand-ins of tests/cpu_ops.py through the same cells: a fixture of the CPU test only, which must pass every check
with every ratio below 1 and whose seeded mutants (`MUTANTS`) must each be rejected on the cell named for it."""
import ctypes as C
import functools
import math
from types import SimpleNamespace

import torch

from cogview_amd import _lib
from oracle import cogview_oracle as O
from tests.gemm_cells import ulp
from tests.gemv_cells import DT_CODE, DT_NAME, DTYPES, EXACT_MAX
from tests.layernorm_cells import E32, Guard, ratio

F32 = torch.float32
CODE = {**DT_CODE, F32: _lib.F32}
NAME = {**DT_NAME, F32: "fp32"}
SEED, STREAM = 977, 5                                            # of every dropout mask
VOCAB_START = 29184                                              # of the cross-entropy cells

# ------------------------------------------------------------------------------------------------------------------ the grids
# flat element-wise: n -> (workgroups, passes of the grid-stride loop, lanes of the last workgroup that has work in the last pass,
# elements of the scalar tail); 8 elements per lane, 256 lanes, at most 2048 workgroups
BIG, BIG_TAIL = 2048 * 256 * 8 + 264 * 8, 2048 * 256 * 8 + 3
FLAT_GRID = (
    (8, (1, 1, 1, 0)),                                           # one lane
    (2040, (1, 1, 255, 0)),                                      # 255 lanes
    (2048, (1, 1, 256, 0)),                                      # one full workgroup
    (2056, (2, 1, 1, 0)),                                        # a second workgroup with one lane
    (BIG, (2048, 2, 8, 0)),                                      # the capped grid loops: second pass of 264 vectors (workgroups 0 and 1)
)
TAIL_GRID = (                                                    # casts and 16-bit absmax only
    (5, (1, 0, 0, 5)),                                           # tail only
    (13, (1, 1, 1, 5)),                                          # a vector plus a tail
    (BIG_TAIL, (2048, 1, 256, 3)),                               # the vector loop on the full capped grid plus a tail
)
FLAT_N = tuple(n for n, _ in FLAT_GRID)
TAIL_N = tuple(n for n, _ in TAIL_GRID)
FLAT_OPS = ("gelu_fwd", "gelu_bwd", "dropout", "add", "scale", "add_stream", "cast_flat", "cast_flat_back")
TAILED = ("cast_flat", "cast_flat_back")
SCALES = (0.8125, 1.5, -0.09375, 3.0, 0.6875, 0.5, -1.25, 2.0)   # at most 8 significant bits
ABSMAX_VARIANTS = ("first", "lastvec", "tail", "nan", "neg")     # where the largest magnitude sits (tail: only where n % 8)
ABSMAX32_N = FLAT_N + (4, 2052)                                  # fp32: 4 elements per lane; one lane, a lane past a workgroup

# embedding forward: (n_tok, h)
EMB_FWD_GRID = (
    ((1, 8), (1, 1, 1)),                                         # smallest
    ((5, 520), (2, 1, 69)),
    ((3, 2056), (4, 1, 3)),
    ((4099, 1032), (2048, 2, 131)),                             # n_tok h / 8 = 528771 > 2048 x 256: the grid-stride loop runs
)
EMB_FWD_SHAPES = tuple(s for s, _ in EMB_FWD_GRID)
# (fp32 out, ids (else x_in), position table, dropout, absmax slot): all eight (out32, pos, dropout) triples, the others alternate
EMB_FWD_CELLS = tuple((o, (o + p + d) % 2 == 0, bool(p), bool(d), (p + 2 * d + o) % 2 == 0) for o in (0, 1) for p in (0, 1) for d in (0, 1))
EMB_FWD_BIG_CELLS = ((0, True, True, True, True), (1, False, True, True, False), (1, True, False, False, True))
EMB_ROWS, EMB_NPOS, EMB_START = 37, 11, 100                      # rows of the word shard, of the position table; first id of the shard

# embedding backward: (n_tok, h) -> (column slabs, lanes of the last slab)
EMB_BWD_GRID = (
    ((1, 8), (1, 1)),                                            # smallest
    ((300, 520), (1, 65)),
    ((600, 2056), (2, 1)),                                       # two column slabs; the second slab has one lane
)
EMB_BWD_SHAPES = tuple(s for s, _ in EMB_BWD_GRID)
EMB_PATTERNS = ("unique", "window", "every", "outside")
WINDOW_TOKENS = (0, 255, 256, 257, 599)                          # one key: both sides of a 256-token scan window, the last window
EMB_WHICH = ("dtable", "dpos", "both")
KINDS = ("exact", "randn")

# column sum: (M, N, ld) -> (column slabs of 512, nslab, rows_per, unrolled iterations of colsum_final_kernel's slice 0, tail iterations)
COLSUM_GRID = (
    ((1, 8, 8), (1, 1, 1, 0, 1)),                                # smallest
    ((3, 72, 88), (1, 1, 3, 0, 1)),                              # ld > N, N < 512
    ((5, 520, 520), (2, 1, 5, 0, 1)),                            # second column slab with one lane
    ((257, 136, 136), (1, 2, 129, 0, 1)),                        # nslab 2, rows_per 129
    ((9472, 8, 8), (1, 37, 256, 1, 2)),                          # nslab 37: unrolled loop and tail
    ((16400, 8, 8), (1, 64, 257, 2, 0)),                         # nslab 64, rows_per 257 (rounded up); unrolled loop twice
)
COLSUM_SHAPES = tuple(s for s, _ in COLSUM_GRID)
FINALIZE_ROWS, FINALIZE_N = (1, 3, 4, 5, 29, 33, 64, 100), (8, 72)

# cross entropy: (rows, v_local) -> (vectors, lanes of the last pass, vectors of thread 0)
CE_GRID = (
    ((1, 8), (1, 1, 1)),                                         # one lane
    ((3, 96), (12, 12, 1)),
    ((2, 2040), (255, 255, 1)),                                  # just under 2048
    ((2, 2048), (256, 256, 1)),
    ((3, 2056), (257, 1, 2)),                                    # thread 0 gets its second vector
    ((2, 4104), (513, 1, 3)),
)
CE_SHAPES = tuple(s for s, _ in CE_GRID)
CE_TARGETS = ("first", "last", "below", "above")                 # t = 0, t = v_local - 1, target = vocab_start - 1, = vocab_start + v_local
CE_SPECIAL = ("noloss", "maxlast", "equal", "neginf", "twoshard")
CE_DTYPES = (torch.float16, torch.bfloat16, F32)
NEGINF_SHAPE = (1, 2056)

# gradient statistics and AdamW: chunk tables (lengths; starts are multiples of 8)
TABLE_LENS = (1, 7, 8, 9, 2047, 2048, 2056, 32768)
STATS_CHUNKS, ADAM_CHUNKS = 2051, 4100                           # past the 2048- / 4096-workgroup caps
ADAM_CELLS = {   # name -> overrides of `adam_args`
    "plain": dict(),
    "clip_inactive": dict(max_norm="above"),                     # clipping asked for, coefficient >= 1
    "clip": dict(max_norm="below"),                              # coefficient < 1
    "l2": dict(adam_w_mode=0),
    "nobc": dict(bias_correction=0),
    "override": dict(max_norm="below", override=True),           # the norm from norm_sumsq_override, stats[0] holds another number
    "scaled": dict(max_norm="below", inv_loss_scale=1.0 / 64),
}
ADAM_STEPS = (1, 2)
OVERFLOWS = ((3, float("inf")), (4, float("nan")))                # (chunk, value in its scalar tail): chunks of 9 and 2047 elements
LR, WD = {0: 0.01, 7: 0.003}, {0: 0.0, 7: 0.1}                   # groups 0 and 7: weight decay 0 and 0.1
BETA1, BETA2, ADAM_EPS = 0.9, 0.95, 1e-8

# Factor on the element-wise bound per (operation, output): 1 = the bound as derived.  An entry is raised only together with a named
# error term read out of the kernel's code, and never above 2 (tests/test_stream_cells_cpu.py asserts that).
BOUNDED = (("gelu_fwd", "y"), ("gelu_bwd", "dx"), ("ce_fwd", "sumexp"), ("ce_fwd", "loss"), ("ce_fwd", "loss2"), ("ce_bwd", "dlogits"),
           ("colsum", "out"), ("colsum_finalize", "out"), ("embedding_bwd", "dtable"), ("embedding_bwd", "dpos"), ("embedding_bwd", "dx"),
           ("grad_stats", "sumsq"), ("adamw", "master"), ("adamw", "exp_avg"), ("adamw", "exp_avg_sq"))
FACTOR = {k: 1.0 for k in BOUNDED}
# Worst |got - fp64 reference| / bound measured on an MI355X over the whole grid and all dtypes.  A 16-bit output sits at 1.00: its
# bound is half a unit in the last place plus the fp32 terms, and round-to-nearest comes within 1e-4 of the half unit on some element
# of every large cell, so the fp32 terms above it are what a wrong kernel has to stay inside.  The fp32 outputs show the fp32 terms
# alone: AdamW's master weight reaches 0.99 where the rounding of w - lr x update falls just above a power of two and the update is
# small, sumexp and loss stay far below their worst case.  No factor had to be raised.
MEASURED = {
    ("gelu_fwd", "y"): 1.0, ("gelu_bwd", "dx"): 0.9999, ("ce_fwd", "sumexp"): 0.1103, ("ce_fwd", "loss"): 0.315, ("ce_fwd", "loss2"): 0.0246,
    ("ce_bwd", "dlogits"): 0.9999, ("colsum", "out"): 0.9999, ("colsum_finalize", "out"): 0.9997, ("embedding_bwd", "dtable"): 1.0,
    ("embedding_bwd", "dpos"): 1.0, ("embedding_bwd", "dx"): 0.9162, ("grad_stats", "sumsq"): 0.0129, ("adamw", "master"): 0.9925,
    ("adamw", "exp_avg"): 0.5147, ("adamw", "exp_avg_sq"): 0.4205,
}


# ------------------------------------------------------------------------------------------ the launch arithmetic, restated
def flat_geometry(n, per=8):
    nvec = n // per
    wgs = min(max((nvec + 255) // 256, 1), 2048)
    stride = wgs * 256
    passes = (nvec + stride - 1) // stride
    rem = nvec - (passes - 1) * stride if passes else 0
    return wgs, passes, rem - ((rem + 255) // 256 - 1) * 256 if rem else 0, n % per


def emb_fwd_geometry(n_tok, h):
    wgs, passes, lanes, _ = flat_geometry(n_tok * h, 8)
    return wgs, passes, lanes


def emb_bwd_geometry(n_tok, h):
    hv = h // 8
    return (hv + 255) // 256, hv - ((hv + 255) // 256 - 1) * 256


def scan_windows(tokens, n_tok):
    """emb_segsum_kernel, workgroup of a key's first token: the 256-token windows it scans -> occurrences found in each"""
    first, remaining, out, w0 = tokens[0], len(tokens) - 1, [], tokens[0] + 1
    while remaining > 0 and w0 < n_tok:
        found = [t for t in tokens[1:] if w0 <= t < w0 + 256]
        out.append(found)
        remaining -= len(found)
        w0 += 256
    return out


def colsum_plan(M):
    nslab = min(max((M + 255) // 256, 1), 64)
    rows_per = (M + nslab - 1) // nslab
    return (M + rows_per - 1) // rows_per, rows_per, nslab


def final_iterations(nslab, part=0):
    """colsum_final_kernel, row slice `part` of 4: (iterations of the 8-way unrolled loop, iterations of the tail loop)"""
    b, unrolled, tail = part, 0, 0
    while b + 28 < nslab:
        unrolled, b = unrolled + 1, b + 32
    while b < nslab:
        tail, b = tail + 1, b + 4
    return unrolled, tail


def colsum_geometry(M, N, ld):
    nslab, rows_per, _ = colsum_plan(M)
    return ((N + 511) // 512, nslab, rows_per) + final_iterations(nslab)


def ce_geometry(v_local):
    nvec = v_local // 8
    return nvec, nvec - (nvec - 1) // 256 * 256, (nvec + 255) // 256


def chunk_passes(nchunks, cap):
    """(workgroups, chunks of workgroup 0) of `for (c = blockIdx.x; c < nchunks; c += gridDim.x)`"""
    g = min(nchunks, cap)
    return g, (nchunks + g - 1) // g


# ------------------------------------------------------------------------------------------ operands
def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 1) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(maxsize=None)
def keep_bool(n, p):
    """bool [n]: what the oracle's element-wise dropout keeps"""
    return torch.from_numpy(O.dropout_keep_mask(n, p, SEED, STREAM) > 0)


def keep_scale(p):
    return 65536.0 / (65536.0 - O._thr16(p))


def spread(g, shape, dtype, lo=-6):
    """values of the 16-bit type with magnitudes in [2^lo, 2^5] (exponent spread 11 bits): the fp32 sum of any two is exact"""
    x = (4.0 * torch.randn(shape, generator=g)).to(dtype).double()
    mag = x.abs().clamp(2.0 ** lo, 32.0)
    return torch.where(x < 0, -mag, mag)


def exact_in_fp32(t):
    return torch.equal(t.float().double(), t)


def round_to(t, dtype):
    """an fp64 tensor that fp32 holds exactly, rounded once to dtype"""
    return t.float().to(dtype)


def bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16 if t.element_size() == 2 else torch.int64)


def _vec(t, dtype, dev):
    """an input inside NaN guards"""
    g = Guard(t.shape[0] if t.dim() == 2 else None, t.shape[-1], dtype, nan=True, device=dev)
    g.view.copy_(t)
    return g


def _out(shape, dtype, dev):
    return Guard(shape[0] if len(shape) == 2 else None, shape[-1], dtype, device=dev)


def _f64(g):
    """a guarded fp32 vector of 2 n elements as n doubles"""
    return g.view.view(torch.float64)


# ------------------------------------------------------------------------------------------ judging
def _where(bad):
    return tuple(bad.nonzero()[0].tolist())


def _judge(fails, ratios, key, got, ref, bound):
    if bool(torch.isnan(got).any()):
        fails.append(f"{key[1]}: NaN (a guard was read, or the output is wrong)")
    r = ratio(got, ref, bound) / FACTOR[key]
    ratios[key] = max(ratios.get(key, 0.0), r)
    if not r <= 1.0:
        bad = ~((got - ref).abs() <= FACTOR[key] * bound.expand_as(got))
        fails.append(f"{key[1]}: err / bound = {r:.3f}, {int(bad.sum())} elements, first {_where(bad)}")


def _judge_bits(fails, name, got, want):
    """got and want in the same storage type: the same value in every element, which for finite numbers is the same bits -- but for the
    sign of a zero, which the kernels (a dropped element is +0.0) and a product with a zero mask choose differently"""
    assert got.shape == want.shape and got.dtype == want.dtype and not bool(torch.isnan(want).any())
    bad = ~(got == want)
    if bool(bad.any()):
        fails.append(f"{name}: {int(bad.sum())} elements are not the exact value, first {_where(bad)}: {float(got[bad][0])} for {float(want[bad][0])}")


class Cell:
    """outputs of one call: name -> Guard; `initial`: name -> values an in-place output starts from"""

    def __init__(self, outputs, initial=None):
        self.outputs, self.initial = outputs, initial or {}
        self.arm()

    def arm(self):
        for n, g in self.outputs.items():
            g.reset()
            if n in self.initial:
                (_f64(g) if n == "stats" else g.view).copy_(self.initial[n])

    def snapshot(self, skip=()):
        return {n: g.buf.clone() for n, g in self.outputs.items() if n not in skip}

    def stray(self):
        return [f"guards of {n} written" for n, g in self.outputs.items() if not g.intact()]


def _twice(cell, call, fails, judge, skip=("workspace",)):
    """the call, the sentinels, `judge`, then the same call on re-armed outputs: the same bits"""
    rc = call()
    if rc != _lib.OK:
        fails.append(f"the call answers {rc}")
        return
    fails += cell.stray()
    first = cell.snapshot(skip)
    judge()
    cell.arm()
    if call() != _lib.OK or not all(torch.equal(v, first[n]) for n, v in cell.snapshot(skip).items()):
        fails.append("the second call gives other bits")


# ------------------------------------------------------------------------------------------ backends
def _arg(a):
    if isinstance(a, torch.Tensor):
        return a.data_ptr()
    if isinstance(a, torch.dtype):
        return CODE[a]
    return a


def adam_desc(a):
    d = _lib.AdamDesc()
    d.dtype = CODE[a["dtype"]]
    for k in ("params", "grads", "master", "exp_avg", "exp_avg_sq", "chunk_start", "chunk_len", "chunk_group", "stats", "norm_sumsq_override"):
        setattr(d, k, _arg(a[k]))
    for k in ("nchunks", "beta1", "beta2", "eps", "step", "bias_correction", "adam_w_mode", "beta1_d", "beta2_d", "inv_loss_scale", "max_grad_norm"):
        setattr(d, k, a[k])
    for i in range(8):
        d.lr[i], d.weight_decay[i] = a["lr"][i], a["weight_decay"][i]
    return d


class Launched:
    """the kernels, through the C ABI"""
    device = "cuda"

    def __init__(self, ops):
        self.stream = ops._stream

    def call(self, name, *args):
        rc = getattr(_lib.lib(), "cogv_" + name)(*[_arg(a) for a in args], self.stream())
        torch.cuda.synchronize()
        return rc

    def adamw(self, a):
        rc = _lib.lib().cogv_adamw_step(C.byref(adam_desc(a)), self.stream())
        torch.cuda.synchronize()
        return rc


# name -> (operation, cell) on which at least one check must reject it
MUTANTS = {
    "the last vector not written": ("flat", ("add", 2056)),
    "the scalar tail skipped": ("flat", ("cast_flat", 13)),
    "the dropout counter off by one group": ("flat", ("dropout", 2056)),
    "position ids not clamped": ("emb_fwd", ((5, 520), (1, True, True, False, True))),
    "an id equal to vocab_end accepted": ("emb_fwd", ((5, 520), (0, True, False, False, True))),
    "one occurrence of a repeated key dropped": ("emb_bwd", ((600, 2056), "window", "exact", 0)),
    "accumulate ignored": ("colsum", ((257, 136, 136), "exact", 1)),
    "column N - 1 of the column sum dropped": ("colsum", ((3, 72, 88), "exact", 0)),
    "the CE target column off by one": ("ce", ((3, 96), "first")),
    "L2 decay applied in decoupled mode": ("adamw", ("plain", 1)),
    "the clip coefficient applied when it is >= 1": ("adamw", ("clip_inactive", 2)),
    "one slab left out of colsum_finalize": ("finalize", (33, 72, "randn")),
}


class StandIn:
    """tests/cpu_ops.py behind the C ABI's argument lists (CPU test fixture); `mutant`: one of MUTANTS"""
    device = "cpu"

    def __init__(self, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.mutant = mutant
        from tests import cpu_ops
        self.ops = cpu_ops

    def call(self, name, *args):
        return getattr(self, name)(*args)

    def adamw(self, a):
        m, chunks = self.mutant, list(zip(a["chunk_start"].tolist(), a["chunk_len"].tolist(), a["chunk_group"].tolist()))
        grads, stats = a["grads"], a["stats"]
        if stats is not None and float(stats[1]) != 0.0:
            return _lib.OK
        if m in ("L2 decay applied in decoupled mode", "the clip coefficient applied when it is >= 1"):
            grads = grads.float()
            ss = float(a["norm_sumsq_override"][0]) if a["norm_sumsq_override"] is not None else float(stats[0]) if stats is not None else 0.0
            coef = a["max_grad_norm"] / (math.sqrt(ss) * a["inv_loss_scale"] + 1e-6) if a["max_grad_norm"] > 0 else 1.0
            gscale = a["inv_loss_scale"] * min(coef, 1.0)
            for s, n, grp in chunks:
                if m.startswith("L2"):
                    grads[s:s + n] += a["weight_decay"][grp & 7] * a["master"][s:s + n] / gscale
                elif coef >= 1.0:
                    grads[s:s + n] *= coef
        self.ops.adamw_step(a["params"], grads, a["master"], a["exp_avg"], a["exp_avg_sq"], a["chunk_start"], a["chunk_len"], a["chunk_group"],
                            a["lr"], a["weight_decay"], a["beta1_d"], a["beta2_d"], a["eps"], a["step"], a["inv_loss_scale"], a["max_grad_norm"],
                            stats, None if a["norm_sumsq_override"] is None else a["norm_sumsq_override"][0], bool(a["bias_correction"]),
                            bool(a["adam_w_mode"]))
        return _lib.OK

    def _store(self, out, val, n):
        cut = n - 8 if self.mutant == "the last vector not written" else n - n % 8 if self.mutant == "the scalar tail skipped" else n
        out[:cut] = val[:cut]
        return _lib.OK

    def gelu_fwd(self, dt, x, y, n):
        return self._store(y, self.ops.gelu_fwd(x), n)

    def gelu_bwd(self, dt, dy, x, dx, n):
        # cpu_ops' formula in double: its tanh form 0.5 (1 + tanh u) cancels in fp32 for x < -3, which the kernels' sigmoid form does not
        return self._store(dx, (dy.double() * self.ops._gelu_grad(x.double())).to(x.dtype), n)

    def dropout(self, dt, x, y, n, p, seed, stream, slot):
        val = self.ops.dropout(x, p, seed, stream, slot)
        if self.mutant == "the dropout counter off by one group":
            keep = torch.roll(keep_bool(n, p), 8)
            val = torch.where(keep, (x.float() * keep_scale(p)).to(x.dtype), torch.zeros_like(x))
        return self._store(y, val, n)

    def add(self, dt, a, b, out, n, slot):
        return self._store(out, self.ops.add(a, b, slot), n)

    def add_stream(self, dt, a, b, out, n, slot):
        return self._store(out, self.ops.add(a, b, slot), n)

    def scale(self, dt, x, y, n, s):
        return self._store(y, self.ops.scale(x, s), n)

    def cast_flat(self, dt, src, dst, n):
        tmp = torch.empty_like(dst)
        self.ops.cast_flat(src, tmp)
        return self._store(dst, tmp, n)

    def cast_flat_back(self, dt, src, dst, n):
        tmp = torch.empty_like(dst)
        self.ops.cast_flat_back(src, tmp)
        return self._store(dst, tmp, n)

    def absmax(self, dt, x, n, out):
        self.ops.absmax(x, out)
        return _lib.OK

    def colsum(self, dt, dy, M, N, ld, out, accumulate, ws, ws_bytes):
        m = self.mutant
        val = out.clone()
        self.ops.colsum(dy[:, :N], out=val, accumulate=bool(accumulate) and m != "accumulate ignored")
        cols = N - 1 if m == "column N - 1 of the column sum dropped" else N
        out[:cols] = val[:cols]
        return _lib.OK

    def colsum_finalize(self, dt, partial, rows, N, out, accumulate):
        self.ops.colsum_finalize(partial[:-1] if self.mutant == "one slab left out of colsum_finalize" else partial, out, bool(accumulate))
        return _lib.OK

    def embedding_fwd(self, dt, ids, table, vs, ve, x_in, pos_ids, pos_table, n_pos, out, slot, n_tok, h, p, seed, stream, out32):
        m = self.mutant
        if m == "position ids not clamped" and pos_ids is not None:
            pos_ids = pos_ids % n_pos                                      # wraps where the kernel clamps
        if m == "an id equal to vocab_end accepted" and ids is not None:
            ids = torch.where(ids == ve, ids - 1, ids)
        out.copy_(self.ops.embedding_fwd(ids, table, vs, pos_ids, pos_table, (p, seed, stream) if p else None, slot, x_in, bool(out32)))
        return _lib.OK

    def embedding_bwd(self, dt, dout, ids, dtable, vs, ve, pos_ids, dpos, n_pos, dx, n_tok, h, p, seed, stream, ws, ws_bytes, d32):
        drop = (p, seed, stream) if p else None
        self.ops.embedding_bwd(dout, None, None, vs, None, None, drop, dx)
        if self.mutant == "one occurrence of a repeated key dropped" and n_tok > 256:
            dout = dout.clone()
            dout[256] = 0
        self.ops.embedding_bwd(dout, ids, dtable, vs, pos_ids, dpos, drop, None)
        return _lib.OK

    def ce_fwd(self, dt, logits, target, vs, rows, v, rowmax, sumexp, predicted, loss):
        if self.mutant == "the CE target column off by one":
            target = target + 1
        r = self.ops.ce_fwd(logits, target, vs, loss is not None)
        for dst, val in zip((rowmax, sumexp, predicted, loss), r):
            if dst is not None:
                dst.copy_(val)
        return _lib.OK

    def ce_bwd(self, dt, logits, target, vs, rows, v, gmax, gsum, grad, dlogits):
        self.ops.ce_bwd(logits, target, vs, gmax, gsum, grad, out=dlogits)
        return _lib.OK

    def grad_stats(self, dt, grads, cs, cl, cn, nchunks, stats, ws, ws_bytes):
        self.ops.grad_stats(grads, cs, cl, cn, stats)
        return _lib.OK


# ------------------------------------------------------------------------------------------ flat element-wise
def gelu_terms(x):
    """fp64 sigmoid s = 1 / (1 + 2^t), its error in gelu_sigmoid_f and u2 = 2 u'(x) (common.cuh: gelu_f, gelu_grad_f)"""
    u2 = 2 * 0.7978845608028654 * (1 + 3 * 0.044715 * x * x)
    t = -2 * 0.7978845608028654 * x * (1 + 0.044715 * x * x)               # natural-log units: s = 1 / (1 + e^t)
    s = torch.sigmoid(-t)
    # the exp2: its argument x fma(K1, x^2, K0) carries the roundings of x^2, the fma, the product and of the two constants (5 e |t|),
    # v_exp_f32 itself one unit (2 e); through s = 1 / (1 + E) that is s (1 - s) times the relative error of E.
    # the rcp: the add 1 + E (e) and v_rcp_f32, one unit (2 e), relative to s
    ds = s * (1 - s) * (2 * E32 + 5 * E32 * t.abs()) + 3 * E32 * s
    return s, ds, u2


def flat_operands(op, n, dtype):
    g = _gen(FLAT_OPS.index(op), n, dtype == torch.bfloat16)
    c = SimpleNamespace(op=op, n=n, dtype=dtype, slot=False, p=0.0, scale=1.0, out_dt=dtype, bitwise=True, bound=None)
    idx = (FLAT_N + TAIL_N).index(n)
    if op in ("gelu_fwd", "gelu_bwd"):
        x = (3.0 * torch.randn(n, generator=g)).to(dtype).double()
        x[:8] = torch.tensor([0.0, -0.0, 10.0, -10.0, 0.5, -0.5, 4.0, -4.0], dtype=torch.float64)[:n]
        s, ds, u2 = gelu_terms(x)
        c.bitwise = False
        if op == "gelu_fwd":
            c.ins, c.ref = [(x, dtype)], O.gelu(x)
            # x s: ds, the product (e) and the 2e-7 |x| common.cuh states for the evaluation as a whole
            err = x.abs() * ds + E32 * c.ref.abs() + 2e-7 * x.abs()
        else:
            dy = torch.randn(n, generator=g).to(dtype).double()
            xr = x.clone().requires_grad_(True)
            O.gelu(xr).sum().backward()
            c.ins, c.ref = [(dy, dtype), (x, dtype)], dy * xr.grad
            # gelu' = fma(x fma(-s, s, s), fma(C1, x^2, C0), s): ds through s and through x s (1 - s) u2, the four roundings of the fmas
            # and of x^2 on each summand (4 e), then the product with dy (e)
            err = dy.abs() * (ds * (1 + x.abs() * u2) + 4 * E32 * (x.abs() * s * (1 - s) * u2 + s)) + E32 * c.ref.abs()
        c.bound = err + ulp(c.ref.abs() + err, dtype) / 2
    elif op == "dropout":
        x = spread(g, n, dtype)
        c.p, c.slot = 0.5, idx % 2 == 0
        c.ins, c.ref = [(x, dtype)], torch.where(keep_bool(n, 0.5), 2.0 * x, torch.zeros_like(x))
    elif op == "add":
        a, b = spread(g, n, dtype), spread(g, n, dtype)
        c.slot, c.ins, c.ref = idx % 2 == 1, [(a, dtype), (b, dtype)], a + b
    elif op == "scale":
        x = spread(g, n, dtype)
        c.scale = SCALES[idx]
        c.ins, c.ref = [(x, dtype)], x * c.scale
    elif op == "add_stream":
        # the fp32 stream: multiples of 2^-12 below 32 (18 significant bits, more than the 16-bit type holds); b at least 2^-2, so its
        # last place is a multiple of 2^-12 too and the fp32 sum is exact
        a, b = torch.randint(-2 ** 17 + 1, 2 ** 17, (n,), generator=g).double() * 2.0 ** -12, spread(g, n, dtype, lo=-2)
        c.slot, c.out_dt, c.ins, c.ref = idx % 2 == 0, F32, [(a, F32), (b, dtype)], a + b
    elif op == "cast_flat":
        x = (8.0 * torch.randn(n, generator=g)).to(dtype).double()
        c.out_dt, c.ins, c.ref = F32, [(x, dtype)], x
    elif op == "cast_flat_back":
        x = (8.0 * torch.randn(n, generator=g)).float().double()
        c.ins, c.ref = [(x, F32)], x
    return c


def flat_call(backend, c, ins, out, slot):
    dt, n, a = c.dtype, c.n, [g.view for g in ins]
    s = None if slot is None else slot.view
    if c.op in ("gelu_fwd", "cast_flat", "cast_flat_back"):
        return backend.call(c.op, dt, a[0], out.view, n)
    if c.op == "gelu_bwd":
        return backend.call(c.op, dt, a[0], a[1], out.view, n)
    if c.op == "dropout":
        return backend.call(c.op, dt, a[0], out.view, n, c.p, SEED, STREAM, s)
    if c.op == "scale":
        return backend.call(c.op, dt, a[0], out.view, n, c.scale)
    return backend.call(c.op, dt, a[0], a[1], out.view, n, s)              # add, add_stream


def run_flat(backend, op, n, dtype):
    """-> (failures, {(operation, output): err / bound})"""
    fails, ratios, dev = [], {}, backend.device
    c = flat_operands(op, n, dtype)
    ins = [_vec(t, dt, dev) for t, dt in c.ins]
    outputs = dict(out=_out((n,), c.out_dt, dev))
    if c.slot:
        outputs["absmax"] = _out((1,), F32, dev)
    cell = Cell(outputs, dict(absmax=torch.zeros(1)))                       # the kernels raise the slot with an atomic max

    def judge():
        got = outputs["out"].view.cpu()
        if c.bitwise:
            _judge_bits(fails, "out", got, round_to(c.ref, c.out_dt))
        else:
            _judge(fails, ratios, (op, "y" if op == "gelu_fwd" else "dx"), got.double(), c.ref, c.bound)
        if c.slot:                                                         # max |stored output|, exactly
            slot, want = float(outputs["absmax"].view[0]), float(got.double().abs().max())
            if slot != want:
                fails.append(f"absmax_out is {slot}, max |stored output| is {want}")
    _twice(cell, lambda: flat_call(backend, c, ins, outputs["out"], outputs.get("absmax")), fails, judge)
    return fails, ratios


def flat_sweep(backend, op, dtype):
    fails, worst = [], {}
    sizes = FLAT_N + (TAIL_N if op in TAILED else ())
    for n in sizes:
        bad, ratios = run_flat(backend, op, n, dtype)
        fails += [f"{op} {NAME[dtype]} n={n}: {b}" for b in bad]
        for k, r in ratios.items():
            worst[k] = max(worst.get(k, 0.0), r)
    return fails, len(sizes), worst


def absmax_cells(n, wide):
    """(variant, index, value) of the flat absmax cells of one size"""
    per = 4 if wide else 8
    cells = [("first", 0, 100.0), ("lastvec", n // per * per - 1, 100.0), ("nan", n // 2, float("nan")), ("neg", n // 3, -100.0)]
    if n // per == 0:
        cells = [c for c in cells if c[0] != "lastvec"]
    if n % per:
        cells += [("tail", n - 1, 100.0), ("nan", n - 1, float("nan"))]
    return cells


def absmax_sweep(backend, dtype):
    """cogv_absmax of a 16-bit (all eight sizes) or an fp32 tensor: the slot is max |x| exactly, NaN where x holds one"""
    fails, cells, dev, wide = [], 0, backend.device, dtype == F32
    for n in (ABSMAX32_N if wide else FLAT_N + TAIL_N):
        base = torch.randn(n, generator=_gen(71, n)).to(dtype)
        x, slot = _vec(base, dtype, dev), _out((1,), F32, dev)
        for variant, i, v in absmax_cells(n, wide):
            x.view[i] = v
            for again in (0, 1):
                slot.reset()
                slot.view[0] = 0.0
                rc = backend.call("absmax", dtype, x.view, n, slot.view)
                got = float(slot.view[0])
                want = float("nan") if v != v else max(float(base.double().abs().max()), abs(v))
                if rc != _lib.OK or not slot.intact() or not (got == want or (got != got and want != want)):
                    fails.append(f"absmax {NAME[dtype]} n={n} {variant}: rc {rc}, {got} for {want}, guards intact {slot.intact()}")
            x.view[i] = base[i]
            cells += 1
    return fails, cells


# ------------------------------------------------------------------------------------------ embedding forward
EDGE_IDS = (EMB_START - 1, EMB_START, EMB_START + EMB_ROWS - 1, EMB_START + EMB_ROWS)
EDGE_POS = (-1, EMB_NPOS, 0, EMB_NPOS - 1)


def emb_fwd_problem(shape, combo, dtype):
    n_tok, h = shape
    out32, use_ids, pos, drop, slot = combo
    si = EMB_FWD_SHAPES.index(shape)
    g = _gen(31, n_tok, h, dtype == torch.bfloat16)
    c = SimpleNamespace(shape=shape, combo=combo, dtype=dtype, n_tok=n_tok, h=h, out_dt=F32 if out32 else dtype, p=0.5 if drop else 0.0)
    c.table, c.pos_table, c.x_in = spread(g, (EMB_ROWS, h), dtype), spread(g, (EMB_NPOS, h), dtype), spread(g, (n_tok, h), dtype)
    c.ids = torch.randint(EMB_START - 4, EMB_START + EMB_ROWS + 4, (n_tok,), generator=g)
    c.pos_ids = torch.randint(0, EMB_NPOS, (n_tok,), generator=g)
    for i in range(min(n_tok, 4)):                                          # the edges: on the first tokens, rotated by the shape
        c.ids[i], c.pos_ids[i] = EDGE_IDS[(i + si) % 4], EDGE_POS[(i + si) % 4]
    if use_ids:
        local = c.ids - EMB_START
        ok = (local >= 0) & (local < EMB_ROWS)
        w = torch.where(ok[:, None], c.table[local.clamp(0, EMB_ROWS - 1)], torch.zeros((n_tok, h), dtype=torch.float64))
    else:
        w = c.x_in
    c.sum_exact = True
    if pos:
        w = w + c.pos_table[c.pos_ids.clamp(0, EMB_NPOS - 1)]
        c.sum_exact = exact_in_fp32(w)
        if not out32:
            w = round_to(w, dtype).double()                                 # a T + T add in the reference: rounded once
    if drop:
        w = torch.where(keep_bool(n_tok * h, 0.5).view(n_tok, h), 2.0 * w, torch.zeros_like(w))
    c.ref = w
    return c


def run_emb_fwd(backend, shape, combo, dtype):
    fails, dev = [], backend.device
    c = emb_fwd_problem(shape, combo, dtype)
    out32, use_ids, pos, drop, slot = combo
    table, pos_table, x_in = _vec(c.table, dtype, dev), _vec(c.pos_table, dtype, dev), _vec(c.x_in, dtype, dev)
    ids, pos_ids = c.ids.to(dev), c.pos_ids.to(dev)
    outputs = dict(out=_out(shape, c.out_dt, dev), absmax=_out((1,), F32, dev))
    cell = Cell(outputs, dict(absmax=torch.zeros(1)))

    def call():
        return backend.call("embedding_fwd", dtype, ids if use_ids else None, table.view if use_ids else None, EMB_START, EMB_START + EMB_ROWS,
                            None if use_ids else x_in.view, pos_ids if pos else None, pos_table.view if pos else None, EMB_NPOS,
                            outputs["out"].view, outputs["absmax"].view if slot else None, c.n_tok, c.h, c.p, SEED, STREAM, int(out32))

    def judge():
        got = outputs["out"].view.cpu()
        _judge_bits(fails, "out", got, round_to(c.ref, c.out_dt))
        have, want = float(outputs["absmax"].view[0]), float(got.double().abs().max()) if slot else 0.0
        if have != want:
            fails.append(f"absmax_out is {have}, expected {want} ({'max |stored output|' if slot else 'its pointer was NULL'})")
    _twice(cell, call, fails, judge)
    return fails


def emb_fwd_cells():
    return [(s, c) for s in EMB_FWD_SHAPES[:3] for c in EMB_FWD_CELLS] + [(EMB_FWD_SHAPES[3], c) for c in EMB_FWD_BIG_CELLS]


def emb_fwd_sweep(backend, dtype):
    fails = []
    for shape, combo in emb_fwd_cells():
        fails += [f"embedding_fwd {NAME[dtype]} (n_tok, h)={shape} (out32, ids, pos, dropout, absmax)={tuple(map(int, combo))}: {b}"
                  for b in run_emb_fwd(backend, shape, combo, dtype)]
    return fails, len(emb_fwd_cells())


# ------------------------------------------------------------------------------------------ embedding backward
def emb_keys(pattern, n_tok, rows, g):
    """local keys [n_tok] in [0, rows) (-1 / rows: outside the shard) of one pattern"""
    if pattern == "unique":
        return torch.randperm(rows, generator=g)[:n_tok]
    if pattern == "every":
        return torch.full((n_tok,), 3 % rows)
    if pattern == "outside":
        return torch.where(torch.arange(n_tok) % 2 == 0, -1, rows)
    keys = torch.randperm(rows, generator=g)[:n_tok]
    shared = keys[0].item()
    for t in WINDOW_TOKENS:
        if t < n_tok:
            keys[t] = shared
    return keys


def emb_bwd_cells(shape):
    """(pattern, kind, fp32 gradient, which tables, dropout): every pattern x kind x D32; the tables and dropout rotate"""
    si, cells = EMB_BWD_SHAPES.index(shape), []
    for pi, pattern in enumerate(EMB_PATTERNS):
        for ki, kind in enumerate(KINDS):
            for d32 in (0, 1):
                which = EMB_WHICH[(pi + ki + d32 + si) % 3]
                if pattern == "outside" and which == "dpos":
                    which = "both"                                          # (position ids are clamped: never outside)
                cells.append((pattern, kind, d32, which, (pi + d32) % 2 == 1))
    return cells


def emb_bwd_problem(shape, pattern, kind, d32, which, drop, dtype):
    n_tok, h = shape
    rows = n_tok + 5
    g = _gen(37, n_tok, h, EMB_PATTERNS.index(pattern), kind == "exact", d32)
    c = SimpleNamespace(shape=shape, pattern=pattern, kind=kind, d32=d32, which=which, dtype=dtype, n_tok=n_tok, h=h, rows=rows,
                        d_dt=F32 if d32 else dtype, p=0.0 if not drop else 0.5 if kind == "exact" else 0.1)
    keys = emb_keys(pattern, n_tok, rows, g)
    c.ids = keys + EMB_START
    pk = emb_keys(pattern, n_tok, rows, g)
    c.pos_ids = pk                                                          # -1 and `rows` are clamped to 0 and rows - 1
    if kind == "exact":
        c.dout = torch.randint(-1, 2, (n_tok, h), generator=g).double()
        c.init = {n: torch.randint(-8, 9, (rows, h), generator=g).double() for n in ("dtable", "dpos")}
    else:
        c.dout = torch.randn((n_tok, h), generator=g).to(c.d_dt).double()
        c.init = {n: torch.randn((rows, h), generator=g).to(dtype).double() for n in ("dtable", "dpos")}
    ks = keep_scale(c.p)
    c.masked = c.dout * ks * keep_bool(n_tok * h, c.p).view(n_tok, h).double() if c.p else c.dout
    c.local = {"dtable": keys, "dpos": pk.clamp(0, rows - 1)}
    c.ref, c.bound, c.count = {}, {}, {}
    for name in ("dtable", "dpos"):
        loc = c.local[name]
        ok = (loc >= 0) & (loc < rows)
        acc = torch.zeros((rows, h), dtype=torch.float64).index_add_(0, loc[ok], c.masked[ok])
        mag = torch.zeros((rows, h), dtype=torch.float64).index_add_(0, loc[ok], c.masked[ok].abs())
        cnt = torch.zeros(rows, dtype=torch.float64).index_add_(0, loc[ok], torch.ones(int(ok.sum()), dtype=torch.float64))
        ref = c.init[name] + acc
        # a key's rows are added in fp32 one after the other (cnt - 1 adds), then to the table row (one more): (cnt) e sum |terms|; the
        # masked gradient itself carries the rounded keep scale and the product (2 e); one rounding to T.  An untouched row: to the bit
        err = cnt[:, None] * E32 * (mag + c.init[name].abs()) + (2 * E32 * mag if c.p else 0.0)
        c.ref[name], c.count[name] = ref, cnt
        c.bound[name] = torch.where(cnt[:, None] > 0, err + ulp(ref.abs() + err, dtype) / 2, torch.zeros_like(ref))
    err = 2 * E32 * c.masked.abs() if c.p else torch.zeros_like(c.masked)
    c.ref["dx"], c.bound["dx"] = c.masked, err if d32 else err + ulp(c.masked.abs() + err, dtype) / 2
    return c


def run_emb_bwd(backend, c):
    fails, ratios, dev = [], {}, backend.device
    dout = _vec(c.dout, c.d_dt, dev)
    ids, pos_ids = c.ids.to(dev), c.pos_ids.to(dev)
    names = [n for n in ("dtable", "dpos") if c.which in (n, "both")]
    ws_bytes = _lib.lib().cogv_embedding_bwd_workspace_bytes(c.rows if "dtable" in names else 0, c.rows if "dpos" in names else 0)
    outputs = dict(dx=_out(c.shape, c.d_dt, dev), workspace=_out((ws_bytes // 4,), F32, dev))
    outputs.update({n: _out((c.rows, c.h), c.dtype, dev) for n in names})
    cell = Cell(outputs, {n: c.init[n] for n in names})
    tab = lambda n: outputs[n].view if n in names else None

    def call():
        return backend.call("embedding_bwd", c.dtype, dout.view, ids, tab("dtable"), EMB_START, EMB_START + c.rows, pos_ids, tab("dpos"), c.rows,
                            outputs["dx"].view, c.n_tok, c.h, c.p, SEED, STREAM, outputs["workspace"].view, ws_bytes, int(c.d32))

    def judge():
        for n in names + ["dx"]:
            got = outputs[n].view.cpu()
            if c.kind == "exact":
                _judge_bits(fails, n, got, round_to(c.ref[n], got.dtype))
            else:
                _judge(fails, ratios, ("embedding_bwd", n), got.double(), c.ref[n], c.bound[n])
            if n != "dx":
                idle = c.count[n] == 0
                if not torch.equal(bits(got[idle]), bits(c.init[n][idle].to(got.dtype))):
                    fails.append(f"{n}: a row no token points to was written")
    _twice(cell, call, fails, judge)
    return fails, ratios


def emb_bwd_sweep(backend, shape, dtype):
    fails, worst = [], {}
    for pattern, kind, d32, which, drop in emb_bwd_cells(shape):
        bad, ratios = run_emb_bwd(backend, emb_bwd_problem(shape, pattern, kind, d32, which, drop, dtype))
        fails += [f"embedding_bwd {NAME[dtype]} (n_tok, h)={shape} {pattern} {kind} D32={d32} {which} dropout={drop}: {b}" for b in bad]
        for k, r in ratios.items():
            worst[k] = max(worst.get(k, 0.0), r)
    return fails, len(emb_bwd_cells(shape)), worst


# ------------------------------------------------------------------------------------------ column sum
@functools.lru_cache(maxsize=None)
def steered_integers(seed, M, N):
    """integers of magnitude 1..2 whose sign opposes the running column sum: every prefix sum, the final one included, stays within +-2"""
    g = _gen(seed, M, N)
    mag = torch.randint(1, 3, (M, N), generator=g).double()
    coin = torch.randint(0, 2, (M, N), generator=g).double() * 2 - 1
    x, s = torch.empty((M, N), dtype=torch.float64), torch.zeros(N, dtype=torch.float64)
    for r in range(M):
        x[r] = torch.where(s == 0, coin[r], -torch.sign(s)) * mag[r]
        s += x[r]
    return x


@functools.lru_cache(maxsize=None)
def colsum_problem(shape, kind, accumulate, dtype):
    M, N, ld = shape
    g = _gen(41, M, N, ld, kind == "exact", accumulate)
    c = SimpleNamespace(shape=shape, kind=kind, accumulate=accumulate, dtype=dtype, M=M, N=N, ld=ld)
    if kind == "exact":
        c.x, c.init = steered_integers(41, M, N), torch.randint(-8, 9, (N,), generator=g).double()
    else:
        c.x, c.init = torch.randn((M, N), generator=g).to(dtype).double(), ((M ** 0.5) * torch.randn(N, generator=g)).to(dtype).double()
    c.ref = c.x.sum(0) + (c.init if accumulate else 0.0)
    # any order of M fp32 additions (four waves, the slabs, the final 8-way sums, `accumulate`): the summation length times 2^-24 times
    # the sum of magnitudes; one rounding to T
    err = (M + 2) * E32 * (c.x.abs().sum(0) + (c.init.abs() if accumulate else 0.0))
    c.bound = err + ulp(c.ref.abs() + err, dtype) / 2
    return c


def run_colsum(backend, c):
    fails, ratios, dev = [], {}, backend.device
    x = Guard(c.M, c.ld, c.dtype, nan=True, device=dev)                    # the pad columns N .. ld stay NaN
    x.view[:, :c.N] = c.x.to(c.dtype)
    ws_bytes = _lib.lib().cogv_colsum_workspace_bytes(c.M, c.N)
    outputs = dict(out=_out((c.N,), c.dtype, dev), workspace=_out((ws_bytes // 4,), F32, dev))
    cell = Cell(outputs, dict(out=c.init) if c.accumulate else {})

    def judge():
        got = outputs["out"].view.cpu()
        if c.kind == "exact":
            _judge_bits(fails, "out", got, round_to(c.ref, c.dtype))
        else:
            _judge(fails, ratios, ("colsum", "out"), got.double(), c.ref, c.bound)
    _twice(cell, lambda: backend.call("colsum", c.dtype, x.view, c.M, c.N, c.ld, outputs["out"].view, c.accumulate, outputs["workspace"].view,
                                      ws_bytes), fails, judge)
    return fails, ratios


def colsum_sweep(backend, dtype):
    fails, worst, cells = [], {}, 0
    for shape in COLSUM_SHAPES:
        for kind in KINDS:
            for accumulate in (0, 1):
                bad, ratios = run_colsum(backend, colsum_problem(shape, kind, accumulate, dtype))
                fails += [f"colsum {NAME[dtype]} (M, N, ld)={shape} {kind} accumulate={accumulate}: {b}" for b in bad]
                for k, r in ratios.items():
                    worst[k] = max(worst.get(k, 0.0), r)
                cells += 1
    return fails, cells, worst


@functools.lru_cache(maxsize=None)
def finalize_problem(rows, N, kind, dtype):
    g = _gen(43, rows, N, kind == "exact")
    c = SimpleNamespace(rows=rows, N=N, kind=kind, dtype=dtype, accumulate=(FINALIZE_ROWS.index(rows) + FINALIZE_N.index(N)) % 2)
    if kind == "exact":
        c.partial, c.init = steered_integers(43, rows, N), torch.randint(-8, 9, (N,), generator=g).double()
    else:
        c.partial, c.init = torch.randn((rows, N), generator=g).float().double(), torch.randn(N, generator=g).to(dtype).double()
    c.ref = c.partial.sum(0) + (c.init if c.accumulate else 0.0)
    err = (rows + 2) * E32 * (c.partial.abs().sum(0) + (c.init.abs() if c.accumulate else 0.0))   # summation length x 2^-24 x sum of magnitudes
    c.bound = err + ulp(c.ref.abs() + err, dtype) / 2
    return c


def run_finalize(backend, c):
    fails, ratios, dev = [], {}, backend.device
    partial = _vec(c.partial, F32, dev)
    outputs = dict(out=_out((c.N,), c.dtype, dev))
    cell = Cell(outputs, dict(out=c.init) if c.accumulate else {})

    def judge():
        got = outputs["out"].view.cpu()
        if c.kind == "exact":
            _judge_bits(fails, "out", got, round_to(c.ref, c.dtype))
        else:
            _judge(fails, ratios, ("colsum_finalize", "out"), got.double(), c.ref, c.bound)
    _twice(cell, lambda: backend.call("colsum_finalize", c.dtype, partial.view, c.rows, c.N, outputs["out"].view, c.accumulate), fails, judge)
    return fails, ratios


def finalize_sweep(backend, dtype):
    fails, worst, cells = [], {}, 0
    for rows in FINALIZE_ROWS:
        for N in FINALIZE_N:
            for kind in KINDS:
                bad, ratios = run_finalize(backend, finalize_problem(rows, N, kind, dtype))
                fails += [f"colsum_finalize {NAME[dtype]} rows={rows} N={N} {kind}: {b}" for b in bad]
                for k, r in ratios.items():
                    worst[k] = max(worst.get(k, 0.0), r)
                cells += 1
    return fails, cells, worst


# ------------------------------------------------------------------------------------------ cross entropy
def ce_logits(shape, tag, ldt):
    rows, v = shape
    g = _gen(47, rows, v, CE_DTYPES.index(ldt))
    l = (3.0 * torch.randn((rows, v), generator=g)).to(ldt).double()
    if tag == "maxlast":
        l[:, -1] = 17.0
    elif tag == "equal":
        l[:] = -2.5
    elif tag == "neginf":
        l[:, :8] = float("-inf")
    return l


def ce_targets(shape, tag):
    rows, v = shape
    if tag == "first":
        return torch.full((rows,), VOCAB_START)
    if tag == "last":
        return torch.full((rows,), VOCAB_START + v - 1)
    if tag == "below":
        return torch.full((rows,), VOCAB_START - 1)
    if tag == "above":
        return torch.full((rows,), VOCAB_START + v)
    return VOCAB_START + (torch.arange(rows) * 37 + v // 2) % v               # the special cells: inside (neginf: v // 2 >= 8)


def ce_reference(l, target, vocab_start):
    """fp64 rowmax, sumexp, predicted, loss of one shard (mpu/cross_entropy.py; the oracle's vocab_parallel_cross_entropy in double
    where the target lies inside) and the bounds of sumexp and loss from ce_fwd_kernel's operations"""
    rows, v = l.shape
    m = l.max(1).values
    d = l - m[:, None]
    term = d.exp()
    S = term.sum(1)
    t = target - vocab_start
    inside = (t >= 0) & (t < v)
    pred = torch.where(inside, l.gather(1, t.clamp(0, v - 1)[:, None])[:, 0], torch.zeros(rows, dtype=torch.float64))
    loss = S.log() + m - pred
    nv = (v // 8 + 255) // 256                                             # vectors of thread 0
    # __expf(x) = exp2(x log2 e): a term reaches the block's sum through exponents that add up to l - max (the subtractions and the
    # products with log2 e: 2 e |l - max|), through at most nv + 1 evaluations and rescalings (v_exp_f32 one unit, the product: 3 e each)
    # and its own addition; the length of the sum: 8 nv additions of a thread, six DPP steps, four waves: (8 nv + 10) e S
    dabs = torch.where(term > 0, d.abs(), torch.zeros_like(d))
    dS = (term * E32 * (2 * dabs + 3 * (nv + 1) + 2)).sum(1) + (8 * nv + 10) * E32 * S
    # loss = logf(gs) + gm - pl: gs's error through the log, logf (one unit), the two additions
    dloss = dS / S + 2 * E32 * S.log().abs() + E32 * (S.log() + m).abs() + E32 * loss.abs()
    return dict(rowmax=m, sumexp=S, predicted=pred, loss=loss), dict(sumexp=dS, loss=dloss)


def run_ce_fwd(backend, shape, tag, ldt):
    fails, ratios, dev = [], {}, backend.device
    rows, v = shape
    l, target = ce_logits(shape, tag, ldt), ce_targets(shape, tag)
    ref, bound = ce_reference(l, target, VOCAB_START)
    logits, tgt = _vec(l, ldt, dev), target.to(dev)
    outputs = {n: _out((rows,), F32, dev) for n in ("rowmax", "sumexp", "predicted", "loss")}
    cell = Cell(outputs)
    want_loss = tag != "noloss"

    def judge():
        for n in ("rowmax", "predicted"):
            _judge_bits(fails, n, outputs[n].view.cpu(), ref[n].float())
        _judge(fails, ratios, ("ce_fwd", "sumexp"), outputs["sumexp"].view.cpu().double(), ref["sumexp"], bound["sumexp"])
        if want_loss:
            _judge(fails, ratios, ("ce_fwd", "loss"), outputs["loss"].view.cpu().double(), ref["loss"], bound["loss"])
        elif not outputs["loss"].untouched():
            fails.append("loss written although its pointer was NULL")
    _twice(cell, lambda: backend.call("ce_fwd", ldt, logits.view, tgt, VOCAB_START, rows, v, outputs["rowmax"].view, outputs["sumexp"].view,
                                      outputs["predicted"].view, outputs["loss"].view if want_loss else None), fails, judge)
    return fails, ratios


def ce_bwd_reference(l, target, vocab_start, gmax, gsum, grad, ldt):
    """fp64 dlogits = grad (exp(l - gmax) / gsum - [column == target]) on gmax, gsum as given (fp32 values) and ce_bwd_kernel's bound"""
    rows, v = l.shape
    d = l - gmax[:, None]
    p = d.exp() / gsum[:, None]
    t = target - vocab_start
    hot = (torch.arange(v)[None, :] == t[:, None]).double()
    ref = (p - hot) * grad[:, None]
    dabs = torch.where(p > 0, d.abs(), torch.zeros_like(d))
    # __expf: the subtraction and the product with log2 e (2 e |l - gmax|), v_exp_f32 (2 e); 1 / gsum (e) and the product (e); the
    # subtraction of 1 (e) and the product with grad (e)
    err = grad.abs()[:, None] * (p * E32 * (2 * dabs + 4) + E32 * (p - hot).abs()) + E32 * ref.abs()
    return ref, err if ldt == F32 else err + ulp(ref.abs() + err, ldt) / 2


def run_ce_bwd(backend, shape, tag, ldt):
    fails, ratios, dev = [], {}, backend.device
    rows, v = shape
    l, target = ce_logits(shape, tag, ldt), ce_targets(shape, tag)
    fwd, _ = ce_reference(l, target, VOCAB_START)
    gmax, gsum = fwd["rowmax"].float().double(), fwd["sumexp"].float().double()      # the fp64 reference rounded to fp32
    grad = torch.tensor([0.0, 1.0, -0.375][:rows] if rows > 1 else [0.625], dtype=torch.float64)
    ref, bound = ce_bwd_reference(l, target, VOCAB_START, gmax, gsum, grad, ldt)
    logits, tgt = _vec(l, ldt, dev), target.to(dev)
    ins = [_vec(t, F32, dev) for t in (gmax, gsum, grad)]
    outputs = dict(dlogits=_out(shape, ldt, dev))
    cell = Cell(outputs)
    _twice(cell, lambda: backend.call("ce_bwd", ldt, logits.view, tgt, VOCAB_START, rows, v, ins[0].view, ins[1].view, ins[2].view, outputs["dlogits"].view),
           fails, lambda: _judge(fails, ratios, ("ce_bwd", "dlogits"), outputs["dlogits"].view.cpu().double(), ref, bound))
    return fails, ratios


def run_ce_two_shards(backend, ldt):
    """two shards of (3, 2056) combined as mpu/cross_entropy.py combines them (MAX of the maxima, SUM of the rescaled sums, SUM of the
    predicted logits), judged against the fp64 loss over the whole vocabulary"""
    fails, ratios, dev = [], {}, backend.device
    rows, v = 3, 2056
    l = (3.0 * torch.randn((rows, 2 * v), generator=_gen(53, CE_DTYPES.index(ldt)))).to(ldt).double()
    target = VOCAB_START + torch.tensor([5, v - 1, v + 9])                  # first shard, its last column, second shard
    lw = l - l.max(1, keepdim=True).values
    whole = lw.exp().sum(1).log() - lw.gather(1, (target - VOCAB_START)[:, None])[:, 0]
    got, rel = [], torch.zeros(rows, dtype=torch.float64)
    for s in range(2):
        shard = l[:, s * v:(s + 1) * v].contiguous()
        ref, bound = ce_reference(shard, target, VOCAB_START + s * v)
        logits, tgt = _vec(shard, ldt, dev), target.to(dev)
        outputs = {n: _out((rows,), F32, dev) for n in ("rowmax", "sumexp", "predicted")}
        rc = backend.call("ce_fwd", ldt, logits.view, tgt, VOCAB_START + s * v, rows, v, outputs["rowmax"].view, outputs["sumexp"].view,
                          outputs["predicted"].view, None)
        if rc != _lib.OK or any(not g.intact() for g in outputs.values()):
            fails.append(f"shard {s}: the call answers {rc} or wrote a guard")
        got.append({n: g.view.cpu().double() for n, g in outputs.items()})
        rel = torch.maximum(rel, bound["sumexp"] / ref["sumexp"])
    gmax = torch.maximum(got[0]["rowmax"], got[1]["rowmax"])
    gsum = sum(o["sumexp"] * (o["rowmax"] - gmax).exp() for o in got)
    loss = gsum.log() - (got[0]["predicted"] + got[1]["predicted"] - gmax)
    _judge(fails, ratios, ("ce_fwd", "loss2"), loss, whole, rel + 1e-12)       # each shard's sum within its own relative bound
    return fails, ratios


def ce_cells():
    return [(s, t) for s in CE_SHAPES for t in CE_TARGETS] + [((3, 2056), "noloss"), ((3, 96), "maxlast"), ((2, 4104), "maxlast"),
                                                              ((3, 2056), "equal"), (NEGINF_SHAPE, "neginf")]


def ce_sweep(backend, ldt):
    fails, worst = [], {}
    for shape, tag in ce_cells():
        for run in (run_ce_fwd, run_ce_bwd):
            bad, ratios = run(backend, shape, tag, ldt)
            fails += [f"{run.__name__[4:]} {NAME[ldt]} (rows, v_local)={shape} {tag}: {b}" for b in bad]
            for k, r in ratios.items():
                worst[k] = max(worst.get(k, 0.0), r)
    bad, ratios = run_ce_two_shards(backend, ldt)
    fails += [f"ce two shards {NAME[ldt]}: {b}" for b in bad]
    worst.update(ratios)
    return fails, 2 * len(ce_cells()) + 1, worst


# ------------------------------------------------------------------------------------------ gradient statistics and AdamW
@functools.lru_cache(maxsize=None)
def chunk_table(name):
    """(starts, lengths, groups, counted in the norm, elements): starts are multiples of 8, the gaps belong to no chunk"""
    if name == "lens":
        lens = list(TABLE_LENS)
    else:
        n = STATS_CHUNKS if name == "stats" else ADAM_CHUNKS
        lens = torch.randint(8, 41, (n,), generator=_gen(59, n)).tolist()
    starts, at = [], 0
    for n in lens:
        starts.append(at)
        at = (at + n + 7) // 8 * 8 + (8 if len(starts) % 3 == 0 else 0)
    groups = [0 if i % 2 == 0 else 7 for i in range(len(lens))]
    counted = [0 if i == 2 else 1 for i in range(len(lens))]
    return (torch.tensor(starts, dtype=torch.int64), torch.tensor(lens, dtype=torch.int32), torch.tensor(groups, dtype=torch.uint8),
            torch.tensor(counted, dtype=torch.uint8), at)


def chunk_mask(table):
    starts, lens, _, _, total = table
    m = torch.zeros(total, dtype=torch.bool)
    for s, n in zip(starts.tolist(), lens.tolist()):
        m[s:s + n] = True
    return m


@functools.lru_cache(maxsize=None)
def grads_of(name, gdt, scale=1.0):
    table = chunk_table(name)
    g = (0.1 * scale * torch.randn(table[4], generator=_gen(61, table[4], CE_DTYPES.index(gdt)))).to(gdt).double()
    return g, chunk_mask(table)


def sumsq_reference(name, gdt, scale=1.0):
    """fp64 sum of squares over the counted chunks and grad_stats_kernel's bound"""
    starts, lens, _, counted, _ = chunk_table(name)
    g, _ = grads_of(name, gdt, scale)
    tot = sum(float((g[s:s + n] ** 2).sum()) for s, n, c in zip(starts.tolist(), lens.tolist(), counted.tolist()) if c)
    # a thread's chain: 8 squares per vector, ceil(len / 2048) vectors, a tail element, the chunks of its workgroup; block_sum: six DPP steps
    # and four waves; each square one rounding: (chain + 11) e sum g^2.  The partials are added in double
    chain = 8 * ((int(lens.max()) + 2047) // 2048) + 1 + chunk_passes(len(lens), 2048)[1]
    return tot, (chain + 11) * E32 * tot + 1e-15 * tot


def run_grad_stats(backend, name, gdt, poison=None):
    """poison: (chunk index, value) put into the scalar tail of that chunk -> stats[1] must be 1"""
    fails, ratios, dev = [], {}, backend.device
    starts, lens, _, counted, total = chunk_table(name)
    g, mask = grads_of(name, gdt)
    g = torch.where(mask, g, torch.full_like(g, float("nan")))              # the gaps belong to no chunk: NaN
    if poison is not None:
        ci, val = poison
        assert int(lens[ci]) % 8
        g[int(starts[ci]) + int(lens[ci]) - 1] = val
    grads = _vec(g, gdt, dev)
    tabs = [t.to(dev) for t in (starts, lens, counted)]
    ws_bytes = _lib.lib().cogv_grad_stats_workspace_bytes()
    outputs = dict(stats=_out((4,), F32, dev), workspace=_out((ws_bytes // 4,), F32, dev))
    cell = Cell(outputs, dict(stats=torch.tensor([3.0, 0.0], dtype=torch.float64)))       # stats[0] is added to
    ref, bound = sumsq_reference(name, gdt)

    def judge():
        st = _f64(outputs["stats"]).cpu()
        if poison is not None:
            if float(st[1]) != 1.0:
                fails.append(f"stats[1] is {float(st[1])} with {poison[1]} in the tail of chunk {poison[0]}")
            return
        if float(st[1]) != 0.0:
            fails.append(f"stats[1] is {float(st[1])} on finite gradients")
        _judge(fails, ratios, ("grad_stats", "sumsq"), st[:1], torch.tensor([3.0 + ref], dtype=torch.float64), torch.tensor([bound], dtype=torch.float64))
    _twice(cell, lambda: backend.call("grad_stats", gdt, grads.view, tabs[0], tabs[1], tabs[2], len(lens), _f64(outputs["stats"]),
                                      outputs["workspace"].view, ws_bytes), fails, judge)
    return fails, ratios


def grad_stats_sweep(backend, gdt):
    fails, worst, cells = [], {}, 0
    for name, poison in (("lens", None), ("stats", None), ("lens", OVERFLOWS[0]), ("lens", OVERFLOWS[1])):
        bad, ratios = run_grad_stats(backend, name, gdt, poison)
        fails += [f"grad_stats {NAME[gdt]} table {name} poison {poison}: {b}" for b in bad]
        worst.update({k: max(worst.get(k, 0.0), r) for k, r in ratios.items()})
        cells += 1
    return fails, cells, worst


def adam_args(cellname, step, name, dtype):
    """the descriptor's scalars of one cell, and the sum of squares AdamW is handed (the fp64 reference's)"""
    o = dict(max_norm=None, adam_w_mode=1, bias_correction=1, inv_loss_scale=1.0, override=False)
    o.update(ADAM_CELLS[cellname])
    scale = 1.0 / o["inv_loss_scale"]                                       # the gradients carry the loss scale
    ss, _ = sumsq_reference(name, dtype, scale)
    norm = math.sqrt(ss) * o["inv_loss_scale"]
    o["max_grad_norm"] = 0.0 if o["max_norm"] is None else 0.5 * norm if o["max_norm"] == "below" else 2.0 * norm
    o.update(sumsq=ss, scale=scale, step=step)
    return o


def adam_reference(g, w, m, v, table, o):
    """fp64 AdamW (apex FusedAdam; decoupled mode with bias correction is oracle.adamw_step) and the bound of each fp32 state tensor
    from adamw_kernel's operations, e = 2^-24"""
    starts, lens, groups, _, total = table
    e = E32
    gs, dgs = o["inv_loss_scale"], 0.0
    if o["max_grad_norm"] > 0:
        coef = o["max_grad_norm"] / (math.sqrt(o["sumsq"]) * o["inv_loss_scale"] + 1e-6)
        if coef < 1:
            gs, dgs = gs * coef, 6 * e      # (float) ss, sqrtf, x inv_scale, + 1e-6, the division, gscale x coef: one rounding each
    bc1 = 1 - BETA1 ** o["step"] if o["bias_correction"] else 1.0
    bc2 = 1 - BETA2 ** o["step"] if o["bias_correction"] else 1.0
    lr, wd = torch.zeros(total, dtype=torch.float64), torch.zeros(total, dtype=torch.float64)
    for s, n, grp in zip(starts.tolist(), lens.tolist(), groups.tolist()):
        lr[s:s + n], wd[s:s + n] = float(torch.tensor(LR[grp], dtype=F32)), float(torch.tensor(WD[grp], dtype=F32))   # the descriptor holds floats
    gr = g * gs
    dgr = gr.abs() * (dgs + e)                                              # g x gscale
    if not o["adam_w_mode"]:
        gr = gr + wd * w
        dgr = dgr + e * (wd * w).abs() + e * gr.abs()                       # L2: the product wd w and the add
    m1 = BETA1 * m + (1 - BETA1) * gr
    # beta1 and 1 - beta1 as floats (e each), the two products (e each), omb1 x gr's own error, the add
    dm = 2 * e * (BETA1 * m).abs() + 2 * e * ((1 - BETA1) * gr).abs() + (1 - BETA1) * dgr + e * m1.abs()
    v1 = BETA2 * v + (1 - BETA2) * gr * gr
    # the same for beta2 with two products on the new term, gr's error twice
    dv = 2 * e * (BETA2 * v).abs() + 3 * e * (1 - BETA2) * gr * gr + 2 * (1 - BETA2) * gr.abs() * dgr + e * v1
    root = (v1 / bc2).sqrt()
    denom = root + ADAM_EPS
    # sqrtf(v) (e, and v's error halved), 1 / sqrtf(bc2) (bc2 as a float, sqrtf, the division: 3 e), their product (e), eps as a float, the add
    safe = torch.where(v1 > 0, v1, torch.ones_like(v1))
    ddenom = root * (0.5 * dv / safe + 5 * e) + e * ADAM_EPS + e * denom
    upd = (m1 / bc1) / denom
    # 1 / bc1 (bc1 as a float, the division: 2 e), the product, the division (e each); m's and the denominator's errors
    dupd = (dm / bc1) / denom + upd.abs() * (4 * e + ddenom / denom)
    if o["adam_w_mode"]:
        upd = upd + wd * w
        dupd = dupd + e * (wd * w).abs() + e * upd.abs()                    # decoupled: the product wd w and the add
    w1 = w - lr * upd
    dw = lr * dupd + e * (lr * upd).abs() + e * w1.abs()                    # lr x upd and the subtraction
    live = chunk_mask(table)
    keep = lambda new, old, d: (torch.where(live, new, old), torch.where(live, d, torch.zeros_like(d)))
    return dict(zip(("master", "exp_avg", "exp_avg_sq"), (keep(w1, w, dw), keep(m1, m, dm), keep(v1, v, dv))))


def adam_state(name, step, dtype):
    table = chunk_table(name)
    total = table[4]
    g = _gen(67, total, step)
    w = torch.randn(total, generator=g).float().double()
    if step == 1:
        return w, torch.zeros(total, dtype=torch.float64), torch.zeros(total, dtype=torch.float64)
    return w, (0.1 * torch.randn(total, generator=g)).float().double(), (0.01 * torch.rand(total, generator=g)).float().double()


def run_adamw(backend, cellname, step, name, dtype, poison=None):
    """poison: (chunk index, value) in the scalar tail of that chunk and stats[1] == 1, as cogv_grad_stats leaves it: the step is skipped"""
    fails, ratios, dev = [], {}, backend.device
    table = chunk_table(name)
    starts, lens, groups, counted, total = table
    o = adam_args(cellname, step, name, dtype)
    g, mask = grads_of(name, dtype, o["scale"])
    w, m, v = adam_state(name, step, dtype)
    gd = torch.where(mask, g, torch.full_like(g, float("nan")))
    if poison:
        gd[int(starts[poison[0]]) + int(lens[poison[0]]) - 1] = poison[1]
    grads = _vec(gd, dtype, dev)
    tabs = [t.to(dev) for t in (starts, lens, groups)]
    outputs = dict(params=_out((total,), dtype, dev), master=_out((total,), F32, dev), exp_avg=_out((total,), F32, dev),
                   exp_avg_sq=_out((total,), F32, dev))
    init = dict(params=w.to(dtype), master=w.float(), exp_avg=m.float(), exp_avg_sq=v.float())
    cell = Cell(outputs, init)
    # stats[0]: the reference's sum of squares -- or, with the override, a number that would not clip
    stats = _vec(torch.tensor([o["sumsq"] * (1e-6 if o["override"] else 1.0), 1.0 if poison else 0.0], dtype=torch.float64).view(F32), F32, dev)
    over = _vec(torch.tensor([o["sumsq"]], dtype=torch.float64).view(F32), F32, dev) if o["override"] else None
    lrs, wds = [0.0] * 8, [0.0] * 8
    for grp in (0, 7):
        lrs[grp], wds[grp] = LR[grp], WD[grp]
    a = dict(dtype=dtype, grads=grads.view, chunk_start=tabs[0], chunk_len=tabs[1], chunk_group=tabs[2], nchunks=len(lens), lr=lrs, weight_decay=wds,
             beta1=BETA1, beta2=BETA2, eps=ADAM_EPS, step=step, bias_correction=o["bias_correction"], adam_w_mode=o["adam_w_mode"],
             beta1_d=BETA1, beta2_d=BETA2, inv_loss_scale=o["inv_loss_scale"], max_grad_norm=o["max_grad_norm"],
             stats=_f64(stats) if o["max_norm"] is not None or poison else None, norm_sumsq_override=None if over is None else _f64(over),
             **{n: outputs[n].view for n in outputs})

    def judge():
        got = {n: outputs[n].view.cpu() for n in outputs}
        if poison:                                                          # overflow: the whole step is skipped
            for n in outputs:
                if not torch.equal(bits(got[n]), bits(init[n])):
                    fails.append(f"{n} changed although stats[1] == 1")
            return
        ref = adam_reference(g, w, m, v, table, o)
        for n, (want, bound) in ref.items():
            _judge(fails, ratios, ("adamw", n), got[n].double(), want, bound)
        # params == round_T(master) in the chunks, untouched outside them
        _judge_bits(fails, "params", got["params"], torch.where(mask, got["master"].to(dtype), init["params"]))
    _twice(cell, lambda: backend.adamw(a), fails, judge)
    return fails, ratios


def adam_cells():
    """(cell, step, chunk table, overflow: (chunk, value) in its scalar tail)"""
    cells = [(c, s, "lens", None) for c in ADAM_CELLS for s in ADAM_STEPS]
    return cells + [("clip", 2, "adam", None), ("plain", 1, "adam", None), ("plain", 2, "lens", OVERFLOWS[0]), ("clip", 1, "lens", OVERFLOWS[1])]


def adam_sweep(backend, dtype):
    fails, worst = [], {}
    for cellname, step, name, poison in adam_cells():
        bad, ratios = run_adamw(backend, cellname, step, name, dtype, poison)
        fails += [f"adamw {NAME[dtype]} {cellname} step {step} table {name}{f' overflow {poison}' if poison else ''}: {b}" for b in bad]
        worst.update({k: max(worst.get(k, 0.0), r) for k, r in ratios.items()})
    return fails, len(adam_cells()), worst


# ------------------------------------------------------------------------------------------ refusals (no launch: they run without a device)
P = [0x10000 * (i + 1) for i in range(12)]                                 # 16-byte-aligned stand-ins that nothing reads
H = CODE[torch.float16]
REFUSAL_BASE = {
    "gelu_fwd": dict(dtype=H, x=P[0], y=P[1], n=64),
    "gelu_bwd": dict(dtype=H, dy=P[0], x=P[1], dx=P[2], n=64),
    "dropout": dict(dtype=H, x=P[0], y=P[1], n=64, p=0.1, seed=1, stream_id=2, absmax_out=None),
    "add": dict(dtype=H, a=P[0], b=P[1], out=P[2], n=64, absmax_out=None),
    "scale": dict(dtype=H, x=P[0], y=P[1], n=64, scale=0.5),
    "add_stream": dict(dtype=H, a=P[0], b=P[1], out=P[2], n=64, absmax_out=None),
    "absmax": dict(dtype=H, x=P[0], n=64, out=P[1]),
    "colsum_finalize": dict(dtype=H, partial=P[0], rows=4, N=8, out=P[1], accumulate=0),
    "colsum": dict(dtype=H, dy=P[0], M=300, N=16, ld=16, out=P[1], accumulate=0, workspace=P[2], workspace_bytes=2 * 16 * 4),
    "embedding_fwd": dict(dtype=H, ids=P[0], table=P[1], vocab_start=0, vocab_end=16, x_in=None, pos_ids=P[2], pos_table=P[3], n_pos=4, out=P[4],
                          absmax_out=None, n_tok=4, h=8, dropout_p=0.1, seed=1, stream_id=2, out_f32=0),
    "embedding_bwd": dict(dtype=H, dout=P[0], ids=P[1], dtable=P[2], vocab_start=0, vocab_end=16, pos_ids=P[3], dpos=P[4], n_pos=4, dx=P[5],
                          n_tok=4, h=8, dropout_p=0.1, seed=1, stream_id=2, workspace=P[6], workspace_bytes=(16 + 4) * 8, dout_f32=0),
    "ce_fwd": dict(logits_dtype=H, logits=P[0], target=P[1], vocab_start=0, rows=2, v_local=8, rowmax=P[2], sumexp=P[3], predicted=P[4], loss=P[5]),
    "ce_bwd": dict(logits_dtype=H, logits=P[0], target=P[1], vocab_start=0, rows=2, v_local=8, gmax=P[2], gsum=P[3], grad=P[4], dlogits=P[5]),
    "grad_stats": dict(dtype=H, grads=P[0], chunk_start=P[1], chunk_len=P[2], chunk_norm=P[3], nchunks=1, stats=P[4], workspace=P[5],
                       workspace_bytes=2048 * 8),
    "cast_flat": dict(dtype=H, src_half=P[0], dst_f32=P[1], n=8),
    "cast_flat_back": dict(dtype=H, src_f32=P[0], dst_half=P[1], n=8),
    "adamw_step": dict(dtype=H, params=P[0], grads=P[1], master=P[2], exp_avg=P[3], exp_avg_sq=P[4], chunk_start=P[5], chunk_len=P[6], chunk_group=P[7],
                       nchunks=1, step=1),
}
A_, U_ = _lib.ERR_ARG, _lib.ERR_UNSUPPORTED
_EW = lambda op, ptrs: ([(op, dict(dtype=_lib.F32), U_), (op, dict(dtype=7), U_), (op, dict(n=60), A_)]
                        + [(op, {k: None}, A_) for k in ptrs] + [(op, {k: REFUSAL_BASE[op][k] + 8}, A_) for k in ptrs])
REFUSALS = tuple(
    _EW("gelu_fwd", ("x", "y")) + _EW("gelu_bwd", ("dy", "x", "dx")) + _EW("dropout", ("x", "y")) + _EW("add", ("a", "b", "out"))
    + _EW("scale", ("x", "y")) + _EW("add_stream", ("a", "b", "out"))
    + [("dropout", dict(p=1.0), A_), ("dropout", dict(p=-0.25), A_), ("dropout", dict(p=float("nan")), A_)]
    + [("absmax", dict(dtype=7), U_), ("absmax", dict(x=None), A_), ("absmax", dict(out=None), A_), ("absmax", dict(n=0), A_),
       ("absmax", dict(x=P[0] + 8), A_), ("absmax", dict(dtype=_lib.F32, n=6), A_)]
    + [("colsum_finalize", dict(dtype=_lib.F32), U_), ("colsum_finalize", dict(partial=None), A_), ("colsum_finalize", dict(out=None), A_),
       ("colsum_finalize", dict(rows=0), A_), ("colsum_finalize", dict(N=0), A_)]
    + [("colsum", dict(dtype=_lib.F32), U_), ("colsum", dict(M=0), A_), ("colsum", dict(N=0), A_), ("colsum", dict(N=12), A_), ("colsum", dict(ld=20), A_),
       ("colsum", dict(dy=None), A_), ("colsum", dict(out=None), A_), ("colsum", dict(workspace=None), A_),
       ("colsum", dict(workspace_bytes=2 * 16 * 4 - 1), A_), ("colsum", dict(dy=P[0] + 8), A_)]
    + [("embedding_fwd", dict(dtype=_lib.F32), U_), ("embedding_fwd", dict(n_tok=0), A_), ("embedding_fwd", dict(h=0), A_), ("embedding_fwd", dict(h=12), A_),
       ("embedding_fwd", dict(out=None), A_), ("embedding_fwd", dict(ids=None), A_), ("embedding_fwd", dict(table=None), A_),
       ("embedding_fwd", dict(pos_ids=None), A_), ("embedding_fwd", dict(n_pos=0), A_), ("embedding_fwd", dict(dropout_p=1.0), A_),
       ("embedding_fwd", dict(dropout_p=-0.5), A_), ("embedding_fwd", dict(table=P[1] + 8), A_), ("embedding_fwd", dict(ids=None, x_in=P[5] + 8), A_),
       ("embedding_fwd", dict(pos_table=P[3] + 8), A_), ("embedding_fwd", dict(out=P[4] + 8), A_)]
    + [("embedding_bwd", dict(dtype=_lib.F32), U_), ("embedding_bwd", dict(n_tok=0), A_), ("embedding_bwd", dict(n_tok=2 ** 31 - 1), A_),
       ("embedding_bwd", dict(h=0), A_), ("embedding_bwd", dict(h=12), A_), ("embedding_bwd", dict(dout=None), A_), ("embedding_bwd", dict(ids=None), A_),
       ("embedding_bwd", dict(vocab_end=0), A_), ("embedding_bwd", dict(pos_ids=None), A_), ("embedding_bwd", dict(n_pos=0), A_),
       ("embedding_bwd", dict(dropout_p=1.0), A_), ("embedding_bwd", dict(dropout_p=-0.5), A_), ("embedding_bwd", dict(dout=P[0] + 8), A_),
       ("embedding_bwd", dict(dtable=P[2] + 8), A_), ("embedding_bwd", dict(dpos=P[4] + 8), A_), ("embedding_bwd", dict(dx=P[5] + 8), A_),
       ("embedding_bwd", dict(workspace=P[6] + 8), A_), ("embedding_bwd", dict(workspace=None), A_),
       ("embedding_bwd", dict(workspace_bytes=(16 + 4) * 8 - 1), A_)]
    + [(op, kw, code) for op, outs in (("ce_fwd", ("rowmax", "sumexp", "predicted")), ("ce_bwd", ("gmax", "gsum", "grad", "dlogits")))
       for kw, code in [(dict(logits_dtype=7), U_), (dict(rows=0), A_), (dict(v_local=0), A_), (dict(v_local=12), A_), (dict(logits=None), A_),
                        (dict(target=None), A_), (dict(logits=P[0] + 8), A_)] + [({k: None}, A_) for k in outs]]
    + [("ce_bwd", dict(dlogits=P[5] + 8), A_)]
    + [("grad_stats", dict(dtype=7), U_), ("grad_stats", dict(grads=None), A_), ("grad_stats", dict(chunk_start=None), A_),
       ("grad_stats", dict(chunk_len=None), A_), ("grad_stats", dict(chunk_norm=None), A_), ("grad_stats", dict(nchunks=0), A_),
       ("grad_stats", dict(stats=None), A_), ("grad_stats", dict(grads=P[0] + 8), A_), ("grad_stats", dict(workspace=None), A_),
       ("grad_stats", dict(workspace=P[5] + 4), A_), ("grad_stats", dict(workspace_bytes=2048 * 8 - 1), A_)]
    + [(op, kw, code) for op, (s, d) in (("cast_flat", ("src_half", "dst_f32")), ("cast_flat_back", ("src_f32", "dst_half")))
       for kw, code in [(dict(dtype=_lib.F32), U_), ({s: None}, A_), ({d: None}, A_), (dict(n=0), A_), ({s: P[0] + 8}, A_), ({d: P[1] + 8}, A_)]]
    + [("adamw_step", dict(dtype=_lib.F32), U_), ("adamw_step", dict(nchunks=0), A_), ("adamw_step", dict(step=0), A_)]
    + [("adamw_step", {k: None}, A_) for k in ("params", "grads", "master", "exp_avg", "exp_avg_sq", "chunk_start", "chunk_len", "chunk_group")]
    + [("adamw_step", {k: REFUSAL_BASE["adamw_step"][k] + 8}, A_) for k in ("params", "grads", "master", "exp_avg", "exp_avg_sq")]
)


def refuse(entry, kw):
    """the code the real entry point answers for its valid base arguments with `kw` on top (None stream; nothing is launched)"""
    a = {**REFUSAL_BASE[entry], **kw}
    if entry == "adamw_step":
        d = _lib.AdamDesc()
        for k, v in a.items():
            setattr(d, k, v)
        d.beta1 = d.beta1_d = 0.9
        d.beta2 = d.beta2_d = 0.95
        return _lib.lib().cogv_adamw_step(C.byref(d), None)
    return getattr(_lib.lib(), "cogv_" + entry)(*a.values(), None)


def run_mutant_cell(backend, name, dtype):
    """the failures of the cell named for one mutant under `backend`"""
    kind, cell = MUTANTS[name]
    if kind == "flat":
        return run_flat(backend, cell[0], cell[1], dtype)[0]
    if kind == "emb_fwd":
        assert cell in emb_fwd_cells()
        return run_emb_fwd(backend, cell[0], cell[1], dtype)
    if kind == "emb_bwd":
        shape, pattern, k, d32 = cell
        which, drop = next((w, d) for p, kk, dd, w, d in emb_bwd_cells(shape) if (p, kk, dd) == (pattern, k, d32))
        return run_emb_bwd(backend, emb_bwd_problem(shape, pattern, k, d32, which, drop, dtype))[0]
    if kind == "colsum":
        return run_colsum(backend, colsum_problem(cell[0], cell[1], cell[2], dtype))[0]
    if kind == "finalize":
        return run_finalize(backend, finalize_problem(cell[0], cell[1], cell[2], dtype))[0]
    if kind == "ce":
        assert cell in ce_cells()
        return run_ce_fwd(backend, cell[0], cell[1], dtype)[0]
    assert (cell[0], cell[1], "lens", None) in adam_cells()
    return run_adamw(backend, cell[0], cell[1], "lens", dtype)[0]
