"""Shared body of the Sandwich-LN cell sweep (cogview_amd/csrc/layernorm.hip: ln_fwd_kernel NV 1..8 x 3 stream modes, the twelve
forms of ln_bwd_kernel, ln_bwd_pair_kernel, ln_bwd_reduce_kernel): the shape grids (tests/test_layernorm_cells_cpu.py proves on the
CPU that they reach the paths named below), the forms, the operands inside guarded allocations, the fp64 references, the
element-wise bounds and the sweeps tests/test_layernorm_cells_gpu.py runs.  Imports without a GPU.

Kinds of cell:
  randn   every operand random, every row with its own offset and scale; judged element by element against fp64:
          |got - ref| <= FACTOR x bound (bounds: `fwd_reference`, `bwd_reference`).
  lowvar  forward only: rows of standard deviation 1e-2, one element of magnitude 80 in a row of its own, so that c = max|x| / 8 = 10
          and eps c^2 = 1e-3 is ten times the variance: the epsilon fold decides y.  The reference is the oracle's definition
          layer_norm(x / c), not the kernel's identity.  The same data runs once with absmax_in = NULL (plain eps).
  exact   backward and pair: mean an even integer, rstd in {0.5, 1, 2}, x = mean + xh / rstd with xh small integers, gamma in
          {+-0.5, +-1, +-2}, dy in {+-4, +-8}, add_in integers, dropout p = 0.5 (keep scale exactly 2).  Columns come in pairs
          (gamma, -gamma) with equal dy and equal xh: sum gamma dy = 0 and sum gamma dy xh = 0 in every row, every fp32 partial sum is
          an integer and both row means are exactly 0, so dx == keep ? 2 rstd gamma dy : 0 (+ add_in) TO THE BIT, and dgamma, dbeta and
          colsum are integers equal to their fp64 sums.  The signs are steered row by row (`exact_operands`) so that every column sum
          (plus the initial value of an `accumulate` cell) stays an integer that bf16 holds.
Marked zeros are built here, not through the GEMM: where the oracle's mask drops an element x holds the 16-bit pattern 0x8000, kept
zeros are +0.0 (exact kind: the kept partner of a dropped element; randn kind: one kept element in 16).

The backward is judged in isolation: mean and rstd are inputs of its ABI and come from the oracle's formula in fp64, rounded to
fp32 (randn), or are chosen directly (exact) -- never from the GPU forward.

Operands: rows are contiguous (no pad columns); inputs lie between 4 guard rows (vectors: 8 guard elements) of NaN, outputs between
sentinels, the partial-sum workspace is exactly cogv_ln_bwd_workspace_bytes (the pair's size) between sentinels.  After every call
all sentinels must be intact, and a second call -- `accumulate` cells: after the initial values are restored -- gives the same bits.

The fp32 emulation at the end (`Emulated`) is a fixture of the CPU test only: it lets the checks be checked -- it must pass them, and
each of its seeded mutants must be rejected -- and is no second implementation of the kernels."""
import ctypes as C
import functools
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from cogview_amd import _lib
from oracle import cogview_oracle as O
from tests.gemm_cells import NAN16, SENT16, SENT32, Guarded, ulp
from tests.gemv_cells import DT_CODE, DT_NAME, DTYPES, EXACT_MAX

ALL_T, IN, OUT = 0, 1, 2                                         # COGV_LN_ALL_T, COGV_LN_STREAM_IN, COGV_LN_STREAM_OUT
EPS = 1e-5
SEED, STREAM = 4242, 11                                          # of the dropout mask
P_RANDN, P_EXACT = 0.1, 0.5
E32 = 2.0 ** -24                                                 # one fp32 rounding, relative
NAN32 = 0x7FFF7FFF
SWITCHES = ("COGV_LN_BWD_LEAN", "COGV_LN_BWD_MARKED_ROWS")       # read on every launch; the once-per-process ones are not used

# ------------------------------------------------------------------------------------------------------------------ the grids
# forward: (rows, h) -> (NV, lanes of the last vector, idle waves of the last workgroup, a wave makes a second pass)
FWD_GRID = (
    ((1, 8), (1, 1, 3, False)),                                  # one lane
    ((5, 520), (2, 1, 3, False)),                                # NV 2, one lane in the second vector, three idle waves
    ((9, 1536), (3, 64, 3, False)),                              # NV 3, full
    ((7, 2040), (4, 63, 1, False)),                              # NV 4, partial
    ((6, 2560), (5, 64, 2, False)),                              # NV 5
    ((5, 3064), (6, 63, 3, False)),                              # NV 6, partial
    ((5, 3576), (7, 63, 3, False)),                              # NV 7, partial
    ((3, 4096), (8, 64, 1, False)),                              # NV 8, full
    ((16389, 72), (1, 9, 0, True)),                              # more rows than 4 x the 4096-workgroup cap: every launch loops
)
FWD_SHAPES = tuple(s for s, _ in FWD_GRID)
LOWVAR_SHAPE = (12, 1024)
FWD_MAX_WAVES = 4 * 4096                                         # blocks = min(ceil(rows / 4), 4096, resident), four waves each
# forward form -> (stream mode, residual)
FWD_FORMS = {"F_T": (ALL_T, False), "F_T_RES": (ALL_T, True), "F_IN": (IN, False), "F_OUT": (OUT, True)}

# backward: (rows, h) -> (waves per row, wide)
BWD_GRID = (
    ((1, 8), (1, False)),                                        # narrow edges
    ((5, 520), (2, False)),
    ((4101, 64), (1, False)),                                    # 1024 workgroups at the workspace bound, a second pass of 5 rows
    ((7, 1544), (4, True)),                                      # narrowest wide row, row tail
    ((1029, 1544), (4, True)),                                   # wide: every form makes a second pass; reduce over 256 / 258 partials
    ((6, 2560), (5, True)),                                      # wide, few rows
    ((3, 4096), (8, True)),                                      # eight waves
)
BWD_SHAPES = tuple(s for s, _ in BWD_GRID)
# backward form -> (stream mode, dropout, marked, add_in, switches).  LN_FORM (mode, R, lean, mark) it reaches: wide / narrow rows
BWD_FORMS = {
    "T": (ALL_T, False, False, False, {}),                                       # (0, 4, 0, 0)
    "T_DROP_ADD": (ALL_T, True, False, True, {}),                                # (0, 2, 0, 0) / (0, 4, 0, 0)
    "T_MARK": (ALL_T, True, True, False, {}),                                    # (0, 4, 0, 1)
    "T_MARK2_ADD": (ALL_T, True, True, True, {"COGV_LN_BWD_MARKED_ROWS": "2"}),  # (0, 2, 0, 1) / (0, 4, 0, 1)
    "IN_ADD": (IN, False, False, True, {}),                                      # (1, 2, 0, 0) / (1, 4, 0, 0)
    "IN_DROP": (IN, True, False, False, {}),                                     # (1, 2, 0, 0) / (1, 4, 0, 0)
    "OUT": (OUT, False, False, False, {}),                                       # (2, 4, 0, 0)
    "OUT_DROP_ADD": (OUT, True, False, True, {}),                                # (2, 2, 0, 0) / (2, 4, 0, 0)
    "OUT_LEAN": (OUT, True, False, False, {}),                                   # (2, 2, 1, 0) / (2, 4, 0, 0)
    "OUT_MARK_ADD": (OUT, True, True, True, {}),                                 # (2, 4, 0, 1)
    "OUT_MARK2_NOLEAN": (OUT, True, True, False, {"COGV_LN_BWD_MARKED_ROWS": "2", "COGV_LN_BWD_LEAN": "0"}),   # (2, 2, 0, 1) / (2, 4, 0, 1)
    "OUT_MARK2_LEAN": (OUT, True, True, False, {"COGV_LN_BWD_MARKED_ROWS": "2"}),                              # (2, 2, 1, 1) / (2, 4, 0, 1)
}
LN_FORMS = {(0, 4, 0, 0), (0, 2, 0, 0), (0, 4, 0, 1), (0, 2, 0, 1), (1, 4, 0, 0), (1, 2, 0, 0),
            (2, 4, 0, 0), (2, 2, 0, 0), (2, 4, 0, 1), (2, 2, 0, 1), (2, 2, 1, 0), (2, 2, 1, 1)}      # the LN_FORM list of layernorm.hip
PAIR_SHAPES = ((1, 1544), (7, 2560), (1029, 1544), (3, 4096))
PAIR_FORMS = {"PAIR": False, "PAIR_DROP": True}
BWD_KINDS = ("exact", "randn")

FWD_OUTPUTS = ("y", "mean", "rstd")
BWD_OUTPUTS = ("dx", "dgamma", "dbeta", "colsum")
PAIR_OUTPUTS = ("dy", "d_ao", "dgamma2", "dbeta2", "dgamma3", "dbeta3", "colsum")
# Factor on the element-wise bound per (form, output): 1 = the bound as derived.  An entry is raised only together with a named
# error term read out of the kernel's code, and never above 2 (tests/test_layernorm_cells_cpu.py asserts that).
# Worst |got - fp64 reference| / bound measured on an MI355X, over both dtypes and the whole grid: see MEASURED below.
FACTOR = {(f, o): 1.0 for f in FWD_FORMS for o in FWD_OUTPUTS}
FACTOR.update({(f, o): 1.0 for f in BWD_FORMS for o in BWD_OUTPUTS})
FACTOR.update({(f, o): 1.0 for f in PAIR_FORMS for o in PAIR_OUTPUTS})
# Every 16-bit output sits at 1.00: its bound is half a unit in the last place plus the fp32 terms, and round-to-nearest reaches
# the half unit on some element of every cell (a tie of an fp32 sum of 16-bit values), so the fp32 terms above it are what a wrong
# kernel has to stay inside.  The fp32 outputs show the fp32 terms alone.  No factor had to be raised.
_M = lambda form, **kw: {(form, o): r for o, r in kw.items()}
MEASURED = {
    **_M("F_T", y=0.9999, mean=0.1143, rstd=0.3742), **_M("F_T_RES", y=0.9999, mean=0.1193, rstd=0.2845),
    **_M("F_IN", y=0.9999, mean=0.1983, rstd=0.3825), **_M("F_OUT", y=0.8600, mean=0.1087, rstd=0.3716),
    **_M("T", dx=0.9998, dgamma=0.9994, dbeta=1.0, colsum=0.9998), **_M("T_DROP_ADD", dx=0.9999, dgamma=0.9997, dbeta=0.9999, colsum=0.9999),
    **_M("T_MARK", dx=0.9997, dgamma=0.9996, dbeta=1.0, colsum=1.0), **_M("T_MARK2_ADD", dx=0.9999, dgamma=0.9999, dbeta=0.9999, colsum=0.9999),
    **_M("IN_ADD", dx=0.4792, dgamma=0.9979, dbeta=1.0, colsum=0.9995), **_M("IN_DROP", dx=0.2740, dgamma=0.9997, dbeta=0.9999, colsum=0.9998),
    **_M("OUT", dx=0.9998, dgamma=0.9996, dbeta=0.9989, colsum=1.0), **_M("OUT_DROP_ADD", dx=0.9999, dgamma=0.9996, dbeta=0.9991, colsum=0.9999),
    **_M("OUT_LEAN", dx=0.9997, dgamma=0.9995, dbeta=0.9998, colsum=1.0), **_M("OUT_MARK_ADD", dx=0.9999, dgamma=0.9996, dbeta=0.9995, colsum=0.9999),
    **_M("OUT_MARK2_NOLEAN", dx=0.9997, dgamma=0.9996, dbeta=0.9998, colsum=1.0),
    **_M("OUT_MARK2_LEAN", dx=0.9996, dgamma=0.9996, dbeta=0.9996, colsum=0.9999),
    **_M("PAIR", dy=0.5832, d_ao=0.9997, dgamma2=0.9996, dbeta2=1.0, dgamma3=0.9998, dbeta3=0.9998, colsum=1.0),
    **_M("PAIR_DROP", dy=0.5234, d_ao=0.9997, dgamma2=0.9997, dbeta2=1.0, dgamma3=0.9994, dbeta3=0.9997, colsum=1.0),
}


def with_switches(monkeypatch, env):
    """sets the per-launch switches of one backward form (monkeypatch restores them)"""
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


# ------------------------------------------------------------------------------------------ the grid arithmetic, restated
def fwd_geometry(rows, h):
    nv = (h + 511) // 512
    blocks = min((rows + 3) // 4, 4096)
    return nv, (h - (nv - 1) * 512) // 8, 4 * blocks - rows if rows < 4 * blocks else 0, rows > FWD_MAX_WAVES


def bwd_plan(mode, rows, h, p, marked, add_in):
    """(code, [rows in flight, lean, marked, workgroups, threads]) of cogv_ln_bwd_plan under the current switches"""
    out = (C.c_int * 5)(-1, -1, -1, -1, -1)
    return _lib.lib().cogv_ln_bwd_plan(mode, rows, h, p, int(marked), int(add_in), out), list(out)


def pair_plan(rows, h, p):
    out = (C.c_int * 5)(-1, -1, -1, -1, -1)
    return _lib.lib().cogv_ln_bwd_pair_plan(rows, h, p, out), list(out)


def passes(rows, rows_in_flight, blocks):
    """iterations of `for (row0 = blockIdx.x * R; row0 < rows; row0 += gridDim.x * R)` of workgroup 0"""
    return (rows + blocks * rows_in_flight - 1) // (blocks * rows_in_flight)


# ------------------------------------------------------------------------------------------ guarded allocations
class Guard(Guarded):
    """tests/gemm_cells.Guarded on any device; fp32 inputs too (NaN around them)"""

    def __init__(self, rows, cols, dtype, nan=False, device="cuda"):
        wide = dtype == torch.float32
        self.fill = (NAN32 if wide else NAN16) if nan else SENT32 if wide else SENT16
        bits = torch.int32 if wide else torch.int16
        if rows is None:
            self.buf = torch.full((cols + 16,), self.fill, dtype=bits, device=device)
            self.region = (slice(8, 8 + cols),)
        else:
            self.buf = torch.full((rows + 8, cols), self.fill, dtype=bits, device=device)
            self.region = (slice(4, 4 + rows), slice(0, cols))
        self.view = self.buf.view(dtype)[self.region]
        self.bits = self.buf[self.region]
        assert self.view.data_ptr() % 16 == 0

    def untouched(self):
        return bool((self.buf == self.fill).all())


def _ptr(g):
    return None if g is None else g.view.data_ptr()


def _in(t, dtype, device, marks=None):
    """an input [rows, h] or [n] inside NaN; `marks`: elements whose 16-bit pattern becomes 0x8000"""
    g = Guard(t.shape[0] if t.dim() == 2 else None, t.shape[-1], dtype, nan=True, device=device)
    g.view.copy_(t)
    if marks is not None:
        g.bits[marks.to(device)] = -32768
    return g


def _out(shape, dtype, device):
    return Guard(shape[0] if len(shape) == 2 else None, shape[-1], dtype, device=device)


# ------------------------------------------------------------------------------------------ operands (CPU, fp64, cached)
def keep_mask(rows, h, p):
    """bool [rows, h]: what the oracle's element-wise dropout keeps"""
    return torch.from_numpy(O.dropout_keep_mask(rows * h, p, SEED, STREAM) > 0).view(rows, h)


def keep_scale(p):
    return 65536.0 / (65536.0 - O._thr16(p))


def _rows_randn(g, rows, h, dtype, scale=1.0):
    """randn with an offset and a scale of its own in every row, as the storage type holds it"""
    off, sc = 2.0 * torch.randn((rows, 1), generator=g), 0.5 + 2.5 * torch.rand((rows, 1), generator=g)
    return ((off + sc * torch.randn((rows, h), generator=g)) * scale).to(dtype).double()


def oracle_stats(x, absmax=True):
    """mean and 1 / sqrt(var + eps c^2) of the rows of x as the oracle's Sandwich-LN defines them: layer_norm(x / c), c = max|x| / 8,
    normalises with mean / c and 1 / sqrt(var / c^2 + eps); in the units of the undivided x that is mean and the latter over c"""
    c = x.abs().max() / 8 if absmax else torch.tensor(1.0, dtype=torch.float64)
    xs = x / c
    return x.mean(1), 1.0 / (c * torch.sqrt(xs.var(1, unbiased=False) + EPS)), c


@functools.lru_cache(maxsize=None)
def fwd_problem(form, shape, kind, dtype, absmax=True):
    rows, h = shape
    mode, has_res = FWD_FORMS[form]
    g = torch.Generator().manual_seed(7919 * rows + h + 17 * mode + has_res)
    idx = (FWD_SHAPES + (LOWVAR_SHAPE,)).index(shape)
    c = SimpleNamespace(form=form, shape=shape, kind=kind, dtype=dtype, rows=rows, h=h, mode=mode, use_absmax=absmax,
                        x_dt=torch.float32 if mode == IN else dtype, y_dt=torch.float32 if mode == OUT else dtype,
                        save_stats=idx not in (2, 5), want_absmax=idx not in (1, 6), res=None)
    if kind == "lowvar":
        x = 0.25 * (torch.rand((rows, 1), generator=g) - 0.5) + 1e-2 * torch.randn((rows, h), generator=g)
        x[rows - 1, h // 3] = -80.0
        c.x = x.to(c.x_dt).double()
    else:
        c.x = _rows_randn(g, rows, h, c.x_dt)
    c.gamma = (1.0 + 0.5 * torch.randn(h, generator=g)).to(dtype).double()
    c.beta = (0.5 * torch.randn(h, generator=g)).to(dtype).double()
    if has_res:
        c.res = _rows_randn(g, rows, h, c.y_dt)
    c.absmax = float(c.x.abs().max()) if absmax else None              # exact in fp32: a stored value
    return c


def fwd_reference(c, fold="c^2"):
    """fp64 y, mean, rstd of the oracle's definition on the inputs as stored, and the element-wise bounds from ln_fwd_kernel's order
    of operations (e = 2^-24).  `fold`: the CPU test's wrong epsilon folds, to show that the data tell them apart."""
    x, g, b, h = c.x, c.gamma, c.beta, c.h
    if fold == "c^2" and c.use_absmax:
        y_ln = O.sandwich_layernorm(x, g, b, EPS)
        mean, rstd, cc = oracle_stats(x)
        eps_eff = EPS * cc * cc
    elif fold == "c^2":                                                  # absmax_in = NULL: plain layer_norm
        y_ln = F.layer_norm(x, (h,), g, b, EPS)
        mean, rstd, _ = oracle_stats(x, absmax=False)
        eps_eff = torch.tensor(EPS, dtype=torch.float64)
    else:                                                                # a wrong fold, spelled out
        cc = x.abs().max() / 8
        eps_eff = {"none": EPS, "c": EPS * cc, "absmax^2": EPS * 64 * cc * cc, "1/c^2": EPS / (cc * cc)}[fold]
        mean = x.mean(1)
        rstd = 1.0 / torch.sqrt(x.var(1, unbiased=False) + eps_eff)
        y_ln = (x - mean[:, None]) * rstd[:, None] * g + b
    var = x.var(1, unbiased=False)
    e, nv = E32, (h + 511) // 512
    depth = 8 * nv + 8                  # one lane's chain of 8 NV adds, six DPP steps, the multiply by 1 / h and 1 / h itself
    dm = depth * e * x.abs().mean(1) + e * mean.abs()                      # reduction error of the mean
    # variance: (x - mean)^2 carries three roundings, its sum `depth` more; the mean's error enters squared (the cross term is 0)
    dvar = (depth + 4) * e * var + dm * dm
    # rstd = 1 / sqrtf(var + eps'): eps' = eps c c (two roundings, at most e relative to var + eps'), the add, sqrtf, the division
    drel = 0.5 * dvar / (var + eps_eff) + 4 * e
    xh = (x - mean[:, None]) * rstd[:, None]
    # o = (x - mean) rstd gamma + beta: x-hat's three roundings and rstd's error, the mean's error times rstd, the add of beta
    err = g.abs() * (xh.abs() * (drel[:, None] + 3 * e) + (dm * rstd)[:, None]) + e * y_ln.abs()
    half = lambda v, er: ulp(v.abs() + er, c.dtype) / 2                  # half a unit in the last place of the 16-bit type
    if c.res is None:
        y = y_ln
        by = err + half(y, err)                                          # one rounding to T
    elif c.mode == OUT:
        y = y_ln + c.res
        by = err + e * y.abs()                                           # the fp32 add; an fp32 stream output has no storage term
    else:                                                                # all-T: LN's output is rounded to T before the residual add
        y = y_ln + c.res
        err = err + half(y_ln, err) + e * y.abs()
        by = err + half(y, err)
    return dict(y=y, mean=mean, rstd=rstd), dict(y=by, mean=dm, rstd=rstd * drel), var, eps_eff


@functools.lru_cache(maxsize=None)
def exact_operands(rows, h, seed, drop, marked, has_add):
    """The exact kind: see the module's docstring.  Column pairs (2 j, 2 j + 1) carry (gamma, -gamma), equal dy and equal x-hat.
    Magnitudes are random per (row, pair); the SIGNS are steered row by row so that no column sum runs away over thousands of rows:
    dy's sign is the one that leaves the running sums -- dbeta, dgamma and the two columns' colsum -- smallest, x-hat's sign
    opposes dgamma's running sum, add_in's sign (per element) opposes colsum's.  Every term is at most 32 + 8, and the CPU test
    asserts that every sum, with an `accumulate` cell's initial value, is an integer bf16 holds (|sum| <= 256).  Marked zeros: a
    pair with a dropped element has x == 0 in both columns, x-hat == -mean rstd there: the dropped one is the pattern 0x8000, a kept
    partner is +0.0."""
    g = torch.Generator().manual_seed(seed)
    npair = h // 2
    keep = keep_mask(rows, h, P_EXACT) if drop else None
    gm = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (npair,), generator=g)]
    gm = gm * (torch.randint(0, 2, (npair,), generator=g).double() * 2 - 1)
    gamma = torch.stack((gm, -gm), 1).reshape(h)
    mean = 2.0 * torch.randint(1, 3, (rows,), generator=g).double() * (torch.randint(0, 2, (rows,), generator=g).double() * 2 - 1)
    rstd = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (rows,), generator=g)]
    z = -mean * rstd
    add = torch.randint(-8, 9, (rows, h), generator=g).double() if has_add else torch.zeros((rows, h), dtype=torch.float64)
    kp = keep if keep is not None else torch.ones((rows, h), dtype=torch.bool)
    ks = 2.0 if keep is not None else 1.0
    w = ks * kp.double() * rstd[:, None] * gamma                            # dx = w dy + add_in
    w0, w1 = w[:, 0::2], w[:, 1::2]
    forced = ~(kp[:, 0::2] & kp[:, 1::2]) if marked else torch.zeros((rows, npair), dtype=torch.bool)
    xmag = torch.randint(1, 4, (rows, npair), generator=g).double()
    tie = torch.randint(0, 2, (rows, npair), generator=g).double() - 0.5
    # |dy| is 4 or 8 at random, but 4 where 8 would make a term of a column sum larger than 32
    big = (rstd[:, None] * gm.abs() * ks >= 4.0) | (forced & (z.abs() >= 8.0)[:, None])
    md = torch.where(big, 4.0, 4.0 * torch.randint(1, 3, (rows, npair), generator=g).double())
    amag = add.abs()
    B, G, C0, C1 = [torch.zeros(npair, dtype=torch.float64) for _ in range(4)]
    dy, xh = torch.zeros((rows, npair), dtype=torch.float64), torch.zeros((rows, npair), dtype=torch.float64)
    left = lambda s, a: (s.abs() - a).abs()                                 # what a freely signed term of size a leaves of the sum s
    for r in range(rows):
        zr, pots = z[r].expand(npair), []
        for d in (md[r], -md[r]):                                           # add_in's sign (per element) follows colsum's running sum
            ng = torch.where(forced[r], (G + d * zr).abs(), left(G, d * xmag[r]))
            pots.append((B + d) ** 2 + ng ** 2 + left(C0 + w0[r] * d, amag[r, 0::2]) ** 2 + left(C1 + w1[r] * d, amag[r, 1::2]) ** 2)
        d = torch.where(pots[0] - pots[1] + tie[r] < 0, md[r], -md[r])      # (the potentials are integers: `tie` decides ties only)
        xr = torch.where(forced[r], zr, torch.where(G * d > 0, -1.0, 1.0) * xmag[r])
        c0, c1 = C0 + w0[r] * d, C1 + w1[r] * d
        add[r, 0::2], add[r, 1::2] = torch.where(c0 > 0, -1.0, 1.0) * amag[r, 0::2], torch.where(c1 > 0, -1.0, 1.0) * amag[r, 1::2]
        dy[r], xh[r] = d, xr
        B, G, C0, C1 = B + d, G + d * xr, c0 + add[r, 0::2], c1 + add[r, 1::2]
    dy, xh = dy.repeat_interleave(2, 1), xh.repeat_interleave(2, 1)
    x = mean[:, None] + xh / rstd[:, None]
    marks = None
    if marked:
        marks = ~kp
        x = torch.where(forced.repeat_interleave(2, 1), torch.zeros_like(x), x)
    return SimpleNamespace(x=x, dy=dy, gamma=gamma, mean=mean, rstd=rstd, add=add if has_add else None, marks=marks, xh=xh)


def acc_init(rows, h, tag, exact):
    """initial values of dgamma, dbeta, colsum in an `accumulate` cell: small integers (exact) / numbers of the sums' size"""
    g = torch.Generator().manual_seed(31 * rows + h + tag)
    if exact:
        return [torch.randint(-8, 9, (h,), generator=g).double() for _ in range(3)]
    return [(rows ** 0.5) * torch.randn(h, generator=g) for _ in range(3)]


def bwd_variant(form, shape, kind):
    """(accumulate, which of dgamma / dbeta / colsum is NULL or None): both ways of `accumulate` and each pointer NULL across the grid"""
    i = BWD_SHAPES.index(shape) + BWD_KINDS.index(kind) + list(BWD_FORMS).index(form)
    return i % 2, (None, "dgamma", "dbeta", "colsum")[(i // 2) % 4]


@functools.lru_cache(maxsize=None)
def bwd_problem(form, shape, kind, dtype):
    rows, h = shape
    mode, drop, marked, has_add, env = BWD_FORMS[form]
    c = SimpleNamespace(form=form, shape=shape, kind=kind, dtype=dtype, rows=rows, h=h, mode=mode, marked=marked, env=env,
                        x_dt=torch.float32 if mode == IN else dtype, dy_dt=torch.float32 if mode == OUT else dtype,
                        p=0.0, keep=None, add=None, marks=None)
    c.accumulate, c.null = bwd_variant(form, shape, kind)
    seed = 104729 * rows + 13 * h + 7 * list(BWD_FORMS).index(form)
    if drop:
        c.p = P_EXACT if kind == "exact" else P_RANDN
        c.keep = keep_mask(rows, h, c.p)
    if kind == "exact":
        e = exact_operands(rows, h, 104729 * rows + 13 * h, drop, marked, has_add)      # (shared by the forms with these three switches)
        c.x, c.dy, c.gamma, c.mean, c.rstd, c.add, c.marks, c.xh = e.x, e.dy, e.gamma, e.mean, e.rstd, e.add, e.marks, e.xh
    else:
        g = torch.Generator().manual_seed(seed)
        c.x = _rows_randn(g, rows, h, c.x_dt)
        if marked:                                                        # dropped: 0x8000; one kept element in 16: +0.0
            c.marks = ~c.keep
            kept_zero = c.keep & (torch.randint(0, 16, (rows, h), generator=g) == 0)
            c.x = torch.where(c.marks | kept_zero, torch.zeros_like(c.x), c.x)
        m, r, _ = oracle_stats(c.x)
        c.mean, c.rstd = m.float().double(), r.float().double()             # the oracle's formula in fp64, rounded to fp32
        c.dy = _rows_randn(g, rows, h, c.dy_dt, 0.25)
        c.gamma = (1.0 + 0.5 * torch.randn(h, generator=g)).to(dtype).double()
        if has_add:
            c.add = _rows_randn(g, rows, h, c.x_dt, 0.25)
    c.init = [t.to(dtype).double() for t in acc_init(rows, h, 1, kind == "exact")] if c.accumulate else None
    return c


def bwd_reference(c):
    """fp64 dx, dgamma, dbeta of LN' on the inputs as stored (mean and rstd as given), and the bounds from ln_bwd_kernel's order of
    operations: x-hat = fma(x, rstd, -mean rstd), gy = gamma dy (rounded), m1 = sum gy / h, m2 = sum gy x-hat / h,
    dx = rstd fma(-x-hat, m2, gy - m1), x keep scale, + add_in, one rounding to the output type; e = 2^-24."""
    e, h, rows = E32, c.h, c.rows
    rstd, mr = c.rstd[:, None], (c.mean * c.rstd)[:, None]
    xh = c.x * rstd - mr
    gy = c.dy * c.gamma
    m1, m2 = gy.mean(1, keepdim=True), (gy * xh).mean(1, keepdim=True)
    inner = gy - m1 - xh * m2
    o = rstd * inner
    dxh = e * (mr.abs() + xh.abs())                                      # the rounded product mean rstd and the fused multiply-add
    # reductions over h: a lane's chain of 8, six DPP steps, up to eight waves in LDS order, the multiply by the rounded 1 / h
    depth = 8 + 6 + 8 + 2
    dm1 = depth * e * gy.abs().mean(1, keepdim=True)                     # gy's own rounding is one of the `depth`
    dm2 = (depth + 1) * e * (gy * xh).abs().mean(1, keepdim=True) + (gy.abs() * dxh).mean(1, keepdim=True)
    # rstd (|gy| + |m1| + |x-hat m2|): the rounding of gy, of gy - m1, of the fma and of the product with rstd
    err = rstd * (e * gy.abs() + dm1 + e * (gy.abs() + m1.abs()) + dxh * m2.abs() + xh.abs() * dm2
                  + e * (gy.abs() + m1.abs() + (xh * m2).abs())) + e * o.abs()
    if c.keep is not None:
        ks = keep_scale(c.p)
        o = o * c.keep.double() * ks
        err = (err * ks + 2 * e * o.abs()) * c.keep.double()             # the rounded scale and the product; a dropped element is 0
    if c.add is not None:
        o = o + c.add
        err = err + e * o.abs()                                          # the fp32 add
    half = lambda v, er: ulp(v.abs() + er, c.dtype) / 2
    bdx = err if c.mode == IN else err + half(o, err)                    # the fp32 stream gradient has no storage term
    ref, bound = dict(dx=o), dict(dx=bdx)
    # column sums over the rows: any order of fp32 additions of n terms is within (n - 1) e sum|terms|; the partials' reduce and the
    # accumulate add are counted in `rows + 2`; dgamma's terms carry x-hat's error
    for name, t, te, k in (("dgamma", c.dy * xh, c.dy.abs() * dxh, 0), ("dbeta", c.dy, None, 1)):
        s = t.sum(0)
        er = (rows + 2) * e * t.abs().sum(0) + (te.sum(0) if te is not None else 0.0)
        if c.init is not None:
            s = s + c.init[k]
            er = er + e * s.abs()
        ref[name], bound[name] = s, er + half(s, er)
    return ref, bound


def colsum_reference(c, dx_stored):
    """colsum's reference is the fp64 sum of the STORED dx: the kernel sums the rounded values"""
    s = dx_stored.sum(0)
    er = (c.rows + 2) * E32 * dx_stored.abs().sum(0)
    if c.init is not None:
        s = s + c.init[2]
        er = er + E32 * s.abs()
    return s, er + ulp(s.abs() + er, c.dtype) / 2


def exact_expected(c):
    """the exact kind: dx, dgamma, dbeta, colsum (fp64 integers; with the initial values of an `accumulate` cell)"""
    dx = c.rstd[:, None] * c.gamma * c.dy
    if c.keep is not None:
        dx = torch.where(c.keep, 2.0 * dx, torch.zeros_like(dx))
    if c.add is not None:
        dx = dx + c.add
    sums = [(c.dy * c.xh).sum(0), c.dy.sum(0), dx.sum(0)]
    if c.init is not None:
        sums = [s if i is None else s + i for s, i in zip(sums, c.init)]
    return dx, sums


@functools.lru_cache(maxsize=None)
def pair_problem(form, shape, kind, dtype):
    """LN2' (STREAM_IN, add_in = dout) and LN3' (STREAM_OUT, marked zeros in ao) as two backward cells; in the exact kind dout is
    chosen so that dy = dout + LN2'(dc) is the dy the second stage's zero row sums need"""
    rows, h = shape
    drop = PAIR_FORMS[form]
    c = SimpleNamespace(form=form, shape=shape, kind=kind, dtype=dtype, rows=rows, h=h, p=0.0, keep=None, marks=None)
    c.accumulate = (PAIR_SHAPES.index(shape) + BWD_KINDS.index(kind)) % 2
    seed = 15485863 + 101 * rows + h
    if drop:
        c.p = P_EXACT if kind == "exact" else P_RANDN
        c.keep = keep_mask(rows, h, c.p)
    if kind == "exact":
        s2 = exact_operands(rows, h, seed, False, False, False)
        s3 = exact_operands(rows, h, seed + 1, drop, drop, False)
        c.dc, c.y, c.gamma2, c.mean2, c.rstd2, c.xh2 = s2.dy, s2.x, s2.gamma, s2.mean, s2.rstd, s2.xh
        c.dy_want = s3.dy
        c.dout = s3.dy - s2.rstd[:, None] * s2.gamma * s2.dy
        c.ao, c.gamma3, c.mean3, c.rstd3, c.xh3, c.marks = s3.x, s3.gamma, s3.mean, s3.rstd, s3.xh, s3.marks
    else:
        g = torch.Generator().manual_seed(seed)
        c.y = _rows_randn(g, rows, h, torch.float32)
        c.ao = _rows_randn(g, rows, h, dtype)
        if drop:
            c.marks = ~c.keep
            kept_zero = c.keep & (torch.randint(0, 16, (rows, h), generator=g) == 0)
            c.ao = torch.where(c.marks | kept_zero, torch.zeros_like(c.ao), c.ao)
        for name, t in (("2", c.y), ("3", c.ao)):
            m, r, _ = oracle_stats(t)
            setattr(c, "mean" + name, m.float().double())
            setattr(c, "rstd" + name, r.float().double())
        c.dc = _rows_randn(g, rows, h, dtype, 0.25)
        c.dout = _rows_randn(g, rows, h, torch.float32, 0.25)
        c.gamma2, c.gamma3 = [(1.0 + 0.5 * torch.randn(h, generator=g)).to(dtype).double() for _ in range(2)]
    # initial values: dgamma2, dbeta2, dgamma3, dbeta3, colsum
    c.init = None
    if c.accumulate:
        a, b = acc_init(rows, h, 2, kind == "exact"), acc_init(rows, h, 3, kind == "exact")
        c.init = [t.to(dtype).double() for t in (a[0], a[1], b[0], b[1], b[2])]
    return c


def pair_stages(c, dy_stored):
    """the two stages of a pair cell as backward cells: LN2' on the inputs, LN3' on the dy the kernel stored (fp32: the values it
    kept in registers, to the bit)"""
    base = dict(form=c.form, shape=c.shape, kind=c.kind, dtype=c.dtype, rows=c.rows, h=c.h, marked=False)
    s2 = SimpleNamespace(mode=IN, x=c.y, dy=c.dc, gamma=c.gamma2, mean=c.mean2, rstd=c.rstd2, add=c.dout, keep=None, p=0.0,
                         init=None if c.init is None else [c.init[0], c.init[1], None], **base)
    s3 = SimpleNamespace(mode=OUT, x=c.ao, dy=dy_stored, gamma=c.gamma3, mean=c.mean3, rstd=c.rstd3, add=None, keep=c.keep, p=c.p,
                         init=None if c.init is None else [c.init[2], c.init[3], c.init[4]], **base)
    return s2, s3


# ------------------------------------------------------------------------------------------ judging
def ratio(got, ref, bound):
    """worst |got - ref| / bound (an element off where the bound is 0 counts as infinite; NaN counts as infinite)"""
    err = (got - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound.expand_as(err))
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    return float(r.max()) if r.numel() else 0.0


def _where(bad):
    return tuple(bad.nonzero()[0].tolist())


def _judge(fails, ratios, form, name, got, ref, bound):
    if bool(torch.isnan(got).any()):
        fails.append(f"{name}: NaN (a guard row or a row past the end was read, or the output is wrong)")
    r = ratio(got, ref, bound) / FACTOR[(form, name)]
    ratios[name] = max(ratios.get(name, 0.0), r)
    if not r <= 1.0:
        bad = ~((got - ref).abs() <= FACTOR[(form, name)] * bound.expand_as(got))
        fails.append(f"{name}: err / bound = {r:.3f}, {int(bad.sum())} elements, first {_where(bad)}")


def _judge_exact(fails, name, got, want):
    if not torch.equal(got, want):
        bad = got != want
        fails.append(f"{name}: {int(bad.sum())} elements are not the exact value, first {_where(bad)}: {float(got[bad][0])} for {float(want[bad][0])}")


# ------------------------------------------------------------------------------------------ staging
class Staged:
    """operands of one cell on a device; `outputs`: name -> Guard (None: the pointer is NULL)"""

    def arm(self):
        for name, g in self.outputs.items():
            if g is not None:
                g.reset()
                if name in self.initial:
                    g.view.copy_(self.initial[name])

    def snapshot(self):
        return {n: g.buf.clone() for n, g in self.outputs.items() if g is not None and n != "workspace"}

    def stray(self):
        return [f"guards of {n} written" for n, g in self.outputs.items() if g is not None and not g.intact()]

    def untouched(self):
        return all(g.untouched() or n in self.initial for n, g in self.outputs.items() if g is not None)

    def get(self, name):
        return self.outputs[name].view.double().cpu()


class FwdStaged(Staged):
    def __init__(self, c, dev):
        self.c = c
        self.x, self.gamma, self.beta = _in(c.x, c.x_dt, dev), _in(c.gamma, c.dtype, dev), _in(c.beta, c.dtype, dev)
        self.res = None if c.res is None else _in(c.res, c.y_dt, dev)
        self.absmax_in = None if c.absmax is None else _in(torch.tensor([c.absmax]), torch.float32, dev)
        self.outputs = dict(y=_out(c.shape, c.y_dt, dev), mean=_out((c.rows,), torch.float32, dev), rstd=_out((c.rows,), torch.float32, dev),
                            absmax=_out((1,), torch.float32, dev))
        self.initial = dict(absmax=torch.zeros(1))                        # the kernel raises the cell with an atomic max
        self.arm()

    def args(self, **kw):
        c, o = self.c, self.outputs
        a = dict(dtype=DT_CODE[c.dtype], x=_ptr(self.x), gamma=_ptr(self.gamma), beta=_ptr(self.beta), res=_ptr(self.res), y=_ptr(o["y"]),
                 mean=_ptr(o["mean"]) if c.save_stats else None, rstd=_ptr(o["rstd"]) if c.save_stats else None,
                 absmax_in=_ptr(self.absmax_in), absmax_out=_ptr(o["absmax"]) if c.want_absmax else None, rows=c.rows, h=c.h, eps=EPS, mode=c.mode)
        a.update(kw)
        return a


class BwdStaged(Staged):
    def __init__(self, c, dev):
        self.c = c
        self.dy, self.x = _in(c.dy, c.dy_dt, dev), _in(c.x, c.x_dt, dev, c.marks)
        self.gamma, self.mean, self.rstd = _in(c.gamma, c.dtype, dev), _in(c.mean, torch.float32, dev), _in(c.rstd, torch.float32, dev)
        self.add = None if c.add is None else _in(c.add, c.x_dt, dev)
        self.ws_bytes = _lib.lib().cogv_ln_bwd_workspace_bytes(c.rows, c.h)
        self.outputs = dict(dx=_out(c.shape, c.x_dt, dev), workspace=_out((self.ws_bytes // 4,), torch.float32, dev))
        for name in ("dgamma", "dbeta", "colsum"):
            self.outputs[name] = None if c.null == name else _out((c.h,), c.dtype, dev)
        self.initial = {} if c.init is None else {n: t for n, t in zip(("dgamma", "dbeta", "colsum"), c.init) if self.outputs[n] is not None}
        self.arm()

    def args(self, **kw):
        c, o = self.c, self.outputs
        a = dict(dtype=DT_CODE[c.dtype], dy=_ptr(self.dy), x=_ptr(self.x), gamma=_ptr(self.gamma), mean=_ptr(self.mean), rstd=_ptr(self.rstd),
                 add=_ptr(self.add), dx=_ptr(o["dx"]), dgamma=_ptr(o["dgamma"]), dbeta=_ptr(o["dbeta"]), colsum=_ptr(o["colsum"]),
                 accumulate=c.accumulate, rows=c.rows, h=c.h, p=c.p, ws=_ptr(o["workspace"]), ws_bytes=self.ws_bytes, mode=c.mode, marked=c.marked)
        a.update(kw)
        return a


class PairStaged(Staged):
    NAMES = ("dgamma2", "dbeta2", "dgamma3", "dbeta3", "colsum")

    def __init__(self, c, dev):
        self.c, f = c, torch.float32
        self.dc, self.y, self.dout, self.ao = _in(c.dc, c.dtype, dev), _in(c.y, f, dev), _in(c.dout, f, dev), _in(c.ao, c.dtype, dev, c.marks)
        self.gamma2, self.gamma3 = _in(c.gamma2, c.dtype, dev), _in(c.gamma3, c.dtype, dev)
        self.stats = [_in(t, f, dev) for t in (c.mean2, c.rstd2, c.mean3, c.rstd3)]
        self.ws_bytes = _lib.lib().cogv_ln_bwd_pair_workspace_bytes(c.rows, c.h)
        self.outputs = dict(dy=_out(c.shape, f, dev), d_ao=_out(c.shape, c.dtype, dev), workspace=_out((self.ws_bytes // 4,), f, dev))
        self.outputs.update({n: _out((c.h,), c.dtype, dev) for n in self.NAMES})
        self.initial = {} if c.init is None else dict(zip(self.NAMES, c.init))
        self.arm()

    def args(self, **kw):
        c, o = self.c, self.outputs
        a = dict(dtype=DT_CODE[c.dtype], dc=_ptr(self.dc), y=_ptr(self.y), gamma2=_ptr(self.gamma2), mean2=_ptr(self.stats[0]),
                 rstd2=_ptr(self.stats[1]), dout=_ptr(self.dout), dy=_ptr(o["dy"]), dgamma2=_ptr(o["dgamma2"]), dbeta2=_ptr(o["dbeta2"]),
                 ao=_ptr(self.ao), gamma3=_ptr(self.gamma3), mean3=_ptr(self.stats[2]), rstd3=_ptr(self.stats[3]), d_ao=_ptr(o["d_ao"]),
                 dgamma3=_ptr(o["dgamma3"]), dbeta3=_ptr(o["dbeta3"]), colsum=_ptr(o["colsum"]), accumulate=c.accumulate, rows=c.rows, h=c.h,
                 p=c.p, ws=_ptr(o["workspace"]), ws_bytes=self.ws_bytes)
        a.update(kw)
        return a


class Launched:
    """the kernels, through the C ABI"""
    device = "cuda"

    def __init__(self, ops):
        self.stream = ops._stream

    def fwd(self, S, **kw):
        a = S.args(**kw)
        rc = _lib.lib().cogv_sandwich_ln_fwd(a["dtype"], a["x"], a["gamma"], a["beta"], a["res"], a["y"], a["mean"], a["rstd"], a["absmax_in"],
                                             a["absmax_out"], a["rows"], a["h"], a["eps"], a["mode"], self.stream())
        torch.cuda.synchronize()
        return rc

    def bwd(self, S, **kw):
        a = S.args(**kw)
        head = (a["dtype"], a["dy"], a["x"], a["gamma"], a["mean"], a["rstd"], a["add"], a["dx"], a["dgamma"], a["dbeta"], a["colsum"],
                a["accumulate"], a["rows"], a["h"], a["p"])
        tail = (a["ws"], a["ws_bytes"], a["mode"], self.stream())
        if a["marked"]:
            rc = _lib.lib().cogv_sandwich_ln_bwd_marked(*head, *tail)
        else:
            rc = _lib.lib().cogv_sandwich_ln_bwd(*head, SEED, STREAM, *tail)
        torch.cuda.synchronize()
        return rc

    def pair(self, S, **kw):
        a = S.args(**kw)
        rc = _lib.lib().cogv_sandwich_ln_bwd_pair(a["dtype"], a["dc"], a["y"], a["gamma2"], a["mean2"], a["rstd2"], a["dout"], a["dy"], a["dgamma2"],
                                                  a["dbeta2"], a["ao"], a["gamma3"], a["mean3"], a["rstd3"], a["d_ao"], a["dgamma3"], a["dbeta3"],
                                                  a["colsum"], a["accumulate"], a["rows"], a["h"], a["p"], a["ws"], a["ws_bytes"], self.stream())
        torch.cuda.synchronize()
        return rc


def _twice(S, call, fails):
    """the call, then (after its results are taken by `take`) the same call again on re-armed outputs: the same bits"""
    rc = call(S)
    if rc != _lib.OK:
        fails.append(f"the call answers {rc}")
        return None
    first = S.snapshot()
    fails += S.stray()

    def again():
        S.arm()
        if call(S) != _lib.OK or not all(torch.equal(v, first[n]) for n, v in S.snapshot().items()):
            fails.append("the second call gives other bits")
    return again


# ------------------------------------------------------------------------------------------ the cells
def run_fwd(backend, c):
    """-> (failures, {output: err / bound})"""
    fails, ratios = [], {}
    S = FwdStaged(c, backend.device)
    again = _twice(S, backend.fwd, fails)
    if again is None:
        return fails, ratios
    ref, bound, _, _ = fwd_reference(c)
    y = S.get("y")
    _judge(fails, ratios, c.form, "y", y, ref["y"], bound["y"])
    for name in ("mean", "rstd"):
        if c.save_stats:
            _judge(fails, ratios, c.form, name, S.get(name), ref[name], bound[name])
        elif not S.outputs[name].untouched():
            fails.append(f"{name} written through a NULL pointer's neighbour")
    got = S.outputs["absmax"].view.cpu()
    if c.want_absmax:                                                     # max|y| of the STORED y, exactly
        if float(got[0]) != float(y.abs().max()):
            fails.append(f"absmax_out is {float(got[0])}, max|y| of the stored y is {float(y.abs().max())}")
    elif float(got[0]) != 0.0:
        fails.append("absmax_out written although its pointer was NULL")
    again()
    return fails, ratios


def run_bwd(backend, c):
    fails, ratios = [], {}
    S = BwdStaged(c, backend.device)
    again = _twice(S, backend.bwd, fails)
    if again is None:
        return fails, ratios
    dx = S.get("dx")
    have = [n for n in ("dgamma", "dbeta", "colsum") if S.outputs[n] is not None]
    if c.kind == "exact":
        want_dx, sums = exact_expected(c)
        _judge_exact(fails, "dx", dx, want_dx)
        for name, want in zip(("dgamma", "dbeta", "colsum"), sums):
            if name in have:
                _judge_exact(fails, name, S.get(name), want)
    else:
        ref, bound = bwd_reference(c)
        ref["colsum"], bound["colsum"] = colsum_reference(c, dx)
        for name in ["dx"] + have:
            _judge(fails, ratios, c.form, name, S.get(name), ref[name], bound[name])
    again()
    return fails, ratios


def run_pair(backend, c):
    fails, ratios = [], {}
    S = PairStaged(c, backend.device)
    again = _twice(S, backend.pair, fails)
    if again is None:
        return fails, ratios
    dy, d_ao = S.get("dy"), S.get("d_ao")
    s2, s3 = pair_stages(c, dy)
    if c.kind == "exact":
        s2.xh, s3.xh, s3.dy = c.xh2, c.xh3, c.dy_want
        want_dy, sums2 = exact_expected(s2)
        want_ao, sums3 = exact_expected(s3)
        assert torch.equal(want_dy, c.dy_want)
        _judge_exact(fails, "dy", dy, want_dy)
        _judge_exact(fails, "d_ao", d_ao, want_ao)
        for name, want in zip(PairStaged.NAMES, sums2[:2] + sums3):
            _judge_exact(fails, name, S.get(name), want)
    else:
        r2, b2 = bwd_reference(s2)
        r3, b3 = bwd_reference(s3)
        cs, bcs = colsum_reference(s3, d_ao)
        for name, ref, bound in (("dy", r2["dx"], b2["dx"]), ("d_ao", r3["dx"], b3["dx"]), ("dgamma2", r2["dgamma"], b2["dgamma"]),
                                 ("dbeta2", r2["dbeta"], b2["dbeta"]), ("dgamma3", r3["dgamma"], b3["dgamma"]),
                                 ("dbeta3", r3["dbeta"], b3["dbeta"]), ("colsum", cs, bcs)):
            _judge(fails, ratios, c.form, name, dy if name == "dy" else d_ao if name == "d_ao" else S.get(name), ref, bound)
    again()
    return fails, ratios


def _collect(fails, worst, tag, bad, ratios, kind):
    fails += [f"{tag}: {b}" for b in bad]
    for name, r in ratios.items():
        for key in (name, f"{name} / {kind}"):
            worst[key] = max(worst.get(key, 0.0), r)


def fwd_cells(form):
    """(shape, kind, absmax_in given) of one forward form: randn on the grid, lowvar with the fold and (all-T) with plain eps"""
    cells = [(s, "randn", True) for s in FWD_SHAPES] + [(LOWVAR_SHAPE, "lowvar", True)]
    return cells + ([(LOWVAR_SHAPE, "lowvar", False)] if form == "F_T" else [])


def fwd_sweep(backend, form, dtype):
    """-> (failures, cells, {output: worst err / bound})"""
    fails, worst = [], {}
    for shape, kind, absmax in fwd_cells(form):
        bad, ratios = run_fwd(backend, fwd_problem(form, shape, kind, dtype, absmax))
        _collect(fails, worst, f"{form} {DT_NAME[dtype]} (rows, h)={shape} {kind}{'' if absmax else ' plain eps'}", bad, ratios, kind)
    return fails, len(fwd_cells(form)), worst


def bwd_sweep(backend, form, dtype, shapes=BWD_SHAPES):
    """every shape x kind of one backward form (the caller has set the form's switches)"""
    fails, worst = [], {}
    mode, _, marked, has_add, _ = BWD_FORMS[form]
    for shape in shapes:
        for kind in BWD_KINDS:
            c = bwd_problem(form, shape, kind, dtype)
            rc, plan = bwd_plan(mode, shape[0], shape[1], c.p, marked, has_add)
            if rc != _lib.OK or (mode, plan[0], plan[1], plan[2]) not in LN_FORMS:
                fails.append(f"{form} {shape}: planned {rc} {plan}")
                continue
            bad, ratios = run_bwd(backend, c)
            _collect(fails, worst, f"{form} {DT_NAME[dtype]} (rows, h)={shape} {kind} LN_FORM{(mode, *plan[:3])} x {plan[3]}", bad, ratios, kind)
    return fails, len(shapes) * len(BWD_KINDS), worst


def pair_sweep(backend, form, dtype):
    fails, worst = [], {}
    for shape in PAIR_SHAPES:
        for kind in BWD_KINDS:
            bad, ratios = run_pair(backend, pair_problem(form, shape, kind, dtype))
            _collect(fails, worst, f"{form} {DT_NAME[dtype]} (rows, h)={shape} {kind}", bad, ratios, kind)
    return fails, len(PAIR_SHAPES) * len(BWD_KINDS), worst


# ------------------------------------------------------------------------------------------ refusals
# (entry point, overrides, code): plan and launch refuse alike and nothing is written.  "misaligned": the pointer + 8 bytes;
# "short": one byte less than the workspace size
REFUSALS = (
    ("fwd", dict(h=516), _lib.ERR_ARG), ("fwd", dict(h=4104), _lib.ERR_ARG), ("fwd", dict(rows=0), _lib.ERR_ARG),
    ("fwd", dict(x="misaligned"), _lib.ERR_ARG), ("fwd", dict(y="misaligned"), _lib.ERR_ARG),
    ("bwd", dict(h=516), _lib.ERR_ARG), ("bwd", dict(h=4104), _lib.ERR_ARG), ("bwd", dict(rows=0), _lib.ERR_ARG), ("bwd", dict(rows=-3), _lib.ERR_ARG),
    ("bwd", dict(p=1.0), _lib.ERR_ARG), ("bwd", dict(p=-0.25), _lib.ERR_ARG), ("bwd", dict(p=0.5, marked=1, mode=IN), _lib.ERR_ARG),
    ("bwd", dict(ws_bytes="short"), _lib.ERR_ARG), ("bwd", dict(dx="misaligned"), _lib.ERR_ARG), ("bwd", dict(dy="misaligned"), _lib.ERR_ARG),
    ("pair", dict(h=2564), _lib.ERR_ARG), ("pair", dict(h=4104), _lib.ERR_ARG), ("pair", dict(rows=0), _lib.ERR_ARG), ("pair", dict(p=1.0), _lib.ERR_ARG),
    ("pair", dict(h=1536), _lib.ERR_UNSUPPORTED), ("pair", dict(h=512), _lib.ERR_UNSUPPORTED),
    ("pair", dict(ws_bytes="short"), _lib.ERR_ARG), ("pair", dict(d_ao="misaligned"), _lib.ERR_ARG), ("pair", dict(y="misaligned"), _lib.ERR_ARG),
)
REFUSAL_SHAPE = (6, 2560)


def refusal_sweep(backend, dtype):
    """-> (failures, descriptors).  The plan queries know shapes and dropout only: pointers and the workspace are the launch's."""
    fails = []
    staged = dict(fwd=FwdStaged(fwd_problem("F_T", REFUSAL_SHAPE, "randn", dtype), backend.device),
                  bwd=BwdStaged(bwd_problem("T", REFUSAL_SHAPE, "randn", dtype), backend.device),
                  pair=PairStaged(pair_problem("PAIR", (7, 2560), "randn", dtype), backend.device))
    for entry, kw, want in REFUSALS:
        S, kw = staged[entry], dict(kw)
        a = S.args()
        for k, v in list(kw.items()):
            if v == "misaligned":
                kw[k] = a[k] + 8
            elif v == "short":
                kw[k] = a[k] - 1
        a = S.args(**kw)
        pointers = any(k not in ("h", "rows", "p", "marked", "mode") for k in kw)
        if entry == "bwd" and not pointers:
            prc = bwd_plan(a["mode"], a["rows"], a["h"], a["p"], a["marked"], 0)[0]
        elif entry == "pair" and not pointers:
            prc = pair_plan(a["rows"], a["h"], a["p"])[0]
        else:
            prc = want
        rc = getattr(backend, entry)(S, **kw)
        if (prc, rc) != (want, want):
            fails.append(f"{entry} {kw}: the plan answers {prc} and the call {rc} where both must refuse with {want}")
        if not S.untouched() or S.stray():
            fails.append(f"{entry} {kw}: a refused call wrote an output or its guards")
            S.arm()
    return fails, len(REFUSALS)


# ------------------------------------------------------------------------------------------ fp32 emulation (CPU test fixture)
MUTANTS = {   # name -> (entry, form, shape, kind) on which at least one check must reject it
    "fold: plain eps": ("fwd", "F_T", LOWVAR_SHAPE, "lowvar"),
    "fold: eps c": ("fwd", "F_IN", LOWVAR_SHAPE, "lowvar"),
    "fold: eps absmax^2": ("fwd", "F_OUT", LOWVAR_SHAPE, "lowvar"),
    "fold: eps / c^2": ("fwd", "F_T_RES", LOWVAR_SHAPE, "lowvar"),
    "1/h over the width rounded up to 512": ("fwd", "F_T", (5, 520), "randn"),
    "last 8-column group skipped": ("fwd", "F_IN", (7, 2040), "randn"),
    "second-pass rows read at the wrong stride": ("fwd", "F_OUT", (16389, 72), "randn"),
    "bwd: second-pass rows read at the wrong stride": ("bwd", "T", (1029, 1544), "exact"),
    "bwd: last 8-column group skipped": ("bwd", "IN_ADD", (7, 1544), "exact"),
    "m1 without 1/h": ("bwd", "OUT", (7, 1544), "randn"),
    "m2 without 1/h": ("bwd", "IN_DROP", (5, 520), "randn"),
    "dropout index shifted by one 8-group": ("bwd", "T_DROP_ADD", (5, 520), "exact"),
    "keep scale missing": ("bwd", "OUT_LEAN", (6, 2560), "exact"),
    "add_in added before the mask": ("bwd", "T_DROP_ADD", (3, 4096), "exact"),
    "marked: the kept +0.0 counts as dropped": ("bwd", "T_MARK", (5, 520), "exact"),
    "one workgroup's partial left out of the reduce": ("bwd", "T", (4101, 64), "exact"),
    "accumulate ignored": ("bwd", "OUT", (7, 1544), "exact"),
    "accumulate applied twice": ("bwd", "OUT", (7, 1544), "exact"),
    "colsum of the unrounded values": ("bwd", "T", (7, 1544), "randn"),
    "pair: dy rounded to 16 bits before the LN3' stage": ("pair", "PAIR", (1029, 1544), "randn"),
    "pair: one workgroup's partial left out of the reduce": ("pair", "PAIR_DROP", (1029, 1544), "exact"),
}


def mutant_cell(name, dtype):
    entry, form, shape, kind = MUTANTS[name]
    if entry == "fwd":
        return entry, fwd_problem(form, shape, kind, dtype)
    return entry, (bwd_problem if entry == "bwd" else pair_problem)(form, shape, kind, dtype)


class Emulated:
    """The kernels' arithmetic in fp32 on the CPU: sums over h and over the rows in fp32 (torch's order), every product and
    difference rounded as the kernels round them, rows dealt to workgroups as the plan says, one rounding of every output."""
    device = "cpu"

    def __init__(self, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.mutant = mutant

    def fwd(self, S, **kw):
        c, m, f = S.c, self.mutant, torch.float32
        x, g, b = S.x.view.float(), S.gamma.view.float(), S.beta.view.float()
        if m == "second-pass rows read at the wrong stride":
            x = torch.cat((x[:FWD_MAX_WAVES], x[FWD_MAX_WAVES - 1:-1]))
        eps = torch.tensor(EPS, dtype=f)
        if S.absmax_in is not None:
            am = S.absmax_in.view[0]
            cc = am * 0.125
            eps = {None: eps * cc * cc, "fold: plain eps": eps, "fold: eps c": eps * cc, "fold: eps absmax^2": eps * am * am,
                   "fold: eps / c^2": eps / (cc * cc)}.get(m, eps * cc * cc)
        inv_h = torch.tensor(1.0 / ((c.h + 511) // 512 * 512 if m == "1/h over the width rounded up to 512" else c.h), dtype=f)
        mean = x.sum(1) * inv_h
        d = x - mean[:, None]
        rstd = 1.0 / torch.sqrt((d * d).sum(1) * inv_h + eps)
        o = d * rstd[:, None] * g + b
        if S.res is not None:
            if c.mode != OUT:
                o = o.to(c.dtype).float()
            o = o + S.res.view.float()
        cols = c.h - 8 if m == "last 8-column group skipped" else c.h
        out = S.outputs
        out["y"].view[:, :cols] = o.to(c.y_dt)[:, :cols]
        if c.save_stats:
            out["mean"].view.copy_(mean)
            out["rstd"].view.copy_(rstd)
        if c.want_absmax:
            out["absmax"].view[0] = torch.maximum(out["absmax"].view[0], out["y"].view[:, :cols].float().abs().max())
        return _lib.OK

    def _ln_bwd(self, dy, x, g, mean, rstd, add, keep, ks, out_dt, R, blocks, marks=None):
        """one LN': (dx as stored, partial sums [blocks, 3, h] of dgamma, dbeta, colsum)"""
        m, f, (rows, h) = self.mutant, torch.float32, x.shape
        if m == "bwd: second-pass rows read at the wrong stride":
            first = blocks * R
            x = torch.cat((x[:first], x[first - 1:-1]))
        inv_h = torch.tensor(1.0 / h, dtype=f)
        rs = rstd[:, None]
        xh = x * rs - (mean * rstd)[:, None]
        gy = dy * g
        m1 = gy.sum(1, keepdim=True) * (1.0 if m == "m1 without 1/h" else inv_h)
        m2 = (gy * xh).sum(1, keepdim=True) * (1.0 if m == "m2 without 1/h" else inv_h)
        o = rs * ((gy - m1) - xh * m2)
        if add is not None and m == "add_in added before the mask":
            o = o + add
        if keep is not None:
            if m == "dropout index shifted by one 8-group":
                keep = torch.roll(keep.flatten(), 8).view(rows, h)
            if m == "marked: the kept +0.0 counts as dropped" and marks is not None:
                keep = keep & (x != 0)
            o = torch.where(keep, o * (1.0 if m == "keep scale missing" else ks), torch.zeros_like(o))
        if add is not None and m != "add_in added before the mask":
            o = o + add
        stored = o.to(out_dt)
        summed = o if m == "colsum of the unrounded values" else stored.float()
        wg = (torch.arange(rows) // R) % blocks
        part = torch.zeros((blocks, 3, h), dtype=f)
        for i, t in enumerate((dy * xh, dy, summed)):
            part[:, i].index_add_(0, wg, t)
        if m in ("last 8-column group skipped", "bwd: last 8-column group skipped"):
            stored = stored[:, :h - 8]
        return stored, part

    def _reduce(self, S, part, names, accumulate):
        m = self.mutant
        if m is not None and "one workgroup's partial left out" in m:
            part = part[:-1]
        for i, name in enumerate(names):
            g = S.outputs.get(name) if name else None
            if g is None:
                continue
            t = part[:, i].sum(0)
            if (accumulate and m != "accumulate ignored") or m == "accumulate applied twice":
                t = t + g.view.float() * (2.0 if m == "accumulate applied twice" and accumulate else 1.0)
            g.view.copy_(t)

    def bwd(self, S, **kw):
        c = S.c
        mode, drop, marked, has_add, _ = BWD_FORMS[c.form]
        rc, plan = bwd_plan(mode, c.rows, c.h, c.p, marked, has_add)
        assert rc == _lib.OK
        keep = c.keep
        if keep is not None and marked:
            keep = S.x.bits != -32768                                     # the marks, as the kernel reads them
        stored, part = self._ln_bwd(S.dy.view.float(), S.x.view.float(), S.gamma.view.float(), S.mean.view, S.rstd.view,
                                    None if S.add is None else S.add.view.float(), keep, torch.tensor(keep_scale(c.p), dtype=torch.float32),
                                    c.x_dt, plan[0], plan[3], c.marks)
        S.outputs["dx"].view[:, :stored.shape[1]] = stored
        self._reduce(S, part, ("dgamma", "dbeta", "colsum"), c.accumulate)
        return _lib.OK

    def pair(self, S, **kw):
        c, f = S.c, torch.float32
        rc, plan = pair_plan(c.rows, c.h, c.p)
        assert rc == _lib.OK
        dy, part2 = self._ln_bwd(S.dc.view.float(), S.y.view, S.gamma2.view.float(), S.stats[0].view, S.stats[1].view, S.dout.view, None, None,
                                 f, plan[0], plan[3])
        S.outputs["dy"].view.copy_(dy)
        if self.mutant == "pair: dy rounded to 16 bits before the LN3' stage":
            dy = dy.to(c.dtype).float()
        keep = (S.ao.bits != -32768) if c.keep is not None else None
        d_ao, part3 = self._ln_bwd(dy, S.ao.view.float(), S.gamma3.view.float(), S.stats[2].view, S.stats[3].view, None, keep,
                                   torch.tensor(keep_scale(c.p), dtype=f), c.dtype, plan[0], plan[3])
        S.outputs["d_ao"].view.copy_(d_ao)
        self._reduce(S, part2, ("dgamma2", "dbeta2", None), c.accumulate)
        self._reduce(S, part3, ("dgamma3", "dbeta3", "colsum"), c.accumulate)
        return _lib.OK
