"""Shared body of the attention cell sweep (cogview_amd/csrc/attention.hip: forward, dQ and dK.dV kernels, dense / dropout / stored
keep bits / flexible instantiations, cogv_sparse_slot_reduce): the shape grid (tests/test_attention_cells_cpu.py proves on the CPU
that it reaches the paths named below), the forms, the operands inside guarded allocations, the fp64 references, the element-wise
bounds, the keep-word decoder and the sweeps tests/test_attention_cells_gpu.py runs.  Imports without a GPU.

Kinds of cell, per (shape, form):
  selector  keys are +-1 codes, query i is 16 x the code of a chosen visible key sel(i), scale 0.125: the selected score is 128, every
            other visible key at least 48 lower (minimum pairwise Hamming distance >= 12, asserted), so its probability is below
            2^-69 and vanishes against 1.0 in every fp32 accumulator.  V integers in [-8, 8] \\ {0}, dO integers in [1, 8], at most 16
            queries per key: O == V[sel], dV[j] == sum of dO over the selectors of j, to the bit; |dQ|, |dK| <= 2^-40 (at the
            selected key dP = dO.V_sel and D = dO.O are the same integer: dS is exactly 0).  Dropout p = 0.5 (keep scale exactly 2):
            O == 2 V[sel] where the oracle keeps (i, sel(i)), |O| <= 2^-40 where it drops it.
  decoy     the same operands, but query i aims at the code of key i + off + 1, the first key it must NOT see: a leak across the
            diagonal gives O ~ V[i + off + 1].  Judged as `randn`.
  randn     element by element against fp64: |got - ref| <= FACTOR x bound (bounds: `reference`), lse row by row.
The selector and decoy kinds run on the forms whose visible set is the left-to-right rule (the three dense forms and the mask tensor
that restates the rule); the random and three-valued mask tensors run the `randn` kind.

Operands: q, k, v are strided views of one [B, s_k, 3 H 64 + 8] buffer (q: the last s_q rows), dO of a [B, s_k, H 64 + 8] one; pad
columns, unused rows and 4 guard rows before and after hold NaN -- dma_tile clamps rows past the end to the last valid row and
load_frag_global zero-fills invalid queries, so no legitimate path reads them.  o, dq, dk, dv have row strides H 64 + 8 or + 24
with sentinel guards, lse / the dvec workspace / the keep words / the column-sum workspace are vectors with 8 guard words each side.
Every sentinel must be intact after every call and a second call must give the same bits.

The fp32 emulation at the end (`Emulated`) is a fixture of the CPU test only: it lets the checks be checked -- it must pass them, and
each of its seeded mutants must be rejected -- and is no second implementation of the kernels."""
import ctypes as C
import functools
import math
from types import SimpleNamespace

import torch

from cogview_amd import _lib
from oracle import cogview_oracle as O
from tests.gemm_cells import NAN16, SENT16, SENT32, Guarded
from tests.gemv_cells import DT_CODE, DT_NAME, DTYPES, EXACT_MAX, U

DENSE, DENSE_DROP, DENSE_BITS, FLEXIBLE = 0, 1, 2, 3             # AttnForm of attention.hip
SCALE = 0.125
SEED, STREAM = 20240, 7                                          # of the dropout mask
P_RANDN, P_EXACT = 0.1, 0.5
TINY = 2.0 ** -40
# absolute floor of one rounding.  fp16: half its subnormal spacing.  bf16 has fp32's exponent range, and so do the kernels' fp32
# intermediates: v_exp_f32 returns 0 for a probability below 2^-126 (fast_exp2 of attention.hip: "no denormal-range fix-up"), where
# fp64 still holds e^-256 = 2^-369 between two +-1 codes.  An output element made of such terms alone (dV of a key no query is
# near, times operands of up to 2^13 each) is compared against 2^-100 instead of against u times itself.
ETA = {torch.float16: 2.0 ** -25, torch.bfloat16: 2.0 ** -100}
LSE_U = 2.0 ** -20
MAX_SELECTORS = 16

# The grid: (B, H, s_q, s_k, sep) -> what the launch plan and the kernels' block arithmetic must say:
#   (grid of forward / dQ, grid of dK.dV, sep_k, key tiles per query block, active waves per query block, query stages per key block)
GRID = (
    ((1, 1, 1, 1, 0), (8, 8, 0, (1,), (1,), (1,))),                      # one query, one key
    ((1, 3, 64, 64, 0), (8, 8, 0, (1,), (2,), (1,))),                    # exactly one key tile; waves 2 and 3 inactive
    ((2, 1, 65, 65, 0), (8, 8, 0, (2,), (3,), (2,))),                    # key tail of 1, query tail of 1 in a third wave
    ((1, 2, 127, 127, 0), (8, 8, 0, (2,), (4,), (2,))),                  # the workgroup boundary from below,
    ((1, 2, 128, 128, 0), (8, 8, 0, (2,), (4,), (2,))),                  # ... exactly,
    ((3, 3, 129, 129, 0), (32, 32, 0, (2, 3), (4, 1), (3, 1))),          # ... and from above; 9 units: a second round per XCD
    ((1, 17, 40, 40, 0), (24, 24, 0, (1,), (2,), (1,))),                 # 17 units: a third round
    ((1, 1, 257, 257, 0), (24, 24, 0, (2, 4, 5), (4, 4, 1), (5, 3, 1))),  # ring stages used an odd and an even number of times
    ((1, 2, 33, 161, 0), (8, 16, 0, (3,), (2,), (1, 1))),                # memory form, off = 128; dK.dV grid follows the keys
    ((1, 2, 96, 160, 5), (8, 16, 69, (3,), (3,), (2, 1))),               # sep_k = 69: one key past the first tile
    ((1, 1, 130, 194, 70), (16, 16, 134, (3, 4), (4, 1), (3, 3))),       # sep_k = 134: crosses a 128-key workgroup
    ((1, 1, 100, 100, 100), (8, 8, 100, (2,), (4,), (2,))),              # everything visible, sep_k == s_k
    ((1, 1, 100, 100, 200), (8, 8, 200, (2,), (4,), (2,))),              # ... sep_k > s_k
    ((1, 1, 1, 200, 0), (8, 16, 0, (4,), (1,), (1, 1))),                 # a single query over four key tiles
)
SHAPES = tuple(s for s, _ in GRID)

# form name -> (AttnForm the plan must answer, dropout, stored keep bits, mask tensor kind)
FORMS = {
    "DENSE": (DENSE, False, False, None),
    "DENSE_DROP": (DENSE_DROP, True, False, None),
    "DENSE_BITS": (DENSE_BITS, True, True, None),
    "MASK_LTR": (FLEXIBLE, False, False, "ltr"),                  # binary, equals the left-to-right rule, shared over the batch
    "MASK_RANDOM": (FLEXIBLE, True, False, "random"),             # random binary per sample, two rows entirely zero; dropout on
    "MASK_THREE": (FLEXIBLE, False, False, "three"),              # values 0, 0.25, 1 per sample
}
KINDS = ("selector", "decoy", "randn")
OUTPUTS = ("o", "lse", "dq", "dk", "dv")
# factor on the element-wise bound per (form, output): 1 = the bound as derived.  An entry is raised only together with a named
# error term read out of the kernel's code, and never above 2 (tests/test_attention_cells_cpu.py asserts that).
FACTOR = {(f, o): 1.0 for f in tuple(FORMS) + ("SPARSE", "SPARSE_DROP", "GATHER") for o in OUTPUTS}


def kinds_of(form):
    return ("randn",) if form in ("MASK_RANDOM", "MASK_THREE") else KINDS


def shapes_of(form):
    return tuple(s for s in SHAPES if FORMS[form][3] is None or s[4] == 0)


def cells_of(form):
    return len(shapes_of(form)) * len(kinds_of(form))


def cell_tag(form, shape, kind, dtype):
    return f"{form} {DT_NAME[dtype]} (B,H,s_q,s_k,sep)={shape} {kind}"


# ------------------------------------------------------------------------------------------ the kernels' block arithmetic, restated
def geometry(s_q, s_k, sep):
    off = s_k - s_q
    return off, (sep + off if sep > 0 else 0)


def fwd_blocks(s_q, s_k, sep_k):
    """attn_fwd_kernel / attn_bwd_dq_kernel, per 128-query workgroup: (nkb, [kend_w of its active waves])"""
    off, out = s_k - s_q, []
    for q0 in range(0, s_q, 128):
        q_last = min(s_q, q0 + 128) - 1
        nkb = (min(s_k, max(q_last + off + 1, sep_k)) + 63) >> 6
        out.append((nkb, [min(s_k, max(min(s_q, q0w + 32) - 1 + off + 1, sep_k)) for q0w in range(q0, min(s_q, q0 + 128), 32)]))
    return out


def dkdv_blocks(s_q, s_k, sep_k):
    """attn_bwd_dkdv_kernel, per 128-key workgroup: (qb0, nqb)"""
    off = s_k - s_q
    return [((0 if k0 < sep_k else max(0, k0 - off)) >> 6, (s_q + 63) >> 6) for k0 in range(0, s_k, 128)]


def kend_of_query(s_q, s_k, sep_k):
    """int64 [s_q]: kend_w of the 32-query group (wave) of each query"""
    q = torch.arange(s_q)
    last = torch.clamp((q // 32) * 32 + 32, max=s_q) - 1
    return torch.clamp(torch.clamp(last + (s_k - s_q) + 1, min=sep_k), max=s_k)


def ltr_visible(s_q, s_k, sep_k):
    """bool [s_q, s_k]: key <= q + off or key < sep_k (`visible` of attention.hip)"""
    i, j = torch.arange(s_q).view(-1, 1), torch.arange(s_k).view(1, -1)
    return (j <= i + (s_k - s_q)) | (j < sep_k)


# ------------------------------------------------------------------------------------------ keep words (AttnArgs::keepbits)
# word [(b H + head)][kb][fg][q], bit 31 - n <-> key 64 kb + 32 (n >> 4) + 8 ((n & 15) >> 2) + 4 fg + (n & 3)
_N = torch.arange(32)
KEY_OF_BIT = torch.stack([32 * (_N >> 4) + 8 * ((_N & 15) >> 2) + 4 * fg + (_N & 3) for fg in (0, 1)])      # [fg][n] -> key in block


def keep_words_count(B, H, s_q, s_k):
    return B * H * ((s_k + 63) // 64) * 2 * s_q


def decode_keep_words(words, B, H, s_q, s_k):
    """int32 words (flat) -> bool [B, H, s_q, 64 nkb]: the keep bit of every (query, key slot of the padded blocks)"""
    nkb = (s_k + 63) // 64
    w = (words.cpu().to(torch.int64) & 0xFFFFFFFF).view(B, H, nkb, 2, s_q)
    bits = (w.unsqueeze(-1) >> (31 - _N)) & 1                                            # [B, H, kb, fg, q, n]
    out = torch.zeros((B, H, s_q, nkb, 64), dtype=torch.bool)
    for fg in (0, 1):
        out[:, :, :, :, KEY_OF_BIT[fg]] = bits[:, :, :, fg].permute(0, 1, 3, 2, 4).bool()
    return out.view(B, H, s_q, nkb * 64)


def written_keep_slots(s_q, s_k, sep_k):
    """bool [s_q, 64 nkb]: slots (query, key < s_k) inside the words the forward kernel writes: key blocks with 64 kb < kend_w"""
    nkb = (s_k + 63) // 64
    j = torch.arange(nkb * 64).view(1, -1)
    return ((j // 64) * 64 < kend_of_query(s_q, s_k, sep_k).view(-1, 1)) & (j < s_k)


# ------------------------------------------------------------------------------------------ operands (CPU, fp64, cached)
def keep_mask(B, H, s_q, s_k, p):
    """bool [B, H, s_q, s_k]: what the oracle's attention dropout keeps"""
    return torch.from_numpy(O.attention_keep_mask(B, H, s_q, s_k, p, SEED, STREAM) > 0)


def min_hamming(codes):
    """smallest pairwise Hamming distance among the +-1 codes [..., n, 64] of each unit (64 where a unit has one key)"""
    n = codes.shape[-2]
    dist = (64.0 - codes @ codes.transpose(-1, -2)) / 2 + 64.0 * torch.eye(n, dtype=codes.dtype)
    return int(dist.min())


@functools.lru_cache(maxsize=None)
def selectors(B, H, s_q, s_k, sep):
    """int64 [B, H, s_q]: the visible key each query selects.  The first and the last query and every third one take the diagonal
    key q + off (the last visible one), a few key 0, a few key min(sep_k, s_k) - 1 where only the prefix rule shows it, the rest a
    random visible key; never more than MAX_SELECTORS queries per key."""
    off, sep_k = geometry(s_q, s_k, sep)
    g = torch.Generator().manual_seed(7919 * s_q + 31 * s_k + sep + 1)
    sel = torch.zeros((B, H, s_q), dtype=torch.int64)
    for b in range(B):
        for h in range(H):
            count = [0] * s_k
            n_first = n_sep = 0
            for i in range(s_q):
                vmax = min(s_k - 1, max(i + off, sep_k - 1))            # the visible keys are [0, vmax]
                if i in (0, s_q - 1) or i % 3 == 0:
                    j = i + off
                elif i % 9 == 1 and n_first < 8:
                    j, n_first = 0, n_first + 1
                elif sep_k > 0 and i % 2 == 1 and i + off < min(sep_k, s_k) - 1 and n_sep < 8:
                    j, n_sep = min(sep_k, s_k) - 1, n_sep + 1
                else:
                    j = int(torch.randint(0, vmax + 1, (1,), generator=g))
                while count[j] >= MAX_SELECTORS:
                    j = (j + 1) % (vmax + 1)
                count[j] += 1
                sel[b, h, i] = j
    return sel


def mask_tensor(kind, B, s_q, s_k):
    """fp64 [B or 1, s_q, s_k]"""
    g = torch.Generator().manual_seed(104729 + 13 * s_q + s_k + B)
    if kind == "ltr":
        return ltr_visible(s_q, s_k, 0).double().unsqueeze(0)
    if kind == "random":
        m = (torch.rand((B, s_q, s_k), generator=g) < 0.6).double()
        m[:, s_q - 1] = 0.0                                              # rows entirely zero: uniform attention over all keys
        m[:, s_q // 2] = 0.0
        return m
    return torch.tensor([0.0, 0.25, 1.0], dtype=torch.float64)[torch.randint(0, 3, (B, s_q, s_k), generator=g)]


@functools.lru_cache(maxsize=None)
def problem(form, shape, kind, dtype):
    """One cell's operands, values the 16-bit type holds, as fp64 [B, H, s, 64] -- shared and never written"""
    B, H, s_q, s_k, sep = shape
    plan_form, drop, bits, mkind = FORMS[form]
    off, sep_k = geometry(s_q, s_k, sep)
    g = torch.Generator().manual_seed(1000003 * s_q + 1009 * s_k + 17 * H + B + {"selector": 0, "decoy": 1, "randn": 2}[kind])
    P = SimpleNamespace(form=form, plan_form=plan_form, shape=shape, kind=kind, dtype=dtype, B=B, H=H, s_q=s_q, s_k=s_k, sep=sep,
                        off=off, sep_k=sep_k, bits=bits, sel=None, M=None, keep=None, p=0.0, index=None, sparse=None)
    if kind == "randn":
        P.q, P.k, P.v, P.do = [torch.randn((B, H, s, 64), generator=g).to(dtype).double() for s in (s_q, s_k, s_k, s_q)]
    else:
        codes = torch.randint(0, 2, (B, H, s_k, 64), generator=g).double() * 2 - 1
        while min_hamming(codes) < 12:                                   # (seeded: the same draw every time; the CPU test asserts it)
            codes = torch.randint(0, 2, (B, H, s_k, 64), generator=g).double() * 2 - 1
        P.sel = selectors(B, H, s_q, s_k, sep)
        aim = P.sel
        if kind == "decoy":
            t = torch.arange(s_q) + off + 1
            aim = torch.where((t < s_k) & (t >= sep_k), t.clamp(max=s_k - 1), P.sel)
        P.aim = aim
        P.k = codes
        P.q = 16.0 * torch.gather(codes, 2, aim.unsqueeze(-1).expand(B, H, s_q, 64))
        P.v = torch.randint(1, 9, (B, H, s_k, 64), generator=g).double() * (torch.randint(0, 2, (B, H, s_k, 64), generator=g).double() * 2 - 1)
        P.do = torch.randint(1, 9, (B, H, s_q, 64), generator=g).double()
    if mkind is not None:
        assert sep == 0
        P.M = mask_tensor(mkind, B, s_q, s_k)
    if drop:
        P.p = P_RANDN if kind == "randn" else P_EXACT
        P.keep = keep_mask(B, H, s_q, s_k, P.p)
    return P


def visibility(P):
    """fp64 multiplier M [B or 1, 1, s_q, s_k] of the scores: the mask tensor, or the left-to-right rule"""
    return P.M.unsqueeze(1) if P.M is not None else ltr_visible(P.s_q, P.s_k, P.sep_k).double().view(1, 1, P.s_q, P.s_k)


# ------------------------------------------------------------------------------------------ reference (fp64) and bounds
def reference(q, k, v, do, M, keep, p, dtype, bias=None):
    """S = scale Q K^T M - 10000 (1 - M) (+ bias), P = softmax S, Pd = P keep / (1 - p), O = Pd V and its gradients, in fp64 on the
    inputs as stored; leading dimensions broadcast.  Returns the five outputs and, per output, the element-wise bound

      O : u (|O| + Pd |V|) + eta (1 + sum_j |V_jd|)              dV: u (|dV| + Pd^T |dO|) + eta (1 + sum_i |dO_id|)
      dQ: u (|dQ| + scale E |K|) + eta (1 + scale sum_j |K_jd|)  dK: u (|dK| + scale E^T |Q|) + eta (1 + scale sum_i |Q_id|)
      E_ij = (|dS_ij| + P_ij A_i) |M_ij|,  u A_i = sum_d |dO_id| bound(O_id)    (D is formed from the ROUNDED O: A carries O's
                                                                                eta term too, u A_i >= eta sum_d |dO_id| (1 + sum_j |V_jd|))
      lse: 2^-20 (1 + |lse| + max_j |S_ij|), the maximum over the keys of non-zero probability

    u = one rounding of the storage type (P, dS and the output are each rounded once), eta = the fp16 subnormal floor."""
    u, eta = U[dtype], ETA[dtype]
    kscale = 65536.0 / (65536.0 - O._thr16(p)) if keep is not None else 1.0
    S = SCALE * (q @ k.transpose(-1, -2))
    S = S * M - 10000.0 * (1.0 - M)
    if bias is not None:
        S = S + bias
    lse = torch.logsumexp(S, -1)
    Pr = torch.exp(S - lse.unsqueeze(-1))
    kp = keep.double() * kscale if keep is not None else torch.ones_like(Pr)
    Pd = Pr * kp
    o = Pd @ v
    dP = (do @ v.transpose(-1, -2)) * kp
    D = (do * o).sum(-1, keepdim=True)
    dS = Pr * (dP - D)
    dSr = dS * M * SCALE
    dq, dk, dv = dSr @ k, dSr.transpose(-1, -2) @ q, Pd.transpose(-1, -2) @ do
    b_o = u * (o.abs() + Pd @ v.abs()) + eta * (1.0 + v.abs().sum(-2, keepdim=True))
    uA = (do.abs() * b_o).sum(-1, keepdim=True)                          # error of D = sum_d dO_id O_id, O rounded as bounded above
    E = (dS.abs() + Pr * (uA / u)) * M.abs()
    smax = torch.where(Pr > 0, S.abs(), torch.zeros_like(S)).amax(-1)
    bound = dict(
        o=b_o,
        dv=u * (dv.abs() + Pd.transpose(-1, -2) @ do.abs()) + eta * (1.0 + do.abs().sum(-2, keepdim=True)),
        dq=u * (dq.abs() + SCALE * (E @ k.abs())) + eta * (1.0 + SCALE * k.abs().sum(-2, keepdim=True)),
        dk=u * (dk.abs() + SCALE * (E.transpose(-1, -2) @ q.abs())) + eta * (1.0 + SCALE * q.abs().sum(-2, keepdim=True)),
        lse=LSE_U * (1.0 + lse.abs() + smax))
    return dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv), bound


@functools.lru_cache(maxsize=None)
def _reference_of(form, shape, kind, dtype):
    P = problem(form, shape, kind, dtype)
    return reference(P.q, P.k, P.v, P.do, visibility(P), P.keep, P.p, dtype)


def ratio(got, ref, bound):
    """worst |got - ref| / bound (an element off where the bound is 0 counts as infinite; NaN counts as infinite)"""
    err = (got - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound.expand_as(err))
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    return float(r.max()) if r.numel() else 0.0


def _first(bad):
    return tuple(bad.nonzero()[0].tolist())


def judge(P, R):
    """Checks (a) - (d) on one cell's outputs R (CPU: o, dq [B, H, s_q, 64], dk, dv [B, H, s_k, 64] fp64, lse [B, H, s_q], the keep
    words or None) -> (failures, {output: err / bound})"""
    fails, ratios = [], {}
    ref, bound = _reference_of(P.form, P.shape, P.kind, P.dtype)
    for name in OUTPUTS:
        if bool(torch.isnan(R[name]).any()):
            fails.append(f"{name}: NaN (an out-of-range operand element was used, or the output is wrong)")
    ratios["lse"] = ratio(R["lse"], ref["lse"], bound["lse"]) / FACTOR[(P.form, "lse")]
    if P.kind == "selector":
        B, H, s_q, s_k = P.B, P.H, P.s_q, P.s_k
        hit = torch.ones((B, H, s_q), dtype=torch.bool) if P.keep is None else torch.gather(P.keep, 3, P.sel.unsqueeze(-1)).squeeze(-1)
        gain = 1.0 if P.keep is None else 2.0
        want_o = gain * torch.gather(P.v, 2, P.sel.unsqueeze(-1).expand(B, H, s_q, 64))
        bad = torch.where(hit.unsqueeze(-1), R["o"] != want_o, ~(R["o"].abs() <= TINY))
        if bool(bad.any()):
            fails.append(f"o: {int(bad.any(-1).sum())} rows are not {'2 ' if gain == 2.0 else ''}V[sel] (or 0 where dropped), first (b, h, q, d) = {_first(bad)}")
        want_dv = torch.zeros((B, H, s_k, 64), dtype=torch.float64)
        want_dv.scatter_add_(2, P.sel.unsqueeze(-1).expand(B, H, s_q, 64), gain * P.do * hit.unsqueeze(-1))
        assert float(want_dv.abs().max()) <= EXACT_MAX[torch.bfloat16]
        bad = torch.where(want_dv != 0, R["dv"] != want_dv, ~(R["dv"].abs() <= TINY))
        if bool(bad.any()):
            fails.append(f"dv: {int(bad.any(-1).sum())} rows are not the sum of dO over the key's selectors, first (b, h, key, d) = {_first(bad)}")
        for name in ("dq", "dk"):
            bad = ~(R[name].abs() <= TINY)
            if bool(bad.any()):
                fails.append(f"{name}: {int(bad.sum())} elements above 2^-40 (max {float(R[name].abs().nan_to_num(posinf=1e300).max()):.3g}), first {_first(bad)}")
    else:
        for name in ("o", "dq", "dk", "dv"):
            ratios[name] = ratio(R[name], ref[name], bound[name]) / FACTOR[(P.form, name)]
    for name, r in ratios.items():
        if not r <= 1.0:
            fails.append(f"{name}: err / bound = {r:.3f}")
    if P.bits:                                                           # (d): every bit the forward pass writes
        got = decode_keep_words(R["words"], P.B, P.H, P.s_q, P.s_k)
        where = written_keep_slots(P.s_q, P.s_k, P.sep_k)
        want = torch.zeros_like(got)
        want[..., :P.s_k] = P.keep
        bad = (got != want) & where
        if bool(bad.any()):
            fails.append(f"stored keep bits: {int(bad.sum())} differ from the oracle's mask, first (b, h, q, key) = {_first(bad)}")
    return fails, ratios


def judge_colsum(P, R):
    """(e): the column-sum partials [B nblk][3 H 64] against the stored dq | dk | dv"""
    fails = []
    part = R["partial"].double().view(-1, 3, P.H, 64).sum(0)              # [3][H][64]
    for i, name in enumerate(("dq", "dk", "dv")):
        stored = R[name]
        sums, absum = stored.sum((0, 2)), stored.abs().sum((0, 2))
        if P.kind == "selector" and name == "dv":                         # exact integers: any order of fp32 sums gives these bits
            if not torch.equal(part[i], sums):
                fails.append(f"column sums of dv: {int((part[i] != sums).sum())} are not the integer sums of the stored rows")
            continue
        # `randn`: u x sum of |rows|.  Selector cells, dq and dk (stored values below 2^-40, exactly 0 in fp16): an fp32 sum of n rows
        lim = (stored.shape[0] * stored.shape[2] * 2.0 ** -24 if P.kind == "selector" else U[P.dtype]) * absum
        if bool(((part[i] - sums).abs() > lim).any()):
            fails.append(f"column sums of {name}: {int(((part[i] - sums).abs() > lim).sum())} beyond the bound on the sum of the stored rows")
    return fails


# ------------------------------------------------------------------------------------------ guarded allocations
class Guard(Guarded):
    """tests/gemm_cells.Guarded on any device"""

    def __init__(self, rows, cols, dtype, pad=0, nan=False, device="cuda"):
        wide = dtype == torch.float32
        assert not (nan and wide)
        self.fill = NAN16 if nan else SENT32 if wide else SENT16
        bits = torch.int32 if wide else torch.int16
        if rows is None:
            self.buf = torch.full((cols + 16,), self.fill, dtype=bits, device=device)
            self.region = (slice(8, 8 + cols),)
        else:
            self.buf = torch.full((rows + 8, cols + pad), self.fill, dtype=bits, device=device)
            self.region = (slice(4, 4 + rows), slice(0, cols))
        self.view = self.buf.view(dtype)[self.region]
        self.bits = self.buf[self.region]
        assert self.view.data_ptr() % 16 == 0


def _bshd(g, B, s, H):
    """[B s, n H 64] strided -> [B, s, n H, 64]"""
    return g.view.unflatten(0, (B, s)).unflatten(-1, (-1, 64))


class Staged:
    """One cell on a device: inputs with NaN around them, outputs with sentinels around them, and the descriptor."""

    def __init__(self, P, device, kv_rows=None, planes=None):
        B, H, s_q, s_k, dt = P.B, P.H, P.s_q, P.s_k, P.dtype
        self.P, C_ = P, H * 64
        rows = kv_rows or s_k                                            # rows of K / V per sample (gathered forms: the pool)
        self.rows = rows
        self.qkv = Guard(B * rows, 3 * C_, dt, 8, nan=True, device=device)
        self.dout = Guard(B * rows, C_, dt, 8, nan=True, device=device)
        x = _bshd(self.qkv, B, rows, H)
        self.q, self.k, self.v = x[:, rows - s_q:, :H], x[:, :, H:2 * H], x[:, :, 2 * H:]
        self.do = _bshd(self.dout, B, rows, H)[:, rows - s_q:]
        for dst, src in ((self.q, P.q), (self.k, P.kpool if kv_rows else P.k), (self.v, P.vpool if kv_rows else P.v), (self.do, P.do)):
            dst.copy_(src.permute(0, 2, 1, 3))
        kplanes = planes or B                                            # sparse training form: one [s_k] plane per (sample, block)
        self.kplanes = kplanes
        self.o, self.dq = Guard(B * s_q, C_, dt, 8, device=device), Guard(B * s_q, C_, dt, 24, device=device)
        self.dk, self.dv = Guard(kplanes * s_k, C_, dt, 24, device=device), Guard(kplanes * s_k, C_, dt, 8, device=device)
        self.lse = Guard(None, B * H * s_q, torch.float32, device=device)
        self.dvec = Guard(None, 2 * B * H * s_q, torch.float32, device=device)
        self.words = Guard(None, keep_words_count(B, H, s_q, s_k), torch.float32, device=device) if P.bits else None
        self.nblk = (s_q + 127) // 128
        self.partial = Guard(None, B * self.nblk * 3 * C_, torch.float32, device=device) if s_q == s_k and P.sparse is None else None
        self.mask = None if P.M is None else P.M.to(dt).to(device).contiguous()
        self.index = None if P.index is None else P.index.to(device).contiguous()
        self.fwd_outputs = [g for g in (self.o, self.lse, self.words) if g is not None]
        self.bwd_outputs = [g for g in (self.dq, self.dk, self.dv, self.dvec, self.partial) if g is not None]

    def desc(self, colsum=False, **kw):
        P, d = self.P, _lib.AttnDesc()
        d.dtype, d.B, d.H, d.s_q, d.s_k, d.head_dim, d.sep = DT_CODE[P.dtype], P.B, P.H, P.s_q, P.s_k, 64, P.sep
        d.scale, d.dropout_p, d.seed, d.stream_id = SCALE, P.p, SEED, STREAM
        rs = self.qkv.buf.shape[1]
        d.q, d.k, d.v, d.dout = self.q.data_ptr(), self.k.data_ptr(), self.v.data_ptr(), self.do.data_ptr()
        d.q_rs = d.k_rs = d.v_rs = rs
        d.q_bs = d.k_bs = d.v_bs = self.rows * rs
        d.do_rs, d.do_bs = self.dout.buf.shape[1], self.rows * self.dout.buf.shape[1]
        for name, g, n in (("o", self.o, P.s_q), ("dq", self.dq, P.s_q), ("dk", self.dk, P.s_k), ("dv", self.dv, P.s_k)):
            setattr(d, name, g.view.data_ptr())
            setattr(d, name + "_rs", g.buf.shape[1])
            setattr(d, name + "_bs", n * g.buf.shape[1])
        d.lse, d.dvec = self.lse.view.data_ptr(), self.dvec.view.data_ptr()
        if self.words is not None:
            d.keep_bits = self.words.view.data_ptr()
        if self.mask is not None:
            d.mask, d.mask_bs = self.mask.data_ptr(), (P.s_q * P.s_k if self.mask.shape[0] > 1 else 0)
        if self.index is not None:
            d.kv_index, d.kv_index_bs = self.index.data_ptr(), self.index.stride(0)
            if P.sparse is not None:
                d.kv_index_gs = self.index.stride(1)
                d.sparse_window, d.sparse_pivots, d.sparse_pivot_bias = P.sparse
        if colsum:
            d.colsum_partial = self.partial.view.data_ptr()
        for key, val in kw.items():
            assert hasattr(d, key), key
            setattr(d, key, val)
        return d

    def arm(self, forward=True):
        for g in (self.fwd_outputs if forward else []) + self.bwd_outputs:
            g.reset()

    def snapshot(self):
        return [g.buf.clone() for g in self.fwd_outputs + self.bwd_outputs]

    def stray(self):
        names = ((self.o, "o"), (self.dq, "dq"), (self.dk, "dk"), (self.dv, "dv"), (self.lse, "lse"), (self.dvec, "dvec"),
                 (self.words, "keep words"), (self.partial, "column-sum workspace"))
        return [f"guards of {name} written" for g, name in names if g is not None and not g.intact()]

    def untouched(self):
        return all(bool((g.buf == g.fill).all()) for g in self.fwd_outputs + self.bwd_outputs)

    def read(self):
        P = self.P
        t = lambda g, n: g.view.unflatten(0, (-1, n)).unflatten(-1, (P.H, 64)).permute(0, 2, 1, 3).double().cpu()
        R = dict(o=t(self.o, P.s_q), dq=t(self.dq, P.s_q), dk=t(self.dk, P.s_k), dv=t(self.dv, P.s_k),
                 lse=self.lse.view.view(P.B, P.H, P.s_q).double().cpu())
        if self.words is not None:
            R["words"] = self.words.bits.cpu()
        if self.partial is not None:
            R["partial"] = self.partial.view.view(P.B * self.nblk, 3 * P.H * 64).cpu()
        return R


class Launched:
    """the kernels, through the C ABI"""
    device = "cuda"

    def __init__(self, ops):
        self.stream = ops._stream

    def forward(self, S, d):
        rc = _lib.lib().cogv_attention_fwd(C.byref(d), self.stream())
        torch.cuda.synchronize()
        return rc

    def backward(self, S, d):
        rc = _lib.lib().cogv_attention_bwd(C.byref(d), self.stream())
        torch.cuda.synchronize()
        return rc


def run_cell(backend, P, colsum=True):
    """One cell: forward + backward, (a) - (e), sentinels, a second call -> (failures, ratios, code of the plan)"""
    S = Staged(P, backend.device)
    d = S.desc()
    out = (C.c_int * 8)()
    prc = _lib.lib().cogv_attention_plan(C.byref(d), 1, out)
    if prc != _lib.OK or out[0] != P.plan_form:
        return [f"planned {prc}, form {out[0]} instead of {P.plan_form}"], {}, prc
    rc = backend.forward(S, d)
    if rc == _lib.OK:
        rc = backend.backward(S, d)
    if rc != _lib.OK:
        return [f"the call answers {rc}"], {}, rc
    first = S.snapshot()
    R = S.read()
    fails, ratios = judge(P, R)
    fails += S.stray()
    if S.partial is not None and not bool((S.partial.buf == S.partial.fill).all()):
        fails.append("the column-sum workspace was written by a call that did not name it")
    S.arm()
    if backend.forward(S, d) != _lib.OK or backend.backward(S, d) != _lib.OK or not all(torch.equal(a, b) for a, b in zip(S.snapshot(), first)):
        fails.append("the second call gives other bits")
    if colsum and S.partial is not None:                                  # (e): the same backward with the fused bias gradient
        S.arm(forward=False)
        if backend.backward(S, S.desc(colsum=True)) != _lib.OK:
            fails.append("the call with colsum_partial fails")
        else:
            R2 = S.read()
            if not all(torch.equal(R2[n], R[n]) for n in ("dq", "dk", "dv")):
                fails.append("dq, dk or dv differ from the call without colsum_partial")
            if not bool((S.partial.bits != SENT32).all()):
                fails.append("the column-sum partials are not fully written")
            fails += judge_colsum(P, R2) + S.stray()
    return fails, ratios, _lib.OK


def sweep(backend, form, dtype, shapes=None):
    """every shape x kind of one (form, dtype): -> (failures: one line each, launched, refused, cells, {output and 'output / kind':
    worst err / bound})"""
    fails, ran, refused, cells, worst = [], 0, 0, 0, {}
    for shape in shapes or shapes_of(form):
        for kind in kinds_of(form):
            cells += 1
            P = problem(form, shape, kind, dtype)
            bad, ratios, rc = run_cell(backend, P)
            if rc == _lib.OK:
                ran += 1
            else:
                refused += 1
            fails += [f"{cell_tag(form, shape, kind, dtype)}: {b}" for b in bad]
            for name, r in ratios.items():                                # per output, over all kinds and per kind
                for key in (name, f"{name} / {kind}"):
                    worst[key] = max(worst.get(key, 0.0), r)
    return fails, ran, refused, cells, worst


# ------------------------------------------------------------------------------------------ (g) refusals through the launching calls
# (descriptor fields as in tests/test_attention_plan.py, backward call?, code): the launch answers the plan's code and writes nothing
REFUSALS = (
    (dict(dtype=2), 0, _lib.ERR_UNSUPPORTED), (dict(head_dim=128), 1, _lib.ERR_UNSUPPORTED), (dict(B=0), 0, _lib.ERR_ARG),
    (dict(s_k=-1), 1, _lib.ERR_ARG), (dict(s_q=64, s_k=32), 0, _lib.ERR_ARG), (dict(dropout_p=1.0), 0, _lib.ERR_ARG),
    (dict(dropout_p=float("nan")), 1, _lib.ERR_ARG), (dict(sparse_window=128), 1, _lib.ERR_ARG), (dict(q=0), 0, _lib.ERR_ARG),
    (dict(o_rs=7), 0, _lib.ERR_ARG), (dict(k_bs=12), 1, _lib.ERR_ARG), (dict(dq=0), 1, _lib.ERR_ARG), (dict(lse=0), 1, _lib.ERR_ARG),
    (dict(dq_rs=-2), 1, _lib.ERR_ARG), (dict(dv_bs=9), 1, _lib.ERR_ARG),
    (dict(q="misaligned"), 0, _lib.ERR_ARG), (dict(o="misaligned"), 1, _lib.ERR_ARG), (dict(dq="misaligned"), 1, _lib.ERR_ARG),
)
REFUSAL_SHAPE = (1, 2, 64, 64, 0)


def refusal_sweep(backend, dtype):
    fails = []
    P = problem("DENSE", REFUSAL_SHAPE, "randn", dtype)
    S = Staged(P, backend.device)
    for kw, backward, want in REFUSALS:
        kw = dict(kw)
        for key in ("q", "o", "dq"):                                      # "misaligned": the real pointer + 8 bytes
            if kw.get(key) == "misaligned":
                kw[key] = getattr(S.desc(), key) + 8
        d = S.desc(**kw)
        out = (C.c_int * 8)()
        prc = _lib.lib().cogv_attention_plan(C.byref(d), backward, out)
        rc = backend.backward(S, d) if backward else backend.forward(S, d)
        if (prc, rc) != (want, want):
            fails.append(f"{kw} {'backward' if backward else 'forward'}: the plan answers {prc} and the call {rc} where both must refuse with {want}")
        if not S.untouched():
            fails.append(f"{kw}: a refused call wrote an output or its guards")
            S.arm()
    return fails, len(REFUSALS)


# ------------------------------------------------------------------------------------------ fp32 emulation (CPU test fixture)
MUTANTS = {   # name -> (form, shape, kind) on which at least one check must reject it
    "diagonal key masked": ("DENSE", (1, 2, 127, 127, 0), "selector"),
    "first masked key visible": ("DENSE", (2, 1, 65, 65, 0), "decoy"),
    "last query row skipped": ("DENSE", (1, 2, 33, 161, 0), "selector"),
    "last key column skipped": ("DENSE", (1, 1, 257, 257, 0), "selector"),
    "sep_k short by one": ("DENSE", (1, 2, 96, 160, 5), "selector"),
    "D from the neighbouring row": ("DENSE", (3, 3, 129, 129, 0), "randn"),
    "keep mask shifted by one 4-key group": ("DENSE_DROP", (1, 1, 130, 194, 70), "selector"),
    "lse off by 2^-12": ("DENSE", (1, 2, 128, 128, 0), "randn"),
    "one element past o's last row": ("DENSE", (1, 3, 64, 64, 0), "randn"),
}
LOG2E = 1.4426950408889634


class Emulated:
    """The kernels' arithmetic in fp32 on the CPU: scores and accumulation in fp32, forward over 64-key blocks with a running
    maximum, P and dS rounded to the storage type, O rounded before D is formed from it, one rounding of every output."""
    device = "cpu"

    def __init__(self, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.mutant = mutant

    def _scores(self, S):
        P, f = S.P, torch.float32
        q, k, v, do = [t.permute(0, 2, 1, 3).float() for t in (S.q, S.k, S.v, S.do)]
        raw = q @ k.transpose(-1, -2)
        masked_raw = torch.tensor(-10000.0 / SCALE, dtype=f)
        if S.mask is not None:
            M = S.mask.float().unsqueeze(1)
            raw = raw * M + masked_raw * (1.0 - M)
        else:
            M = None
            sep_k = P.sep_k - 1 if self.mutant == "sep_k short by one" and P.sep_k > 0 else P.sep_k
            vis = ltr_visible(P.s_q, P.s_k, sep_k)
            i, j = torch.arange(P.s_q).view(-1, 1), torch.arange(P.s_k).view(1, -1)
            if self.mutant == "diagonal key masked":
                vis = vis & ~((j == i + P.off) & (j >= sep_k))
            if self.mutant == "first masked key visible":
                vis = vis | (j == i + P.off + 1)
            raw = torch.where(vis, raw, masked_raw)
        if self.mutant == "last key column skipped":
            raw[..., P.s_k - 1] = -float("inf")
        keep = None
        if P.p > 0:
            keep = decode_keep_words(S.words.bits, P.B, P.H, P.s_q, P.s_k)[..., :P.s_k] if P.bits and self._have_words else P.keep
            if self.mutant == "keep mask shifted by one 4-key group":
                keep = torch.roll(keep, -4, -1)
            keep = keep.float()
        kscale = 65536.0 / (65536.0 - O._thr16(P.p)) if P.p > 0 else 1.0
        return q, k, v, do, raw, M, keep, kscale

    def forward(self, S, d):
        P, dt, f = S.P, S.P.dtype, torch.float32
        self._have_words = False
        q, k, v, do, raw, M, keep, kscale = self._scores(S)
        sl2 = torch.tensor(SCALE * LOG2E, dtype=f)
        kofs = math.log2(kscale)
        m = torch.full((P.B, P.H, P.s_q, 1), -float("inf"), dtype=f)
        l, acc = torch.zeros_like(m), torch.zeros((P.B, P.H, P.s_q, 64), dtype=f)
        for k0 in range(0, P.s_k, 64):
            t = raw[..., k0:k0 + 64] * sl2
            m_new = torch.maximum(m, t.amax(-1, keepdim=True))
            alpha = torch.exp2(m - m_new)
            pv = torch.exp2(t + (kofs - m_new))
            l = l * alpha + pv.sum(-1, keepdim=True)
            if keep is not None:
                pv = pv * keep[..., k0:k0 + 64]
            acc = acc * alpha + pv.to(dt).float() @ v[..., k0:k0 + 64, :]
            m = m_new
        o = (acc * (kscale / l)).to(dt)
        lse = (m + torch.log2(l) - kofs).squeeze(-1) * 0.6931471805599453
        if self.mutant == "lse off by 2^-12":
            lse = lse + 2.0 ** -12
        rows = P.s_q - 1 if self.mutant == "last query row skipped" else P.s_q
        S.o.view.unflatten(0, (P.B, P.s_q)).unflatten(-1, (P.H, 64))[:, :rows].copy_(o.permute(0, 2, 1, 3)[:, :rows])
        S.lse.view.view(P.B, P.H, P.s_q).copy_(lse)
        if self.mutant == "one element past o's last row":
            S.o.buf[S.o.region[0].stop, 5] = 0
        if P.bits:                                                       # the words the forward kernel writes, from the oracle's mask
            nkb = (P.s_k + 63) // 64
            kp = torch.zeros((P.B, P.H, P.s_q, nkb * 64), dtype=torch.int64)
            kp[..., :P.s_k] = P.keep
            kp = kp.view(P.B, P.H, P.s_q, nkb, 64)
            w = torch.stack([(kp[..., KEY_OF_BIT[fg]] << (31 - _N)).sum(-1) for fg in (0, 1)], dim=-1)     # [B, H, q, kb, fg]
            w = w.permute(0, 1, 3, 4, 2)                                  # [B, H, kb, fg, q]
            w = torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)
            wrote = (torch.arange(nkb).view(-1, 1) * 64 < kend_of_query(P.s_q, P.s_k, P.sep_k).view(1, -1)).view(1, 1, nkb, 1, P.s_q)
            cur = S.words.bits.view(P.B, P.H, nkb, 2, P.s_q)
            cur.copy_(torch.where(wrote, w, cur))
        return _lib.OK

    def backward(self, S, d):
        P, dt, f = S.P, S.P.dtype, torch.float32
        self._have_words = True
        q, k, v, do, raw, M, keep, kscale = self._scores(S)
        o = S.o.view.unflatten(0, (P.B, P.s_q)).unflatten(-1, (P.H, 64)).permute(0, 2, 1, 3).float()
        lse2 = S.lse.view.view(P.B, P.H, P.s_q, 1) * torch.tensor(LOG2E, dtype=f)
        pr = torch.exp2(raw * torch.tensor(SCALE * LOG2E, dtype=f) - lse2)
        D = (do * o).sum(-1, keepdim=True)
        if self.mutant == "D from the neighbouring row":
            D = torch.roll(D, 1, -2)
        dp = do @ v.transpose(-1, -2)
        kp = keep * kscale if keep is not None else 1.0
        ds = pr * (dp * kp - D)
        if M is not None:
            ds = ds * M
        ds16, pd16 = ds.to(dt).float(), (pr * kp).to(dt).float()
        dq = ((ds16 @ k) * SCALE).to(dt)
        dk = ((ds16.transpose(-1, -2) @ q) * SCALE).to(dt)
        dv = (pd16.transpose(-1, -2) @ do).to(dt)
        rows_q = P.s_q - 1 if self.mutant == "last query row skipped" else P.s_q
        rows_k = P.s_k - 1 if self.mutant == "last key column skipped" else P.s_k
        for g, t, n, rows in ((S.dq, dq, P.s_q, rows_q), (S.dk, dk, P.s_k, rows_k), (S.dv, dv, P.s_k, rows_k)):
            g.view.unflatten(0, (P.B, n)).unflatten(-1, (P.H, 64))[:, :rows].copy_(t.permute(0, 2, 1, 3)[:, :rows])
        S.dvec.view.zero_()
        if d.colsum_partial:
            part = S.partial.view.view(P.B, S.nblk, 3, P.H, 64)
            for i, t in enumerate((dq, dk, dv)):
                for bx in range(S.nblk):
                    part[:, bx, i] = t[:, :, 128 * bx:128 * bx + 128].float().sum(2)
        return _lib.OK


# ------------------------------------------------------------------------------------------ (f) gathered and sparse forms
# gathered inference form (kv_index, forward only): (name, rows of the K / V pool, slots, dropout); B = 1, H = 2, s_q = 5
GATHER_CELLS = (("identity", 333, 333, False), ("sorted", 333, 200, True))
GATHER_FLAGGED = (0, 7, 64, 130)                                 # slots of the sorted table with bit 31 set
SPARSE = dict(B=1, H=2, w=128, s=384, times=2, n_piv=24)         # the sparse training cell
FLAG = -(1 << 31)


def _slots_reference(P):
    """fp64 reference of a problem in slot space, from the table's own semantics: slot j of (sample, block) reads row
    entry & 0x7fffffff of K / V, bit 31 masks it, the first n_piv slots take the bias, the block's queries are its last slots and the
    left-to-right rule runs on slots.  -> (outputs, bounds) with leading dimensions [B, H, G]"""
    B, H = P.B, P.H
    tab = P.index.to(torch.int64).view(B, -1, P.s_k)                       # [B, G, n]
    G, n = tab.shape[1], P.s_k
    wq = P.s_q // G
    rows, flag = tab & 0x7FFFFFFF, tab < 0
    take = lambda t: torch.stack([t[b][:, rows[b]] for b in range(B)])    # [B, H, G, n, 64]
    k, v = take(P.kpool), take(P.vpool)
    q, do = P.q.view(B, H, G, wq, 64), P.do.view(B, H, G, wq, 64)
    M = (ltr_visible(wq, n, 0).view(1, 1, wq, n) & ~flag.view(B, G, 1, n)).double().unsqueeze(1)      # [B, 1, G, wq, n]
    bias = None
    if P.sparse is not None:
        bias = torch.zeros(n, dtype=torch.float64)
        bias[:P.sparse[1]] = P.sparse[2]
    keep = None if P.keep is None else P.keep.view(B, H, G, wq, n)
    return reference(q, k, v, do, M, keep, P.p, P.dtype, bias)


def gather_problem(name, dtype):
    _, rows, n, drop = next(c for c in GATHER_CELLS if c[0] == name)
    B, H, s_q = 1, 2, 5
    g = torch.Generator().manual_seed(rows + n)
    P = SimpleNamespace(form="GATHER", plan_form=FLEXIBLE, shape=(B, H, s_q, n, 0), kind="randn", dtype=dtype, B=B, H=H, s_q=s_q, s_k=n,
                        sep=0, off=n - s_q, sep_k=0, bits=False, sel=None, M=None, keep=None, p=0.0, sparse=None)
    P.q, P.do = [torch.randn((B, H, s_q, 64), generator=g).to(dtype).double() for _ in range(2)]
    P.kpool, P.vpool = [torch.randn((B, H, rows, 64), generator=g).to(dtype).double() for _ in range(2)]
    if name == "identity":
        idx = torch.arange(n).view(1, n)
    else:
        idx = torch.sort(torch.randperm(rows, generator=g)[:n]).values.view(1, n)
        idx[0, list(GATHER_FLAGGED)] += FLAG
    P.index = idx.to(torch.int32)
    P.k = P.v = P.kpool[:, :, :n]                                         # (shapes only: the staged K / V are the pool)
    if drop:
        P.p, P.keep = P_RANDN, keep_mask(B, H, s_q, n, P_RANDN)
    return P


def sparse_table(pivot_idx, s, w, times):
    """[B, s // w, n_piv + times w] int32: block g's slots are the pivots (masked unless the pivot lies before the block's window,
    O.sparse_rmask) and the window keys (g - times + 1) w ... (g + 1) w - 1 (padding in front of the sequence: row 0, masked)"""
    B, n_piv = pivot_idx.shape
    G = s // w
    tab = torch.zeros((B, G, n_piv + times * w), dtype=torch.int64)
    for g in range(G):
        first = (g - times + 1) * w
        tab[:, g, :n_piv] = pivot_idx + FLAG * (pivot_idx >= first)
        win = first + torch.arange(times * w)
        tab[:, g, n_piv:] = win.clamp(min=0) + FLAG * (win < 0)
    return tab.to(torch.int32)


def fold_slots(ds, pivot_idx, s, w, times):
    """what cogv_sparse_slot_reduce documents: slot-space gradients [B, H, G, n, 64] -> [B, H, s, 64].  Key r is a window slot of the
    blocks g = r / w ... r / w + times - 1 (slot n_piv + r - (g - times + 1) w) and, when it is pivot j, slot j of every block
    g >= r / w + times."""
    B, H, G, n, _ = ds.shape
    n_piv = pivot_idx.shape[1]
    out = torch.zeros((B, H, s, 64), dtype=ds.dtype)
    for r in range(s):
        g0 = r // w
        for g in range(g0, min(G - 1, g0 + times - 1) + 1):
            out[:, :, r] += ds[:, :, g, n_piv + r - (g - times + 1) * w]
    for b in range(B):
        for j, r in enumerate(pivot_idx[b].tolist()):
            for g in range(r // w + times, G):
                out[b, :, r] += ds[b, :, g, j]
    return out


@functools.lru_cache(maxsize=None)
def sparse_problem(form, dtype, s=None):
    c = SPARSE
    B, H, w, times, n_piv = c["B"], c["H"], c["w"], c["times"], c["n_piv"]
    s = s or c["s"]
    g = torch.Generator().manual_seed(77 + s)
    n = n_piv + times * w
    P = SimpleNamespace(form=form, plan_form=FLEXIBLE, shape=(B, H, s, n, 0), kind="randn", dtype=dtype, B=B, H=H, s_q=s, s_k=n, sep=0,
                        off=0, sep_k=0, bits=False, sel=None, M=None, keep=None, p=0.0)
    P.q, P.kpool, P.vpool, P.do = [torch.randn((B, H, s, 64), generator=g).to(dtype).double() for _ in range(4)]
    P.k = P.v = P.kpool[:, :, :n]
    # distinct pivots, 7 of them inside the first block (visible to the blocks whose window starts after it)
    P.pivot_idx = torch.stack([torch.cat((torch.randperm(w, generator=g)[:7], w + torch.randperm(s - w, generator=g)[:n_piv - 7])) for _ in range(B)])
    P.index = sparse_table(P.pivot_idx, s, w, times)
    P.sparse = (w, n_piv, math.log(s // n_piv))
    P.times = times
    if form == "SPARSE_DROP":
        P.p, P.keep = P_RANDN, keep_mask(B, H, s, n, P_RANDN)
    return P


def _forward_backward(backend, S, d, backward=True):
    rc = backend.forward(S, d)
    if rc == _lib.OK and backward:
        rc = backend.backward(S, d)
    return rc


def gather_sweep(backend, dtype):
    """-> (failures, launched, {output: worst err / bound})"""
    fails, ran, worst = [], 0, {}
    for name, rows, n, _ in GATHER_CELLS:
        P = gather_problem(name, dtype)
        tag = f"GATHER {DT_NAME[dtype]} {name} table, {n} slots of {rows} rows"
        S = Staged(P, backend.device, kv_rows=rows)
        d = S.desc()
        out = (C.c_int * 8)()
        if _lib.lib().cogv_attention_plan(C.byref(d), 0, out) != _lib.OK or out[0] != FLEXIBLE:
            fails.append(f"{tag}: planned form {out[0]}")
            continue
        if backend.forward(S, d) != _lib.OK:
            fails.append(f"{tag}: the call fails")
            continue
        ran += 1
        first, R = S.snapshot(), S.read()
        ref, bound = _slots_reference(P)
        for nm in ("o", "lse"):
            got = R[nm].view(ref[nm].shape)
            r = ratio(got, ref[nm], bound[nm]) / FACTOR[("GATHER", nm)]
            worst[nm] = max(worst.get(nm, 0.0), r)
            if not r <= 1.0:
                fails.append(f"{tag}: {nm}: err / bound = {r:.3f}")
        fails += [f"{tag}: {b}" for b in S.stray()]
        S.arm()
        if backend.forward(S, d) != _lib.OK or not all(torch.equal(a, b) for a, b in zip(S.snapshot(), first)):
            fails.append(f"{tag}: the second call gives other bits")
        S.arm()                                                           # the plain gathered form is inference only
        if backend.backward(S, d) != _lib.ERR_UNSUPPORTED or not S.untouched():
            fails.append(f"{tag}: the backward call must refuse with {_lib.ERR_UNSUPPORTED} and write nothing")
    return fails, ran, worst


def sparse_cell(backend, form, dtype):
    """forward, dQ and the slot-space dK / dV of the sparse training form -> (failures, {output: err / bound})"""
    P = sparse_problem(form, dtype)
    B, H, s, n = P.B, P.H, P.s_q, P.s_k
    G = s // P.sparse[0]
    S = Staged(P, backend.device, kv_rows=s, planes=B * G)
    d = S.desc()
    out = (C.c_int * 8)()
    if _lib.lib().cogv_attention_plan(C.byref(d), 1, out) != _lib.OK or (out[0], out[6]) != (FLEXIBLE, B * G):
        return [f"planned form {out[0]}, {out[6]} planes"], {}
    if _forward_backward(backend, S, d) != _lib.OK:
        return ["the call fails"], {}
    first, R = S.snapshot(), S.read()
    ref, bound = _slots_reference(P)
    fails, ratios = [], {}
    got = dict(o=R["o"].view(B, H, G, -1, 64), dq=R["dq"].view(B, H, G, -1, 64), lse=R["lse"].view(B, H, G, -1),
               dk=R["dk"].view(B, G, H, n, 64).transpose(1, 2), dv=R["dv"].view(B, G, H, n, 64).transpose(1, 2))
    for nm in OUTPUTS:
        if bool(torch.isnan(got[nm]).any()):
            fails.append(f"{nm}: NaN")
        ratios[nm] = ratio(got[nm], ref[nm], bound[nm]) / FACTOR[(form, nm)]
        if not ratios[nm] <= 1.0:
            fails.append(f"{nm}: err / bound = {ratios[nm]:.3f}")
    flagged = (P.index < 0).view(B, 1, G, n, 1).expand_as(got["dk"])
    if bool((got["dk"][flagged] != 0).any()) or bool((got["dv"][flagged] != 0).any()):
        fails.append("a masked slot has a gradient that is not exactly 0")
    fails += S.stray()
    S.arm()
    if _forward_backward(backend, S, d) != _lib.OK or not all(torch.equal(a, b) for a, b in zip(S.snapshot(), first)):
        fails.append("the second call gives other bits")
    return [f"{form} {DT_NAME[dtype]}: {f}" for f in fails], ratios


def slot_reduce_cell(backend, dtype):
    """cogv_sparse_slot_reduce on integer slot gradients (|x| <= 4; a key has at most G <= 5 copies): bit-equal to fold_slots.
    s = 5 w, times = 2: keys that are window slots of two blocks and pivot slots of up to three (pivots in block 0), window slots
    only (not a pivot), a pivot no later block uses (last blocks), a window slot of one block (last block)."""
    B, H, w, times, n_piv, s = 2, 2, 128, 2, 24, 640
    G, n, C_ = s // w, n_piv + times * w, H * 64
    g = torch.Generator().manual_seed(5)
    pivot_idx = torch.stack([torch.cat((torch.randperm(w, generator=g)[:7], w + torch.randperm(s - w, generator=g)[:n_piv - 7])) for _ in range(B)])
    assert int((pivot_idx >= s - w).sum()) > 0 and int((pivot_idx < w).sum()) == 7 * B
    inv = torch.full((B, s), -1, dtype=torch.int32)
    inv.scatter_(1, pivot_idx, torch.arange(n_piv, dtype=torch.int32).expand(B, n_piv))
    dks, dvs = [torch.randint(-4, 5, (B, H, G, n, 64), generator=g).double() for _ in range(2)]
    want_k, want_v = fold_slots(dks, pivot_idx, s, w, times), fold_slots(dvs, pivot_idx, s, w, times)
    assert float(max(want_k.abs().max(), want_v.abs().max())) <= 4 * G <= 128
    dev = backend.device
    src = [Guard(B * G * n, C_, dtype, 0, nan=True, device=dev) for _ in range(2)]       # contiguous [B][G][n][H 64]
    for gd, t in zip(src, (dks, dvs)):
        gd.view.view(B, G, n, H, 64).copy_(t.permute(0, 2, 3, 1, 4))
    dk, dv = Guard(B * s, C_, dtype, 24, device=dev), Guard(B * s, C_, dtype, 8, device=dev)
    inv_d = inv.to(dev)
    fails = []

    def call():
        rc = _lib.lib().cogv_sparse_slot_reduce(DT_CODE[dtype], src[0].view.data_ptr(), src[1].view.data_ptr(), inv_d.data_ptr(),
                                                dk.view.data_ptr(), dv.view.data_ptr(), s * dk.buf.shape[1], dk.buf.shape[1],
                                                s * dv.buf.shape[1], dv.buf.shape[1], B, s, H, w, times, n_piv, backend.stream())
        torch.cuda.synchronize()
        return rc
    if call() != _lib.OK:
        return [f"slot reduce {DT_NAME[dtype]}: the call fails"]
    for name, gd, want in (("dk", dk, want_k), ("dv", dv, want_v)):
        got = gd.view.view(B, s, H, 64).permute(0, 2, 1, 3).double().cpu()
        if not torch.equal(got, want):
            fails.append(f"{name}: {int((got != want).any(-1).sum())} rows are not the fold of their slots")
        if not gd.intact():
            fails.append(f"guards of {name} written")
    first = (dk.buf.clone(), dv.buf.clone())
    dk.reset()
    dv.reset()
    if call() != _lib.OK or not (torch.equal(dk.buf, first[0]) and torch.equal(dv.buf, first[1])):
        fails.append("the second call gives other bits")
    return [f"slot reduce {DT_NAME[dtype]}: {f}" for f in fails]
