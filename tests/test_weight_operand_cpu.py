"""CPU: what the skinny decode products (M <= 8: plain, combine prologue, LayerNorm prologue) refuse, with which code, on the three
weight operands -- 16-bit weights in d->B, E4M3 (cogv_w8_weight), MXFP4 (cogv_w4_weight) -- as one literal table.  Every cell is a
fault (or two: the order of the checks) in an otherwise good call of M = 1, N = 8, K = 512 on stand-in pointers; the plan query
must answer the tabled code and leave `out` alone, and the launching entry point must answer the same code before it touches a
device.  The two-fault cells carry the wide entry points' (cogv_gemm_rows*) answers next to the skinny ones: the two fronts check
the operand at different points relative to the shape, and the table shows where.  tests/test_gemm_rows_q_plan.py has the wide
products' own refusals."""
import ctypes as C

import pytest

from cogview_amd import _lib

KINDS = ("plain", "attn", "ln")
FORMATS = ("w16", "e4m3", "mxfp4")
M, N, K = 1, 8, 512
_ = None                                   # the fault does not exist for that kind or format


def _desc(fmt, fields, faults):
    if fields is None:
        return None
    k = fields.get("K", K)
    d = _lib.GemmDesc()
    d.dtype, d.M, d.N, d.K, d.lda, d.ldb, d.ldc, d.splitk = _lib.F16, M, N, k, k, k, 16, 1
    d.A, d.B, d.C = 0x1000, 0x2000, 0x3000
    for name, v in fields.items():
        setattr(d, name, v)
    if fmt == "w16":                       # the 16-bit operand is the descriptor's B / ldb: elements, so 8 of them are 16 bytes
        for f in faults:
            if f == "q_null":
                d.B = 0
            elif f == "q_off8":
                d.B = 0x2008
            elif f == "ld_mod16":
                d.ldb = k + 4
            elif f == "ld_short":
                d.ldb = k - 8
    return d


def _operand(fmt, k, faults):
    """the quantized operand of a K = k product with the named faults; None: a NULL operand"""
    if faults is None:
        return None
    if fmt == "e4m3":
        w = _lib.W8Weight()
        w.q, w.ldq, w.scale = 0x2000, k, 0x4000
    else:
        w = _lib.W4Weight()
        w.q, w.ldq, w.scale, w.lds = 0x2000, k // 2, 0x4000, k // 32
    for f in faults:
        if f == "q_null":
            w.q = 0
        elif f == "scale_null":
            w.scale = 0
        elif f == "q_off8":
            w.q = 0x2008
        elif f == "scale_off4":
            w.scale = 0x4004
        elif f == "ld_mod16":
            w.ldq += 8
        elif f == "ld_short":
            w.ldq -= 16
        elif f == "lds_short":
            w.lds -= 1
    return w


def _prologue(fields):
    ln = _lib.LnPrologue()
    ln.z, ln.gamma, ln.beta, ln.eps = 0x8000, 0x9000, 0xA000, 1e-5
    ln.gamma_post, ln.beta_post, ln.residual = 0xB000, 0xC000, 0xD000
    for name, v in fields.items():
        setattr(ln, name, v)
    return ln


# which faults a kind or a format has at all
_OPERAND_ONLY = {"scale_null", "scale_off4", "lds_short"}        # no such thing on 16-bit weights
_W4_ONLY = {"lds_short"}


def applies(kind, fmt, fault):
    w = fault.get("w", ())
    if w is None:
        return fmt != "w16"                                        # (a NULL operand IS the 16-bit call)
    if fmt == "w16" and _OPERAND_ONLY & set(w) or fmt == "e4m3" and _W4_ONLY & set(w):
        return False
    if kind == "wide":
        return "ln" not in fault and "nsplit" not in fault
    return ("ln" not in fault or kind == "ln") and ("nsplit" not in fault or kind == "attn")


def observe(kind, fmt, fault, launch):
    """(the plan query's code, whether it left out alone, the launching entry point's code or None where `launch` is False) of a
    cell at a skinny kind or at the wide entry points (kind "wide")"""
    lib = _lib.lib()
    fields, faults = fault.get("d", {}), fault.get("w", ())
    d = _desc(fmt, fields, faults or ())
    k = K if fields is None else fields.get("K", K)
    w = None if fmt == "w16" else _operand(fmt, k, faults)
    dp, wp = (None if d is None else C.byref(d)), (None if w is None else C.byref(w))
    sfx = {"w16": "", "e4m3": "_w8", "mxfp4": "_w4"}[fmt]
    if kind == "wide":
        n = _lib.GEMM_ROWS_PLAN_INTS
        out = (C.c_int * n)(*([-1] * n))
        extra = () if fmt == "w16" else (wp,)
        rc = getattr(lib, f"cogv_gemm_rows{sfx}_plan")(dp, *extra, out)
        return rc, list(out) == [-1] * n, getattr(lib, f"cogv_gemm_rows{sfx}")(dp, *extra, None) if launch else None
    n = _lib.GEMV_PLAN_INTS
    out = (C.c_int * n)(*([-1] * n))
    nsplit = fault.get("nsplit", 1)
    query = lib.cogv_gemv_w4_plan if fmt == "mxfp4" else lib.cogv_gemv_plan
    rc = query(KINDS.index(kind), dp, wp, nsplit, out)
    got = None
    if launch:
        extra = () if fmt == "w16" else (wp,)
        if kind == "plain":
            got = getattr(lib, "cogv_gemm" + sfx)(dp, *extra, None)
        elif kind == "attn":
            got = getattr(lib, "cogv_gemv_attn" + sfx)(dp, *extra, 0x7000, k // 64, 128 * nsplit, None)
        else:
            got = getattr(lib, "cogv_gemv_ln" + sfx)(dp, C.byref(_prologue(fault.get("ln", {}))), *extra, None)
    return rc, list(out) == [-1] * n, got


def launches(kind, fmt, code):
    """Whether a cell's launching entry point is called: only where it must refuse, so nothing is ever launched.  cogv_gemm hands
    what the skinny kernels do not take (3) to the tile kernels, so on 16-bit weights its plain kind is called for bad arguments
    alone."""
    launch_code = code[1] if isinstance(code, tuple) else code
    return launch_code != 0 and not (kind == "plain" and fmt == "w16" and launch_code != 1)


BIAS, COLSUM, GELU = _lib.EPI_BIAS, _lib.EPI_COLSUM, _lib.EPI_GELU
# (cell, fault, codes of plain | combine | LayerNorm on 16-bit, E4M3, MXFP4 weights, codes of the wide entry points on the same or None)
# 0: accepted (the query fills out; no launch is made).  (q, l): the plan query answers q and the launch l -- the query is not given
# the prologue, cogv_gemv_plan with a NULL operand IS the 16-bit query, and 33 key splits cannot be asked of a launch (its capacity
# ends at 4096: 1).  The codes were recorded from a build of the commit before the host paths were merged into one; they are never taken
# from the code under test.
CELLS = [
    ("NULL descriptor", dict(d=None),
     (1, 1, 1,  1, 1, 1,  1, 1, 1), None),
    ("NULL operand", dict(w=None),
     (_, (0, 1), 1,  _, (0, 1), 1,  _, (0, 1), 1), None),
    ("NULL q", dict(w=('q_null',)),
     (0, 1, 1,  0, 1, 1,  0, 1, 1), None),
    ("NULL scale", dict(w=('scale_null',)),
     (_, 1, 1,  _, 1, 1,  _, 1, 1), None),
    ("q off by 8 bytes", dict(w=('q_off8',)),
     (1, 1, 1,  1, 1, 1,  1, 1, 1), None),
    ("scale off by 4 bytes", dict(w=('scale_off4',)),
     (_, 1, 0,  _, 1, 0,  _, 1, 0), None),
    ("ldq % 16 != 0", dict(w=('ld_mod16',)),
     (1, 1, 1,  1, 1, 1,  1, 1, 1), None),
    ("ldq 16 bytes short of a row", dict(w=('ld_short',)),
     (0, 3, 3,  0, 3, 3,  0, 3, 3), None),
    ("lds = K / 32 - 1", dict(w=('lds_short',)),
     (_, _, 1,  _, _, 1,  _, _, 1), None),
    ("M = 9", dict(d=dict(M=9)),
     (3, 3, 3,  3, 3, 3,  3, 3, 3), None),
    ("N = 12", dict(d=dict(N=12)),
     (1, 3, 3,  1, 3, 3,  1, 3, 3), None),
    ("K = 768", dict(d=dict(K=768)),
     (3, 3, 3,  3, 3, 3,  3, 3, 3), None),
    ("K = 10752", dict(d=dict(K=10752)),
     (0, 3, 3,  0, 3, 3,  3, 3, 3), None),
    ("trans_b", dict(d=dict(trans_b=1)),
     (3, 3, 3,  3, 3, 3,  3, 3, 3), None),
    ("COLSUM flag", dict(d=dict(flags=COLSUM, colsum_partial=0x5000)),
     (3, 3, 3,  3, 3, 3,  3, 3, 3), None),
    ("GELU flag", dict(d=dict(flags=GELU)),
     (0, 0, 0,  3, 3, 3,  0, 0, 0), None),
    ("out_f32", dict(d=dict(out_f32=1)),
     (0, 3, 3,  3, 3, 3,  3, 3, 3), None),
    ("splitk = 2", dict(d=dict(splitk=2, workspace=0x10000, workspace_bytes=1 << 20)),
     (0, 3, 3,  3, 3, 3,  3, 3, 3), None),
    ("aux set", dict(d=dict(aux=0x6000, ldaux=8)),
     (0, 3, 3,  0, 0, 0,  0, 3, 3), None),
    ("K = 4608", dict(d=dict(K=4608)),
     (0, 0, 0,  0, 0, 0,  3, 3, 3), None),
    ("nsplit = 33", dict(nsplit=33),
     (_, _, _,  (0, 1), (3, 1), (3, 1),  _, _, _), None),
    ("NULL gamma", dict(ln=dict(gamma=0)),
     (_, _, _,  _, _, _,  (0, 1), (0, 1), (0, 1)), None),
    ("residual off by 8 bytes", dict(ln=dict(residual=0xD008)),
     (_, _, _,  _, _, _,  (0, 1), (0, 1), (0, 1)), None),
    ("M = 9 and q off by 8 bytes", dict(d=dict(M=9), w=('q_off8',)),
     (1, 3, 3,  1, 3, 3,  1, 3, 3), (1, 1, 1)),
    ("N = 12 and NULL q", dict(d=dict(N=12), w=('q_null',)),
     (1, 1, 1,  1, 1, 1,  1, 1, 1), (1, 1, 1)),
    ("trans_b and scale off by 4 bytes", dict(d=dict(trans_b=1), w=('scale_off4',)),
     (_, 3, 3,  _, 3, 3,  _, 3, 3), (_, 1, 3)),
    ("out_f32 and lds = K / 32 - 1", dict(d=dict(out_f32=1), w=('lds_short',)),
     (_, _, 3,  _, _, 3,  _, _, 3), (_, _, 1)),
    ("short ldq and lds = K / 32 - 1", dict(w=('ld_short', 'lds_short')),
     (_, _, 1,  _, _, 1,  _, _, 1), (_, _, 1)),
    ("K = 768 and short ldq", dict(d=dict(K=768), w=('ld_short',)),
     (3, 3, 3,  3, 3, 3,  3, 3, 3), (1, 1, 1)),
    ("M = 9 and a BIAS flag without bias", dict(d=dict(M=9, flags=BIAS)),
     (1, 3, 3,  1, 3, 3,  1, 3, 3), (1, 1, 1)),
    ("aux set and ldq % 16 != 0", dict(d=dict(aux=0x6000, ldaux=8), w=('ld_mod16',)),
     (1, 1, 1,  1, 1, 1,  1, 1, 1), (1, 1, 1)),
    ("K = 4608 and NULL gamma", dict(d=dict(K=4608), ln=dict(gamma=0)),
     (_, _, _,  _, _, _,  3, 3, 3), None),
    ("short ldq and residual off by 8 bytes", dict(w=('ld_short',), ln=dict(residual=0xD008)),
     (_, _, _,  _, _, _,  (0, 1), (3, 1), (3, 1)), None),
]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("kind", KINDS)
def test_every_cell_with_its_code_and_out_untouched(kind, fmt):
    col = 3 * KINDS.index(kind) + FORMATS.index(fmt)
    seen = 0
    for name, fault, codes, wide in CELLS:
        code = codes[col]
        assert (code is not None) == applies(kind, fmt, fault), name
        if code is None:
            continue
        q, l = code if isinstance(code, tuple) else (code, code)
        launch = launches(kind, fmt, code)
        rc, untouched, got = observe(kind, fmt, fault, launch)
        assert rc == q and untouched == (q != 0), (name, rc, untouched)
        assert not launch or got == l, (name, got)
        seen += 1
    assert seen >= 20


@pytest.mark.parametrize("fmt", FORMATS)
def test_the_two_fault_cells_at_the_wide_entry_points(fmt):
    seen = 0
    for name, fault, codes, wide in CELLS:
        if wide is None:
            continue
        code = wide[FORMATS.index(fmt)]
        assert (code is not None) == applies("wide", fmt, fault), name
        if code is None:
            continue
        rc, untouched, got = observe("wide", fmt, fault, code != 0)
        assert rc == code and untouched == (code != 0) and (code == 0 or got == code), (name, rc, untouched, got)
        seen += 1
    assert seen >= 4


def test_the_good_call_is_taken_everywhere():
    for kind in KINDS + ("wide",):
        for fmt in FORMATS:
            rc, untouched, got = observe(kind, fmt, {}, False)
            assert rc == _lib.OK and not untouched, (kind, fmt)
