"""CPU: the launch plans of the wide decode products on quantized weights (cogv_gemm_rows_w8_plan / cogv_gemm_rows_w4_plan,
GWQ_CLASSES of csrc/gemv_wide_plan.h) as literals worked out by hand from the class list, every refusal with its code, header <->
ctypes <-> library, the opt-in `wide` keyword of the refusal rule, the routing of a 12-row quantized GraphDecoder._step on
recording stubs, and the proof that the GPU sweep's grid (tests/gemm_rows_q_cells.py) reaches every entry of both formats' plan
tables in both dtypes."""
import contextlib
import ctypes as C
import os
import re

import pytest
import torch

from cogview_amd import _lib
from cogview_amd import functional as F_
from cogview_amd.generation import GraphDecoder, decoder
from tests import gemm_rows_q_cells as QC

ARG, UNS = _lib.ERR_ARG, _lib.ERR_UNSUPPORTED
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cogv_gemm_rows_w8", "cogv_gemm_rows_w4", "cogv_gemm_rows_w8_plan", "cogv_gemm_rows_w4_plan")

# one K per class of GWQ_CLASSES: (NWK waves per tile, LP units of 128 contraction elements per wave at most, guarded)
CLASS_OF_K = {1024: (4, 2, 0), 2560: (4, 5, 0), 4096: (8, 4, 0), 10240: (8, 10, 0), 512: (4, 2, 1), 1536: (4, 5, 1), 5632: (8, 10, 1)}
LOADS = {"e4m3": 2, "mxfp4": 1}                 # 16-byte weight loads of a lane per unit and column tile
# units in flight = floor((256 - 4 RG CT - 40 - 16 [- 8: e4m3's row scales]) / (16 RG + (8 | 5) CT)), at most LP: by hand per (RG, CT)
DEPTH = {"e4m3": {(1, 1): 7, (2, 1): 4, (2, 2): 3, (3, 1): 3, (3, 2): 2, (4, 1): 2, (4, 2): 2},       # 188/24 184/40 176/48 180/56 168/64 176/72 160/80
         "mxfp4": {(1, 1): 9, (2, 1): 5, (2, 2): 4, (3, 1): 3, (3, 2): 3, (4, 1): 2, (4, 2): 2}}      # 196/21 192/37 184/42 188/53 176/58 184/69 168/74
# dynamic LDS = R (NWK + 1) KB, R = min(RG CT tiles, NWK, 32 / NWK) tiles summed per round
LDS = {4: {1: 5120, 2: 10240, 3: 15360, 4: 20480, 6: 20480, 8: 20480}, 8: {1: 9216, 2: 18432, 3: 27648, 4: 36864, 6: 36864, 8: 36864}}


def _expected(fmt, M, N, K):
    nwk, lp, guard = CLASS_OF_K[K]
    rg = {1: 1, 16: 1, 17: 2, 32: 2, 33: 3, 48: 3, 49: 4, 64: 4}[M]
    ct = 2 if (rg >= 2 and N >= 4096) else 1
    return [rg, nwk, ct, LOADS[fmt] * lp * ct, guard, 0, 64 * nwk, -(-N // (16 * ct)), LDS[nwk][rg * ct], min(lp, DEPTH[fmt][(rg, ct)])]


@pytest.mark.parametrize("fmt", QC.FORMATS)
@pytest.mark.parametrize("dtype", QC.DTYPES, ids=QC.DT_NAME.get)
def test_plan_integers_of_every_row_group_and_class(fmt, dtype):
    for K in CLASS_OF_K:
        for M in (1, 16, 17, 32, 33, 48, 49, 64):
            for N in (40, 136, 4096, 4104):
                rc, out = QC.plan(fmt, dtype, M, N, K)
                assert rc == _lib.OK and out == _expected(fmt, M, N, K), (M, N, K, out, _expected(fmt, M, N, K))
    # spelled out: the 4B step's products at 12 and 24 rows, and a guarded class with two tiles
    want = {"e4m3": ([1, 4, 1, 10, 0, 0, 256, 160, 5120, 5], [2, 8, 1, 20, 0, 0, 512, 160, 18432, 4], [4, 8, 2, 40, 1, 0, 512, 129, 36864, 2]),
            "mxfp4": ([1, 4, 1, 5, 0, 0, 256, 160, 5120, 5], [2, 8, 1, 10, 0, 0, 512, 160, 18432, 5], [4, 8, 2, 20, 1, 0, 512, 129, 36864, 2])}[fmt]
    assert QC.plan(fmt, dtype, 12, 2560, 2560)[1] == want[0]
    assert QC.plan(fmt, dtype, 24, 2560, 10240)[1] == want[1]
    assert QC.plan(fmt, dtype, 64, 4104, 5632)[1] == want[2]
    # strided operands plan like contiguous ones
    kw = dict(ldq=2560 + 16) if fmt == "e4m3" else dict(ldq=1280 + 16, lds=96)
    assert QC.plan(fmt, dtype, 12, 2560, 2560, **kw)[1] == want[0]


def _desc(M=16, N=40, K=512, dtype=_lib.F16, **kw):
    d = _lib.GemmDesc()
    d.dtype, d.M, d.N, d.K, d.lda, d.ldb, d.ldc, d.splitk = dtype, M, N, K, K, K, N, 1
    d.A, d.B, d.C = 0x1000, 0x2000, 0x3000
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _w8(K=512, **kw):
    w = _lib.W8Weight()
    w.q, w.ldq, w.scale = 0x2000, K, 0x4000
    for k, v in kw.items():
        setattr(w, k, v)
    return w


def _w4(K=512, **kw):
    w = _lib.W4Weight()
    w.q, w.ldq, w.scale, w.lds = 0x2000, K // 2, 0x4001, K // 32               # (the block scales are bytes: no alignment asked)
    for k, v in kw.items():
        setattr(w, k, v)
    return w


# (descriptor fields, operand fields, code): cogv_gemm_rows' codes, and 1 for what cogv_gemm_w8 / cogv_gemm_w4 call a bad operand
DESC_REFUSALS = [
    (dict(M=0), ARG), (dict(M=65), UNS), (dict(N=44), ARG), (dict(K=768, lda=768), UNS), (dict(K=256, lda=256), UNS),
    (dict(K=10752, lda=10752), UNS), (dict(trans_a=1), UNS), (dict(trans_b=1), UNS), (dict(flags=_lib.EPI_ACCUM), UNS),
    (dict(flags=_lib.EPI_BIAS | _lib.EPI_DROPOUT, bias=0x4000), UNS), (dict(dtype=_lib.F32), UNS), (dict(out_f32=1), UNS), (dict(splitk=2), UNS),
    (dict(lda=504), ARG), (dict(flags=_lib.EPI_BIAS), ARG), (dict(A=0x1008), ARG), (dict(C=0x3004), ARG), (dict(flags=_lib.EPI_BIAS, bias=0x4008), ARG),
]
W8_REFUSALS = [(dict(q=0), ARG), (dict(scale=0), ARG), (dict(q=0x2008), ARG), (dict(scale=0x4004), ARG), (dict(ldq=520), ARG), (dict(ldq=496), ARG)]
W4_REFUSALS = [(dict(q=0), ARG), (dict(scale=0), ARG), (dict(q=0x2008), ARG), (dict(ldq=264), ARG), (dict(ldq=240), ARG), (dict(lds=15), ARG)]


def _refusals(fmt):
    """(descriptor, operand, code) of every refusal of a format"""
    mk = _w8 if fmt == "e4m3" else _w4
    for kw, code in DESC_REFUSALS:
        K = kw.get("K", 512)
        yield _desc(**kw), mk(K), code, kw
    for kw, code in (W8_REFUSALS if fmt == "e4m3" else W4_REFUSALS):
        yield _desc(), mk(512, **kw), code, kw


@pytest.mark.parametrize("fmt", QC.FORMATS)
def test_every_refusal_with_its_code_and_out_untouched(fmt):
    lib = _lib.lib()
    query = _lib.gemm_rows_w8_plan if fmt == "e4m3" else _lib.gemm_rows_w4_plan
    launch, raw = (lib.cogv_gemm_rows_w8, lib.cogv_gemm_rows_w8_plan) if fmt == "e4m3" else (lib.cogv_gemm_rows_w4, lib.cogv_gemm_rows_w4_plan)
    for d, w, code, kw in _refusals(fmt):
        rc, out = query(None, 0, 0, 0, desc=d, w=w)
        assert rc == code and out == [-1] * _lib.GEMM_ROWS_PLAN_INTS, (kw, rc, out)
        # a refused call is refused by the launch before anything is touched (no device here)
        assert launch(C.byref(d), C.byref(w), None) == code, kw
    out = (C.c_int * _lib.GEMM_ROWS_PLAN_INTS)()
    good = _w8() if fmt == "e4m3" else _w4()
    assert raw(None, C.byref(good), out) == ARG and raw(C.byref(_desc()), None, out) == ARG and raw(C.byref(_desc()), C.byref(good), None) == ARG
    assert launch(None, None, None) == ARG and launch(C.byref(_desc()), None, None) == ARG
    assert raw(C.byref(_desc()), C.byref(good), out) == _lib.OK             # (the stand-ins above are a good call)


def test_header_ctypes_and_library_agree():
    header = open(os.path.join(ROOT, "include", "cogview_hip.h")).read()
    lib = _lib.lib()
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/cogview_hip.h"
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(m.group(1).split(",")), name
        assert getattr(lib, name) is not None
    assert int(re.search(r"#define\s+COGV_GEMM_ROWS_PLAN_INTS\s+(\d+)", header).group(1)) == _lib.GEMM_ROWS_PLAN_INTS
    # the skinny entry points keep their 8 rows
    assert lib.cogv_gemm_w8(C.byref(_desc(M=9)), C.byref(_w8()), None) == UNS
    assert lib.cogv_gemm_w4(C.byref(_desc(M=9)), C.byref(_w4()), None) == UNS


def _model(dtype=torch.float16, hidden=512, heads=8, layers=1):
    from cogview_amd.model import GPT2Model
    torch.manual_seed(0)
    return GPT2Model(layers, 64, hidden, heads, 0.0, 0.0, 0.0, 32, 32, False).to(dtype).eval()


@pytest.mark.parametrize("fmt", QC.FORMATS)
def test_refusal_rule_with_and_without_wide(fmt):
    for dtype in QC.DTYPES:
        m = _model(dtype)
        for rows in (9, 12, 33, 64):
            assert F_.decode_wide_q_supported(m.transformer, rows, fmt) is None
            decoder.refuse_unsupported(weights=fmt, batch=rows, model=m, wide=True)
        for rows in (8, 65):
            assert isinstance(F_.decode_wide_q_supported(m.transformer, rows, fmt), str)
        with pytest.raises(NotImplementedError, match="65 rows"):
            decoder.refuse_unsupported(weights=fmt, batch=65, model=m, wide=True)
        # up to 8 rows the keyword changes nothing: the skinny kernels' plan is asked
        decoder.refuse_unsupported(weights=fmt, batch=8, model=m, wide=True)
        # without the keyword: the parent's refusal, word for word
        for kw in (dict(), dict(wide=False)):
            with pytest.raises(NotImplementedError) as e:
                decoder.refuse_unsupported(weights=fmt, batch=9, model=m, **kw)
            assert str(e.value) == f"weights={fmt!r}: batch 9 > 8 rows"
        # chunk keeps batch * chunk <= 8
        with pytest.raises(ValueError, match="batch \\* chunk <= 8"):
            decoder.refuse_unsupported(weights=fmt, batch=9, model=m, chunk=2, wide=True)
    with pytest.raises(NotImplementedError, match="float32"):
        decoder.refuse_unsupported(weights=fmt, batch=12, model=_model(torch.float32), wide=True)
    with pytest.raises(NotImplementedError, match="contraction length 320"):
        decoder.refuse_unsupported(weights=fmt, batch=12, model=_model(hidden=320, heads=5), wide=True)
    # 16-bit weights: the keyword has no effect
    decoder.refuse_unsupported(batch=12, model=_model(), wide=True)


def test_one_partition_only(monkeypatch):
    monkeypatch.setattr(F_, "mp_world_size_or_1", lambda: 2)
    assert isinstance(F_.decode_wide_q_supported(_model().transformer, 12, "e4m3"), str)


class _Ops:
    """recording stand-ins for the ops a layer-by-layer decode step calls (tests/test_gemm_rows_plan.py's pattern)"""

    def __init__(self):
        self.calls = []

    @staticmethod
    def scalar_slab(slab):
        return contextlib.nullcontext()

    def _quant(self, name, w):
        return (name, tuple(w.shape))

    def quantize_rows_e4m3(self, w):
        return self._quant("e4m3", w)

    def quantize_rows_mxfp4(self, w):
        return self._quant("mxfp4", w)

    def _rows(self, name, a, qs, gelu):
        assert qs[0] == {"gemm_rows_w8": "e4m3", "gemm_rows_w4": "mxfp4"}[name]
        self.calls.append((name, qs[1], a.shape[0], gelu))
        return torch.zeros(a.shape[0], qs[1][0], dtype=a.dtype)

    def gemm_rows_w8(self, a, qs, bias=None, gelu=False, absmax=None, out=None):
        return self._rows("gemm_rows_w8", a, qs, gelu)

    def gemm_rows_w4(self, a, qs, bias=None, gelu=False, absmax=None, out=None):
        return self._rows("gemm_rows_w4", a, qs, gelu)

    def gemm_rows(self, *a, **k):
        self.calls.append(("gemm_rows",))
        raise AssertionError("the 16-bit wide product on a quantized decoder")

    def gemm_w8(self, *a, **k):
        raise AssertionError("the skinny product above 8 rows")

    gemm_w4 = gemm = gemm_w8

    def attention_decode(self, qkv, cache, pos_index, heads, combine=True):
        self.calls.append(("attention_decode", combine))
        return torch.zeros(qkv.shape[0], 1, heads * 64, dtype=qkv.dtype)

    def sandwich_ln_fwd(self, x, gamma, beta, eps, absmax_in, residual=None, absmax_out=None, save_stats=True):
        self.calls.append(("ln",))
        return torch.zeros(x.shape, dtype=gamma.dtype), None, None

    @staticmethod
    def new_absmax_slot(dev):
        return torch.zeros(1)


@pytest.mark.parametrize("fmt,name", (("e4m3", "gemm_rows_w8"), ("mxfp4", "gemm_rows_w4")))
def test_twelve_row_quantized_step_routes_every_product_to_the_wide_form(monkeypatch, fmt, name):
    L_, V_, H_, rows = 2, 64, 512, 12
    m = _model(layers=L_)
    o = _Ops()
    monkeypatch.setattr(F_, "ops", o)
    monkeypatch.setattr(decoder, "ops", o)
    with pytest.raises(NotImplementedError):
        GraphDecoder(m, batch=rows, capacity=64, weights=fmt)
    dec = GraphDecoder(m, batch=rows, capacity=64, weights=fmt, wide=True)
    assert dec.wide_q and dec.wq is not None
    tr = m.transformer
    h0 = torch.zeros(rows, 1, H_, dtype=torch.float16)
    h0._cogv_absmax = torch.ones(1)
    monkeypatch.setattr(type(tr), "embed", lambda self, tok, pos, emb: h0)
    logits = dec._step()
    assert logits.shape == (rows, 1, V_)
    prods = [c for c in o.calls if c[0] == name]
    assert len(prods) == 4 * L_ + 1 and {c[0] for c in o.calls} == {name, "ln", "attention_decode"}
    assert [c[1] for c in prods] == [(3 * H_, H_), (H_, H_), (4 * H_, H_), (H_, 4 * H_)] * L_ + [(V_, H_)]
    assert [c[3] for c in prods] == [False, False, True, False] * L_ + [False] and {c[2] for c in prods} == {rows}
    # up to 8 rows the keyword changes nothing
    assert not GraphDecoder(m, batch=8, capacity=64, weights=fmt, wide=True).wide_q
    assert not GraphDecoder(m, batch=12, capacity=64, wide=True).wide_q


def test_the_gpu_sweep_grid_reaches_every_plan():
    """Every distinct entry of a format's plan table -- (class, row groups, tiles per workgroup) with everything that follows from
    them -- over ALL shapes the kernel takes has a cell in the grid of tests/test_gemm_rows_q_gpu.py, in both dtypes."""
    for fmt in QC.FORMATS:
        for dtype in QC.DTYPES:
            every = {}
            for K in range(512, 10240 + 1, 512):
                for M in range(1, 65):
                    for N in (8, 4088, 4096, 65536):
                        rc, out = QC.plan(fmt, dtype, M, N, K)
                        assert rc == _lib.OK, (M, N, K)
                        every.setdefault(QC.plan_id(out), (M, N, K))
            grid = {QC.plan_id(QC.plan(fmt, dtype, M, N, K)[1]) for K in QC.KS for M in QC.MS for N in QC.NS}
            assert len(every) == 7 * 7                               # 7 classes x (1 row group | 2, 3, 4 with one or two tiles)
            missing = {pid: where for pid, where in every.items() if pid not in grid}
            assert not missing, missing
