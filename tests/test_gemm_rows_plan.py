"""CPU: the launch plan of the wide decode products (cogv_gemm_rows_plan, csrc/gemv_wide_plan.h) as literals worked out by hand
from the class list, every refusal with its code, functional.decode_wide_supported on toy models, the routing of a 12-row and
an 8-row GraphDecoder._step on recording stubs, and the proof that the GPU sweep's grid (tests/gemm_rows_cells.py) reaches
every entry of the plan table in both dtypes."""
import contextlib
import ctypes as C

import pytest
import torch

from cogview_amd import _lib
from cogview_amd import functional as F_
from cogview_amd.generation import GraphDecoder, decoder
from tests import gemm_rows_cells as RC

ARG, UNS = _lib.ERR_ARG, _lib.ERR_UNSUPPORTED

# one K per class of GW_CLASSES: (NWK waves per tile, LP load pairs per wave at most, guarded)
CLASS_OF_K = {1024: (4, 4, 0), 2560: (8, 5, 0), 4096: (16, 4, 0), 10240: (16, 10, 0), 512: (4, 4, 1), 1536: (8, 5, 1), 5632: (16, 10, 1)}
# load pairs in flight = floor((registers - 4 RG CT - 40) / (8 (RG + CT))), registers = 128 at 16 waves and 256 below, at most LP:
# by hand, per (NWK, LP) and (RG, CT)
DEPTH = {
    (4, 4): {(1, 1): 4, (2, 1): 4, (2, 2): 4, (3, 1): 4, (3, 2): 4, (4, 1): 4, (4, 2): 3},          # 13, 8, 6, 6, 4, 5 -> LP = 4; 184 / 48 = 3
    (8, 5): {(1, 1): 5, (2, 1): 5, (2, 2): 5, (3, 1): 5, (3, 2): 4, (4, 1): 5, (4, 2): 3},          # 192 / 40 = 4; 184 / 48 = 3
    (16, 4): {(1, 1): 4, (2, 1): 3, (2, 2): 2, (3, 1): 2, (3, 2): 1, (4, 1): 1, (4, 2): 1},         # 84 / 16 = 5 -> 4; 80 / 24; 72 / 32; 76 / 32; 64 / 40; 72 / 40; 56 / 48
    (16, 10): {(1, 1): 5, (2, 1): 3, (2, 2): 2, (3, 1): 2, (3, 2): 1, (4, 1): 1, (4, 2): 1},
}
# dynamic LDS = R (NWK + 1) KB, R = min(RG CT tiles, NWK, 32 / NWK) tiles summed per round
LDS = {4: {1: 5120, 2: 10240, 3: 15360, 4: 20480, 6: 20480, 8: 20480}, 8: {1: 9216, 2: 18432, 3: 27648, 4: 36864, 6: 36864, 8: 36864},
       16: {1: 17408, 2: 34816, 3: 34816, 4: 34816, 6: 34816, 8: 34816}}


def _expected(M, N, K):
    nwk, lp, guard = CLASS_OF_K[K]
    rg = {1: 1, 16: 1, 17: 2, 32: 2, 33: 3, 48: 3, 49: 4, 64: 4}[M]
    ct = 2 if (rg >= 2 and N >= 4096) else 1
    return [rg, nwk, ct, 2 * lp * ct, guard, 0, 64 * nwk, -(-N // (16 * ct)), LDS[nwk][rg * ct], DEPTH[(nwk, lp)][(rg, ct)]]


@pytest.mark.parametrize("dtype", RC.DTYPES, ids=RC.DT_NAME.get)
def test_plan_integers_of_every_row_group_and_class(dtype):
    for K in CLASS_OF_K:
        for M in (1, 16, 17, 32, 33, 48, 49, 64):
            for N in (40, 136, 4096, 4104):
                rc, out = RC.plan(dtype, M, N, K)
                assert rc == _lib.OK and out == _expected(M, N, K), (M, N, K, out, _expected(M, N, K))
    # grid and LDS spelled out: one tile per workgroup at N = 40 and 136, two from 17 rows on at N >= 4096
    assert RC.plan(dtype, 64, 40, 2560)[1] == [4, 8, 1, 10, 0, 0, 512, 3, 36864, 5]
    assert RC.plan(dtype, 64, 136, 2560)[1] == [4, 8, 1, 10, 0, 0, 512, 9, 36864, 5]
    assert RC.plan(dtype, 12, 40, 1024)[1] == [1, 4, 1, 8, 0, 0, 256, 3, 5120, 4]
    assert RC.plan(dtype, 12, 136, 10240)[1] == [1, 16, 1, 20, 0, 0, 1024, 9, 17408, 5]
    assert RC.plan(dtype, 33, 136, 512)[1] == [3, 4, 1, 8, 1, 0, 256, 9, 15360, 4]
    assert RC.plan(dtype, 16, 4104, 4096)[1] == [1, 16, 1, 8, 0, 0, 1024, 257, 17408, 4]
    assert RC.plan(dtype, 17, 4104, 4096)[1] == [2, 16, 2, 16, 0, 0, 1024, 129, 34816, 2]
    assert RC.plan(dtype, 64, 4104, 5632)[1] == [4, 16, 2, 40, 1, 0, 1024, 129, 34816, 1]
    # the 4B step at 12 rows: 160 workgroups for the attention-output projection where the tile kernel has 20
    assert RC.plan(dtype, 12, 2560, 2560)[1][7] == 160 and RC.plan(dtype, 12, 7680, 2560)[1][7] == 480


def _desc(M=16, N=40, K=512, dtype=_lib.F16, **kw):
    d = _lib.GemmDesc()
    d.dtype, d.M, d.N, d.K, d.lda, d.ldb, d.ldc, d.splitk = dtype, M, N, K, K, K, N, 1
    d.A, d.B, d.C = 0x1000, 0x2000, 0x3000
    for k, v in kw.items():
        setattr(d, k, v)
    return d


# (descriptor fields, code): 1 where cogv_gemm reports a bad argument, 3 for what only this kernel does not take
REFUSALS = [
    (dict(M=0), ARG), (dict(M=65), UNS), (dict(N=44), ARG), (dict(K=520, lda=520, ldb=520), UNS), (dict(K=256, lda=256, ldb=256), UNS),
    (dict(K=10752, lda=10752, ldb=10752), UNS), (dict(trans_a=1), UNS), (dict(trans_b=1), UNS),
    (dict(flags=_lib.EPI_ACCUM), UNS), (dict(flags=_lib.EPI_BIAS | _lib.EPI_DROPOUT, bias=0x4000), UNS), (dict(dtype=_lib.F32), UNS),
    (dict(out_f32=1), UNS), (dict(splitk=2), UNS), (dict(lda=504), ARG), (dict(flags=_lib.EPI_BIAS), ARG), (dict(A=0x1008), ARG),
]


def test_every_refusal_with_its_code_and_out_untouched():
    for kw, code in REFUSALS:
        rc, out = _lib.gemm_rows_plan(None, 0, 0, 0, desc=_desc(**kw))
        assert rc == code and out == [-1] * _lib.GEMM_ROWS_PLAN_INTS, (kw, rc, out)
    lib = _lib.lib()
    out = (C.c_int * _lib.GEMM_ROWS_PLAN_INTS)()
    assert lib.cogv_gemm_rows_plan(None, out) == ARG and lib.cogv_gemm_rows_plan(C.byref(_desc()), None) == ARG
    assert lib.cogv_gemm_rows(None, None) == ARG
    # a refused descriptor is refused by the launch before anything is touched (no device here)
    for kw, code in REFUSALS:
        assert lib.cogv_gemm_rows(C.byref(_desc(**kw)), None) == code, kw


def _model(dtype=torch.float16, hidden=512, heads=8, layers=1):
    from cogview_amd.model import GPT2Model
    torch.manual_seed(0)
    return GPT2Model(layers, 64, hidden, heads, 0.0, 0.0, 0.0, 32, 32, False).to(dtype).eval()


def test_decode_wide_supported(monkeypatch):
    monkeypatch.setattr(F_, "_DECODE_WIDE", True)
    # the bound as shipped: the largest row count the measurements of DESIGN 4.5.5 leave on by default
    cap = F_._DECODE_WIDE_MAX_ROWS
    assert F_.DECODE_WIDE_KERNEL_ROWS == 64 and 9 <= cap <= 64
    tr = _model().transformer
    assert [F_.decode_wide_supported(tr, r) for r in (8, 9, cap, cap + 1)] == [False, True, True, False]
    # with the bound at the kernel's own 64 rows
    monkeypatch.setattr(F_, "_DECODE_WIDE_MAX_ROWS", 64)
    for dtype in RC.DTYPES:
        tr = _model(dtype).transformer
        assert [F_.decode_wide_supported(tr, r) for r in (1, 8, 9, 12, 64, 65)] == [False, False, True, True, True, False]
    assert not F_.decode_wide_supported(_model(torch.float32).transformer, 12)
    assert not F_.decode_wide_supported(_model(hidden=320, heads=5).transformer, 12)          # h % 512 != 0: the plan refuses
    tr = _model().transformer
    monkeypatch.setattr(F_, "_DECODE_WIDE", False)
    assert not F_.decode_wide_supported(tr, 9) and not F_.decode_wide_supported(tr, 64)
    monkeypatch.setattr(F_, "_DECODE_WIDE", True)
    monkeypatch.setattr(F_, "mp_world_size_or_1", lambda: 2)
    assert not F_.decode_wide_supported(tr, 9) and not F_.decode_wide_supported(tr, 64)


def test_the_switch_is_read_once_from_the_environment():
    import os
    import subprocess
    import sys
    code = "from cogview_amd import functional as F; print(F._DECODE_WIDE)"
    for value, want in ((None, "True"), ("0", "False")):
        env = {k: v for k, v in os.environ.items() if k != "COGV_DECODE_WIDE"}
        if value is not None:
            env["COGV_DECODE_WIDE"] = value
        assert subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, check=True).stdout.strip() == want


class _Ops:
    """recording stand-ins for the ops a layer-by-layer decode step calls (tests/test_w8_cpu.py's pattern)"""

    def __init__(self):
        self.calls = []

    @staticmethod
    def scalar_slab(slab):
        return contextlib.nullcontext()

    def gemm_rows(self, a, w, bias=None, gelu=False, absmax=None, out=None):
        self.calls.append(("gemm_rows", tuple(w.shape), a.shape[0], gelu))
        return torch.zeros(a.shape[0], w.shape[0], dtype=a.dtype)

    def gemm(self, a, b, **kw):
        self.calls.append(("gemm", tuple(b.shape), a.shape[0], bool(kw.get("gelu"))))
        return torch.zeros(a.shape[0], b.shape[0], dtype=a.dtype)

    def attention_decode(self, qkv, cache, pos_index, heads, combine=True):
        self.calls.append(("attention_decode", combine))
        return torch.zeros(qkv.shape[0], 1, heads * 64, dtype=qkv.dtype)

    def sandwich_ln_fwd(self, x, gamma, beta, eps, absmax_in, residual=None, absmax_out=None, save_stats=True):
        self.calls.append(("ln",))
        return torch.zeros(x.shape, dtype=gamma.dtype), None, None

    @staticmethod
    def new_absmax_slot(dev):
        return torch.zeros(1)


def _stubbed_step(monkeypatch, rows, layers=2):
    V_, H_ = 64, 512
    m = _model(layers=layers)
    o = _Ops()
    monkeypatch.setattr(F_, "ops", o)
    monkeypatch.setattr(decoder, "ops", o)
    monkeypatch.setattr(F_, "_DECODE_WIDE", True)
    dec = GraphDecoder(m, batch=rows, capacity=64)
    tr = m.transformer
    h0 = torch.zeros(rows, 1, H_, dtype=torch.float16)
    h0._cogv_absmax = torch.ones(1)
    monkeypatch.setattr(type(tr), "embed", lambda self, tok, pos, emb: h0)
    # today's path above the chain's rows (the modules' own forward): stand-ins that say they ran
    monkeypatch.setattr(type(tr.layers[0]), "forward", lambda self, h, *a, **k: (o.calls.append(("layer",)), h)[1])
    monkeypatch.setattr(type(tr.final_layernorm), "forward", lambda self, h: h)
    monkeypatch.setattr(F_, "tied_logits", lambda out, w: (o.calls.append(("tied_logits",)), torch.zeros(rows, 1, V_))[1])
    logits = dec._step()
    assert logits.shape == (rows, 1, V_)
    return o.calls, (V_, H_)


def test_twelve_row_step_routes_every_product_to_gemm_rows(monkeypatch):
    L_ = 2
    calls, (V_, H_) = _stubbed_step(monkeypatch, 12, L_)
    rows = [c for c in calls if c[0] == "gemm_rows"]
    assert len(rows) == 4 * L_ + 1 and not [c for c in calls if c[0] in ("gemm", "layer", "tied_logits")]
    assert [c[1] for c in rows] == [(3 * H_, H_), (H_, H_), (4 * H_, H_), (H_, 4 * H_)] * L_ + [(V_, H_)]
    assert [c[3] for c in rows] == [False, False, True, False] * L_ + [False] and {c[2] for c in rows} == {12}
    assert [c[0] for c in calls] == ["ln", "gemm_rows", "attention_decode", "gemm_rows", "ln", "ln", "gemm_rows", "gemm_rows", "ln"] * L_ + ["ln", "gemm_rows"]


def test_eight_row_step_and_switched_off_step_never_call_gemm_rows(monkeypatch):
    calls, _ = _stubbed_step(monkeypatch, 8)
    assert [c[0] for c in calls] == ["layer", "layer", "tied_logits"]
    monkeypatch.setattr(F_, "decode_wide_supported", lambda tr, rows: False)          # what COGV_DECODE_WIDE=0 answers
    calls, _ = _stubbed_step(monkeypatch, 12)
    assert [c[0] for c in calls] == ["layer", "layer", "tied_logits"]


def test_the_gpu_sweep_grid_reaches_every_plan():
    """Every distinct entry of the plan table -- (class, row groups, tiles per workgroup) with everything that follows from them --
    over ALL shapes the kernel takes has a cell in the grid of tests/test_gemm_rows_gpu.py, in both dtypes."""
    for dtype in RC.DTYPES:
        every = {}
        for K in range(512, 10240 + 1, 512):
            for M in range(1, 65):
                for N in (8, 4088, 4096, 65536):
                    rc, out = RC.plan(dtype, M, N, K)
                    assert rc == _lib.OK, (M, N, K)
                    every.setdefault(RC.plan_id(out), (M, N, K))
        grid = {RC.plan_id(RC.plan(dtype, M, N, K)[1]) for K in RC.KS for M in RC.MS for N in RC.NS}
        assert len(every) == 7 * 7                                   # 7 classes x (1 row group | 2, 3, 4 with one or two tiles)
        missing = {pid: where for pid, where in every.items() if pid not in grid}
        assert not missing, missing
        assert all(RC.plan(dtype, M, N, K)[0] == _lib.OK for K in RC.KS for M in RC.MS for N in RC.NS)
