"""CPU: what the skinny-M products of the decode step decide before they launch (cogv_gemv_plan: a host-only query that calls the
function every launch uses, csrc/gemv_plan.h): generation, class, grid, threads and dynamic LDS for the three kinds (plain,
attention-combine prologue, LayerNorm prologue) on 16-bit and E4M3 weights, and every refusal with its code.  A wrong grid or LDS
size shows on a GPU only as a fault or as columns nobody computed.
Every expectation below is a literal worked out by hand from the six if-ladders this plan replaced (csrc/gemv.hip before the
class list: one ladder per kind and weight format), not computed by the library: LDS = MT * (K + XPAD) * 2 with XPAD = 0 for the
V forms and 8 for the M forms (K / 2 in the two-halves kernel), refused above 56 KB = 57344 B except in that kernel; V forms have
4 waves of J columns, M forms NWK * tiles waves on 16 * tiles columns."""
import ctypes
import json
import os
import subprocess
import sys
import types

import pytest
import torch

from cogview_amd import _lib
from cogview_amd import functional as F_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG, ERR_UNSUPPORTED = 0, 1, 3
F16, BF16 = 0, 1
PLAIN, ATTN, LN = 0, 1, 2
KIND = {"plain": PLAIN, "attn": ATTN, "ln": LN}
W16, W8 = False, True
V, M = 0, 1
MT = {1: 1, 2: 2, 3: 4, 4: 4, 5: 8, 8: 8}
UNTOUCHED = [-1] * 11


def G1(grid40, grid136, lds):
    """first generation (16-bit only): 8 columns per workgroup of 256 threads; the LayerNorm kind keeps MT rows of K in LDS"""
    return (None, 0, 0, 0, 0, 0, 256, grid40, grid136, lds)


# (kind, format) -> K -> one entry per MT = 1, 2, 4, 8:
#   (form, J | NWK, KCMAX | LMAX, guarded, tiles per workgroup, two halves, threads, grid at N = 40, grid at N = 136, LDS bytes),
#   G1(...): first generation, or None: unsupported (3)
PLANS = {
    ("plain", W16): {
        512: [(V, 2, 20, 1, 1, 0, 256, 5, 17, 1024), (M, 4, 20, 1, 1, 0, 256, 3, 9, 2080), (M, 4, 20, 1, 1, 0, 256, 3, 9, 4160), (M, 4, 20, 1, 1, 0, 256, 3, 9, 8320)],
        1024: [(V, 8, 2, 0, 1, 0, 256, 2, 5, 2048), (M, 4, 8, 0, 1, 0, 256, 3, 9, 4128), (M, 4, 8, 0, 1, 0, 256, 3, 9, 8256), (M, 4, 8, 0, 1, 0, 256, 3, 9, 16512)],
        1536: [(V, 2, 20, 1, 1, 0, 256, 5, 17, 3072), (M, 4, 20, 1, 1, 0, 256, 3, 9, 6176), (M, 4, 20, 1, 1, 0, 256, 3, 9, 12352), (M, 4, 20, 1, 1, 0, 256, 3, 9, 24704)],
        2560: [(V, 4, 5, 0, 1, 0, 256, 3, 9, 5120), (M, 4, 20, 0, 1, 0, 256, 3, 9, 10272), (M, 4, 20, 0, 1, 0, 256, 3, 9, 20544), (M, 4, 20, 0, 1, 0, 256, 3, 9, 41088)],
        3072: [(V, 2, 20, 1, 1, 0, 256, 5, 17, 6144), (M, 8, 20, 1, 1, 0, 512, 3, 9, 12320), (M, 8, 20, 1, 1, 0, 512, 3, 9, 24640), (M, 8, 20, 1, 1, 0, 512, 3, 9, 49280)],
        3584: [(V, 2, 20, 1, 1, 0, 256, 5, 17, 7168), (M, 8, 20, 1, 1, 0, 512, 3, 9, 14368), (M, 8, 20, 1, 1, 0, 512, 3, 9, 28736), G1(5, 17, 0)],
        4096: [(V, 2, 8, 0, 1, 0, 256, 5, 17, 8192), (M, 8, 16, 0, 1, 0, 512, 3, 9, 16416), (M, 8, 16, 0, 1, 0, 512, 3, 9, 32832), G1(5, 17, 0)],
        5120: [(V, 2, 20, 1, 1, 0, 256, 5, 17, 10240), (M, 8, 20, 1, 1, 0, 512, 3, 9, 20512), (M, 8, 20, 1, 1, 0, 512, 3, 9, 41024), G1(5, 17, 0)],
        5632: [(V, 2, 20, 1, 1, 0, 256, 5, 17, 11264), G1(5, 17, 0), G1(5, 17, 0), G1(5, 17, 0)],
        10240: [(V, 2, 20, 0, 1, 0, 256, 5, 17, 20480), (M, 16, 20, 0, 1, 0, 1024, 3, 9, 40992), (M, 16, 20, 0, 1, 1, 1024, 3, 9, 41024), (M, 16, 20, 0, 1, 1, 1024, 3, 9, 82048)],
    },
    ("attn", W16): {
        512: [(V, 2, 20, 1, 1, 0, 256, 5, 17, 1024), (M, 4, 20, 1, 1, 0, 256, 3, 9, 2080), (M, 4, 20, 1, 1, 0, 256, 3, 9, 4160), (M, 4, 20, 1, 1, 0, 256, 3, 9, 8320)],
        1024: [(V, 8, 2, 0, 1, 0, 256, 2, 5, 2048), (M, 4, 8, 0, 1, 0, 256, 3, 9, 4128), (M, 4, 8, 0, 1, 0, 256, 3, 9, 8256), (M, 4, 8, 0, 1, 0, 256, 3, 9, 16512)],
        1536: [(V, 2, 20, 1, 1, 0, 256, 5, 17, 3072), (M, 4, 20, 1, 1, 0, 256, 3, 9, 6176), (M, 4, 20, 1, 1, 0, 256, 3, 9, 12352), (M, 4, 20, 1, 1, 0, 256, 3, 9, 24704)],
        2560: [(V, 4, 5, 0, 1, 0, 256, 3, 9, 5120), (M, 4, 20, 0, 1, 0, 256, 3, 9, 10272), (M, 4, 20, 0, 1, 0, 256, 3, 9, 20544), (M, 4, 20, 0, 1, 0, 256, 3, 9, 41088)],
        3072: [(V, 2, 20, 1, 1, 0, 256, 5, 17, 6144), (M, 8, 20, 1, 1, 0, 512, 3, 9, 12320), (M, 8, 20, 1, 1, 0, 512, 3, 9, 24640), (M, 8, 20, 1, 1, 0, 512, 3, 9, 49280)],
        3584: [(V, 2, 20, 1, 1, 0, 256, 5, 17, 7168), (M, 8, 20, 1, 1, 0, 512, 3, 9, 14368), (M, 8, 20, 1, 1, 0, 512, 3, 9, 28736), G1(5, 17, 0)],
        4096: [(V, 2, 20, 1, 1, 0, 256, 5, 17, 8192), G1(5, 17, 0), G1(5, 17, 0), G1(5, 17, 0)],
        5120: [(V, 2, 20, 1, 1, 0, 256, 5, 17, 10240), (M, 8, 20, 1, 1, 0, 512, 3, 9, 20512), (M, 8, 20, 1, 1, 0, 512, 3, 9, 41024), G1(5, 17, 0)],
        5632: [(V, 2, 20, 1, 1, 0, 256, 5, 17, 11264), G1(5, 17, 0), G1(5, 17, 0), G1(5, 17, 0)],
        10240: [(V, 2, 20, 1, 1, 0, 256, 5, 17, 20480), G1(5, 17, 0), G1(5, 17, 0), G1(5, 17, 0)],
    },
    ("ln", W16): {
        512: [(V, 2, 8, 1, 1, 0, 256, 5, 17, 1024), (M, 4, 20, 1, 1, 0, 256, 3, 9, 2080), (M, 4, 20, 1, 2, 0, 512, 2, 5, 4160), (M, 4, 20, 1, 2, 0, 512, 2, 5, 8320)],
        1024: [(V, 8, 2, 0, 1, 0, 256, 2, 5, 2048), (M, 4, 8, 0, 1, 0, 256, 3, 9, 4128), (M, 4, 8, 0, 2, 0, 512, 2, 5, 8256), (M, 4, 8, 0, 2, 0, 512, 2, 5, 16512)],
        1536: [(V, 2, 8, 1, 1, 0, 256, 5, 17, 3072), (M, 4, 20, 1, 1, 0, 256, 3, 9, 6176), (M, 4, 20, 1, 2, 0, 512, 2, 5, 12352), (M, 4, 20, 1, 2, 0, 512, 2, 5, 24704)],
        2560: [(V, 4, 5, 0, 1, 0, 256, 3, 9, 5120), (M, 4, 20, 0, 1, 0, 256, 3, 9, 10272), (M, 4, 20, 0, 2, 0, 512, 2, 5, 20544), (M, 4, 20, 0, 2, 0, 512, 2, 5, 41088)],
        3072: [(V, 2, 8, 1, 1, 0, 256, 5, 17, 6144), (M, 8, 20, 1, 1, 0, 512, 3, 9, 12320), (M, 8, 20, 1, 1, 0, 512, 3, 9, 24640), (M, 8, 20, 1, 1, 0, 512, 3, 9, 49280)],
        3584: [(V, 2, 8, 1, 1, 0, 256, 5, 17, 7168), (M, 8, 20, 1, 1, 0, 512, 3, 9, 14368), (M, 8, 20, 1, 1, 0, 512, 3, 9, 28736), G1(5, 17, 57344)],
        4096: [(V, 2, 8, 1, 1, 0, 256, 5, 17, 8192), (M, 8, 20, 1, 1, 0, 512, 3, 9, 16416), (M, 8, 20, 1, 1, 0, 512, 3, 9, 32832), G1(5, 17, 65536)],
    },
    ("plain", W8): {
        512: [(V, 4, 20, 1, 1, 0, 256, 3, 9, 1024), (M, 2, 20, 1, 1, 0, 128, 3, 9, 2080), (M, 2, 20, 1, 1, 0, 128, 3, 9, 4160), (M, 2, 20, 1, 1, 0, 128, 3, 9, 8320)],
        1024: [(V, 16, 2, 0, 1, 0, 256, 1, 3, 2048), (M, 2, 8, 0, 1, 0, 128, 3, 9, 4128), (M, 2, 8, 0, 1, 0, 128, 3, 9, 8256), (M, 2, 8, 0, 1, 0, 128, 3, 9, 16512)],
        1536: [(V, 4, 20, 1, 1, 0, 256, 3, 9, 3072), (M, 2, 20, 1, 1, 0, 128, 3, 9, 6176), (M, 2, 20, 1, 1, 0, 128, 3, 9, 12352), (M, 2, 20, 1, 1, 0, 128, 3, 9, 24704)],
        2560: [(V, 8, 5, 0, 1, 0, 256, 2, 5, 5120), (M, 2, 20, 0, 1, 0, 128, 3, 9, 10272), (M, 2, 20, 0, 1, 0, 128, 3, 9, 20544), (M, 2, 20, 0, 1, 0, 128, 3, 9, 41088)],
        3072: [(V, 4, 20, 1, 1, 0, 256, 3, 9, 6144), (M, 4, 20, 1, 1, 0, 256, 3, 9, 12320), (M, 4, 20, 1, 1, 0, 256, 3, 9, 24640), (M, 4, 20, 1, 1, 0, 256, 3, 9, 49280)],
        3584: [(V, 4, 20, 1, 1, 0, 256, 3, 9, 7168), (M, 4, 20, 1, 1, 0, 256, 3, 9, 14368), (M, 4, 20, 1, 1, 0, 256, 3, 9, 28736), None],
        4096: [(V, 4, 8, 0, 1, 0, 256, 3, 9, 8192), (M, 4, 16, 0, 1, 0, 256, 3, 9, 16416), (M, 4, 16, 0, 1, 0, 256, 3, 9, 32832), (M, 4, 16, 0, 1, 1, 256, 3, 9, 32896)],
        5120: [(V, 4, 20, 1, 1, 0, 256, 3, 9, 10240), (M, 4, 20, 1, 1, 0, 256, 3, 9, 20512), (M, 4, 20, 1, 1, 0, 256, 3, 9, 41024), None],
        5632: [(V, 4, 20, 1, 1, 0, 256, 3, 9, 11264), None, None, None],
        10240: [(V, 4, 20, 0, 1, 0, 256, 3, 9, 20480), (M, 8, 20, 0, 1, 0, 512, 3, 9, 40992), (M, 8, 20, 0, 1, 1, 512, 3, 9, 41024), (M, 8, 20, 0, 1, 1, 512, 3, 9, 82048)],
    },
    ("attn", W8): {
        512: [(V, 4, 20, 1, 1, 0, 256, 3, 9, 1024), (M, 2, 20, 1, 1, 0, 128, 3, 9, 2080), (M, 2, 20, 1, 1, 0, 128, 3, 9, 4160), (M, 2, 20, 1, 1, 0, 128, 3, 9, 8320)],
        1024: [(V, 16, 2, 0, 1, 0, 256, 1, 3, 2048), (M, 2, 8, 0, 1, 0, 128, 3, 9, 4128), (M, 2, 8, 0, 1, 0, 128, 3, 9, 8256), (M, 2, 8, 0, 1, 0, 128, 3, 9, 16512)],
        1536: [(V, 4, 20, 1, 1, 0, 256, 3, 9, 3072), (M, 2, 20, 1, 1, 0, 128, 3, 9, 6176), (M, 2, 20, 1, 1, 0, 128, 3, 9, 12352), (M, 2, 20, 1, 1, 0, 128, 3, 9, 24704)],
        2560: [(V, 8, 5, 0, 1, 0, 256, 2, 5, 5120), (M, 2, 20, 0, 1, 0, 128, 3, 9, 10272), (M, 2, 20, 0, 1, 0, 128, 3, 9, 20544), (M, 2, 20, 0, 1, 0, 128, 3, 9, 41088)],
        3072: [(V, 4, 20, 1, 1, 0, 256, 3, 9, 6144), (M, 4, 20, 1, 1, 0, 256, 3, 9, 12320), (M, 4, 20, 1, 1, 0, 256, 3, 9, 24640), (M, 4, 20, 1, 1, 0, 256, 3, 9, 49280)],
        3584: [(V, 4, 20, 1, 1, 0, 256, 3, 9, 7168), (M, 4, 20, 1, 1, 0, 256, 3, 9, 14368), (M, 4, 20, 1, 1, 0, 256, 3, 9, 28736), None],
        4096: [(V, 4, 20, 1, 1, 0, 256, 3, 9, 8192), (M, 4, 20, 1, 1, 0, 256, 3, 9, 16416), (M, 4, 20, 1, 1, 0, 256, 3, 9, 32832), None],
        5120: [(V, 4, 20, 1, 1, 0, 256, 3, 9, 10240), (M, 4, 20, 1, 1, 0, 256, 3, 9, 20512), (M, 4, 20, 1, 1, 0, 256, 3, 9, 41024), None],
        5632: [(V, 4, 20, 1, 1, 0, 256, 3, 9, 11264), None, None, None],
        10240: [(V, 4, 20, 1, 1, 0, 256, 3, 9, 20480), None, None, None],
    },
    ("ln", W8): {
        512: [(V, 4, 8, 1, 1, 0, 256, 3, 9, 1024), (M, 2, 20, 1, 2, 0, 256, 2, 5, 2080), (M, 2, 20, 1, 4, 0, 512, 1, 3, 4160), (M, 2, 20, 1, 4, 0, 512, 1, 3, 8320)],
        1024: [(V, 16, 2, 0, 1, 0, 256, 1, 3, 2048), (M, 2, 8, 0, 2, 0, 256, 2, 5, 4128), (M, 2, 8, 0, 4, 0, 512, 1, 3, 8256), (M, 2, 8, 0, 4, 0, 512, 1, 3, 16512)],
        1536: [(V, 4, 8, 1, 1, 0, 256, 3, 9, 3072), (M, 2, 20, 1, 2, 0, 256, 2, 5, 6176), (M, 2, 20, 1, 4, 0, 512, 1, 3, 12352), (M, 2, 20, 1, 4, 0, 512, 1, 3, 24704)],
        2560: [(V, 8, 5, 0, 1, 0, 256, 2, 5, 5120), (M, 2, 20, 0, 2, 0, 256, 2, 5, 10272), (M, 2, 20, 0, 4, 0, 512, 1, 3, 20544), (M, 2, 20, 0, 4, 0, 512, 1, 3, 41088)],
        3072: [(V, 4, 8, 1, 1, 0, 256, 3, 9, 6144), (M, 4, 20, 1, 2, 0, 512, 2, 5, 12320), (M, 4, 20, 1, 2, 0, 512, 2, 5, 24640), (M, 4, 20, 1, 2, 0, 512, 2, 5, 49280)],
        3584: [(V, 4, 8, 1, 1, 0, 256, 3, 9, 7168), (M, 4, 20, 1, 2, 0, 512, 2, 5, 14368), (M, 4, 20, 1, 2, 0, 512, 2, 5, 28736), None],
        4096: [(V, 4, 8, 1, 1, 0, 256, 3, 9, 8192), (M, 4, 20, 1, 2, 0, 512, 2, 5, 16416), (M, 4, 20, 1, 2, 0, 512, 2, 5, 32832), None],
    },
}


def query(kind, w8, M, N, K, dtype=F16, nsplit=9, desc=None, weight=None):
    """(code, out) of cogv_gemv_plan for a contiguous product; desc / weight: fields to overwrite"""
    d = _lib.GemmDesc()
    d.dtype, d.M, d.N, d.K, d.lda, d.ldb, d.ldc, d.splitk = dtype, M, N, K, K, K, N, 1
    d.A, d.B, d.C = 0x1000, 0x2000, 0x3000
    for k, v in (desc or {}).items():
        assert hasattr(d, k), k
        setattr(d, k, v)
    w = None
    if w8:
        w = _lib.W8Weight()
        w.q, w.ldq, w.scale = 0x4000, K, 0x5000
        for k, v in (weight or {}).items():
            setattr(w, k, v)
    out = (ctypes.c_int * 11)(*UNTOUCHED)
    rc = _lib.lib().cogv_gemv_plan(KIND[kind], ctypes.byref(d), ctypes.byref(w) if w8 else None, nsplit, out)
    return rc, list(out)


def expected(entry, mt, N):
    if entry is None:
        return ERR_UNSUPPORTED, UNTOUCHED
    form, p0, p1, guard, tw, k2, threads, g40, g136, lds = entry
    grid = {40: g40, 136: g136}[N]
    if form is None:
        return OK, [1, 0, 0, 0, 0, mt, 0, 0, threads, grid, lds]
    return OK, [2, form, p0, p1, guard, mt, tw, k2, threads, grid, lds]


@pytest.mark.parametrize("kind,w8", list(PLANS))
def test_plan_grid(kind, w8):
    """kind x format x dtype x M in {1, 2, 3, 4, 5, 8} x K x N in {40, 136}; the LayerNorm kind above K = 4096: test_refusals"""
    n = 0
    for K, row in PLANS[(kind, w8)].items():
        for M_, mt in MT.items():
            for N in (40, 136):
                for dtype in (F16, BF16):
                    assert query(kind, w8, M_, N, K, dtype) == expected(row[(1, 2, 4, 8).index(mt)], mt, N), (kind, w8, dtype, M_, N, K)
                    n += 1
    assert n == (7 if kind == "ln" else 10) * 6 * 2 * 2


@pytest.mark.parametrize("kind,w8", list(PLANS))
def test_the_gpu_sweep_grid_reaches_every_plan(kind, w8):
    """tests/gemv_cells.py (the grid tests/test_gemv_cells_gpu.py launches): every distinct entry of PLANS -- the first generation's
    included -- is the plan of some (M, K) of that grid, in both dtypes.  An entry is (generation, form, J | NWK, KCMAX | LMAX,
    guarded, tiles, two halves, MT); the grid columns do not identify it.  No exemptions: a new entry wants a new grid point."""
    from tests import gemv_cells as GC

    def ident(entry, mt):
        form, p0, p1, guard, tw, k2 = entry[:6]
        return (1, 0, 0, 0, 0, 0, 0, mt) if form is None else (2, form, p0, p1, guard, tw, k2, mt)

    want = {ident(e, mt) for row in PLANS[(kind, w8)].values() for e, mt in zip(row, (1, 2, 4, 8)) if e is not None}
    assert len(want) >= 8
    for dtype in (F16, BF16):
        reached = set()
        for K in GC.ks(kind):
            for M_ in GC.MS:
                rc, out = query(kind, w8, M_, 136, K, dtype)
                if rc == OK:
                    assert out[5] == MT[M_]
                    reached.add(GC.plan_id(out))
        assert not want - reached, (kind, w8, dtype, sorted(want - reached))
    # ... and the two K of the first generation's LayerNorm kernel that take their LDS by attribute are both grid points
    assert {3584, 4096} <= set(GC.ks("ln")) and 8 in GC.MS


@pytest.mark.parametrize("kind,w8,M_,K,want", [
    ("plain", W16, 1, 2560, (OK, [2, V, 4, 5, 0, 1, 1, 0, 256, 9, 5120])),
    ("plain", W8, 1, 1024, (OK, [2, V, 16, 2, 0, 1, 1, 0, 256, 3, 2048])),
    ("plain", W16, 4, 10240, (OK, [2, M, 16, 20, 0, 4, 1, 1, 1024, 9, 4 * 5128 * 2])),
    ("plain", W16, 8, 10240, (OK, [2, M, 16, 20, 0, 8, 1, 1, 1024, 9, 82048])),
    ("ln", W8, 2, 1024, (OK, [2, M, 2, 8, 0, 2, 2, 0, 256, 5, 2 * 1032 * 2])),
    ("plain", W16, 8, 4096, (OK, [1, 0, 0, 0, 0, 8, 0, 0, 256, 17, 0])),               # 8 x 4104 x 2 = 65664 B > 57344
    ("attn", W16, 2, 4096, (OK, [1, 0, 0, 0, 0, 2, 0, 0, 256, 17, 0])),                # the exact class is not instantiated for this kind
    ("plain", W16, 3, 5632, (OK, [1, 0, 0, 0, 0, 4, 0, 0, 256, 17, 0])),               # 11 chunks: above the guarded M classes
    ("attn", W8, 8, 4096, (ERR_UNSUPPORTED, UNTOUCHED)),
    ("ln", W8, 8, 4096, (ERR_UNSUPPORTED, UNTOUCHED)),
    ("plain", W8, 2, 5632, (ERR_UNSUPPORTED, UNTOUCHED)),
])
def test_seeds(kind, w8, M_, K, want):
    assert query(kind, w8, M_, 136, K) == want


def test_plain_and_attention_kind_share_the_association():
    """The combine-prologue form and the two-launch form of the attention-output projection agree bit for bit because, for every
    (format, M, K) both kinds take in generation 2, the form is the same and so is NWK (M form: the split of the contraction over
    waves); V forms may differ in J only (a column's arithmetic does not depend on how many columns its wave owns)."""
    both = 0
    for w8 in (W16, W8):
        for K, row in PLANS[("plain", w8)].items():
            for p, a in zip(row, PLANS[("attn", w8)][K]):
                if p is None or a is None or p[0] is None or a[0] is None:
                    continue
                both += 1
                assert p[0] == a[0], (w8, K)
                if p[0] == M:
                    assert p[1] == a[1], (w8, K)
    assert both == 29 + 31
    # and the library says the same, asked directly
    for w8 in (W16, W8):
        for K in PLANS[("plain", w8)]:
            for M_ in (1, 2, 3, 4, 5, 8):
                (rp, p), (ra, a) = query("plain", w8, M_, 136, K), query("attn", w8, M_, 136, K)
                if rp == OK and ra == OK and p[0] == 2 and a[0] == 2:
                    assert p[1] == a[1] and (p[1] == V or p[2] == a[2]), (w8, M_, K)


REFUSALS = [
    # (kind, format, M, N, K, keywords) -> code.  16-bit descriptors pass cogv_gemm's argument checks first (N % 8, K % 8: bad
    # argument); the 8-bit entry points look at the shape before the arguments.
    (("plain", W16, 2, 136, 1032, {}), ERR_UNSUPPORTED), (("attn", W16, 2, 136, 1032, {}), ERR_UNSUPPORTED),      # K % 512
    (("ln", W16, 2, 136, 1032, {}), ERR_UNSUPPORTED), (("plain", W16, 2, 136, 1028, {}), ERR_ARG),
    (("plain", W8, 2, 136, 1032, {}), ERR_UNSUPPORTED), (("attn", W8, 1, 136, 1032, {}), ERR_UNSUPPORTED), (("ln", W8, 4, 136, 520, {}), ERR_UNSUPPORTED),
    (("plain", W16, 2, 132, 1024, {}), ERR_ARG), (("attn", W16, 2, 132, 1024, {}), ERR_ARG), (("ln", W16, 2, 132, 1024, {}), ERR_ARG),      # N % 8
    (("plain", W8, 2, 132, 1024, {}), ERR_UNSUPPORTED), (("attn", W8, 2, 132, 1024, {}), ERR_UNSUPPORTED), (("ln", W8, 2, 132, 1024, {}), ERR_UNSUPPORTED),
    (("plain", W16, 0, 136, 1024, {}), ERR_ARG), (("attn", W16, 0, 136, 1024, {}), ERR_ARG), (("ln", W16, 0, 136, 1024, {}), ERR_ARG),      # M = 0
    (("plain", W8, 0, 136, 1024, {}), ERR_ARG), (("attn", W8, 0, 136, 1024, {}), ERR_ARG), (("ln", W8, 0, 136, 1024, {}), ERR_ARG),
    (("plain", W16, 9, 136, 1024, {}), ERR_UNSUPPORTED), (("attn", W16, 9, 136, 1024, {}), ERR_UNSUPPORTED),      # M = 9 (cogv_gemm: a GEMM, not these kernels)
    (("ln", W16, 9, 136, 1024, {}), ERR_UNSUPPORTED),
    (("plain", W8, 9, 136, 1024, {}), ERR_UNSUPPORTED), (("attn", W8, 9, 136, 1024, {}), ERR_UNSUPPORTED), (("ln", W8, 9, 136, 1024, {}), ERR_UNSUPPORTED),
    (("ln", W16, 1, 136, 4608, {}), ERR_UNSUPPORTED), (("ln", W16, 8, 136, 5120, {}), ERR_UNSUPPORTED), (("ln", W8, 1, 136, 4608, {}), ERR_UNSUPPORTED),      # ln: K > 4096
    (("ln", W8, 2, 136, 10240, {}), ERR_UNSUPPORTED),
    (("attn", W8, 1, 136, 1024, dict(nsplit=33)), ERR_UNSUPPORTED), (("attn", W8, 4, 136, 2560, dict(nsplit=33)), ERR_UNSUPPORTED),
    (("attn", W16, 1, 136, 1024, dict(nsplit=0)), ERR_ARG), (("attn", W8, 1, 136, 1024, dict(nsplit=0)), ERR_ARG),
    (("plain", W8, 1, 136, 1024, dict(weight=dict(ldq=1032))), ERR_ARG), (("ln", W8, 2, 136, 1024, dict(weight=dict(ldq=1032))), ERR_ARG),      # ldq % 16
    (("attn", W8, 8, 136, 1024, dict(weight=dict(ldq=1032))), ERR_ARG),
    (("plain", W8, 1, 136, 1024, dict(weight=dict(ldq=512))), ERR_UNSUPPORTED), (("ln", W8, 2, 136, 1024, dict(weight=dict(ldq=1008))), ERR_UNSUPPORTED),   # ldq < K
    (("attn", W8, 8, 136, 1024, dict(weight=dict(ldq=0))), ERR_UNSUPPORTED),
    (("plain", W8, 1, 136, 1024, dict(weight=dict(scale=0))), ERR_ARG), (("ln", W8, 2, 136, 1024, dict(weight=dict(scale=0))), ERR_ARG),      # scale
    (("attn", W8, 8, 136, 1024, dict(weight=dict(scale=0))), ERR_ARG),
    (("plain", W8, 1, 136, 1024, dict(weight=dict(scale=0x5004))), ERR_ARG), (("ln", W8, 2, 136, 1024, dict(weight=dict(scale=0x5008))), ERR_ARG),
    (("attn", W8, 8, 136, 1024, dict(weight=dict(scale=0x5001))), ERR_ARG),
    (("plain", W8, 1, 136, 1024, dict(weight=dict(q=0))), ERR_ARG), (("plain", W8, 1, 136, 1024, dict(weight=dict(q=0x4008))), ERR_ARG),
    # what the entry points refuse of a descriptor: layouts, epilogues, dtypes
    (("plain", W16, 2, 136, 1024, dict(desc=dict(trans_b=1))), ERR_UNSUPPORTED), (("ln", W16, 2, 136, 1024, dict(desc=dict(trans_b=1))), ERR_UNSUPPORTED),
    (("plain", W16, 2, 136, 1024, dict(desc=dict(flags=64, colsum_partial=0x6000))), ERR_UNSUPPORTED),      # column sums
    (("attn", W16, 2, 136, 1024, dict(desc=dict(flags=2))), ERR_UNSUPPORTED), (("attn", W8, 2, 136, 1024, dict(desc=dict(flags=2))), ERR_UNSUPPORTED),      # GeLU
    (("ln", W16, 2, 136, 1024, dict(desc=dict(out_f32=1))), ERR_UNSUPPORTED), (("plain", W8, 2, 136, 1024, dict(desc=dict(out_f32=1))), ERR_UNSUPPORTED),
    (("plain", W16, 2, 136, 1024, dict(dtype=2)), ERR_UNSUPPORTED), (("plain", W8, 2, 136, 1024, dict(dtype=2)), ERR_UNSUPPORTED),
    (("plain", W16, 2, 136, 1024, dict(desc=dict(C=0x3008))), ERR_ARG), (("ln", W8, 2, 136, 1024, dict(desc=dict(ldc=132))), ERR_ARG),
]


@pytest.mark.parametrize("case,rc", REFUSALS)
def test_refusals(case, rc):
    """... with the launch's code, and `out` left untouched"""
    kind, w8, M_, N, K, kw = case
    assert query(kind, w8, M_, N, K, **kw) == (rc, UNTOUCHED)


def test_refusals_of_the_call_itself():
    lib, out = _lib.lib(), (ctypes.c_int * 11)()
    d = _lib.GemmDesc()
    assert lib.cogv_gemv_plan(PLAIN, None, None, 1, out) == ERR_ARG
    assert lib.cogv_gemv_plan(PLAIN, ctypes.byref(d), None, 1, None) == ERR_ARG
    assert lib.cogv_gemv_plan(3, ctypes.byref(d), None, 1, out) == ERR_ARG and lib.cogv_gemv_plan(-1, ctypes.byref(d), None, 1, out) == ERR_ARG


def test_more_key_splits_than_the_combine_prologue_holds():
    """nsplit > 32 (not reachable through cogv_gemv_attn: capacity <= 4096 = 32 x 128): the second-generation kernel keeps 32
    partial maxima; the 16-bit product goes to the first generation, the 8-bit one has none (test_refusals)."""
    assert query("attn", W16, 1, 136, 1024, nsplit=32) == (OK, [2, V, 8, 2, 0, 1, 1, 0, 256, 5, 2048])
    assert query("attn", W16, 1, 136, 1024, nsplit=33) == (OK, [1, 0, 0, 0, 0, 1, 0, 0, 256, 17, 0])
    assert query("attn", W8, 1, 136, 1024, nsplit=32) == (OK, [2, V, 16, 2, 0, 1, 1, 0, 256, 3, 2048])


def test_strided_weights_change_nothing():
    assert query("plain", W16, 2, 136, 1024, desc=dict(ldb=4096)) == query("plain", W16, 2, 136, 1024)
    assert query("ln", W8, 2, 136, 1024, weight=dict(ldq=4096)) == query("ln", W8, 2, 136, 1024)


def test_first_generation_only_in_a_fresh_process():
    """COGV_GEMV2=0 is read once per process: every 16-bit plan is the first generation's, the 8-bit plans are what they were."""
    code = (
        "import json, sys; sys.path.insert(0, %r)\n"
        "from tests.test_gemv_plan import query, PLANS, MT\n"
        "print(json.dumps([[kind, int(w8), M_, K, query(kind, w8, M_, 136, K)] for (kind, w8), rows in PLANS.items() for K in rows for M_ in MT]))\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, COGV_GEMV2="0"), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(got) == (3 * 10 - 3 + 3 * 10 - 3) * 6
    for kind, w8, M_, K, (rc, out) in got:
        mt = MT[M_]
        if w8:
            assert (rc, out) == tuple(expected(PLANS[(kind, W8)][K][(1, 2, 4, 8).index(mt)], mt, 136)), (kind, M_, K)
        else:
            assert rc == OK and out[0] == 1 and out[1:5] == [0, 0, 0, 0] and out[5:8] == [mt, 0, 0] and out[8:10] == [256, 17], (kind, M_, K)
    first = {(kind, M_, K): out[10] for kind, w8, M_, K, (rc, out) in got if not w8}
    assert first[("plain", 8, 10240)] == 0 and first[("attn", 1, 1024)] == 0
    assert first[("ln", 1, 1024)] == 2048 and first[("ln", 3, 2560)] == 4 * 2560 * 2 and first[("ln", 8, 4096)] == 65536


# ---------------------------------------------------------------------------------------------------------------------------
# functional.w8_decode_supported asks this plan for the products the step will issue; its predecessor kept a table of its own:
def _old_w8_decode_supported(h, f, batch):
    if batch > 8:
        return f"batch {batch} > 8 rows"
    for k in (h, f):
        if k % 512 or k > 10240 or (batch > 1 and k > 5120 and k not in (10240,)) or (batch > 4 and k > 3072 and k not in (4096, 10240)):
            return f"contraction length {k} at {batch} row(s) is outside the 8-bit kernels' classes"
    return None


def _transformer(h, f):
    """the attributes w8_decode_supported reads, on meta tensors"""
    def lin(n, k):
        return types.SimpleNamespace(weight=torch.empty(n, k, dtype=torch.float16, device="meta"))
    layer = types.SimpleNamespace(input_layernorm=types.SimpleNamespace(weight=torch.empty(h, dtype=torch.float16, device="meta")),
                                  attention=types.SimpleNamespace(num_attention_heads_per_partition=h // 64, query_key_value=lin(3 * h, h), dense=lin(h, h)),
                                  mlp=types.SimpleNamespace(dense_h_to_4h=lin(f, h), dense_4h_to_h=lin(h, f)))
    return types.SimpleNamespace(layers=[layer])


@pytest.mark.parametrize("chain_rows", [8, 4, 0])
def test_w8_decode_supported_against_its_predecessor(monkeypatch, chain_rows):
    """batch 1 .. 9 x h in {512 .. 4096 step 512} with f = 4h, under both step forms (the chain up to COGV_DECODE_CHAIN_MAX_ROWS
    = 8 / 4 rows, 0: layer by layer).  The new predicate accepts nothing the old one refused, and with f = 4h the two agree
    EVERYWHERE: the old table's hole -- it modelled the plain kind only, so h = 4096 at 5 .. 8 rows passed although the
    LayerNorm- and combine-prologue kinds need 8 x 4104 x 2 = 65664 B > 57344 -- is hidden at f = 4h by 4h = 16384 > 10240,
    which the old table already refused.  A model with f = h (second sweep) shows it: under the chain at 8 rows the
    disagreements are exactly h = 4096 at 5 .. 8 rows, each a product whose plan the library refuses."""
    monkeypatch.setattr(F_, "_DECODE_CHAIN_MAX_ROWS", chain_rows)
    for mult, want in ((4, []), (1, [(4096, b) for b in (5, 6, 7, 8)] if chain_rows == 8 else [])):
        disagree = []
        for h in range(512, 4097, 512):
            for batch in range(1, 10):
                old, new = _old_w8_decode_supported(h, mult * h, batch), F_.w8_decode_supported(_transformer(h, mult * h), batch)
                assert not (old is not None and new is None), (h, mult, batch)
                if old is None and new is not None:
                    disagree.append((h, batch))
                    assert _lib.gemv_plan(_lib.GEMV_LN, F16, batch, 3 * h, h, w8=True)[0] == ERR_UNSUPPORTED
        assert disagree == want


def test_w8_decode_supported_messages():
    assert "rows" in F_.w8_decode_supported(_transformer(512, 2048), 9)
    assert "contraction length 320" in F_.w8_decode_supported(_transformer(320, 1280), 1)
    assert F_.w8_decode_supported(_transformer(2560, 10240), 4) is None
