"""CPU: which form of the Sandwich-LN backward runs, and on which grid (cogv_ln_bwd_plan / cogv_ln_bwd_pair_plan: host-only
queries that call the function the launch itself uses).  Results do not depend on the grid and all forms are bit-identical, so
no GPU test can see a wrong choice; it only costs occupancy.  Every expectation below is a literal: the table of
cogview_amd/csrc/layernorm.hip::ln_bwd_plan written out by hand, not recomputed."""
import ctypes
import os
import subprocess
import sys

import pytest

from cogview_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_T, IN, OUT = 0, 1, 2            # COGV_LN_ALL_T, COGV_LN_STREAM_IN, COGV_LN_STREAM_OUT
OK, ERR_ARG, ERR_UNSUPPORTED = 0, 1, 3
SWITCHES = ("COGV_LN_BWD_LEAN", "COGV_LN_BWD_MARKED_ROWS")


def plan(mode, rows, h, p=0.0, marked=0, add_in=0):
    """(error code, [rows in flight, lean, marked, workgroups, threads])"""
    out = (ctypes.c_int * 5)(-1, -1, -1, -1, -1)
    rc = _lib.lib().cogv_ln_bwd_plan(mode, rows, h, p, marked, add_in, out)
    return rc, list(out)


def pair_plan(rows, h, p=0.0):
    out = (ctypes.c_int * 5)(-1, -1, -1, -1, -1)
    rc = _lib.lib().cogv_ln_bwd_pair_plan(rows, h, p, out)
    return rc, list(out)


@pytest.fixture
def defaults(monkeypatch):
    for name in SWITCHES:
        monkeypatch.delenv(name, raising=False)
    return monkeypatch


# (mode, rows, h, p, marked, add_in) -> [R, lean, mark, workgroups, threads]; the 4B step runs 32640 rows of 2560
HOT = [
    ((OUT, 32640, 2560, 0.1, 1, 0), [4, 0, 1, 256, 320]),      # LN4': mask from marked zeros, one four-row workgroup per CU
    ((OUT, 32640, 2560, 0.1, 1, 1), [4, 0, 1, 256, 320]),
    ((ALL_T, 32640, 2560, 0.1, 1, 0), [4, 0, 1, 256, 320]),
    ((OUT, 32640, 2560, 0.1, 0, 0), [2, 1, 0, 768, 320]),      # model-parallel replay: lean, three workgroups per CU
    ((OUT, 32640, 2560, 0.1, 0, 1), [2, 0, 0, 512, 320]),      # add_in rules the lean form out: two rows, two per CU
    ((ALL_T, 32640, 2560, 0.1, 0, 0), [2, 0, 0, 512, 320]),
    ((IN, 32640, 2560, 0.1, 0, 1), [2, 0, 0, 512, 320]),
    ((IN, 32640, 2560, 0.0, 0, 1), [2, 0, 0, 256, 320]),       # LN1' / LN2': two rows, yet one workgroup per CU (167 vs 178 us)
    ((IN, 32640, 2560, 0.0, 0, 0), [2, 0, 0, 256, 320]),
    ((ALL_T, 32640, 2560, 0.0, 0, 0), [4, 0, 0, 256, 320]),
    ((OUT, 32640, 2560, 0.0, 0, 0), [4, 0, 0, 256, 320]),
    ((ALL_T, 32640, 4096, 0.0, 0, 0), [4, 0, 0, 256, 512]),
    ((OUT, 32640, 1544, 0.1, 0, 0), [2, 1, 0, 768, 256]),      # the narrowest wide row: four waves
]
NARROW = [
    ((ALL_T, 1088, 1024, 0.0, 0, 0), [4, 0, 0, 272, 128]),
    ((IN, 1088, 1024, 0.0, 0, 1), [4, 0, 0, 272, 128]),
    ((IN, 1088, 1024, 0.1, 0, 1), [4, 0, 0, 272, 128]),
    ((OUT, 1088, 1024, 0.0, 0, 0), [4, 0, 0, 272, 128]),
    ((OUT, 1088, 1024, 0.1, 0, 0), [4, 0, 0, 272, 128]),
    ((OUT, 1088, 1024, 0.1, 1, 0), [4, 0, 1, 272, 128]),
    ((ALL_T, 1088, 1024, 0.1, 1, 1), [4, 0, 1, 272, 128]),
    ((OUT, 32640, 1024, 0.1, 0, 0), [4, 0, 0, 1024, 128]),     # many small workgroups, up to the workspace bound
    ((OUT, 32640, 1536, 0.1, 0, 0), [4, 0, 0, 853, 192]),      # three waves per row: 2560 / 3 workgroups
    ((ALL_T, 32640, 512, 0.0, 0, 0), [4, 0, 0, 1024, 64]),
]
SMALL = [       # few rows: the row count decides, not the cap
    ((ALL_T, 1, 2560, 0.0, 0, 0), [4, 0, 0, 1, 320]),
    ((OUT, 1, 2560, 0.1, 0, 0), [2, 1, 0, 1, 320]),
    ((OUT, 1, 2560, 0.1, 1, 0), [4, 0, 1, 1, 320]),
    ((ALL_T, 5, 2560, 0.0, 0, 0), [4, 0, 0, 2, 320]),
    ((OUT, 5, 2560, 0.1, 0, 0), [2, 1, 0, 2, 320]),            # three pairs of rows, but the workspace holds ceil(5 / 4) partials
    ((IN, 5, 1024, 0.0, 0, 1), [4, 0, 0, 2, 128]),
    ((ALL_T, 600, 2560, 0.0, 0, 0), [4, 0, 0, 150, 320]),
    ((OUT, 600, 2560, 0.1, 0, 0), [2, 1, 0, 150, 320]),
    ((OUT, 600, 2560, 0.1, 0, 1), [2, 0, 0, 150, 320]),
    ((OUT, 600, 2560, 0.1, 1, 0), [4, 0, 1, 150, 320]),
    ((OUT, 2000, 2560, 0.1, 0, 0), [2, 1, 0, 500, 320]),
    ((OUT, 2000, 2560, 0.1, 0, 1), [2, 0, 0, 500, 320]),
    ((OUT, 2000, 2560, 0.0, 0, 0), [4, 0, 0, 256, 320]),
    ((OUT, 3500, 2560, 0.1, 0, 0), [2, 1, 0, 768, 320]),
]


@pytest.mark.parametrize("args,want", HOT + NARROW + SMALL)
def test_plan_defaults(defaults, args, want):
    assert plan(*args) == (OK, want)


@pytest.mark.parametrize("env,args,want", [
    ({"COGV_LN_BWD_MARKED_ROWS": "2"}, (OUT, 32640, 2560, 0.1, 1, 0), [2, 1, 1, 768, 320]),        # the replay's geometry
    ({"COGV_LN_BWD_MARKED_ROWS": "2"}, (OUT, 32640, 2560, 0.1, 1, 1), [2, 0, 1, 512, 320]),
    ({"COGV_LN_BWD_MARKED_ROWS": "2"}, (ALL_T, 32640, 2560, 0.1, 1, 0), [2, 0, 1, 512, 320]),
    ({"COGV_LN_BWD_MARKED_ROWS": "2"}, (OUT, 1088, 1024, 0.1, 1, 0), [4, 0, 1, 272, 128]),         # narrow rows: four, always
    ({"COGV_LN_BWD_MARKED_ROWS": "2"}, (OUT, 32640, 2560, 0.1, 0, 0), [2, 1, 0, 768, 320]),        # not marked: untouched
    ({"COGV_LN_BWD_MARKED_ROWS": "2", "COGV_LN_BWD_LEAN": "0"}, (OUT, 32640, 2560, 0.1, 1, 0), [2, 0, 1, 512, 320]),
    ({"COGV_LN_BWD_MARKED_ROWS": "4"}, (OUT, 32640, 2560, 0.1, 1, 0), [4, 0, 1, 256, 320]),
    ({"COGV_LN_BWD_LEAN": "0"}, (OUT, 32640, 2560, 0.1, 0, 0), [2, 0, 0, 512, 320]),
    ({"COGV_LN_BWD_LEAN": "0"}, (OUT, 600, 2560, 0.1, 0, 0), [2, 0, 0, 150, 320]),
    ({"COGV_LN_BWD_LEAN": "0"}, (OUT, 32640, 2560, 0.1, 1, 0), [4, 0, 1, 256, 320]),
    ({"COGV_LN_BWD_LEAN": "1"}, (OUT, 32640, 2560, 0.1, 0, 0), [2, 1, 0, 768, 320]),
])
def test_plan_other_side_of_each_switch(defaults, env, args, want):
    """COGV_LN_BWD_LEAN and COGV_LN_BWD_MARKED_ROWS are read on every launch (the GPU tests flip them inside one process)."""
    for k, v in env.items():
        defaults.setenv(k, v)
    assert plan(*args) == (OK, want)
    for k in env:
        defaults.delenv(k)
    assert plan(OUT, 32640, 2560, 0.1, 1, 0) == (OK, [4, 0, 1, 256, 320])
    assert plan(OUT, 32640, 2560, 0.1, 0, 0) == (OK, [2, 1, 0, 768, 320])


def test_plan_dropout_below_the_16_bit_threshold_is_no_dropout(defaults):
    """thr16 = (uint32_t)(p * 65536 + 0.5): p < 2^-17 leaves it 0, and then `marked` selects nothing."""
    assert plan(OUT, 32640, 2560, 7e-6, 1, 0) == (OK, [4, 0, 0, 256, 320])
    assert plan(OUT, 32640, 2560, 7e-6, 0, 0) == (OK, [4, 0, 0, 256, 320])
    assert plan(ALL_T, 32640, 2560, 7e-6, 1, 1) == (OK, [4, 0, 0, 256, 320])
    assert plan(OUT, 1088, 1024, 7e-6, 1, 0) == (OK, [4, 0, 0, 272, 128])
    assert plan(OUT, 32640, 2560, 8e-6, 1, 0) == (OK, [4, 0, 1, 256, 320])
    assert plan(OUT, 32640, 2560, 8e-6, 0, 0) == (OK, [2, 1, 0, 768, 320])


@pytest.mark.parametrize("args", [
    (IN, 32640, 2560, 0.1, 1, 0),       # marked zeros live in a 16-bit x
    (IN, 32640, 2560, 0.0, 1, 0),
    (OUT, 32640, 2564, 0.0, 0, 0),      # h % 8
    (OUT, 32640, 4104, 0.0, 0, 0),      # h > 4096
    (OUT, 32640, 0, 0.0, 0, 0),
    (OUT, 0, 2560, 0.0, 0, 0),
    (OUT, -4, 2560, 0.0, 0, 0),
    (OUT, 32640, 2560, 1.0, 0, 0),
    (OUT, 32640, 2560, -0.1, 0, 0),
    (OUT, 32640, 2560, float("nan"), 0, 0),
    (3, 32640, 2560, 0.0, 0, 0),
    (-1, 32640, 2560, 0.0, 0, 0),
])
def test_plan_refuses_what_the_launch_refuses(defaults, args):
    assert plan(*args) == (ERR_ARG, [-1] * 5)


def test_pair_plan(defaults):
    """LN2' + LN3' in one pass: two rows in flight, two workgroups per CU, rows of at least four waves."""
    assert pair_plan(32640, 2560, 0.1) == (OK, [2, 0, 1, 512, 320])
    assert pair_plan(32640, 2560, 0.0) == (OK, [2, 0, 0, 512, 320])
    assert pair_plan(32640, 1600, 0.1) == (OK, [2, 0, 1, 512, 256])
    assert pair_plan(32640, 4096, 0.1) == (OK, [2, 0, 1, 512, 512])
    assert pair_plan(600, 2560, 0.1) == (OK, [2, 0, 1, 150, 320])
    assert pair_plan(5, 2560, 0.1) == (OK, [2, 0, 1, 2, 320])
    assert pair_plan(1, 2560, 0.0) == (OK, [2, 0, 0, 1, 320])
    for rows, h, p, rc in ((32640, 1536, 0.1, ERR_UNSUPPORTED), (1088, 1024, 0.0, ERR_UNSUPPORTED), (32640, 1604, 0.1, ERR_ARG),
                           (32640, 4104, 0.1, ERR_ARG), (0, 2560, 0.1, ERR_ARG), (32640, 2560, 1.0, ERR_ARG)):
        assert pair_plan(rows, h, p) == (rc, [-1] * 5), (rows, h, p)


def test_switches_read_once_per_process():
    """COGV_LN_BWD_ROWS and COGV_LN_BWD_PAIR_BLOCKS are fixed at the first launch of a process: a fresh one for each side."""
    code = ("import ctypes; from cogview_amd import _lib; L = _lib.lib(); o = (ctypes.c_int * 5)(); "
            "assert L.cogv_ln_bwd_plan(1, 32640, 2560, 0.0, 0, 1, o) == 0; a = list(o); "
            "assert L.cogv_ln_bwd_pair_plan(32640, 2560, 0.1, o) == 0; print(a, list(o))")

    def run(**env):
        e = {k: v for k, v in os.environ.items() if k not in ("COGV_LN_BWD_ROWS", "COGV_LN_BWD_PAIR_BLOCKS")}
        e.update(env)
        return subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, capture_output=True, text=True, check=True).stdout.strip()
    assert run() == "[2, 0, 0, 256, 320] [2, 0, 1, 512, 320]"
    assert run(COGV_LN_BWD_ROWS="4", COGV_LN_BWD_PAIR_BLOCKS="256") == "[4, 0, 0, 256, 320] [2, 0, 1, 256, 320]"
    assert run(COGV_LN_BWD_ROWS="2", COGV_LN_BWD_PAIR_BLOCKS="768") == "[2, 0, 0, 256, 320] [2, 0, 1, 768, 320]"
