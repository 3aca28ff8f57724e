"""CPU: what cogv_gemm and cogv_gemm_grouped decide before they launch (cogv_gemm_plan: a host-only query that calls the functions
every launch uses, csrc/gemm_plan.h): kernel generation, tiles, effective split-K, grid, threads, dynamic LDS, the split-K reduce's
blocks, the exact-prefetch switch of generation 4, and every refusal with its code.  A wrong grid or LDS size shows on a GPU only
as a fault or as tiles nobody computed.
Every expectation below is a literal worked out by hand from the dispatch this plan replaced (launch_gemm, launch_pp64,
launch_glds and build_gemm_args of csrc/gemm.hip before it), for a device of 256 CUs; none is computed by the library:
    generation 1 (kernel_variant 1; K % 64 != 0, M or N < 64)        128x128 tiles, grid (tiles, splitk), 256 threads, 65536 B
    generation 2 (3; M or N < 256, an operand of 4 GiB or more)      256x128 tiles, grid (tiles, splitk), 256 threads, 3 * (256 + 128) * 2 * 32 = 73728 B
    generation 3 (9)                                                 256x256 tiles, grid min(items, CUs - reserved), 512 threads, 2 * 65536 = 131072 B
    generation 4 (10; auto for M, N >= 256 unless generation 2 fills its 2 * CUs slots 1.1 x better)     the same with 256 threads, 131072 + 4 * 4096 = 147456 B
    split-K: clamped to the ceil(K / 64) k-tiles, then re-derived from ceil(k-tiles / splits) so that no split is empty; the reduce
    pass runs min(ceil(M * N / 8 / 256), 2048) blocks."""
import ctypes
import json
import os
import subprocess
import sys

import pytest

from cogview_amd import _lib
from cogview_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, ERR_ARG, ERR_UNSUPPORTED = 0, 1, 3
F16, BF16 = 0, 1
BIAS, GELU, DGELU, DROPOUT, ABSMAX, ACCUM, COLSUM, GELU_DAUX, MULAUX = 1, 2, 4, 8, 16, 32, 64, 128, 256
INTS = 17
UNTOUCHED = [-1] * INTS
NT, NN, TN, TA = 0, 1, 2, 3                       # layout index: -, trans_b, both, trans_a only
SKINNY = [1] + [0] * 16


def desc(M, N, K, layout=NT, dtype=F16, **kw):
    """A contiguous problem whose pointers are dummy non-null, 16-byte aligned integers (never dereferenced by the query); the
    split-K workspace is there and large enough whenever splitk asks for one."""
    d = _lib.GemmDesc()
    d.dtype, d.M, d.N, d.K = dtype, M, N, K
    d.trans_a, d.trans_b = int(layout in (TN, TA)), int(layout in (NN, TN))
    d.lda, d.ldb, d.ldc = (M if d.trans_a else K), (N if d.trans_b else K), N
    d.A, d.B, d.C = 0x10000, 0x20000, 0x30000
    d.workspace, d.workspace_bytes = 0x40000, 1 << 40
    for k, v in kw.items():
        assert hasattr(d, k), k
        setattr(d, k, v)
    return d


def plan(d, cus=256):
    out = (ctypes.c_int * INTS)(*UNTOUCHED)
    rc = _lib.lib().cogv_gemm_plan(ctypes.byref(d) if d is not None else None, 0, cus, out)
    return rc, list(out)


def plan_group(descs, cus=256, count=None):
    arr = (_lib.GemmDesc * max(len(descs), 1))(*descs)
    out = (ctypes.c_int * (INTS * 16))(*([-1] * (INTS * 16)))
    rc = _lib.lib().cogv_gemm_plan(arr, len(descs) if count is None else count, cus, out)
    return rc, [list(out[i * INTS:(i + 1) * INTS]) for i in range(16)]


def G1(tm, tn, splitk=1, kps=1, reduce=0, layout=NT):
    return [0, 1, 128, 128, tm, tn, splitk, kps, 0, tm * tn * splitk, tm * tn, splitk, 256, 65536, reduce, 0, layout]


def G2(tm, tn, splitk=1, kps=1, reduce=0, layout=NT):
    return [0, 2, 256, 128, tm, tn, splitk, kps, 0, tm * tn * splitk, tm * tn, splitk, 256, 73728, reduce, 0, layout]


def G3(tm, tn, grid, splitk=1, kps=1, reduce=0, layout=NT, items=None, start=0):
    return [0, 3, 256, 256, tm, tn, splitk, kps, start, tm * tn * splitk if items is None else items, grid, 1, 512, 131072, reduce, 0, layout]


def G4(tm, tn, grid, splitk=1, kps=1, reduce=0, xp=0, layout=NT, items=None, start=0):
    return [0, 4, 256, 256, tm, tn, splitk, kps, start, tm * tn * splitk if items is None else items, grid, 1, 256, 147456, reduce, xp, layout]


# the transformer layers' launches in the two training configurations bench.py times (30 sequences x 1088 positions = 32640 tokens
# x features, 256 CUs): forward NT, dgrad NN; the weight gradients are grouped launches (test_grouped_plan)
FWD_4B = [0, 4, 256, 256, 128, 40, 1, 40, 0, 5120, 256, 1, 256, 147456, 0, 1, NT]
TRAIN_STEP = [
    # 4B: h = 2560, 32640 tokens -- QKV, attention output, h -> 4h, 4h -> h, each forward and dgrad
    ((32640, 7680, 2560, NT), G4(128, 30, 256, kps=40, xp=1)), ((32640, 2560, 7680, NN), G4(128, 10, 256, kps=120, xp=1, layout=NN)),
    ((32640, 2560, 2560, NT), G4(128, 10, 256, kps=40, xp=1)), ((32640, 2560, 2560, NN), G4(128, 10, 256, kps=40, xp=1, layout=NN)),
    ((32640, 10240, 2560, NT), FWD_4B), ((32640, 2560, 10240, NN), G4(128, 10, 256, kps=160, xp=1, layout=NN)),
    ((32640, 2560, 10240, NT), G4(128, 10, 256, kps=160, xp=1)), ((32640, 10240, 2560, NN), G4(128, 40, 256, kps=40, xp=1, layout=NN)),
    # 336M: h = 1024, the same 32640 tokens
    ((32640, 3072, 1024, NT), G4(128, 12, 256, kps=16, xp=1)), ((32640, 1024, 3072, NN), G4(128, 4, 256, kps=48, xp=1, layout=NN)),
    ((32640, 1024, 1024, NT), G4(128, 4, 256, kps=16, xp=1)), ((32640, 1024, 1024, NN), G4(128, 4, 256, kps=16, xp=1, layout=NN)),
    ((32640, 4096, 1024, NT), G4(128, 16, 256, kps=16, xp=1)), ((32640, 1024, 4096, NN), G4(128, 4, 256, kps=64, xp=1, layout=NN)),
    ((32640, 1024, 4096, NT), G4(128, 4, 256, kps=64, xp=1)), ((32640, 4096, 1024, NN), G4(128, 16, 256, kps=16, xp=1, layout=NN)),
]


@pytest.mark.parametrize("shape,want", TRAIN_STEP)
def test_training_step_launches(shape, want):
    M, N, K, layout = shape
    for dtype in (F16, BF16):
        assert plan(desc(M, N, K, layout, dtype)) == (OK, want)


@pytest.mark.parametrize("d,want", [
    # auto dispatch
    (desc(256, 256, 128), G4(1, 1, 1, kps=2)),                                        # 2 k-tiles: no exact prefetch
    (desc(33024, 384, 64), G2(129, 3)),                                               # fill: 387 of 512 slots against 258 of 512 (x 1.1)
    (desc(128, 512, 64), G2(1, 4)), (desc(512, 128, 64), G2(2, 1)),                   # M or N in [64, 256)
    (desc(255, 256, 64), G2(1, 2)), (desc(64, 64, 64), G2(1, 1)),
    (desc(512, 512, 72), G1(4, 4, kps=2)), (desc(64, 64, 72), G1(1, 1, kps=2)),       # K % 64 != 0
    (desc(56, 512, 64), G1(1, 4)), (desc(512, 56, 64), G1(4, 1)),                     # M or N < 64
    (desc(8, 512, 64), G1(1, 4)), (desc(9, 512, 512), G1(1, 4, kps=8)),               # few rows outside the skinny-M kernels' shapes
    (desc(8, 512, 512), SKINNY), (desc(1, 8, 512), SKINNY), (desc(8, 512, 512, splitk=4), SKINNY),       # M <= 8, K % 512 == 0
    (desc(8, 512, 512, NN), G1(1, 4, kps=8, layout=NN)),                              # ... which take the NT layout only
    (desc(8, 512, 512, kernel_variant=3), G1(1, 4, kps=8)),                           # ... and auto dispatch only
    (desc(264, 520, 256), G4(2, 3, 6, kps=4)),                                        # edge tiles; 6 items <= 256 CUs: no exact prefetch
    (desc(264, 136, 128, TA), G2(2, 2, kps=2, layout=TA)), (desc(256, 256, 64, TA), G4(1, 1, 1, layout=TA)),
    (desc(256, 256, 64, TN), G4(1, 1, 1, layout=TN)), (desc(64, 64, 4, TN), G1(1, 1, layout=TN)),
    # an operand of 4 GiB: generation 2 (64-bit addresses); one row stride less: generation 4
    (desc(256, 256, 64, lda=1 << 23), G2(1, 2)), (desc(256, 256, 64, lda=(1 << 23) - 8), G4(1, 1, 1)),
    (desc(256, 256, 64, ldb=1 << 23), G2(1, 2)), (desc(256, 256, 64, NN, ldb=1 << 25), G2(1, 2, layout=NN)),
    (desc(256, 256, 64, TN, lda=1 << 25), G2(1, 2, layout=TN)), (desc(256, 256, 64, TN, lda=(1 << 25) - 8), G4(1, 1, 1, layout=TN)),
    # explicit variants on a shape each takes
    (desc(512, 512, 128, kernel_variant=1), G1(4, 4, kps=2)), (desc(512, 512, 128, kernel_variant=3), G2(2, 4, kps=2)),
    (desc(512, 512, 128, kernel_variant=9), G3(2, 2, 4, kps=2)), (desc(512, 512, 128, kernel_variant=10), G4(2, 2, 4, kps=2)),
    (desc(33024, 384, 64, kernel_variant=10), G4(129, 2, 256)),                       # ... also where auto prefers generation 2
    (desc(512, 512, 128, NN, BF16, kernel_variant=9), G3(2, 2, 4, kps=2, layout=NN)),
    # 9 and 10 where the persistent kernels do not take the problem: what auto picks
    (desc(255, 512, 128, kernel_variant=9), G2(1, 4, kps=2)), (desc(255, 512, 128, kernel_variant=10), G2(1, 4, kps=2)),
    (desc(255, 512, 128), G2(1, 4, kps=2)), (desc(256, 256, 64, lda=1 << 23, kernel_variant=10), G2(1, 2)),
    (desc(512, 512, 72, kernel_variant=9), G1(4, 4, kps=2)), (desc(56, 512, 64, kernel_variant=3), G1(1, 4)),
    # an unknown variant is auto
    (desc(512, 512, 128, kernel_variant=7), G4(2, 2, 4, kps=2)), (desc(33024, 384, 64, kernel_variant=2), G2(129, 3)),
    (desc(512, 512, 128, kernel_variant=-1), G4(2, 2, 4, kps=2)),
    # the fused column sums: generation 4 unless 3 is asked for, also where auto would take generation 2
    (desc(512, 512, 128, flags=COLSUM, colsum_partial=0x50000), G4(2, 2, 4, kps=2)),
    (desc(512, 512, 128, flags=COLSUM, colsum_partial=0x50000, kernel_variant=9), G3(2, 2, 4, kps=2)),
    (desc(512, 512, 128, flags=COLSUM, colsum_partial=0x50000, kernel_variant=7), G4(2, 2, 4, kps=2)),
    (desc(33024, 384, 64, NN, flags=COLSUM, colsum_partial=0x50000), G4(129, 2, 256, layout=NN)),
])
def test_dispatch(d, want):
    assert plan(d) == (OK, want)


@pytest.mark.parametrize("d,want", [
    (desc(512, 512, 320, splitk=4), G4(2, 2, 12, splitk=3, kps=2, reduce=128)),       # 5 k-tiles at 4 -> 2 per split -> 3 splits
    (desc(128, 512, 128, splitk=8), G2(1, 4, splitk=2, kps=1, reduce=32)),            # clamped to the 2 k-tiles
    (desc(128, 512, 64, splitk=8), G2(1, 4)),                                         # one k-tile: no split, no reduce
    (desc(4096, 4096, 128, splitk=2), G4(16, 16, 256, splitk=2, kps=1, reduce=2048)), # 8192 blocks of 256 x 8 outputs: capped
    (desc(264, 520, 256, splitk=2), G4(2, 3, 12, splitk=2, kps=2, reduce=68)),        # 264 x 65 = 17160 vectors -> 67.03 -> 68
    (desc(56, 64, 256, splitk=2), G1(1, 1, splitk=2, kps=2, reduce=2)),
    (desc(64, 64, 72, splitk=2), G1(1, 1, splitk=2, kps=1, reduce=2)),                # ceil(72 / 64) = 2 k-tiles
    (desc(64, 64, 256, splitk=2), G2(1, 1, splitk=2, kps=2, reduce=2)),
    (desc(256, 256, 256, splitk=2, kernel_variant=9), G3(1, 1, 2, splitk=2, kps=2, reduce=32)),
    (desc(256, 256, 256, splitk=3), G4(1, 1, 2, splitk=2, kps=2, reduce=32)),         # 4 k-tiles at 3 -> 2 per split -> 2 splits
    (desc(256, 256, 256, splitk=0), G4(1, 1, 1, kps=4)), (desc(256, 256, 256, splitk=-3), G4(1, 1, 1, kps=4)),
    # the split takes part in the fill rule: 129 x 3 x 2 = 774 of 1024 slots against 129 x 2 x 2 = 516 of 768 (x 1.1 = 0.739 < 0.756)
    (desc(33024, 384, 128, splitk=2), G2(129, 3, splitk=2, kps=1, reduce=2048)),
])
def test_split_k(d, want):
    assert plan(d) == (OK, want)


@pytest.mark.parametrize("d,cus,want", [
    # exact prefetch: one problem, no split, an even number >= 4 of k-tiles, more items than CUs -- one case on each side of each term
    (desc(8192, 8192, 512), 256, G4(32, 32, 256, kps=8, xp=1)),
    (desc(8192, 8192, 512, splitk=2), 256, G4(32, 32, 256, splitk=2, kps=4, reduce=2048)),
    (desc(8192, 8192, 128), 256, G4(32, 32, 256, kps=2)), (desc(8192, 8192, 256), 256, G4(32, 32, 256, kps=4, xp=1)),
    (desc(8192, 8192, 320), 256, G4(32, 32, 256, kps=5)), (desc(8192, 8192, 384), 256, G4(32, 32, 256, kps=6, xp=1)),
    (desc(4096, 4096, 256), 256, G4(16, 16, 256, kps=4)), (desc(4352, 4096, 256), 256, G4(17, 16, 256, kps=4, xp=1)),
    # ... against the CUs of the device, whatever is reserved
    (desc(4352, 4096, 256), 304, G4(17, 16, 272, kps=4)), (desc(4096, 4096, 256), 128, G4(16, 16, 128, kps=4, xp=1)),
    (desc(8192, 8192, 512, kernel_variant=9), 256, G3(32, 32, 256, kps=8)),           # generation 3 has none
])
def test_exact_prefetch_terms(d, cus, want):
    assert plan(d, cus) == (OK, want)


def test_exact_prefetch_switch_in_a_fresh_process():
    """COGV_GEMM_XP=0 (read per launch) changes nothing but the switch."""
    code = ("import json, sys; sys.path.insert(0, %r)\n"
            "from tests.test_gemm_plan import plan, desc\n"
            "print(json.dumps([plan(desc(32640, 10240, 2560)), plan(desc(8192, 8192, 256))]))\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, COGV_GEMM_XP="0"), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got == [[OK, FWD_4B[:15] + [0, NT]], [OK, G4(32, 32, 256, kps=4)]]
    assert plan(desc(32640, 10240, 2560)) == (OK, FWD_4B) and FWD_4B[15] == 1


def test_reserved_cus():
    """the persistent grid is max(CUs - reserved, 8), at most the items; the fill rule and the prefetch term look at all CUs"""
    lib = _lib.lib()
    prev = lib.cogv_gemm_reserve_cus(16)
    try:
        assert plan(desc(32640, 10240, 2560)) == (OK, FWD_4B[:10] + [240] + FWD_4B[11:])
        assert plan(desc(32640, 10240, 2560), 304) == (OK, FWD_4B[:10] + [288] + FWD_4B[11:])
        assert plan(desc(512, 512, 128)) == (OK, G4(2, 2, 4, kps=2))
        assert plan(desc(8192, 8192, 512, kernel_variant=9)) == (OK, G3(32, 32, 240, kps=8))
        assert plan(desc(33024, 384, 64)) == (OK, G2(129, 3))
        assert plan_group([desc(768, 256, 256, TN), desc(1024, 256, 256, TN)])[1][0][10] == 7
        lib.cogv_gemm_reserve_cus(60)
        assert plan(desc(32640, 10240, 2560), 64) == (OK, FWD_4B[:10] + [8] + FWD_4B[11:])
        assert plan(desc(4096, 4096, 256), 64) == (OK, G4(16, 16, 8, kps=4, xp=1))
        assert lib.cogv_gemm_reserve_cus(-1) == 60
    finally:
        lib.cogv_gemm_reserve_cus(prev)
    assert plan(desc(32640, 10240, 2560)) == (OK, FWD_4B)


PARTIAL = dict(flags=COLSUM, colsum_partial=0x50000)
REFUSALS = [
    # build_gemm_args, in its order
    (dict(dtype=2), ERR_UNSUPPORTED), (dict(dtype=-1), ERR_UNSUPPORTED), (dict(dtype=2, M=0), ERR_UNSUPPORTED), (dict(dtype=2, N=260), ERR_UNSUPPORTED),
    (dict(M=0), ERR_ARG), (dict(N=-8), ERR_ARG), (dict(K=0), ERR_ARG),
    (dict(N=260), ERR_ARG), (dict(ldc=516), ERR_ARG), (dict(lda=132), ERR_ARG), (dict(ldb=4), ERR_ARG),
    (dict(K=132, lda=136, ldb=136), ERR_ARG), (dict(K=132, lda=136, ldb=512, trans_b=1), ERR_ARG), (dict(K=132, lda=512, ldb=136, trans_a=1), ERR_ARG),
    (dict(M=260, lda=264, trans_a=1), ERR_ARG),
    (dict(A=0x10008), ERR_ARG), (dict(B=0x20004), ERR_ARG), (dict(C=0x30001), ERR_ARG),
    (dict(flags=BIAS), ERR_ARG), (dict(flags=BIAS, bias=0x60008), ERR_ARG),
    (dict(flags=DGELU), ERR_ARG), (dict(flags=MULAUX), ERR_ARG), (dict(flags=DGELU | MULAUX, aux=0x70000, ldaux=512), ERR_ARG),
    (dict(flags=GELU_DAUX), ERR_ARG), (dict(flags=GELU, aux=0x70004, ldaux=512), ERR_ARG), (dict(flags=DGELU, aux=0x70000, ldaux=516), ERR_ARG),
    (dict(flags=ABSMAX), ERR_ARG),
    (dict(flags=DROPOUT, dropout_p=1.0), ERR_ARG), (dict(flags=DROPOUT, dropout_p=-0.5), ERR_ARG), (dict(flags=DROPOUT, dropout_p=float("nan")), ERR_ARG),
    (dict(dropout_row0=-1), ERR_ARG),
    (dict(flags=COLSUM), ERR_ARG), (dict(flags=COLSUM, colsum_partial=0x50004), ERR_ARG), (dict(PARTIAL, splitk=2), ERR_ARG), (dict(PARTIAL, out_f32=1), ERR_ARG),
    (dict(PARTIAL, K=64, splitk=2), ERR_ARG),                                         # the split asked for, not the effective one
    (dict(splitk=2, workspace=0), ERR_ARG), (dict(splitk=2, workspace=0x40008), ERR_ARG), (dict(splitk=2, workspace_bytes=2 * 512 * 512 * 4 - 1), ERR_ARG),
    # ... which come before what the dispatch refuses
    (dict(PARTIAL, M=56, colsum_partial=0), ERR_ARG), (dict(PARTIAL, kernel_variant=3, C=0x30008), ERR_ARG),
    # the dispatch: the fused column sums exist in generations 3 and 4 only
    (dict(PARTIAL, M=56), ERR_UNSUPPORTED), (dict(PARTIAL, K=72), ERR_UNSUPPORTED), (dict(PARTIAL, kernel_variant=1), ERR_UNSUPPORTED),      # not an LDS-ring shape
    (dict(PARTIAL, M=8, K=512), ERR_UNSUPPORTED),                                     # (nor the skinny-M kernels')
    (dict(PARTIAL, M=255), ERR_UNSUPPORTED), (dict(PARTIAL, N=248), ERR_UNSUPPORTED), (dict(PARTIAL, M=128, N=128), ERR_UNSUPPORTED),
    (dict(PARTIAL, lda=1 << 22), ERR_UNSUPPORTED), (dict(PARTIAL, ldb=1 << 22), ERR_UNSUPPORTED),       # 512 rows x 2^22 x 2 B = 4 GiB
    (dict(PARTIAL, kernel_variant=3), ERR_UNSUPPORTED), (dict(PARTIAL, M=255, kernel_variant=9), ERR_UNSUPPORTED),
]


@pytest.mark.parametrize("kw,rc", REFUSALS)
def test_refusals(kw, rc):
    """a 512 x 512 x 128 forward product with `kw` changed: the launch's code, and `out` left untouched"""
    assert plan(desc(**dict(dict(M=512, N=512, K=128), **kw))) == (rc, UNTOUCHED)


def test_refusals_leave_no_false_positives():
    """each refusal above is one step away from a plan"""
    assert plan(desc(512, 512, 128, **PARTIAL)) == (OK, G4(2, 2, 4, kps=2))
    assert plan(desc(512, 512, 128, splitk=2, workspace_bytes=2 * 512 * 512 * 4)) == (OK, G4(2, 2, 8, splitk=2, kps=1, reduce=128))
    assert plan(desc(512, 512, 128, flags=BIAS | GELU | GELU_DAUX | ABSMAX | DROPOUT | ACCUM, bias=0x60000, aux=0x70000, ldaux=512,
                     absmax=0x80000, dropout_p=0.1, dropout_row0=4096)) == (OK, G4(2, 2, 4, kps=2))
    assert plan(desc(512, 512, 128, lda=(1 << 22) - 8, **PARTIAL)) == (OK, G4(2, 2, 4, kps=2))


def test_refusals_of_the_call_itself():
    lib, out = _lib.lib(), (ctypes.c_int * (INTS * 16))()
    d = desc(512, 512, 128)
    assert lib.cogv_gemm_plan(None, 0, 256, out) == ERR_ARG and lib.cogv_gemm_plan(None, 2, 256, out) == ERR_ARG
    assert lib.cogv_gemm_plan(ctypes.byref(d), 0, 256, None) == ERR_ARG
    assert lib.cogv_gemm_plan(ctypes.byref(d), -1, 256, out) == ERR_ARG and lib.cogv_gemm_plan(ctypes.byref(d), 17, 256, out) == ERR_ARG
    assert lib.cogv_gemm_plan(ctypes.byref(d), 0, -1, out) == ERR_ARG


# ---------------------------------------------------------------------------------------------------------------------------
# cogv_gemm_grouped: the four weight gradients of tests/test_kernels_gpu.py::test_gemm_grouped_wgrads, (out, in) features
WGRADS = [(768, 256), (256, 256), (1024, 256), (256, 1024)]


def test_grouped_plan():
    """generation 4 for every problem; the work list is the problems' items one after the other: 3, 1, 4, 4 tiles"""
    rc, out = plan_group([desc(M, N, 1088, TN) for M, N in WGRADS])
    assert rc == OK
    assert out[:4] == [G4(3, 1, 12, kps=17, layout=TN, items=12, start=0), G4(1, 1, 12, kps=17, layout=TN, items=12, start=3),
                       G4(4, 1, 12, kps=17, layout=TN, items=12, start=4), G4(1, 4, 12, kps=17, layout=TN, items=12, start=8)]
    assert out[4:] == [UNTOUCHED] * 12
    # split in two: 17 k-tiles -> 9 per split; items 6, 2, 8, 8; each problem has its reduce pass
    rc, out = plan_group([desc(M, N, 1088, TN, BF16, splitk=2) for M, N in WGRADS])
    assert rc == OK
    assert out[:4] == [G4(3, 1, 24, 2, 9, 96, layout=TN, items=24, start=0), G4(1, 1, 24, 2, 9, 32, layout=TN, items=24, start=6),
                       G4(4, 1, 24, 2, 9, 128, layout=TN, items=24, start=8), G4(1, 4, 24, 2, 9, 128, layout=TN, items=24, start=16)]
    # sixteen problems of 300 tiles fill the grid; several problems: no exact prefetch, one problem: as cogv_gemm's
    rc, out = plan_group([desc(7680, 2560, 256, TN)] * 16)
    assert rc == OK and [o[8] for o in out] == [300 * i for i in range(16)] and all(o[9:11] == [4800, 256] and o[15] == 0 for o in out)
    assert plan_group([desc(7680, 2560, 256, TN)])[1][0] == G4(30, 10, 256, kps=4, xp=1, layout=TN) == plan(desc(7680, 2560, 256, TN))[1]
    assert plan_group([desc(7680, 2560, 256, TN)] * 2)[1][1] == G4(30, 10, 256, kps=4, layout=TN, items=600, start=300)
    # the training steps' launches: the four weight gradients of four layers, K = 32640 tokens = 510 k-tiles, no split
    for h, tiles in ((2560, [300, 100, 400, 400]), (1024, [48, 16, 64, 64])):
        layer = [desc(3 * h, h, 32640, TN), desc(h, h, 32640, TN), desc(4 * h, h, 32640, TN), desc(h, 4 * h, 32640, TN)]
        rc, out = plan_group(layer * 4)
        starts = [sum((tiles * 4)[:i]) for i in range(16)]
        assert rc == OK and [o[8] for o in out] == starts and starts[4] == sum(tiles) and starts[15] == 4 * sum(tiles) - tiles[3]
        assert all(o[:4] == [0, 4, 256, 256] and o[6:8] == [1, 510] and o[9:] == [4 * sum(tiles), 256, 1, 256, 147456, 0, 0, TN] for o in out)
        assert [o[4] * o[5] for o in out] == tiles * 4 and out[0][4:6] == [3 * h // 256, h // 256] and out[3][4:6] == [h // 256, 4 * h // 256]
    # kernel_variant is not looked at
    assert plan_group([desc(768, 256, 64, TN, kernel_variant=3)])[1][0] == G4(3, 1, 3, layout=TN)


@pytest.mark.parametrize("descs,rc", [
    ([desc(768, 256, 64, TN), desc(256, 248, 64, TN)], ERR_UNSUPPORTED), ([desc(128, 256, 64, TN)], ERR_UNSUPPORTED),
    ([desc(768, 256, 72, TN)], ERR_UNSUPPORTED), ([desc(768, 256, 64, TN, lda=1 << 25)], ERR_UNSUPPORTED),
    ([desc(768, 256, 64, TN), desc(768, 256, 64, TN, BF16)], ERR_ARG), ([desc(768, 256, 64, TN), desc(768, 256, 64, NN)], ERR_ARG),
    ([desc(768, 256, 64, TN), desc(260, 256, 64, TN, lda=264)], ERR_ARG),
    ([desc(768, 248, 64, TN), desc(768, 256, 64, TN, A=0x10008)], ERR_UNSUPPORTED),   # the first problem's refusal comes first
    ([desc(768, 256, 64, TN, A=0x10008), desc(768, 248, 64, TN)], ERR_ARG),
    ([desc(768, 256, 64, TN)] * 17, ERR_ARG),
])
def test_grouped_refusals(descs, rc):
    assert plan_group(descs) == (rc, [UNTOUCHED] * 16)


# ---------------------------------------------------------------------------------------------------------------------------
# ops.gemm (fused column sums) and ops.gemm_grouped ask this plan whether the persistent kernel takes a problem; their
# predecessors restated it in Python.  The record of the predecessors, on the numbers a descriptor carries:
def _old_fuse_colsum(M, N, K, a_rows, lda, b_rows, ldb, trans_a, trans_b, variant, out_f32):
    return (M >= 256 and N >= 256 and K % 64 == 0 and variant in (0, 9, 10) and not out_f32 and lda * a_rows * 2 < 2 ** 32
            and ldb * b_rows * 2 < 2 ** 32 and (trans_b is False or N % 8 == 0) and not trans_a)


def _old_grouped_ok(M, N, K):
    return M >= 256 and N >= 256 and K % 64 == 0


def test_python_predicates_against_their_predecessors():
    """Over layouts x M x N x K x operand spans (x variant x output type for the column sums): the library-backed predicates accept
    nothing the Python ones refused, and refuse what those accepted in exactly three cases, each a problem the library itself
    refuses -- an operand span of 4 GiB or more (the grouped predicate had no such term), M % 8 under trans_a, and N % 8 (the
    persistent kernels' term under trans_b, the argument check's in any layout)."""
    kinds = {"fuse": {"span": 0, "M & 7 under trans_a": 0, "N & 7": 0}, "grouped": {"span": 0, "M & 7 under trans_a": 0, "N & 7": 0}}
    n = 0
    for trans_a in (False, True):
        for trans_b in (False, True):
            for M in (248, 256, 260, 264):
                for N in (248, 256, 260, 264):
                    for K in (64, 96, 128):
                        a_rows, b_rows = (K if trans_a else M), (K if trans_b else N)
                        a_ld, b_ld = (M + 7) // 8 * 8 if trans_a else K, (N + 7) // 8 * 8 if trans_b else K
                        a_big, b_big = (-(-2 ** 31 // a_rows) + 7) // 8 * 8, (-(-2 ** 31 // b_rows) + 7) // 8 * 8     # the first stride at 4 GiB
                        for lda, ldb in ((a_ld, b_ld), (a_big, b_ld), (a_big - 8, b_ld), (a_ld, b_big), (a_ld, b_big - 8)):
                            d = desc(M, N, K, lda=lda, ldb=ldb, trans_a=int(trans_a), trans_b=int(trans_b), ldc=(N + 7) // 8 * 8)
                            span = lda * a_rows * 2 >= 2 ** 32 or ldb * b_rows * 2 >= 2 ** 32
                            why = {"span": span, "M & 7 under trans_a": trans_a and M % 8 != 0, "N & 7": N % 8 != 0}
                            cases = [("grouped", _old_grouped_ok(M, N, K), ops._persistent_takes(d))]
                            for variant in (0, 1, 3, 9, 10):
                                for out_f32 in (0, 1):
                                    d.out_f32 = out_f32
                                    cases.append(("fuse", _old_fuse_colsum(M, N, K, a_rows, lda, b_rows, ldb, trans_a, trans_b, variant, out_f32),
                                                  ops._fuse_colsum(d, variant)))
                            d.out_f32 = 0
                            for which, old, new in cases:
                                n += 1
                                assert not (new and not old), (which, trans_a, trans_b, M, N, K, lda, ldb)
                                assert (old and not new) == (old and any(why.values())), (which, trans_a, trans_b, M, N, K, lda, ldb)
                                if old and not new:
                                    for k, v in why.items():
                                        kinds[which][k] += bool(v)
    assert n == 2 * 2 * 4 * 4 * 3 * 5 * 11
    # the grouped predicate disagrees in all three ways; the column sums' already knew the spans and never had trans_a
    assert all(v > 0 for v in kinds["grouped"].values()), kinds
    assert kinds["fuse"]["span"] == 0 and kinds["fuse"]["M & 7 under trans_a"] == 0 and kinds["fuse"]["N & 7"] > 0, kinds


# ---------------------------------------------------------------------------------------------------------------------------
# The grid of tests/gemm_cells.py (tests/test_gemm_cells_gpu.py executes it): it reaches every path it is there for.
from tests import gemm_cells as GC  # noqa: E402


def _cell_desc(gen, shape, layout, dtype, cell):
    M, N, K, splitk, _ = shape
    return desc(M, N, K, layout, dtype, splitk=splitk, kernel_variant=GC.VARIANT[gen], flags=cell.flags, out_f32=int(cell.out_f32),
                bias=0x60000, aux=0x70000, ldaux=N, absmax=0x80000, dropout_p=0.5, dropout_row0=cell.row0, colsum_partial=0x50000)


def test_cell_grid_plans_what_its_rows_name():
    """every cell: the generation of its row, that generation's tile, the tiles, effective split-K and k-tiles per split written
    beside the shape -- or the refusal code listed for it, with `out` untouched"""
    n = refused = 0
    for gen in GC.GENERATIONS:
        for shape, (tm, tn, splitk, kps) in GC.GRID[gen]:
            for layout in GC.LAYOUTS:
                for dtype in (F16, BF16):
                    for cell in GC.cells_of(shape[3]):
                        rc, out = plan(_cell_desc(gen, shape, layout, dtype, cell))
                        want = GC.refusal(gen, shape[3], cell)
                        n += 1
                        if want != OK:
                            refused += 1
                            assert (rc, out) == (want, UNTOUCHED), (gen, shape, layout, cell)
                        else:
                            assert rc == OK and out[:8] == [0, gen, *GC.TILE[gen], tm, tn, splitk, kps] and out[16] == layout, (gen, shape, layout, cell, out)
    # 20 cells on a shape without split-K, 7 on one with: generation 1 has 3 + 2 shapes, 2 has 2 + 1, 3 and 4 have 3 + 2 each;
    # refused: 4 of the 20 in generations 1 and 2, 1 in 3 and 4, 1 of the 7 everywhere
    assert n == ((3 * 20 + 2 * 7) + (2 * 20 + 7) + 2 * (3 * 20 + 2 * 7)) * 8 and refused == (14 + 9 + 5 + 5) * 8
    # the refusals by their rows: the column sums in generations 1 and 2 (3), with split-K or an fp32 output anywhere (1)
    sums = [c for c in GC.CELLS if c.flags & COLSUM and not c.out_f32]
    assert [c.flags for c in sums] == [DGELU | COLSUM, MULAUX | COLSUM, COLSUM | ACCUM]
    assert [GC.refusal(g, 1, c) for g in GC.GENERATIONS for c in sums] == [ERR_UNSUPPORTED] * 6 + [OK] * 6
    assert all(GC.refusal(g, 2, GC.Cell(MULAUX | COLSUM)) == ERR_ARG and GC.refusal(g, 1, GC.Cell(MULAUX | COLSUM, out_f32=True)) == ERR_ARG for g in GC.GENERATIONS)
    assert GC.Cell(MULAUX | COLSUM) in GC.SPLIT_CELLS and GC.Cell(MULAUX | COLSUM, out_f32=True) in GC.CELLS


def test_cell_grid_reaches_every_path():
    """each generation: an edge tile in M and in N (one of 8 rows, one of 8 columns), a full tile, one, two and three or more
    k-tiles per split, and a split with uneven k-tiles; generation 1 also a ragged K with a tail of 8"""
    for gen in GC.GENERATIONS:
        tile_m, tile_n = GC.TILE[gen]
        shapes = [s for s, _ in GC.GRID[gen]]
        assert any(M % tile_m == 8 for M, N, K, s, w in shapes) and any(N % tile_n == 8 for M, N, K, s, w in shapes), gen
        assert any(M >= tile_m and N >= tile_n for M, N, K, s, w in shapes), gen
        assert any((K + 63) // 64 == 1 for M, N, K, s, w in shapes), gen
        nk = {(K + 63) // 64 for M, N, K, s, w in shapes}
        assert {1, 2} <= nk and max(nk) >= 3, (gen, nk)
        assert any(p[2] > 1 and ((K + 63) // 64) % p[2] != 0 for (M, N, K, s, w), p in GC.GRID[gen]), gen
        assert all(M % 8 == 0 and N % 8 == 0 and K % 8 == 0 for M, N, K, s, w in shapes)
    assert any(K % 64 == 8 for (M, N, K, s, w), _ in GC.GRID[1])
    assert GC.GRID[1][0][0][:2] == (56, 64) and (200, 136, 200, 1, False) in [s for s, _ in GC.GRID[1]]       # 200 = 128 + 72: an edge tile of 72 rows too
    # the rows of the grid as they were decided, literally
    assert [s[:4] for s, _ in GC.GRID[1]][:3] == [(56, 64, 72, 1), (200, 136, 200, 1), (136, 264, 328, 2)]
    assert [s[:4] for s, _ in GC.GRID[2]] == [(64, 64, 64, 1), (264, 136, 128, 1), (520, 264, 192, 2)]
    for gen in (3, 4):
        assert [s for s, _ in GC.GRID[gen]] == [(256, 256, 64, 1, False), (264, 520, 128, 1, False), (520, 264, 192, 2, False),
                                                (520, 520, 192, 1, True), (520, 520, 192, 2, True)]
    assert GC.GROUP == ((256, 264, 128, ACCUM, 1), (520, 256, 192, 0, 2), (264, 520, 64, ACCUM, 1))


def test_cell_flag_sets():
    """the nine flag sets generations 3 and 4 compile an epilogue for (csrc/gemm_gen3.cuh, gemm_gen4.cuh: the chain of p.flags ==
    tests), at least five that only the run-time-flag instance serves, and the fp32 output"""
    compiled = [0, BIAS, ACCUM, BIAS | DROPOUT | ABSMAX, BIAS | GELU, DGELU | COLSUM, DGELU, BIAS | GELU | GELU_DAUX, MULAUX | COLSUM]
    assert sorted(GC.COMPILED) == sorted(compiled)
    sixteen_bit = {c.flags for c in GC.CELLS if not c.out_f32}
    assert set(compiled) <= sixteen_bit
    outside = sixteen_bit - set(compiled)
    assert len(outside) >= 5 and {ABSMAX, BIAS | ACCUM, MULAUX, DROPOUT | ACCUM} <= outside and outside == set(GC.RUNTIME_ONLY)
    assert GC.Cell(BIAS | GELU, aux=True) in GC.CELLS and any(c.row0 == 16 and c.flags & DROPOUT for c in GC.CELLS)
    assert {c.flags for c in GC.CELLS if c.out_f32} == {0, BIAS | ACCUM, BIAS | DROPOUT | ABSMAX, MULAUX | COLSUM}
    assert [(c.flags, c.out_f32) for c in GC.SPLIT_CELLS[:6]] == [(0, False), (BIAS, False), (ACCUM, False), (BIAS | DROPOUT | ABSMAX, False),
                                                                 (BIAS | GELU, False), (ACCUM, True)]
    assert (GC.BIAS, GC.GELU, GC.DGELU, GC.DROPOUT, GC.ABSMAX, GC.ACCUM, GC.COLSUM, GC.GELU_DAUX, GC.MULAUX) == \
        (BIAS, GELU, DGELU, DROPOUT, ABSMAX, ACCUM, COLSUM, GELU_DAUX, MULAUX) == \
        (_lib.EPI_BIAS, _lib.EPI_GELU, _lib.EPI_DGELU, _lib.EPI_DROPOUT, _lib.EPI_ABSMAX, _lib.EPI_ACCUM, _lib.EPI_COLSUM, _lib.EPI_GELU_DAUX, _lib.EPI_MULAUX)


def test_cell_grid_item_hand_over():
    """the 8-workgroup cells: 9 or 18 items on a grid of 8 under the reserve (a workgroup takes a second item), one workgroup per
    item without it; the grouped launch: 14 items over three problems, the second split in two"""
    lib = _lib.lib()
    small = [(gen, s) for gen in (3, 4) for s, _ in GC.GRID[gen] if s[4]]
    assert len(small) == 4 and all(gen in (3, 4) or not s[4] for gen in GC.GENERATIONS for s, _ in GC.GRID[gen])
    group = [desc(M, N, K, TN, splitk=s, flags=f) for M, N, K, f, s in GC.GROUP]
    for gen, s in small:
        assert plan(_cell_desc(gen, s, NN, BF16, GC.Cell(0)))[1][9:11] == [9 * s[3], 9 * s[3]]
    assert [o[8:11] for o in plan_group(group)[1][:3]] == [[0, 14, 14], [2, 14, 14], [8, 14, 14]] and GC.GROUP_ITEMS == 14
    prev = lib.cogv_gemm_reserve_cus(256 - 8)
    try:
        for gen, s in small:
            out = plan(_cell_desc(gen, s, NN, BF16, GC.Cell(0)))[1]
            assert out[9] == 9 * s[3] and out[10] == 8 < out[9], (gen, s, out)
        rc, out = plan_group(group)
        assert rc == OK and [o[8:11] for o in out[:3]] == [[0, 14, 8], [2, 14, 8], [8, 14, 8]] and [o[6:8] for o in out[:3]] == [[1, 2], [2, 2], [1, 1]]
    finally:
        lib.cogv_gemm_reserve_cus(prev)
