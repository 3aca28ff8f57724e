"""GPU: the generation-4 GEMM kernel (csrc/gemm_gen4.cuh) starts every item's accumulators from the first k-tile's MFMAs (C = 0
as an operand) instead of clearing them.  What that can break is an accumulator block that is NOT started on some path into the
k-loop: the tile then carries the sums of the workgroup's previous item -- or of the previous launch, the AGPR file survives one.
Every path is run here: one k-tile (only the second form of the first k-tile), two, an odd count, five; a workgroup's first item
(not certified) and its later ones (certified: set-up + prologue between the items); the cross-item prefetch, which the plan takes
only with an even number (>= 4) of k-tiles and more items than the device has CUs -- so not on the 8-workgroup grid: a problem of
16 tile columns and enough tile rows, K = 256, asserted; split-K items of 2 and 1 k-tiles; problems of different K in one grouped
launch.

Operands are integers in [-4, 4]: every fp32 partial sum is an integer below 2^24, exact in any order, so the output must EQUAL
the fp64 product rounded once.  A stale accumulator shows as a wrong integer.  Per case: C pre-filled with sentinels (guards
intact afterwards), the launch under test issued right behind a launch of OTHER operands on the same grid, and a second launch
that must give the same bits.  Epilogues: plain and BIAS (the epilogues are not what changed)."""
import ctypes as C
import functools

import pytest
import torch

from cogview_amd import _lib
from tests import gemm_cells as GC

pytestmark = pytest.mark.gpu

LAYOUTS = (GC.NT, GC.NN, GC.TN)
DTYPES = (torch.float16, torch.bfloat16)
PARAMS = [(layout, dtype) for layout in LAYOUTS for dtype in DTYPES]
IDS = [f"{GC.LAYOUT_NAME[layout]}-{GC.DT_NAME[dtype]}" for layout, dtype in PARAMS]
GEN4 = GC.VARIANT[4]
CELLS = (GC.Cell(0), GC.Cell(GC.BIAS))


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X; run with -m 'not gpu' elsewhere"
    from cogview_amd import ops as _ops
    return _ops


@functools.lru_cache(maxsize=None)
def operands(M, N, K, seed):
    """CPU, fp64, shared and never written: A [M, K], B [N, K], bias [N] of integers in [-4, 4], and A B^T"""
    g = torch.Generator().manual_seed(7919 * seed + 1000003 * M + 1009 * N + K)
    rnd = lambda shape: torch.randint(-4, 5, shape, generator=g).double()
    a, b, bias = rnd((M, K)), rnd((N, K)), rnd((N,))
    return a, b, bias, a @ b.t()


def want_of(M, N, K, seed, cell, dtype):
    _, _, bias, dot = operands(M, N, K, seed)
    return (dot + bias if cell.flags & GC.BIAS else dot).to(dtype).cuda()


def stage(ops, M, N, K, layout, dtype, seed, splitk=1):
    a, b, bias, _ = operands(M, N, K, seed)
    return GC.Staged(ops, M, N, K, layout, dtype, a, b, bias, splitk)


def check_problem(ops, M, N, K, layout, dtype, splitk=1, wg8=False, xp=None):
    """one problem through cogv_gemm, kernel_variant 10 -> failures"""
    fails = []
    tag = f"M={M} N={N} K={K}" + (f" splitk={splitk}" if splitk > 1 else "") + (" 8 workgroups" if wg8 else "")
    with GC.eight_workgroups(ops, wg8):
        S, other = stage(ops, M, N, K, layout, dtype, 1, splitk), stage(ops, M, N, K, layout, dtype, 2, splitk)
        for cell in CELLS:
            d, d_other = S.desc(cell, GEN4), other.desc(cell, GEN4)
            rc, plan = _lib.gemm_plan(d)
            assert rc == _lib.OK and plan[0]["generation"] == 4 and plan[0]["splitk"] == splitk, (tag, rc, plan)
            if wg8:
                assert plan[0]["grid_x"] == 8 < plan[0]["items"], (tag, plan)
            if xp is not None:
                assert bool(plan[0]["xp_ok"]) == xp, (tag, plan)
            S.arm(cell)
            other.arm(cell)
            # the launch under test right behind a launch of other operands: same grid, same stream, nothing in between
            rcs = (_lib.lib().cogv_gemm(C.byref(d_other), ops._stream()), _lib.lib().cogv_gemm(C.byref(d), ops._stream()))
            torch.cuda.synchronize()
            assert rcs == (_lib.OK, _lib.OK), (tag, rcs)
            where = f"{tag} flags={GC.flags_name(cell.flags)}"
            for T, seed, name in ((S, 1, "second launch of the pair"), (other, 2, "first launch of the pair")):
                w = GC._wrong(T.C16.view, want_of(M, N, K, seed, cell, dtype))
                if w:
                    fails.append(f"{where} {name}: {w}")
                fails += [f"{where} {name}: {b}" for b in T.stray(cell)]
            first = [o.buf.clone() for o in S.outputs]
            S.arm(cell)
            if S.call(d) != _lib.OK or not all(torch.equal(o.buf, f) for o, f in zip(S.outputs, first)):
                fails.append(f"{where}: the second call gives other bits")
    return fails


@pytest.mark.parametrize("layout,dtype", PARAMS, ids=IDS)
def test_one_item(ops, layout, dtype):
    """one 256 x 256 item, never certified: 1, 2, 3 (odd tail) and 5 k-tiles"""
    fails = []
    for K in (64, 128, 192, 320):
        fails += check_problem(ops, 256, 256, K, layout, dtype)
    assert not fails, "\n".join(fails[:40])


@pytest.mark.parametrize("layout,dtype", PARAMS, ids=IDS)
def test_second_item(ops, layout, dtype):
    """3 x 3 tiles on 8 workgroups: a second item through the queue, certified by the set-up + prologue path (two, three and four
    k-tiles); M = 760: the same with one ragged edge"""
    fails = []
    for M in (768, 760):
        for K in (128, 192, 256):
            fails += check_problem(ops, M, 768, K, layout, dtype, wg8=True, xp=False)
    assert not fails, "\n".join(fails[:40])


@pytest.mark.parametrize("layout,dtype", PARAMS, ids=IDS)
def test_cross_item_prefetch(ops, layout, dtype):
    """more items than CUs, four k-tiles: the plan takes the cross-item prefetch (asserted), every workgroup that gets a second
    item starts it on k-tiles fetched inside the first one's loop; M - 8: ragged last tile row, the kernel refuses the prefetch
    for pairs with a tile of that row and takes it for the others"""
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    rows = cus // 16 + 1                                        # 16 x rows tiles > CUs
    fails = []
    for M in (256 * rows, 256 * rows - 8):
        fails += check_problem(ops, M, 4096, 256, layout, dtype, xp=True)
    assert not fails, "\n".join(fails[:40])


@pytest.mark.parametrize("layout,dtype", PARAMS, ids=IDS)
def test_split_k(ops, layout, dtype):
    """3 k-tiles split 2 + 1: alone (two workgroups, one item each) and 18 items chained on 8 workgroups"""
    fails = check_problem(ops, 256, 256, 192, layout, dtype, splitk=2)
    fails += check_problem(ops, 768, 768, 192, layout, dtype, splitk=2, wg8=True)
    assert not fails, "\n".join(fails[:40])


@pytest.mark.parametrize("layout,dtype", PARAMS, ids=IDS)
def test_grouped(ops, layout, dtype):
    """problems of different K in one launch on 8 workgroups, 2 x 2 tiles each: K = 128 then 64 (8 items), and K = 128, 64, 64,
    128 (16 items: workgroups 0-3 go from two k-tiles to one, workgroups 4-7 from one to two)"""
    fails = []
    with GC.eight_workgroups(ops):
        for Ks in ((128, 64), (128, 64, 64, 128)):
            sets = []
            for seed in (2, 1):                                  # the launch of seed 1 is the one behind other operands
                probs = [(stage(ops, 512, 512, K, layout, dtype, seed + 10 * i), CELLS[i & 1], K, seed + 10 * i) for i, K in enumerate(Ks)]
                for S, cell, _, _ in probs:
                    S.arm(cell)
                descs = (_lib.GemmDesc * len(probs))(*[S.desc(cell, 0) for S, cell, _, _ in probs])
                sets.append((probs, descs))
            rc, plan = _lib.gemm_plan(sets[0][1], len(Ks))
            assert rc == _lib.OK and all(p["generation"] == 4 and p["items"] == 4 * len(Ks) and p["grid_x"] == 8 for p in plan), (rc, plan)
            rcs = tuple(_lib.lib().cogv_gemm_grouped(descs, len(Ks), ops._stream()) for _, descs in sets)
            torch.cuda.synchronize()
            assert rcs == (_lib.OK, _lib.OK), rcs
            for probs, _ in sets:
                for i, (S, cell, K, seed) in enumerate(probs):
                    where = f"grouped K={Ks} problem {i} (seed {seed}) flags={GC.flags_name(cell.flags)}"
                    w = GC._wrong(S.C16.view, want_of(512, 512, K, seed, cell, dtype))
                    if w:
                        fails.append(f"{where}: {w}")
                    fails += [f"{where}: {b}" for b in S.stray(cell)]
            probs, descs = sets[1]
            first = [S.C16.buf.clone() for S, _, _, _ in probs]
            for S, cell, _, _ in probs:
                S.arm(cell)
            rc = _lib.lib().cogv_gemm_grouped(descs, len(Ks), ops._stream())
            torch.cuda.synchronize()
            if rc != _lib.OK or not all(torch.equal(S.C16.buf, f) for (S, _, _, _), f in zip(probs, first)):
                fails.append(f"grouped K={Ks}: the second call gives other bits")
    assert not fails, "\n".join(fails[:40])
