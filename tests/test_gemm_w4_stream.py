"""CPU: the instruction stream around the MFMAs of the generation-4 GEMM kernel (csrc/gemm_gen4.cuh), counted in the device
assembly of units 4, 5 and 6 (fp16 NT, NN, TN) compiled with csrc/build.py's own flags.  The k-loop is hand scheduled; what
the schedule needs per two k-tiles is the 256 MFMAs, the fragment reads, 32 LDS-DMA pieces each with its M0 write, 4 barriers,
one landing wait per quarter-step, one DMA certificate per half-step and a handful of loop instructions.  What this file refuses
is what crept in beside that before: a clearing pass over the accumulators, one landing wait per fragment, a temporary plus a
move for every M0, and a multiplication by the k-tile index for every DMA source.

A basic block here is a run of instructions between labels and instructions that name a label."""
import concurrent.futures
import os
import re
import subprocess
import tempfile

import pytest

UNITS = {4: "NT", 5: "NN", 6: "TN"}
# the two-k-tile loop block (256 MFMAs): instructions in it at the commit before this file, and now
PARENT_TOTAL = {"NT": 527, "TN": 613}
ACHIEVED_TOTAL = {"NT": 450, "NN": 482, "TN": 514}
# MFMAs, LDS fragment reads, LDS-DMA pieces of that block: what the commit before had (a natural fragment is one 128-bit read,
# a transposed one two 64-bit reads; NN has one operand of each kind)
LOOP_COUNTS = {"NT": (256, 64, 32), "NN": (256, 96, 32), "TN": (256, 128, 32)}


def _compile(unit, out):
    from cogview_amd.csrc import build as B
    src = os.path.join(B.HERE, "gemm.hip")
    r = subprocess.run([B._hipcc()] + B.FLAGS + [f"-DCOGV_W4_TU={unit}", "--cuda-device-only", "-S", src, "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return open(out).read().splitlines()


@pytest.fixture(scope="module")
def asm():
    """{layout name: device assembly lines of its fp16 unit}, compiled once, the three units side by side"""
    with tempfile.TemporaryDirectory() as td:
        with concurrent.futures.ThreadPoolExecutor(max_workers=min(16, len(UNITS))) as ex:
            futs = {name: ex.submit(_compile, unit, os.path.join(td, f"w4_{unit}.s")) for unit, name in UNITS.items()}
            return {name: f.result() for name, f in futs.items()}


def kernel_blocks(lines):
    """[(label, [instruction text])] of gemm_w4_kernel, in layout order"""
    blocks, cur, label, inside = [], [], None, False
    for ln in lines:
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            inside, label, cur = "gemm_w4_kernel" in m.group(1), m.group(1), []
            continue
        if not inside:
            continue
        t = ln.split(";")[0].strip()
        if ln.startswith(".Lfunc_end"):
            blocks.append((label, cur))
            inside = False
            continue
        m = re.match(r"^(\.LBB\d+_\d+):", ln)
        if m:
            blocks.append((label, cur))
            label, cur = m.group(1), []
            continue
        if not t or t.startswith(".") or t.endswith(":"):
            continue
        cur.append(t)
        if re.search(r"\s\.LBB\d+_\d+$", t):                   # names a label: the block ends here
            blocks.append((label, cur))
            label, cur = label + "+", []
    return [(lb, ins) for lb, ins in blocks if ins]


def op(t):
    return t.split()[0]


def count(ins, prefix):
    return sum(1 for t in ins if op(t).startswith(prefix))


def waits(ins, counter):
    return [t for t in ins if op(t) == "s_waitcnt" and counter in t]


def heavy(blocks):
    return [(lb, ins) for lb, ins in blocks if count(ins, "v_mfma") >= 64]


def loop_block(blocks):
    """the block that ends by naming its own label with 256 MFMAs in it: two k-tiles"""
    found = [(lb, ins) for lb, ins in blocks if ins[-1].endswith(" " + lb) and count(ins, "v_mfma") == 256]
    assert len(found) == 1, [(lb, len(ins), count(ins, "v_mfma")) for lb, ins in blocks if count(ins, "v_mfma")]
    return found[0][1]


@pytest.mark.parametrize("name", list(UNITS.values()))
def test_no_accumulator_clear(asm, name):
    blocks = kernel_blocks(asm[name])
    assert blocks and len(heavy(blocks)) >= 4
    n = sum(count(ins, "v_accvgpr_write_b32") for _, ins in blocks)
    assert n == 0, f"{name}: {n} v_accvgpr_write_b32 in gemm_w4_kernel"


@pytest.mark.parametrize("name", list(UNITS.values()))
def test_blocks_around_the_mfmas(asm, name):
    for lb, ins in heavy(kernel_blocks(asm[name])):
        mfma, dma = count(ins, "v_mfma"), count(ins, "global_load_lds")
        where = f"{name} block {lb} ({len(ins)} instructions, {mfma} MFMAs)"
        assert count(ins, "s_mul_i32") == 0 and count(ins, "s_mul_hi_u32") == 0, where
        # one landing per quarter-step (32 MFMAs); one DMA certificate per half-step (64 MFMAs), always vmcnt(16)
        lg, vm = waits(ins, "lgkmcnt"), waits(ins, "vmcnt")
        assert len(lg) * 32 <= mfma, (where, len(lg))
        assert len(vm) * 64 <= mfma and all("vmcnt(16)" in t for t in vm), (where, vm)
        # M0: never more moves than DMA pieces, and none fed by an add that serves nothing else
        moves = [i for i, t in enumerate(ins) if re.match(r"s_mov_b32 m0,", t)]
        assert len(moves) <= dma, (where, len(moves), dma)
        for i in moves:
            src = ins[i].split(",")[1].strip()
            defs = [j for j in range(i) if re.match(r"\S+ " + re.escape(src) + r",", ins[j])]
            if not defs or op(ins[defs[-1]]) != "s_add_i32":
                continue
            j = defs[-1]
            nxt = [k for k in range(i + 1, len(ins)) if re.match(r"\S+ " + re.escape(src) + r",", ins[k])]
            end = nxt[0] if nxt else len(ins)
            uses = [k for k in range(j + 1, end) if k != i and re.search(r"[ ,\[]" + re.escape(src) + r"\b", ins[k].split(" ", 1)[1])]
            assert uses, f"{where}: '{ins[j]}' only feeds '{ins[i]}'"


@pytest.mark.parametrize("name", list(UNITS.values()))
def test_two_k_tile_loop(asm, name):
    ins = loop_block(kernel_blocks(asm[name]))
    got = (count(ins, "v_mfma"), count(ins, "ds_read"), count(ins, "global_load_lds"))
    print(f"{name}: {len(ins)} instructions per 256 MFMAs ({len(ins) / 256:.2f} per MFMA), MFMA / LDS reads / DMA = {got}")
    assert got == LOOP_COUNTS[name]
    assert len(ins) <= ACHIEVED_TOTAL[name], (name, len(ins))
    if name in PARENT_TOTAL:
        assert ACHIEVED_TOTAL[name] < PARENT_TOTAL[name]


@pytest.mark.parametrize("name", list(UNITS.values()))
def test_no_register_read_before_its_wait(asm, name):
    from cogview_amd.csrc.build import scan_asm_hazards
    assert scan_asm_hazards(asm[name]) == []
