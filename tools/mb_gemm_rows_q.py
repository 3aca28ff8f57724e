"""The wide decode products of the 4B step, one launch at a time: ops.gemm_rows (16-bit weights), ops.gemm_rows_w8 (E4M3) and
ops.gemm_rows_w4 (MXFP4) on the five weight shapes of a layer and the logits, at the row counts given (default 12 24 32 64).

    python tools/mb_gemm_rows_q.py [rows ...]

Every (shape, rows) rotates through enough copies of the weight operand that a launch never finds its weights in the 256 MB
last-level cache (at least 640 MB in flight per format), the three formats are timed in turn, three times over, and the smallest
microseconds per launch are printed with the launch plan (row groups, waves per tile, column tiles, units in flight) and the
x bytes requested from L2 per weight byte.  For the A/B of a plan constant build a variant library (csrc/build.py: COGV_VARIANT,
COGV_HIPCC_EXTRA="-DGWQ_CT2_MIN_N=...") and select it with COGVIEW_HIP_LIB."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from cogview_amd import _lib, ops

SHAPES = (("qkv", 7680, 2560), ("out", 2560, 2560), ("h->4h", 10240, 2560), ("4h->h", 2560, 10240), ("logits", 58240, 2560))
ROWS = [int(a) for a in sys.argv[1:]] or [12, 24, 32, 64]
DT = torch.bfloat16
MIN_BYTES = 640 << 20


def _time(fn, operands, x, launches=40):
    n = len(operands)
    for i in range(n):
        fn(x, operands[i])
    best = float("inf")
    for rep in range(3):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for i in range(launches):
            fn(x, operands[i % n])
        stop.record()
        torch.cuda.synchronize()
        best = min(best, start.elapsed_time(stop) * 1e3 / launches)
    return best


def main():
    g = torch.Generator().manual_seed(0)
    print(f"library {_lib.LIB_PATH}", flush=True)
    for name, N, K in SHAPES:
        w = (torch.randn((N, K), generator=g) * 0.05).to(DT).cuda()
        q8, q4 = ops.quantize_rows_e4m3(w), ops.quantize_rows_mxfp4(w)
        copies = {"w16": [w.clone() for _ in range(-(-MIN_BYTES // (2 * N * K)))],
                  "e4m3": [tuple(t.clone() for t in q8) for _ in range(-(-MIN_BYTES // (N * K)))],
                  "mxfp4": [tuple(t.clone() for t in q4) for _ in range(-(-2 * MIN_BYTES // (N * K)))]}
        fns = {"w16": ops.gemm_rows, "e4m3": ops.gemm_rows_w8, "mxfp4": ops.gemm_rows_w4}
        plans = {"w16": _lib.gemm_rows_plan, "e4m3": _lib.gemm_rows_w8_plan, "mxfp4": _lib.gemm_rows_w4_plan}
        per_x = {"w16": 1, "e4m3": 2, "mxfp4": 4}                   # x bytes per weight byte at one row group and one column tile
        nbytes = {"w16": 2 * N * K, "e4m3": N * K + 4 * N, "mxfp4": N * K // 2 + N * K // 32}
        for M in ROWS:
            x = torch.randn((M, K), generator=g).to(DT).cuda()
            us = {f: [] for f in fns}
            for rep in range(3):
                for f in fns:
                    us[f].append(_time(fns[f], copies[f], x))
            line = f"{name:7s} N={N:5d} K={K:5d} M={M:2d}:"
            for f in fns:
                rc, pl = plans[f](_lib.BF16, M, N, K)
                t = min(us[f])
                line += (f"  {f} {t:6.1f} us {nbytes[f] / t / 1e6:5.2f} TB/s [rg {pl[0]} nwk {pl[1]} ct {pl[2]} depth {pl[9]} grid {pl[7]} "
                         f"x/w {per_x[f] * pl[0] / pl[2]:.1f}]")
            print(line, flush=True)
        del copies, w, q8, q4
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
