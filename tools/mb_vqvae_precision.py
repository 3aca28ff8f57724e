"""Images per second of the production tokenizer (vqvae.new_model(), 256 x 256 images) in its two precision modes, measured
against each other in one process: "fp32" (exact-fp32 MFMA convolutions, the default) and "bf16x3" (split-bf16 convolutions,
VQVAE.set_precision).  Per batch: a warm-up of both modes, then img2code and code2img_u8 with the two modes alternating, median
of --reps repetitions each (the protocol of tools/mb_vqvae_train.py); then one pass per mode with every launch bracketed by
events (ops.timed_launch) for the per-layer table and the conv family's total.

Each batch runs in a child process of its own under `timeout -k 10`; the driver itself never opens the GPU and stops at the
first child that fails.  Progress goes to stderr, one JSON line per batch to stdout.

    python tools/mb_vqvae_precision.py [--batches 32,256] [--reps 7] [--size 256] [--step-timeout 300]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MODES = ("fp32", "bf16x3")


def say(msg):
    print(msg, file=sys.stderr, flush=True)


def worker(batch, size, reps):
    import torch
    from cogview_amd import ops, vqvae
    assert torch.cuda.is_available(), "needs an MI355X: nothing here is measured on a CPU"

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    torch.manual_seed(0)
    model = vqvae.new_model().cuda().eval()
    g = torch.Generator("cuda").manual_seed(batch)
    img = torch.randn(batch, 3, size, size, device="cuda", generator=g)
    code = torch.randint(0, 8192, (batch, size // 8, size // 8), device="cuda", generator=g)
    work = {"img2code": lambda: vqvae.img2code(model, img), "code2img_u8": lambda: vqvae.code2img_u8(model, code)}
    res = {"batch": batch, "size": size, "reps": reps}
    for name, fn in work.items():
        for mode in MODES:                               # warm-up: code objects, packed weights and limb planes, allocator
            vqvae.set_precision(model, mode)
            t = [timed(fn) for _ in range(2)]
            say(f"batch {batch}: {name} {mode} warmed up ({t[0]:.2f} s, {t[1] * 1e3:.1f} ms)")
        times = {m: [] for m in MODES}
        for _ in range(reps):
            for mode in MODES:
                vqvae.set_precision(model, mode)
                times[mode].append(timed(fn))
        res[name] = {}
        for mode, ts in times.items():
            med = sorted(ts)[len(ts) // 2]
            res[name][mode] = {"images_per_s_median": round(batch / med, 1), "ms_median": round(med * 1e3, 2),
                               "ms_all": [round(t * 1e3, 2) for t in ts]}
        res[name]["bf16x3_over_fp32"] = round(res[name]["bf16x3"]["images_per_s_median"] / res[name]["fp32"]["images_per_s_median"], 3)
        layers = {}
        for mode in MODES:
            vqvae.set_precision(model, mode)
            ops.enable_gemm_timing()
            fn()
            stats = ops.collect_gemm_timing()
            layers[mode] = {"by_layer": {k: {"ms": round(v["avg_ms"] * v["launches"], 3), "tflops": v["tflops"]} for k, v in stats["by_shape"].items()},
                            "by_family_ms": {k: round(v["total_ms"], 3) for k, v in stats["by_variant"].items()},
                            "conv_tflops": round(stats["by_variant"]["conv"]["tflops"], 1) if "conv" in stats["by_variant"] else None,
                            "kernel_ms_total": round(stats["total_ms"], 3)}
        res[name]["timed_launch"] = layers
        fam = [layers[m]["by_family_ms"].get("conv") for m in MODES]
        if all(fam):
            res[name]["conv_family_fp32_over_bf16x3_time"] = round(fam[0] / fam[1], 3)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="32,256")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds per batch (its own `timeout -k 10`)")
    ap.add_argument("--worker", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker, args.size, args.reps)
    for b in [int(x) for x in args.batches.split(",")]:
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--worker", str(b),
               "--reps", str(args.reps), "--size", str(args.size)]
        rc = subprocess.run(cmd, cwd=ROOT).returncode
        if rc != 0:
            say(f"batch {b}: exit status {rc}; nothing more is started on the GPU")
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
