"""bench.py launch contract (round-2 verdict, missing #2): `python bench.py --gpus N` with no launcher around it must
spawn its own N ranks (the reference's launcher does: scripts/pretrain_single_node.sh:49) and print ONE JSON line with
n_gpus = N; the `torch.distributed.run ... bench.py --gpus N` form keeps working."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_becomes_its_own_launcher(monkeypatch):
    """CPU: without WORLD_SIZE, --gpus 4 re-execs under torch.distributed.run with one rank per GPU on 127.0.0.1 and
    hands its own arguments through; with WORLD_SIZE set (a launcher is already there) it does not."""
    sys.path.insert(0, ROOT)
    import bench
    calls = []

    class Stop(Exception):
        pass

    def fake_execv(exe, argv):
        calls.append((exe, list(argv)))
        raise Stop()
    monkeypatch.setattr(os, "execv", fake_execv)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "7", "--warmup", "2"])
    args = type("A", (), {"gpus": 4})()
    with pytest.raises(Stop):
        bench.setup_dist(args)
    exe, argv = calls[0]
    assert exe == sys.executable and argv[1:3] == ["-m", "torch.distributed.run"]
    assert "--nproc-per-node=4" in argv and "--nnodes=1" in argv
    assert argv[argv.index("--master-addr") + 1] == "127.0.0.1" and int(argv[argv.index("--master-port") + 1]) > 0
    i = argv.index(os.path.join(ROOT, "bench.py"))
    assert argv[i + 1:] == ["--gpus", "4", "--steps", "7", "--warmup", "2"]
    # a launcher is already around the script: no re-exec (the world-size check is what runs next)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(AssertionError, match="WORLD_SIZE=2"):
        bench.setup_dist(args)
    assert len(calls) == 1


@pytest.mark.gpu
def test_bench_gpus_2_spawns_two_ranks_and_prints_one_line():
    """GPU box (one GPU): `python bench.py --gpus 2` end to end -- both spawned ranks share cuda:0 and exchange gradients
    over gloo (COGV_BENCH_ONE_DEVICE=1, development switch; RCCL refuses two ranks on one device), the 336M model at a
    tiny batch.  One JSON line, n_gpus 2, whole-job throughput."""
    env = dict(os.environ, COGV_BENCH_ONE_DEVICE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--config", "cogview-small-336M",
                        "--batch", "2", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--dtype", "bf16"],
                       capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 2 and out["warmup"] == 1 and out["scaling"] == "weak"
    assert out["config"]["global_batch"] == 4 and out["config"]["parallelism"] == "dp2"
    assert out["value"] > 0 and abs(out["value"] - 4 * 1088 / (out["ms_per_step"] / 1e3)) < 1e-6 * out["value"]


@pytest.mark.gpu
def test_bench_model_parallel_2_on_one_device():
    """GPU box (one GPU): `python bench.py --gpus 2 --model-parallel 2` end to end (BASELINE configs[2] in miniature) -- the two
    model-parallel ranks share cuda:0 and exchange over gloo (COGV_BENCH_ONE_DEVICE=1), the 336M model at a tiny batch: the
    row-parallel Linears run in row chunks with their all-reduces started behind each chunk (2176 rows = 9 tiles = 4 chunks).
    One JSON line, n_gpus 2, data-parallel size 1."""
    env = dict(os.environ, COGV_BENCH_ONE_DEVICE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--model-parallel", "2",
                        "--config", "cogview-small-336M", "--batch", "2", "--steps", "2", "--warmup", "1",
                        "--no-cpu-baseline", "--dtype", "fp16"],
                       capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 2 and out["config"]["global_batch"] == 2
    assert out["config"]["parallelism"].startswith("mp2") or "mp2" in out["config"]["parallelism"], out["config"]["parallelism"]
    assert out["value"] > 0 and out["config"]["skipped_last_step"] in (0, 1)


def test_dump_helpers_write_fixed_samples_within_the_limit(tmp_path, monkeypatch):
    """CPU: --dump-outputs' sample is the same on every call (seeded positions), small tensors are kept whole, integer and
    float64 data are written as float64 and everything else as float32, and the 64 MB budget is enforced."""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    t = torch.randn(100000).half()
    a, b = bench.seeded_sample(t, 512, 7), bench.seeded_sample(t, 512, 7)
    assert a.dtype == torch.float32 and a.shape == (512,) and torch.equal(a, b)
    assert not torch.equal(a, bench.seeded_sample(t, 512, 8))
    assert torch.equal(bench.seeded_sample(t[:100], 512, 7), t[:100].float())
    bench.write_dump(str(tmp_path / "d"), {"loss": torch.tensor(2.5, dtype=torch.float64), "ids": torch.arange(6).view(2, 3),
                                           "sample": a})
    got = {n: np.load(str(tmp_path / "d" / (n + ".npy"))) for n in ("loss", "ids", "sample")}
    assert got["loss"].dtype == np.float64 and got["loss"] == 2.5
    assert got["ids"].dtype == np.float64 and got["ids"].tolist() == [[0, 1, 2], [3, 4, 5]]
    assert got["sample"].dtype == np.float32 and np.array_equal(got["sample"], a.numpy())
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1000)
    with pytest.raises(AssertionError, match="limit"):
        bench.write_dump(str(tmp_path / "e"), {"big": torch.zeros(1000)})
    assert not (tmp_path / "e").exists()


@pytest.mark.gpu
def test_bench_dump_outputs_writes_the_last_timed_step(tmp_path):
    """GPU box: `bench.py --dump-outputs DIR` on configs[0] writes the loss the JSON line reports, the skip flag and the
    parameter sample for each dtype leg, float32 / float64, within 64 MB."""
    import numpy as np
    out_dir = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "cogview-tiny-18M", "--steps", "3",
                        "--warmup", "1", "--no-cpu-baseline", "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert out["steps"] == 3
    files = sorted(p.name for p in out_dir.iterdir())
    assert files == sorted(f"{d}_{n}.npy" for d in ("fp16", "bf16") for n in ("loss", "skipped", "params_sample"))
    arrs = {f[:-4]: np.load(str(out_dir / f)) for f in files}
    assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
    assert float(arrs["fp16_loss"]) == out["config"]["loss"] and float(arrs["bf16_loss"]) == out["bf16_leg"]["loss"]
    assert arrs["fp16_params_sample"].shape == arrs["bf16_params_sample"].shape and np.isfinite(arrs["fp16_params_sample"]).all()


@pytest.mark.gpu
def test_bench_plain_run_is_the_headline_of_the_full_run(tmp_path):
    """GPU box: a plain run carries only what its headline needs.  On configs[0] its line has no bf16 leg, no CPU baseline
    and no measured logits error, all of which the `--full` line has; given --dump-outputs it writes the same arrays as the
    `--full` run, bit for bit (both dtype legs)."""
    import numpy as np
    runs = {}
    for name, extra in (("plain", []), ("plain_dump", ["--dump-outputs", str(tmp_path / "plain_dump")]),
                        ("full_dump", ["--full", "--dump-outputs", str(tmp_path / "full_dump")])):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--config", "cogview-tiny-18M", "--steps", "3",
                            "--warmup", "1"] + extra, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        out_dir = tmp_path / name
        runs[name] = json.loads(lines[0]), ({p.name[:-4]: np.load(str(p)) for p in out_dir.iterdir()} if out_dir.exists() else None)
    plain, full = runs["plain"][0], runs["full_dump"][0]
    plain_arrs, full_arrs = runs["plain_dump"][1], runs["full_dump"][1]
    assert runs["plain"][1] is None
    assert sorted(plain_arrs) == sorted(full_arrs) == sorted(f"{d}_{n}" for d in ("fp16", "bf16") for n in ("loss", "skipped", "params_sample"))
    assert all(np.array_equal(a, full_arrs[k]) for k, a in plain_arrs.items())
    assert plain["dtype"] == full["dtype"] == "fp16" and plain["steps"] == full["steps"] == 3
    assert plain["config"]["loss"] == full["config"]["loss"] == float(plain_arrs["fp16_loss"])
    assert "bf16_leg" not in plain and "cpu_baseline" not in plain and "cpu_baseline_reference" not in plain
    assert plain["config"]["logits_rel_l2_vs_fp32_reference"]["measured"] is None
    assert runs["plain_dump"][0]["config"]["logits_rel_l2_vs_fp32_reference"]["measured"] is None
    assert full["bf16_leg"]["dtype"] == "bf16" and full["cpu_baseline"]["value"] > 0
    assert full["config"]["logits_rel_l2_vs_fp32_reference"]["measured"] < full["config"]["logits_rel_l2_vs_fp32_reference"]["tolerance_in_tests"]
