"""bench.py's launch contract (CPU, gloo): `python bench.py --gpus N` WITHOUT a launcher starts the N ranks itself and proves
they met (world_size_seen from an all-reduce), the launcher form `python -m torch.distributed.run ... bench.py --gpus N` works
the same, a WORLD_SIZE that disagrees with --gpus is an error, and the N = 1 line keeps its shape.  --dry-run swaps the model
for a no-op (there is no CPU path for the model) but runs the real launch / rendezvous / weight-broadcast / barrier / timing-
reduction code; its `value` is null so it can never be mistaken for a measurement."""
import json
import os
import socket
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env():
    e = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    e["OMP_NUM_THREADS"] = "2"
    return e


def _last_json(out):
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert lines, out[-2000:]
    return json.loads(lines[-1])


def test_self_spawn_two_ranks_over_gloo():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "2", "--warmup", "1", "--dry-run", "--full"], env=_env(), cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0, out[-3000:]
    line = _last_json(out)
    assert line["n_gpus"] == 2 and line["world_size_seen"] == 2 and line["backend"] == "gloo"
    assert line["dry_run"] is True and line["value"] is None          # plumbing only: never a measurement
    assert len(line["per_rank_fps"]) == 2 and all(v > 0 for v in line["per_rank_fps"])
    assert line["rccl_bcast_ms"] > 0 and line["bcast_bytes"] > 1e6      # the weight blob really crossed the process boundary
    assert line["steps"] == 2 and line["scaling"] == "weak"
    assert sum(1 for l in out.splitlines() if l.startswith("{")) == 1    # ONE line, from rank 0
    # the N-rank line verifies itself: every rank contributed a digest (dry run: of the broadcast weight bytes), MIN == MAX
    assert line["rank_check"]["ranks_agree"] is True and "FAILED" not in line["rank_check"]
    assert len(line["init_s_per_rank"]) == 2 and all(v > 0 for v in line["init_s_per_rank"])


def test_a_rank_with_different_weights_fails_the_run():
    """--perturb-rank (TEST ONLY) makes rank 1 hold a slightly different weight tensor after the broadcast: the line must carry
    ranks_agree false and EVERY rank must exit non-zero -- an 8-GPU scaling run cannot pass with one rank computing something else."""
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "2", "--warmup", "1", "--dry-run", "--full", "--perturb-rank", "1"],
                       env=_env(), cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode(errors="replace")
    assert r.returncode != 0, out[-2000:]
    line = _last_json(out)
    assert line["rank_check"]["ranks_agree"] is False and line["rank_check"]["FAILED"] is True


def test_launcher_form_and_world_size_mismatch():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    base = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
            "--master-port", str(port), BENCH]
    r = subprocess.run(base + ["--gpus", "2", "--steps", "2", "--warmup", "1", "--dry-run"], env=_env(), cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    assert _last_json(r.stdout.decode(errors="replace"))["world_size_seen"] == 2
    # the driver's launcher started 2 ranks but the flag says 4: refuse, do not print a line under the wrong label
    r = subprocess.run(base + ["--gpus", "4", "--steps", "2", "--warmup", "1", "--dry-run"], env=_env(), cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode(errors="replace")
    assert r.returncode != 0 and not [l for l in out.splitlines() if l.startswith("{")], out[-2000:]


def test_single_rank_line_and_no_gpu_refusal():
    r = subprocess.run([sys.executable, BENCH, "--steps", "3", "--warmup", "1", "--dry-run"], env=_env(), cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode(errors="replace")[-3000:]
    line = _last_json(r.stdout.decode(errors="replace"))
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "world_size_seen"):
        assert k in line, k
    assert line["n_gpus"] == 1 and line["world_size_seen"] == 1 and line["rccl_bcast_ms"] == 0.0
    # without --dry-run there is no CPU path: --gpus 2 on a box without 2 GPUs must exit non-zero instead of running one rank
    import torch
    if not torch.cuda.is_available() or torch.cuda.device_count() < 2:
        r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "2"], env=_env(), cwd=ROOT,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        out = r.stdout.decode(errors="replace")
        assert r.returncode != 0 and "refusing" in out and not [l for l in out.splitlines() if l.startswith("{")]


def test_eight_ranks_the_size_of_the_scaling_run():
    """the first time this code meets 8 ranks must not be the driver's RCCL run.  The same dry run at world_size 8
    (the line carries every rank's CPU placement and host launch cost), and a perturbed LAST rank must fail all eight."""
    r = subprocess.run([sys.executable, BENCH, "--gpus", "8", "--steps", "2", "--warmup", "1", "--dry-run", "--full"], env=_env(), cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0, out[-3000:]
    line = _last_json(out)
    assert line["n_gpus"] == 8 and line["world_size_seen"] == 8 and line["backend"] == "gloo"
    assert len(line["per_rank_fps"]) == 8 and len(line["init_s_per_rank"]) == 8
    assert len(line["host_launch_us_per_frame"]) == 8 and all(v >= 0 for v in line["host_launch_us_per_frame"])
    assert isinstance(line["cpu_affinity"], list) and len(line["cpu_affinity"]) == 8 and all("cpus" in s for s in line["cpu_affinity"])
    assert line["omp_num_threads"] >= 1
    assert line["rank_check"]["ranks_agree"] is True
    assert sum(1 for l in out.splitlines() if l.startswith("{")) == 1
    r = subprocess.run([sys.executable, BENCH, "--gpus", "8", "--steps", "2", "--warmup", "1", "--dry-run", "--full", "--perturb-rank", "7"],
                       env=_env(), cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    out = r.stdout.decode(errors="replace")
    assert r.returncode != 0, out[-2000:]
    assert _last_json(out)["rank_check"]["ranks_agree"] is False


def test_eight_rank_dry_run_line_schema():
    """The WHOLE `bench.py --gpus 8` self-spawn path (launcher, rendezvous, pinning plan, weight broadcast, the solo reference run of rank 0, the
    8-rank timed loop, reductions, rank check) over gloo on the CPU, and the schema of the line the driver's scaling run will read: the
    collective block (backend, bytes, GB/s, hardware queues per rank), per-rank frames/s with min / max / spread, and the scaling check."""
    r = subprocess.run([sys.executable, BENCH, "--gpus", "8", "--steps", "2", "--warmup", "1", "--dry-run", "--full"], env=_env(), cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0, out[-3000:]
    line = _last_json(out)
    assert line["n_gpus"] == 8 and line["world_size_seen"] == 8 and line["dry_run"] is True and line["value"] is None
    assert len(line["per_rank_fps"]) == 8 and len(line["init_s_per_rank"]) == 8 and len(line["host_launch_us_per_frame"]) == 8
    lo, hi, spread = line["per_rank_fps_min_max_spread"]
    assert lo == min(line["per_rank_fps"]) and hi == max(line["per_rank_fps"]) and 0.0 <= spread < 1.0
    c = line["collective"]
    assert c["backend"] == "gloo" and c["bcast_bytes"] == line["bcast_bytes"] > 1e6 and c["bcast_ms"] > 0 and c["bcast_GBps"] > 0
    assert len(c["hw_queues_per_rank"]) == 8 and all("GPU_MAX_HW_QUEUES" in q for q in c["hw_queues_per_rank"])
    sc = line["scaling_check"]
    assert set(sc) >= {"solo_fps_rank0", "per_gpu_fps", "scaling_efficiency", "what"} and sc["scaling_efficiency"] is None   # dry run: never a number
    assert line["rank_check"]["ranks_agree"] is True
    assert line["warmup"] >= line["warmup_requested"] == 1
    assert isinstance(line["cpu_affinity"], list) and len(line["cpu_affinity"]) == 8


def test_plain_run_times_the_steps_and_nothing_else():
    """Without --full the line is the headline alone: the K timed steps and the fields that describe them.  The N-rank checks (solo
    run, rank digests), the host launch frames and everything else beside the headline come only with --full (tests above)."""
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "3", "--warmup", "1", "--dry-run"], env=_env(), cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0, out[-3000:]
    line = _last_json(out)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "world_size_seen"):
        assert k in line, k
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["world_size_seen"] == 2
    for k in ("rank_check", "scaling_check", "sustained", "roofline", "cpu_baseline", "parity", "other_configs", "hipgraph"):
        assert k not in line, k
    assert line["host_launch_us_per_frame"] is None                  # not measured: no frames beyond warm-up and the K steps


def test_dump_outputs_writes_float32_files_within_budget(tmp_path, monkeypatch):
    """--dump-outputs (bench.dump_outputs): one .npy per returned array, float32, whole when it fits the budget, else the documented
    seeded stride sample -- the same elements in every run -- and never more than the budget over all files."""
    import numpy as np
    import torch
    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET_ELEMS", 1000)
    g = torch.Generator().manual_seed(0)
    small = torch.randn(1, 19, 3, 5, generator=g)
    files = bench.dump_outputs([small], str(tmp_path / "a"), 0, 1, torch, np)
    assert list(files) == ["logits.npy"]
    a = np.load(str(tmp_path / "a" / "logits.npy"))
    assert a.dtype == np.float32 and a.shape == (1, 19, 3, 5) and np.array_equal(a, small.numpy())
    big = [torch.randn(1, 19, 33, 65, generator=g) for _ in range(2)]
    for d in ("b", "c"):
        files = bench.dump_outputs(big, str(tmp_path / d), 0, 1, torch, np)
        assert sorted(files) == ["logits_0_sample.npy", "logits_1_sample.npy"]
    total = 0
    for i, o in enumerate(big):
        b = np.load(str(tmp_path / "b" / ("logits_%d_sample.npy" % i)))
        c = np.load(str(tmp_path / "c" / ("logits_%d_sample.npy" % i)))
        assert b.dtype == np.float32 and np.array_equal(b, c)
        n = o.numel()
        stride = -(-n // 500)
        k = n // stride
        idx = np.arange(k) * stride + np.random.default_rng([k, n]).integers(0, stride, k)
        assert np.array_equal(b, o.reshape(-1).numpy()[idx])
        total += b.size
    assert total <= 1000
    files = bench.dump_outputs([small], str(tmp_path / "r"), 1, 2, torch, np)   # N ranks: every rank its own file
    assert list(files) == ["rank1_logits.npy"]
