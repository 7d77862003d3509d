"""bench.py driver contract (task spec): one JSON line from rank 0 with the
required keys, run here under torchrun with two gloo ranks on CPU."""

import json
import os
import socket
import subprocess
import sys

from .helpers import ROOT

REQUIRED = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config"}


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(args, nproc=None, rc=0, env=None):
    cmd = [sys.executable]
    if nproc:
        cmd += ["-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr",
                "127.0.0.1", "--master-port", str(_port())]
    cmd += [os.path.join(ROOT, "bench.py"), *args]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT,
                       env=dict(os.environ, OMP_NUM_THREADS="1", **(env or {})))
    if rc:  # torchrun reports a failed rank as 1 whatever the rank's own code
        assert r.returncode != 0, r.stdout[-2000:]
        return r
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_bench_contract_two_ranks_cpu():
    rec = _run(["--gpus", "2", "--device", "cpu", "--size", "96", "--steps", "3", "--warmup", "1", "--full"], nproc=2)
    assert REQUIRED <= set(rec)
    assert rec["n_gpus"] == 2 and rec["steps"] == 3 and rec["warmup"] == 1 and rec["scaling"] == "weak"
    assert rec["higher_is_better"] is True and rec["value"] > 0 and rec["verified_bit_exact"] is True
    assert rec["metric"] == json.load(open(os.path.join(ROOT, "BASELINE.json")))["metric"]
    assert rec["config"]["parallelism"].startswith("slab2")
    # value is the whole-job aggregate: N * size^2 * steps / time
    assert abs(rec["value"] - 2 * 96 * 96 / (rec["ms_per_step"] * 1e-3) / 1e9) < 1e-3 * max(1.0, rec["value"])
    # streaming run: measured and verified N-rank == one device
    assert rec["value_streaming"] > 0 and rec["verified_bit_exact_streaming"] is True
    assert rec["verified_pixels_streaming"] == 6 * 2 * 96 * 96
    assert abs(rec["value_streaming"] - 2 * 96 * 96 / (rec["ms_per_step_streaming"] * 1e-3) / 1e9) \
        < 1e-3 * max(1.0, rec["value_streaming"])


def test_bench_json_carries_no_hard_coded_ratio():
    """every ratio in the JSON is computed in the run (no
    literal same-method ratio), and vs_baseline says what it compares."""
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert "vs_reference_same_method" not in src and "SAME_METHOD" not in src
    rec = _run(["--device", "cpu", "--size", "64", "--steps", "2", "--warmup", "1", "--rotate", "2", "--no-stream"])
    assert "vs_reference_same_method" not in rec and "value_streaming" not in rec
    assert "estimate" in rec["vs_baseline_note"]
    assert abs(rec["vs_baseline"] - rec["value"] / 4.4) < 0.01 + 1e-3 * rec["vs_baseline"]


def test_bench_measurement_hygiene_fields_cpu():
    """the CPU baseline is a median of >= 5 runs (min too), the
    published-methodology serial -O0 time rides along, and the time-based
    warm-up reports what it ran (the driver's "warmup" field stays W)."""
    rec = _run(["--device", "cpu", "--size", "64", "--steps", "2", "--warmup", "1", "--rotate", "2", "--no-stream",
                "--warmup-ms", "5", "--full"])
    assert rec["warmup"] == 1 and rec["warmup_ms"] >= 5.0 and rec["warmup_steps_run"] >= 2
    # the sustained-load rate rides along (same K steps after >= sustain_ms of load)
    assert rec["value_sustained"] > 0 and rec["sustain_ms"] == 50.0
    assert abs(rec["value_sustained"] - 64 * 64 / (rec["ms_per_step_sustained"] * 1e-3) / 1e9) \
        < 1e-3 * max(1.0, rec["value_sustained"])
    # steady state (VERDICT r5 Next #4): K-step windows after >= 300 ms of load,
    # with a clock record per rank (None on the CPU)
    assert rec["value_steady"] > 0 and len(rec["value_steady_windows"]) == 5 and rec["steady_ms"] == 300.0
    assert rec["steady_clocks"] == [None]
    assert rec["cpu_runs"] >= 5 and 0 < rec["cpu_ms_per_image_min"] <= rec["cpu_ms_per_image"]
    # the host's enqueue time of the timed steps rides along, never above the step time
    assert 0 < rec["host_enqueue_ms_per_step"] <= rec["ms_per_step"]
    assert rec["config"]["host_wait"] is None  # CPU: no HIP wait policy
    assert abs(rec["speedup_vs_cpu"] - rec["cpu_ms_per_image"] / rec["gpu_ms_per_image"]) \
        < 0.051 + 1e-3 * rec["speedup_vs_cpu"]
    if os.path.exists(os.path.join(ROOT, "labs", "lab2", "src", "cpu_exe")):
        assert rec["cpu_serial_o0_ms_per_image"] > 0
        assert abs(rec["speedup_vs_cpu_serial_o0"] - rec["cpu_serial_o0_ms_per_image"] / rec["gpu_ms_per_image"]) \
            < 0.051 + 1e-3 * rec["speedup_vs_cpu_serial_o0"]
    rec0 = _run(["--device", "cpu", "--size", "64", "--steps", "2", "--warmup", "1", "--rotate", "2", "--no-stream",
                 "--warmup-ms", "0", "--no-warm"])
    assert rec0["warmup_ms"] == 0 and rec0["warmup_steps_run"] == 0


def test_bench_contract_single_process_cpu():
    rec = _run(["--device", "cpu", "--size", "64", "--steps", "2", "--warmup", "1", "--overlap", "pipeline"])
    assert REQUIRED <= set(rec) and rec["n_gpus"] == 1


MOVED_BEHIND_FULL = {"value_sustained", "value_steady", "value_warm_cache", "value_warm_cache_1stream",
                     "value_streaming", "cpu_ms_per_image", "speedup_vs_cpu", "clocks", "steady_clocks"}


def test_bench_plain_run_measures_the_headline_only():
    """A plain run (no --full) sets up, warms up, times the K steps and prints
    the result line: none of the secondary measurements, no comparison with
    the CPU reference (verified_bit_exact null), whatever their own options
    say; --full brings them back."""
    args = ["--device", "cpu", "--size", "64", "--steps", "4", "--warmup", "1", "--rotate", "2", "--clocks", "50"]
    rec = _run(args)
    assert REQUIRED <= set(rec) and rec["full"] is False and rec["status"] == "ok"
    assert not MOVED_BEHIND_FULL & set(rec), MOVED_BEHIND_FULL & set(rec)
    assert rec["verified_bit_exact"] is None and rec["verified_pixels"] == 0
    assert rec["steps"] == 4 and rec["ms_per_step"] > 0 and rec["dtype"] == "fp32" and rec["unit"] == "Gpixel/s"
    assert abs(rec["ms_per_step"] * 4 - rec["job_span_ms"]) <= 1e-3 * rec["job_span_ms"] + 1e-4
    full = _run(args + ["--full"])
    assert full["full"] is True and full["verified_bit_exact"] is True and full["verified_pixels"] == 2 * 64 * 64
    # (on the CPU: no clock sampler, and one stream, whose cache-resident rate is value_warm_cache)
    assert MOVED_BEHIND_FULL - {"clocks", "steady_clocks", "value_warm_cache_1stream"} <= set(full)


def test_bench_dump_outputs_cpu(tmp_path):
    """--dump-outputs: the last timed step's output slab as float32, the same
    from run to run (seeded inputs), and equal to the CPU reference on the
    regenerated input of the pair that step used."""
    import numpy as np
    import torch

    import bench
    from cuda_mpi_openmp_amd import ops

    args = ["--device", "cpu", "--size", "67", "--steps", "4", "--warmup", "1", "--rotate", "3"]
    a, b = tmp_path / "a", tmp_path / "b"
    _run(args + ["--dump-outputs", str(a)])
    _run(args + ["--dump-outputs", str(b), "--full"])
    assert sorted(os.listdir(a)) == sorted(os.listdir(b)) == ["out_rank0.npy", "rows_rank0.npy"]
    out, rows = np.load(a / "out_rank0.npy"), np.load(a / "rows_rank0.npy")
    assert out.dtype == np.float32 and out.shape == (67, 67, 4) and rows.dtype == np.float64
    assert np.array_equal(rows, np.arange(67)) and np.array_equal(out, np.load(b / "out_rank0.npy"))
    img = bench.regen_slab(1234 + 7919 * ((4 - 1) % 3), 67, 67, torch.device("cpu"))  # the last step's pair
    assert np.array_equal(out, ops.conv(img, "sobel5").numpy().astype(np.float32))


def test_bench_dump_outputs_samples_rows_of_a_large_slab(tmp_path, monkeypatch):
    """A slab above the size budget is written as a fixed seeded choice of its
    rows: sorted, distinct, with the first and last two, the same every time,
    within the budget, and the ranks share the budget."""
    import argparse

    import numpy as np
    import torch

    import bench

    out = bench.regen_slab(5, 40, 8, torch.device("cpu"))
    monkeypatch.setattr(bench, "DUMP_BYTES", 20 * 8 * 4 * 4)  # 20 rows of float32
    for world, keep in ((1, 20), (2, 10)):
        ctx = argparse.Namespace(world=world, rank=world - 1)
        for d in ("x", "y"):
            bench.dump_outputs(str(tmp_path / f"{d}{world}"), out, ctx)
        rows = np.load(tmp_path / f"x{world}" / f"rows_rank{world - 1}.npy")
        vals = np.load(tmp_path / f"x{world}" / f"out_rank{world - 1}.npy")
        assert len(rows) == keep and list(rows) == sorted(set(rows)) and {0, 1, 38, 39} <= set(rows)
        assert vals.dtype == np.float32 and vals.nbytes <= bench.DUMP_BYTES // world
        assert np.array_equal(vals, out.numpy()[rows.astype(int)].astype(np.float32))
        assert np.array_equal(rows, np.load(tmp_path / f"y{world}" / f"rows_rank{world - 1}.npy"))


def test_bench_jacobi_two_ranks_cpu():
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
           "127.0.0.1", "--master-port", str(_port()), os.path.join(ROOT, "tools", "bench_jacobi.py"), "--device", "cpu",
           "--size", "64", "--iters", "12", "--warmup", "2", "--check-every", "4"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, OMP_NUM_THREADS="1"))
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert rec["n_gpus"] == 2 and rec["scaling"] == "strong" and rec["residual"] is not None and rec["value"] > 0
    assert rec["verified"] is True  # gathered 2-rank field == one-device run


def test_bench_jacobi_catches_injected_halo_corruption():
    """a silently corrupted halo value on one rank must fail the
    N-rank == one-device check (exit 3 from the rank, non-zero from torchrun)."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr",
           "127.0.0.1", "--master-port", str(_port()), os.path.join(ROOT, "tools", "bench_jacobi.py"), "--device", "cpu",
           "--size", "64", "--iters", "12", "--warmup", "2", "--check-every", "4"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, OMP_NUM_THREADS="1", MPX_FAULT_INJECT="halo:1:5"))
    assert r.returncode != 0
    rec = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][0])
    assert rec["verified"] is False


def test_bench_self_launches_ranks_cpu():
    """--gpus N without a torchrun environment launches N ranks itself."""
    rec = _run(["--gpus", "3", "--device", "cpu", "--size", "64", "--steps", "2", "--warmup", "1", "--rotate", "2",
                "--full"])
    assert rec["n_gpus"] == 3 and rec["world_size_seen"]["torch_distributed"] == 3
    # one entry per rank naming the device it ran on (PCI location on GPUs)
    assert rec["rank_devices"] == ["cpu"] * 3 and rec["distinct_devices"] == 1
    assert len(rec["per_rank_ms_per_step"]) == 3 and rec["verified_bit_exact"] is True
    # every pixel of every rotated slab on every rank was compared
    assert rec["verified_pixels"] == 3 * 2 * 64 * 64


def test_bench_refuses_world_mismatch_cpu():
    r = _run(["--gpus", "3", "--device", "cpu", "--size", "64", "--steps", "1", "--warmup", "0"], nproc=2, rc=2)
    assert "WORLD_SIZE=2" in r.stderr


def _torchrun(script, args, nproc, env):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
           "--master-addr", "127.0.0.1", "--master-port", str(_port()), os.path.join(ROOT, script), *args]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT,
                       env=dict(os.environ, OMP_NUM_THREADS="1", **env))
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def test_job_span_charges_injected_start_skew():
    """VERDICT r4 Next #1: rates come from the job span max(t1) - min(t0) on the
    node's shared clock. A 300 ms start delay injected on rank 1 of an
    independent-steps job (lab1 vsub: no inter-rank traffic in the timed
    region) lands in job_span_ms and lowers value; the slowest rank's own span
    (the round-4 figure) does not see it."""
    args = ["--workload", "vsub", "--device", "cpu", "--elems", "4096", "--steps", "3", "--warmup", "1"]
    base = _torchrun("tools/bench_workloads.py", args, 2, {})
    rec = _torchrun("tools/bench_workloads.py", args, 2, {"MPX_BENCH_START_DELAY": "1:300"})
    for r in (base, rec):
        assert r["verified"] is True and r["job_span_ms"] >= r["max_rank_span_ms"] > 0
        assert len(r["per_rank_ms_per_step"]) == 2
        # value and ms_per_step come from the job span
        assert abs(r["ms_per_step"] * r["steps"] - r["job_span_ms"]) <= 1e-3 * r["job_span_ms"] + 1e-4
    # (rank 0's own start may slip a few ms on a loaded CPU: the delay shows
    # up as the skew between the two ranks' starts, less that slip)
    assert rec["start_skew_ms"] >= 250.0 and rec["job_span_ms"] >= rec["start_skew_ms"]
    # without the hook the ranks leave at one agreed instant (aligned_start): the
    # skew is the spin's resolution plus scheduling noise, not barrier wake-ups
    # (bounded well below the injected 300 ms: a loaded CI host can deschedule
    # a spinning rank for tens of ms)
    assert base["start_skew_ms"] < 100.0
    assert rec["max_rank_span_ms"] < 150.0  # no rank's own span holds the delay
    assert rec["value"] < base["value"] * (base["job_span_ms"] / 300.0)


def test_bench_value_is_job_span_with_start_skew():
    """bench.py: with a 200 ms start delay on rank 1 the job span holds the
    delay and value = N * size^2 * K / job span (the slowest-rank figure and
    the skews ride along)."""
    rec = _run(["--gpus", "2", "--device", "cpu", "--size", "64", "--steps", "2", "--warmup", "1", "--rotate", "2",
                "--no-stream", "--no-warm", "--sustain-ms", "0", "--no-cpu-baseline"], nproc=2,
               env={"MPX_BENCH_START_DELAY": "1:200"})
    assert rec["start_skew_ms"] >= 150.0 and rec["job_span_ms"] >= rec["start_skew_ms"]
    assert rec["job_span_ms"] >= rec["max_rank_span_ms"]
    assert abs(rec["ms_per_step"] * 2 - rec["job_span_ms"]) <= 1e-3 * rec["job_span_ms"] + 1e-4
    assert abs(rec["value"] - 2 * 64 * 64 * 2 / (rec["job_span_ms"] * 1e-3) / 1e9) < 1e-3 * max(1e-3, rec["value"])


def test_scale_driver_job_is_the_driver_command():
    """SCALE N = 1 equals BENCH: tools/scale.py's conv/driver job runs exactly
    the driver's bench.py --gpus N --steps K --warmup W, plus --full (the
    headline first, then the streaming curve and the verification)."""
    import argparse
    import importlib.util

    spec = importlib.util.spec_from_file_location("scale", os.path.join(ROOT, "tools", "scale.py"))
    scale = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(scale)
    a = argparse.Namespace(device="auto", rehearse=False, contract=False, quick=False, driver_steps=20,
                           driver_warmup=5)
    for n in (1, 2, 8):
        job = [j for j in scale.plan(n, a, 8) if j["name"] == "conv/driver"][0]
        assert job["cmd"][1:] == ["bench.py", "--gpus", str(n), "--steps", "20", "--warmup", "5", "--full"]
        assert job["skip"] is None


def test_bench_streaming_timeout_on_one_rank_cpu():
    """VERDICT r5 Next #7 / ADVICE r5: a device-side halo wait that gives up on
    ONE rank during the timed streaming steps (MPX_BENCH_INJECT_STREAM_TIMEOUT)
    makes every rank leave the streaming phase together (no hang): the static
    headline stays measured and verified, value_streaming is null, and the
    record's status says streaming_failed; --strict-streaming turns it into a
    non-zero exit."""
    args = ["--gpus", "2", "--device", "cpu", "--size", "64", "--steps", "2", "--warmup", "1", "--rotate", "2",
            "--no-warm", "--sustain-ms", "0", "--no-cpu-baseline", "--full"]
    rec = _run(args, nproc=2, env={"MPX_BENCH_INJECT_STREAM_TIMEOUT": "1"})
    assert rec["value"] > 0 and rec["verified_bit_exact"] is True and rec["verified_pixels"] == 2 * 2 * 64 * 64
    assert rec["value_streaming"] is None and "timed out" in rec["streaming_error"]
    assert rec["verified_bit_exact_streaming"] is None and rec["status"] == "streaming_failed"
    ok = _run(args, nproc=2)
    assert ok["status"] == "ok" and ok["value_streaming"] > 0
    _run(args + ["--strict-streaming"], nproc=2, env={"MPX_BENCH_INJECT_STREAM_TIMEOUT": "0"}, rc=3)


def test_bench_records_multi_node_clock_policy():
    """the job span uses one shared clock only on one node; the
    record says which clock it used (here: one host, shared)."""
    rec = _run(["--gpus", "2", "--device", "cpu", "--size", "64", "--steps", "2", "--warmup", "1", "--rotate", "2",
                "--no-stream", "--no-warm", "--sustain-ms", "0", "--no-cpu-baseline"], nproc=2)
    assert rec["clock"] == "shared-monotonic" and rec["start_skew_ms"] is not None


def test_bench_strong_layout_equals_one_device_cpu():
    """VERDICT r5 Next #2: --layout strong splits ONE global image over the
    ranks (rows_per_rank = size / N, uneven at N = 3); the gathered N-rank
    output of every rotated frame equals a one-device run on every pixel, and
    the record says strong."""
    for n in (2, 3):
        rec = _run(["--gpus", str(n), "--device", "cpu", "--layout", "strong", "--size", "97", "--steps", "2",
                    "--warmup", "1", "--rotate", "2", "--no-warm", "--sustain-ms", "0", "--no-cpu-baseline", "--full"],
                   nproc=n)
        assert rec["scaling"] == "strong" and rec["config"]["layout"] == "strong"
        assert rec["config"]["image_hw"] == [97, 97] and sum(rec["config"]["rows_per_rank"]) == 97
        assert rec["verified_one_device"] is True and rec["verified_bit_exact"] is True
        assert rec["verified_pixels"] == 2 * 97 * 97 and rec["verified_bit_exact_streaming"] is True
        # value: the ONE image's pixels per step over the job span
        assert abs(rec["value"] - 97 * 97 / (rec["ms_per_step"] * 1e-3) / 1e9) < 1e-3 * max(1e-3, rec["value"])
    one = _run(["--device", "cpu", "--layout", "strong", "--size", "64", "--steps", "2", "--warmup", "1",
                "--rotate", "2", "--no-stream", "--no-warm", "--sustain-ms", "0", "--no-cpu-baseline", "--full"])
    assert one["n_gpus"] == 1 and one["config"]["image_hw"] == [64, 64] and one["verified_one_device"] is True


def test_scale_plans_strong_conv_job():
    import argparse
    import importlib.util

    spec = importlib.util.spec_from_file_location("scale", os.path.join(ROOT, "tools", "scale.py"))
    scale = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(scale)
    a = argparse.Namespace(device="auto", rehearse=False, contract=False, quick=False, driver_steps=20,
                           driver_warmup=5)
    job = [j for j in scale.plan(8, a, 8) if j["name"] == "conv/strong"][0]
    assert job["kind"] == "strong" and "--layout" in job["cmd"] and job["cmd"][job["cmd"].index("--layout") + 1] \
        == "strong"
    rows = [{"name": "conv/strong", "kind": "strong", "n": 1, "status": "ok", "ms": 0.024},
            {"name": "conv/strong", "kind": "strong", "n": 8, "status": "ok", "ms": 0.004}]
    scale.efficiencies(rows)
    assert rows[1]["efficiency"] == round(0.024 / (8 * 0.004), 4) and rows[1]["speedup"] == 6.0
