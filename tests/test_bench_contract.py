"""bench.py prints ONE JSON line with the fields the driver reads (a reduced workload here; the default run is the
driver's).  Guards the contract, not the numbers."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [[], ["--search", "gumbel", "--sims", "384"], ["--precision", "bf16"]])
def test_bench_line_has_the_contract_fields(extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--games", "256",
           "--sims", "48", "--no-cpu-baseline"] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-500:]
    out = json.loads(lines[0])
    for key, typ in (("metric", str), ("value", float), ("unit", str), ("n_gpus", int), ("steps", int), ("warmup", int),
                     ("ms_per_step", float), ("higher_is_better", bool), ("scaling", str), ("dtype", str), ("data", str),
                     ("config", dict), ("roofline", dict)):
        assert isinstance(out[key], typ), (key, out[key])
    assert out["vs_baseline"] is None and out["n_gpus"] == 1 and out["steps"] == 2 and out["warmup"] == 1
    assert out["metric"] == "mcts_simulations_per_s" and out["scaling"] == "weak" and out["higher_is_better"] is True
    assert "workload" in out["config"] and "model" not in out["config"]
    rf = out["roofline"]
    assert rf["bound"] == "mfma" and rf["unit"] == "TFLOP/s" and rf["peak"] == 2500.0
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-9 and rf["achieved"] > 0
    assert out["value"] > 0 and out["ms_per_step"] > 0
    expect = "bf16" if "bf16" in extra else "f16"   # fp16 storage is the default (within 1e-3 of the fp32 graph)
    assert out["dtype"] == expect


@pytest.mark.gpu
def test_dumped_outputs_are_the_same_from_run_to_run(tmp_path):
    """--dump-outputs DIR: what the last timed step computed, as float32 / float64 .npy files; the same arguments give the
    same inputs, so two runs write the same arrays."""
    import numpy as np

    dumps = []
    for run in range(2):
        d = tmp_path / ("run%d" % run)
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "6", "--warmup", "1", "--games", "256",
               "--sims", "16", "--no-cpu-baseline", "--no-precision-report", "--dump-outputs", str(d)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        assert json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])["steps"] == 6
        dumps.append({p.stem: np.load(p) for p in d.glob("*.npy")})
    a, b = dumps
    assert sorted(a) == sorted(b) and {"positions", "root_visit_count", "child_visits", "child_logit", "target_policy"} <= set(a)
    assert sum(os.path.getsize(p) for p in (tmp_path / "run0").glob("*.npy")) <= 64 << 20
    for k in a:
        assert a[k].dtype in (np.float32, np.float64), k
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert a["root_visit_count"].shape == (256,) and a["positions"].shape[0] == 256 and a["child_visits"].sum() > 0


@pytest.mark.gpu
def test_plain_run_leaves_out_what_full_adds():
    """A plain run prints the headline figures alone; --full adds what takes runs of its own after the timed steps (here
    the Agent surface: the CPU stand-in is switched off, and the other precisions run at the full 4096 games only)."""
    outs = []
    for flags in ([], ["--full", "--no-cpu-baseline"]):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "1", "--games", "256",
               "--sims", "16"] + flags
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0]))
    plain, full = outs
    assert not {"agent_surface", "cpu_baseline", "precisions", "within_1e-3_at_trained_scale"} & set(plain)
    assert isinstance(plain["roofline"], dict) and plain["value"] > 0
    assert "cpu_baseline" not in full and "error" not in full["agent_surface"]
    assert full["agent_surface"]["batch_128"]["ms_per_call"] > 0 and full["agent_surface"]["batch_1"]["ms_per_call"] > 0


def test_dump_outputs_keeps_a_fixed_sample_under_the_limit(tmp_path):
    import numpy as np

    import bench

    arrays = {"small": np.arange(10, dtype=np.uint16), "big": np.arange(400_000, dtype=np.float32).reshape(4000, 100),
              "wide": np.ones((4000, 50), np.uint32)}
    for run in range(2):
        bench.dump_outputs(str(tmp_path / str(run)), arrays, limit=1 << 20)
    files = sorted(p.name for p in (tmp_path / "0").glob("*.npy"))
    assert files == ["big.npy", "big_rows.npy", "small.npy", "small_rows.npy", "wide.npy", "wide_rows.npy"]
    assert sum(os.path.getsize(p) for p in (tmp_path / "0").glob("*.npy")) <= 1 << 20
    big, rows = np.load(tmp_path / "0" / "big.npy"), np.load(tmp_path / "0" / "big_rows.npy")
    assert big.dtype == np.float32 and np.load(tmp_path / "0" / "wide.npy").dtype == np.float64
    assert np.array_equal(big, arrays["big"][rows.astype(np.int64)]) and np.all(np.diff(rows) > 0)
    assert all(np.array_equal(np.load(tmp_path / "0" / f), np.load(tmp_path / "1" / f)) for f in files)
    bench.dump_outputs(str(tmp_path / "whole"), arrays)
    assert np.array_equal(np.load(tmp_path / "whole" / "wide.npy"), arrays["wide"]) and not (tmp_path / "whole" / "wide_rows.npy").exists()


@pytest.mark.gpu
def test_two_rank_launch_as_the_driver_does_it():
    """python -m torch.distributed.run --nproc-per-node 2 bench.py --gpus 2 ...: both ranks on this box's one GPU with
    the target exchange over gloo (TZ_BENCH_BACKEND / TZ_BENCH_DEVICE are the rehearsal switches; on the 8-GPU node the
    default is RCCL, one rank per GPU).  Rank 0 prints the one line; value aggregates both ranks."""
    env = dict(os.environ, TZ_BENCH_BACKEND="gloo", TZ_BENCH_DEVICE="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29617", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--games", "128", "--sims", "32", "--no-cpu-baseline"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-800:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["scaling"] == "weak" and out["value"] > 0
    # the line says what carried the exchange: here the rehearsal switches (gloo process group, shared-directory transport)
    assert out["backend"] == "gloo" and out["world"] == 2
    assert out["exchange"]["transport"] == "fs" and out["exchange"]["world"] == 2 and out["exchange"]["collectives"] == 1 + 3 * 3   # the probe + 3 gathers per move
    assert out["targets_gathered"] >= 0
    # whole-job aggregate: 2 ranks x 128 games x 33 simulate calls per move x 2 timed moves
    assert abs(out["value"] * out["ms_per_step"] * 2 / 1000.0 - 2 * 128 * 33 * 2) < 0.02 * 2 * 128 * 33 * 2


@pytest.mark.gpu
def test_two_rank_launch_through_the_rccl_communicator_of_the_library(tmp_path):
    """The same two-rank launch with the hand-over through the library's RCCL communicator - what the 8-GPU run does - on this
    box's one GPU: RCCL refuses two ranks on one device, so TZ_RCCL_LIB points the library at the stand-in of tests/mock_rccl.cpp
    (RCCL's entry points, bytes through files) and TZ_BENCH_COMM=rccl selects the communicator although the process group is
    gloo.  Covers takzero_amd/comm.py's unique id, its broadcast to the ranks, tz_comm_create_rccl at world 2 and the per-move
    all-gathers from Python."""
    mock = str(tmp_path / "libmockrccl.so")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "-shared", "-fPIC", "-O1", "-w", os.path.join(ROOT, "tests", "mock_rccl.cpp"), "-o", mock],
                       capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("cannot build the stand-in library here: " + r.stderr[-300:])
    env = dict(os.environ, TZ_BENCH_BACKEND="gloo", TZ_BENCH_DEVICE="0", TZ_BENCH_COMM="rccl", TZ_RCCL_LIB=mock)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29619", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--games", "128", "--sims", "32", "--no-cpu-baseline"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-800:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["world"] == 2 and out["value"] > 0
    assert out["exchange"]["transport"] == "rccl" and out["exchange"]["world"] == 2 and out["exchange"]["collectives"] == 1 + 3 * 3
    assert "native_exchange_error" not in out["exchange"]


@pytest.mark.gpu
def test_the_rccl_set_up_of_a_multi_gpu_run_with_one_rank():
    """What the driver's N > 1 launch does before the timed region, on this box's one GPU (TZ_BENCH_FORCE_DIST=1): torchrun,
    process group over nccl (= RCCL), the all_reduce probe, the communicator id broadcast through it, the library's own RCCL
    communicator (ncclCommInitRank on PyTorch's RCCL copy - one RCCL, one HIP runtime in the process), the data probe.  The
    line must name them."""
    env = dict(os.environ, TZ_BENCH_FORCE_DIST="1")
    for k in ("TZ_BENCH_BACKEND", "TZ_BENCH_DEVICE", "TZ_BENCH_EXCHANGE"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
           "--master-port", "29641", os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--games", "256",
           "--sims", "32", "--no-cpu-baseline", "--no-precision-report"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2500:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-800:]
    out = json.loads(lines[0])
    assert out["backend"] == "nccl" and out["world"] == 1 and out["n_gpus"] == 1
    assert out["exchange"]["transport"] == "rccl" and out["exchange"]["api"].startswith("tz_comm") and out["exchange"]["collectives"] >= 1
    assert "double free" not in r.stderr and "Aborted" not in r.stderr


@pytest.mark.gpu
def test_plain_invocation_with_gpus_2_launches_its_own_ranks():
    env = dict(os.environ, TZ_BENCH_BACKEND="gloo", TZ_BENCH_DEVICE="0")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "1", "--games", "128",
                        "--sims", "16", "--no-cpu-baseline"], capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1 and json.loads(lines[0])["n_gpus"] == 2


def test_requested_rccl_that_cannot_form_is_a_failed_run_not_a_fallback():
    """ADVICE r1 / VERDICT r1 #2a: `--gpus 2` with the default backend (nccl = RCCL) where RCCL cannot come up (this
    container has no GPU) must end non-zero with the reason on stderr and print no JSON line: a SCALE record can then never
    show a number that a silent gloo fallback produced."""
    import torch

    if torch.cuda.is_available():
        pytest.skip("needs a box without a GPU: on the GPU box two ranks would contend for one device")
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "TZ_BENCH_BACKEND", "TZ_BENCH_DEVICE"):
        env.pop(k, None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29633", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--games", "16",
           "--sims", "4", "--no-cpu-baseline"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert r.returncode != 0
    assert "backend nccl (RCCL) requested and unavailable" in r.stderr
    assert not [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
