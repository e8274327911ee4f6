"""Times the learn step of net4_rnd (16 blocks, batch 128, fp32) with the predictor tower trained in the step (tz_trainer_rnd4_enable), with
it off, and on a checkout of the parent commit, and sums the tower kernels of one step from a kernel trace.

  python tools/rnd4_learn_bench.py [--steps N] [--batch B] [--parent-root DIR] [--no-trace] [--out profiles/rnd4_learn_bench.json]

Three runs of each variant, interleaved (on, off, parent, on, off, parent, ...), every run a fresh process of this file in --child mode.
--parent-root names a checkout of the parent commit with its library built; without it that column is left out.  One more run of the
enabled variant goes under `rocprofv3 --kernel-trace --stats --output-format csv` for the summed time of the tower kernels (r4l_*) per step; counters, if wanted, belong in a run of their own.  The comparison is on minus off: if it exceeds the runs' spread by more than
the tower kernels' summed time, the side stream is not overlapping.  Nothing here is a pass / fail number."""
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARMUP = 3


def _arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def child():
    """one timing run: prints {"ms_per_step": ..}; --root picks the tree the package is imported from"""
    sys.path.insert(0, _arg("--root", ROOT))
    import takzero_amd.api as A
    from takzero_amd import learn as L
    from takzero_amd import weights as W
    from takzero_amd.selfplay import SelfPlay

    steps, B, n = _arg("--steps", 100), _arg("--batch", 128), 4
    tr = L.Trainer(arch=A.ARCH_NET4_RND, batch=B).load_tensors(W.init_weights(W.ARCH_NET4_RND, seed=123))
    if "--on" in sys.argv:
        tr.rnd4_enable()
    sp = SelfPlay(A.BatchedMCTS(B, n, 4, agent_kind=A.AGENT_DUMMY, node_capacity=1 << 10), 0, seed=1, search="random")
    targets = []
    while len(targets) < B:
        targets.extend(sp.play_move()[0])
    tensors = L.target_tensors(targets[:B], n)
    for _ in range(WARMUP):
        tr.step(*tensors, train_ube=True)
    t0 = time.perf_counter()
    for _ in range(steps):
        tr.step(*tensors, train_ube=True)
    line = {"ms_per_step": (time.perf_counter() - t0) / steps * 1e3}
    if "--on" in sys.argv:
        line["loss_rnd"] = tr.rnd4_last()[0]
    print(json.dumps(line))


def _run(extra, prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), "--child"] + extra
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError("%s failed: %s" % (" ".join(cmd), r.stderr[-2000:]))
    return json.loads([s for s in r.stdout.splitlines() if s.startswith("{")][-1])


def main():
    steps, B = _arg("--steps", 100), _arg("--batch", 128)
    parent = _arg("--parent-root", "")
    common = ["--steps", str(steps), "--batch", str(B)]
    variants = [("feature_on", common + ["--on"]), ("feature_off", common)]
    if parent:
        variants.append(("parent_commit", common + ["--root", parent]))
    runs = {name: [] for name, _ in variants}
    loss = None
    for _ in range(3):
        for name, extra in variants:
            line = _run(extra)
            runs[name].append(round(line["ms_per_step"], 3))
            loss = line.get("loss_rnd", loss)
    mean = {k: round(sum(v) / len(v), 3) for k, v in runs.items()}
    spread = round(max(max(v) - min(v) for v in runs.values()), 3)
    out = {"what": "tools/rnd4_learn_bench.py --steps %d --batch %d (net4_rnd, 16 blocks, fp32) on one MI355X, the variants interleaved, three "
                   "runs each; ms per step" % (steps, B),
           "ms_per_step": runs, "mean_ms_per_step": mean, "on_minus_off_ms": round(mean["feature_on"] - mean["feature_off"], 3),
           "largest_spread_of_a_variant_ms": spread, "loss_rnd_after_the_run": loss}
    if "--no-trace" not in sys.argv:
        with tempfile.TemporaryDirectory() as d:
            traced = 20
            _run(["--steps", str(traced), "--batch", str(B), "--on"], ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "rnd4", "--"])
            per_step, total = {}, traced + WARMUP
            for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
                for row in csv.DictReader(open(path)):
                    if "r4l_" in row["Name"]:
                        short = row["Name"].split("r4l_")[1].split("(")[0].split("<")[0]
                        per_step[short] = per_step.get(short, 0.0) + float(row["TotalDurationNs"]) / total / 1e3
            if not per_step:
                raise RuntimeError("the kernel trace holds no r4l_* kernel")
            out["tower_kernels_us_per_step (kernel-trace stats of %d steps)" % total] = {k: round(v, 1) for k, v in sorted(per_step.items())}
            out["tower_kernels_sum_ms_per_step"] = round(sum(per_step.values()) / 1e3, 3)
            over = out["on_minus_off_ms"] - spread
            out["reading"] = ("on minus off exceeds the runs' spread by more than the tower kernels' summed time: the side stream is not overlapping"
                              if over > out["tower_kernels_sum_ms_per_step"] else
                              "on minus off stays within the runs' spread plus the tower kernels' summed time: no sign that the side stream fails to overlap")
    path = _arg("--out", os.path.join(ROOT, "profiles", "rnd4_learn_bench.json"))
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    child() if "--child" in sys.argv else main()
