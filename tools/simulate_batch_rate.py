"""Simulations per second of tz_search_simulate_batch (Node::simulate_batch on the device) on net5, f16, 5x5.

Two things are reported, each after a warm-up of 256 simulations per tree and timed over 2048 more to tz_search_sync:
  * 128 trees: leaves 8 and 32, set against tz_search_simulate (lock-step, one leaf per tree per network call) on the same
    128 trees in the same process;
  * 1 tree, leaves 128 (the shape of the reference's tei / analysis): simulations/s and the split of a round between the forward
    kernel, the network and the backward pass from HIP events (tz_search_batch_profile).

    python tools/simulate_batch_rate.py [--out profiles/simulate_batch_rate.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import takzero_amd.api as A  # noqa: E402


def fresh(net, trees):
    m = A.BatchedMCTS(trees, 5, 4, agent=net)
    m.new_openings(np.arange(trees) % 16)
    return m


WARM, TIMED = 256, 2048     # simulations per tree: together they stay inside the default node pool of a 5x5 tree (262 144 slots)


def timed(m, run):
    """simulations (forwards made, by the handle's own counter) per second of run(), timed to tz_search_sync"""
    m.sync()
    s0 = m.counters()[0]
    t0 = time.perf_counter()
    run()
    m.sync()
    dt = time.perf_counter() - t0
    return (m.counters()[0] - s0) / dt, dt


def measure_batch(net, trees, leaves):
    m = fresh(net, trees)
    betas = np.zeros(trees, np.float32)
    m.simulate_batch(betas, leaves, WARM // leaves)
    rate, dt = timed(m, lambda: m.simulate_batch(betas, leaves, TIMED // leaves))
    m.profile(1)
    m.simulate_batch(betas, leaves, 4)
    split = m.batch_profile()
    m.profile(2)
    n = max(1, split["rounds"])
    row = dict(trees=trees, leaves=leaves, path="tz_search_simulate_batch", simulations_per_s=round(rate), seconds=round(dt, 4),
               rounds_timed=TIMED // leaves,
               round_ms=dict(forward=round(split["forward_ms"] / n, 4), net=round(split["net_ms"] / n, 4),
                             backward=round(split["backward_ms"] / n, 4)),
               pool_used=int(m.pool_usage()[0]), pool_overflows=int(m.pool_overflows()))
    m.close()
    return row


def measure_lock_step(net, trees):
    m = fresh(net, trees)
    betas = np.zeros(trees, np.float32)
    m.simulate(betas, WARM)
    rate, dt = timed(m, lambda: m.simulate(betas, TIMED))
    row = dict(trees=trees, leaves=1, path="tz_search_simulate", simulations_per_s=round(rate), seconds=round(dt, 4),
               pool_used=int(m.pool_usage()[0]), pool_overflows=int(m.pool_overflows()))
    m.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    net = A.Net.new(arch=A.ARCH_NET5, seed=1, precision=A.PREC_F16)
    out = dict(net="net5", precision="f16", board=5, rows=[])
    out["rows"].append(measure_lock_step(net, 128))
    for leaves in (8, 32):
        out["rows"].append(measure_batch(net, 128, leaves))
    out["rows"].append(measure_batch(net, 1, 128))
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
