"""Simulations per second of the three in-tree selection rules (tz_search_set_selection: puct, uct, improved) on net5, f16, 5x5.

Per rule, each after a warm-up and timed to tz_search_sync:
  * 128 and 4096 games: lock-step tz_search_simulate (256 warm-up + 512 timed simulations per game) and Gumbel halving
    (tz_search_gumbel_sh, 64 sampled actions, budget 768; one warm-up call on fresh trees, one timed call on fresh trees);
  * 1 tree with tz_search_simulate_batch(leaves=128): 256 warm-up + 2048 timed simulations.
The improved rule pays one exp per child and level and a serial sum; uct drops puct's prior term.  There is no target for either.

    python tools/selection_rate.py [--out profiles/selection_rate.json] [--games 128,4096]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import takzero_amd.api as A  # noqa: E402

RULES = ("puct", "uct", "improved")


def fresh(net, games, rule):
    m = A.BatchedMCTS(games, 5, 4, agent=net)
    m.set_selection(rule)
    m.new_openings(np.arange(games) % 16)
    return m


def timed(m, run):
    """simulations (forwards made, by the handle's own counter) per second of run(), timed to tz_search_sync"""
    m.sync()
    s0 = m.counters()[0]
    t0 = time.perf_counter()
    run()
    m.sync()
    dt = time.perf_counter() - t0
    return (m.counters()[0] - s0) / dt, dt


def row(m, rule, games, path, rate, dt):
    return dict(rule=rule, games=games, path=path, simulations_per_s=round(rate), seconds=round(dt, 4),
                pool_used=int(m.pool_usage()[0]), pool_overflows=int(m.pool_overflows()))


def lock_step(net, games, rule, warm=256, sims=512):
    m = fresh(net, games, rule)
    betas = np.zeros(games, np.float32)
    m.simulate(betas, warm)
    rate, dt = timed(m, lambda: m.simulate(betas, sims))
    r = row(m, rule, games, "tz_search_simulate", rate, dt)
    m.close()
    return r


def gumbel(net, games, rule, k=64, budget=768):
    m = fresh(net, games, rule)
    betas = np.zeros(games, np.float32)
    g = np.random.default_rng(1).gumbel(size=(games, 512)).astype(np.float32)
    m.gumbel_sequential_halving(betas, k, budget, g)       # warm-up: allocations and graph capture
    m.new_openings(np.arange(games) % 16)
    rate, dt = timed(m, lambda: m.gumbel_sequential_halving(betas, k, budget, g))
    r = row(m, rule, games, "tz_search_gumbel_sh %d/%d" % (k, budget), rate, dt)
    m.close()
    return r


def one_tree(net, rule, leaves=128, warm=256, sims=2048):
    m = fresh(net, 1, rule)
    betas = np.zeros(1, np.float32)
    m.simulate_batch(betas, leaves, warm // leaves)
    rate, dt = timed(m, lambda: m.simulate_batch(betas, leaves, sims // leaves))
    r = row(m, rule, 1, "tz_search_simulate_batch leaves=%d" % leaves, rate, dt)
    m.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "selection_rate.json"))
    ap.add_argument("--games", default="128,4096")
    args = ap.parse_args()
    net = A.Net.new(arch=A.ARCH_NET5, seed=1, precision=A.PREC_F16)
    out = dict(net="net5", precision="f16", board=5, rows=[])
    for games in [int(x) for x in args.games.split(",") if x]:
        for rule in RULES:
            out["rows"].append(lock_step(net, games, rule))
            print(json.dumps(out["rows"][-1]), flush=True)
        for rule in RULES:
            out["rows"].append(gumbel(net, games, rule))
            print(json.dumps(out["rows"][-1]), flush=True)
    for rule in RULES:
        out["rows"].append(one_tree(net, rule))
        print(json.dumps(out["rows"][-1]), flush=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
