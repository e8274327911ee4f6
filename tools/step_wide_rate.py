"""Wall time of tz_search_step against tz_search_step_wide on one tree of an engine's size.

Twin one-game 5x5 handles on a small ARCH_TEST net (2 blocks, random init), node_capacity 8 M, are grown with
simulate_batch(leaves=128) until about 10^5 and about 10^6 node slots are allocated; then one steps the most visited move with
tz_search_step and the other with tz_search_step_wide, each timed from a synchronised stream to the call's return (both calls
synchronise).  Three runs per size, each on freshly grown trees (a step consumes its tree), the order of the two calls alternating; one
untimed step of each kind comes first, so that no timed call allocates.
Both numbers are recorded as measured; no ratio is asserted.  The two handles must agree on the root and the pool afterwards.

    python tools/step_wide_rate.py [--out profiles/step_wide_rate.json] [--sizes 100000,1000000]
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
from takzero_amd import weights as W  # noqa: E402

CAPACITY = 8 << 20
LEAVES = 128


def grow(m, target):
    """from the empty board to at least `target` allocated node slots"""
    m.set_positions([0], [A.state_from_tps("x5/x5/x5/x5/x5 1 1", 5, 4)])
    betas = np.zeros(1, np.float32)
    while m.pool_usage()[0] < target:
        m.simulate_batch(betas, LEAVES, 4)
    m.sync()


def timed(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "step_wide_rate.json"))
    ap.add_argument("--sizes", default="100000,1000000")
    args = ap.parse_args()
    nets = [A.Net(arch=A.ARCH_TEST, n=5, precision=A.PREC_F16, blocks=2).load_tensors(W.init_weights(W.ARCH_TEST, n=5, blocks=2, seed=3))
            for _ in range(2)]
    a, b = (A.BatchedMCTS(1, 5, 4, agent=net, node_capacity=CAPACITY) for net in nets)
    for m in (a, b):                            # untimed: the first calls allocate (the wide step its scan scratch)
        grow(m, 1000)
    first = a.select_best_actions()
    a.step(first)
    b.step_wide(first)
    out = dict(net="ARCH_TEST 5x5, 2 blocks", node_capacity=CAPACITY, leaves=LEAVES, rows=[])
    for target in [int(x) for x in args.sizes.split(",") if x]:
        row = dict(target_slots=target, step_ms=[], step_wide_ms=[])
        for run in range(3):
            grow(a, target)
            grow(b, target)
            assert a.root_info().tobytes() == b.root_info().tobytes() and a.pool_usage() == b.pool_usage()
            action = a.select_best_actions()
            row["slots_before"], row["root_visits"] = int(a.pool_usage()[0]), int(a.root_info()["visit_count"][0])
            calls = [("step_ms", lambda: a.step(action)), ("step_wide_ms", lambda: b.step_wide(action))]
            for key, call in (calls if run % 2 == 0 else calls[::-1]):
                row[key].append(round(timed(call), 3))
            assert a.root_info().tobytes() == b.root_info().tobytes() and a.pool_usage() == b.pool_usage()
            row["slots_kept"], row["kept_visits"] = int(a.pool_usage()[0]), int(a.root_info()["visit_count"][0])
        out["rows"].append(row)
        print(json.dumps(row), flush=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
