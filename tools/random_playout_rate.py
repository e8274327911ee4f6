"""Wall time of random playouts on the device, and of one seen-ratio experiment at the reference's size.

1. BatchedMCTS.random_steps(60) (one launch, tz_search_random_steps) against the per-ply emulation the tree already has
   (NativeSelfPlay(..., search="random"): one simulation to expand the root, a read-back of every root's child row, the host's pick
   and a step, 60 times) at 64, 4096 and 65 536 games on 4x4 and 5x5.  Both on the same handle (Dummy agent), in the same
   process, interleaved, three runs each, every run from fresh openings; each timed from a synchronised stream to the return of
   the last call.  One untimed run of each kind comes first.
2. One eee.seen_ratio(plies 0..99, 65 536 games, batch 4096) on a random-init net4_lcghash: 324 M random moves.

The numbers are recorded as measured; nothing is asserted.

    python tools/random_playout_rate.py [--out profiles/random_playout_rate.json] [--games 64,4096,65536] [--no-seen-ratio]
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
from takzero_amd import eee  # noqa: E402
from takzero_amd.selfplay import NativeSelfPlay  # noqa: E402

STEPS = 60
RUNS = 3


def timed(call):
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def spread(ms):
    return dict(ms=[round(x, 3) for x in ms], median_ms=round(float(np.median(ms)), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "random_playout_rate.json"))
    ap.add_argument("--games", default="64,4096,65536")
    ap.add_argument("--no-seen-ratio", action="store_true")
    args = ap.parse_args()
    out = dict(steps=STEPS, runs=RUNS, rows=[])
    for n in (4, 5):
        for B in [int(x) for x in args.games.split(",") if x]:
            # the emulation expands every root once per ply: room for a root and its children (at most 192 / 512 here)
            m = A.BatchedMCTS(B, n, 4, agent_kind=A.AGENT_DUMMY, node_capacity=256 if n == 4 else 1024)
            choice = np.arange(B, dtype=np.int32) % 16
            sp = NativeSelfPlay(m, 1, seed=1, search="random")

            def kernel():
                m.random_steps(STEPS, 1)

            def emulation():
                for _ in range(STEPS):
                    sp.play_move()
                m.sync()

            row = dict(board=n, games=B, random_steps_ms=[], emulation_ms=[])
            for run in range(RUNS + 1):
                for name, call in (("random_steps_ms", kernel), ("emulation_ms", emulation)):
                    m.new_openings(choice)
                    m.sync()
                    ms = timed(call)
                    if run:                      # run 0 is untimed
                        row[name].append(ms)
            row["random_steps"] = spread(row.pop("random_steps_ms"))
            row["emulation"] = spread(row.pop("emulation_ms"))
            row["moves_per_s_random_steps"] = round(B * STEPS / (row["random_steps"]["median_ms"] * 1e-3))
            out["rows"].append(row)
            print(json.dumps(row), flush=True)
            sp.close()
            m.close()
    if not args.no_seen_ratio:
        net = A.Net.new(arch=A.ARCH_NET4_LCGHASH, seed=1, precision=A.PREC_F16)
        m = A.BatchedMCTS(4096, 4, 4, agent=net, node_capacity=1)
        eee.seen_ratio(m, plies=range(2), games=4096)        # untimed
        res = []
        ms = timed(lambda: res.extend(eee.seen_ratio(m, plies=range(100), games=65536, seed=123)))
        out["seen_ratio"] = dict(net="net4_lcghash, random init, empty set", plies=100, games=65536, batch=4096, wall_s=round(ms / 1e3, 3),
                                 ratios_first_last=[res[0], res[-1]])
        print(json.dumps(out["seen_ratio"]), flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
