"""What the engine session (api.Tei, tz_tei_*) does in a two-second think, on net5 and net6_simhash at random init, f16.

Per net: `go movetime 2000` from the start position on a one-game handle with node_capacity 8 M and 128 leaves per round; the last
info line's `nodes` and `nps` are recorded, the pool in use, and then the wall time of the `position startpos moves <bestmove>
<reply>` that follows (the reply is the second move of the last principal variation): two tz_search_step_wide calls on the tree
the think has built.

    python tools/tei_rate.py [--out profiles/tei_rate.json] [--movetime 2000]
"""
import argparse
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import takzero_amd.api as A  # noqa: E402

INFO = re.compile(r"^info time (\d+) nodes (\d+) nps (\d+) .* pv ?(.*)$")


def think(name, arch, n, movetime):
    net = A.Net.new(arch=arch, seed=1, precision=A.PREC_F16)
    mcts = A.BatchedMCTS(1, n, 4, agent=net, node_capacity=8 << 20)
    infos = []
    tei = A.Tei(mcts, leaves=128, sink=lambda text: infos.append(text) and False)
    assert tei.line("isready") == ["readyok"]
    assert tei.line("position startpos") == []
    lines = tei.line("go movetime %d" % movetime)
    last = INFO.match(infos[-1])
    best = [l.split()[1] for l in lines if l.startswith("bestmove ")][0]
    pv = last.group(4).split()
    row = dict(net=name, board=n, movetime_ms=movetime, info_lines=len(infos), time_ms=int(last.group(1)), nodes=int(last.group(2)),
               nps=int(last.group(3)), pool_used=int(mcts.pool_usage()[0]), pool_overflows=int(mcts.pool_overflows()),
               pool_full="info string node pool full" in lines, bestmove=best)
    if len(pv) >= 2 and pv[0] == best:
        t0 = time.perf_counter()
        out = tei.line("position startpos moves %s %s" % (pv[0], pv[1]))
        row["position_two_moves_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        assert out == [], out
        row["kept_visits"], row["kept_slots"] = int(mcts.root_info()["visit_count"][0]), int(mcts.pool_usage()[0])
    tei.close()
    mcts.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tei_rate.json"))
    ap.add_argument("--movetime", type=int, default=2000)
    args = ap.parse_args()
    out = dict(precision="f16", leaves=128, node_capacity=8 << 20, rows=[])
    for name, arch, n in (("net5", A.ARCH_NET5, 5), ("net6_simhash", A.ARCH_NET6_SIMHASH, 6)):
        out["rows"].append(think(name, arch, n, args.movetime))
        print(json.dumps(out["rows"][-1]), flush=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
