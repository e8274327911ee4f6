"""What the LCG hash of net4_lcghash costs beside the SimHash of net4_simhash, on one device in one process:

  * the index-plus-lookup kernel alone (lcghash_state_kernel / simhash_state_kernel through tz_debug_hash_bench: HIP events around
    `iters` launches) at 128 and 4096 4x4 positions, the two archs interleaved, `repeats` times;
  * lock-step search (PUCT, random-init nets, f16) at 64 and 4096 games, simulations/s, the two archs interleaved, `repeats` times.

Writes profiles/lcghash_rate.json with every repeat, the medians and the repeat-to-repeat spread (max - min).
python tools/lcghash_rate.py [repeats] [sims]"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import takzero_amd.api as A
from takzero_amd import weights as W
from takzero_amd.precision import sample_positions

repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
sims = int(sys.argv[2]) if len(sys.argv) > 2 else 200
ARCHS = (("net4_lcghash", A.ARCH_NET4_LCGHASH, W.ARCH_NET4_LCGHASH), ("net4_simhash", A.ARCH_NET4_SIMHASH, W.ARCH_NET4_SIMHASH))
nets = {name: A.Net(arch=a).load_tensors(W.init_weights(w, seed=123)) for name, a, w in ARCHS}


def summary(xs):
    return {"runs": [float(x) for x in xs], "median": float(np.median(xs)), "spread": float(max(xs) - min(xs))}


out = {"repeats": repeats, "sims": sims, "kernel_us": {}, "search_sims_per_s": {}}
positions = sample_positions(4, 4, 4096, seed=11, plies=12)
for batch in (128, 4096):
    st = A._states(positions[:batch])
    runs = {name: [] for name in nets}
    for rep in range(repeats + 1):                      # the first pass warms both up and is dropped
        for name, net in nets.items():
            ms = C.c_float()
            A.check(net.lib.tz_debug_hash_bench(net.h, batch, st.ctypes.data, 200, C.byref(ms)))
            if rep:
                runs[name].append(1000.0 * ms.value)
    out["kernel_us"][str(batch)] = {name: summary(r) for name, r in runs.items()}
    print("%4d positions: " % batch + ", ".join("%s %.2f us (spread %.2f)" % (n, np.median(r), max(r) - min(r)) for n, r in runs.items()))

for games in (64, 4096):
    searches = {}
    for name, net in nets.items():
        m = A.BatchedMCTS(games, 4, 4, agent=net)
        m.new_openings(np.arange(games) % 16)
        searches[name] = m
    betas = np.zeros(games, np.float32)
    runs = {name: [] for name in nets}
    for rep in range(repeats + 1):
        for name, m in searches.items():
            m.new_openings(np.arange(games) % 16)       # every repeat searches the same trees
            m.simulate(betas, 20)
            m.sync()
            s0, _ = m.counters()
            t0 = time.perf_counter()
            m.simulate(betas, sims)
            m.sync()
            dt = time.perf_counter() - t0
            s1, _ = m.counters()
            if rep:
                runs[name].append((s1 - s0) / dt)
    out["search_sims_per_s"][str(games)] = {name: summary(r) for name, r in runs.items()}
    print("%4d games: " % games + ", ".join("%s %.0f simulations/s (spread %.0f)" % (n, np.median(r), max(r) - min(r)) for n, r in runs.items()))
    for m in searches.values():
        del m
    searches.clear()

os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "lcghash_rate.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps({k: out[k] for k in ("kernel_us", "search_sims_per_s")}))
