"""What the RND towers of net4_rnd cost beside net4_simhash, on one device in one process, the two archs interleaved, `repeats` times:

  * the tower kernel alone (rnd4_tower_mfma_kernel through tz_debug_rnd4_bench: HIP events around `iters` launches) at 128 and 4096
    4x4 positions, beside SimHash's index-plus-lookup kernel (tz_debug_hash_bench);
  * forward_raw (upload, trunk, heads, the uncertainty kernel, download) at 128 and 4096 positions, microseconds per call;
  * lock-step search (PUCT, random-init nets, f16) at 64 and 4096 games, simulations/s.

Writes profiles/rnd4_rate.json with every repeat, the medians and the repeat-to-repeat spread (max - min).
python tools/rnd4_rate.py [repeats] [sims]"""
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
ARCHS = (("net4_rnd", A.ARCH_NET4_RND, W.ARCH_NET4_RND), ("net4_simhash", A.ARCH_NET4_SIMHASH, W.ARCH_NET4_SIMHASH))
nets = {name: A.Net(arch=a).load_tensors(W.init_weights(w, seed=123)) for name, a, w in ARCHS}
BENCH = {"net4_rnd": "tz_debug_rnd4_bench", "net4_simhash": "tz_debug_hash_bench"}


def summary(xs):
    return {"runs": [float(x) for x in xs], "median": float(np.median(xs)), "spread": float(max(xs) - min(xs))}


out = {"repeats": repeats, "sims": sims, "kernel_us": {}, "forward_raw_us": {}, "search_sims_per_s": {}}
positions = sample_positions(4, 4, 4096, seed=11, plies=12)
for batch in (128, 4096):
    st = A._states(positions[:batch])
    runs = {name: [] for name in nets}
    fwd = {name: [] for name in nets}
    for rep in range(repeats + 1):                      # the first pass warms both up and is dropped
        for name, net in nets.items():
            ms = C.c_float()
            A.check(getattr(net.lib, BENCH[name])(net.h, batch, st.ctypes.data, 200, C.byref(ms)))
            net.forward_raw(st)
            t0 = time.perf_counter()
            for _ in range(20):
                net.forward_raw(st)
            dt = (time.perf_counter() - t0) / 20
            if rep:
                runs[name].append(1000.0 * ms.value)
                fwd[name].append(1e6 * dt)
    out["kernel_us"][str(batch)] = {name: summary(r) for name, r in runs.items()}
    out["forward_raw_us"][str(batch)] = {name: summary(r) for name, r in fwd.items()}
    print("%4d positions, uncertainty kernel: " % batch + ", ".join("%s %.2f us (spread %.2f)" % (n, np.median(r), max(r) - min(r)) for n, r in runs.items()))
    print("%4d positions, forward_raw: " % batch + ", ".join("%s %.1f us (spread %.1f)" % (n, np.median(r), max(r) - min(r)) for n, r in fwd.items()))

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
with open(os.path.join(ROOT, "profiles", "rnd4_rate.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
print(json.dumps({k: out[k] for k in ("kernel_us", "forward_raw_us", "search_sims_per_s")}))
