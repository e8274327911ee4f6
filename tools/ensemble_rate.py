"""What net4_ensemble costs beside net4_simhash (the same trunk with the SimHash side kernel instead of the sixteen heads), on one
device in one process, the two archs interleaved, `repeats` times after a dropped warm-up pass:

  * the forward (forward_raw: upload, every launch of tz_net_forward_device, read-back; wall clock over `iters` calls) at 128 and 4096
    4x4 positions - the difference of the two archs is the ensemble heads' launch plus the fused kernel's store of its last image,
    against the SimHash kernel;
  * lock-step search (PUCT, random-init nets, f16) at 64 and 4096 games, simulations/s;
  * the learn step at batch 128, net4_ensemble armed (tz_trainer_set_ensemble_targets) against unarmed, ms per step.

Writes profiles/ensemble_rate.json with every repeat, the medians and the repeat-to-repeat spread (max - min), and prints the README's
table row.
python tools/ensemble_rate.py [repeats] [sims]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import takzero_amd.api as A
from takzero_amd import learn as L
from takzero_amd import weights as W
from takzero_amd.precision import sample_positions

repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
sims = int(sys.argv[2]) if len(sys.argv) > 2 else 200
ARCHS = (("net4_ensemble", A.ARCH_NET4_ENSEMBLE, W.ARCH_NET4_ENSEMBLE), ("net4_simhash", A.ARCH_NET4_SIMHASH, W.ARCH_NET4_SIMHASH))
nets = {name: A.Net(arch=a).load_tensors(W.init_weights(w, seed=123)) for name, a, w in ARCHS}


def summary(xs):
    return {"runs": [float(x) for x in xs], "median": float(np.median(xs)), "spread": float(max(xs) - min(xs))}


out = {"repeats": repeats, "sims": sims, "forward_us": {}, "search_sims_per_s": {}, "learn_step_ms": {}}
positions = sample_positions(4, 4, 4096, seed=11, plies=12)
for batch, iters in ((128, 200), (4096, 40)):
    st = A._states(positions[:batch])
    runs = {name: [] for name in nets}
    for rep in range(repeats + 1):                      # the first pass warms both up and is dropped
        for name, net in nets.items():
            net.forward_raw(st)
            t0 = time.perf_counter()
            for _ in range(iters):
                net.forward_raw(st)
            if rep:
                runs[name].append(1e6 * (time.perf_counter() - t0) / iters)
    out["forward_us"][str(batch)] = {name: summary(r) for name, r in runs.items()}
    print("%4d positions: " % batch + ", ".join("%s %.1f us (spread %.1f)" % (n, np.median(r), max(r) - min(r)) for n, r in runs.items()))

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
        m.close()
    searches.clear()
for net in nets.values():
    net.close()

# the learn step at batch 128: one trainer of the architecture, armed and unarmed in turn (apply = 0: the same weights every time)
B = 128
tr = L.Trainer(arch=A.ARCH_NET4_ENSEMBLE, batch=B).load_tensors(W.init_weights(W.ARCH_NET4_ENSEMBLE, seed=123))
rng = np.random.default_rng(3)
st = A._states(positions[:B])
size = A.policy_size(4)
policy = rng.random((B, size)).astype(np.float32)
policy /= policy.sum(axis=1, keepdims=True)
mask = np.zeros((B, size), np.uint8)
value, ube = rng.uniform(-1, 1, B).astype(np.float32), rng.uniform(0.1, 3.0, B).astype(np.float32)
targets = rng.uniform(-0.9, 0.9, (B, A.ENSEMBLE_SIZE)).astype(np.float32)
runs = {"armed": [], "unarmed": []}
for rep in range(repeats + 1):
    for name in runs:
        tr.set_ensemble_targets(targets if name == "armed" else None)
        tr.step(st, policy, mask, value, ube, apply=False)
        t0 = time.perf_counter()
        for _ in range(10):
            tr.step(st, policy, mask, value, ube, apply=False)
        if rep:
            runs[name].append(1e3 * (time.perf_counter() - t0) / 10)
out["learn_step_ms"][str(B)] = {name: summary(r) for name, r in runs.items()}
print(" learn step, batch %d: " % B + ", ".join("%s %.3f ms (spread %.3f)" % (n, np.median(r), max(r) - min(r)) for n, r in runs.items()))
tr.close()

os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "ensemble_rate.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
med = lambda group, key, name: out[group][key][name]["median"]
print("| net4_ensemble against net4_simhash | forward %.0f / %.0f us at 128, %.0f / %.0f us at 4096 positions | search %.0f k / %.0f k simulations/s at 64 games, "
      "%.3f M / %.3f M at 4096 | learn step armed %.2f ms, unarmed %.2f ms at batch 128 |" % (
          med("forward_us", "128", "net4_ensemble"), med("forward_us", "128", "net4_simhash"), med("forward_us", "4096", "net4_ensemble"),
          med("forward_us", "4096", "net4_simhash"), med("search_sims_per_s", "64", "net4_ensemble") / 1e3, med("search_sims_per_s", "64", "net4_simhash") / 1e3,
          med("search_sims_per_s", "4096", "net4_ensemble") / 1e6, med("search_sims_per_s", "4096", "net4_simhash") / 1e6,
          med("learn_step_ms", str(B), "armed"), med("learn_step_ms", str(B), "unarmed")))
