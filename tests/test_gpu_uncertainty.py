"""The net5 variance against an fp64 reference, in every precision.

The variance is clamp(max(exp(ube), local), 0, 4) with local = clamp((raw - min) / (max - min), 0, 1) * 4 and raw the squared
distance of the two RND MLPs' outputs (net5.rs:193-211,271-278).  It feeds the search through the nodes' std_dev
(csrc/tz_tree.hip), so a wrong variance is a wrong move.  Random-init RND nets under the initial min 0 / max 1 give
local = 1.56-1.57 on every position, so the fixtures here (`rnd_fixture`) make the check sensitive:

  * ube.linear.weight = 0, ube.linear.bias = c: ube == c exactly, and the reference needs no trunk forward;
  * c at the 30th percentile of log(local): exp(ube) wins on some positions and loses on others;
  * "calibrated": min / max of update_rnd (learn/src/rnd_normalization.rs:74-78, restated in fp64 by nets_torch.rnd_calibrate),
    which magnify raw ~1400x - local spans (0, 4) and hits both clamps; "clamped": c = 2, where the variance clamps at 4.

Two checks per position.  The sharp one inverts the normalisation to recover the kernel's raw and holds it to the same arithmetic
rounded where the kernels store (nets_torch.rnd_raw_storage; fp64 nets_torch.rnd_raw for TZ_PREC_F32), which a wrong input
permutation, RND-input write or min would break by orders of magnitude.  The absolute one holds the variance to fp64 within the
storage type's own error."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import oracle_lib as O
from gpu_util import random_positions, require_gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAXIMUM_VARIANCE = 4.0
PRECISIONS = ("f32", "bf16", "f16", "f16x2", "f16c8", "f16c6")
# 32- and 128-row tile tails of the RND layers, the several-CU / one-CU switch at 256, the full-size workgroups past 1024
BATCHES = (1, 31, 32, 33, 128, 129, 256, 257, 1025)
# |raw implied by the variance - raw of the reference arithmetic|: what is left is the kernels' fp32 accumulation against the
# reference's fp64 one, where it moves a stored h1 / h2 element across a rounding boundary.  torch's fp32 GEMMs in place of fp64 give
# 3.4e-6 (fp16 storage) and 1.2e-5 (bf16) on the fixture's positions: the bf16 bound is a property of the storage type, as its
# absolute error below is.  Measured on the MI355X: f32 5.1e-8, fp16 storage 3.4e-6, bf16 4.7e-6
SHARP_RAW_TOL = {"f32": 5e-7, "f16": 4e-6, "bf16": 1e-5}
# |variance - fp64 variance|, per fixture and storage type; measured on the MI355X (every fp16-storage precision alike):
#   deployed    f32 2.1e-7, fp16 5.6e-5, bf16 3.5e-4
#   calibrated  f32 6.6e-5, fp16 1.8e-2, bf16 0.11  (raw magnified ~1400x: fp16 / bf16 storage's own error, not a kernel's)
ABS_TOL = {("deployed", "f32"): 1e-6, ("deployed", "f16"): 1.5e-4, ("deployed", "bf16"): 1e-3,
           ("calibrated", "f32"): 2e-4, ("calibrated", "f16"): 2.5e-2, ("calibrated", "bf16"): 0.2}

_FIXTURES = {}


def storage_of(prec):
    """The RND path's arithmetic: fp32 FMA, or 16-bit storage (every fp16-storage precision runs the fp16 RND kernels)."""
    return prec if prec in ("f32", "bf16") else "f16"


def reference_positions(oracle, ply, count, rng):
    """random_env / reference_games (learn/src/rnd_normalization.rs:24-58): `ply + i % 2` random moves from the start, fewer only
    if a position has no move."""
    out = []
    for i in range(count):
        s = O.state_default(oracle, 5, 4)
        for _ in range(ply + i % 2):
            moves = O.possible_moves(oracle, s)
            if not moves:
                break
            s = O.play(oracle, s, moves[int(rng.integers(len(moves)))])
        out.append(s)
    return out


def _planes(oracle, states):
    return np.stack([O.game_repr(oracle, s) for s in states]).reshape(len(states), -1, 5, 5)


def local_of(raw, mn, mx):
    """local = clamp((raw - min) / (max - min), 0, 1) * 4 in fp64 (numpy's clip maps +-inf like torch's clamp)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.clip((raw - mn) / (mx - mn), 0.0, 1.0) * MAXIMUM_VARIANCE


def variance_of(raw, mn, mx, c):
    return np.clip(np.maximum(np.exp(np.float64(c)), local_of(raw, mn, mx)), 0.0, MAXIMUM_VARIANCE)


def _base(oracle):
    if "base" not in _FIXTURES:
        import nets_torch as T
        import torch
        from takzero_amd import weights as W

        w = W.init_weights(W.ARCH_NET5, seed=42)
        rng = np.random.default_rng(77)
        early = _planes(oracle, reference_positions(oracle, 4, 256, rng))
        late = _planes(oracle, reference_positions(oracle, 120, 256, rng))
        # positions of every stage (ply 0-130); ~0.5 % of late positions lie above the calibrated max, so the 24 of largest raw
        # out of 3000 more late ones are spread through the set, where every batch but the smallest meets some
        states = random_positions(oracle, O, 5, 4, max(BATCHES), 1234, max_ply=130)
        pool = reference_positions(oracle, 120, 3000, rng)
        top = np.argsort(T.rnd_raw(w, _planes(oracle, pool), torch.float64).numpy())[-24:]
        for at, i in zip(np.linspace(20, max(BATCHES) - 1, 24).astype(int), top):
            states[at] = pool[i]
        planes = _planes(oracle, states)
        _FIXTURES["base"] = dict(
            w=w, states=states, arr=O.states_array(states), acts=[O.possible_moves(oracle, s) for s in states],
            raw={"f32": T.rnd_raw(w, planes, torch.float64).numpy(), "f16": T.rnd_raw_storage(w, planes, torch.float16).numpy(),
                 "bf16": T.rnd_raw_storage(w, planes, torch.bfloat16).numpy()},
            calibration=T.rnd_calibrate(w, early, late))
    return _FIXTURES["base"]


def rnd_fixture(oracle, kind):
    """Net5 weights whose variance depends on the position, with the positions and their reference raw.

    kind: "deployed" (min 0 / max 1, as every net is initialised and the deployed trainer leaves it), "calibrated" (min / max from
    update_rnd), "clamped" (calibrated with c = 2: exp(2) > 4).  Returns dict(w, arr, acts, raw={"f32": fp64 graph, "f16" / "bf16":
    storage-rounded}, mn, mx, c) with mn, mx, c the float32 values the network holds.  Asserts its own coverage."""
    key = "fixture-" + kind
    if key in _FIXTURES:
        return _FIXTURES[key]
    base = _base(oracle)
    raw = base["raw"]["f32"]
    mn, mx = (0.0, 1.0) if kind == "deployed" else base["calibration"]
    mn, mx = float(np.float32(mn)), float(np.float32(mx))
    local = local_of(raw, mn, mx)
    inside = (local > 0) & (local < MAXIMUM_VARIANCE)
    assert inside.sum() >= 100, (kind, int(inside.sum()))
    if kind == "clamped":
        c = 2.0
        assert np.exp(c) > MAXIMUM_VARIANCE
    else:
        c = float(np.float32(np.percentile(np.log(local[local > 0]), 30)))
        wins = np.exp(c) > local
        assert wins.sum() >= 50 and (~wins & inside).sum() >= 50, (kind, int(wins.sum()))
    if kind != "deployed":      # under min 0 / max 1 raw (~0.39) is far from both clamps
        assert (local == 0).sum() >= 5 and (local == MAXIMUM_VARIANCE).sum() >= 5, (kind, int((local == 0).sum()), int((local == 4).sum()))
    w = dict(base["w"])
    w["ube.linear.weight"] = np.zeros_like(w["ube.linear.weight"])
    w["ube.linear.bias"] = np.full(1, c, np.float32)
    w["min"] = np.full(1, mn, np.float32)
    w["max"] = np.full(1, mx, np.float32)
    _FIXTURES[key] = dict(w=w, arr=base["arr"], acts=base["acts"], raw=base["raw"], mn=mn, mx=mx, c=c)
    return _FIXTURES[key]


def implied_raw(var, mn, mx):
    """raw recovered from a variance that local decided: variance = (raw - min) / (max - min) * 4."""
    return mn + var.astype(np.float64) / MAXIMUM_VARIANCE * (mx - mn)


def sharp_check(var, raw_ref, mn, mx, c, tol):
    """Where local (by the reference arithmetic) is inside (0, 4) and beats exp(c) by more than `tol` in raw: the raw implied by the
    variance, off raw_ref by at most `tol` (asserted by the caller).  Where exp(c) wins by that much: variance == expf(c) to its last
    bits.  Returns (max raw error, positions checked by raw)."""
    eps = 2 * tol * MAXIMUM_VARIANCE / abs(mx - mn)          # the tolerance in local's units, twice
    local = local_of(raw_ref, mn, mx)
    ec = np.exp(np.float64(np.float32(c)))
    by_raw = (local > eps) & (local < MAXIMUM_VARIANCE - eps) & (local > ec + eps)
    err = np.abs(implied_raw(var[by_raw], mn, mx) - raw_ref[by_raw])
    by_exp = local < ec - eps
    assert np.allclose(var[by_exp], ec, rtol=1e-6, atol=0), np.abs(var[by_exp] - ec).max()
    return (float(err.max()) if err.size else 0.0), int(by_raw.sum())


# ---------------------------------------------------------------------------------------------- CPU: the reference itself


def test_rnd_raw_fp32_agrees_with_fp64(oracle):
    import nets_torch as T
    import torch
    from takzero_amd import weights as W

    w = W.init_weights(W.ARCH_NET5, seed=3)
    planes = _planes(oracle, random_positions(oracle, O, 5, 4, 64, 5, max_ply=60))
    r32 = T.rnd_raw(w, planes, torch.float32).numpy().astype(np.float64)
    r64 = T.rnd_raw(w, planes, torch.float64).numpy()
    assert r64.dtype == np.float64 and np.all(r64 > 0)
    assert np.abs(r32 - r64).max() <= 1e-6 * np.abs(r64).max()
    # the fp32 graph is the one nets_torch.rnd normalises
    local = T.rnd(w, planes).numpy()
    assert np.abs(local - local_of(r64, 0.0, 1.0)).max() < 1e-5


def test_rnd_raw_storage_rounds_where_the_kernels_store(oracle):
    """The 16-bit emulation is not the fp64 graph (it rounds), and its fp16 error is well under its bf16 error."""
    import nets_torch as T
    import torch
    from takzero_amd import weights as W

    w = W.init_weights(W.ARCH_NET5, seed=3)
    planes = _planes(oracle, random_positions(oracle, O, 5, 4, 64, 5, max_ply=60))
    r64 = T.rnd_raw(w, planes, torch.float64).numpy()
    e16 = np.abs(T.rnd_raw_storage(w, planes, torch.float16).numpy() - r64).max()
    ebf = np.abs(T.rnd_raw_storage(w, planes, torch.bfloat16).numpy() - r64).max()
    print("raw: fp16 storage %.3g, bf16 storage %.3g off fp64" % (e16, ebf))
    assert 1e-7 < e16 < 1e-4 and 4 * e16 < ebf < 1e-3


def test_rnd_calibrate_takes_min_over_early_and_max_over_late(oracle):
    import nets_torch as T
    import torch
    from takzero_amd import weights as W

    w = W.init_weights(W.ARCH_NET5, seed=42)
    rng = np.random.default_rng(5)
    early_states = reference_positions(oracle, 4, 16, rng)
    late_states = reference_positions(oracle, 120, 16, rng)
    assert [s.ply for s in early_states] == [4 + i % 2 for i in range(16)]
    early, late = _planes(oracle, early_states), _planes(oracle, late_states)
    re, rl = T.rnd_raw(w, early, torch.float64).numpy(), T.rnd_raw(w, late, torch.float64).numpy()
    mn, mx = T.rnd_calibrate(w, early, late)
    assert mn == re.min() and mx == rl.max()
    assert (mn, mx) != T.rnd_calibrate(w, late, early)
    assert mn < mx


@pytest.mark.parametrize("kind", ["deployed", "calibrated", "clamped"])
def test_fixture_coverage(oracle, kind):
    """rnd_fixture asserts its coverage; this runs it without a GPU and checks the weights it hands out."""
    f = rnd_fixture(oracle, kind)
    assert not f["w"]["ube.linear.weight"].any() and f["w"]["ube.linear.bias"][0] == np.float32(f["c"])
    assert f["w"]["min"][0] == np.float32(f["mn"]) and f["w"]["max"][0] == np.float32(f["mx"])
    if kind == "calibrated":
        span = f["mx"] - f["mn"]
        print("calibrated min %.6f max %.6f span %.3g; c = %.4f" % (f["mn"], f["mx"], span, f["c"]))
        assert 0 < span < 0.05


# ---------------------------------------------------------------------------------------------- GPU


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["deployed", "calibrated", "clamped"])
@pytest.mark.parametrize("prec", PRECISIONS)
def test_variance_against_fp64(oracle, prec, kind):
    """Every batch size through policy_value_uncertainty (tz_net_eval): ube == c bit for bit, the sharp raw check and the absolute
    variance check, with the bounds and measured figures above (SHARP_RAW_TOL, ABS_TOL)."""
    A = require_gpu()
    f = rnd_fixture(oracle, kind)
    st = storage_of(prec)
    net = A.Net(arch=A.ARCH_NET5, precision=A.PREC_NAMES[prec]).load_tensors(f["w"])
    want = variance_of(f["raw"]["f32"], f["mn"], f["mx"], f["c"])
    worst_abs, worst_raw, checked, failed = 0.0, 0.0, 0, []
    for B in BATCHES:
        arr, acts = f["arr"][:B], f["acts"][:B]
        ube = net.forward_raw(arr)[2]
        assert np.all(ube == np.float32(f["c"])), (B, ube[ube != np.float32(f["c"])][:4])
        var = net.policy_value_uncertainty(arr, acts)[2]
        assert np.all(np.isfinite(var)), B
        if kind == "clamped":
            assert np.all(var == np.float32(MAXIMUM_VARIANCE)), B
            continue
        r, n = sharp_check(var, f["raw"][st][:B], f["mn"], f["mx"], f["c"], SHARP_RAW_TOL[st])
        a = float(np.abs(var - want[:B]).max())
        if r > SHARP_RAW_TOL[st] or a > ABS_TOL[(kind, st)]:
            failed.append((B, r, a))
        worst_raw, worst_abs, checked = max(worst_raw, r), max(worst_abs, a), checked + n
    net.close()
    print("%s %s: variance %.3g off fp64 (bound %.3g); raw %.3g off the %s reference arithmetic (bound %.3g) over %d positions" %
          (prec, kind, worst_abs, ABS_TOL.get((kind, st), 0), worst_raw, st, SHARP_RAW_TOL[st], checked))
    assert not failed, failed
    if kind != "clamped":
        assert checked >= 500


_CHILD = ("import sys, numpy as np; sys.path[:0] = [%r]; import takzero_amd.api as A\n"
          "d = np.load(sys.argv[1], allow_pickle=True); arr = d['arr'].view(A._lib.STATE_DTYPE).reshape(-1); acts = list(d['acts'])\n"
          "net = A.Net(arch=A.ARCH_NET5, precision=int(sys.argv[2])).load(sys.argv[3])\n"
          "np.savez(sys.argv[4], **{'u%%d' %% B: net.policy_value_uncertainty(arr[:B], acts[:B])[2] for B in (257, 1025)})\n")


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["f16", "f16x2", "f16c6"])
def test_rnd_prep_kernel_gives_the_variance_bits_of_the_fused_write(oracle, prec):
    """Past 256 positions the fused trunk kernel (net_mfma_kernel; tz_nn_c6.hip for f16c6) writes the RND input while it builds its
    planes; TZ_RND_PREP_KERNEL=1 makes rnd_prep_state_kernel write it instead.  Same variance bits either way, on the calibrated
    fixture (1400x magnification of raw)."""
    from takzero_amd import weights as W

    A = require_gpu()
    f = rnd_fixture(oracle, "calibrated")
    net = A.Net(arch=A.ARCH_NET5, precision=A.PREC_NAMES[prec]).load_tensors(f["w"])
    fused = {B: net.policy_value_uncertainty(f["arr"][:B], f["acts"][:B])[2] for B in (257, 1025)}
    net.close()
    with tempfile.TemporaryDirectory() as d:
        W.save_tzw(os.path.join(d, "w.tzw"), f["w"])
        np.savez(os.path.join(d, "in.npz"), arr=np.frombuffer(f["arr"].tobytes(), np.uint8), acts=np.array(f["acts"], dtype=object))
        r = subprocess.run([sys.executable, "-c", _CHILD % ROOT, os.path.join(d, "in.npz"), str(A.PREC_NAMES[prec]),
                            os.path.join(d, "w.tzw"), os.path.join(d, "out.npz")],
                           env=dict(os.environ, TZ_RND_PREP_KERNEL="1"), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-1500:]
        prep = np.load(os.path.join(d, "out.npz"))
        for B in (257, 1025):
            differ = fused[B].view(np.uint32) != prep["u%d" % B].view(np.uint32)
            assert not differ.any(), (prec, B, int(differ.sum()), float(np.abs(fused[B] - prep["u%d" % B]).max()))


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["f32", "f16"])
def test_normalisation_edges(oracle, prec):
    """rnd_finish_kernel where max - min is not a positive span: min > max (the normalisation inverted), and min == max with raw on
    either side of it (+-inf clamped to 4 and 0).  Against the same formula in fp64."""
    A = require_gpu()
    f = rnd_fixture(oracle, "calibrated")
    st = storage_of(prec)
    raw = f["raw"][st]
    B = 300
    for mn, mx in ((f["mx"], f["mn"]), (float(np.float32(np.median(raw[:B]))),) * 2):
        w = dict(f["w"], min=np.full(1, mn, np.float32), max=np.full(1, mx, np.float32))
        net = A.Net(arch=A.ARCH_NET5, precision=A.PREC_NAMES[prec]).load_tensors(w)
        var = net.policy_value_uncertainty(f["arr"][:B], f["acts"][:B])[2]
        net.close()
        if mn != mx:
            r, n = sharp_check(var, raw[:B], mn, mx, f["c"], SHARP_RAW_TOL[st])
            print("%s, min > max: raw %.3g off over %d positions" % (prec, r, n))
            assert r <= SHARP_RAW_TOL[st] and n >= 50
        else:
            far = np.abs(raw[:B] - mn) > SHARP_RAW_TOL[st]
            want = variance_of(raw[:B], mn, mx, f["c"])
            assert np.all(np.isin(want[far], (np.exp(np.float64(np.float32(f["c"]))), MAXIMUM_VARIANCE)))
            assert np.allclose(var[far], want[far], rtol=1e-6, atol=0), np.abs(var[far] - want[far]).max()
            assert (want[far] == MAXIMUM_VARIANCE).sum() >= 50 and (want[far] < MAXIMUM_VARIANCE).sum() >= 50
