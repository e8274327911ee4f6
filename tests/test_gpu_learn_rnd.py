"""Training net5's RND predictor in the learn step (csrc/tz_learn.hip, tz_trainer_rnd_*; net5.rs:193-218, learn/src/main.rs:404-405,
415-416) against fp64 autograd (tests/rnd_ref.py), by the method of test_gpu_learn_fp64.py: the step layer by layer, that nothing else
moves, apply=False and Adam's own step count, bit reproducibility, the falling loss, calibration, the hand-off to the inference net
and the native loop.  The trainer is net5 (its trunk is always 20 blocks deep; the RND path does not see it) at batch 64: one row
tile, K = 800 padded to 832, the NCHW / NHWC order; one case at the shipped batch of 128, two row tiles."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import oracle_lib as O
from gpu_util import random_positions, require_gpu
from test_gpu_learn import _batch
from test_gpu_learn_fp64 import FORCED_MAX, KINK_FACTOR, TOL, _outputs, _rel, _snapshot

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

LR = 1e-4
# |trainer - fp64| in the units of test_gpu_learn_fp64.TOL; each bound is the worst value measured on an MI355X over both cases of
# test_step_matches_fp64_autograd (3 steps each) times at most 4, and none is looser than that file's random-init column (checked
# below).  The MLP's sums are at most 1024 long.
RND_TOL = {
    # both hidden activations and the output of both MLPs, relative to the layer's largest entry       measured 2.13e-7 (batch 64)
    "activation": 8e-7,
    # raw[b] relative to the largest raw of the batch                                                   measured 1.22e-7 (batch 64)
    "raw": 4.5e-7,
    # |loss_rnd - fp64| / (1 + |fp64|): half an ulp of a loss of 0.4 is 1.1e-8 in these units          measured 9.55e-9 (batch 128)
    "loss": 3.8e-8,
    # each of the six gradients, relative to the tensor's largest fp64 entry                            measured 2.53e-7 (batch 128)
    "gradient": 1e-6,
    # Adam's first moment against torch.optim.Adam's exp_avg, relative to the largest entry             measured 4.06e-7 (batch 128)
    "adam m": 1.6e-6,
    # ... the second against exp_avg_sq (1 - 0.999f is 1.3e-5 off 0.001)                                measured 1.32e-5 (batch 64)
    "adam v": 5e-5,
    # the update against Adam applied in fp64 to the trainer's own moments, in units of lr               measured 2.88e-5 (both)
    "adam update / lr": 1.15e-4,
    # weights after the step against torch's, 99th percentile of |diff| in units of lr                  measured 1.83e-5 (both)
    "weights q99 / lr": 7.3e-5,
    # ... and the largest |diff| in lr (no weight of the MLP has a gradient near zero on these batches)  measured 1.94e-3 (batch 128)
    "weights max / lr": 7.7e-3,
}
_SAME_AS = {"raw": "output"}
for _k, _v in RND_TOL.items():
    assert _v <= TOL[_SAME_AS.get(_k, _k)][0], _k

_CACHE = {}


def _weights():
    from takzero_amd import weights as W

    if "w" not in _CACHE:
        _CACHE["w"] = W.init_weights(W.ARCH_NET5, blocks=1, seed=91, trained_stats=True)
    return _CACHE["w"]


def _batches(oracle, B):
    if ("batches", B) not in _CACHE:
        _CACHE[("batches", B)] = [_batch(oracle, 5, B, 1500 + 10 * B + step) for step in range(3)]
    return _CACHE[("batches", B)]


def _trainer(B, enable=True, w=None):
    A = require_gpu()
    from takzero_amd import learn as L

    tr = L.Trainer(arch=A.ARCH_NET5, batch=B, lr=LR).load_tensors(_weights() if w is None else w)
    return tr.rnd_enable() if enable else tr


def _planes(oracle, states):
    return np.stack([O.game_repr(oracle, s) for s in states]).reshape(len(states), -1, 5, 5)


def _calibration_sets(oracle):
    """70 early positions (ply <= 5) and 64 late ones (ply >= 60): one count is no multiple of the batch"""
    if "cal" not in _CACHE:
        early = random_positions(oracle, O, 5, 4, 70, 31, min_ply=0, max_ply=5)
        late = random_positions(oracle, O, 5, 4, 64, 32, min_ply=60, max_ply=90)
        _CACHE["cal"] = (O.states_array(early), _planes(oracle, early), O.states_array(late), _planes(oracle, late))
    return _CACHE["cal"]


def _rnd_snapshot(tr):
    from takzero_amd import learn as L

    loss, raw = tr.rnd_last()
    out = {"loss": np.float32(loss), "raw": raw}
    for net in range(2):
        for layer in range(3):
            out["activation %d %d" % (net, layer)] = tr.rnd_activation(net, layer)
    for k in tr.RND_NAMES:
        for what in (L.PARAM, L.GRAD, L.ADAM_M, L.ADAM_V):
            out["%s %d" % (k, what)] = tr.tensor(k, what)
    return out


@pytest.mark.parametrize("B", [64, 128])
def test_step_matches_fp64_autograd(B):
    import rnd_ref as R
    import torch
    from takzero_amd import learn as L

    oracle = O.load()
    w = _weights()
    tr = _trainer(B)
    p = R.make_params(w)
    opt = R.adam(p, LR)
    worst = {}

    def note(key, value, bound=None):
        worst[key] = max(worst.get(key, 0.0), value)
        return value <= (RND_TOL[key] if bound is None else bound)

    for step, train_ube in enumerate((True, False, True)):
        states, planes, policy, mask, value, ube = _batches(oracle, B)[step]
        before = {k: tr.tensor(k) for k in tr.RND_NAMES}
        tr.step(states, policy, mask, value, ube, train_ube=train_ube, apply=True)
        loss, raw = tr.rnd_last()
        acts = [[tr.rnd_activation(net, layer) for layer in range(3)] for net in range(2)]
        after = {k: tr.tensor(k) for k in tr.RND_NAMES}
        grads = {k: tr.tensor(k, L.GRAD) for k in tr.RND_NAMES}
        m1 = {k: tr.tensor(k, L.ADAM_M) for k in tr.RND_NAMES}
        m2 = {k: tr.tensor(k, L.ADAM_V) for k in tr.RND_NAMES}

        # activations against the plain fp64 forward; the predictor's hidden layers give the kink thresholds
        with torch.no_grad():
            plain = R.forward_rnd(p, planes)[1]
        kinks = []
        for net in range(2):
            for layer in range(3):
                ref = plain[net][layer][1].numpy()
                err = float(np.abs(acts[net][layer] - ref).max())
                rel = err / float(np.abs(ref).max())
                assert note("activation", rel), (step, net, layer, rel)
                if net == 0 and layer < 2:
                    kinks.append(KINK_FACTOR * err)

        # the step's graph in fp64, the two hidden ReLUs' kinks decided as the trainer did within each layer's own threshold
        opt.zero_grad(set_to_none=True)
        masks = [torch.from_numpy(acts[0][layer] > 0) for layer in range(2)]
        raw_t, layers = R.forward_rnd(p, planes, masks, kinks)
        loss_t = raw_t.mean()
        loss_t.backward()
        forced = []
        for layer in range(2):
            pre = layers[0][layer][0].detach()
            near = pre.abs() < kinks[layer]
            forced.append((int(near.sum()), int((near & ((pre > 0) != masks[layer])).sum())))
            assert note("forced fraction", float(near.sum()) / near.numel(), FORCED_MAX), (step, layer, kinks[layer])
        print("B %d step %d: forced ReLU entries per hidden layer (within the kink, of them on the other side): %s" % (B, step, forced))

        assert note("raw", _rel(raw, raw_t.detach().numpy())), (step, "raw")
        lt = float(loss_t.detach())
        assert note("loss", abs(loss - lt) / (1 + abs(lt))), (step, loss, lt)
        for k in tr.RND_NAMES:
            rel = _rel(grads[k], p[k].grad.numpy())
            assert note("gradient", rel), (step, k, rel)
        opt.step()
        for k in tr.RND_NAMES:
            st = opt.state[p[k]]
            assert int(st["step"]) == step + 1
            for what, got_m, key in (("adam m", m1[k], "exp_avg"), ("adam v", m2[k], "exp_avg_sq")):
                rel = _rel(got_m, st[key].numpy())
                assert note(what, rel), (step, k, what, rel)
            t = step + 1
            m, v = m1[k].astype(np.float64), m2[k].astype(np.float64)
            exact = before[k] - LR / (1 - 0.9 ** t) * m / (np.sqrt(v) / np.sqrt(1 - 0.999 ** t) + 1e-8)
            err = float(np.abs(after[k] - exact).max()) / LR
            assert note("adam update / lr", err), (step, k, err)
            diff = np.abs(after[k] - p[k].detach().numpy()) / LR
            q99 = float(np.quantile(diff, 0.99))
            assert note("weights q99 / lr", q99), (step, k, q99)
            assert note("weights max / lr", float(diff.max())), (step, k, float(diff.max()))
        # both sides go on from the trainer's weights, torch's Adam state stays its own (as in test_gpu_learn_fp64.py)
        with torch.no_grad():
            for k in tr.RND_NAMES:
                p[k].copy_(torch.from_numpy(after[k]))
        # the frozen side keeps every bit
        held = tr.extras()
        for k in held:
            if k.startswith("rnd_target.") or k in ("min", "max"):
                assert np.array_equal(held[k], w[k]), k
    print("rnd B %d: worst over 3 steps: %s" % (B, ", ".join("%s %.3g" % kv for kv in sorted(worst.items()))))


def test_nothing_else_moves():
    """Two trainers, the same weights and batches, one with RND training enabled: every trained tensor in all four arenas, the three
    losses, the outputs and every trunk activation agree in every bit; the enabled one leaves rnd_target.*, min and max alone, the
    disabled one rnd_learning.* too."""
    oracle = O.load()
    w = _weights()
    B = 64
    on, off = _trainer(B, True), _trainer(B, False)
    assert list(on.names) == list(off.names) and not any(k.startswith("rnd_") for k in on.names)
    for step, train_ube in enumerate((True, False, True)):
        states, planes, policy, mask, value, ube = _batches(oracle, B)[step]
        snaps = [_snapshot(tr, tr.step(states, policy, mask, value, ube, train_ube=train_ube), 41) for tr in (on, off)]
        differ = [k for k in snaps[0] if not np.array_equal(snaps[0][k], snaps[1][k])]
        assert not differ, (step, differ[:8])
    held_on, held_off = on.tensors(), off.tensors()
    assert set(held_on) == set(held_off) == set(w)
    for k in w:
        if k.startswith("rnd_target.") or k in ("min", "max"):
            assert np.array_equal(held_on[k], w[k]) and np.array_equal(held_off[k], w[k]), k
        if k.startswith("rnd_learning."):
            assert np.array_equal(held_off[k], w[k]), k
            assert not np.array_equal(held_on[k], w[k]) and held_on[k].shape == w[k].shape, k
    from takzero_amd.api import TakzeroError

    with pytest.raises(TakzeroError):   # the predictor's names answer only while its training is enabled
        off.tensor("rnd_learning.final_linear.bias")


def test_apply_false_then_the_first_step_of_the_rnd_group():
    """Enabled after two plain steps (the trunk's Adam count is 2): apply=False leaves the predictor's weights and moments alone and
    gives gradients; the next step is torch Adam's step 1 on the trainer's gradients."""
    import rnd_ref as R
    import torch
    from takzero_amd import learn as L

    oracle = O.load()
    w = _weights()
    B = 64
    tr = _trainer(B, False)
    batches = _batches(oracle, B)
    for step in range(2):
        states, planes, policy, mask, value, ube = batches[step]
        tr.step(states, policy, mask, value, ube)
    tr.rnd_enable()
    states, planes, policy, mask, value, ube = batches[2]
    tr.step(states, policy, mask, value, ube, apply=False)
    for k in tr.RND_NAMES:
        assert np.array_equal(tr.tensor(k), w[k]), k
        assert not tr.tensor(k, L.ADAM_M).any() and not tr.tensor(k, L.ADAM_V).any(), k
        assert tr.tensor(k, L.GRAD).any(), k
    states, planes, policy, mask, value, ube = batches[0]
    tr.step(states, policy, mask, value, ube, apply=True)
    p = R.make_params(w)
    opt = R.adam(p, LR)
    for k in tr.RND_NAMES:
        p[k].grad = torch.from_numpy(tr.tensor(k, L.GRAD).astype(np.float64))
    opt.step()
    moments, update = 0.0, 0.0
    for k in tr.RND_NAMES:
        st = opt.state[p[k]]
        assert int(st["step"]) == 1
        for what, key in ((L.ADAM_M, "exp_avg"), (L.ADAM_V, "exp_avg_sq")):
            rel = _rel(tr.tensor(k, what), st[key].numpy())
            moments = max(moments, rel)
            # the same gradients on both sides: m = 0.1 g, v = 0.001 g^2 up to fp32 rounding; 1 - 0.999f is 1.3e-5 off 0.001
            # (test_gpu_learn_fp64.py holds the trunk to the same 4e-5)
            assert rel <= 4e-5, (k, what, rel)
        err = float(np.abs(tr.tensor(k) - p[k].detach().numpy()).max()) / LR
        update = max(update, err)
        assert err <= RND_TOL["adam update / lr"], (k, err)
    print("rnd first Adam step after two plain steps: moments within %.3g, weights within %.3g lr" % (moments, update))


def test_rnd_step_is_bit_reproducible():
    oracle = O.load()
    B = 64
    trs = [_trainer(B), _trainer(B)]
    for step, train_ube in enumerate((True, False, True)):
        states, planes, policy, mask, value, ube = _batches(oracle, B)[step]
        snaps = []
        for tr in trs:
            tr.step(states, policy, mask, value, ube, train_ube=train_ube)
            snaps.append(_rnd_snapshot(tr))
        differ = [k for k in snaps[0] if not np.array_equal(snaps[0][k], snaps[1][k])]
        assert not differ, (step, differ[:8])


def test_loss_falls_on_the_device_as_in_fp64():
    """The 20-step run of test_learn_rnd_host.py on the trainer (train_ube=False; the trunk does not reach the RND path): loss_rnd
    falls at every step, and the value before step k lies within (k + 1) x the loss bound of the fp64 trajectory (k + 1 forward
    passes have been taken when it is read).  Measured: 0.4098 -> 0.0501, worst error / (k + 1) 1.93e-8."""
    from test_learn_rnd_host import fp64_trajectory, rnd_inputs

    oracle = O.load()
    w, states, planes = rnd_inputs(oracle)
    B = 64
    rng = np.random.default_rng(5)
    out = (3 + 4 * 30) * 25
    policy, mask = np.zeros((B, out), np.float32), np.ones((B, out), np.uint8)
    for i, s in enumerate(states):
        mv = np.array(O.possible_moves(oracle, s), np.int64)
        policy[i, mv] = 1.0 / len(mv)
        mask[i, mv] = 0
    value, ube = rng.uniform(-1, 1, B).astype(np.float32), rng.uniform(0.1, 4, B).astype(np.float32)
    tr = _trainer(B, True, w)
    got = []
    for _ in range(20):
        tr.step(O.states_array(states), policy, mask, value, ube, train_ube=False)
        got.append(tr.rnd_last()[0])
    want = fp64_trajectory(w, planes)
    errs = [abs(g - t) / (1 + abs(t)) for g, t in zip(got, want)]
    print("rnd loss on the device: %.4f -> %.4f; |device - fp64| / (1 + |fp64|) / (k + 1), worst: %.3g"
          % (got[0], got[-1], max(e / (k + 1) for k, e in enumerate(errs))))
    assert all(b < a for a, b in zip(got, got[1:])), got
    for k, e in enumerate(errs):
        assert e <= RND_TOL["loss"] * (k + 1), (k, got[k], want[k], e)


def test_calibration():
    import nets_torch as T
    from takzero_amd import learn as L
    from takzero_amd.api import TakzeroError

    oracle = O.load()
    w = _weights()
    early, early_planes, late, late_planes = _calibration_sets(oracle)
    tr = _trainer(64)
    import torch

    scale = {"early": float(T.rnd_raw(w, early_planes, torch.float64).max()), "late": float(T.rnd_raw(w, late_planes, torch.float64).max())}
    mn, mx = tr.rnd_calibrate(early, late, apply=False)
    want = T.rnd_calibrate(w, early_planes, late_planes)
    print("rnd calibrate: got (%.8g, %.8g), fp64 (%.8g, %.8g)" % (mn, mx, want[0], want[1]))
    assert abs(mn - want[0]) <= RND_TOL["raw"] * scale["early"] and abs(mx - want[1]) <= RND_TOL["raw"] * scale["late"]
    held = tr.tensors()
    assert all(np.array_equal(held[k], w[k]) for k in w), [k for k in w if not np.array_equal(held[k], w[k])]
    other = T.rnd_calibrate(w, late_planes, early_planes)
    assert other[1] > other[0]   # a property of these positions: the swapped call is a valid calibration too
    mn2, mx2 = tr.rnd_calibrate(late, early, apply=False)
    assert abs(mn2 - other[0]) <= RND_TOL["raw"] * scale["late"] and abs(mx2 - other[1]) <= RND_TOL["raw"] * scale["early"]
    assert (mn2, mx2) != (mn, mx)
    assert tr.rnd_calibrate(early, late, apply=True) == (mn, mx)
    held = tr.tensors()
    assert held["min"].shape == (1,) and held["min"][0] == np.float32(mn) and held["max"][0] == np.float32(mx)
    with pytest.raises(TakzeroError) as e:
        tr.rnd_calibrate(early[:1], early[:1], apply=True)
    assert e.value.code == -6
    held = tr.tensors()
    assert held["min"][0] == np.float32(mn) and held["max"][0] == np.float32(mx)
    off = _trainer(64, False)
    with pytest.raises(TakzeroError) as e:
        off.rnd_calibrate(early, late, apply=False)
    assert e.value.code == -6


def test_trained_predictor_reaches_the_inference_net(tmp_path):
    """Three enabled steps and a calibration on the reference's sets (256 positions at ply 4 / 5, 256 at ply 120 / 121, what the bound
    of test_gpu_uncertainty.py was measured under): to_net, save as .ot and .tzw, Net.load_tensors(tensors()) and
    ot.save_ot(tensors()) give the same fp32 net, whose variance is that of nets_torch on tensors() (measured 4.2e-5 against the
    bound of 2e-4) and not that of the untrained predictor."""
    import nets_torch as T
    import torch
    from takzero_amd import ot
    from test_gpu_uncertainty import ABS_TOL, reference_positions

    A = require_gpu()
    oracle = O.load()
    w = _weights()
    B = 64
    tr = _trainer(B)
    for step in range(3):
        states, planes, policy, mask, value, ube = _batches(oracle, B)[step]
        tr.step(states, policy, mask, value, ube)
    rng = np.random.default_rng(77)
    early, late = reference_positions(oracle, 4, 256, rng), reference_positions(oracle, 120, 256, rng)
    late = [s for s in late if oracle.tzo_terminal(C.byref(s)) == -1]
    mn, mx = tr.rnd_calibrate(O.states_array(early), O.states_array(late), apply=True)
    held = tr.tensors()
    assert held["min"][0] == np.float32(mn) and held["max"][0] == np.float32(mx)
    routes = {"Net.load_tensors(tensors())": A.Net(arch=A.ARCH_NET5, precision=A.PREC_F32).load_tensors(held)}
    net = A.Net(arch=A.ARCH_NET5, precision=A.PREC_F32)
    tr.to_net(net)
    routes["to_net"] = net
    for ext in ("ot", "tzw"):
        path = str(tmp_path / ("model." + ext))
        tr.save(path)
        routes["save ." + ext] = A.Net(arch=A.ARCH_NET5, precision=A.PREC_F32).load(path)
    d = tmp_path / "py"
    d.mkdir()
    ot.save_ot(str(d / "model.ot"), held)
    routes["ot.save_ot(tensors())"] = A.Net(arch=A.ARCH_NET5, precision=A.PREC_F32).load(str(d / "model.ot"))
    fresh = random_positions(oracle, O, 5, 4, 96, 4321, max_ply=110)
    arr, planes = O.states_array(fresh), _planes(oracle, fresh)
    legal = [np.array(O.possible_moves(oracle, s)) for s in fresh]
    ref = None
    for route, n_ in routes.items():
        got = _outputs(A, n_, arr, legal)
        if ref is None:
            ref = got
        for i, (a, b) in enumerate(zip(got, ref)):
            assert np.array_equal(a, b), (route, i)
    ube_out, var = ref[2], ref[5]
    want = T.variance(held, planes, torch.from_numpy(np.asarray(ube_out, np.float32)), 5).numpy().astype(np.float64)
    err = float(np.abs(var - want).max())
    print("rnd hand-off: variance within %.3g of nets_torch on tensors(); min %.6g max %.6g" % (err, mn, mx))
    assert err <= ABS_TOL[("calibrated", "f32")], err
    untrained = dict(held)
    untrained.update({k: w[k] for k in tr.RND_NAMES})
    var0 = A.Net(arch=A.ARCH_NET5, precision=A.PREC_F32).load_tensors(untrained).policy_value_uncertainty(arr, legal)[2]
    assert float(np.abs(var0 - var).max()) > 100 * ABS_TOL[("calibrated", "f32")]


def _terminal(oracle, state):
    return oracle.tzo_terminal(C.byref(O.TzState.from_buffer_copy(state.tobytes()))) != -1


def test_reference_positions_from_a_dummy_search():
    A = require_gpu()
    from takzero_amd import learn as L

    oracle = O.load()
    mcts = A.BatchedMCTS(32, 5, 4, agent_kind=A.AGENT_DUMMY, node_capacity=1 << 10)
    early, late = L.rnd_reference(mcts, seed=9, n_early=40, early_ply=4, n_late=24, late_ply=60)   # 40 games: two waves of the handle
    again = L.rnd_reference(mcts, seed=9, n_early=40, early_ply=4, n_late=24, late_ply=60)
    assert early.tobytes() == again[0].tobytes() and late.tobytes() == again[1].tobytes()
    other = L.rnd_reference(mcts, seed=10, n_early=40, early_ply=4, n_late=24, late_ply=60)
    assert early.tobytes() != other[0].tobytes() and late.tobytes() != other[1].tobytes()
    assert len({e.tobytes() for e in early}) > 30   # the games differ from one another
    for states, ply in ((early, 4), (late, 60)):
        for i, s in enumerate(states):
            assert not _terminal(oracle, s), (ply, i)
            assert int(s["n"]) == 5 and int(s["half_komi"]) == 4
            if int(s["ply"]) != ply + i % 2:   # fewer only where the game ended: some move from here ends it
                assert int(s["ply"]) < ply + i % 2 and ply == 60, (ply, i, int(s["ply"]))
                st = O.TzState.from_buffer_copy(s.tobytes())
                assert any(oracle.tzo_terminal(C.byref(O.play(oracle, st, m))) != -1 for m in O.possible_moves(oracle, st)), (ply, i)
    assert sum(int(s["ply"]) == 60 + i % 2 for i, s in enumerate(late)) >= 12


@pytest.mark.parametrize("train_rnd", [True, False])
def test_native_loop_trains_and_calibrates(tmp_path, train_rnd):
    """run_learn_native, 6 steps with a save every 3: with train_rnd the model_latest.ot written last holds a predictor that moved
    and the min / max of a calibration of its own weights on the reference positions; without, everything RND is as at the start."""
    A = require_gpu()
    from takzero_amd import formats as F
    from takzero_amd import learn as L
    from takzero_amd import ot
    from test_learn_host import _targets

    w = _weights()
    d, B = str(tmp_path), 64
    with open(os.path.join(d, "targets-selfplay.txt"), "w") as f:
        f.write("".join(F.format_target(5, *t) for t in _targets(5, 160, 8)))
    mcts = A.BatchedMCTS(32, 5, 4, agent_kind=A.AGENT_DUMMY, node_capacity=1 << 10)
    reference = L.rnd_reference(mcts, seed=3, n_early=40, early_ply=4, n_late=40, late_ply=60)
    tr = _trainer(B, False)
    steps = L.run_learn_native(d, tr, steps=6, seed=1, min_selfplay=B, steps_before_reanalyze=10 ** 9, steps_per_save=3,
                               steps_per_checkpoint=10 ** 9, pre_training_steps=0, read_interval=0.0, sleep=0.01, max_wait=20,
                               train_rnd=train_rnd, rnd_reference=reference)
    assert steps == 6
    latest = ot.load_ot(os.path.join(d, "model_latest.ot"))
    assert not np.array_equal(latest["policy.conv2d.weight"], w["policy.conv2d.weight"])
    if not train_rnd:
        for k in w:
            if k.startswith("rnd_") or k in ("min", "max"):
                assert np.array_equal(np.ravel(latest[k]), np.ravel(w[k])), k
        return
    for k in tr.RND_NAMES:
        assert not np.array_equal(latest[k], w[k]), k
        assert np.array_equal(latest[k], tr.tensor(k)), k
    for k in w:
        if k.startswith("rnd_target."):
            assert np.array_equal(latest[k], w[k]), k
    mn, mx = tr.rnd_calibrate(reference[0], reference[1], apply=False)
    assert float(np.ravel(latest["min"])[0]) == mn and float(np.ravel(latest["max"])[0]) == mx and mx > mn
    assert (mn, mx) != (0.0, 1.0)
