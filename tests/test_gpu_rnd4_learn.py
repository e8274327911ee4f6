"""Training net4_rnd's predictor tower in the learn step (csrc/tz_learn_rnd4.hip, tz_trainer_rnd4_*; net4_rnd.rs:126-166, 210-223,
learn/src/main.rs:404-405, 415-416) against fp64 autograd (tests/rnd4_learn_ref.py), by the method of test_gpu_learn_rnd.py: the step
layer by layer, that nothing else moves, apply=False and Adam's own step count, bit reproducibility, the falling loss, calibration
through the inference tower, the hand-off to the inference net, the refusals, the native loop and learn_cli.  Weights and batches come
from tests/rnd4_learn_util.py; tests/test_rnd4_learn_ref.py holds the condition of that fixture on the CPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import rnd4_learn_ref as LR4
import rnd4_learn_util as U
import rnd4_ref as R
from gpu_util import random_positions, require_gpu
from test_gpu_learn_fp64 import FORCED_MAX, KINK_FACTOR, TOL, _rel, _snapshot

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

LR = 1e-4
# |trainer - fp64| in the units of test_gpu_learn_fp64.TOL; each bound is the worst value measured on an MI355X over the three cases of
# test_step_matches_fp64_autograd (3 steps each) times at most 4, and none is looser than that file's random-init column (checked
# below).  A conv's sums are 288 long, the batch statistics' 16 * batch.
RND4_TOL = {
    # LayerNorm output, the ten conv outputs before BatchNorm and the ten layer outputs of the predictor, the target's eleven, each
    # relative to the tensor's largest entry                                                            measured 1.55e-6 (batch 192)
    "activation": 6e-6,
    # raw[b] relative to the largest raw of the batch                                                   measured 7.96e-7 (batch 192)
    "raw": 3e-6,
    # |loss_rnd - fp64| / (1 + |fp64|)                                                                  measured 4.89e-8 (batch 128)
    "loss": 1.9e-7,
    # each of the 32 gradients, relative to the tensor's largest fp64 entry                             measured 1.65e-6 (batch 64)
    "gradient": 6.5e-6,
    # the 20 running statistics, relative to the tensor's largest entry                                 measured 1.25e-7 (batch 64)
    "running statistics": 4e-7,
    # Adam's first moment against torch.optim.Adam's exp_avg, relative to the largest entry             measured 1.49e-6 (batch 128)
    "adam m": 5.9e-6,
    # ... the second against exp_avg_sq (1 - 0.999f is 1.3e-5 off 0.001)                                measured 1.50e-5 (batch 128)
    "adam v": 5e-5,
    # the update against Adam applied in fp64 to the trainer's own moments, in units of lr: the        measured 6.04e-4 (batch 64)
    # rounding of the stored weight (half an ulp of a weight near 1 is 6e-4 lr)
    "adam update / lr": 2e-3,
    # weights after the step against torch's, 99th percentile of |diff| in units of lr                  measured 5.89e-4 (batch 64)
    "weights q99 / lr": 1e-3,
    # ... and the largest |diff| in lr                                                                  measured 0.0111 (batch 64)
    "weights max / lr": 0.044,
}
MEASURED_ACTIVATION = 1.55e-6   # the worst of the table's first row: what tests/test_rnd4_learn_ref.py takes for the size of a kink
_SAME_AS = {"raw": "output"}
for _k, _v in RND4_TOL.items():
    assert _v <= TOL[_SAME_AS.get(_k, _k)][0], _k

_CACHE = {}


def _trainer(B, enable=True, w=None):
    A = require_gpu()
    from takzero_amd import learn as L

    tr = L.Trainer(arch=A.ARCH_NET4_RND, batch=B, lr=LR).load_tensors(U.weights() if w is None else w)
    return tr.rnd4_enable() if enable else tr


def _nchw(act):
    """tz_trainer_rnd4_activation's [B][16][32] -> [B, 32, 4, 4]"""
    return act.transpose(0, 2, 1).reshape(len(act), 32, 4, 4)


def _planes(oracle, states):
    return np.stack([O.game_repr(oracle, s) for s in states]).reshape(len(states), -1, 4, 4)


def _tower_bits(store):
    return {k: np.asarray(store[k], np.float32).tobytes() for k in R.tensor_names()}


def _rnd4_snapshot(tr):
    from takzero_amd import learn as L

    loss, raw = tr.rnd4_last()
    out = {"loss": np.float32(loss), "raw": raw}
    for l in range(21):
        out["activation 0 %d" % l] = tr.rnd4_activation(0, l)
    for l in range(11):
        out["activation 1 %d" % l] = tr.rnd4_activation(1, l)
    for k in tr.RND4_TRAINED:
        for what in (L.PARAM, L.GRAD, L.ADAM_M, L.ADAM_V):
            out["%s %d" % (k, what)] = tr.tensor(k, what)
    for k in tr.RND4_STATS:
        out[k] = tr.tensor(k)
    return out


@pytest.mark.parametrize("B", U.BATCHES)
def test_step_matches_fp64_autograd(B):
    import torch
    from takzero_amd import learn as L

    oracle = O.load()
    w = U.weights()
    tr = _trainer(B)
    assert tuple(tr.RND4_TRAINED) == LR4.NAMES and tuple(tr.RND4_STATS) == LR4.STATS
    p = LR4.make_params(w)
    opt = LR4.adam(p, LR)
    worst = {}

    def note(key, value, bound=None):
        worst[key] = max(worst.get(key, 0.0), value)
        return value <= (RND4_TOL[key] if bound is None else bound)

    for step, train_ube in enumerate((True, False, True)):
        states, planes, policy, mask, value, ube = U.batches(oracle, B)[step]
        before = {k: tr.tensor(k) for k in tr.RND4_NAMES}
        tr.step(states, policy, mask, value, ube, train_ube=train_ube, apply=True)
        loss, raw = tr.rnd4_last()
        acts = [[tr.rnd4_activation(t, 0)] + [_nchw(tr.rnd4_activation(t, l)) for l in range(1, 11)] for t in range(2)]
        pres = [_nchw(tr.rnd4_activation(0, 10 + l)) for l in range(1, 11)]
        after = {k: tr.tensor(k) for k in tr.RND4_NAMES}
        grads = {k: tr.tensor(k, L.GRAD) for k in tr.RND4_TRAINED}
        m1 = {k: tr.tensor(k, L.ADAM_M) for k in tr.RND4_TRAINED}
        m2 = {k: tr.tensor(k, L.ADAM_V) for k in tr.RND4_TRAINED}

        # activations against the plain fp64 forward; the predictor's nine ReLU layers give the kink thresholds
        with torch.no_grad():
            plain = LR4.forward_rnd(p, planes, train=True)
        kinks = []
        for t in range(2):
            for l in range(11):
                ref = plain["acts"][t][l].numpy()
                err = float(np.abs(acts[t][l] - ref).max())
                assert note("activation", err / float(np.abs(ref).max())), (step, "tower", t, "layer", l, err / float(np.abs(ref).max()))
                if t == 0 and 1 <= l <= 9:
                    kinks.append(KINK_FACTOR * err)
        for l in range(10):
            rel = _rel(pres[l], plain["pre"][0][l].numpy())
            assert note("activation", rel), (step, "conv output before BatchNorm", l, rel)

        # the step's graph in fp64, the ReLUs' kinks decided as the trainer did within each layer's own threshold
        opt.zero_grad(set_to_none=True)
        masks = [torch.from_numpy(acts[0][l + 1] > 0) for l in range(9)]
        out = LR4.forward_rnd(p, planes, True, masks, kinks)
        loss_t = LR4.loss(out["raw"])
        loss_t.backward()
        forced = []
        for l in range(9):
            z = out["z"][0][l].detach()
            near = z.abs() < kinks[l]
            forced.append((int(near.sum()), int((near & ((z > 0) != masks[l])).sum())))
            assert note("forced fraction", float(near.sum()) / near.numel(), FORCED_MAX), (step, l, kinks[l])
        print("B %d step %d: forced ReLU entries per layer (within the kink, of them on the other side): %s" % (B, step, forced))

        assert note("raw", _rel(raw, out["raw"].detach().numpy())), (step, "raw")
        lt = float(loss_t.detach())
        assert note("loss", abs(loss - lt) / (1 + abs(lt))), (step, loss, lt)
        for k in tr.RND4_TRAINED:
            rel = _rel(grads[k], p[k].grad.numpy().reshape(grads[k].shape))
            assert note("gradient", rel), (step, k, rel)
        for k in tr.RND4_STATS:
            rel = _rel(after[k], out["running"][k].numpy())
            assert note("running statistics", rel), (step, k, rel)
        opt.step()
        for k in tr.RND4_TRAINED:
            st = opt.state[p[k]]
            assert int(st["step"]) == step + 1
            for what, got_m, key in (("adam m", m1[k], "exp_avg"), ("adam v", m2[k], "exp_avg_sq")):
                rel = _rel(got_m, st[key].numpy().reshape(got_m.shape))
                assert note(what, rel), (step, k, what, rel)
            t = step + 1
            m, v = m1[k].astype(np.float64), m2[k].astype(np.float64)
            exact = before[k] - LR / (1 - 0.9 ** t) * m / (np.sqrt(v) / np.sqrt(1 - 0.999 ** t) + 1e-8)
            err = float(np.abs(after[k] - exact).max()) / LR
            assert note("adam update / lr", err), (step, k, err)
            diff = np.abs(after[k] - p[k].detach().numpy().reshape(after[k].shape)) / LR
            q99 = float(np.quantile(diff, 0.99))
            assert note("weights q99 / lr", q99), (step, k, q99)
            assert note("weights max / lr", float(diff.max())), (step, k, float(diff.max()))
        # both sides go on from the trainer's weights and running statistics, torch's Adam state stays its own
        with torch.no_grad():
            for k in tr.RND4_NAMES:
                p[k].copy_(torch.from_numpy(after[k].reshape(p[k].shape)))
        # the frozen side keeps every bit
        held = tr.extras()
        assert sorted(held) == sorted(R.tensor_names())
        for k in held:
            if k.startswith("rnd_target.") or k in ("min", "max"):
                assert np.array_equal(np.ravel(held[k]), np.ravel(w[k])), k
    print("rnd4 B %d: worst over 3 steps: %s" % (B, ", ".join("%s %.3g" % kv for kv in sorted(worst.items()))))


def test_nothing_else_moves():
    """Twin trainers, one enabled: every trunk tensor in all four arenas, the three losses, the outputs and every trunk activation agree
    in every bit; the enabled one leaves rnd_target.*, min and max alone, the disabled one the predictor and its running statistics too."""
    from takzero_amd.api import TakzeroError

    oracle = O.load()
    w = U.weights()
    B = 64
    on, off = _trainer(B, True), _trainer(B, False)
    assert list(on.names) == list(off.names) and not any(k.startswith("rnd_") for k in on.names)
    for step, train_ube in enumerate((True, False, True)):
        states, planes, policy, mask, value, ube = U.batches(oracle, B)[step]
        snaps = [_snapshot(tr, tr.step(states, policy, mask, value, ube, train_ube=train_ube), 33) for tr in (on, off)]
        differ = [k for k in snaps[0] if not np.array_equal(snaps[0][k], snaps[1][k])]
        assert not differ, (step, differ[:8])
    held_on, held_off = on.tensors(), off.tensors()
    assert set(held_on) == set(held_off) == set(w)
    for k in w:
        if k.startswith("rnd_target.") or k in ("min", "max"):
            assert np.array_equal(np.ravel(held_on[k]), np.ravel(w[k])) and np.array_equal(np.ravel(held_off[k]), np.ravel(w[k])), k
        if k.startswith("rnd_predictor."):
            assert np.array_equal(np.ravel(held_off[k]), np.ravel(w[k])), k
            assert not np.array_equal(np.ravel(held_on[k]), np.ravel(w[k])) and held_on[k].shape == np.shape(w[k]), k
    with pytest.raises(TakzeroError):   # the predictor's names answer only while its training is enabled
        off.tensor("rnd_predictor.layer_norm.bias")


def test_apply_false_then_the_first_step_of_the_predictor_group():
    """Enabled after two plain steps (the trunk's Adam count is 2).  apply=False gives the loss and every gradient and moves nothing of
    the tower: no weight, no moment and no running statistic (the step's apply flag gates the tower's statistics with its weights,
    where the trunk's forward moves its own at every call).  The next step is torch Adam's step 1 on the trainer's gradients."""
    import torch
    from takzero_amd import learn as L

    oracle = O.load()
    w = U.weights()
    B = 64
    tr = _trainer(B, False)
    batches = U.batches(oracle, B)
    for step in range(2):
        states, planes, policy, mask, value, ube = batches[step]
        tr.step(states, policy, mask, value, ube)
    tr.rnd4_enable()
    states, planes, policy, mask, value, ube = batches[2]
    tr.step(states, policy, mask, value, ube, apply=False)
    assert tr.rnd4_last()[0] > 0
    for k in tr.RND4_TRAINED:
        assert np.array_equal(np.ravel(tr.tensor(k)), np.ravel(w[k])), k
        assert not tr.tensor(k, L.ADAM_M).any() and not tr.tensor(k, L.ADAM_V).any(), k
        assert tr.tensor(k, L.GRAD).any(), k
    for k in tr.RND4_STATS:
        assert np.array_equal(tr.tensor(k), w[k]), k
    states, planes, policy, mask, value, ube = batches[0]
    tr.step(states, policy, mask, value, ube, apply=True)
    for k in tr.RND4_STATS:
        assert not np.array_equal(tr.tensor(k), w[k]), k
    p = LR4.make_params(w)
    opt = LR4.adam(p, LR)
    for k in tr.RND4_TRAINED:
        p[k].grad = torch.from_numpy(tr.tensor(k, L.GRAD).astype(np.float64)).reshape(p[k].shape)
    opt.step()
    moments, update = 0.0, 0.0
    for k in tr.RND4_TRAINED:
        st = opt.state[p[k]]
        assert int(st["step"]) == 1
        for what, key in ((L.ADAM_M, "exp_avg"), (L.ADAM_V, "exp_avg_sq")):
            rel = _rel(tr.tensor(k, what), st[key].numpy().reshape(tr.tensor(k, what).shape))
            moments = max(moments, rel)
            # the same gradients on both sides: m = 0.1 g, v = 0.001 g^2 up to fp32 rounding; 1 - 0.999f is 1.3e-5 off 0.001
            assert rel <= 4e-5, (k, what, rel)
        err = float(np.abs(tr.tensor(k) - p[k].detach().numpy().reshape(tr.tensor(k).shape)).max()) / LR
        update = max(update, err)
        assert err <= RND4_TOL["adam update / lr"], (k, err)
    print("rnd4 first Adam step after two plain steps: moments within %.3g, weights within %.3g lr" % (moments, update))


def test_rnd4_step_is_bit_reproducible():
    oracle = O.load()
    B = 128
    trs = [_trainer(B), _trainer(B)]
    for step, train_ube in enumerate((True, False, True)):
        states, planes, policy, mask, value, ube = U.batches(oracle, B)[step]
        snaps = []
        for tr in trs:
            tr.step(states, policy, mask, value, ube, train_ube=train_ube)
            snaps.append(_rnd4_snapshot(tr))
        differ = [k for k in snaps[0] if not np.array_equal(snaps[0][k], snaps[1][k])]
        assert not differ, (step, differ[:8])


def test_loss_follows_the_fp64_trajectory():
    """20 steps on one fixed batch: the device loss before step k lies within (k + 1) x the loss bound of the fp64 trajectory (k + 1
    forward passes have been taken when it is read), and the run ends below its start."""
    oracle = O.load()
    w = U.weights()
    B = 64
    states, planes, policy, mask, value, ube = U.batches(oracle, B)[0]
    tr = _trainer(B)
    got = []
    for _ in range(20):
        tr.step(states, policy, mask, value, ube, train_ube=False)
        got.append(tr.rnd4_last()[0])
    p = LR4.make_params(w)
    opt = LR4.adam(p, LR)
    want = []
    for _ in range(20):
        opt.zero_grad(set_to_none=True)
        out = LR4.forward_rnd(p, planes, train=True)
        loss = LR4.loss(out["raw"])
        loss.backward()
        LR4.commit_running(p, out["running"])
        opt.step()
        want.append(float(loss.detach()))
    errs = [abs(g - t) / (1 + abs(t)) for g, t in zip(got, want)]
    print("rnd4 loss on the device: %.4f -> %.4f (fp64 %.4f -> %.4f); |device - fp64| / (1 + |fp64|) / (k + 1), worst: %.3g"
          % (got[0], got[-1], want[0], want[-1], max(e / (k + 1) for k, e in enumerate(errs))))
    assert got[-1] < got[0] and want[-1] < want[0], (got, want)
    for k, e in enumerate(errs):
        assert e <= RND4_TOL["loss"] * (k + 1), (k, got[k], want[k], e)


def _calibration_sets(oracle):
    """70 early positions (ply <= 5) and 64 late ones (ply >= 12): one count is no multiple of the batch"""
    if "cal" not in _CACHE:
        early = random_positions(oracle, O, 4, 4, 70, 31, min_ply=0, max_ply=5)
        late = random_positions(oracle, O, 4, 4, 64, 32, min_ply=12, max_ply=30)
        _CACHE["cal"] = (O.states_array(early), O.states_array(late))
    return _CACHE["cal"]


def test_calibration():
    A = require_gpu()
    from takzero_amd.api import TakzeroError

    oracle = O.load()
    w = U.weights()
    early, late = _calibration_sets(oracle)
    B = 64
    tr = _trainer(B)
    for step in range(2):   # the predictor and its running statistics are no longer the loaded ones
        states, planes, policy, mask, value, ube = U.batches(oracle, B)[step]
        tr.step(states, policy, mask, value, ube)
    net = A.Net(arch=A.ARCH_NET4_RND, precision=A.PREC_F32)
    tr.to_net(net)
    want = (float(net.rnd_raw(early).min()), float(net.rnd_raw(late).max()))
    before = _tower_bits(tr.extras())
    got = tr.rnd4_calibrate(early, late, apply=False)
    print("rnd4 calibrate: got (%.9g, %.9g), the f32 net (%.9g, %.9g)" % (got + want))
    assert np.float32(got[0]).tobytes() == np.float32(want[0]).tobytes() and np.float32(got[1]).tobytes() == np.float32(want[1]).tobytes()
    assert got[1] > got[0] and _tower_bits(tr.extras()) == before
    assert tr.rnd4_calibrate(early, late, apply=True) == got
    held = tr.extras()
    assert held["min"].shape == (1,) and held["min"][0] == np.float32(got[0]) and held["max"][0] == np.float32(got[1])
    # exact towers: every raw is the same integer, so max is not above min
    ew, total = R.exact_towers(3)
    exact = dict(w)
    exact.update(ew)
    exact["min"], exact["max"] = np.array([0.25], np.float32), np.array([7.5], np.float32)
    te = _trainer(B, True, exact)
    with pytest.raises(TakzeroError) as e:
        te.rnd4_calibrate(early, late, apply=True)
    assert e.value.code == -6
    held = te.extras()
    assert held["min"][0] == np.float32(0.25) and held["max"][0] == np.float32(7.5)
    mn = te.lib.tz_trainer_rnd4_calibrate   # the extremes are still reported
    import ctypes as C
    lo, hi = C.c_float(), C.c_float()
    assert mn(te.h, early.ctypes.data, len(early), late.ctypes.data, len(late), 0, C.byref(lo), C.byref(hi)) == -6
    assert lo.value == hi.value == total
    off = _trainer(B, False)
    with pytest.raises(TakzeroError) as e:
        off.rnd4_calibrate(early, late, apply=False)
    assert e.value.code == -6


def test_trained_predictor_reaches_the_inference_net(tmp_path):
    """After 3 steps save -> load, to_net, tensors() and extras() carry the same moved predictor and running statistics; an inference
    net built by each route returns the same rnd_raw bits, which are not those from before the training."""
    A = require_gpu()
    from takzero_amd import learn as L

    oracle = O.load()
    w = U.weights()
    B = 64
    tr = _trainer(B)
    for step in range(3):
        states, planes, policy, mask, value, ube = U.batches(oracle, B)[step]
        tr.step(states, policy, mask, value, ube)
    held, extras = tr.tensors(), tr.extras()
    want = _tower_bits(extras)
    assert _tower_bits(held) == want
    for k in tr.RND4_NAMES:
        assert np.array_equal(np.ravel(extras[k]), np.ravel(tr.tensor(k))), k
        assert not np.array_equal(np.ravel(extras[k]), np.ravel(w[k])), k
    routes = {"Net.load_tensors(tensors())": A.Net(arch=A.ARCH_NET4_RND, precision=A.PREC_F32).load_tensors(held)}
    net = A.Net(arch=A.ARCH_NET4_RND, precision=A.PREC_F32)
    tr.to_net(net)
    routes["to_net"] = net
    for ext in ("ot", "tzw"):
        path = str(tmp_path / ("model." + ext))
        tr.save(path)
        routes["save ." + ext] = A.Net(arch=A.ARCH_NET4_RND, precision=A.PREC_F32).load(path)
        back = L.Trainer(arch=A.ARCH_NET4_RND, batch=B).load(path)
        assert _tower_bits(back.extras()) == want, ext
        back.rnd4_enable()   # a load while enabled re-uploads the model's
        back.load(path)
        assert _tower_bits(back.extras()) == want, ext
        back.close()
    arr = O.states_array(random_positions(oracle, O, 4, 4, 96, 4321, max_ply=30))
    raws = {route: n_.rnd_raw(arr) for route, n_ in routes.items()}
    first = raws["to_net"]
    for route, raw in raws.items():
        assert raw.tobytes() == first.tobytes(), route
        assert _tower_bits(routes[route].tensors()) == want, route
    untrained = A.Net(arch=A.ARCH_NET4_RND, precision=A.PREC_F32).load_tensors(w).rnd_raw(arr)
    assert not np.array_equal(untrained, first)
    print("rnd4 hand-off: mean raw %.6g before, %.6g after 3 steps" % (float(untrained.mean()), float(first.mean())))


def test_refusals():
    A = require_gpu()
    from takzero_amd import learn as L
    from takzero_amd import weights as W

    for arch, n in ((A.ARCH_NET5, 5), (A.ARCH_NET4_SIMHASH, 4)):
        tr = L.Trainer(arch=arch, batch=64).load_tensors(W.init_weights(arch, seed=3))
        with pytest.raises(A.TakzeroError) as e:
            tr.rnd4_enable()
        assert e.value.code == -1
        tr.close()
    tr = _trainer(64)
    with pytest.raises(A.TakzeroError):
        tr.rnd_enable()   # net5's call stays net5's
    bare = L.Trainer(arch=A.ARCH_NET4_RND, batch=64).load_tensors(W.init_weights(A.ARCH_NET4_SIMHASH, seed=3))
    with pytest.raises(A.TakzeroError) as e:
        bare.rnd4_enable()   # no towers among the loaded variables
    assert e.value.code == -6
    with pytest.raises(A.TakzeroError):
        tr.rnd4_activation(1, 11)   # the target keeps no conv outputs
    with pytest.raises(A.TakzeroError):
        tr.tensor("rnd_predictor.batch_norm.running_mean", L.GRAD)   # a running statistic has no gradient


def _target_file(d, count=160):
    from takzero_amd import formats as F
    from test_learn_host import _targets

    with open(os.path.join(d, "targets-selfplay.txt"), "w") as f:
        f.write("".join(F.format_target(4, *t) for t in _targets(4, count, 8)))


@pytest.mark.parametrize("train_rnd", [True, False])
def test_native_loop_trains_and_calibrates(tmp_path, train_rnd):
    """run_learn_native, 6 steps with a save every 3: with train_rnd the model_latest.ot written last holds a predictor that moved,
    running statistics that moved and the min / max of a calibration of its own weights on the reference positions; without, every
    tower tensor is the input's bits."""
    A = require_gpu()
    from takzero_amd import learn as L
    from takzero_amd import ot

    w = U.weights()
    d, B = str(tmp_path), 64
    _target_file(d)
    mcts = A.BatchedMCTS(32, 4, 4, agent_kind=A.AGENT_DUMMY, node_capacity=1 << 10)
    reference = L.rnd_reference(mcts, seed=3, n_early=40, early_ply=4, n_late=40, late_ply=20)
    tr = _trainer(B, False)
    steps = L.run_learn_native(d, tr, steps=6, seed=1, min_selfplay=B, steps_before_reanalyze=10 ** 9, steps_per_save=3,
                               steps_per_checkpoint=10 ** 9, pre_training_steps=0, read_interval=0.0, sleep=0.01, max_wait=20,
                               train_rnd=train_rnd, rnd_reference=reference)
    assert steps == 6
    latest = ot.load_ot(os.path.join(d, "model_latest.ot"))
    assert not np.array_equal(latest["policy.conv2d.weight"], w["policy.conv2d.weight"])
    if not train_rnd:
        for k in tr.RND4_NAMES:   # the predictor and its running statistics first, by name
            assert np.asarray(latest[k], np.float32).tobytes() == np.asarray(w[k], np.float32).tobytes(), k
        assert _tower_bits(latest) == _tower_bits(w)
        return
    for k in tr.RND4_NAMES:
        assert not np.array_equal(np.ravel(latest[k]), np.ravel(w[k])), k
        assert np.array_equal(np.ravel(latest[k]), np.ravel(tr.tensor(k))), k
    for k in w:
        if k.startswith("rnd_target."):
            assert np.array_equal(np.ravel(latest[k]), np.ravel(w[k])), k
    mn, mx = tr.rnd4_calibrate(reference[0], reference[1], apply=False)
    assert float(np.ravel(latest["min"])[0]) == mn and float(np.ravel(latest["max"])[0]) == mx and mx > mn


def test_learn_cli_trains_the_tower(tmp_path):
    """learn_cli --arch net4_rnd --train-rnd on a small directory: exit status 0, and model_latest.ot holds a predictor that is not
    model_0000000.ot's, an untouched target and a calibrated max > min."""
    require_gpu()
    from takzero_amd import ot
    from test_gpu_native_driver import _build_example

    exe = _build_example(tmp_path, "learn_cli")
    d = tmp_path / "run"
    d.mkdir()
    _target_file(str(d))
    r = subprocess.run([exe, "--directory", str(d), "--arch", "net4_rnd", "--train-rnd", "--batch", "64", "--steps", "6", "--seed", "5",
                        "--pre-training-steps", "0", "--min-selfplay", "64", "--steps-before-reanalyze", "1000000000", "--steps-per-save", "3",
                        "--read-interval", "0", "--sleep", "0.01", "--wait-limit", "20"], capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "model_steps 6 " in r.stdout, (r.stdout, r.stderr[-2000:])
    first, latest = ot.load_ot(str(d / "model_0000000.ot")), ot.load_ot(str(d / "model_latest.ot"))
    for k in LR4.NAMES + LR4.STATS:
        assert not np.array_equal(latest[k], first[k]), k
    for k in first:
        if k.startswith("rnd_target."):
            assert np.array_equal(latest[k], first[k]), k
    assert float(np.ravel(latest["max"])[0]) > float(np.ravel(latest["min"])[0])
    assert (float(np.ravel(latest["min"])[0]), float(np.ravel(latest["max"])[0])) != (0.0, 1.0)
