"""The learn step (csrc/tz_learn.hip) against fp64 autograd (oracle/learn_torch.py, dtype=torch.float64) where the toy test of
test_gpu_learn.py does not reach: 3x3 and 6x6 boards, batch 192, and the shipped nets at the shipped batch (net4_simhash and
net6_simhash with 16 blocks, net5 with 20, batch 128), net5 also with its heads at trained scale.  Every step is held, layer by
layer, to the exact graph: each trunk activation, the training-mode outputs and the three losses, every gradient, the BatchNorm
running statistics, both Adam moments and the weights after the step.  Then: bit-for-bit determinism at net5 / batch 128, a step
with apply=False, and the hand-off from the trainer to the inference net by every route, extras (RND nets, SimHash matrix)
included."""
import os
import sys

import numpy as np
import pytest

import oracle_lib as O
from gpu_util import require_gpu
from test_gpu_learn import _batch

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))

LR = 1e-4
# The trainer is fp32 throughout; the bounds are its distance from the exact (fp64) graph, each within 4x of the worst value measured
# on an MI355X over the cases of test_step_matches_fp64_autograd (3 steps each).  Two columns: heads at random-init scale (the six
# other cases; the worst case named) and heads at trained scale (net5-bs128-trained-heads).  At trained scale the value head's linear
# layer is ~100x larger, so the trunk's fp32 error reaches the value output amplified, and through tanh near saturation
# (d/dv of 1 - v^2) every gradient the value loss feeds; the weights are large enough that one ulp is a sizeable part of lr.
TOL = {
    # max |trainer - fp64| / max |fp64| of each trunk layer's activation               measured 4.8e-6 (net6_simhash), 3.9e-6
    "activation": (1.5e-5, 1.5e-5),
    # each training-mode output, relative to its largest entry                          5.0e-6 (net6_simhash ube), 8.8e-5 (value)
    "output": (1.5e-5, 3e-4),
    # |trainer - fp64| / (1 + |fp64|) of each loss                                      2.3e-7 (net5 ube), 6.9e-7
    "loss": (8e-7, 2.5e-6),
    # each gradient, relative to the tensor's largest fp64 entry                        2.9e-5 (net4_simhash), 2.8e-3
    "gradient": (1e-4, 1e-2),
    # running mean / variance, relative to the tensor's largest entry                   1.3e-7 (all), 1.3e-7
    "running statistics": (4e-7, 4e-7),
    # Adam's first moment against torch.optim.Adam's exp_avg, relative to the largest   1.5e-5 (net5), 5.5e-4
    "adam m": (5e-5, 2e-3),
    # ... the second against exp_avg_sq (1 - 0.999f is 1.3e-5 off 0.001)               1.7e-5 (test5x5-bs192), 1.1e-3
    "adam v": (5e-5, 4e-3),
    # the weight update against Adam applied in fp64 to the trainer's own moments, in   5.9e-4 (net6_simhash), 0.068
    # units of lr: the rounding of the stored weight (half an ulp of a weight near 1 is 6e-4 lr)
    "adam update / lr": (2e-3, 0.25),
    # weights after the step against torch's, 99th percentile of |diff| in units of lr   3.0e-4 (test5x5-bs192), 0.068
    "weights q99 / lr": (1e-3, 0.25),
    # ... and the largest |diff| in lr: a weight whose gradient is ~0 moves by +-lr      1.19 (net5, net6_simhash), 2.0
    # on either side of zero
    "weights max / lr": (2.5, 2.5),
}
# The ReLU-kink rule: where a trunk ReLU's fp64 input is within KINK_FACTOR x (that layer's measured |trainer - fp64| activation
# error) of zero, the reference takes the side the trainer took (every entry where the two sides differ lies within 1x).  At most
# FORCED_MAX of a layer's entries may be decided so (measured 7.5e-5 at worst, on net5; 1.05e-4 on net6_simhash with a factor of 2).
KINK_FACTOR = 1.5
FORCED_MAX = 1e-4

CASES = [
    # arch, n, blocks, batch, heads at trained scale
    pytest.param("test", 3, 2, 64, False, id="test3x3-b2-bs64"),     # 27 -> 64 policy channels, 9-pixel boards across gather slabs
    pytest.param("test", 6, 2, 64, False, id="test6x6-b2-bs64"),     # 251 -> 256 policy channels, K 324 -> 384, nn = 36 in the heads
    pytest.param("test", 5, 2, 192, False, id="test5x5-b2-bs192"),   # M = 4800: other stream-K splits
    pytest.param("net4_simhash", 4, 16, 128, False, id="net4_simhash-bs128"),
    pytest.param("net5", 5, 20, 128, False, id="net5-bs128"),
    pytest.param("net5", 5, 20, 128, True, id="net5-bs128-trained-heads"),
    pytest.param("net6_simhash", 6, 16, 128, False, id="net6_simhash-bs128"),
]


def _arch(A, name):
    return {"test": A.ARCH_TEST, "net4_simhash": A.ARCH_NET4_SIMHASH, "net5": A.ARCH_NET5, "net6_simhash": A.ARCH_NET6_SIMHASH}[name]


def _rel(a, b):
    """max |a - b| / max |b|, b the fp64 reference"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(float(np.abs(b).max()), 1e-30))


def _nchw(act, B, n):
    """tz_trainer_activation's [B][n*n][256] -> [B, 256, n, n]"""
    return act.transpose(0, 2, 1).reshape(B, 256, n, n)


@pytest.mark.parametrize("arch_name,n,blocks,B,trained", CASES)
def test_step_matches_fp64_autograd(arch_name, n, blocks, B, trained):
    import torch

    import learn_torch as LT
    A = require_gpu()
    from takzero_amd import learn as L
    from takzero_amd import weights as W

    oracle = O.load()
    arch = _arch(A, arch_name)
    f64 = torch.float64
    w = W.init_weights(arch, n=n, blocks=blocks, seed=40 + n + blocks, trained_stats=True)
    batches = [_batch(oracle, n, B, 500 + 10 * n + step) for step in range(3)]
    if trained:
        from test_gpu_net import _trained_scale

        w = _trained_scale(w, batches[0][1], blocks)
    tr = L.Trainer(arch=arch, n=n, blocks=blocks, batch=B, lr=LR).load_tensors(w)
    assert (tr.n, tr.blocks) == (n, blocks)
    p = LT.make_params(w, f64)
    opt = LT.adam(p, LR)
    layers = 1 + 2 * blocks
    tol = {k: v[1 if trained else 0] for k, v in TOL.items()}
    worst = {}

    def note(key, value, bound):
        """keeps the worst value of `key` for the report; True when `value` is within `bound`"""
        worst[key] = max(worst.get(key, 0.0), value)
        return value <= bound

    for step, train_ube in enumerate((True, False, True)):
        states, planes, policy, mask, value, ube = batches[step]
        before = {k: tr.tensor(k) for k in tr.names}
        got = tr.step(states, policy, mask, value, ube, train_ube=train_ube, apply=True)
        acts = [_nchw(tr.activation(l), B, n) for l in range(layers)]
        outs = tr.outputs()
        after = {k: tr.tensor(k) for k in tr.names}
        trained_names = [k for k in tr.names if "running_" not in k]
        grads = {k: tr.tensor(k, L.GRAD) for k in trained_names}
        m1 = {k: tr.tensor(k, L.ADAM_M) for k in trained_names}
        m2 = {k: tr.tensor(k, L.ADAM_V) for k in trained_names}
        inputs = [torch.from_numpy(x) for x in (planes, mask.astype(bool), policy, value, ube)]

        # activations: the plain fp64 forward (on copies of the running statistics, which a training-mode forward moves)
        q = {k: (t.detach().clone() if "running_" in k else t.detach()) for k, t in p.items()}
        with torch.no_grad():
            plain = LT.forward_t(q, inputs[0], blocks, True, dtype=f64, return_layers=True)[3]
        kinks = []
        for l in range(layers):
            ref = plain[l][1].numpy()
            err = float(np.abs(acts[l] - ref).max())
            rel = err / float(np.abs(ref).max())
            assert note("activation", rel, tol["activation"]), (step, "layer", l, rel)
            kinks.append(KINK_FACTOR * err)

        # the step's graph in fp64, each trunk ReLU's kink decided as the trainer did within that layer's own threshold
        opt.zero_grad(set_to_none=True)
        relu_masks = [torch.from_numpy(a > 0) for a in acts]
        want, wouts, wlayers = LT.losses(p, *inputs, blocks, train_ube, relu_masks=relu_masks, kink=kinks, dtype=f64,
                                         return_layers=True)
        (want[0] + want[1] + want[2]).backward()
        forced = []
        for l in range(layers):
            pre = wlayers[l][0].detach()
            near = pre.abs() < kinks[l]
            flipped = int((near & ((pre > 0) != relu_masks[l])).sum())
            frac = float(near.sum()) / near.numel()
            forced.append((int(near.sum()), flipped))
            assert note("forced fraction", frac, FORCED_MAX), (step, "layer", l, frac, kinks[l])
        print("%s step %d: forced ReLU entries per layer (within the kink, of them on the other side of zero): %s"
              % (arch_name, step, forced))

        for name, g, t in zip(("policy", "value", "ube"), outs, wouts):
            rel = _rel(g, t.detach().numpy())
            assert note("output " + name, rel, tol["output"]), (step, name, rel)
        for name, g, t in zip(("policy", "value", "ube"), got, want):
            err = abs(g - float(t.detach())) / (1 + abs(float(t.detach())))
            assert note("loss " + name, err, tol["loss"]), (step, name, got, [float(x.detach()) for x in want])
        for k in trained_names:
            tg = p[k].grad
            if tg is None:
                assert k.startswith("ube.") and not train_ube, k
                continue
            rel = _rel(grads[k], tg.numpy().reshape(grads[k].shape))
            assert note("gradient", rel, tol["gradient"]), (step, k, rel)
        for k in tr.names:
            if "running_" in k:   # moved by the training-mode forward above, as by the trainer's
                rel = _rel(after[k], p[k].numpy())
                assert note("running statistics", rel, tol["running statistics"]), (step, k, rel)

        opt.step()
        for k in trained_names:
            st = opt.state[p[k]]
            for what, got_m, key in (("adam m", m1[k], "exp_avg"), ("adam v", m2[k], "exp_avg_sq")):
                rel = _rel(got_m, st[key].numpy().reshape(got_m.shape))
                assert note(what, rel, tol[what]), (step, k, what, rel)
            if k.startswith("ube.") and not train_ube:   # not stepped: the weights keep every bit
                assert np.array_equal(after[k], before[k]), k
                continue
            # the update itself: Adam with the step's bias corrections, in fp64, from the trainer's own moments
            t = int(st["step"])
            m, v = m1[k].astype(np.float64), m2[k].astype(np.float64)
            exact = before[k] - LR / (1 - 0.9 ** t) * m / (np.sqrt(v) / np.sqrt(1 - 0.999 ** t) + 1e-8)
            err = float(np.abs(after[k] - exact).max()) / LR
            assert note("adam update / lr", err, tol["adam update / lr"]), (step, k, err)
            # and the weights against torch's step from its own fp64 gradients and moments
            diff = np.abs(after[k] - p[k].detach().numpy().reshape(after[k].shape)) / LR
            q99 = float(np.quantile(diff, 0.99))
            assert note("weights q99 / lr", q99, tol["weights q99 / lr"]), (step, k, q99)
            assert note("weights max / lr", float(diff.max()), tol["weights max / lr"]), (step, k, float(diff.max()))
        # both sides go on from the trainer's weights (a weight whose gradient is ~0 moves by +-lr on either side of zero; this
        # keeps that from compounding), while torch's Adam state (step counts, both moments) stays its own
        with torch.no_grad():
            for k in tr.names:
                p[k].copy_(torch.from_numpy(after[k].reshape(p[k].shape)))
    print("%s: worst over 3 steps: %s" % (arch_name, ", ".join("%s %.3g" % kv for kv in sorted(worst.items()))))


def _snapshot(tr, losses, layers):
    from takzero_amd import learn as L

    out = {"losses": np.array(losses, np.float32)}
    for i, o in enumerate(tr.outputs()):
        out["output %d" % i] = o
    for l in range(layers):
        out["activation %d" % l] = tr.activation(l)
    for k in tr.names:
        for what in (L.PARAM, L.GRAD, L.ADAM_M, L.ADAM_V):
            out["%s %d" % (k, what)] = tr.tensor(k, what)
    return out


def test_step_is_bit_reproducible_at_net5_batch_128():
    """gemm_sk_kernel / gemm_fixup_kernel and the reductions sum in a fixed order: two trainers with the same weights, fed the same
    three batches, agree in every bit (losses, outputs, activations, gradients, parameters, running statistics, both moments)."""
    A = require_gpu()
    from takzero_amd import learn as L
    from takzero_amd import weights as W

    oracle = O.load()
    w = W.init_weights(W.ARCH_NET5, seed=61, trained_stats=True)
    trs = [L.Trainer(arch=A.ARCH_NET5, batch=128).load_tensors(w) for _ in range(2)]
    for step, train_ube in enumerate((True, False, True)):
        states, planes, policy, mask, value, ube = _batch(oracle, 5, 128, 700 + step)
        snaps = [_snapshot(tr, tr.step(states, policy, mask, value, ube, train_ube=train_ube), 41) for tr in trs]
        differ = [k for k in snaps[0] if not np.array_equal(snaps[0][k], snaps[1][k])]
        assert not differ, (step, differ[:8])


def test_apply_false_then_the_first_adam_step():
    """apply=False: parameters and both Adam moments keep every bit, the running statistics move as torch's training-mode forward
    moves them.  The next apply=True step is torch Adam's first step (bias corrections of step 1) on the trainer's gradients."""
    import torch

    import learn_torch as LT
    A = require_gpu()
    from takzero_amd import learn as L
    from takzero_amd import weights as W

    oracle = O.load()
    n, blocks, B = 5, 20, 128
    w = W.init_weights(W.ARCH_NET5, seed=71, trained_stats=True)
    tr = L.Trainer(arch=A.ARCH_NET5, batch=B, lr=LR).load_tensors(w)
    trained_names = [k for k in tr.names if "running_" not in k]
    assert all(not tr.tensor(k, what).any() for k in trained_names for what in (L.ADAM_M, L.ADAM_V))
    states, planes, policy, mask, value, ube = _batch(oracle, n, B, 800)
    tr.step(states, policy, mask, value, ube, train_ube=True, apply=False)
    for k in trained_names:
        assert np.array_equal(tr.tensor(k), w[k]), k
        for what in (L.ADAM_M, L.ADAM_V):
            assert not tr.tensor(k, what).any(), (k, what)
    p = LT.make_params(w, torch.float64)
    with torch.no_grad():
        LT.forward_t(p, torch.from_numpy(planes), blocks, True)
    stats = 0.0
    for k in tr.names:
        if "running_" in k:
            assert not np.array_equal(tr.tensor(k), w[k]), k
            stats = max(stats, _rel(tr.tensor(k), p[k].numpy()))
    assert stats <= TOL["running statistics"][0], stats

    states, planes, policy, mask, value, ube = _batch(oracle, n, B, 801)
    tr.step(states, policy, mask, value, ube, train_ube=True, apply=True)
    opt = LT.adam(p, LR)
    for k in trained_names:
        p[k].grad = torch.from_numpy(tr.tensor(k, L.GRAD).astype(np.float64))
    opt.step()
    moments, update = 0.0, 0.0
    for k in trained_names:
        st = opt.state[p[k]]
        assert int(st["step"]) == 1
        for what, key in ((L.ADAM_M, "exp_avg"), (L.ADAM_V, "exp_avg_sq")):
            rel = _rel(tr.tensor(k, what), st[key].numpy())
            moments = max(moments, rel)
            # the same gradients on both sides: m = 0.1 g, v = 0.001 g^2 up to fp32 rounding, and 1 - 0.999f is 1.3e-5 off 0.001
            # (measured 1.3e-5)
            assert rel <= 4e-5, (k, what, rel)
        err = float(np.abs(tr.tensor(k) - p[k].detach().numpy()).max()) / LR
        update = max(update, err)
        assert err <= TOL["adam update / lr"][0], (k, err)
    print("apply=False: running statistics within %.3g; first Adam step: moments within %.3g, weights within %.3g lr"
          % (stats, moments, update))


def _outputs(A, net, states, legal):
    pol, val, ube = net.forward_raw(states)
    logits, val2, var = net.policy_value_uncertainty(states, legal)
    out = [pol, val, ube, np.concatenate(logits), val2, var]
    if net.arch in (A.ARCH_NET4_SIMHASH, A.ARCH_NET6_SIMHASH):
        out.append(net.hash_indices(states))
    return out


@pytest.mark.parametrize("arch_name", ["net5", "net6_simhash"])
def test_trainer_hands_every_variable_to_the_inference_net(arch_name, tmp_path):
    """A trainer loaded by load_tensors and one loaded by from_net, two steps each on the same batches: Net.load_tensors(tensors()),
    to_net, save -> Net.load and ot.save_ot(tensors()) -> Net.load all give the same inference net, bit for bit, the RND variance
    and the SimHash indices included (these come from the variables the step never touches)."""
    A = require_gpu()
    from takzero_amd import learn as L
    from takzero_amd import ot
    from takzero_amd import weights as W

    oracle = O.load()
    arch = _arch(A, arch_name)
    n, B = W.arch_board(arch), 128
    w = W.init_weights(arch, seed=81, trained_stats=True)
    source = A.Net(arch=arch, precision=A.PREC_F32).load_tensors(w)
    by_dict = L.Trainer(arch=arch, batch=B).load_tensors(w)
    by_net = L.Trainer(arch=arch, batch=B).from_net(source)
    want = source.tensors()
    for tr in (by_dict, by_net):   # before any step, either way in, tensors() is the net's VarStore exactly, in its shapes
        held = tr.tensors()
        assert set(held) == set(want) == set(w), set(held) ^ set(want)
        for k in want:
            assert np.array_equal(np.ravel(held[k]), want[k]) and np.shape(held[k]) == np.shape(w[k]), k
    for step in range(2):
        states, planes, policy, mask, value, ube = _batch(oracle, n, B, 900 + step)
        for tr in (by_dict, by_net):
            tr.step(states, policy, mask, value, ube)
    states, planes, policy, mask, value, ube = _batch(oracle, n, B, 950)
    legal = [np.nonzero(mask[i] == 0)[0] for i in range(B)]
    ref = None
    for which, tr in (("load_tensors", by_dict), ("from_net", by_net)):
        routes = {"Net.load_tensors(tensors())": A.Net(arch=arch, precision=A.PREC_F32).load_tensors(tr.tensors())}
        net = A.Net(arch=arch, precision=A.PREC_F32)
        tr.to_net(net)
        routes["to_net"] = net
        for ext in ("ot", "tzw"):
            d = tmp_path / ("%s_save_%s" % (which, ext))
            d.mkdir()
            tr.save(str(d / ("model." + ext)))
            routes["save ." + ext] = A.Net(arch=arch, precision=A.PREC_F32).load(str(d / ("model." + ext)))
        d = tmp_path / ("%s_save_ot_py" % which)
        d.mkdir()
        ot.save_ot(str(d / "model.ot"), tr.tensors())
        routes["ot.save_ot(tensors())"] = A.Net(arch=arch, precision=A.PREC_F32).load(str(d / "model.ot"))
        for route, net in routes.items():
            got = _outputs(A, net, states, legal)
            if ref is None:
                ref = got
                assert all(np.isfinite(np.asarray(x, np.float64)).all() for x in got)
            for i, (a, b) in enumerate(zip(got, ref)):
                assert np.array_equal(a, b), (which, route, i)
    # the trained weights did move, the carried variables did not
    moved = by_dict.tensors()
    assert not np.array_equal(moved["policy.conv2d.weight"], w["policy.conv2d.weight"])
    for k in w:
        if k not in by_dict.names:
            assert np.array_equal(moved[k], w[k]), k
