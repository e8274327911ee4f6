"""The fp64 reference of net4_rnd's predictor training (tests/rnd4_learn_ref.py) held on the CPU: its eval mode against the inference
reference, the whole step against a restatement in torch.nn modules, its sensitivity to the faults a wrong kernel chain would have, the
condition of the fixture the GPU test runs on, and the symbols of the feature."""
import os
import re
import subprocess

import numpy as np
import pytest

import rnd4_learn_ref as LR4
import rnd4_learn_util as U
import rnd4_ref as R
from test_gpu_learn_fp64 import FORCED_MAX, KINK_FACTOR, TOL
from test_rnd4_ref import _random_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR = 1e-4


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(float(np.abs(b).max()), 1e-300))


def test_eval_mode_is_the_inference_reference():
    import torch

    w, planes = _random_case(7, 24)
    with torch.no_grad():
        got = LR4.forward_rnd(LR4.make_params(w), planes, train=False)
    want = R.raw(w, planes, "f64")
    assert _rel(got["raw"].numpy(), want) < 1e-12 and want.std() > 0
    assert not got["running"]
    for t, name in enumerate(R.TOWERS):
        assert _rel(got["acts"][t][-1].numpy(), R.tower(w, name, planes, "f64")) < 1e-12


def _module_step(w, planes, lr):
    """the step restated with torch.nn modules: the predictor in .train(), the target in .eval() and detached"""
    import torch
    from torch import nn

    t64 = lambda a, shape=None: torch.from_numpy(np.array(a, np.float32, copy=True)).to(torch.float64).reshape(shape or np.shape(a))

    class Tower(nn.Module):
        def __init__(self, prefix):
            super().__init__()
            self.ln = nn.LayerNorm([28, 4, 4], eps=1e-5).double()
            self.ln.weight.data, self.ln.bias.data = t64(w[prefix + ".layer_norm.weight"], (28, 4, 4)), t64(w[prefix + ".layer_norm.bias"], (28, 4, 4))
            self.convs, self.norms = nn.ModuleList(), nn.ModuleList()
            for l, (conv, norm) in enumerate(R.layer_names(prefix)):
                c, b = nn.Conv2d(28 if l == 0 else 32, 32, 3, padding=1, bias=False).double(), nn.BatchNorm2d(32, eps=1e-5, momentum=0.1).double()
                c.weight.data = t64(w[conv + ".weight"])
                b.weight.data, b.bias.data = t64(w[norm + ".weight"]), t64(w[norm + ".bias"])
                b.running_mean.data, b.running_var.data = t64(w[norm + ".running_mean"]), t64(w[norm + ".running_var"])
                self.convs.append(c)
                self.norms.append(b)

        def forward(self, x):
            small = lambda l, v: self.norms[l](self.convs[l](v))
            x = torch.relu(small(0, self.ln(x)))
            for b in range(4):
                x = torch.relu(small(2 + 2 * b, torch.relu(small(1 + 2 * b, x))) + x)
            return small(9, x).flatten(1, 3)

        def named(self, prefix):
            out = {prefix + ".layer_norm.weight": self.ln.weight, prefix + ".layer_norm.bias": self.ln.bias}
            for l, (conv, norm) in enumerate(R.layer_names(prefix)):
                out[conv + ".weight"] = self.convs[l].weight
                for v in ("weight", "bias", "running_mean", "running_var"):
                    out[norm + "." + v] = getattr(self.norms[l], v)
            return out

    predictor, target = Tower(LR4.PREDICTOR).train(), Tower(LR4.TARGET).eval()
    named = predictor.named(LR4.PREDICTOR)
    opt = torch.optim.Adam([named[k] for k in LR4.NAMES], lr=lr)
    x = torch.from_numpy(np.asarray(planes, np.float64))
    loss = (predictor(x) - target(x).detach()).square().sum(dim=1).mean()
    loss.backward()
    grads = {k: named[k].grad.clone() for k in LR4.NAMES}
    opt.step()
    return float(loss.detach()), grads, {k: v.detach() for k, v in named.items()}, target.named(LR4.TARGET)


def test_the_step_against_torch_modules():
    import torch

    w, planes = _random_case(11, 24)
    p = LR4.make_params(w)
    opt = LR4.adam(p, LR)
    out = LR4.forward_rnd(p, planes, train=True)
    loss = LR4.loss(out["raw"])
    loss.backward()
    want_loss, want_grads, want_after, target_after = _module_step(w, planes, LR)
    assert abs(float(loss.detach()) - want_loss) <= 1e-12 * abs(want_loss)
    for k in LR4.NAMES:
        assert _rel(p[k].grad.numpy(), want_grads[k].numpy()) < 1e-12, k
        assert float(p[k].grad.abs().max()) > 0, k
    LR4.commit_running(p, out["running"])
    for k in LR4.STATS:
        assert _rel(p[k].numpy(), want_after[k].numpy()) < 1e-12, k
        assert not np.array_equal(p[k].numpy(), np.asarray(w[k], np.float64)), k
    opt.step()
    for k in LR4.NAMES:
        assert _rel(p[k].detach().numpy(), want_after[k].numpy()) < 1e-12, k
    for k, v in target_after.items():   # the module restatement leaves the target alone as well
        assert np.array_equal(v.detach().numpy().ravel(), np.asarray(w[k], np.float64).ravel()), k


def _checked(w, planes, **faults):
    """the quantities the GPU test checks, after one step at LR: activations, raw, loss, gradients, running statistics, weights in lr"""
    import torch

    p = LR4.make_params(w)
    if faults.get("target_grad"):
        for k in LR4.trained_names(LR4.TARGET):
            p[k].requires_grad_(True)
    opt = torch.optim.Adam([t for t in p.values() if t.requires_grad], lr=LR)
    out = LR4.forward_rnd(p, planes, train=True, **faults)
    loss = LR4.loss(out["raw"], **faults)
    loss.backward()
    q = {"raw": out["raw"].detach().numpy(), "loss": np.array([float(loss.detach())])}
    for t in range(2):
        for l, a in enumerate(out["acts"][t]):
            q["activation %d %d" % (t, l)] = a.detach().numpy()
    for k in LR4.NAMES:
        q["gradient " + k] = np.zeros(p[k].shape) if p[k].grad is None else p[k].grad.numpy().copy()
    for k, v in out["running"].items():
        q["running " + k] = v.numpy()
    before = {k: p[k].detach().numpy().copy() for k in p}
    opt.step()
    for k in p:
        if "running_" not in k:   # in units of lr, as the GPU test measures weights
            q["weights / lr " + k] = (p[k].detach().numpy() - before[k]) / LR
    return q


FAULTS = {
    "running variance from the biased estimate": dict(biased_running_var=True),
    "momentum 0.9": dict(momentum=0.9),
    "target run in training mode": dict(target_train=True),
    "gradient reaching the target": dict(target_grad=True),
    "a residual branch missing in the backward": dict(residual_backward_missing=True),
    "LayerNorm affine without gradient": dict(ln_affine_detached=True),
    "LayerNorm sample variance": dict(ln_sample_variance=True),
    "loss averaged over 512 * batch": dict(loss_over_512=True),
    "last block followed by a ReLU": dict(final_relu=True),
}


@pytest.mark.parametrize("fault", list(FAULTS), ids=lambda s: s.replace(" ", "-"))
def test_reference_notices_a_wrong_step(fault):
    """Each fault moves a checked quantity by more than 1e-3 of its largest entry (ten times test_gpu_learn_fp64.TOL["gradient"][0], the
    loosest random-init bound for this arithmetic).  One position: the biased and the unbiased variance of n = 16 * batch rows differ
    by 1 / (n - 1), and momentum 0.1 keeps a tenth of that beside nine tenths of the old value, so from 7 positions on no running
    variance can move by 1e-3 however wrong the estimate; at the GPU test's batches (n >= 1024) that fault moves it by up to 9.8e-5, which is held there against the
    running-statistics bound of 4e-7 (asserted below at batch 64 with a margin of 50).  The weights are measured in units of lr, as
    the GPU test measures them: a gradient that reaches the target moves its variables by about one lr where the test wants no bit
    to move."""
    w, planes = _random_case(13, 64)
    assert TOL["gradient"][0] * 10 == pytest.approx(1e-3)
    good, bad = _checked(w, planes[:1]), _checked(w, planes[:1], **FAULTS[fault])
    moved = {k: float(np.abs(bad[k] - good[k]).max() / max(float(np.abs(good[k]).max()), 1.0 if k.startswith("weights") else 1e-300))
             for k in good}
    worst = max(moved, key=moved.get)
    print("%s: moves %s by %.3g of its largest entry" % (fault, worst, moved[worst]))
    assert moved[worst] > 1e-3, (fault, worst, moved[worst])
    if fault.startswith("running variance"):
        good, bad = _checked(w, planes), _checked(w, planes, **FAULTS[fault])
        at64 = max(_rel(bad[k], good[k]) for k in good if k.startswith("running "))
        print("%s at batch 64: running statistics move by %.3g" % (fault, at64))
        assert at64 > 50 * TOL["running statistics"][0]


@pytest.mark.parametrize("B", U.BATCHES)
def test_fixture_condition(oracle, B):
    """On every batch the GPU test runs: no predictor BatchNorm channel has a batch variance below 1e-6 of its layer's mean channel
    variance (such a channel's 1 / sqrt(var + eps) would amplify the fp32 error of the conv below it beyond any bound), and the
    reference alone, with the kink KINK_FACTOR x (the worst activation error measured on the device x the layer's largest entry: the GPU
    test takes each layer's own error, of which that is the largest, and holds the cap itself), decides at most FORCED_MAX of a layer's ReLU entries by the mask."""
    import torch
    from test_gpu_rnd4_learn import MEASURED_ACTIVATION

    w = U.weights()
    assert not all(np.all(w[t + ".layer_norm.weight"] == 1) for t in R.TOWERS)
    p = LR4.make_params(w)
    for step, batch in enumerate(U.batches(oracle, B)):
        with torch.no_grad():
            out = LR4.forward_rnd(p, batch[1], train=True)
        for l, y in enumerate(out["pre"][0]):
            var = y.var(dim=(0, 2, 3), unbiased=False).numpy()
            assert var.min() >= 1e-6 * var.mean(), (B, step, l, float(var.min()), float(var.mean()))
        for l in range(LR4.LAYERS - 1):
            z, a = out["z"][0][l], out["acts"][0][l + 1]
            kink = KINK_FACTOR * MEASURED_ACTIVATION * float(a.abs().max())
            share = float((z.abs() < kink).sum()) / z.numel()
            assert share <= FORCED_MAX, (B, step, l, share)


def test_symbols(tmp_path):
    """the header declares the four entry points, the built library exports them, _lib.py binds them, learn_cli --help names net4_rnd
    beside --train-rnd"""
    from takzero_amd import _lib
    from takzero_amd import learn as L

    names = ["tz_trainer_rnd4_enable", "tz_trainer_rnd4_last", "tz_trainer_rnd4_activation", "tz_trainer_rnd4_calibrate"]
    header = open(os.path.join(ROOT, "include", "takzero_hip.h")).read()
    for name in names:
        assert re.search(r"\bint %s\(tz_trainer\* t," % name, header), name
    lib = _lib.load()
    for name in names:
        assert getattr(lib, name).argtypes, name
    assert tuple(L.Trainer.RND4_NAMES) == LR4.NAMES + LR4.STATS
    assert set(L.Trainer.RND4_NAMES) < set(R.tensor_names())
    for attr in ("rnd4_enable", "rnd4_last", "rnd4_activation", "rnd4_calibrate"):
        assert callable(getattr(L.Trainer, attr)), attr
    exe = str(tmp_path / "learn_cli")
    r = subprocess.run(["g++", "-std=c++17", "-O2", os.path.join(ROOT, "examples", "learn_cli.cpp"), "-I" + os.path.join(ROOT, "include"),
                        "-L" + os.path.dirname(_lib.LIB_PATH), "-ltakzero_hip", "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe, "--help"], capture_output=True, text=True)
    line = [s for s in r.stdout.splitlines() if s.lstrip().startswith("--train-rnd")]
    assert r.returncode == 0 and line and "net4_rnd" in line[0] and "net5" in line[0], r.stdout
