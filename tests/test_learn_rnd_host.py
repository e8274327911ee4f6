"""CPU side of RND training (net5.rs:193-218; learn/src/main.rs:404-405, 415-416): the library exports the new calls, the fp64
reference of the GPU tests (tests/rnd_ref.py) is the graph of oracle/nets_torch.py and does learn, and learn_cli knows the flags.
The step itself is in test_gpu_learn_rnd.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
from gpu_util import random_positions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

RND_SYMBOLS = ("tz_trainer_rnd_enable", "tz_trainer_rnd_last", "tz_trainer_rnd_activation", "tz_trainer_rnd_calibrate",
               "tz_learn_set_rnd", "tz_learn_rnd_reference")


def test_library_exports_the_rnd_calls():
    from takzero_amd import _lib
    from takzero_amd import learn as L

    lib = _lib.load()
    for name in RND_SYMBOLS:
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    header = open(os.path.join(ROOT, "include", "takzero_hip.h")).read()
    for name in RND_SYMBOLS:
        assert "int %s(" % name in header, name
    assert len(L.Trainer.RND_NAMES) == 6 and all(k.startswith("rnd_learning.") for k in L.Trainer.RND_NAMES)
    for f in ("rnd_enable", "rnd_last", "rnd_activation", "rnd_calibrate"):
        assert callable(getattr(L.Trainer, f)), f
    assert callable(L.NativeLearnLoop.set_rnd) and callable(L.rnd_reference)


def rnd_inputs(oracle):
    """Weights and the one fixed batch of the loss-falls tests (here in fp64, on the trainer in test_gpu_learn_rnd.py)."""
    from takzero_amd import weights as W

    w = W.init_weights(W.ARCH_NET5, blocks=1, seed=91)
    states = random_positions(oracle, O, 5, 4, 64, 1234, max_ply=24)
    planes = np.stack([O.game_repr(oracle, s) for s in states]).reshape(64, -1, 5, 5)
    return w, states, planes


def fp64_trajectory(w, planes, steps=20, lr=1e-4):
    """loss_rnd before each of `steps` fp64 Adam steps on one batch"""
    import rnd_ref as R

    p = R.make_params(w)
    opt = R.adam(p, lr)
    out = []
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        loss = R.forward_rnd(p, planes)[0].mean()
        loss.backward()
        opt.step()
        out.append(float(loss.detach()))
    return out


def test_reference_is_the_oracle_graph_and_learns(oracle):
    """rnd_ref.forward_rnd equals nets_torch.rnd_raw (and so rnd_calibrate) exactly in fp64; 20 Adam steps at lr 1e-4 on one fixed
    batch lower loss_rnd at every step (0.4098 -> 0.0501 when this was written)."""
    import nets_torch as T
    import rnd_ref as R
    import torch

    w, _states, planes = rnd_inputs(oracle)
    p = R.make_params(w)
    with torch.no_grad():
        raw = R.forward_rnd(p, planes)[0]
    want = T.rnd_raw(w, planes, torch.float64)
    assert torch.equal(raw, want)
    early, late = planes[:30], planes[30:]
    assert T.rnd_calibrate(w, early, late) == (float(raw[:30].min()), float(raw[30:].max()))
    # the kink rule with masks taken from the reference itself changes nothing
    with torch.no_grad():
        layers = R.forward_rnd(p, planes)[1]
        masks = [layers[0][i][1] > 0 for i in range(2)]
        assert torch.equal(R.forward_rnd(p, planes, masks, [1e-9, 1e-9])[0], want)
    losses = fp64_trajectory(w, planes)
    print("fp64 loss_rnd over 20 steps: %.4f -> %.4f" % (losses[0], losses[-1]))
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    assert abs(losses[0] - 0.4098) < 1e-3 and losses[-1] / losses[0] < 0.2, losses


def _learn_cli(tmp_path):
    exe = str(tmp_path / "learn_cli")
    from takzero_amd import _lib

    _lib.load()
    r = subprocess.run(["g++", "-std=c++17", "-O2", os.path.join(ROOT, "examples", "learn_cli.cpp"), "-I" + os.path.join(ROOT, "include"),
                        "-L" + os.path.dirname(_lib.LIB_PATH), "-ltakzero_hip", "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def test_learn_cli_lists_the_flags_and_refuses_rnd_without_net5(tmp_path):
    exe = _learn_cli(tmp_path)
    r = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--train-rnd" in r.stdout and "--rnd-calibrate-every" in r.stdout, (r.stdout, r.stderr)
    for arch in ("4", "6", "100"):
        r = subprocess.run([exe, "--directory", str(tmp_path), "--arch", arch, "--train-rnd"], capture_output=True, text=True)
        assert r.returncode == 2 and "--train-rnd" in r.stderr and "net5" in r.stderr, (arch, r.stdout, r.stderr)
    assert not any(name.endswith(".ot") for name in os.listdir(tmp_path))
