"""The learn step's reference itself (oracle/learn_torch.py), on the CPU: its fp64 graph is the fp32 graph to fp32 rounding, it
returns every trunk layer, and the ReLU-kink rule acts only within its threshold, per layer."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))

N, BLOCKS, B = 3, 2, 16


def _inputs(seed):
    import torch

    from takzero_amd import weights as W

    rng = np.random.default_rng(seed)
    w = W.init_weights(W.ARCH_TEST, n=N, blocks=BLOCKS, seed=seed, trained_stats=True)
    planes = (rng.random((B, W.input_channels(N), N, N)) < 0.3).astype(np.float32)
    out = W.output_channels(N) * N * N
    mask = rng.random((B, out)) > 0.2
    mask[:, 0] = False                       # at least one legal move per row
    policy = np.where(mask, 0.0, rng.random((B, out))).astype(np.float32)
    policy /= policy.sum(1, keepdims=True)
    value = rng.uniform(-1, 1, B).astype(np.float32)
    ube = rng.uniform(1e-6, 5.0, B).astype(np.float32)
    return w, [torch.from_numpy(x) for x in (planes, mask, policy, value, ube)]


def _run(w, inputs, dtype, **kw):
    import learn_torch as LT

    p = LT.make_params(w, dtype)
    got = LT.losses(p, *inputs, BLOCKS, True, dtype=dtype, **kw)
    sum(got[0]).backward()
    return p, got


def test_fp64_reference_is_the_fp32_reference_to_rounding():
    import torch

    w, inputs = _inputs(5)
    p32, (l32, o32, t32) = _run(w, inputs, torch.float32, return_layers=True)
    p64, (l64, o64, t64) = _run(w, inputs, torch.float64, return_layers=True)
    assert all(x.dtype == torch.float64 for x in l64 + o64) and all(x.dtype == torch.float32 for x in l32 + o32)
    # measured (seeds 5, 11, 12; the worst): losses 5.4e-8 relative, outputs 6.7e-7 of their largest entry, trunk layers 4.1e-7,
    # gradients 8.3e-7 of the tensor's largest, running statistics 1.05e-7 of the largest
    for a, b in zip(l32, l64):
        a, b = float(a.detach()), float(b.detach())
        assert abs(a - b) <= 2e-7 * (1 + abs(b)), (a, b)
    for a, b in zip(o32, o64):
        assert float((a.double() - b).abs().max()) <= 2e-6 * float(b.abs().max())
    assert len(t32) == len(t64) == 1 + 2 * BLOCKS
    for (pre32, a32), (pre64, a64) in zip(t32, t64):
        assert torch.equal(a64, torch.relu(pre64))
        assert float((a32.double() - a64).abs().max()) <= 1.6e-6 * float(a64.abs().max())
    for k, t in p64.items():
        if t.requires_grad:
            g = t.grad
            assert float((p32[k].grad.double() - g).abs().max()) <= 2.5e-6 * float(g.abs().max()), k
        else:   # running statistics, updated by the training-mode forward
            assert float((p32[k].double() - t).abs().max()) <= 4e-7 * float(t.abs().max()), k


def test_kink_rule_acts_only_within_its_threshold_and_per_layer():
    import torch

    w, inputs = _inputs(6)
    _, (l0, o0, t0) = _run(w, inputs, torch.float64, return_layers=True)
    none = [torch.zeros_like(a, dtype=torch.bool) for _, a in t0]
    # threshold 0: the mask is never consulted, the graph is the plain one
    _, (l1, o1, t1) = _run(w, inputs, torch.float64, relu_masks=none, kink=0.0, return_layers=True)
    assert all(torch.equal(a, b) for a, b in zip(o0, o1))
    # an infinite threshold with the input's own signs as the mask is the plain graph too
    own = [pre.detach() > 0 for pre, _ in t0]
    _, (l2, o2) = _run(w, inputs, torch.float64, relu_masks=own, kink=float("inf"))
    assert all(torch.equal(a, b) for a, b in zip(o0, o2))
    # one threshold per layer: only layer 1 is forced shut, and only layer 1 is zero
    kinks = [0.0] * len(t0)
    kinks[1] = float("inf")
    _, (_, _, t3) = _run(w, inputs, torch.float64, relu_masks=none, kink=kinks, return_layers=True)
    assert torch.equal(t3[0][1], t0[0][1]) and float(t3[1][1].abs().max()) == 0.0
    assert float(t0[1][1].abs().max()) > 0 and float(t3[2][1].abs().max()) > 0
    # a finite threshold forces exactly the entries below it: here those of layer 0 within 0.05 of zero, shut
    pre = t0[0][0].detach()
    _, (_, _, t4) = _run(w, inputs, torch.float64, relu_masks=[own[0] & (pre.abs() >= 0.05)], kink=0.05, return_layers=True)
    forced = (pre.abs() < 0.05) & (pre > 0)
    assert int(forced.sum()) > 0
    assert torch.equal(t4[0][1], torch.where(forced, torch.zeros_like(pre), torch.relu(pre)))


@pytest.mark.parametrize("dtype_name", ["float32", "float64"])
def test_reference_defaults_to_the_parameters_dtype(dtype_name):
    import torch

    import learn_torch as LT

    dtype = getattr(torch, dtype_name)
    w, inputs = _inputs(7)
    p = LT.make_params(w, dtype)
    assert all(t.dtype == dtype for t in p.values())
    pol, val, ube = LT.forward_t(p, inputs[0], BLOCKS)
    assert pol.dtype == val.dtype == ube.dtype == dtype
