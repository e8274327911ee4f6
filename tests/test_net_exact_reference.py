"""The integer-valued nets of tests/exact_net.py meet, on the CPU, the conditions under which every arithmetic of the HIP forward
must return the bits of the fp64 graph (tests/test_gpu_net_forms.py relies on them): asserted here for the test architecture at
3x3 and for the three shipped nets, three weight seeds each, on positions the calibration has not seen."""
import os
import sys

import numpy as np
import pytest

import exact_net as E
import oracle_lib as O

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))

NETS = [E.NETS[n] for n in (3, 5, 4, 6)]
POSITIONS = 128


@pytest.fixture(scope="module")
def boards(oracle):
    out = {}
    for n in (3, 4, 5, 6):
        states = E.distinct_positions(oracle, O, n, POSITIONS, 31)
        out[n] = (E.planes_of(oracle, O, E.distinct_positions(oracle, O, n, 96, 5), n), E.planes_of(oracle, O, states, n))
    return out


def test_positions_are_all_different_and_hold_the_special_ones(oracle):
    import ctypes as C

    for n in (3, 4, 5, 6):
        states = E.distinct_positions(oracle, O, n, 300, 3)
        arr = O.states_array(states)
        assert len({arr[i:i + 1].tobytes() for i in range(len(arr))}) == 300
        assert arr["ply"][0] == 0 and arr["height"][0].sum() == 0                       # the opening position
        assert (arr["height"][1][:n * n] > 0).all()                                     # a full board
        assert len(O.possible_moves(oracle, states[1])) > 0                             # stacks can still be spread: the Agent surface takes it
        assert all(oracle.tzo_terminal(C.byref(s)) == -1 for s in states[2:])
    wide = E.distinct_positions(oracle, O, 6, 8, 3)
    assert max(len(O.possible_moves(oracle, s)) for s in wide[2:5]) == 592


@pytest.mark.parametrize("seed", E.SEEDS)
@pytest.mark.parametrize("arch,n,blocks", NETS)
def test_generator_conditions(boards, arch, n, blocks, seed):
    import nets_torch as T
    import torch
    import torch.nn.functional as F

    calibration, planes = boards[n]
    w = E.exact_weights(arch, n, blocks, seed, calibration)
    # folded as bn_fold does it, in fp32: scale exactly 1, integer bias
    assert np.float32(np.float32(1) - np.float32(1e-5)) + np.float32(1e-5) == np.float32(1)
    for p, (scale, bias) in E.folded_batch_norms(w).items():
        assert np.all(scale == np.float32(1)) and np.array_equal(bias, np.rint(bias)), p
    # conv weights: {-1, 0, +1}, two entries per output channel; nothing on the non-dyadic input planes
    for name, v in w.items():
        if name.endswith("conv2d.weight") and v.shape[-1] == 3:
            assert set(np.unique(v)) <= {-1.0, 0.0, 1.0} and np.all((v != 0).sum(axis=(1, 2, 3)) == 2), name
    cin = planes.shape[1]
    dead = [c for c in range(cin) if c not in E.dyadic_input_channels(n)]
    assert len(dead) == 5 and not w["core.input_conv2d.weight"][:, dead].any()
    assert set(np.unique(planes[:, E.dyadic_input_channels(n)])) <= {0.0, 1.0}
    assert any(np.abs(planes[:, c] * 8 - np.rint(planes[:, c] * 8)).max() > 1e-3 for c in dead)     # and those planes are indeed not dyadic

    ref = E.exact_reference(w, planes, blocks)
    E.assert_reference_is_exact(ref)                      # every output and trunk activation within 1e-3 of its grid point, at most 256
    share = ref["stats"]["nonzero_share"]
    assert share.min() >= 0.10 and share.max() <= 0.60, share
    trace = []
    p32, v32, u32 = T.forward(w, planes, blocks, trace=trace)
    # the fp32 graph equals the rounded fp64 graph bit for bit (value: the same argument, tanh of two libraries)
    assert np.array_equal(p32.reshape(len(planes), -1).numpy(), ref["policy"]) and np.array_equal(u32.numpy(), ref["ube"])
    named = dict(trace)
    assert np.array_equal(named["value.pre"].numpy().astype(np.float64), ref["value_pre"])
    assert np.abs(v32.numpy() - ref["value"]).max() < 1e-6
    assert np.abs(ref["value_pre"]).max() < 8 and np.unique(ref["value"]).size >= 8                   # tanh not saturated, several values
    # per layer: channels alive, sum |w||x| below 2^24 with bias and residual, every square fed through every tap that lands on the board
    layers = [("core.input_conv2d", "core.batch_norm", torch.from_numpy(planes), None)]
    x = named["core.input"]
    for b in range(blocks):
        p = "core.res_block_%d" % b
        layers.append((p + ".a.conv2d", p + ".a.batch_norm", x, None))
        layers.append((p + ".b.conv2d", p + ".b.batch_norm", named[p + ".a"], x))
        x = named[p]
    layers.append(("policy.conv2d", None, x, None))
    for _, t in trace:
        if t.dim() == 4:
            assert bool((t != 0).any(dim=0).any(dim=-1).any(dim=-1).all())              # every channel non-zero somewhere in the batch
    for conv, norm, inp, res in layers:
        wt = torch.from_numpy(w[conv + ".weight"])
        bias = np.abs(w[norm + ".bias"] if norm else w[conv + ".bias"]).max()
        total = F.conv2d(inp.abs().double(), wt.abs().double(), padding=1).max() + float(bias) + (float(res.max()) if res is not None else 0.0)
        assert float(total) < 2 ** 24, conv
        assert not E.unfed_taps(wt.numpy(), inp.numpy()), conv


def test_forward_dtype_argument_leaves_the_fp32_default_alone(oracle):
    import nets_torch as T
    import torch
    from takzero_amd import weights as W

    w = W.init_weights(W.ARCH_TEST, n=4, blocks=2, seed=3, trained_stats=True)
    planes = E.planes_of(oracle, O, E.distinct_positions(oracle, O, 4, 12, 1), 4)
    a = T.forward(w, planes, 2)
    b = T.forward(w, planes, 2, dtype=torch.float32)
    c = T.forward(w, planes, 2, dtype=torch.float64)
    assert all(x.dtype == torch.float32 and torch.equal(x, y) for x, y in zip(a, b))
    assert all(z.dtype == torch.float64 and float((x.double() - z).abs().max()) < 1e-5 for x, z in zip(a, c))
