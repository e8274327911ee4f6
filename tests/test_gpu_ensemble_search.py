"""The searches over net4_ensemble, 64 games on 4x4: lock-step simulate with beta = 0.5, Gumbel halving (k = 16, budget 64) and
simulate_batch(leaves = 8) must equal, in every byte of the root statistics, the CPU oracle search driven by an agent that returns this
net's own policy_value_uncertainty (the way tests/test_gpu_lcghash.py holds its searches) - and the variance must steer: with beta = 0
some root's visit counts differ.  The UBE head is pushed down, so that var_16 and not expf(ube) is the variance the searches see."""
import numpy as np
import pytest

import ensemble_ref as R
import oracle_lib as O
from gpu_util import require_gpu

pytestmark = pytest.mark.gpu
B = 64


def spread_weights(seed=11):
    from takzero_amd import weights as W

    w = W.init_weights(W.ARCH_NET4_ENSEMBLE, seed=seed, trained_stats=True)
    for i in range(16):
        gain = np.float32(2.0 + 0.75 * i) * (1 if i % 2 else -1)
        w[R.name(i, "linear.weight")] = w[R.name(i, "linear.weight")] * gain
        w[R.name(i, "linear.bias")] = w[R.name(i, "linear.bias")] * gain
    w["ube.linear.bias"] = w["ube.linear.bias"] - np.float32(5.0)
    return w


def _net(A, oracle):
    """The exact net of tests/test_gpu_ensemble.py with its UBE head pushed down: its trunk output depends strongly on the position, so
    var_16 differs from child to child (0.03 .. 0.41 over the test positions; a random-init trunk gives 0.443 .. 0.445 on every
    opening, and the same bonus for every child steers nothing)."""
    from test_gpu_ensemble import exact

    w = dict(exact(oracle)["ens"])
    w["ube.linear.bias"] = w["ube.linear.bias"] - np.float32(16.0)
    return A.Net(arch=A.ARCH_NET4_ENSEMBLE, precision=A.PREC_F16).load_tensors(w)


def _pair(A, oracle, net, choice):
    from test_gpu_engine import _agent_over

    gpu = A.BatchedMCTS(B, 4, 4, agent=net, node_capacity=1 << 12)
    ora = O.OracleSearch(oracle, B, 4, 4, agent_kind=0, agent_fn=_agent_over(net))
    gpu.new_openings(choice)
    ora.new_openings(choice)
    return gpu, ora


def test_lock_step_gumbel_and_simulate_batch_against_the_oracle(oracle, tmp_path):
    A = require_gpu()
    from test_gpu_tree import assert_same_roots

    net = _net(A, oracle)
    choice = (np.arange(B) * 5 + 2).astype(np.int32) % 16
    betas = np.full(B, 0.5, np.float32)
    gpu, ora = _pair(A, oracle, net, choice)
    # the variance the searches see is var_16: on the roots it beats expf(ube) and stays below the clamp
    roots = gpu.get_positions()
    values = net.ensemble_values(roots)
    _, _, var = net.policy_value_uncertainty(roots, [O.possible_moves(oracle, O.TzState.from_buffer_copy(roots[i:i + 1].tobytes())) for i in range(B)])
    v16 = R.var16_f32(values)
    assert np.array_equal(var.view(np.uint32), np.minimum(v16, np.float32(4)).view(np.uint32)) and (v16 > 1e-4).all() and (v16 < 4).all()
    for phase in range(3):                       # two eager simulations, a captured one, replays
        gpu.simulate(betas, 8)
        ora.simulate(betas, 8)
        assert_same_roots(gpu, ora, "lock-step phase %d" % phase)
    assert np.array_equal(gpu.select_best_actions(), ora.select_best_actions()) and gpu.counters() == ora.counters()
    visits = gpu.root_children()["visits"].copy()
    ora.close()
    # beta = 0: the same search without the uncertainty bonus visits other children somewhere
    plain = A.BatchedMCTS(B, 4, 4, agent=net, node_capacity=1 << 12)
    plain.new_openings(choice)
    plain.simulate(np.zeros(B, np.float32), 24)
    other = plain.root_children(visits.shape[1])["visits"]
    differing = int((visits != other).any(axis=1).sum())
    print("beta 0.5 against beta 0: the visit counts of %d of %d roots differ" % (differing, B))
    assert differing >= 1
    # Gumbel sequential halving, 16 sampled actions, budget 64
    gpu, ora = _pair(A, oracle, net, choice)
    gumbel = np.random.default_rng(5).gumbel(size=(B, 512)).astype(np.float32)
    a = gpu.gumbel_sequential_halving(betas, 16, 64, gumbel)
    b = ora.gumbel_sequential_halving(betas, 16, 64, gumbel)
    assert np.array_equal(a, b)
    assert_same_roots(gpu, ora, "gumbel 16 / 64")
    assert gpu.counters() == ora.counters()
    ora.close()
    # simulate_batch: 8 leaves per tree per call, against the batched reference search with the same agent
    import simulate_batch_util as U
    from test_gpu_engine import _agent_over

    ref_lib = U.build(tmp_path)
    gpu2 = A.BatchedMCTS(B, 4, 4, agent=net, node_capacity=1 << 12)
    ref = U.RefSearch(ref_lib, B, 4, 4, agent_kind=0, agent_fn=_agent_over(net))
    gpu2.set_positions(np.arange(B), roots)
    ref.set_positions(np.arange(B), roots)
    for rounds in (1, 3):
        gpu2.simulate_batch(betas, 8, rounds)
        ref.simulate_batch(betas, 8, rounds)
        assert U.compare(gpu2, ref, "simulate_batch %d" % rounds) > B
    ref.close()
    net.close()
