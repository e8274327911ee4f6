"""tz_search_simulate_batch at the widths it is benchmarked at, against the CPU restatement of Node::simulate_batch
(tests/simulate_batch_ref.cpp through simulate_batch_util.RefSearch), bit for bit as in tests/test_gpu_simulate_batch.py.

What the narrow module (B <= 5 trees) cannot reach:

  1. compact_batch_kernel's offsets past lane 4 of wave 0: per-wave scans, the sixteen wave sums and the carry across 1024-tree
     chunks, with trees that collect 0, some and all of their leaves in the same round (offset[] and index[] are then not g * leaves + j);
  2. the same raggedness feeding a network call through the index gather, with a full round of 1040 positions and ragged ones below 1024;
  3. more than 4096 positions in one network call (5120), which also grows the net's work buffers from inside simulate_batch;
  4. the SimHash launch reading `index`, with a populated set so that std_dev depends on the gathered position;
  5. 6x6 and 3x3 through a network;
  6. leaf scratch growing on a handle that also runs lock-step simulations (captured as a HIP graph) between the calls.

Wide cases compare the root and all root children of every tree, and walk depth 2 and the principal variation on trees 0, 63, 64, 65,
1023, 1024, 1025 and B - 1 where they exist.  Each case first asserts, on the restatement alone, that the committed seeds still
produce the edge it is there for; tests/test_simulate_batch_ref.py holds those of case 1 without a GPU."""
import numpy as np
import pytest

import oracle_lib as O
import simulate_batch_util as U
from gpu_util import require_gpu
from test_gpu_simulate_batch import _agent_over, _counters_match

pytestmark = pytest.mark.gpu

WIDE_SEED = 1


@pytest.fixture(scope="module")
def ref_lib(tmp_path_factory):
    return U.build(tmp_path_factory.mktemp("simulate_batch_ref_wide"))


def _betas(B):
    return np.where(np.arange(B) % 2 == 0, 0.0, 0.25).astype(np.float32)


def _test_net(A, n, blocks, precision, seed=123):
    from takzero_amd import weights as W

    return A.Net(arch=A.ARCH_TEST, n=n, precision=A.PREC_NAMES[precision], blocks=blocks).load_tensors(
        W.init_weights(W.ARCH_TEST, n=n, blocks=blocks, seed=seed))


# ---- 1. offsets across waves and chunks, ragged
@pytest.mark.parametrize("agent", [1, 2], ids=["dummy", "simple"])
def test_offsets_across_waves_and_chunks_with_ragged_trees(oracle, ref_lib, agent):
    B, n, leaves, rounds = 1100, 4, 8, 3
    starts = U.mixed_starts(oracle, B, n, 4, WIDE_SEED)
    betas = _betas(B)
    ref = U.RefSearch(ref_lib, B, n, 4, agent_kind=agent)
    U.apply_starts(ref, starts)
    per_round = []
    for _ in range(rounds):
        ref.simulate_batch(betas, leaves, 1)
        per_round.append(ref.round_leaves())
    # on the reference alone, before the GPU is touched
    assert any(U.ragged(r, leaves) for r in per_round), [np.bincount(r, minlength=leaves + 1).tolist() for r in per_round]
    assert ref.counts()["short_rounds"] > 0
    ref.close()
    A = require_gpu()
    ref = U.RefSearch(ref_lib, B, n, 4, agent_kind=agent)
    gpu = A.BatchedMCTS(B, n, 4, agent_kind=agent, node_capacity=1 << 12)
    U.apply_starts(ref, starts)
    U.apply_starts(gpu, starts)
    deep = U.deep_trees(B)
    assert deep == [0, 63, 64, 65, 1023, 1024, 1025, 1099]
    for r in range(rounds):
        ref.simulate_batch(betas, leaves, 1)
        gpu.simulate_batch(betas, leaves, 1)
        assert np.array_equal(ref.round_leaves(), per_round[r])
        assert U.compare(gpu, ref, "round %d" % r, deep=deep) >= B
        _counters_match(gpu, ref)
    assert gpu.pool_overflows() == 0


# ---- 2. the same raggedness through a network
@pytest.mark.parametrize("precision", ["f32", "f16"])
def test_ragged_rounds_through_a_network(oracle, ref_lib, precision):
    """130 trees x 8 leaves = 1040 slots: the net's launch is sized for 1040 positions in every round, the number it evaluates is read
    on the device.  A round can only be full while every tree is alive, and a finished start never collects a leaf, so round one runs
    from fresh openings on every tree (1040 positions); then the start mix of case 1 is set on the trees it names and rounds two to
    four are ragged (the trees that keep their opening keep their subtree)."""
    A = require_gpu()
    B, n, leaves, rounds = 130, 4, 8, 4
    net = _test_net(A, n, 1, precision, seed=7)
    choice, idx, states = U.mixed_starts(oracle, B, n, 4, WIDE_SEED)
    betas = _betas(B)
    deep = U.deep_trees(B)

    ref = U.RefSearch(ref_lib, B, n, 4, agent_kind=0, agent_fn=_agent_over(net))
    gpu = A.BatchedMCTS(B, n, 4, agent=net, node_capacity=1 << 12)
    ref.new_openings(choice)
    gpu.new_openings(choice)
    totals, before, ragged = [], 0, []
    for r in range(rounds):
        if r == 1:
            ref.set_positions(idx, states)
            gpu.set_positions(idx, O.states_array(states))
        ref.simulate_batch(betas, leaves, 1)
        gpu.simulate_batch(betas, leaves, 1)
        now = ref.counts()["leaves"]
        totals.append(now - before)
        before = now
        ragged.append(U.ragged(ref.round_leaves(), leaves))
        assert U.compare(gpu, ref, "%s round %d" % (precision, r), deep=deep) >= B
        _counters_match(gpu, ref)
    print("leaves per round:", totals)
    assert any(t == B * leaves == 1040 for t in totals), totals                # a full round, past 1024
    assert any(0 < t < 1024 and rg for t, rg in zip(totals, ragged)), (totals, ragged)      # a ragged one below it
    assert gpu.pool_overflows() == 0


# ---- 3. more than 4096 positions in one network call
@pytest.mark.parametrize("blocks,precision", [(2, "f16"), (2, "f16x2"), (3, "f16c6")])
def test_more_than_4096_positions_in_one_network_call(ref_lib, blocks, precision):
    """40 fresh 5x5 openings x 128 leaves: round one is 5120 copies of roots in one call, for which simulate_batch grows the net's
    work buffers (for f16c6 - the ARCH_TEST entry (100, 5, 3, 19) of test_gpu_net.C6_NETS - its seed scratch too) from the 40
    positions the handle's creation sized them for."""
    from test_gpu_net import C6_NETS

    A = require_gpu()
    assert (100, 5, 3, 19) in C6_NETS
    B, n, leaves, rounds = 40, 5, 128, 2
    net = _test_net(A, n, blocks, precision)
    choice = (np.arange(B) * 3 + 1).astype(np.int32) % 16
    betas = _betas(B)
    ref = U.RefSearch(ref_lib, B, n, 4, agent_kind=0, agent_fn=_agent_over(net))
    ref.new_openings(choice)
    ref.simulate_batch(betas, leaves, 1)
    assert ref.counts()["leaves"] == B * leaves == 5120 > 4096
    ref.simulate_batch(betas, leaves, rounds - 1)
    gpu = A.BatchedMCTS(B, n, 4, agent=net, node_capacity=1 << 14)
    gpu.new_openings(choice)
    gpu.simulate_batch(betas, leaves, rounds)
    assert U.compare(gpu, ref, precision, deep=U.deep_trees(B)) >= B
    _counters_match(gpu, ref)
    assert gpu.pool_overflows() == 0


# ---- 4. SimHash through the leaf gather
def test_simhash_reads_the_gathered_leaves(oracle, ref_lib):
    """net4_simhash with the constant UBE head of tests/test_gpu_simhash.py (variance 0.5 on seen positions, 4 on the others).  A first
    run of the restatement over the net with its empty set records the positions the search reaches; every second distinct index among
    them is marked as seen; the compared run's std_dev then depends on which position the in-search hash launch read for each slot."""
    from takzero_amd import weights as W
    from test_gpu_engine import _watched
    from test_gpu_simhash import constant_ube

    A = require_gpu()
    B, n, leaves, rounds = 5, 4, 32, 4
    net = A.Net(arch=A.ARCH_NET4_SIMHASH, precision=A.PREC_F16).load_tensors(
        constant_ube(W.init_weights(W.ARCH_NET4_SIMHASH, seed=3), float(np.float32(np.log(0.5)))))
    choice = (np.arange(B) * 3 + 1).astype(np.int32) % 16
    betas = _betas(B)
    met = []
    first = U.RefSearch(ref_lib, B, n, 4, agent_kind=0, agent_fn=_watched(_agent_over(net), states_seen=met))
    first.new_openings(choice)
    first.simulate_batch(betas, leaves, rounds)
    first.close()
    distinct = np.concatenate(list({s.tobytes(): s for s in met}.values()))
    idx = net.hash_indices(distinct)
    order = np.sort(np.unique(idx, return_index=True)[1])
    assert len(order) >= 8, len(order)
    net.hash_indices(distinct[np.isin(idx, idx[order[::2]])], update=True)
    variances = []
    ref = U.RefSearch(ref_lib, B, n, 4, agent_kind=0, agent_fn=_watched(_agent_over(net), variances=variances))
    gpu = A.BatchedMCTS(B, n, 4, agent=net, node_capacity=1 << 13)
    ref.new_openings(choice)
    gpu.new_openings(choice)
    for r in range(rounds):
        ref.simulate_batch(betas, leaves, 1)
        gpu.simulate_batch(betas, leaves, 1)
        assert U.compare(gpu, ref, "simhash round %d" % r) > 20
        _counters_match(gpu, ref)
    var = np.array(variances, np.float32)
    assert np.all((var == 4) | np.isclose(var, 0.5, rtol=1e-6, atol=0))
    # both levels went into the compared trees, and the visited root children do not all carry the same std_dev
    assert (var == 4).sum() >= 10 and (var < 4).sum() >= 10, ((var == 4).sum(), (var < 4).sum())
    stds = np.concatenate([c["std_dev"][c["visits"] > 0] for c in (ref.node(g, [])[1] for g in range(B))])
    assert np.unique(stds).size >= 2, stds[:8]


# ---- 5. 6x6 and 3x3
@pytest.mark.parametrize("n", [6, 3])
def test_six_by_six_and_three_by_three_through_a_network(oracle, ref_lib, n):
    from exact_net import WIDE_6X6

    A = require_gpu()
    B, leaves, rounds = 3, 16, 4
    komi = 4 if n == 6 else 0
    net = _test_net(A, n, 2, "f16")
    betas = _betas(B)
    ref = U.RefSearch(ref_lib, B, n, komi, agent_kind=0, agent_fn=_agent_over(net))
    gpu = A.BatchedMCTS(B, n, komi, agent=net, node_capacity=1 << 15)
    if n == 6:
        starts = [O.state_from_tps(oracle, t, n, komi) for t in WIDE_6X6]
        ref.set_positions(np.arange(B), starts)
        gpu.set_positions(np.arange(B), O.states_array(starts))
    else:
        choice = np.array([0, 5, 10], np.int32)
        ref.new_openings(choice)
        gpu.new_openings(choice)
    for r in range(rounds):
        ref.simulate_batch(betas, leaves, 1)
        gpu.simulate_batch(betas, leaves, 1)
        assert U.compare(gpu, ref, "%dx%d round %d" % (n, n, r)) > 10
        _counters_match(gpu, ref)
    assert ref.counts()["leaves"] > leaves * B
    assert gpu.pool_overflows() == 0


# ---- 6. scratch growth beside lock-step
def test_leaf_scratch_grows_beside_lock_step_simulations(ref_lib):
    """simulate / simulate_batch alternating on one handle: six lock-step simulations are two eager ones, a capture and three replays,
    and simulate_batch(leaves=64) in between replaces the leaf scratch and grows the net's work buffers (8 -> 512 positions) that the
    captured simulation names.  The restatement makes the same calls (sbr_simulate is BatchedMCTS::simulate over the same trees)."""
    A = require_gpu()
    B, n = 8, 5
    net = _test_net(A, n, 2, "f16")
    choice = (np.arange(B) * 3 + 1).astype(np.int32) % 16
    betas = _betas(B)
    ref = U.RefSearch(ref_lib, B, n, 4, agent_kind=0, agent_fn=_agent_over(net))
    gpu = A.BatchedMCTS(B, n, 4, agent=net, node_capacity=1 << 14)
    ref.new_openings(choice)
    gpu.new_openings(choice)
    for step, (call, arg) in enumerate([("simulate", 6), ("simulate_batch", 4), ("simulate", 6), ("simulate_batch", 64), ("simulate", 6),
                                        ("simulate_batch", 4)]):
        getattr(ref, call)(betas, arg)
        getattr(gpu, call)(betas, arg)
        assert U.compare(gpu, ref, "step %d: %s(%d)" % (step, call, arg)) > 10
        _counters_match(gpu, ref)
    assert gpu.pool_overflows() == 0
