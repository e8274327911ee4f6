"""CPU side of tz_search_simulate_batch / tz_search_principal_variation: the restatement the GPU tests compare against
(tests/simulate_batch_ref.cpp) tied to the pinned oracle, its visit accounting, and the declarations of the new entry points."""
import os
import re

import numpy as np
import pytest

import oracle_lib as O
import simulate_batch_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ref_lib(tmp_path_factory):
    return U.build(tmp_path_factory.mktemp("simulate_batch_ref"))


@pytest.mark.parametrize("agent", [1, 2])
def test_one_leaf_per_round_is_the_lock_step_search_of_the_oracle(ref_lib, agent):
    """leaves = 1 from a 5x5 opening: with no Known result inside a round, a round is one simulate_simple, which is what
    BatchedMCTS::simulate does for one game: node for node the same tree"""
    oracle = O.load()
    rounds = 60
    ref = U.RefSearch(ref_lib, 1, 5, 4, agent_kind=agent)
    ora = O.OracleSearch(oracle, 1, 5, 4, agent_kind=agent)
    ref.new_openings([3])
    ora.new_openings([3])
    betas = np.array([0.25], np.float32)
    ref.simulate_batch(betas, 1, rounds)
    ora.simulate(betas, rounds)
    c = ref.counts()
    assert c["known_in_round"] == 0 and c["forwards"] == rounds and c["leaves"] == rounds and c["duplicate_leaves"] == 0, c
    ref_pv = ref.principal_variation

    class WithPv:       # OracleSearch has no principal_variation: walk the PV nodes of the restatement in the oracle's tree
        batch = 1
        node = staticmethod(ora.node)
        principal_variation = staticmethod(ref_pv)

    assert U.compare(ref, WithPv, "leaves=1") > 50
    assert ref.node(0, [])[0]["visit_count"] == rounds


@pytest.mark.parametrize("leaves", [2, 128])
def test_root_visits_grow_by_the_forwards_made(ref_lib, leaves):
    ref = U.RefSearch(ref_lib, 1, 5, 4, agent_kind=2)
    ref.new_openings([5])
    betas = np.zeros(1, np.float32)
    before_v, before_f = 0, 0
    for call in range(4):
        ref.simulate_batch(betas, leaves, 1)
        v, f = int(ref.node(0, [])[0]["visit_count"]), ref.counts()["forwards"]
        assert v - before_v == f - before_f and f - before_f >= leaves, (call, v, f)
        before_v, before_f = v, f
    c = ref.counts()
    assert c["duplicate_leaves"] >= leaves - 1, c      # the first round stops `leaves` times at the fresh root


@pytest.mark.parametrize("agent", [1, 2])
def test_lock_step_simulate_of_the_restatement_is_the_oracle_search(ref_lib, agent):
    """sbr_simulate (the lock-step calls of tests/test_gpu_simulate_batch_wide.py's last case) against BatchedMCTS::simulate of the
    pinned oracle: several games, one of them finished, root and children of every game and depth 2, and the same event counts"""
    oracle = O.load()
    B, n = 4, 4
    starts = [U.finished_position(oracle, n, 4, 5)]
    ref = U.RefSearch(ref_lib, B, n, 4, agent_kind=agent)
    ora = O.OracleSearch(oracle, B, n, 4, agent_kind=agent)
    for s in (ref, ora):
        s.new_openings([1, 4, 7, 10])
        s.set_positions([2], starts)
    betas = np.array([0.0, 0.25, 0.0, 0.5], np.float32)
    for sims in (1, 40):
        ref.simulate(betas, sims)
        ora.simulate(betas, sims)

    class NoPv:
        batch = B
        node = staticmethod(ora.node)

    assert U.compare(ref, NoPv, "lock-step") > 50
    c = ref.counts()
    assert (c["forwards"], c["leaves"]) == ora.counters() and c["leaves"] < c["forwards"] == 41 * B, (c, ora.counters())


@pytest.mark.parametrize("agent", [1, 2])
def test_the_wide_start_mix_gives_ragged_rounds(ref_lib, agent):
    """The preconditions of the 1100-tree case of tests/test_gpu_simulate_batch_wide.py, with its seed, without a GPU: in one round
    some tree collects nothing, some tree between 1 and leaves - 1, some tree all of its leaves; finished starts collect nothing; and the trees walked in depth are the
    ones on either side of the 64-tree and 1024-tree boundaries."""
    from test_gpu_simulate_batch_wide import WIDE_SEED

    oracle = O.load()
    B, n, leaves = 1100, 4, 8
    starts = U.mixed_starts(oracle, B, n, 4, WIDE_SEED)
    assert all(oracle.tzo_terminal(starts[2][k]) != -1 for k in range(0, len(starts[1]), 2))       # g % 3 == 1: finished
    assert all(oracle.tzo_terminal(starts[2][k]) == -1 for k in range(1, len(starts[1]), 2))       # g % 3 == 2: still running
    ref = U.RefSearch(ref_lib, B, n, 4, agent_kind=agent)
    U.apply_starts(ref, starts)
    betas = np.where(np.arange(B) % 2 == 0, 0.0, 0.25).astype(np.float32)
    seen, total = [], 0
    for _ in range(3):
        ref.simulate_batch(betas, leaves, 1)
        r = ref.round_leaves()
        seen.append(U.ragged(r, leaves))
        total += int(r.sum())
        assert r.max() <= leaves and np.all(r[1::3] == 0) and total == ref.counts()["leaves"]
    assert any(seen) and ref.counts()["short_rounds"] > 0
    assert U.deep_trees(B) == [0, 63, 64, 65, 1023, 1024, 1025, 1099] and U.deep_trees(5) == [0, 4]


def test_the_header_declares_both_entry_points():
    header = open(os.path.join(ROOT, "include", "takzero_hip.h")).read()
    assert re.search(r"int tz_search_simulate_batch\(tz_search\* s, const float\* betas, int leaves, int rounds\);", header)
    assert re.search(r"int tz_search_principal_variation\(tz_search\* s, int game, uint16_t\* moves_out, int cap, int\* len_out\);", header)
    bound = int(re.search(r"#define TZ_SIMULATE_BATCH_MAX_SLOTS (\d+)", header).group(1))
    assert bound >= 1 * 1024 and bound >= 128 * 32


def test_the_python_api_has_both_methods():
    import takzero_amd.api as A

    assert callable(A.BatchedMCTS.simulate_batch) and callable(A.BatchedMCTS.principal_variation)
    assert {"tz_search_simulate_batch", "tz_search_principal_variation"} <= set(A._lib.SYMBOLS)
    lib = A._lib.load()
    assert hasattr(lib, "tz_search_simulate_batch") and hasattr(lib, "tz_search_principal_variation")
