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
