"""CPU side of tz_search_set_selection: the restatement the GPU tests compare against (tests/selection_ref.cpp) tied to the pinned
oracle under PUCT, the known answer of UCT, the scores of UCT and of the improved policy recomputed in numpy float32, and the
declarations of the new entry points.  Every comparison is on bits."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_lib as O
import selection_util as S
import simulate_batch_util as U
from gpu_util import random_positions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINUE = "a3 c1 c2 c3 b3 c3-"        # the start of the reference's find_tinue_easy, mcts.rs:352


@pytest.fixture(scope="module")
def ref_lib(tmp_path_factory):
    return S.build(tmp_path_factory.mktemp("selection_ref"))


@pytest.fixture(scope="module")
def batch_lib(tmp_path_factory):
    return U.build(tmp_path_factory.mktemp("simulate_batch_ref"))


def position(oracle, n, half_komi, ptn):
    s = O.state_default(oracle, n, half_komi)
    for mv in ptn.split():
        s = O.play(oracle, s, O.from_ptn(oracle, n, mv))
    return s


def wide_position(oracle):
    """a 5x5 playout position with more than 128 legal moves"""
    wide = S.wide_positions(oracle)[1]
    assert len(O.possible_moves(oracle, wide)) > 128
    return wide


# ---- 1. under PUCT the restatement is the oracle
CASES = [("3x3 simple", 3, 0, 2, 1, 1.0, 500), ("5x5 dummy", 5, 4, 1, 8, 0.25, 100)]


def _start(search, n, B):
    if n == 3:
        search.set_positions(np.arange(B), [O.state_default(O.load(), 3, 0)] * B)
    else:
        search.new_openings((np.arange(B) * 3 + 1).astype(np.int32) % 16)


@pytest.mark.parametrize("name,n,komi,agent,B,beta,sims", CASES, ids=[c[0] for c in CASES])
def test_puct_lock_step_is_the_oracle(oracle, ref_lib, name, n, komi, agent, B, beta, sims):
    betas = np.full(B, beta, np.float32)
    ref = S.RefSearch(ref_lib, B, n, komi, agent_kind=agent, rule=S.PUCT)
    ora = O.OracleSearch(oracle, B, n, komi, agent_kind=agent)
    _start(ref, n, B)
    _start(ora, n, B)
    ref.simulate(betas, sims)
    ora.simulate(betas, sims)
    assert S.compare(ora, ref, name) > 10 * B
    assert int(ref.node(0, [])[0]["visit_count"]) == sims


@pytest.mark.parametrize("name,n,komi,agent,B,beta,sims", CASES, ids=[c[0] for c in CASES])
def test_puct_simulate_batch_is_the_restated_simulate_batch(ref_lib, batch_lib, name, n, komi, agent, B, beta, sims):
    betas = np.full(B, beta, np.float32)
    leaves = 4
    ref = S.RefSearch(ref_lib, B, n, komi, agent_kind=agent, rule=S.PUCT)
    old = U.RefSearch(batch_lib, B, n, komi, agent_kind=agent)
    _start(ref, n, B)
    _start(old, n, B)
    ref.simulate_batch(betas, leaves, sims // leaves)
    old.simulate_batch(betas, leaves, sims // leaves)
    assert S.compare(old, ref, name) > 10 * B


@pytest.mark.parametrize("name,n,komi,agent,B,beta,sims", CASES, ids=[c[0] for c in CASES])
def test_puct_gumbel_halving_is_the_oracle(oracle, ref_lib, name, n, komi, agent, B, beta, sims):
    betas = np.full(B, beta, np.float32)
    k, budget = (4, 32) if n == 3 else (16, 64)
    gumbel = np.random.default_rng(5).gumbel(size=(B, 512)).astype(np.float32)
    ref = S.RefSearch(ref_lib, B, n, komi, agent_kind=agent, rule=S.PUCT)
    ora = O.OracleSearch(oracle, B, n, komi, agent_kind=agent)
    _start(ref, n, B)
    _start(ora, n, B)
    assert np.array_equal(ref.gumbel_sequential_halving(betas, k, budget, gumbel), ora.gumbel_sh(betas, k, budget, gumbel))
    assert S.compare(ora, ref, name) > 10 * B


# ---- 2. the known answer of UCT: ln(N) / 0 = +inf, and ties go to the last index
def test_uct_visits_the_unvisited_children_from_the_last_to_the_first(oracle, ref_lib):
    starts = {3: [O.state_default(oracle, 3, 0)], 5: [O.state_default(oracle, 5, 4), wide_position(oracle)]}
    for n, komi in ((3, 0), (5, 4)):
        for start in starts[n]:
            nc = len(O.possible_moves(oracle, start))
            ref = S.RefSearch(ref_lib, 1, n, komi, agent_kind=1, rule=S.UCT)
            ref.set_positions([0], [start])
            betas = np.zeros(1, np.float32)
            ref.simulate(betas, 1)
            assert len(ref.root_visits(0)) == nc and not ref.root_visits(0).any()
            done = 0
            for k in sorted({1, 2, nc // 2, 65 if nc > 65 else 1, nc - 1}):
                ref.simulate(betas, k - done)
                done = k
                v = ref.root_visits(0)
                assert v[nc - k:].tolist() == [1] * k and not v[:nc - k].any(), (n, nc, k, v)
            ref.simulate(betas, nc - done)
            assert ref.root_visits(0).tolist() == [1] * nc
            assert int(ref.node(0, [])[0]["visit_count"]) == 1 + nc and not ref.nan_seen()


# ---- 3. the index each rule selects at a root is the arg-max of its formula, recomputed in numpy float32
def _last_argmax(score, eligible):
    idx = np.flatnonzero(eligible)
    s = score[idx]
    assert not np.isnan(s).any()
    return int(idx[len(s) - 1 - int(np.argmax(s[::-1]))])


def _q_values(oracle, tag, bits_):
    """child.q_value() = NotNan::from(evaluation.negate()), node/mod.rs:114-124"""
    neg = {O_WIN: O_LOSS, O_LOSS: O_WIN, O_DRAW: O_DRAW}
    out = np.zeros(len(tag), np.float32)
    for i, (t, b) in enumerate(zip(tag, bits_)):
        out[i] = -np.uint32(b).view(np.float32) if t == 0 else oracle.tzo_eval_to_f32(neg[int(t)], int(b) + 1)
    return out


O_WIN, O_LOSS, O_DRAW = 1, 2, 3


@pytest.mark.parametrize("name,n,komi,agent,ptn", [("3x3 tinue", 3, 0, 1, TINUE), ("5x5 simple", 5, 4, 2, "a5 e1 c3 d3")])
def test_the_selected_index_is_the_arg_max_of_the_formula(oracle, ref_lib, name, n, komi, agent, ptn):
    start = position(oracle, n, komi, ptn)
    for beta, sims in ((0.5, 50), (0.0, 3000 if n == 3 else 50)):
        betas = np.full(1, beta, np.float32)
        ref = S.RefSearch(ref_lib, 1, n, komi, agent_kind=agent, rule=S.PUCT)
        ora = O.OracleSearch(oracle, 1, n, komi, agent_kind=agent)
        ref.set_positions([0], [start])
        ora.set_positions([0], [start])
        ref.simulate(betas, sims)
        ora.simulate(betas, sims)       # the same tree (test 1), so the oracle's own improved_policy wrapper speaks for it
        info, ch = ora.node(0, [])
        nc, V = int(info["n_children"]), int(info["visit_count"])
        visits = ch["visits"].astype(np.float32)
        eligible = (info["eval_tag"] == O_LOSS) | (ch["eval_tag"] != O_WIN)
        # improved: pi - n / (N + 1) with N the root's visit count after this forward's increment (policy.rs:64-66)
        pi = ora.improved_policy(float(ch["visits"].max()))[0, :nc]
        score = (pi - visits / np.float32(np.uint32(V + 1) + np.uint32(1))).astype(np.float32)
        assert ref.select_at_root(0, S.IMPROVED, beta) == _last_argmax(score, eligible), (name, beta)
        # uct: (q + sqrt(ln N / n)) + std_dev * beta (policy.rs:110-114, 158-164), ln from the library both sides use
        ln = np.float32(ref_lib.sel_m_ln(np.float32(V + 1)))
        with np.errstate(divide="ignore"):
            uct = np.sqrt(ln / visits).astype(np.float32)
        score = ((_q_values(oracle, ch["eval_tag"], ch["eval_bits"]) + uct).astype(np.float32) + ch["std_dev"] * np.float32(beta)).astype(np.float32)
        assert ref.select_at_root(0, S.UCT, beta) == _last_argmax(score, eligible), (name, beta)
        if n == 3 and beta == 0.0:
            assert (ch["eval_tag"] == O_WIN).any() or info["eval_tag"] != 0      # the win filter or a solved root is in play


# ---- 4. the rules differ, so a setter that does nothing cannot pass the GPU tests
def test_the_three_rules_give_different_trees(ref_lib):
    B, sims = 8, 200
    betas = np.zeros(B, np.float32)
    visits = {}
    for rule in (S.PUCT, S.UCT, S.IMPROVED):
        ref = S.RefSearch(ref_lib, B, 5, 4, agent_kind=2, rule=rule)
        ref.new_openings((np.arange(B) * 3 + 1).astype(np.int32) % 16)
        ref.simulate(betas, sims)
        visits[rule] = [ref.root_visits(g) for g in range(B)]
        assert not ref.nan_seen()
    for a, b in ((S.PUCT, S.UCT), (S.PUCT, S.IMPROVED), (S.UCT, S.IMPROVED)):
        assert any(not np.array_equal(x, y) for x, y in zip(visits[a], visits[b])), (a, b)


# ---- declarations
def test_the_header_declares_the_rules_and_both_entry_points():
    header = open(os.path.join(ROOT, "include", "takzero_hip.h")).read()
    assert re.search(r"int tz_search_set_selection\(tz_search\* s, int rule\);", header)
    assert re.search(r"int tz_search_get_selection\(tz_search\* s, int\* rule_out\);", header)
    for name, value, lines in (("PUCT", 0, "78-95"), ("UCT", 1, "104-117"), ("IMPROVED", 2, "57-69")):
        assert re.search(r"#define TZ_SELECT_%s %d\s+/\*[^\n]*policy\.rs:%s" % (name, value, lines), header), name


def test_the_python_api_has_the_setter_the_property_and_the_constants():
    import takzero_amd.api as A

    assert (A.SELECT_PUCT, A.SELECT_UCT, A.SELECT_IMPROVED) == (0, 1, 2)
    assert callable(A.BatchedMCTS.set_selection) and isinstance(A.BatchedMCTS.selection, property)
    assert {"tz_search_set_selection", "tz_search_get_selection"} <= set(A._lib.SYMBOLS)
    lib = A._lib.load()
    assert hasattr(lib, "tz_search_set_selection") and hasattr(lib, "tz_search_get_selection")
