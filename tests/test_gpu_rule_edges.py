"""The device Tak rules, the searches built on them, the net's input encoder and Gumbel sequential halving against the CPU oracle at
the edges that uniformly random playouts do not reach (edge_positions.py; test_edge_positions.py proves on the CPU that the
fixture reaches them): the 100-ply draw and the resets of its counter, reserves that run empty, a capstone as the only piece left to
place, full boards, stacks whose colours cross bit 32 of colors[], the komi comparison on both sides of a draw, a spread that
completes both colours' roads, and halving with fewer root children than sampled actions.  Everything is compared for equality:
bytes of tz_state, move lists, tags, bit patterns of floats.  Dummy / Simple agents unless a test says otherwise."""
import ctypes as C

import numpy as np
import pytest

import edge_positions as E
import oracle_lib as O
from gpu_util import require_gpu
from test_gpu_tree import assert_same_roots

pytestmark = pytest.mark.gpu
SIZES = (3, 4, 5, 6)
STRIDE = 37
# Round r plays child (r * STRIDE) % n_children, which is the first child in round 0; round 1 plays the last child instead, which no
# fixed stride reaches for every child count.  Rounds 6 to 8 play the moves the fixture names for a position (out of the tall stack,
# onto it, off the 99th ply, into the double road); a position with fewer named moves goes on with the stride, so every position is
# stepped nine times.
STRIDE_ROUNDS = 6
DIRECTED_ROUNDS = 3
EVAL_TAG = {0: 1, 1: 2, 2: 3}                # TZ_TERMINAL_WIN / LOSS / DRAW -> TZ_EVAL_WIN / LOSS / DRAW
_moves = {}


def _legal(oracle, n):
    """possible_moves of every fixture position of one size ([] where the game is over), computed once."""
    if n not in _moves:
        _moves[n] = [O.possible_moves(oracle, s) if oracle.tzo_terminal(C.byref(s)) == -1 else [] for _, s in E.fixture(oracle, n).positions]
    return _moves[n]


def _check_roots(oracle, n, gpu, states, moves, ctx):
    """After one simulation on fresh trees the root's children are the legal moves in order, or the root carries the result."""
    info = gpu.root_info()
    ch = gpu.root_children(max(1, int(info["n_children"].max())))
    for g, (s, mv) in enumerate(zip(states, moves)):
        where = (ctx, n, g, O.to_tps(oracle, s), s.reversible_plies, list(s.stones), list(s.caps), s.half_komi)
        term = oracle.tzo_terminal(C.byref(s))
        assert int(info["is_terminal_env"][g]) == (term != -1), where
        assert int(info["n_children"][g]) == len(mv), where
        if term != -1:
            assert int(info["eval_tag"][g]) == EVAL_TAG[term], where
        else:
            assert int(info["eval_tag"][g]) == 0, where
            assert list(ch["move_idx"][g, :len(mv)]) == mv, where


@pytest.mark.parametrize("n", SIZES)
def test_device_rules_match_the_oracle_at_the_edges(oracle, n):
    """gen_moves, terminal (with reason and winner) and apply_move on every fixture position of one size."""
    A = require_gpu()
    fx = E.fixture(oracle, n)
    labels, states = [label for label, _ in fx.positions], [s for _, s in fx.positions]
    B, hk = len(states), fx.half_komi
    arr, every, betas = O.states_array(states), np.arange(B), np.zeros(B, np.float32)
    moves = _legal(oracle, n)
    gpu = A.BatchedMCTS(B, n, hk, agent_kind=A.AGENT_DUMMY, node_capacity=4096)
    ora = O.OracleSearch(oracle, B, n, hk, agent_kind=1)

    # terminal, reason and winner; the games that are over restart from an opening, the others stay
    gpu.set_positions(every, arr)
    ora.set_positions(every, states)
    tg, to = gpu.restart_terminal_envs(np.zeros(B, np.int32)), ora.restart_terminal(np.zeros(B, np.int32))
    assert np.array_equal(tg, to), [(labels[g], int(tg[g]), int(to[g])) for g in np.nonzero(tg != to)[0][:8]]
    (rg, wg), (ro, wo) = gpu.terminal_details(), ora.terminal_details()
    over = to != -1
    assert np.array_equal(rg[over], ro[over]) and np.array_equal(wg[over], wo[over]), [labels[g] for g in np.nonzero(over & ((rg != ro) | (wg != wo)))[0][:8]]
    assert np.array_equal(rg[~over], np.zeros((~over).sum(), np.int8))
    for reason, label in ((3, "shuffle/100"), (3, "crowd/100"), (2, "walls/full"), (2, "komi/draw"), (1, "road2/after-white")) + (((2, "deplete/end"),) if n >= 4 else ()):
        assert all(rg[g] == reason for g in range(B) if labels[g] == label), label
    assert gpu.get_positions().tobytes() == ora.get_positions().tobytes()

    for r in range(STRIDE_ROUNDS + DIRECTED_ROUNDS):
        gpu.set_positions(every, arr)
        gpu.simulate(betas, 1)
        if r == 0:
            _check_roots(oracle, n, gpu, states, moves, "fixture")
        acts, after = np.zeros(B, np.uint16), []
        for g, mv in enumerate(moves):
            if not mv:                                   # step leaves a finished game alone
                after.append(states[g])
                continue
            k = r - STRIDE_ROUNDS
            if 0 <= k < len(fx.directed.get(g, ())):
                acts[g] = fx.directed[g][k]
            else:
                acts[g] = mv[0 if r == 0 else len(mv) - 1 if r == 1 else (r * STRIDE) % len(mv)]
            after.append(O.play(oracle, states[g], int(acts[g])))
        gpu.step(acts)
        got, want = gpu.get_positions(), O.states_array(after)
        for g in range(B):
            assert got[g].tobytes() == want[g].tobytes(), (n, r, labels[g], O.to_tps(oracle, states[g]), O.ptn(oracle, n, int(acts[g])),
                                                            A.state_to_tps(got[g]), O.to_tps(oracle, after[g]), int(got[g]["reversible_plies"]))
        if r in (1, STRIDE_ROUNDS):                      # the rules again on what the device itself played
            gpu.simulate(betas, 1)
            _check_roots(oracle, n, gpu, after, [O.possible_moves(oracle, s) if oracle.tzo_terminal(C.byref(s)) == -1 else [] for s in after],
                         "after round %d" % r)
    gpu.close()
    ora.close()


def _assert_same_paths(gpu, ora, B):
    """Statistics and children of the nodes along every game's most-visited path (as test_nodes_below_the_root_match_the_oracle)."""
    deepest = 0
    for g in range(B):
        path = []
        while True:
            got, want = gpu.node(g, path), ora.node(g, path)
            assert want is not None
            for f in ("visit_count", "n_children", "eval_tag", "eval_bits", "std_dev", "logit", "probability", "ply", "is_terminal_env"):
                assert got[0][f] == want[0][f] or (np.isnan(got[0][f]) and np.isnan(want[0][f])), (g, path, f)
            for f in ("move_idx", "visits", "eval_tag", "eval_bits", "logit", "prob", "std_dev"):
                assert np.array_equal(got[1][f].view(np.uint8), want[1][f].view(np.uint8)), (g, path, f)
            if len(got[1]["visits"]) == 0 or got[1]["visits"].max() == 0:
                break
            path.append(int(got[1]["move_idx"][int(np.argmax(got[1]["visits"]))]))
        deepest = max(deepest, len(path))
    return deepest


# Where a search starts and which ending it has to meet below the root: the label of the start, the reason of the ending
# (1 road, 2 flat count, 3 reversible plies) and a condition on the finished position.  Starts three, two and one ply before each
# ending: 200 simulations spread over a few hundred root children do not get three plies deep on the larger boards, and an ending
# one or two plies down is met on every size.
SEARCH_STARTS = [("shuffle/97", 3, None), ("shuffle/98", 3, None), ("shuffle/99", 3, None),
                 ("crowd/97", 3, None), ("crowd/98", 3, None), ("crowd/99", 3, None),
                 ("deplete/end-3", 2, E.depleted), ("deplete/end-2", 2, E.depleted), ("deplete/end-1", 2, E.depleted),
                 ("capheld/cap-only", 2, E.depleted), ("capheld/end-3", 2, E.depleted), ("capheld/end-2", 2, E.depleted),
                 ("capheld/end-1", 2, E.depleted),
                 ("walls/full-3", 2, lambda s: E.empties(s) == 0), ("walls/full-1", 2, lambda s: E.empties(s) == 0),
                 ("road2/before-white", 1, None), ("road2/before-black", 1, None)]
# Which starts must meet their ending in every game.  These are conditions on the oracle's search alone, read off the oracle's
# tree before the device's node is looked at, as the conditions of test_edge_positions.py are on the oracle's rules.  One ply before
# an ending it is among the root's children: on a full board bar one square, and with one stone left, every placement ends the
# game; before the double road one spread does; on the crowded boards (at most 9 placements, two or more spreads that draw) and
# 200 simulations either agent visits a drawing spread.  The Simple agent gives a placement e^3 times the prior of a spread, so on
# the open boards of shuffle/99, with up to 78 placements, only Dummy has to reach the draw.  From two and three plies away the
# figure is printed and whatever ending is met is compared; 200 simulations over some hundred root children do not get that deep
# in every game.
EVERY_GAME = {1: ("shuffle/99", "crowd/99", "deplete/end-1", "capheld/end-1", "walls/full-1", "road2/before-white", "road2/before-black"),
              2: ("crowd/99", "deplete/end-1", "capheld/end-1", "walls/full-1", "road2/before-white", "road2/before-black")}


def _finished_below(oracle, ora, g, start, reason, cond):
    """Depth-first over the visited nodes of the oracle's tree of game g: the path to a node whose position is finished for `reason`
    (and satisfies `cond`), with that position; (None, None) if the search met none."""
    stack = [([], start)]
    while stack:
        path, s = stack.pop()
        info, ch = ora.node(g, path, 1024)
        if path and info["is_terminal_env"]:
            _, why, _ = E.outcomes(oracle, s.n, s.half_komi, [s])
            if why[0] == reason and (cond is None or cond(s)):
                return path, s
            continue
        for i in np.nonzero(ch["visits"] > 0)[0][::-1]:
            m = int(ch["move_idx"][i])
            stack.append((path + [m], O.play(oracle, s, m)))
    return None, None


def _assert_same_node(gpu, ora, g, path):
    got, want = gpu.node(g, path), ora.node(g, path, 1024)
    assert want is not None
    for f in ("visit_count", "n_children", "eval_tag", "eval_bits", "std_dev", "logit", "probability", "ply", "is_terminal_env"):
        assert got[0][f] == want[0][f] or (np.isnan(got[0][f]) and np.isnan(want[0][f])), (g, path, f)
    for f in ("move_idx", "visits", "eval_tag", "eval_bits", "logit", "prob", "std_dev"):
        assert np.array_equal(got[1][f].view(np.uint8), want[1][f].view(np.uint8)), (g, path, f)
    return got


@pytest.mark.parametrize("agent", (1, 2), ids=("dummy", "simple"))
@pytest.mark.parametrize("n", SIZES)
def test_search_into_the_edges_matches_the_oracle(oracle, n, agent):
    """200 lock-step simulations from one, two and three plies before each ending (and from the tall stacks).  The ending a start
    leads to - the 100-ply draw, the flat count on empty reserves or on a full board, the double road - is looked for as a finished
    node below the root of the oracle's tree; from one ply away it has to be there in every game (EVERY_GAME), so on every size and
    with both agents the draw, both flat counts and the double road are leaves inside a tree.  The device's node on the same path
    is that node, bit for bit, with the result's tag; every node on the way there and along the most-visited paths is compared too."""
    A = require_gpu()
    fx = E.fixture(oracle, n)
    starts, plan = [], []
    for label, reason, cond in SEARCH_STARTS:
        for s in [s for have, s in fx.positions if have == label]:
            plan.append((label, reason, cond))
            starts.append(s)
    tall = E.labelled(oracle, n, "tower/tall")[::4] + E.labelled(oracle, n, "tower/onto")[::4]
    starts += tall
    B, sims = len(starts), 200
    gpu = A.BatchedMCTS(B, n, fx.half_komi, agent_kind=agent, node_capacity=1 << (17 if n >= 5 else 16))
    ora = O.OracleSearch(oracle, B, n, fx.half_komi, agent_kind=agent)
    gpu.set_positions(np.arange(B), O.states_array(starts))
    ora.set_positions(np.arange(B), starts)
    betas = np.where(np.arange(B) % 2 == 0, 0.0, 0.25).astype(np.float32)
    gpu.simulate(betas, sims)
    ora.simulate(betas, sims)
    assert gpu.pool_overflows() == 0
    assert_same_roots(gpu, ora, "%dx%d edges" % (n, n))
    assert _assert_same_paths(gpu, ora, B) >= 2
    assert gpu.counters() == ora.counters()
    met = {}
    for g, (label, reason, cond) in enumerate(plan):
        path, end = _finished_below(oracle, ora, g, starts[g], reason, cond)
        met.setdefault(label, []).append(path is not None)
        if path is None:
            continue
        if reason == 3:
            assert len(path) == E.LIMIT - starts[g].reversible_plies and end.reversible_plies == E.LIMIT
        for depth in range(1, len(path) + 1):
            got = _assert_same_node(gpu, ora, g, path[:depth])
        assert got[0]["is_terminal_env"] == 1 and got[0]["n_children"] == 0 and got[0]["ply"] == starts[g].ply + len(path)
        assert got[0]["eval_tag"] == EVAL_TAG[oracle.tzo_terminal(C.byref(end))] and got[0]["eval_bits"] == 0, (label, g, path)
        if reason == 3:
            assert got[0]["eval_tag"] == A.EVAL_DRAW
    print("%dx%d agent %d: endings met below the root, games per start label: %s" % (
        n, n, agent, ", ".join("%s %d/%d" % (k, sum(v), len(v)) for k, v in met.items())))
    for label in EVERY_GAME[agent]:
        if label.startswith("deplete/") and n < 4 or label.startswith("capheld/") and n < 5:
            continue                                     # the fixture has these from 4x4 and 5x5 on
        assert met[label] and all(met[label]), (n, agent, label, met[label])
    ip_g, ip_o = gpu.improved_policy(float(sims), 1024), ora.improved_policy(float(sims), 1024)
    assert np.array_equal(ip_g.view(np.uint32), ip_o.view(np.uint32))
    gpu.close()
    ora.close()


@pytest.mark.parametrize("n", SIZES)
def test_encoder_matches_game_repr_on_tall_stacks_and_empty_reserves(oracle, n):
    A = require_gpu()
    from takzero_amd import weights as W

    states = E.labelled(oracle, n, "tower/", "deplete/", "capheld/")
    assert max(E.tallest(s)[1] for s in states) >= E.TOWER_MIN[n]
    net = A.Net(arch=A.ARCH_TEST, n=n, precision=A.PREC_F32, blocks=1)
    net.load_tensors(W.init_weights(W.ARCH_TEST, n=n, blocks=1, seed=1))
    got = net.encode(O.states_array(states))
    want = np.stack([O.game_repr(oracle, s) for s in states])
    bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))[0]
    assert len(bad) == 0, (n, [O.to_tps(oracle, states[i]) for i in bad[:3]])
    net.close()


def _two_halvings(gpu, ora, states, k, budget, seed):
    """Two calls of sequential halving with a step and a restart between them (as test_gumbel_sequential_halving_bit_exact):
    selected actions, every root statistic and the improved policy, equal."""
    B = len(states)
    amax = 1024 if gpu.n == 6 else 512
    rng = np.random.default_rng(seed)
    gpu.set_positions(np.arange(B), O.states_array(states))
    ora.set_positions(np.arange(B), states)
    betas = np.where(np.arange(B) % 2 == 0, 0.25, 0.0).astype(np.float32)
    for it in range(2):
        gumbel = rng.gumbel(size=(B, amax)).astype(np.float32)
        sg = gpu.gumbel_sequential_halving(betas, k, budget, gumbel)
        so = ora.gumbel_sh(betas, k, budget, gumbel)
        assert np.array_equal(sg, so), (it, np.nonzero(sg != so)[0][:8])
        assert_same_roots(gpu, ora, "halving %d" % it)
        ip_g, ip_o = gpu.improved_policy(float(budget), amax), ora.improved_policy(float(budget), amax)
        assert np.array_equal(ip_g.view(np.uint32), ip_o.view(np.uint32)), it
        gpu.step(sg)
        ora.step(so)
        assert gpu.get_positions().tobytes() == ora.get_positions().tobytes(), it
        choice = rng.integers(0, 16, B)
        assert np.array_equal(gpu.restart_terminal_envs(choice), ora.restart_terminal(choice)), it
    assert gpu.counters() == ora.counters()


# 3x3 k = 16: most roots have fewer than 16 children (the i % size wrap), k = 2: the smallest k; 4x4 k = 64: every root below k,
# k = 8: none; 6x6 k = 32; 5x5 from three plies and one ply before the reserves run out, where sampled children end the game
HALVING_CASES = [(3, 16, 64, ("gumbel/root",)), (3, 2, 8, ("gumbel/root",)), (4, 64, 384, ("gumbel/root",)), (4, 8, 48, ("gumbel/root",)),
                 (6, 32, 320, ("gumbel/root",)), (5, 16, 64, ("deplete/end-3", "capheld/end-3", "deplete/end-1", "capheld/end-1"))]


@pytest.mark.parametrize("n,k,budget,labels", HALVING_CASES, ids=["%dx%d-k%d-%d" % (c[0], c[0], c[1], c[2]) for c in HALVING_CASES])
def test_gumbel_halving_matches_the_oracle_off_the_usual_shape(oracle, n, k, budget, labels):
    A = require_gpu()
    states = E.labelled(oracle, n, *labels)
    hk = E.HALF_KOMI[n]
    gpu = A.BatchedMCTS(len(states), n, hk, agent_kind=A.AGENT_SIMPLE, node_capacity=1 << (16 if n == 6 else 15))
    ora = O.OracleSearch(oracle, len(states), n, hk, agent_kind=2)
    _two_halvings(gpu, ora, states, k, budget, 100 * n + k)
    assert gpu.pool_overflows() == 0
    gpu.close()
    ora.close()


def test_gumbel_halving_with_a_real_net_on_3x3(oracle):
    """The halving keys from real logits: the 3x3 test net in fp32 on the device against the oracle search driving the same net."""
    A = require_gpu()
    from takzero_amd import weights as W
    from test_gpu_engine import _agent_over

    states = E.labelled(oracle, 3, "gumbel/root")
    net = A.Net(arch=A.ARCH_TEST, n=3, precision=A.PREC_F32, blocks=1)
    net.load_tensors(W.init_weights(W.ARCH_TEST, n=3, blocks=1, seed=123))
    gpu = A.BatchedMCTS(len(states), 3, 0, agent=net, node_capacity=1 << 14)
    ora = O.OracleSearch(oracle, len(states), 3, 0, agent_kind=0, agent_fn=_agent_over(net))
    _two_halvings(gpu, ora, states, 16, 64, 303)
    gpu.close()
    ora.close()
    net.close()
