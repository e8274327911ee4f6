"""tz_search_step_wide against tz_search_step: twin handles built identically, one stepped with step(), the other with
step_wide().  Equal means: root_info, pool_usage and get_positions are equal in every byte; every node reachable through node() is
equal in every returned array, walked over all expanded nodes; and both trees are equal again after further simulations on both,
which a wrong child0 or a wrong alloc would not survive (new children would land on kept nodes, or the walk would find other
nodes).

The wide step scans a level's child counts in blocks of TZ_STEP_WIDE_BLOCK parents and one wave scans the block sums
TZ_STEP_WIDE_SUMS at a time, so the 5x5 case asserts that its kept subtree has a level wider than BLOCK * SUMS parents."""
import re

import numpy as np
import pytest

from gpu_util import require_gpu
from capacity_positions import POSITIONS

pytestmark = pytest.mark.gpu

CHILD_FIELDS = ("move_idx", "visits", "eval_tag", "eval_bits", "logit", "prob", "std_dev")
TERMINAL = {3: "1,1,1/2,2,x/x3 2 3", 5: "1,1,1,1,1/2,2,2,2,x/x5/x5/x5 2 5"}      # a white road; black to move


def _constants():
    import os

    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "takzero_hip.h")).read()
    return tuple(int(re.search(r"#define %s (\d+)" % k, text).group(1)) for k in ("TZ_STEP_WIDE_BLOCK", "TZ_STEP_WIDE_SUMS"))


def _bytes_equal(a, b, where):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), where


def same_trees(a, b, where):
    """the equality of the module text; returns the number of decided (solved) nodes met on the walk"""
    _bytes_equal(a.root_info(), b.root_info(), (where, "root_info"))
    assert a.pool_usage() == b.pool_usage(), (where, a.pool_usage(), b.pool_usage())
    _bytes_equal(a.get_positions(), b.get_positions(), (where, "positions"))
    decided = 0
    for g in range(a.batch):
        level = [()]
        while level:
            below = []
            for path in level:
                ia, ca = a.node(g, list(path))
                ib, cb = b.node(g, list(path))
                _bytes_equal(ia, ib, (where, g, path, "info"))
                for k in CHILD_FIELDS:
                    _bytes_equal(ca[k], cb[k], (where, g, path, k))
                decided += int(ia["eval_tag"] != 0)
                # an expanded child has been visited; the others have no children to walk
                below += [path + (int(m),) for m, v in zip(ca["move_idx"], ca["visits"]) if v > 0]
            level = below
    return decided


def _pair(A, batch, n, half_komi, capacity=0):
    return A.BatchedMCTS(batch, n, half_komi, node_capacity=capacity), A.BatchedMCTS(batch, n, half_komi, node_capacity=capacity)


def _both(pair, call):
    for s in pair:
        call(s)


def _step_and_compare(pair, actions, where, more=64):
    a, b = pair
    a.step(actions)
    b.step_wide(actions)
    same_trees(a, b, (where, "after the step"))
    betas = np.zeros(a.batch, np.float32)
    _both(pair, lambda s: s.simulate(betas, more))
    same_trees(a, b, (where, "after %d more simulations" % more))
    _both(pair, lambda s: s.simulate_batch(betas, 8, 2))
    same_trees(a, b, (where, "after simulate_batch"))
    assert a.pool_overflows() == 0 and b.pool_overflows() == 0


def test_3x3_with_solver_results():
    """White threatens c3, black to move: every reply but the block loses at once, so the solver decides root children.  The first
    step goes into a decided child (the kept subtree is solver results throughout), the later ones follow the best action."""
    A = require_gpu()
    pair = _pair(A, 1, 3, 0)
    st = A.state_from_tps("1,1,x/x,2,x/2,x,1 2 3", 3, 0)
    betas = np.zeros(1, np.float32)
    _both(pair, lambda s: s.set_positions([0], [st]))
    a, b = pair
    lost = []
    for _ in range(10):                                  # 300 simulations at a time until a visited root child is decided
        _both(pair, lambda s: s.simulate(betas, 300))
        ch = a.node(0, [])[1]
        lost = [int(m) for m, v, tag in zip(ch["move_idx"], ch["visits"], ch["eval_tag"]) if v > 1 and tag != A.EVAL_VALUE]
        if lost:
            break
    assert lost, "no decided child below the 3x3 root: the case does not cover solver results"
    actions = np.array([lost[0]], np.uint16)
    decided = 0
    for k in range(3):                                   # both banks; the third root is the end of the game or close to it
        a.step(actions)
        b.step_wide(actions)
        decided += same_trees(a, b, "3x3 step %d" % k)
        _both(pair, lambda s: s.simulate(betas, 100))
        same_trees(a, b, "3x3 step %d, 100 more simulations" % k)
        actions = a.select_best_actions()
        if actions[0] == 0xFFFF:
            actions[0] = A.move_from_ptn(3, "c2")
    assert decided >= 2, decided                         # the decided child and the terminal node below it, at the least


def _widest_level_below(s, first):
    """the widest level of the subtree of game 0 below the root child `first`: the children of one depth's expanded nodes"""
    widest, level = 0, [(int(first),)]
    while level:
        below, children = [], 0
        for path in level:
            ch = s.node(0, list(path))[1]
            children += len(ch["visits"])
            below += [path + (int(m),) for m, v in zip(ch["move_idx"], ch["visits"]) if v > 0]
        widest, level = max(widest, children), below
    return widest


def test_5x5_levels_wider_than_a_block_and_than_a_block_of_block_sums():
    """A level of more than TZ_STEP_WIDE_BLOCK parents takes more than one workgroup's scan; one of more than BLOCK * SUMS parents
    takes the wave that scans the block sums round its loop with a carry.  The tree is grown until the subtree that the step will
    keep has such a level."""
    A = require_gpu()
    block, sums = _constants()
    pair = _pair(A, 1, 5, 4, capacity=1 << 20)
    betas = np.zeros(1, np.float32)
    a, b = pair
    widest = 0
    for _ in range(8):
        _both(pair, lambda s: s.simulate(betas, 1500))
        actions = a.select_best_actions()
        widest = _widest_level_below(a, actions[0])
        if widest > block * sums:
            break
    assert widest > block * sums and widest > block, (widest, block, sums)
    a.step(actions)
    b.step_wide(actions)
    same_trees(a, b, "5x5 after the step")
    _both(pair, lambda s: s.simulate(betas, 200))
    same_trees(a, b, "5x5 after 200 more simulations")
    assert a.pool_overflows() == 0 and b.pool_overflows() == 0


def test_root_with_more_than_128_children():
    A = require_gpu()
    label, count, tps = POSITIONS[5][1]                             # exactly max_actions = 512 legal moves
    assert count > 128
    pair = _pair(A, 1, 5, 4)
    st = A.state_from_tps(tps, 5, 4)
    betas = np.zeros(1, np.float32)
    _both(pair, lambda s: (s.set_positions([0], [st]), s.simulate(betas, 600)))
    assert pair[0].root_info()["n_children"][0] == count
    _step_and_compare(pair, pair[0].select_best_actions(), "wide root")


def test_action_not_among_the_roots_children():
    A = require_gpu()
    pair = _pair(A, 1, 5, 4)
    betas = np.zeros(1, np.float32)
    first = np.array([A.move_from_ptn(5, "a1")], np.uint16)
    _both(pair, lambda s: (s.simulate(betas, 50), s.step(first), s.simulate(betas, 300)))
    children = pair[0].node(0, [])[1]["move_idx"]
    assert len(children) == 24 and first[0] not in children       # a1 is taken: a flat there is no child of the root
    _step_and_compare(pair, first, "action outside the children")


def test_fresh_unexpanded_root():
    A = require_gpu()
    pair = _pair(A, 1, 5, 4)
    assert pair[0].root_info()["n_children"][0] == 0
    _step_and_compare(pair, np.array([A.move_from_ptn(5, "c3")], np.uint16), "fresh root")


def test_terminal_root():
    A = require_gpu()
    pair = _pair(A, 1, 3, 0)
    st = A.state_from_tps(TERMINAL[3], 3, 0)
    betas = np.zeros(1, np.float32)
    _both(pair, lambda s: (s.set_positions([0], [st]), s.simulate(betas, 3)))
    info = pair[0].root_info()
    assert info["is_terminal_env"][0] == 1 and info["eval_tag"][0] != A.EVAL_VALUE and info["eval_bits"][0] == 0
    before = pair[1].get_positions().tobytes()
    _step_and_compare(pair, np.array([A.move_from_ptn(3, "c1")], np.uint16), "terminal root", more=2)
    assert pair[1].get_positions().tobytes() == before              # a terminal root is skipped: no move is played


def test_three_games_of_very_different_size_in_one_call():
    A = require_gpu()
    pair = _pair(A, 3, 5, 4)
    states = [A.state_from_tps(POSITIONS[5][1][2], 5, 4), A.state_from_tps(TERMINAL[5], 5, 4), A.state_from_tps("x5/x5/x5/x5/x5 1 1", 5, 4)]
    betas = np.zeros(3, np.float32)
    _both(pair, lambda s: (s.set_positions([0, 1, 2], states), s.simulate(betas, 400)))
    info = pair[0].root_info()
    assert list(info["n_children"]) == [512, 0, 25] and info["is_terminal_env"][1] == 1
    actions = pair[0].select_best_actions()
    actions[1] = A.move_from_ptn(5, "e1")
    _step_and_compare(pair, actions, "three games")
    _step_and_compare(pair, pair[0].select_best_actions(), "three games, second step")


def test_two_wide_steps_in_a_row_use_both_banks():
    A = require_gpu()
    pair = _pair(A, 1, 4, 4)
    betas = np.zeros(1, np.float32)
    _both(pair, lambda s: s.simulate(betas, 2000))
    a, b = pair
    for k in range(2):
        actions = a.select_best_actions()
        a.step(actions)
        b.step_wide(actions)
        same_trees(a, b, "4x4 step %d" % k)
    _both(pair, lambda s: s.simulate(betas, 100))
    same_trees(a, b, "4x4 after two steps and 100 simulations")


def test_captured_graph_stays_valid_across_a_wide_step(oracle, monkeypatch):
    """Lock-step simulate(8) - two eager simulations, one captured, five replayed - then step_wide, then simulate(8) replayed from
    the same graph: equal to a twin created under TZ_NO_GRAPH=1 (tests/test_gpu_graph_lifetime.py), which steps with step()."""
    from takzero_amd import weights as W
    from test_gpu_graph_lifetime import Twins

    A = require_gpu()
    n, B = 4, 4
    t = Twins(A, monkeypatch, lambda: A.Net(arch=A.ARCH_TEST, n=n, precision=A.PREC_F16, blocks=2).load_tensors(
        W.init_weights(W.ARCH_TEST, n=n, blocks=2, seed=31)))
    gpu, twin = t.search(B, n, 1 << 14)
    betas = np.array([0.0, 0.25, 0.0, 0.25], np.float32)
    for phase in range(3):
        gpu.simulate(betas, 8)
        twin.simulate(betas, 8)
        t.check("simulate %d" % phase)
        same_trees(gpu, twin, "graph case, simulate %d" % phase)
        actions = twin.select_best_actions()
        gpu.step_wide(actions)
        twin.step(actions)
        same_trees(gpu, twin, "graph case, step %d" % phase)
    assert gpu.pool_overflows() == 0 and twin.pool_overflows() == 0
