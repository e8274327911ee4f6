"""The rule-edge fixture (edge_positions.py) reaches every edge it names, judged by the CPU oracle alone.  These are conditions on the
fixture, not measurements of the engine: test_gpu_rule_edges.py compares the device with the oracle on exactly these positions, and
a policy that quietly stopped reaching an edge would turn that comparison into one more random-playout test."""
import ctypes as C

import numpy as np
import pytest

import edge_positions as E
import oracle_lib as O

SIZES = (3, 4, 5, 6)
_outcomes = {}


def _judged(oracle, n):
    """(labels, states, terminal, reason, winner) of the whole list of one size, judged once."""
    if n not in _outcomes:
        fx = E.fixture(oracle, n)
        states = [s for _, s in fx.positions]
        _outcomes[n] = ([label for label, _ in fx.positions], states) + tuple(E.outcomes(oracle, n, fx.half_komi, states))
    return _outcomes[n]


def _where(oracle, n, label):
    labels, states, term, reason, winner = _judged(oracle, n)
    idx = [i for i, have in enumerate(labels) if have == label]
    assert idx, "no %dx%d position carries the label %s" % (n, n, label)
    return idx, states, term, reason, winner


def _expected_labels(n):
    want = ["%s/%d" % (kind, r) for kind in ("shuffle", "crowd") for r in (97, 98, 99, 100)] + ["crowd/reset"] + ["shuffle/reset", "tower/tall", "tower/spread", "tower/onto", "tower/landed", "walls/full-3", "walls/full-1",
                                                            "walls/full", "komi/white", "komi/draw", "komi/black"]
    want += ["road2/%s-%s" % (when, who) for when in ("before", "after") for who in ("white", "black")]
    if n >= 4:
        want += ["deplete/end-3", "deplete/end-2", "deplete/end-1", "deplete/end"]
    if n >= 5:
        want += ["capheld/cap-only", "capheld/end-3", "capheld/end-2", "capheld/end-1", "capheld/end"]
    if n in E.GUMBEL_ROOTS:
        want.append("gumbel/root")
    return want


@pytest.mark.parametrize("n", SIZES)
def test_every_label_is_carried_and_the_list_fits_one_call(oracle, n):
    fx = E.fixture(oracle, n)
    have = E.counts(oracle, n)
    print("%dx%d: %d positions: %s" % (n, n, len(fx.positions), ", ".join("%s %d" % kv for kv in sorted(have.items()))))
    for label in _expected_labels(n):
        assert have.get(label, 0) >= 1, "no %dx%d position carries the label %s" % (n, n, label)
    assert len(fx.positions) <= E.MAX_POSITIONS
    for label, s in fx.positions:
        assert s.n == n and (s.half_komi == fx.half_komi or label.startswith("komi/")), label
    # deterministic: a second build from scratch gives the same bytes
    again = E._build(oracle, n)
    assert [(label, bytes(s)) for label, s in again.positions] == [(label, bytes(s)) for label, s in fx.positions]
    assert again.directed == fx.directed and again.tower_spreads == fx.tower_spreads and again.komi == fx.komi
    assert again.tower_drops == fx.tower_drops


@pytest.mark.parametrize("n,kind,least", [(4, "deplete", 4), (5, "deplete", 4), (6, "deplete", 4), (5, "capheld", 1), (6, "capheld", 1)])
def test_reserves_run_empty_and_the_three_plies_before_are_there(oracle, n, kind, least):
    ends, states, term, reason, _ = _where(oracle, n, kind + "/end")
    assert len(ends) >= least
    for i in ends:
        s = states[i]
        assert term[i] != -1 and reason[i] == 2 and E.depleted(s), (n, i)
        assert E.empties(s) > 0, "a full board would end the game without the reserves"
    for back in (3, 2, 1):
        idx = _where(oracle, n, "%s/end-%d" % (kind, back))[0]
        assert len(idx) == len(ends)
        for i in idx:
            assert term[i] == -1 and not E.depleted(states[i]), (n, back, i)
    # consecutive in the list: end-3, end-2, end-1, end of one game, each one legal move from the one before
    labels = _judged(oracle, n)[0]
    for i in ends:
        assert [labels[j] for j in range(i - 3, i)] == ["%s/end-%d" % (kind, b) for b in (3, 2, 1)]
        for j in range(i - 3, i):
            assert any(bytes(O.play(oracle, states[j], m)) == bytes(states[j + 1]) for m in O.possible_moves(oracle, states[j]))


@pytest.mark.parametrize("n", SIZES)
def test_boards_fill_up_without_a_road(oracle, n):
    full, states, term, reason, _ = _where(oracle, n, "walls/full")
    assert len(full) >= 2
    for i in full:
        assert term[i] != -1 and reason[i] == 2 and E.empties(states[i]) == 0 and not E.depleted(states[i]), (n, i)
    for label, left in (("walls/full-3", 3), ("walls/full-1", 1)):
        for i in _where(oracle, n, label)[0]:
            assert term[i] == -1 and E.empties(states[i]) == left, (n, label, i)


@pytest.mark.parametrize("n", SIZES)
def test_the_counter_reaches_its_limit_on_a_crowded_board(oracle, n):
    """Few placements compete with the spreads there, so that a search whose priors favour placements still plays into the draw."""
    for r in (97, 98, 99, 100):
        idx, states, term, reason, _ = _where(oracle, n, "crowd/%d" % r)
        assert len(idx) >= 4
        for i in idx:
            s = states[i]
            assert s.reversible_plies == r and (term[i], reason[i]) == ((2, 3) if r == 100 else (-1, 0)), (n, r, i)
            assert E.empties(s) <= 3
            if r == 99:
                moves = O.possible_moves(oracle, s)
                draws = [m for m in moves if m >= 3 * n * n and oracle.tzo_terminal(C.byref(O.play(oracle, s, m))) == 2]
                assert len(draws) >= 2 and sum(m < 3 * n * n for m in moves) <= 9
    for i in _where(oracle, n, "crowd/reset")[0]:
        assert states[i].reversible_plies == 0


@pytest.mark.parametrize("n", SIZES)
def test_the_counter_reaches_its_limit_and_goes_back(oracle, n):
    for r in (97, 98, 99):
        idx, states, term, _, _ = _where(oracle, n, "shuffle/%d" % r)
        assert len(idx) >= 4
        for i in idx:
            assert states[i].reversible_plies == r and term[i] == -1, (n, r, i)
    idx, states, term, reason, winner = _where(oracle, n, "shuffle/100")
    assert len(idx) >= 4
    for i in idx:
        assert states[i].reversible_plies == E.LIMIT and term[i] == 2 and reason[i] == 3 and winner[i] == 2, (n, i)
        assert oracle.tzo_terminal(C.byref(states[i])) == 2
    fx = E.fixture(oracle, n)
    resets = _where(oracle, n, "shuffle/reset")[0]
    assert len(resets) >= 2
    for i in resets:
        assert states[i].reversible_plies == 0
    # each reset is a 99-position after the placement the fixture names for it
    seen = 0
    for i in _where(oracle, n, "shuffle/99")[0]:
        after = O.play(oracle, states[i], fx.directed[i][0])
        assert fx.directed[i][0] < 3 * n * n and after.reversible_plies == 0
        seen += any(bytes(after) == bytes(states[j]) for j in resets)
        for m in fx.directed[i][1:]:                     # a capstone flattening a wall
            assert m >= 3 * n * n and O.play(oracle, states[i], m).reversible_plies == 0
    assert seen >= 2


@pytest.mark.parametrize("n", (5, 6))
def test_the_capstone_is_the_only_piece_left_to_place(oracle, n):
    idx, states, term, _, _ = _where(oracle, n, "capheld/cap-only")
    assert len(idx) >= 4
    nn = n * n
    for i in idx:
        s = states[i]
        assert term[i] == -1 and s.stones[s.to_move] == 0 and s.caps[s.to_move] == 1, (n, i)
        moves = O.possible_moves(oracle, s)
        assert not any(m < 2 * nn for m in moves), "a flat or a wall placement without a stone"
        assert sum(1 for m in moves if 2 * nn <= m < 3 * nn) == E.empties(s) > 0


@pytest.mark.parametrize("n", SIZES)
def test_stacks_cross_the_word_boundaries_of_colors(oracle, n):
    idx, states, term, _, _ = _where(oracle, n, "tower/tall")
    assert len(idx) >= 4
    fx = E.fixture(oracle, n)
    patterns = set()
    for i in idx:
        s = states[i]
        sq, h = E.tallest(s)
        assert h >= E.TOWER_MIN[n] and term[i] == -1 and E.owner(s, sq) == s.to_move, (n, i, h)
        patterns.add(s.colors[sq] & 0xFF)
    assert len(patterns) >= 3, "the stacks' colours should not all follow one pattern"
    if n >= 5:
        assert E.TOWER_MIN[n] >= 33                      # bit 32 of colors[sq] is in use
    spreads = _where(oracle, n, "tower/spread")[0]
    assert len(fx.tower_spreads) == len(spreads) and any(c == n for _, _, c, _ in fx.tower_spreads)
    for parent, move, carried, succ in fx.tower_spreads:
        sq = E.tallest(states[parent])[0]
        kind, src, _, drops = E.decode(n, move)
        assert kind == "spread" and src == sq and sum(drops) == carried
        assert move in fx.directed[parent] and bytes(O.play(oracle, states[parent], move)) == bytes(states[succ])
        assert states[succ].height[sq] == states[parent].height[sq] - carried


@pytest.mark.parametrize("n", SIZES)
def test_pieces_are_dropped_onto_a_stack_that_reaches_the_boundary(oracle, n):
    """apply_move shifts what it drops by the height of the stack below (<< dh): on 5x5 and 6x6 by 32 or more."""
    fx = E.fixture(oracle, n)
    _, states, term, _, _ = _where(oracle, n, "tower/onto")
    assert len(fx.tower_drops) >= 2
    below = []
    for before, move, after in fx.tower_drops:
        s, t = states[before], states[after]
        target, h = E.tallest(s)
        kind, sq, step, drops = E.decode(n, move)
        landed = sum(c for k, c in enumerate(drops) if sq + (k + 1) * step == target)
        assert kind == "spread" and sq != target and landed >= 1 and h >= E.TOWER_MIN[n] - 1 and term[before] == -1
        assert fx.directed[before] == [move] and bytes(O.play(oracle, s, move)) == bytes(t)
        assert t.height[target] == h + landed
        below.append(h)
    if n >= 5:
        assert min(below) >= 32 and E.TOWER_MIN[n] - 1 >= 32
    assert any(E.owner(states[after], E.tallest(states[before])[0]) == 1 for before, _, after in fx.tower_drops), "a set bit above the boundary"


@pytest.mark.parametrize("n", SIZES)
def test_the_komi_sweep_gives_all_three_outcomes(oracle, n):
    fx = E.fixture(oracle, n)
    labels, states, term, reason, winner = _judged(oracle, n)
    assert len(fx.komi) >= 3
    for base, (iw, id_, ib) in fx.komi:
        assert reason[base] == 2
        d = oracle.tzo_flat_diff(C.byref(states[base]))
        for i, hk, won in ((iw, 2 * d - 1, 0), (id_, 2 * d, 2), (ib, 2 * d + 1, 1)):
            s = states[i]
            assert s.half_komi == hk and reason[i] == 2 and winner[i] == won, (n, base, i)
            assert oracle.tzo_result(C.byref(s)) == {0: 1, 1: 2, 2: 3}[won]
            t = E.copy_state(s)
            t.half_komi = states[base].half_komi
            assert bytes(t) == bytes(states[base]), "only half_komi may differ"


@pytest.mark.parametrize("n", SIZES)
def test_a_road_for_both_colours_goes_to_the_mover(oracle, n):
    fx = E.fixture(oracle, n)
    for mover, name in ((0, "white"), (1, "black")):
        (before,), states, term, _, _ = _where(oracle, n, "road2/before-" + name)
        (after,), _, _, reason, winner = _where(oracle, n, "road2/after-" + name)
        s, t = states[before], states[after]
        assert term[before] == -1 and s.to_move == mover
        assert bytes(O.play(oracle, s, fx.directed[before][0])) == bytes(t)
        assert reason[after] == 1 and winner[after] == mover and term[after] == 1      # a loss for the side now to move
        # the road of the other colour is complete as well: with the side to move flipped back the other colour is "the mover"
        u = E.copy_state(t)
        u.to_move = mover
        assert oracle.tzo_result(C.byref(u)) == {0: 2, 1: 1}[mover]


def test_gumbel_roots_have_fewer_children_than_sampled_actions(oracle):
    kids = {n: [len(O.possible_moves(oracle, s)) for s in E.labelled(oracle, n, "gumbel/root")] for n in E.GUMBEL_ROOTS}
    assert len(kids[3]) == 16 and sum(k < 16 for k in kids[3]) >= 8 and min(kids[3]) <= 8, kids[3]
    assert len(kids[4]) == 16 and all(k < 64 for k in kids[4]), kids[4]
    assert min(kids[4]) > 8, "k = 8 on 4x4 is the case without the wrap"
    assert len(kids[6]) == 8 and max(kids[6]) > 32, kids[6]
    for n in E.GUMBEL_ROOTS:
        assert all(oracle.tzo_terminal(C.byref(s)) == -1 for s in E.labelled(oracle, n, "gumbel/root"))
    # the 5x5 halving runs three plies and one ply before the reserves run out: at the latter a sampled child ends the game
    last = E.labelled(oracle, 5, "deplete/end-1", "capheld/end-1")
    assert len(last) >= 4
    for s in last:
        assert any(oracle.tzo_terminal(C.byref(O.play(oracle, s, m))) != -1 for m in O.possible_moves(oracle, s))
