"""What tests/capacity_positions.py promises, on the CPU oracle: every literal parses, round-trips, is not finished and has the
labelled number of legal moves at, one under and over the device searches' max_actions; the tests of test_gpu_action_capacity.py
rest on these counts."""
import ctypes as C

import pytest

import capacity_positions as P
import oracle_lib as O

SIZES = (3, 4, 5, 6)


def test_the_caps_the_fixture_assumes():
    """default_max_actions (csrc/tz_capi.hip); test_gpu_action_capacity.py holds tz_search_shape to the same table"""
    assert P.CAPS == {3: 64, 4: 192, 5: 512, 6: 1024}
    assert P.HALF_KOMI == {3: 0, 4: 4, 5: 4, 6: 4}


@pytest.mark.parametrize("n", SIZES)
def test_every_position_parses_round_trips_and_is_not_finished(oracle, n):
    for label, count, tps in P.POSITIONS[n]:
        s = O.state_from_tps(oracle, tps, n, P.HALF_KOMI[n])
        assert O.to_tps(oracle, s) == tps, label
        assert bytes(O.state_from_tps(oracle, O.to_tps(oracle, s), n, P.HALF_KOMI[n])) == bytes(s), label
        assert oracle.tzo_terminal(C.byref(s)) == -1, label
        assert s.to_move == 0 and s.n == n, label


@pytest.mark.parametrize("n", SIZES)
def test_move_counts_are_the_labelled_ones(oracle, n):
    fx, cap = P.fixture(oracle, n), P.CAPS[n]
    assert fx.cap == cap and fx.half_komi == P.HALF_KOMI[n]
    labels = [label for label, _, _ in fx.positions]
    for want in ("cap-1", "cap", "over/near", "over/far"):
        assert labels.count(want) == 1, (n, want)
    literal = {label: count for label, count, _ in P.POSITIONS[n]}
    for label, s, moves in fx.positions:
        assert moves == O.possible_moves(oracle, s), label                     # possible_moves order
        assert len(set(moves)) == len(moves) and all(0 <= m < (3 + 4 * ((1 << n) - 2)) * n * n for m in moves), label
        if label in literal:
            assert len(moves) == literal[label], (n, label, len(moves))
        if label == "cap-1":
            assert len(moves) == cap - 1
        elif label == "cap":
            assert len(moves) == cap
        elif label == "over/near":
            assert cap + 1 <= len(moves) <= cap + 32
        elif label == "over/far":
            assert len(moves) >= cap + P.FAR[n]
        else:
            assert label == "under" and len(moves) <= cap


@pytest.mark.parametrize("n", sorted(P.UNDER_OVER))
def test_the_under_over_pair_puts_an_over_wide_node_below_the_root(oracle, n):
    fx, cap = P.fixture(oracle, n), P.CAPS[n]
    tps, ptn, before, after = P.UNDER_OVER[n]
    index, move, successor = fx.under_over
    label, s, moves = fx.positions[index]
    assert label == "under" and O.to_tps(oracle, s) == tps and len(moves) == before <= cap
    assert move in moves and O.ptn(oracle, n, move) == ptn
    assert successor.to_move == 1 and oracle.tzo_terminal(C.byref(successor)) == -1
    assert len(O.possible_moves(oracle, successor)) == after > cap


def test_possible_moves_does_not_truncate_the_widest_position(oracle):
    widest = max(len(moves) for n in SIZES for _, _, moves in P.fixture(oracle, n).positions)
    assert widest == 1144
