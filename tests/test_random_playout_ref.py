"""The CPU reference of the random playouts (tests/random_playout_ref.py) held to itself: the finaliser's values, the split
invariance that the ply counter gives, independence of games, the three stop rules, and the evenness of the index rule."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import random_playout_ref as R


@pytest.fixture(scope="module")
def lib():
    return O.load()


# tz_mix64 (csrc/tz_math.h) compiled as C and printed once for these inputs
MIX64_KAT = [
    (0x0000000000000000, 0xE220A8397B1DCDAF),
    (0x000000000000007B, 0xB4DC9BD462DE412B),
    (0xFFFFFFFFFFFFFFFF, 0xE4D971771B652C20),
]


def test_mix64_known_values():
    for x, want in MIX64_KAT:
        assert R.mix64(x) == want, (hex(x), hex(R.mix64(x)), hex(want))


def _same(a, b):
    return bytes(a) == bytes(b)


@pytest.mark.parametrize("n,steps,cut", [(3, 40, 10), (4, 60, 17), (5, 50, 1)])
def test_two_calls_equal_one(lib, n, steps, cut):
    for g in range(8):
        st = R.opening(lib, n, 4, g)
        one = R.playout(lib, st, 77, 1000 + g, steps)
        a = R.playout(lib, st, 77, 1000 + g, cut)
        b = R.playout(lib, a["state"], 77, 1000 + g, steps - cut)
        if a["played"] < cut:           # the first part already ran out of moves
            assert b["played"] == 0
        assert a["moves"] + b["moves"] == one["moves"] and a["nlegal"] + b["nlegal"] == one["nlegal"]
        assert _same(b["state"], one["state"])


def test_another_seed_or_game_is_another_game(lib):
    st = R.opening(lib, 5, 4, 0)
    base = R.playout(lib, st, 5, 9, 30)["moves"]
    assert R.playout(lib, st, 5, 9, 30)["moves"] == base
    assert R.playout(lib, st, 6, 9, 30)["moves"] != base
    assert R.playout(lib, st, 5, 10, 30)["moves"] != base
    assert R.playout(lib, st, 5, 9 + 2**40, 30)["moves"] != base


@pytest.mark.parametrize("n", [3, 4])
def test_stop_flag_never_moves_from_a_terminal_position(lib, n):
    ended = 0
    for g in range(32):
        r = R.playout(lib, O.state_default(lib, n, 4), 11, g, 150, stop_at_terminal=True, record_positions=True)
        for p in r["positions"]:
            assert lib.tzo_terminal(C.byref(p)) == -1
        if r["played"] < 150:
            assert lib.tzo_terminal(C.byref(r["state"])) != -1 or not O.possible_moves(lib, r["state"])
            ended += 1
    assert ended == 32      # every 3x3 and 4x4 random game ends well within 150 plies


def test_without_the_flag_3x3_games_run_past_their_end_until_no_move_is_left(lib):
    past_end, out_of_moves = 0, 0
    for g in range(64):
        r = R.playout(lib, O.state_default(lib, 3, 4), 11, g, 150, record_positions=True)
        first_terminal = next((i for i, p in enumerate(r["positions"]) if lib.tzo_terminal(C.byref(p)) != -1), None)
        if first_terminal is not None:
            past_end += 1               # a move was played from a terminal position
            assert first_terminal >= 5  # no 3x3 road before ply 5
        if r["played"] < 150:
            assert not O.possible_moves(lib, r["state"]) and not r["overflow"]
            assert r["played"] >= 9     # nine squares have to fill before a 3x3 board can lock
            out_of_moves += 1
    assert past_end > 0 and out_of_moves > 0, (past_end, out_of_moves)


def test_the_locked_3x3_position_parses_and_has_no_move(lib):
    st = O.state_from_tps(lib, "1S,2S,1S/2S,1S,2S/1S,2S,1S 2 10", 3, 4)
    assert O.possible_moves(lib, st) == []
    for flag in (False, True):
        r = R.playout(lib, st, 1, 0, 5, stop_at_terminal=flag)
        assert r["played"] == 0 and _same(r["state"], st)


def test_index_rule_is_even_over_200000_draws():
    """n = 7, 2000 games x 100 plies: each index within 5 standard deviations of 1/7 (a condition on this seed, checked once)"""
    counts = np.zeros(7, np.int64)
    for g in range(2000):
        key = R.game_key(2024, g)
        for ply in range(100):
            j = R.draw_index(key, ply, 7)
            assert 0 <= j < 7
            counts[j] += 1
    total = 200000
    sd = (total * (1 / 7) * (6 / 7)) ** 0.5
    assert counts.sum() == total
    assert np.all(np.abs(counts - total / 7) < 5 * sd), counts


def test_opening_choices_of_the_package_are_the_references():
    """takzero_amd.eee draws the openings in uint64 arrays; the reference in Python integers"""
    from takzero_amd import eee

    for seed, base in ((123, 0), (5, 2**40 + 5), (2**64 - 1, 2**64 - 10), (0, 65536 * 99)):
        got = eee.opening_choices(seed, base, 300)
        assert got.dtype == np.int32 and got.tolist() == [R.opening_choice(seed, base + g) for g in range(300)]
        assert eee.mix64(seed) == R.mix64(seed)
    assert set(eee.opening_choices(1, 0, 300).tolist()) == set(range(16))


def test_index_rule_edges():
    assert R.draw_index(0, 0, 1) == 0
    for n in (1, 2, 185, 1024):
        assert ((2**32 - 1) * n) >> 32 == n - 1     # the largest high word still indexes the row
        assert all(0 <= R.draw_index(k, p, n) < n for k in (0, 1, R.M64) for p in (0, 1, 0xFFFF))
