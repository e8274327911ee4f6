"""Positions at and beyond a search handle's widest child list (max_actions: 64 on 3x3, 192 on 4x4, 512 on 5x5, 1024 on 6x6).

Every position is a TPS literal, parsed by the oracle (which accounts for the reserves and refuses too many pieces), white to move,
not finished.  Labels, per board size:
  cap-1        exactly max_actions - 1 legal moves
  cap          exactly max_actions
  over/near    max_actions + 1 .. max_actions + 32
  over/far     at least max_actions + 8 (3x3, 4x4) or max_actions + 20 (5x5, 6x6)
  under        the first half of an under->over pair: at most max_actions moves, and UNDER_OVER[n][1] is a legal move whose
               successor (black to move) has more than max_actions (the over-wide node is then below the root)

The literals that were not found by hand come from tune() and search() below (run this file to print them again);
tests parse the literals and count their moves, they do not search.  fixture(lib, n) is built once per process and board size."""
import ctypes as C
import itertools
import random
from collections import namedtuple

import oracle_lib as O

CAPS = {3: 64, 4: 192, 5: 512, 6: 1024}                # default_max_actions of the device searches, held to tz_search_shape on the GPU
HALF_KOMI = {3: 0, 4: 4, 5: 4, 6: 4}
FAR = {3: 8, 4: 8, 5: 20, 6: 20}

# label, legal moves, TPS
POSITIONS = {
    3: [("cap-1", 63, "x,2221,x/11,x,1221/2121,2211,x 1 40"),
        ("cap", 64, "221,x,211/x,21,x/x,2121,111 1 40"),
        ("over/near", 73, "121,211,x/221,x,121/x,21,221 1 40"),
        ("over/far", 73, "121,211,x/221,x,121/x,21,221 1 40")],
    4: [("cap-1", 191, "x,2121,x,2221/1,1,x2/2121,x,2211,2221/x3,2121 1 40"),
        ("cap", 192, "2121,x,2211,2221/221,x3/1211,x,221,x/x3,11121 1 40"),
        ("over/near", 193, "x,2211,x,2121/1,x2,221/x,221,2221,x/1111,2121,x2 1 40"),
        ("over/far", 204, "x,2211,2221,x/11211,x,2111,2211/x,221,2221,x/x4 1 40")],
    5: [("cap-1", 511, "11121,12221,12111,22111,x/x4,22221/x2,2221,x,12221/x5/22221,x4 1 40"),
        ("cap", 512, "11121,12221,12111,22111,x/x,1,x2,22221/x2,2221,x,12221/x5/22221,x4 1 40"),      # tune() of cap-1
        ("over/near", 532, "x5/x3,22211,x/x3,11221,x/x,22121,22221,1,22111/x,12211,12221,x,21211 1 40"),
        ("over/far", 532, "x5/x3,22211,x/x3,11221,x/x,22121,22221,1,22111/x,12211,12221,x,21211 1 40")],
    6: [("cap-1", 1023, "x,2211221,x4/x,122221,122211,x2,1121111/x,2212221,x4/21211,x3,222221,x/x5,2112211/x6 1 40"),
        ("cap", 1024, "x2,2112221,x3/x6/x,1121211,222211,x3/2212111,x5/2211221,2121211,21121,x3/x2,2,x2,1111221 1 40"),
        ("over/near", 1025, "x,2112121,211121,x2,1/x,211221,x4/x,2222221,x4/2221,1212211,x4/x2,221221,x,2121,x/x5,112221 1 40"),
        ("over/far", 1144, "x,111211,1221221,x3/222211,1122211,x3,1221221/x4,121211,1/22211,x4,2122121/x6/x4,222211,x 1 40")],
}
# n: (TPS of the position at or under the cap, PTN of the move, legal moves before, legal moves after)
UNDER_OVER = {3: ("x,112,1122/212,x2/112,x,122 1 40", "a3", 8, 66),
              6: ("x4,12112,x/222122,x4,112112/x4,2212212,211112/x2,1122112,x,2122112,x/x,111212,x4/x,221112,x4 1 40", "a1", 81, 1136)}
SEARCH_SEED = 1                                         # of search(), which finds the 3x3 and 6x6 pairs and none on 4x4 and 5x5

Fixture = namedtuple("Fixture", "n half_komi cap positions under_over")    # positions: [(label, TzState, [move, ...])]
_cache = {}


def _candidate(rng, n):
    """One random board as TPS: 6 to 9 stacks of height n-1 to n+1 on random squares (3 to n+2 stacks on 3x3 and 4x4), a flat of either
    colour on top, and up to three extra single flats or walls of either colour."""
    nn = n * n
    stacks = rng.randint(6, 9) if n >= 5 else rng.randint(3, n + 2)
    squares = rng.sample(range(nn), min(nn, stacks + rng.randint(0, 3)))
    cells = ["x"] * nn
    for k, sq in enumerate(squares):
        if k < stacks:
            h = rng.randint(n - 1, n + 1)
            cells[sq] = "".join(rng.choice("12") for _ in range(h - 1)) + rng.choice("12")
        else:
            cells[sq] = rng.choice(("1", "2", "1S", "2S"))
    return "/".join(",".join(cells[y * n:(y + 1) * n]) for y in range(n - 1, -1, -1)) + " 1 40"


def _count(lib, s):
    out = (C.c_uint16 * 4096)()
    return lib.tzo_possible_moves(C.byref(s), out, 4096)


def _cells(tps):
    """the board of a TPS string as rows of cells, "x" for an empty square"""
    rows = []
    for rank in tps.split(" ")[0].split("/"):
        row = []
        for c in rank.split(","):
            row += ["x"] * int(c[1:] or 1) if c[0] == "x" else [c]
        rows.append(row)
    return rows


def _tps(rows, tail="1 40"):
    return "/".join(",".join(r) for r in rows) + " " + tail


def tune(lib, n, base, target):
    """Up to two extra single flats or walls of either colour on empty squares of `base`, in a fixed order: the first board with exactly
    `target` legal moves, as (count, TPS); None if there is none.  (Random boards of search() stay below 512 moves on 5x5.)"""
    rows, s = _cells(base), O.TzState()
    empty = [(y, x) for y in range(n) for x in range(n) if rows[y][x] == "x"]
    for k in (1, 2):
        for squares in itertools.combinations(empty, k):
            for pieces in itertools.product(("1", "2", "1S", "2S"), repeat=k):
                trial = [r[:] for r in rows]
                for (y, x), p in zip(squares, pieces):
                    trial[y][x] = p
                tps = _tps(trial)
                if lib.tzo_state_from_tps(tps.encode(), n, HALF_KOMI[n], C.byref(s)) != 0 or lib.tzo_terminal(C.byref(s)) != -1:
                    continue
                if _count(lib, s) == target:
                    return target, O.to_tps(lib, s)
    return None


def search(lib, n, seed, candidates=400000):
    """Bounded and deterministic: the first random board with at most CAPS[n] moves and a placement whose successor has more than
    CAPS[n], as (TPS, PTN, count before, count after).  None when the budget runs out."""
    rng, cap, hk = random.Random(seed), CAPS[n], HALF_KOMI[n]
    s = O.TzState()
    for _ in range(candidates):
        tps = _candidate(rng, n)
        if lib.tzo_state_from_tps(tps.encode(), n, hk, C.byref(s)) != 0 or lib.tzo_terminal(C.byref(s)) != -1:
            continue
        cnt = _count(lib, s)
        if cnt > cap:
            continue
        other = O.TzState.from_buffer_copy(bytes(s))
        other.to_move ^= 1
        if _count(lib, other) <= cap:                   # a placement takes moves from the other side, it gives none
            continue
        for m in O.possible_moves(lib, s):
            if m >= 3 * n * n:
                break
            t = O.play(lib, s, m)
            if lib.tzo_terminal(C.byref(t)) == -1 and _count(lib, t) > cap:
                return O.to_tps(lib, s), O.ptn(lib, n, m), cnt, _count(lib, t)
    return None


def _build(lib, n):
    hk, positions = HALF_KOMI[n], []
    for label, count, tps in POSITIONS[n]:
        s = O.state_from_tps(lib, tps, n, hk)
        positions.append((label, s, O.possible_moves(lib, s)))
    pair = None
    if n in UNDER_OVER:
        tps, ptn, before, after = UNDER_OVER[n]
        s = O.state_from_tps(lib, tps, n, hk)
        move = O.from_ptn(lib, n, ptn)
        positions.append(("under", s, O.possible_moves(lib, s)))
        pair = (len(positions) - 1, move, O.play(lib, s, move))
    return Fixture(n, hk, CAPS[n], positions, pair)


def fixture(lib, n):
    if n not in _cache:
        _cache[n] = _build(lib, n)
    return _cache[n]


def labelled(lib, n, *labels):
    """The states of board size n with one of `labels`, in fixture order."""
    return [s for label, s, _ in fixture(lib, n).positions if label in labels]


if __name__ == "__main__":
    lib = O.load()
    print(5, "cap", tune(lib, 5, POSITIONS[5][0][2], CAPS[5]))
    for n in (3, 4, 5, 6):
        print(n, "under->over", search(lib, n, SEARCH_SEED))             # None on 4x4 and 5x5
