"""Positions at the edges of the Tak rules, reached on the CPU oracle by directed playouts.

Uniformly random playouts (gpu_util.random_positions) almost never empty a reserve, fill a 6x6 board, build a stack taller than
eight or play a hundred spreads in a row, so the branches of the device rules for those cases need positions made on purpose.
Every position here is reached by legal play through tzo_play from the empty board, with two hand-made exceptions: the komi
sweep (a copy of a finished game with another half_komi) and the double road (from TPS).

fixture(lib, n) is deterministic (fixed seeds, np.random.default_rng only) and built once per process and board size.

Labels, per board size:
  deplete/end-3 .. deplete/end   a game that ends because a reserve is empty, and the three plies before its end
  capheld/cap-only               not finished, the side to move has no stones and one capstone (5x5, 6x6)
  capheld/end-3 .. capheld/end   the end of those games (reserves empty as well)
  shuffle/97 .. shuffle/100      reversible_plies at 97, 98, 99 and 100 (the draw)
  shuffle/reset                  a 99-position after a placement: the counter is back at 0
  shuffle/reset-flatten          the same after a capstone flattened a wall (kept where a game offers it)
  crowd/97 .. crowd/100, reset   the same on a board with few empty squares: few placements beside the spreads that lead to the draw
  tower/tall                     a stack that crosses bit 8 (3x3), bit 16 (4x4) or bit 32 (5x5, 6x6) of colors[], its owner to move
  tower/spread                   such a position after a spread out of that stack
  tower/onto, tower/landed       one ply before a spread drops pieces onto a stack that already reaches the boundary, and after it
  walls/full-3, full-1, full     a board filled without a road, three plies and one ply before, and full
  komi/white, draw, black        a finished flat count with half_komi at 2d - 1, 2d, 2d + 1 (d = white flats - black flats)
  road2/before-*, road2/after-*  one ply before a spread that completes a road for both colours, and after it (* = mover)
  gumbel/root                    roots for sequential halving from random playouts (3x3, 4x4, 6x6)
"""
import ctypes as C
from collections import namedtuple

import numpy as np

import oracle_lib as O
from gpu_util import random_positions

HALF_KOMI = {3: 0, 4: 4, 5: 4, 6: 4}
LIMIT = 100                                             # the reversible-plies draw both engines share
TOWER_MIN = {3: 9, 4: 20, 5: 33, 6: 33}                 # past bit 8 / bit 16 / bit 32 of colors[sq]
GUMBEL_ROOTS = {3: (16, 4, 14), 4: (16, 6, 30), 6: (8, 2, 40)}     # count, min ply, max ply
MAX_POSITIONS = 256

# positions: [(label, TzState)]; directed: {index: [move, ...]} moves a test should play from that position;
# tower_spreads: [(index of the tall position, move, pieces carried, index of the successor)];
# tower_drops: [(index of the position before the drop, move, index of the successor)];
# komi: [(index of the finished game, [index at 2d-1, at 2d, at 2d+1])]
Fixture = namedtuple("Fixture", "n half_komi positions directed tower_spreads tower_drops komi")

_cache = {}


# ---------------------------------------------------------------------------------------------- small helpers
def copy_state(s):
    return O.TzState.from_buffer_copy(bytes(s))


def terminal(lib, s):
    return lib.tzo_terminal(C.byref(s))


def decode(n, move):
    """move index -> ("place", piece 0 flat / 1 wall / 2 cap, square) or ("spread", square, step between squares, drops)."""
    nn = n * n
    channel, sq = divmod(int(move), nn)
    if channel < 3:
        return ("place", channel, sq)
    slot, v = divmod(channel - 3, (1 << n) - 2)
    v += 1
    p0 = (v & -v).bit_length() - 1
    drops, cur = [], 0
    for b in range(p0, n):
        if (v >> b) & 1:
            if cur:
                drops.append(cur)
            cur = 1
        else:
            cur += 1
    drops.append(cur)
    step = {0: n, 1: 1, 2: -n, 3: -1}[slot]            # up, right, down, left
    return ("spread", sq, step, drops)


def tallest(s):
    nn = s.n * s.n
    h = [s.height[q] for q in range(nn)]
    sq = int(np.argmax(h))
    return sq, h[sq]


def owner(s, sq):
    return (s.colors[sq] >> (s.height[sq] - 1)) & 1


def depleted(s):
    return (s.stones[0] == 0 and s.caps[0] == 0) or (s.stones[1] == 0 and s.caps[1] == 0)


def empties(s):
    return sum(1 for q in range(s.n * s.n) if s.top[q] == 0)


def outcomes(lib, n, half_komi, states):
    """tzo_terminal, the reason (0 none, 1 road, 2 flat count, 3 reversible plies) and the winner (0 white, 1 black, 2 draw) of each
    state, as the oracle's search reports them for finished games."""
    ora = O.OracleSearch(lib, len(states), n, half_komi, agent_kind=1)
    ora.set_positions(np.arange(len(states)), list(states))
    term = ora.restart_terminal(np.zeros(len(states), np.int32))
    reason, winner = ora.terminal_details()
    ora.close()
    return term, reason, winner


def _shuffled(rng, items):
    return [items[i] for i in rng.permutation(len(items))]


def _first(lib, s, moves, accept):
    for m in moves:
        t = O.play(lib, s, m)
        if accept(t):
            return m, t
    return None, None


# ---------------------------------------------------------------------------------------------- the policies
def _deplete_game(lib, n, hk, rng, hold_cap, dwell=0):
    """Place while three squares are empty, else free a square; never into a finished game unless a reserve ran out.
    Returns (history, cap-only positions met)."""
    nn = n * n
    s = O.state_default(lib, n, hk)
    hist, cap_only = [s], []
    for _ in range(900):
        if terminal(lib, s) != -1:
            break
        mv = O.possible_moves(lib, s)
        me = s.to_move
        places = [m for m in mv if m < 3 * nn]
        spreads = [m for m in mv if m >= 3 * nn]
        if hold_cap and s.ply >= 2 and s.stones[me] > 0:
            places = [m for m in places if m < 2 * nn]
        want_spread = False
        if s.ply >= 2 and s.stones[me] == 0 and s.caps[me] == 1:
            cap_only.append(s)
            want_spread = len(cap_only) <= dwell
        if want_spread:
            pref = _shuffled(rng, spreads)
        elif empties(s) >= 3 and places:
            pref = _shuffled(rng, places)
        else:
            pref = []
            for m in _shuffled(rng, spreads):
                _, sq, step, drops = decode(n, m)
                lands_on_empty = sum(1 for k in range(len(drops)) if s.top[sq + (k + 1) * step] == 0)
                if sum(drops) == s.height[sq] and lands_on_empty == 0:
                    pref.append(m)
        chosen = set(pref)
        rest = _shuffled(rng, [m for m in places + spreads if m not in chosen])
        m, t = _first(lib, s, pref + rest, lambda t: terminal(lib, t) == -1 or depleted(t))
        if m is None:
            t = O.play(lib, s, mv[int(rng.integers(len(mv)))])
        s = t
        hist.append(s)
    return hist, cap_only


def _shuffle_game(lib, n, hk, rng, crowded=False):
    """A few opening placements, then nothing but spreads that leave the game open, until the counter reaches the limit.
    crowded: placements until two squares are empty, then spreads that free no square where there are any, so that few placements
    compete with the spreads in a search.  Returns {counter: state} for 97..100 plus "reset" / "reset-flatten", or None if the
    spreads ran out."""
    nn = n * n
    s = O.state_default(lib, n, hk)
    for _ in range(nn - 2 if crowded else min(10, nn - 3)):
        mv = [m for m in O.possible_moves(lib, s) if m < 3 * nn]
        walls = [m for m in mv if nn <= m < 2 * nn]
        pool = _shuffled(rng, walls) + _shuffled(rng, mv) if rng.random() < 0.6 else _shuffled(rng, mv)
        m, t = _first(lib, s, pool, lambda t: terminal(lib, t) == -1)
        if m is None:
            return None
        s = t
    out = {}
    for _ in range(1200):
        r = s.reversible_plies
        if r >= LIMIT - 3:
            out[r] = s
        if r >= LIMIT:
            return out
        mv = O.possible_moves(lib, s)
        spreads = _shuffled(rng, [m for m in mv if m >= 3 * nn])
        if crowded:
            def freed(m):
                _, sq, step, drops = decode(n, m)
                return (sum(drops) == s.height[sq]) - sum(1 for k in range(len(drops)) if s.top[sq + (k + 1) * step] == 0)
            spreads.sort(key=freed)
        if r == LIMIT - 1:
            m, t = _first(lib, s, _shuffled(rng, [m for m in mv if m < 3 * nn]), lambda t: True)
            if m is not None:
                out["reset"] = (m, t)
            m, t = _first(lib, s, spreads, lambda t: t.reversible_plies == 0)
            if m is not None:
                out["reset-flatten"] = (m, t)
        # a spread that flattens a wall puts the counter back: take those last
        m, t = _first(lib, s, spreads, lambda t: t.reversible_plies > 0 and (terminal(lib, t) == -1 or t.reversible_plies >= LIMIT))
        if m is None:
            m, t = _first(lib, s, spreads, lambda t: terminal(lib, t) == -1)
        if m is None:
            return None
        s = t
    return None


def _tower_game(lib, n, hk, rng, plies):
    """Greedily take the spread that raises the tallest stack, else place a flat in line with it.
    Returns the positions where the stack is at least TOWER_MIN high and its owner is to move, and (position, move) one ply before
    a spread lands on that stack when it is already TOWER_MIN - 1 high: the drop is shifted past the word boundary."""
    nn = n * n
    s = O.state_default(lib, n, hk)
    kept, onto = [], []
    for _ in range(plies):
        if terminal(lib, s) != -1:
            break
        mv = O.possible_moves(lib, s)
        T, hT = tallest(s)
        if hT >= TOWER_MIN[n] and owner(s, T) == s.to_move:
            kept.append(s)
        gains = []
        for m in mv:
            d = decode(n, m)
            if d[0] != "spread" or d[1] == T:
                continue
            _, sq, step, drops = d
            g = sum(c for k, c in enumerate(drops) if sq + (k + 1) * step == T)
            if g > 0:
                gains.append((-g, float(rng.random()), m))
        greedy = [m for _, _, m in sorted(gains)]
        tx, ty = T % n, T // n
        flats = [m for m in mv if m < nn]
        near = sorted(flats, key=lambda m: (0 if (m % n == tx or m // n == ty) else 1, abs(m % n - tx) + abs(m // n - ty), float(rng.random())))
        # captures beside the stack mix the colours that later go onto it: a stack of strictly alternating colours would hide a
        # shift that is off by two
        side = _shuffled(rng, [m for m in mv if m >= 3 * nn and decode(n, m)[1] != T and m not in greedy])
        r = rng.random()
        if r < 0.55:
            pool = greedy + near + side
        elif r < 0.7:
            pool = _shuffled(rng, greedy) + near + side
        elif r < 0.85:
            pool = near + greedy + side
        else:
            pool = side + near + greedy
        pool += _shuffled(rng, mv)
        m, t = _first(lib, s, pool, lambda t: terminal(lib, t) == -1)
        if m is None:
            break
        if hT >= TOWER_MIN[n] - 1 and m in greedy:
            onto.append((s, m))
        s = t
    return kept, onto


def _walls_game(lib, n, hk, rng):
    """Fill the board: walls mostly, flats where they complete no road, a wall on the last square.  Returns {empties: state}."""
    nn = n * n
    s = O.state_default(lib, n, hk)
    out = {}
    for _ in range(nn):
        e = empties(s)
        out[e] = s
        mv = O.possible_moves(lib, s)
        flats, walls = [m for m in mv if m < nn], [m for m in mv if nn <= m < 2 * nn]
        if s.ply < 2 or (e > 1 and rng.random() < 0.4):
            pool = _shuffled(rng, flats) + _shuffled(rng, walls)
        else:
            pool = _shuffled(rng, walls)
        m, t = _first(lib, s, pool, lambda t: terminal(lib, t) == -1 or e == 1)
        if m is None:
            return None
        s = t
    out[0] = s
    return out


def _double_road(lib, n, hk, mover, col):
    """Rank 1 is the mover's but for one square, rank 2 the opponent's but for the same square, and above it stands the mover's
    stack of two with the opponent's piece below: two pieces down, one each, completes both roads."""
    me, opp = ("1", "2") if mover == 0 else ("2", "1")
    ranks = []
    for y in range(n - 1, -1, -1):
        if y == 2:
            cells = [opp + me if x == col else "x" for x in range(n)]
        elif y == 1:
            cells = ["x" if x == col else opp for x in range(n)]
        elif y == 0:
            cells = ["x" if x == col else me for x in range(n)]
        else:
            cells = ["x"] * n
        ranks.append(",".join(cells))
    before = O.state_from_tps(lib, "%s %d %d" % ("/".join(ranks), mover + 1, n + 1), n, hk)
    move = O.from_ptn(lib, n, "2%s3-11" % "abcdef"[col])
    assert move in O.possible_moves(lib, before)
    return before, move, O.play(lib, before, move)


# ---------------------------------------------------------------------------------------------- assembly
def _build(lib, n):
    hk = HALF_KOMI[n]
    positions, directed, tower_spreads, tower_drops, komi = [], {}, [], [], []

    def add(label, s):
        positions.append((label, s))
        return len(positions) - 1

    finished = []                                        # indices of games over by flat count, for the komi sweep

    def add_ending(prefix, hist):
        """The last four positions of a game that ended on empty reserves; False if it ended otherwise."""
        end = hist[-1]
        if len(hist) < 4 or not depleted(end):
            return False
        term, reason, _ = outcomes(lib, n, hk, [end])
        if term[0] == -1 or reason[0] != 2:
            return False
        for back in (3, 2, 1):
            add("%s/end-%d" % (prefix, back), hist[-1 - back])
        finished.append(add(prefix + "/end", end))
        return True

    # Deplete, on 4x4 and larger (3x3 meets the flat count on full boards below)
    if n >= 4:
        games = 0
        for seed in range(40):
            if games == 8:
                break
            hist, _ = _deplete_game(lib, n, hk, np.random.default_rng(1000 * n + seed), hold_cap=False)
            games += add_ending("deplete", hist)

    # Cap held back
    if n >= 5:
        games = 0
        for seed in range(40):
            if games == 5:
                break
            hist, cap_only = _deplete_game(lib, n, hk, np.random.default_rng(2000 * n + seed), hold_cap=True, dwell=2)
            cap_only = [s for s in cap_only if terminal(lib, s) == -1][:3]
            if not cap_only:
                continue
            for s in cap_only:
                add("capheld/cap-only", s)
            add_ending("capheld", hist)
            games += 1

    # Shuffle
    games = 0
    for seed in range(60):
        if games == 6:
            break
        got = _shuffle_game(lib, n, hk, np.random.default_rng(3000 * n + seed))
        if not got or "reset" not in got or any(r not in got for r in range(LIMIT - 3, LIMIT + 1)):
            continue
        games += 1
        for r in range(LIMIT - 3, LIMIT + 1):
            i = add("shuffle/%d" % r, got[r])
            if r == LIMIT - 1:
                directed[i] = [got["reset"][0]]
                add("shuffle/reset", got["reset"][1])
                if "reset-flatten" in got:
                    directed[i].append(got["reset-flatten"][0])
                    add("shuffle/reset-flatten", got["reset-flatten"][1])

    # Shuffle on a crowded board
    games = 0
    for seed in range(60):
        if games == 4:
            break
        got = _shuffle_game(lib, n, hk, np.random.default_rng(3500 * n + seed), crowded=True)
        if not got or "reset" not in got or any(r not in got for r in range(LIMIT - 3, LIMIT + 1)):
            continue
        games += 1
        for r in range(LIMIT - 3, LIMIT + 1):
            i = add("crowd/%d" % r, got[r])
            if r == LIMIT - 1:
                directed[i] = [got["reset"][0]]
                add("crowd/reset", got["reset"][1])

    # Tower
    seen = set()
    for seed in range(4):
        kept, onto = _tower_game(lib, n, hk, np.random.default_rng(4000 * n + seed), plies=400)
        # the drop of the most pieces onto the stack, and the last one of the game
        for s, m in ([max(onto, key=lambda sm: sum(decode(n, sm[1])[3]))] + onto[-1:] if onto else []):
            if bytes(s) in seen:
                continue
            seen.add(bytes(s))
            i = add("tower/onto", s)
            directed[i] = [m]
            tower_drops.append((i, m, add("tower/landed", O.play(lib, s, m))))
        for s in [kept[i] for i in sorted(set(np.linspace(0, len(kept) - 1, 4).astype(int)))] if kept else []:
            if bytes(s) in seen:
                continue
            seen.add(bytes(s))
            T, _ = tallest(s)
            out_of = [m for m in O.possible_moves(lib, s) if m >= 3 * n * n and decode(n, m)[1] == T]
            carried = {m: sum(decode(n, m)[3]) for m in out_of}
            most = max(carried.values()) if carried else 0
            full = [m for m in out_of if carried[m] == most]
            picks = []
            for m in full[:1] + full[-1:] + [m for m in out_of if carried[m] == 1][:1]:
                if m not in picks:
                    picks.append(m)
            i = add("tower/tall", s)
            directed[i] = picks
            for m in picks:
                tower_spreads.append((i, m, carried[m], add("tower/spread", O.play(lib, s, m))))

    # Walls
    games = 0
    for seed in range(20):
        if games == 3:
            break
        got = _walls_game(lib, n, hk, np.random.default_rng(5000 * n + seed))
        if not got:
            continue
        term, reason, _ = outcomes(lib, n, hk, [got[0]])
        if reason[0] != 2 or depleted(got[0]):
            continue
        games += 1
        add("walls/full-3", got[3])
        add("walls/full-1", got[1])
        finished.append(add("walls/full", got[0]))

    # Komi sweep (hand-made: only half_komi changes)
    swept = finished[:5] + finished[-3:] if len(finished) > 8 else finished
    for i in swept:
        base = positions[i][1]
        d = lib.tzo_flat_diff(C.byref(base))
        idx = []
        for label, k in (("komi/white", 2 * d - 1), ("komi/draw", 2 * d), ("komi/black", 2 * d + 1)):
            s = copy_state(base)
            s.half_komi = max(-128, min(127, k))
            idx.append(add(label, s))
        komi.append((i, idx))

    # Double road (hand-made, from TPS)
    for mover, col in ((0, 1), (1, n - 1)):
        before, move, after = _double_road(lib, n, hk, mover, col)
        name = "white" if mover == 0 else "black"
        directed[add("road2/before-" + name, before)] = [move]
        add("road2/after-" + name, after)

    # Gumbel roots
    if n in GUMBEL_ROOTS:
        count, lo, hi = GUMBEL_ROOTS[n]
        for s in random_positions(lib, O, n, hk, count, 6000 + n, min_ply=lo, max_ply=hi):
            add("gumbel/root", s)

    assert len(positions) <= MAX_POSITIONS, (n, len(positions))
    return Fixture(n, hk, positions, directed, tower_spreads, tower_drops, komi)


def fixture(lib, n):
    if n not in _cache:
        _cache[n] = _build(lib, n)
    return _cache[n]


def labelled(lib, n, *prefixes):
    """The states of board size n whose label starts with one of `prefixes`, in fixture order."""
    return [s for label, s in fixture(lib, n).positions if label.startswith(prefixes)]


def counts(lib, n):
    out = {}
    for label, _ in fixture(lib, n).positions:
        out[label] = out.get(label, 0) + 1
    return out
