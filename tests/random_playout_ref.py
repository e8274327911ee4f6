"""CPU reference of tz_search_random_steps: uniformly random legal play (Environment::new_opening_with_random_steps after the
opening, env.rs:81-95) with the engine's keyed draw, written from its definition over the oracle's rules.

    u = mix64(mix64(mix64(seed) ^ game_id) ^ ply)        ply = the position's own ply counter
    j = ((u >> 32) * n) >> 32                            n = the number of legal moves, j indexes them in move order

mix64 is splitmix64's finaliser in Python integers.  A game stops when it has no legal move, when its move list is wider than
ROW (1024), or, with stop_at_terminal, when its position is terminal; without that flag the end of a game is not looked at."""
import ctypes as C

import numpy as np

import oracle_lib as O

M64 = (1 << 64) - 1
ROW = 1024
OPENING_COUNTER = 0xFFFFFFFF   # the counter of the opening choice: no ply reaches it


def mix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def game_key(seed, game_id):
    return mix64(mix64(seed & M64) ^ (game_id & M64))


def draw_index(key, ply, n):
    u = mix64(key ^ ply)
    return ((u >> 32) * n) >> 32


def opening_choice(seed, game_id):
    return mix64(game_key(seed, game_id) ^ OPENING_COUNTER) % 16


def playout(lib, state, seed, game_id, steps, stop_at_terminal=False, record_positions=False):
    """-> dict(moves, nlegal, played, state, overflow[, positions]): moves / nlegal are lists of length `played`; `positions` the
    position before each move; overflow = the playout met a position with more than ROW legal moves."""
    key = game_key(seed, game_id)
    s = O.TzState()
    C.memmove(C.byref(s), C.byref(state), C.sizeof(O.TzState))
    moves, nlegal, positions = [], [], []
    overflow = False
    for _ in range(steps):
        if stop_at_terminal and lib.tzo_terminal(C.byref(s)) != -1:
            break
        legal = O.possible_moves(lib, s)
        n = len(legal)
        if n == 0:
            break
        if n > ROW:
            overflow = True
            break
        a = legal[draw_index(key, s.ply, n)]
        if record_positions:
            positions.append(s)
        moves.append(a)
        nlegal.append(n)
        s = O.play(lib, s, a)
    out = dict(moves=moves, nlegal=nlegal, played=len(moves), state=s, overflow=overflow)
    if record_positions:
        out["positions"] = positions
    return out


def playout_batch(lib, states, seed, game_base, steps, stop_at_terminal=False):
    """What BatchedMCTS.random_steps returns, plus the final positions: (moves[B, steps] u16, nlegal[B, steps] u16, played[B] i32,
    states[B] STATE_DTYPE, overflow: any game met a position wider than ROW)."""
    B = len(states)
    moves = np.full((B, steps), 0xFFFF, np.uint16)
    nlegal = np.zeros((B, steps), np.uint16)
    played = np.zeros(B, np.int32)
    finals, overflow = [], False
    for g, st in enumerate(states):
        r = playout(lib, st, seed, game_base + g, steps, stop_at_terminal)
        moves[g, :r["played"]] = r["moves"]
        nlegal[g, :r["played"]] = r["nlegal"]
        played[g] = r["played"]
        finals.append(r["state"])
        overflow = overflow or r["overflow"]
    return moves, nlegal, played, O.states_array(finals), overflow


def opening(lib, n, half_komi, choice):
    s = O.TzState()
    lib.tzo_new_opening(n, half_komi, int(choice), C.byref(s))
    return s


def as_tzstates(arr):
    """numpy STATE_DTYPE records -> list of TzState"""
    arr = np.ascontiguousarray(arr, dtype=O.STATE_DTYPE).reshape(-1)
    out = []
    for i in range(len(arr)):
        s = O.TzState()
        C.memmove(C.byref(s), arr.ctypes.data + i * 376, 376)
        out.append(s)
    return out


def reference_envs(lib, n, half_komi, batch, ply, count, seed, first_game=0):
    """eee.reference_envs on the CPU (utils.rs:14-32): game i opens with opening_choice(seed, first_game + i) and plays `ply` random
    moves.  `batch` has no influence here (the device works in waves of it; game ids are consecutive either way)."""
    finals = []
    for i in range(count):
        gid = first_game + i
        st = opening(lib, n, half_komi, opening_choice(seed, gid))
        finals.append(playout(lib, st, seed, gid, ply)["state"])
    return O.states_array(finals)
