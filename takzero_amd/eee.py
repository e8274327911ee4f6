"""The exploration experiments of the reference's `eee` crate that sit on random playouts, on the device:

    reference_envs  <- eee/src/utils.rs:14-32      positions reached by uniformly random legal play from the openings
    seen_ratio      <- eee/src/seen_ratio.rs:16-29 share of such positions, per ply, that a hash net has not seen

The reference draws from one StdRng stream; here every game has its own key, (seed, game_id), and draws by counter
(tz_search_random_steps): the ply for a move, OPENING_COUNTER for the opening choice.  A handle for these calls can be small:
batch 4096 and node_capacity 1, since a playout uses no tree beyond the root slot."""
import numpy as np

from ._lib import STATE_DTYPE

_M64 = (1 << 64) - 1
OPENING_COUNTER = 0xFFFFFFFF   # a counter no ply reaches (plies are 16 bits)


def mix64(x):
    """tz_mix64 (csrc/tz_math.h) in Python integers"""
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def opening_choices(seed, game_base, count):
    """opening choice in [0, 16) of games game_base .. game_base + count - 1: the playout's key with the opening's counter"""
    ids = (np.arange(count, dtype=np.uint64) + np.uint64(int(game_base) & _M64))     # uint64 array arithmetic wraps
    keys = _mix64_array(ids ^ np.uint64(mix64(int(seed) & _M64)))
    return (_mix64_array(keys ^ np.uint64(OPENING_COUNTER)) % np.uint64(16)).astype(np.int32)


def _mix64_array(x):
    x = x + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def reference_envs(mcts, ply, count, seed, game_base=0):
    """`count` positions, each a fresh opening followed by `ply` uniformly random legal moves (fewer if the game runs out of
    moves), made in waves of the handle's batch; game i has id game_base + i.  Returns STATE_DTYPE[count]."""
    out = np.zeros(count, STATE_DTYPE)
    for _, lo, hi in _waves(mcts, ply, count, seed, game_base):
        out[lo:hi] = mcts.get_positions()[:hi - lo]
    return out


def _waves(mcts, ply, count, seed, game_base):
    """runs the waves of reference_envs; after each, the handle's first hi - lo games hold positions lo .. hi - 1"""
    B = mcts.batch
    for lo in range(0, count, B):
        hi = min(count, lo + B)
        mcts.new_openings(opening_choices(seed, game_base + lo, B))
        mcts.random_steps(ply, seed, game_base=game_base + lo)
        yield mcts, lo, hi


def seen_ratio(mcts, plies=range(100), games=65536, seed=123):
    """[(ply, ratio)]: for each ply, `games` fresh random games of that many moves and the share of their positions that the
    handle's hash net has not seen (forward_hash().mean() / MAXIMUM_VARIANCE, seen_ratio.rs:24-26).  Game ids differ between
    plies, as the reference's generator moves on: game_base = ply * games + the wave's offset.  The positions stay on the device."""
    out = []
    for ply in plies:
        unseen = 0
        for m, lo, hi in _waves(mcts, ply, games, seed, ply * games):
            unseen += int((m.hash_seen()[:hi - lo] == 0).sum())
        out.append((ply, float(np.float32(unseen / games))))
    return out
