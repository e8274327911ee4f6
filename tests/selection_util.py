"""Builds tests/selection_ref.cpp (the CPU restatement of the three in-tree selection rules and of the loops around Node::forward,
over the oracle's primitives) and wraps it with the call surface the selection tests need; compare() holds a device search, or the
oracle's own, to it bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PUCT, UCT, IMPROVED = 0, 1, 2
RULE_NAMES = {PUCT: "puct", UCT: "uct", IMPROVED: "improved"}
CHILD_KEYS = ("move_idx", "visits", "eval_tag", "eval_bits", "logit", "prob", "std_dev")


def load(so):
    lib = C.CDLL(so)
    vp, ci = C.c_void_p, C.c_int
    lib.sel_m_ln.restype = C.c_float
    lib.sel_m_ln.argtypes = [C.c_float]
    lib.sel_create.restype = vp
    lib.sel_create.argtypes = [ci, O.AGENT_FN, vp, ci, ci, ci]
    lib.sel_destroy.argtypes = [vp]
    lib.sel_set_rule.argtypes = [vp, ci]
    lib.sel_nan_seen.argtypes = [vp]
    lib.sel_set_positions.argtypes = [vp, ci, vp, vp]
    lib.sel_new_openings.argtypes = [vp, vp]
    lib.sel_simulate.argtypes = [vp, vp, ci]
    lib.sel_simulate_batch.argtypes = [vp, vp, ci, ci]
    lib.sel_gumbel_sh.argtypes = [vp, vp, ci, ci, vp, ci, vp]
    lib.sel_select_at_root.argtypes = [vp, ci, ci, C.c_float]
    lib.sel_tree_size.restype = C.c_uint64
    lib.sel_tree_size.argtypes = [vp, ci]
    lib.sel_node.argtypes = [vp, ci, vp, ci, vp, ci] + [vp] * 7
    lib.path = so
    return lib


def build(out_dir):
    """g++ with the flags of oracle/Makefile; the library goes into out_dir (a temporary directory)"""
    so = os.path.join(str(out_dir), "libselection_ref.so")
    cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unused-function", "-shared",
           "-o", so, os.path.join(ROOT, "tests", "selection_ref.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return load(so)


class RefSearch:
    """The restatement with the call surface of takzero_amd.api.BatchedMCTS, as far as these tests use it."""

    def __init__(self, lib, batch, n, half_komi, agent_kind=1, agent_fn=None, rule=PUCT):
        self.lib, self.batch, self.n, self.half_komi = lib, batch, n, half_komi
        self._cb = O.AGENT_FN(agent_fn) if agent_fn is not None else C.cast(None, O.AGENT_FN)
        self.h = lib.sel_create(agent_kind, self._cb, None, batch, n, half_komi)
        self.set_selection(rule)

    def close(self):
        if self.h:
            self.lib.sel_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def set_selection(self, rule):
        assert self.lib.sel_set_rule(self.h, rule) == 0

    def nan_seen(self):
        return bool(self.lib.sel_nan_seen(self.h))

    def set_positions(self, idx, states):
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        arr = O.states_array(states) if isinstance(states, list) else states
        assert self.lib.sel_set_positions(self.h, len(idx), idx.ctypes.data, arr.ctypes.data) == 0

    def new_openings(self, choice):
        choice = np.ascontiguousarray(choice, dtype=np.int32)
        self.lib.sel_new_openings(self.h, choice.ctypes.data)

    def simulate(self, betas, n_sims=1):
        betas = np.ascontiguousarray(betas, dtype=np.float32)
        assert self.lib.sel_simulate(self.h, betas.ctypes.data, n_sims) == 0

    def simulate_batch(self, betas, leaves, rounds=1):
        betas = np.ascontiguousarray(betas, dtype=np.float32)
        assert self.lib.sel_simulate_batch(self.h, betas.ctypes.data, leaves, rounds) == 0

    def gumbel_sequential_halving(self, betas, k, budget, gumbel):
        betas = np.ascontiguousarray(betas, dtype=np.float32)
        gumbel = np.ascontiguousarray(gumbel, dtype=np.float32)
        out = np.zeros(self.batch, np.uint16)
        assert self.lib.sel_gumbel_sh(self.h, betas.ctypes.data, k, budget, gumbel.ctypes.data, gumbel.shape[1], out.ctypes.data) == 0
        return out

    def select_at_root(self, game, rule, beta):
        return self.lib.sel_select_at_root(self.h, game, rule, beta)

    def node(self, game, path, amax=1024):
        p = np.ascontiguousarray(path, dtype=np.uint16)
        info = np.zeros(1, O.ROOT_INFO_DTYPE)
        out = dict(move_idx=np.zeros(amax, np.uint16), visits=np.zeros(amax, np.uint32), eval_tag=np.zeros(amax, np.uint8),
                   eval_bits=np.zeros(amax, np.uint32), logit=np.zeros(amax, np.float32), prob=np.zeros(amax, np.float32),
                   std_dev=np.zeros(amax, np.float32))
        rc = self.lib.sel_node(self.h, game, p.ctypes.data if len(p) else None, len(p), info.ctypes.data, amax,
                               *[out[k].ctypes.data for k in CHILD_KEYS])
        if rc != 0:
            return None
        nc = int(info[0]["n_children"])
        return info[0], {k: v[:nc] for k, v in out.items()}

    def tree_size(self, game):
        return int(self.lib.sel_tree_size(self.h, game))

    def root_visits(self, game):
        return self.node(game, [])[1]["visits"].copy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else a


def same_node(a, b, where):
    """visit count, eval tag and bits, logit / probability / std_dev bits of the node; child order and the same of every child"""
    assert a is not None and b is not None, where
    (ia, ca), (ib, cb) = a, b
    for k in ("visit_count", "n_children", "eval_tag", "eval_bits"):
        assert ia[k] == ib[k], (where, k, ia[k], ib[k])
    for k in ("std_dev", "logit", "probability"):
        assert np.float32(ia[k]).view(np.uint32) == np.float32(ib[k]).view(np.uint32), (where, k, ia[k], ib[k])
    for k in CHILD_KEYS:
        assert np.array_equal(bits(ca[k]), bits(cb[k])), (where, k, np.flatnonzero(bits(ca[k]) != bits(cb[k]))[:8])


def compare(dev, ref, where=""):
    """Per game: the root and everything about all its children, then the node one ply and the node two plies down the most
    visited line (last maximum), each with everything about its children.  dev has root_children() when it is a device handle
    (tz_search_root_children is then held to the same rows); dev.node and ref.node have the same signature.  Returns the number
    of nodes whose statistics were compared."""
    nodes = 0
    rc = dev.root_children() if hasattr(dev, "root_children") else None
    for g in range(ref.batch):
        root = ref.node(g, [])
        same_node(dev.node(g, []), root, (where, g, "root"))
        nc = len(root[1]["move_idx"])
        nodes += 1 + nc
        if rc is not None:
            for k in CHILD_KEYS:
                assert np.array_equal(bits(rc[k][g, :nc]), bits(root[1][k])), (where, g, "root_children", k)
                assert not rc[k][g, nc:].any(), (where, g, "root_children tail", k)
        path, cur = [], root
        for ply in (1, 2):
            v = cur[1]["visits"]
            if len(v) == 0 or v.max() == 0:
                break
            path.append(int(cur[1]["move_idx"][len(v) - 1 - int(np.argmax(v[::-1]))]))
            cur = ref.node(g, path)
            same_node(dev.node(g, path), cur, (where, g, tuple(path)))
            nodes += 1 + len(cur[1]["move_idx"])
    return nodes


def agent_over(net):
    """the restatement's Agent = the HIP network through tz_net_eval, as in tests/test_gpu_engine.py: both sides get the same
    network outputs"""
    def fn(user, n_envs, states, legal_idx, legal_count, amax, logits_out, value_out, variance_out):
        rc = net.lib.tz_net_eval(net.h, n_envs, C.cast(states, C.c_void_p), C.cast(legal_idx, C.c_void_p),
                                 C.cast(legal_count, C.c_void_p), amax, C.cast(logits_out, C.c_void_p),
                                 C.cast(value_out, C.c_void_p), C.cast(variance_out, C.c_void_p))
        assert rc == 0, net.lib.tz_last_error()
    return fn


def switch_case(A, lib):
    """Switching the rule on a live handle: 10 PUCT simulations (past the two eager warm-up calls, so the simulation graph is
    captured and replaying unless TZ_NO_GRAPH is set), then IMPROVED and 10 more, then UCT and 10 more, one simulation per call;
    the restatement switches at the same points.  Returns the number of nodes compared."""
    B, n, komi = 8, 5, 4
    choice = (np.arange(B) * 3 + 1).astype(np.int32) % 16
    betas = np.full(B, 0.25, np.float32)
    ref = RefSearch(lib, B, n, komi, agent_kind=2)
    gpu = A.BatchedMCTS(B, n, komi, agent_kind=A.AGENT_SIMPLE)
    ref.new_openings(choice)
    gpu.new_openings(choice)
    nodes = 0
    assert gpu.selection == "puct"
    for rule in (PUCT, IMPROVED, UCT):
        ref.set_selection(rule)
        gpu.set_selection(rule)
        assert gpu.selection == RULE_NAMES[rule]
        for _ in range(10):
            ref.simulate(betas, 1)
            gpu.simulate(betas, 1)
        nodes += compare(gpu, ref, "after 10 of " + RULE_NAMES[rule])
    assert gpu.pool_overflows() == 0 and not ref.nan_seen()
    return nodes


def wide_positions(oracle, seed=4, plies=80):
    """Positions of one 5x5 playout in which both sides mostly (4 plies in 5) play the move that leaves the two of them the most
    legal moves, so that stacks grow: plain random playouts stay below 100 legal moves.  Returns (a position with more than 64 and
    at most 128 legal moves, a position with more than 128 and at most 169, SURVEY.md section 6's 5x5 maximum)."""
    def options(t):
        u = O.TzState.from_buffer_copy(bytes(t))
        u.to_move ^= 1
        return len(O.possible_moves(oracle, t)) + len(O.possible_moves(oracle, u))

    rng = np.random.default_rng(seed)
    s = O.state_default(oracle, 5, 4)
    mid, wide = None, None
    for ply in range(plies):
        if oracle.tzo_terminal(C.byref(s)) != -1:
            break
        mv = O.possible_moves(oracle, s)
        if 64 < len(mv) <= 128 and mid is None:
            mid = s
        if 128 < len(mv) <= 169 and (wide is None or len(mv) > len(O.possible_moves(oracle, wide))):
            wide = s
        if rng.random() < 0.2 or ply < 2:
            s = O.play(oracle, s, mv[int(rng.integers(len(mv)))])
            continue
        after = [O.play(oracle, s, m) for m in mv]
        s = after[int(np.argmax([-1 if oracle.tzo_terminal(C.byref(t)) != -1 else options(t) for t in after]))]
    assert mid is not None and wide is not None
    return mid, wide
