"""Builds tests/simulate_batch_ref.cpp (the CPU restatement of Node::simulate_batch over the oracle's primitives) and wraps it with
the call surface the simulate_batch tests need; compare() holds a device search to it bit for bit."""
import ctypes as C
import os
import subprocess

import numpy as np

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT_NAMES = ("forwards", "known_in_round", "leaves", "duplicate_leaves", "short_rounds")
CHILD_KEYS = ("move_idx", "visits", "eval_tag", "eval_bits", "logit", "prob", "std_dev")


def build(out_dir):
    """g++ with the flags of oracle/Makefile; the library goes into out_dir (a temporary directory)"""
    so = os.path.join(str(out_dir), "libsimulate_batch_ref.so")
    cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unused-function", "-shared",
           "-o", so, os.path.join(ROOT, "tests", "simulate_batch_ref.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lib = C.CDLL(so)
    vp, ci = C.c_void_p, C.c_int
    lib.sbr_create.restype = vp
    lib.sbr_create.argtypes = [ci, O.AGENT_FN, vp, ci, ci, ci]
    lib.sbr_destroy.argtypes = [vp]
    lib.sbr_set_positions.argtypes = [vp, ci, vp, vp]
    lib.sbr_new_openings.argtypes = [vp, vp]
    lib.sbr_simulate_batch.argtypes = [vp, vp, ci, ci]
    lib.sbr_simulate.argtypes = [vp, vp, ci]
    lib.sbr_step.argtypes = [vp, vp]
    lib.sbr_counts.argtypes = [vp, vp]
    lib.sbr_round_leaves.argtypes = [vp, vp]
    lib.sbr_principal_variation.argtypes = [vp, ci, vp, ci]
    lib.sbr_tree_size.restype = C.c_uint64
    lib.sbr_tree_size.argtypes = [vp, ci]
    lib.sbr_node.argtypes = [vp, ci, vp, ci, vp, ci] + [vp] * 7
    return lib


class RefSearch:
    """The restatement with the call surface of takzero_amd.api.BatchedMCTS, as far as these tests use it."""

    def __init__(self, lib, batch, n, half_komi, agent_kind=1, agent_fn=None):
        self.lib, self.batch, self.n, self.half_komi = lib, batch, n, half_komi
        self._cb = O.AGENT_FN(agent_fn) if agent_fn is not None else C.cast(None, O.AGENT_FN)
        self.h = lib.sbr_create(agent_kind, self._cb, None, batch, n, half_komi)

    def close(self):
        if self.h:
            self.lib.sbr_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def set_positions(self, idx, states):
        idx = np.ascontiguousarray(idx, dtype=np.int32)
        arr = O.states_array(states) if isinstance(states, list) else states
        assert self.lib.sbr_set_positions(self.h, len(idx), idx.ctypes.data, arr.ctypes.data) == 0

    def new_openings(self, choice):
        choice = np.ascontiguousarray(choice, dtype=np.int32)
        self.lib.sbr_new_openings(self.h, choice.ctypes.data)

    def simulate_batch(self, betas, leaves, rounds=1):
        betas = np.ascontiguousarray(betas, dtype=np.float32)
        assert self.lib.sbr_simulate_batch(self.h, betas.ctypes.data, leaves, rounds) == 0

    def simulate(self, betas, n_sims=1):
        """lock-step BatchedMCTS::simulate on the same trees"""
        betas = np.ascontiguousarray(betas, dtype=np.float32)
        assert self.lib.sbr_simulate(self.h, betas.ctypes.data, n_sims) == 0

    def step(self, actions):
        actions = np.ascontiguousarray(actions, dtype=np.uint16)
        self.lib.sbr_step(self.h, actions.ctypes.data)

    def counts(self):
        out = np.zeros(len(COUNT_NAMES), np.uint64)
        self.lib.sbr_counts(self.h, out.ctypes.data)
        return dict(zip(COUNT_NAMES, (int(x) for x in out)))

    def round_leaves(self):
        """per tree, the leaves it collected in the latest simulate_batch round"""
        out = np.zeros(self.batch, np.uint32)
        self.lib.sbr_round_leaves(self.h, out.ctypes.data)
        return out

    def tree_size(self, game):
        return int(self.lib.sbr_tree_size(self.h, game))

    def principal_variation(self, game):
        out = np.zeros(512, np.uint16)
        n = self.lib.sbr_principal_variation(self.h, game, out.ctypes.data, len(out))
        assert 0 <= n <= len(out), n
        return out[:n].copy()

    def node(self, game, path, amax=1024):
        p = np.ascontiguousarray(path, dtype=np.uint16)
        info = np.zeros(1, O.ROOT_INFO_DTYPE)
        out = dict(move_idx=np.zeros(amax, np.uint16), visits=np.zeros(amax, np.uint32), eval_tag=np.zeros(amax, np.uint8),
                   eval_bits=np.zeros(amax, np.uint32), logit=np.zeros(amax, np.float32), prob=np.zeros(amax, np.float32),
                   std_dev=np.zeros(amax, np.float32))
        rc = self.lib.sbr_node(self.h, game, p.ctypes.data if len(p) else None, len(p), info.ctypes.data, amax,
                               *[out[k].ctypes.data for k in CHILD_KEYS])
        if rc != 0:
            return None
        nc = int(info[0]["n_children"])
        return info[0], {k: v[:nc] for k, v in out.items()}


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
        assert np.array_equal(bits(ca[k]), bits(cb[k])), (where, k)


def compare(dev, ref, where="", deep=None):
    """The root, all its children, every node to depth 2, every node along the principal variation, and the PV itself.
    `deep` lists the trees walked below the root and along the PV (all trees when None); the root and all its children are
    compared on every tree.
    A node query returns the node and the statistics of all its children, so the queries of the root and of every depth-1 node
    cover every node to depth 2; the depth-2 nodes that were visited are queried too, for their child lists (an unvisited node
    has none).  dev.node and ref.node have the same signature (api.BatchedMCTS.node / RefSearch.node or OracleSearch.node)."""
    nodes = 0
    for g in range(ref.batch):
        root = ref.node(g, [])
        same_node(dev.node(g, []), root, (where, g, "root"))
        nodes += 1
        if deep is not None and g not in deep:
            continue
        for m1 in root[1]["move_idx"]:
            n1 = ref.node(g, [m1])
            same_node(dev.node(g, [m1]), n1, (where, g, int(m1)))
            nodes += 1
            if n1[0]["visit_count"] == 0:
                continue        # never reached: no children to look at
            for m2 in n1[1]["move_idx"][n1[1]["visits"] > 0]:
                same_node(dev.node(g, [m1, m2]), ref.node(g, [m1, m2]), (where, g, int(m1), int(m2)))
                nodes += 1
        if hasattr(ref, "principal_variation"):
            pv = ref.principal_variation(g)
            assert np.array_equal(dev.principal_variation(g), pv), (where, g, "pv")
            for d in range(3, len(pv) + 1):
                same_node(dev.node(g, pv[:d]), ref.node(g, pv[:d]), (where, g, "pv", d))
                nodes += 1
    return nodes


# ---- starts of the wide cases (tests/test_gpu_simulate_batch_wide.py; tests/test_simulate_batch_ref.py holds their preconditions)
WIDE_TREES = (0, 63, 64, 65, 1023, 1024, 1025)      # either side of a wave of 64 trees and of compact_batch_kernel's 1024-tree chunk


def deep_trees(batch):
    """the trees a wide case walks in depth: WIDE_TREES where they exist, and the last tree"""
    return sorted({g for g in WIDE_TREES if g < batch} | {batch - 1})


def finished_position(oracle, n, half_komi, seed):
    """the end of a random playout: a tree started here collects nothing"""
    return playout(oracle, n, half_komi, seed)[-1]


def playout(oracle, n, half_komi, seed):
    """every position of one random game, the finished one last"""
    rng = np.random.default_rng(seed)
    s = O.state_default(oracle, n, half_komi)
    out = [s]
    while oracle.tzo_terminal(C.byref(s)) == -1:
        mv = O.possible_moves(oracle, s)
        s = O.play(oracle, s, mv[int(rng.integers(len(mv)))])
        out.append(s)
    return out


def mixed_starts(oracle, batch, n, half_komi, seed):
    """Starts by tree index: g % 3 == 0 a fresh opening (the returned choice, applied by new_openings), g % 3 == 1 the finished
    position of a random playout (collects nothing), g % 3 == 2 a position one to three plies before the end of one (Known results
    inside its rounds end them short).  Returns (choice for new_openings, tree indices, states for set_positions)."""
    games = [playout(oracle, n, half_komi, seed * 1000 + k) for k in range(96)]
    choice = (np.arange(batch) * 3 + 1).astype(np.int32) % 16
    idx, states = [], []
    for g in range(batch):
        game = games[(g // 3) % len(games)]
        if g % 3 == 1:
            idx.append(g)
            states.append(game[-1])
        elif g % 3 == 2:
            idx.append(g)
            states.append(game[max(0, len(game) - 2 - (g // 3) % 3)])
    return choice, np.array(idx, np.int32), states


def apply_starts(search, starts):
    choice, idx, states = starts
    search.new_openings(choice)
    search.set_positions(idx, O.states_array(states))


def ragged(round_leaves, leaves):
    """does one round hold a tree without a leaf, a tree with some and a tree with all of them"""
    r = np.asarray(round_leaves)
    return bool((r == 0).any() and ((r > 0) & (r < leaves)).any() and (r == leaves).any())
