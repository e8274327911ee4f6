"""A search handle's captured simulation graph against what happens to the network it names.

one_simulation (csrc/tz_capi.hip) runs a handle's first two lock-step simulations eagerly, captures the third as a HIP graph and
replays it from then on.  The captured launches hold, by value, the net's weights, its work buffers and its SimHash set; each of
them can be freed and replaced while the handle lives: by a host-side net call with a larger batch than the search's (forward_raw,
policy_value_uncertainty, hash_indices), by a second, larger handle on the same net, by simulate_batch on any handle of the net, by a
weight reload, by load_bitset.  tz_net_invalidate_captures (csrc/tz_nn.hip) is the one point all of them pass, and one_simulation drops
a graph of an older generation and captures again (DESIGN.md lists what a capture names and what replaces it).

The reference is a twin: a second Net with the same tensors and a second BatchedMCTS created under TZ_NO_GRAPH=1 (read in
tz_search_create), fed the same calls in the same order.  After every phase root_info, every field of root_children and
select_best_actions must be equal in every byte; at the end of a case forward_raw and policy_value_uncertainty of the two nets on
fixed positions must be equal and finite.  Every case runs simulate(8) - two eager simulations, one captured, five replayed - then
the event, simulate(8), the event at a still larger size, simulate(4).

For the events that grow buffers a pass proves no more than that the library behaves like eager execution.  That a library without
the invalidation is wrong - a replay that reads and writes freed device memory - rests on reading the code, not on a run: no test
here, and no variant of the library, provokes that on a GPU."""
import os

import numpy as np
import pytest

import oracle_lib as O
from exact_net import distinct_positions
from gpu_util import require_gpu
from test_gpu_engine import _agent_over
from test_gpu_tree import assert_same_roots

pytestmark = pytest.mark.gpu

CHILD_FIELDS = ("move_idx", "visits", "eval_tag", "eval_bits", "logit", "prob", "std_dev")
_POSITIONS = {}


def _positions(oracle, n, count):
    """`count` distinct positions (exact_net.distinct_positions), their array and their legal moves; built once per board size"""
    if n not in _POSITIONS or len(_POSITIONS[n][0]) < count:
        states = distinct_positions(oracle, O, n, max(count, 600), seed=17)
        _POSITIONS[n] = (O.states_array(states), [O.possible_moves(oracle, s) for s in states])
    arr, acts = _POSITIONS[n]
    return arr[:count], acts[:count]


def _bytes_equal(a, b, where):
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), where


def same_searches(gpu, twin, where):
    _bytes_equal(gpu.root_info(), twin.root_info(), (where, "root_info"))
    amax = max(1, int(twin.root_info()["n_children"].max()))
    gc, tc = gpu.root_children(amax), twin.root_children(amax)
    for k in CHILD_FIELDS:
        _bytes_equal(gc[k], tc[k], (where, "root_children", k))
    _bytes_equal(gpu.select_best_actions(), twin.select_best_actions(), (where, "select_best_actions"))


class Twins:
    """The graph-run side (index 0) and the eager twin (index 1): two nets of the same tensors, and searches created in pairs."""

    def __init__(self, A, monkeypatch, make_net):
        self.A, self.monkeypatch = A, monkeypatch
        self.nets = (make_net(), make_net())
        self.pairs = []

    def search(self, B, n, capacity):
        self.monkeypatch.delenv("TZ_NO_GRAPH", raising=False)
        gpu = self.A.BatchedMCTS(B, n, 4, agent=self.nets[0], node_capacity=capacity)
        self.monkeypatch.setenv("TZ_NO_GRAPH", "1")
        twin = self.A.BatchedMCTS(B, n, 4, agent=self.nets[1], node_capacity=capacity)
        self.monkeypatch.delenv("TZ_NO_GRAPH")
        self.pairs.append((gpu, twin))
        return gpu, twin

    def check(self, where):
        for k, (gpu, twin) in enumerate(self.pairs):
            same_searches(gpu, twin, (where, "handle %d" % k))

    def finish(self, oracle, n):
        """forward_raw and policy_value_uncertainty on fixed positions: equal between the two nets, and finite"""
        arr, acts = _positions(oracle, n, 48)
        for name, call in (("forward_raw", lambda net: net.forward_raw(arr)), ("policy_value_uncertainty", lambda net: net.policy_value_uncertainty(arr, acts))):
            a, b = call(self.nets[0]), call(self.nets[1])
            flat = lambda out: [np.concatenate(x) if isinstance(x, list) else x for x in out]
            for x, y in zip(flat(a), flat(b)):
                _bytes_equal(x, y, name)
                assert np.all(np.isfinite(x)), name
        for gpu, twin in self.pairs:
            assert gpu.pool_overflows() == 0 and twin.pool_overflows() == 0


def _base(A, monkeypatch, B=64, n=5, seed=123):
    from takzero_amd import weights as W

    t = Twins(A, monkeypatch, lambda: A.Net(arch=A.ARCH_TEST, n=n, precision=A.PREC_F16, blocks=2).load_tensors(
        W.init_weights(W.ARCH_TEST, n=n, blocks=2, seed=seed)))
    gpu, twin = t.search(B, n, 1 << 16)
    choice = (np.arange(B) * 3 + 1).astype(np.int32) % 16
    gpu.new_openings(choice)
    twin.new_openings(choice)
    betas = np.where(np.arange(B) % 2 == 0, 0.0, 0.25).astype(np.float32)
    return t, gpu, twin, choice, betas


def _run(t, gpu, twin, betas, event):
    """simulate(8), event(0), simulate(8), event(1), simulate(4), compared after every phase"""
    for phase, sims in enumerate((8, 8, 4)):
        gpu.simulate(betas, sims)
        twin.simulate(betas, sims)
        t.check("simulate %d" % phase)
        if phase < 2:
            event(phase)
            t.check("event %d" % phase)


# ---- host-side net calls with more positions than the search has games
def test_forward_raw_grows_the_buffers_under_a_captured_search(oracle, monkeypatch):
    """... and the one case that is also held to the CPU oracle search fed by the net's own tz_net_eval, as tests/test_gpu_engine.py
    does it: forward_raw leaves the trees alone, so the oracle makes the 20 simulations without it."""
    A = require_gpu()
    t, gpu, twin, choice, betas = _base(A, monkeypatch)
    arr, _ = _positions(oracle, 5, 600)

    def event(k):
        size = (200, 600)[k]
        out = [net.forward_raw(arr[:size]) for net in t.nets]
        for x, y in zip(*out):
            _bytes_equal(x, y, ("forward_raw", size))

    _run(t, gpu, twin, betas, event)
    t.finish(oracle, 5)
    ora = O.OracleSearch(oracle, gpu.batch, 5, 4, agent_kind=0, agent_fn=_agent_over(t.nets[0]))
    ora.new_openings(choice)
    ora.simulate(betas, 20)
    assert_same_roots(gpu, ora, "against the oracle search")
    assert np.array_equal(gpu.select_best_actions(), ora.select_best_actions())
    assert gpu.counters() == ora.counters()


def test_policy_value_uncertainty_grows_the_buffers_under_a_captured_search(oracle, monkeypatch):
    A = require_gpu()
    t, gpu, twin, _, betas = _base(A, monkeypatch)
    arr, acts = _positions(oracle, 5, 600)

    def event(k):
        size = (200, 600)[k]
        out = [net.policy_value_uncertainty(arr[:size], acts[:size]) for net in t.nets]
        _bytes_equal(np.concatenate(out[0][0]), np.concatenate(out[1][0]), ("logits", size))
        _bytes_equal(out[0][1], out[1][1], ("value", size))
        _bytes_equal(out[0][2], out[1][2], ("variance", size))

    _run(t, gpu, twin, betas, event)
    t.finish(oracle, 5)


# ---- a second, larger handle on the same net
def test_a_larger_handle_on_the_same_net(oracle, monkeypatch):
    A = require_gpu()
    t, gpu, twin, _, betas = _base(A, monkeypatch)

    def event(k):
        B2 = (256, 1024)[k]
        big, big_twin = t.search(B2, 5, 1 << 10)
        choice = (np.arange(B2) * 5 + 2).astype(np.int32) % 16
        big.new_openings(choice)
        big_twin.new_openings(choice)
        b2 = np.where(np.arange(B2) % 2 == 0, 0.25, 0.0).astype(np.float32)
        for i in range(3):                     # old and new handles in alternation
            big.simulate(b2, 1)
            big_twin.simulate(b2, 1)
            gpu.simulate(betas, 1)
            twin.simulate(betas, 1)
            t.check("%d games, simulation %d" % (B2, i))

    _run(t, gpu, twin, betas, event)
    assert len(t.pairs) == 3
    t.finish(oracle, 5)


# ---- simulate_batch, on the handle itself and on a one-tree handle of the same net
def test_simulate_batch_grows_the_buffers_under_a_captured_search(oracle, monkeypatch):
    A = require_gpu()
    t, gpu, twin, _, betas = _base(A, monkeypatch)
    one, one_twin = t.search(1, 5, 1 << 17)
    for s in (one, one_twin):
        s.new_openings([3])
    b1 = np.zeros(1, np.float32)

    def event(k):
        leaves = (16, 64)[k]                   # 64 games x 16 / 64 leaves = 1024 / 4096 positions
        gpu.simulate_batch(betas, leaves, 1)
        twin.simulate_batch(betas, leaves, 1)

    _run(t, gpu, twin, betas, event)

    def event_one(k):
        leaves = (128, 1024)[k]                # 4096 positions are there by now: 1 x 128 replaces nothing, 1 x 1024 only leaf scratch
        one.simulate_batch(b1, leaves, 1)
        one_twin.simulate_batch(b1, leaves, 1)

    _run(t, gpu, twin, betas, event_one)
    t.finish(oracle, 5)


def test_simulate_batch_on_a_one_tree_handle_grows_the_buffers(oracle, monkeypatch):
    """the one-tree handle first: 1 x 128, then 1 x 1024 positions replace the buffers sized for the 64 games"""
    A = require_gpu()
    t, gpu, twin, _, betas = _base(A, monkeypatch)
    one, one_twin = t.search(1, 5, 1 << 17)
    for s in (one, one_twin):
        s.new_openings([3])
    b1 = np.zeros(1, np.float32)

    def event(k):
        leaves = (128, 1024)[k]
        one.simulate_batch(b1, leaves, 1)
        one_twin.simulate_batch(b1, leaves, 1)

    _run(t, gpu, twin, betas, event)
    t.finish(oracle, 5)


# ---- a weight reload: the path that was held already
def test_load_tensors_under_a_captured_search(oracle, monkeypatch):
    from takzero_amd import weights as W

    A = require_gpu()
    t, gpu, twin, _, betas = _base(A, monkeypatch)

    def event(k):
        w = W.init_weights(W.ARCH_TEST, n=5, blocks=2, seed=(7, 8)[k])
        for net in t.nets:
            net.load_tensors(w)

    _run(t, gpu, twin, betas, event)
    t.finish(oracle, 5)


# ---- the second graph slot: simulations that start below the root
def test_gumbel_halving_around_forward_raw(oracle, monkeypatch):
    """gumbel_sequential_halving(16, 128) in place of simulate: one simulation from the roots and 128 from sampled root children, which
    are captured in the handle's second graph."""
    A = require_gpu()
    t, gpu, twin, _, betas = _base(A, monkeypatch)
    arr, _ = _positions(oracle, 5, 600)
    gumbel = np.random.default_rng(5).gumbel(size=(gpu.batch, 512)).astype(np.float32)
    for phase in range(3):
        a = gpu.gumbel_sequential_halving(betas, 16, 128, gumbel)
        b = twin.gumbel_sequential_halving(betas, 16, 128, gumbel)
        _bytes_equal(a, b, ("selected", phase))
        t.check("halving %d" % phase)
        if phase < 2:
            size = (200, 600)[phase]
            out = [net.forward_raw(arr[:size]) for net in t.nets]
            for x, y in zip(*out):
                _bytes_equal(x, y, ("forward_raw", size))
            t.check("event %d" % phase)
    t.finish(oracle, 5)


# ---- the SimHash set
def test_hash_indices_and_load_bitset_under_a_captured_search(oracle, monkeypatch, tmp_path):
    """net4_simhash, 32 games, f16, the constant UBE head of tests/test_gpu_simhash.py (variance expf(c) = 0.5 on seen positions, 4 on
    the others).  hash_indices on 300 positions grows the work buffers, on 700 with update=True grows them again and fills the set;
    load_bitset replaces the set by a file written by numpy.  The roots are then set to 32 decided positions of that file's fixture,
    the file holding the fp64 index of every second one.  After one more simulation (a replay of a fresh capture) every root child
    carries its root's sqrtf(variance): exactly 2 where the root's index is not in the file, sqrtf(expf(c)) where it is - expf to
    rtol 1e-6 as in that file, a correctly rounded sqrtf halves that and adds 2^-24, so the std_dev is held to rtol 1e-6."""
    from test_gpu_simhash import UBE_CONSTANTS, constant_ube, simhash_fixture

    A = require_gpu()
    f = simhash_fixture(oracle, 4)
    B, n, c = 32, 4, UBE_CONSTANTS[0]
    t = Twins(A, monkeypatch, lambda: A.Net(arch=f["arch"], precision=A.PREC_F16).load_tensors(constant_ube(f["w"], c)))
    gpu, twin = t.search(B, n, 1 << 12)
    choice = (np.arange(B) * 3 + 1).astype(np.int32) % 16
    gpu.new_openings(choice)
    twin.new_openings(choice)
    betas = np.where(np.arange(B) % 2 == 0, 0.0, 0.25).astype(np.float32)

    def event(k):
        lo, hi, update = ((0, 300, False), (300, 1000, True))[k]
        out = [net.hash_indices(f["arr"][lo:hi], update=update) for net in t.nets]
        _bytes_equal(out[0], out[1], ("hash_indices", hi - lo))
        d = f["decided"][lo:hi]
        assert np.array_equal(out[0][d], f["ref"][lo:hi][d])

    _run(t, gpu, twin, betas, event)
    # the new set: the fp64 index of every second of the first 32 decided positions past the ones inserted above
    roots = np.flatnonzero(f["decided"] & (np.arange(len(f["decided"])) >= 1000))[:B]
    in_file = np.unique(f["ref"][roots[::2]])
    path = tmp_path / "bitvec.bin"
    mm = np.memmap(path, dtype=np.uint8, mode="w+", shape=(1 << 29,))
    for i in in_file.astype(np.uint64):
        mm[int(i) >> 3] |= np.uint8(1 << (int(i) & 7))
    mm.flush()
    del mm
    seen = np.isin(f["ref"][roots], in_file)
    assert 8 <= seen.sum() <= B - 8, seen.sum()
    for net in t.nets:
        net.load_bitset(path)
    os.remove(path)
    for s in (gpu, twin):
        s.set_positions(np.arange(B), f["arr"][roots])
        s.simulate(betas, 1)
    t.check("after load_bitset")
    info, ch = gpu.root_info(), gpu.root_children()
    assert np.all(info["n_children"] > 0)
    want_seen = np.sqrt(np.exp(np.float64(np.float32(c))))
    for g in range(B):
        std = ch["std_dev"][g, :info["n_children"][g]]
        if seen[g]:
            assert np.all(np.isclose(std, want_seen, rtol=1e-6, atol=0)), (g, std[:4], want_seen)
        else:
            assert np.all(std == np.float32(2.0)), (g, std[:4])
    _bytes_equal(ch["std_dev"], twin.root_children()["std_dev"], "std_dev")
    gpu.simulate(betas, 7)
    twin.simulate(betas, 7)
    t.check("seven more")
    t.finish(oracle, 4)
