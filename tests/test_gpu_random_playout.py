"""tz_search_random_steps, tz_search_hash_seen / tz_net_hash_seen, takzero_amd.eee and examples/seen_ratio_cli.cpp on the device
against the CPU reference of tests/random_playout_ref.py (the playout written from its definition over the oracle's rules).

Playouts are compared byte for byte: moves, legal-move counts, played, and every byte of the final tz_state of get_positions()."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import capacity_positions as CP
import edge_positions as E
import oracle_lib as O
import random_playout_ref as R
from gpu_util import require_gpu
from test_gpu_tree import assert_same_roots

pytestmark = pytest.mark.gpu

HK = {3: 0, 4: 4, 5: 4, 6: 4}
LOCKED_3X3 = "1S,2S,1S/2S,1S,2S/1S,2S,1S 2 10"


def _handle(A, states, n, capacity=64):
    m = A.BatchedMCTS(len(states), n, HK[n], agent_kind=A.AGENT_DUMMY, node_capacity=capacity)
    m.set_positions(np.arange(len(states)), O.states_array(states))
    return m


def _same(got, ref, where):
    for name, a, b in zip(("moves", "nlegal", "played", "positions"), got, ref):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.dtype.itemsize == b.dtype.itemsize and a.shape == b.shape, (where, name, a.dtype, b.dtype, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            bad = np.nonzero(np.frombuffer(a.tobytes(), np.uint8) != np.frombuffer(b.tobytes(), np.uint8))[0]
            raise AssertionError((where, name, "first differing byte", int(bad[0]), "of", a.nbytes))


def _check(A, oracle, n, states, seed, base, steps, flag, where):
    m = _handle(A, states, n)
    moves, nlegal, played = m.random_steps(steps, seed, game_base=base, stop_at_terminal=flag)
    ref = R.playout_batch(oracle, states, seed, base, steps, flag)
    assert not ref[4]
    _same((moves, nlegal, played, m.get_positions()), ref[:4], where)
    return played, ref


def _openings(oracle, n, count):
    return [R.opening(oracle, n, HK[n], g % 16) for g in range(count)]


@pytest.mark.parametrize("n,games,steps,flag", [(3, 64, 40, False), (3, 64, 40, True), (4, 64, 60, False), (5, 33, 150, False),
                                                (6, 16, 150, False), (4, 1, 60, True), (5, 1, 30, False)])
def test_playouts_from_the_openings_equal_the_reference(oracle, n, games, steps, flag):
    A = require_gpu()
    played, _ = _check(A, oracle, n, _openings(oracle, n, games), 123, 0, steps, flag, (n, games, steps, flag))
    if n == 3 and games == 64:
        assert played.min() < steps     # 3x3: games end (flag) or run out of moves (no flag) well within 40 plies


def test_zero_steps_change_nothing_and_bad_arguments_are_refused(oracle):
    A = require_gpu()
    states = _openings(oracle, 4, 8)
    m = _handle(A, states, 4)
    m.simulate(np.zeros(8, np.float32), 4)
    before = m.root_info().tobytes()
    moves, nlegal, played = m.random_steps(0, 5)
    assert moves.shape == (8, 0) and nlegal.shape == (8, 0) and not played.any()
    assert m.get_positions().tobytes() == O.states_array(states).tobytes() and m.root_info().tobytes() == before   # trees kept too
    lib = m.lib
    assert lib.tz_search_random_steps(m.h, 1, 0, -1, 0, None, None, None) == -1
    assert lib.tz_search_random_steps(m.h, 1, 0, 3, 2, None, None, None) == -1
    assert lib.tz_search_random_steps(None, 1, 0, 3, 0, None, None, None) == -1
    assert lib.tz_search_random_steps(m.h, 1, 0, 3, 0, None, None, None) == 0        # every output may be NULL
    assert m.get_positions().tobytes() == R.playout_batch(oracle, states, 1, 0, 3)[3].tobytes()


def test_game_base_beyond_32_bits(oracle):
    A = require_gpu()
    states = _openings(oracle, 4, 16)
    _, ref = _check(A, oracle, 4, states, 9, 2**40 + 5, 20, False, "2^40 + 5")
    assert ref[0].tobytes() != R.playout_batch(oracle, states, 9, 5, 20)[0].tobytes()     # the high bits take part in the key


def test_split_invariance_on_the_device(oracle):
    A = require_gpu()
    states = _openings(oracle, 3, 64)
    one = _handle(A, states, 3)
    m1, n1, p1 = one.random_steps(40, 7, game_base=100)
    two = _handle(A, states, 3)
    ma, na, pa = two.random_steps(10, 7, game_base=100)
    mb, nb, pb = two.random_steps(30, 7, game_base=100)
    assert one.get_positions().tobytes() == two.get_positions().tobytes()
    assert np.array_equal(p1, pa + pb) and pb[pa < 10].max(initial=0) == 0
    for g in range(64):
        assert np.array_equal(m1[g, :p1[g]], np.concatenate([ma[g, :pa[g]], mb[g, :pb[g]]]))
        assert np.array_equal(n1[g, :p1[g]], np.concatenate([na[g, :pa[g]], nb[g, :pb[g]]]))


@pytest.mark.parametrize("n", [3, 4, 5, 6])
@pytest.mark.parametrize("flag", [False, True])
def test_edge_positions(oracle, n, flag):
    """empty reserves, full boards, stacks past bit 32, the 100-ply draw counter, finished games; on 3x3 also the locked board"""
    A = require_gpu()
    states = [s for _, s in E.fixture(oracle, n).positions]
    if n == 3:
        states.append(O.state_from_tps(oracle, LOCKED_3X3, 3, HK[3]))
    terminal = np.array([oracle.tzo_terminal(C.byref(s)) != -1 for s in states])
    assert terminal.any() and not terminal.all()
    played, _ = _check(A, oracle, n, states, 31, 1000, 8, flag, (n, flag))
    if flag:
        assert not played[terminal].any()
    else:
        assert played[terminal].any()          # random moves go on over a finished game
    if n == 3:
        assert played[-1] == 0


def _raw_random_steps(m, seed, base, steps, flags=0):
    B = m.batch
    moves, nlegal, played = np.zeros((B, steps), np.uint16), np.zeros((B, steps), np.uint16), np.full(B, -7, np.int32)
    rc = m.lib.tz_search_random_steps(m.h, seed, base, steps, flags, moves.ctypes.data, nlegal.ctypes.data, played.ctypes.data)
    return rc, moves, nlegal, played


def test_capacity_edge_on_6x6(oracle):
    A = require_gpu()
    cap, = CP.labelled(oracle, 6, "cap")
    assert len(O.possible_moves(oracle, cap)) == R.ROW
    # exactly 1024 legal moves: plays on
    _check(A, oracle, 6, [cap, R.opening(oracle, 6, 4, 3)], 5, 0, 6, False, "cap")
    # more: the game stays where it is, the others finish, the call reports it, the next call works
    over = CP.labelled(oracle, 6, "over/near", "over/far")
    assert len(over) == 2 and all(len(O.possible_moves(oracle, s)) > R.ROW for s in over)
    states = [R.opening(oracle, 6, 4, 1), over[0], cap, over[1], R.opening(oracle, 6, 4, 6)]
    m = _handle(A, states, 6)
    rc, moves, nlegal, played = _raw_random_steps(m, 5, 40, 6)
    assert rc == -5 and "more legal moves than max_actions" in m.lib.tz_last_error().decode()
    ref = R.playout_batch(oracle, states, 5, 40, 6)
    assert ref[4] and played[1] == 0 and played[3] == 0
    _same((moves, nlegal, played, m.get_positions()), ref[:4], "over")
    good = [0, 2, 4]
    m.set_positions([1, 3], O.states_array([states[0], states[4]]))
    now = R.as_tzstates(m.get_positions())
    rc, moves, nlegal, played = _raw_random_steps(m, 6, 0, 4)
    assert rc == 0 and played[good].min() > 0
    _same((moves, nlegal, played, m.get_positions()), R.playout_batch(oracle, now, 6, 0, 4)[:4], "after")


def test_tree_is_reset_and_the_handle_searches_like_a_fresh_one(oracle):
    A = require_gpu()
    n, B = 5, 16
    states = _openings(oracle, n, B)
    gpu = _handle(A, states, n, capacity=4096)
    betas = np.zeros(B, np.float32)
    gpu.simulate(betas, 8)                       # a tree to forget
    gpu.random_steps(12, 3)
    info = gpu.root_info()
    assert not info["visit_count"].any() and not info["n_children"].any() and gpu.pool_usage()[0] == 1
    ora = O.OracleSearch(oracle, B, n, HK[n], agent_kind=1)
    ora.set_positions(np.arange(B), R.playout_batch(oracle, states, 3, 0, 12)[3])
    gpu.simulate(betas, 32)
    ora.simulate(betas, 32)
    assert_same_roots(gpu, ora, "after random_steps")
    assert np.array_equal(gpu.select_best_actions(), ora.select_best_actions())


def test_captured_graph_survives_random_steps(oracle, monkeypatch):
    """simulate (captured from the third simulation on), random_steps, simulate: equal to a twin created under TZ_NO_GRAPH=1"""
    A = require_gpu()
    n, B = 4, 16
    states = _openings(oracle, n, B)
    monkeypatch.delenv("TZ_NO_GRAPH", raising=False)
    gpu = _handle(A, states, n, capacity=4096)
    monkeypatch.setenv("TZ_NO_GRAPH", "1")
    twin = _handle(A, states, n, capacity=4096)
    monkeypatch.delenv("TZ_NO_GRAPH")
    betas = np.zeros(B, np.float32)
    for m in (gpu, twin):
        m.simulate(betas, 8)
        m.random_steps(5, 21, game_base=3)
        m.simulate(betas, 8)
    assert gpu.get_positions().tobytes() == twin.get_positions().tobytes()
    assert_same_roots(gpu, twin, "graph against eager")
    ora = O.OracleSearch(oracle, B, n, HK[n], agent_kind=1)
    ora.set_positions(np.arange(B), R.playout_batch(oracle, states, 21, 3, 5)[3])
    ora.simulate(betas, 8)
    assert_same_roots(gpu, ora, "graph against the oracle")


HASH_NETS = ["net4_lcghash", "net4_simhash", "net6_simhash"]


def _hash_net(A, name, seed=11):
    return A.Net.new(arch={"net4_lcghash": A.ARCH_NET4_LCGHASH, "net4_simhash": A.ARCH_NET4_SIMHASH, "net6_simhash": A.ARCH_NET6_SIMHASH}[name],
                     seed=seed, precision=A.PREC_F16)


@pytest.mark.parametrize("name", HASH_NETS)
def test_hash_seen_and_forward_hash(oracle, name):
    A = require_gpu()
    net = _hash_net(A, name)
    n, B = net.n, 48
    fed = R.reference_envs(oracle, n, HK[n], B, 6, B, 1)
    fresh = R.reference_envs(oracle, n, HK[n], B, 9, B, 2)
    assert not net.hash_seen(fed).any()                             # an empty set
    fed_idx = net.hash_indices(fed, update=True)
    assert np.array_equal(net.hash_indices(fed, update=False), fed_idx)
    members = set(int(i) for i in fed_idx)
    both = np.concatenate([fed, fresh])
    idx = net.hash_indices(both, update=False)
    want = np.array([int(i) in members for i in idx], np.uint8)
    seen = net.hash_seen(both)
    assert seen.dtype == np.uint8 and np.array_equal(seen, want)
    assert seen[:B].all()                                           # what was fed is seen
    assert np.array_equal(seen[B:] != 0, np.isin(idx[B:], fed_idx))   # fresh ones only where their index collides
    fh = net.forward_hash(both)
    assert fh.dtype == np.float32 and np.array_equal(fh, np.where(want != 0, np.float32(0.0), np.float32(4.0)))
    assert np.array_equal(net.hash_indices(both, update=False), idx)    # a lookup sets nothing
    assert np.array_equal(net.hash_seen(fresh), want[B:])
    # the handle's positions, without an upload
    m = A.BatchedMCTS(2 * B, n, HK[n], agent=net, node_capacity=8)
    m.set_positions(np.arange(2 * B), both)
    assert np.array_equal(m.hash_seen(), want)
    m.random_steps(3, 5)
    assert np.array_equal(m.hash_seen(), net.hash_seen(m.get_positions()))


def test_hash_seen_refuses_other_agents(oracle):
    A = require_gpu()
    dummy = A.BatchedMCTS(4, 4, 4, agent_kind=A.AGENT_DUMMY, node_capacity=8)
    out = np.zeros(4, np.uint8)
    assert dummy.lib.tz_search_hash_seen(dummy.h, out.ctypes.data) == -1
    from takzero_amd import weights as W
    net5 = A.Net(arch=A.ARCH_TEST, n=5, blocks=1).load_tensors(W.init_weights(W.ARCH_TEST, n=5, blocks=1, seed=1))
    m = A.BatchedMCTS(4, 5, 4, agent=net5, node_capacity=8)
    assert m.lib.tz_search_hash_seen(m.h, out.ctypes.data) == -1
    st = m.get_positions()
    assert m.lib.tz_net_hash_seen(net5.h, 4, st.ctypes.data, out.ctypes.data) == -1
    with pytest.raises(A.TakzeroError):
        m.hash_seen()


def _cpu_seen_ratio(oracle, net, n, plies, games, seed):
    out = []
    for ply in plies:
        pos = R.reference_envs(oracle, n, HK[n], 0, ply, games, seed, first_game=ply * games)
        unseen = int((net.hash_seen(pos) == 0).sum())
        out.append((ply, float(np.float32(unseen / games))))
    return out


def test_seen_ratio_and_its_cli(oracle, tmp_path):
    """eee.seen_ratio at 4 plies x 256 games on a 64-game handle, and seen_ratio_cli on the saved net, against the CPU reference's
    positions and the set built here from hash_indices"""
    A = require_gpu()
    from takzero_amd import eee
    net = _hash_net(A, "net4_lcghash", seed=5)
    n, games, plies, seed = 4, 256, range(4), 123
    # mark half of the positions the experiment will meet, so that the ratios are neither 0 nor 1
    for ply in plies:
        pos = R.reference_envs(oracle, n, HK[n], 0, ply, games, seed, first_game=ply * games)
        net.hash_indices(pos[::2], update=True)
    want = _cpu_seen_ratio(oracle, net, n, plies, games, seed)
    assert any(0.0 < r < 1.0 for _, r in want), want
    m = A.BatchedMCTS(64, n, HK[n], agent=net, node_capacity=1)
    envs = eee.reference_envs(m, 3, 100, seed, game_base=3 * games)           # 100: a last wave that is not full
    assert envs.tobytes() == R.reference_envs(oracle, n, HK[n], 64, 3, 100, seed, first_game=3 * games).tobytes()
    got = eee.seen_ratio(m, plies=plies, games=games, seed=seed)
    assert got == want, (got, want)
    # the program
    model = str(tmp_path / "model.ot")
    net.save(model)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "seen_ratio_cli")
    r = subprocess.run(["g++", "-std=c++17", "-O2", os.path.join(root, "examples", "seen_ratio_cli.cpp"), "-I" + os.path.join(root, "include"),
                        "-L" + os.path.join(root, "takzero_amd"), "-ltakzero_hip", "-Wl,-rpath," + os.path.join(root, "takzero_amd"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe, "--model", model, "--arch", "net4_lcghash", "--games", str(games), "--plies", "4", "--batch", "64", "--seed", str(seed)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().split("\n")
    assert lines[0] == "random = [" and lines[-1] == "]" and len(lines) == 6, r.stdout
    rows = [re.fullmatch(r"    \((\d+), ([0-9.e+-]+)\),", ln) for ln in lines[1:-1]]
    assert all(rows), r.stdout
    assert [(int(x.group(1)), float(np.float32(float(x.group(2))))) for x in rows] == want
