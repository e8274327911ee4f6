"""tz_search_simulate_batch / tz_search_principal_variation on the device against the CPU restatement of Node::simulate_batch
(tests/simulate_batch_ref.cpp over the oracle's forward / backward primitives).  Every comparison is bit-exact: visit counts, eval
tag and bits, logit / probability / std_dev bits and child order of the root, all its children, every node to depth 2, every node
along the principal variation, and the PV itself.  Each case first asserts that the restatement's event counts show the edge the
case is there for."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import simulate_batch_util as U
from gpu_util import random_positions, require_gpu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref_lib(tmp_path_factory):
    return U.build(tmp_path_factory.mktemp("simulate_batch_ref"))


def _agent_over(net):
    """the restatement's Agent = the HIP network through tz_net_eval, as in tests/test_gpu_engine.py"""
    def fn(user, n_envs, states, legal_idx, legal_count, amax, logits_out, value_out, variance_out):
        rc = net.lib.tz_net_eval(net.h, n_envs, C.cast(states, C.c_void_p), C.cast(legal_idx, C.c_void_p),
                                 C.cast(legal_count, C.c_void_p), amax, C.cast(logits_out, C.c_void_p),
                                 C.cast(value_out, C.c_void_p), C.cast(variance_out, C.c_void_p))
        assert rc == 0, net.lib.tz_last_error()
    return fn


def _counters_match(gpu, ref):
    sims, evals = gpu.counters()
    c = ref.counts()
    assert sims == c["forwards"] and evals == c["leaves"], (sims, evals, c)


# ---- 1. duplicates and fresh roots
@pytest.mark.parametrize("leaves", [1, 2, 7, 64, 128])
@pytest.mark.parametrize("agent", [1, 2], ids=["dummy", "simple"])
def test_duplicate_leaves_and_fresh_roots(ref_lib, agent, leaves):
    A = require_gpu()
    B, n, rounds = 3, 4, 6
    choice = np.array([0, 5, 10], np.int32)
    betas = np.array([0.0, 0.25, 0.5], np.float32)
    ref = U.RefSearch(ref_lib, B, n, 4, agent_kind=agent)
    ref.new_openings(choice)
    ref.simulate_batch(betas, leaves, 1)
    # all `leaves` forwards of round one stop at the fresh root: leaves - 1 repeats per tree (none when a round is one leaf)
    assert ref.counts()["duplicate_leaves"] == B * (leaves - 1), ref.counts()
    ref.simulate_batch(betas, leaves, rounds - 1)
    c = ref.counts()
    assert c["duplicate_leaves"] >= B * (leaves - 1) and (leaves == 1 or c["duplicate_leaves"] > 0), c
    gpu = A.BatchedMCTS(B, n, 4, agent_kind=agent)
    gpu.new_openings(choice)
    gpu.simulate_batch(betas, leaves, rounds)
    assert U.compare(gpu, ref, "leaves=%d" % leaves) > 10
    _counters_match(gpu, ref)


# ---- 2. Known results inside a round, the solver, short rounds
def test_known_results_inside_a_round_and_short_rounds(oracle, ref_lib):
    A = require_gpu()
    n, leaves = 3, 16
    s = O.state_default(oracle, n, 0)
    for mv in "a3 c1 c2 c3 b3 c3-".split():        # the start of the reference's find_tinue_easy, mcts.rs:352
        s = O.play(oracle, s, O.from_ptn(oracle, n, mv))
    starts = [s] + random_positions(oracle, O, n, 0, 2, seed=11, min_ply=6, max_ply=10)
    B = len(starts)
    betas = np.zeros(B, np.float32)
    ref = U.RefSearch(ref_lib, B, n, 0, agent_kind=2)
    ref.set_positions(np.arange(B), starts)
    rounds = 0
    while not any(ref.node(g, [])[0]["eval_tag"] != 0 for g in range(B)):      # until the first root is solved
        ref.simulate_batch(betas, leaves, 1)
        rounds += 1
        assert rounds < 400
    c = ref.counts()
    assert c["known_in_round"] > 0 and c["short_rounds"] > 0, c
    gpu = A.BatchedMCTS(B, n, 0, agent_kind=A.AGENT_SIMPLE)
    gpu.set_positions(np.arange(B), O.states_array(starts))
    gpu.simulate_batch(betas, leaves, rounds)
    assert U.compare(gpu, ref, "solver") > 10
    _counters_match(gpu, ref)


# ---- 3. no leaf at all
def _finished_position(oracle, n, half_komi, seed):
    rng = np.random.default_rng(seed)
    s = O.state_default(oracle, n, half_komi)
    while oracle.tzo_terminal(C.byref(s)) == -1:
        mv = O.possible_moves(oracle, s)
        s = O.play(oracle, s, mv[int(rng.integers(len(mv)))])
    return s


def test_a_tree_whose_root_is_terminal_collects_nothing(oracle, ref_lib):
    A = require_gpu()
    n, leaves, rounds = 4, 8, 3
    starts = [_finished_position(oracle, n, 4, 5), random_positions(oracle, O, n, 4, 1, seed=6, min_ply=4, max_ply=8)[0]]
    betas = np.zeros(2, np.float32)
    ref = U.RefSearch(ref_lib, 2, n, 4, agent_kind=2)
    ref.set_positions(np.arange(2), starts)
    gpu = A.BatchedMCTS(2, n, 4, agent_kind=A.AGENT_SIMPLE)
    gpu.set_positions(np.arange(2), O.states_array(starts))
    for r in range(rounds):
        ref.simulate_batch(betas, leaves, 1)
        gpu.simulate_batch(betas, leaves, 1)
        info = gpu.root_info()
        assert info["visit_count"][0] == 4 * leaves * (r + 1) and info["n_children"][0] == 0, info[0]
    assert ref.counts()["short_rounds"] >= rounds
    assert U.compare(gpu, ref, "terminal root beside a live one") > 5
    _counters_match(gpu, ref)


def test_a_round_without_any_leaf_makes_no_network_call(oracle):
    A = require_gpu()
    from takzero_amd import weights as W

    n, leaves = 4, 8
    net = A.Net(arch=A.ARCH_TEST, n=n, precision=A.PREC_F16, blocks=1).load_tensors(W.init_weights(W.ARCH_TEST, n=n, blocks=1, seed=7))
    gpu = A.BatchedMCTS(1, n, 4, agent=net, node_capacity=1 << 10)
    gpu.set_positions([0], O.states_array([_finished_position(oracle, n, 4, 5)]))
    before = gpu.counters()
    gpu.simulate_batch(np.zeros(1, np.float32), leaves, 2)        # raises unless TZ_OK
    after = gpu.counters()
    assert after[1] == before[1] and after[0] - before[0] == 2 * 4 * leaves, (before, after)
    info = gpu.root_info()
    assert info["visit_count"][0] == 2 * 4 * leaves and info["n_children"][0] == 0 and info["eval_tag"][0] != 0
    assert len(gpu.principal_variation(0)) == 0


# ---- 4. a real net in the reference's shape, and 5. subtree reuse after it
def _net(A, arch, precision):
    from takzero_amd import weights as W

    if arch == A.ARCH_NET5:
        return A.Net.new(arch=A.ARCH_NET5, seed=3, precision=precision)
    return A.Net(arch=A.ARCH_TEST, n=5, precision=precision, blocks=2).load_tensors(W.init_weights(W.ARCH_TEST, n=5, blocks=2, seed=123))


@pytest.mark.parametrize("arch,precision,B,leaves", [("test", "f32", 1, 128), ("test", "f32", 5, 32), ("test", "f16", 1, 128),
                                                     ("test", "f16", 5, 32), ("net5", "f16", 1, 128)])
def test_real_net_in_the_reference_shape_then_reuse(ref_lib, arch, precision, B, leaves):
    A = require_gpu()
    net = _net(A, A.ARCH_NET5 if arch == "net5" else A.ARCH_TEST, A.PREC_F32 if precision == "f32" else A.PREC_F16)
    rounds = 8
    choice = (np.arange(B) * 3 + 1).astype(np.int32) % 16
    betas = np.where(np.arange(B) % 2 == 0, 0.0, 0.25).astype(np.float32)
    ref = U.RefSearch(ref_lib, B, 5, 4, agent_kind=0, agent_fn=_agent_over(net))
    ref.new_openings(choice)
    ref.simulate_batch(betas, leaves, rounds)
    c = ref.counts()
    assert c["leaves"] == B * leaves * rounds and c["duplicate_leaves"] >= B * (leaves - 1), c
    gpu = A.BatchedMCTS(B, 5, 4, agent=net)
    gpu.new_openings(choice)
    gpu.simulate_batch(betas, leaves, rounds)
    assert U.compare(gpu, ref, "net") > 20
    _counters_match(gpu, ref)
    # reuse: tz_search_step with the PV's first move (the restatement calls descend and env.step), then 4 more rounds
    first = np.array([ref.principal_variation(g)[0] for g in range(B)], np.uint16)
    ref.step(first)
    gpu.step(first)
    assert min(int(ref.node(g, [])[0]["visit_count"]) for g in range(B)) > 0      # a kept subtree, not a fresh root
    ref.simulate_batch(betas, leaves, 4)
    gpu.simulate_batch(betas, leaves, 4)
    assert U.compare(gpu, ref, "net, after step") > 20
    _counters_match(gpu, ref)


# ---- 6. capacity
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "lenient"])
def test_a_pool_that_fills_in_round_three(ref_lib, monkeypatch, strict):
    A = require_gpu()
    n, leaves = 4, 16
    choice = np.array([2], np.int32)
    betas = np.zeros(1, np.float32)
    ref = U.RefSearch(ref_lib, 1, n, 4, agent_kind=2)
    ref.new_openings(choice)
    ref.simulate_batch(betas, leaves, 2)
    after_two = ref.tree_size(0)
    ref.simulate_batch(betas, leaves, 1)
    after_three = ref.tree_size(0)
    assert after_three > after_two + 2
    capacity = (after_two + after_three) // 2          # rounds one and two fit; round three does not
    ref.simulate_batch(betas, leaves, 1)
    assert ref.counts()["known_in_round"] == 0          # so every round makes exactly `leaves` forwards, on any tree
    if strict:
        monkeypatch.setenv("TZ_STRICT_CAPACITY", "1")
    else:
        monkeypatch.delenv("TZ_STRICT_CAPACITY", raising=False)
    gpu = A.BatchedMCTS(1, n, 4, agent_kind=A.AGENT_SIMPLE, node_capacity=capacity)
    gpu.new_openings(choice)
    gpu.simulate_batch(betas, leaves, 2)
    assert gpu.pool_overflows() == 0 and gpu.pool_usage()[0] == after_two
    if strict:
        with pytest.raises(A._lib.TakzeroError) as e:
            gpu.simulate_batch(betas, leaves, 1)
        assert e.value.code == -5           # TZ_ECAPACITY
        return
    gpu.simulate_batch(betas, leaves, 2)                # TZ_OK
    assert gpu.pool_overflows() > 0
    assert gpu.root_info()["visit_count"][0] == (2 + 2) * leaves == gpu.counters()[0]      # the forwards of four rounds


# ---- 7. arguments
def test_argument_errors():
    A = require_gpu()
    lib = A._lib.load()
    gpu = A.BatchedMCTS(2, 4, 4, agent_kind=A.AGENT_DUMMY, node_capacity=1 << 10)
    wide = A.BatchedMCTS(128, 4, 4, agent_kind=A.AGENT_DUMMY, node_capacity=1 << 8)
    betas = np.zeros(128, np.float32)
    bound = 16384                                       # TZ_SIMULATE_BATCH_MAX_SLOTS
    EINVAL = -1
    assert lib.tz_search_simulate_batch(gpu.h, betas.ctypes.data, 0, 1) == EINVAL
    assert lib.tz_search_simulate_batch(gpu.h, betas.ctypes.data, -3, 1) == EINVAL
    assert lib.tz_search_simulate_batch(gpu.h, betas.ctypes.data, 4, -1) == EINVAL
    assert lib.tz_search_simulate_batch(gpu.h, None, 4, 1) == EINVAL
    assert lib.tz_search_simulate_batch(None, betas.ctypes.data, 4, 1) == EINVAL
    assert lib.tz_search_simulate_batch(gpu.h, betas.ctypes.data, bound // 2 + 1, 1) == EINVAL
    assert lib.tz_search_simulate_batch(wide.h, betas.ctypes.data, bound // 128 + 1, 1) == EINVAL
    assert gpu.counters() == (0, 0) and wide.counters() == (0, 0)
    assert lib.tz_search_simulate_batch(gpu.h, betas.ctypes.data, 4, 0) == 0           # no rounds: nothing happens
    assert gpu.root_info()["visit_count"].tolist() == [0, 0]
    assert lib.tz_search_simulate_batch(wide.h, betas.ctypes.data, 32, 1) == 0         # 128 x 32 is within the bound
    one = A.BatchedMCTS(1, 4, 4, agent_kind=A.AGENT_DUMMY, node_capacity=1 << 12)
    assert lib.tz_search_simulate_batch(one.h, betas.ctypes.data, 1024, 1) == 0        # and so is 1 x 1024
    assert one.root_info()["visit_count"][0] == 1024
    moves, n = np.zeros(8, np.uint16), C.c_int(-1)
    assert lib.tz_search_principal_variation(None, 0, moves.ctypes.data, 8, C.byref(n)) == EINVAL
    assert lib.tz_search_principal_variation(gpu.h, 2, moves.ctypes.data, 8, C.byref(n)) == EINVAL
    assert lib.tz_search_principal_variation(gpu.h, -1, moves.ctypes.data, 8, C.byref(n)) == EINVAL
    assert lib.tz_search_principal_variation(gpu.h, 0, None, 8, C.byref(n)) == EINVAL
    assert lib.tz_search_principal_variation(gpu.h, 0, moves.ctypes.data, -1, C.byref(n)) == EINVAL
    assert lib.tz_search_principal_variation(gpu.h, 0, moves.ctypes.data, 8, None) == EINVAL
    # len_out is the whole length even when cap is smaller
    assert lib.tz_search_principal_variation(one.h, 0, None, 0, C.byref(n)) == 0 and n.value == len(one.principal_variation(0)) >= 1


# ---- 8. the example program
def test_analysis_cli_prints_what_the_api_gives(oracle, tmp_path):
    A = require_gpu()
    from takzero_amd import _lib
    from takzero_amd import weights as W

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "analysis_cli")       # built as tests/test_gpu_native_driver.py builds the other examples
    r = subprocess.run(["g++", "-std=c++17", "-O2", os.path.join(root, "examples", "analysis_cli.cpp"), "-I" + os.path.join(root, "include"),
                        "-L" + os.path.dirname(_lib.LIB_PATH), "-ltakzero_hip", "-Wl,-rpath," + os.path.dirname(_lib.LIB_PATH), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-1500:]
    tensors = W.init_weights(W.ARCH_TEST, n=5, blocks=1, seed=21)
    model = os.path.join(str(tmp_path), "random.tzw")
    W.save_tzw(model, tensors)
    start = random_positions(oracle, O, 5, 4, 1, seed=9, min_ply=6, max_ply=12)[0]
    tps = O.to_tps(oracle, start)
    leaves, rounds = 32, 4
    r = subprocess.run([exe, "--tps", tps, "--model", model, "--arch", "100", "--n", "5", "--blocks", "1", "--leaves", str(leaves),
                        "--rounds", str(rounds)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr[-1500:])
    lines = dict(l.split(":", 1) for l in r.stdout.splitlines() if not l.startswith("child:"))
    net = A.Net(arch=A.ARCH_TEST, n=5, precision=A.PREC_F16, blocks=1).load_tensors(tensors)
    gpu = A.BatchedMCTS(1, 5, 4, agent=net)
    gpu.set_positions([0], O.states_array([start]))
    gpu.simulate_batch(np.zeros(1, np.float32), leaves, rounds)
    assert lines["tps"].strip() == tps
    assert int(lines["visits"]) == int(gpu.root_info()["visit_count"][0]) >= leaves * rounds
    pv = [O.ptn(oracle, 5, int(m)) for m in gpu.principal_variation(0)]
    assert lines["pv"].split() == pv and len(pv) >= 1
    shown = [l.split() for l in r.stdout.splitlines() if l.startswith("child:")]
    visits = [int(f[3]) for f in shown]
    ch = gpu.root_children()
    by_move = {O.ptn(oracle, 5, int(m)): int(v) for m, v in zip(ch["move_idx"][0], ch["visits"][0])}
    assert visits == sorted(by_move.values(), reverse=True)[:len(shown)] and all(by_move[f[1]] == int(f[3]) for f in shown)
