"""The device searches and the Agent surface at the edge of max_actions, a handle's widest child list (64 / 192 / 512 / 1024 on
3x3 .. 6x6; tests/capacity_positions.py has the positions, tests/test_capacity_positions.py their move counts on the CPU).

At the cap (nact == max_actions and max_actions - 1) everything is held to the CPU references bit for bit: lock-step simulate under
the three selection rules, simulate_batch, Gumbel halving, the root-side calls with rows max_actions wide, a real net in the loop.
The wide games sit at game 0, in the middle and at B - 1, ordinary positions between them: leaf_act and the leaf-batch rows of
neighbouring games are adjacent in memory and game B - 1 is the last row of its allocation, so a row written one entry too far shows
in the neighbour or nowhere - hence both `cap` and `cap-1`, and every byte of the neighbours.

Beyond the cap the contract of include/takzero_hip.h (tz_search_shape) is held sentence by sentence: TZ_ECAPACITY naming
max_actions, the over-wide node never expanded, the other games equal to the oracle's run without that game, the handle as good as a
fresh one once set_positions has replaced the game.  The Agent surface (tz_net_eval takes its own amax) has no such limit and is run
on every fixture position, 1144 legal moves included.  Nothing here has a tolerance."""
import ctypes as C

import numpy as np
import pytest

import capacity_positions as P
import exact_net as E
import oracle_lib as O
import selection_util as S
import simulate_batch_util as U
from gpu_util import random_positions, require_gpu
from test_gpu_engine import _agent_over
from test_gpu_tree import assert_same_roots

pytestmark = pytest.mark.gpu
SIZES = (3, 4, 5, 6)
B = 8
MIDDLE = 3
WIDE = (0, MIDDLE, MIDDLE + 1, B - 1)                   # cap, cap-1, cap-1, cap; betas 0, 0, 0.5, 0.5
SIMS = 48
POOL = {3: 1 << 13, 4: 1 << 15, 5: 1 << 17, 6: 1 << 18}
POOL_BATCH = {3: 1 << 14, 4: 1 << 16, 5: 1 << 18, 6: 1 << 20}      # 64 leaves a round, most of them new nodes with ~cap children
ECAPACITY = -5
FIELDS = ("move_idx", "visits", "eval_tag", "eval_bits", "logit", "prob", "std_dev")
PRECS = {"bf16": 0, "f32": 1, "f16": 2, "f16x2": 3, "f16c8": 4, "f16c6": 5}
NET_CASES = [(n, p) for n in SIZES for p in PRECS if p != "f16c6" or n in (5, 6)]
_cache = {}


class Ora(O.OracleSearch):
    """OracleSearch whose node() returns up to 1024 children by default, as BatchedMCTS.node does on 6x6"""

    def node(self, game, path, amax=1024):
        return super().node(game, path, amax)


@pytest.fixture(scope="module")
def sel_lib(tmp_path_factory):
    return S.build(tmp_path_factory.mktemp("capacity_selection_ref"))


@pytest.fixture(scope="module")
def batch_lib(tmp_path_factory):
    return U.build(tmp_path_factory.mktemp("capacity_simulate_batch_ref"))


def fill(oracle, n, count=B, seed=0):
    """ordinary positions: early random playouts, far below the cap"""
    key = ("fill", n, count, seed)
    if key not in _cache:
        _cache[key] = random_positions(oracle, O, n, P.HALF_KOMI[n], count, 50 + n + seed, min_ply=4, max_ply=20)
    return _cache[key]


def cap_batch(oracle, n):
    """B positions with `cap` at game 0 and B - 1 and `cap-1` at the two middle games; betas 0 in the first half, 0.5 in the second"""
    cap, under = P.labelled(oracle, n, "cap")[0], P.labelled(oracle, n, "cap-1")[0]
    states = list(fill(oracle, n))
    for g, s in zip(WIDE, (cap, under, under, cap)):
        states[g] = s
    return states, np.where(np.arange(B) < B // 2, 0.0, 0.5).astype(np.float32)


def over_batch(oracle, n, label, index):
    states = list(fill(oracle, n))
    states[index] = P.labelled(oracle, n, label)[0]
    return states, np.where(np.arange(B) % 2 == 0, 0.0, 0.5).astype(np.float32)


def start(search, states):
    search.set_positions(np.arange(len(states)), O.states_array(states) if not isinstance(search, O.OracleSearch) else states)


def widths_at_the_cap(gpu, n):
    nc = gpu.root_info()["n_children"]
    assert [int(nc[g]) for g in WIDE] == [P.CAPS[n], P.CAPS[n] - 1, P.CAPS[n] - 1, P.CAPS[n]], nc


@pytest.mark.parametrize("n", SIZES)
def test_the_caps_are_the_ones_the_fixture_assumes(n):
    A = require_gpu()
    gpu = A.BatchedMCTS(2, n, P.HALF_KOMI[n], agent_kind=A.AGENT_DUMMY, node_capacity=256)
    out = [C.c_int(-1) for _ in range(4)]
    A.check(gpu.lib.tz_search_shape(gpu.h, *[C.byref(v) for v in out]))
    assert [v.value for v in out] == [2, n, P.HALF_KOMI[n], P.CAPS[n]]
    gpu.close()


# ---------------------------------------------------------------------------------------------- 2. at the cap
@pytest.mark.parametrize("rule", (S.PUCT, S.UCT, S.IMPROVED), ids=("puct", "uct", "improved"))
@pytest.mark.parametrize("agent", (1, 2), ids=("dummy", "simple"))
@pytest.mark.parametrize("n", SIZES)
def test_lock_step_at_the_cap(oracle, sel_lib, n, agent, rule):
    """48 lock-step simulations: gen_moves fills leaf_act rows to their last and last but one entry, expand_kernel's lg / ex rows and
    (improved) the SelectRow are as long as they get; roots, all root children, the nodes to depth 2 below the wide roots and the most
    visited lines against the restatement of the rule, and under PUCT the oracle's own search as well."""
    A = require_gpu()
    states, betas = cap_batch(oracle, n)
    ref = S.RefSearch(sel_lib, B, n, P.HALF_KOMI[n], agent_kind=agent, rule=rule)
    gpu = A.BatchedMCTS(B, n, P.HALF_KOMI[n], agent_kind=agent, node_capacity=POOL[n])
    gpu.set_selection(rule)
    ref.set_positions(np.arange(B), states)
    start(gpu, states)
    ref.simulate(betas, SIMS)
    gpu.simulate(betas, SIMS)
    widths_at_the_cap(gpu, n)
    assert S.compare(gpu, ref, "lock-step") > 2 * P.CAPS[n]
    assert U.compare(gpu, ref, "lock-step", deep=WIDE) > 2 * P.CAPS[n]
    if rule == S.PUCT:
        ora = Ora(oracle, B, n, P.HALF_KOMI[n], agent_kind=agent)
        start(ora, states)
        ora.simulate(betas, SIMS)
        assert_same_roots(gpu, ora, "lock-step")
        assert np.array_equal(gpu.select_best_actions(), ora.select_best_actions())
        assert gpu.counters() == ora.counters()
        ora.close()
    assert gpu.pool_overflows() == 0 and not ref.nan_seen()
    gpu.close()
    ref.close()


@pytest.mark.parametrize("leaves", (1, 7, 64))
@pytest.mark.parametrize("agent", (1, 2), ids=("dummy", "simple"))
@pytest.mark.parametrize("n", SIZES)
def test_simulate_batch_at_the_cap(oracle, batch_lib, n, agent, leaves):
    """6 rounds: the act / logit / prob rows of every leaf slot are max_actions long, slot (B - 1, leaves - 1) the last of its allocation"""
    A = require_gpu()
    states, betas = cap_batch(oracle, n)
    ref = U.RefSearch(batch_lib, B, n, P.HALF_KOMI[n], agent_kind=agent)
    gpu = A.BatchedMCTS(B, n, P.HALF_KOMI[n], agent_kind=agent, node_capacity=POOL_BATCH[n])
    ref.set_positions(np.arange(B), states)
    start(gpu, states)
    ref.simulate_batch(betas, leaves, 6)
    gpu.simulate_batch(betas, leaves, 6)
    widths_at_the_cap(gpu, n)
    assert U.compare(gpu, ref, "leaves=%d" % leaves, deep=WIDE) > 2 * P.CAPS[n]
    sims, evals = gpu.counters()
    c = ref.counts()
    assert sims == c["forwards"] and evals == c["leaves"], (sims, evals, c)
    assert gpu.pool_overflows() == 0
    gpu.close()
    ref.close()


@pytest.mark.parametrize("n", (4, 5))
def test_a_solved_wide_root_answers_with_a_best_child_beyond_its_first_64(oracle, batch_lib, n):
    """After six rounds of seven leaves (Dummy agent) the wide roots are proven wins and the one lost child, the first minimum of
    Node::select_best_action, is child 163 of 192 or 511 of 512: a lane of select_best_child meets it in its third or eighth
    iteration.  tz_search_select_best_actions and tz_search_principal_variation have to answer with its move."""
    A = require_gpu()
    states, betas = cap_batch(oracle, n)
    ref = U.RefSearch(batch_lib, B, n, P.HALF_KOMI[n], agent_kind=1)
    gpu = A.BatchedMCTS(B, n, P.HALF_KOMI[n], agent_kind=A.AGENT_DUMMY, node_capacity=POOL_BATCH[n])
    ref.set_positions(np.arange(B), states)
    start(gpu, states)
    ref.simulate_batch(betas, 7, 6)
    gpu.simulate_batch(betas, 7, 6)
    best = gpu.select_best_actions()
    for g in WIDE:
        info, ch = ref.node(g, [])
        lost = np.flatnonzero(ch["eval_tag"] == A.EVAL_LOSS)
        assert info["eval_tag"] == A.EVAL_WIN and len(lost) and lost[0] >= 64, (g, info, lost)
        S.same_node(gpu.node(g, []), (info, ch), (n, g))
        pv = ref.principal_variation(g)
        assert list(pv) == [ch["move_idx"][lost[0]]] and np.array_equal(gpu.principal_variation(g), pv), (g, pv)
        assert best[g] == pv[0], (g, best[g], pv)
    gpu.close()
    ref.close()


GUMBEL = [(n, k, budget) for n in SIZES for k, budget in ((4, 8), (16, 64), (64, 768)) if k < 64 or n >= 5]


@pytest.mark.parametrize("n,k,budget", GUMBEL, ids=["%dx%d-k%d-%d" % (n, n, k, b) for n, k, b in GUMBEL])
def test_gumbel_halving_at_the_cap(oracle, n, k, budget):
    """Gumbel rows [B, max_actions]: the wide roots read them to their last entry"""
    A = require_gpu()
    states, betas = cap_batch(oracle, n)
    cap = P.CAPS[n]
    gumbel = np.random.default_rng(100 * n + k).gumbel(size=(B, cap)).astype(np.float32)
    gpu = A.BatchedMCTS(B, n, P.HALF_KOMI[n], agent_kind=A.AGENT_SIMPLE, node_capacity=POOL_BATCH[n])
    ora = Ora(oracle, B, n, P.HALF_KOMI[n], agent_kind=2)
    start(gpu, states)
    start(ora, states)
    got, want = gpu.gumbel_sequential_halving(betas, k, budget, gumbel), ora.gumbel_sh(betas, k, budget, gumbel)
    assert np.array_equal(got, want), np.nonzero(got != want)[0]
    widths_at_the_cap(gpu, n)
    assert_same_roots(gpu, ora, "halving")
    assert U.compare(gpu, ora, "halving", deep=WIDE) > 2 * cap
    ip_g, ip_o = gpu.improved_policy(float(budget), cap), ora.improved_policy(float(budget), cap)
    assert np.array_equal(ip_g.view(np.uint32), ip_o.view(np.uint32))
    assert gpu.counters() == ora.counters() and gpu.pool_overflows() == 0
    gpu.close()
    ora.close()


def same_children(gpu, ora, amax, where):
    gc, oc = gpu.root_children(amax), ora.root_children(amax)
    nc = ora.root_info()["n_children"]
    for f in FIELDS:
        assert gc[f].tobytes() == oc[f].tobytes(), (where, f)
        assert not any(gc[f][g, nc[g]:].any() for g in range(B)), (where, f, "tail")


@pytest.mark.parametrize("n", (4, 6))
def test_root_side_calls_at_the_cap(oracle, n):
    """apply_noise with a [B, max_actions] Dirichlet row, root_children(max_actions), improved_policy, ube_target, select_best_actions,
    and two steps down the most visited line with simulations between them: step_kernel copies subtrees below the wide roots."""
    A = require_gpu()
    states, betas = cap_batch(oracle, n)
    cap = P.CAPS[n]
    gpu = A.BatchedMCTS(B, n, P.HALF_KOMI[n], agent_kind=A.AGENT_SIMPLE, node_capacity=POOL[n])
    ora = Ora(oracle, B, n, P.HALF_KOMI[n], agent_kind=2)
    noise = np.random.default_rng(n).dirichlet(np.full(cap, 0.3), size=B).astype(np.float32)
    for m in (gpu, ora):
        start(m, states)
        m.simulate(betas, 1)
        m.apply_noise(noise, 0.25)
        m.simulate(betas, SIMS - 1)
    widths_at_the_cap(gpu, n)
    assert_same_roots(gpu, ora, "noise")
    same_children(gpu, ora, cap, "noise")
    for visits in (float(SIMS), 800.0):
        assert gpu.improved_policy(visits, cap).tobytes() == ora.improved_policy(visits, cap).tobytes(), visits
    for beta in (0.0, 0.5):
        assert gpu.ube_target(beta).tobytes() == ora.ube_target(beta).tobytes(), beta
    for ply in range(2):
        acts = ora.select_best_actions()
        assert np.array_equal(gpu.select_best_actions(), acts), ply
        gpu.step(acts)
        ora.step(acts)
        assert gpu.get_positions().tobytes() == ora.get_positions().tobytes(), ply
        assert_same_roots(gpu, ora, "kept subtree %d" % ply)
        kept = ora.root_info()["n_children"]
        for m in (gpu, ora):
            m.simulate(betas, SIMS // 2)
        assert_same_roots(gpu, ora, "step %d" % ply)
        same_children(gpu, ora, cap, "step %d" % ply)
        assert U.compare(gpu, ora, "step %d" % ply, deep=(0, B - 1)) >= B
        if n == 6 and ply == 1:      # the subtree kept by the second step held a node about as wide as the root, with its children
            assert min(kept[g] for g in WIDE) > cap // 2, kept
    assert gpu.counters() == ora.counters() and gpu.pool_overflows() == 0
    gpu.close()
    ora.close()


@pytest.mark.parametrize("n,prec", [(5, "f32"), (5, "f16"), (6, "f32"), (6, "f16")])
def test_a_real_net_in_the_loop_at_the_cap(oracle, n, prec):
    """agent = net: the engine's legal-logit gather reads max_actions entries of a policy row; the oracle's search drives the same net
    through tz_net_eval"""
    A = require_gpu()
    from takzero_amd import weights as W

    states, betas = cap_batch(oracle, n)
    net = A.Net(arch=A.ARCH_TEST, n=n, precision=PRECS[prec], blocks=1).load_tensors(W.init_weights(W.ARCH_TEST, n=n, blocks=1, seed=3))
    gpu = A.BatchedMCTS(B, n, P.HALF_KOMI[n], agent=net, node_capacity=POOL[n])
    ora = Ora(oracle, B, n, P.HALF_KOMI[n], agent_kind=0, agent_fn=_agent_over(net))
    for m in (gpu, ora):
        start(m, states)
        m.simulate(betas, 40)
    widths_at_the_cap(gpu, n)
    assert_same_roots(gpu, ora, prec)
    assert U.compare(gpu, ora, prec, deep=(0, MIDDLE)) > 2 * P.CAPS[n]
    assert gpu.counters() == ora.counters() and gpu.pool_overflows() == 0
    gpu.close()
    ora.close()
    net.close()


# ---------------------------------------------------------------------------------------------- 3. the Agent surface beyond the cap
def agent_world(oracle, n):
    """every fixture position of one size (the over-wide successor of the under->over pair too) and ordinary positions up to 65"""
    if ("world", n) not in _cache:
        fx = P.fixture(oracle, n)
        states = [s for _, s, _ in fx.positions] + ([fx.under_over[2]] if fx.under_over else [])
        wide = len(states)
        states += E.distinct_positions(oracle, O, n, 65 - wide, 31)
        acts = [O.possible_moves(oracle, s) for s in states]
        assert max(len(a) for a in acts) == {3: 73, 4: 204, 5: 532, 6: 1144}[n]
        _cache["world", n] = dict(states=states, arr=O.states_array(states), acts=acts, wide=wide)
    return _cache["world", n]


def eval_equals(net, arr, acts, policy, value, where, bitwise=True):
    logits, val, _ = net.policy_value_uncertainty(arr, acts)
    for i, a in enumerate(acts):
        want = policy[i, np.asarray(a, np.int64)]
        assert len(logits[i]) == len(a), (where, i, len(a))
        if bitwise:
            assert np.array_equal(logits[i].view(np.uint32), want.view(np.uint32)), (where, i, len(a))
        else:               # against the fp64 graph: equal numbers (its zeros carry no sign worth comparing)
            assert np.array_equal(logits[i], want), (where, i, len(a), np.flatnonzero(logits[i] != want)[:8])
    if value is not None:
        assert np.array_equal(val.view(np.uint32), value.view(np.uint32)), where


@pytest.mark.parametrize("n,prec", NET_CASES)
def test_agent_surface_on_positions_wider_than_any_search(oracle, n, prec):
    """Net.policy_value_uncertainty with legal lists up to 1144 entries, alone and in a batch of 65: the logits are forward_raw's
    policy at the legal indices and the value is forward_raw's, bit for bit"""
    A = require_gpu()
    from takzero_amd import weights as W

    world = agent_world(oracle, n)
    arr, acts = world["arr"], world["acts"]
    net = A.Net(arch=A.ARCH_TEST, n=n, precision=PRECS[prec], blocks=1).load_tensors(W.init_weights(W.ARCH_TEST, n=n, blocks=1, seed=5))
    for i in range(world["wide"]):
        pol, val, _ = net.forward_raw(arr[i:i + 1])
        eval_equals(net, arr[i:i + 1], acts[i:i + 1], pol, val, (n, prec, "alone", i))
    pol, val, _ = net.forward_raw(arr)
    assert np.isfinite(pol).all() and np.abs(pol).max() > 0.01
    eval_equals(net, arr, acts, pol, val, (n, prec, "batch of 65"))
    net.close()


def exact_world(oracle, n):
    """An exact net (tests/exact_net.py) calibrated on ordinary positions and on the fixture's, and its fp64 graph on agent_world"""
    if ("exact", n) not in _cache:
        arch, _, blocks = E.NETS[n]
        world = agent_world(oracle, n)
        planes = E.planes_of(oracle, O, world["states"], n)
        calibration = np.concatenate([E.planes_of(oracle, O, E.distinct_positions(oracle, O, n, 96, 5), n), planes[:world["wide"]]])
        w = E.exact_weights(arch, n, blocks, 0, calibration)
        ref = E.exact_reference(w, planes, blocks)
        E.assert_reference_is_exact(ref)
        _cache["exact", n] = (w, ref)
    return _cache["exact", n]


@pytest.mark.parametrize("n,prec", NET_CASES)
def test_agent_surface_on_exact_nets_equals_the_fp64_graph(oracle, n, prec):
    A = require_gpu()
    arch, _, blocks = E.NETS[n]
    world = agent_world(oracle, n)
    w, ref = exact_world(oracle, n)
    net = A.Net(arch=arch, n=n, precision=PRECS[prec], blocks=blocks).load_tensors(w)
    arr, acts = world["arr"], world["acts"]
    for i in range(world["wide"]):
        eval_equals(net, arr[i:i + 1], acts[i:i + 1], ref["policy"][i:i + 1], None, (n, prec, "alone", i), bitwise=False)
    eval_equals(net, arr, acts, ref["policy"], None, (n, prec, "batch of 65"), bitwise=False)
    net.close()


# ---------------------------------------------------------------------------------------------- 4. over the cap
def raises_capacity(call):
    A = require_gpu()
    with pytest.raises(A.TakzeroError, match="max_actions") as e:
        call()
    assert e.value.code == ECAPACITY


def others_equal(gpu, ref, skip, where):
    """Every game but `skip` against a reference that runs without it: the root, everything about all its children, and below the two
    neighbours of `skip` every depth-1 node with its children"""
    games = [g for g in range(B) if g != skip]
    info = gpu.root_info()
    rc = gpu.root_children(P.CAPS[gpu.n])
    for j, g in enumerate(games):
        root = ref.node(j, [])
        S.same_node(gpu.node(g, []), root, (where, g, "root"))
        assert info["visit_count"][g] == root[0]["visit_count"] and info["n_children"][g] == root[0]["n_children"], (where, g)
        nc = len(root[1]["move_idx"])
        for f in FIELDS:
            assert np.array_equal(S.bits(rc[f][g, :nc]), S.bits(root[1][f])) and not rc[f][g, nc:].any(), (where, g, f)
        if abs(g - skip) == 1:
            for m in root[1]["move_idx"]:
                S.same_node(gpu.node(g, [m]), ref.node(j, [m]), (where, g, int(m)))
    return games


def unexpanded_root(gpu, game, visits):
    """the over-wide root after the error: no children, no evaluation, one visit per simulation that reached it (none backed up)"""
    info = gpu.root_info()
    assert info["n_children"][game] == 0 and info["eval_tag"][game] == 0 and info["visit_count"][game] == visits, (game, info)
    assert gpu.pool_overflows() == 0


def replacement(oracle, n):
    return fill(oracle, n, B + 1)[B]


OVER = [(n, label, index) for n in SIZES for label in ("over/near", "over/far") for index in (0, MIDDLE, B - 1)]


@pytest.mark.parametrize("graph", (True, False), ids=("graph", "eager"))
@pytest.mark.parametrize("n,label,index", OVER, ids=["%dx%d-%s-game%d" % (n, n, label.split("/")[1], i) for n, label, i in OVER])
def test_over_the_cap_simulate_errors_spares_the_others_and_recovers(oracle, monkeypatch, n, label, index, graph):
    """set_positions takes the position (it generates no moves); simulate returns TZ_ECAPACITY after running all its simulations on the
    other games, which equal the oracle's run without the over-wide game; the over-wide root is never expanded and keeps no
    evaluation, its visits are counted; after set_positions replaces it the handle equals a fresh one, and the oracle, through further simulations (replayed from the captured graph, or
    eagerly under TZ_NO_GRAPH=1)."""
    A = require_gpu()
    if not graph:
        monkeypatch.setenv("TZ_NO_GRAPH", "1")
    hk = P.HALF_KOMI[n]
    states, betas = over_batch(oracle, n, label, index)
    gpu = A.BatchedMCTS(B, n, hk, agent_kind=A.AGENT_SIMPLE, node_capacity=POOL[n])
    start(gpu, states)                                   # accepted
    assert gpu.get_positions()[index].tobytes() == O.states_array(states)[index].tobytes()
    raises_capacity(lambda: gpu.simulate(betas, SIMS))
    games = [g for g in range(B) if g != index]
    ora = Ora(oracle, B - 1, n, hk, agent_kind=2)
    ora.set_positions(np.arange(B - 1), [states[g] for g in games])
    ora.simulate(betas[games], SIMS)
    others_equal(gpu, ora, index, "after the error")
    unexpanded_root(gpu, index, SIMS)
    raises_capacity(lambda: gpu.simulate(betas, 1))      # the position is still there: every call that meets it says so
    unexpanded_root(gpu, index, SIMS + 1)
    # recovery: the same history on a fresh handle and on the oracle, with an ordinary position where the over-wide one was
    new = replacement(oracle, n)
    calm = states[:index] + [new] + states[index + 1:]
    fresh = A.BatchedMCTS(B, n, hk, agent_kind=A.AGENT_SIMPLE, node_capacity=POOL[n])
    whole = Ora(oracle, B, n, hk, agent_kind=2)
    for m in (fresh, whole):
        start(m, calm)
        m.simulate(betas, SIMS + 1)
    for m in (gpu, fresh, whole):
        m.set_positions(np.array([index], np.int32), O.states_array([new]) if m is not whole else [new])
        m.simulate(betas, SIMS // 2)
    assert_same_roots(gpu, whole, "recovered")
    assert_same_roots(fresh, whole, "fresh")
    assert U.compare(gpu, whole, "recovered", deep=sorted({max(index - 1, 0), index, min(index + 1, B - 1)})) > 10
    assert gpu.select_best_actions().tobytes() == fresh.select_best_actions().tobytes()
    assert gpu.pool_overflows() == 0
    for m in (gpu, fresh, ora, whole):
        m.close()


# 7 leaves a round at every place, and 1 leaf a round at game B - 1: its only slot is then the last act row of the allocation
OVER_BATCH = [c + (7,) for c in OVER] + [c + (1,) for c in OVER if c[2] == B - 1]


@pytest.mark.parametrize("n,label,index,leaves", OVER_BATCH,
                         ids=["%dx%d-%s-game%d-leaves%d" % (n, n, label.split("/")[1], i, k) for n, label, i, k in OVER_BATCH])
def test_over_the_cap_simulate_batch_errors_spares_the_others_and_recovers(oracle, batch_lib, n, label, index, leaves):
    """The same for simulate_batch: the over-wide leaf is not collected (its tree makes one forward a round and stops), the rows of
    the neighbours' slots stay theirs.  The row gen_moves fills is the tree's first slot, index * leaves: with one leaf a round and
    the game at B - 1 nothing lies behind it."""
    A = require_gpu()
    hk = P.HALF_KOMI[n]
    states, betas = over_batch(oracle, n, label, index)
    gpu = A.BatchedMCTS(B, n, hk, agent_kind=A.AGENT_SIMPLE, node_capacity=POOL_BATCH[n])
    start(gpu, states)
    raises_capacity(lambda: gpu.simulate_batch(betas, leaves, 5))
    games = [g for g in range(B) if g != index]
    ref = U.RefSearch(batch_lib, B - 1, n, hk, agent_kind=2)
    ref.set_positions(np.arange(B - 1), [states[g] for g in games])
    ref.simulate_batch(betas[games], leaves, 5)
    others_equal(gpu, ref, index, "after the error")
    unexpanded_root(gpu, index, 5)
    new = replacement(oracle, n)
    calm = states[:index] + [new] + states[index + 1:]
    whole = U.RefSearch(batch_lib, B, n, hk, agent_kind=2)
    whole.set_positions(np.arange(B), calm)
    whole.simulate_batch(betas, leaves, 5)
    whole.set_positions(np.array([index], np.int32), [new])
    gpu.set_positions(np.array([index], np.int32), O.states_array([new]))
    whole.simulate_batch(betas, leaves, 4)
    gpu.simulate_batch(betas, leaves, 4)
    assert U.compare(gpu, whole, "recovered", deep=sorted({max(index - 1, 0), index, min(index + 1, B - 1)})) > 10
    assert gpu.pool_overflows() == 0
    for m in (gpu, ref, whole):
        m.close()


@pytest.mark.parametrize("call", ("simulate", "simulate_batch", "gumbel"))
@pytest.mark.parametrize("n", sorted(P.UNDER_OVER))
def test_an_over_wide_node_below_the_root_errors_and_is_not_expanded(oracle, batch_lib, n, call):
    """The under->over pair at the middle game: the root fits, one of its children does not.  The error comes when the search reaches
    that child; the child stays without children and its visits are counted; the other games equal the reference's run without this
    game (simulate, simulate_batch).  Halving (k = 4, budget 8: two steps of four simulations) returns the error at the end of its first
    step: every game's four sampled children have one visit each, half of what a finished halving leaves."""
    A = require_gpu()
    fx, hk = P.fixture(oracle, n), P.HALF_KOMI[n]
    index, (at, move, _) = MIDDLE, fx.under_over
    states, betas = list(fill(oracle, n)), np.zeros(B, np.float32)
    states[index] = fx.positions[at][1]
    child = fx.positions[at][2].index(move)
    gpu = A.BatchedMCTS(B, n, hk, agent_kind=A.AGENT_SIMPLE, node_capacity=POOL_BATCH[n])
    start(gpu, states)
    games = [g for g in range(B) if g != index]
    if call == "simulate":
        raises_capacity(lambda: gpu.simulate(betas, 2 * SIMS))
        ref = Ora(oracle, B - 1, n, hk, agent_kind=2)
        ref.set_positions(np.arange(B - 1), [states[g] for g in games])
        ref.simulate(betas[games], 2 * SIMS)
        others_equal(gpu, ref, index, call)
    elif call == "simulate_batch":
        raises_capacity(lambda: gpu.simulate_batch(betas, 7, 12))
        ref = U.RefSearch(batch_lib, B - 1, n, hk, agent_kind=2)
        ref.set_positions(np.arange(B - 1), [states[g] for g in games])
        ref.simulate_batch(betas[games], 7, 12)
        others_equal(gpu, ref, index, call)
    else:
        gumbel = np.zeros((B, P.CAPS[n]), np.float32)
        gumbel[index, child] = 100.0                     # the over-wide child is among the sampled actions
        raises_capacity(lambda: gpu.gumbel_sequential_halving(betas, 4, 8, gumbel))
        visits = gpu.root_children(P.CAPS[n])["visits"]
        assert [int(v.sum()) for v in visits] == [4] * B and visits.max() == 1 and visits[index, child] == 1, visits.sum(axis=1)
    info, ch = gpu.node(index, [])
    assert info["n_children"] == len(fx.positions[at][2]) and ch["move_idx"][child] == move
    below = gpu.node(index, [move])
    assert below[0]["n_children"] == 0 and below[0]["eval_tag"] == 0 and len(below[1]["move_idx"]) == 0
    assert ch["visits"][child] == below[0]["visit_count"]
    if call != "simulate_batch":     # its rounds may end at another over-wide child of this root before they come to this one
        assert below[0]["visit_count"] >= 1
    if call == "simulate":
        assert info["visit_count"] == 2 * SIMS
    assert gpu.pool_overflows() == 0
    gpu.close()


@pytest.mark.parametrize("n,label,index", OVER, ids=["%dx%d-%s-game%d" % (n, n, label.split("/")[1], i) for n, label, i in OVER])
def test_over_the_cap_gumbel_halving_errors_and_a_reset_handle_recovers(oracle, n, label, index):
    """Halving ends at the error (here at its first simulation) and selects nothing; the trees keep the simulations made so far (one
    visit of every root, the other roots expanded as the oracle's first simulation expands them), so the halving is started again
    after set_positions of every game, and then equals the oracle's"""
    A = require_gpu()
    hk, cap = P.HALF_KOMI[n], P.CAPS[n]
    states, betas = over_batch(oracle, n, label, index)
    gumbel = np.random.default_rng(n).gumbel(size=(B, cap)).astype(np.float32)
    gpu = A.BatchedMCTS(B, n, hk, agent_kind=A.AGENT_SIMPLE, node_capacity=POOL[n])
    start(gpu, states)
    raises_capacity(lambda: gpu.gumbel_sequential_halving(betas, 16, 64, gumbel))
    assert np.array_equal(gpu.root_info()["visit_count"], np.ones(B, np.uint32))
    unexpanded_root(gpu, index, 1)
    games = [g for g in range(B) if g != index]
    first = Ora(oracle, B - 1, n, hk, agent_kind=2)
    first.set_positions(np.arange(B - 1), [states[g] for g in games])
    first.simulate(betas[games], 1)
    others_equal(gpu, first, index, "after the error")
    first.close()
    calm = states[:index] + [replacement(oracle, n)] + states[index + 1:]
    ora = Ora(oracle, B, n, hk, agent_kind=2)
    start(gpu, calm)
    start(ora, calm)
    got, want = gpu.gumbel_sequential_halving(betas, 16, 64, gumbel), ora.gumbel_sh(betas, 16, 64, gumbel)
    assert np.array_equal(got, want)
    assert_same_roots(gpu, ora, "halving after the reset")
    assert gpu.counters()[1] > 0 and gpu.pool_overflows() == 0
    gpu.close()
    ora.close()


@pytest.mark.parametrize("n", SIZES)
def test_play_moves_on_positions_wider_than_max_actions(oracle, n):
    """tz_search_play_moves judges a move against a row of 1024: on 3x3 .. 5x5 the over-wide positions (73, 204, 532 moves) are like
    any other, their last legal move included.  On 6x6 (1025 and 1144 moves) the last legal move lies beyond the row: the call
    applies the other games' moves, leaves those two positions alone and returns TZ_ECAPACITY; their first legal move is applied."""
    A = require_gpu()
    hk = P.HALF_KOMI[n]
    states = list(fill(oracle, n))
    wide = (0, B - 1)
    states[0], states[B - 1] = P.labelled(oracle, n, "over/near")[0], P.labelled(oracle, n, "over/far")[0]
    legal = [O.possible_moves(oracle, s) for s in states]
    gpu = A.BatchedMCTS(B, n, hk, agent_kind=A.AGENT_DUMMY, node_capacity=256)
    start(gpu, states)
    last = np.array([m[-1] for m in legal], np.uint16)
    if n < 6:
        assert list(gpu.play_moves(last)) == [1] * B
        judged = range(B)
    else:
        raises_capacity(lambda: gpu.play_moves(last))
        judged = [g for g in range(B) if g not in wide]
    for g in judged:
        states[g] = O.play(oracle, states[g], int(last[g]))
    assert gpu.get_positions().tobytes() == O.states_array(states).tobytes()
    if n == 6:
        first = np.full(B, 0xFFFF, np.uint16)
        for g in wide:
            first[g] = legal[g][0]
            states[g] = O.play(oracle, states[g], legal[g][0])
        assert list(gpu.play_moves(first)) == [1] + [0] * (B - 2) + [1]
        assert gpu.get_positions().tobytes() == O.states_array(states).tobytes()
    assert gpu.pool_overflows() == 0
    gpu.close()
