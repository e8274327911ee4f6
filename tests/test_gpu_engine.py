"""End-to-end parity: the HIP engine (tree kernels + MFMA net on the device, no host round trip
inside a simulation) against the CPU oracle search whose agent is the *same* HIP network called
through tz_net_eval.  With identical priors on both sides visit counts and chosen moves must be
equal (north_star: 'visit counts and chosen moves matching ... under a fixed RNG seed')."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
from gpu_util import random_positions, require_gpu
from test_gpu_tree import assert_same_roots

pytestmark = pytest.mark.gpu


def _agent_over(net):
    def fn(user, n_envs, states, legal_idx, legal_count, amax, logits_out, value_out, variance_out):
        rc = net.lib.tz_net_eval(net.h, n_envs, C.cast(states, C.c_void_p), C.cast(legal_idx, C.c_void_p),
                                 C.cast(legal_count, C.c_void_p), amax, C.cast(logits_out, C.c_void_p),
                                 C.cast(value_out, C.c_void_p), C.cast(variance_out, C.c_void_p))
        assert rc == 0, net.lib.tz_last_error()
    return fn


def _watched(agent, states_seen=None, variances=None, sizes=None):
    """`agent` (an _agent_over) with the states it is given, the variances it returns and its batch sizes kept for the caller."""
    def fn(user, n_envs, states, legal_idx, legal_count, amax, logits_out, value_out, variance_out):
        agent(user, n_envs, states, legal_idx, legal_count, amax, logits_out, value_out, variance_out)
        if sizes is not None:
            sizes.append(n_envs)
        if states_seen is not None:
            raw = np.frombuffer(C.string_at(states, n_envs * O.STATE_DTYPE.itemsize), dtype=O.STATE_DTYPE)
            clean = np.zeros(n_envs, O.STATE_DTYPE)      # field by field: the struct's padding is not part of a position
            clean[...] = raw
            states_seen.extend(clean[i:i + 1] for i in range(n_envs))
        if variances is not None:
            variances.extend(np.ctypeslib.as_array(variance_out, (n_envs,)).tolist())
    return fn


def _starts_with_and_without_a_move_that_ends_the_game(oracle, n, B):
    """Positions from random playouts for the games of a "seen" case: odd games start where some move ends the game, even games where
    none does.  A leaf that ends the game needs no network, so the list of games that do (game_index in the net's kernels, compacted
    in ascending game order) stops being 0, 1, 2, ... - from the openings a search of two moves never gets that far."""
    lo, hi = {4: (8, 40), 6: (80, 160)}[n]          # random 6x6 games run long before a single move can end them
    pool = random_positions(oracle, O, n, 4, max(12 * B, 100), 31 + n, min_ply=lo, max_ply=hi)
    ends = [any(oracle.tzo_terminal(C.byref(O.play(oracle, s, m))) != -1 for m in O.possible_moves(oracle, s)) for s in pool]
    with_end, without = [s for s, e in zip(pool, ends) if e], [s for s, e in zip(pool, ends) if not e]
    assert len(with_end) >= B // 2 and len(without) >= B - B // 2, (len(with_end), len(without))
    return O.states_array([(with_end if g % 2 else without)[g // 2] for g in range(B)])


def _populate_set_from_what_the_search_meets(oracle, net, B, n, sims, moves, starts):
    """The SimHash set filled from the search's own positions: the oracle search of the test below runs once over the net with its
    empty set, and of the distinct states its agent was asked about those under every second distinct index are marked as seen
    (update_counts)."""
    met = []
    ora = O.OracleSearch(oracle, B, n, 4, agent_kind=0, agent_fn=_watched(_agent_over(net), states_seen=met))
    rng = np.random.default_rng(2024)
    rng.integers(0, 16, B)
    ora.set_positions(np.arange(B), starts)
    betas = np.where(np.arange(B) % 2 == 0, 0.25, 0.0).astype(np.float32)
    for mv in range(moves):
        ora.simulate(betas, 1)
        info = ora.root_info()
        noise = np.zeros((B, max(1, int(info["n_children"].max()))), np.float32)
        for g in range(B):
            noise[g, :info["n_children"][g]] = rng.dirichlet([0.05] * int(info["n_children"][g])).astype(np.float32)
        ora.apply_noise(noise, 0.2)
        ora.simulate(betas, sims)
        ora.step(ora.select_best_actions())
        ora.restart_terminal(rng.integers(0, 16, B))
    ora.close()
    distinct = np.concatenate(list({s.tobytes(): s for s in met}.values()))      # in the order of first meeting
    # The positions of a search are close relatives and SimHash gives relatives the same index: with every second distinct *state*
    # marked, a 4x4 search from the openings had 97 % of its evaluations come back as seen.  So every second distinct *index*, in the
    # order of first meeting, is marked, through the states that carry it.
    idx = net.hash_indices(distinct)
    first = np.sort(np.unique(idx, return_index=True)[1])
    assert len(first) >= 20, len(first)
    net.hash_indices(distinct[np.isin(idx, idx[first[::2]])], update=True)
    return len(met), len(distinct), len(first)


# (100,...) small nets; (5,...) full net5 = config 2 at test size; (4,...) config 1: 4x4, 64 games, 100 sims/move,
# net4_simhash; (6,...) config 4 at test size: 6x6, net6_simhash.  rnd "calibrated": net5 with the RND min / max of update_rnd and a
# constant UBE (test_gpu_uncertainty.rnd_fixture), so that the std_dev compared bit for bit carries a variance that depends on the
# position (under min 0 / max 1 it is 1.56-1.57 everywhere).  "seen": a SimHash net in fp16 with a constant UBE of ln 0.5 and a set
# populated from the search's own positions, so that the variance is 0.5 or 4 by the position: the std_dev compared bit for bit then
# depends on the in-search launch's state gather (game_index), its count (count_dev) and the set, where an empty set gives 2 everywhere.
# Its games start from positions of random playouts, every second one with a move that ends the game, so that game_index is not 0, 1, 2 ...
ENGINE_CASES = [(100, 5, 2, 0, 24, 30, 5, None), (100, 4, 1, 1, 16, 25, 4, None), (5, 5, 20, 0, 12, 24, 3, None),
                (5, 5, 20, 2, 12, 24, 2, None), (4, 4, 16, 0, 64, 100, 2, None), (6, 6, 16, 0, 8, 40, 2, None),
                (5, 5, 20, 2, 12, 24, 2, "calibrated"), (4, 4, 16, 2, 64, 100, 2, "seen"), (6, 6, 16, 2, 8, 40, 2, "seen")]


@pytest.mark.parametrize("arch,n,blocks,prec,B,sims,moves,rnd", ENGINE_CASES,
                         ids=["-".join(str(v) for v in case if v is not None) for case in ENGINE_CASES])
def test_engine_matches_oracle_search_with_same_net(oracle, arch, n, blocks, prec, B, sims, moves, rnd):
    A = require_gpu()
    from takzero_amd import weights as W

    net = A.Net(arch=arch, n=n, precision=prec, blocks=blocks)
    variances = sizes = None
    if rnd == "seen":
        from test_gpu_simhash import constant_ube

        net.load_tensors(constant_ube(W.init_weights(arch, n=n, blocks=blocks, seed=123), float(np.float32(np.log(0.5)))))
        starts = _starts_with_and_without_a_move_that_ends_the_game(oracle, n, B)
        met, distinct, indices = _populate_set_from_what_the_search_meets(oracle, net, B, n, sims, moves, starts)
        variances, sizes = [], []
    elif rnd:
        from test_gpu_uncertainty import rnd_fixture

        net.load_tensors(rnd_fixture(oracle, rnd)["w"])
    else:
        net.load_tensors(W.init_weights(arch, n=n, blocks=blocks, seed=123))
    gpu = A.BatchedMCTS(B, n, 4, agent=net, node_capacity=1 << 14)
    ora = O.OracleSearch(oracle, B, n, 4, agent_kind=0, agent_fn=_watched(_agent_over(net), variances=variances, sizes=sizes))
    rng = np.random.default_rng(2024)
    choice = rng.integers(0, 16, B)
    if rnd == "seen":
        gpu.set_positions(np.arange(B), starts)
        ora.set_positions(np.arange(B), starts)
    else:
        gpu.new_openings(choice)
        ora.new_openings(choice)
    betas = np.where(np.arange(B) % 2 == 0, 0.25, 0.0).astype(np.float32)
    for mv in range(moves):
        gpu.simulate(betas, 1)
        ora.simulate(betas, 1)
        info = ora.root_info()
        amax = max(1, int(info["n_children"].max()))
        noise = np.zeros((B, amax), np.float32)
        for g in range(B):
            noise[g, :info["n_children"][g]] = rng.dirichlet([0.05] * int(info["n_children"][g])).astype(np.float32)
        gpu.apply_noise(noise, 0.2)
        ora.apply_noise(noise, 0.2)
        gpu.simulate(betas, sims)
        ora.simulate(betas, sims)
        assert_same_roots(gpu, ora, "move %d" % mv)
        acts = gpu.select_best_actions()
        assert np.array_equal(acts, ora.select_best_actions())
        gpu.step(acts)
        ora.step(acts)
        choice = rng.integers(0, 16, B)
        assert np.array_equal(gpu.restart_terminal_envs(choice), ora.restart_terminal(choice))
    assert gpu.counters() == ora.counters()
    if variances is not None:
        var = np.array(variances, np.float32)
        low, high = float((var < 4).mean()), float((var == 4).mean())
        print("%dx%d: the first search met %d states, %d distinct, under %d indices, every second index marked as seen; of %d evaluations "
              "of the second search %.1f %% came back below 4, %.1f %% at 4" % (n, n, met, distinct, indices, var.size, 100 * low, 100 * high))
        assert np.all((var == 4) | np.isclose(var, 0.5, rtol=1e-6, atol=0))
        assert low >= 0.1 and high >= 0.1
        partial = float((np.array(sizes) < B).mean())
        print("%dx%d: %.1f %% of the net's batches held fewer than the %d games; %r of %r leaves went to the net" % ((n, n, 100 * partial, B) + gpu.counters()[::-1]))
        assert partial >= 0.1 and gpu.counters()[1] < gpu.counters()[0]


def test_gumbel_search_at_trained_scale_agrees_with_the_fp32_path():
    """The reference's current self-play search - Gumbel sequential halving, 64 sampled actions, budget 768 - reads the logits
    directly (gumbel + logit picks the candidates, then sigma(q) + logit ranks them), so it is the search most exposed to logit
    error.  Same positions, same Gumbel noise, weights at a trained net's logit scale: the action chosen under each arithmetic against
    the one chosen under the fp32 validation network, and the visit counts at the root.  The two arithmetics that hold the 1e-3
    logit tolerance choose the same action in (nearly) every game; the fp16 default is reported."""
    A = require_gpu()
    from takzero_amd import precision as P

    n, B, k, budget = 5, 128, 64, 768
    states = P.sample_positions(5, 4, B, seed=11, plies=10)
    w = P.trained_scale_weights(A.ARCH_NET5, states[:64], seed=123)
    rng = np.random.default_rng(3)
    gumbel = rng.gumbel(size=(B, 512)).astype(np.float32)      # one draw per child, in possible_moves order
    results = {}
    for name in ("f32", "f16x2", "f16c8", "f16c6", "f16"):
        net = A.Net(arch=A.ARCH_NET5, precision=A.PREC_NAMES[name]).load_tensors(w)
        mcts = A.BatchedMCTS(B, n, 4, agent=net, node_capacity=1 << 14)
        mcts.set_positions(np.arange(B), states)
        top = mcts.gumbel_sequential_halving(np.zeros(B, np.float32), k, budget, gumbel)
        ch = mcts.root_children()
        results[name] = (top.copy(), ch["visits"].astype(np.int64))
        mcts.close()
        net.close()
    ref_top, ref_vis = results["f32"]
    # the fp16 default is gated too, below what round 2 measured for it (0.93 / 0.61), so that a regression of it shows
    for name, min_same, min_identical in (("f16x2", 0.99, 0.97), ("f16c8", 0.98, 0.94), ("f16c6", 0.98, 0.94), ("f16", 0.85, 0.45)):
        top, vis = results[name]
        same = float((top == ref_top).mean())
        identical = float((vis == ref_vis).all(1).mean())
        print("gumbel 64/768 at trained scale, %s vs f32 over %d games: same chosen action %.4f, identical root visit counts %.4f" % (name, B, same, identical))
        assert same >= min_same and identical >= min_identical, name


@pytest.mark.parametrize("scale,B,gates", [
    # (precision, min fraction of games with the same chosen move, min fraction with identical visit counts at every root child,
    #  max mean total-variation distance of the visit distributions)
    ("random-init", 512, (("f16x2", 0.995, 0.98, 0.002), ("f16c8", 0.995, 0.97, 0.003), ("f16c6", 0.995, 0.97, 0.003), ("f16", 0.98, 0.95, 0.02), ("bf16", 0.90, 0.85, 0.10))),
    ("trained", 128, (("f16x2", 0.99, 0.97, 0.005), ("f16c8", 0.99, 0.95, 0.008), ("f16c6", 0.99, 0.95, 0.008), ("f16", 0.90, 0.50, 0.10))),
])
def test_search_with_the_mfma_nets_agrees_with_the_fp32_path_on_moves_and_visits(scale, B, gates):
    """North star: visit counts and chosen moves match the reference's fp32 path.  Bit-exactness of the tree is proven
    against the oracle fed the same network outputs (above); this is the other half: the MFMA precisions against the fp32
    validation network (within 1e-6 of LibTorch) under the same search, same roots, same Dirichlet noise - how far do the
    logit differences move 400-simulation searches?  Random-init weights (|logit| ~ 0.2, flat priors) on 512 games, and weights at
    a trained net's output scale (|logit| = 8, sharp priors: takzero_amd.precision.trained_scale_weights) on 128."""
    A = require_gpu()
    from takzero_amd import precision as P
    from takzero_amd import weights as W

    n, sims = 5, 400
    if scale == "trained":
        w = P.trained_scale_weights(A.ARCH_NET5, P.sample_positions(5, 4, 64, seed=7), seed=123)
    else:
        w = W.init_weights(W.ARCH_NET5, seed=123)
    rng = np.random.default_rng(7)
    choice = rng.integers(0, 16, B)
    results = {}
    noise = None
    for name in ("f32",) + tuple(g[0] for g in gates):
        net = A.Net(arch=A.ARCH_NET5, precision=A.PREC_NAMES[name]).load_tensors(w)
        mcts = A.BatchedMCTS(B, n, 4, agent=net, node_capacity=1 << 15)
        mcts.new_openings(choice)
        betas = np.zeros(B, np.float32)
        mcts.simulate(betas, 1)
        if noise is None:
            info = mcts.root_info()
            amax = int(info["n_children"].max())
            noise = np.zeros((B, amax), np.float32)
            for g in range(B):
                noise[g, :info["n_children"][g]] = rng.dirichlet([0.05] * int(info["n_children"][g])).astype(np.float32)
        mcts.apply_noise(noise, 0.25)
        mcts.simulate(betas, sims)
        ch = mcts.root_children()
        results[name] = (mcts.select_best_actions().copy(), ch["visits"].astype(np.float64), ch["move_idx"].copy())
        mcts.close()
        net.close()
    ref_act, ref_vis, ref_moves = results["f32"]
    for name, min_same, min_identical, max_tv in gates:
        act, vis, moves = results[name]
        assert np.array_equal(moves, ref_moves)
        same = float((act == ref_act).mean())
        tv = 0.5 * np.abs(vis / vis.sum(1, keepdims=True) - ref_vis / ref_vis.sum(1, keepdims=True)).sum(1)
        identical = float((vis == ref_vis).all(1).mean())
        print("%s, %s vs f32 over %d games: same chosen move %.4f of games, identical visit counts %.4f of games, total-variation "
              "distance of the visit distributions mean %.5f max %.4f" % (scale, name, B, same, identical, tv.mean(), tv.max()))
        assert same >= min_same and identical >= min_identical and tv.mean() <= max_tv, name
