"""The searches over net4_rnd on 4x4 with 32 simulations and beta = 0.5, at 8 and 64 games: lock-step simulate under the three
selection rules, simulate_batch(leaves = 8) and Gumbel halving (4 sampled actions: the budget is a multiple of k log2 k) must equal, in every byte, the CPU searches driven by an agent that
returns this net's own policy_value_uncertainty (tests/test_gpu_ensemble_search.py and tests/test_gpu_selection.py are the patterns).
The net is the fixture's (tests/rnd4_fixture.py): min / max at the 10th / 90th percentile, so the variance differs from child to child.

Then a captured search against what happens to the net it names (tests/test_gpu_graph_lifetime.py's twins under TZ_NO_GRAPH=1), and
`selfplay_cli --arch net4_rnd`."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import rnd4_fixture as FX
import selection_util as S
from gpu_util import require_gpu

pytestmark = pytest.mark.gpu
SIMS = 32


def _net(A, oracle):
    fx = FX.fixture(oracle)
    return A.Net(arch=A.ARCH_NET4_RND, precision=A.PREC_F16).load_tensors(FX.with_range(fx["w"], fx["min"], fx["max"]))


@pytest.fixture(scope="module")
def ref_lib(tmp_path_factory):
    return S.build(tmp_path_factory.mktemp("selection_ref"))


@pytest.mark.parametrize("games", [8, 64])
def test_lock_step_under_the_three_selection_rules(oracle, ref_lib, games):
    A = require_gpu()
    net = _net(A, oracle)
    choice = (np.arange(games) * 5 + 2).astype(np.int32) % 16
    betas = np.full(games, 0.5, np.float32)
    for rule in (S.PUCT, S.UCT, S.IMPROVED):
        ref = S.RefSearch(ref_lib, games, 4, 4, agent_kind=0, agent_fn=S.agent_over(net), rule=rule)
        gpu = A.BatchedMCTS(games, 4, 4, agent=net, node_capacity=1 << 12)
        gpu.set_selection(rule)
        gpu.new_openings(choice)
        ref.new_openings(choice)
        for phase in range(2):                      # eager simulations, a captured one, replays
            gpu.simulate(betas, SIMS // 2)
            ref.simulate(betas, SIMS // 2)
            assert S.compare(gpu, ref, "%s phase %d" % (S.RULE_NAMES[rule], phase)) > games
        assert gpu.pool_overflows() == 0 and not ref.nan_seen()
        ch = gpu.root_children()
        seen = ch["std_dev"][ch["visits"] > 0]
        assert len(set(seen.tolist())) >= 2 and seen.min() > 0         # exp(ube) on most children, the towers' local value where it is larger
        ref.close()
    net.close()


@pytest.mark.parametrize("games", [8, 64])
def test_gumbel_halving_and_simulate_batch(oracle, tmp_path, games):
    A = require_gpu()
    import simulate_batch_util as U
    from test_gpu_engine import _agent_over
    from test_gpu_tree import assert_same_roots

    net = _net(A, oracle)
    choice = (np.arange(games) * 3 + 1).astype(np.int32) % 16
    betas = np.full(games, 0.5, np.float32)
    gpu = A.BatchedMCTS(games, 4, 4, agent=net, node_capacity=1 << 12)
    ora = O.OracleSearch(oracle, games, 4, 4, agent_kind=0, agent_fn=_agent_over(net))
    gpu.new_openings(choice)
    ora.new_openings(choice)
    roots = gpu.get_positions()
    gumbel = np.random.default_rng(5).gumbel(size=(games, 512)).astype(np.float32)
    a = gpu.gumbel_sequential_halving(betas, 4, SIMS, gumbel)
    b = ora.gumbel_sequential_halving(betas, 4, SIMS, gumbel)
    assert np.array_equal(a, b)
    assert_same_roots(gpu, ora, "gumbel 4 / %d" % SIMS)
    assert gpu.counters() == ora.counters()
    ora.close()
    ref = U.RefSearch(U.build(tmp_path), games, 4, 4, agent_kind=0, agent_fn=_agent_over(net))
    gpu2 = A.BatchedMCTS(games, 4, 4, agent=net, node_capacity=1 << 12)
    gpu2.set_positions(np.arange(games), roots)
    ref.set_positions(np.arange(games), roots)
    for rounds in (1, 3):                            # 8 + 24 = 32 simulations per tree
        gpu2.simulate_batch(betas, 8, rounds)
        ref.simulate_batch(betas, 8, rounds)
        assert U.compare(gpu2, ref, "simulate_batch %d" % rounds) > games
    ref.close()
    net.close()


def test_larger_call_reload_and_new_range_under_a_captured_search(oracle, monkeypatch):
    """A capture names the net's work buffers (raw and variance among them), the towers' weights and min / max by value: a larger
    host-side call, a weight reload and a new min / max between simulations must each make the next simulation capture again."""
    A = require_gpu()
    from test_gpu_graph_lifetime import Twins, _bytes_equal

    fx = FX.fixture(oracle)
    B, arr = 32, fx["arr"]
    w = FX.with_range(fx["w"], fx["min"], fx["max"])
    t = Twins(A, monkeypatch, lambda: A.Net(arch=A.ARCH_NET4_RND, precision=A.PREC_F16).load_tensors(w))
    gpu, twin = t.search(B, 4, 1 << 12)
    choice = (np.arange(B) * 3 + 1).astype(np.int32) % 16
    gpu.new_openings(choice)
    twin.new_openings(choice)
    betas = np.where(np.arange(B) % 2 == 0, 0.5, 0.25).astype(np.float32)

    def simulate(where):
        for s, tw in t.pairs:
            s.simulate(betas, 8)
            tw.simulate(betas, 8)
        t.check(where)

    simulate("first")
    out = [net.rnd_raw(arr[:300]) for net in t.nets]
    _bytes_equal(out[0], out[1], "rnd_raw 300")
    simulate("after a larger host-side call")
    other = dict(w)
    other["rnd_predictor.last_small_block.batch_norm.bias"] = w["rnd_predictor.last_small_block.batch_norm.bias"] + np.float32(0.05)
    before = t.nets[0].rnd_raw(arr[:B])
    for net in t.nets:
        net.load_tensors(other)
    after = [net.rnd_raw(arr[:B]) for net in t.nets]
    _bytes_equal(after[0], after[1], "rnd_raw after the reload")
    assert not np.array_equal(before, after[0])
    simulate("after the reload")
    for net in t.nets:
        net.load_tensors(FX.with_range(other, np.float32(fx["min"]) + np.float32(0.5), np.float32(fx["max"]) - np.float32(0.5)))
    simulate("after a new min / max")
    t.finish(oracle, 4)


def test_selfplay_program_runs_net4_rnd(oracle, tmp_path):
    A = require_gpu()
    from takzero_amd import formats as F
    from test_gpu_native_driver import _build_example, _fields

    exe = _build_example(tmp_path, "selfplay_cli")
    d = str(tmp_path / "run")
    os.makedirs(d)
    net = _net(A, oracle)
    net.save(os.path.join(d, "model_latest.ot"))
    net.close()
    assert sorted(os.listdir(d)) == ["model_latest.ot"]
    open(os.path.join(d, "buffer_lengths.txt"), "w").write(F.format_buffer_lengths(0, 0))
    r = subprocess.run([exe, "--directory", d, "--arch", "net4_rnd", "--games", "32", "--sims", "8", "--sampled-actions", "4", "--search", "gumbel",
                        "--wait-limit", "5", "--moves", "3", "--seed", "9"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr[-1500:])
    f = _fields(r.stdout)
    assert f["moves"] == "3" and int(f["model_reloads"]) >= 1
    path = os.path.join(d, "targets-selfplay.txt")
    data = open(path, "rb").read() if os.path.exists(path) else b""
    targets, used, skipped = F.parse_targets(data, 4, 4)
    assert used == len(data) and skipped == 0 and len(targets) == int(f["targets"]) == data.count(b"\n")
