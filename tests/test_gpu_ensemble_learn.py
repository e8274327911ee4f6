"""The learn step of net4_ensemble (eee/src/ensemble.rs:264-351) at batch 64 with the architecture's 16 blocks.

Unarmed, a trainer of this architecture is a net4_simhash trainer that carries sixteen more heads: losses, every gradient and the
updated weights are the same bytes.  Armed (tz_trainer_set_ensemble_targets), the step also trains the heads on its own detached last
activation: loss_ensemble, the [64][16] values and the 64 gradients are held to tests/ensemble_ref.py's fp64 autograd on the activation
the trainer itself reports (tz_trainer_activation), with the tolerances tests/test_gpu_learn.py applies to outputs (2e-5), losses
(1e-5 relative to 1 + |loss|) and gradients (1e-4 of the tensor's largest entry); after apply_step the weights are held the way that
file holds them (99 % within 0.05 lr, all within 2.5 lr of torch's Adam) and the moments to the gradient tolerance.  No head conv
output of the batch lies within 1e-6 of ReLU's kink (asserted), so the reference needs no side taken for it."""
import ctypes as C

import numpy as np
import pytest

import ensemble_ref as R
import oracle_lib as O
from gpu_util import require_gpu
from test_gpu_learn import _batch

pytestmark = pytest.mark.gpu
B, LAST = 64, 32          # the trunk's last layer: 1 + 2 * 16 - 1
OTOL, LTOL, GTOL = 2e-5, 1e-5, 1e-4


def _weights(seed=21):
    from takzero_amd import weights as W

    ens = W.init_weights(W.ARCH_NET4_ENSEMBLE, seed=seed, trained_stats=True)
    sim = {k: v for k, v in ens.items() if not k.startswith("ensemble head")}
    sim["simhash_matrix"] = W.init_weights(W.ARCH_NET4_SIMHASH, seed=seed)["simhash_matrix"]
    return ens, sim


def _same_bytes(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def test_unarmed_trainer_is_the_simhash_trainer_with_heads_carried(oracle):
    A = require_gpu()
    from takzero_amd import learn as L

    ens, sim = _weights()
    te = L.Trainer(arch=A.ARCH_NET4_ENSEMBLE, batch=B).load_tensors(ens)
    ts = L.Trainer(arch=A.ARCH_NET4_SIMHASH, batch=B).load_tensors(sim)
    assert set(te.names) == set(ts.names)
    batch = _batch(oracle, 4, B, 100)
    states, _, policy, mask, value, ube = batch
    assert te.step(states, policy, mask, value, ube, apply=True) == ts.step(states, policy, mask, value, ube, apply=True)
    for k in te.names:
        assert _same_bytes(te.tensor(k, L.GRAD), ts.tensor(k, L.GRAD)), ("gradient", k)
        assert _same_bytes(te.tensor(k), ts.tensor(k)), ("weight", k)
    extras = te.extras()
    assert sorted(extras) == sorted(R.names()) and all(_same_bytes(np.asarray(extras[k]).reshape(-1), ens[k].reshape(-1)) for k in R.names())
    with pytest.raises(A.TakzeroError):
        ts.set_ensemble_targets(np.zeros((B, 16), np.float32))            # TZ_EINVAL unless TZ_ARCH_NET4_ENSEMBLE
    with pytest.raises(A.TakzeroError):
        te.ensemble_last()                                                # TZ_ESTATE before an armed step
    te.close()
    ts.close()


def test_armed_step_against_fp64_autograd(oracle):
    import torch

    A = require_gpu()
    from takzero_amd import learn as L

    lr = 1e-4
    ens, _ = _weights()
    armed = L.Trainer(arch=A.ARCH_NET4_ENSEMBLE, batch=B, lr=lr).load_tensors(ens)
    plain = L.Trainer(arch=A.ARCH_NET4_ENSEMBLE, batch=B, lr=lr).load_tensors(ens)
    states, _, policy, mask, value, ube = _batch(oracle, 4, B, 100)
    targets = np.random.default_rng(8).uniform(-0.9, 0.9, size=(B, 16)).astype(np.float32)
    targets[3] = R.DISCOUNT
    want_losses = plain.step(states, policy, mask, value, ube, apply=False)
    got_losses = armed.step(states, policy, mask, value, ube, apply=False, ensemble_targets=targets)
    assert got_losses == want_losses                                      # the three existing losses: the same bytes
    for k in armed.names:
        assert _same_bytes(armed.tensor(k, L.GRAD), plain.tensor(k, L.GRAD)), ("trunk gradient", k)
    act = armed.activation(LAST)
    assert _same_bytes(act, plain.activation(LAST))
    heads = {k: armed.tensor(k) for k in R.names()}
    assert all(_same_bytes(heads[k], ens[k]) for k in R.names())           # apply = 0 leaves them alone
    loss, values = armed.ensemble_last()
    cw, cb, _, _ = R.stacked(heads)
    conv = np.einsum("bsc,hc->bhs", act.astype(np.float64), cw) + cb[None, :, None]
    assert np.abs(conv).min() > 1e-6, "a head conv output on ReLU's kink: take another batch"
    ref_loss, ref_values, ref_grads = R.loss_and_grads(act, heads, targets)
    print("armed step: loss_ensemble %.6f (fp64 %.6f), max |value - fp64| %.3g" % (loss, ref_loss, np.abs(values - ref_values).max()))
    assert np.abs(values - ref_values).max() <= OTOL and abs(loss - ref_loss) <= LTOL * (1 + abs(ref_loss))
    grads = {k: armed.tensor(k, L.GRAD) for k in R.names()}
    for k in R.names():
        scale = float(np.abs(ref_grads[k]).max()) + 1e-12
        assert grads[k].shape == ens[k].shape and float(np.abs(grads[k] - ref_grads[k]).max()) <= GTOL * scale + 1e-7, (k, scale)
    # the same step applied: Adam on the heads (step 1 of their own count), against torch's Adam on the reference gradients
    armed.step(states, policy, mask, value, ube, apply=True)
    plain.step(states, policy, mask, value, ube, apply=True)
    for k in armed.names:
        assert _same_bytes(armed.tensor(k), plain.tensor(k)), ("trunk weight after the step", k)
    params = {k: torch.tensor(heads[k].astype(np.float64), requires_grad=True) for k in R.names()}
    opt = torch.optim.Adam(list(params.values()), lr=lr)
    for k in R.names():
        params[k].grad = torch.tensor(ref_grads[k])
    opt.step()
    for k in R.names():
        diff = np.abs(armed.tensor(k) - params[k].detach().numpy())
        assert float(np.quantile(diff, 0.99)) <= 0.05 * lr and float(diff.max()) <= 2.5 * lr, (k, float(diff.max()))
        scale = float(np.abs(ref_grads[k]).max()) + 1e-12
        assert float(np.abs(armed.tensor(k, L.ADAM_M) - 0.1 * ref_grads[k]).max()) <= 0.1 * (GTOL * scale + 1e-7), k
        assert float(np.abs(armed.tensor(k, L.ADAM_V) - 0.001 * ref_grads[k] ** 2).max()) <= 0.001 * 2.1 * scale * (GTOL * scale + 1e-7) + 1e-20, k
    moved = np.concatenate([(armed.tensor(k) - heads[k]).reshape(-1) for k in R.names()])
    assert np.abs(moved).max() <= lr * 1.01 and (np.abs(moved) > 0.5 * lr).mean() > 0.5
    # disarming restores the unarmed behaviour: the heads stay, the step is the plain step
    armed.set_ensemble_targets(None)
    kept = armed.extras()
    a, b = armed.step(states, policy, mask, value, ube, apply=True), plain.step(states, policy, mask, value, ube, apply=True)
    assert a == b and all(_same_bytes(armed.tensor(k), plain.tensor(k)) for k in armed.names)
    after = armed.extras()
    assert all(_same_bytes(np.asarray(kept[k]), np.asarray(after[k])) for k in R.names())
    assert not _same_bytes(np.asarray(after[R.name(0, "conv2d.weight")]).reshape(-1), ens[R.name(0, "conv2d.weight")].reshape(-1))      # the trained heads were kept
    armed.close()
    plain.close()


def _ending_positions(oracle):
    """(state, the move that ends the game) twice: a road in one move, and the last flat on a full board."""
    out = []
    for tps in ("x4/x4/2,2,x2/1,1,1,x 1 4", "1,2,1,2/2,1,2,1/1,2,1,2/2,1,2,x 1 9"):
        s = O.state_from_tps(oracle, tps, 4, 4)
        assert oracle.tzo_terminal(C.byref(s)) == -1
        ending = [m for m in O.possible_moves(oracle, s) if oracle.tzo_terminal(C.byref(O.play(oracle, s, m))) != -1]
        assert ending, tps
        out.append((s, ending[0]))
    return out


def test_ensemble_targets_against_the_reference_rule(oracle):
    A = require_gpu()
    from gpu_util import random_positions
    from takzero_amd import learn as L

    ens, _ = _weights()
    net = A.Net(arch=A.ARCH_NET4_ENSEMBLE, precision=A.PREC_F16).load_tensors(ens)
    rng = np.random.default_rng(4)
    states = random_positions(oracle, O, 4, 4, B - 2, 17, max_ply=20)
    policies = []
    for s in states:
        mv = np.array(O.possible_moves(oracle, s), np.int64)
        p = rng.random(len(mv)).astype(np.float32)
        policies.append((mv, p / p.sum()))
    draws = rng.random(B)
    for where, (s, move) in zip((5, 40), _ending_positions(oracle)):          # the whole policy on the move that ends the game
        mv = np.array(O.possible_moves(oracle, s), np.int64)
        states.insert(where, s)
        policies.insert(where, (mv, (mv == move).astype(np.float32)))
    mcts = A.BatchedMCTS(32, 4, 4, agent=net, node_capacity=1 << 10)          # a scratch handle narrower than the batch: two chunks
    got = L.ensemble_targets(net, mcts, O.states_array(states), policies, draws)
    nxt = [O.play(oracle, s, R.sample_action(mv, p, d)) for s, (mv, p), d in zip(states, policies, draws)]
    terminals = np.array([oracle.tzo_terminal(C.byref(s)) for s in nxt])
    assert (terminals[[5, 40]] != R.NONE).all() and (terminals != R.NONE).sum() >= 2
    want = R.bootstrap_targets(net.ensemble_values(O.states_array(nxt)), terminals)
    assert got.dtype == np.float32 and got.shape == (B, 16)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), np.argwhere(got != want)[:4]
    for i in np.flatnonzero(terminals != R.NONE):
        assert np.all(got[i] == R.terminal_value(terminals[i])) and got[i, 0] in (np.float32(0.997), np.float32(-0.997), np.float32(0))
    net.close()


def test_ten_armed_steps_lower_the_loss_and_the_heads_reach_a_net(oracle):
    A = require_gpu()
    import sys

    from takzero_amd import learn as L

    ens, _ = _weights()
    tr = L.Trainer(arch=A.ARCH_NET4_ENSEMBLE, batch=B, lr=1e-3).load_tensors(ens)
    states, planes, policy, mask, value, ube = _batch(oracle, 4, B, 100)
    targets = np.random.default_rng(9).uniform(-0.9, 0.9, size=(B, 16)).astype(np.float32)
    # Twenty unarmed steps first: Adam's first steps move every trunk weight by the full lr = 1e-3 (5 % of a weight), and the heads'
    # input with them - measured without the warm-up: 0.36909, 0.39735, 0.39052, 0.32844, 0.30641, ... (the trunk's doing, not the
    # heads').  On a trunk whose optimiser has settled on the batch, what moves loss_ensemble is the heads' own steps.
    for _ in range(20):
        tr.step(states, policy, mask, value, ube, apply=True)
    losses = []
    for step in range(10):
        tr.step(states, policy, mask, value, ube, apply=True, ensemble_targets=targets if step == 0 else None)
        losses.append(tr.ensemble_last()[0])
    print("loss_ensemble over ten armed steps:", ["%.5f" % x for x in losses])
    assert all(b < a for a, b in zip(losses, losses[1:])), losses
    net = A.Net(arch=A.ARCH_NET4_ENSEMBLE, precision=A.PREC_F32)
    tr.to_net(net)
    trained = tr.tensors()
    assert set(trained) == set(ens) and not np.array_equal(np.asarray(trained[R.name(4, "linear.weight")]).reshape(-1), ens[R.name(4, "linear.weight")].reshape(-1))
    # the trainer's eval-mode values: the fp64 graph with the running statistics in place (tests/test_gpu_learn.py's to-net check, 1e-3)
    from test_gpu_ensemble import trunk_output_f64

    shaped = {k: np.asarray(v, np.float64).reshape(ens[k].shape) for k, v in trained.items()}
    want = R.heads_f64(trunk_output_f64(shaped, planes.astype(np.float64), 16), shaped)
    err = float(np.abs(net.ensemble_values(states) - want).max())
    print("ensemble_values of the trained heads against fp64 eval mode: %.3g" % err)
    assert err <= 1e-3, err
    net.close()
    tr.close()
