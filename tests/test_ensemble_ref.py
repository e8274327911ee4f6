"""net4_ensemble without a GPU: the architecture constant, the initial weights, the 64 head variables (names with spaces) through the
model files, and the reference module tests/ensemble_ref.py held to a plain restatement on a fixed 8-position example - and shown to be
sensitive: with the unbiased variance, a permuted head, a head without its tanh, the discount's sign flipped or the terminal overwrite
skipped, the same checks fail."""
import math
import os
import re
import types

import numpy as np
import pytest

import ensemble_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD_SHAPES = {"conv2d.weight": (1, 256, 1, 1), "conv2d.bias": (1,), "linear.weight": (1, 16), "linear.bias": (1,)}


def test_arch_constant_has_one_value_everywhere():
    from takzero_amd import api as A
    from takzero_amd import weights as W

    header = open(os.path.join(ROOT, "include", "takzero_hip.h")).read()
    archs = {k: int(v) for k, v in re.findall(r"^#define\s+(TZ_ARCH_\w+)\s+(\d+)\s*$", header, flags=re.M)}
    assert archs["TZ_ARCH_NET4_ENSEMBLE"] == 24 and list(archs.values()).count(24) == 1, archs
    assert A.ARCH_NET4_ENSEMBLE == W.ARCH_NET4_ENSEMBLE == 24
    assert re.findall(r"^#define\s+TZ_ENSEMBLE_SIZE\s+(\d+)\s*$", header, flags=re.M) == ["16"] and A.ENSEMBLE_SIZE == W.ENSEMBLE_SIZE == R.SIZE == 16
    sys_rs = open(os.path.join(ROOT, "bindings", "takzero-hip-sys", "src", "lib.rs")).read()
    assert re.findall(r"pub const TZ_ARCH_NET4_ENSEMBLE: c_int = (\d+);", sys_rs) == ["24"]
    assert re.findall(r"pub const TZ_ENSEMBLE_SIZE: c_int = (\d+);", sys_rs) == ["16"]
    for fn in ("tz_net_ensemble_values", "tz_trainer_set_ensemble_targets", "tz_trainer_ensemble_last"):
        assert ("pub fn %s(" % fn) in sys_rs and re.search(r"^int %s\(" % fn, header, flags=re.M), fn
    arg = open(os.path.join(ROOT, "examples", "arch_arg.h")).read()
    assert 'a == "net4_ensemble") return TZ_ARCH_NET4_ENSEMBLE;' in arg


def test_init_weights():
    from takzero_amd import weights as W

    w = W.init_weights(W.ARCH_NET4_ENSEMBLE, seed=3)
    s = W.init_weights(W.ARCH_NET4_SIMHASH, seed=3)
    heads = {R.name(i, p): HEAD_SHAPES[p] for i in range(16) for p in R.PARTS}
    want = {k: v.shape for k, v in s.items() if k != "simhash_matrix"}
    want.update(heads)
    assert {k: v.shape for k, v in w.items()} == want and len(heads) == 64
    assert all(v.dtype == np.float32 for v in w.values())
    assert all(np.array_equal(w[k], s[k]) for k in s if k != "simhash_matrix")          # the trunk and heads of net4_simhash, same draws
    keys = list(w)
    assert keys[keys.index("ube.linear.bias") + 1:] == R.names()                        # created after ube, head by head
    for p in R.PARTS:
        assert not np.array_equal(w[R.name(0, p)], w[R.name(1, p)]), p                 # two heads of one seed differ
    again = W.init_weights(W.ARCH_NET4_ENSEMBLE, seed=3)
    assert all(np.array_equal(w[k], again[k]) for k in w)
    other = W.init_weights(W.ARCH_NET4_ENSEMBLE, seed=4)
    assert not np.array_equal(w[R.name(7, "conv2d.weight")], other[R.name(7, "conv2d.weight")])
    bound = 1.0 / 16.0                                                                  # the value head's initialisers: U(+-1/sqrt(fan_in))
    assert np.abs(w[R.name(3, "conv2d.weight")]).max() <= bound and np.abs(w[R.name(3, "linear.weight")]).max() <= 0.25
    assert W.arch_board(W.ARCH_NET4_ENSEMBLE) == 4 and W.arch_blocks(W.ARCH_NET4_ENSEMBLE) == 16


# ---- the model files
def _small_store():
    """The ensemble net's variable names at a size that keeps the archive small: ARCH_TEST's trunk on 4x4 with one block + sixteen heads."""
    from takzero_amd import weights as W

    w = W.init_weights(W.ARCH_TEST, n=4, blocks=1, seed=5, trained_stats=True)
    rng = np.random.default_rng(11)
    for i in range(16):
        for p in R.PARTS:
            w[R.name(i, p)] = rng.normal(0, 0.3, size=HEAD_SHAPES[p]).astype(np.float32)
    return w


def _same(a, b):
    return set(a) == set(b) and all(np.asarray(a[k]).shape == np.asarray(b[k]).shape and
                                    np.array_equal(np.asarray(a[k], np.float32).view(np.uint32), np.asarray(b[k], np.float32).view(np.uint32)) for k in a)


def test_tzw_round_trip():
    from takzero_amd import weights as W

    w = _small_store()
    assert _same(W.loads_tzw(W.dumps_tzw(w)), w)


def test_tch_names_put_the_heads_after_ube_in_head_order():
    from takzero_amd import ot

    got = [n for n, _ in ot.tch_names(_small_store())]
    assert got[-64:] == R.names() and got[-65] == "ube.linear.bias"


def test_ot_native_writer_and_reader(tmp_path):
    """save_ot (tz_weights_convert: .tzw -> .ot, csrc/tz_ot.cpp) and back through the native reader and load_tzw, bit for bit."""
    from takzero_amd import ot

    w = _small_store()
    path = ot.save_ot(tmp_path / "model_latest.ot", w)
    assert _same(ot.load_ot(path), w)


def test_ot_native_writer_against_libtorchs_reader(tmp_path):
    from takzero_amd import ot

    w = _small_store()
    path = ot.save_ot(tmp_path / "model_latest.ot", w)
    named = ot.read_ot_libtorch(path)
    assert list(named) == [n for n, _ in ot.tch_names(w)] and list(named)[-64:] == R.names()        # creation order, not name order
    assert named["ensemble head 3.conv2d.weight"].shape == (1, 256, 1, 1) and named["ensemble head 3.linear.weight"].shape == (1, 16)
    assert _same(ot.canonical_names(named), w)


@pytest.fixture(scope="module")
def ot_writer():
    from takzero_amd import ot

    try:
        return ot.build_writer()
    except RuntimeError as e:
        pytest.skip(str(e))


def test_ot_native_reader_against_libtorchs_writer(ot_writer, tmp_path):
    from takzero_amd import ot

    w = _small_store()
    path = ot.save_ot_libtorch(tmp_path / "model_latest.ot", w)
    assert _same(ot.load_ot(path), w)
    assert _same(ot.canonical_names(ot.read_ot_libtorch(path)), w)


# ---- the reference module on a fixed example
def _example():
    rng = np.random.default_rng(2024)
    act = np.maximum(rng.integers(-6, 9, size=(8, 16, 256)), 0).astype(np.float32)           # a trunk output after its ReLU
    w = {}
    for i in range(16):
        w[R.name(i, "conv2d.weight")] = (rng.integers(-3, 4, size=(1, 256, 1, 1)) / 64.0).astype(np.float32)
        w[R.name(i, "conv2d.bias")] = np.array([rng.integers(-8, 9) / 8.0], np.float32)
        w[R.name(i, "linear.weight")] = (rng.integers(-5, 6, size=(1, 16)) / 32.0).astype(np.float32)
        w[R.name(i, "linear.bias")] = np.array([(i - 6) / 16.0], np.float32)
    nxt = rng.uniform(-0.9, 0.9, size=(8, 16)).astype(np.float32)
    terminals = np.array([R.NONE, R.LOSS, R.NONE, R.DRAW, R.NONE, R.WIN, R.NONE, R.NONE])
    ube = np.array([-9.0, -1.0, 0.5, -3.0, 2.0, -0.2, -5.0, 1.0], np.float32)
    return act, w, nxt, terminals, ube


def _plain_values(act, w):
    out = np.zeros((len(act), 16))
    for b in range(len(act)):
        for h in range(16):
            cw, cb = w[R.name(h, "conv2d.weight")].reshape(-1), float(w[R.name(h, "conv2d.bias")][0])
            lw, lb = w[R.name(h, "linear.weight")].reshape(-1), float(w[R.name(h, "linear.bias")][0])
            lin = lb
            for s in range(16):
                lin += max(0.0, math.fsum(float(act[b, s, c]) * float(cw[c]) for c in range(256)) + cb) * float(lw[s])
            out[b, h] = math.tanh(lin)
    return out


def _plain_var(v):
    f = np.float32
    out = []
    for row in v:
        total = f(row[0])
        for x in row[1:]:
            total = f(total + f(x))
        m = f(total * f(0.0625))
        s = f(0)
        for x in row:
            d = f(f(x) - m)
            s = f(s + f(d * d))
        out.append(f(s * f(0.0625)))
    return np.array(out, np.float32)


def _check_example(M):
    """Every rule of module `M` against a plain restatement on the fixed example."""
    act, w, nxt, terminals, ube = _example()
    want = _plain_values(act, w)
    got = M.heads_f64(act, w)
    assert got.shape == (8, 16) and np.abs(got - want).max() < 1e-12
    assert np.abs(np.diff(want, axis=1)).min() > 1e-6 and np.abs(np.abs(want) - 0.5).max() < 0.5        # the heads differ, none saturated
    v32 = want.astype(np.float32)
    var = M.var16_f32(v32)
    assert var.dtype == np.float32 and np.array_equal(var.view(np.uint32), _plain_var(v32).view(np.uint32))
    assert np.abs(var.astype(np.float64) - want.var(axis=1)).max() < 1e-6
    rule = M.variance_rule(np.exp(ube), var * np.float32(20))
    plain = [min(4.0, max(0.0, max(float(np.exp(u)), float(np.float32(x) * np.float32(20))))) for u, x in zip(ube, var)]
    assert np.array_equal(rule, np.array(plain, np.float32))
    wins = [float(np.exp(u)) >= float(x * np.float32(20)) for u, x in zip(ube, var)]
    assert any(wins) and not all(wins) and rule.max() == 4.0                                            # all three outcomes occur
    tg = M.bootstrap_targets(nxt, terminals)
    f = np.float32
    for i, t in enumerate(terminals):
        row = {R.NONE: [f(f(-0.997) * x) for x in nxt[i]], R.LOSS: [f(0.997)] * 16, R.WIN: [f(-0.997)] * 16, R.DRAW: [f(0)] * 16}[int(t)]
        assert np.array_equal(tg[i], np.array(row, np.float32)), (i, t)


def test_reference_module_on_the_fixed_example():
    _check_example(R)


def _mutant(**replace):
    m = types.SimpleNamespace(**{k: getattr(R, k) for k in dir(R) if not k.startswith("__")})
    for k, v in replace.items():
        setattr(m, k, v)
    return m


def _no_tanh_on_head_5(act, w):
    out = R.heads_f64(act, w)
    out[:, 5] = R.heads_pre_f64(act, w)[:, 5]
    return out


MUTANTS = {
    "unbiased variance": dict(var16_f32=lambda v: R.var16_f32(v, unbiased=True)),
    "a head permuted": dict(heads_f64=lambda act, w: R.heads_f64(act, w)[:, [1, 0] + list(range(2, 16))]),
    "a head's tanh dropped": dict(heads_f64=_no_tanh_on_head_5),
    "the discount's sign flipped": dict(bootstrap_targets=lambda n, t: R.bootstrap_targets(n, t, discount=-R.DISCOUNT)),
    "the terminal overwrite skipped": dict(bootstrap_targets=lambda n, t: R.bootstrap_targets(n, t, overwrite=False)),
}


@pytest.mark.parametrize("what", list(MUTANTS))
def test_the_checks_fail_on_a_wrong_reference(what):
    with pytest.raises(AssertionError):
        _check_example(_mutant(**MUTANTS[what]))


def test_loss_and_gradients_against_finite_differences():
    act, w, nxt, terminals, _ = _example()
    targets = R.bootstrap_targets(nxt, terminals)
    loss, values, grads = R.loss_and_grads(act, w, targets)
    assert np.abs(values - _plain_values(act, w)).max() < 1e-12
    assert abs(loss - float(((targets.astype(np.float64) - values) ** 2).mean())) < 1e-14
    assert set(grads) == set(R.names()) and all(grads[k].shape == w[k].shape for k in grads)
    rng = np.random.default_rng(3)
    for k in [R.name(2, "conv2d.weight"), R.name(9, "conv2d.bias"), R.name(4, "linear.weight"), R.name(15, "linear.bias")]:
        idx = tuple(int(rng.integers(d)) for d in w[k].shape)
        eps = 1e-6
        lo, hi = dict(w), dict(w)
        lo[k], hi[k] = w[k].astype(np.float64), w[k].astype(np.float64)
        lo[k][idx] -= eps
        hi[k][idx] += eps
        fd = (R.loss_and_grads(act, hi, targets)[0] - R.loss_and_grads(act, lo, targets)[0]) / (2 * eps)
        assert abs(fd - grads[k][idx]) < 1e-7 * max(1.0, abs(fd)), (k, idx, fd, grads[k][idx])


def test_sample_action_takes_the_first_action_past_the_draw():
    moves, probs = [7, 3, 9], [0.25, 0.5, 0.25]
    assert [R.sample_action(moves, probs, d) for d in (0.0, 0.24, 0.25, 0.74, 0.75, 0.999)] == [7, 7, 3, 3, 9, 9]
    # the library's draw rule (learn.sample_actions, what learn.ensemble_targets plays) against the reference's, edges included
    from takzero_amd import learn

    rng = np.random.default_rng(12)
    policies, draws = [], []
    for i in range(200):
        k = int(rng.integers(1, 40))
        p = rng.random(k).astype(np.float32)
        p[rng.random(k) < 0.2] = 0.0                                   # actions of probability zero are never drawn ...
        p[int(rng.integers(k))] += np.float32(0.1)                     # ... and one is always left
        policies.append((rng.permutation(500)[:k].astype(np.uint16), p / p.sum() * np.float32(0.97 if i % 3 == 0 else 1.0)))
        draws.append([0.0, 1.0 - 2.0 ** -53, float(rng.random())][i % 3])
    for d in (0.0, 0.24, 0.25, 0.74, 0.75, 0.999):
        policies.append((np.array(moves, np.uint16), np.array(probs, np.float32)))
        draws.append(d)
    got = learn.sample_actions(policies, np.array(draws))
    want = [R.sample_action(m, p, d) for (m, p), d in zip(policies, draws)]
    assert got.dtype == np.uint16 and got.tolist() == want
    assert all(p[list(m).index(a)] > 0 for (m, p), a in zip(policies, got.tolist()))
