"""net4_rnd on the device: the tower kernel (csrc/tz_nn_rnd4.hip) behind tz_net_rnd_raw, tz_net_eval and tz_net_forward_raw.

Exact towers (tests/rnd4_ref.py `exact_towers`): raw must be the fp64 integer in every bit, in every precision, at the batch sizes that
cross the trunk's dispatch edges and the tower kernel's four boards per workgroup.  On the fixture (tests/rnd4_fixture.py) raw and
variance are held to the fp64 reference with the tolerances measured on the CPU there; a position's raw and variance are the same bits
at every slot, batch size and 16-bit precision; the variance is the stated rule of raw, ube, min and max bit for bit.

TZ_PREC_F16C6 is built for the 5x5 and 6x6 networks: tz_net_create refuses it on 4x4, for this net as for net4_simhash (one test says so).
The trainer takes batches in multiples of 64, so the carried-variables test steps at batch 64."""
import numpy as np
import pytest

import oracle_lib as O
import rnd4_fixture as FX
import rnd4_ref as R
from gpu_util import require_gpu

pytestmark = pytest.mark.gpu
PRECS = ("f32", "bf16", "f16", "f16x2", "f16c8")      # f16c6 is not built for 4x4: test_f16c6_is_refused_on_4x4_as_for_net4_simhash
SIZES = (1, 2, 3, 4, 5, 15, 16, 17, 128, 129, 257, 1025)      # 3, 4, 5: either side of the tower kernel's boards per workgroup
_cache = {}


def _bits(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _where(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    return "no difference" if not len(bad) else "%d differ, first at %d: got %r, want %r" % (len(bad), bad[0], got[bad[0]], want[bad[0]])


def _exp_dev(A, x):
    x = np.ascontiguousarray(x, np.float32)
    out = np.zeros_like(x)
    A.check(A._lib.load().tz_device_math(0, x.ctypes.data, x.ctypes.data, out.ctypes.data, len(x)))
    return out


def _restated(A, raw, ube, lo, hi):
    """The variance rule in numpy fp32 on the kernel's own raw and the returned ube, with the device's exponential."""
    return R.variance(_exp_dev(A, ube), R.local(raw, np.float32(lo), np.float32(hi), np.float32))


def _acts(oracle, fx, count):
    key = "acts"
    if key not in _cache:
        _cache[key] = [O.possible_moves(oracle, s) for s in fx["states"]]
    return _cache[key][:count]


def _net(A, prec, w):
    return A.Net(arch=A.ARCH_NET4_RND, precision=A.PREC_NAMES[prec]).load_tensors(w)


def test_f16c6_is_refused_on_4x4_as_for_net4_simhash():
    A = require_gpu()
    for arch in (A.ARCH_NET4_SIMHASH, A.ARCH_NET4_RND):
        with pytest.raises(A.TakzeroError, match="TZ_PREC_F16C6"):
            A.Net(arch=arch, precision=A.PREC_F16C6)


@pytest.mark.parametrize("prec", PRECS)
def test_exact_towers_in_every_precision_and_batch_size(oracle, prec):
    A = require_gpu()
    fx = FX.fixture(oracle)
    arr = fx["arr"]
    for seed in (0, 1):
        towers, total = R.exact_towers(seed)
        net = _net(A, prec, dict(fx["w"], **towers))
        for size in SIZES if seed == 0 else (5, 129):
            got = net.rnd_raw(arr[:size])
            assert got.shape == (size,) and _bits(got, np.full(size, total, np.float32)), (prec, seed, size, _where(got, np.full(size, total, np.float32)))
        net.close()


@pytest.mark.parametrize("prec", PRECS)
def test_fixture_against_fp64(oracle, prec):
    A = require_gpu()
    fx = FX.fixture(oracle)
    arr, n = fx["arr"], len(fx["raw64"])
    f32 = prec == "f32"
    want_raw, raw_tol, var_tol = (fx["raw64"], fx["raw_tol_f32"], fx["var_tol_f32"]) if f32 else (fx["emu64"], fx["raw_tol"], fx["var_tol"])
    e64 = float(np.exp(np.float64(fx["c"])))
    e_dev = _exp_dev(A, np.array([fx["c"]], np.float32))[0]
    for lo, hi in ((np.float32(0), np.float32(1)), (fx["min"], fx["max"])):
        net = _net(A, prec, FX.with_range(fx["w"], lo, hi))
        raw = net.rnd_raw(arr)
        _, _, ube = net.forward_raw(arr)
        _, _, var = net.policy_value_uncertainty(arr, _acts(oracle, fx, n))
        net.close()
        assert _bits(ube, np.full(n, fx["c"], np.float32))
        raw_err = float(np.abs(raw.astype(np.float64) - want_raw).max())
        loc = R.local(fx["raw64"], lo, hi)
        want_var = np.minimum(np.maximum(e64, loc), 4.0)
        tol = var_tol * (float(fx["max"]) - float(fx["min"])) / (float(hi) - float(lo))      # 4 / (max - min) x the raw terms, for this pair
        var_err = float(np.abs(var.astype(np.float64) - want_var).max())
        sharp = e64 > loc + tol
        close = int((np.abs(e64 - loc) <= tol).sum())
        print("%s min %.6g max %.6g: max |raw - reference| = %.3g (bound %.3g), max |variance - fp64| = %.3g (bound %.3g), exp(c) wins sharply on %d, %d within the tolerance of the tie"
              % (prec, lo, hi, raw_err, raw_tol, var_err, tol, int(sharp.sum()), close))
        assert raw_err <= raw_tol, (prec, raw_err, raw_tol)
        assert var_err <= tol, (prec, var_err, tol)
        assert close < 0.05 * n
        assert _bits(var[sharp], np.full(int(sharp.sum()), e_dev, np.float32)), (prec, _where(var[sharp], np.full(int(sharp.sum()), e_dev, np.float32)))
        if hi > 1:
            assert sharp.sum() >= 300 and (var == 4).sum() >= 80 and ((var > e_dev) & (var < 4)).sum() >= 300


def test_same_bits_at_every_slot_batch_size_precision_and_entry_point(oracle):
    A = require_gpu()
    fx = FX.fixture(oracle)
    arr, n = fx["arr"], len(fx["raw64"])
    w = FX.with_range(fx["w"], fx["min"], fx["max"])
    first = None
    for prec in ("f16", "bf16", "f16x2", "f16c8"):
        net = _net(A, prec, w)
        full = net.rnd_raw(arr)
        _, _, ube = net.forward_raw(arr)
        assert _bits(net.rnd_raw(arr), full)                                  # the raw of the last arithmetic, whichever call ran it
        _, _, var = net.policy_value_uncertainty(arr, _acts(oracle, fx, n))
        assert _bits(var, _restated(A, full, ube, fx["min"], fx["max"])), (prec, _where(var, _restated(A, full, ube, fx["min"], fx["max"])))
        if first is None:
            first = (full, var)
        assert _bits(full, first[0]) and _bits(var, first[1]), (prec, _where(full, first[0]))
        p, a, b = 700, 3, 911
        for order in ([p, a, b], [a, p, b], [a, b, p]):
            idx = np.array(order)
            assert _bits(net.rnd_raw(arr[idx]), full[idx]), (prec, order)
            _, _, v3 = net.policy_value_uncertainty(arr[idx], [_acts(oracle, fx, n)[i] for i in order])
            assert _bits(v3, var[idx]), (prec, order)
        for lo, hi in ((0, 1), (0, 130), (500, 629), (1024, 1025), (698, 703)):
            assert _bits(net.rnd_raw(arr[lo:hi]), full[lo:hi]), (prec, lo, hi)
        net.close()
    assert first is not None and len(set(first[0].tolist())) > 1000


def test_normalisation_edges_and_a_reload(oracle, tmp_path):
    A = require_gpu()
    from takzero_amd import weights as W

    fx = FX.fixture(oracle)
    arr, acts = fx["arr"][:130], _acts(oracle, fx, 130)
    net = _net(A, "f16", fx["w"])
    raw = net.rnd_raw(arr)
    _, _, ube = net.forward_raw(arr)
    order = np.argsort(raw)
    a, b = order[20], order[100]
    e = _exp_dev(A, ube[:1])[0]
    cases = {"raw at min and at max": (raw[a], raw[b]), "max just above min": (raw[a], np.nextafter(raw[a], np.float32(np.inf))),
             "max far away": (np.float32(0), np.float32(1e6))}
    for tag, (lo, hi) in cases.items():
        net.load_tensors(FX.with_range(fx["w"], lo, hi))
        _, _, var = net.policy_value_uncertainty(arr, acts)
        assert _bits(net.rnd_raw(arr), raw), tag
        assert _bits(var, _restated(A, raw, ube, lo, hi)), (tag, _where(var, _restated(A, raw, ube, lo, hi)))
        if tag == "raw at min and at max":
            assert var[a] == e and var[b] == 4 and var[order[0]] == e and var[order[-1]] == 4 and ((var > e) & (var < 4)).any()
        if tag == "max just above min":
            assert var[a] == e and (var[raw > raw[a]] == 4).all() and (var[raw <= raw[a]] == e).all()
        if tag == "max far away":
            assert (var == e).all()
    # a file with another min / max, loaded into the live net: the next eval uses them
    W.save_tzw(tmp_path / "other.tzw", FX.with_range(fx["w"], raw[order[40]], raw[order[90]]))
    net.load(tmp_path / "other.tzw")
    _, _, var = net.policy_value_uncertainty(arr, acts)
    assert _bits(var, _restated(A, raw, ube, raw[order[40]], raw[order[90]])) and var[order[40]] == e and var[order[90]] == 4
    net.close()


def test_layer_norm_edges(oracle):
    """The empty board, a full board, tall stacks, both sides to move - against the storage-emulating reference with the fixture's
    bound - and two positions that differ in the colour of one buried piece (two plane elements, the smallest difference the
    encoding has: a stack plane is set for one side or the other) must get different raw values."""
    import exact_net as E

    A = require_gpu()
    fx = FX.fixture(oracle)
    tps = ["x4/x4/x4/x4 1 1", "x4/x4/x4/x4 2 1", E.full_board_tps(4), "x4/x,2121212,x2/x2,121212S,x/x4 1 10", "x4/x,2121212,x2/x2,121212S,x/x4 2 10",
           "x4/x,2121212,x2/x2,121212S,x/x3,1 2 10", "x4/x,2121212,x2/x2,121212S,x/x3,1 1 11",
           "x4/x,2121212,x2/x4/x4 1 10"]
    states = [O.state_from_tps(oracle, t, 4, 4) for t in tps]
    flipped = O.TzState.from_buffer_copy(bytes(states[-1]))          # the third piece from the bottom of the stack in the other colour, reserves untouched
    flipped.colors[[i for i in range(16) if flipped.height[i] == 7][0]] ^= 1 << 2
    states.append(flipped)
    planes = E.planes_of(oracle, O, states, 4).astype(np.float64)
    assert int((planes[-1] != planes[-2]).sum()) == 2 and planes[0].reshape(28, 16).std(axis=1).max() == 0
    want = R.raw(fx["w"], planes, "emu64")
    for prec in ("f16", "f32"):
        net = _net(A, prec, fx["w"])
        got = net.rnd_raw(O.states_array(states))
        net.close()
        ref, tol = (R.raw(fx["w"], planes, "f64"), fx["raw_tol_f32"]) if prec == "f32" else (want, fx["raw_tol"])
        err = np.abs(got.astype(np.float64) - ref)
        print("LayerNorm edges %s: raw %s, max |raw - reference| = %.3g (bound %.3g)" % (prec, np.round(got, 4).tolist(), err.max(), tol))
        assert np.isfinite(got).all() and err.max() <= tol and got[-1] != got[-2] and got[0] != got[1] and len(set(got.tolist())) == len(states)


def test_files_clone_and_partial_load(oracle, tmp_path):
    A = require_gpu()
    from takzero_amd import weights as W

    fx = FX.fixture(oracle)
    arr, acts = fx["arr"][:40], _acts(oracle, fx, 40)
    a = A.Net.new(arch=A.ARCH_NET4_RND, seed=5)
    t = a.tensors()
    init = W.init_weights(W.ARCH_NET4_RND)
    assert {k: np.asarray(v).size for k, v in t.items()} == {k: v.size for k, v in init.items()}
    assert (t["rnd_predictor.layer_norm.weight"] == 1).all() and (t["rnd_target.layer_norm.bias"] == 0).all() and t["min"].tolist() == [0.0] and t["max"].tolist() == [1.0]
    assert not np.array_equal(t["rnd_predictor.input_conv2d.weight"], t["rnd_target.input_conv2d.weight"])
    want = a.rnd_raw(arr)
    out = a.policy_value_uncertainty(arr, acts)
    assert np.isfinite(want).all() and want.std() > 0 and not _bits(A.Net.new(arch=A.ARCH_NET4_RND, seed=6).rnd_raw(arr), want)
    a.save(tmp_path / "model_latest.ot")
    a.save(tmp_path / "model.tzw")
    assert sorted(p.name for p in tmp_path.iterdir()) == ["model.tzw", "model_latest.ot"]      # no set of seen positions beside it
    for path in ("model_latest.ot", "model.tzw"):
        b = A.Net(arch=A.ARCH_NET4_RND).load(tmp_path / path)
        assert _bits(b.rnd_raw(arr), want) and _bits(b.policy_value_uncertainty(arr, acts)[2], out[2]), path
        b.close()
    c = a.clone(0)
    assert _bits(c.rnd_raw(arr), want) and _bits(c.policy_value_uncertainty(arr, acts)[2], out[2])
    c.close()
    # net4_simhash's model into this net: exactly the towers, min and max are missing, and they stay as initialised
    sim = A.Net.new(arch=A.ARCH_NET4_SIMHASH, seed=8)
    W.save_tzw(tmp_path / "simhash.tzw", sim.tensors())
    e = A.Net.new(arch=A.ARCH_NET4_RND, seed=5)
    assert sorted(e.load_partial(tmp_path / "simhash.tzw")) == sorted(R.tensor_names())
    te = e.tensors()
    assert all(_bits(np.ravel(te[k]), np.ravel(t[k])) for k in R.tensor_names()) and _bits(e.rnd_raw(arr), want)
    for name, p, q in zip(("policy", "value", "ube"), e.forward_raw(arr), sim.forward_raw(arr)):
        assert _bits(p, q), name
    # the call belongs to this architecture, and the architecture is 4x4
    with pytest.raises(A.TakzeroError):
        sim.rnd_raw(arr)
    five = A.Net.new(arch=A.ARCH_NET5, seed=1)
    with pytest.raises(A.TakzeroError):
        five.rnd_raw(arr)
    with pytest.raises(A.TakzeroError):
        A.Net(arch=A.ARCH_NET4_RND, n=5)
    for net in (a, e, sim, five):
        net.close()


def test_trainer_carries_the_towers(oracle, tmp_path):
    A = require_gpu()
    from takzero_amd import learn as L
    from test_gpu_learn import _batch

    fx = FX.fixture(oracle)
    arr = fx["arr"][:40]
    w = FX.with_range(fx["w"], fx["min"], fx["max"])
    net = _net(A, "f16", w)
    raw = net.rnd_raw(arr)
    tr = L.Trainer(arch=A.ARCH_NET4_RND, batch=64).from_net(net)
    assert not set(tr.names) & set(R.tensor_names())
    states, _, policy, mask, value, ube = _batch(oracle, 4, 64, 100)
    before = tr.tensor("core.res_block_3.a.conv2d.weight").copy()
    for _ in range(3):
        tr.step(states, policy, mask, value, ube, apply=True)
    assert not np.array_equal(before, tr.tensor("core.res_block_3.a.conv2d.weight"))
    same = lambda store: sorted(k for k in R.tensor_names() if k not in store or np.asarray(store[k], np.float32).tobytes() != np.asarray(w[k], np.float32).tobytes())
    assert sorted(tr.extras()) == sorted(R.tensor_names()) and same(tr.extras()) == []
    with pytest.raises(A.TakzeroError):
        tr.rnd_enable(True)                      # training the predictor stays net5's
    tr.save(tmp_path / "model_latest.ot")
    back = L.Trainer(arch=A.ARCH_NET4_RND, batch=64).load(tmp_path / "model_latest.ot")
    assert same(back.extras()) == []
    other = A.Net.new(arch=A.ARCH_NET4_RND, seed=2)
    tr.to_net(other)
    assert same(other.tensors()) == [] and _bits(other.rnd_raw(arr), raw)
    assert not _bits(other.forward_raw(arr)[0], net.forward_raw(arr)[0])
    for h in (tr, back, other, net):
        h.close()
