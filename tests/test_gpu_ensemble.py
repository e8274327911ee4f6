"""net4_ensemble on the device: the sixteen heads (ensemble_heads_kernel behind every launch form a 4x4 net reaches), the variance
rule, and the model files.

Exact nets: the integer-valued net4_simhash-shaped trunk of tests/exact_net.py plus sixteen different heads with small dyadic weights
(tests/ensemble_ref.py `dyadic_heads`).  Every one of the 16 * B head values must be the same bits in every precision and launch form
and within 1e-4 of fp64 tanh of the exact pre-activation (the bound the project holds the value head to); policy, value and UBE of the
same net are the bits net4_simhash returns for the same trunk.  The batch sizes are 4x4's dispatch edges (tests/test_gpu_net_forms.py);
TZ_TOWER and TZ_NET_SPLIT are read once per process, so those cases run in children (tests/ensemble_forms_child.py), which run
net4_simhash under the same switch for that comparison.

The variance of tz_net_eval must equal clip(max(exp_dev(ube), var16_f32(values)), 0, 4) bit for bit, with `values` the bits
tz_net_ensemble_values returned, var16_f32 the reference's fp32 two-pass formula and exp_dev the device's expf (tz_device_math op 0)."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import ensemble_ref as R
import exact_net as E
import oracle_lib as O
from ensemble_forms_child import PRECS, SIZES
from gpu_util import require_gpu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

EVAL_UP_TO = 129
VALUE_TOL = {"f32": 1e-3, "bf16": 5e-3, "f16": 1e-3, "f16x2": 1e-3, "f16c8": 1e-3}      # tests/test_gpu_net.py: F32_TOL, BF16_VALUE_TOL
_cache = {}


def _where(got, want):
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    return "no difference" if not len(bad) else "%d differ, first at %s: got %r, want %r" % (
        len(bad), tuple(bad[0]), np.asarray(got)[tuple(bad[0])], np.asarray(want)[tuple(bad[0])])


def _bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def trunk_output_f64(w, planes, blocks, chunk=256):
    """The tower's last activation in fp64 as [B, 16 squares, 256 channels] (oracle/nets_torch.py's trace)."""
    import nets_torch as T
    import torch

    out = []
    for lo in range(0, len(planes), chunk):
        trace = []
        T.forward(w, planes[lo:lo + chunk], blocks, dtype=torch.float64, trace=trace)
        x = [t for k, t in trace if k.startswith("core.")][-1]
        out.append(x.permute(0, 2, 3, 1).reshape(x.shape[0], -1, x.shape[1]).numpy())
    return np.concatenate(out)


def world(oracle):
    if "world" not in _cache:
        states = E.distinct_positions(oracle, O, 4, max(SIZES), 77)
        arr = O.states_array(states)
        acts = [O.possible_moves(oracle, s) for s in states[:EVAL_UP_TO]]
        calibration = E.planes_of(oracle, O, E.distinct_positions(oracle, O, 4, 96, 5), 4)
        _cache["world"] = dict(arr=arr, planes=E.planes_of(oracle, O, states, 4), acts=acts, calibration=calibration)
    return _cache["world"]


def exact(oracle):
    """Once per module: the exact trunk with net4_simhash's variables, the same trunk with sixteen dyadic heads, and the fp64
    pre-activations of the heads on every position."""
    if "exact" not in _cache:
        from takzero_amd import weights as W

        wd = world(oracle)
        t0 = time.time()
        sim = E.exact_weights(W.ARCH_NET4_SIMHASH, 4, 16, 0, wd["calibration"])
        act = trunk_output_f64(sim, wd["planes"], 16)
        assert np.abs(act - np.rint(act)).max() < 1e-3 and act.max() <= E.MAX_ACTIVATION
        act = np.rint(act)
        heads = R.dyadic_heads(0, act[:256])
        ens = {k: v for k, v in sim.items() if k != "simhash_matrix"}
        ens.update(heads)
        pre = R.heads_pre_f64(act, heads)
        assert np.abs(pre).max() < 4.0 and len({heads[R.name(i, "conv2d.weight")].tobytes() for i in range(16)}) == 16
        print("exact ensemble net: fp64 trunk of %d positions in %.1f s, |pre-activation| up to %.2f" % (len(act), time.time() - t0, np.abs(pre).max()))
        _cache["exact"] = dict(sim=sim, ens=ens, act=act, pre=pre, want=np.tanh(pre))
    return _cache["exact"]


def _check_values(tag, got, x, size):
    """got [size, 16] against fp64 tanh, and against the bits the first caller saw."""
    assert got.shape == (size, 16) and got.dtype == np.float32, tag
    err = np.abs(got.astype(np.float64) - x["want"][:size]).max()
    assert err < 1e-4, (tag, err)
    first = _cache.setdefault("value bits", np.full(x["want"].shape, np.nan, np.float32))
    fresh = np.isnan(first[:size])
    first[:size][fresh] = got[fresh]
    assert _bits(first[:size], got), (tag, _where(got, first[:size]))


@pytest.mark.parametrize("prec", PRECS)
def test_exact_heads_are_the_same_bits_in_every_precision_and_batch_size(oracle, prec):
    A = require_gpu()
    x, wd = exact(oracle), world(oracle)
    arr, acts = wd["arr"], wd["acts"]
    net = A.Net(arch=A.ARCH_NET4_ENSEMBLE, precision=A.PREC_NAMES[prec]).load_tensors(x["ens"])
    sim = A.Net(arch=A.ARCH_NET4_SIMHASH, precision=A.PREC_NAMES[prec]).load_tensors(x["sim"])
    for size in SIZES:
        _check_values((prec, size), net.ensemble_values(arr[:size]), x, size)
        for name, a, b in zip(("policy", "value", "ube"), net.forward_raw(arr[:size]), sim.forward_raw(arr[:size])):
            assert _bits(a, b), (prec, size, name, _where(a, b))
        if size <= EVAL_UP_TO:
            la, va, _ = net.policy_value_uncertainty(arr[:size], acts[:size])
            lb, vb, _ = sim.policy_value_uncertainty(arr[:size], acts[:size])
            assert _bits(va, vb) and all(_bits(p, q) for p, q in zip(la, lb)), (prec, size, "eval")
    net.close()
    sim.close()


@pytest.mark.parametrize("switch", [{"TZ_TOWER": "0"}, {"TZ_TOWER": "1"}, {"TZ_TOWER": "2"}, {"TZ_NET_SPLIT": "0"}],
                         ids=lambda s: "-".join("%s=%s" % kv for kv in s.items()))
def test_exact_heads_in_the_switched_launch_forms(oracle, tmp_path, switch):
    A = require_gpu()
    from takzero_amd import weights as W

    x, wd = exact(oracle), world(oracle)
    np.save(tmp_path / "states.npy", np.frombuffer(wd["arr"][:max(SIZES)].tobytes(), np.uint8))
    W.save_tzw(tmp_path / "exact.tzw", x["ens"])
    W.save_tzw(tmp_path / "sim.tzw", x["sim"])
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "ensemble_forms_child.py"), str(tmp_path)], env=dict(os.environ, **switch),
                           capture_output=True, text=True, timeout=600)
    except subprocess.TimeoutExpired:
        pytest.exit("ensemble_forms_child.py under %r did not finish: nothing more is started on the GPU" % (switch,), returncode=1)
    if r.returncode < 0:
        pytest.exit("ensemble_forms_child.py under %r died on signal %d: nothing more is started on the GPU\n%s" % (switch, -r.returncode, r.stderr[-2000:]),
                    returncode=1)
    assert r.returncode == 0, r.stderr[-3000:]
    for prec in PRECS:
        got = np.load(tmp_path / ("out_%s.npz" % prec))
        for size in SIZES:
            _check_values((switch, prec, size), got["ens_%d" % size], x, size)
            for k, name in enumerate(("policy", "value", "ube")):          # the bits net4_simhash returns under the same switch
                a, b = got["raw_%d_%d" % (size, k)], got["sim_%d_%d" % (size, k)]
                assert a.shape == b.shape and _bits(a, b), (switch, prec, size, name, _where(a, b))


def _exp_dev(A, x):
    x = np.ascontiguousarray(x, np.float32)
    out = np.zeros_like(x)
    A.check(A._lib.load().tz_device_math(0, x.ctypes.data, x.ctypes.data, out.ctypes.data, len(x)))
    return out


def test_variance_is_the_rule_applied_to_the_returned_values(oracle):
    """Three nets on the exact trunk: UBE pushed far down (var_16 wins everywhere), UBE bias raised (expf(ube) wins), UBE head scaled
    up (the clamp at 4 bites)."""
    A = require_gpu()
    x, wd = exact(oracle), world(oracle)
    arr, acts = wd["arr"], wd["acts"]
    ulw, ulb = x["ens"]["ube.linear.weight"], x["ens"]["ube.linear.bias"]
    variants = {"var16": dict(x["ens"], **{"ube.linear.bias": ulb - np.float32(16.0)}),
                "expf": dict(x["ens"], **{"ube.linear.weight": ulw * np.float32(0.125), "ube.linear.bias": np.array([0.75], np.float32)}),
                "clamp": dict(x["ens"], **{"ube.linear.weight": ulw * np.float32(4.0), "ube.linear.bias": np.array([2.0], np.float32)})}
    seen = dict(var16=0, expf=0, clamp=0)
    for prec in ("f16", "f32", "f16x2"):
        for tag, w in variants.items():
            net = A.Net(arch=A.ARCH_NET4_ENSEMBLE, precision=A.PREC_NAMES[prec]).load_tensors(w)
            for size in (1, 65, EVAL_UP_TO):
                values = net.ensemble_values(arr[:size])
                _, _, ube = net.forward_raw(arr[:size])
                _, _, var = net.policy_value_uncertainty(arr[:size], acts[:size])
                v16, e = R.var16_f32(values), _exp_dev(A, ube)
                want = R.variance_rule(e, v16)
                assert _bits(var, want), (prec, tag, size, _where(var, want))
                if size == EVAL_UP_TO:
                    seen["var16"] += int(((v16 > e) & (v16 < 4)).sum())
                    seen["expf"] += int(((e > v16) & (e < 4)).sum())
                    seen["clamp"] += int((np.maximum(e, v16) > 4).sum())
            net.close()
    print("variance outcomes over the tested positions:", seen)
    assert all(n > 0 for n in seen.values()), seen


def _dense(oracle, prec):
    from takzero_amd import weights as W
    from test_gpu_net import _trained_scale

    w = W.init_weights(W.ARCH_NET4_ENSEMBLE, seed=9, trained_stats=True)
    if prec in ("f16x2", "f16c8"):
        w = _trained_scale(w, world(oracle)["planes"][:64], 16)
    return w


@pytest.mark.parametrize("prec", PRECS)
def test_dense_heads_against_fp64_and_across_batch_sizes(oracle, prec):
    A = require_gpu()
    wd = world(oracle)
    arr = wd["arr"]
    w = _dense(oracle, prec)
    if ("dense ref", prec in ("f16x2", "f16c8")) not in _cache:
        _cache["dense ref", prec in ("f16x2", "f16c8")] = R.heads_f64(trunk_output_f64(w, wd["planes"][:64], 16), w)
    want = _cache["dense ref", prec in ("f16x2", "f16c8")]
    net = A.Net(arch=A.ARCH_NET4_ENSEMBLE, precision=A.PREC_NAMES[prec]).load_tensors(w)
    got = net.ensemble_values(arr[:64])
    err = float(np.abs(got.astype(np.float64) - want).max())
    print("dense heads %s: max |value - fp64| = %.3g over %d values, spread of the heads %.3g" % (prec, err, got.size, float(got.std(axis=1).mean())))
    assert got.std(axis=1).min() > 1e-3 and err < VALUE_TOL[prec], (prec, err)
    full = net.ensemble_values(arr[:1030])
    parts = np.concatenate([net.ensemble_values(arr[lo:lo + 64]) for lo in range(0, 1030, 64)])
    assert _bits(full, parts), (prec, _where(full, parts))
    for size in (1, 65, 129, 305):
        assert _bits(net.ensemble_values(arr[:size]), full[:size]), (prec, size)
    net.close()


def test_files(oracle, tmp_path):
    A = require_gpu()
    from takzero_amd import weights as W

    arr = world(oracle)["arr"][:40]
    a = A.Net.new(arch=A.ARCH_NET4_ENSEMBLE, seed=5)
    t = a.tensors()
    assert set(t) == set(W.init_weights(W.ARCH_NET4_ENSEMBLE)) and not np.array_equal(t[R.name(0, "conv2d.weight")], t[R.name(1, "conv2d.weight")])
    want = a.ensemble_values(arr)
    assert want.std(axis=1).min() > 0 and _bits(A.Net.new(arch=A.ARCH_NET4_ENSEMBLE, seed=5).ensemble_values(arr), want)
    assert not _bits(A.Net.new(arch=A.ARCH_NET4_ENSEMBLE, seed=6).ensemble_values(arr), want)
    a.save(tmp_path / "model_latest.ot")
    a.save(tmp_path / "model.tzw")
    for path in ("model_latest.ot", "model.tzw"):
        b = A.Net(arch=A.ARCH_NET4_ENSEMBLE).load(tmp_path / path)
        assert _bits(b.ensemble_values(arr), want), path
        b.close()
    c = a.clone(0)
    assert _bits(c.ensemble_values(arr), want)
    c.close()
    # an archive without head 7: exactly its four names are reported, and the head keeps its values
    shapes = {k: v.shape for k, v in W.init_weights(W.ARCH_NET4_ENSEMBLE).items()}
    other = {k: v.reshape(shapes[k]) for k, v in A.Net.new(arch=A.ARCH_NET4_ENSEMBLE, seed=6).tensors().items()}
    W.save_tzw(tmp_path / "partial.tzw", {k: v for k, v in other.items() if not k.startswith("ensemble head 7.")})
    d = A.Net.new(arch=A.ARCH_NET4_ENSEMBLE, seed=5)
    assert sorted(d.load_partial(tmp_path / "partial.tzw")) == sorted(R.name(7, p) for p in R.PARTS)
    got, six = d.ensemble_values(arr), A.Net.new(arch=A.ARCH_NET4_ENSEMBLE, seed=6).ensemble_values(arr)
    assert _bits(np.delete(got, 7, axis=1), np.delete(six, 7, axis=1)) and not _bits(got[:, 7], six[:, 7])
    # net4_simhash's model into this net: the sixteen heads stay at their initial values
    sim = A.Net.new(arch=A.ARCH_NET4_SIMHASH, seed=8)
    W.save_tzw(tmp_path / "simhash.tzw", sim.tensors())          # (tz_net_save would write the 512 MiB set beside it)
    e = A.Net.new(arch=A.ARCH_NET4_ENSEMBLE, seed=5)
    missing = e.load_partial(tmp_path / "simhash.tzw")
    assert sorted(missing) == sorted(R.names())
    te = e.tensors()
    assert all(_bits(te[k], t[k]) for k in R.names()) and _bits(te["value.linear.weight"], sim.tensors()["value.linear.weight"])
    for name, p, q in zip(("policy", "value", "ube"), e.forward_raw(arr), sim.forward_raw(arr)):
        assert _bits(p, q), name
    # the other architectures refuse the call, and the architecture is 4x4 only
    with pytest.raises(A.TakzeroError):
        sim.ensemble_values(arr)
    with pytest.raises(A.TakzeroError):
        A.Net(arch=A.ARCH_NET4_ENSEMBLE, n=5)
    for net in (a, d, e, sim):
        net.close()
