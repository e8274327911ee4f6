"""Every launch form of the inference forward (net_mfma_kernel / net_c6_kernel behind net_fused_et, tz_nn_launch_split and
tz_nn_launch_c6, and the per-conv / tower kernels behind TZ_TOWER) at the batch sizes that select it, on positions that are all
different, held to two things:

  (a) the integer-valued nets of tests/exact_net.py: policy and UBE equal the fp64 graph (oracle/nets_torch.py, rounded to the grid)
      for every position, in every precision - no tolerance, the arithmetic is exact; the value is the same bits in every precision
      and form and within 1e-4 of fp64 tanh; SimHash nets report a variance of exactly 4 (empty set);
  (b) dense random weights (BatchNorm statistics of a trained net, for the split precisions heads at trained scale): every position
      at the large batch equals, bit for bit, the same position evaluated in chunks of at most 64 through forward_raw (a one-board
      form, which tests/test_gpu_net.py ties to PyTorch within its tolerances).

SIZES sit on both sides of every threshold of the dispatch (csrc/tz_nn.hip): net_small_p (256, 512, 1024), NET_SPLIT_MAX_GROUPS
(64 groups of 1, 2 or 4 boards: 64, 128, 256 on 5x5; 64, 128 on 4x4 and 6x6), `max_positions >= 1024` (6x6 split precisions and
f16c6: 4 boards) and `max_positions >= 2048` (6x6: 8 boards); 4096 positions are the only size with two 5x5 workgroups per CU.
Both entry points reach net_fused with the batch size and so select the same form: the several-CU forms serve forward_raw as well
as policy_value_uncertainty; the one-CU forms below their thresholds run under TZ_NET_SPLIT=0 only and are covered by
test_switched_paths.  Zeros compare equal whatever their sign (the reference rounds -1e-9 to -0)."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import exact_net as E
import oracle_lib as O
from gpu_util import require_gpu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

NETS = E.NETS
SIZES = {5: (1, 7, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 4096, 4099),
         6: (1, 64, 65, 128, 129, 256, 257, 512, 513, 1023, 1024, 1027, 2047, 2048, 2051),
         4: (1, 64, 65, 128, 129, 300, 305, 1030),     # 305: a ragged last workgroup of the 12- and 6-board forms
         3: (1, 64, 65, 128, 129, 300, 307, 1030)}     # 300, 307: ragged for the 16- and 8-board forms
EVAL_UP_TO = {5: 257, 6: 129, 4: 129, 3: 129}          # policy_value_uncertainty: through the several-CU forms and one size past them
PRECS = {"bf16": 0, "f32": 1, "f16": 2, "f16x2": 3, "f16c8": 4, "f16c6": 5}
CASES = [(n, p) for n in (3, 4, 5, 6) for p in PRECS if p != "f16c6" or n in (5, 6)]
SWITCH_SIZES = (1, 37, 1030)
_cache = {}


def _world(oracle, n):
    """Positions (all different), their packed states, encoded planes and legal moves."""
    if ("world", n) not in _cache:
        states = E.distinct_positions(oracle, O, n, max(SIZES[n]), 77)
        arr = O.states_array(states)
        assert len({arr[i:i + 1].tobytes() for i in range(len(arr))}) == len(arr)
        acts = [O.possible_moves(oracle, s) for s in states[:EVAL_UP_TO[n]]]
        calibration = E.planes_of(oracle, O, E.distinct_positions(oracle, O, n, 96, 5), n)
        _cache["world", n] = dict(arr=arr, planes=E.planes_of(oracle, O, states, n), acts=acts, calibration=calibration)
    return _cache["world", n]


def _exact(oracle, n, seed):
    """Weights and fp64 reference of one exact net, computed once per module."""
    if ("exact", n, seed) not in _cache:
        arch, _, blocks = NETS[n]
        world = _world(oracle, n)
        count = len(world["arr"])
        t0 = time.time()
        w = E.exact_weights(arch, n, blocks, seed, world["calibration"])
        ref = E.exact_reference(w, world["planes"][:count], blocks)
        print("exact net %dx%d seed %d: fp64 reference of %d positions in %.1f s, largest activation %d" %
              (n, n, seed, count, time.time() - t0, ref["stats"]["max_activation"]))
        E.assert_reference_is_exact(ref)
        _cache["exact", n, seed] = (w, ref, count)
    return _cache["exact", n, seed]


def _where(got, want):
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    return "no difference" if not len(bad) else "%d differ, first at %s: got %r, want %r" % (
        len(bad), tuple(bad[0]), np.asarray(got)[tuple(bad[0])], np.asarray(want)[tuple(bad[0])])


def _check_exact(tag, out, ref, count, n, seed):
    """out = (policy [B, OUT*N*N], value, ube) of the first `count` positions against the reference; index = (position, channel * N*N + square)."""
    pol, val, ube = out
    assert np.array_equal(pol, ref["policy"][:count]), (tag, "policy", _where(pol, ref["policy"][:count]))
    assert np.array_equal(ube, ref["ube"][:count]), (tag, "ube", _where(ube, ref["ube"][:count]))
    assert np.abs(val.astype(np.float64) - ref["value"][:count]).max() < 1e-4, (tag, "value")
    first = _cache.setdefault(("value bits", n, seed), np.full(len(ref["value"]), np.nan, np.float32))
    fresh = np.isnan(first[:count])
    first[:count][fresh] = val[fresh]
    assert np.array_equal(first[:count].view(np.uint32), val.view(np.uint32)), (tag, "value bits", _where(val, first[:count]))


@pytest.mark.parametrize("n,prec", CASES)
def test_exact_nets_equal_the_fp64_graph_in_every_form(oracle, n, prec):
    A = require_gpu()
    arch, _, blocks = NETS[n]
    world = _world(oracle, n)
    arr, acts = world["arr"], world["acts"]
    for seed in E.SEEDS:
        w, ref, count = _exact(oracle, n, seed)
        net = A.Net(arch=arch, n=n, precision=PRECS[prec], blocks=blocks).load_tensors(w)
        for size in [s for s in SIZES[n] if s <= count]:
            _check_exact((n, prec, seed, size, "forward_raw"), net.forward_raw(arr[:size]), ref, size, n, seed)
            if size <= EVAL_UP_TO[n]:
                for rep in range(2):
                    logits, val, var = net.policy_value_uncertainty(arr[:size], acts[:size])
                    for i in range(size):
                        want = ref["policy"][i, np.asarray(acts[i], np.int64)]
                        assert np.array_equal(logits[i], want), (n, prec, seed, size, rep, "eval logits of position", i, _where(logits[i], want))
                    assert np.abs(val.astype(np.float64) - ref["value"][:size]).max() < 1e-4
                    assert np.array_equal(val.view(np.uint32), _cache["value bits", n, seed][:size].view(np.uint32)), (n, prec, seed, size, rep)
                    if arch in (4, 6):
                        assert np.all(var == 4.0), (n, prec, seed, size, rep)
        net.close()


def _dense_weights(oracle, n, prec):
    from takzero_amd import weights as W
    from test_gpu_net import _trained_scale

    arch, _, blocks = NETS[n]
    w = W.init_weights(arch, n=n, blocks=blocks, seed=9, trained_stats=True)
    if prec in ("f16x2", "f16c8", "f16c6"):
        w = _trained_scale(w, _world(oracle, n)["planes"][:64], blocks)
    return w


@pytest.mark.parametrize("n,prec", CASES)
def test_dense_nets_give_every_position_the_bits_of_the_one_board_form(oracle, n, prec):
    A = require_gpu()
    arch, _, blocks = NETS[n]
    world = _world(oracle, n)
    arr, acts = world["arr"], world["acts"]
    net = A.Net(arch=arch, n=n, precision=PRECS[prec], blocks=blocks).load_tensors(_dense_weights(oracle, n, prec))
    parts = [net.forward_raw(arr[lo:lo + 64]) for lo in range(0, len(arr), 64)]
    base = [np.concatenate([p[k] for p in parts]) for k in range(3)]
    assert all(np.isfinite(b).all() for b in base) and np.abs(base[0]).max() > 0.05
    for size in SIZES[n]:
        out = net.forward_raw(arr[:size])
        for name, x, y in zip(("policy", "value", "ube"), out, base):
            assert np.array_equal(x.view(np.uint32), y[:size].view(np.uint32)), (n, prec, size, name, _where(x, y[:size]))
        if size <= EVAL_UP_TO[n]:
            for rep in range(2):
                logits, val, var = net.policy_value_uncertainty(arr[:size], acts[:size])
                for i in range(size):
                    want = base[0][i, np.asarray(acts[i], np.int64)]
                    assert np.array_equal(logits[i].view(np.uint32), want.view(np.uint32)), (n, prec, size, rep, i)
                assert np.array_equal(val.view(np.uint32), base[1][:size].view(np.uint32)), (n, prec, size, rep)
                if arch in (4, 6):
                    assert np.all(var == 4.0)
    net.close()


# TZ_TOWER=0: conv_mfma_kernel once per conv + heads_kernel, in both tilings (TZ_CONV_CFG); TZ_TOWER=1: tower_mfma_kernel between the
# per-conv first layer and policy conv; TZ_NET_SPLIT=0: the one-CU forms of net_mfma_kernel below the several-CU thresholds.  The
# switches act on the 16-bit storage types only: the f32 path has one form, the split precisions (f16x2, f16c8, f16c6) exist in the fused
# launch alone and ignore TZ_TOWER (tz_net_forward_device).
# TZ_NET_ROWS=board with TZ_NET_P=full: the board-major forms launch_net<3,1,ET,false>, <5,1,ET,false> and <6,2,ET,false> (at 1030 positions;
# the several-CU forms keep the smaller batches).
SWITCHES = [{"TZ_TOWER": "0", "TZ_CONV_CFG": "0"}, {"TZ_TOWER": "0", "TZ_CONV_CFG": "1"}, {"TZ_TOWER": "1"}, {"TZ_NET_SPLIT": "0"},
            {"TZ_NET_ROWS": "board", "TZ_NET_P": "full"}]
# Dense weights against the default path.  All kernels sum tap-major, k-chunk-minor, but conv_mfma_kernel starts its accumulators at zero
# and adds bias, then residual, in its epilogue ("f32x4 v = acc[rt][j] + bias; ... v[k] += (float)rv[k]"), where net_mfma_kernel and
# tower_mfma_kernel start them at residual + bias ("acc[rt][j][k] = (float)xv[k] + b4[k]") and add the products onto that: another order of
# the same sum.  TZ_TOWER=0 runs every conv through conv_mfma_kernel, TZ_TOWER=1 the first and the policy conv, so both give other bits
# (measured: 2e-7 .. 3e-3) and are held to the tolerances of tests/test_gpu_net.py (policy, value, ube).  TZ_NET_SPLIT=0 and the
# board-major rows are the same k-loop per output ("an output does not depend on SPLIT", "what is skipped adds exact zeros",
# csrc/tz_nn.hip) and are held bit for bit.
SWITCH_TOL = {"bf16": (1.2e-2, 5e-3, 5e-3), "f16": (1e-3, 1e-3, 2e-3)}


def _switch_inputs(oracle, A):
    """Once per module: the states and weight files the children read, and this process's default-path outputs on the dense weights."""
    import tempfile

    from takzero_amd import weights as W

    if "switch default" not in _cache:
        _cache["switch tmp"] = tempfile.TemporaryDirectory()
        d = _cache["switch dir"] = _cache["switch tmp"].name
        default = {}
        for n in (3, 4, 5, 6):
            arch, _, blocks = NETS[n]
            world = _world(oracle, n)
            np.save(os.path.join(d, "states_%d.npy" % n), np.frombuffer(world["arr"][:max(SWITCH_SIZES)].tobytes(), np.uint8))
            W.save_tzw(os.path.join(d, "exact_%d.tzw" % n), _exact(oracle, n, 0)[0])
            dense = _dense_weights(oracle, n, "f16")
            W.save_tzw(os.path.join(d, "dense_%d.tzw" % n), dense)
            for prec in SWITCH_TOL:
                net = A.Net(arch=arch, n=n, precision=PRECS[prec], blocks=blocks).load_tensors(dense)
                for size in SWITCH_SIZES:
                    default[n, prec, size] = net.forward_raw(world["arr"][:size])
                net.close()
        _cache["switch default"] = default
    return _cache["switch default"]


@pytest.mark.parametrize("switch", SWITCHES, ids=lambda s: "-".join("%s=%s" % kv for kv in s.items()))
def test_switched_paths(oracle, tmp_path, switch):
    """Each setting in a child process of its own (the switches are read once), board sizes 3 to 6, bf16 and f16, batches 1, 37 and
    1030: the exact nets against the fp64 graph bit for bit, dense weights against this process's default path."""
    A = require_gpu()
    default = _switch_inputs(oracle, A)
    for name in os.listdir(_cache["switch dir"]):
        os.symlink(os.path.join(_cache["switch dir"], name), tmp_path / name)
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "net_forms_child.py"), str(tmp_path)], env=dict(os.environ, **switch),
                           capture_output=True, text=True, timeout=900)
    except subprocess.TimeoutExpired:
        pytest.exit("net_forms_child.py under %r did not finish: nothing more is started on the GPU" % (switch,), returncode=1)
    if r.returncode < 0:
        pytest.exit("net_forms_child.py under %r died on signal %d: nothing more is started on the GPU\n%s" % (switch, -r.returncode, r.stderr[-2000:]),
                    returncode=1)
    assert r.returncode == 0, r.stderr[-3000:]
    for n in (3, 4, 5, 6):
        ref = _exact(oracle, n, 0)[1]
        for prec in SWITCH_TOL:
            got = np.load(tmp_path / ("out_%d_%s.npz" % (n, prec)))
            for size in SWITCH_SIZES:
                out = [got["exact_%d_%d" % (size, k)] for k in range(3)]
                _check_exact((switch, n, prec, size), out, ref, size, n, 0)
                out = [got["dense_%d_%d" % (size, k)] for k in range(3)]
                same = all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(out, default[n, prec, size]))
                err = [float(np.abs(x - y).max()) for x, y in zip(out, default[n, prec, size])]
                print("switch %r %dx%d %s batch %d: dense weights against the default path: %s, max |delta| policy %.3g value %.3g ube %.3g" %
                      (switch, n, n, prec, size, "same bits" if same else "other bits", *err))
                if "TZ_TOWER" not in switch:
                    assert same, (switch, n, prec, size, err)
                assert all(e < t for e, t in zip(err, SWITCH_TOL[prec])), (switch, n, prec, size, err)
