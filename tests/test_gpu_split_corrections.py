"""The correction products wl*xh + wh*xl of TZ_PREC_F16X2, TZ_PREC_F16C8 and TZ_PREC_F16C6 against the CPU emulation of
tests/split_emulation.py (written from DESIGN.md section 4 and the kernels' comments, held to its own conditions by
tests/test_split_emulation_reference.py; no expected value here comes from the library):

  (a) the exact nets with lo parts of tests/exact_net.py (`exact_weights_with_lo`): 64 all-different positions in one forward_raw
      call - the smallest workgroup form of every arithmetic, to which tests/test_gpu_net_forms.py ties every other form bit for
      bit.  Every policy and UBE output that the exactness condition covers (`decided`: no fp32 accumulator it depends on can round,
      in any order, see tests/exact_net.py `assert_reference_is_exact`) must equal the emulation in every bit (zeros of either sign
      equal).  That is 59 .. 100 % of the policy (f16c6 59 .. 89 %, f16x2 89 .. 99 %, f16c8 95 .. 100 %).  The heads add 16 channels
      on every square, so few of their outputs are decided: 0 .. 56 % of the UBE and 1.6 .. 59 % of the value outputs (f16x2: 0 to 3
      of 64 positions on 4x4, 5x5 and 6x6) - the UBE is NOT compared bit for bit as a whole, and what the heads read is held by (b)
      and by the head-side fault of tests/test_split_emulation_reference.py.  Every other output must lie within 8 D of the fp64
      emulation, D computed in the test as in (b) on the same net (and at least one fp32 step at the largest output); the value
      within 1e-4 of tanh of the emulated pre-activation; then 7 positions through policy_value_uncertainty against the same
      numbers and, bit for bit, against forward_raw;
  (b) dense random weights with trained BatchNorm statistics and heads at trained scale (`_dense_weights` of
      tests/test_gpu_net_forms.py), where every FP8 / E2M3 scale, cap and remainder byte works in its real range: the kernel must
      lie within 8 D of the fp64 emulation, D the largest difference (per output) between the emulation with fp64 sums and with
      torch's fp32 sums on the same rounded operands - the size of the only effect that separates a correct kernel from the fp64
      emulation (fp32 summation in some order and the storage-rounding flips it causes).  The 8 is for the kernel's summation
      order, which is neither torch's nor fp64's.  Nothing here is a recorded number; D and the distances are printed.

Measured on an MI355X (DESIGN.md section 4 has the table): (a) every decided output equal in all 20 cases, the others off by at most
two fp32 steps (9.5e-7 on the policy, 2.5e-7 on the UBE) but for one case with a flipped lo byte (5x5 f16c8 seed 0: 1.2e-4, one E4M3
step, where D is 1.2e-4 as well); (b) kernel / D between 0.6 and 3.8 - policy D 2.0e-6 .. 3.3e-6 and kernel
6.7e-6 .. 9.5e-6 for f16x2, D 2.1e-5 .. 4.2e-5 and kernel 3.2e-5 .. 5.1e-5 for f16c8 / f16c6; value D 1.0e-7 .. 1.6e-6, kernel 2.0e-7 .. 9.3e-7;
UBE D 1.2e-7 .. 1.6e-5, kernel 3.6e-7 .. 2.8e-5.  Dropping either correction product moves the emulation's logits by 2e-3."""
import os
import sys

import numpy as np
import pytest

import exact_net as E
import oracle_lib as O
import split_emulation as M
from gpu_util import require_gpu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

PRECS = {"f16x2": 3, "f16c8": 4, "f16c6": 5}
EXACT_CASES = [(n, p, s) for n in (5, 6, 3, 4) for p in E.LO_ARITHMETICS[n] for s in E.LO_SEEDS]
DENSE_NETS = {5: (100, 5, 3), 6: (100, 6, 2), 4: (100, 4, 2)}
DENSE_CASES = [(5, "f16x2"), (5, "f16c8"), (5, "f16c6"), (6, "f16x2"), (6, "f16c8"), (6, "f16c6"), (4, "f16x2"), (4, "f16c8")]
MARGIN = 8.0
DENSE_SEED = 10          # a seed with which both heads are alive on every board size (seed 9 of the forms test leaves the UBE head's ReLU dead on 5x5 and 6x6)
_cache = {}


def _world(oracle, n):
    if n not in _cache:
        states = E.distinct_positions(oracle, O, n, E.LO_POSITIONS, E.LO_POSITION_SEED)
        _cache[n] = dict(arr=O.states_array(states), planes=E.planes_of(oracle, O, states, n), acts=[O.possible_moves(oracle, s) for s in states[:7]],
                         calibration=E.planes_of(oracle, O, E.distinct_positions(oracle, O, n, 96, E.LO_CALIBRATION_SEED), n))
    return _cache[n]


def _where(got, want):
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    return "no difference" if not len(bad) else "%d of %d differ, first at %s: got %r, want %r, largest |difference| %.3g" % (
        len(bad), np.asarray(got).size, tuple(bad[0]), np.asarray(got)[tuple(bad[0])], np.asarray(want)[tuple(bad[0])],
        float(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).max()))


@pytest.mark.parametrize("n,prec,seed", EXACT_CASES)
def test_exact_nets_with_lo_parts_equal_the_emulation_wherever_no_accumulator_can_round(oracle, n, prec, seed):
    A = require_gpu()
    arch, _, blocks = E.LO_NETS[n]
    world = _world(oracle, n)
    w = E.exact_weights_with_lo(arch, n, blocks, seed, world["calibration"])
    ref = M.emulate(prec, w, world["planes"], blocks, stats=True)
    E.assert_reference_is_exact(ref)
    e32 = M.emulate(prec, w, world["planes"], blocks, accumulate="fp32")
    net = A.Net(arch=arch, n=n, precision=PRECS[prec], blocks=blocks).load_tensors(w)
    pol, val, ube = net.forward_raw(world["arr"])
    dec = ref["decided"]
    got = dict(policy=pol, ube=ube)
    D, dist = {}, {}
    for k in got:
        want = ref[k].astype(np.float64)
        # the emulation with fp32 sums against the one with fp64 sums, and never less than one fp32 step at the largest output: torch's
        # order of the sums can happen to be exact where another order rounds once
        D[k] = max(float(np.abs(want - e32[k]).max()), float(np.spacing(np.float32(np.abs(want).max()))))
        dist[k] = float(np.abs(got[k].astype(np.float64) - want).max())
        assert np.array_equal(e32[k][dec[k]], ref[k][dec[k]]), (n, prec, seed, k, "the fp32 sums reach a decided output")
    print("exact net with lo parts %dx%d %s seed %d: decided share policy %.3f value %.3f ube %.3f; decided policy: %s; all policy: %s (D %.3g); ube: %s (D %.3g); value off by %.3g" %
          (n, n, prec, seed, dec["policy"].mean(), dec["value"].mean(), dec["ube"].mean(), _where(np.where(dec["policy"], pol, 0), np.where(dec["policy"], ref["policy"], 0)),
           _where(pol, ref["policy"]), D["policy"], _where(ube, ref["ube"]), D["ube"], float(np.abs(val.astype(np.float64) - ref["value"]).max())))
    for k in got:
        # the outputs the exactness condition covers: every bit (== : zeros of either sign are equal); the others: within 8 D, as the dense nets
        assert np.array_equal(got[k][dec[k]], ref[k][dec[k]]), (n, prec, seed, k, _where(np.where(dec[k], got[k], 0), np.where(dec[k], ref[k], 0)))
        assert dist[k] <= MARGIN * D[k], (n, prec, seed, k, dist[k], D[k])
    assert np.abs(val.astype(np.float64) - ref["value"]).max() < 1e-4, (n, prec, seed, "value")
    logits, val7, _ = net.policy_value_uncertainty(world["arr"][:7], world["acts"])
    for i in range(7):
        idx = np.asarray(world["acts"][i], np.int64)
        want, d = ref["policy"][i, idx], dec["policy"][i, idx]
        assert np.array_equal(logits[i][d], want[d]), (n, prec, seed, "eval logits of position", i, _where(logits[i], want))
        assert np.array_equal(logits[i].view(np.uint32), pol[i, idx].view(np.uint32)), (n, prec, seed, "eval logits against forward_raw", i)
    assert np.abs(val7.astype(np.float64) - ref["value"][:7]).max() < 1e-4
    net.close()


def _dense_weights(oracle, n, blocks):
    """As tests/test_gpu_net_forms.py makes them for the split precisions: random weights, BatchNorm statistics of a trained net,
    heads rescaled to max |logit| = 8, value pre-activation 1.5, |ube| 2 on the tested positions."""
    from takzero_amd import weights as W
    from test_gpu_net import _trained_scale

    w = W.init_weights(100, n=n, blocks=blocks, seed=DENSE_SEED, trained_stats=True)
    return _trained_scale(w, _world(oracle, n)["planes"], blocks)


@pytest.mark.parametrize("n,prec", DENSE_CASES)
def test_dense_nets_lie_within_the_fp32_summation_effect_of_the_emulation(oracle, n, prec):
    A = require_gpu()
    arch, _, blocks = DENSE_NETS[n]
    world = _world(oracle, n)
    w = _dense_weights(oracle, n, blocks)
    e64 = M.emulate(prec, w, world["planes"], blocks)
    e32 = M.emulate(prec, w, world["planes"], blocks, accumulate="fp32")
    net = A.Net(arch=arch, n=n, precision=PRECS[prec], blocks=blocks).load_tensors(w)
    pol, val, ube = net.forward_raw(world["arr"])
    net.close()
    got = dict(policy=pol, value=val, ube=ube)
    assert all(np.isfinite(v).all() for v in got.values()) and 7.0 < np.abs(e64["policy"]).max() < 9.0
    assert np.ptp(e64["value"]) > 0.02 and np.ptp(e64["ube"]) > 0.02                          # both heads alive
    D = {k: float(np.abs(e64[k].astype(np.float64) - e32[k].astype(np.float64)).max()) for k in got}
    dist = {k: float(np.abs(got[k].astype(np.float64) - e64[k].astype(np.float64)).max()) for k in got}
    print("dense %dx%d %s: D (fp64 against fp32 sums) policy %.3g value %.3g ube %.3g; kernel against the fp64 emulation policy %.3g value %.3g ube %.3g" %
          (n, n, prec, D["policy"], D["value"], D["ube"], dist["policy"], dist["value"], dist["ube"]))
    for k in got:
        assert D[k] > 0.0, (n, prec, k, "the two emulations agree in every bit: the positions do not exercise the sums")
        assert dist[k] <= MARGIN * D[k], (n, prec, k, dist[k], D[k])
