"""The fixture net4_rnd's kernel is measured on (tests/test_rnd4_ref.py asserts its coverage, tests/test_gpu_rnd4.py runs it): 1025
different 4x4 positions from the oracle's random playouts, a dense net with non-trivial BatchNorm statistics and LayerNorm affines,
`min` / `max` at the 10th / 90th percentile of the fp64 raw values, and the UBE head forced to the constant c = ln(median local value
among the positions inside (0, 4)), so that both clamp ends, the inside, and both winners of max(exp(ube), local) occur.

Tolerances, all measured here on the CPU:
  raw_tol      8 x max |fp32-accumulating emulation - fp64-accumulating emulation| (the factor of tests/test_gpu_split_corrections.py
               for a maximum over about a thousand positions of rounding-boundary crossings); the kernel's raw against "emu64"
  emu_dist     max |emu64 - plain fp64|
  var_tol      4 / (max - min) x (raw_tol + emu_dist); the kernel's variance against the fp64 variance
  raw_tol_f32  8 x max |plain fp32 - plain fp64|, var_tol_f32 = 4 / (max - min) x raw_tol_f32: the same for TZ_PREC_F32"""
import numpy as np

import exact_net as E
import oracle_lib as O
import rnd4_ref as R

POSITIONS, SEED = 1025, 34
_cache = {}


def weights(seed=11):
    from takzero_amd import weights as W

    w = W.init_weights(W.ARCH_NET4_RND, seed=seed, trained_stats=True)
    rng = np.random.default_rng(seed)
    for t in R.TOWERS:
        w[t + ".layer_norm.weight"] = rng.normal(1, 0.2, size=(28, 4, 4)).astype(np.float32)
        w[t + ".layer_norm.bias"] = rng.normal(0, 0.2, size=(28, 4, 4)).astype(np.float32)
    return w


def fixture(oracle):
    if "fx" not in _cache:
        states = E.distinct_positions(oracle, O, 4, POSITIONS, SEED)
        planes = E.planes_of(oracle, O, states, 4).astype(np.float64)
        w = weights()
        raw64, emu64, emu32, f32 = (R.raw(w, planes, m).astype(np.float64) for m in ("f64", "emu64", "emu32", "f32"))
        lo, hi = np.float32(np.percentile(raw64, 10)), np.float32(np.percentile(raw64, 90))
        loc = R.local(raw64, lo, hi)
        inside = (loc > 0) & (loc < 4)
        c = np.float32(np.log(np.median(loc[inside])))
        w["ube.linear.weight"] = np.zeros_like(w["ube.linear.weight"])
        w["ube.linear.bias"] = np.array([c], np.float32)
        raw_tol, emu_dist = 8 * float(np.abs(emu32 - emu64).max()), float(np.abs(emu64 - raw64).max())
        raw_tol_f32 = 8 * float(np.abs(f32 - raw64).max())
        gain = 4.0 / (float(hi) - float(lo))
        _cache["fx"] = dict(states=states, arr=O.states_array(states), planes=planes, w=w, raw64=raw64, emu64=emu64, min=lo, max=hi, c=c, local=loc,
                            raw_tol=raw_tol, emu_dist=emu_dist, var_tol=gain * (raw_tol + emu_dist), raw_tol_f32=raw_tol_f32, var_tol_f32=gain * raw_tol_f32)
    return _cache["fx"]


def with_range(w, lo, hi):
    return dict(w, min=np.array([lo], np.float32), max=np.array([hi], np.float32))
