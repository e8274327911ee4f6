"""The LCG hash of net4_lcghash (net4_lcghash.rs:202-242) without a GPU: tests/lcghash_ref.py, the numpy reference the GPU tests
compare the kernel with, against two other statements of the same function -

  * `transcribed_get_indices`: get_indices line by line in torch on the CPU (split, in-place int64 `*=` / `+=`, squeeze, abs, shift);
  * `closed_form`: H = K + sum v[c][r][f] * M**((27-c) + (3-r) + (3-f)) modulo 2**64 in Python's integers, K = the increments alone -

on random planes, real positions, products that are all -0.0, batch size 1 and subnormal products.  All three must agree on every
index: integer arithmetic modulo 2**64 leaves no room for a tolerance.  Then the pieces around it that need no GPU: the new variable
in init_weights and in `.ot` files, and the arch constant."""
import os
import re

import numpy as np
import pytest

import lcghash_ref as R
import oracle_lib as O
from gpu_util import random_positions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C4, N4 = 28, 4


def transcribed_get_indices(xs, init):
    """get_indices, net4_lcghash.rs:202-242, statement by statement."""
    import torch

    MULTIPLIER, INCREMENT, HASH_BITS = 6_364_136_223_846_793_005, 1, 32
    xs, init = torch.from_numpy(np.ascontiguousarray(xs, np.float32)), torch.from_numpy(np.ascontiguousarray(init, np.float32))
    batch_size, channels, rows, _cols = xs.shape
    parts = (xs * init).view(torch.int32).split(1, 3)
    acc = torch.zeros([batch_size, channels, rows], dtype=torch.int64)
    for x in parts:
        acc *= MULTIPLIER
        acc += INCREMENT
        acc += x.squeeze()
    parts = acc.split(1, 2)
    acc = torch.zeros([batch_size, channels], dtype=torch.int64)
    for x in parts:
        acc *= MULTIPLIER
        acc += INCREMENT
        acc += x.squeeze()
    parts = acc.split(1, 1)
    acc = torch.zeros([batch_size], dtype=torch.int64)
    for x in parts:
        acc *= MULTIPLIER
        acc += INCREMENT
        acc += x.squeeze()
    out = []
    for x in acc.tolist():
        a = x if x >= 0 else (-x if x != -2 ** 63 else x)        # i64::abs in a release build wraps at MIN
        out.append((a >> (63 - HASH_BITS)) & 0xFFFFFFFF)         # the engine's mask; a no-op unless x is MIN
    return np.array(out, np.uint64).astype(np.uint32)


def closed_form(xs, init):
    """The chains unrolled, in Python integers reduced modulo 2**64 once per position."""
    v = R.product_bits(xs, init)
    B, Cn, Rn, Fn = v.shape
    M, MOD = R.MULTIPLIER, 1 << 64
    K = (sum(pow(M, Cn - 1 - c, MOD) for c in range(Cn))
         + sum(pow(M, (Cn - 1 - c) + (Rn - 1 - r), MOD) for c in range(Cn) for r in range(Rn))
         + sum(pow(M, (Cn - 1 - c) + (Rn - 1 - r) + (Fn - 1 - f), MOD) for c in range(Cn) for r in range(Rn) for f in range(Fn)))
    out = []
    for b in range(B):
        h = K
        for c in range(Cn):
            for r in range(Rn):
                for f in range(Fn):
                    h += int(v[b, c, r, f]) * pow(M, (Cn - 1 - c) + (Rn - 1 - r) + (Fn - 1 - f), MOD)
        h %= MOD
        if h >= 1 << 63:
            h -= MOD                                              # as int64
        a = abs(h) if h != -(1 << 63) else h
        out.append((a >> 31) & 0xFFFFFFFF)
    return np.array(out, np.uint64).astype(np.uint32)


def all_three(xs, init):
    ref = R.indices(xs, init)
    assert ref.dtype == np.uint32 and ref.shape == (len(xs),)
    assert np.array_equal(ref, transcribed_get_indices(xs, init))
    assert np.array_equal(ref, closed_form(xs, init))
    return ref


def planes_of(oracle, states, n=4):
    return np.stack([O.game_repr(oracle, s) for s in states]).reshape(len(states), -1, n, n)


def test_random_planes():
    rng = np.random.default_rng(1)
    xs = rng.normal(0, 3, size=(64, C4, N4, N4)).astype(np.float32)
    xs[rng.random(xs.shape) < 0.5] = 0.0
    init = rng.uniform(-100, 100, size=(C4, N4, N4)).astype(np.float32)
    ref = all_three(xs, init)
    assert len(set(ref.tolist())) == 64 and (ref >= 2 ** 31).any() and (ref < 2 ** 31).any()
    # another board shape: the chains follow the tensor's dimensions, nothing is fixed to 4x4
    all_three(rng.normal(size=(5, 3, 2, 6)).astype(np.float32), rng.normal(size=(3, 2, 6)).astype(np.float32))


def test_real_positions(oracle):
    from takzero_amd import weights as W

    states = random_positions(oracle, O, 4, 4, 96, 7, max_ply=50) + [O.state_default(oracle, 4, 4)]
    xs = planes_of(oracle, states)
    assert xs.shape[1:] == (C4, N4, N4)
    init = W.init_weights(W.ARCH_NET4_LCGHASH, seed=3)["lcghash_init"]
    ref = all_three(xs, init)
    assert xs[:, C4 - 2].min() == 0.0 and xs[:, C4 - 2].max() == 1.0        # both colours to move ...
    other = xs.copy()
    other[:, C4 - 2] = 1.0 - other[:, C4 - 2]
    assert np.all(R.indices(other, init) != ref)                            # ... and the colour plane is hashed, unlike SimHash's


def test_every_product_is_minus_zero():
    """An all-zero position tensor under a negative init: every product is -0.0, bits 0x80000000, value -2**31 - a hash that skipped
    zero planes, or tested x != 0 before multiplying, would see zeros."""
    xs = np.zeros((3, C4, N4, N4), np.float32)
    init = -np.random.default_rng(2).uniform(1, 100, size=(C4, N4, N4)).astype(np.float32)
    assert np.all(R.product_bits(xs, init) == -2 ** 31)
    ref = all_three(xs, init)
    assert len(set(ref.tolist())) == 1
    assert ref[0] != all_three(xs, -init)[0]                                 # +0.0 everywhere is another index


def test_batch_of_one(oracle):
    """squeeze() drops the batch dimension too when it is 1: the in-place adds broadcast it back."""
    rng = np.random.default_rng(3)
    init = rng.uniform(-100, 100, size=(C4, N4, N4)).astype(np.float32)
    xs = planes_of(oracle, random_positions(oracle, O, 4, 4, 4, 9, max_ply=30))
    full = all_three(xs, init)
    for i in range(4):
        assert all_three(xs[i:i + 1], init)[0] == full[i]


def subnormal_init(seed=4):
    """An init whose products with the reserve ratios (channels 22 and 24 on 4x4: k / 15) and with the flat-difference plane (27) are
    subnormal: 1e-38 * 14/15 lies below the smallest normal fp32, and 1e-39 is subnormal itself."""
    init = np.random.default_rng(seed).uniform(-100, 100, size=(C4, N4, N4)).astype(np.float32)
    init[22] = np.float32(1e-38)
    init[24] = np.float32(-1e-38)
    init[27] = np.float32(1e-39)
    return init


def test_subnormal_products(oracle):
    init = subnormal_init()
    states = random_positions(oracle, O, 4, 4, 32, 11, min_ply=4, max_ply=40)
    xs = planes_of(oracle, states)
    p = R.products(xs, init)
    tiny = np.float32(np.finfo(np.float32).tiny)
    sub = (p != 0) & (np.abs(p) < tiny)
    assert sub[:, 22].all() and sub[:, 24].all() and sub[:, 27].any(), "the fixture's products are not subnormal"
    ref = all_three(xs, init)
    flushed = np.where(sub, np.copysign(np.float32(0), p), p)               # what a flush-to-zero multiply would give
    assert np.all(R.shift(R._chain(R._chain(R._chain(flushed.view(np.int32).astype(np.int64))))) != ref)


def test_shift_edges():
    h = np.array([0, 1, -1, 2 ** 31, -2 ** 31, 2 ** 63 - 1, -2 ** 63 + 1, -2 ** 63], np.int64)
    assert R.shift(h).tolist() == [0, 0, 0, 1, 1, 2 ** 32 - 1, 2 ** 32 - 1, 0]


def test_elements_of_one_anti_diagonal_are_interchangeable():
    """The weight of an element depends on the sum of its reversed indices only: under a constant init, moving a value along an
    anti-diagonal (in any two of the three dimensions) keeps the index; moving it off the anti-diagonal changes it."""
    init = np.full((C4, N4, N4), -3.0, np.float32)
    xs = np.zeros((4, C4, N4, N4), np.float32)
    xs[0, 5, 1, 2] = 1.0
    xs[1, 5, 2, 1] = 1.0      # r + f the same
    xs[2, 6, 1, 1] = 1.0      # c + r + f the same
    xs[3, 5, 2, 2] = 1.0      # not
    ref = all_three(xs, init)
    assert ref[0] == ref[1] == ref[2] != ref[3]


def test_seen_set():
    s = R.SeenSet()
    assert s.local([1, 2 ** 32 - 1]).tolist() == [4.0, 4.0]
    s.update(np.array([2 ** 32 - 1, 33], np.uint32))
    assert s.local([1, 2 ** 32 - 1, 33]).tolist() == [4.0, 0.0, 0.0] and s.sorted().tolist() == [33, 2 ** 32 - 1]


def test_init_weights_has_the_variable():
    from takzero_amd import weights as W

    w = W.init_weights(W.ARCH_NET4_LCGHASH, seed=3)
    t = w["lcghash_init"]
    assert t.shape == (C4, N4, N4) and t.dtype == np.float32
    assert t.min() >= -100.0 and t.max() < 100.0 and t.min() < -90 and t.max() > 90 and (t < 0).sum() > 150 and (t > 0).sum() > 150
    assert "simhash_matrix" not in w
    # the trunk and the heads are those of net4_simhash (net4_lcghash.rs:39-118): the same variables, the same shapes
    s = W.init_weights(W.ARCH_NET4_SIMHASH, seed=3)
    assert {k: v.shape for k, v in w.items() if k != "lcghash_init"} == {k: v.shape for k, v in s.items() if k != "simhash_matrix"}
    assert W.arch_board(W.ARCH_NET4_LCGHASH) == 4 and W.arch_blocks(W.ARCH_NET4_LCGHASH) == 16
    assert not np.array_equal(t, W.init_weights(W.ARCH_NET4_LCGHASH, seed=4)["lcghash_init"])


def test_arch_constant_has_one_value_everywhere():
    from takzero_amd import api as A
    from takzero_amd import weights as W

    header = open(os.path.join(ROOT, "include", "takzero_hip.h")).read()
    archs = {k: int(v) for k, v in re.findall(r"^#define\s+(TZ_ARCH_\w+)\s+(\d+)\s*$", header, flags=re.M)}
    value = archs["TZ_ARCH_NET4_LCGHASH"]
    assert list(archs.values()).count(value) == 1, archs
    assert A.ARCH_NET4_LCGHASH == W.ARCH_NET4_LCGHASH == value
    sys_rs = open(os.path.join(ROOT, "bindings", "takzero-hip-sys", "src", "lib.rs")).read()
    assert re.findall(r"pub const TZ_ARCH_NET4_LCGHASH: c_int = (\d+);", sys_rs) == [str(value)]


@pytest.fixture(scope="module")
def ot_writer():
    from takzero_amd import ot

    try:
        return ot.build_writer()
    except RuntimeError as e:
        pytest.skip(str(e))


def _small_lcg_store():
    """A store with the LCG net's variable names at a size that keeps the archive small: ARCH_TEST's trunk on 4x4 + lcghash_init."""
    from takzero_amd import weights as W

    w = W.init_weights(W.ARCH_TEST, n=4, blocks=1, seed=5, trained_stats=True)
    w["lcghash_init"] = subnormal_init(6)          # subnormals and negatives must survive the file
    return w


def test_ot_native_writer_against_libtorchs_reader(tmp_path):
    from takzero_amd import ot

    w = _small_lcg_store()
    path = ot.save_ot(tmp_path / "model_latest.ot", w)
    named = ot.read_ot_libtorch(path)
    assert list(named) == [n for n, _ in ot.tch_names(w)] and list(named)[-1] == "lcghash_init"     # created last, net4_lcghash.rs:131
    assert named["lcghash_init"].shape == (C4, N4, N4)
    assert named["lcghash_init"].view(np.uint32).tolist() == w["lcghash_init"].view(np.uint32).tolist()
    back = ot.load_ot(path)
    assert set(back) == set(w) and all(np.array_equal(back[k].view(np.uint32), np.asarray(w[k], np.float32).view(np.uint32)) for k in w)


def test_ot_native_reader_against_libtorchs_writer(ot_writer, tmp_path):
    from takzero_amd import ot

    w = _small_lcg_store()
    path = ot.save_ot_libtorch(tmp_path / "model_latest.ot", w)
    back = ot.load_ot(path)
    assert set(back) == set(w) and back["lcghash_init"].shape == (C4, N4, N4)
    assert all(np.array_equal(back[k].view(np.uint32), np.asarray(w[k], np.float32).view(np.uint32)) for k in w)
    # and through the other container
    from takzero_amd import weights as W

    again = W.loads_tzw(W.dumps_tzw(w))
    assert again["lcghash_init"].shape == (C4, N4, N4) and np.array_equal(again["lcghash_init"].view(np.uint32), w["lcghash_init"].view(np.uint32))
