"""net4_lcghash on the device against the numpy reference of its hash (tests/lcghash_ref.py, held to two other statements of
get_indices in tests/test_lcghash_ref.py): indices, the set, the variance, the files, the searches, the learn loop.

The hash is integer arithmetic modulo 2**64 on the bit patterns of fp32 products of one multiply each, so nothing here has a
tolerance and no position is left out: every index of every position must equal the reference's in every bit.  With
ube.linear.weight = 0 and ube.linear.bias = c the variance of a position is one of two exactly known numbers, 4 (unseen) or
clamp(expf(c), 0, 4) (seen), the latter held to rtol 1e-6 (test_gpu_uncertainty.sharp_check's bound on expf) as in
tests/test_gpu_simhash.py; the searches use c = 0, where expf(c) = 1 exactly, so that the oracle search can be handed the
reference's variance and compared in every byte.  The expected set is always built from the reference's indices."""
import ctypes as C
import os

import numpy as np
import pytest

import lcghash_ref as R
import oracle_lib as O
from gpu_util import random_positions, require_gpu

MAXIMUM_VARIANCE = np.float32(4.0)
COUNT = 2051
BPW = 4                                   # boards per workgroup of lcghash_state_kernel, one wave each
# one position, the tails of a workgroup on either side, the SimHash test's sizes, many workgroups with a tail of 3
BATCHES = (1, BPW - 1, BPW, BPW + 1, 7, 8, 9, 63, 64, 65, COUNT)
# policy_value_uncertainty: the sizes above that sit on either side of the Agent surface's small-batch forms (64 and 128 groups on
# 4x4, tests/test_gpu_net_forms.py) and the full-batch form
EVAL_BATCHES = (1, BPW, BPW + 1, 63, 64, 65, 128, 129, 300, COUNT)
# (source, copy) slots of exact duplicates, each pair in two different workgroups; (2, 8) lies inside the 9-position batch
DUPLICATES = ((2, 8), (3, 1000), (17, 2050), (63, 64), (500, 1501))
START_SLOTS = (5, 2047)
EXHAUSTED_SLOTS = (11, 1203)              # a reserve ratio of 0: positions whose side to move / other side has no stones left
UBE_CONSTANTS = (float(np.float32(np.log(0.5))), -20.0, 2.0)      # exp(c) = 0.5; 2e-9, still > 0; above the clamp at 4
PRECISIONS = ("f32", "f16", "bf16", "f16x2", "f16c8")              # those of net4_simhash
C4, N4 = 28, 4

_FIXTURE = {}


def planes_of(oracle, states):
    return np.stack([O.game_repr(oracle, s) for s in states]).reshape(len(states), C4, N4, N4)


def _without_stones(oracle, s, side):
    """`s` with the reserve of one side emptied: a position the rules end, but the hash (and the net) is asked about whatever it is given."""
    t = O.TzState.from_buffer_copy(bytes(s))
    t.stones[side] = 0
    return t


def lcg_fixture(oracle):
    """The shipped net4_lcghash (init_weights, seed 3) with 2051 positions of every stage of a game, exact duplicates in different
    workgroups, the start position and two positions with an exhausted reserve; their planes, reference indices and the half chosen
    to be marked as seen.  Asserts its own coverage with the reference alone and prints the figures."""
    if _FIXTURE:
        return _FIXTURE
    from takzero_amd import weights as W

    w = W.init_weights(W.ARCH_NET4_LCGHASH, seed=3)
    states = random_positions(oracle, O, 4, 4, COUNT, 5, max_ply=60)
    for at, side in zip(EXHAUSTED_SLOTS, (0, 1)):
        states[at] = _without_stones(oracle, states[at], side)
    for src, dst in DUPLICATES:
        assert src // BPW != dst // BPW
        states[dst] = states[src]
    for at in START_SLOTS:
        states[at] = O.state_default(oracle, 4, 4)
    planes = planes_of(oracle, states)
    init = w["lcghash_init"]
    assert init.shape == planes.shape[1:] == (C4, N4, N4)
    ref = R.indices(planes, init)
    keys = np.array([planes[i].tobytes() for i in range(COUNT)], dtype=object)
    slots = np.arange(COUNT)
    chosen = slots % 2 == 0
    seen = np.isin(ref, ref[chosen])
    seen_indices = np.unique(ref[chosen])
    plies = np.array([s.ply for s in states])
    to_move, ratios, komi = planes[:, 26, 0, 0], planes[:, [22, 24], 0, 0], planes[:, 27, 0, 0]
    dyadic = ratios * 16 == np.round(ratios * 16)
    top = float((ref >= 2 ** 31).mean())
    distinct_positions, distinct_indices = len(set(keys)), len(set(ref.tolist()))
    print("4x4 LCG hash: %d positions, %d distinct -> %d distinct indices; index >= 2^31 on %.1f %%; black to move on %.1f %%; "
          "%d reserve ratios of 0, %d not dyadic; flat-difference plane negative on %d, positive on %d; %d seen / %d unseen" %
          (COUNT, distinct_positions, distinct_indices, 100 * top, 100 * float(to_move.mean()), int((ratios == 0).sum()), int((~dyadic).sum()),
           int((komi < 0).sum()), int((komi > 0).sum()), int(seen.sum()), int((~seen).sum())))
    assert set(np.unique(to_move).tolist()) == {0.0, 1.0} and 0.3 <= to_move.mean() <= 0.7         # both colours to move
    assert (ratios[list(EXHAUSTED_SLOTS)] == 0).sum() == 2 and (~dyadic).sum() >= 1000              # ratio 0; k / 15 in most positions
    assert (komi < 0).sum() >= 100 and (komi > 0).sum() >= 100                                      # the start position's is -2 / 16
    assert 0.3 <= top <= 0.7                                                                        # the top bit takes part in index >> 5
    assert np.bincount(plies // 10, minlength=6)[:6].min() >= 100                                   # every stage: plies 0-9 ... 50-59
    assert seen.sum() >= 900 and (~seen).sum() >= 900
    for src, dst in DUPLICATES:
        assert ref[src] == ref[dst] and keys[src] == keys[dst]
    assert ref[START_SLOTS[0]] == ref[START_SLOTS[1]]
    # 2051 positions in 2**32 slots do not collide under a uniform init (the fixture says so if they ever do): the pair of distinct
    # positions with one index comes from the anti-diagonal property under a constant init, see collision_fixture
    assert distinct_positions - distinct_indices >= 0
    _FIXTURE.update(w=w, init=init, states=states, arr=O.states_array(states), acts=[O.possible_moves(oracle, s) for s in states], planes=planes,
                    ref=ref, keys=keys, chosen=chosen, seen=seen, seen_indices=seen_indices, collisions=distinct_positions - distinct_indices)
    return _FIXTURE


def collision_fixture(oracle):
    """Sixteen positions that differ in where one flat lies, hashed under a constant init: the weight of an element depends on the sum
    of its reversed indices only, so two of them share an index exactly where the flat stays on one anti-diagonal.  Returns the
    states, their array, the init and the reference indices; asserts that there are colliding and non-colliding pairs."""
    base = O.state_default(oracle, 4, 4)
    moves = O.possible_moves(oracle, base)
    states = [O.play(oracle, base, m) for m in moves]           # the first ply of a game: one flat on each of the 16 squares
    assert len(states) == 16
    planes = planes_of(oracle, states)
    assert len({planes[i].tobytes() for i in range(16)}) == 16
    init = np.full((C4, N4, N4), -7.25, np.float32)              # negative as well: every zero plane contributes -0.0
    ref = R.indices(planes, init)
    assert len(set(ref.tolist())) == 7, ref                      # the 7 anti-diagonals of a 4x4 board
    return states, O.states_array(states), init, ref


def constant_ube(w, c):
    w = dict(w)
    w["ube.linear.weight"] = np.zeros_like(w["ube.linear.weight"])
    w["ube.linear.bias"] = np.full(1, c, np.float32)
    return w


def seen_variance(c):
    return min(float(np.exp(np.float64(np.float32(c)))), 4.0)


def check_variances(var, c, seen, label):
    """Every variance against the two exactly known numbers."""
    seen = np.asarray(seen, bool)
    assert var.shape == seen.shape and np.all(np.isfinite(var)), label
    wrong = np.flatnonzero(~seen & (var != MAXIMUM_VARIANCE))
    assert wrong.size == 0, (label, "unseen positions below 4", wrong[:8], var[wrong[:8]])
    want = seen_variance(c)
    if want == 4.0:
        wrong = np.flatnonzero(seen & (var != MAXIMUM_VARIANCE))
    else:
        wrong = np.flatnonzero(seen & ~(np.isclose(var, want, rtol=1e-6, atol=0) & (var > 0)))
    assert wrong.size == 0, (label, "seen positions off %r" % want, wrong[:8], var[wrong[:8]])


def insert_chosen(net, f):
    """update_counts on the chosen half in three calls: all of them in the order of their reference indices (neighbours in the set side
    by side, a ragged last workgroup), every third one again, forty of them twice within one batch."""
    slots = np.flatnonzero(f["chosen"])
    calls = [slots[np.argsort(f["ref"][slots], kind="stable")], slots[::3], np.repeat(slots[:40], 2)]
    got = [net.hash_indices(f["arr"][c], update=True) for c in calls]
    return np.concatenate(calls), np.concatenate(got)


def set_bits_of_file(path):
    """Indices of the set bits of a bitvec.bin in the layout of BitBox<usize, Lsb0> on a little-endian host: bit i in byte i >> 3, bit i & 7."""
    mm = np.memmap(path, dtype=np.uint8, mode="r")
    assert mm.shape == (1 << 29,)
    out = []
    for lo in range(0, 1 << 29, 1 << 26):
        for i in np.flatnonzero(mm[lo:lo + (1 << 26)]):
            byte = int(mm[lo + i])
            out.extend(((lo + int(i)) << 3) + b for b in range(8) if byte >> b & 1)
    del mm
    return np.array(sorted(out), dtype=np.uint64)


def write_bits_file(path, indices):
    mm = np.memmap(path, dtype=np.uint8, mode="w+", shape=(1 << 29,))
    for i in np.unique(np.asarray(indices)).astype(np.uint64):
        mm[int(i) >> 3] |= np.uint8(1 << (int(i) & 7))
    mm.flush()
    del mm


# ---------------------------------------------------------------------------------------------- CPU: the fixtures themselves


def test_fixture_coverage(oracle):
    f = lcg_fixture(oracle)
    assert f["arr"].shape == (COUNT,) and len(f["acts"]) == COUNT and max(BATCHES) == max(EVAL_BATCHES) == COUNT
    assert {1, BPW - 1, BPW, BPW + 1}.issubset(BATCHES) and COUNT % BPW and COUNT // BPW > 500
    same_word = int(((f["seen_indices"][1:] >> 5) == (f["seen_indices"][:-1] >> 5)).sum())
    print("pairs of seen indices in one 32-bit word among the fixture's: %d (the collision fixture supplies one by construction)" % same_word)
    states, arr, init, ref = collision_fixture(oracle)
    assert np.unique(ref).size < len(ref)


# ---------------------------------------------------------------------------------------------- GPU


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["f32", "f16", "bf16"])
def test_indices_equal_the_reference_in_every_bit(oracle, prec):
    """hash_indices at every batch size, every position.  A batch's indices do not depend on its neighbours, and update=False leaves
    the set alone."""
    A = require_gpu()
    f = lcg_fixture(oracle)
    net = A.Net(arch=A.ARCH_NET4_LCGHASH, precision=A.PREC_NAMES[prec]).load_tensors(constant_ube(f["w"], UBE_CONSTANTS[0]))
    for B in BATCHES:
        got = net.hash_indices(f["arr"][:B])
        assert got.dtype == np.uint32 and got.shape == (B,)
        wrong = np.flatnonzero(got != f["ref"][:B])
        assert wrong.size == 0, (prec, B, wrong[:8], got[wrong[:8]], f["ref"][wrong[:8]])
    rng = np.random.default_rng(4)
    for count in (COUNT, 65, 9, 1):
        perm = rng.permutation(COUNT)[:count]
        assert np.array_equal(net.hash_indices(f["arr"][perm]), f["ref"][perm]), (prec, count)
    var = net.policy_value_uncertainty(f["arr"], f["acts"])[2]
    assert np.all(var == MAXIMUM_VARIANCE)       # update=False throughout: nothing has been marked as seen
    net.close()


def _subnormal_init():
    from test_lcghash_ref import subnormal_init

    return subnormal_init()


def _one_hot_inits():
    out = []
    for c, r, q, v in ((0, 0, 0, 3.5), (27, 3, 3, -2.0), (22, 1, 2, 100.0), (26, 2, 1, -0.375), (13, 3, 0, 1.0)):
        init = np.zeros((C4, N4, N4), np.float32)
        init[c, r, q] = v
        out.append(("one-hot %d,%d,%d" % (c, r, q), init))
    return out


@pytest.mark.gpu
def test_edited_lcghash_init(oracle):
    """lcghash_init replaced through load_tensors: all negative (every zero plane gives -0.0 = -2**31), all zero, one-hot at a few
    places, a constant (distinct positions that share an index), and values whose products with the reserve ratios and the
    flat-difference plane are subnormal - a multiply that flushes them would fail here, and the kernel is what would have to change."""
    A = require_gpu()
    f = lcg_fixture(oracle)
    rng = np.random.default_rng(8)
    cases = [("negative", -rng.uniform(0.5, 100, size=(C4, N4, N4)).astype(np.float32)), ("zero", np.zeros((C4, N4, N4), np.float32)),
             ("minus zero", np.full((C4, N4, N4), -0.0, np.float32)), ("subnormal", _subnormal_init())] + _one_hot_inits()
    net = A.Net(arch=A.ARCH_NET4_LCGHASH, precision=A.PREC_F16)
    B = 301
    for name, init in cases:
        net.load_tensors(dict(f["w"], lcghash_init=init))
        want = R.indices(f["planes"][:B], init)
        got = net.hash_indices(f["arr"][:B])
        wrong = np.flatnonzero(got != want)
        assert wrong.size == 0, (name, wrong[:8], got[wrong[:8]], want[wrong[:8]])
        if name == "subnormal":
            p = R.products(f["planes"][:B], init)
            assert ((p != 0) & (np.abs(p) < np.finfo(np.float32).tiny)).any(axis=(1, 2, 3)).all()
        if name in ("zero", "minus zero"):
            assert len(set(want.tolist())) <= 2                  # the sign of a product is all that is left: that of the komi plane
    # distinct positions that share an index, and one of them marked as seen
    states, arr, init, ref = collision_fixture(oracle)
    c = UBE_CONSTANTS[0]
    net.load_tensors(dict(constant_ube(f["w"], c), lcghash_init=init))
    assert np.array_equal(net.hash_indices(arr), ref)
    acts = [O.possible_moves(oracle, s) for s in states]
    assert np.all(net.policy_value_uncertainty(arr, acts)[2] == MAXIMUM_VARIANCE)
    first = int(np.flatnonzero(np.bincount(np.unique(ref, return_inverse=True)[1]) > 1)[0])
    group = np.flatnonzero(np.unique(ref, return_inverse=True)[1] == first)
    assert len(group) >= 2
    assert net.hash_indices(arr[group[:1]], update=True)[0] == ref[group[0]]
    check_variances(net.policy_value_uncertainty(arr, acts)[2], c, np.isin(np.arange(16), group), "collision")
    net.close()


@pytest.mark.gpu
@pytest.mark.parametrize("prec", PRECISIONS)
def test_variance_is_one_of_two_known_numbers(oracle, prec):
    """policy_value_uncertainty (tz_net_eval) after update_counts on the chosen half, for three constants and every batch size, through
    the small-batch forms and the full-batch form; the same from a clone; 4 everywhere from a fresh net.  The variances of the first
    precision are kept: every other precision must give the same bits."""
    A = require_gpu()
    f = lcg_fixture(oracle)
    net = A.Net(arch=A.ARCH_NET4_LCGHASH, precision=A.PREC_NAMES[prec]).load_tensors(constant_ube(f["w"], UBE_CONSTANTS[0]))
    slots, got = insert_chosen(net, f)
    assert np.array_equal(got, f["ref"][slots])
    for c in UBE_CONSTANTS:
        net.load_tensors(constant_ube(f["w"], c))            # the set belongs to the net, not to its weights
        full = None
        for B in EVAL_BATCHES[::-1]:
            ube = net.forward_raw(f["arr"][:B])[2]
            assert np.all(ube == np.float32(c)), (prec, c, B)
            var = net.policy_value_uncertainty(f["arr"][:B], f["acts"][:B])[2]
            check_variances(var, c, f["seen"][:B], (prec, c, B))
            full = var if full is None else full
            assert np.array_equal(var.view(np.uint32), full[:B].view(np.uint32)), (prec, c, B)      # every form, the same bits
        first = _FIXTURE.setdefault(("variance", c), full)
        assert np.array_equal(first.view(np.uint32), full.view(np.uint32)), (prec, c)              # every precision, the same bits
    net.load_tensors(constant_ube(f["w"], UBE_CONSTANTS[0]))
    var = net.policy_value_uncertainty(f["arr"], f["acts"])[2]
    clone = net.clone(0)
    assert np.array_equal(clone.hash_indices(f["arr"][:65]), f["ref"][:65])
    assert np.array_equal(clone.policy_value_uncertainty(f["arr"], f["acts"])[2].view(np.uint32), var.view(np.uint32))
    clone.close()
    fresh = A.Net(arch=A.ARCH_NET4_LCGHASH, precision=A.PREC_NAMES[prec]).load_tensors(constant_ube(f["w"], UBE_CONSTANTS[0]))
    assert np.all(fresh.policy_value_uncertainty(f["arr"], f["acts"])[2] == MAXIMUM_VARIANCE)
    fresh.close()
    net.close()


def near_index_inits():
    """Values w for lcghash_init[26][3][3] (the colour plane's last element, weight M**1) with bits(w) * M small modulo 2**64: under an
    init that is zero elsewhere, a position with black to move and one with white to move then differ in H by that small number, and in
    index by a few units.  (bits, dH) are short vectors of the lattice spanned by (1, M) and (0, 2**64), found by Gauss reduction with
    the first coordinate weighted by 32; kept where bits is the pattern of a positive normal fp32 and 2**31 <= |dH| < 2**36."""
    M, MOD, S = R.MULTIPLIER, 1 << 64, 32
    norm = lambda a: (a[0] * S) ** 2 + a[1] ** 2
    u, v = (1, M), (0, MOD)
    while True:
        if norm(u) > norm(v):
            u, v = v, u
        num, den = u[0] * v[0] * S * S + u[1] * v[1], norm(u)
        m = (2 * num + den) // (2 * den)
        if m == 0:
            break
        v = (v[0] - m * u[0], v[1] - m * u[1])
    out = []
    for i in range(-6, 7):
        for j in range(-6, 7):
            b, h = i * u[0] + j * v[0], i * u[1] + j * v[1]
            if 0 < b < 2 ** 31 and 0 < (b >> 23) < 255 and 2 ** 31 <= abs(h) < 2 ** 36:
                assert (b * M - h) % MOD == 0
                out.append(np.uint32(b).view(np.float32))
    assert len(out) >= 4
    return out


@pytest.mark.gpu
def test_two_indices_of_one_word_in_one_batch(oracle):
    """bitset_set_kernel's atomicOr on one 32-bit word from two lanes of one launch.  near_index_inits gives inits under which the
    positions with black to move have indices a few units from those with white to move; the reference picks an init and two
    positions whose indices differ and share a word, both are inserted in one batch, twice each, and every position's variance is
    then what the reference's set says."""
    A = require_gpu()
    f = lcg_fixture(oracle)
    c = UBE_CONSTANTS[0]
    found = None
    for w26 in near_index_inits():               # the reference alone decides which init is used
        init = np.zeros((C4, N4, N4), np.float32)
        init[26, 3, 3] = w26
        ref = R.indices(f["planes"], init)
        u = np.unique(ref)
        for a in u:
            near = u[(u != a) & (u >> 5 == a >> 5)]
            if near.size:
                found = (init, ref, int(a), int(near[0]))
                break
        if found:
            break
    assert found is not None, "no init puts two of the fixture's indices into one word"
    init, ref, a, b = found
    assert a != b and a >> 5 == b >> 5
    net = A.Net(arch=A.ARCH_NET4_LCGHASH, precision=A.PREC_F16).load_tensors(dict(constant_ube(f["w"], c), lcghash_init=init))
    assert np.array_equal(net.hash_indices(f["arr"]), ref)
    pa, pb = int(np.flatnonzero(ref == a)[0]), int(np.flatnonzero(ref == b)[0])
    got = net.hash_indices(f["arr"][[pa, pb, pa, pb]], update=True)
    assert got.tolist() == [a, b, a, b]
    seen = np.isin(ref, [a, b])
    print("one word: indices %d and %d (word %d), %d positions seen, %d unseen, %d distinct indices" % (a, b, a >> 5, seen.sum(), (~seen).sum(), np.unique(ref).size))
    assert seen.sum() >= 2 and (~seen).sum() >= 2
    check_variances(net.policy_value_uncertainty(f["arr"], f["acts"])[2], c, seen, "one word")
    net.close()


@pytest.mark.gpu
def test_files(oracle, tmp_path):
    """save writes the model and a bitvec.bin of 2**29 bytes whose set bits are the reference's; load, clone and load_bitset restore
    them; a failed load keeps the old lcghash_init and the old set."""
    A = require_gpu()
    f = lcg_fixture(oracle)
    c = UBE_CONSTANTS[0]
    w = constant_ube(f["w"], c)
    net = A.Net(arch=A.ARCH_NET4_LCGHASH, precision=A.PREC_F16).load_tensors(w)
    insert_chosen(net, f)
    var = net.policy_value_uncertainty(f["arr"], f["acts"])[2]
    check_variances(var, c, f["seen"], "before save")
    d = tmp_path / "a"
    os.makedirs(d)
    net.save(d / "model_latest.ot")
    assert (d / "bitvec.bin").stat().st_size == 1 << 29
    want = np.unique(f["ref"][f["chosen"]]).astype(np.uint64)
    got = set_bits_of_file(d / "bitvec.bin")
    assert got.size == want.size and np.array_equal(got, want), (got.size, want.size)
    assert (want >= 2 ** 31).sum() >= 100            # the upper half of the file is in use
    from takzero_amd import ot

    named = ot.load_ot(d / "model_latest.ot")
    assert named["lcghash_init"].shape == (C4, N4, N4) and np.array_equal(named["lcghash_init"].view(np.uint32), f["init"].view(np.uint32))
    # load: the variables and the set beside them, into a net that held another init and an empty set
    other_init = np.random.default_rng(21).uniform(-100, 100, size=(C4, N4, N4)).astype(np.float32)
    other = A.Net(arch=A.ARCH_NET4_LCGHASH, precision=A.PREC_F16).load_tensors(dict(w, lcghash_init=other_init))
    assert np.array_equal(other.hash_indices(f["arr"][:65]), R.indices(f["planes"][:65], other_init))
    other.load(d / "model_latest.ot")
    assert np.array_equal(other.hash_indices(f["arr"]), f["ref"])
    assert np.array_equal(other.policy_value_uncertainty(f["arr"], f["acts"])[2].view(np.uint32), var.view(np.uint32))
    assert np.array_equal(other.tensors()["lcghash_init"].view(np.uint32), f["init"].ravel().view(np.uint32))
    clone = other.clone(0)
    assert np.array_equal(clone.hash_indices(f["arr"]), f["ref"])
    assert np.array_equal(clone.policy_value_uncertainty(f["arr"], f["acts"])[2].view(np.uint32), var.view(np.uint32))
    clone.close()
    os.remove(d / "bitvec.bin")
    # load_bitset: the other half, written by numpy
    written = tmp_path / "other.bin"
    write_bits_file(written, f["ref"][~f["chosen"]])
    other.load_bitset(written)
    seen_other = np.isin(f["ref"], f["ref"][~f["chosen"]])
    assert (seen_other != f["seen"]).sum() >= 900
    var_other = other.policy_value_uncertainty(f["arr"], f["acts"])[2]
    check_variances(var_other, c, seen_other, "load_bitset")
    # failed loads: a truncated set, a model file that does not parse, a model without the variable
    os.truncate(written, (1 << 29) - 1)
    with pytest.raises(A.TakzeroError):
        other.load_bitset(written)
    os.remove(written)
    bad = tmp_path / "bad.ot"
    bad.write_bytes(open(d / "model_latest.ot", "rb").read()[:4096])
    with pytest.raises(A.TakzeroError):
        other.load(bad)
    with pytest.raises(A.TakzeroError):
        other.load_tensors({k: v for k, v in w.items() if k != "lcghash_init"})
    with pytest.raises(A.TakzeroError):
        other.load_tensors(dict(w, lcghash_init=f["init"][:, :, :2]))
    assert np.array_equal(other.hash_indices(f["arr"]), f["ref"])                                          # the old lcghash_init ...
    assert np.array_equal(other.policy_value_uncertainty(f["arr"], f["acts"])[2].view(np.uint32), var_other.view(np.uint32))    # ... and the old set
    # the other arch's entry points keep refusing what they refused
    plain = A.Net(arch=A.ARCH_TEST, n=4, blocks=1, precision=A.PREC_F16)
    with pytest.raises(A.TakzeroError):
        plain.save_bitset(tmp_path / "no.bin")
    plain.close()
    with pytest.raises(A.TakzeroError):
        A.Net(arch=A.ARCH_NET4_LCGHASH, n=5)
    other.close()
    net.close()


# ---------------------------------------------------------------------------------------------- searches


def reference_agent(oracle, net, init, seen_set, met=None):
    """An agent for the oracle searches: logits and value are the device's own (tz_net_eval), the variance is the reference's -
    clamp(max(expf(0), local), 0, 4) = 1 where the reference index of the position is in `seen_set`, 4 where it is not."""
    def fn(user, n_envs, states, legal_idx, legal_count, amax, logits_out, value_out, variance_out):
        rc = net.lib.tz_net_eval(net.h, n_envs, C.cast(states, C.c_void_p), C.cast(legal_idx, C.c_void_p), C.cast(legal_count, C.c_void_p), amax,
                                 C.cast(logits_out, C.c_void_p), C.cast(value_out, C.c_void_p), C.cast(variance_out, C.c_void_p))
        assert rc == 0, net.lib.tz_last_error()
        planes = planes_of(oracle, [states[i] for i in range(n_envs)])
        idx = R.indices(planes, init)
        want = np.maximum(np.float32(1.0), seen_set.local(idx))
        device = np.ctypeslib.as_array(variance_out, (n_envs,))
        if met is not None:
            met.append((idx, device.copy()))
        device[:] = want
    return fn


def _search_net(A, f, prec="f16"):
    return A.Net(arch=A.ARCH_NET4_LCGHASH, precision=A.PREC_NAMES[prec]).load_tensors(constant_ube(f["w"], 0.0))


def _seen_from_a_first_search(oracle, net, f, B, starts, sims):
    """The set a search meets: an oracle search over the empty set records the reference indices of what it evaluates; every second
    distinct index, in the order of first meeting, is marked as seen on the device through a position that carries it."""
    met_states = []
    from test_gpu_engine import _agent_over, _watched

    ora = O.OracleSearch(oracle, B, 4, 4, agent_kind=0, agent_fn=_watched(_agent_over(net), states_seen=met_states))
    ora.set_positions(np.arange(B), starts)
    ora.simulate(np.full(B, 0.25, np.float32), sims)
    ora.close()
    distinct = np.concatenate(list({s.tobytes(): s for s in met_states}.values()))
    states = [O.TzState.from_buffer_copy(distinct[i:i + 1].tobytes()) for i in range(len(distinct))]
    idx = R.indices(planes_of(oracle, states), f["init"])
    first = np.sort(np.unique(idx, return_index=True)[1])
    marked = idx[first[::2]]
    got = net.hash_indices(distinct[np.isin(idx, marked)], update=True)
    assert np.isin(got, marked).all() and np.isin(marked, got).all()
    return R.SeenSet(marked), len(first)


@pytest.mark.gpu
def test_lock_step_search_and_simulate_batch_against_the_oracle(oracle, tmp_path):
    """simulate with beta > 0 on 16 games from mid-game positions, against OracleSearch whose agent returns the device's logits and
    value and the reference's variance: roots equal in every field.  Then simulate_batch on the same handle against the batched
    reference search of tests/simulate_batch_util.py with the same agent."""
    A = require_gpu()
    from test_gpu_tree import assert_same_roots

    f = lcg_fixture(oracle)
    B, sims = 16, 24
    net = _search_net(A, f)
    starts = f["arr"][np.flatnonzero((np.arange(COUNT) > 100) & ~np.isin(np.arange(COUNT), EXHAUSTED_SLOTS))[:B]]
    seen, n_indices = _seen_from_a_first_search(oracle, net, f, B, starts, sims)
    met = []
    gpu = A.BatchedMCTS(B, 4, 4, agent=net, node_capacity=1 << 12)
    ora = O.OracleSearch(oracle, B, 4, 4, agent_kind=0, agent_fn=reference_agent(oracle, net, f["init"], seen, met))
    gpu.set_positions(np.arange(B), starts)
    ora.set_positions(np.arange(B), starts)
    betas = np.where(np.arange(B) % 2 == 0, 0.25, 0.5).astype(np.float32)
    for phase in range(3):                       # two eager simulations, a captured one, replays
        gpu.simulate(betas, sims // 3)
        ora.simulate(betas, sims // 3)
        assert_same_roots(gpu, ora, "phase %d" % phase)
    assert np.array_equal(gpu.select_best_actions(), ora.select_best_actions()) and gpu.counters() == ora.counters()
    idx = np.concatenate([m[0] for m in met])
    device = np.concatenate([m[1] for m in met])
    want = np.maximum(np.float32(1.0), seen.local(idx))
    assert np.array_equal(device.view(np.uint32), want.view(np.uint32))                   # tz_net_eval's own variance is the reference's
    low = float((want < 4).mean())
    print("lock-step: %d evaluations, %d distinct indices in the first search, %.1f %% seen" % (len(idx), n_indices, 100 * low))
    assert 0.1 <= low <= 0.9
    ora.close()
    # simulate_batch: 8 leaves per tree per call
    import simulate_batch_util as U

    ref_lib = U.build(tmp_path)
    gpu2 = A.BatchedMCTS(B, 4, 4, agent=net, node_capacity=1 << 12)
    ref = U.RefSearch(ref_lib, B, 4, 4, agent_kind=0, agent_fn=reference_agent(oracle, net, f["init"], seen))
    gpu2.set_positions(np.arange(B), starts)
    ref.set_positions(np.arange(B), starts)
    for rounds in (1, 3):
        gpu2.simulate_batch(betas, 8, rounds)
        ref.simulate_batch(betas, 8, rounds)
        assert U.compare(gpu2, ref, "simulate_batch %d" % rounds) > B
    ref.close()
    net.close()


@pytest.mark.gpu
def test_gumbel_halving_against_the_oracle(oracle):
    """Gumbel sequential halving, 16 sampled actions, budget 64, the same way."""
    A = require_gpu()
    from test_gpu_tree import assert_same_roots

    f = lcg_fixture(oracle)
    B = 16
    net = _search_net(A, f)
    starts = f["arr"][np.flatnonzero((np.arange(COUNT) > 300) & ~np.isin(np.arange(COUNT), EXHAUSTED_SLOTS))[:B]]
    seen, _ = _seen_from_a_first_search(oracle, net, f, B, starts, 24)
    gpu = A.BatchedMCTS(B, 4, 4, agent=net, node_capacity=1 << 12)
    ora = O.OracleSearch(oracle, B, 4, 4, agent_kind=0, agent_fn=reference_agent(oracle, net, f["init"], seen))
    gpu.set_positions(np.arange(B), starts)
    ora.set_positions(np.arange(B), starts)
    betas = np.where(np.arange(B) % 2 == 0, 0.25, 0.0).astype(np.float32)
    gumbel = np.random.default_rng(5).gumbel(size=(B, 512)).astype(np.float32)
    a = gpu.gumbel_sequential_halving(betas, 16, 64, gumbel)
    b = ora.gumbel_sequential_halving(betas, 16, 64, gumbel)
    assert np.array_equal(a, b)
    assert_same_roots(gpu, ora, "gumbel 16 / 64")
    assert gpu.counters() == ora.counters()
    ora.close()
    net.close()


# ---------------------------------------------------------------------------------------------- learn


@pytest.mark.gpu
def test_learn_loop_with_a_hash_net(oracle, tmp_path):
    """A trainer of the new arch at batch 64 inside tz_learn_run with an LCG-hash net as hash_net (tz_learn_set_save_points): after
    three steps the net's set holds exactly the reference indices of the three batches and bitvec.bin beside model_latest.ot says
    the same; lcghash_init comes back from the files and from to_net with the bytes that went in; and the three losses are those of a
    net4_simhash trainer with the same trunk and head tensors on the same batches - the hash tensor does not leak into the step.
    The batches are the states on_step is handed (tz_learn_last_batch reads the first of tz_learn_run's two batch slots, which is the
    step's own batch only on every other step)."""
    A = require_gpu()
    from takzero_amd import formats as F
    from takzero_amd import learn as L
    from takzero_amd import ot
    from takzero_amd import weights as W
    from takzero_amd._lib import check
    from test_learn_host import _targets

    n, B, steps = 4, 64, 3
    targets = _targets(n, 256, 5)
    text = "".join(F.format_target(n, *t) for t in targets)
    w = W.init_weights(W.ARCH_NET4_LCGHASH, seed=3)
    init = w["lcghash_init"]
    simhash_w = {k: v for k, v in w.items() if k != "lcghash_init"}
    simhash_w["simhash_matrix"] = W.init_weights(W.ARCH_NET4_SIMHASH, seed=3)["simhash_matrix"]

    def run(arch, tensors, d, hash_net):
        os.makedirs(d)
        with open(os.path.join(d, "targets-selfplay.txt"), "w") as fh:
            fh.write(text)
        trainer = L.Trainer(arch=arch, batch=B).load_tensors(tensors)
        loop = L.NativeLearnLoop(trainer, 4, seed=1)
        check(loop.lib.tz_learn_set_save_points(loop.h, steps, 10 ** 9, hash_net.h if hash_net is not None else None))
        batches, losses = [], []

        def on_step(step_no, ls, states):
            clean = np.zeros(len(states), O.STATE_DTYPE)          # field by field: the struct's padding is not part of a position
            clean[...] = states
            batches.append(clean)
            losses.append(tuple(np.float32(x) for x in ls))

        done = loop.run(d, 0, steps, min_selfplay=B, steps_before_reanalyze=10 ** 9, read_interval=0.0, sleep=0.01, max_wait=30, on_step=on_step)
        assert done == steps and len(batches) == steps
        loop.close()
        return trainer, batches, losses

    hash_net = A.Net(arch=A.ARCH_NET4_LCGHASH, precision=A.PREC_F16).load_tensors(constant_ube(w, UBE_CONSTANTS[0]))
    d = str(tmp_path / "lcg")
    trainer, batches, losses = run(A.ARCH_NET4_LCGHASH, w, d, hash_net)
    assert "lcghash_init" not in trainer.names and set(trainer.extras()) == {"lcghash_init"}
    arr = np.concatenate(batches)
    states = [O.TzState.from_buffer_copy(arr[i:i + 1].tobytes()) for i in range(len(arr))]
    assert len({a.tobytes() for a in batches}) == steps
    ref = R.indices(planes_of(oracle, states), init)
    want = np.unique(ref).astype(np.uint64)
    assert sorted(os.listdir(d)).count("bitvec.bin") == 1 and "model_latest.ot" in os.listdir(d)
    assert np.array_equal(set_bits_of_file(os.path.join(d, "bitvec.bin")), want)         # written at the save point after the third step
    hash_net.save_bitset(os.path.join(d, "now.bin"))
    assert np.array_equal(set_bits_of_file(os.path.join(d, "now.bin")), want)            # the net's set: exactly the three batches
    os.remove(os.path.join(d, "now.bin"))
    # lcghash_init: carried through the step, the save point's file, save, extras and to_net
    bits = init.view(np.uint32)
    assert np.array_equal(ot.load_ot(os.path.join(d, "model_latest.ot"))["lcghash_init"].view(np.uint32), bits)
    assert np.array_equal(trainer.extras()["lcghash_init"].view(np.uint32), bits)
    trainer.save(os.path.join(d, "saved.ot"))
    assert np.array_equal(ot.load_ot(os.path.join(d, "saved.ot"))["lcghash_init"].view(np.uint32), bits)
    trainer.save(os.path.join(d, "saved.tzw"))
    assert np.array_equal(W.load_tzw(os.path.join(d, "saved.tzw"))["lcghash_init"].view(np.uint32), bits)
    trainer.to_net(hash_net)
    assert np.array_equal(hash_net.tensors()["lcghash_init"].view(np.uint32), bits.ravel())
    assert np.array_equal(hash_net.hash_indices(arr[:65]), ref[:65])
    back = L.Trainer(arch=A.ARCH_NET4_LCGHASH, batch=B).from_net(hash_net)
    assert np.array_equal(back.extras()["lcghash_init"].view(np.uint32), bits)
    back.close()
    # a fresh net picks model and set up from the directory, as self-play does
    fresh = A.Net(arch=A.ARCH_NET4_LCGHASH, precision=A.PREC_F16).load(os.path.join(d, "model_latest.ot"))
    extra = random_positions(oracle, O, 4, 4, 100, 77, max_ply=60)
    all_arr = np.concatenate([arr, O.states_array(extra)])
    all_ref = np.concatenate([ref, R.indices(planes_of(oracle, extra), init)])
    assert np.array_equal(fresh.hash_indices(all_arr), all_ref)
    acts = [O.possible_moves(oracle, s) for s in states + extra]
    var = fresh.policy_value_uncertainty(all_arr, acts)[2]
    seen = np.isin(all_ref, ref)
    assert seen[:len(arr)].all() and (~seen).sum() >= 50
    assert np.all(var[~seen] == MAXIMUM_VARIANCE) and np.all(var[seen] < MAXIMUM_VARIANCE)
    fresh.close()
    os.remove(os.path.join(d, "bitvec.bin"))
    # the twin: net4_simhash, the same trunk and heads, the same seed -> the same batches, and then the same losses
    twin, twin_batches, twin_losses = run(A.ARCH_NET4_SIMHASH, simhash_w, str(tmp_path / "simhash"), None)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(batches, twin_batches))
    print("losses: %r" % (losses,))
    assert np.array_equal(np.array(losses, np.float32).view(np.uint32), np.array(twin_losses, np.float32).view(np.uint32)), (losses, twin_losses)
    assert all(np.isfinite(l).all() and l[0] > 0 for l in losses)
    twin.close()
    trainer.close()
    hash_net.close()
