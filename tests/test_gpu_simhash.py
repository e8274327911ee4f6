"""The SimHash uncertainty path of net4_simhash / net6_simhash against an fp64 reference: indices, the set, the variance.

local = 0 where a position's 32-bit index is in the net's set of seen indices and 4 where it is not; the index's bit j is set
where the projection of the planes (black-to-move plane zeroed) on column j of simhash_matrix is not below zero
(net6_simhash.rs:202-256); variance = clamp(max(exp(ube), local), 0, 4) (:311-318) becomes the nodes' std_dev in the search.
Nothing here needs a measured tolerance:

  * a bit is *decided* where |dot in fp64| exceeds nets_torch.simhash_margin, the a-priori bound K * 2**-24 * (|x| @ |matrix|) of an
    fp32 evaluation of that dot product in any order, with or without FMA.  On decided bits the kernel must give dot64 >= 0
    exactly; a position is decided when all 32 bits are, and only decided positions take part in index and variance comparisons.
    The fixture caps the undecided: at most 0.1 % of (position, bit) pairs and 2 % of positions;
  * with ube.linear.weight = 0 and ube.linear.bias = c, ube == c bit for bit, and the variance of a position is one of two exactly
    known numbers: 4 (unseen) or clamp(expf(c), 0, 4) (seen), the latter held to rtol 1e-6 (test_gpu_uncertainty.sharp_check's
    bound on expf).  Only decided positions are inserted, so the expected set is the reference's indices, not the kernel's.

Not covered: `!(s < 0.0f)` against `s > 0.0f` in simhash_state_kernel - a dot product of exactly zero does not occur on real
positions (the start position's smallest |dot| is 0.086 on 4x4, 0.48 on 6x6)."""
import os
import sys

import numpy as np
import pytest

import oracle_lib as O
from gpu_util import random_positions, require_gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))

MAXIMUM_VARIANCE = np.float32(4.0)
COUNT = 2051
# the tails of simhash_state_kernel's 8-board workgroup on either side, one position, many workgroups with a tail of 3
BATCHES = (1, 7, 8, 9, 63, 64, 65, COUNT)
# (source, copy) slots of exact duplicates, each pair in two different 8-board workgroups; (2, 8) lies inside the 9-position batch
DUPLICATES = ((2, 8), (3, 1000), (17, 2050), (63, 64), (500, 1501))
START_SLOTS = (5, 2047)            # the start position (an empty board: only the reserve and komi planes are set)
MAX_UNDECIDED_PAIRS, MAX_UNDECIDED_POSITIONS = 0.001, 0.02
UBE_CONSTANTS = (float(np.float32(np.log(0.5))), -20.0, 2.0)      # exp(c) = 0.5; 2e-9, still > 0; above the clamp at 4
# the precisions each SimHash arch accepts (f16c6 is built for 5x5 and 6x6)
PRECISIONS = {4: ("f32", "f16", "bf16", "f16x2", "f16c8"), 6: ("f32", "f16", "bf16", "f16x2", "f16c8", "f16c6")}
POWERS = np.uint64(1) << np.arange(32, dtype=np.uint64)

_FIXTURES = {}


def _planes(oracle, states, n):
    return np.stack([O.game_repr(oracle, s) for s in states]).reshape(len(states), -1, n, n)


def reference_indices(dots):
    """The index get_indices builds from the projections: powers_of_two.masked_fill(dots < 0, 0).sum(1), as uint32."""
    return ((dots >= 0).astype(np.uint64) * POWERS).sum(axis=1).astype(np.uint32)


def _hashed_keys(planes):
    """What the hash reads of a position (planes with the black-to-move plane zeroed), as bytes: two positions are distinct for the
    hash where these differ."""
    x = planes.copy()
    x[:, x.shape[1] - 2] = 0.0
    return np.array([x[i].tobytes() for i in range(len(x))], dtype=object)


def simhash_fixture(oracle, n):
    """The shipped SimHash net of board size n with 2051 positions of every stage, a few exact duplicates in different workgroups and the
    start position; their fp64 projections, margins, reference indices, which are decided, and the half chosen to be marked as
    seen.  Asserts its own coverage and prints the figures."""
    if n in _FIXTURES:
        return _FIXTURES[n]
    import nets_torch as T
    from takzero_amd import weights as W

    arch = {4: W.ARCH_NET4_SIMHASH, 6: W.ARCH_NET6_SIMHASH}[n]
    w = W.init_weights(arch, seed=3)
    states = random_positions(oracle, O, n, 4, COUNT, 5, max_ply=60)
    for src, dst in DUPLICATES:
        assert src // 8 != dst // 8
        states[dst] = states[src]
    for at in START_SLOTS:
        states[at] = O.state_default(oracle, n, 4)
    planes = _planes(oracle, states, n)
    assert planes.shape[1] == 4 * n + 12 and w["simhash_matrix"].shape == (planes.shape[1] * n * n, 32)
    dots = T.simhash_dots(w, planes).numpy()
    margin = T.simhash_margin(w, planes).numpy()
    assert dots.dtype == np.float64 and margin.dtype == np.float64 and dots.shape == margin.shape == (COUNT, 32)
    decided_bits = np.abs(dots) > margin
    decided = decided_bits.all(axis=1)
    ref = reference_indices(dots)
    keys = _hashed_keys(planes)
    slots = np.arange(COUNT)
    # every second decided position is marked as seen; a position never inserted whose index equals a seen one counts as seen too
    chosen = decided & (slots % 2 == 0)
    seen = np.isin(ref, ref[chosen])
    colliding = decided & ~chosen & seen & ~np.isin(keys, keys[chosen])
    seen_indices = np.unique(ref[chosen])
    same_word = int(((seen_indices[1:] >> 5) == (seen_indices[:-1] >> 5)).sum())
    undecided_pairs, undecided_positions = float((~decided_bits).mean()), float((~decided).mean())
    top_bit = float((ref[decided] >= 2 ** 31).mean())
    distinct_positions, distinct_indices = len(set(keys[decided])), len(set(ref[decided].tolist()))
    plies = np.array([s.ply for s in states])
    print("%dx%d: %d of %d (position, bit) pairs undecided (%.4f %%), %d positions (%.2f %%); index >= 2^31 on %.1f %%; %d distinct decided "
          "positions -> %d distinct indices; %d seen / %d unseen decided positions, %d of the seen never inserted (a collision); %d "
          "pairs of seen indices in one 32-bit word" %
          (n, n, int((~decided_bits).sum()), decided_bits.size, 100 * undecided_pairs, int((~decided).sum()), 100 * undecided_positions,
           100 * top_bit, distinct_positions, distinct_indices, int((decided & seen).sum()), int((decided & ~seen).sum()),
           int(colliding.sum()), same_word))
    assert undecided_pairs <= MAX_UNDECIDED_PAIRS and undecided_positions <= MAX_UNDECIDED_POSITIONS
    assert 0.15 <= top_bit <= 0.85                      # the top bit takes part in index >> 5
    assert distinct_positions - distinct_indices >= 50  # distinct positions that share an index
    assert colliding.sum() >= 20
    assert (decided & seen).sum() >= 500 and (decided & ~seen).sum() >= 500
    assert same_word >= 2                               # bitset_set_kernel's atomicOr: two indices of one word, in one batch
    assert np.bincount(plies // 10, minlength=6)[:6].min() >= 100      # every stage of a game: plies 0-9, 10-19, ... 50-59
    for src, dst in DUPLICATES:
        assert ref[src] == ref[dst] and keys[src] == keys[dst]
    _FIXTURES[n] = dict(n=n, arch=arch, w=w, states=states, arr=O.states_array(states), acts=[O.possible_moves(oracle, s) for s in states],
                        planes=planes, dots=dots, margin=margin, decided_bits=decided_bits, decided=decided, ref=ref, keys=keys,
                        chosen=chosen, seen=seen, colliding=colliding)
    return _FIXTURES[n]


def index_variants(ref, decided_bits):
    """Every index an fp32 evaluation may give the undecided positions: the reference's with each undecided bit either way."""
    out = set()
    for i in np.flatnonzero(~decided_bits.all(axis=1)):
        free = [int(b) for b in np.flatnonzero(~decided_bits[i])]
        assert len(free) <= 8
        base = int(ref[i]) & ~sum(1 << b for b in free)
        for m in range(1 << len(free)):
            out.add(base | sum(1 << b for k, b in enumerate(free) if m >> k & 1))
    return out


def constant_ube(w, c):
    """test_gpu_uncertainty.rnd_fixture's weights: ube == c on every position, and no trunk reference is needed."""
    w = dict(w)
    w["ube.linear.weight"] = np.zeros_like(w["ube.linear.weight"])
    w["ube.linear.bias"] = np.full(1, c, np.float32)
    return w


def seen_variance(c):
    """clamp(expf(c), 0, 4) in fp64 of the float32 c."""
    return min(float(np.exp(np.float64(np.float32(c)))), 4.0)


def insert_chosen(net, f, chosen=None):
    """Mark the chosen positions as seen (update_counts) in three calls: all of them in the order of their reference indices (indices
    of one 32-bit word of the set side by side, and a tail workgroup), every third one again (positions repeated from an earlier
    call), and forty of them twice within one batch.  Returns the indices the calls gave with the slots they belong to."""
    slots = np.flatnonzero(f["chosen"] if chosen is None else chosen)
    assert f["decided"][slots].all()
    calls = [slots[np.argsort(f["ref"][slots], kind="stable")], slots[::3], np.repeat(slots[:40], 2)]
    got = [net.hash_indices(f["arr"][c], update=True) for c in calls]
    return np.concatenate(calls), np.concatenate(got)


def check_variances(f, var, B, c, seen, label):
    """The variances of the first B positions against the two exactly known numbers, on decided positions.  Returns (seen, unseen)
    positions checked."""
    decided, seen = f["decided"][:B], seen[:B]
    assert np.all(np.isfinite(var)), (label, B)
    unseen_at, seen_at = decided & ~seen, decided & seen
    wrong = np.flatnonzero(unseen_at & (var != MAXIMUM_VARIANCE))
    assert wrong.size == 0, (label, B, "unseen positions below 4", wrong[:8], var[wrong[:8]])
    want = seen_variance(c)
    if want == 4.0:
        wrong = np.flatnonzero(seen_at & (var != MAXIMUM_VARIANCE))
    else:
        wrong = np.flatnonzero(seen_at & ~(np.isclose(var, want, rtol=1e-6, atol=0) & (var > 0)))
    assert wrong.size == 0, (label, B, "seen positions off %r" % want, wrong[:8], var[wrong[:8]],
                             "never inserted (index collision): %r" % np.flatnonzero(f["colliding"][:B])[:8].tolist())
    return int(seen_at.sum()), int(unseen_at.sum())


# ---------------------------------------------------------------------------------------------- CPU: the reference itself


@pytest.mark.parametrize("n", [4, 6])
def test_fixture_coverage(oracle, n):
    """simhash_fixture asserts its caps and coverage (undecided share, top bit, collisions, seen / unseen); this runs it without a GPU."""
    f = simhash_fixture(oracle, n)
    assert f["arr"].shape == (COUNT,) and len(f["acts"]) == COUNT and max(BATCHES) == COUNT
    assert f["decided"][list(START_SLOTS)].all() and f["ref"][START_SLOTS[0]] == f["ref"][START_SLOTS[1]]
    assert not f["chosen"][~f["decided"]].any()
    # the constant-UBE weights change nothing the hash reads
    w = constant_ube(f["w"], UBE_CONSTANTS[0])
    assert not w["ube.linear.weight"].any() and w["ube.linear.bias"][0] == np.float32(np.log(0.5)) and w["simhash_matrix"] is f["w"]["simhash_matrix"]


@pytest.mark.parametrize("n", [4, 6])
def test_fp32_and_fp64_projections_agree_on_every_decided_bit(oracle, n):
    """torch's fp32 matmul is one of the fp32 evaluations the margin bounds: inside it everywhere, so equal to fp64 in sign on decided bits."""
    import nets_torch as T
    import torch

    f = simhash_fixture(oracle, n)
    d32 = T.simhash_dots(f["w"], f["planes"], torch.float32).numpy()
    assert d32.dtype == np.float32
    assert np.all(np.abs(d32.astype(np.float64) - f["dots"]) <= f["margin"])
    db = f["decided_bits"]
    assert np.array_equal((d32 >= 0)[db], (f["dots"] >= 0)[db])
    # the margin is small against the projections' scale: it decides nearly everything without being loose about it
    assert np.median(f["margin"]) < 1e-3 * np.median(np.abs(f["dots"]))


@pytest.mark.parametrize("n", [4, 6])
def test_simhash_indices_are_the_signs_of_simhash_dots(oracle, n):
    import nets_torch as T
    import torch

    f = simhash_fixture(oracle, n)
    idx, dots = T.simhash_indices(f["w"], f["planes"], f["planes"].shape[1], return_dots=True)
    assert np.array_equal(dots, T.simhash_dots(f["w"], f["planes"], torch.float32).numpy())
    assert np.array_equal(idx.astype(np.uint32), reference_indices(dots))
    d = f["decided"]
    assert np.array_equal(idx.astype(np.uint32)[d], f["ref"][d])
    assert idx.min() >= 0 and idx.max() < 2 ** 32


def test_bit_order_is_two_to_the_column(oracle):
    """Bit 0 of the index is column 0 of simhash_matrix (2 ** arange(32), net6_simhash.rs:204-206): a matrix with one non-zero column j,
    positive on a plane every position has set, gives index 2**j; negative, 0."""
    import nets_torch as T
    from takzero_amd import weights as W

    f = simhash_fixture(oracle, 4)
    planes = f["planes"][:16]
    for j in (0, 1, 5, 31):
        for sign in (1.0, -1.0):
            m = np.zeros_like(f["w"]["simhash_matrix"])
            hashed = planes.copy()
            hashed[:, hashed.shape[1] - 2] = 0.0
            m[:, j] = sign * (hashed.reshape(16, -1).min(axis=0) > 0)      # squares of planes positive on all 16 positions
            assert m[:, j].any()
            w = dict(f["w"], simhash_matrix=m)
            dots = T.simhash_dots(w, planes).numpy()
            others = np.delete(np.arange(32), j)
            assert np.all(dots[:, others] == 0) and np.all(np.sign(dots[:, j]) == sign)
            want = sum(2 ** int(k) for k in others) + (2 ** j if sign > 0 else 0)          # a zero projection is not below zero: bit set
            assert np.all(T.simhash_indices(w, planes, planes.shape[1]) == want)
            assert np.all(reference_indices(dots) == np.uint32(want))
    assert W.HASH_BITS == 32


def test_margin_zeroes_the_colour_plane_and_scales_with_the_inputs(oracle):
    import nets_torch as T

    f = simhash_fixture(oracle, 6)
    planes = f["planes"][:32]
    cin = planes.shape[1]
    other = planes.copy()
    other[:, cin - 2] = 1.0 - other[:, cin - 2]
    assert np.array_equal(T.simhash_dots(f["w"], planes).numpy(), T.simhash_dots(f["w"], other).numpy())
    assert np.array_equal(T.simhash_margin(f["w"], planes).numpy(), T.simhash_margin(f["w"], other).numpy())
    flat = planes.copy()
    flat[:, cin - 2] = 0.0
    flat = np.abs(flat.reshape(32, -1).astype(np.float64))
    want = cin * 36 * 2.0 ** -24 * (flat @ np.abs(f["w"]["simhash_matrix"].astype(np.float64)))
    assert np.allclose(T.simhash_margin(f["w"], planes).numpy(), want, rtol=1e-12, atol=0)


# ---------------------------------------------------------------------------------------------- GPU


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("n", [4, 6])
def test_indices_against_fp64(oracle, n, prec):
    """hash_indices at every batch size: the reference index on every decided position, and on the others a difference in undecided
    bits only.  A batch's indices do not depend on its neighbours, and update=False leaves the set alone."""
    A = require_gpu()
    f = simhash_fixture(oracle, n)
    net = A.Net(arch=f["arch"], precision=A.PREC_NAMES[prec]).load_tensors(constant_ube(f["w"], UBE_CONSTANTS[0]))
    undecided_mask = ((~f["decided_bits"]).astype(np.uint64) * POWERS).sum(axis=1).astype(np.uint32)
    full = None
    for B in BATCHES:
        got = net.hash_indices(f["arr"][:B])
        assert got.dtype == np.uint32 and got.shape == (B,)
        d = f["decided"][:B]
        wrong = np.flatnonzero(d & (got != f["ref"][:B]))
        assert wrong.size == 0, (n, prec, B, wrong[:8], got[wrong[:8]], f["ref"][wrong[:8]])
        stray = (got ^ f["ref"][:B]) & ~undecided_mask[:B]
        assert not stray.any(), (n, prec, B, np.flatnonzero(stray)[:8])
        full = got
    print("%dx%d %s: %d decided positions equal the fp64 index at every batch size; %d undecided differ in %d undecided bits" %
          (n, n, prec, int(f["decided"].sum()), int((~f["decided"]).sum()), int(np.unpackbits((full ^ f["ref"]).view(np.uint8)).sum())))
    rng = np.random.default_rng(n)
    for count in (COUNT, 65, 9, 1):
        perm = rng.permutation(COUNT)[:count]
        assert np.array_equal(net.hash_indices(f["arr"][perm]), full[perm]), (n, prec, count)
    var = net.policy_value_uncertainty(f["arr"], f["acts"])[2]
    assert np.all(var == MAXIMUM_VARIANCE)       # update=False throughout: nothing has been marked as seen
    net.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n,prec", [(n, p) for n in (4, 6) for p in PRECISIONS[n]])
def test_variance_is_one_of_two_known_numbers(oracle, n, prec):
    """policy_value_uncertainty (tz_net_eval) after update_counts on the chosen half: 4 on unseen positions, clamp(expf(c), 0, 4) on seen
    ones, for three constants c and every batch size; then the same from a clone, and 4 everywhere from a fresh net of the same weights."""
    A = require_gpu()
    f = simhash_fixture(oracle, n)
    net = A.Net(arch=f["arch"], precision=A.PREC_NAMES[prec]).load_tensors(constant_ube(f["w"], UBE_CONSTANTS[0]))
    slots, got = insert_chosen(net, f)
    assert np.array_equal(got, f["ref"][slots])          # what was set is the reference's set
    checked = [0, 0]
    for c in UBE_CONSTANTS:
        net.load_tensors(constant_ube(f["w"], c))        # the set belongs to the net, not to its weights
        for B in BATCHES:
            ube = net.forward_raw(f["arr"][:B])[2]
            assert np.all(ube == np.float32(c)), (n, prec, c, B, ube[ube != np.float32(c)][:4])
            var = net.policy_value_uncertainty(f["arr"][:B], f["acts"][:B])[2]
            s, u = check_variances(f, var, B, c, f["seen"], (n, prec, c))
            if B == COUNT:
                checked = [checked[0] + s, checked[1] + u]
    assert checked[0] >= 3 * 500 and checked[1] >= 3 * 500, checked
    never = np.flatnonzero(f["colliding"])
    print("%dx%d %s: %d seen and %d unseen decided positions per constant; seen without having been inserted (index collision): %d, slots %r ..." %
          (n, n, prec, checked[0] // 3, checked[1] // 3, never.size, never[:6].tolist()))
    net.load_tensors(constant_ube(f["w"], UBE_CONSTANTS[0]))                  # the clone is compared where the two levels differ
    var = net.policy_value_uncertainty(f["arr"], f["acts"])[2]
    assert never.size >= 20 and np.all(var[never] < MAXIMUM_VARIANCE)
    clone = net.clone(0)
    assert np.array_equal(clone.policy_value_uncertainty(f["arr"], f["acts"])[2].view(np.uint32), var.view(np.uint32))
    clone.close()
    fresh = A.Net(arch=f["arch"], precision=A.PREC_NAMES[prec]).load_tensors(constant_ube(f["w"], UBE_CONSTANTS[0]))
    assert np.all(fresh.policy_value_uncertainty(f["arr"], f["acts"])[2] == MAXIMUM_VARIANCE)
    fresh.close()
    net.close()


def _set_bits_of_file(path):
    """The indices of the set bits of a bitvec.bin read as the reference's BitBox<usize, Lsb0> lays them out on a little-endian host:
    bit i in byte i >> 3, bit i & 7."""
    mm = np.memmap(path, dtype=np.uint8, mode="r")
    assert mm.shape == (1 << 29,)
    out = []
    for lo in range(0, 1 << 29, 1 << 26):
        at = np.flatnonzero(mm[lo:lo + (1 << 26)])
        for i in at:
            byte = int(mm[lo + i])
            out.extend(((lo + int(i)) << 3) + b for b in range(8) if byte >> b & 1)
    del mm
    return np.array(sorted(out), dtype=np.uint64)


@pytest.mark.gpu
def test_bitvec_file_has_the_reference_layout(oracle, tmp_path):
    """save_bitset / load_bitset against files read and written by numpy in the reference's layout (net6_simhash.rs:152-190), 4x4: one
    save, one load, one refused load."""
    A = require_gpu()
    f = simhash_fixture(oracle, 4)
    c = UBE_CONSTANTS[0]
    net = A.Net(arch=f["arch"], precision=A.PREC_F16).load_tensors(constant_ube(f["w"], c))
    insert_chosen(net, f)
    saved = tmp_path / "bitvec.bin"
    net.save_bitset(saved)
    assert saved.stat().st_size == 1 << 29
    want = np.unique(f["ref"][f["chosen"]]).astype(np.uint64)
    got = _set_bits_of_file(saved)
    assert got.size == want.size and np.array_equal(got, want), (got.size, want.size)
    assert (want >= 2 ** 31).sum() >= 100            # the upper half of the file is in use
    os.remove(saved)
    # the other half of the decided positions, written by numpy; sparse where the file system allows
    other = f["decided"] & ~f["chosen"]
    written = tmp_path / "other.bin"
    mm = np.memmap(written, dtype=np.uint8, mode="w+", shape=(1 << 29,))
    for i in np.unique(f["ref"][other]).astype(np.uint64):
        mm[int(i) >> 3] |= np.uint8(1 << (int(i) & 7))
    mm.flush()
    del mm
    net.load_bitset(written)
    seen_other = np.isin(f["ref"], f["ref"][other])
    assert (f["decided"] & (seen_other != f["seen"])).sum() >= 500      # the two sets tell many positions apart
    var = net.policy_value_uncertainty(f["arr"], f["acts"])[2]
    s, u = check_variances(f, var, COUNT, c, seen_other, "loaded")
    assert s >= 500 and u >= 500
    os.truncate(written, (1 << 29) - 1)
    with pytest.raises(A.TakzeroError):
        net.load_bitset(written)
    assert np.array_equal(net.policy_value_uncertainty(f["arr"], f["acts"])[2].view(np.uint32), var.view(np.uint32))   # the old set stays
    os.remove(written)
    net.close()


class _RecordingHashNet:
    """A hash_net for run_learn / run_learn_native that passes everything on to a Net and keeps the states of every update_counts."""

    def __init__(self, net):
        self.net, self.batches = net, []

    def hash_indices(self, states, update=False):
        assert update
        self.batches.append(np.array(states, copy=True))
        return self.net.hash_indices(states, update=update)

    def save_bitset(self, path):
        return self.net.save_bitset(path)


@pytest.mark.gpu
@pytest.mark.parametrize("loop", ["run_learn_native", "run_learn"])
def test_learn_loop_updates_the_set_with_every_batch(oracle, tmp_path, loop):
    """learn::main's net.update_counts(&tensors.input) on every batch (learn/src/main.rs:418) and bitvec.bin beside every model it saves:
    three steps over a small directory of targets with a net4_simhash as hash_net (the trainer is ARCH_TEST-sized: the loop takes the two
    apart).  Afterwards the set holds the reference indices of the batches' states, and bitvec.bin beside model_latest.ot gives a fresh
    net the same variances."""
    A = require_gpu()
    import nets_torch as T
    from takzero_amd import formats as F
    from takzero_amd import learn as L
    from takzero_amd import weights as W
    from test_learn_host import _targets

    n, B, steps = 4, 64, 3
    d = str(tmp_path)
    targets = _targets(n, 256, 5)
    with open(os.path.join(d, "targets-selfplay.txt"), "w") as fh:
        fh.write("".join(F.format_target(n, *t) for t in targets))
    trainer = L.Trainer(arch=A.ARCH_TEST, n=n, blocks=1, batch=B).load_tensors(W.init_weights(W.ARCH_TEST, n=n, blocks=1, seed=2))
    c = UBE_CONSTANTS[0]
    w = constant_ube(W.init_weights(W.ARCH_NET4_SIMHASH, seed=3), c)
    hash_net = _RecordingHashNet(A.Net(arch=A.ARCH_NET4_SIMHASH, precision=A.PREC_F16).load_tensors(w))
    done = getattr(L, loop)(d, trainer, steps=steps, seed=1, hash_net=hash_net, min_selfplay=B, steps_before_reanalyze=10 ** 9,
                            steps_per_save=steps, steps_per_checkpoint=10 ** 9, pre_training_steps=0, read_interval=0.0, sleep=0.01,
                            max_wait=30)
    assert done == steps and len(hash_net.batches) == steps and all(len(b) == B for b in hash_net.batches)
    arr = np.concatenate(hash_net.batches)
    states = [O.TzState.from_buffer_copy(arr[i:i + 1].tobytes()) for i in range(len(arr))]
    assert all(s.n == n and s.half_komi == 4 for s in states) and len({A.state_to_tps(arr[i]) for i in range(len(arr))}) > B
    planes = _planes(oracle, states, n)
    dots, margin = T.simhash_dots(w, planes).numpy(), T.simhash_margin(w, planes).numpy()
    decided_bits = np.abs(dots) > margin
    decided = decided_bits.all(axis=1)
    ref = reference_indices(dots)
    assert decided.mean() >= 1 - MAX_UNDECIDED_POSITIONS
    # an undecided position of a batch was inserted too, under one of a few indices: positions that meet one of those are left out
    unsure = np.array(sorted(index_variants(ref, decided_bits) - set(ref[decided].tolist())), dtype=np.uint32)
    files = sorted(os.listdir(d))
    assert "bitvec.bin" in files and "model_latest.ot" in files, files
    bits = _set_bits_of_file(os.path.join(d, "bitvec.bin"))
    must, may = np.unique(ref[decided]).astype(np.uint64), np.unique(ref).size
    assert np.isin(must, bits).all() and must.size <= bits.size <= may, (must.size, bits.size, may)
    # fresh positions next to the batches': seen where the index is one of the batches', unseen otherwise
    extra = random_positions(oracle, O, n, 4, 200, 77, max_ply=60)
    xplanes = _planes(oracle, extra, n)
    xdots = T.simhash_dots(w, xplanes).numpy()
    xdecided = (np.abs(xdots) > T.simhash_margin(w, xplanes).numpy()).all(axis=1)
    f = dict(decided=np.concatenate([decided & ~np.isin(ref, unsure), xdecided & ~np.isin(reference_indices(xdots), unsure)]),
             colliding=np.zeros(len(arr) + 200, bool))
    all_arr, all_acts = np.concatenate([arr, O.states_array(extra)]), [O.possible_moves(oracle, s) for s in states + extra]
    seen = np.isin(np.concatenate([ref, reference_indices(xdots)]), ref[decided])
    var = hash_net.net.policy_value_uncertainty(all_arr, all_acts)[2]
    s, u = check_variances(f, var, len(all_arr), c, seen, loop)
    assert s >= f["decided"][:len(arr)].sum() >= (1 - MAX_UNDECIDED_POSITIONS) * len(arr) and u >= 50, (s, u)
    fresh = A.Net(arch=A.ARCH_NET4_SIMHASH, precision=A.PREC_F16).load_tensors(w)
    fresh.load_bitset(os.path.join(d, "bitvec.bin"))
    assert np.array_equal(fresh.policy_value_uncertainty(all_arr, all_acts)[2].view(np.uint32), var.view(np.uint32))
    fresh.close()
    hash_net.net.close()
    os.remove(os.path.join(d, "bitvec.bin"))
