"""A search handle's captured simulation graph against what happens to the net4_lcghash it names, in the style of
tests/test_gpu_graph_lifetime.py: a twin net and a twin search created under TZ_NO_GRAPH=1 are fed the same calls, and after every
phase both handles must be equal in every byte.

A capture holds lcghash_init and the set's pointer by value.  Between simulations the weights are reloaded with another lcghash_init
(which frees the old tensor) and another set is loaded (which frees the old bitset); a replay that still named the old ones would read
freed memory, and - where the allocator hands the same addresses out again - at best the old values.  The roots are then set to
positions of which the reference says which are in the new set under the new init, and their children's std_dev is exactly
sqrtf(1) = 1 (seen, expf(0) = 1) or sqrtf(4) = 2 (unseen)."""
import os

import numpy as np
import pytest

import lcghash_ref as R
from gpu_util import require_gpu
from test_gpu_graph_lifetime import Twins, _bytes_equal
from test_gpu_lcghash import C4, COUNT, EXHAUSTED_SLOTS, N4, constant_ube, lcg_fixture, write_bits_file

pytestmark = pytest.mark.gpu


def test_reload_and_load_bitset_under_a_captured_search(oracle, monkeypatch, tmp_path):
    A = require_gpu()
    f = lcg_fixture(oracle)
    B, n = 32, 4
    w = constant_ube(f["w"], 0.0)
    t = Twins(A, monkeypatch, lambda: A.Net(arch=A.ARCH_NET4_LCGHASH, precision=A.PREC_F16).load_tensors(w))
    gpu, twin = t.search(B, n, 1 << 12)
    choice = (np.arange(B) * 3 + 1).astype(np.int32) % 16
    gpu.new_openings(choice)
    twin.new_openings(choice)
    betas = np.where(np.arange(B) % 2 == 0, 0.0, 0.25).astype(np.float32)
    rng = np.random.default_rng(31)
    inits = [rng.uniform(-100, 100, size=(C4, N4, N4)).astype(np.float32) for _ in range(2)]
    roots = np.flatnonzero((np.arange(COUNT) >= 1000) & ~np.isin(np.arange(COUNT), EXHAUSTED_SLOTS))[:B]
    for phase in range(3):
        gpu.simulate(betas, 8)                   # two eager simulations, one captured, five replayed
        twin.simulate(betas, 8)
        t.check("simulate %d" % phase)
        if phase == 2:
            break
        init = inits[phase]
        ref = R.indices(f["planes"], init)
        for net in t.nets:                       # a reload replaces lcghash_init ...
            net.load_tensors(dict(w, lcghash_init=init))
        out = [net.hash_indices(f["arr"][:300]) for net in t.nets]
        _bytes_equal(out[0], out[1], "hash_indices")
        assert np.array_equal(out[0], ref[:300])
        in_file = np.unique(ref[roots[phase::2]])
        path = tmp_path / "bitvec.bin"
        write_bits_file(path, in_file)
        for net in t.nets:                       # ... and a new set replaces the bitset pointer
            net.load_bitset(path)
        os.remove(path)
        seen = np.isin(ref[roots], in_file)
        assert 8 <= seen.sum() <= B - 8
        for s in (gpu, twin):
            s.set_positions(np.arange(B), f["arr"][roots])
            s.simulate(betas, 1)
        t.check("after reload %d" % phase)
        info, ch = gpu.root_info(), gpu.root_children()
        assert np.all(info["n_children"] > 0)
        for g in range(B):
            std = ch["std_dev"][g, :info["n_children"][g]]
            assert np.all(std == np.float32(1.0 if seen[g] else 2.0)), (phase, g, bool(seen[g]), std[:4])
    t.finish(oracle, 4)
