"""A search handle's captured simulation graph against what happens to the net4_ensemble it names, in the style of
tests/test_gpu_graph_lifetime.py: a twin net of the same tensors and a twin search created under TZ_NO_GRAPH=1 are fed the same calls,
and after every phase both handles must be equal in every byte.

A capture names the net's work buffers by value, among them the image the fused launch stores for the ensemble heads and the heads'
values (tz_net_ensure_batch frees and replaces both with the rest), and the heads' weights (a load replaces them).  Between simulations
a host-side ensemble_values call larger than the search's batch grows the buffers, a larger handle on the same net runs, and the weights
are reloaded with other heads; a replay that still named the old buffers would read freed memory."""
import numpy as np
import pytest

import ensemble_ref as R
from gpu_util import require_gpu
from test_gpu_ensemble import world
from test_gpu_ensemble_search import spread_weights
from test_gpu_graph_lifetime import Twins, _bytes_equal

pytestmark = pytest.mark.gpu


def test_larger_call_larger_handle_and_reload_under_a_captured_search(oracle, monkeypatch):
    A = require_gpu()
    B, n = 32, 4
    w = spread_weights()
    arr = world(oracle)["arr"]
    t = Twins(A, monkeypatch, lambda: A.Net(arch=A.ARCH_NET4_ENSEMBLE, precision=A.PREC_F16).load_tensors(w))
    gpu, twin = t.search(B, n, 1 << 12)
    choice = (np.arange(B) * 3 + 1).astype(np.int32) % 16
    gpu.new_openings(choice)
    twin.new_openings(choice)
    betas = np.where(np.arange(B) % 2 == 0, 0.5, 0.25).astype(np.float32)

    def simulate(where):
        for s, tw in t.pairs:
            s.simulate(betas[:1].repeat(s.batch) if s.batch != B else betas, 8)        # two eager simulations, one captured, five replayed
            tw.simulate(betas[:1].repeat(tw.batch) if tw.batch != B else betas, 8)
        t.check(where)

    simulate("first")
    out = [net.ensemble_values(arr[:300]) for net in t.nets]           # a host-side call larger than the search's batch: new buffers
    _bytes_equal(out[0], out[1], "ensemble_values 300")
    simulate("after a larger host-side call")
    big, big_twin = t.search(128, n, 1 << 11)                          # a larger handle on the same net
    wide = (np.arange(128) * 7 + 3).astype(np.int32) % 16
    big.new_openings(wide)
    big_twin.new_openings(wide)
    simulate("with a larger handle")
    other = dict(w)
    for i in range(16):                                                # a reload: other heads (and so another variance) under the capture
        other[R.name(i, "linear.bias")] = w[R.name(i, "linear.bias")] + np.float32(0.5 - i / 16.0)
    before = t.nets[0].ensemble_values(arr[:B])
    for net in t.nets:
        net.load_tensors(other)
    after = [net.ensemble_values(arr[:B]) for net in t.nets]
    _bytes_equal(after[0], after[1], "ensemble_values after the reload")
    assert not np.array_equal(before, after[0])
    simulate("after the reload")
    t.finish(oracle, 4)
