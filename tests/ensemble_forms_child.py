"""Child of tests/test_gpu_ensemble.py: runs under the environment switches its parent set (TZ_TOWER, TZ_NET_SPLIT are read once per
process).  argv[1] is a directory holding states.npy, exact.tzw (a net4_ensemble store) and sim.tzw (the net4_simhash store of the same
trunk and heads); for every precision but f16c6 it writes out_PREC.npz with ensemble_values, policy, value and UBE of the first SIZES
positions, and policy, value and UBE of the net4_simhash net under the same switches.  It compares nothing: the parent does."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import takzero_amd.api as A  # noqa: E402

SIZES = (1, 64, 65, 128, 129, 300, 305, 1030)
PRECS = ("bf16", "f32", "f16", "f16x2", "f16c8")


def main(d):
    assert A._lib.load().tz_device_count() > 0, "no HIP device"
    arr = np.load(os.path.join(d, "states.npy")).view(A._lib.STATE_DTYPE).reshape(-1)
    for prec in PRECS:
        out = {}
        net = A.Net(arch=A.ARCH_NET4_ENSEMBLE, precision=A.PREC_NAMES[prec]).load(os.path.join(d, "exact.tzw"))
        for size in SIZES:
            out["ens_%d" % size] = net.ensemble_values(arr[:size])
            for k, x in enumerate(net.forward_raw(arr[:size])):
                out["raw_%d_%d" % (size, k)] = x
        net.close()
        sim = A.Net(arch=A.ARCH_NET4_SIMHASH, precision=A.PREC_NAMES[prec]).load(os.path.join(d, "sim.tzw"))
        for size in SIZES:
            for k, x in enumerate(sim.forward_raw(arr[:size])):
                out["sim_%d_%d" % (size, k)] = x
        sim.close()
        np.savez(os.path.join(d, "out_%s.npz" % prec), **out)


if __name__ == "__main__":
    main(sys.argv[1])
