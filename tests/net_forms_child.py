"""Child of tests/test_gpu_net_forms.py::test_switched_paths: runs under the environment switches its parent set (TZ_TOWER, TZ_CONV_CFG,
TZ_NET_SPLIT are read once per process).  argv[1] is a directory holding states_N.npy, exact_N.tzw and dense_N.tzw for N = 3..6; for
every board size and both 16-bit storage types it writes out_N_PREC.npz with policy, value and UBE of the first 1, 37 and 1030 positions.
It compares nothing: the parent does."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import takzero_amd.api as A  # noqa: E402
from exact_net import NETS  # noqa: E402


def main(d):
    assert A._lib.load().tz_device_count() > 0, "no HIP device"
    for n, (arch, _, blocks) in NETS.items():
        arr = np.load(os.path.join(d, "states_%d.npy" % n)).view(A._lib.STATE_DTYPE).reshape(-1)
        for name, prec in (("bf16", A.PREC_BF16), ("f16", A.PREC_F16)):
            out = {}
            net = A.Net(arch=arch, n=n, precision=prec, blocks=blocks)
            for kind in ("exact", "dense"):
                net.load(os.path.join(d, "%s_%d.tzw" % (kind, n)))
                for size in (1, 37, 1030):
                    for k, x in enumerate(net.forward_raw(arr[:size])):
                        out["%s_%d_%d" % (kind, size, k)] = x
            net.close()
            np.savez(os.path.join(d, "out_%d_%s.npz" % (n, name)), **out)


if __name__ == "__main__":
    main(sys.argv[1])
