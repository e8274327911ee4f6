"""Child of tests/test_gpu_selection.py::test_switching_the_rule_on_a_live_handle: runs selection_util.switch_case under the
environment its parent set (TZ_NO_GRAPH is read when a search handle is created).  argv[1] is the restatement's library, built by
the parent.  Prints the number of nodes compared; any mismatch is an assertion error."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import takzero_amd.api as A  # noqa: E402
import selection_util as S  # noqa: E402

if __name__ == "__main__":
    assert A._lib.load().tz_device_count() > 0, "no HIP device"
    print("nodes", S.switch_case(A, S.load(sys.argv[1])))
