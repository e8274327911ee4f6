"""`--arch net4_ensemble` in the example programs: selfplay_cli on a directory whose model_latest.ot was written by tz_net_save.  The
three-move run must exit 0 having loaded that model; whatever target lines it wrote must parse.  No 4x4 game ends within three moves
of its opening, so the lines that carry the `ube` column come from a second, longer run of the same command line: they must parse
(tz_parse_targets) and their ube column must not be constant - the search saw this net's variance."""
import os
import subprocess

import numpy as np
import pytest

from gpu_util import require_gpu
from test_gpu_ensemble_search import spread_weights
from test_gpu_native_driver import _build_example, _fields

pytestmark = pytest.mark.gpu


def test_selfplay_program_runs_the_ensemble_net(tmp_path):
    A = require_gpu()
    from takzero_amd import formats as F

    exe = _build_example(tmp_path, "selfplay_cli")
    d = str(tmp_path / "run")
    os.makedirs(d)
    net = A.Net(arch=A.ARCH_NET4_ENSEMBLE).load_tensors(spread_weights())
    net.save(os.path.join(d, "model_latest.ot"))                      # tz_net_save: a LibTorch archive with the 64 `ensemble head i.*`
    net.close()
    assert sorted(os.listdir(d)) == ["model_latest.ot"]               # no set of seen positions beside it
    open(os.path.join(d, "buffer_lengths.txt"), "w").write(F.format_buffer_lengths(0, 0))
    play = [exe, "--directory", d, "--arch", "net4_ensemble", "--games", "32", "--sims", "8", "--sampled-actions", "4", "--search", "gumbel",
            "--wait-limit", "5"]

    def lines():
        path = os.path.join(d, "targets-selfplay.txt")
        data = open(path, "rb").read() if os.path.exists(path) else b""
        targets, used, skipped = F.parse_targets(data, 4, 4)          # tz_parse_targets
        assert used == len(data) and skipped == 0
        return targets, data.decode()

    first = subprocess.run(play + ["--moves", "3", "--seed", "9"], capture_output=True, text=True, timeout=300)
    assert first.returncode == 0, (first.stdout, first.stderr[-1500:])
    f1 = _fields(first.stdout)
    assert f1["moves"] == "3" and int(f1["model_reloads"]) >= 1
    parsed, text = lines()
    assert len(parsed) == int(f1["targets"]) == text.count("\n")
    second = subprocess.run(play + ["--moves", "40", "--seed", "10"], capture_output=True, text=True, timeout=300)
    assert second.returncode == 0, (second.stdout, second.stderr[-1500:])
    parsed, text = lines()
    assert len(parsed) == text.count("\n") >= 64
    ube = np.array([t[4] for t in parsed], np.float64)
    print("%d target lines, ube column between %.4g and %.4g" % (len(ube), ube.min(), ube.max()))
    assert np.isfinite(ube).all() and ube.min() >= 0 and ube.std() > 1e-4
