"""`--arch net4_lcghash` in the example programs: selfplay_cli and learn_cli in a closed loop on one directory, three processes one
after the other so that nothing depends on their timing.  Self-play from Net::new writes targets; learn trains on them, updates the
LCG-hash set with every batch and writes model_latest.ot with bitvec.bin beside it; self-play started again picks both up."""
import os
import subprocess

import numpy as np
import pytest

from gpu_util import require_gpu
from test_gpu_lcghash import C4, N4, set_bits_of_file
from test_gpu_native_driver import _build_example, _fields

pytestmark = pytest.mark.gpu


def test_selfplay_and_learn_programs_close_the_loop(tmp_path):
    A = require_gpu()
    from takzero_amd import formats as F
    from takzero_amd import ot

    selfplay, learn = _build_example(tmp_path, "selfplay_cli"), _build_example(tmp_path, "learn_cli")
    d = str(tmp_path / "run")
    os.makedirs(d)
    open(os.path.join(d, "buffer_lengths.txt"), "w").write(F.format_buffer_lengths(0, 0))
    play = [selfplay, "--directory", d, "--arch", "net4_lcghash", "--games", "32", "--sims", "8", "--sampled-actions", "4", "--search", "gumbel",
            "--wait-limit", "5"]
    first = subprocess.run(play + ["--moves", "40", "--seed", "9"], capture_output=True, text=True, timeout=300)
    assert first.returncode == 0, (first.stdout, first.stderr[-1500:])
    f1 = _fields(first.stdout)
    assert f1["moves"] == "40" and f1["model_reloads"] == "0" and int(f1["targets"]) >= 128
    steps, batch = 4, 64
    lr = subprocess.run([learn, "--directory", d, "--arch", "net4_lcghash", "--batch", str(batch), "--steps", str(steps), "--seed", "5",
                         "--pre-training-steps", "0", "--min-selfplay", "128", "--steps-per-save", "2", "--steps-per-checkpoint", "1000",
                         "--steps-before-reanalyze", "1000", "--read-interval", "0.1", "--sleep", "0.1", "--wait-limit", "60"],
                        capture_output=True, text=True, timeout=300)
    assert lr.returncode == 0, (lr.stdout, lr.stderr[-1500:])
    lf = _fields(lr.stdout)
    assert lf["model_steps"] == str(steps) and lf["rc"] == "0"
    names = sorted(os.listdir(d))
    assert "model_0000000.ot" in names and "model_latest.ot" in names and "bitvec.bin" in names, names
    bits = set_bits_of_file(os.path.join(d, "bitvec.bin"))
    assert 1 <= bits.size <= steps * batch, bits.size              # update_counts of every batch: at most one index per position
    start, latest = ot.load_ot(os.path.join(d, "model_0000000.ot")), ot.load_ot(os.path.join(d, "model_latest.ot"))
    assert start["lcghash_init"].shape == (C4, N4, N4)
    assert np.array_equal(start["lcghash_init"].view(np.uint32), latest["lcghash_init"].view(np.uint32))       # carried, not trained
    assert not np.array_equal(start["core.res_block_0.b.conv2d.weight"], latest["core.res_block_0.b.conv2d.weight"])   # the trunk was
    # a net of the arch picks the model and the set up from the directory, as self-play does
    net = A.Net(arch=A.ARCH_NET4_LCGHASH).load(os.path.join(d, "model_latest.ot"))
    net.save_bitset(os.path.join(d, "copy.bin"))
    assert np.array_equal(set_bits_of_file(os.path.join(d, "copy.bin")), bits)
    os.remove(os.path.join(d, "copy.bin"))
    net.close()
    second = subprocess.run(play + ["--moves", "5", "--seed", "10"], capture_output=True, text=True, timeout=300)
    assert second.returncode == 0, (second.stdout, second.stderr[-1500:])
    f2 = _fields(second.stdout)
    assert f2["moves"] == "5" and int(f2["model_reloads"]) >= 1
    os.remove(os.path.join(d, "bitvec.bin"))
    bad = subprocess.run([selfplay, "--directory", d, "--arch", "net4_nothing", "--moves", "1"], capture_output=True, text=True, timeout=60)
    assert bad.returncode != 0 and "unknown architecture" in bad.stderr
