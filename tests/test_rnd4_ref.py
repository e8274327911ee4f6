"""net4_rnd without a GPU: the numpy reference of its RND towers (tests/rnd4_ref.py) against torch.nn modules and against its own
sensitivity, the variable names and model files, the fixture the GPU tests measure on, and the example programs' --arch name."""
import os
import re
import subprocess

import numpy as np
import pytest

import rnd4_fixture as FX
import rnd4_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_arch_constant_has_one_value_everywhere():
    from takzero_amd import _lib
    from takzero_amd import api as A
    from takzero_amd import weights as W

    header = open(os.path.join(ROOT, "include", "takzero_hip.h")).read()
    archs = {k: int(v) for k, v in re.findall(r"^#define\s+(TZ_ARCH_\w+)\s+(\d+)\s*$", header, flags=re.M)}
    assert archs["TZ_ARCH_NET4_RND"] == 34 and list(archs.values()).count(34) == 1, archs
    assert A.ARCH_NET4_RND == W.ARCH_NET4_RND == 34
    sys_rs = open(os.path.join(ROOT, "bindings", "takzero-hip-sys", "src", "lib.rs")).read()
    assert re.findall(r"pub const TZ_ARCH_NET4_RND: c_int = (\d+);", sys_rs) == ["34"]
    assert "pub fn tz_net_rnd_raw(" in sys_rs and re.search(r"^int tz_net_rnd_raw\(", header, flags=re.M) and "tz_net_rnd_raw" in _lib.SYMBOLS
    assert "pub fn rnd_raw(" in open(os.path.join(ROOT, "bindings", "takzero-hip", "src", "lib.rs")).read()


def test_arch_name_of_the_example_programs(tmp_path):
    src = tmp_path / "arch.cpp"
    src.write_text('#include <cstdio>\n#include "takzero_hip.h"\n#include "arch_arg.h"\n'
                   'int main(int c, char** v) { int a = arch_from_arg(v[1]); printf("%d %d %d\\n", a, arch_board(a), (int)arch_has_set(a)); return 0; }\n')
    exe = str(tmp_path / "arch")
    subprocess.run(["g++", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "examples"), str(src), "-o", exe], check=True)
    out = lambda a: subprocess.run([exe, a], capture_output=True, text=True, check=True).stdout.split()
    assert out("net4_rnd") == ["34", "4", "0"] and out("34") == ["34", "4", "0"] and out("net4_simhash") == ["4", "4", "1"]
    for name in ("selfplay_cli", "reanalyze_cli", "evaluation_cli", "analysis_cli", "learn_cli"):
        assert "|net4_rnd|" in open(os.path.join(ROOT, "examples", name + ".cpp")).read(), name


def test_init_weights():
    from takzero_amd import weights as W

    w = W.init_weights(W.ARCH_NET4_RND, seed=3)
    s = W.init_weights(W.ARCH_NET4_SIMHASH, seed=3)
    keys = list(w)
    assert keys[keys.index("ube.linear.bias") + 1:] == R.tensor_names() and len(R.tensor_names()) == 2 * (2 + 10 * 5) + 2
    assert all(np.array_equal(w[k], s[k]) for k in s if k != "simhash_matrix") and "simhash_matrix" not in w
    assert all(v.dtype == np.float32 for v in w.values())
    for t in R.TOWERS:
        assert w[t + ".layer_norm.weight"].shape == (28, 4, 4) and (w[t + ".layer_norm.weight"] == 1).all() and (w[t + ".layer_norm.bias"] == 0).all()
        assert w[t + ".input_conv2d.weight"].shape == (32, 28, 3, 3) and w[t + ".res_block_3.b.conv2d.weight"].shape == (32, 32, 3, 3)
        assert w[t + ".last_small_block.batch_norm.running_var"].shape == (32,)
    assert not np.array_equal(w["rnd_predictor.input_conv2d.weight"], w["rnd_target.input_conv2d.weight"])
    assert w["min"].tolist() == [0.0] and w["max"].tolist() == [1.0]
    assert W.arch_board(W.ARCH_NET4_RND) == 4 and W.arch_blocks(W.ARCH_NET4_RND) == 16


# ---- the reference against torch.nn
def _torch_tower(w, prefix):
    import torch
    from torch import nn

    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch.float64)

    def small(conv, norm, cin):
        c, b = nn.Conv2d(cin, 32, 3, padding=1, bias=False).double(), nn.BatchNorm2d(32, eps=1e-5).double()
        c.weight.data = t64(w[conv + ".weight"])
        b.weight.data, b.bias.data = t64(w[norm + ".weight"]), t64(w[norm + ".bias"])
        b.running_mean.data, b.running_var.data = t64(w[norm + ".running_mean"]), t64(w[norm + ".running_var"])
        return nn.Sequential(c, b).eval()

    ln = nn.LayerNorm([28, 4, 4], eps=1e-5).double()
    ln.weight.data, ln.bias.data = t64(w[prefix + ".layer_norm.weight"]), t64(w[prefix + ".layer_norm.bias"])
    names = R.layer_names(prefix)
    mods = [small(*names[0], 28)] + [small(*n, 32) for n in names[1:]]

    def forward(x):
        with torch.no_grad():
            x = torch.relu(mods[0](ln(x)))
            for b in range(4):
                x = torch.relu(mods[2 + 2 * b](torch.relu(mods[1 + 2 * b](x))) + x)
            return mods[9](x).flatten(1, 3)
    return forward


def _random_case(seed, count=24):
    from takzero_amd import weights as W

    w = W.init_weights(W.ARCH_NET4_RND, seed=seed, trained_stats=True)
    rng = np.random.default_rng(seed)
    for t in R.TOWERS:
        w[t + ".layer_norm.weight"] = rng.normal(1, 0.3, size=(28, 4, 4)).astype(np.float32)
        w[t + ".layer_norm.bias"] = rng.normal(0, 0.3, size=(28, 4, 4)).astype(np.float32)
    planes = (rng.random((count, 28, 4, 4)) < 0.3).astype(np.float64) + rng.random((count, 28, 1, 1)) * (rng.random((1, 28, 1, 1)) < 0.2)
    return w, planes


def test_reference_against_torch_modules():
    import torch

    w, planes = _random_case(5)
    assert any(np.abs(w[k]).max() > 0.01 for k in w if k.endswith("running_mean"))
    p, t = (_torch_tower(w, name)(torch.from_numpy(planes)) for name in R.TOWERS)
    want = (p - t).square().sum(dim=1).numpy()
    got = R.raw(w, planes, "f64")
    rel = np.abs(got - want).max() / np.abs(want).max()
    print("reference against torch.nn: relative difference %.3g, raw between %.4g and %.4g" % (rel, want.min(), want.max()))
    assert rel < 1e-12 and want.std() > 0
    for name in R.TOWERS:
        a, b = R.tower(w, name, planes, "f64").reshape(len(planes), -1), _torch_tower(w, name)(torch.from_numpy(planes)).numpy()
        assert np.abs(a - b).max() < 1e-12 * np.abs(b).max()


@pytest.mark.parametrize("switch", [dict(sample_variance=True), dict(ln_eps=0.0), dict(last_block_relu=False), dict(final_relu=True)],
                         ids=lambda s: next(iter(s)))
def test_reference_notices_a_wrong_graph(switch):
    """Each mistake moves raw by more than the tolerance the GPU tests hold the kernel to on the fixture (relative to raw's size)."""
    w, planes = _random_case(6)
    if "ln_eps" in switch:      # eps matters where a position's variance is small: scale the planes down (reserve planes of an almost empty board)
        planes = planes * 1e-3
    good, bad = R.raw(w, planes, "f64"), R.raw(w, planes, "f64", **switch)
    tol = 8 * np.abs(R.raw(w, planes, "emu32").astype(np.float64) - R.raw(w, planes, "emu64")).max()
    moved = np.abs(good - bad).max()
    print("%s moves raw by up to %.3g (tolerance of this case %.3g)" % (switch, moved, tol))
    assert moved > tol > 0


def test_reference_notices_min_and_max_swapped():
    raw = np.linspace(0.0, 10.0, 41)
    good, bad = R.local(raw, 2.0, 8.0), R.local(raw, 2.0, 8.0, swapped=True)
    assert good[0] == 0 and good[-1] == 4 and bad[0] == 4 and bad[-1] == 0 and np.abs(good - bad).max() == 4
    assert np.array_equal(R.variance(np.full(41, 0.5), good), np.maximum(good, 0.5))


def test_storage_emulation_rounds_where_the_kernel_stores():
    w, planes = _random_case(7)
    f64, e64, e32, f32 = (R.raw(w, planes, m).astype(np.float64) for m in ("f64", "emu64", "emu32", "f32"))
    assert 0 < np.abs(e32 - e64).max() < np.abs(e64 - f64).max() < 0.05 * f64.max()      # accumulation type < fp16 storage < the signal
    assert 0 < np.abs(f32 - f64).max() < np.abs(e64 - f64).max()


def test_exact_towers():
    for seed in (0, 1):
        w, total = R.exact_towers(seed)
        planes = (np.random.default_rng(seed).random((3, 28, 4, 4)) < 0.3).astype(np.float64)
        for mode in ("f64", "f32", "emu64", "emu32"):
            got = R.raw(w, planes, mode)
            # the folded modes see the BatchNorm scale the library folds, exactly 1; as a layer in fp64 it is 1 + 7e-9 (running_var is
            # a float32 and eps is not), which sums of +-4000 next to biases of their size and nine layers of gain carry to 1e-3 of raw
            assert (np.abs(got - total).max() < 2e-3 * total) if mode == "f64" else (got == total).all(), (seed, mode, got, total)
        for t in R.TOWERS:
            assert len(set(w[t + ".layer_norm.bias"].ravel().tolist())) == 448
            assert all(len({w[c + ".weight"][:, :, tap // 3, tap % 3].tobytes() for tap in range(9)}) == 9 for c, _ in R.layer_names(t))
    assert R.exact_towers(0)[1] != R.exact_towers(1)[1]


# ---- names and files
def _small_store():
    """net4_rnd's variable names on ARCH_TEST's trunk with one block: a small archive."""
    from takzero_amd import weights as W

    w = W.init_weights(W.ARCH_TEST, n=4, blocks=1, seed=5, trained_stats=True)
    full = W.init_weights(W.ARCH_NET4_RND, seed=5, trained_stats=True)
    for k in R.tensor_names():
        w[k] = full[k]
    w["min"], w["max"] = np.array([123.456], np.float32), np.array([789.987], np.float32)
    return w


def _same(a, b):
    return set(a) == set(b) and all(np.asarray(a[k]).shape == np.asarray(b[k]).shape and
                                    np.array_equal(np.asarray(a[k], np.float32).view(np.uint32), np.asarray(b[k], np.float32).view(np.uint32)) for k in a)


def _want_tch_names():
    """Creation order of net4_rnd.rs:169-189 from ube on, counting variables for the `__N` suffixes (trunk: 1 + 4 + 1 block of 10 + 10 head variables)."""
    out, count = [], 1 + 4 + 10 + 10
    for t in R.TOWERS:
        names = [t + ".layer_norm.weight", t + ".layer_norm.bias", t + ".input_conv2d.weight"] + [t + ".batch_norm." + v for v in ("weight", "bias", "running_mean", "running_var")]
        for b in range(4):
            first = ["%s.res_block_%d.conv2d.weight" % (t, b)] + ["%s.res_block_%d.batch_norm.%s" % (t, b, v) for v in ("weight", "bias", "running_mean", "running_var")]
            names += first + ["%s__%d" % (n, count + len(names) + 5 + i) for i, n in enumerate(first)]
        names += [t + ".last_small_block.conv2d.weight"] + [t + ".last_small_block.batch_norm." + v for v in ("weight", "bias", "running_mean", "running_var")]
        out += names
        count += len(names)
    return out + ["min", "max"]


def test_tch_names_and_their_inverse():
    from takzero_amd import ot

    w = _small_store()
    named = ot.tch_names(w)
    got = [n for n, _ in named]
    assert got[got.index("ube.linear.bias") + 1:] == _want_tch_names()
    assert got[got.index("rnd_predictor.res_block_0.conv2d.weight") + 5] == "rnd_predictor.res_block_0.conv2d.weight__37"
    assert _same(ot.canonical_names(dict(named)), w)
    from takzero_amd import weights as W
    full = [n for n, _ in ot.tch_names(W.init_weights(W.ARCH_NET4_RND))]
    assert len(full) == len(set(full)) == 5 + 16 * 10 + 10 + 2 * 52 + 2 and full[-2:] == ["min", "max"]


@pytest.mark.parametrize("arch", ["NET4_SIMHASH", "NET5", "NET6_SIMHASH", "NET4_LCGHASH", "NET4_ENSEMBLE", "NET4_RND", "TEST"])
def test_tch_names_keep_every_tensor_of_every_architecture(arch):
    """net5's RND MLP shares the prefix `rnd_target.` with net4_rnd's second tower: neither may lose a variable to the other's rule."""
    from takzero_amd import ot
    from takzero_amd import weights as W

    w = W.init_weights(getattr(W, "ARCH_" + arch), n=5, blocks=2)
    named = ot.tch_names(w)
    assert len(named) == len(w) == len({n for n, _ in named})
    assert _same(ot.canonical_names(dict(named)), w)
    if arch == "NET5":
        names = [n for n, _ in named]
        assert names[-2:] == ["min", "max"] and names[-8:-2] == ["rnd_target.%s.%s" % (l, p) for l in ("input_linear", "hidden_linear", "final_linear") for p in ("weight", "bias")]


def test_ot_native_writer_and_reader(tmp_path):
    from takzero_amd import ot

    w = _small_store()
    path = ot.save_ot(tmp_path / "model_latest.ot", w)
    assert _same(ot.load_ot(path), w)
    named = ot.read_ot_libtorch(path)      # an archive saved by the library, read by LibTorch
    assert list(named) == [n for n, _ in ot.tch_names(w)] and _same(ot.canonical_names(named), w)
    assert named["rnd_target.layer_norm.weight"].shape == (28, 4, 4)


def test_ot_native_reader_against_libtorchs_writer(tmp_path):
    from takzero_amd import ot

    try:
        ot.build_writer()
    except RuntimeError as e:
        pytest.skip(str(e))
    w = _small_store()
    path = ot.save_ot_libtorch(tmp_path / "model_latest.ot", w)      # LibTorch's own writer, read by tz_weights_convert
    assert _same(ot.load_ot(path), w)


# ---- the fixture of tests/test_gpu_rnd4.py
def test_fixture_covers_the_variance_rule(oracle):
    fx = FX.fixture(oracle)
    n = len(fx["raw64"])
    loc, e = fx["local"], float(np.exp(np.float64(fx["c"])))
    low, high, inside = int((loc == 0).sum()), int((loc == 4).sum()), (loc > 0) & (loc < 4)
    wins = int((e > loc[inside]).sum())
    close = int((np.abs(e - loc) <= fx["var_tol"]).sum())
    print("fixture: %d positions, raw %.4g .. %.4g, min %.6g max %.6g, %d at 0, %d at 4, %d inside, exp(c) = %.4g wins on %d of them; "
          "bounds: raw %.3g (8 x %.3g), emulation against fp64 %.3g, variance %.3g; f32: raw %.3g, variance %.3g; %d positions within the tolerance of the tie"
          % (n, fx["raw64"].min(), fx["raw64"].max(), fx["min"], fx["max"], low, high, int(inside.sum()), e, wins, fx["raw_tol"], fx["raw_tol"] / 8,
             fx["emu_dist"], fx["var_tol"], fx["raw_tol_f32"], fx["var_tol_f32"], close))
    assert n == 1025 and low >= 80 and high >= 80 and inside.sum() >= 300
    assert 0.4 * inside.sum() <= wins <= 0.6 * inside.sum()
    assert close < 0.05 * n and int((np.abs(e - loc) <= fx["var_tol_f32"]).sum()) < 0.05 * n
    assert 0 < fx["raw_tol"] < 0.01 * (fx["max"] - fx["min"]) and 0 < fx["raw_tol_f32"] < fx["raw_tol"]
