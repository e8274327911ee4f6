"""numpy reference of net4_rnd's two RND towers and its variance rule (net4_rnd.rs:126-166, 210-230, 289-297; residual.rs:8-63).

A tower: LayerNorm([28,4,4]) (elementwise affine, eps 1e-5, population variance over a position's 448 elements), conv 3x3 28->32
without bias + BatchNorm (eps 1e-5) + ReLU, four ResidualBlock(32, 32) = relu(conv+BN(relu(conv+BN(x))) + x), SmallBlock(32, 32) =
conv + BN without ReLU, 512 outputs.  raw = sum_512 (predictor - target)^2; local = clamp((raw - min) / (max - min), 0, 1) * 4;
variance = clamp(max(exp(ube), local), 0, 4).

`raw(w, planes, mode)`:
  "f64"    the graph as written, BatchNorm applied as a layer, everything fp64
  "f32"    BatchNorm folded in fp32 the way the library folds it (scale into the weights, the rest a bias), everything fp32: the
           arithmetic of the TZ_PREC_F32 kernel up to summation order
  "emu64"  storage emulation of the MFMA kernel: folded weights held as fp16, every stored activation (the LayerNorm output and the
           nine ReLU outputs of a tower) rounded to fp16, the last layer's outputs, the difference and the sum not rounded; sums in fp64
  "emu32"  the same with the LayerNorm statistics and every sum in fp32
The keyword switches break the graph one way each (tests/test_rnd4_ref.py holds the reference to noticing them)."""
import numpy as np

CIN, N, FILTERS, BLOCKS, OUT, EPS = 28, 4, 32, 4, 512, 1e-5
TOWERS = ("rnd_predictor", "rnd_target")
MAXIMUM_VARIANCE = 4.0


def layer_names(prefix):
    """(conv, batch norm) paths of a tower's ten layers in order, `.a.` / `.b.` spelling."""
    out = [(prefix + ".input_conv2d", prefix + ".batch_norm")]
    for b in range(BLOCKS):
        for half in "ab":
            p = "%s.res_block_%d.%s" % (prefix, b, half)
            out.append((p + ".conv2d", p + ".batch_norm"))
    out.append((prefix + ".last_small_block.conv2d", prefix + ".last_small_block.batch_norm"))
    return out


def tensor_names():
    """Every variable net4_rnd has beyond net4_simhash's trunk and heads."""
    out = []
    for t in TOWERS:
        out += [t + ".layer_norm.weight", t + ".layer_norm.bias"]
        for conv, norm in layer_names(t):
            out.append(conv + ".weight")
            out += [norm + "." + v for v in ("weight", "bias", "running_mean", "running_var")]
    return out + ["min", "max"]


def conv3x3(x, wt):
    """x [B,C,4,4], wt [co,C,3,3], padding 1, in x's dtype (cross-correlation, as torch conv2d)."""
    b, c = x.shape[:2]
    xp = np.zeros((b, c, N + 2, N + 2), x.dtype)
    xp[:, :, 1:N + 1, 1:N + 1] = x
    cols = np.stack([xp[:, :, ky:ky + N, kx:kx + N] for ky in range(3) for kx in range(3)], axis=2)      # [B,C,9,4,4]
    cols = np.ascontiguousarray(cols.transpose(0, 3, 4, 1, 2)).reshape(b * N * N, c * 9)
    y = cols @ np.ascontiguousarray(wt.reshape(wt.shape[0], c * 9).astype(x.dtype).T)
    return y.reshape(b, N, N, wt.shape[0]).transpose(0, 3, 1, 2)


def fold_f32(w, conv, norm):
    """bn_fold of the library in fp32: (weights * scale, bias)."""
    f = np.float32
    g, b, mean, var = (np.asarray(w[norm + "." + v], f) for v in ("weight", "bias", "running_mean", "running_var"))
    scale = (g / np.sqrt(var + f(EPS))).astype(f)
    bias = (b - (mean * scale).astype(f)).astype(f)
    return (np.asarray(w[conv + ".weight"], f) * scale[:, None, None, None]).astype(f), bias


def layer_norm(x, weight, bias, dtype, sample_variance=False, eps=EPS):
    x = x.astype(dtype)
    flat = x.reshape(len(x), -1)
    mean = flat.sum(axis=1, dtype=dtype) / dtype(flat.shape[1])
    d = flat - mean[:, None]
    var = (d * d).sum(axis=1, dtype=dtype) / dtype(flat.shape[1] - (1 if sample_variance else 0))
    xh = d * (dtype(1) / np.sqrt(var + dtype(eps)))[:, None]
    return (xh.reshape(x.shape) * np.asarray(weight, dtype)[None] + np.asarray(bias, dtype)[None]).astype(dtype)


def tower(w, prefix, planes, mode="f64", sample_variance=False, ln_eps=EPS, last_block_relu=True, final_relu=False):
    """The 512 outputs as [B,32,4,4]."""
    emu = mode.startswith("emu")
    dtype = np.float64 if mode in ("f64", "emu64") else np.float32
    store = (lambda a: a.astype(np.float16).astype(dtype)) if emu else (lambda a: a)
    relu = lambda a: np.maximum(a, dtype(0))
    shape = (CIN, N, N)
    x = layer_norm(np.asarray(planes), np.asarray(w[prefix + ".layer_norm.weight"]).reshape(shape),
                   np.asarray(w[prefix + ".layer_norm.bias"]).reshape(shape), dtype, sample_variance, ln_eps)
    x = store(x)

    def layer(a, names):
        conv, norm = names
        if mode == "f64":
            y = conv3x3(a, np.asarray(w[conv + ".weight"], np.float64))
            g, b, mean, var = (np.asarray(w[norm + "." + v], np.float64)[None, :, None, None] for v in ("weight", "bias", "running_mean", "running_var"))
            return (y - mean) / np.sqrt(var + EPS) * g + b
        wt, bias = fold_f32(w, conv, norm)
        if emu:
            wt = wt.astype(np.float16)
        return (conv3x3(a, wt.astype(dtype)) + bias.astype(dtype)[None, :, None, None]).astype(dtype)

    names = layer_names(prefix)
    x = store(relu(layer(x, names[0])))
    for b in range(BLOCKS):
        t = store(relu(layer(x, names[1 + 2 * b])))
        y = layer(t, names[2 + 2 * b]) + x
        x = store(relu(y) if last_block_relu or b < BLOCKS - 1 else y)
    y = layer(x, names[-1])
    return relu(y) if final_relu else y


def raw(w, planes, mode="f64", chunk=512, **switches):
    """sum_512 (predictor - target)^2 per position (forward_rnd, net4_rnd.rs:210-223), in the mode's accumulation type."""
    out = []
    for lo in range(0, len(planes), chunk):
        p, t = (tower(w, name, planes[lo:lo + chunk], mode, **switches) for name in TOWERS)
        d = (p - t).reshape(len(p), -1)
        out.append((d * d).sum(axis=1, dtype=d.dtype))
    return np.concatenate(out)


def local(raw_values, lo, hi, dtype=np.float64, swapped=False):
    """normalized_rnd (net4_rnd.rs:225-230); `swapped` takes min for max and max for min."""
    r, lo, hi = np.asarray(raw_values, dtype), dtype(lo), dtype(hi)
    if swapped:
        lo, hi = hi, lo
    with np.errstate(divide="ignore", invalid="ignore"):
        q = (r - lo) / (hi - lo)
    return (np.minimum(np.maximum(q, dtype(0)), dtype(1)) * dtype(MAXIMUM_VARIANCE)).astype(dtype)


def variance(exp_ube, local_values):
    """clamp(max(exp(ube), local), 0, 4) (net4_rnd.rs:289-297); exp is handed in (the device's expf in the GPU tests)."""
    e = np.asarray(exp_ube)
    return np.minimum(np.maximum(np.maximum(e, np.asarray(local_values, e.dtype)), e.dtype.type(0)), e.dtype.type(MAXIMUM_VARIANCE))


EXACT_CAP = 16      # the largest stored activation of an exact tower


def exact_towers(seed):
    """Tower variables for which every product, sum and stored activation is a small integer, and the fp64 raw they give (the same
    for every position: the LayerNorm weight is 0, so a tower's input is its LayerNorm bias).

      LayerNorm   weight 0, bias the 448 different integers -224 .. 223 in a random arrangement
      conv        per (output channel, tap) one non-zero weight from {-2, -1, 1, 2} at a random input channel
      BatchNorm   weight 1, running_mean 0, running_var float32(1) - float32(1e-5) (tests/exact_net.py: the folded scale is exactly 1),
                  bias a non-positive integer that brings the channel's largest output on the board down to EXACT_CAP (a channel
                  with nothing above zero is lifted to 1), so that stored activations stay within [0, 16] and every sum within 2^12

    Returns (tensors, raw)."""
    rng = np.random.default_rng(4400 + seed)
    w, outs = {}, []
    for t in TOWERS:
        w[t + ".layer_norm.weight"] = np.zeros((CIN, N, N), np.float32)
        w[t + ".layer_norm.bias"] = (rng.permutation(CIN * N * N) - 224).astype(np.float32).reshape(CIN, N, N)
        x = w[t + ".layer_norm.bias"].astype(np.float64)[None]
        names = layer_names(t)
        keep = None
        for i, (conv, norm) in enumerate(names):
            ci = CIN if i == 0 else FILTERS
            wt = np.zeros((FILTERS, ci, 3, 3), np.float32)
            for co in range(FILTERS):
                for tap in range(9):
                    wt[co, rng.integers(ci), tap // 3, tap % 3] = rng.choice([-2.0, -1.0, 1.0, 2.0])
            pre = conv3x3(x, wt.astype(np.float64))
            second = i >= 2 and i % 2 == 0 and i < len(names) - 1
            if second:
                pre = pre + keep
            top = pre.max(axis=(0, 2, 3))
            bias = np.where(top > EXACT_CAP, EXACT_CAP - top, np.where(top <= 0, 1 - top, 0.0))
            if i == len(names) - 1:
                bias = rng.integers(-3, 4, size=FILTERS).astype(np.float64)
            w[conv + ".weight"] = wt
            w[norm + ".weight"] = np.ones(FILTERS, np.float32)
            w[norm + ".running_mean"] = np.zeros(FILTERS, np.float32)
            w[norm + ".running_var"] = np.full(FILTERS, np.float32(1) - np.float32(1e-5), np.float32)
            w[norm + ".bias"] = bias.astype(np.float32)
            y = pre + bias[None, :, None, None]
            if i < len(names) - 1:
                y = np.maximum(y, 0.0)
                assert y.max() <= EXACT_CAP and (y > 0).any(axis=(0, 2, 3)).all()
                if i % 2 == 0:
                    keep = y
            x = y
        outs.append(x)
    d = outs[0] - outs[1]
    total = float((d * d).sum())
    assert total == np.rint(total) and 0 < total < 2 ** 24 and np.abs(d).max() > 0
    return w, total
