"""Integer-valued networks and all-different positions for the tests of the net kernels' launch forms
(tests/test_net_exact_reference.py holds the generator to its conditions on the CPU, tests/test_gpu_net_forms.py runs the nets).

`exact_weights` builds weights for which every product, every partial sum and every stored activation of the forward is an
integer that fp32, bf16 and fp16 (and with them the hi parts of the split arithmetics, whose lo parts are then exactly zero)
all represent exactly, so that every precision and every launch form must return the same bits as the fp64 graph
(oracle/nets_torch.py `forward(dtype=torch.float64)`, rounded to the grid):

  conv weights   {-1, 0, +1}, two non-zero entries per output channel at random (input channel, tap) places.  In the tower one is +1
                 and the other -1: the difference of two non-negative activations is no larger than the larger of them, so only the
                 residual sum grows, and it grows slowly (with two +1 the largest activation of net5 passes 2^16 on a few hundred
                 positions; a channel with two -1 never passes its ReLU).  The first conv (inputs 0 or 1) and the policy conv
                 (nothing follows it) take +1 and a random sign.  Three or more entries per channel grow past 2^11 in 15 blocks.
  BatchNorm      weight 1, running_mean 0, running_var float32(1) - float32(1e-5): fl32(var + 1e-5f) == 1.0f, so the folded scale
                 (bn_fold, csrc/tz_nn.hip) is exactly 1 and the folded bias is the BatchNorm bias.
  BatchNorm bias a non-positive integer per channel, calibrated layer by layer on `calibration` positions so that about 35 % of the
                 channel's outputs pass the ReLU (0 where a channel would otherwise be dead) and no activation exceeds
                 MAX_CALIBRATED there; the tests assert the bound of 256 (exact in bf16's 8 bits) on the positions they run.
  heads          1x1 conv weights {-1, 0, +1} (16 entries) with an integer bias, linear weights +-2^-s with s chosen so that
                 the value's pre-activation stays within about +-2 (tanh not saturated), linear bias 1/4: sums of dyadic numbers.

The first conv has zero weight on the five scalar input planes that are not dyadic (reserve and capstone ratios of both colours
such as 17/21, flat difference / n^2): each precision stores those differently.  Those planes stay with the dense-weight tests
(tests/test_gpu_net.py and the dense half of tests/test_gpu_net_forms.py); the colour-to-move plane (0 or 1) is used.

`exact_weights_with_lo` gives the same nets a small lo part on every non-zero 3x3 weight, so that the correction products of the split
arithmetics decide output bits; those nets are compared with the CPU emulation of tests/split_emulation.py
(tests/test_split_emulation_reference.py holds nets and emulation to their conditions, tests/test_gpu_split_corrections.py runs them).

`distinct_positions` returns positions that are all different (by their bytes): the opening position, a full board, on 6x6 the
three wide positions of tests/test_gpu_edges.py, then every ply of random playouts."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))

MAX_CALIBRATED = 160      # calibration keeps every activation at or below this on its own positions; the tests assert 256
MAX_ACTIVATION = 256      # integers up to 2^8 are exact in bf16 (8 significant bits), fp16 (11) and fp32 (24)
SURVIVE = 0.35
MIN_SHARE = 0.05
SEEDS = (0, 1, 2)
NETS = {3: (100, 3, 2), 4: (4, 4, 16), 5: (5, 5, 20), 6: (6, 6, 16)}      # board size -> (arch, n, blocks): the test architecture at 3x3, the three shipped nets
WIDE_6X6 = ["x6/x6/x2,212121,212121,x2/x2,212121,212121,x2/x6/x6 1 30",
            "x6/x6/x2,212121,x3/x3,212121,x2/x6/x6 1 20",
            "x6/x,21212121,x4/x6/x3,2121212121,x2/x6/x6 1 30"]


def full_board_tps(n):
    rows = [",".join("12"[(x + y) & 1] for x in range(n)) for y in range(n)]
    return "/".join(rows) + " 1 %d" % (n * n // 2 + 1)


def distinct_positions(oracle, O, n, count, seed, half_komi=4):
    """`count` positions of board size n, all different by their bytes: specials first, then every ply of random playouts."""
    rng = np.random.default_rng(seed)
    out, seen = [], set()

    def add(s):
        key = O.states_array([s]).tobytes()
        if key not in seen:
            seen.add(key)
            out.append(s)

    add(O.state_default(oracle, n, half_komi))
    add(O.state_from_tps(oracle, full_board_tps(n), n, half_komi))
    if n == 6:
        for t in WIDE_6X6:
            add(O.state_from_tps(oracle, t, n, half_komi))
    while len(out) < count:
        s = O.state_default(oracle, n, half_komi)
        for _ in range(8 * n * n):
            if oracle.tzo_terminal(C.byref(s)) != -1:
                break
            mv = O.possible_moves(oracle, s)
            s = O.play(oracle, s, mv[int(rng.integers(len(mv)))])
            if oracle.tzo_terminal(C.byref(s)) == -1:
                add(s)
    out = out[:count]
    arr = O.states_array(out)
    assert len({arr[i:i + 1].tobytes() for i in range(count)}) == count
    return out


def planes_of(oracle, O, states, n):
    return np.stack([O.game_repr(oracle, s) for s in states]).reshape(len(states), -1, n, n)


def dyadic_input_channels(n):
    """Input planes whose values are 0 or 1: all but the four reserve ratios and the flat difference (repr.rs:169-228)."""
    from takzero_amd import weights as W

    cin = W.input_channels(n)
    return [c for c in range(cin) if c not in (cin - 6, cin - 5, cin - 4, cin - 3, cin - 1)]


def _sparse_conv(rng, cout, cin, allowed, p=None, second=None):
    """Two entries per output channel: +1 at a place drawn with probabilities `p` over the `allowed` input channels, `second`
    (or a random sign) at a place drawn evenly."""
    w = np.zeros((cout, cin, 3, 3), np.float32)
    allowed = np.asarray(allowed)
    for co in range(cout):
        while True:
            ci = (rng.choice(allowed, p=p), rng.choice(allowed))
            tap = rng.integers(9, size=2)
            if ci[0] != ci[1] or tap[0] != tap[1]:
                break
        w[co, ci[0], tap[0] // 3, tap[0] % 3] = 1.0
        w[co, ci[1], tap[1] // 3, tap[1] % 3] = second if second is not None else (1.0 if rng.integers(2) else -1.0)
    return w


def _calibrate_bias(pre, ceiling=MAX_CALIBRATED):
    """pre [B,C,N,N] (integers, fp64): per channel the non-positive integer bias -k for which the share of outputs above zero is
    closest to SURVIVE, at least MIN_SHARE where a k >= 0 allows it (a positive bias only for a channel whose outputs are all <= 0), and
    the largest output at most `ceiling`."""
    c = pre.shape[1]
    flat = np.rint(pre.transpose(1, 0, 2, 3).reshape(c, -1)).astype(np.int64)
    bias = np.zeros(c, np.float32)
    for ch in range(c):
        v = flat[ch]
        top = int(v.max())
        if top >= 1:
            k0 = min(max(0, int(np.floor(np.quantile(v, 1.0 - SURVIVE)))), top - 1)
            k = min((kk for kk in (k0, k0 - 1) if kk >= 0), key=lambda kk: abs(float((v > kk).mean()) - SURVIVE))
            while k > 0 and float((v > k).mean()) < MIN_SHARE:
                k -= 1
        else:
            k = top - 1
        bias[ch] = -max(k, top - ceiling)
    return bias


def unfed_taps(weight, x):
    """The (output square, tap) pairs of a 3x3 conv, tap on the board, through which no non-zero product arrives anywhere in the batch:
    weight [cout,cin,3,3], x [B,cin,n,n] (numpy or torch).  Empty when every square is fed through every tap that lands on the board."""
    used = (np.asarray(weight) != 0).any(axis=0)          # [cin,3,3]: input channels that some output channel reads through the tap
    live = (np.asarray(x) != 0).any(axis=0)               # [cin,n,n]: squares where the input channel is non-zero somewhere
    n, out = live.shape[-1], []
    for ky in range(3):
        for kx in range(3):
            fed = live[used[:, ky, kx]].any(axis=0)
            for y in range(n):
                for xx in range(n):
                    sy, sx = y + ky - 1, xx + kx - 1
                    if 0 <= sy < n and 0 <= sx < n and not fed[sy, sx]:
                        out.append(((y, xx), (ky, kx)))
    return out


def exact_weights(arch, n, blocks, seed, calibration, ceiling=MAX_CALIBRATED):
    """Weights of `arch` as described in the module docstring; `calibration` are planes [B,C,N,N] (fp32) of encoded positions;
    `ceiling` is the largest activation the calibration allows on them."""
    import torch
    import torch.nn.functional as F
    from takzero_amd import weights as W

    n, blocks = W.arch_board(arch, n), W.arch_blocks(arch, blocks)
    w = dict(W.init_weights(arch, n=n, blocks=blocks, seed=1000 + seed))      # RND MLPs / SimHash matrix as initialised
    rng = np.random.default_rng(7000 + seed)
    cin, nn, f = W.input_channels(n), n * n, W.FILTERS
    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch.float64)

    def bn(prefix, bias):
        w[prefix + ".weight"] = np.ones(f, np.float32)
        w[prefix + ".running_mean"] = np.zeros(f, np.float32)
        w[prefix + ".running_var"] = np.full(f, np.float32(1) - np.float32(1e-5), np.float32)
        w[prefix + ".bias"] = bias

    def layer(conv, norm, x, residual, cin_l, allowed, p, second):
        """Draw the conv, calibrate its BatchNorm bias; channels that stay nearly dead on the calibration positions are drawn again."""
        wt = _sparse_conv(rng, f, cin_l, allowed, p, second)
        for _ in range(16):
            pre = F.conv2d(x, t64(wt), padding=1)
            if residual is not None:
                pre = pre + residual
            b = _calibrate_bias(pre.numpy(), ceiling)
            y = F.relu(pre + t64(b).view(1, -1, 1, 1))
            weak = np.flatnonzero((y != 0).double().mean(dim=(0, 2, 3)).numpy() < MIN_SHARE)
            if weak.size == 0:
                break
            wt[weak] = _sparse_conv(rng, weak.size, cin_l, allowed, p, second)
        w[conv + ".weight"] = wt
        bn(norm, b)
        return y

    # the first conv: the +1 entry sits on a plane in proportion to how often it is set (most stack planes are almost never set), the other anywhere
    dy = dyadic_input_channels(n)
    density = calibration[:, dy].mean(axis=(0, 2, 3))
    x = layer("core.input_conv2d", "core.batch_norm", t64(calibration), None, cin, dy, density / density.sum(), None)
    for blk in range(blocks):
        p = "core.res_block_%d" % blk
        y = layer(p + ".a.conv2d", p + ".a.batch_norm", x, None, f, np.arange(f), None, -1.0)
        x = layer(p + ".b.conv2d", p + ".b.batch_norm", y, x, f, np.arange(f), None, -1.0)
    out = W.output_channels(n)
    for _ in range(64):      # the small boards' policy convs have few channels: draw until every square is fed through every tap
        w["policy.conv2d.weight"] = _sparse_conv(rng, out, f, np.arange(f))
        if not unfed_taps(w["policy.conv2d.weight"], x.numpy()):
            break
    w["policy.conv2d.bias"] = rng.integers(-3, 4, size=out).astype(np.float32)
    for head in ("value", "ube"):
        hw = np.zeros((1, f, 1, 1), np.float32)
        idx = rng.choice(f, size=16, replace=False)
        hw[0, idx, 0, 0] = np.where(np.arange(16) % 2 == 0, 1.0, -1.0)
        pre = F.conv2d(x, t64(hw))
        hb = np.float32(-np.floor(np.quantile(pre.numpy(), 0.5)))          # half of the squares pass the head's ReLU
        h = F.relu(pre + float(hb)).reshape(x.shape[0], -1)
        sign = np.where(rng.integers(2, size=nn) == 1, 1.0, -1.0)
        raw = (h.numpy() * sign[None, :]).sum(axis=1)
        s = int(np.clip(np.ceil(np.log2(max(1.0, np.abs(raw).max()) / 2.0)), 2, 12))
        w[head + ".conv2d.weight"] = hw
        w[head + ".conv2d.bias"] = np.array([hb], np.float32)
        w[head + ".linear.weight"] = (sign * 2.0 ** -s).astype(np.float32).reshape(1, nn)
        w[head + ".linear.bias"] = np.array([0.25], np.float32)
    return w


LO_STEP = 2.0 ** -14      # exact_weights_with_lo: a weight is +-(1 + q * LO_STEP)
LO_QMAX = 7
LO_QMIN = 4               # q >= -4: 1 - 5 * 2^-14 and below round to the half 1 - 2^-11, and the hi parts would no longer be +-1 (-4 is a tie, to even)
LO_NETS = {5: (100, 5, 3), 6: (100, 6, 2), 3: (100, 3, 2), 4: (100, 4, 2)}      # board size -> (arch, n, blocks): the test architecture
LO_SEEDS = (0, 1)
LO_ARITHMETICS = {5: ("f16x2", "f16c8", "f16c6"), 6: ("f16x2", "f16c8", "f16c6"), 3: ("f16x2", "f16c8"), 4: ("f16x2", "f16c8")}
LO_POSITIONS, LO_POSITION_SEED, LO_CALIBRATION_SEED = 64, 77, 5
LO_MIN_SHARE = 0.05
LO_MIN_DECIDED = 0.5      # share of the policy outputs that the exactness condition covers, at least
CONV_3X3 = lambda name, v: name.endswith("conv2d.weight") and v.shape[-1] == 3


def exact_weights_with_lo(arch, n, blocks, seed, calibration, qmax=LO_QMAX, ceiling=MAX_CALIBRATED):
    """`exact_weights` with a lo part on every non-zero weight of the first conv, the tower convs and the policy conv:
    w = +-(1 + q * 2^-14), q a random integer in [-min(qmax, 4), qmax].  fp16(w) is still +-1, and the lo part q * 2^-14 is exact in fp16
    (times 2^11), in E4M3 (times 2^11 and the layer's power of two) and in a block-scaled E2M3 code (integers up to 7 in units of
    the block scale).  Structure, BatchNorms and the calibrated integer biases are those of the integer net; the heads keep their
    dyadic weights.  With qmax = 0 the weights are `exact_weights` unchanged.  Activations are then integers plus a small lo part
    (and a few tiny ones where the integers cancel), so the correction products of the split arithmetics decide output bits;
    what has to hold for a bit-exact comparison is asserted by `assert_reference_is_exact` on the emulation's statistics."""
    w = exact_weights(arch, n, blocks, seed, calibration, ceiling)
    rng = np.random.default_rng(9000 + seed)
    for name in sorted(k for k, v in w.items() if CONV_3X3(k, v)):
        q = rng.integers(-min(qmax, LO_QMIN), qmax + 1, size=w[name].shape).astype(np.float64)
        w[name] = (w[name].astype(np.float64) * (1.0 + q * LO_STEP)).astype(np.float32)
    return w


def head_steps(w):
    """The grid steps 2^-s of the value head's pre-activation and of the UBE output."""
    return tuple(float(np.abs(w[h + ".linear.weight"]).max()) for h in ("value", "ube"))


def folded_batch_norms(w):
    """(scale, bias) of every BatchNorm as bn_fold (csrc/tz_nn.hip) computes them, in numpy fp32."""
    out = {}
    for name in w:
        if name.endswith(".running_var"):
            p = name[:-len(".running_var")]
            s = w[p + ".weight"].astype(np.float32) / np.sqrt(w[name].astype(np.float32) + np.float32(1e-5), dtype=np.float32)
            out[p] = (s, w[p + ".bias"].astype(np.float32) - w[p + ".running_mean"].astype(np.float32) * s)
    return out


def exact_reference(w, planes, blocks, chunk=512):
    """The fp64 graph on `planes`, rounded to the grid.  Returns policy [B, OUT*N*N] (fp32, integers), value_pre [B] (fp64, multiples
    of the value step), value [B] (fp64 tanh of it), ube [B] (fp32) and `stats`: the largest distance of any fp64 output or trunk
    activation from its grid point, the largest trunk activation, per layer the share of non-zero activations."""
    import nets_torch as T
    import torch
    from takzero_amd import weights as W

    vstep, ustep = head_steps(w)
    pol, vpre, ube = [], [], []
    dev, top, share = 0.0, 0.0, None
    for lo in range(0, len(planes), chunk):
        trace = []
        p, _, _ = T.forward(w, planes[lo:lo + chunk], blocks, dtype=torch.float64, trace=trace)
        named = dict(trace)
        acts = [t for k, t in trace if k.startswith("core.")]
        for t in acts:
            dev = max(dev, float((t - t.round()).abs().max()))
            top = max(top, float(t.abs().max()))
        nz = np.array([float((t.round() != 0).sum()) for t in acts])
        share = nz if share is None else share + nz
        p = p.reshape(p.shape[0], -1)
        v, u = named["value.pre"], named["ube.pre"]
        dev = max(dev, float((p - p.round()).abs().max()), float((v / vstep - (v / vstep).round()).abs().max() * vstep),
                  float((u / ustep - (u / ustep).round()).abs().max() * ustep))
        pol.append(p.round().to(torch.float32).numpy())
        vpre.append(((v / vstep).round() * vstep).numpy())
        ube.append(((u / ustep).round() * ustep).to(torch.float32).numpy())
    per_layer = planes.shape[0] * W.FILTERS * planes.shape[2] * planes.shape[3]
    vpre = np.concatenate(vpre)
    return dict(policy=np.concatenate(pol), value_pre=vpre, value=np.tanh(vpre), ube=np.concatenate(ube),
                stats=dict(deviation=dev, max_activation=top, nonzero_share=share / per_layer))


def assert_reference_is_exact(ref):
    """The conditions under which the bits of every precision must agree, on the positions a test runs (not only the calibration's)."""
    st = ref["stats"]
    if "quotient" in st:
        # A net with lo parts, emulated by tests/split_emulation.py.  The condition for a bit-exact comparison is not that values are
        # integers but that no fp32 accumulator can round, in whatever order it adds: sum |terms| / (a power of two that divides
        # every term) below 2^24, per output, for every accumulator of every layer.  Roundings then remain only at single,
        # order-free operations (storage conversions and the one fp32 addition that merges the accumulators), which the emulation
        # performs as the kernels do.  Activations near zero keep second-order bits (lo x lo sized, 2^-28) alive in their hi parts,
        # and a block input carries 22 or more bits into the main accumulator, so the condition does not hold for every output of
        # a net with a residual block, whatever the range of q, the calibration ceiling or the depth
        # (tests/test_split_emulation_reference.py `test_the_levers_of_the_generator_do_not_make_the_condition_hold_everywhere`).  It is therefore applied per output: `decided` marks the outputs for which
        # it holds in every accumulator they depend on, through every layer; those are compared bit for bit, and they must be
        # most of the policy, on the positions a test runs.  No floor is set for the heads: they add 16 channels on every square, and
        # few of their outputs (on some nets none) are decided.
        dec = ref["decided"]
        assert dec["policy"].mean() >= LO_MIN_DECIDED, dec["policy"].mean()
        assert dec["policy"].any(axis=1).all()                # some decided logit in every position
        return
    assert st["deviation"] < 1e-3, st
    assert st["max_activation"] <= MAX_ACTIVATION, st
