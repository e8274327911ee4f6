"""CPU emulation of the three split arithmetics of the inference forward - TZ_PREC_F16X2, TZ_PREC_F16C8, TZ_PREC_F16C6 - written from
their stated definition, not from their output: DESIGN.md section 4 ("Precision" and the rules S1 .. S12 under "What the split
arithmetics round, rule by rule") and the comments above k_loop_split, k_loop_c8, c8_parts, build_layer (csrc/tz_nn.hip) and k_loop_c6
(csrc/tz_nn_c6.hip).  Each rule below names the sentence it restates.  The module restates index maps and rounding rules; it never
calls the library, and nothing in it was adjusted to what a kernel returns.

`emulate(prec, w, planes, blocks)` computes the forward of a net (first conv, residual blocks, policy conv, both heads) from the
weights dict and the encoded planes.  Every operand is rounded where the arithmetic rounds it (fp16 by torch.float16, E4M3 by
torch.float8_e4m3fn, E2M3 by tests/e2m3_ref.py, fp32 by torch.float32: one round to nearest even each); the sums between two
roundings are taken in fp64 (`accumulate="fp64"`) or, for the dense-weight gate of tests/test_gpu_split_corrections.py, by torch's
fp32 conv2d on the same rounded operands (`accumulate="fp32"`).

An accumulator of a layer is a list of (activation operand, weight operand) products summed onto a start value; a layer's
pre-activation is sum over its accumulators of scale * accumulator, rounded to fp32 once.  f16x2 and f16c8 have two accumulators
(main, correction), f16c6 one.  With `stats=True` the emulation also returns, per layer and accumulator, the largest
sum |terms| / unit over the outputs, `unit` a power of two that divides every term of that output (the unit of an output is the finest unit among its own non-zero terms and its start value, computed exactly; below 2^24 no fp32
accumulator can round, in whatever order it adds); per layer the share of stored activations whose lo part is not zero; and `decided`, the
policy / value / UBE outputs for which that quotient is below 2^24 in every accumulator they depend on, through every layer (an
output that reads an undecided activation through a non-zero weight, as a residual or, in f16c6, through its block's scale is
undecided): those a kernel must return bit for bit (tests/exact_net.py `assert_reference_is_exact`).

`fault=(name, layer)` is for tests/test_split_emulation_reference.py alone: it breaks the arithmetic the way a kernel fault would,
to show that the fixtures can see it.  Layers count 0 = first conv, 1 .. 2 * blocks = the tower, 2 * blocks + 1 = the policy conv."""
import numpy as np
import torch
import torch.nn.functional as F

from e2m3_ref import block_scale_byte, round_to_e2m3

T64 = torch.float64
ARITHMETICS = ("f16x2", "f16c8", "f16c6")
FAULTS = ("no_wl_xh", "no_wh_xl", "lo_lo", "lo_scale_x2", "drop_tap", "drop_block", "no_remainder", "e8m0_off_by_one")
HEAD_FAULT = "heads_read_hi_only"      # the heads' input without its lo part (f16x2), its bytes (f16c8), from the image's hi instead of `seeds` (f16c6)
FAULT_TAP = (1, 1)       # drop_tap: the centre tap (on the board for every square)
FAULT_BLOCK = 3          # drop_block / e8m0_off_by_one: input channels 96 .. 127


def faults_of(prec, n):
    """The faults a fixture has to see: the remainder byte is f16c8's, and it is asked of the 5x5 nets (6x6 has no remainder byte; on 3x3
    and 4x4 the lo parts of the exact nets rarely need more than the lo byte's four bits, and no output bit depends on the remainder:
    there the byte is held by the dense weights alone); the E8M0 scale is f16c6's."""
    out = [f for f in FAULTS[:6]]
    if prec == "f16c8" and n == 5:
        out.append("no_remainder")
    if prec == "f16c6":
        out.append("e8m0_off_by_one")
    return out


# ---- roundings: each is one round to nearest even of values that fp32 holds exactly (asserted: no double rounding through fp32)
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64)))


def f32(t):
    return t.to(torch.float32).to(T64)


def _in_f32(t):
    assert bool((t.to(torch.float32).to(T64) == t).all()), "operand of a storage conversion is not an fp32 value"
    return t.to(torch.float32)


def f16(t):
    """Elem<_Float16>::cvt: saturating at the largest finite half."""
    return _in_f32(t).clamp(-65504.0, 65504.0).to(torch.float16).to(T64)


def e4m3(t):
    """OCP FP8 E4M3 of values already clamped to +-448 (pack_e4m3 / c8_parts clamp first, tz_f32_to_e4m3 saturates)."""
    return _in_f32(t).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).to(torch.float32).to(T64)


def e2m3(t):
    """OCP MX FP6 E2M3 in units of the block scale, saturating at 7.5 (tests/e2m3_ref.py)."""
    return _t(round_to_e2m3(t.numpy()))


def split16(v):
    """S1: hi = fp16(x), lo = fp16((x - hi) * 2^11) (kept times 2^11); x - hi is exact in fp32."""
    hi = f16(v)
    return hi, f16((v - hi) * 2048.0)


def _inv_lsb(t):
    """1 / (the largest power of two that divides the value), 0 for zero."""
    a = np.abs(t.numpy()).astype(np.float64)
    m, e = np.frexp(a)
    mant = (m * 2.0 ** 53).astype(np.int64)
    low = (mant & -mant).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(a == 0, 0.0, 1.0 / np.ldexp(np.where(low == 0, 1.0, low), e - 53))
    return torch.from_numpy(inv)


_P = 13      # _finest: the 13-norm of up to 2^13 terms is below twice their maximum


def _finest(terms):
    """Per output, 1 / (the smallest power of two unit among its non-zero terms x * w): the largest 1 / (unit(x) unit(w)).  The units are
    powers of two, so the maximum is the power of two at or below the 13-norm of the terms' 1 / unit, which a conv2d computes."""
    total = None
    for x, w in terms:
        assert x.shape[1] * w.shape[-1] * w.shape[-2] * len(terms) < 2 ** _P
        c = F.conv2d(_inv_lsb(x) ** _P, _inv_lsb(w) ** _P, padding=w.shape[-1] // 2)
        total = c if total is None else total + c
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(total.numpy()) / _P + 1e-9)
    return torch.from_numpy(np.where(total.numpy() > 0, np.exp2(e), 0.0))


class _Sum:
    """The sums between two roundings: fp64, or torch's fp32 kernels with every accumulator an fp32 number."""

    def __init__(self, accumulate, stats):
        assert accumulate in ("fp64", "fp32")
        self.fp32 = accumulate == "fp32"
        self.stats = stats
        self.quotient, self.lo_share = {}, {}
        self.viol = self.taint = self.block_in = self.policy_taint = None      # stats: which outputs an accumulator could have rounded for
        self.head_taint = {}
        self.blockwise = False          # f16c6: a stored activation also depends on its block's largest value

    def conv(self, x, w):
        pad = w.shape[-1] // 2
        if self.fp32:
            return F.conv2d(_in_f32(x), _in_f32(w), padding=pad).to(T64)
        return F.conv2d(x, w, padding=pad)

    def accumulator(self, name, terms, start=None):
        """start + sum of conv(x, w) over the terms, as one fp32 accumulator would hold it if it never rounded."""
        total = None
        for x, w in terms:
            c = self.conv(x, w)
            total = c if total is None else (f32(total + c) if self.fp32 else total + c)
        if start is not None:
            total = start if total is None else (f32(total + start) if self.fp32 else total + start)
        if self.stats and terms:
            mag = sum(F.conv2d(x.abs(), w.abs(), padding=w.shape[-1] // 2) for x, w in terms)
            fine = _finest(terms)
            if start is not None:
                mag = mag + start.abs()
                fine = torch.maximum(fine, _inv_lsb(start))
            self.quotient[name] = float((mag * fine).max())
            bad = (mag * fine) >= 2.0 ** 24
            self.viol = bad if self.viol is None else (self.viol | bad)
        return total

    def layer_done(self, wt, kind):
        """Which outputs of the layer are not decided: one of their accumulators could round (quotient of that output at or above
        2^24), or they read - through a non-zero weight, or as the residual - an activation that is not decided.  `kind`: "first",
        "a", "b" (adds the block input), "policy"."""
        if not self.stats:
            return
        t = self.viol
        if self.taint is not None:
            t = t | (F.conv2d(self.taint.to(T64), (wt != 0).to(T64), padding=1) > 0)
        if kind == "b":
            t = t | self.block_in
        self.viol = None
        if kind == "policy":
            self.policy_taint = t
            return
        if self.blockwise:
            t = _blocks32(t, lambda u: u.any(dim=2))
        self.taint = t
        if kind in ("first", "b"):
            self.block_in = t

    def share(self, name, lo):
        if self.stats:
            self.lo_share[name] = float((lo != 0).to(T64).mean())


# ---- weights as build_layer / build_weights (csrc/tz_nn.hip) convert them
def _folded(w, conv, norm):
    """S0 (bn_fold, build_layer): s = weight / sqrtf(var + 1e-5f), bias = b - mean * s, the conv weight times s, all in fp32.  (numpy
    rounds mean * s before it subtracts; a host compiler that contracts the two into an fma moves a bias by at most one of its
    ulps, which is part of what the dense gate's D measures.  On the exact nets mean is 0 and s is 1.)"""
    wt = np.asarray(w[conv + ".weight"], np.float32)
    if norm is None:
        return _t(wt), _t(np.asarray(w[conv + ".bias"], np.float32)).view(1, -1, 1, 1)
    s = np.asarray(w[norm + ".weight"], np.float32) / np.sqrt(np.asarray(w[norm + ".running_var"], np.float32) + np.float32(1e-5), dtype=np.float32)
    b = np.asarray(w[norm + ".bias"], np.float32) - np.asarray(w[norm + ".running_mean"], np.float32) * s
    return _t((wt * s[:, None, None, None]).astype(np.float32)), _t(b.astype(np.float32)).view(1, -1, 1, 1)


def _layers(w, blocks):
    out = [("core.input_conv2d", "core.batch_norm")]
    for b in range(blocks):
        p = "core.res_block_%d" % b
        out += [(p + ".a.conv2d", p + ".a.batch_norm"), (p + ".b.conv2d", p + ".b.batch_norm")]
    return [_folded(w, c, n) for c, n in out] + [_folded(w, "policy.conv2d", None)]


def _c8_weights(wt):
    """build_layer, with_c8: s = the power of two that brings the layer's largest |w| to [128, 256) (fp32 log2f / floorf / exp2f);
    E4M3 codes of hi * s and of (w - hi) * 2^11 * s; c8_scale = 1 / (2^11 * s * 4)."""
    wmax = np.float32(wt.abs().max())
    sw = float(np.exp2(np.floor(np.log2(np.float32(256.0) / wmax)))) if wmax > 0 else 1.0
    hi = f16(wt)
    return hi, e4m3(hi * sw), e4m3((wt - hi) * 2048.0 * sw), sw, 1.0 / (2048.0 * sw * 4.0)


def _blocks32(t, reduce):
    """Per block of 32 consecutive channels (dim 1): c6_channel_at / c6_position_of put the 32 output channels of wave w into the 32
    input places that one lane of the next conv's E2M3 MFMA reads, and build_layer's in_perm moves the weights' input channels
    to the same places: a block of the image and a block of the weights is the channels 32 w .. 32 w + 31, per pixel / per
    (output channel, tap)."""
    s = t.shape
    return reduce(t.reshape(s[0], s[1] // 32, 32, *s[2:])).repeat_interleave(32, dim=1)


def _c6_scale(amax, min_byte):
    return _t(np.ldexp(1.0, block_scale_byte(amax.numpy(), min_byte) - 127))


def _c6_weights(wt):
    """build_layer, with_c6: per (output channel, tap, block of 32 input channels) hi = fp16(w), lo = w - hi (fp32), each with the
    scale of tz_e2m3_block_scale_byte of its block's largest magnitude, converted by tz_f32_to_e2m3 (saturating)."""
    hi = f16(wt)
    lo = wt - hi
    amax = lambda t: t.abs().amax(dim=2)
    sh, sl = _c6_scale(_blocks32(hi, amax), 1), _c6_scale(_blocks32(lo, amax), 1)
    return hi, e2m3(hi / sh) * sh, e2m3(lo / sl) * sl


# ---- the faults of the sensitivity test
def _hit(fault, name, layer):
    return fault is not None and fault[0] == name and (fault[1] is None or fault[1] == layer)


def _faulty(corr, fault, layer):
    """corr: [(tag, x, w)] with tag "wl_xh" / "wh_xl" / "wl_xl"; returns the (x, w) pairs a broken kernel would add."""
    out = []
    for tag, x, w in corr:
        if tag == "wl_xl" and not _hit(fault, "lo_lo", None):
            continue
        if (tag == "wl_xh" and _hit(fault, "no_wl_xh", None)) or (tag == "wh_xl" and _hit(fault, "no_wh_xl", None)):
            continue
        if tag != "wl_xl" and w.shape[-1] == 3 and _hit(fault, "drop_tap", layer):
            w = w.clone()
            w[:, :, FAULT_TAP[0], FAULT_TAP[1]] = 0.0
        if tag != "wl_xl" and _hit(fault, "drop_block", layer):
            w = w.clone()
            w[:, 32 * FAULT_BLOCK:32 * FAULT_BLOCK + 32] = 0.0
        out.append((x, w))
    return out


def _heads(S, xf, w, n):
    """S10: both heads read xf, the tower's output as the arithmetic carries it; dot with the 1x1 conv weights (fp32), + conv bias,
    ReLU, dot with the linear weights over the squares, + linear bias; value = tanhf of it."""
    out = {}
    for head in ("value", "ube"):
        hw = _t(np.asarray(w[head + ".conv2d.weight"], np.float32)).view(1, -1, 1, 1)
        pre = S.accumulator("head." + head + ".conv", [(xf, hw)])
        if S.stats:
            t = S.viol | (F.conv2d(S.taint.to(T64), (hw != 0).to(T64)) > 0)
            S.head_taint[head] = t.reshape(t.shape[0], -1).any(dim=1)
            S.viol = None
        h = f32(F.relu(f32(pre + float(np.float32(w[head + ".conv2d.bias"][0])))))
        lw = _t(np.asarray(w[head + ".linear.weight"], np.float32)).view(1, n * n)
        dot = _linear(S, "head." + head + ".linear", h.reshape(h.shape[0], -1), lw)
        out[head] = f32(dot + float(np.float32(w[head + ".linear.bias"][0])))
    return out["value"].numpy(), out["ube"].to(torch.float32).numpy()


def _linear(S, name, h, lw):
    if S.fp32:
        dot = F.linear(_in_f32(h), _in_f32(lw)).to(T64)[:, 0]
    else:
        dot = F.linear(h, lw)[:, 0]
    if S.stats:
        mag = (h.abs() * lw.abs()).sum(dim=1)
        fine = (_inv_lsb(h) * _inv_lsb(lw)).amax(dim=1)
        S.quotient[name] = float((mag * fine).max())
        S.head_taint[name.split(".")[1]] |= (mag * fine) >= 2.0 ** 24
    return dot


def _result(S, policy, heads):
    vpre, ube = heads
    out = dict(policy=policy.reshape(policy.shape[0], -1).to(torch.float32).numpy(), value_pre=vpre, value=np.tanh(vpre), ube=ube)
    if S.stats:
        out["stats"] = dict(quotient=S.quotient, lo_share=S.lo_share)
        out["decided"] = dict(policy=(~S.policy_taint).reshape(policy.shape[0], -1).numpy(), value=(~S.head_taint["value"]).numpy(),
                              ube=(~S.head_taint["ube"]).numpy())
    return out


def _relu_sat(t):
    """fmed3(v, 0, 65504): ReLU and fp16's saturation in one."""
    return t.clamp(0.0, 65504.0)


def _split_first_conv(planes, wt, fault):
    """S2: the first conv of all three arithmetics is the split form on hi / lo halves of the input planes and of the weights."""
    xh, xl = split16(_t(planes))
    wh, wl = split16(wt)
    corr = _faulty([("wl_xh", xh, wl), ("wh_xl", xl, wh), ("wl_xl", xl, wl)], fault, 0)
    lolo = corr.pop() if _hit(fault, "lo_lo", None) else None
    return xh, wh, corr, lolo


# ---------------------------------------------------------------------------------------------------------------------------------
def emulate_f16x2(w, planes, blocks, accumulate="fp64", stats=False, fault=None):
    """TZ_PREC_F16X2 (comment above k_loop_split; DESIGN.md 4 "TZ_PREC_F16X2 is the mode ..."): wh*xh into the main accumulator, which
    starts at bias (S3) or at residual + bias (S4); wl*xh + wh*xl into the correction accumulator, which starts at zero and is
    multiplied by 2^-11 once per layer and added (S5: one fp32 operation); lo*lo dropped; ReLU; stored as hi / lo halves (S1)."""
    S = _Sum(accumulate, stats)
    n = planes.shape[-1]
    L = _layers(w, blocks)

    def layer(i, xh, xl, start):
        wh, wl = split16(L[i][0])
        main = S.accumulator("layer%d.main" % i, [(xh, wh)], start)
        corr = _faulty([("wl_xh", xh, wl), ("wh_xl", xl, wh), ("wl_xl", xl, wl)], fault, i)
        lolo = S.accumulator("layer%d.lolo" % i, [corr.pop()]) * 2.0 ** -22 if _hit(fault, "lo_lo", None) else 0.0
        c = S.accumulator("layer%d.correction" % i, corr)
        c = 0.0 if c is None else c
        scale = 2.0 ** -10 if _hit(fault, "lo_scale_x2", i) else 2.0 ** -11
        S.layer_done(L[i][0], "first" if i == 0 else "policy" if i == 2 * blocks + 1 else "a" if i % 2 else "b")
        return f32(main + c * scale + lolo)                       # S5

    xh, xl = split16(_t(planes))
    xh, xl = split16(F.relu(layer(0, xh, xl, L[0][1])))          # S3, S1
    S.share("layer0", xl)
    for b in range(blocks):
        a, s = 1 + 2 * b, 2 + 2 * b
        start = f32(f32(xh + xl * 2.0 ** -11) + L[s][1])          # S4: (hi + lo * 2^-11) + bias, two fp32 additions
        xh, xl = split16(F.relu(layer(a, xh, xl, L[a][1])))
        S.share("layer%d" % a, xl)
        xh, xl = split16(F.relu(layer(s, xh, xl, start)))
        S.share("layer%d" % s, xl)
    policy = layer(2 * blocks + 1, xh, xl, L[-1][1])              # S11: no ReLU, fp32 out
    return _result(S, policy, _heads(S, xh if _hit(fault, HEAD_FAULT, None) else f32(xh + xl * 2.0 ** -11), w, n))   # S10 (f16x2): hi + lo * 2^-11 in fp32


def _c8_store(v, want_r):
    """c8_parts (v post-ReLU, at most 65504): hi = fp16(v); the FP8 copy of hi is E4M3(min(hi, 112) * 4); the lo part v - hi is
    clamped to +-448 / 2^13 and stored as E4M3((v - hi) * 2^13); the remainder byte is E4M3 of what that byte misses, times 16 more.
    Returned as code values: h8 (units of 1/4), l8 (units of 2^-13), r8 (units of 2^-17)."""
    hi = f16(v)
    t = (v - hi).clamp(-448.0 / 8192.0, 448.0 / 8192.0)
    h8 = e4m3(hi.clamp(max=112.0) * 4.0)
    l8 = e4m3(t * 8192.0)
    r8 = e4m3(f32(t * 8192.0 - l8) * 16.0) if want_r else torch.zeros_like(l8)
    return hi, h8, l8, r8


def _c8_value(hi, l8, r8):
    """c8_value: (float)hi + (l8 + r8 / 16) * 2^-13, the inner sum and the outer one an fp32 addition each (S7)."""
    return f32(hi + f32(l8 + r8 / 16.0) / 8192.0)


def emulate_f16c8(w, planes, blocks, accumulate="fp64", stats=False, fault=None):
    """TZ_PREC_F16C8 (comments above k_loop_c8, c8_parts, build_layer; DESIGN.md 4 "TZ_PREC_F16C8 carries ..."): the main product on fp16
    hi parts; the corrections wl8 * xh8 + wh8 * xl8 on E4M3 copies into a correction accumulator scaled by c8_scale (S6); the block
    input carried as hi + lo byte + remainder byte (S7), on 6x6 as hi + one byte (S8); the first conv in the split form (S2)."""
    S = _Sum(accumulate, stats)
    n = planes.shape[-1]
    r8_kept = n != 6 and not _hit(fault, "no_remainder", None)      # S8: every 6x6 form is without remainder bytes
    L = _layers(w, blocks)

    xh, wh, corr, lolo = _split_first_conv(planes, L[0][0], fault)
    main = S.accumulator("layer0.main", [(xh, wh)], L[0][1])
    c = S.accumulator("layer0.correction", corr)
    c = 0.0 if c is None else c
    extra = S.accumulator("layer0.lolo", [lolo]) * 2.0 ** -22 if lolo is not None else 0.0
    S.layer_done(L[0][0], "first")
    v = _relu_sat(f32(main + c * (2.0 ** -10 if _hit(fault, "lo_scale_x2", 0) else 2.0 ** -11) + extra))       # S5 (first conv: 2^-11)
    hi, h8, l8, r8 = _c8_store(v, r8_kept)                          # the first conv's output is a block input
    S.share("layer0", l8)

    def layer(i, hi, h8, l8, start):
        wh, wh8, wl8, sw, cs = _c8_weights(L[i][0])
        main = S.accumulator("layer%d.main" % i, [(hi, wh)], start)
        corr = _faulty([("wl_xh", h8, wl8), ("wh_xl", l8, wh8), ("wl_xl", l8, wl8)], fault, i)
        extra = S.accumulator("layer%d.lolo" % i, [corr.pop()]) / (2048.0 * sw * 8192.0) if _hit(fault, "lo_lo", None) else 0.0
        c = S.accumulator("layer%d.correction" % i, corr)
        c = 0.0 if c is None else c
        S.layer_done(L[i][0], "policy" if i == 2 * blocks + 1 else "a" if i % 2 else "b")
        return f32(main + c * (cs * 2.0 if _hit(fault, "lo_scale_x2", i) else cs) + extra)      # S6

    for b in range(blocks):
        a, s = 1 + 2 * b, 2 + 2 * b
        start = f32(_c8_value(hi, l8, r8) + L[s][1])               # S7
        hi, h8, l8, _ = _c8_store(_relu_sat(layer(a, hi, h8, l8, L[a][1])), False)     # inside a block: no remainder byte
        S.share("layer%d" % a, l8)
        hi, h8, l8, r8 = _c8_store(_relu_sat(layer(s, hi, h8, l8, start)), r8_kept)
        S.share("layer%d" % s, l8)
    policy = layer(2 * blocks + 1, hi, h8, l8, L[-1][1])           # S11
    return _result(S, policy, _heads(S, hi if _hit(fault, HEAD_FAULT, None) else _c8_value(hi, l8, r8), w, n))      # S10 (f16c8): hi + both bytes


def _c6_store(v):
    """The epilogue of net_c6_kernel (v post-ReLU, at most 65504, fp32): hi = fp16(v); lo = (v - hi) * 2^11 in fp32, rounded to a
    half (S9); per block of 32 channels of a pixel the scale byte of xh's copy from the largest v (at least 1) and of xl's from
    the largest |lo| in fp32 (at least 12, stored less 11); xh's E2M3 copy is made in the k-loop from the fp16 hi, saturating
    at 7.5; xl's in the epilogue from the half.  Returns hi, xh6, xl6 as the values the MFMA multiplies."""
    hi = f16(v)
    lo32 = (v - hi) * 2048.0
    lo16 = f16(lo32)
    amax = lambda t: t.abs().amax(dim=2)
    sh, sl = _c6_scale(_blocks32(v, amax), 1), _c6_scale(_blocks32(lo32, amax), 12)
    return hi, e2m3(hi / sh) * sh, e2m3(lo16 / sl) * sl / 2048.0


def emulate_f16c6(w, planes, blocks, accumulate="fp64", stats=False, fault=None):
    """TZ_PREC_F16C6 (comments above k_loop_c6 and at the head of csrc/tz_nn_c6.hip; DESIGN.md 4 "TZ_PREC_F16C6 (round 3) ..."): E2M3 copies
    with one E8M0 scale per block of 32, every product into one accumulator; block inputs and the heads' input in fp32 from
    `seeds` (S12); the first conv in the split form through the one accumulator (S2)."""
    S = _Sum(accumulate, stats)
    S.blockwise = True
    n = planes.shape[-1]
    L = _layers(w, blocks)

    # S2 (f16c6): correction products first, the accumulator times 2^-11 plus bias (one fp32 operation), then the main product on top
    xh, wh, corr, lolo = _split_first_conv(planes, L[0][0], fault)
    c = S.accumulator("layer0.correction", corr)
    c = 0.0 if c is None else c
    extra = S.accumulator("layer0.lolo", [lolo]) * 2.0 ** -22 if lolo is not None else 0.0
    start = f32(c * (2.0 ** -10 if _hit(fault, "lo_scale_x2", 0) else 2.0 ** -11) + L[0][1] + extra)
    v = _relu_sat(f32(S.accumulator("layer0.main", [(xh, wh)], start)))
    S.layer_done(L[0][0], "first")

    def layer(i, hi, xh6, xl6, start):
        wh, wh6, wl6 = _c6_weights(L[i][0])
        if _hit(fault, "lo_scale_x2", i):
            wl6 = wl6 * 2.0
        if _hit(fault, "e8m0_off_by_one", i):
            xl6 = xl6.clone()
            xl6[:, 32 * FAULT_BLOCK:32 * FAULT_BLOCK + 32] *= 2.0
        terms = [(hi, wh)] + _faulty([("wl_xh", xh6, wl6), ("wh_xl", xl6, wh6), ("wl_xl", xl6, wl6)], fault, i)
        out = f32(S.accumulator("layer%d" % i, terms, start))
        S.layer_done(L[i][0], "policy" if i == 2 * blocks + 1 else "a" if i % 2 else "b")
        return out

    hi, xh6, xl6 = _c6_store(v)
    S.share("layer0", xl6)
    for b in range(blocks):
        a, s = 1 + 2 * b, 2 + 2 * b
        seed = f32(v + L[s][1])                                     # S12: block input + the second conv's bias, fp32, in `seeds`
        hi, xh6, xl6 = _c6_store(_relu_sat(layer(a, hi, xh6, xl6, L[a][1])))
        S.share("layer%d" % a, xl6)
        v = _relu_sat(layer(s, hi, xh6, xl6, seed))
        hi, xh6, xl6 = _c6_store(v)
        S.share("layer%d" % s, xl6)
    policy = layer(2 * blocks + 1, hi, xh6, xl6, L[-1][1])         # S11
    return _result(S, policy, _heads(S, hi if _hit(fault, HEAD_FAULT, None) else v, w, n))                   # S10 (f16c6): the fp32 tower output


EMULATIONS = {"f16x2": emulate_f16x2, "f16c8": emulate_f16c8, "f16c6": emulate_f16c6}


def emulate(prec, w, planes, blocks, accumulate="fp64", stats=False, fault=None):
    return EMULATIONS[prec](w, np.asarray(planes, np.float32), blocks, accumulate=accumulate, stats=stats, fault=fault)
