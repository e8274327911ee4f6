"""OCP MX FP6 E2M3 in numpy (1 sign, 2 exponent, 3 mantissa bits, bias 1, no infinities / NaN): the statement of the format that
tests/test_fp6_host.py holds the host conversion (takzero_amd/csrc/tz_fp6.h) to, and that tests/split_emulation.py rounds with.
`ref_code` is the scalar statement; `round_to_e2m3` and `block_scale_byte` are the same rules on arrays
(tests/test_split_emulation_reference.py holds them to the scalar one on every code point, tie and neighbour of a tie)."""
import numpy as np


def e2m3_values():
    v = []
    for c in range(32):
        e, m = c >> 3, c & 7
        v.append(m / 8.0 if e == 0 else (1.0 + m / 8.0) * 2.0 ** (e - 1))
    return np.array(v, np.float64)   # ascending: 0 .. 7.5


def ref_code(x):
    """round to nearest even onto the grid, saturating; ties between codes c and c + 1 go to the even code"""
    vals = e2m3_values()
    a = abs(float(x))
    if a != a:
        c = 31
    elif a >= 7.75:
        c = 31
    else:
        i = int(np.searchsorted(vals, a, side="right")) - 1
        i = max(0, min(30, i))
        lo, hi = vals[i], vals[i + 1]
        if a - lo < hi - a:
            c = i
        elif a - lo > hi - a:
            c = i + 1
        else:
            c = i if i % 2 == 0 else i + 1
    sign = 32 if np.signbit(np.float32(x)) else 0
    return sign | c


def round_to_e2m3(x):
    """`ref_code` on an array (fp64, in units of the block scale), returned as the values the codes stand for."""
    vals = e2m3_values()
    x = np.asarray(x, np.float64)
    a = np.abs(x)
    i = np.clip(np.searchsorted(vals, a, side="right") - 1, 0, 30)
    lo, hi = vals[i], vals[i + 1]
    up = (a - lo > hi - a) | ((a - lo == hi - a) & (i % 2 == 1))
    c = np.where((a >= 7.75) | (a != a), 31, i + up)
    return np.copysign(vals[c], x)


def block_scale_byte(amax, min_byte=1):
    """tz_e2m3_block_scale_byte (csrc/tz_fp6.h) / c6_scale_byte (csrc/tz_nn_c6.hip) on an array: the exponent field of the fp32
    product amax * (16 / 15), less 2, never below `min_byte`: the power of two s = 2^(byte - 127) with amax / s in [3.75, 7.5)."""
    t = (np.asarray(amax, np.float32) * np.float32(16.0 / 15.0)).astype(np.float32)
    b = (t.view(np.uint32) >> 23).astype(np.int64) & 0xff
    return np.maximum(b, min_byte + 2) - 2
