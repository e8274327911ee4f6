"""numpy reference of HashNetwork::get_indices of net4_lcghash (takzero/src/network/net4_lcghash.rs:202-242) and what hangs on it.

    1. p = planes * lcghash_init in fp32, one multiply per element (28 x 4 x 4 on 4x4; the black-to-move plane takes part);
    2. v = the 32 bits of p as int32, sign-extended to int64;
    3. three nested chains acc = acc * M + 1 + v from acc = 0 in wrapping int64: over the last dimension, then over the other
       spatial dimension, then over the channels, giving H;
    4. index = wrapping |H| >> 31, masked to 32 bits (H = i64::MIN, where the reference's index is out of bounds, gives 0).

All integer arithmetic is modulo 2**64 on purpose: it is done on uint64 arrays, where numpy wraps silently, and the overflow
warnings of the remaining signed steps are silenced, not avoided."""
import numpy as np

MULTIPLIER = 6364136223846793005
INCREMENT = 1
HASH_BITS = 32
MAXIMUM_VARIANCE = np.float32(4.0)
_M = np.uint64(MULTIPLIER)
_ONE = np.uint64(INCREMENT)


def products(planes, init):
    """Step 1: the fp32 products, shape [batch, channels, n, n]."""
    planes, init = np.asarray(planes, np.float32), np.asarray(init, np.float32)
    assert planes.ndim == 4 and init.shape == planes.shape[1:], (planes.shape, init.shape)
    p = planes * init
    assert p.dtype == np.float32
    return p


def product_bits(planes, init):
    """Step 2: int64 values of the products' bit patterns."""
    return np.ascontiguousarray(products(planes, init)).view(np.int32).astype(np.int64)


def _chain(v):
    """acc = acc * M + 1 + v[..., i] over the last axis, modulo 2**64."""
    v = np.ascontiguousarray(v).view(np.uint64)
    acc = np.zeros(v.shape[:-1], np.uint64)
    with np.errstate(over="ignore"):
        for i in range(v.shape[-1]):
            acc = acc * _M + _ONE + v[..., i]
    return acc.view(np.int64)


def unshifted(planes, init):
    """Step 3: H, int64 [batch]."""
    return _chain(_chain(_chain(product_bits(planes, init))))


def shift(h):
    """Step 4 on int64 H."""
    h = np.asarray(h, np.int64)
    with np.errstate(over="ignore"):
        a = np.abs(h)                      # wraps at i64::MIN, like i64::wrapping_abs
    return ((a >> np.int64(63 - HASH_BITS)) & np.int64(0xFFFFFFFF)).astype(np.uint32)


def indices(planes, init):
    return shift(unshifted(planes, init))


class SeenSet:
    """The reference's BitBox as a set of indices: update_counts (:244-249) and forward_hash (:251-264)."""

    def __init__(self, seen=()):
        self.seen = set(int(i) for i in seen)

    def update(self, idx):
        self.seen.update(int(i) for i in np.asarray(idx).ravel())

    def contains(self, idx):
        return np.array([int(i) in self.seen for i in np.asarray(idx).ravel()], bool)

    def local(self, idx):
        return np.where(self.contains(idx), np.float32(0.0), MAXIMUM_VARIANCE).astype(np.float32)

    def sorted(self):
        return np.array(sorted(self.seen), np.uint64)
