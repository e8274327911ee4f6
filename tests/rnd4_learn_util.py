"""TEST INFRASTRUCTURE: the weights and batches shared by tests/test_rnd4_learn_ref.py (CPU) and tests/test_gpu_rnd4_learn.py (GPU), so
that what the CPU test asserts about the fixture is asserted about what the GPU test runs."""
import numpy as np

import rnd4_ref as R

SEED = 34
BATCHES = (64, 128, 192)   # the smallest batch the trainer accepts, the shipped one, a row count that is no power of two
_CACHE = {}


def weights():
    """init_weights at trained statistics with a dense LayerNorm affine on both towers (tch's default is weight 1, bias 0)"""
    from takzero_amd import weights as W

    if "w" not in _CACHE:
        w = W.init_weights(W.ARCH_NET4_RND, seed=SEED, trained_stats=True)
        rng = np.random.default_rng(SEED)
        for t in R.TOWERS:
            w[t + ".layer_norm.weight"] = rng.normal(1, 0.3, size=(28, 4, 4)).astype(np.float32)
            w[t + ".layer_norm.bias"] = rng.normal(0, 0.3, size=(28, 4, 4)).astype(np.float32)
        _CACHE["w"] = w
    return _CACHE["w"]


def batches(oracle, B):
    """three batches of B positions: (states, planes, policy, mask, value, ube) as test_gpu_learn._batch makes them"""
    from test_gpu_learn import _batch

    if B not in _CACHE:
        _CACHE[B] = [_batch(oracle, 4, B, 3400 + 10 * B + step) for step in range(3)]
    return _CACHE[B]
