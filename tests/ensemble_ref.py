"""net4_ensemble restated for the tests, in numpy / torch and nothing of the library (tests/test_ensemble_ref.py holds this module to its
own sensitivity; the GPU tests compare the kernels with it):

  heads_f64         the sixteen heads on a trunk output, fp64: conv1x1(256 -> 1) + bias, ReLU, view 16, Linear(16 -> 1) + bias, tanh
                    (net4_ensemble.rs:107-131, 157-171)
  var16_f32         the population variance over the sixteen values in fp32, two passes in index order:
                    m = (((v0 + v1) + v2) + ... + v15) * 0.0625, s = sum_i (v_i - m) * (v_i - m), var = s * 0.0625
  variance_rule     clamp(max(exp(ube), var_16), 0, 4)  (net4_ensemble.rs:225-233); exp is handed in (the device's expf in the GPU tests)
  bootstrap_targets -0.997 * values of the next position, every entry of a finished game overwritten by
                    f32::from(Eval::from(terminal).negate())  (eee/src/ensemble.rs:298-315; eval.rs:40-47, 95-105)
  loss_and_grads    mean over [B, 16] of (target - value)^2 and its autograd gradients with respect to the heads' 64 variables, the trunk
                    output detached (ensemble.rs:335-337; net4_ensemble.rs:153)

`act` is the trunk's output as [B, 16 squares, 256 channels] (the layout of tz_trainer_activation); head weights come by the variable
names tch gives them: `ensemble head i.conv2d.weight` [1,256,1,1], `.conv2d.bias` [1], `.linear.weight` [1,16], `.linear.bias` [1]."""
import numpy as np

SIZE = 16
DISCOUNT = np.float32(0.997)
WIN, LOSS, DRAW, NONE = 0, 1, 2, -1          # Terminal from the side to move (env.rs:27-31)
PARTS = ("conv2d.weight", "conv2d.bias", "linear.weight", "linear.bias")


def name(i, part):
    return "ensemble head %d.%s" % (i, part)


def names():
    return [name(i, p) for i in range(SIZE) for p in PARTS]


def stacked(w, dtype=np.float64):
    """(conv weights [16,256], conv biases [16], linear weights [16,16 squares], linear biases [16]) of a store."""
    cw = np.stack([np.asarray(w[name(i, PARTS[0])], dtype).reshape(-1) for i in range(SIZE)])
    cb = np.array([np.asarray(w[name(i, PARTS[1])], dtype).reshape(()) for i in range(SIZE)])
    lw = np.stack([np.asarray(w[name(i, PARTS[2])], dtype).reshape(-1) for i in range(SIZE)])
    lb = np.array([np.asarray(w[name(i, PARTS[3])], dtype).reshape(()) for i in range(SIZE)])
    return cw, cb, lw, lb


def heads_pre_f64(act, w):
    """The heads' pre-activations (before tanh), fp64: [B, 16]."""
    cw, cb, lw, lb = stacked(w)
    conv = np.einsum("bsc,hc->bhs", np.asarray(act, np.float64), cw) + cb[None, :, None]
    return np.einsum("bhs,hs->bh", np.maximum(conv, 0.0), lw) + lb[None, :]


def heads_f64(act, w, tanh=True):
    pre = heads_pre_f64(act, w)
    return np.tanh(pre) if tanh else pre


def var16_f32(values, unbiased=False):
    """values [B, 16] fp32 -> [B] fp32, every operation rounded to fp32 in the order of the module docstring."""
    v = np.asarray(values, np.float32)
    assert v.shape[1] == SIZE
    total = v[:, 0].copy()
    for i in range(1, SIZE):
        total = (total + v[:, i]).astype(np.float32)
    m = (total * np.float32(0.0625)).astype(np.float32)
    s = np.zeros(len(v), np.float32)
    for i in range(SIZE):
        d = (v[:, i] - m).astype(np.float32)
        s = (s + (d * d).astype(np.float32)).astype(np.float32)
    if unbiased:
        return (s / np.float32(SIZE - 1)).astype(np.float32)
    return (s * np.float32(0.0625)).astype(np.float32)


def variance_rule(exp_ube, var16):
    return np.clip(np.maximum(np.asarray(exp_ube, np.float32), np.asarray(var16, np.float32)), np.float32(0), np.float32(4)).astype(np.float32)


def terminal_value(terminal):
    """f32::from(Eval::from(t).negate()): Win(0) -> Loss(1) -> -0.997, Loss(0) -> Win(1) -> 0.997, Draw(0) -> Draw(1) -> 0.997 * 0."""
    return DISCOUNT * np.float32({WIN: -1.0, LOSS: 1.0, DRAW: 0.0}[int(terminal)])


def bootstrap_targets(next_values, terminals, discount=DISCOUNT, overwrite=True):
    """next_values [B, 16] fp32 (the net on the positions after the sampled move), terminals [B] (NONE where the game goes on)."""
    out = (-np.float32(discount) * np.asarray(next_values, np.float32)).astype(np.float32)
    if overwrite:
        for i, t in enumerate(terminals):
            if int(t) != NONE:
                out[i, :] = terminal_value(t)
    return out


def sample_action(moves, probs, draw):
    """The first action whose cumulative probability passes draw * total (choose_weighted with the randomness handed in)."""
    cum = np.cumsum(np.asarray(probs, np.float64))
    return int(np.asarray(moves)[min(int(np.searchsorted(cum, draw * cum[-1], side="right")), len(cum) - 1)])


def loss_and_grads(act, w, targets, dtype=None, relu_mask=None):
    """(loss, values [B,16], {variable name: gradient}) by torch autograd in `dtype` (default fp64).  relu_mask [B,16 heads,16 squares]
    (optional, bool): the side of ReLU's kink to take, where another implementation's conv output decides it (tests/learn_check.py's rule)."""
    import torch

    dtype = dtype or torch.float64
    params = {k: torch.tensor(np.asarray(w[k], np.float64), dtype=dtype, requires_grad=True) for k in names()}
    x = torch.tensor(np.asarray(act, np.float64), dtype=dtype)           # detached: no gradient reaches the trunk
    cw = torch.stack([params[name(i, PARTS[0])].reshape(-1) for i in range(SIZE)])
    cb = torch.stack([params[name(i, PARTS[1])].reshape(()) for i in range(SIZE)])
    lw = torch.stack([params[name(i, PARTS[2])].reshape(-1) for i in range(SIZE)])
    lb = torch.stack([params[name(i, PARTS[3])].reshape(()) for i in range(SIZE)])
    conv = torch.einsum("bsc,hc->bhs", x, cw) + cb[None, :, None]
    h = torch.relu(conv) if relu_mask is None else conv * torch.tensor(np.asarray(relu_mask), dtype=dtype)
    values = torch.tanh(torch.einsum("bhs,hs->bh", h, lw) + lb[None, :])
    loss = (torch.tensor(np.asarray(targets, np.float64), dtype=dtype) - values).square().mean()
    loss.backward()
    return float(loss.detach()), values.detach().numpy(), {k: p.grad.numpy().reshape(np.asarray(w[k]).shape) for k, p in params.items()}


def dyadic_heads(seed, act, scale_bits=None):
    """Sixteen different heads in the style of tests/exact_net.py's value head, for an integer-valued trunk output `act` [B,16,256]: conv
    weights +-1 on 16 channels, an integer bias that lets about half of the squares pass the ReLU, linear weights +-2^-s with s chosen
    so that the pre-activation stays within about +-2, linear bias a multiple of 1/8.  Returns the 64 variables."""
    rng = np.random.default_rng(4000 + seed)
    act = np.asarray(act, np.float64)
    out = {}
    for i in range(SIZE):
        cw = np.zeros(256, np.float32)
        idx = rng.choice(256, size=16, replace=False)
        cw[idx] = np.where(rng.integers(2, size=16) == 1, 1.0, -1.0)
        pre = act @ cw.astype(np.float64)
        cb = np.float32(-np.floor(np.quantile(pre, 0.5)))
        h = np.maximum(pre + float(cb), 0.0)
        sign = np.where(rng.integers(2, size=16) == 1, 1.0, -1.0)
        raw = (h * sign[None, :]).sum(axis=1)
        s = int(np.clip(np.ceil(np.log2(max(1.0, np.abs(raw).max()) / 2.0)), 2, 12)) if scale_bits is None else scale_bits
        out[name(i, PARTS[0])] = cw.reshape(1, 256, 1, 1)
        out[name(i, PARTS[1])] = np.array([cb], np.float32)
        out[name(i, PARTS[2])] = (sign * 2.0 ** -s).astype(np.float32).reshape(1, 16)
        out[name(i, PARTS[3])] = np.array([(i % 5 - 2) / 8.0], np.float32)
    return out
