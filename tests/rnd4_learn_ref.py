"""TEST INFRASTRUCTURE: the distillation step of net4_rnd's predictor tower (net4_rnd.rs:126-166, 210-223; residual.rs:8-63;
learn/src/main.rs:404-405) in plain PyTorch with autograd, fp64: forward_rnd(xs, true) = the predictor in training mode (BatchNorm with
batch statistics, running statistics tracked with momentum 0.1 and the unbiased variance), the target detached and in eval mode, raw =
sum_512 (predictor - target)^2, loss = raw.mean(), torch.optim.Adam on the predictor's 32 trained variables.  tests/rnd_ref.py is the
model; tests/rnd4_ref.py holds the same towers in numpy for inference.

The keyword switches of forward_rnd / loss break the graph one way each (tests/test_rnd4_learn_ref.py holds the reference to noticing
them)."""
import numpy as np
import torch
import torch.nn.functional as F

import rnd4_ref as R

EPS, MOMENTUM, LAYERS = 1e-5, 0.1, 10
PREDICTOR, TARGET = R.TOWERS


def trained_names(prefix=PREDICTOR):
    """LayerNorm weight and bias, then ten times conv weight, BatchNorm weight, BatchNorm bias"""
    out = [prefix + ".layer_norm.weight", prefix + ".layer_norm.bias"]
    for conv, norm in R.layer_names(prefix):
        out += [conv + ".weight", norm + ".weight", norm + ".bias"]
    return out


def stat_names(prefix=PREDICTOR):
    return [norm + "." + v for _conv, norm in R.layer_names(prefix) for v in ("running_mean", "running_var")]


NAMES = tuple(trained_names())
STATS = tuple(stat_names())


def make_params(w, dtype=torch.float64):
    """name -> tensor of `dtype` for both towers; the predictor's trained variables require grad, nothing else does."""
    p = {}
    for name in R.tensor_names()[:-2]:
        p[name] = torch.from_numpy(np.array(w[name], dtype=np.float32, copy=True)).to(dtype)
        if name.endswith(".layer_norm.weight") or name.endswith(".layer_norm.bias"):
            p[name] = p[name].reshape(R.CIN, R.N, R.N)
    for name in NAMES:
        p[name].requires_grad_(True)
    return p


def adam(p, lr):
    return torch.optim.Adam([p[k] for k in NAMES], lr=lr)


def residual(l):
    """layer l (0..9) adds the block's input before its ReLU"""
    return l >= 2 and l % 2 == 0 and l < LAYERS - 1


def _tower(p, prefix, x, train, masks, kinks, f):
    """-> ([LayerNorm output, a_1 .. a_10], [conv outputs before BatchNorm], [ReLU inputs], new running statistics)"""
    flat = x.reshape(len(x), -1)
    mean = flat.mean(dim=1, keepdim=True)
    var = flat.var(dim=1, unbiased=bool(f.get("ln_sample_variance")), keepdim=True)
    xhat = ((flat - mean) / torch.sqrt(var + EPS)).reshape(x.shape)
    lw, lb = p[prefix + ".layer_norm.weight"], p[prefix + ".layer_norm.bias"]
    if f.get("ln_affine_detached"):
        lw, lb = lw.detach(), lb.detach()
    h = xhat * lw + lb
    acts, pres, zs, running = [h], [], [], {}
    keep = None
    for l, (conv, norm) in enumerate(R.layer_names(prefix)):
        y = F.conv2d(h, p[conv + ".weight"], padding=1)
        g, b = p[norm + ".weight"].view(1, -1, 1, 1), p[norm + ".bias"].view(1, -1, 1, 1)
        rm, rv = p[norm + ".running_mean"], p[norm + ".running_var"]
        if train:
            n = y.numel() // y.shape[1]
            m, v = y.mean(dim=(0, 2, 3)), y.var(dim=(0, 2, 3), unbiased=False)
            mom = f.get("momentum", MOMENTUM)
            tracked = v.detach() if f.get("biased_running_var") else v.detach() * n / (n - 1)
            running[norm + ".running_mean"] = (1 - mom) * rm + mom * m.detach()
            running[norm + ".running_var"] = (1 - mom) * rv + mom * tracked
        else:
            m, v = rm, rv
        z = (y - m.view(1, -1, 1, 1)) / torch.sqrt(v.view(1, -1, 1, 1) + EPS) * g + b
        if residual(l):
            z = z + (keep.detach() if f.get("residual_backward_missing") else keep)
        if l < LAYERS - 1 or f.get("final_relu"):
            if masks is None or l >= LAYERS - 1:
                h = F.relu(z)
            else:   # within the kink the mask decides the side, as in oracle/learn_torch.forward_t
                h = z * torch.where(z.detach().abs() < kinks[l], masks[l], z.detach() > 0).to(z.dtype)
        else:
            h = z
        if l % 2 == 0:
            keep = h
        pres.append(y)
        zs.append(z)
        acts.append(h)
    return acts, pres, zs, running


def forward_rnd(p, planes, train=True, masks=None, kinks=None, **faults):
    """forward_rnd(xs, train) -> dict: raw [B]; acts[tower] = [LayerNorm output [B,28,4,4], a_1 .. a_10 [B,32,4,4]]; pre[tower] = the ten conv
    outputs before BatchNorm; z[tower] = the inputs of the ReLUs (the last layer's has none); running = the predictor's running
    statistics after the forward (train only; p itself is not changed).  masks[l] / kinks[l], l = 0..8 (predictor only): where a
    ReLU's input is within kinks[l] of zero, masks[l] decides the side."""
    x = torch.from_numpy(np.asarray(planes)) if not torch.is_tensor(planes) else planes
    x = x.reshape(len(x), R.CIN, R.N, R.N).to(torch.float64)
    pa, pp, pz, running = _tower(p, PREDICTOR, x, train, masks, kinks, faults)
    target_train = bool(faults.get("target_train"))
    ta, tp, tz, _ = _tower(p, TARGET, x, target_train, None, None, {"final_relu": faults.get("final_relu")})
    out_t = ta[-1] if faults.get("target_grad") else ta[-1].detach()
    raw = (pa[-1] - out_t).flatten(1, 3).square().sum(dim=1)
    return {"raw": raw, "acts": (pa, ta), "pre": (pp, tp), "z": (pz, tz), "running": running}


def loss(raw, **faults):
    """learn/src/main.rs:404: forward_rnd(input, true).mean()"""
    return raw.sum() / (512 * len(raw)) if faults.get("loss_over_512") else raw.mean()


def commit_running(p, running):
    with torch.no_grad():
        for k, v in running.items():
            p[k].copy_(v)


def calibrate(w, early, late):
    """update_rnd (learn/src/rnd_normalization.rs:74-78): (min of forward_rnd(early, false), max of forward_rnd(late, false)) in fp64"""
    p = make_params(w)
    with torch.no_grad():
        return float(forward_rnd(p, early, train=False)["raw"].min()), float(forward_rnd(p, late, train=False)["raw"].max())
