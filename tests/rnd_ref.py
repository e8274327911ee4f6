"""TEST INFRASTRUCTURE: the RND distillation step (net5.rs:193-204; learn/src/main.rs:404) in plain PyTorch with autograd, fp64 by
default: forward_rnd of both MLPs on x / sum(x^2), loss_rnd = mean of the squared distance, torch.optim.Adam on the predictor.
The same formulas as oracle/nets_torch.rnd_raw, which runs under no_grad and cannot give gradients."""
import numpy as np
import torch
import torch.nn.functional as F

LAYERS = ("input_linear", "hidden_linear", "final_linear")
NAMES = tuple("rnd_learning.%s.%s" % (layer, part) for layer in LAYERS for part in ("weight", "bias"))


def make_params(w, dtype=torch.float64):
    """name -> tensor of `dtype` for both MLPs; the predictor's require grad, the target's do not."""
    p = {}
    for net in ("rnd_learning", "rnd_target"):
        for layer in LAYERS:
            for part in ("weight", "bias"):
                name = "%s.%s.%s" % (net, layer, part)
                p[name] = torch.from_numpy(np.array(w[name], dtype=np.float32, copy=True)).to(dtype)
                if net == "rnd_learning":
                    p[name].requires_grad_(True)
    return p


def forward_rnd(p, planes, relu_masks=None, kink=None, dtype=torch.float64):
    """-> (raw [B], layers): layers[net] = [(pre-activation, activation)] of the two hidden layers + (output, output), net 0 the
    predictor and 1 the target.  relu_masks[layer] / kink[layer] (predictor only, the one with a backward): where a ReLU's input
    is within kink of zero the mask decides the side, as in oracle/learn_torch.forward_t."""
    x = torch.from_numpy(planes) if isinstance(planes, np.ndarray) else planes
    x = x.reshape(x.shape[0], -1).to(dtype)
    x = x / x.square().sum(dim=1, keepdim=True)
    layers = []
    for net in ("rnd_learning", "rnd_target"):
        h, mine = x, []
        for i, layer in enumerate(LAYERS):
            t = F.linear(h, p["%s.%s.weight" % (net, layer)], p["%s.%s.bias" % (net, layer)])
            if i == 2:
                h = t
            elif relu_masks is None or net == "rnd_target":
                h = F.relu(t)
            else:
                h = t * torch.where(t.detach().abs() < kink[i], relu_masks[i], t.detach() > 0).to(t.dtype)
            mine.append((t, h))
        layers.append(mine)
    raw = (layers[0][2][1] - layers[1][2][1].detach()).square().sum(dim=1)
    return raw, layers


def adam(p, lr):
    return torch.optim.Adam([p[k] for k in NAMES], lr=lr)
