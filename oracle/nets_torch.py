"""Plain PyTorch fp32 restatement of the reference's network graphs (test infrastructure only).

    net5          takzero/src/network/net5.rs:44-218      (20 blocks, RND uncertainty)
    net4/6 simhash takzero/src/network/net6_simhash.rs:43-256 (16 blocks, SimHash uncertainty)
    residual      takzero/src/network/residual.rs:13-63

The reference executes these graphs through LibTorch (tch 0.22); torch in this image is the same
ATen code on CPU, so this module is the numeric oracle for the HIP forward.
Parity unpinned for the forward's *values*: the reference holds no input/output vector for its nets (its
tests check shapes), so tests/golden/net_forward.json is this module's output, not the reference's.
Weights come from takzero_amd.weights (name -> ndarray)."""
import numpy as np
import torch
import torch.nn.functional as F

MAXIMUM_VARIANCE = 4.0


def _t(w, name):
    return torch.from_numpy(np.ascontiguousarray(w[name]))


def forward(w, planes, blocks, dtype=torch.float32, trace=None):
    """planes [B,C,N,N] fp32 -> (policy [B,OUT,N,N], value [B], ube [B]); net5.rs:184-191.  `dtype` is the arithmetic of the
    whole graph (fp32 as the reference runs it, or torch.float64: every tensor converted, eps added in double).  `trace`, a
    list, receives (name, tensor) for every stored trunk activation - "core.input", "core.res_block_i.a" (after its ReLU),
    "core.res_block_i" (the block's output) - and for the heads' outputs before tanh ("value.pre", "ube.pre")."""
    x = torch.from_numpy(planes) if isinstance(planes, np.ndarray) else planes
    p_ = lambda name: _t(w, name).to(dtype)
    bn = lambda x, p: F.batch_norm(x, p_(p + ".running_mean"), p_(p + ".running_var"), p_(p + ".weight"), p_(p + ".bias"),
                                   training=False, eps=1e-5)
    keep = (lambda name, t: trace.append((name, t))) if trace is not None else (lambda name, t: None)
    with torch.no_grad():
        x = F.relu(bn(F.conv2d(x.to(dtype), p_("core.input_conv2d.weight"), padding=1), "core.batch_norm"))
        keep("core.input", x)
        for b in range(blocks):
            p = "core.res_block_%d" % b
            y = F.relu(bn(F.conv2d(x, p_(p + ".a.conv2d.weight"), padding=1), p + ".a.batch_norm"))   # residual.rs:13-37
            keep(p + ".a", y)
            y = bn(F.conv2d(y, p_(p + ".b.conv2d.weight"), padding=1), p + ".b.batch_norm")
            x = F.relu(y + x)  # residual.rs:58-62
            keep(p, x)
        policy = F.conv2d(x, p_("policy.conv2d.weight"), p_("policy.conv2d.bias"), padding=1)
        heads = []
        for head in ("value", "ube"):
            h = F.relu(F.conv2d(x, p_(head + ".conv2d.weight"), p_(head + ".conv2d.bias")))
            h = h.view(h.shape[0], -1)
            heads.append(F.linear(h, p_(head + ".linear.weight"), p_(head + ".linear.bias")).view(-1))
            keep(head + ".pre", heads[-1])
        return policy, torch.tanh(heads[0]), heads[1]


def rnd_raw(w, planes, dtype=torch.float32):
    """forward_rnd (net5.rs:193-204) in `dtype` throughout: the squared distance of the two RND MLPs' outputs, [B]."""
    x = torch.from_numpy(planes) if isinstance(planes, np.ndarray) else planes
    with torch.no_grad():
        x = x.reshape(x.shape[0], -1).to(dtype)
        x = x / x.square().sum(dim=1, keepdim=True)
        outs = []
        for net in ("rnd_learning", "rnd_target"):
            p = lambda layer, part: _t(w, "%s.%s.%s" % (net, layer, part)).to(dtype)
            h = F.relu(F.linear(x, p("input_linear", "weight"), p("input_linear", "bias")))
            h = F.relu(F.linear(h, p("hidden_linear", "weight"), p("hidden_linear", "bias")))
            outs.append(F.linear(h, p("final_linear", "weight"), p("final_linear", "bias")))
        return (outs[0] - outs[1]).square().sum(dim=1)


def rnd_raw_storage(w, planes, storage):
    """rnd_raw of the 16-bit MFMA path (storage torch.float16 or torch.bfloat16), rounded where the kernels store and exact
    (fp64) in between: x / sum(x^2) computed in fp32 and stored (rnd_prep_state_kernel, the fused kernels' RND-input write); the
    weights as build_layer converts them (round to nearest even); h1 and h2 as the linear layers' epilogue writes them (fp32
    accumulator + bias, ReLU, converted); the final layer's output kept in fp32 (out_f32).  The distance is summed in fp64."""
    x = torch.from_numpy(planes) if isinstance(planes, np.ndarray) else planes
    st = lambda t: t.to(torch.float32).to(storage).to(torch.float64)
    with torch.no_grad():
        x = x.reshape(x.shape[0], -1).to(torch.float32)
        x = st(x / x.square().sum(dim=1, keepdim=True))
        outs = []
        for net in ("rnd_learning", "rnd_target"):
            wt = lambda layer: st(_t(w, "%s.%s.weight" % (net, layer)))
            b = lambda layer: _t(w, "%s.%s.bias" % (net, layer)).to(torch.float64)
            h = st(F.relu(F.linear(x, wt("input_linear"), b("input_linear"))))
            h = st(F.relu(F.linear(h, wt("hidden_linear"), b("hidden_linear"))))
            outs.append(F.linear(h, wt("final_linear"), b("final_linear")).to(torch.float32).to(torch.float64))
        return (outs[0] - outs[1]).square().sum(dim=1)


def rnd_calibrate(w, early, late):
    """update_rnd (learn/src/rnd_normalization.rs:74-78) in fp64: min of rnd_raw over the early reference positions, max over
    the late ones; returns (min, max) as Python floats."""
    return float(rnd_raw(w, early, torch.float64).min()), float(rnd_raw(w, late, torch.float64).max())


def rnd(w, planes):
    """normalized_rnd, net5.rs:193-211."""
    with torch.no_grad():
        raw = rnd_raw(w, planes)
        mn, mx = _t(w, "min"), _t(w, "max")
        return ((raw - mn) / (mx - mn)).clamp(0.0, 1.0) * MAXIMUM_VARIANCE


def simhash_indices(w, planes, cin, return_dots=False):
    """get_indices, net6_simhash.rs:202-236 (with return_dots also the 32 projections whose signs are the bits)."""
    x = torch.from_numpy(planes.copy())
    with torch.no_grad():
        x[:, cin - 2] = 0.0
        dots = x.reshape(x.shape[0], -1) @ _t(w, "simhash_matrix")
        bits = (~(dots < 0.0)).to(torch.int64)
        idx = (bits * (2 ** torch.arange(32, dtype=torch.int64))).sum(dim=1).numpy()
        return (idx, dots.numpy()) if return_dots else idx


def simhash_dots(w, planes, dtype=torch.float64):
    """The 32 projections of get_indices (net6_simhash.rs:202-233) in `dtype` throughout: the colour plane cin - 2 zeroed,
    view(-1, cin * n * n) @ simhash_matrix.  [B, 32]; bit j of a position's index is set where column j is not below zero."""
    x = torch.from_numpy(np.array(planes, dtype=np.float32, copy=True))
    with torch.no_grad():
        x[:, x.shape[1] - 2] = 0.0
        return x.reshape(x.shape[0], -1).to(dtype) @ _t(w, "simhash_matrix").to(dtype)


def simhash_margin(w, planes):
    """Per (position, bit) the a-priori bound on the error of an fp32 evaluation of that projection, whatever the order of the
    sum and with or without FMA: K * 2**-24 * (|x| @ |matrix|), K = cin * n * n terms, 2**-24 the unit roundoff (every one of
    the K - 1 additions and K products is off by at most one relative unit roundoff of a partial result no larger than
    sum |x_k m_k|; K u bounds the compounded (1 + u)**K - 1 to first order, and the planes are mostly zero, which adds nothing).
    Derived, not measured.  fp64, [B, 32].  A bit is decided where |simhash_dots| exceeds it."""
    x = torch.from_numpy(np.array(planes, dtype=np.float32, copy=True))
    with torch.no_grad():
        x[:, x.shape[1] - 2] = 0.0
        flat = x.reshape(x.shape[0], -1).to(torch.float64)
        return flat.shape[1] * 2.0 ** -24 * (flat.abs() @ _t(w, "simhash_matrix").to(torch.float64).abs())


def variance(w, planes, ube, arch, seen=None):
    """net5.rs:271-278 / net6_simhash.rs:311-318."""
    with torch.no_grad():
        if arch == 5:
            local = rnd(w, planes)
        elif arch in (4, 6):
            idx = simhash_indices(w, planes, planes.shape[1])
            local = torch.tensor([0.0 if (seen is not None and int(i) in seen) else MAXIMUM_VARIANCE for i in idx])
        else:
            local = torch.zeros_like(ube)
        return torch.maximum(ube.exp(), local).clamp(0.0, MAXIMUM_VARIANCE)
