"""The `learn` step on the GPU (learn/src/main.rs:322-423): tensors from a batch of targets
(create_input_and_target_tensors) and compute_loss_and_take_step, over the tz_trainer_* ABI."""
import ctypes as C

import numpy as np

from . import _lib, api
from ._lib import check

BATCH_SIZE = 128        # learn/src/main.rs:43
LEARNING_RATE = 1e-4    # learn/src/main.rs:46
PARAM, GRAD, ADAM_M, ADAM_V = 0, 1, 2, 3


def target_tensors(targets, n, rng=None):
    """create_input_and_target_tensors (learn/src/main.rs:330-374): states, dense policy target (policy_tensor), mask of
    non-legal outputs (move_mask), value and UBE targets (raw variances; the log and clamp are applied inside the
    step).  `targets` = (state, moves, policy, value, ube) tuples; with `rng` every target is first put through a
    random board symmetry (target.augment(rng), target.rs:41-53).  Vectorised over the batch."""
    B, out = len(targets), api.policy_size(n)
    states = np.zeros(B, api.STATE_DTYPE)
    for i, t in enumerate(targets):
        states[i] = t[0]
    counts = np.fromiter((len(t[1]) for t in targets), np.int64, B)
    moves = np.concatenate([np.asarray(t[1], np.int64) for t in targets]) if B else np.zeros(0, np.int64)
    probs = np.concatenate([np.asarray(t[2], np.float32) for t in targets]) if B else np.zeros(0, np.float32)
    rows = np.repeat(np.arange(B), counts)
    if rng is not None:
        from . import augment as AU

        states, moves = AU.augment_batch(states, moves, rows, rng, n)
    policy = np.zeros((B, out), np.float32)
    mask = np.ones((B, out), np.uint8)
    policy[rows, moves] = probs
    mask[rows, moves] = 0
    value = np.fromiter((t[3] for t in targets), np.float32, B)
    ube = np.fromiter((t[4] for t in targets), np.float32, B)
    return states, policy, mask, value, ube


class Trainer:
    """Net + Adam optimizer of learn::main (learn/src/main.rs:100-110) on one GPU."""

    # the variables of net5's RND predictor (net5.rs:114-148): trained by the step while rnd_enable() is on, and then
    # readable / writable through tensor() like the names of `names`
    RND_NAMES = tuple("rnd_learning.%s.%s" % (layer, part) for layer in ("input_linear", "hidden_linear", "final_linear")
                      for part in ("weight", "bias"))

    # the variables of net4_ensemble's sixteen heads (net4_ensemble.rs:107-131): trained by the step while ensemble targets are
    # set, and then readable / writable through tensor() like the names of `names`
    ENSEMBLE_NAMES = tuple("ensemble head %d.%s" % (i, part) for i in range(api.ENSEMBLE_SIZE)
                           for part in ("conv2d.weight", "conv2d.bias", "linear.weight", "linear.bias"))

    # the variables of net4_rnd's predictor tower (net4_rnd.rs:126-166): LayerNorm weight and bias, then ten times conv weight,
    # BatchNorm weight and bias (the 32 trained ones), then the 20 running statistics; trained / tracked by the step while
    # rnd4_enable() is on, and then readable / writable through tensor() (the running statistics with what = PARAM only)
    RND4_LAYERS = ("input_conv2d|batch_norm",) + tuple("res_block_%d.%s.conv2d|res_block_%d.%s.batch_norm" % (b, h, b, h)
                                                        for b in range(4) for h in "ab") + ("last_small_block.conv2d|last_small_block.batch_norm",)
    RND4_TRAINED = ("rnd_predictor.layer_norm.weight", "rnd_predictor.layer_norm.bias") + tuple(
        "rnd_predictor." + name for layer in RND4_LAYERS for name in
        (layer.split("|")[0] + ".weight", layer.split("|")[1] + ".weight", layer.split("|")[1] + ".bias"))
    RND4_STATS = tuple("rnd_predictor.%s.%s" % (layer.split("|")[1], part) for layer in RND4_LAYERS for part in ("running_mean", "running_var"))
    RND4_NAMES = RND4_TRAINED + RND4_STATS

    def __init__(self, arch=api.ARCH_NET5, n=0, blocks=0, batch=BATCH_SIZE, lr=LEARNING_RATE, device=0):
        from . import weights as W

        self.lib = _lib.load()
        self.arch, self.n = arch, W.arch_board(arch, n)
        self.blocks, self.batch = W.arch_blocks(arch, blocks), batch
        self.h = C.c_void_p()
        check(self.lib.tz_trainer_create(self.n, arch, device, self.blocks, batch, lr, C.byref(self.h)))
        self.names = {}
        buf = C.create_string_buffer(256)
        cnt = C.c_uint64()
        for i in range(self.lib.tz_trainer_tensor_count(self.h)):
            check(self.lib.tz_trainer_tensor_info(self.h, i, buf, 256, C.byref(cnt)))
            self.names[buf.value.decode()] = int(cnt.value)
        self.shapes = {name: self._shape(name, count) for name, count in self.names.items()}

    def _shape(self, name, count):
        """The variable's shape in the reference's VarStore (param_dims in csrc/tz_learn.hip), whichever way it was loaded."""
        from . import weights as W

        if name in ("value.conv2d.weight", "ube.conv2d.weight"):
            return (1, count, 1, 1)
        if name.endswith("conv2d.weight"):
            co = W.output_channels(self.n) if name.startswith("policy.") else W.FILTERS
            return (co, count // (9 * co), 3, 3)
        if name.endswith(".linear.weight"):
            return (1, count)
        return (count,)

    def close(self):
        if self.h:
            self.lib.tz_trainer_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load_tensors(self, tensors):
        """VarStore contents by name (takzero_amd.weights / takzero_amd.ot).  The tensors the step never touches (RND nets,
        SimHash matrix, lcghash_init) go to the library with the rest, so save / to_net / the native save points carry them."""
        from .weights import dumps_tzw

        missing = [k for k in self.names if k not in tensors]
        if missing:
            raise ValueError("missing tensors: %s" % missing[:4])
        blob = dumps_tzw(tensors)
        buf = (C.c_char * len(blob)).from_buffer_copy(blob)
        check(self.lib.tz_trainer_load_weights_mem(self.h, C.addressof(buf), len(blob)))
        return self

    def load(self, path):
        """Network::load on the trainer's VarStore (learn/src/main.rs:107-120): a LibTorch archive or a .tzw container."""
        check(self.lib.tz_trainer_load(self.h, str(path).encode()))
        return self

    def save(self, path):
        """Network::save (learn/src/main.rs:247-266): a LibTorch archive under tch's variable names (or .tzw), written natively."""
        check(self.lib.tz_trainer_save(self.h, str(path).encode()))

    def from_net(self, net):
        check(self.lib.tz_trainer_from_net(self.h, net.h))
        return self

    def to_net(self, net):
        check(self.lib.tz_trainer_to_net(self.h, net.h))

    def tensor(self, name, what=PARAM):
        if name in self.RND_NAMES:
            shape = self._rnd_shape(name)
            out = np.zeros(shape, np.float32)
            check(self.lib.tz_trainer_get_tensor(self.h, name.encode(), what, out.ctypes.data, out.size))
            return out
        if name in self.RND4_NAMES:
            out = np.zeros(self._rnd4_shape(name), np.float32)
            check(self.lib.tz_trainer_get_tensor(self.h, name.encode(), what, out.ctypes.data, out.size))
            return out
        if name in self.ENSEMBLE_NAMES:
            shape = {"conv2d.weight": (1, 256, 1, 1), "conv2d.bias": (1,), "linear.weight": (1, self.n * self.n),
                     "linear.bias": (1,)}[name.split(".", 1)[1]]
            out = np.zeros(shape, np.float32)
            check(self.lib.tz_trainer_get_tensor(self.h, name.encode(), what, out.ctypes.data, out.size))
            return out
        out = np.zeros(self.names[name], np.float32)
        check(self.lib.tz_trainer_get_tensor(self.h, name.encode(), what, out.ctypes.data, out.size))
        return out.reshape(self.shapes.get(name, out.shape))

    def _rnd_shape(self, name):
        from . import weights as W

        _net, layer, part = name.split(".")
        cin = W.input_channels(self.n) * self.n * self.n
        out, inp = {"input_linear": (W.RND_HIDDEN, cin), "hidden_linear": (W.RND_HIDDEN, W.RND_HIDDEN),
                    "final_linear": (W.RND_OUT, W.RND_HIDDEN)}[layer]
        return (out, inp) if part == "weight" else (out,)

    @staticmethod
    def _rnd4_shape(name):
        from . import weights as W

        if ".layer_norm." in name:
            return (28, 4, 4)
        if name.endswith("conv2d.weight"):
            return (W.RND4_FILTERS, 28 if name.endswith(".input_conv2d.weight") else W.RND4_FILTERS, 3, 3)
        return (W.RND4_FILTERS,)

    def rnd4_enable(self, on=True):
        """tz_trainer_rnd4_enable: the step also trains net4_rnd's predictor tower (loss_rnd, learn/src/main.rs:404-405)."""
        check(self.lib.tz_trainer_rnd4_enable(self.h, 1 if on else 0))
        return self

    def rnd4_last(self):
        """(loss_rnd, forward_rnd(xs, true) [batch]) of the last enabled step, before that step's update."""
        loss, raw = C.c_float(), np.zeros(self.batch, np.float32)
        check(self.lib.tz_trainer_rnd4_last(self.h, C.byref(loss), raw.ctypes.data))
        return float(loss.value), raw

    def rnd4_activation(self, which, layer):
        """What the last enabled step left in tower `which` (0 predictor, 1 target): layer 0 the LayerNorm output [batch, 28, 4, 4];
        1..10 a conv layer's output after BatchNorm, residual and ReLU [batch, 16, 32]; 11..20 (predictor) the conv outputs before
        BatchNorm [batch, 16, 32]."""
        out = np.zeros((self.batch, 28, 4, 4) if layer == 0 else (self.batch, 16, 32), np.float32)
        check(self.lib.tz_trainer_rnd4_activation(self.h, which, layer, out.ctypes.data, out.size))
        return out

    def rnd4_calibrate(self, early, late, apply=True):
        """update_rnd (learn/src/rnd_normalization.rs:74-78) for net4_rnd: (min over the early states, max over the late ones) of the
        f32 inference tower on the current variables; with `apply` they become the variables min / max."""
        e, l = api._states(early), api._states(late)
        mn, mx = C.c_float(), C.c_float()
        check(self.lib.tz_trainer_rnd4_calibrate(self.h, e.ctypes.data, len(e), l.ctypes.data, len(l), 1 if apply else 0,
                                                 C.byref(mn), C.byref(mx)))
        return float(mn.value), float(mx.value)

    def _rnd_calls(self):
        """(enable, calibrate) of the trainer's RND predictor: net4_rnd's tower or net5's MLP."""
        if self.arch == api.ARCH_NET4_RND:
            return self.rnd4_enable, self.rnd4_calibrate
        return self.rnd_enable, self.rnd_calibrate

    def set_tensor(self, name, data, what=PARAM):
        """One trained variable (a name of `names`, or of RND_NAMES while RND training is enabled) in the reference's layout."""
        data = np.ascontiguousarray(data, np.float32)
        check(self.lib.tz_trainer_set_tensor(self.h, name.encode(), what, data.ctypes.data, data.size))

    def rnd_enable(self, on=True):
        """tz_trainer_rnd_enable: the step also trains net5's RND predictor (loss_rnd, learn/src/main.rs:404-405)."""
        check(self.lib.tz_trainer_rnd_enable(self.h, 1 if on else 0))
        return self

    def rnd_last(self):
        """(loss_rnd, forward_rnd [batch]) of the last step, before that step's update."""
        loss, raw = C.c_float(), np.zeros(self.batch, np.float32)
        check(self.lib.tz_trainer_rnd_last(self.h, C.byref(loss), raw.ctypes.data))
        return float(loss.value), raw

    def rnd_activation(self, which, layer):
        """What the last RND forward left in MLP `which` (0 learning, 1 target): layer 0 / 1 after the ReLU [batch, 1024],
        2 the output [batch, 512]."""
        from . import weights as W

        out = np.zeros((self.batch, W.RND_OUT if layer == 2 else W.RND_HIDDEN), np.float32)
        check(self.lib.tz_trainer_rnd_activation(self.h, which, layer, out.ctypes.data, out.size))
        return out

    def rnd_calibrate(self, early, late, apply=True):
        """update_rnd (learn/src/rnd_normalization.rs:74-78): (min over the early states, max over the late ones); with
        `apply` they become the variables min / max."""
        e, l = api._states(early), api._states(late)
        mn, mx = C.c_float(), C.c_float()
        check(self.lib.tz_trainer_rnd_calibrate(self.h, e.ctypes.data, len(e), l.ctypes.data, len(l), 1 if apply else 0,
                                                C.byref(mn), C.byref(mx)))
        return float(mn.value), float(mx.value)

    def set_ensemble_targets(self, targets):
        """tz_trainer_set_ensemble_targets: [batch, 16] targets arm the trainer (every later step also trains the sixteen heads,
        eee/src/ensemble.rs:318-351); None disarms it."""
        if targets is None:
            check(self.lib.tz_trainer_set_ensemble_targets(self.h, None))
            return self
        t = np.ascontiguousarray(targets, np.float32)
        if t.shape != (self.batch, api.ENSEMBLE_SIZE):
            raise ValueError("set_ensemble_targets: want [%d, %d] targets" % (self.batch, api.ENSEMBLE_SIZE))
        check(self.lib.tz_trainer_set_ensemble_targets(self.h, t.ctypes.data))
        return self

    def ensemble_last(self):
        """(loss_ensemble, the heads' values [batch, 16]) of the last armed step, before that step's update."""
        loss, values = C.c_float(), np.zeros((self.batch, api.ENSEMBLE_SIZE), np.float32)
        check(self.lib.tz_trainer_ensemble_last(self.h, C.byref(loss), values.ctypes.data))
        return float(loss.value), values

    def extras(self):
        """The variables the step never touches (RND nets, SimHash matrix, lcghash_init), as the library carries them."""
        from .weights import loads_tzw

        size = C.c_uint64()
        check(self.lib.tz_trainer_get_extras(self.h, None, 0, C.byref(size)))
        buf = (C.c_char * size.value)()
        check(self.lib.tz_trainer_get_extras(self.h, C.addressof(buf), size.value, C.byref(size)))
        return loads_tzw(bytes(buf))

    def tensors(self):
        """Current weights by name, ready for Net.load_tensors / weights.save_tzw."""
        out = {name: self.tensor(name) for name in self.names}
        out.update(self.extras())
        return out

    def step(self, states, policy, mask, value, ube, train_ube=True, apply=True, ensemble_targets=None):
        """compute_loss_and_take_step -> (loss_policy, loss_value, loss_ube).  `ensemble_targets` [batch, 16] (net4_ensemble) arm the
        trainer for this and later steps (set_ensemble_targets; loss_ensemble through ensemble_last)."""
        if ensemble_targets is not None:
            self.set_ensemble_targets(ensemble_targets)
        st = api._states(states)
        B = self.batch
        out = api.policy_size(self.n)
        policy = np.ascontiguousarray(policy, np.float32)
        mask = np.ascontiguousarray(mask, np.uint8)
        value = np.ascontiguousarray(value, np.float32)
        ube = np.ascontiguousarray(ube, np.float32)
        if len(st) != B or policy.shape != (B, out) or mask.shape != (B, out) or value.shape != (B,) or ube.shape != (B,):
            raise ValueError("step: batch tensors do not match the trainer's batch size %d" % B)
        losses = np.zeros(3, np.float32)
        check(self.lib.tz_trainer_step(self.h, st.ctypes.data, policy.ctypes.data, mask.ctypes.data, value.ctypes.data,
                                       ube.ctypes.data, 1 if train_ube else 0, 1 if apply else 0, losses.ctypes.data))
        return tuple(float(x) for x in losses)

    def outputs(self):
        B, out = self.batch, api.policy_size(self.n)
        pol, val, ube = np.zeros((B, out), np.float32), np.zeros(B, np.float32), np.zeros(B, np.float32)
        check(self.lib.tz_trainer_outputs(self.h, pol.ctypes.data, val.ctypes.data, ube.ctypes.data))
        return pol, val, ube

    def activation(self, layer):
        """Output of trunk layer `layer` in the last step's forward, [batch, n*n, 256] (tz_trainer_activation)."""
        out = np.zeros((self.batch, self.n * self.n, 256), np.float32)
        check(self.lib.tz_trainer_activation(self.h, layer, out.ctypes.data, out.size))
        return out


def sample_actions(policies, draws):
    """choose_weighted with the randomness handed in (eee/src/ensemble.rs:274-280): for every (move indices, probabilities) pair the first
    action whose cumulative probability passes draw * total, draw in [0, 1).  Returns the move indices, uint16."""
    draws = np.asarray(draws, np.float64)
    assert draws.shape == (len(policies),)
    actions = np.zeros(len(policies), np.uint16)
    for i, (moves, probs) in enumerate(policies):
        cum = np.cumsum(np.asarray(probs, np.float64))
        k = int(np.searchsorted(cum, draws[i] * cum[-1], side="right"))
        actions[i] = np.asarray(moves)[min(k, len(cum) - 1)]
    return actions


def ensemble_targets(net, mcts, states, policies, draws):
    """get_ensemble_targets (eee/src/ensemble.rs:265-316): for every position an action drawn in proportion to its improved policy, one
    step of the game, and -DISCOUNT_FACTOR * the net's sixteen head values there; where the step ended the game all sixteen entries are
    f32::from(Eval::from(terminal).negate()) instead (eval.rs:40-47, 95-105: a game the mover has won is Loss(0) for the side to move,
    negated Win(1) = 0.997; a draw is 0).  `policies[i]` = (move indices, probabilities) of position i; `draws[i]` in [0, 1) picks the
    action (sample_actions; the randomness stays with the caller).  `mcts` is a scratch
    search handle of the same board size: its positions are replaced.  Returns [B, 16] fp32."""
    st = api._states(states)
    B, W = len(st), mcts.batch
    assert len(policies) == B
    actions = sample_actions(policies, draws)
    out = np.zeros((B, api.ENSEMBLE_SIZE), np.float32)
    for lo in range(0, B, W):
        k = min(W, B - lo)
        chunk, act = np.repeat(st[lo:lo + 1], W), np.full(W, 0xFFFF, np.uint16)
        chunk[:k], act[:k] = st[lo:lo + k], actions[lo:lo + k]
        mcts.set_positions(np.arange(W), chunk)
        ok = mcts.play_moves(act)
        if not np.all(ok[:k] == 1):
            raise ValueError("ensemble_targets: the sampled action of position %d is not legal there" % (lo + int(np.argmax(ok[:k] != 1))))
        after = mcts.get_positions()[:k]
        out[lo:lo + k] = -api.DISCOUNT_FACTOR * net.ensemble_values(after)
        ended = mcts.restart_terminal_envs(np.zeros(W, np.int32))[:k] != api.TERMINAL_NONE
        _reason, winner = mcts.terminal_details()
        for i in np.flatnonzero(ended):
            # the terminal as the side to move after the step sees it, negated: one ply further, from the other side
            sign = 0.0 if winner[i] == 2 else (-1.0 if winner[i] == after["to_move"][i] else 1.0)
            out[lo + i] = api.DISCOUNT_FACTOR * np.float32(sign)
    return out


# ---------------------------------------------------------------------------------------------
# learn::main (learn/src/main.rs:99-289): replay buffers with forced uses, back-pressure file, model files
STEPS_PER_SAVE = 100               # :44
STEPS_PER_CHECKPOINT = 50_000      # :45
INITIAL_RANDOM_TARGETS = BATCH_SIZE * 2_000  # :49
PRE_TRAINING_STEPS = 1_000         # :50
STEPS_BEFORE_REANALYZE = 5000      # :54
MIN_SELFPLAY_BUFFER_LEN = 10_000   # :55
MIN_REANALYZE_BUFFER_LEN = 2_000   # :57
SELFPLAY_TARGET_FORCED_USES = 4    # :59
REANALYZE_TARGET_FORCED_USES = 4   # :60


class TargetBuffer:
    """Vec<TargetWithContext> fed from an append-only targets file (fill_buffer_with_targets, :291-319)."""

    def __init__(self, n, half_komi, forced_uses):
        self.n, self.half_komi, self.forced_uses = n, half_komi, forced_uses
        self.items = []   # [target, remaining uses, model steps when read]
        self.seek = 0

    def __len__(self):
        return len(self.items)

    def fill(self, path, model_steps):
        from . import formats

        with open(path, "rb") as f:
            f.seek(self.seek)
            data = f.read()
        targets, consumed, _skipped = formats.parse_targets(data, self.n, self.half_komi)  # bad lines are skipped (:308)
        self.seek += consumed
        self.items.extend([t, self.forced_uses, model_steps] for t in targets)
        return len(targets)

    def take(self, rng, count):
        """`count` targets drawn uniformly without replacement and removed — what shuffling the whole buffer and
        draining its tail does (create_batch, :493-499), in O(count) instead of O(len)."""
        pick = sorted((int(i) for i in rng.choice(len(self.items), size=count, replace=False)), reverse=True)
        batch = []
        for i in pick:              # swap-remove, largest index first so earlier picks stay valid
            batch.append(self.items[i])
            self.items[i] = self.items[-1]
            self.items.pop()
        order = rng.permutation(count)
        return [batch[i] for i in order]

    def give_back(self, batch):
        for item in batch:  # TargetWithContext::reuse
            if item[1] > 1:
                item[1] -= 1
                self.items.append(item)


def model_path_with_most_steps(directory):
    """get_model_path_with_most_steps (:272-289): model_<steps>.ot with the largest number."""
    import os

    best = None
    for name in os.listdir(directory):
        stem, ext = os.path.splitext(name)
        if ext != ".ot" or "_" not in stem:
            continue
        tail = stem.split("_", 1)[1]
        if tail.isdigit() and (best is None or int(tail) > best[0]):
            best = (int(tail), os.path.join(directory, name))
    return best


def create_batch(using_reanalyze, exploitation, reanalyze, rng, n, batch=BATCH_SIZE, augment=True):
    """create_batch + create_input_and_target_tensors (:486-516, :330-374)."""
    if using_reanalyze:
        a, b = exploitation.take(rng, batch // 2), reanalyze.take(rng, batch // 2)
        items = a + b
    else:
        a, b = exploitation.take(rng, batch), []
        items = a
    tensors = target_tensors([it[0] for it in items], n, rng if augment else None)
    exploitation.give_back(a)
    reanalyze.give_back(b)
    return tensors


def pre_training(trainer, mcts, rng_seed, directory=None, initial_targets=INITIAL_RANDOM_TARGETS,
                 steps=PRE_TRAINING_STEPS, log=None):
    """pre_training (:425-484): uniformly random games from the openings, uniform policy targets, discounted game
    result as value, UBE target 4 - eps; the UBE head is not trained.  `mcts`: a BatchedMCTS with the Dummy agent."""
    import os

    from . import formats
    from .selfplay import SelfPlay

    sp = SelfPlay(mcts, 0, seed=rng_seed, search="random")
    rng = np.random.default_rng([rng_seed, 11])
    buffer = []
    while len(buffer) < initial_targets:
        targets, _ = sp.play_move()
        buffer.extend(targets)
    order = rng.permutation(len(buffer))
    buffer = [buffer[i] for i in order]
    if directory is not None:
        with open(os.path.join(directory, "targets-initial.txt"), "w") as f:
            f.write(formats.format_targets(mcts.n, buffer))
    B, losses = trainer.batch, []
    for s in range(min(steps, len(buffer) // B)):
        losses.append(trainer.step(*target_tensors(buffer[s * B:(s + 1) * B], mcts.n, rng), train_ube=False))
        if log and s % 100 == 0:
            log("pre-training step %d: %r" % (s, losses[-1]))
    return losses


def rnd_reference(mcts, seed=0, n_early=256, early_ply=4, n_late=256, late_ply=120):
    """reference_games (learn/src/rnd_normalization.rs:23-58) through tz_learn_rnd_reference: (early, late) state arrays.
    `mcts`: a BatchedMCTS of any agent kind; its positions are overwritten."""
    early, late = np.zeros(n_early, api.STATE_DTYPE), np.zeros(n_late, api.STATE_DTYPE)
    check(_lib.load().tz_learn_rnd_reference(mcts.h, seed, n_early, early_ply, n_late, late_ply, early.ctypes.data, late.ctypes.data))
    return early, late


def save_model(trainer, path, hash_net=None, background=None):
    """Network::save (network/mod.rs:16-18; net6_simhash.rs:152-171 also writes bitvec.bin beside the model).  The
    weights are read back from the GPU here; with `background` (a runner.AsyncAppender) the archive itself is written
    by that thread while training goes on."""
    import os

    from . import ot

    snapshot = trainer.tensors()
    if hash_net is not None:
        hash_net.save_bitset(os.path.join(os.path.dirname(str(path)), "bitvec.bin"))
    if background is None:
        ot.save_ot(path, snapshot)
    else:
        background.submit(lambda: ot.save_ot(path, snapshot))


def run_learn(directory, trainer, half_komi=4, steps=None, seed=0, pre_train_mcts=None, hash_net=None,
              min_selfplay=MIN_SELFPLAY_BUFFER_LEN, min_reanalyze=MIN_REANALYZE_BUFFER_LEN,
              steps_before_reanalyze=STEPS_BEFORE_REANALYZE, steps_per_save=STEPS_PER_SAVE,
              steps_per_checkpoint=STEPS_PER_CHECKPOINT, pre_training_steps=PRE_TRAINING_STEPS,
              initial_targets=INITIAL_RANDOM_TARGETS, restart_targets=None, read_interval=10.0, sleep=30.0,
              max_wait=None, log=None, train_rnd=False, rnd_reference=None, rnd_calibrate_every=0):
    """learn::main (:99-270).  `trainer` must already hold initial weights (Net::new) unless the directory has a
    model_<steps>.ot to resume from.  Returns the number of training steps the model has seen.
    train_rnd: the steps of the main loop also train the RND predictor (net5's MLP or net4_rnd's tower, :404-405); rnd_reference = (early, late) states: update_rnd
    (:415-416) runs before every model file written from then on and every rnd_calibrate_every steps (0: only before files)."""
    import os
    import time

    from . import formats, ot

    from .runner import AsyncAppender

    n, rng = trainer.n, np.random.default_rng([seed, 5])

    def calibrate():
        if train_rnd and rnd_reference is not None:
            trainer._rnd_calls()[1](rnd_reference[0], rnd_reference[1], apply=True)

    saver = AsyncAppender()   # model files are written behind the training loop, in order
    resume = model_path_with_most_steps(directory)
    if resume is not None:
        starting_steps = resume[0]
        trainer.load_tensors(ot.load_ot(resume[1]))
    else:
        starting_steps = 0
        save_model(trainer, os.path.join(directory, "model_0000000.ot"), hash_net)
    if restart_targets is not None:
        # --restart-targets (:126-147): one pass over a saved target file, UBE head not trained
        with open(restart_targets) as f:
            saved = []
            for line in f:
                try:
                    saved.append(formats.parse_target(line, n, half_komi))
                except Exception:
                    continue
        rng.shuffle(saved)
        B = trainer.batch
        for s in range(len(saved) // B):
            trainer.step(*target_tensors(saved[s * B:(s + 1) * B], n, rng), train_ube=False)
            starting_steps += 1
        save_model(trainer, os.path.join(directory, "model_%07d.ot" % starting_steps), hash_net)
    elif resume is None:
        if pre_train_mcts is not None and pre_training_steps > 0:
            pre_training(trainer, pre_train_mcts, seed, directory, initial_targets, pre_training_steps, log)
            starting_steps += pre_training_steps
            save_model(trainer, os.path.join(directory, "model_%07d.ot" % starting_steps), hash_net)
    if train_rnd:
        trainer._rnd_calls()[0](True)
    calibrate()
    save_model(trainer, os.path.join(directory, "model_latest.ot"), hash_net)
    exploitation = TargetBuffer(n, half_komi, SELFPLAY_TARGET_FORCED_USES)
    reanalyze = TargetBuffer(n, half_komi, REANALYZE_TARGET_FORCED_USES)
    last_loaded = -1e18
    model_steps = starting_steps
    done = 0
    t0 = time.monotonic()
    # The step of batch k runs on a worker thread (inside a ctypes call, interpreter lock released) while this thread
    # samples, augments and densifies batch k+1; results are collected in step order, so logs and model files are those
    # of the sequential loop.
    from concurrent.futures import ThreadPoolExecutor

    def finish(step_no, fut, states):
        losses = fut.result()
        if hash_net is not None:
            hash_net.hash_indices(states, update=True)  # net.update_counts(&tensors.input), :418
        if log:
            log("step %d: loss_policy %.5f loss_value %.5f loss_ube %.5f" % ((step_no,) + losses))
        if step_no % steps_per_save == 0 or step_no % steps_per_checkpoint == 0 or (
                rnd_calibrate_every > 0 and step_no % rnd_calibrate_every == 0):
            calibrate()
        if step_no % steps_per_save == 0:
            save_model(trainer, os.path.join(directory, "model_latest.ot"), hash_net, saver)
        if step_no % steps_per_checkpoint == 0:
            save_model(trainer, os.path.join(directory, "model_%07d.ot" % step_no), hash_net, saver)

    pending = None
    with ThreadPoolExecutor(1) as pool:
        try:
            while steps is None or done < steps:
                model_steps += 1
                using_reanalyze = restart_targets is not None or model_steps >= steps_before_reanalyze
                while True:
                    if time.monotonic() - last_loaded >= read_interval:
                        for buf, name, use in ((exploitation, "targets-selfplay.txt", True),
                                               (reanalyze, "targets-reanalyze.txt", using_reanalyze)):
                            if use:
                                try:
                                    buf.fill(os.path.join(directory, name), model_steps)
                                except OSError as err:
                                    if log:
                                        log("Cannot read %s: %s" % (name, err))
                        last_loaded = time.monotonic()
                        with open(os.path.join(directory, "buffer_lengths.txt"), "w") as f:
                            f.write(formats.format_buffer_lengths(len(exploitation), len(reanalyze)))
                    if len(exploitation) >= min_selfplay and (not using_reanalyze or len(reanalyze) >= min_reanalyze):
                        break
                    if max_wait is not None and time.monotonic() - t0 > max_wait:
                        raise TimeoutError("not enough targets (%d selfplay, %d reanalyze)" % (len(exploitation), len(reanalyze)))
                    time.sleep(sleep)
                tensors = create_batch(using_reanalyze, exploitation, reanalyze, rng, n, trainer.batch)
                if pending is not None:
                    finish(*pending)
                pending = (model_steps, pool.submit(trainer.step, *tensors, train_ube=True), tensors[0])
                time.sleep(0.0005)   # hand the interpreter lock over so the worker enters its (lock-free) native call now
                done += 1
        finally:
            try:
                if pending is not None:
                    finish(*pending)
            finally:
                saver.close()
    return model_steps


# ---------------------------------------------------------------------------------------------
class NativeLearnLoop:
    """learn::main's buffers, batch construction and training loop in native code (csrc/tz_host_learn.cpp, tz_learn_*)."""

    def __init__(self, trainer, half_komi=4, seed=0, forced_uses=(SELFPLAY_TARGET_FORCED_USES, REANALYZE_TARGET_FORCED_USES)):
        self.trainer, self.lib = trainer, _lib.load()
        self.h = C.c_void_p()
        check(self.lib.tz_learn_create(trainer.h, half_komi, seed, forced_uses[0], forced_uses[1], C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None):
            self.lib.tz_learn_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def feed(self, which, path, model_steps=0):
        added = C.c_uint64()
        check(self.lib.tz_learn_feed(self.h, which, str(path).encode(), model_steps, C.byref(added)))
        return added.value

    def add_lines(self, which, text, model_steps=0):
        data = text if isinstance(text, bytes) else text.encode()
        added = C.c_uint64()
        check(self.lib.tz_learn_add_lines(self.h, which, data, len(data), model_steps, C.byref(added)))
        return added.value

    def buffer_len(self, which):
        n = C.c_uint64()
        check(self.lib.tz_learn_buffer_len(self.h, which, C.byref(n)))
        return n.value

    def step(self, using_reanalyze=False, train_ube=True, augment=True):
        losses = np.zeros(3, np.float32)
        check(self.lib.tz_learn_step(self.h, 1 if using_reanalyze else 0, 1 if train_ube else 0, 1 if augment else 0, losses.ctypes.data))
        return tuple(float(x) for x in losses)

    def set_rnd(self, train_rnd=True, early=None, late=None, calibrate_every=0):
        """tz_learn_set_rnd: every step of the loop trains the RND predictor; with reference positions, run() calibrates min / max
        before every model file it writes itself and every `calibrate_every` steps."""
        e = api._states(early) if early is not None else np.zeros(0, api.STATE_DTYPE)
        l = api._states(late) if late is not None else np.zeros(0, api.STATE_DTYPE)
        check(self.lib.tz_learn_set_rnd(self.h, 1 if train_rnd else 0, e.ctypes.data if len(e) else None, len(e),
                                        l.ctypes.data if len(l) else None, len(l), calibrate_every))
        return self

    def last_batch(self):
        B, out = self.trainer.batch, api.policy_size(self.trainer.n)
        states = np.zeros(B, api.STATE_DTYPE)
        policy, mask = np.zeros((B, out), np.float32), np.zeros((B, out), np.uint8)
        value, ube = np.zeros(B, np.float32), np.zeros(B, np.float32)
        check(self.lib.tz_learn_last_batch(self.h, states.ctypes.data, policy.ctypes.data, mask.ctypes.data, value.ctypes.data,
                                           ube.ctypes.data))
        return states, policy, mask, value, ube

    def run(self, directory, starting_steps, steps, min_selfplay=MIN_SELFPLAY_BUFFER_LEN, min_reanalyze=MIN_REANALYZE_BUFFER_LEN,
            steps_before_reanalyze=STEPS_BEFORE_REANALYZE, read_interval=10.0, sleep=30.0, max_wait=None, on_step=None):
        """tz_learn_run; on_step(model_steps, losses, states) is called after every step."""
        cb_type = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_float), C.c_void_p, C.c_int)
        failure = []

        def trampoline(_user, step_no, losses, states, batch):
            try:
                if on_step is not None:
                    st = np.frombuffer((C.c_char * (batch * api.STATE_DTYPE.itemsize)).from_address(states), dtype=api.STATE_DTYPE)
                    on_step(int(step_no), (losses[0], losses[1], losses[2]), st)
                return 0
            except BaseException as e:   # surfaces after the native loop returns
                failure.append(e)
                return 1

        cb = cb_type(trampoline)
        out = C.c_int64()
        rc = self.lib.tz_learn_run(self.h, str(directory).encode(), starting_steps, -1 if steps is None else steps, min_selfplay,
                                   min_reanalyze, steps_before_reanalyze, read_interval, sleep, -1.0 if max_wait is None else max_wait,
                                   C.cast(cb, C.c_void_p), None, C.byref(out))
        if failure:
            raise failure[0]
        if rc == -6 and "not enough targets" in self.lib.tz_last_error().decode(errors="replace"):
            raise TimeoutError(self.lib.tz_last_error().decode(errors="replace"))
        check(rc)
        return out.value


def run_learn_native(directory, trainer, half_komi=4, steps=None, seed=0, pre_train_mcts=None, hash_net=None,
                     min_selfplay=MIN_SELFPLAY_BUFFER_LEN, min_reanalyze=MIN_REANALYZE_BUFFER_LEN,
                     steps_before_reanalyze=STEPS_BEFORE_REANALYZE, steps_per_save=STEPS_PER_SAVE,
                     steps_per_checkpoint=STEPS_PER_CHECKPOINT, pre_training_steps=PRE_TRAINING_STEPS,
                     initial_targets=INITIAL_RANDOM_TARGETS, read_interval=10.0, sleep=30.0, max_wait=None, log=None,
                     train_rnd=False, rnd_reference=None, rnd_calibrate_every=0):
    """learn::main (learn/src/main.rs:99-270) with the buffers, batch construction and loop in native code; this function
    keeps what touches files in the reference's formats through host tools: model discovery / resume and the save
    points (LibTorch archives).
    train_rnd: the steps of the main loop also train the RND predictor (net5's MLP or net4_rnd's tower, :404-405); rnd_reference = (early, late) states
    (rnd_reference() makes them): update_rnd (:415-416) runs before every model file written from then on and every
    rnd_calibrate_every steps (0: only before files)."""
    import os

    from . import ot
    from .runner import AsyncAppender
    from .selfplay import NativeSelfPlay

    saver = AsyncAppender()
    try:
        resume = model_path_with_most_steps(directory)
        if resume is not None:
            starting_steps = resume[0]
            trainer.load_tensors(ot.load_ot(resume[1]))
        else:
            starting_steps = 0
            save_model(trainer, os.path.join(directory, "model_0000000.ot"), hash_net)
            if pre_train_mcts is not None and pre_training_steps > 0:   # pre_training (:425-484)
                sp = NativeSelfPlay(pre_train_mcts, 0, seed=seed, search="random")
                lines = []
                while len(lines) < initial_targets:
                    sp.play_move()
                    lines.extend(sp.take_text(0).splitlines(keepends=True))
                np.random.default_rng([seed, 11]).shuffle(lines)
                with open(os.path.join(directory, "targets-initial.txt"), "wb") as f:
                    f.write(b"".join(lines))
                pre = NativeLearnLoop(trainer, half_komi, seed + 1, forced_uses=(1, 1))   # every target used once
                pre.add_lines(0, b"".join(lines))
                for s in range(min(pre_training_steps, len(lines) // trainer.batch)):
                    losses = pre.step(using_reanalyze=False, train_ube=False, augment=True)
                    if log and s % 100 == 0:
                        log("pre-training step %d: %r" % (s, losses))
                pre.close()
                starting_steps += pre_training_steps
                save_model(trainer, os.path.join(directory, "model_%07d.ot" % starting_steps), hash_net)
        loop = NativeLearnLoop(trainer, half_komi, seed)
        have_reference = train_rnd and rnd_reference is not None
        if train_rnd:
            # the native loop calibrates on the multiples of rnd_calibrate_every; the files are written here, so is their calibration
            loop.set_rnd(True, rnd_reference[0] if have_reference else None, rnd_reference[1] if have_reference else None,
                         rnd_calibrate_every)
        if have_reference:
            trainer._rnd_calls()[1](rnd_reference[0], rnd_reference[1], apply=True)
        save_model(trainer, os.path.join(directory, "model_latest.ot"), hash_net)

        def on_step(step_no, losses, states):
            if hash_net is not None:
                hash_net.hash_indices(states, update=True)
            if log:
                log("step %d: loss_policy %.5f loss_value %.5f loss_ube %.5f" % ((step_no,) + tuple(losses)))
            if have_reference and (step_no % steps_per_save == 0 or step_no % steps_per_checkpoint == 0):
                trainer._rnd_calls()[1](rnd_reference[0], rnd_reference[1], apply=True)
            if step_no % steps_per_save == 0:
                save_model(trainer, os.path.join(directory, "model_latest.ot"), hash_net, saver)
            if step_no % steps_per_checkpoint == 0:
                save_model(trainer, os.path.join(directory, "model_%07d.ot" % step_no), hash_net, saver)

        return loop.run(directory, starting_steps, steps, min_selfplay, min_reanalyze, steps_before_reanalyze, read_interval, sleep,
                        max_wait, on_step)
    finally:
        saver.close()
