"""optax-shaped optimisers over a whole parameter set in one launch (csrc/optim.hip).  The names are re-exported
by `eqxvision_amd.grad`, so they are `eqv.optim.sgd`, `eqv.optim.adamw`, `eqv.optim.clip_by_global_norm`, `eqv.optim.chain`, `eqv.optim.ema` and the
schedules `eqv.optim.constant_schedule` / `cosine_decay_schedule` / `warmup_cosine_decay_schedule`.

    optimizer = eqv.optim.chain(eqv.optim.clip_by_global_norm(1.0), eqv.optim.adamw(eqv.optim.cosine_decay_schedule(1e-3, 1000)))
    opt_state = optimizer.init(eqv.filter(net, eqv.is_array))
    updates, opt_state = optimizer.update(grads, opt_state, net)
    net = eqv.apply_updates(net, updates)

One `mv_optim_tensor` record per float leaf, all records in one device buffer (`launch`); the buffer is rebuilt only when a
pointer of the set changes.  A gradient that is `None` (a leaf frozen by filter_value_and_grad's `arg`) is skipped: no record, `None`
in the updates, its moments untouched.  A schedule is a host function of the integer step count, evaluated in float64 at the count
BEFORE the increment (the first update uses schedule(0), as in optax); the rate reaches the kernel as a launch argument.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib
from . import grad as _g                 # _float_leaf / _upload / _Adam (grad.py imports this module at its end)
from ._act import device, stream_ptr
from ._module import DevArray, tree_leaves, tree_map

CHUNK = _lib.OPTIM_CHUNK


# ------------------------------------------------------------------------------------------------------------ schedules
def constant_schedule(value):
    value = float(value)
    return lambda count: value


def cosine_decay_schedule(init_value, decay_steps, alpha=0.0):
    """optax.cosine_decay_schedule: init_value ((1 - alpha) (1 + cos(pi min(count, decay_steps) / decay_steps)) / 2 + alpha)."""
    if not decay_steps > 0:
        raise ValueError(f"cosine_decay_schedule: decay_steps = {decay_steps} must be positive")
    init_value, alpha = float(init_value), float(alpha)

    def schedule(count):
        c = min(max(int(count), 0), decay_steps)
        cosine = 0.5 * (1.0 + math.cos(math.pi * c / decay_steps))
        return init_value * ((1.0 - alpha) * cosine + alpha)
    return schedule


def warmup_cosine_decay_schedule(init_value, peak_value, warmup_steps, decay_steps, end_value=0.0):
    """optax.warmup_cosine_decay_schedule: linear from init_value to peak_value over warmup_steps, then a cosine from peak_value to
    end_value that ends at decay_steps (which counts the warm-up in)."""
    init_value, peak_value, end_value = float(init_value), float(peak_value), float(end_value)
    warmup_steps = int(warmup_steps)
    cosine = cosine_decay_schedule(peak_value, decay_steps - warmup_steps, 0.0 if peak_value == 0.0 else end_value / peak_value)

    def schedule(count):
        count = max(int(count), 0)
        if count < warmup_steps:
            return init_value + (peak_value - init_value) * (count / warmup_steps)
        return cosine(count - warmup_steps)
    return schedule


def rate(learning_rate, count: int) -> float:
    """The rate of the update that follows `count` finished ones."""
    return float(learning_rate(count)) if callable(learning_rate) else float(learning_rate)


# ------------------------------------------------------------------------------------------------------------ records
def plan(sizes):
    """(first_block of every tensor, total_blocks): a tensor of n elements takes ceil(n / CHUNK) workgroups, in order."""
    first, total = [], 0
    for n in sizes:
        if n <= 0:
            raise ValueError(f"optimiser records: a tensor of {n} elements")
        first.append(total)
        total += -(-int(n) // CHUNK)
    return first, total


def records(cache: dict, rows):
    """The device buffer of mv_optim_tensor records for `rows` = [(grad, param, m, v, out, n)] (addresses, 0 = NULL).  `cache`
    keeps the last buffer and hands it out again while the rows repeat."""
    key = tuple(rows)
    if cache.get("key") != key:
        first, total = plan([r[5] for r in rows])
        a = np.empty((len(rows), 7), np.int64)
        a[:, :6] = np.asarray(rows, np.int64)
        a[:, 6] = first
        cache.update(key=key, recs=torch.from_numpy(a).to(device()), total=total)
    return cache["recs"], len(rows), cache["total"]


def sqnorm(cache: dict, rows, max_norm: float) -> torch.Tensor:
    """[sum of squares of every gradient of the set, clip_by_global_norm's factor] on the device (mv_optim_sqnorm_f32)."""
    recs, n, total = records(cache, rows)
    part = cache.get("partial")
    if part is None or part.numel() < total:
        part = cache["partial"] = torch.empty(total, dtype=torch.float32, device=device())
    out2 = torch.empty(2, dtype=torch.float32, device=device())
    _lib.call("mv_optim_sqnorm_f32", recs.data_ptr(), n, total, part.data_ptr(), out2.data_ptr(), float(max_norm), stream_ptr())
    return out2


def launch(cache: dict, rows, kind: int, nesterov: bool = False, lr: float = 0.0, b1: float = 0.0, b2: float = 0.0, eps: float = 0.0,
           weight_decay: float = 0.0, bc1: float = 1.0, bc2: float = 1.0, scale=None):
    """One mv_optim_step_f32 over `rows`.  1 - b1 and 1 - b2 are taken in float64 here and rounded once."""
    recs, n, total = records(cache, rows)
    _lib.call("mv_optim_step_f32", recs.data_ptr(), n, total, int(kind), int(bool(nesterov)), float(lr), float(b1), float(b2),
              1.0 - float(b1), 1.0 - float(b2), float(eps), float(weight_decay), float(bc1), float(bc2),
              None if scale is None else scale.data_ptr(), stream_ptr())


def leaf_index(params):
    """(index, sizes): for every position of the tree (tree_leaves with None kept) the number of its float leaf, -1 elsewhere; and
    the element count of every float leaf.  A gradient tree has None at its frozen leaves, so positions, not leaf counts, pair it
    with the state."""
    index, sizes = [], []
    for leaf in tree_leaves(params, none_is_leaf=True):
        if _g._float_leaf(leaf):
            index.append(len(sizes))
            sizes.append(int(np.prod(leaf.shape)))
        else:
            index.append(-1)
    return index, sizes


def _zeros(n):
    return torch.zeros(n, dtype=torch.float32, device=device())


class _Set:
    """The float leaves of one gradient tree, paired with the state's slots (and the parameters): rows for `launch`, and the
    updates tree once the launch is enqueued."""

    def __init__(self, who, grads, index, params=None, mu=None, nu=None):
        gl = tree_leaves(grads, none_is_leaf=True)
        if len(gl) != len(index):
            raise ValueError(f"{who}.update: the gradients do not have the structure of the tree given to init")
        pl = None
        if params is not None:
            pl = tree_leaves(params, none_is_leaf=True)
            if len(pl) != len(gl):
                raise ValueError(f"{who}.update: `params` does not have the structure of the gradients")
        self.grads, self.rows, self.outs, self.keep = grads, [], [], []
        for k, g in enumerate(gl):
            if not _g._float_leaf(g):
                continue
            i = index[k]
            if i < 0:
                raise ValueError(f"{who}.update: the gradients do not have the structure of the tree given to init")
            gd = _g._upload(g).contiguous()
            n = gd.numel()
            if mu is not None and mu[i].numel() != n:
                raise ValueError(f"{who}.update: a gradient of {n} elements for a leaf of {mu[i].numel()}")
            out = torch.empty(n, dtype=torch.float32, device=device())
            self.outs.append(out.reshape(tuple(g.shape)))
            if n == 0:
                continue
            p = 0
            if pl is not None:
                if not _g._float_leaf(pl[k]) or int(np.prod(pl[k].shape)) != n:
                    raise ValueError(f"{who}.update: `params` does not have the structure of the gradients")
                pd = _g._upload(pl[k]).contiguous()
                self.keep.append(pd)
                p = pd.data_ptr()
            self.keep.append(gd)
            self.rows.append((gd.data_ptr(), p, 0 if mu is None else mu[i].data_ptr(), 0 if nu is None else nu[i].data_ptr(),
                              out.data_ptr(), n))

    def updates(self):
        it = iter(self.outs)
        return tree_map(lambda leaf: DevArray(next(it)) if _g._float_leaf(leaf) else leaf, self.grads, none_is_leaf=True)


# ------------------------------------------------------------------------------------------------------------ the rules
class _Sgd:
    """optax.sgd(learning_rate, momentum, nesterov): -lr g, or optax.trace's m = g + momentum m with -lr m (-lr (g + momentum m) with
    nesterov).  One launch per update."""
    name = "sgd"

    def __init__(self, learning_rate, momentum=None, nesterov: bool = False):
        self.lr = learning_rate if callable(learning_rate) else float(learning_rate)
        self.momentum = None if momentum is None else float(momentum)
        self.nesterov = bool(nesterov) and momentum is not None
        self._records = {}

    def init(self, params):
        index, sizes = leaf_index(params)
        return {"count": 0, "index": index, "mu": None if self.momentum is None else [_zeros(n) for n in sizes]}

    def update(self, grads, state, params=None, _max_norm=None):
        s = _Set(self.name, grads, state["index"], mu=state["mu"])
        if s.rows:
            scale = None if _max_norm is None else sqnorm(self._records, s.rows, _max_norm)
            launch(self._records, s.rows, _lib.OPT_SGD, nesterov=self.nesterov, lr=rate(self.lr, state["count"]),
                   b1=self.momentum or 0.0, scale=scale)
        return s.updates(), {"count": state["count"] + 1, "index": state["index"], "mu": state["mu"]}


class _AdamW:
    """optax.adamw(learning_rate, b1, b2, eps, weight_decay): Adam's direction plus weight_decay * param, times -lr (the decay is
    decoupled: it does not pass through the moments).  One launch per update; `update` needs `params`."""
    name = "adamw"

    def __init__(self, learning_rate, b1: float = 0.9, b2: float = 0.999, eps: float = 1e-8, weight_decay: float = 1e-4):
        self.lr = learning_rate if callable(learning_rate) else float(learning_rate)
        self.b1, self.b2, self.eps, self.wd = float(b1), float(b2), float(eps), float(weight_decay)
        self._records = {}

    def init(self, params):
        index, sizes = leaf_index(params)
        return {"count": 0, "index": index, "mu": [_zeros(n) for n in sizes], "nu": [_zeros(n) for n in sizes]}

    def update(self, grads, state, params=None, _max_norm=None):
        if params is None:
            raise ValueError("adamw.update needs `params` (the weight decay reads them): update(grads, state, params)")
        count = state["count"] + 1
        s = _Set(self.name, grads, state["index"], params=params, mu=state["mu"], nu=state["nu"])
        if s.rows:
            scale = None if _max_norm is None else sqnorm(self._records, s.rows, _max_norm)
            launch(self._records, s.rows, _lib.OPT_ADAMW, lr=rate(self.lr, state["count"]), b1=self.b1, b2=self.b2, eps=self.eps,
                   weight_decay=self.wd, bc1=1.0 - self.b1 ** count, bc2=1.0 - self.b2 ** count, scale=scale)
        return s.updates(), {"count": count, "index": state["index"], "mu": state["mu"], "nu": state["nu"]}


class _Clip:
    """optax.clip_by_global_norm(max_norm): only inside `chain`."""

    def __init__(self, max_norm):
        self.max_norm = float(max_norm)
        if not self.max_norm > 0.0:
            raise ValueError(f"clip_by_global_norm: max_norm = {max_norm} must be positive")


_SUPPORTED = "chain([clip_by_global_norm(max_norm),] sgd(...) | adamw(...) | adam(...))"


class _Chain:
    """Zero or one clip in front of one optimiser.  The clip costs the two launches of the squared norm; sgd and adamw then read
    the factor from the device inside their own launch, adam gets its gradients scaled by one more (MV_OPT_SGD with lr = -1 is
    g * factor) and runs as it does alone.  Nothing is synchronised."""

    def __init__(self, clip, opt):
        self.clip, self.opt = clip, opt
        self._records = {}

    def init(self, params):
        return self.opt.init(params)

    def update(self, grads, state, params=None):
        if self.clip is None:
            return self.opt.update(grads, state, params)
        if not isinstance(self.opt, _g._Adam):
            return self.opt.update(grads, state, params, _max_norm=self.clip.max_norm)
        s = _Set("chain", grads, state["index"])
        if s.rows:
            launch(self._records, s.rows, _lib.OPT_SGD, lr=-1.0, scale=sqnorm(self._records, s.rows, self.clip.max_norm))
        return self.opt.update(s.updates(), state, params)


class _Ema:
    """torchvision's `ExponentialMovingAverage(model, decay)` (the `--model-ema` of its reference training script) over the whole
    parameter set: e = decay e + (1 - decay) p as fadd(fmul(decay, e), fmul(1 - decay, p)), 1 - decay taken in float64 and
    rounded once.  `init(params)` copies the float leaves to device slots; `update(params, state)` is ONE launch
    (mv_optim_step_f32, MV_OPT_EMA) that overwrites the slots, and the first one after `init` copies the parameters, as
    torch's AveragedModel does; `state_params(state, like)` is the tree `like` with the averages as `DevArray` leaves.  A leaf that
    is `None` (frozen) or not a float array has no slot and is passed through."""
    name = "ema"

    def __init__(self, decay):
        self.decay = float(decay)
        if not 0.0 <= self.decay <= 1.0:
            raise ValueError(f"ema: decay = {decay} must lie in [0, 1]")
        self._records = {}

    def init(self, params):
        index, _ = leaf_index(params)
        slots = [_g._upload(leaf).reshape(-1).clone() for leaf in tree_leaves(params, none_is_leaf=True) if _g._float_leaf(leaf)]
        return {"count": 0, "index": index, "ema": slots}

    def update(self, params, state):
        index, slots = state["index"], state["ema"]
        pl = tree_leaves(params, none_is_leaf=True)
        if len(pl) != len(index):
            raise ValueError("ema.update: `params` does not have the structure of the tree given to init")
        rows, keep = [], []
        for k, leaf in enumerate(pl):
            if not _g._float_leaf(leaf):
                continue
            i = index[k]
            if i < 0:
                raise ValueError("ema.update: `params` does not have the structure of the tree given to init")
            pd = _g._upload(leaf).contiguous()
            if pd.numel() != slots[i].numel():
                raise ValueError(f"ema.update: a parameter of {pd.numel()} elements for a leaf of {slots[i].numel()}")
            if pd.numel():
                keep.append(pd)
                rows.append((pd.data_ptr(), 0, 0, 0, slots[i].data_ptr(), pd.numel()))
        if rows:
            launch(self._records, rows, _lib.OPT_EMA, nesterov=state["count"] == 0, b1=self.decay)
        return {"count": state["count"] + 1, "index": index, "ema": slots}

    def state_params(self, state, like):
        index, slots = state["index"], state["ema"]
        pos = iter(index)

        def leaf(x):
            i = next(pos, None)
            if not _g._float_leaf(x):
                return x
            if i is None or i < 0 or slots[i].numel() != int(np.prod(x.shape)):
                raise ValueError("ema.state_params: `like` does not have the structure of the tree given to init")
            return DevArray(slots[i].reshape(tuple(x.shape)))
        return tree_map(leaf, like, none_is_leaf=True)


def ema(decay) -> _Ema:
    return _Ema(decay)


def sgd(learning_rate, momentum=None, nesterov: bool = False) -> _Sgd:
    return _Sgd(learning_rate, momentum, nesterov)


def adamw(learning_rate, b1: float = 0.9, b2: float = 0.999, eps: float = 1e-8, weight_decay: float = 1e-4) -> _AdamW:
    return _AdamW(learning_rate, b1, b2, eps, weight_decay)


def clip_by_global_norm(max_norm) -> _Clip:
    return _Clip(max_norm)


def chain(*transforms) -> _Chain:
    ok = 1 <= len(transforms) <= 2 and isinstance(transforms[-1], (_Sgd, _AdamW, _g._Adam)) \
        and (len(transforms) == 1 or isinstance(transforms[0], _Clip))
    if not ok:
        raise ValueError(f"chain({', '.join(type(t).__name__.lstrip('_').lower() for t in transforms)}) is not supported: {_SUPPORTED}")
    return _Chain(transforms[0] if len(transforms) == 2 else None, transforms[-1])
