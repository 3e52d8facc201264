"""Instruments for the one-launch optimisers (csrc/optim.hip, eqxvision_amd/_optim.py); used by test_optim_host.py and
test_optim_gpu.py.

Reference.  float64 `torch.optim.SGD` (dampening 0, with and without nesterov) and `torch.optim.AdamW`: the update rules of
optax.sgd / optax.adamw (optax.trace is m = g + mu m; adamw adds weight_decay * param to Adam's direction before the -lr; torch
writes the same step as p *= 1 - lr wd; p -= lr mhat / (sqrt(vhat) + eps)), as `adam_reference` in tests/_rule_grad.py argues for
Adam.  `clip64` and the schedules are written out in float64 numpy.

Bound.  Every element of every update and of every parameter after `apply_updates` must lie within
`ops_bound(ref, mag, n_ops, "fp32")` (tests/_strict.py) of the reference: n_ops roundings of 2^-23 relative to `mag` (the same
expression on absolute values, so cancellation does not shrink it) plus the store's half ulp.  n_ops is counted from the kernel
source (optim_step_kernel / opt_rule), every fp32 operation and every hyper-parameter rounded from float64 as 1, a division or a
sqrtf as 3, a quantity under a square root passing on half its count:

    g' = g * scale[1]                          n_g = 0 without a clip, else N_CLIP + 1 (below)
  sgd, step s = 1, 2, ...
    m_s = g' + mu m_(s-1)                      n_m(s) = max(n_g, n_m(s-1) + 2) + 1 <= n_g + 3 s           (mu, product, sum)
    out = -lr m_s | -lr (g' + mu m_s) | -lr g' n_u(s) = n_m(s) + 3 + 2 = n_g + 3 s + 5                    (nesterov: mu, product, sum; lr, product)
  adamw
    m_s = b1 m_(s-1) + omb1 g'                 n_m(s) = max(n_m(s-1), n_g) + 3 = n_g + 3 s
    v_s = b2 v_(s-1) + omb2 g' g'              n_v(s) = max(n_v(s-1) + 2, 2 n_g + 3) + 1 = 2 n_g + 3 s + 1
    den = sqrtf(v_s / bc2) + eps               n_den = ceil((n_v + 4) / 2) + 3 + 2
    dir = (m_s / bc1) / den + wd p             n_dir = max(n_m + 4 + n_den + 3, 3) + 1
    out = -lr dir                              n_u(s) = n_dir + 2 = n_g + 3 s + ceil((2 n_g + 3 s + 5) / 2) + 15
  parameter after s steps: p_0 + u_1 + ... + u_s, mag = |p_0| + the updates' mags, n_ops = n_u(s) + s + 1 (s sums, and the
  parameter's own error read back by the weight decay).
  squared norm: an element passes through 16 fused multiply-adds of its lane, 6 butterfly steps, 3 sums over the waves, then
  ceil(blocks / 256) + 6 + 3 sums of the second launch: n_ops = that chain + 1.  The factor max_norm / sqrtf(sum) then carries
  N_CLIP = ceil(n_sq / 2) + 3 + 3 + 1.

Emulation.  `emulate` runs the kernels' contract in fp32 numpy in the kernels' order (lane t of a chunk owns elements 1024 j + 4 t
+ k; the reductions as block_sum_ordered) and takes ONE defect switch (DEFECTS); test_optim_host.py shows that the bound passes the
emulation and sees every defect.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from tests import _strict as ST

F32, F64 = np.float32, np.float64
CHUNK = 4096
DEFECTS = ("nesterov_ignored", "wd_coupled", "count_minus_1", "clip_inverted", "schedule_at_count", "tail_dropped")

# the tensor set: tail (n % 4), chunk boundary, a multi-block tensor, a 4-D leaf, 300 records for the search, one unaligned view
SIZES = [(1,), (3,), (4,), (5,), (4095,), (4096,), (4097,), (8193,), (7, 3, 3, 3)] + [(1,)] * 300 + [(1030,)]
UNALIGNED = len(SIZES) - 1               # this tensor is handed over as a view 4 bytes into its allocation
STEPS = 3
MAX_NORM = 1.0                           # the set's gradient norm is ~ 148: the clip is active
B1, B2, EPS = 0.9, 0.999, 1e-8

# rule cases: name -> (kind, hyper-parameters).  Every case runs at cosine_decay_schedule(0.05, 5): three different rates.
LR_INIT, LR_STEPS = 0.05, 5
RULES = {"sgd": ("sgd", {"momentum": None, "nesterov": False}),
         "sgd_momentum": ("sgd", {"momentum": 0.9, "nesterov": False}),
         "sgd_nesterov": ("sgd", {"momentum": 0.9, "nesterov": True}),
         "adamw_wd0": ("adamw", {"weight_decay": 0.0}),
         "adamw_wd05": ("adamw", {"weight_decay": 0.05})}


def n_blocks(sizes=SIZES):
    return [-(-int(np.prod(s)) // CHUNK) for s in sizes]


def tensor_set(seed=0):
    """(params, [gradients of step 1..STEPS]): fp32 Gaussians of SIZES."""
    rng = ST.rng_of(seed)
    draw = lambda: [rng.standard_normal(s).astype(F32) for s in SIZES]
    return draw(), [draw() for _ in range(STEPS)]


# ------------------------------------------------------------------------------------------------ schedules, clip (float64)
def cosine64(count, init_value, decay_steps, alpha=0.0):
    c = np.minimum(np.asarray(count, F64), decay_steps)
    return init_value * ((1.0 - alpha) * 0.5 * (1.0 + np.cos(np.pi * c / decay_steps)) + alpha)


def warmup_cosine64(count, init_value, peak_value, warmup_steps, decay_steps, end_value=0.0):
    count = np.asarray(count, F64)
    warm = init_value + (peak_value - init_value) * count / max(warmup_steps, 1)
    return np.where(count < warmup_steps, warm, cosine64(count - warmup_steps, peak_value, decay_steps - warmup_steps, end_value / peak_value))


def rates(steps=STEPS, defect=None):
    """The rate of update s = 1..steps: the schedule at the count BEFORE the increment."""
    off = 1 if defect == "schedule_at_count" else 0
    return [float(cosine64(s + off, LR_INIT, LR_STEPS)) for s in range(steps)]


def sqnorm64(grads):
    return float(sum((np.asarray(g, F64) ** 2).sum() for g in grads))


def scale64(grads, max_norm):
    norm = math.sqrt(sqnorm64(grads))
    return 1.0 if norm < max_norm else max_norm / norm


# ------------------------------------------------------------------------------------------------ n_ops (derivation: module docstring)
def n_sqnorm(total_blocks):
    return 16 + 6 + 3 + -(-total_blocks // 256) + 6 + 3 + 1


def n_grad(clip, total_blocks):
    return 0 if not clip else -(-n_sqnorm(total_blocks) // 2) + 3 + 3 + 1 + 1


def n_update(kind, s, n_g):
    if kind == "sgd":
        return n_g + 3 * s + 5
    return n_g + 3 * s + -(-(2 * n_g + 3 * s + 5) // 2) + 15


def n_param(kind, s, n_g):
    return n_update(kind, s, n_g) + s + 1


# ------------------------------------------------------------------------------------------------ float64 reference + mags
def reference(rule, params, grad_steps, max_norm=None, lrs=None):
    """torch.optim in float64, fed the (clipped) gradients -> per step {"updates", "params", "mag_u", "mag_p"} (lists over leaves)."""
    kind, hp = RULES[rule]
    lrs = lrs or rates(len(grad_steps))
    ps = [torch.from_numpy(np.asarray(p, F64).copy()).requires_grad_(True) for p in params]
    if kind == "sgd":
        opt = torch.optim.SGD(ps, lr=lrs[0], momentum=hp["momentum"] or 0.0, dampening=0.0, nesterov=hp["nesterov"])
    else:
        opt = torch.optim.AdamW(ps, lr=lrs[0], betas=(B1, B2), eps=EPS, weight_decay=hp["weight_decay"], amsgrad=False)
    mu = hp.get("momentum") or 0.0
    mag_m = [np.zeros(p.shape, F64) for p in params]
    v = [np.zeros(p.shape, F64) for p in params]
    mag_p = [np.abs(np.asarray(p, F64)) for p in params]
    out = []
    for s, (grads, lr) in enumerate(zip(grad_steps, lrs), 1):
        sc = 1.0 if max_norm is None else scale64(grads, max_norm)
        gs = [np.asarray(g, F64) * sc for g in grads]
        before = [p.detach().numpy().copy() for p in ps]
        for p, g in zip(ps, gs):
            p.grad = torch.from_numpy(g.copy())
        for grp in opt.param_groups:
            grp["lr"] = lr
        opt.step()
        after = [p.detach().numpy().copy() for p in ps]
        mag_u = []
        for i, g in enumerate(gs):
            a = np.abs(g)
            if kind == "sgd":
                if hp["momentum"] is None:
                    mu_i = lr * a
                else:
                    mag_m[i] = a + mu * mag_m[i]
                    mu_i = lr * (a + mu * mag_m[i]) if hp["nesterov"] else lr * mag_m[i]
            else:
                mag_m[i] = B1 * mag_m[i] + (1 - B1) * a
                v[i] = B2 * v[i] + (1 - B2) * g * g
                den = np.sqrt(v[i] / (1 - B2 ** s)) + EPS
                mu_i = lr * (mag_m[i] / (1 - B1 ** s) / den + hp["weight_decay"] * np.abs(before[i]))
            mag_u.append(mu_i)
        mag_p = [m + u for m, u in zip(mag_p, mag_u)]
        out.append({"updates": [a - b for a, b in zip(after, before)], "params": after, "mag_u": mag_u, "mag_p": list(mag_p)})
    return out


def check_run(rule, clip, got_updates, got_params, ref, total_blocks=None):
    """Worst err / bound over every element of every update and parameter of every step -> (ok, worst ratio, what failed)."""
    kind = RULES[rule][0]
    n_g = n_grad(clip, total_blocks if total_blocks is not None else sum(n_blocks()))
    worst, failed = 0.0, []
    for s, (gu, gp, r) in enumerate(zip(got_updates, got_params, ref), 1):
        for what, got, want, mag, n in (("update", gu, r["updates"], r["mag_u"], n_update(kind, s, n_g)),
                                        ("param", gp, r["params"], r["mag_p"], n_param(kind, s, n_g))):
            for i, (a, b, m) in enumerate(zip(got, want, mag)):
                info = ST.check_bound(np.asarray(a, F64).reshape(b.shape), b, m, None, "fp32", n_ops=n)
                if not info["ok"]:
                    failed.append((s, what, i, info.get("worst", info.get("err"))))
                worst = max(worst, info.get("worst", np.inf))
    return not failed, worst, failed[:5]


# ------------------------------------------------------------------------------------------------ fp32 emulation of the kernels
def _chunks(g, drop_tail):
    """A tensor as its workgroups see it: [blocks, trips j = 4, lanes t = 256, k = 4], zero where no element exists."""
    g = np.asarray(g, F32).reshape(-1)
    n = g.size - (g.size % 4 if drop_tail else 0)
    pad = np.zeros(-(-g.size // CHUNK) * CHUNK, F32)
    pad[:n] = g[:n]
    return pad.reshape(-1, 4, 256, 4)


def _fma(a, b, c):
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


def _block_sum(lanes):
    """block_sum_ordered: [blocks, 256] -> [blocks]; xor butterfly over each wave of 64, then ((w0 + w1) + w2) + w3."""
    w = lanes.reshape(-1, 4, 64).astype(F32)
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = (w + w[:, :, idx ^ o]).astype(F32)
    w = w[:, :, 0]
    return (((w[:, 0] + w[:, 1]).astype(F32) + w[:, 2]).astype(F32) + w[:, 3]).astype(F32)


def emu_sqnorm(grads, max_norm, defect=None):
    """mv_optim_sqnorm_f32 -> (sum, factor) as float32."""
    c = np.concatenate([_chunks(g, defect == "tail_dropped") for g in grads])
    acc = np.zeros(c.shape[:1] + (256,), F32)
    for j in range(4):
        for k in range(4):
            acc = _fma(c[:, j, :, k], c[:, j, :, k], acc)
    part = _block_sum(acc)
    lanes = np.zeros(256, F32)
    for i in range(0, part.size, 256):
        seg = part[i:i + 256]
        lanes[:seg.size] = (lanes[:seg.size] + seg).astype(F32)
    s = _block_sum(lanes[None])[0]
    norm = np.sqrt(s, dtype=F32)
    below = norm < F32(max_norm)
    if defect == "clip_inverted":
        below = not below
    return s, (F32(1.0) if below else F32(max_norm) / norm)


def emulate(rule, params, grad_steps, max_norm=None, defect=None):
    """The optimiser + apply_updates in fp32 in the kernels' order -> (updates per step, parameters per step)."""
    kind, hp = RULES[rule]
    lrs = rates(len(grad_steps), defect)
    p = [np.asarray(a, F32).copy() for a in params]
    m = [np.zeros(a.shape, F32) for a in params]
    v = [np.zeros(a.shape, F32) for a in params]
    b1, b2, omb1, omb2, eps = F32(B1), F32(B2), F32(1.0 - B1), F32(1.0 - B2), F32(EPS)
    ups, pars = [], []
    for s, (grads, lr) in enumerate(zip(grad_steps, lrs), 1):
        lr = F32(lr)
        sc = F32(1.0) if max_norm is None else emu_sqnorm(grads, max_norm, defect)[1]
        count = s - 1 if defect == "count_minus_1" else s
        bc1, bc2 = F32(1.0 - B1 ** count), F32(1.0 - B2 ** count)
        step_u = []
        for i, g in enumerate(grads):
            g = (np.asarray(g, F32) * sc).astype(F32)
            with np.errstate(all="ignore"):
                if kind == "sgd":
                    if hp["momentum"] is None:
                        u = -lr * g
                    else:
                        mu = F32(hp["momentum"])
                        m[i] = g + mu * m[i]
                        u = -lr * (g + mu * m[i]) if hp["nesterov"] and defect != "nesterov_ignored" else -lr * m[i]
                else:
                    wd = F32(hp["weight_decay"])
                    if defect == "wd_coupled":
                        g = g + wd * p[i]
                    m[i] = b1 * m[i] + omb1 * g
                    v[i] = b2 * v[i] + omb2 * g * g
                    u = (m[i] / bc1) / (np.sqrt(v[i] / bc2) + eps)
                    u = -lr * (u if defect == "wd_coupled" else u + wd * p[i])
            u = np.asarray(u, F32)
            if defect == "tail_dropped" and u.size % 4:
                u = u.copy()
                u.reshape(-1)[u.size - u.size % 4:] = 0.0
            step_u.append(u)
            p[i] = (p[i] + u).astype(F32)
        ups.append(step_u)
        pars.append([a.copy() for a in p])
    return ups, pars
