"""The optimiser's share of a training step: wall time and launches of `update` + `apply_updates` per step on a model's parameter
set with random gradients (no forward / backward), in one process, the variants taking turns round by round so that clock and
allocator drift hit all of them alike:
    adam_per_leaf      adam + the per-leaf apply (one mv_adam_step_f32 and one mv_add_fwd per leaf: the path before csrc/optim.hip)
    adam               adam (per leaf) + the one-launch apply_updates
    adamw              one launch + the one-launch apply_updates
    clip+adamw         chain(clip_by_global_norm(1.0), adamw)
usage: time_optim.py [MODEL=resnet50] [ROUNDS=20] [STEPS=10]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import eqxvision_amd as eqv
from eqxvision_amd import _lib
from eqxvision_amd._module import DevArray, tree_map

model = sys.argv[1] if len(sys.argv) > 1 else "resnet50"
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 20
steps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
opt = eqv.optim
is_f = lambda l: eqv.is_array(l) and l.dtype.kind == "f"
rng = np.random.Generator(np.random.PCG64(0))
net0 = getattr(eqv.models, model)(num_classes=1000, key=eqv.random.PRNGKey(0))
net0 = tree_map(lambda l: DevArray(torch.from_numpy(np.ascontiguousarray(l, np.float32)).cuda()) if is_f(l) else l, net0)
grads = tree_map(lambda l: DevArray(torch.from_numpy(rng.standard_normal(l.shape).astype(np.float32)).cuda()) if is_f(l) else l, net0)
leaves = [l for l in eqv.tree_leaves(net0) if is_f(l)]
S = lambda: torch.cuda.current_stream().cuda_stream


def apply_per_leaf(net, updates):
    ups = iter([u for u in eqv.tree_leaves(updates) if is_f(u)])

    def step(leaf):
        if not is_f(leaf):
            return leaf
        u, out = next(ups), torch.empty_like(leaf.dev)
        _lib.call("mv_add_fwd", leaf.dev.data_ptr(), u.dev.data_ptr(), out.data_ptr(), out.numel(), _lib.ACT_NONE, _lib.F32, S())
        return DevArray(out)
    return tree_map(step, net)


VARIANTS = {"adam_per_leaf": (lambda: opt.adam(1e-3), apply_per_leaf),
            "adam": (lambda: opt.adam(1e-3), eqv.apply_updates),
            "adamw": (lambda: opt.adamw(1e-3), eqv.apply_updates),
            "clip+adamw": (lambda: opt.chain(opt.clip_by_global_norm(1.0), opt.adamw(1e-3)), eqv.apply_updates)}
launches = {}
orig = _lib.call


def run(name, count=False):
    make, apply = VARIANTS[name]
    o = make()
    net, st = net0, o.init(net0)
    n = [0]
    if count:
        _lib.call = lambda nm, *a: (n.__setitem__(0, n[0] + (2 if nm == "mv_optim_sqnorm_f32" else 1)), orig(nm, *a))[1]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        updates, st = o.update(grads, st, net)
        net = apply(net, updates)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    _lib.call = orig
    if count:
        launches[name] = n[0] / steps
    return 1e3 * dt


for name in VARIANTS:                      # warm-up: allocator, first launches; counts the launches per step (the squared norm is two)
    run(name, count=True)
times = {name: [] for name in VARIANTS}
for _ in range(rounds):
    for name in VARIANTS:
        times[name].append(run(name))
print(f"{model}: {len(leaves)} float leaves, {sum(l.size for l in leaves) / 1e6:.1f} M parameters; {rounds} rounds of {steps} steps")
for name, t in times.items():
    t = np.asarray(t)
    print(f"  {name:14s} {np.median(t):7.3f} ms / step (min {t.min():.3f}, max {t.max():.3f}), {launches[name]:.0f} launches / step")
