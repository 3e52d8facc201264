"""SqueezeNet inference throughput on one MI355X (bench.py does not know the family): usage time_squeezenet.py [B] [repeats] [archs]

Synthetic weights, `tree_inference`, `filter_jit(lanes=2)` graph replay.  In ONE process and alternating, every architecture (default
squeezenet1_1,squeezenet1_0) is timed on the fused path and with "no_fire_expand" (the literal composition: three convolutions and
the concatenation per Fire).  Then every distinct Fire of the architecture at a 224 input is timed on its own, eagerly, both ways
(squeeze included in both).  One JSON line: img/s and ms/step per configuration (medians and the spread over the repeats), the
fused / literal ratio, and the per-Fire milliseconds."""
import json
import os
import sys
import tempfile
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import eqxvision_amd as eqv
from eqxvision_amd import _lib, ops
from eqxvision_amd._act import Act
from oracle import state as S

VERSION = {"squeezenet1_0": "1_0", "squeezenet1_1": "1_1"}


def _load(factory, sd):
    with tempfile.TemporaryDirectory() as td:
        p = os.path.join(td, "w.pth")
        S.save_pth(sd, p)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return eqv.tree_inference(factory(torch_weights=p), True)


def _fire_maps(net, size=224):
    """[(features index, Fire, H)] with the map size each Fire sees at a size x size input."""
    L = net.features.layers
    h = (size - L[0].kernel_size[0]) // 2 + 1
    out = []
    for i, layer in enumerate(L[2:], start=2):
        if isinstance(layer, eqv.nn.MaxPool2d):
            h = layer.output_size(h, h)[0]
        else:
            out.append((i, layer, h))
    return out


def _time_fire(fire, B, H, iters=30):
    x = Act(torch.randn(B, H, H, fire.inplanes, device="cuda").to(torch.bfloat16), "map", True)
    res = {}
    for off, name in ((0, "fused"), (1, "literal")):
        _lib.set_flag("no_fire_expand", off)
        _lib.set_flag("fire_expand_always", 1)             # also where ops.fire keeps the composition: both ways are measured
        try:
            for _ in range(3):
                ops.fire(x, fire)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
            e0.record()
            for _ in range(iters):
                ops.fire(x, fire)
            e1.record()
            torch.cuda.synchronize()
            res[name] = round(e0.elapsed_time(e1) / iters, 4)
        finally:
            _lib.set_flag("no_fire_expand", 0)
            _lib.set_flag("fire_expand_always", 0)
    return res


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    archs = (sys.argv[3] if len(sys.argv) > 3 else "squeezenet1_1,squeezenet1_0").split(",")
    steps = 20
    from tests import _squeezenet_ref as R
    nets = {a: _load(getattr(eqv.models, a), R.squeezenet_state(VERSION[a])) for a in archs}
    x = torch.as_tensor(S.synthetic_images(B, 224, seed=0)).cuda()
    keys = eqv.random.split(eqv.random.PRNGKey(0), B)

    def body(n, im, k):
        return eqv.vmap(n, axis_name="batch")(im, key=k)

    fwd = {(a, off): eqv.filter_jit(body, lanes=2) for a in archs for off in (0, 1)}

    def step(cfg):
        _lib.set_flag("no_fire_expand", cfg[1])
        try:
            return fwd[cfg](nets[cfg[0]], x, keys)
        finally:
            _lib.set_flag("no_fire_expand", 0)

    out = {"batch": B, "steps": steps, "repeats": reps}
    with eqv.precision("bf16"):
        for cfg in fwd:                                    # capture + warm-up
            for _ in range(3):
                step(cfg)
        torch.cuda.synchronize()
        times = {cfg: [] for cfg in fwd}
        for _ in range(reps):
            for cfg in fwd:                                # alternating
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    step(cfg)
                torch.cuda.synchronize()
                times[cfg].append((time.perf_counter() - t0) / steps)
        for a in archs:
            res = {}
            for off, name in ((0, "fused"), (1, "literal")):
                ts = np.asarray(times[(a, off)])
                med = float(np.median(ts))
                res[name] = {"img_s": round(B / med, 1), "ms_step": round(med * 1e3, 3),
                             "spread_pct": round(100 * float(ts.max() - ts.min()) / med, 2)}
            res["fused_over_literal"] = round(res["fused"]["img_s"] / res["literal"]["img_s"], 4)
            res["fires_ms"] = {}
            for i, fire, h in _fire_maps(nets[a]):
                tag = f"features.{i} {fire.inplanes}->{fire.squeeze.out_channels}->{2 * fire.expand1x1.out_channels} @{h}x{h}"
                res["fires_ms"][tag] = _time_fire(fire, B, h)
            out[a] = res
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
