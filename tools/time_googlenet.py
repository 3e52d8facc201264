"""GoogLeNet inference throughput on one MI355X (bench.py does not know the family): usage time_googlenet.py [B] [repeats]

Synthetic weights, `tree_inference`, `filter_jit(lanes=2)` graph replay.  In ONE process and alternating, the network is timed on the
fused path (4 launches per Inception module) and with "no_inception_fused" (the literal composition: six convolutions, the pool and
four copies per module).  Then every Inception module at a 224 input is timed on its own, eagerly, both ways.  One JSON line: img/s
and ms/step per configuration (medians and the spread over the repeats), the fused / literal ratio, and the per-module
milliseconds."""
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

SWITCH = "no_inception_fused"


def _load(sd):
    with tempfile.TemporaryDirectory() as td:
        p = os.path.join(td, "w.pth")
        S.save_pth(sd, p)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return eqv.tree_inference(eqv.models.googlenet(torch_weights=p), True)


def _time_module(mod, B, H, C, iters=20):
    x = Act(torch.randn(B, H, H, C, device="cuda").to(torch.bfloat16), "map", True)
    res = {}
    for off, name in ((0, "fused"), (1, "literal")):
        _lib.set_flag(SWITCH, off)
        _lib.set_flag("inception_always", 1)               # also where ops.inception keeps the composition: both ways are measured
        try:
            for _ in range(3):
                ops.inception(x, mod)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
            e0.record()
            for _ in range(iters):
                ops.inception(x, mod)
            e1.record()
            torch.cuda.synchronize()
            res[name] = round(e0.elapsed_time(e1) / iters, 4)
        finally:
            _lib.set_flag(SWITCH, 0)
            _lib.set_flag("inception_always", 0)
    return res


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    steps = 20
    from tests import _googlenet_ref as R
    net = _load(R.googlenet_state())
    x = torch.as_tensor(S.synthetic_images(B, 224, seed=0)).cuda()
    keys = eqv.random.split(eqv.random.PRNGKey(0), B)

    def body(n, im, k):
        return eqv.vmap(n, axis_name="batch")(im, key=k)

    fwd = {off: eqv.filter_jit(body, lanes=2) for off in (0, 1)}

    def step(off):
        _lib.set_flag(SWITCH, off)
        try:
            return fwd[off](net, x, keys)
        finally:
            _lib.set_flag(SWITCH, 0)

    out = {"batch": B, "steps": steps, "repeats": reps}
    with eqv.precision("bf16"):
        for off in fwd:                                    # capture + warm-up
            for _ in range(3):
                step(off)
        torch.cuda.synchronize()
        times = {off: [] for off in fwd}
        for _ in range(reps):
            for off in fwd:                                # alternating
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    step(off)
                torch.cuda.synchronize()
                times[off].append((time.perf_counter() - t0) / steps)
        res = {}
        for off, name in ((0, "fused"), (1, "literal")):
            ts = np.asarray(times[off])
            med = float(np.median(ts))
            res[name] = {"img_s": round(B / med, 1), "ms_step": round(med * 1e3, 3),
                         "spread_pct": round(100 * float(ts.max() - ts.min()) / med, 2)}
        res["fused_over_literal"] = round(res["fused"]["img_s"] / res["literal"]["img_s"], 4)
        res["inceptions_ms"] = {}
        for name, spec in R.INCEPTIONS.items():
            h = R.MAP_224[name]
            tag = f"{name} {spec[0]}->{spec[1]}+{spec[3]}+{spec[5]}+{spec[6]} @{h}x{h}"
            res["inceptions_ms"][tag] = _time_module(getattr(net, name), B, h, spec[0])
        out["googlenet"] = res
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
