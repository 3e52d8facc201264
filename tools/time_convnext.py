"""convnext_tiny inference throughput on one MI355X (bench.py does not know ConvNeXt): usage time_convnext.py [B] [repeats]

Synthetic weights, `tree_inference`, `filter_jit(lanes=2)` graph replay.  In ONE process and alternating, three configurations are
timed: convnext_tiny on the fused block kernels, convnext_tiny with "no_cnblock_dw" + "no_ln_mlp" + "no_ln_mlp_stream" (the
composition of the generic entries), and swin_t at the same batch (same widths and GFLOP per image).  One JSON line: img/s, ms/step
and the whole-forward fraction of 2.5 PFLOP/s (dense bf16) per configuration, medians and the spread over the repeats."""
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
from eqxvision_amd import _lib
from oracle import state as S

PEAK = 2.5e15
FLAGS_OFF = ("no_cnblock_dw", "no_ln_mlp", "no_ln_mlp_stream")


def convnext_gflop(setting=((96, 192, 3), (192, 384, 3), (384, 768, 9), (768, None, 3)), size=224, classes=1000):
    """2 x MACs of the convolutions and Linears, from the shapes."""
    hw = (size // 4) ** 2
    macs = hw * 3 * 16 * setting[0][0]                                          # stem 4x4/4
    for cin, cout, n in setting:
        macs += n * hw * (cin * 49 + 2 * cin * 4 * cin)                          # dw 7x7 + fc1 + fc2
        if cout is not None:
            hw //= 4
            macs += hw * cin * 4 * cout                                          # 2x2/2 downsample
    macs += (setting[-1][1] or setting[-1][0]) * classes
    return 2 * macs / 1e9


def _load(factory, sd):
    with tempfile.TemporaryDirectory() as td:
        p = os.path.join(td, "w.pth")
        S.save_pth(sd, p)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return eqv.tree_inference(factory(torch_weights=p), True)


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    steps = 20
    from tests import _convnext_ref as R
    cnx = _load(eqv.models.convnext_tiny, R.convnext_state(R.SETTINGS["convnext_tiny"]))
    swin = _load(eqv.models.swin_t, S.swin_state(1))
    x = torch.as_tensor(S.synthetic_images(B, 224, seed=0)).cuda()
    keys = eqv.random.split(eqv.random.PRNGKey(0), B)

    def body(n, im, k):
        return eqv.vmap(n, axis_name="batch")(im, key=k)

    def flags(v):
        for f in FLAGS_OFF:
            _lib.set_flag(f, v)

    fwd = {"convnext_tiny": eqv.filter_jit(body, lanes=2), "convnext_tiny_off": eqv.filter_jit(body, lanes=2),
           "swin_t": eqv.filter_jit(body, lanes=2)}
    nets = {"convnext_tiny": cnx, "convnext_tiny_off": cnx, "swin_t": swin}

    def step(name):
        flags(1 if name.endswith("_off") else 0)
        try:
            return fwd[name](nets[name], x, keys)
        finally:
            flags(0)

    with eqv.precision("bf16"):
        for name in fwd:                                   # capture + warm-up
            for _ in range(3):
                step(name)
        torch.cuda.synchronize()
        times = {n: [] for n in fwd}
        for _ in range(reps):
            for name in fwd:                               # alternating
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(steps):
                    step(name)
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) / steps)
    g = {"convnext_tiny": convnext_gflop(), "convnext_tiny_off": convnext_gflop(), "swin_t": 8.7}
    out = {"batch": B, "steps": steps, "repeats": reps, "gflop_per_img": {"convnext_tiny": round(g["convnext_tiny"], 3), "swin_t": 8.7}}
    for name, ts in times.items():
        ts = np.asarray(ts)
        med = float(np.median(ts))
        out[name] = {"img_s": round(B / med, 1), "ms_step": round(med * 1e3, 3),
                     "spread_pct": round(100 * float(ts.max() - ts.min()) / med, 2),
                     "peak_frac": round(B * g[name] * 1e9 / med / PEAK, 4)}
    out["fused_over_off"] = round(out["convnext_tiny"]["img_s"] / out["convnext_tiny_off"]["img_s"], 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
