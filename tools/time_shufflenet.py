"""ShuffleNetV2 inference throughput on one MI355X (bench.py does not know the family): usage time_shufflenet.py [B] [repeats] [archs]

Synthetic weights, `tree_inference`, `filter_jit(lanes=2)` graph replay.  In ONE process and alternating, every architecture (default
shufflenet_v2_x0_5,shufflenet_v2_x1_0,shufflenet_v2_x2_0) is timed on the folded path and with "no_shuffle_dwpw" (the literal
composition: split, convolutions, concatenation, channel gather).  One JSON line: img/s and ms/step per configuration (medians and
the spread over the repeats), the fused / literal ratio, and the computed HBM bytes per image of the fused launch list with the
fraction of 8 TB/s they imply at the measured rate."""
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
from oracle import state as S

HBM_PEAK = 8.0e12


def fused_bytes_per_image(setting, size=224, classes=1000):
    """bf16 activation bytes every launch of the fused list reads and writes at least once, per image (weights not counted: they
    are shared by the batch).  -> (fused, literal): the literal list adds the split, the concatenation, the shuffle and the
    depthwise intermediate."""
    repeats, widths = setting
    hw = (size // 2) ** 2
    fused = size * size * 3 * 4 + hw * widths[0] * 2                   # conv1 (fp32 image in, bf16 out)
    fused += hw * widths[0] * 2 + hw // 4 * widths[0] * 2              # maxpool
    literal = fused
    hw //= 4
    cphys, cin = widths[0], widths[0]
    for n, cout in zip(repeats, widths[1:4]):
        bf, P = ops.shuffle_layout(cout // 2)
        ho = hw // 4
        # stride 2: branch1 tail (x -> L), first 1x1 (x -> t1), branch2 tail (t1 -> R)
        fused += (hw * cphys + ho * P) * 2 + (hw * cphys + hw * P) * 2 + (hw * P + ho * P) * 2
        literal += (hw * cin + ho * cin) * 2 + (ho * cin + ho * bf) * 2 + (hw * cin + hw * bf) * 2 + (hw * bf + ho * bf) * 2 \
            + 2 * ho * bf * 2 + 4 * ho * bf * 2 + 2 * ho * cout * 2
        # stride 1: first 1x1 (x -> t1), tail + pass-through (t1, x -> y)
        fused += (n - 1) * ((ho * 2 * P + ho * P) * 2 + (ho * P + ho * 2 * P + ho * 2 * P) * 2)
        literal += (n - 1) * (2 * ho * cout * 2 + 3 * 2 * ho * bf * 2 + 2 * ho * cout * 2 + 2 * ho * cout * 2)
        hw, cphys, cin = ho, 2 * P, cout
    tail = hw * cphys * 2 + hw * widths[4] * 2 + hw * widths[4] * 2 + widths[4] * 4 + classes * 4
    return fused + tail, literal + tail


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
    archs = (sys.argv[3] if len(sys.argv) > 3 else "shufflenet_v2_x0_5,shufflenet_v2_x1_0,shufflenet_v2_x2_0").split(",")
    steps = 20
    from tests import _shufflenet_ref as R
    nets = {a: _load(getattr(eqv.models, a), R.shufflenet_state(R.SETTINGS[a])) for a in archs}
    x = torch.as_tensor(S.synthetic_images(B, 224, seed=0)).cuda()
    keys = eqv.random.split(eqv.random.PRNGKey(0), B)

    def body(n, im, k):
        return eqv.vmap(n, axis_name="batch")(im, key=k)

    fwd = {(a, off): eqv.filter_jit(body, lanes=2) for a in archs for off in (0, 1)}

    def step(cfg):
        _lib.set_flag("no_shuffle_dwpw", cfg[1])
        try:
            return fwd[cfg](nets[cfg[0]], x, keys)
        finally:
            _lib.set_flag("no_shuffle_dwpw", 0)

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
    out = {"batch": B, "steps": steps, "repeats": reps}
    for a in archs:
        res = {}
        for off, name in ((0, "fused"), (1, "literal")):
            ts = np.asarray(times[(a, off)])
            med = float(np.median(ts))
            res[name] = {"img_s": round(B / med, 1), "ms_step": round(med * 1e3, 3), "spread_pct": round(100 * float(ts.max() - ts.min()) / med, 2)}
        fb, lb = fused_bytes_per_image(R.SETTINGS[a])
        res["fused_over_literal"] = round(res["fused"]["img_s"] / res["literal"]["img_s"], 4)
        res["hbm_bytes_per_img"] = {"fused": int(fb), "literal": int(lb)}
        res["hbm_peak_frac_fused"] = round(fb * res["fused"]["img_s"] / HBM_PEAK, 4)
        out[a] = res
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
