"""DenseNet inference throughput on one MI355X (bench.py does not know the family): usage time_densenet.py [MODEL] [B] [repeats]

Synthetic weights, `tree_inference`, `filter_jit(lanes=2)` graph replay.  In ONE process and alternating, the network is timed on the
fused path (two launches per dense layer, one per transition) and with "no_dense_fused" (the literal composition on the kernels the
package already had: a concatenation, a BatchNorm + ReLU pass and two convolutions per layer).  Then every dense block and every
transition at a 224 input is timed on its own, eagerly, both ways (the classes of ops.DENSE_LITERAL_SHAPES), and the 3x3 slice kernel
with its 64- and its 128-pixel tile on the four maps.  One JSON line: img/s and ms/step per configuration (medians and the spread over
the repeats), the fused / literal ratio, and the per-class milliseconds."""
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

SWITCH = "no_dense_fused"


def _load(variant, sd):
    with tempfile.TemporaryDirectory() as td:
        p = os.path.join(td, "w.pth")
        S.save_pth(sd, p)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return eqv.tree_inference(getattr(eqv.models, variant)(torch_weights=p), True)


def _timed(fn, iters=10):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / iters, 4)


def _ab(fn):
    res = {}
    for off, name in ((0, "fused"), (1, "literal"), (0, "fused_again")):         # the third figure is the run-to-run spread
        _lib.set_flag(SWITCH, off)
        _lib.set_flag("dense_always", 1)                   # also where ops.dense_block keeps the composition: both ways are measured
        try:
            res[name] = _timed(fn)
        finally:
            _lib.set_flag(SWITCH, 0)
            _lib.set_flag("dense_always", 0)
    return res


def _tiles(B, mid, g):
    out = {}
    wf = torch.from_numpy(ops.inception_fragments(np.zeros((g, mid, 3, 3), np.float32))).to(torch.bfloat16).cuda()
    for H in (56, 28, 14, 7):
        t = torch.randn(B, H, H, mid, device="cuda").to(torch.bfloat16)
        y = torch.empty(B, H, H, 8 * g, device="cuda", dtype=torch.bfloat16)
        st = torch.cuda.current_stream().cuda_stream
        row = {}
        for flag, name in (("dense3x3_m64", "m64"), ("dense3x3_m128", "m128"), ("dense3x3_m64", "m64_again")):
            _lib.set_flag(flag, 1)
            try:
                row[name] = _timed(lambda: _lib.call("mv_conv3x3_slice_fwd", t.data_ptr(), mid, mid, wf.data_ptr(), y.data_ptr(), 8 * g, g, g,
                                                     B, H, H, _lib.BF16, _lib.BF16, st), iters=20)
            finally:
                _lib.set_flag(flag, 0)
        out[f"S{mid} N{g} @{H}x{H} ({B * H * H} px)"] = row
    return out


def main():
    variant = sys.argv[1] if len(sys.argv) > 1 else "densenet121"
    B = int(sys.argv[2]) if len(sys.argv) > 2 else 256
    reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    steps = 10
    from tests import _densenet_ref as R
    net = _load(variant, R.densenet_state(variant, head_scale_=1.0))
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

    out = {"model": variant, "batch": B, "steps": steps, "repeats": reps}
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
        g, cfg, c = R.VARIANTS[variant]
        L = net.features.layers
        res["blocks_ms"], res["transitions_ms"] = {}, {}
        h = 56
        for b, n in enumerate(cfg):
            xb = Act(torch.randn(B, h, h, c, device="cuda").to(torch.bfloat16), "map", True)
            res["blocks_ms"][f"block{b + 1} (C0={c}, L={n}, g={g}, H={h})"] = _ab(lambda: ops.dense_block(xb, L[4 + 2 * b]))
            c += n * g
            if b != len(cfg) - 1:
                xt = Act(torch.randn(B, h, h, c, device="cuda").to(torch.bfloat16), "map", True)
                res["transitions_ms"][f"transition{b + 1} ({c}->{c // 2} @{h}x{h})"] = _ab(lambda: ops.dense_transition(xt, L[5 + 2 * b]))
                c, h = c // 2, h // 2
        res["slice_tiles_ms"] = _tiles(B, R.BN_SIZE * g, g)
        out[variant] = res
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
