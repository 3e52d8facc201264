"""Times the preprocessing launch (eqxvision_amd.preprocess.imagenet_eval: uint8 -> resize 256 -> crop 224 -> normalise) on one GPU.

    python tools/time_preprocess.py B [Hin Win]          (default image size 500 x 375)

Prints (a) images/s and achieved bytes/s of the launch alone (it reads Hin * Win * 3 bytes and writes 3 * 224^2 * 2 bytes per image
as bf16; HBM peak for comparison), and (b) the resnet50 bf16 forward alone against preprocess + forward, each ONE hipGraph from
`filter_jit`, timed in the same process in alternating rounds (A B A B ...), median and spread over the rounds.  The expectation it
checks: preprocess + forward is not slower than the forward alone by more than the launch's own time plus the run-to-run spread.
One JSON line at the end."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import eqxvision_amd as eqv  # noqa: E402

HBM_PEAK = 8.0e12          # bytes/s, MI355X specification; a float4 copy reaches about 6.3e12
ROUNDS, ITERS = 7, 20


def timed(fn, iters):
    """ms per call: `iters` back-to-back calls between two events, after the queue has drained."""
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / iters


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    hin, win = (int(sys.argv[2]), int(sys.argv[3])) if len(sys.argv) > 3 else (500, 375)
    rng = np.random.default_rng(0)
    u8 = torch.from_numpy(rng.integers(0, 256, (B, hin, win, 3), dtype=np.uint8)).cuda()
    x224 = torch.from_numpy(rng.standard_normal((B, 3, 224, 224)).astype(np.float32)).cuda().to(torch.bfloat16)
    net = eqv.tree_inference(eqv.utils.randomize_batchnorm(eqv.models.resnet50(key=eqv.random.PRNGKey(0)), 1), True)
    keys = eqv.random.split(eqv.random.PRNGKey(0), B)

    def fwd(n, im):
        return eqv.vmap(n, axis_name="batch")(im, key=keys)

    with eqv.precision("bf16"):
        prep = eqv.filter_jit(lambda im: eqv.preprocess.imagenet_eval(im, dtype="bf16"), clone_outputs=False)
        alone = eqv.filter_jit(fwd, clone_outputs=False)
        both = eqv.filter_jit(lambda n, im: fwd(n, eqv.preprocess.imagenet_eval(im, dtype="bf16")), clone_outputs=False)
        runs = {"prep": lambda: prep(u8), "fwd": lambda: alone(net, x224), "prep+fwd": lambda: both(net, u8)}
        for f in runs.values():                 # record, capture, and warm replays
            for _ in range(5):
                f()
        ms = {k: [] for k in runs}
        for _ in range(ROUNDS):                 # alternating: every round times all three
            for k, f in runs.items():
                ms[k].append(timed(f, ITERS))
    eqv._lib.check_device_status()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    spread = {k: float((max(v) - min(v)) / np.median(v)) for k, v in ms.items()}
    nbytes = B * (hin * win * 3 + 3 * 224 * 224 * 2)
    res = {
        "B": B, "Hin": hin, "Win": win, "rounds": ROUNDS, "iters": ITERS,
        "prep_ms": med["prep"], "prep_img_s": B / med["prep"] * 1e3, "prep_bytes_s": nbytes / med["prep"] * 1e3,
        "prep_frac_of_hbm_peak": nbytes / med["prep"] * 1e3 / HBM_PEAK,
        "fwd_ms": med["fwd"], "fwd_img_s": B / med["fwd"] * 1e3,
        "prep_fwd_ms": med["prep+fwd"], "prep_fwd_img_s": B / med["prep+fwd"] * 1e3,
        "spread": spread,
    }
    allowed = med["fwd"] + med["prep"] + max(spread["fwd"], spread["prep+fwd"]) * med["fwd"]
    res["extra_ms"] = med["prep+fwd"] - med["fwd"]
    res["within_expectation"] = bool(med["prep+fwd"] <= allowed)
    print(f"preprocess alone : {med['prep']:.3f} ms  {res['prep_img_s']:.0f} img/s  {res['prep_bytes_s'] / 1e12:.2f} TB/s "
          f"({100 * res['prep_frac_of_hbm_peak']:.0f} % of the {HBM_PEAK / 1e12:.0f} TB/s HBM peak)  spread {100 * spread['prep']:.1f} %")
    print(f"resnet50 bf16    : {med['fwd']:.3f} ms  {res['fwd_img_s']:.0f} img/s  spread {100 * spread['fwd']:.1f} %")
    print(f"preprocess + fwd : {med['prep+fwd']:.3f} ms  {res['prep_fwd_img_s']:.0f} img/s  spread {100 * spread['prep+fwd']:.1f} %  "
          f"(+{res['extra_ms']:.3f} ms over the forward; allowed {allowed - med['fwd']:.3f})")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
