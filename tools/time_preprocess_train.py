"""Times the training-time input pipeline (eqxvision_amd.preprocess.imagenet_train) on a batch of differently sized images on one GPU.

    python tools/time_preprocess_train.py B          (default 256)

The batch is a fixed, seeded mix of the sizes 500x375, 375x500, 500x333, 333x500 and 640x480 (H x W), random pixels, resident on
the device as uint8 tensors; output 224 x 224, bf16 NCHW.  Every call draws fresh boxes and flips from a fresh key, as a training
step does.  Compared, alternating in one process (A B A B ..., median and spread over the rounds), wall time per batch,
synchronised before and after:
  train     one `imagenet_train(list, key)` call: the sampler, one pack, one record upload, one launch
  baseline  what the package offered before: the same sampler, then per image a crop of the device tensor, a single-image
            `resize_crop_normalize` of the crop (a new geometry nearly every time: two float64 tables built and uploaded), and
            `torch.flip` where the flag is set; one `torch.stack` at the end
Also the device time of the one launch alone (events around it, every buffer prepared beforehand), and the host time of the
sampler and of the record building.  Both routes compute the same transform for the same key; the tool compares them once
(bit-equal unless a weight of the tables and the generated one round differently: at most one bf16 ulp).
The parent process never opens the GPU: the measurement is a child process under its own `timeout`.  One JSON line at the end."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(500, 375), (375, 500), (500, 333), (333, 500), (640, 480)]
ROUNDS, ITERS, LAUNCH_ITERS = 7, 3, 20
CHILD_LIMIT_S = 400


def child(B):
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    from eqxvision_amd import _lib
    from eqxvision_amd import preprocess as P
    from eqxvision_amd import random as jr

    rng = np.random.default_rng(0)
    sizes = [SIZES[i] for i in rng.integers(0, len(SIZES), B)]
    ims = [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda() for h, w in sizes]
    step = [0]

    def next_key():
        step[0] += 1
        return jr.PRNGKey(step[0])

    def wall(fn, iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters * 1e3

    def events(fn, iters):
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(iters):
            fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) / iters

    def train(key=None):
        return P.imagenet_train(ims, next_key() if key is None else key, dtype="bf16")

    def baseline(key=None):
        k_box, k_flip = jr.split(next_key() if key is None else key, 2)
        boxes, flips = P.random_resized_crop_boxes(k_box, sizes), P.random_flips(k_flip, B)
        out = []
        for im, (top, left, h, w), f in zip(ims, boxes.tolist(), flips):
            y = P.resize_crop_normalize(im[top:top + h, left:left + w].contiguous(), (224, 224), (0, 0, 224, 224), dtype="bf16")
            out.append(torch.flip(y, dims=[2]) if f else y)
        return torch.stack(out)

    # the launch alone: every operand on the device beforehand
    k_box, k_flip = jr.split(jr.PRNGKey(0), 2)
    rec, _ = P.boxes_plan(sizes, P.random_resized_crop_boxes(k_box, sizes), P.random_flips(k_flip, B), 224)
    a, b = P._device_affine(P.IMAGENET_MEAN, P.IMAGENET_STD)
    x = P.pack_images(ims)
    rec_dev = torch.from_numpy(rec.view(np.uint8)).cuda()
    yB = torch.empty((B, 3, 224, 224), dtype=torch.bfloat16, device="cuda")
    args = (x.data_ptr(), x.numel(), yB.data_ptr(), rec.ctypes.data, rec_dev.data_ptr(), a.data_ptr(), b.data_ptr(), B, 224, 224, 0,
            _lib.BF16, 0, P.stream_ptr())

    def launch():
        _lib.call("mv_preprocess_u8_boxes_fwd", *args)

    runs = {"train": (wall, train, ITERS), "baseline": (wall, baseline, ITERS), "launch": (events, launch, LAUNCH_ITERS)}
    for _, f, _ in runs.values():              # warm: the allocator, the affine vectors, code objects
        for _ in range(2):
            f()
    ms = {k: [] for k in runs}
    for _ in range(ROUNDS):
        for k, (timer, f, iters) in runs.items():
            ms[k].append(timer(f, iters))
    _lib.check_device_status()
    y_train, y_base = train(jr.PRNGKey(12345)), baseline(jr.PRNGKey(12345))
    same = bool(torch.equal(y_train, y_base))           # table weights and generated weights are both one rounding of the same
    worst = float((y_train.float() - y_base.float()).abs().max())      # float64 value; their sums may be added in another order

    def host_ms(fn, iters=5):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        return (time.perf_counter() - t0) / iters * 1e3

    boxes = P.random_resized_crop_boxes(k_box, sizes)
    res = {"B": B, "rounds": ROUNDS, "same_bits": same, "max_abs_diff": worst, "input_MB": sum(h * w * 3 for h, w in sizes) / 1e6,
           "output_MB": B * 3 * 224 * 224 * 2 / 1e6,
           "sampler_ms": host_ms(lambda: P.random_resized_crop_boxes(k_box, sizes)),
           "records_ms": host_ms(lambda: P.boxes_plan(sizes, boxes, None, 224)),
           "pack_ms": wall(lambda: P.pack_images(ims), 5)}
    for k, v in ms.items():
        res[k + "_ms"] = float(np.median(v))
        res[k + "_spread"] = float((max(v) - min(v)) / np.median(v))
    print(f"imagenet_train of {B} images {res['train_ms']:.3f} ms (spread {100 * res['train_spread']:.1f} %)   baseline "
          f"{res['baseline_ms']:.3f} ms (spread {100 * res['baseline_spread']:.1f} %)   x{res['baseline_ms'] / res['train_ms']:.2f}")
    print(f"launch alone {res['launch_ms']:.3f} ms (spread {100 * res['launch_spread']:.1f} %), {res['input_MB']:.1f} MB in the buffer, "
          f"{res['output_MB']:.1f} MB out;  host: sampler {res['sampler_ms']:.3f} ms, records {res['records_ms']:.3f} ms, device pack "
          f"{res['pack_ms']:.3f} ms;  same bits as the baseline: {same} (max |diff| {worst:.3g})")
    print("RESULT " + json.dumps(res))
    return 0 if worst <= 2.0 ** -6 else 1            # one bf16 ulp at the largest normalised value (2.64)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        sys.exit(child(int(sys.argv[2])))
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    r = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", str(B)],
                       stdout=subprocess.PIPE, text=True)
    sys.stdout.write(r.stdout)
    if r.returncode != 0:
        print(f"measurement failed (exit status {r.returncode})")
        sys.exit(r.returncode)
    print(json.dumps(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])))


if __name__ == "__main__":
    main()
