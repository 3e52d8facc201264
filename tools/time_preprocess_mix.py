"""Times the full classification training input (eqxvision_amd.preprocess.imagenet_train_mixed) against the composition that was
available before it, on one GPU.

    python tools/time_preprocess_mix.py B [Hin Win]      (default 256 500 375)

The batch is B random uint8 images of Hin x Win, resident on the device as one array; output 224 x 224, fp32 NCHW, 1000 classes,
label smoothing 0.1, random erasing with p = 0.25.  Every call draws from a fresh key, as a training step does.  Compared,
alternating in one process (A B A B ..., median and spread over the rounds), wall time per batch, synchronised before and after,
once with the batch draw forced to mixup (two resamples per pixel in the one launch) and once forced to cutmix:
  mixed        one `imagenet_train_mixed(batch, labels, key, 1000)` call: the draws, two record uploads, one launch
  composition  `imagenet_train` with the same boxes and flips, then torch device ops on the fp32 batch -- the erase rectangles filled
               with 0, `roll`, `mul_` / `add_` (mixup) or a box copy (cutmix), as torchvision's reference transforms do -- and the
               soft targets made on the host (one-hot, smoothing, the same mix) and uploaded
Both routes use the same draws for the same key; the tool compares them once per branch.  The parent process never opens the
GPU: the measurement is a child process under its own `timeout`.  One JSON line at the end."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUNDS, ITERS = 7, 3
K, EPS, ERASE_P, SIZE = 1000, 0.1, 0.25, 224
CHILD_LIMIT_S = 400


def child(B, hin, win):
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    from eqxvision_amd import _lib
    from eqxvision_amd import preprocess as P
    from eqxvision_amd import random as jr

    rng = np.random.default_rng(0)
    ims = torch.from_numpy(rng.integers(0, 256, (B, hin, win, 3), dtype=np.uint8)).cuda()
    labels = rng.integers(0, K, B)
    sizes = [(hin, win)] * B
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

    def alphas(branch):
        return dict(mixup_alpha=0.2, cutmix_alpha=0.0) if branch == "mixup" else dict(mixup_alpha=0.0, cutmix_alpha=1.0)

    def mixed(branch, key=None):
        return P.imagenet_train_mixed(ims, labels, next_key() if key is None else key, K, erase_p=ERASE_P, label_smoothing=EPS,
                                      **alphas(branch))

    def composition(branch, key=None):
        k_box, k_flip, k_mix, k_erase = jr.split(next_key() if key is None else key, 4)
        boxes, flips = P.random_resized_crop_boxes(k_box, sizes), P.random_flips(k_flip, B)
        partner, lam, cut, lam_t = P.mixup_cutmix_draw(k_mix, B, SIZE, **alphas(branch))
        erase = P.random_erasing_draw(k_erase, B, SIZE, ERASE_P)
        x = P.crop_resize_normalize(ims, boxes, SIZE, flips)
        for i, (y0, x0, y1, x1) in enumerate(erase.tolist()):
            if y1 > y0 and x1 > x0:
                x[i, :, y0:y1, x0:x1] = 0.0
        rolled = x.roll(1, 0)
        y0, x0, y1, x1 = cut[0].tolist()
        if branch == "mixup":
            rolled.mul_(float(np.float32(1.0 - np.float64(lam[0]))))
            x.mul_(float(lam[0])).add_(rolled)
        elif y1 > y0 and x1 > x0:
            x[:, :, y0:y1, x0:x1] = rolled[:, :, y0:y1, x0:x1]
        s = np.full((B, K), np.float32(EPS / K), np.float32)
        s[np.arange(B), labels] = np.float32(1.0 - EPS + EPS / K)
        lt = np.float32(lam_t[0])
        t = lt * s + np.float32(1.0 - np.float64(lt)) * np.roll(s, 1, 0)
        return x, torch.from_numpy(t).cuda()

    res = {"B": B, "Hin": hin, "Win": win, "rounds": ROUNDS}
    status = 0
    for branch in ("mixup", "cutmix"):
        runs = {"mixed": lambda: mixed(branch), "composition": lambda: composition(branch)}
        for f in runs.values():                    # warm: the allocator, the affine vectors, code objects
            for _ in range(2):
                f()
        ms = {k: [] for k in runs}
        for _ in range(ROUNDS):
            for k, f in runs.items():
                ms[k].append(wall(f, ITERS))
        _lib.check_device_status()
        key = jr.PRNGKey(12345)
        (xa, ta), (xb, tb) = mixed(branch, key), composition(branch, key)
        same_x, same_t = bool(torch.equal(xa, xb)), bool(torch.equal(ta.dev, tb))
        worst = float((xa - xb).abs().max())
        for k, v in ms.items():
            res[f"{branch}_{k}_ms"] = float(np.median(v))
            res[f"{branch}_{k}_spread"] = float((max(v) - min(v)) / np.median(v))
        res[f"{branch}_ratio"] = res[f"{branch}_composition_ms"] / res[f"{branch}_mixed_ms"]
        res[f"{branch}_same_bits"] = same_x and same_t
        print(f"{branch}: imagenet_train_mixed of {B} images {hin}x{win} {res[branch + '_mixed_ms']:.3f} ms (spread "
              f"{100 * res[branch + '_mixed_spread']:.1f} %)   composition {res[branch + '_composition_ms']:.3f} ms (spread "
              f"{100 * res[branch + '_composition_spread']:.1f} %)   composition / mixed = {res[branch + '_ratio']:.2f};  same bits: "
              f"images {same_x}, targets {same_t} (max |diff| {worst:.3g})")
        if worst > 2.0 ** -20:                     # torch's mul_ / add_ round like the kernel; a contraction on either side would show here
            status = 1
    print("RESULT " + json.dumps(res))
    return status


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        sys.exit(child(*(int(v) for v in sys.argv[2:5])))
    args = [int(v) for v in sys.argv[1:4]]
    B, hin, win = (args + [256, 500, 375][len(args):]) if len(args) in (0, 1, 3) else sys.exit(__doc__)
    r = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", str(B), str(hin),
                        str(win)], stdout=subprocess.PIPE, text=True)
    sys.stdout.write(r.stdout)
    if r.returncode != 0:
        print(f"measurement failed (exit status {r.returncode})")
        sys.exit(r.returncode)
    print(json.dumps(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])))


if __name__ == "__main__":
    main()
