"""Times the segmentation training input pipeline (eqxvision_amd.preprocess.segmentation_train) on a batch of differently sized
images and masks on one GPU.

    python tools/time_preprocess_seg.py B          (default 16)

The batch is a fixed, seeded mix of the sizes 500x375, 375x500, 500x333, 333x500 and 640x480 (H x W), random pixels and labels,
resident on the device as uint8 tensors; base size 520, crop 480, fp32 NCHW and int32 labels.  Every call draws fresh sizes, flips
and origins from a fresh key, as a training step does.  Compared, alternating in one process (A B A B ..., median and spread over
the rounds), wall time per batch, synchronised before and after:
  seg       one `segmentation_train(list, list, key)` call: the samplers, two packs, one record upload, one launch
  torch     the same draws, then per image the same transform composed from torch device ops: interpolate(antialias=True) of the
            image, interpolate(mode="nearest-exact") of the mask, flip, pad, slice, normalise; one `torch.stack` each at the end
Also the device time of the one launch alone (events around it, every buffer prepared beforehand), and a `deeplabv3` (ResNet-50)
training step -- forward, per-pixel loss on out and aux, backward, sgd update -- alone and with the `segmentation_train` call
in front of it.  The two routes are compared once: the share of labels that differ and the largest image difference are
reported (torch evaluates both rules with an fp32 scale and fp32 weights).
The parent process never opens the GPU: the measurement is a child process under its own `timeout`.  One JSON line at the end."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(500, 375), (375, 500), (500, 333), (333, 500), (640, 480)]
BASE, CROP = 520, 480
ROUNDS, ITERS, LAUNCH_ITERS, STEP_ITERS = 5, 3, 20, 2
CHILD_LIMIT_S = 500


def child(B):
    import numpy as np
    import torch
    import torch.nn.functional as F

    sys.path.insert(0, ROOT)
    import eqxvision_amd as eqv
    from eqxvision_amd import _lib
    from eqxvision_amd import preprocess as P
    from eqxvision_amd import random as jr
    from eqxvision_amd.models.classification import resnet as RN

    rng = np.random.default_rng(0)
    sizes = [SIZES[i] for i in rng.integers(0, len(SIZES), B)]
    ims = [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda() for h, w in sizes]
    mks = [torch.from_numpy(rng.integers(0, 21, (h, w), dtype=np.uint8)).cuda() for h, w in sizes]
    mean = torch.tensor(P.IMAGENET_MEAN, device="cuda").view(3, 1, 1)
    std = torch.tensor(P.IMAGENET_STD, device="cuda").view(3, 1, 1)
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

    def draws(key):
        k_size, k_flip, k_origin = jr.split(key, 3)
        rs = P.random_resize_sizes(k_size, sizes, int(0.5 * BASE), int(2.0 * BASE))
        return rs, P.random_flips(k_flip, B), P.random_crop_origins(k_origin, rs, CROP)

    def seg(key=None):
        return P.segmentation_train(ims, mks, next_key() if key is None else key, BASE, CROP)

    def composed(key=None):
        rs, flips, og = draws(next_key() if key is None else key)
        xs, ls = [], []
        for im, mk, (hr, wr), f, (top, left) in zip(ims, mks, rs.tolist(), flips, og.tolist()):
            x = F.interpolate(im.permute(2, 0, 1)[None].float(), size=(hr, wr), mode="bilinear", antialias=True, align_corners=False)[0]
            lab = F.interpolate(mk[None, None].float(), size=(hr, wr), mode="nearest-exact")[0, 0]
            if f:
                x, lab = torch.flip(x, dims=[2]), torch.flip(lab, dims=[1])
            ph, pw = max(CROP - hr, 0), max(CROP - wr, 0)
            x, lab = F.pad(x, (0, pw, 0, ph), value=0.0), F.pad(lab, (0, pw, 0, ph), value=255.0)
            x, lab = x[:, top:top + CROP, left:left + CROP], lab[top:top + CROP, left:left + CROP]
            xs.append((x / 255.0 - mean) / std)
            ls.append(lab.to(torch.int32))
        return torch.stack(xs), torch.stack(ls)

    # the launch alone: every operand on the device beforehand
    rs, flips, og = draws(jr.PRNGKey(0))
    rec, _ = P.seg_plan(sizes, rs, og, flips, CROP)
    a, b = P._device_affine(P.IMAGENET_MEAN, P.IMAGENET_STD)
    x, m = P.pack_images(ims), P.pack_images(mks)
    rec_dev = torch.from_numpy(rec.view(np.uint8)).cuda()
    yB = torch.empty((B, 3, CROP, CROP), dtype=torch.float32, device="cuda")
    lB = torch.empty((B, CROP, CROP), dtype=torch.int32, device="cuda")
    args = (x.data_ptr(), x.numel(), m.data_ptr(), m.numel(), yB.data_ptr(), lB.data_ptr(), rec.ctypes.data, rec_dev.data_ptr(),
            a.data_ptr(), b.data_ptr(), B, CROP, CROP, 0, 255, 0, _lib.F32, 0, P.stream_ptr())

    def launch():
        _lib.call("mv_preprocess_u8_seg_fwd", *args)

    # a deeplabv3 training step, alone and behind the pipeline
    bb = RN._resnet(RN._ResNetBottleneck, [3, 4, 6, 3], None, replace_stride_with_dilation=[False, True, True])
    net = [eqv.models.deeplabv3(num_classes=21, backbone=bb, intermediate_layers=lambda mm: [mm.layer3, mm.layer4], aux_in_channels=1024,
                                key=jr.PRNGKey(0))]
    keys = jr.split(jr.PRNGKey(1), B)
    xent = eqv.optim.softmax_cross_entropy_with_integer_labels
    opt = eqv.optim.sgd(learning_rate=0.01)
    state = [opt.init(eqv.filter(net[0], eqv.is_array))]

    @eqv.filter_value_and_grad
    def compute_loss(model, xx, yy):
        aux, out = eqv.vmap(model, axis_name="batch")(xx, key=keys)
        ww = yy != 255
        return xent(out, yy, axis=1, where=ww).mean() + 0.4 * xent(aux, yy, axis=1, where=ww).mean()

    fixed = seg(jr.PRNGKey(77))

    def train_step(batch=None):
        xx, yy = fixed if batch is None else batch
        _, grads = compute_loss(net[0], xx, yy)
        updates, state[0] = opt.update(grads, state[0])
        net[0] = eqv.apply_updates(net[0], updates)

    def seg_and_step():
        train_step(seg())

    runs = {"seg": (wall, seg, ITERS), "torch": (wall, composed, ITERS), "launch": (events, launch, LAUNCH_ITERS),
            "step": (wall, train_step, STEP_ITERS), "seg_step": (wall, seg_and_step, STEP_ITERS)}
    for _, f, _ in runs.values():              # warm: the allocator, the affine vectors, code objects
        for _ in range(2):
            f()
    ms = {k: [] for k in runs}
    for _ in range(ROUNDS):
        for k, (timer, f, iters) in runs.items():
            ms[k].append(timer(f, iters))
    _lib.check_device_status()
    (ys, ls), (yt, lt) = seg(jr.PRNGKey(12345)), composed(jr.PRNGKey(12345))
    # torch evaluates both rules with an fp32 scale: a label whose centre falls on (or within rounding of) a source pixel edge may
    # come from the neighbour, and its filter weights are fp32; the kernel's rule is the integer one and its weights float64
    label_mismatch = float((ls != lt).float().mean())
    worst = float((ys - yt).abs().max())

    res = {"B": B, "rounds": ROUNDS, "label_mismatch": label_mismatch, "max_abs_diff": worst,
           "input_MB": sum(h * w * 4 for h, w in sizes) / 1e6, "output_MB": B * CROP * CROP * (3 * 4 + 4) / 1e6}
    for k, v in ms.items():
        res[k + "_ms"] = float(np.median(v))
        res[k + "_spread"] = float((max(v) - min(v)) / np.median(v))
    print(f"segmentation_train of {B} images {res['seg_ms']:.3f} ms (spread {100 * res['seg_spread']:.1f} %)   torch ops "
          f"{res['torch_ms']:.3f} ms (spread {100 * res['torch_spread']:.1f} %)   x{res['torch_ms'] / res['seg_ms']:.2f}")
    print(f"launch alone {res['launch_ms']:.3f} ms (spread {100 * res['launch_spread']:.1f} %), {res['input_MB']:.1f} MB in the buffers, "
          f"{res['output_MB']:.1f} MB out;  labels that differ from torch's: {100 * label_mismatch:.4f} %, max |image diff| {worst:.3g}")
    print(f"deeplabv3 training step {res['step_ms']:.1f} ms (spread {100 * res['step_spread']:.1f} %), with segmentation_train in front "
          f"{res['seg_step_ms']:.1f} ms (spread {100 * res['seg_step_spread']:.1f} %)")
    print("RESULT " + json.dumps(res))
    return 0 if label_mismatch <= 1e-2 and worst <= 1e-2 else 1          # a sanity check of the comparison, not a test of the kernel


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        sys.exit(child(int(sys.argv[2])))
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    r = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", str(B)],
                       stdout=subprocess.PIPE, text=True)
    sys.stdout.write(r.stdout)
    if r.returncode != 0:
        print(f"measurement failed (exit status {r.returncode})")
        sys.exit(r.returncode)
    print(json.dumps(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])))


if __name__ == "__main__":
    main()
