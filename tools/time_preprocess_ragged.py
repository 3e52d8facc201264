"""Times preprocessing of a batch of DIFFERENTLY sized images (eqxvision_amd.preprocess.imagenet_eval given a list) on one GPU.

    python tools/time_preprocess_ragged.py B          (default 256)

The batch is a fixed, seeded mix of the sizes 500x375, 375x500, 500x333, 333x500 and 640x480 (H x W), random pixels, bf16 NCHW
output.  Compared, alternating in one process (A B A B ..., median and spread over the rounds):
  loop  B single-image `imagenet_eval` calls with warm caches (device tap tables of every geometry already uploaded)
  list  one `imagenet_eval(list)` call: one packed upload, one table upload, one record upload, one launch
once with the images in host memory (numpy) and once with device-resident tensors; wall time per batch, synchronised before and
after.  Also the device time of the launches alone (events around them, every buffer prepared beforehand): the B launches of
`mv_preprocess_u8_fwd` against the one launch of `mv_preprocess_u8_ragged_fwd`; and where the host time of the list call goes
(building records and tables, packing and uploading, the rest).
The parent process never opens the GPU: each of the two measurements is a child process under its own `timeout`, and the second
is not started if the first fails.  One JSON line at the end."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(500, 375), (375, 500), (500, 333), (333, 500), (640, 480)]
ROUNDS, ITERS, LAUNCH_ITERS = 7, 3, 20
CHILD_LIMIT_S = 300


def child(mode, B):
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    import eqxvision_amd as eqv
    from eqxvision_amd import _lib
    from eqxvision_amd import preprocess as P

    rng = np.random.default_rng(0)
    sizes = [SIZES[i] for i in rng.integers(0, len(SIZES), B)]
    ims = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    if mode == "device":
        ims = [torch.from_numpy(im).cuda() for im in ims]
    kw = dict(dtype="bf16")

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

    def loop():
        return [eqv.preprocess.imagenet_eval(im, **kw) for im in ims]

    def one_list():
        return eqv.preprocess.imagenet_eval(ims, **kw)

    # the launches alone: every operand on the device beforehand
    resized = [P.resized_size(h, w, 256) for h, w in sizes]
    boxes = [P.center_crop_box(hr, wr, 224) for hr, wr in resized]
    a, b = P._device_affine(P.IMAGENET_MEAN, P.IMAGENET_STD)
    dev_ims = [im if isinstance(im, torch.Tensor) else torch.from_numpy(im).cuda() for im in ims]
    y1 = torch.empty((1, 3, 224, 224), dtype=torch.bfloat16, device="cuda")
    singles = []
    for t, (h, w), (hr, wr), (top, left, ho, wo) in zip(dev_ims, sizes, resized, boxes):
        th, tw, mh, mw = P._device_tables(h, w, hr, wr, top, left, ho, wo)
        singles.append((t.data_ptr(), y1.data_ptr(), th.data_ptr(), tw.data_ptr(), a.data_ptr(), b.data_ptr(), 1, h, w, hr, wr, top,
                        left, ho, wo, mh, mw, 0, _lib.BF16, 0, P.stream_ptr()))
    rec, tables, _ = P.ragged_plan(sizes, resized, boxes)
    x = P.pack_images(dev_ims)
    tab, rec_dev = torch.from_numpy(tables).cuda(), torch.from_numpy(rec.view(np.uint8)).cuda()
    yB = torch.empty((B, 3, 224, 224), dtype=torch.bfloat16, device="cuda")
    ragged = (x.data_ptr(), x.numel(), yB.data_ptr(), rec.ctypes.data, rec_dev.data_ptr(), tab.data_ptr(), tab.numel(), a.data_ptr(),
              b.data_ptr(), B, 224, 224, 0, _lib.BF16, 0, P.stream_ptr())

    def launches_loop():
        for s in singles:
            _lib.call("mv_preprocess_u8_fwd", *s)

    def launch_list():
        _lib.call("mv_preprocess_u8_ragged_fwd", *ragged)

    runs = {"loop": (wall, loop, ITERS), "list": (wall, one_list, ITERS),
            "loop_launches": (events, launches_loop, ITERS), "list_launch": (events, launch_list, LAUNCH_ITERS)}
    for _, f, _ in runs.values():              # warm: device tables of every geometry, the host axis cache, the allocator
        for _ in range(2):
            f()
    ms = {k: [] for k in runs}
    for _ in range(ROUNDS):
        for k, (timer, f, iters) in runs.items():
            ms[k].append(timer(f, iters))
    _lib.check_device_status()
    same = all(bool(torch.equal(o, q)) for o, q in zip(loop(), one_list()))

    def host_ms(fn, iters=5):                   # host-only pieces of the list call, warm cache
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        return (time.perf_counter() - t0) / iters * 1e3

    plan_ms = host_ms(lambda: P.ragged_plan(sizes, resized, boxes))
    check_ms = host_ms(lambda: P._check_list(ims, None))
    pack_ms = wall(lambda: P.pack_images(ims), 5)
    res = {"mode": mode, "B": B, "rounds": ROUNDS, "same_bits": same,
           "distinct_sizes": len(set(sizes)), "input_MB": sum(h * w * 3 for h, w in sizes) / 1e6,
           "plan_ms": plan_ms, "check_ms": check_ms, "pack_ms": pack_ms}
    for k, v in ms.items():
        res[k + "_ms"] = float(np.median(v))
        res[k + "_spread"] = float((max(v) - min(v)) / np.median(v))
    print(f"[{mode} images] loop of {B} calls {res['loop_ms']:.3f} ms (spread {100 * res['loop_spread']:.1f} %)   one list call "
          f"{res['list_ms']:.3f} ms (spread {100 * res['list_spread']:.1f} %)   x{res['loop_ms'] / res['list_ms']:.2f}")
    print(f"[{mode} images] launches alone: {B} x preprocess_u8 {res['loop_launches_ms']:.3f} ms, 1 x preprocess_u8_ragged "
          f"{res['list_launch_ms']:.3f} ms;  list call on the host: records + tables {plan_ms:.3f} ms, checks {check_ms:.3f} ms, "
          f"pack + upload {pack_ms:.3f} ms;  same bits: {same}")
    print("RESULT " + json.dumps(res))
    return 0 if same else 1


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        sys.exit(child(sys.argv[2], int(sys.argv[3])))
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    out = {}
    for mode in ("host", "device"):
        r = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", mode, str(B)],
                           stdout=subprocess.PIPE, text=True)
        sys.stdout.write(r.stdout)
        if r.returncode != 0:                   # a failed or timed-out GPU step: nothing more is started on the GPU
            print(f"{mode}: measurement failed (exit status {r.returncode}); stopping")
            sys.exit(r.returncode)
        out[mode] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
