"""The confusion matrix of a validation batch on the device, timed in ONE process, alternating.
usage: time_metrics.py fcn|deeplabv3 [BATCH] [SIZE]

On the head logits of the model at [BATCH, 3, SIZE, SIZE] and labels with 255 in a border (preprocess.segmentation_eval's padding):
(a) ConfusionMatrix.update_logits_fused: one launch, neither logits nor labels at full resolution are written;
(b) ConfusionMatrix.update_logits as shipped -- postprocess.upsample_argmax's launch, then ConfusionMatrix.update's: the uint8
    label map in between;
(c) the route before `eqv.metrics`: the label map, then torch.bincount on the device (c1), or the map fetched and numpy.bincount
    on the host (c2).
All run ROUNDS times in turn, STEPS steps per round between two device events (c2: wall clock, it synchronises); the figures are
the median round and the spread (min .. max).  The matrices of all paths are compared first.  Then the counter placements of the
kernel (`confusion_mode`: global / one LDS histogram / one per wave) on label maps of 21, 64 and 128 classes, uniform regions and
random labels, and `TopK.update` on [BATCH, 1000] against torch.topk + compare.  One JSON line per figure."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import eqxvision_amd as eqv
from eqxvision_amd import _lib, ops
from eqxvision_amd._act import wrap

ROUNDS, STEPS, WARMUP = 7, 20, 3


def timed(fn, steps):
    e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def wall(fn, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def alternate(fns, steps, clock=timed):
    """{name: [ms per step of every round]}: round r runs every function once, in turn."""
    for fn in fns.values():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    ms = {n: [] for n in fns}
    for _ in range(ROUNDS):
        for n, fn in fns.items():
            ms[n].append(clock(fn, steps))
    return ms


def figures(ms):
    return {"ms": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def main():
    kind = sys.argv[1]
    B = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    size = int(sys.argv[3]) if len(sys.argv) > 3 else 520
    C = 21
    eqv.set_compute_dtype("bf16")
    build = {"fcn": eqv.models.fcn, "deeplabv3": eqv.models.deeplabv3}[kind]
    net = build(num_classes=C, intermediate_layers=lambda m: [m.layer3, m.layer4], aux_in_channels=1024)
    net = eqv.tree_inference(eqv.utils.randomize_batchnorm(net, 1), True)
    x = torch.rand((B, 3, size, size), dtype=torch.float32).cuda()
    keys = eqv.random.split(eqv.random.PRNGKey(0), B)
    k_backbone, k_clf, _ = eqv.random.split(keys, 3)
    logits = ops.as_map(net.classifier(net.backbone(wrap(x, batched=True), key=k_backbone)[1][-1], key=k_clf)).t
    # targets: blocks of 40 x 40 pixels of one class, a 20-pixel border of 255
    rng = np.random.default_rng(0)
    blocks = rng.integers(0, C, (B, (size + 39) // 40, (size + 39) // 40)).astype(np.uint8)
    lab = np.kron(blocks, np.ones((40, 40), np.uint8))[:, :size, :size].copy()
    lab[:, :20], lab[:, -20:], lab[:, :, :20], lab[:, :, -20:] = 255, 255, 255, 255
    labels = torch.from_numpy(lab).cuda()
    cm = eqv.metrics.ConfusionMatrix(C)

    def path_a():
        cm.update_logits_fused(logits, labels)

    def path_b():
        cm.update(eqv.postprocess.upsample_argmax(logits, (size, size)), labels)

    def bincount_device():
        pred = eqv.postprocess.upsample_argmax(logits, (size, size))
        keep = labels < C
        return torch.bincount(labels[keep].to(torch.int64) * C + pred[keep].to(torch.int64), minlength=C * C).reshape(C, C)

    def bincount_host():
        pred = eqv.postprocess.upsample_argmax(logits, (size, size)).cpu().numpy()
        keep = lab < C
        return np.bincount(lab[keep].astype(np.int64) * C + pred[keep], minlength=C * C).reshape(C, C)

    mats = []
    for fn in (path_a, path_b):
        cm.reset()
        fn()
        mats.append(cm.mat.cpu().numpy().copy())
    mats += [bincount_device().cpu().numpy(), bincount_host()]
    same = all(np.array_equal(mats[0], m) for m in mats[1:])
    head = {"model": kind, "B": B, "size": size, "logits": list(logits.shape), "classes": C}
    ms = alternate({"a": path_a, "b": path_b, "c1": bincount_device}, STEPS)
    print(json.dumps({**head, "what": "update_logits_fused, one launch (a)", **figures(ms["a"]), "matrices_equal": same}))
    print(json.dumps({**head, "what": "upsample_argmax + update = update_logits (b)", **figures(ms["b"])}))
    print(json.dumps({**head, "what": "upsample_argmax + torch.bincount on the device (c1)", **figures(ms["c1"])}))
    ms = alternate({"c2": bincount_host}, 2, clock=wall)
    print(json.dumps({**head, "what": "upsample_argmax + fetch + numpy.bincount (c2, wall clock)", **figures(ms["c2"])}))

    # counter placements: the counting stage alone, on label maps
    n = B * size * size
    for classes in (21, 64, 128):
        for data in ("regions", "random"):
            if data == "regions":
                t = torch.from_numpy(np.kron(rng.integers(0, classes, (n // 4096 + 1,)).astype(np.uint8), np.ones(4096, np.uint8))[:n]).cuda()
                p = torch.roll(t, 1000)
            else:
                t = torch.from_numpy(rng.integers(0, classes, (n,)).astype(np.uint8)).cuda()
                p = torch.from_numpy(rng.integers(0, classes, (n,)).astype(np.uint8)).cuda()
            m = eqv.metrics.ConfusionMatrix(classes)
            fns, names = {}, {1: "global", 2: "lds", 3: "lds per wave"}

            def make(mode):
                def run():
                    _lib.set_flag("confusion_mode", mode)
                    m.update(p, t)
                return run
            for mode in (1, 2, 3):
                if mode == 3 and 16 * classes * classes > 65536:
                    continue
                fns[names[mode]] = make(mode)
            ms = alternate(fns, STEPS)
            _lib.set_flag("confusion_mode", 0)
            for name, v in ms.items():
                print(json.dumps({"what": f"update, counters: {name}", "classes": classes, "labels": data, "n": n, **figures(v),
                                  "GBps": round(2 * n / (statistics.median(v) * 1e-3) / 1e9, 1)}))

    # top-k accuracy of [B, 1000] logits
    lg = torch.randn((B, 1000), dtype=torch.float32, device="cuda")
    tl = torch.randint(0, 1000, (B,), dtype=torch.int32, device="cuda")
    acc = eqv.metrics.TopK((1, 5))

    def torch_topk():
        hit = torch.topk(lg, 5, dim=1)[1] == tl[:, None].to(torch.int64)
        return hit[:, :1].sum(), hit.sum()
    ms = alternate({"torch": torch_topk, "eqv": lambda: acc.update(lg, tl)}, 200)
    acc.reset()
    acc.update(lg, tl)
    t1, t5 = (int(v) for v in torch_topk())
    print(json.dumps({"B": B, "K": 1000, "what": "torch.topk + compare", **figures(ms["torch"])}))
    print(json.dumps({"B": B, "K": 1000, "what": "metrics.TopK.update", **figures(ms["eqv"]),
                      "counts_equal": acc.counts.cpu().numpy().tolist() == [t1, t5, B]}))


if __name__ == "__main__":
    main()
