"""Label maps and top-k on the device against the path without them, timed in ONE process, alternating.
usage: time_postprocess.py fcn|deeplabv3 [BATCH] [SIZE]

(a) the path before `eqv.postprocess`: filter_jit(vmap(net)) writes the fp32 [B, classes, H, W] logits, then
    out.argmax(1).to(torch.uint8) reads them back (torch kernels);
(b) filter_jit(eqv.postprocess.segment): backbone + classifier + ONE label launch, the auxiliary head skipped.
Both run ROUNDS times in turn, STEPS steps per round between two device events; the figures are the median round and the spread
(min .. max) of the rounds, so a difference can be read against what the same code does from round to round.  The label maps of
the two paths are compared first.  Then the label kernel alone (GB/s of its stores: B H W bytes) and `topk` on [B, 1000] against
torch.softmax + torch.topk, the same way.  One JSON line per figure."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import eqxvision_amd as eqv
from eqxvision_amd import ops
from eqxvision_amd._act import wrap

ROUNDS, STEPS, WARMUP = 7, 10, 3


def timed(fn, steps):
    e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def alternate(fns, steps):
    """{name: [ms per step of every round]}: round r runs every function once, in turn."""
    for fn in fns.values():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    ms = {n: [] for n in fns}
    for _ in range(ROUNDS):
        for n, fn in fns.items():
            ms[n].append(timed(fn, steps))
    return ms


def figures(ms):
    return {"ms": round(statistics.median(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def main():
    kind = sys.argv[1]
    B = int(sys.argv[2]) if len(sys.argv) > 2 else 32
    size = int(sys.argv[3]) if len(sys.argv) > 3 else 224
    eqv.set_compute_dtype("bf16")
    build = {"fcn": eqv.models.fcn, "deeplabv3": eqv.models.deeplabv3}[kind]
    net = build(intermediate_layers=lambda m: [m.layer3, m.layer4], aux_in_channels=1024)
    net = eqv.tree_inference(eqv.utils.randomize_batchnorm(net, 1), True)
    x = torch.rand((B, 3, size, size), dtype=torch.float32).cuda()
    keys = eqv.random.split(eqv.random.PRNGKey(0), B)

    full = eqv.filter_jit(lambda n, im, k: eqv.vmap(n, axis_name="batch")(im, key=k), clone_outputs=False)
    seg = eqv.filter_jit(eqv.postprocess.segment, clone_outputs=False)
    path_a = lambda: full(net, x, keys)[1].argmax(1).to(torch.uint8)
    path_b = lambda: seg(net, x, key=keys)
    same = bool(torch.equal(path_a(), path_b()))
    ms = alternate({"a": path_a, "b": path_b}, STEPS)
    head = {"model": kind, "B": B, "size": size}
    print(json.dumps({**head, "what": "full logits + torch argmax (a)", **figures(ms["a"])}))
    print(json.dumps({**head, "what": "segment (b)", **figures(ms["b"]), "labels_equal": same}))

    # the label kernel alone, on the logits the head produces
    a = wrap(x, batched=True)
    k_backbone, k_clf, _ = eqv.random.split(keys, 3)
    logits = ops.as_map(net.classifier(net.backbone(a, key=k_backbone)[1][-1], key=k_clf)).t
    lab = alternate({"label": lambda: eqv.postprocess.upsample_argmax(logits, (size, size))}, 50)["label"]
    f = figures(lab)
    print(json.dumps({**head, "what": "label kernel alone", "logits": list(logits.shape), **f,
                      "store_GBps": round(B * size * size / (f["ms"] * 1e-3) / 1e9, 1)}))

    # top-k of [B, 1000] logits
    lg = torch.randn((B, 1000), dtype=torch.float32, device="cuda")

    def torch_topk():
        return torch.topk(torch.softmax(lg, dim=1), 5, dim=1)
    ms = alternate({"torch": torch_topk, "eqv": lambda: eqv.postprocess.topk(lg, 5)}, 200)
    ti, ei = torch_topk()[1], eqv.postprocess.topk(lg, 5)[1]
    print(json.dumps({"B": B, "K": 1000, "k": 5, "what": "torch.softmax + torch.topk", **figures(ms["torch"])}))
    print(json.dumps({"B": B, "K": 1000, "k": 5, "what": "eqv.postprocess.topk", **figures(ms["eqv"]),
                      "indices_equal": bool(torch.equal(ti.to(torch.int32), ei))}))


if __name__ == "__main__":
    main()
