"""swin_v2_t at 256 px under filter_jit(lanes=2): the fused V2 lowering against the library switch "no_swin_v2_fused", alternating
inside ONE process (box-to-box variance is +-3%; bench.py runs its models at 224 px, which is not a multiple of the 8 x 8 window).
usage: time_swin_v2.py [B] [repeats]  -> images/s per repeat and variant, then the median and the spread of each."""
import os
import statistics
import sys
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import eqxvision_amd as eqv
from eqxvision_amd import _lib

B = int(sys.argv[1]) if len(sys.argv) > 1 else 64
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
STEPS = 20
eqv.set_compute_dtype("bf16")
with warnings.catch_warnings():
    warnings.simplefilter("ignore")
    net = eqv.tree_inference(eqv.models.swin_v2_t(), True)
images = torch.rand((B, 3, 256, 256), dtype=torch.float32).cuda()
keys = eqv.random.split(eqv.random.PRNGKey(0), B)
fw = {}
for v in (0, 1):
    _lib.set_flag("no_swin_v2_fused", v)
    fw[v] = eqv.filter_jit(lambda n, im, k: eqv.vmap(n, axis_name="batch")(im, key=k), use_graph=True, clone_outputs=False, lanes=2)
    for _ in range(4):
        fw[v](net, images, keys)
torch.cuda.synchronize()
rate = {0: [], 1: []}
for r in range(reps):
    for v in (0, 1):
        _lib.set_flag("no_swin_v2_fused", v)           # the jit cache keys on the switch settings
        e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
        e0.record()
        for _ in range(STEPS):
            fw[v](net, images, keys)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / STEPS
        rate[v].append(B / ms * 1e3)
        print(f"no_swin_v2_fused={v}: {ms:.4f} ms/step  {rate[v][-1]:.0f} img/s", flush=True)
_lib.set_flag("no_swin_v2_fused", 0)
for v, name in ((0, "fused"), (1, "literal")):
    print(f"{name}: median {statistics.median(rate[v]):.0f} img/s, spread {min(rate[v]):.0f} - {max(rate[v]):.0f} over {reps} repeats (B = {B})")
