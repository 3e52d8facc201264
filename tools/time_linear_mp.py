"""The three mixed-precision Linear entries (csrc/linear_mp.hip) alone, against what the fp32 path of grad.g_linear launches for the
same product:
    fwd    mv_linear_mp_fwd    vs  mv_linear_fwd fp32
    wgrad  mv_linear_mp_wgrad  vs  two mv_transpose2d_f32 + mv_linear_fwd fp32          (both with the backward's scratch on offer)
    dgrad  mv_linear_mp_dgrad  vs  mv_linear_fwd fp32 on the pre-transposed weight      (the transpose is cached per step: not timed)
Shapes: ViT-B/16's four Linears at M = 4 x 197 and 64 x 197, swin_t's stage-2 Linears at B = 64 (28 x 28 tokens, C = 192).
Both sides alternate in one process: ROUNDS rounds of (REPS launches of one side, REPS of the other) between device events; the
figure is the median over the rounds, the spread their min .. max.
usage: time_linear_mp.py [ROUNDS=7] [REPS=20]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from eqxvision_amd import _lib

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 20
F32, NONE = _lib.F32, _lib.ACT_NONE
SCRATCH = 64 << 20

VIT = [("qkv", 768, 2304), ("proj", 768, 768), ("fc1", 768, 3072), ("fc2", 3072, 768)]
SWIN2 = [("qkv", 192, 576), ("proj", 192, 192), ("fc1", 192, 768), ("fc2", 768, 192)]
CASES = [(f"vit_b/{n}/M{4 * 197}", 4 * 197, N, K) for n, K, N in VIT] + [(f"vit_b/{n}/M{64 * 197}", 64 * 197, N, K) for n, K, N in VIT] + \
        [(f"swin_t.s2/{n}/M{64 * 784}", 64 * 784, N, K) for n, K, N in SWIN2]


def main():
    dev = torch.device("cuda")
    st = torch.cuda.current_stream().cuda_stream
    ws = torch.zeros(SCRATCH, dtype=torch.uint8, device=dev)
    p = lambda t: t.data_ptr()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPS):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / REPS          # us per launch group

    print(f"{'case':28s} {'entry':6s} {'fp32 us':>10s} {'bf16 us':>10s} {'fp32 spread':>17s} {'bf16 spread':>17s} {'speed-up':>9s}  kernel")
    for tag, M, N, K in CASES:
        g = torch.Generator(device="cpu").manual_seed(1)
        x = torch.randn((M, K), generator=g).to(dev)
        w = (torch.randn((N, K), generator=g) / K ** 0.5).to(dev)
        gy = torch.randn((M, N), generator=g).to(dev)
        bias = torch.randn((N,), generator=g).to(dev)
        wt = w.t().contiguous()
        y, dx, dw = torch.empty((M, N), device=dev), torch.empty((M, K), device=dev), torch.empty((N, K), device=dev)
        gT, xT = torch.empty((N, M), device=dev), torch.empty((K, M), device=dev)

        def offer():
            _lib.call("mv_set_scratch", p(ws), SCRATCH, st)

        def wgrad32():
            _lib.call("mv_transpose2d_f32", p(gy), p(gT), M, N, 0, st)
            _lib.call("mv_transpose2d_f32", p(x), p(xT), M, K, 0, st)
            _lib.call("mv_linear_fwd", p(gT), p(xT), None, None, None, p(dw), N, K, M, NONE, F32, F32, st)

        def wgrad16():
            offer()
            _lib.call("mv_linear_mp_wgrad", p(gy), p(x), p(dw), M, N, K, st)

        sides = {
            "fwd": (lambda: _lib.call("mv_linear_fwd", p(x), p(w), None, p(bias), None, p(y), M, N, K, NONE, F32, F32, st),
                    lambda: _lib.call("mv_linear_mp_fwd", p(x), p(w), p(bias), p(y), M, N, K, st)),
            "wgrad": (wgrad32, wgrad16),
            "dgrad": (lambda: _lib.call("mv_linear_fwd", p(gy), p(wt), None, None, None, p(dx), M, K, N, NONE, F32, F32, st),
                      lambda: _lib.call("mv_linear_mp_dgrad", p(gy), p(w), p(dx), M, N, K, st)),
        }
        for entry, (f32, f16) in sides.items():
            f32(); f16()
            kern = _lib.last_kernel()
            torch.cuda.synchronize()
            t32, t16 = [], []
            for _ in range(ROUNDS):
                t32.append(timed(f32))
                t16.append(timed(f16))
            m32, m16 = float(np.median(t32)), float(np.median(t16))
            print(f"{tag:28s} {entry:6s} {m32:10.1f} {m16:10.1f} {min(t32):8.1f}..{max(t32):<8.1f} {min(t16):8.1f}..{max(t16):<8.1f} "
                  f"{m32 / m16:8.2f}x  {kern}")
        _lib.call("mv_set_scratch", None, 0, st)
    _lib.check_device_status()


if __name__ == "__main__":
    main()
