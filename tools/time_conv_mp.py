"""The three mixed-precision Conv2d entries (csrc/conv_mp.hip) alone, against what the default path of grad.g_conv2d launches for the
same product:
    fwd    mv_conv2d_mp_fwd    vs  mv_conv2d_nhwc_fwd fp32
    dgrad  mv_conv2d_mp_dgrad  vs  mv_conv2d_dgrad_nhwc_f32
    wgrad  mv_conv2d_mp_wgrad  vs  mv_conv2d_wgrad_nhwc_f32        (both with the backward's scratch on offer)
Shapes: resnet50's 3x3 convolutions of layers 1 to 4, its 7x7 / 2 stem, the strided 1x1 shortcut of layer 2, deeplabv3's dilated 3x3 of
layer 4 at 65 x 65; each at B = 4 and B = 32.
Both sides alternate in one process: ROUNDS rounds of (REPS launches of one side, REPS of the other) between device events; the
figure is the median over the rounds, the spread their min .. max.
usage: time_conv_mp.py [ROUNDS=5] [REPS=10] [B,B,...=4,32]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from eqxvision_amd import _lib

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
BATCHES = [int(b) for b in sys.argv[3].split(",")] if len(sys.argv) > 3 else [4, 32]
F32, NONE = _lib.F32, _lib.ACT_NONE
SCRATCH = 64 << 20

# (name, H, W, C, K, R, S, stride, pad, dil)
SHAPES = [
    ("r50.layer1/3x3", 56, 56, 64, 64, 3, 3, 1, 1, 1),
    ("r50.layer2/3x3", 28, 28, 128, 128, 3, 3, 1, 1, 1),
    ("r50.layer3/3x3", 14, 14, 256, 256, 3, 3, 1, 1, 1),
    ("r50.layer4/3x3", 7, 7, 512, 512, 3, 3, 1, 1, 1),
    ("r50.stem/7x7s2", 224, 224, 3, 64, 7, 7, 2, 3, 1),
    ("r50.layer2/1x1s2", 56, 56, 256, 512, 1, 1, 2, 0, 1),
    ("dlv3.layer4/3x3d4", 65, 65, 512, 512, 3, 3, 1, 4, 4),
]


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

    print(f"{'case':26s} {'entry':6s} {'fp32 us':>10s} {'bf16 us':>10s} {'fp32 spread':>19s} {'bf16 spread':>19s} {'speed-up':>9s}  kernels")
    for B in BATCHES:
        for name, H, W, C, K, R, S, s, pd, d in SHAPES:
            Ho, Wo = (H + 2 * pd - d * (R - 1) - 1) // s + 1, (W + 2 * pd - d * (S - 1) - 1) // s + 1
            g = torch.Generator(device="cpu").manual_seed(1)
            x = torch.randn((B, H, W, C), generator=g).to(dev)
            w = (torch.randn((K, R, S, C), generator=g) / (R * S * C) ** 0.5).to(dev)
            dy = torch.randn((B, Ho, Wo, K), generator=g).to(dev)
            bias = torch.randn((K,), generator=g).to(dev)
            y, dx, dw = torch.empty_like(dy), torch.empty_like(x), torch.empty_like(w)
            geom = (B, H, W, C, K, R, S, s, s, pd, pd, d, d)

            def offer():
                _lib.call("mv_set_scratch", p(ws), SCRATCH, st)

            def wgrad32():
                offer()
                _lib.call("mv_conv2d_wgrad_nhwc_f32", p(x), p(dy), p(dw), *geom, 1, st)

            def wgrad16():
                offer()
                _lib.call("mv_conv2d_mp_wgrad", p(x), p(dy), p(dw), *geom, st)

            sides = {
                "fwd": (lambda: _lib.call("mv_conv2d_nhwc_fwd", p(x), p(w), None, p(bias), None, p(y), *geom, 1, NONE, F32, F32, st),
                        lambda: _lib.call("mv_conv2d_mp_fwd", p(x), p(w), p(bias), p(y), *geom, st)),
                "dgrad": (lambda: _lib.call("mv_conv2d_dgrad_nhwc_f32", p(dy), p(w), p(dx), *geom, 1, st),
                          lambda: _lib.call("mv_conv2d_mp_dgrad", p(dy), p(w), p(dx), *geom, st)),
                "wgrad": (wgrad32, wgrad16),
            }
            for entry, (f32, f16) in sides.items():
                f32()
                k32 = _lib.last_kernel()
                f16()
                k16 = _lib.last_kernel()
                torch.cuda.synchronize()
                t32, t16 = [], []
                for _ in range(ROUNDS):
                    t32.append(timed(f32))
                    t16.append(timed(f16))
                m32, m16 = float(np.median(t32)), float(np.median(t16))
                print(f"{name + '/B' + str(B):26s} {entry:6s} {m32:10.1f} {m16:10.1f} {min(t32):9.1f}..{max(t32):<9.1f} {min(t16):9.1f}..{max(t16):<9.1f} "
                      f"{m32 / m16:8.2f}x  {k32} | {k16}", flush=True)
            _lib.call("mv_set_scratch", None, 0, st)
            del x, w, dy, y, dx, dw
    _lib.check_device_status()


if __name__ == "__main__":
    main()
