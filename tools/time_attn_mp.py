"""The mixed-precision attention core (csrc/attn_mp.hip) alone, against what the fp32 path of grad.g_qkv_attention launches:
    fwd    mv_mha_mp_fwd (probs = NULL)  vs  mv_mha_fwd fp32 (which always writes probs [B, H, N, N])
    bwd    mv_mha_mp_bwd                 vs  mv_mha_bwd_f32 (two launches, a [B, H, N, N] scratch)
    both   the two in sequence, as a training step runs them
at ViT-B's head shape (N = 197, dh = 64, H = 12) for B in {4, 32, 64}, Gaussian operands.  Both sides alternate in one process: ROUNDS
rounds of (REPS launches of one side, REPS of the other) between device events; the figure is the median over the rounds, the spread
their min .. max.  --parts P forces the backward's workgroups per (image, head) (the library's `mha_mp_bwd_parts` debug switch; 0 = the product's single workgroup).
usage: time_attn_mp.py [ROUNDS=7] [REPS=20] [--parts P]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from eqxvision_amd import _lib

argv = list(sys.argv[1:])
PARTS = 0
if "--parts" in argv:
    i = argv.index("--parts")
    PARTS = int(argv[i + 1])
    del argv[i:i + 2]
ROUNDS = int(argv[0]) if len(argv) > 0 else 7
REPS = int(argv[1]) if len(argv) > 1 else 20
N, H, DH = 197, 12, 64
BATCHES = (4, 32, 64)


def main():
    dev = torch.device("cuda")
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()
    scale = DH ** -0.5
    _lib.set_flag("mha_mp_bwd_parts", PARTS)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPS):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / REPS          # us per launch group

    print(f"N = {N}, H = {H}, dh = {DH}; backward workgroups per (image, head): {PARTS or 1}")
    print(f"{'B':>4s} {'entry':5s} {'fp32 us':>10s} {'bf16 us':>10s} {'fp32 spread':>19s} {'bf16 spread':>19s} {'speed-up':>9s}")
    for B in BATCHES:
        g = torch.Generator(device="cpu").manual_seed(1)
        D = H * DH
        qkv = torch.randn((B, N, 3 * D), generator=g).to(dev)
        dout = torch.randn((B, N, D), generator=g).to(dev)
        out32, out16 = torch.empty((B, N, D), device=dev), torch.empty((B, N, D), device=dev)
        probs, ds = torch.empty((B, H, N, N), device=dev), torch.empty((B, H, N, N), device=dev)
        lse = torch.empty((B, H, N), device=dev)
        dq32, dq16 = torch.empty((B, N, 3 * D), device=dev), torch.empty((B, N, 3 * D), device=dev)

        fwd32 = lambda: _lib.call("mv_mha_fwd", p(qkv), p(out32), p(probs), B, N, H, DH, scale, _lib.F32, st)
        bwd32 = lambda: _lib.call("mv_mha_bwd_f32", p(qkv), p(probs), p(dout), p(ds), p(dq32), B, N, H, DH, scale, st)
        fwd16 = lambda: _lib.call("mv_mha_mp_fwd", p(qkv), p(out16), p(lse), None, B, N, H, DH, scale, st)
        bwd16 = lambda: _lib.call("mv_mha_mp_bwd", p(qkv), p(out16), p(dout), p(lse), p(dq16), B, N, H, DH, scale, st)
        sides = {"fwd": (fwd32, fwd16), "bwd": (bwd32, bwd16), "both": (lambda: (fwd32(), bwd32()), lambda: (fwd16(), bwd16()))}
        for entry, (f32, f16) in sides.items():
            f32(); f16()
            torch.cuda.synchronize()
            t32, t16 = [], []
            for _ in range(ROUNDS):
                t32.append(timed(f32))
                t16.append(timed(f16))
            m32, m16 = float(np.median(t32)), float(np.median(t16))
            print(f"{B:4d} {entry:5s} {m32:10.1f} {m16:10.1f} {min(t32):9.1f}..{max(t32):<9.1f} {min(t16):9.1f}..{max(t16):<9.1f} {m32 / m16:8.2f}x")
        rel = float((dq16 - dq32).norm() / dq32.norm())
        print(f"{B:4d} check relative L2 of dqkv, bf16 pair against fp32 pair: {rel:.2e}")
    _lib.set_flag("mha_mp_bwd_parts", 0)
    _lib.check_device_status()


if __name__ == "__main__":
    main()
