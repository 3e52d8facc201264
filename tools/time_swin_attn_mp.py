"""The mixed-precision Swin window attention (csrc/swin_attn_mp.hip) alone, against what the fp32 path of grad.g_swin_window_attention
launches:
    fwd    mv_swin_attn_mp_fwd                    vs  mv_swin_window_attn_fwd in fp32 mode
    bwd    mv_swin_attn_mp_bwd (with its parts)   vs  mv_swin_window_attn_bwd_f32 (which writes a [B nW, heads n n] scratch)
    both   the two in sequence, as a training step runs them
at swin_t's four stages (maps 56 / 28 / 14 / 7, C 96 / 192 / 384 / 768, heads 3 / 6 / 12 / 24, window 7), shift 0 and 3, for B in {4, 64},
Gaussian operands.  Both sides alternate in one process: ROUNDS rounds of (REPS launches of one side, REPS of the other) between
device events; the figure is the median over the rounds, the spread their min .. max.  The column sum over the fp32 side's scratch
and over the bf16 side's parts is timed with neither (both sides launch one).
usage: time_swin_attn_mp.py [ROUNDS=7] [REPS=10] [--batches 4,64]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from eqxvision_amd import _lib

argv = list(sys.argv[1:])
BATCHES = (4, 64)
if "--batches" in argv:
    i = argv.index("--batches")
    BATCHES = tuple(int(v) for v in argv[i + 1].split(","))
    del argv[i:i + 2]
ROUNDS = int(argv[0]) if len(argv) > 0 else 7
REPS = int(argv[1]) if len(argv) > 1 else 10
STAGES = ((56, 96, 3), (28, 192, 6), (14, 384, 12), (7, 768, 24))      # (map, C, heads)
WS = 7


def main():
    dev = torch.device("cuda")
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()
    lib = _lib.load()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(REPS):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / REPS          # us per launch group

    print(f"window {WS}, dh 32; rounds {ROUNDS}, launches per round {REPS}")
    print(f"{'B':>3s} {'map':>3s} {'C':>4s} {'sh':>2s} {'P':>4s} {'entry':5s} {'fp32 us':>10s} {'bf16 us':>10s} {'fp32 spread':>19s} {'bf16 spread':>19s} {'speed-up':>9s}")
    for B in BATCHES:
        for Hf, C, heads in STAGES:
            for sh in (0, 3):
                g = torch.Generator(device="cpu").manual_seed(1)
                n, nW, scale = WS * WS, (Hf // WS) ** 2, float((C // heads) ** -0.5)
                qkv = torch.randn((B, Hf, Hf, 3 * C), generator=g).to(dev)
                dout = torch.randn((B, Hf, Hf, C), generator=g).to(dev)
                bias = (0.5 * torch.randn((heads, n, n), generator=g)).to(dev)
                out32, out16 = torch.empty((B, Hf, Hf, C), device=dev), torch.empty((B, Hf, Hf, C), device=dev)
                lse = torch.empty((B * nW, heads, n), device=dev)
                gw = torch.empty((B * nW, heads * n * n), device=dev)
                P = lib.mv_swin_attn_mp_bwd_parts(B, Hf, Hf, heads, WS, WS)
                parts = torch.empty((P, heads * n * n), device=dev)
                dq32, dq16 = torch.empty((B, Hf, Hf, 3 * C), device=dev), torch.empty((B, Hf, Hf, 3 * C), device=dev)
                ga = (B, Hf, Hf, C, heads, WS, WS, sh, sh)

                fwd32 = lambda: _lib.call("mv_swin_window_attn_fwd", p(qkv), p(bias), p(out32), *ga, _lib.F32, st)
                bwd32 = lambda: _lib.call("mv_swin_window_attn_bwd_f32", p(qkv), p(bias), p(dout), p(dq32), p(gw), *ga, st)
                fwd16 = lambda: _lib.call("mv_swin_attn_mp_fwd", p(qkv), p(bias), p(out16), p(lse), *ga, scale, st)
                bwd16 = lambda: _lib.call("mv_swin_attn_mp_bwd", p(qkv), p(bias), p(out16), p(dout), p(lse), p(dq16), p(parts), *ga, scale, st)
                sides = {"fwd": (fwd32, fwd16), "bwd": (bwd32, bwd16), "both": (lambda: (fwd32(), bwd32()), lambda: (fwd16(), bwd16()))}
                for entry, (f32, f16) in sides.items():
                    f32(); f16()
                    torch.cuda.synchronize()
                    t32, t16 = [], []
                    for _ in range(ROUNDS):
                        t32.append(timed(f32))
                        t16.append(timed(f16))
                    m32, m16 = float(np.median(t32)), float(np.median(t16))
                    print(f"{B:3d} {Hf:3d} {C:4d} {sh:2d} {P:4d} {entry:5s} {m32:10.1f} {m16:10.1f} {min(t32):9.1f}..{max(t32):<9.1f} "
                          f"{min(t16):9.1f}..{max(t16):<9.1f} {m32 / m16:8.2f}x", flush=True)
                rel = float((dq16 - dq32).norm() / dq32.norm())
                relb = float((parts.sum(0) - gw.sum(0)).norm() / gw.sum(0).norm())
                print(f"{B:3d} {Hf:3d} {C:4d} {sh:2d} check relative L2, bf16 pair against fp32 pair: dqkv {rel:.2e}, dbias {relb:.2e}; "
                      f"bias-gradient scratch {gw.numel() * 4 / 2 ** 20:.1f} MiB -> parts {parts.numel() * 4 / 2 ** 20:.1f} MiB", flush=True)
    _lib.check_device_status()


if __name__ == "__main__":
    main()
