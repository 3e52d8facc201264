"""The launchers execute what route.h says: for every kernel name of tests/data/routes.json the recorded call with the fewest
operand bytes is replayed (one launch each, uninitialised operands: the numbers are test_gpu_parity.py's and test_strict_gpu.py's
business) and `mv_last_kernel()` must give the recorded name.  Routing thresholds are on M and K, so the smallest row of a name is
the smallest shape at which that route can be taken at all."""
import ctypes as C
import json
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "data", "routes.json")) as _f:
    ROWS = json.load(_f)["rows"]

F32, BF16 = 0, 1


def _esize(dt):
    return 4 if dt == F32 else 2


def _operands(entry, a):
    """-> ([(bytes or None for a NULL pointer)] in pointer-argument order, the integer arguments)"""
    if entry in ("mv_conv2d_nhwc_fwd", "mv_conv2d_nhwc_grouped64_fwd"):
        N, H, W, Cc, K, R, S, sh, sw, ph, pw, dh, dw, groups, act, idt, odt = a[6:]
        M = N * ((H + 2 * ph - dh * (R - 1) - 1) // sh + 1) * ((W + 2 * pw - dw * (S - 1) - 1) // sw + 1)
        wc = Cc // groups if entry == "mv_conv2d_nhwc_fwd" else Cc + 64         # grouped64: the expanded window is at most C rounded up
        sizes = [N * H * W * Cc * _esize(idt), K * R * S * wc * _esize(idt), K * 4, K * 4, M * K * 4, M * K * _esize(odt)]
    elif entry in ("mv_linear_fwd", "mv_linear_split_fwd"):
        M, N, K, act, idt, odt = a[6:]
        sizes = [M * K * _esize(idt), N * K * _esize(idt) * (2 if entry == "mv_linear_split_fwd" else 1), N * 4, N * 4, M * N * 4,
                 M * N * _esize(odt)]
    elif entry == "mv_linear_heads_fwd":
        M, N, K = a[5:8]
        sizes = [M * K * 2, N * K * 2, N * 4, N * 4, M * N * 2]
    else:
        assert entry == "mv_conv1x1_dual_fwd", entry
        N, Ho, Wo, C1, H2, W2, C2, s2, K = a[6:15]
        sizes = [N * Ho * Wo * C1 * 2, N * H2 * W2 * C2 * 2, K * (C1 + C2) * 2, K * 4, K * 4, N * Ho * Wo * K * 2]
    n = len(sizes)
    return [sz if a[i] else None for i, sz in enumerate(sizes)], a[n:]


def _smallest_per_name():
    best = {}
    for row in ROWS:
        entry, args, flags, scratch, name = row
        if not name:
            continue
        nbytes = sum(s or 0 for s in _operands(entry, args)[0]) + scratch
        if name not in best or nbytes < best[name][0]:
            best[name] = (nbytes, row)
    return [best[k][1] for k in sorted(best)]


CASES = _smallest_per_name()


@pytest.mark.gpu
@pytest.mark.parametrize("row", CASES, ids=[r[4] for r in CASES])
def test_recorded_route_is_launched(row):
    import torch
    from eqxvision_amd import _lib
    from eqxvision_amd._act import stream_ptr
    entry, args, flags, scratch, name = row
    sizes, ints = _operands(entry, args)
    bufs = [None if s is None else torch.empty((s,), dtype=torch.uint8, device="cuda") for s in sizes]
    ptrs = [None if b is None else C.c_void_p(b.data_ptr()) for b in bufs]
    ws = torch.zeros((scratch,), dtype=torch.uint8, device="cuda") if scratch else None        # split-K arrival words start at zero
    st = stream_ptr()
    for k, v in flags.items():
        _lib.set_flag(k, v)
    try:
        if ws is not None:
            _lib.call("mv_set_scratch", C.c_void_p(ws.data_ptr()), scratch, st)
        _lib.call(entry, *ptrs, *ints, st)
        got = _lib.last_kernel()
        torch.cuda.synchronize()
    finally:
        _lib.call("mv_set_scratch", None, 0, st)
        for k in flags:
            _lib.set_flag(k, 0)
    assert got == name
