"""`-m gpu`: exact and per-element checks of mv_swin_block_attn_fwd -- y = x + proj(window_attention(qkv(LayerNorm(x)))) in one
launch -- at its four kernels: swin_block_attn_c384, swin_block_attn_c192, swin_block_attn_c96 (flag swin_c96_shared) and swin_win96.
Instruments, derivations, facts from the source (and the SUPPOSED ones) and the case table: tests/_strict_swinblock.py; the CPU
proof that the instruments see each seeded defect: tests/test_strict_swinblock_host.py.

Every test calls the C ABI entry with operands laid out by ops.swin_block_attn_fragments, writes into a sentinel-filled destination
with a guard behind it, names the kernel it must reach (`_lib.last_kernel()`), and prints its figures (`pytest -s`): exact -> the
number of wrong elements; bound -> the worst |got - ref| / bound and the violations.  The rounding-bias rule does not apply (fp32
output).

Shapes: 14 x 14 (4 windows), 14 x 21 and 21 x 14 (6 windows, nWw != nWh, a window pair across two window rows), 21 x 21 (9 windows, an
interior window without mask; one-window kernels only -- the two-window kernels must refuse it), B = 2; shifts (0, 0), (3, 3) and, on
the rectangular maps, (2, 5).

Measured on an MI355X: worst |got - ref| / bound per kernel over all its cases, next to the CPU emulation's figure at its one case
(14 x 21, shifts (2, 5)) in brackets.  a-select, a-tie and b: 0 wrong elements in every case of every kernel.
    kernel                 a-flat          a-mask          b-soft          gauss
    swin_block_attn_c384   0.800 (0.595)   0.777 (0.595)   0.443 (0.447)   0.001 (0.001)
    swin_block_attn_c192   0.792 (0.785)   0.792 (0.785)   0.448 (0.349)   0.002 (0.002)
    swin_block_attn_c96    0.696 (0.676)   0.675 (0.676)   0.440 (0.390)   0.006 (0.004)
    swin_win96             0.696 (0.676)   0.675 (0.676)   0.440 (0.390)   0.006 (0.004)
No bound was violated, every guard was intact and no sentinel was left inside an output.  The SUPPOSED facts held (__expf(0) = 1,
__expf(<= -128) = 0, 1.f / 1.f = 1 and 1.f / 2.f = 0.5: every select and tie case is bit-equal).  No kernel body had to be changed.
The entry was: mv_swin_block_attn_supported refused C = 96 maps with an odd window count (21 x 21) although swin_win96, the default,
runs one window per workgroup; the pairing requirement now applies to C = 96 only under swin_c96_shared.
"""
import numpy as np
import pytest
import torch

from eqxvision_amd import _lib, ops
from tests import _strict_swinblock as W
from tests._slices import GUARD, SENTINEL, _dest, _read
from tests._strict_gpu import _dev, _Flags, _need_gpu, _p, _stream  # noqa: F401  (_need_gpu: the module fixture)

pytestmark = pytest.mark.gpu

F64 = np.float64
assert W.SENTINEL == SENTINEL
MV_E_INVALID, MV_E_UNSUPPORTED = -1, -2


def _operands(op):
    wf, bq, wpf, b64 = ops.swin_block_attn_fragments(np.asarray(op["wqkv"]), np.asarray(op["bqkv"]), np.asarray(op["wp"]), np.asarray(op["bias"]))
    return [_dev(np.array(op["x"]), "fp32"), _dev(wf, "bf16"), _dev(bq, "fp32"), _dev(wpf, "bf16"), _dev(np.array(op["bp"]), "fp32"),
            _dev(b64, "fp32")]


def _launch(kernel, op, tag):
    C, _, flags, _ = W.KERNELS[kernel]
    B, Hf, Wf, shh, shw = op["geom"]
    M = B * Hf * Wf
    d = _operands(op)
    y = _dest(M, C, torch.float32)
    with _Flags(flags):
        assert _lib.load().mv_swin_block_attn_supported(Hf, Wf, C, C // 32, 7, 7, _lib.F32) == 1, tag
        _lib.call("mv_swin_block_attn_fwd", _p(d[0]), _p(d[1]), _p(d[2]), _p(d[3]), _p(d[4]), _p(d[5]), _p(y), B, Hf, Wf, C, C // 32, 7, 7,
                  shh, shw, W.EPS, _lib.F32, _stream())
        kern = _lib.last_kernel()
    torch.cuda.synchronize()
    body, guard = _read(y, M, C)
    assert guard.numel() == GUARD and bool((guard == SENTINEL).all()), f"{tag}: guard behind the destination overwritten"
    return body.numpy().astype(F64), kern


def _judge(kernel, name, op, tag):
    got, kern = _launch(kernel, op, tag)
    info = W.check(op, got)
    if op["bound"] is None:
        print(f"{tag} [{kern}]: exact {info['ok']}, wrong {info.get('nbad')} of {info.get('n')}, sentinels left {info['left']}")
    else:
        print(f"{tag} [{kern}]: worst |got-ref|/bound {info.get('worst', float('nan')):.3f} over {info.get('n')} elements, "
              f"violations {info.get('nviol')}, sentinels left {info['left']}")
    assert kern == kernel, f"{tag}: served by {kern!r}, expected {kernel!r}"
    assert info["left"] == 0, f"{tag}: {info['left']} sentinel values left inside the output"
    assert info["ok"], f"{tag}: {info}"


@pytest.mark.parametrize("case", W.CASES, ids=W.case_id)
def test_exact_by_bias(case):
    """Form (a): +-1 rows, logits from the bias alone, integer v and proj.  select and tie: bit equality with x + Wp v[pi(i)] + bp (or
    the tie's average); flat, and mask on shifted maps: the region mean within the derived bound."""
    kernel, geom = case
    for kind in W.KINDS_A:
        if kind == "mask" and geom[3] + geom[4] == 0:
            continue
        _judge(kernel, kind, W.exact_a(kernel, geom, kind), f"swinblock/a-{kind}/{W.case_id(case)}")


@pytest.mark.parametrize("case", W.CASES, ids=W.case_id)
def test_exact_by_codes(case):
    """Form (b): the codes ride in the +-1 rows; the q . k path, the scale, the mask and the head pairing decide the winner, one
    permutation per (image, window, head): bit equality.  Then the same rows at gain 1: a real softmax over exact operands, bounded."""
    kernel, geom = case
    _judge(kernel, "b", W.exact_b(kernel, geom), f"swinblock/b/{W.case_id(case)}")
    _judge(kernel, "b-soft", W.exact_b(kernel, geom, True), f"swinblock/b-soft/{W.case_id(case)}")


@pytest.mark.parametrize("case", W.CASES, ids=W.case_id)
def test_bound(case):
    """Gaussian rows (offset rows, one constant row), folded gamma / beta, against float64 on the kernel's own operands: every
    element within the bound composed through LayerNorm, qkv, the softmax, P . V, the two bf16 packs, proj and the residual."""
    kernel, geom = case
    _judge(kernel, "gauss", W.gauss(kernel, geom), f"swinblock/gauss/{W.case_id(case)}")


# ================================================================================================ refusals
def test_supported_refuses():
    sup = _lib.load().mv_swin_block_attn_supported
    F, BF = _lib.F32, _lib.BF16
    assert sup(14, 14, 384, 12, 7, 7, F) == 1 and sup(14, 21, 192, 6, 7, 7, F) == 1 and sup(14, 14, 96, 3, 7, 7, F) == 1
    assert sup(14, 7, 384, 12, 7, 7, F) == 0 and sup(7, 14, 384, 12, 7, 7, F) == 0            # a 7-wide map
    assert sup(14, 16, 384, 12, 7, 7, F) == 0 and sup(15, 14, 96, 3, 7, 7, F) == 0            # not a multiple of 7
    assert sup(21, 21, 384, 12, 7, 7, F) == 1                                                 # an odd window count: one window per workgroup
    assert sup(21, 21, 192, 6, 7, 7, F) == 0                                                  # NWIN = 2
    assert sup(21, 21, 96, 3, 7, 7, F) == 1                                                   # swin_win96: one window per workgroup
    with _Flags(("swin_c96_shared",)):
        assert sup(21, 21, 96, 3, 7, 7, F) == 0
    assert sup(14, 14, 384, 6, 7, 7, F) == 0 and sup(14, 14, 96, 4, 7, 7, F) == 0             # heads * 32 != C
    assert sup(16, 16, 384, 12, 8, 8, F) == 0 and sup(14, 14, 384, 12, 7, 14, F) == 0         # a window that is not 7 x 7
    assert sup(14, 14, 128, 4, 7, 7, F) == 0                                                  # C = 128
    assert sup(14, 14, 384, 12, 7, 7, BF) == 0                                                # a bf16 stream
    with _Flags(("no_swin_block_attn",)):
        assert sup(14, 14, 384, 12, 7, 7, F) == 0
    assert sup(14, 14, 384, 12, 7, 7, F) == 1


def test_fwd_refuses_and_leaves_the_destination_alone():
    kernel, geom = "swin_block_attn_c192", (2, 14, 14, 3, 3)
    op = W.gauss(kernel, geom)
    C, (B, Hf, Wf, shh, shw) = 192, geom
    d = _operands(op)
    y = _dest(B * Hf * Wf, C, torch.float32)
    fwd = _lib.load().mv_swin_block_attn_fwd

    def go(ptrs, B_=B, Hf_=Hf, Wf_=Wf, sh=(shh, shw)):
        return fwd(*ptrs, B_, Hf_, Wf_, C, C // 32, 7, 7, sh[0], sh[1], W.EPS, _lib.F32, _stream())
    good = [_p(t) for t in d] + [_p(y)]
    for sh in ((7, 3), (3, 7), (-1, 3), (3, -1)):
        assert go(good, sh=sh) == MV_E_UNSUPPORTED, sh                                         # a shift outside [0, 7)
    assert go(good, Hf_=21, Wf_=21) == MV_E_UNSUPPORTED                                        # an odd window count at NWIN = 2
    assert go(good[:6] + [good[0]]) == MV_E_INVALID                                            # x == y
    assert go(good, B_=0) == MV_E_INVALID
    for i in range(7):
        assert go(good[:i] + [None] + good[i + 1:]) == MV_E_INVALID, f"null operand {i}"
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all()), "a refused call wrote into the destination"
    assert bool((d[0].cpu() == torch.from_numpy(np.array(op["x"]))).all()), "a refused call wrote into x"
