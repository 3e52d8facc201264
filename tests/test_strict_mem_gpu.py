"""`-m gpu`: exact and per-element parity checks of the memory-bound kernels (instruments, case data and emulations: tests/_strict.py;
CPU proof that the instruments see each defect: tests/test_strict_host.py).

Every destination is filled with the sentinel and has a guard behind it (tests/_slices.py); the guard must be intact and no sentinel
may survive where the reference is not the sentinel's value.  Operands are rounded to the storage type before both sides see them;
the reference is float64.  Every case names the kernel it must reach and prints kernel, worst |got - ref| / bound ratio and rounding
bias (`pytest -s`).

Exact instrument (np.array_equal): max pool, cast, NCHW <-> NHWC, copy_rows, the patch-merge and channel gathers, ReLU through
mv_eltwise_fwd / mv_add_fwd on integers (with one grid-stride case each for `eltwise_x8` and scalar `add`: grid_vec8 caps at 8192
blocks, grid_for at 4096, of 256 threads), average pools with power-of-two windows and fp32 output, bilinear resize at x2 / x4, the
global average pool's backward at HW = 64.
Bound instrument (`S.ops_bound`, n_ops counted from the kernel source next to each case; the rounding bias where the output is bf16
and >= 4096 reference elements have |ref| >= 2^-6, decided from the reference): the six activations, add, channel scale, channel
affine with and without residual, the adaptive / global / plain average pools, resize at ragged ratios, and the fp32 backward
kernels mv_channel_scale_bwd_f32, mv_avgpool_global_bwd_nhwc_f32, mv_bn_dgamma_f32, mv_bn_train_dz_coef_f32.
The moments and BatchNorm fold kernels and the forward LayerNorm kernels (plain, vectorised, slim, post-norm add, patch merge) are in
test_strict_norm_gpu.py; the GEMMs that normalise their rows on the way in (mv_ln_linear_fwd, mv_ln_mlp*_fwd: exact +-1 rows and a
composed per-element bound), mv_cnblock_dw_fwd, mv_patch4_ln_fwd and mv_linear_lnout_fwd -> mv_linear_lnin_fwd are in
test_strict_lngemm_gpu.py.  The dropout / PRNG kernels are compared bit for bit in `_cases`.  mv_se_scale_fwd (exact on the
activations' lattices and a bound composed from squeeze.hip's roundings) is in test_strict_act_gpu.py.
mv_maxpool2d_out_nhwc_fwd is exact in test_squeezenet_gpu.py.  The training backward kernels (conv dgrad / wgrad,
mv_maxpool2d_bwd_nhwc_f32, mv_colsum_f32, the softmax / attention backward, the gathers' adjoints: exact and bounded;
mv_act_bwd_f32, the LayerNorm backward, the cross-entropy, the Swin window backward: float64 reference at edge shapes) are in
test_strict_bwd_gpu.py, the forward attention kernels in test_strict_attn_gpu.py.

Worst fp32-output ratios |got - ref| / bound of the activations that use v_exp_f32 / v_rcp_f32 (bound: S.act_n_ops, which rests on
the ISA's stated 1-ulp accuracy of both), measured on an MI355X, kernels eltwise_x8 / eltwise:
    sigmoid    0.202 (eltwise_x8), 0.202 (eltwise)
    silu       0.191, 0.191
    gelu_tanh  0.207, 0.207
"""
import functools

import numpy as np
import pytest
import torch

from eqxvision_amd import _lib
from oracle import np_ops as O
from tests import _strict as S
from tests._slices import GUARD, SENTINEL, _dest, _read
from tests._strict_gpu import DT, _dev, _Flags, _need_gpu, _p, _stream  # noqa: F401  (_need_gpu: the module fixture)

pytestmark = pytest.mark.gpu

F64 = np.float64
TT = {"bf16": torch.bfloat16, "fp32": torch.float32}
DTYPES = ["bf16", "fp32"]
MV_E_UNSUPPORTED = -2
assert S.SENTINEL == SENTINEL


def _run(entry, args, shape, out, flags=()):
    """Launches `entry` on a sentinel-filled, guarded destination; args(y_ptr) gives the argument list.  Returns (values, kernel)."""
    n = int(np.prod(shape))
    y = _dest(1, n, TT[out])
    with _Flags(flags):
        _lib.call(entry, *args(_p(y)))
        kern = _lib.last_kernel()
    torch.cuda.synchronize()
    body, guard = _read(y, 1, n)
    assert guard.numel() == GUARD and bool((guard == SENTINEL).all()), f"{entry}: guard behind the destination overwritten"
    return body.numpy().astype(F64).reshape(shape), kern


def _judge(tag, kern, expect, got, ref, out, mag=None, n_ops=None, bound=None):
    """Prints the figures, then asserts the kernel name, the sentinel and the instrument: exact when neither n_ops nor bound is given."""
    ref = np.asarray(ref, F64)
    left = int(((got == SENTINEL) & (ref != SENTINEL)).sum())
    if n_ops is None and bound is None:
        info = S.check_exact(got, ref)
        print(f"{tag} [{kern}]: exact {info['ok']} wrong {info.get('nbad')} of {info.get('n')} | bound n/a | bias n/a")
        infos = [("exact", info)]
    else:
        a = S.check_bound(got, ref, mag, 0, out, n_ops=n_ops, bound=bound)
        # the bias rule is a property of the case's reference, decided before the output is looked at
        eligible = int((np.abs(ref) >= 2.0 ** -6).sum())
        applies = out == "bf16" and eligible >= S.BIAS_MIN_ELEMS
        b = S.check_bias(got, ref, out) if applies else {"ok": True, "bias": float("nan"), "n_bias": 0}
        print(f"{tag} [{kern}]: worst |got-ref|/bound {a.get('worst', float('nan')):.3f} over {a.get('n')} elements, "
              f"violations {a.get('nviol')} | bias {b['bias']:+.4f} over {b['n_bias']}")
        infos = [("bound", a), ("bias", b)]
    assert kern == expect, f"{tag}: served by {kern!r}, expected {expect!r}"
    assert left == 0, f"{tag}: {left} sentinel values left inside the output"
    for name, i in infos:
        assert i["ok"], f"{tag} {name}: {i}"


def _ints(rng, shape, lim, step=1):
    return (rng.integers(-lim // step, lim // step + 1, shape) * step).astype(np.float32)


# ================================================================================================ exact: max pool
MAXPOOL = [(16, "bf16", "maxpool_nhwc_bf16x8"), (13, "bf16", "maxpool_nhwc"), (13, "fp32", "maxpool_nhwc")]


@pytest.mark.parametrize("below", [False, True], ids=["gauss", "below_minus_1"])
@pytest.mark.parametrize("k,s,p", [(3, 2, 1), (2, 2, 0), (3, 1, 1)], ids=["3x3s2p1", "2x2s2p0", "3x3s1p1"])
@pytest.mark.parametrize("C,dtype,expect", MAXPOOL, ids=[f"C{c}_{d}" for c, d, _ in MAXPOOL])
def test_maxpool_exact(C, dtype, expect, k, s, p, below):
    """below_minus_1: every value is below -1, so a padded tap read as 0 would win."""
    x = S.wide_data(S.rng_of(21), (2, 9, 11, C), dtype)
    if below:
        x = S.q_of(dtype)(-2.0 - np.abs(x))
        assert (x < -1.0).all()
    ref = S.maxpool64(x, k, s, p)
    xd = _dev(x, dtype)
    got, kern = _run("mv_maxpool2d_nhwc_fwd", lambda y: (_p(xd), y, 2, 9, 11, C, k, k, s, s, p, p, DT[dtype], _stream()), ref.shape, dtype)
    _judge(f"maxpool/C{C}/{dtype}/{k}x{k}s{s}p{p}/{'below' if below else 'gauss'}", kern, expect, got, ref, dtype)


# ================================================================================================ exact: cast and layouts
def _cast_ref(x, dout):
    return O.bf16_round(x).astype(F64) if dout == "bf16" else np.asarray(x, F64)


@pytest.mark.parametrize("dout", DTYPES)
@pytest.mark.parametrize("din", DTYPES)
def test_cast_exact(din, dout):
    """f32 -> bf16 must equal O.bf16_round(x) bit for bit; the other three pairs must equal x."""
    n = 100003
    x = S.wide_data(S.rng_of(22), (n,), din)
    xd = _dev(x, din)
    got, kern = _run("mv_cast", lambda y: (_p(xd), y, n, DT[din], DT[dout], _stream()), (n,), dout)
    _judge(f"cast/{din}->{dout}", kern, "cast", got, _cast_ref(x, dout), dout)


@pytest.mark.parametrize("dout", DTYPES)
@pytest.mark.parametrize("din", DTYPES)
@pytest.mark.parametrize("N,C,H,W", [(3, 37, 9, 11), (2, 64, 8, 8)], ids=["ragged_37x99", "full_64x64"])
@pytest.mark.parametrize("entry", ["mv_nchw_to_nhwc", "mv_nhwc_to_nchw"])
def test_layout_exact(entry, N, C, H, W, din, dout):
    """32 x 33 LDS tiles over (C, HW): 37 x 99 is ragged in both directions, 64 x 64 in neither."""
    to_nhwc = entry == "mv_nchw_to_nhwc"
    x = S.wide_data(S.rng_of(23), (N, C, H, W) if to_nhwc else (N, H, W, C), din)
    ref = _cast_ref(np.ascontiguousarray(x.transpose(0, 2, 3, 1) if to_nhwc else x.transpose(0, 3, 1, 2)), dout)
    xd = _dev(x, din)
    got, kern = _run(entry, lambda y: (_p(xd), y, N, C, H, W, DT[din], DT[dout], _stream()), ref.shape, dout)
    _judge(f"{entry}/{C}x{H * W}/{din}->{dout}", kern, entry[3:], got, ref, dout)


# ================================================================================================ exact: copies and gathers
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("row_bytes,src_pitch,dst_pitch", [(48, 64, 80), (36, 44, 52)], ids=["16B_pieces", "2B_pieces"])
def test_copy_rows_exact(row_bytes, src_pitch, dst_pitch, dtype):
    """Strided source and destination; the bytes between the destination's rows must keep the sentinel."""
    rows, esz = 7, 2 if dtype == "bf16" else 4
    src = S.wide_data(S.rng_of(24), (rows, src_pitch // esz), dtype)
    ref = np.full((rows, dst_pitch // esz), SENTINEL, F64)
    ref[:, :row_bytes // esz] = src[:, :row_bytes // esz]
    sd = _dev(src, dtype)
    got, kern = _run("mv_copy_rows", lambda y: (_p(sd), y, rows, row_bytes, src_pitch, dst_pitch, _stream()), ref.shape, dtype)
    _judge(f"copy_rows/{row_bytes}B/{dtype}", kern, "copy_rows", got, ref, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,expect", [(8, "patch_merge_gather_vec"), (5, "patch_merge_gather")], ids=["vec", "scalar"])
def test_patch_merge_gather_exact(C, expect, dtype):
    """Odd H and W: the taps past the map are zeros.  Block order (0::2, 0::2) | (1::2, 0::2) | (0::2, 1::2) | (1::2, 1::2)."""
    B, H, W = 2, 5, 7
    x = S.wide_data(S.rng_of(25), (B, H, W, C), dtype)
    xp = np.zeros((B, H + 1, W + 1, C), np.float32)
    xp[:, :H, :W] = x
    ref = np.concatenate([xp[:, 0::2, 0::2], xp[:, 1::2, 0::2], xp[:, 0::2, 1::2], xp[:, 1::2, 1::2]], -1)
    xd = _dev(x, dtype)
    got, kern = _run("mv_patch_merge_gather_nhwc", lambda y: (_p(xd), y, B, H, W, C, DT[dtype], _stream()), ref.shape, dtype)
    _judge(f"patch_merge/C{C}/{dtype}", kern, expect, got, ref, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C_in,kind", [(13, "permutation"), (24, "subset")])
def test_channel_gather_exact(C_in, kind, dtype):
    rows, C_out = 35, 13
    rng = S.rng_of(26)
    x = S.wide_data(rng, (rows, C_in), dtype)
    idx = rng.permutation(C_in)[:C_out].astype(np.int32)
    assert len(set(idx.tolist())) == C_out and (kind == "subset") == (C_out < C_in)
    xd, idxd = _dev(x, dtype), torch.from_numpy(idx).cuda()
    got, kern = _run("mv_channel_gather_nhwc_fwd", lambda y: (_p(xd), _p(idxd), y, rows, C_in, C_out, DT[dtype], _stream()),
                     (rows, C_out), dtype)
    _judge(f"channel_gather/{kind}/{dtype}", kern, "channel_gather_" + ("bf16" if dtype == "bf16" else "f32"), got, x[:, idx], dtype)


# ================================================================================================ exact: ReLU / add on integers
INT_N = [(4096 + 8, (), "_x8"), (100003, (), ""), (4096 + 8, ("eltwise_scalar",), "")]
INT_IDS = ["x8_4104", "scalar_100003", "scalar_flag_4104"]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,flags,suffix", INT_N, ids=INT_IDS)
def test_relu_exact(n, flags, suffix, dtype):
    x = S.int_tensor(S.rng_of(27), (n,), 64)
    xd = _dev(x, dtype)
    got, kern = _run("mv_eltwise_fwd", lambda y: (_p(xd), y, n, 1, DT[dtype], _stream()), (n,), dtype, flags)
    _judge(f"relu/{n}/{dtype}", kern, "eltwise" + suffix, got, np.maximum(x, 0), dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,flags,suffix", INT_N, ids=INT_IDS)
def test_add_relu_exact(n, flags, suffix, dtype):
    rng = S.rng_of(28)
    a, b = S.int_tensor(rng, (n,), 64), S.int_tensor(rng, (n,), 64)
    ad, bd = _dev(a, dtype), _dev(b, dtype)
    got, kern = _run("mv_add_fwd", lambda y: (_p(ad), _p(bd), y, n, 1, DT[dtype], _stream()), (n,), dtype, flags)
    _judge(f"add_relu/{n}/{dtype}", kern, "add" + suffix, got, np.maximum(a + b, 0), dtype)


def _grid_stride(entry, n, expect, two):
    rng = S.rng_of(29)
    ops_ = [rng.integers(-64, 65, n, dtype=np.int8) for _ in range(2 if two else 1)]
    devs = [torch.from_numpy(o).cuda().to(torch.bfloat16) for o in ops_]
    ref = np.maximum(ops_[0].astype(np.int16) + (ops_[1] if two else 0), 0).astype(np.float32)
    y = _dest(1, n)
    _lib.call(entry, *[_p(d) for d in devs], _p(y), n, 1, DT["bf16"], _stream())
    kern = _lib.last_kernel()
    torch.cuda.synchronize()
    host = y.float().cpu().numpy()
    ok = np.array_equal(host[:n], ref)
    print(f"grid_stride/{entry}/{n} [{kern}]: exact {ok} | bound n/a | bias n/a")
    assert kern == expect
    assert (host[n:] == SENTINEL).all(), "guard overwritten"
    assert ok, f"first wrong indices {np.flatnonzero(host[:n] != ref)[:8].tolist()}"


def test_grid_stride_eltwise_x8():
    """grid_vec8 caps at 8192 blocks x 256 threads = 2^21 vectors per trip: 2^21 + 257 vectors force a second, partial trip."""
    _grid_stride("mv_eltwise_fwd", 8 * (2 ** 21 + 257), "eltwise_x8", False)


def test_grid_stride_add_scalar():
    """grid_for caps at 4096 blocks x 256 threads = 2^20 elements per trip (reachable below 2^25): 2^20 + 257 elements, an odd count,
    so the scalar kernel, take a second, partial trip."""
    _grid_stride("mv_add_fwd", 2 ** 20 + 257, "add", True)


# ================================================================================================ exact: average pools, fp32 output
def _adaptive(x, oh, ow, din, dout, flags=()):
    N, H, W, C = x.shape
    xd = _dev(x, din)
    return _run("mv_adaptive_avgpool2d_nhwc_fwd", lambda y: (_p(xd), y, N, H, W, C, oh, ow, DT[din], DT[dout], _stream()),
                (N, oh, ow, C), dout, flags)


AVG_EXACT = [("wide_16x16_C64_bf16", (2, 16, 16, 64), 1, "bf16", "global_avgpool_wide_bf16x8"),
             ("wide_16x16_C64_fp32", (2, 16, 16, 64), 1, "fp32", "global_avgpool_wide_f32x8"),
             ("x8_4x4_C16", (2, 4, 4, 16), 1, "bf16", "global_avgpool_bf16x8"),
             ("generic_8x8_to_2x2_bf16", (2, 8, 8, 13), 2, "bf16", "adaptive_avgpool_nhwc"),
             ("generic_8x8_to_2x2_fp32", (2, 8, 8, 13), 2, "fp32", "adaptive_avgpool_nhwc")]


@pytest.mark.parametrize("tag,shape,o,din,expect", AVG_EXACT, ids=[c[0] for c in AVG_EXACT])
def test_adaptive_avgpool_exact(tag, shape, o, din, expect):
    """Integers in [-8, 8] and a power-of-two window: every partial sum, 1 / HW and the mean are exact in fp32."""
    x = S.int_tensor(S.rng_of(30), shape, 8)
    ref, _, win = S.adaptive_ref(x, o, o)
    assert (np.log2(win) % 1 == 0).all() and np.array_equal(ref.astype(np.float32).astype(F64), ref)
    got, kern = _adaptive(x, o, o, din, "fp32")
    _judge(f"avgpool_exact/{tag}", kern, expect, got, ref, "fp32")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,expect", [(16, "avgpool2d_nhwc_x8"), (13, "avgpool2d_nhwc")])
def test_avgpool2d_exact(C, expect, dtype):
    """2x2 s2 of integers in [-8, 8]: the means are multiples of 1/4 below 8, exact in bf16 too (the entry stores its input type)."""
    N, H, W = 2, 6, 10
    x = S.int_tensor(S.rng_of(31), (N, H, W, C), 8)
    ref, _ = S.avgpool2d_ref(x, 2, 2)
    assert np.array_equal(S.bf(ref).astype(F64), ref)
    xd = _dev(x, dtype)
    got, kern = _run("mv_avgpool2d_nhwc_fwd", lambda y: (_p(xd), y, N, H, W, C, 2, 2, 2, 2, DT[dtype], _stream()), ref.shape, dtype)
    _judge(f"avgpool2d_exact/C{C}/{dtype}", kern, expect, got, ref, dtype)


# ================================================================================================ resize
# (variant, out_nchw, out dtype): the float4 kernel serves NCHW fp32 with W % 4 == 0, the scalar kernel every other variant
RESIZE_VARIANTS = [("nchw_f32", 1, "fp32"), ("nhwc_f32", 0, "fp32"), ("nhwc_bf16", 0, "bf16")]
RN, RC = 2, 3


def _resize(x, H, W, din, dout, nchw):
    N, h, w, C = x.shape
    xd = _dev(x, din)
    shape = (N, C, H, W) if nchw else (N, H, W, C)
    return _run("mv_resize_bilinear_nhwc_fwd", lambda y: (_p(xd), y, N, h, w, C, H, W, DT[din], DT[dout], nchw, _stream()), shape, dout)


@pytest.mark.parametrize("din", DTYPES)
@pytest.mark.parametrize("variant,nchw,dout", RESIZE_VARIANTS, ids=[v[0] for v in RESIZE_VARIANTS])
@pytest.mark.parametrize("h,w,H,W,step", [(7, 5, 14, 10, 16), (8, 8, 32, 32, 64)], ids=["7x5_x2", "8x8_x4"])
def test_resize_exact(h, w, H, W, step, variant, nchw, dout, din):
    """Power-of-two ratios: the tap weights are multiples of 1/4 (x2) or 1/8 (x4), so products of two weights are multiples of 1/16
    or 1/64.  Inputs are multiples of 16 in [-128, 128] at x2 and, of those, the multiples of 64 at x4: every output and every
    intermediate is then an integer <= 128, exact in fp32 and in bf16 (asserted).  NCHW fp32: W = 32 takes the float4 kernel,
    W = 10 the scalar one."""
    for n_in, n_out in ((h, H), (w, W)):
        assert np.array_equal(S.tap_matrix32(n_in, n_out), O._resize_weights(n_in, n_out)), "float32 taps differ from the float64 weights"
    x = _ints(S.rng_of(32), (RN, h, w, RC), 128, step)
    ref, _ = S.resize_ref(x, H, W)
    assert np.array_equal(np.rint(ref), ref) and np.abs(ref).max() <= 128 and np.array_equal(S.emu_resize(x, H, W, dout), ref)
    got, kern = _resize(x, H, W, din, dout, nchw)
    _judge(f"resize_exact/{h}x{w}->{H}x{W}/{variant}/{din}", kern, "resize_bilinear_nhwc_to_nchw" if nchw else "resize_bilinear_nhwc",
           got, ref.transpose(0, 3, 1, 2) if nchw else ref, dout)


RESIZE_RAGGED = [(7, 5, 17, 13, v) for v in RESIZE_VARIANTS] + [(9, 9, 33, 33, v) for v in RESIZE_VARIANTS] + \
                [(9, 9, 33, 36, RESIZE_VARIANTS[0])]          # W = 36: the float4 kernel at a ragged ratio


@pytest.mark.parametrize("din", DTYPES)
@pytest.mark.parametrize("h,w,H,W,var", RESIZE_RAGGED, ids=[f"{c[0]}x{c[1]}_to_{c[2]}x{c[3]}_{c[4][0]}" for c in RESIZE_RAGGED])
def test_resize_bound(h, w, H, W, var, din):
    """Bound S.resize_bound: (8 + 2 max(h, w)) 2^-23 M + half_ulp_out, M = max |x| of the image and channel.  The float32 emulation
    of the kernel's formula must stay inside it before anything is launched."""
    variant, nchw, dout = var
    x = S.q_of(din)(S.rng_of(33).standard_normal((RN, h, w, RC)))
    ref, M = S.resize_ref(x, H, W)
    bound = S.resize_bound(ref, M, h, w, dout)
    e = S.check_bound(S.emu_resize(x, H, W, dout), ref, None, 0, dout, bound=bound)
    assert e["ok"], f"the emulation leaves the derived bound: {e}"
    got, kern = _resize(x, H, W, din, dout, nchw)
    t = (lambda a: a.transpose(0, 3, 1, 2)) if nchw else (lambda a: a)
    _judge(f"resize/{h}x{w}->{H}x{W}/{variant}/{din}", kern, "resize_bilinear_nhwc_to_nchw" if nchw else "resize_bilinear_nhwc",
           got, t(ref), dout, bound=t(bound))


# ================================================================================================ bound: element-wise
ELT_N = [(40008, "eltwise_x8"), (40003, "eltwise")]


@functools.lru_cache(maxsize=None)
def _act_data(n, dtype):
    return S.act_input(S.rng_of(40), n, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,expect", ELT_N, ids=["x8", "scalar"])
@pytest.mark.parametrize("act", ["relu", "gelu_tanh", "hard_swish", "hard_sigmoid", "sigmoid", "silu"])
def test_eltwise_bound(act, n, expect, dtype):
    """x uniform in [-8, 8] with exact hits on -3, 0, 3; mag = |ref|; n_ops per activation as derived in S.act_n_ops from common.h:
    relu 0, hard_sigmoid 3, hard_swish 4; sigmoid 2 |t| + 5 with t = log2(e) x (two roundings of the exponent's argument count |t|
    each, v_exp_f32 2, the add 1, v_rcp_f32 2), silu one more, gelu_tanh 5 |t| + 6 with t = x (k1 x^2 + k0) (five roundings of the
    argument, exp 2, add 1, rcp 2, x * (.) 1).  The bf16 cases are dominated by the store's half ulp."""
    x = _act_data(n, dtype)
    ref = S.act64(x, act)
    xd = _dev(x, dtype)
    got, kern = _run("mv_eltwise_fwd", lambda y: (_p(xd), y, n, S.ACT_CODES[act], DT[dtype], _stream()), (n,), dtype)
    _judge(f"eltwise/{act}/{n}/{dtype}", kern, expect, got, ref, dtype, mag=np.abs(ref), n_ops=S.act_n_ops(x, act))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,expect", [(40008, "add_x8"), (40003, "add")], ids=["x8", "scalar"])
@pytest.mark.parametrize("act", ["none", "relu"])
def test_add_bound(act, n, expect, dtype):
    """One fp32 add: n_ops = 1, mag = |a| + |b|."""
    rng = S.rng_of(41)
    a, b = (S.q_of(dtype)(rng.standard_normal(n)) for _ in range(2))
    ref = S.act64(a.astype(F64) + b, act)
    ad, bd = _dev(a, dtype), _dev(b, dtype)
    got, kern = _run("mv_add_fwd", lambda y: (_p(ad), _p(bd), y, n, S.ACT_CODES[act], DT[dtype], _stream()), (n,), dtype)
    _judge(f"add/{act}/{n}/{dtype}", kern, expect, got, ref, dtype, mag=np.abs(a).astype(F64) + np.abs(b), n_ops=1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,expect", [(72, "channel_scale_x8"), (13, "channel_scale")])
def test_channel_scale_bound(C, expect, dtype):
    """One fp32 multiply: n_ops = 1, mag = |x| |s|."""
    x, s = S.scale_data(C, dtype)
    ref = x.astype(F64) * s.astype(F64)[:, None, :]
    xd, sd = _dev(x, dtype), _dev(s, dtype)
    got, kern = _run("mv_channel_scale_nhwc_fwd", lambda y: (_p(xd), _p(sd), y, 3, 50, C, DT[dtype], _stream()), ref.shape, dtype)
    _judge(f"channel_scale/C{C}/{dtype}", kern, expect, got, ref, dtype, mag=np.abs(ref), n_ops=1)


AFFINE = [("scale", 24, True, False, "none", (), "channel_affine_x8"), ("shift", 24, False, True, "none", (), "channel_affine_x8"),
          ("both", 24, True, True, "none", (), "channel_affine_x8"), ("both_relu", 24, True, True, "relu", (), "channel_affine_x8"),
          ("both_relu_C13", 13, True, True, "relu", (), "channel_affine"),
          ("both_relu_scalar_flag", 24, True, True, "relu", ("affine_scalar",), "channel_affine")]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tag,C,use_scale,use_shift,act,flags,expect", AFFINE, ids=[c[0] for c in AFFINE])
def test_channel_affine_bound(tag, C, use_scale, use_shift, act, flags, expect, dtype):
    """x * scale[c] + shift[c]: a multiply and an add in the scalar kernel, one fma in the 8-wide one: n_ops = 2 covers both;
    mag = |x| |scale| + |shift|."""
    rows = 50
    x, sc, sh, _ = S.affine_data(rows, C, dtype, use_scale, use_shift)
    ref, mag = S.affine_ref(x, sc, sh, None, act)
    xd, scd, shd = _dev(x, dtype), (None if sc is None else _dev(sc, "fp32")), (None if sh is None else _dev(sh, "fp32"))
    got, kern = _run("mv_channel_affine_fwd", lambda y: (_p(xd), _p(scd), _p(shd), y, rows, C, S.ACT_CODES[act], DT[dtype], _stream()),
                     (rows, C), dtype, flags)
    _judge(f"channel_affine/{tag}/{dtype}", kern, expect, got, ref, dtype, mag=mag, n_ops=2)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act", ["none", "relu"])
@pytest.mark.parametrize("rows,C", [(50, 24), (33, 264)])
def test_channel_affine_res_bound(rows, C, act, dtype):
    """fma(x, scale, shift) + residual: 2 roundings; n_ops = 3, mag = |x| |scale| + |shift| + |res|; every 5th scale negative."""
    x, sc, sh, r = S.affine_data(rows, C, dtype, res=True)
    ref, mag = S.affine_ref(x, sc, sh, r, act)
    xd, scd, shd, rd = _dev(x, dtype), _dev(sc, "fp32"), _dev(sh, "fp32"), _dev(r, dtype)
    got, kern = _run("mv_channel_affine_res_fwd",
                     lambda y: (_p(xd), _p(scd), _p(shd), _p(rd), y, rows, C, S.ACT_CODES[act], DT[dtype], _stream()), (rows, C), dtype)
    _judge(f"channel_affine_res/{rows}x{C}/{act}/{dtype}", kern, "channel_affine_res_x8", got, ref, dtype, mag=mag, n_ops=3)


@pytest.mark.parametrize("dtype", DTYPES)
def test_channel_affine_res_odd_width_unsupported(dtype):
    """The residual entry has no scalar kernel: C = 13 is MV_E_UNSUPPORTED and nothing is written."""
    rows, C = 50, 13
    x, sc, sh, r = S.affine_data(rows, C, dtype, res=True)
    xd, scd, shd, rd = _dev(x, dtype), _dev(sc, "fp32"), _dev(sh, "fp32"), _dev(r, dtype)
    y = _dest(rows, C, TT[dtype])
    rc = _lib.load().mv_channel_affine_res_fwd(_p(xd), _p(scd), _p(shd), _p(rd), _p(y), rows, C, 1, DT[dtype], _stream())
    torch.cuda.synchronize()
    assert rc == MV_E_UNSUPPORTED, rc
    assert bool((y == SENTINEL).all()), "an unsupported call wrote to its destination"


# ================================================================================================ bound: average pools
_ADAPTIVE = [("wide_25x25_C40", (2, 25, 25, 40), 1, 1, None, DTYPES), ("wide_7x7_C264", (3, 7, 7, 264), 1, 1, None, DTYPES),
             ("x8_5x5_C16", (2, 5, 5, 16), 1, 1, "global_avgpool_bf16x8", ["bf16"]),          # this kernel reads bf16 only
             ("generic_7x5_to_3x2_C13", (2, 7, 5, 13), 3, 2, "adaptive_avgpool_nhwc", DTYPES)]
ADAPTIVE = [(*c[:5], din, dout) for c in _ADAPTIVE for din in c[5] for dout in DTYPES]


@pytest.mark.parametrize("tag,shape,oh,ow,expect,din,dout", ADAPTIVE, ids=[f"{c[0]}_{c[5]}_to_{c[6]}" for c in ADAPTIVE])
def test_adaptive_avgpool_bound(tag, shape, oh, ow, expect, din, dout):
    """n_ops = window + 2 (window - 1 adds in any order, 1 / n, the multiply -- or one division), mag = the window's mean |x|.
    wide, C = 40: cpb = 5 chunks per block, pl = 204 pixel lanes, 4 idle threads, the 4-in-flight loop taken (lanes below 13);
    wide, C = 264: 33 chunks, the second channel block holds one.  x8 5x5: the HW % 4 tail.  7x5 -> 3x2: windows of 3|2|2 x 3|2."""
    if expect is None:
        expect = "global_avgpool_wide_bf16x8" if din == "bf16" else "global_avgpool_wide_f32x8"
        cpb, pl, idle, blocks = S.wide_geometry(shape[3])
        assert (cpb, pl, idle, blocks) == ((5, 204, 4, 1) if shape[3] == 40 else (32, 32, 0, 2))
    x = S.q_of(din)(S.rng_of(44).standard_normal(shape))
    ref, mag, win = S.adaptive_ref(x, oh, ow)
    got, kern = _adaptive(x, oh, ow, din, dout)
    _judge(f"adaptive_avgpool/{tag}/{din}->{dout}", kern, expect, got, ref, dout, mag=mag, n_ops=win + 2)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,expect", [(16, "avgpool2d_nhwc_x8"), (13, "avgpool2d_nhwc")])
def test_avgpool2d_bound(C, expect, dtype):
    """3x3 s2 on 7x9: n_ops = 9 + 2, mag = the window's mean |x|."""
    N, H, W = 2, 7, 9
    x = S.q_of(dtype)(S.rng_of(45).standard_normal((N, H, W, C)))
    ref, mag = S.avgpool2d_ref(x, 3, 2)
    xd = _dev(x, dtype)
    got, kern = _run("mv_avgpool2d_nhwc_fwd", lambda y: (_p(xd), y, N, H, W, C, 3, 3, 2, 2, DT[dtype], _stream()), ref.shape, dtype)
    _judge(f"avgpool2d/C{C}/{dtype}", kern, expect, got, ref, dtype, mag=mag, n_ops=11)


# ================================================================================================ backward kernels, fp32
def _f(a):
    return _dev(np.asarray(a, np.float32), "fp32")


def test_channel_scale_bwd_bound():
    """ds[b, c] = sum_p g x: HW fma in four row groups and three adds; n_ops = HW + 2, mag = sum |g| |x|."""
    B, HW, C = 3, 50, 72
    rng = S.rng_of(46)
    g, x = (rng.standard_normal((B, HW, C)).astype(np.float32) for _ in range(2))
    ref, mag = (g.astype(F64) * x).sum(1), (np.abs(g).astype(F64) * np.abs(x)).sum(1)
    gd, xd = _f(g), _f(x)
    got, kern = _run("mv_channel_scale_bwd_f32", lambda y: (_p(gd), _p(xd), y, B, HW, C, _stream()), (B, C), "fp32")
    _judge("channel_scale_bwd", kern, "channel_scale_bwd_f32", got, ref, "fp32", mag=mag, n_ops=HW + 2)


@pytest.mark.parametrize("HW,exact", [(49, False), (64, True)], ids=["HW49_bound", "HW64_int_exact"])
def test_avgpool_global_bwd(HW, exact):
    """dx = dy * (1 / HW): n_ops = 2 (the reciprocal, the multiply); HW = 64 with integer dy: 1 / 64 and the products are exact."""
    N, C = 3, 40
    rng = S.rng_of(47)
    dy = S.int_tensor(rng, (N, C), 64) if exact else rng.standard_normal((N, C)).astype(np.float32)
    ref = np.broadcast_to((dy.astype(F64) / HW)[:, None, :], (N, HW, C))
    dyd = _f(dy)
    got, kern = _run("mv_avgpool_global_bwd_nhwc_f32", lambda y: (_p(dyd), y, N, HW, C, _stream()), (N, HW, C), "fp32")
    _judge(f"avgpool_global_bwd/HW{HW}", kern, "avgpool_global_bwd_f32", got, ref, "fp32",
           **({} if exact else {"mag": np.abs(ref), "n_ops": 2}))


def _bn_sums(C=300):
    rng = S.rng_of(48)

    def f(s):
        return (s * rng.standard_normal(C)).astype(np.float32)
    return {"s1": f(30.0), "s2": f(60.0), "s0": f(500.0), "mean": f(0.5), "var": rng.uniform(0.3, 2.0, C).astype(np.float32),
            "scale": S.gauss_scale(rng, C)}


def test_bn_dgamma_bound():
    """(dyz - mean dys) rsqrt(var + eps), C = 300 (two blocks): the product, the difference, var + eps, rsqrtf (2), the last product:
    n_ops = 6, mag = (|dyz| + |mean dys|) rstd."""
    C, eps = 300, float(np.float32(1e-5))
    d = _bn_sums(C)
    rstd = 1.0 / np.sqrt(d["var"].astype(F64) + eps)
    ref = (d["s2"].astype(F64) - d["mean"].astype(F64) * d["s1"]) * rstd
    mag = (np.abs(d["s2"]).astype(F64) + np.abs(d["mean"].astype(F64) * d["s1"])) * rstd
    dv = {k: _f(v) for k, v in d.items()}
    got, kern = _run("mv_bn_dgamma_f32", lambda y: (_p(dv["s2"]), _p(dv["s1"]), _p(dv["mean"]), _p(dv["var"]), eps, y, C, _stream()),
                     (C,), "fp32")
    _judge("bn_dgamma", kern, "bn_dgamma_f32", got, ref, "fp32", mag=mag, n_ops=6)


@pytest.mark.parametrize("device_count", [True, False], ids=["device_count", "host_rows"])
def test_bn_train_dz_coef_bound(device_count):
    """The header's formula in float64; n_ops 10 for B and 16 for A, magnitudes as derived in S.bn_dz_coef64 (B's error goes into
    A's)."""
    C, n, a, eps = 300, 6272.0, float(np.float32(0.01)), float(np.float32(1e-5))
    d = _bn_sums(C)
    A, magA, B, magB = S.bn_dz_coef64(d["s1"], d["s2"], d["s0"], d["mean"], d["var"], d["scale"], n, a, eps)
    dv = {k: _f(v) for k, v in d.items()}
    cnt = _f([n]) if device_count else None
    out = _dest(2, C, torch.float32)                    # A then B, one guarded buffer
    _lib.call("mv_bn_train_dz_coef_f32", _p(dv["s1"]), _p(dv["s2"]), _p(dv["s0"]), _p(dv["mean"]), _p(dv["var"]), _p(dv["scale"]), _p(cnt),
              0.0 if device_count else n, a, eps, _p(out), _p(out) + 4 * C, C, _stream())
    kern = _lib.last_kernel()
    torch.cuda.synchronize()
    body, guard = _read(out, 2, C)
    assert bool((guard == SENTINEL).all())
    got = body.numpy().astype(F64)
    _judge("bn_train_dz_coef/B", kern, "bn_train_dz_coef_f32", got[1], B, "fp32", mag=magB, n_ops=10)
    _judge("bn_train_dz_coef/A", kern, "bn_train_dz_coef_f32", got[0], A, "fp32", mag=magA, n_ops=16)
