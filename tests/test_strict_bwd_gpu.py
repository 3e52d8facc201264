"""`-m gpu`: exact-integer and per-element parity checks of the training backward kernels (csrc/train_bwd.hip; all fp32).  Instruments,
case data, float64 references and emulations: tests/_strict.py; CPU proof that the instruments see each defect:
tests/test_strict_bwd_host.py.

Every destination is filled with the sentinel and has a guard behind it (tests/_slices.py); the kernel that served the call is asserted
(`_lib.last_kernel()`); references are float64, computed from the fp32 operands both sides see; every case prints the kernel and the
worst |got - ref| / bound (`pytest -s`).

Exact (np.array_equal with the float64 reference; `S.prove_exact(..., out="fp32")` asserted before each launch; operands are integers
in [-2, 2], probabilities multiples of 1/8): mv_conv2d_dgrad_nhwc_f32 and mv_conv2d_wgrad_nhwc_f32 at the eleven shapes of
S.CONV_BWD_SHAPES on the matrix-core and on the VALU path (the weight gradient without scratch, with 8 MiB, with room for two parts
and with room for one; bytes [0, 4096) of the offer must stay zero), mv_colsum_f32 with and without scratch and with an offer one part short, mv_softmax_bwd_f32,
mv_mha_bwd_f32 (dqkv and ds_scratch), mv_maxpool2d_bwd_nhwc_f32 (distinct integers per channel, also all below -1),
mv_patch_merge_gather_bwd_f32 at odd sizes, mv_transpose2d_f32 with a row stride, mv_scatter_rows_sum_f32.
Bounded on Gaussian operands:
    conv dgrad   S.elem_bound, kred = K / groups * R * S   (the reduction of one input element: conv_dgrad_mfma_kernel's three loops)
    conv wgrad   S.elem_bound, kred = P = N * Ho * Wo      (a summation tree over n terms is at most n - 1 deep: no term for the split)
    colsum       S.ops_bound, n_ops = 1 + ceil(rows / 4) + 2 (+ split)   (S.colsum_n_ops: colsum_kernel, colsum_part_kernel, sum_parts_kernel)
    softmax_bwd  S.ops_bound, n_ops = ceil(cols / 64) + 10 of |scale p| (|dp| + sum |p dp|): the lane's products and adds, 6 shuffle
                 adds, the difference, two products (softmax_bwd_kernel)
    mha_bwd      S.ops_bound, dS: dh + ceil(N / 64) + 9; dQ, dK: that + N; dV: N   (S.mha_bwd_ref: mha_bwd_q_kernel, mha_bwd_kv_kernel)
Tolerance of tests/_cases.py (`_cmp` at 1e-3 max(1, max|ref|)) against a float64 reference at new shapes: mv_softmax_xent_f32 (second
lane trip, second trip of the mean, |logit| = 90, soft targets), mv_layernorm_bwd_f32 with and without gamma, mv_act_bwd_f32 with the
corners of the hard activations (S.act_grad64 states the side), mv_swin_window_attn_bwd_f32 on rectangular maps and windows.
Out of scope: the dropout / PRNG kernels, and seg_bwd.hip, which has test_seg_grad_gpu.py; mv_avgpool_global_bwd_nhwc_f32 is in
test_strict_mem_gpu.py.

Worst |got - ref| / bound per kernel family, measured on an MI355X:
    conv dgrad   0.060 (conv_dgrad_mfma_f32, 1x1 K = 21), 0.062 (conv_dgrad_f32, depthwise)
    conv wgrad   0.105 (conv_wgrad_mfma_f32 and conv_wgrad_f32 alike, the Wo = 1 shape, P = 9)
    colsum       0.078 (colsum_f32, 3 x 5 product), 0.004 (colsum_split_f32, 515 x 70)
    softmax_bwd  0.043 (4 x 130)
    mha_bwd      0.055 (dS, N = 65), 0.184 (dqkv, N = 5, dh = 72: dV's bound counts N operations only)
Every exact case was bit-equal on both paths and under every scratch regime; no defect was found in train_bwd.hip.
"""
import functools

import numpy as np
import pytest
import torch

from eqxvision_amd import _lib
from tests import _strict as S
from tests._cases import TOL_F32, _cmp
from tests._slices import GUARD, SENTINEL, _dest, _read
from tests._strict_gpu import _dev, _Flags, _need_gpu, _p, _stream  # noqa: F401  (_need_gpu: the module fixture)
from tests.test_strict_mem_gpu import _judge, _run

pytestmark = pytest.mark.gpu

F64 = np.float64
SYNC = 4096                   # route.h, SCRATCH_SYNC_BYTES: the head of every scratch offer
AMPLE = 8 << 20


def _f(a):
    return _dev(np.ascontiguousarray(np.asarray(a, np.float32)), "fp32")


def _run_n(entry, args, shapes, flags=()):
    """`_run` for an entry with several destinations: args(*pointers) gives the argument list.  Returns (list of values, kernel)."""
    sizes = [int(np.prod(s)) for s in shapes]
    ys = [_dest(1, n, torch.float32) for n in sizes]
    with _Flags(flags):
        _lib.call(entry, *args(*[_p(y) for y in ys]))
        kern = _lib.last_kernel()
    torch.cuda.synchronize()
    out = []
    for y, n, s in zip(ys, sizes, shapes):
        body, guard = _read(y, 1, n)
        assert guard.numel() == GUARD and bool((guard == SENTINEL).all()), f"{entry}: guard behind a destination overwritten"
        out.append(body.numpy().astype(F64).reshape(s))
    return out, kern


class _Scratch:
    """A zero-initialised offer of `nbytes` (None: no offer) for the one launch inside the scope; afterwards the offer is withdrawn
    whether it was taken or not, and the split-K arrival words at its head must still be zero."""

    def __init__(self, nbytes):
        self.nbytes = nbytes
        self.ws = None if nbytes is None else torch.zeros(AMPLE, dtype=torch.uint8, device="cuda")

    def __enter__(self):
        if self.ws is not None:
            assert SYNC < self.nbytes <= AMPLE
            _lib.call("mv_set_scratch", _p(self.ws), int(self.nbytes), _stream())
        return self

    def __exit__(self, *a):
        _lib.call("mv_set_scratch", None, 0, _stream())
        if self.ws is not None and a[0] is None:
            torch.cuda.synchronize()
            assert not bool(self.ws[:SYNC].any()), "the first 4096 bytes of the scratch offer were written"


def _tol(tag, kern, expect, got, ref):
    """The criterion of tests/_cases.py for fp32 outputs, figures printed first."""
    ref = np.asarray(ref, F64)
    i = _cmp(got, ref, TOL_F32)
    print(f"{tag} [{kern}]: max |got-ref| {i.get('err')} of {i.get('lim')} allowed")
    assert kern == expect, f"{tag}: served by {kern!r}, expected {expect!r}"
    assert int(((np.asarray(got) == SENTINEL) & (ref != SENTINEL)).sum()) == 0, f"{tag}: sentinel values left inside the output"
    assert i["ok"], f"{tag}: {i}"


# ================================================================================================ conv dgrad / wgrad
SHAPES = S.CONV_BWD_SHAPES
SHAPE_IDS = [g.tag for g in SHAPES]


@functools.lru_cache(maxsize=None)
def _conv(i, kind):
    g = SHAPES[i]
    x, w, dy = S.conv_bwd_data(g, kind)
    return (g, x, w, dy) + S.conv_bwd_ref(x, w, dy, g)


def _dgrad_kernel(g):
    return "conv_dgrad_mfma_f32" if g.groups == 1 and g.C >= 8 else "conv_dgrad_f32"


def _dgrad(g, w, dy, flags=()):
    wd, dyd = _f(w), _f(dy)
    return _run("mv_conv2d_dgrad_nhwc_f32", lambda y: (_p(dyd), _p(wd), y, *g.args(), _stream()), (g.N, g.H, g.W, g.C), "fp32", flags)


def _wgrad(g, x, dy, flags=(), offer=None):
    xd, dyd = _f(x), _f(dy)
    with _Scratch(offer):
        return _run("mv_conv2d_wgrad_nhwc_f32", lambda y: (_p(xd), _p(dyd), y, *g.args(), _stream()), (g.K, g.R, g.S, g.Cg), "fp32", flags)


def _regimes(g):
    """(name, bytes on offer): none, ample, room for two parts and a half (fit = 2), room for one and a half (fit < 2)."""
    return [("no_offer", None), ("ample", AMPLE), ("fit2", SYNC + int(2.5 * g.out_elems * 4)), ("fit1", SYNC + int(1.5 * g.out_elems * 4))]


def test_clamp_shape_reaches_the_clamp():
    """The split as mv_conv2d_wgrad_nhwc_f32's comment states it (tiles x chunks ~ 4096 waves, >= 128 positions per chunk): the clamp
    shape wants more than two chunks, so the fit2 offer runs `split > fit` and the fit1 offer runs `fit < 2`."""
    g = S.CONV_BWD_CLAMP
    offers = dict(_regimes(g))
    assert g.wgrad_split()[0] > 2
    assert g.wgrad_split(offers["ample"])[1] == g.wgrad_split()[0]
    assert g.wgrad_split(offers["fit2"])[1] == 2 and g.wgrad_split(offers["fit1"])[1] == 1 and g.wgrad_split(None)[1] == 1


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=SHAPE_IDS)
def test_conv_dgrad_exact(i):
    g, x, w, dy, dx, mx, _, _ = _conv(i, "int")
    S.prove_exact(g.tag, dx, mx, S.conv_bwd_weights(x, w, dy, g)[0], out="fp32")
    got, kern = _dgrad(g, w, dy)
    _judge(f"dgrad_exact/{g.tag}", kern, _dgrad_kernel(g), got, dx, "fp32")
    got, kern = _dgrad(g, w, dy, ("dgrad_valu",))
    _judge(f"dgrad_exact/{g.tag}/valu", kern, "conv_dgrad_f32", got, dx, "fp32")


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=SHAPE_IDS)
def test_conv_wgrad_exact(i):
    g, x, w, dy, _, _, dw, mw = _conv(i, "int")
    S.prove_exact(g.tag, dw, mw, S.conv_bwd_weights(x, w, dy, g)[1], out="fp32")
    for name, offer in _regimes(g):
        got, kern = _wgrad(g, x, dy, offer=offer)
        _judge(f"wgrad_exact/{g.tag}/{name}/split{g.wgrad_split(offer)[1]}", kern, "conv_wgrad_mfma_f32", got, dw, "fp32")
    got, kern = _wgrad(g, x, dy, ("wgrad_valu",))
    _judge(f"wgrad_exact/{g.tag}/valu", kern, "conv_wgrad_f32", got, dw, "fp32")


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=SHAPE_IDS)
def test_conv_dgrad_bound(i):
    g, x, w, dy, dx, mx, _, _ = _conv(i, "gauss")
    bound = S.elem_bound(dx, mx, g.Kg * g.R * g.S, "fp32")
    got, kern = _dgrad(g, w, dy)
    _judge(f"dgrad/{g.tag}", kern, _dgrad_kernel(g), got, dx, "fp32", bound=bound)
    got, kern = _dgrad(g, w, dy, ("dgrad_valu",))
    _judge(f"dgrad/{g.tag}/valu", kern, "conv_dgrad_f32", got, dx, "fp32", bound=bound)


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=SHAPE_IDS)
def test_conv_wgrad_bound(i):
    g, x, w, dy, _, _, dw, mw = _conv(i, "gauss")
    bound = S.elem_bound(dw, mw, g.P, "fp32")
    for name, offer in _regimes(g)[:3]:
        got, kern = _wgrad(g, x, dy, offer=offer)
        _judge(f"wgrad/{g.tag}/{name}/split{g.wgrad_split(offer)[1]}", kern, "conv_wgrad_mfma_f32", got, dw, "fp32", bound=bound)
    got, kern = _wgrad(g, x, dy, ("wgrad_valu",))
    _judge(f"wgrad/{g.tag}/valu", kern, "conv_wgrad_f32", got, dw, "fp32", bound=bound)


# ================================================================================================ colsum
COLSUM = [(3, 5), (515, 70), (1029, 64)]


@pytest.mark.parametrize("kind", ["int", "gauss"])
@pytest.mark.parametrize("product", [False, True], ids=["sum", "product"])
@pytest.mark.parametrize("M,C", COLSUM, ids=[f"{m}x{c}" for m, c in COLSUM])
def test_colsum(M, C, product, kind):
    """Integers in [-2, 2]: exact.  Gaussian: n_ops = S.colsum_n_ops (the product, ceil(rows / 4) adds of a row group, two adds across
    the groups, `split` adds over the parts), mag = sum |a| |b|.  Without scratch colsum_f32; with it colsum_split_f32 from 512 rows."""
    rng = S.rng_of(61)
    a, b = ((S.int_tensor(rng, (M, C), 2) if kind == "int" else rng.standard_normal((M, C)).astype(np.float32)) for _ in range(2))
    b = b if product else None
    ref, mag = S.colsum_ref(a, b)
    if kind == "int":
        S.prove_exact(f"colsum/{M}x{C}", ref, mag, [a.T] + ([b.T] if product else []), out="fp32")
    ad, bd = _f(a), (_f(b) if product else None)
    for offer in (None, AMPLE):
        split = S.colsum_split(M)[0] if offer else 1
        with _Scratch(offer):
            got, kern = _run("mv_colsum_f32", lambda y: (_p(ad), _p(bd), y, M, C, _stream()), (C,), "fp32")
        _judge(f"colsum/{M}x{C}/{'product' if product else 'sum'}/{kind}/split{split}", kern, "colsum_split_f32" if split > 1 else "colsum_f32",
               got, ref, "fp32", **({} if kind == "int" else {"mag": mag, "n_ops": S.colsum_n_ops(M, split)}))


def test_colsum_takes_all_its_parts_or_none():
    """1030 x 70 wants 5 parts, i.e. 4096 + 5 * 70 * 4 bytes.  An offer with room for 4 is left alone: colsum_f32, bit-equal to the run
    without an offer (and to S.emu_colsum's single part), and not one byte of the offer written."""
    M, C = 1030, 70
    assert S.colsum_split(M)[0] == 5
    a = S.rng_of(67).standard_normal((M, C)).astype(np.float32)
    ad = _f(a)
    runs = []
    for offer in (None, SYNC + 4 * C * 4):
        with _Scratch(offer) as sc:
            got, kern = _run("mv_colsum_f32", lambda y: (_p(ad), None, y, M, C, _stream()), (C,), "fp32")
        print(f"colsum/all_or_nothing/offer {offer}: served by {kern}")
        assert kern == "colsum_f32"
        if offer is not None:
            assert not bool(sc.ws.any()), "an offer that is too small for every part was written"
        runs.append(np.asarray(got, np.float32))
    assert np.array_equal(runs[0].view(np.uint32), runs[1].view(np.uint32))
    assert np.array_equal(runs[0].view(np.uint32), S.emu_colsum(a, None, 1).view(np.uint32))


# ================================================================================================ softmax_bwd / mha_bwd
@pytest.mark.parametrize("kind", ["int", "gauss"])
@pytest.mark.parametrize("rows,cols", [(5, 65), (6, 3), (4, 130)])
def test_softmax_bwd(rows, cols, kind):
    """ds = scale p (dp - sum_j p dp), scale = 0.5.  Exact: p multiples of 1/8, dp integers -- every value a multiple of 2^-7 far below
    2^17.  Gaussian: n_ops = ceil(cols / 64) + 10 of |scale p| (|dp| + sum |p dp|), counted from softmax_bwd_kernel: the lane's
    ceil(cols / 64) products and adds (the product counted once, in the 10), 6 shuffle adds, the difference, two products."""
    rng = S.rng_of(64)
    if kind == "int":
        p, dp = S.eighths(rng, (rows, cols)), S.int_tensor(rng, (rows, cols), 2)
    else:
        e = np.exp(rng.standard_normal((rows, cols)))
        p, dp = (e / e.sum(-1, keepdims=True)).astype(np.float32), rng.standard_normal((rows, cols)).astype(np.float32)
    ref, mag = S.softmax_bwd_ref(p, dp, 0.5)
    if kind == "int":
        S.prove_exact(f"softmax_bwd/{rows}x{cols}", ref * 128.0, mag * 128.0, [p], out="fp32")
    pd, dpd = _f(p), _f(dp)
    got, kern = _run("mv_softmax_bwd_f32", lambda y: (_p(pd), _p(dpd), y, rows, cols, 0.5, _stream()), (rows, cols), "fp32")
    _judge(f"softmax_bwd/{rows}x{cols}/{kind}", kern, "softmax_bwd_f32", got, ref, "fp32",
           **({} if kind == "int" else {"mag": mag, "n_ops": -(-cols // 64) + 10}))


@pytest.mark.parametrize("kind", ["int", "gauss"])
@pytest.mark.parametrize("B,N,H,dh", [(2, 65, 2, 8), (1, 5, 3, 72), (1, 64, 1, 16)])
def test_mha_bwd(B, N, H, dh, kind):
    """The four contractions of the kernel's comment in float64 (S.mha_bwd_ref, with the operation counts).  Exact: probs multiples of
    1/8 in a buffer of their own, qkv and dout integers in [-2, 2], scale = 0.25: every value a multiple of 2^-8; the preconditions are
    proven on 2^8 times the values.  N = 65 takes the lane loops' second trip, dh = 72 the d loops', N = 64 fills the wave."""
    qkv, probs, dout = S.mha_bwd_data(B, N, H, dh, kind)
    scale = 0.25 if kind == "int" else float(np.float32(dh ** -0.5))
    r = S.mha_bwd_ref(qkv, probs, dout, scale, H, dh)
    if kind == "int":
        for key in ("ds", "dqkv"):
            S.prove_exact(f"mha_bwd/{key}", r[key][0] * 256.0, r[key][1] * 256.0, [qkv.reshape(B * N, -1).T], out="fp32")
    qd, pd, gd = _f(qkv), _f(probs), _f(dout)
    (ds, dq), kern = _run_n("mv_mha_bwd_f32", lambda ds_, dq_: (_p(qd), _p(pd), _p(gd), ds_, dq_, B, N, H, dh, scale, _stream()),
                            [(B, H, N, N), (B, N, 3 * H * dh)])
    for key, got in (("ds", ds), ("dqkv", dq)):
        ref, mag, n_ops = r[key]
        _judge(f"mha_bwd/{key}/B{B}_N{N}_H{H}_dh{dh}/{kind}", kern, "mha_bwd_f32", got, ref, "fp32",
               **({} if kind == "int" else {"mag": mag, "n_ops": n_ops}))


# ================================================================================================ exact: pools, gathers, layouts
@pytest.mark.parametrize("below", [False, True], ids=["centred", "below_minus_1"])
@pytest.mark.parametrize("k,s,p", [(3, 2, 1), (2, 2, 0), (3, 1, 1)], ids=["3x3s2p1", "2x2s2p0", "3x3s1p1"])
@pytest.mark.parametrize("C", [5, 96])
def test_maxpool_bwd_exact(C, k, s, p, below):
    """Per channel a permutation of distinct integers: no ties, so the gradient is defined and float64 autograd is the reference.
    below_minus_1: every value below -1, so a padded tap read as 0 would win its window.  C = 5 leaves 59 threads of the block idle,
    C = 96 takes the channel loop's second trip."""
    N, H, W = 2, 9, 11
    rng = S.rng_of(65)
    x = S.distinct_ints(rng, (N, H, W, C))
    if below:
        x = x - np.float32(x.max() + 2.0)
        assert (x < -1.0).all()
    Ho, Wo = S.pool_out(H, k, s, p), S.pool_out(W, k, s, p)
    dy = S.int_nz(rng, (N, Ho, Wo, C), 2)
    ref = S.maxpool_bwd64(x, dy, k, s, p)
    S.prove_exact("maxpool_bwd", ref, S.maxpool_bwd64(x, np.abs(dy), k, s, p), [], stored=[dy], out="fp32")
    xd, dyd = _f(x), _f(dy)
    got, kern = _run("mv_maxpool2d_bwd_nhwc_f32", lambda y: (_p(xd), _p(dyd), y, N, H, W, C, k, k, s, s, p, p, _stream()), (N, H, W, C), "fp32")
    _judge(f"maxpool_bwd/C{C}/{k}x{k}s{s}p{p}/{'below' if below else 'centred'}", kern, "maxpool_bwd_f32", got, ref, "fp32")


@pytest.mark.parametrize("B,H,W,C", [(2, 5, 7, 6), (1, 6, 4, 5)])
def test_patch_merge_gather_bwd_exact(B, H, W, C):
    """The forward (mv_patch_merge_gather_nhwc; ops.patch_merge_gather) pads the map with zeros to even sizes and concatenates the
    blocks (0::2, 0::2) | (1::2, 0::2) | (0::2, 1::2) | (1::2, 1::2); the backward is its adjoint: the gradient of a padded tap
    reaches nothing.  (grad.g_patch_merge_gather refuses odd maps today; the kernel does not.)"""
    dy = S.int_nz(S.rng_of(66), (B, (H + 1) // 2, (W + 1) // 2, 4 * C), 64)
    ref = S.patch_merge_bwd_ref(dy, H, W)
    dyd = _f(dy)
    got, kern = _run("mv_patch_merge_gather_bwd_f32", lambda y: (_p(dyd), y, B, H, W, C, _stream()), (B, H, W, C), "fp32")
    _judge(f"patch_merge_bwd/{B}x{H}x{W}x{C}", kern, "patch_merge_bwd_f32", got, ref, "fp32")


@pytest.mark.parametrize("R,C,stride", [(33, 65, 0), (33, 65, 80), (3, 2401, 0)])
def test_transpose2d_exact(R, C, stride):
    """With a row stride the source's columns C .. stride hold the sentinel: none of them may reach the output."""
    ld = stride or C
    x = np.full((R, ld), SENTINEL, np.float32)
    x[:, :C] = S.wide_data(S.rng_of(67), (R, C), "fp32")
    assert not (x[:, :C] == SENTINEL).any()
    xd = _f(x)
    got, kern = _run("mv_transpose2d_f32", lambda y: (_p(xd), y, R, C, stride, _stream()), (C, R), "fp32")
    _judge(f"transpose2d/{R}x{C}/stride{stride}", kern, "transpose2d_f32", got, x[:, :C].T, "fp32")


def test_scatter_rows_sum_exact():
    """49 rows of 3 columns into a table of 30: rows repeat, and table rows that no index names must be written as 0."""
    M, C, T = 49, 3, 30
    rng = S.rng_of(68)
    src = S.int_nz(rng, (M, C), 8)
    idx = rng.integers(0, T - 4, M).astype(np.int32)          # the last four table rows are never hit
    idx[:3] = 7
    hit = np.unique(idx)
    assert len(hit) < M and (np.bincount(idx, minlength=T) > 1).any() and not np.isin(np.arange(T - 4, T), hit).any()
    ref = np.zeros((T, C))
    np.add.at(ref, idx, src.astype(F64))
    sd, idxd = _f(src), torch.from_numpy(idx).cuda()
    got, kern = _run("mv_scatter_rows_sum_f32", lambda y: (_p(sd), _p(idxd), y, M, C, T, _stream()), (T, C), "fp32")
    _judge("scatter_rows_sum", kern, "scatter_rows_sum_f32", got, ref, "fp32")
    assert (got[T - 4:] == 0).all()


# ================================================================================================ tolerance of _cases.py, new shapes
XENT = [("B70_K65", 70, 65, None, False), ("B3_K1000", 3, 1000, None, False), ("B5_K10_logit90", 5, 10, 90.0, False),
        ("B4_K33_soft", 4, 33, None, True)]


@pytest.mark.parametrize("tag,B,K,reach,soft", XENT, ids=[c[0] for c in XENT])
def test_softmax_xent(tag, B, K, reach, soft):
    """K = 65 / 1000: the lane loop's second and sixteenth trip; B = 70: mean_kernel's second; |logit| up to 90: exp overflows fp32
    without the max subtraction; soft targets whose rows sum to 0.5 and 1.0 (loss = ts lse - sum t l).  Tolerance: xent_adam_case's."""
    rng = S.rng_of(69)
    logits = (3 * rng.standard_normal((B, K))).astype(np.float32)
    if reach:
        logits = (logits * (reach / np.abs(logits).max())).astype(np.float32)
        assert 89.0 < np.abs(logits).max() <= 90.001
    if soft:
        t = rng.uniform(0.0, 1.0, (B, K))
        t = (t / t.sum(-1, keepdims=True) * np.array([0.5, 1.0] * (B // 2))[:, None]).astype(np.float32)
    else:
        t = np.zeros((B, K), np.float32)
        t[np.arange(B), rng.integers(0, K, B)] = 1
    rows, mean, dl = S.xent64(logits, t)
    ld, td = _f(logits), _f(t)
    (g_rows, g_mean, g_dl), kern = _run_n("mv_softmax_xent_f32", lambda a, b, c: (_p(ld), _p(td), a, b, c, B, K, _stream()), [(B,), (1,), (B, K)])
    for name, got, ref in (("loss_rows", g_rows, rows), ("loss_mean", g_mean, np.asarray([mean])), ("dlogits", g_dl, dl)):
        assert np.isfinite(got).all(), (tag, name)
        _tol(f"softmax_xent/{tag}/{name}", kern, "softmax_xent_f32", got, ref)


@pytest.mark.parametrize("use_gamma", [True, False], ids=["gamma", "no_gamma"])
@pytest.mark.parametrize("M,C", [(5, 33), (2, 130), (7, 64)])
def test_layernorm_bwd(M, C, use_gamma):
    """C = 33 leaves lanes idle, 130 takes three trips, 64 fills the wave; M = 5 and 7 leave rows of the last block of four idle."""
    rng = S.rng_of(71)
    x, dy = (1.5 * rng.standard_normal((M, C))).astype(np.float32), rng.standard_normal((M, C)).astype(np.float32)
    gam = rng.uniform(0.5, 1.5, C).astype(np.float32) if use_gamma else None
    eps = float(np.float32(1e-5))
    dx, dyxh = S.layernorm_bwd64(x, gam, dy, eps)
    xd, dyd, gd = _f(x), _f(dy), (_f(gam) if use_gamma else None)
    (g_dx, g_xh), kern = _run_n("mv_layernorm_bwd_f32", lambda a, b: (_p(xd), _p(gd), _p(dyd), a, b, M, C, eps, _stream()), [(M, C), (M, C)])
    _tol(f"layernorm_bwd/{M}x{C}/dx", kern, "layernorm_bwd_f32", g_dx, dx)
    _tol(f"layernorm_bwd/{M}x{C}/dy_xhat", kern, "layernorm_bwd_f32", g_xh, dyxh)


@pytest.mark.parametrize("act", ["relu", "gelu_tanh", "hard_swish", "hard_sigmoid", "sigmoid", "silu"])
def test_act_bwd(act):
    """dx = dy act'(x) on S.act_input (exact hits on -3, 0 and 3), n = 1031.  At the corners the reference takes the side
    act_bwd_kernel's comparisons take (S.act_grad64): relu 0 at 0; hard_sigmoid 0 at -3 and at 3; hard_swish 0 at -3 and 1 at 3."""
    n = 1031
    rng = S.rng_of(72)
    x, dy = S.act_input(rng, n, "fp32"), rng.standard_normal(n).astype(np.float32)
    assert {-3.0, 0.0, 3.0} <= set(x.tolist())
    ref = dy.astype(F64) * S.act_grad64(x, act)
    xd, dyd = _f(x), _f(dy)
    got, kern = _run("mv_act_bwd_f32", lambda y: (_p(dyd), _p(xd), y, n, S.ACT_CODES[act], _stream()), (n,), "fp32")
    _tol(f"act_bwd/{act}", kern, "act_bwd_f32", got, ref)
    corners = np.isin(x, (-3.0, 0.0, 3.0))
    if act in ("relu", "hard_swish", "hard_sigmoid"):
        assert np.abs(got[corners] - ref[corners]).max() <= 1e-6, (act, got[corners], ref[corners])


SWIN = [(1, 8, 8, 8, 2, (4, 4), (2, 2)), (1, 8, 16, 16, 2, (8, 8), (0, 3)), (2, 6, 9, 6, 1, (3, 3), (1, 1))]


@pytest.mark.parametrize("B,Hf,Wf,C,heads,ws,shift", SWIN, ids=["8x8_w4x4_s22", "8x16_w8x8_s03", "6x9_w3x3_s11"])
def test_swin_window_attn_bwd(B, Hf, Wf, C, heads, ws, shift):
    """16 and 9 tokens leave threads of the block idle, 64 fill it; 8x16 is one window high (the entry drops that axis's shift, the
    reference too), so the shift acts on the columns only; 6x9 is a rectangular map."""
    rng = S.rng_of(73)
    n = ws[0] * ws[1]
    qkv = rng.standard_normal((B, Hf, Wf, 3 * C)).astype(np.float32)
    bias = (0.5 * rng.standard_normal((heads, n, n))).astype(np.float32)
    dout = rng.standard_normal((B, Hf, Wf, C)).astype(np.float32)
    dq_ref, g_ref = S.swin_bwd64(qkv, bias, dout, heads, ws, shift)
    qd, bd, gd = _f(qkv), _f(bias), _f(dout)
    (dq, gw), kern = _run_n("mv_swin_window_attn_bwd_f32",
                            lambda a, b: (_p(qd), _p(bd), _p(gd), a, b, B, Hf, Wf, C, heads, ws[0], ws[1], shift[0], shift[1], _stream()),
                            [dq_ref.shape, g_ref.shape])
    _tol(f"swin_attn_bwd/{Hf}x{Wf}/dqkv", kern, "swin_attn_bwd_f32", dq, dq_ref)
    _tol(f"swin_attn_bwd/{Hf}x{Wf}/g_windows", kern, "swin_attn_bwd_f32", gw, g_ref)
