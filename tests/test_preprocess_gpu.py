"""GPU: `mv_preprocess_u8_fwd` and `eqxvision_amd.preprocess` against the float64 restatement of tests/_preprocess_ref.py.

Every kernel run goes twice, each time into a fresh sentinel-filled buffer with a guard behind it: the two results must have the
same bits, every element must have been written, the guard must be untouched.  Where the arithmetic is exact the comparison is
bit for bit; elsewhere it is the per-element bound derived in `_preprocess_ref.reference` -- not a measured tolerance -- and the
worst error-to-bound ratio is printed."""
import functools

import numpy as np
import pytest
import torch

import eqxvision_amd as eqv
from eqxvision_amd import _lib
from eqxvision_amd import preprocess as P
from tests import _preprocess_ref as R
from tests._cases import TOL_F32
from tests._slices import GUARD, SENTINEL, _stream

pytestmark = pytest.mark.gpu

MV_E_UNSUPPORTED = -2


def _affine(kind):
    if kind == "unit":
        return np.ones(3, np.float32), np.zeros(3, np.float32)
    return P.affine(P.IMAGENET_MEAN, P.IMAGENET_STD)


def _tables(case):
    (hin, win), (hr, wr), (top, left, hout, wout) = R.CASES[case]
    return P.axis_table(hin, hr, top, hout), P.axis_table(win, wr, left, wout)


def _run(u8_hwc, case, a, b, chw=False, dtype="fp32", nhwc=False):
    """Two launches of the entry on `u8_hwc` [B, H, W, 3] (given to the kernel as CHW when `chw`); returns the result as float64
    [B, 3, Hout, Wout] whatever the layout it was stored in."""
    (hin, win), (hr, wr), (top, left, hout, wout) = R.CASES[case]
    th, tw = _tables(case)
    B = u8_hwc.shape[0]
    x = torch.from_numpy(np.ascontiguousarray(u8_hwc.transpose(0, 3, 1, 2) if chw else u8_hwc)).cuda()
    dev = [torch.from_numpy(v).cuda() for v in (P.pack_table(*th), P.pack_table(*tw), a, b)]
    n = B * 3 * hout * wout
    tdt = torch.float32 if dtype == "fp32" else torch.bfloat16
    outs = []
    for _ in range(2):
        y = torch.full((n + GUARD,), SENTINEL, dtype=tdt, device="cuda")
        _lib.call("mv_preprocess_u8_fwd", x.data_ptr(), y.data_ptr(), dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(),
                  dev[3].data_ptr(), B, hin, win, hr, wr, top, left, hout, wout, th[2].shape[1], tw[2].shape[1], int(chw),
                  P.DT[dtype], int(nhwc), _stream())
        outs.append(y)
    torch.cuda.synchronize()
    _lib.check_device_status()
    raw = [o.view(torch.int32 if dtype == "fp32" else torch.int16).cpu().numpy() for o in outs]
    assert np.array_equal(raw[0], raw[1]), (case, "two runs differ")
    host = outs[0].float().cpu().numpy().astype(np.float64)
    assert np.all(host[n:] == SENTINEL), (case, "guard overwritten")
    assert not np.any(host[:n] == SENTINEL) and np.isfinite(host[:n]).all(), (case, "elements left unwritten")
    y = host[:n].reshape((B, hout, wout, 3) if nhwc else (B, 3, hout, wout))
    return y.transpose(0, 3, 1, 2) if nhwc else y


@functools.lru_cache(maxsize=None)
def _ref(case, kind, B=2):
    """(images, y, bound) of a case, computed once: the float64 reference on the fp32 weights and affine vectors the kernel gets."""
    (hin, win), resized, box = R.CASES[case]
    u8 = R.images((hin, win), B)
    a, b = _affine(kind)
    th, tw = _tables(case)
    y, bound = R.reference(u8, resized, box, a, b, wh=R.dense(*th, hin), ww=R.dense(*tw, win))
    for v in (u8, y, bound):
        v.setflags(write=False)
    return u8, y, bound


def _check_bound(tag, got, y, bound, bf16=False):
    if bf16:                       # one more rounding, of the fp32 value to 8 bits: half a bf16 ulp at the largest it can be
        bound = bound + R.bf16_half_ulp(np.abs(y) + bound)
    err = np.abs(got - y)
    ratio = float((err / bound).max())
    print(f"{tag}: worst |got - ref| / bound = {ratio:.3f} (max err {err.max():.3e})")
    assert np.all(err <= bound), (tag, ratio, np.argwhere(err > bound)[:8].tolist())
    return ratio


def test_identity_is_the_affine_map_bit_for_bit():
    """8x8 -> 8x8: one tap of weight 1.0 per axis, so acc is the pixel and the output must be fma(p, a, b) in fp32.  The host
    forms p * a + b in float64: p has 8 bits, a 24, the product 32 (exact); it is a multiple of ulp(a) >= 2^-30 below 2^3 and b
    a multiple of 2^-23, so the sum needs at most 33 bits -- exact in float64 -- and `astype(float32)` is the fma's one rounding.
    bf16: that value rounded once more, ties to even."""
    u8, _, _ = _ref("identity", "imagenet")
    a, b = _affine("imagenet")
    want = (u8.astype(np.float64).transpose(0, 3, 1, 2) * a.astype(np.float64).reshape(1, 3, 1, 1)
            + b.astype(np.float64).reshape(1, 3, 1, 1)).astype(np.float32)
    got = _run(u8, "identity", a, b)
    assert np.array_equal(got.astype(np.float32).view(np.int32), want.view(np.int32))
    got16 = _run(u8, "identity", a, b, dtype="bf16")
    want16 = torch.from_numpy(want).to(torch.bfloat16).float().numpy()
    assert np.array_equal(got16.astype(np.float32).view(np.int32), want16.view(np.int32))


def test_exact_2x_downsampling():
    """16x24 -> 8x12: interior weights 1/8 3/8 3/8 1/8 (the border rows renormalise by 7/4 and are not dyadic).  With a = 1, b = 0
    every difference, product and sum of an interior output is a small multiple of 1/64: exact in fp32, so the kernel must give
    the float64 reference bit for bit there; the border outputs answer to the bound."""
    u8, y, bound = _ref("down2", "unit")
    a, b = _affine("unit")
    got = _run(u8, "down2", a, b)
    inner = (slice(None), slice(None), slice(1, -1), slice(1, -1))
    assert np.array_equal(got[inner].astype(np.float32), y[inner].astype(np.float32))
    assert np.array_equal(y[inner], y[inner].astype(np.float32).astype(np.float64))          # the claim itself: nothing to round
    _check_bound("down2", got, y, bound)


@pytest.mark.parametrize("case", ["ragged", "up", "down8", "multi"])
def test_per_element_bound(case):
    u8, y, bound = _ref(case, "imagenet")
    a, b = _affine("imagenet")
    _check_bound(case, _run(u8, case, a, b), y, bound)


@pytest.mark.parametrize("variant", ["chw_in", "nhwc_out", "bf16_out"])
def test_layout_and_dtype_variants(variant):
    u8, y, bound = _ref("ragged", "imagenet")
    a, b = _affine("imagenet")
    got = _run(u8, "ragged", a, b, chw=variant == "chw_in", nhwc=variant == "nhwc_out",
               dtype="bf16" if variant == "bf16_out" else "fp32")
    _check_bound(f"ragged/{variant}", got, y, bound, bf16=variant == "bf16_out")


def test_imagenet_eval_preset():
    """The real preset on a small image through the public wrapper, B = 3: 300x260 -> 295x256 -> centre 224x224 (7 x 7 tiles)."""
    u8, y, bound = _ref("preset", "imagenet", 3)
    for src in (u8, torch.from_numpy(u8).cuda(), np.ascontiguousarray(u8.transpose(0, 3, 1, 2))):
        out = P.imagenet_eval(src)
        assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (3, 3, 224, 224)
        _check_bound("preset", out.cpu().numpy().astype(np.float64), y, bound)
    out = P.imagenet_eval(u8, dtype="bf16")
    assert out.dtype == torch.bfloat16
    _check_bound("preset/bf16", out.float().cpu().numpy().astype(np.float64), y, bound, bf16=True)
    one = P.imagenet_eval(u8[1])
    assert tuple(one.shape) == (3, 224, 224)
    _check_bound("preset/single", one.cpu().numpy().astype(np.float64)[None], y[1:2], bound[1:2])
    _lib.check_device_status()


@pytest.mark.parametrize("case", ["ragged", "up", "down8"])
def test_constant_image(case):
    """A flat image stays flat: every output of channel c is fma(v, a[c], b[c]) within 2 ulp, borders included -- weights that do
    not sum to 1 where the filter is cut off by the edge of the image show up here."""
    (hin, win), _, _ = R.CASES[case]
    a, b = _affine("imagenet")
    for v in (0, 255, 128):
        u8 = np.full((1, hin, win, 3), v, np.uint8)
        want = (v * a.astype(np.float64) + b.astype(np.float64)).astype(np.float32)          # exact in float64, as in the identity test
        got = _run(u8, case, a, b)
        ulps = np.abs(got - want.astype(np.float64).reshape(1, 3, 1, 1)) / np.spacing(np.abs(want)).astype(np.float64).reshape(1, 3, 1, 1)
        print(f"{case} v={v}: worst {ulps.max():.2f} ulp")
        assert ulps.max() <= 2.0, (case, v, float(ulps.max()))


@functools.lru_cache(maxsize=None)
def _resnet18():
    from oracle import state as S
    from tests._model_cases import _load
    return _load(eqv.models.resnet18, S.resnet_state(1, "basic", (2, 2, 2, 2), 10), num_classes=10)


def _forward(net, x):
    keys = eqv.random.split(eqv.random.PRNGKey(0), x.shape[0])
    return eqv.vmap(net, axis_name="batch")(x, key=keys)


def test_end_to_end_resnet18():
    """vmap(resnet18)(imagenet_eval(u8)) against vmap(resnet18)(x_ref), x_ref the float64 reference rounded to fp32, fp32 mode."""
    u8, y, _ = _ref("preset", "imagenet", 3)
    net = _resnet18()
    with eqv.precision("fp32"):
        got = _forward(net, P.imagenet_eval(u8)).cpu().numpy()
        ref = _forward(net, torch.from_numpy(y.astype(np.float32)).cuda()).cpu().numpy()
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"resnet18 logits: max |got - ref| = {err:.3e} (limit {TOL_F32})")
    assert np.isfinite(got).all() and err <= TOL_F32


def test_captured_in_a_graph():
    """filter_jit of preprocess + model: the recording call, the capturing call and the replay return the bits of an eager call; a
    replay on new pixels in the same buffer follows them (the launch is in the graph, the input is read in place)."""
    u8, _, _ = _ref("preset", "imagenet", 3)
    net = _resnet18()
    x = torch.from_numpy(u8).cuda()
    with eqv.precision("fp32"):
        eager = _forward(net, P.imagenet_eval(x)).cpu().numpy()
        fwd = eqv.filter_jit(lambda n, im: _forward(n, P.imagenet_eval(im)))
        outs = [fwd(net, x).cpu().numpy() for _ in range(3)]
        for o in outs:
            assert np.array_equal(o.view(np.int32), eager.view(np.int32))
        flipped = torch.from_numpy(np.ascontiguousarray(u8[:, ::-1])).cuda()
        eager2 = _forward(net, P.imagenet_eval(flipped)).cpu().numpy()
        x.copy_(flipped)
        again = fwd(net, x).cpu().numpy()
        assert np.array_equal(again.view(np.int32), eager2.view(np.int32)) and not np.array_equal(again, eager)
        host = eqv.filter_jit(lambda n, im: _forward(n, P.imagenet_eval(im)))      # a host array: staged as uint8, refreshed per call
        for im, want in ((u8, eager), (u8, eager), (np.ascontiguousarray(u8[:, ::-1]), eager2)):
            assert np.array_equal(host(net, im).cpu().numpy().view(np.int32), want.view(np.int32))
    _lib.check_device_status()


def test_inside_value_and_grad():
    """Under the tape the launch is allowed and its output is a constant (the input is data): a step that preprocesses inside
    `filter_value_and_grad` gives the loss of the step that was handed the preprocessed tensor."""
    u8, _, _ = _ref("preset", "imagenet", 3)
    net = _resnet18()
    x = torch.from_numpy(u8).cuda()
    labels = np.arange(3) % 10
    keys = eqv.random.split(eqv.random.PRNGKey(0), 3)

    def loss_of(prep):
        @eqv.filter_value_and_grad
        def step(model, im, y):
            out = eqv.vmap(model, axis_name="batch")(prep(im), key=keys)
            return eqv.optim.softmax_cross_entropy(out, eqv.optim.one_hot(y, 10)).mean()
        return step

    with eqv.precision("fp32"):
        inside, _ = loss_of(P.imagenet_eval)(net, x, labels)
        outside, _ = loss_of(lambda im: im)(net, P.imagenet_eval(x), labels)
    assert np.isfinite(float(inside)) and float(inside) == float(outside)


def test_refusals():
    """More taps than the maximum and a crop outside the resized image: MV_E_UNSUPPORTED with a message, nothing launched, the
    device status clean afterwards."""
    lib = _lib.load()
    x = torch.zeros((1, 260, 8, 3), dtype=torch.uint8, device="cuda")
    y = torch.full((3 * 20 * 8 + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    tab = torch.zeros((4096,), dtype=torch.int32, device="cuda")
    ab = torch.ones((3,), dtype=torch.float32, device="cuda")

    def call(hin, win, hr, wr, top, left, hout, wout, mh, mw, xp=None, yp=None):
        return lib.mv_preprocess_u8_fwd(x.data_ptr() if xp is None else xp, y.data_ptr() if yp is None else yp, tab.data_ptr(),
                                        tab.data_ptr(), ab.data_ptr(), ab.data_ptr(), 1, hin, win, hr, wr, top, left, hout, wout,
                                        mh, mw, 0, _lib.F32, 0, _stream())

    assert call(260, 8, 20, 8, 0, 0, 20, 8, 24, 1) == MV_E_UNSUPPORTED              # 13x: 27 taps needed
    assert b"taps" in lib.mv_last_error()
    assert call(64, 8, 8, 8, 0, 0, 8, 8, P.MAX_TAPS + 1, 1) == MV_E_UNSUPPORTED     # a table wider than the maximum
    assert b"taps" in lib.mv_last_error()
    for box in ((1, 0, 8, 8), (0, 1, 8, 8), (-1, 0, 8, 8), (0, 0, 9, 8)):
        assert call(16, 16, 8, 8, *box, 4, 4) == MV_E_UNSUPPORTED
        assert b"crop" in lib.mv_last_error()
    assert call(16, 16, 8, 8, 0, 0, 8, 8, 4, 4, yp=0) == MV_E_UNSUPPORTED
    assert b"null" in lib.mv_last_error()
    assert call(16, 8, 8, 8, 0, 0, 8, 8, 4, 1, yp=x.data_ptr() + 64) == MV_E_UNSUPPORTED
    assert b"overlap" in lib.mv_last_error()
    with pytest.raises(_lib.MVError, match="crop"):
        _lib.call("mv_preprocess_u8_fwd", x.data_ptr(), y.data_ptr(), tab.data_ptr(), tab.data_ptr(), ab.data_ptr(), ab.data_ptr(),
                  1, 16, 16, 8, 8, 4, 4, 8, 8, 4, 4, 0, _lib.F32, 0, _stream())
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all())
    assert _lib.check_device_status() == 0
