"""`-m gpu`: `eqxvision_amd.postprocess` on the MI355X -- the label kernel (mv_resize_argmax_nhwc_fwd) and the softmax + top-k kernel
(mv_softmax_topk_f32) through the C ABI, then `segment` / `upsample_argmax` / `topk` at model level and under `filter_jit`.

Every direct kernel call runs twice, into two buffers filled with two DIFFERENT sentinels and followed by a guard region: the two
results must be byte-equal (so every element was written, and written the same) and both guards untouched."""
import functools

import numpy as np
import pytest
import torch

import eqxvision_amd as eqv
from eqxvision_amd import _lib
from eqxvision_amd import postprocess as P
from tests import _postprocess_ref as R
from tests import _strict as S

pytestmark = pytest.mark.gpu

GUARD = 256                      # bytes behind (and in front of) every destination
SENT = (0xEE, 0x11)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev_logits(x, dtype):
    t = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
    return t.to(torch.bfloat16) if dtype == "bf16" else t


def _twice(nbytes, launch, skew=0):
    """launch(ptr) twice into sentinel-filled byte buffers [GUARD + skew | nbytes | GUARD] -> the nbytes of the result (numpy uint8);
    `skew` moves the destination off the allocation's alignment."""
    outs, front = [], GUARD + skew
    for s in SENT:
        buf = torch.full((front + nbytes + GUARD,), s, dtype=torch.uint8, device="cuda")
        launch(buf.data_ptr() + front)
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        assert np.all(host[:front] == s) and np.all(host[front + nbytes:] == s), "guard overwritten"
        outs.append(host[front:front + nbytes].copy())
    assert np.array_equal(outs[0], outs[1]), "two runs differ, or bytes were left unwritten"
    return outs[0]


def _labels(x, H, W, dtype="fp32"):
    """(labels uint8 (N, H, W), kernel name) of NHWC logits x through the C entry."""
    N, h, w, C = x.shape
    t = _dev_logits(x, dtype)
    got = _twice(N * H * W, lambda p: _lib.call("mv_resize_argmax_nhwc_fwd", t.data_ptr(), p, N, h, w, C, H, W,
                                                _lib.BF16 if dtype == "bf16" else _lib.F32, _stream()))
    return got.reshape(N, H, W), _lib.last_kernel()


def _full_resolution(x, H, W, dtype="fp32"):
    """The project's own resize kernel: fp32 NCHW (N, C, H, W), as the segmentation models return it."""
    N, h, w, C = x.shape
    t = _dev_logits(x, dtype)
    y = torch.empty((N, C, H, W), dtype=torch.float32, device="cuda")
    _lib.call("mv_resize_bilinear_nhwc_fwd", t.data_ptr(), y.data_ptr(), N, h, w, C, H, W, _lib.BF16 if dtype == "bf16" else _lib.F32,
              _lib.F32, 1, _stream())
    torch.cuda.synchronize()
    return y.cpu().numpy()


# ------------------------------------------------------------------------------------------------ label kernel, test 1
EXACT = [((2, 5, 7, 21), (40, 56), "fp32"), ((1, 9, 9, 21), (65, 65), "fp32"), ((2, 4, 6, 3), (4, 6), "fp32"),
         ((1, 3, 5, 1), (6, 10), "fp32"), ((1, 2, 3, 256), (5, 7), "fp32"), ((1, 8, 8, 19), (30, 53), "fp32"),
         ((2, 5, 7, 21), (40, 56), "bf16"),
         ((3, 6, 5, 8), (13, 12), "fp32"), ((3, 6, 5, 8), (13, 12), "bf16"), ((1, 4, 4, 16), (9, 11), "bf16")]   # the 16-byte loads


@pytest.mark.parametrize("shape,size,dtype", EXACT, ids=[f"{'x'.join(map(str, c[0]))}_to_{c[1][0]}x{c[1][1]}_{c[2]}" for c in EXACT])
def test_labels_are_the_argmax_of_the_resize_kernel(shape, size, dtype):
    """labels == argmax over the classes (first index) of what mv_resize_bilinear_nhwc_fwd writes as fp32 NCHW: zero mismatches."""
    x = S.rng_of(61).standard_normal(shape).astype(np.float32)
    if shape[3] == 256:
        x[0, 1, 2, 255] = 50.0                               # label 255 must occur
    if dtype == "bf16":
        x = S.bf(x).astype(np.float32)
    got, kern = _labels(x, *size, dtype)
    vec = shape[3] % (8 if dtype == "bf16" else 4) == 0
    assert kern == ("resize_argmax_nhwc_v16" if vec else "resize_argmax_nhwc"), kern
    want = np.argmax(_full_resolution(x, *size, dtype), axis=1)
    bad = int((got != want).sum())
    print(f"{shape} -> {size} {dtype} [{kern}]: {bad} of {want.size} labels differ; classes seen {np.unique(got).size}")
    assert bad == 0
    if shape[3] == 256:
        assert (got == 255).any()
    if shape[3] == 1:
        assert not got.any()


# ------------------------------------------------------------------------------------------------ label kernel, test 2
RATIOS = [((2, 6, 5, 21), 2), ((1, 5, 6, 8), 4), ((1, 5, 6, 21), 4)]


@pytest.mark.parametrize("shape,ratio", RATIOS, ids=[f"{'x'.join(map(str, s))}_x{r}" for s, r in RATIOS])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_integer_logits_select_exactly(shape, ratio, dtype):
    """Integer logits in [-2, 2] at x2 / x4: every weight is a multiple of 1/8, every product and sum a multiple of 1/64 below 8 --
    exact in fp32 (and the inputs exact in bf16), so the labels are the float64 first-index argmax, ties included (asserted: the
    map has ties between the two best classes)."""
    N, h, w, C = shape
    H, W = h * ratio, w * ratio
    x = S.rng_of(62).integers(-2, 3, shape).astype(np.float32)
    ref = R.resize64(x, H, W)
    assert np.array_equal(ref * 64, np.rint(ref * 64))
    assert (R.top2_gap(ref)[2] == 0).mean() > 0.05, "no ties to break"
    got, _ = _labels(x, H, W, dtype)
    assert np.array_equal(got, R.argmax_first(ref, -1))
    # a constant map: every class ties everywhere
    got, _ = _labels(np.full(shape, 1.5, np.float32), H, W, dtype)
    assert not got.any()
    # two identical channels above all others: the lower index everywhere
    y = x.copy()
    y[..., 5] = y[..., 2] = x[..., 2] + 10.0
    got, _ = _labels(y, H, W, dtype)
    assert np.all(got == 2)


@pytest.mark.parametrize("ratio", [2, 4])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_nan_wins_where_its_pixel_is_tapped(ratio, dtype):
    """One NaN in channel 7 of one source pixel: label 7 at exactly the output pixels whose taps include that pixel with a non-zero
    weight (at x2 / x4 no tap of an interior sample has weight zero, so these are all the pixels that read it); channel 7 is -100
    elsewhere, so it wins nowhere else.  A NaN in channels 3 and 7 of the pixel: the first one, 3."""
    N, h, w, C = 2, 5, 6, 21
    H, W = h * ratio, w * ratio
    x = S.rng_of(63).integers(-2, 3, (N, h, w, C)).astype(np.float32)
    x[..., 7] = x[..., 3] = -100.0
    clean = R.argmax_first(R.resize64(x, H, W), -1)
    assert not np.isin(clean, (3, 7)).any()
    for (n, iy, ix) in ((1, 2, 3), (0, 0, 5)):                                    # an interior pixel, a corner-row pixel
        mask = np.zeros((N, H, W), bool)
        mask[n] = np.outer(R.touched_by(h, H, iy), R.touched_by(w, W, ix))
        assert 0 < mask.sum() < H * W
        for chans, winner in (((7,), 7), ((3, 7), 3), ((7, 3), 3)):
            y = x.copy()
            for c in chans:
                y[n, iy, ix, c] = np.nan
            got, _ = _labels(y, H, W, dtype)
            assert np.array_equal(got == winner, mask), (n, iy, ix, chans)
            assert np.array_equal(got[~mask], clean[~mask])


# ------------------------------------------------------------------------------------------------ label kernel, test 3
def _judge_against_float64(labels, ref, bound):
    """Pixels whose label is not the float64 argmax: each needs a float64 top-two gap of at most the sum of the two per-element
    bounds (at most twice the bound), and there may be at most 0.1 % of them.  -> (number of them, worst gap / allowance)."""
    first, second, gap = R.top2_gap(ref)
    allow = np.take_along_axis(bound, first[..., None], -1)[..., 0] + np.take_along_axis(bound, second[..., None], -1)[..., 0]
    diff = labels != first
    worst = float((gap[diff] / allow[diff]).max()) if diff.any() else 0.0
    assert np.all(gap[diff] <= allow[diff]), f"a label differs where the float64 gap is {worst:.2f} x the allowance"
    assert diff.sum() <= 1e-3 * diff.size, f"{int(diff.sum())} of {diff.size} labels differ from the float64 argmax"
    return int(diff.sum()), worst


@pytest.mark.parametrize("shape,size", [((1, 9, 9, 21), (65, 65)), ((1, 8, 8, 19), (30, 53))])
def test_labels_against_float64_at_ragged_ratios(shape, size):
    """Standard-normal logits, independent float64 resize + argmax.  A pixel may differ only where the float64 gap between its two
    best classes is within the per-element bound of the strict suite for the ragged resize (tests/_strict.py: resize_bound,
    (8 + 2 max(h, w)) 2^-23 M + half an fp32 ulp) taken at both classes, and at most 0.1 % of the map may.  The fp32 restatement of
    the kernel arithmetic (S.emu_resize -- without the fused multiply-adds the compiler forms, which move a value by less than the
    bound as well) is held to the same rule on the CPU first: for seed 64 it differs from the float64 argmax at 0 pixels of both
    shapes."""
    N, h, w, C = shape
    H, W = size
    x = S.rng_of(64).standard_normal(shape).astype(np.float32)
    ref, M = S.resize_ref(x, H, W)
    assert float(np.abs(ref - R.resize64(x, H, W)).max()) <= 1e-12          # the suite's float64 resize and this file's agree
    bound = S.resize_bound(ref, M, h, w, "fp32")
    n_emu, _ = _judge_against_float64(np.argmax(S.emu_resize(x, H, W, "fp32"), -1), ref, bound)
    got, _ = _labels(x, H, W)
    n_got, worst = _judge_against_float64(got, ref, bound)
    print(f"{shape} -> {size}: kernel differs from float64 at {n_got} pixels (emulation {n_emu}), worst gap / allowance {worst:.3f}")


def test_unaligned_label_buffer():
    """A destination that does not start on a 4-byte boundary takes the byte stores: the same labels."""
    x = S.rng_of(65).standard_normal((2, 4, 4, 5)).astype(np.float32)
    t = _dev_logits(x, "fp32")
    want, _ = _labels(x, 8, 8)
    got = _twice(2 * 64, lambda p: _lib.call("mv_resize_argmax_nhwc_fwd", t.data_ptr(), p, 2, 4, 4, 5, 8, 8, _lib.F32, _stream()), skew=1)
    assert np.array_equal(got.reshape(2, 8, 8), want)


# ------------------------------------------------------------------------------------------------ public entry
def test_upsample_argmax_inputs():
    """numpy / torch, host / device, fp32 / bf16, one sample / a batch, channels first: all the labels of the C entry."""
    x = S.bf(S.rng_of(66).standard_normal((2, 5, 7, 21))).astype(np.float32)
    want, _ = _labels(x, 20, 21)
    for arg in (x, torch.from_numpy(x), torch.from_numpy(x).cuda(), torch.from_numpy(x).cuda().to(torch.bfloat16)):
        got = P.upsample_argmax(arg, (20, 21))
        assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == (2, 20, 21)
        assert np.array_equal(got.cpu().numpy(), want)
    one = P.upsample_argmax(x[1], (20, 21))
    assert tuple(one.shape) == (20, 21) and np.array_equal(one.cpu().numpy(), want[1])
    chw = P.upsample_argmax(np.ascontiguousarray(x.transpose(0, 3, 1, 2)), (20, 21), channels_last=False)
    assert np.array_equal(chw.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------ model level
SIZE, BATCH, CLASSES = 64, 2, 21


@functools.lru_cache(maxsize=None)
def _net(name):
    if name == "lraspp_mobilenet_v3_large":
        net = eqv.models.lraspp_mobilenet_v3_large(num_classes=CLASSES)
    else:
        net = getattr(eqv.models, name)(num_classes=CLASSES, intermediate_layers=lambda m: [m.layer3, m.layer4], aux_in_channels=1024)
    return eqv.tree_inference(eqv.utils.randomize_batchnorm(net, 1), True)


def _images(seed):
    return S.rng_of(seed).random((BATCH, 3, SIZE, SIZE), dtype=np.float32)


def _keys():
    return eqv.random.split(eqv.random.PRNGKey(0), BATCH)


def _model_labels(net, x):
    """argmax over the classes of what the model itself returns (fp32 [B, classes, H, W])."""
    out = eqv.vmap(net, axis_name="batch")(torch.from_numpy(x).cuda(), key=_keys())[1]
    assert tuple(out.shape) == (BATCH, CLASSES, SIZE, SIZE) and out.dtype == torch.float32
    return np.argmax(out.cpu().numpy(), axis=1)


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
@pytest.mark.parametrize("name", ["fcn", "deeplabv3", "lraspp_mobilenet_v3_large"])
def test_segment_is_the_argmax_of_the_model(name, mode):
    """Same head, same interpolation arithmetic: segment(net, x) == argmax(vmap(net)(x)[1], axis=1), every pixel.  (The heads are
    randomly initialised, so their maps show few classes -- the count is printed; maps with every class are the kernel tests above.)"""
    net, x = _net(name), _images(71)
    with eqv.precision(mode):
        want = _model_labels(net, x)
        got = P.segment(net, torch.from_numpy(x).cuda(), key=_keys())
    assert got.dtype == torch.uint8 and tuple(got.shape) == (BATCH, SIZE, SIZE)
    got = got.cpu().numpy()
    print(f"{name} {mode}: {int((got != want).sum())} labels differ; classes seen {np.unique(want).size}")
    assert np.array_equal(got, want)
    _lib.check_device_status()


def test_segment_under_filter_jit():
    """Recording call, capturing call and replays: two different image batches give two different label maps, each the argmax of the
    model's own result, and they come back as uint8."""
    net = _net("fcn")
    xs = [_images(72), _images(73)]
    with eqv.precision("bf16"):
        wants = [_model_labels(net, x) for x in xs]
        assert not np.array_equal(wants[0], wants[1])
        seg = eqv.filter_jit(P.segment)
        for i in (0, 1, 0, 1):
            got = seg(net, xs[i], key=_keys())
            assert got.dtype == torch.uint8 and tuple(got.shape) == (BATCH, SIZE, SIZE)
            assert np.array_equal(got.cpu().numpy(), wants[i]), f"call with batch {i}"
        assert seg._entries()[0].replays >= 2
    _lib.check_device_status()


def test_segment_refuses_training_mode_and_classifiers():
    x = torch.from_numpy(_images(74)).cuda()
    training = eqv.tree_inference(_net("fcn"), False)
    with pytest.raises(ValueError, match="training mode"):
        P.segment(training, x)
    with pytest.raises(ValueError, match="segmentation model"):
        P.segment(_alexnet(), x)
    with pytest.raises(ValueError, match=r"\[B, 3, H, W\]"):
        P.segment(_net("fcn"), x[0])


# ------------------------------------------------------------------------------------------------ softmax + top-k
def _topk(x, k, want_prob):
    """(values fp32 (B, k), indices int32 (B, k)) through the C entry."""
    B, K = x.shape
    t = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
    out = {}

    def run(which):
        other = torch.empty((B * k,), dtype=torch.int32, device="cuda")
        def launch(p):
            v, i = (p, other.data_ptr()) if which == "values" else (other.data_ptr(), p)
            _lib.call("mv_softmax_topk_f32", t.data_ptr(), v, i, B, K, k, want_prob, _stream())
        return _twice(B * k * 4, launch)
    out["values"] = run("values").view(np.float32).reshape(B, k)
    out["indices"] = run("indices").view(np.int32).reshape(B, k)
    assert _lib.last_kernel() == "softmax_topk"
    return out["values"], out["indices"]


TOPK = [(3, 1000, 5), (1, 1001, 16), (2, 10, 10), (1, 1, 1), (2, 65536, 3)]


@pytest.mark.parametrize("B,K,k", TOPK, ids=[f"{b}x{K}_k{k}" for b, K, k in TOPK])
def test_topk_selection_and_probabilities(B, K, k):
    """Integer logits in [-8, 8] (many ties): indices are the stable descending order exactly; want_prob = 0 returns the gathered
    inputs bit for bit; want_prob = 1 is within (K + 48) 2^-24 p64 of the float64 softmax (R.prob_bound)."""
    x = S.rng_of(81).integers(-8, 9, (B, K)).astype(np.float32)
    p64, v64, idx = R.topk64(x, k)
    vals, got_idx = _topk(x, k, 0)
    assert np.array_equal(got_idx, idx)
    assert np.array_equal(vals.view(np.int32), np.take_along_axis(x, idx, -1).view(np.int32))
    probs, got_idx = _topk(x, k, 1)
    assert np.array_equal(got_idx, idx)
    ratio = float((np.abs(probs.astype(np.float64) - p64) / R.prob_bound(p64, K)).max())
    print(f"B={B} K={K} k={k}: worst |p - p64| / bound = {ratio:.4f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("B,K,k", TOPK, ids=[f"{b}x{K}_k{k}" for b, K, k in TOPK])
def test_topk_of_equal_logits(B, K, k):
    """A row of equal logits: indices 0 .. k - 1, p = 1 / K within the same bound."""
    x = np.full((B, K), 3.0, np.float32)
    probs, idx = _topk(x, k, 1)
    assert np.array_equal(idx, np.broadcast_to(np.arange(k), (B, k)))
    ratio = float((np.abs(probs.astype(np.float64) - 1.0 / K) / R.prob_bound(1.0 / K, K)).max())
    print(f"B={B} K={K} k={k}: worst |p - 1/K| / bound = {ratio:.4f}")
    assert ratio <= 1.0
    vals, idx = _topk(x, k, 0)
    assert np.array_equal(idx, np.broadcast_to(np.arange(k), (B, k))) and np.all(vals == 3.0)


def test_topk_zeros_tie_and_keep_their_sign():
    """-0 and +0 are equal values: ordered by index, and returned with the bits they came with; infinities order as numbers."""
    x = np.array([[0.0, -0.0, 0.0, -0.0, -1.0, np.inf, -np.inf]], np.float32)
    vals, idx = _topk(x, 7, 0)
    assert idx.tolist() == [[5, 0, 1, 2, 3, 4, 6]]
    assert np.array_equal(vals.view(np.int32), x[0, idx[0]][None].view(np.int32))


@functools.lru_cache(maxsize=None)
def _alexnet():
    return eqv.tree_inference(eqv.models.alexnet(num_classes=10), True)


def test_topk_of_a_classifier():
    """topk(vmap(alexnet)(x), 3) against the float64 top-3 of the same logits; single rows and host arrays give the same."""
    x = torch.from_numpy(S.rng_of(82).random((2, 3, 224, 224), dtype=np.float32)).cuda()
    keys = eqv.random.split(eqv.random.PRNGKey(0), 2)
    logits = eqv.vmap(_alexnet(), axis_name="batch")(x, key=keys)
    host = logits.cpu().numpy()
    assert host.shape == (2, 10) and np.abs(host).max() <= 8.0
    p64, v64, idx = R.topk64(host, 3)
    assert np.all(np.diff(v64, axis=-1) < 0), "tied logits: the comparison below would still hold, but say so"
    probs, got = P.topk(logits, 3)
    assert probs.dtype == torch.float32 and got.dtype == torch.int32 and probs.is_cuda and tuple(got.shape) == (2, 3)
    assert np.array_equal(got.cpu().numpy(), idx)
    assert np.all(np.abs(probs.cpu().numpy().astype(np.float64) - p64) <= R.prob_bound(p64, 10))
    vals, got = P.topk(host, 3, probabilities=False)
    assert np.array_equal(got.cpu().numpy(), idx) and np.array_equal(vals.cpu().numpy(), v64.astype(np.float32))
    p1, i1 = P.topk(logits[1], 3)
    assert tuple(i1.shape) == (3,) and np.array_equal(i1.cpu().numpy(), idx[1]) and np.array_equal(p1.cpu().numpy(), probs[1].cpu().numpy())


def test_topk_under_filter_jit():
    """Replays return the int32 indices as int32 and follow the input."""
    top = eqv.filter_jit(lambda l: P.topk(l, 4))
    rows = [S.rng_of(83 + i).integers(-8, 9, (3, 100)).astype(np.float32) for i in range(2)]
    for i in (0, 1, 0, 1):
        probs, idx = top(rows[i])
        p64, _, want = R.topk64(rows[i], 4)
        assert idx.dtype == torch.int32 and probs.dtype == torch.float32
        assert np.array_equal(idx.cpu().numpy(), want)
        assert np.all(np.abs(probs.cpu().numpy().astype(np.float64) - p64) <= R.prob_bound(p64, 100))


def test_refused_inside_value_and_grad():
    """argmax has no gradient: under the tape the launches are refused by the guard, not run."""
    x = S.rng_of(84).standard_normal((1, 4, 4, 5)).astype(np.float32)

    @eqv.filter_value_and_grad
    def step(model, im):
        return P.upsample_argmax(im, (8, 8))
    with pytest.raises(NotImplementedError, match="mv_resize_argmax_nhwc_fwd"):
        step(None, x)
