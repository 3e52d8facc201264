"""CPU: the host half of the training-time input pipeline of `eqxvision_amd.preprocess` -- the box sampler against a numpy
restatement fed the same uniforms, the flips, the records `mv_preprocess_u8_boxes_fwd` receives, every refusal, and the weight
recipe of the kernel (restated in tests/_augment_ref.py) against `axis_table` on every axis the GPU file uses.  The library call
is replaced by one that copies what its pointers point to; "the device" is host memory."""
import ctypes

import numpy as np
import pytest
import torch

from eqxvision_amd import _act, _lib
from eqxvision_amd import preprocess as P
from eqxvision_amd import random as jr
from tests import _augment_ref as A
from tests import _preprocess_ref as R

SIZES = A.SIZES + [(224, 224), (500, 375), (375, 500), (10, 400), (400, 10), (1, 1), (3, 1000)]


def _uniforms(key, B):
    return np.stack([jr.uniform(k, (10, 4)) for k in jr.split(key, B)])


def _bytes_at(ptr, n):
    return np.ctypeslib.as_array((ctypes.c_uint8 * n).from_address(ptr)).copy()


@pytest.fixture
def on_host(monkeypatch):
    calls = []

    def fake_call(name, *a):
        assert name == "mv_preprocess_u8_boxes_fwd" and len(a) == len(_lib.PROTOTYPES[name])
        x, x_bytes, y, rec_host, rec_dev, ca, cb, B, hout, wout, chw, dt, nhwc, stream = a
        calls.append({"x": _bytes_at(x, x_bytes), "rec_host": _bytes_at(rec_host, B * P.BOX.itemsize).view(P.BOX),
                      "rec_dev": _bytes_at(rec_dev, B * P.BOX.itemsize).view(P.BOX), "a": _bytes_at(ca, 12).view(np.float32),
                      "b": _bytes_at(cb, 12).view(np.float32), "B": B, "hout": hout, "wout": wout, "chw": chw, "dtype": dt,
                      "nhwc": nhwc})
        return 0

    monkeypatch.setattr(_lib, "call", fake_call)
    monkeypatch.setattr(P, "device", lambda: torch.device("cpu"))
    monkeypatch.setattr(P, "empty", lambda shape, dtype: torch.empty(tuple(shape), dtype=dtype))
    monkeypatch.setattr(P, "stream_ptr", lambda: 0)
    monkeypatch.setattr(P, "_affines", {})
    return calls


@pytest.fixture
def no_launch(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a refused call reached the library or the device")
    monkeypatch.setattr(_lib, "call", refuse)
    monkeypatch.setattr(P, "device", refuse)


# ---- sampler ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scale,ratio", [((0.08, 1.0), (3 / 4, 4 / 3)), ((0.35, 1.0), (0.5, 2.0)), ((1.0, 1.0), (1.0, 1.0))])
def test_sampler_equals_the_numpy_restatement_on_the_same_uniforms(scale, ratio):
    for seed in range(6):
        key = jr.PRNGKey(seed)
        got = P.random_resized_crop_boxes(key, SIZES, scale, ratio)
        want, _ = A.rrc_boxes(_uniforms(key, len(SIZES)), SIZES, scale, ratio)
        assert got.dtype == np.int32 and got.shape == (len(SIZES), 4)
        assert np.array_equal(got, want), (seed, got.tolist(), want.tolist())


def test_same_key_same_boxes_and_other_keys_other_boxes():
    a, b = P.random_resized_crop_boxes(jr.PRNGKey(7), SIZES), P.random_resized_crop_boxes(jr.PRNGKey(7), SIZES)
    c = P.random_resized_crop_boxes(jr.PRNGKey(8), SIZES)
    assert np.array_equal(a, b) and not np.array_equal(a, c)
    # image i draws from split(key, B)[i]: two equal images in one batch get different boxes
    two = P.random_resized_crop_boxes(jr.PRNGKey(7), [(224, 224), (224, 224)])
    assert not np.array_equal(two[0], two[1])


def test_boxes_lie_inside_their_images_and_winners_respect_scale_and_ratio():
    """A winning attempt has w = round(sqrt(area ar)), h = round(sqrt(area / ar)) with area / (H W) in `scale` and ar in `ratio`:
    each side is within 1/2 of its real value, so (w - 1/2) / (h + 1/2) <= ar <= (w + 1/2) / (h - 1/2) has to meet `ratio`, and
    (w - 1/2)(h - 1/2) <= area <= (w + 1/2)(h + 1/2) has to meet `scale`."""
    scale, ratio = (0.08, 1.0), (3 / 4, 4 / 3)
    winners = 0
    for seed in range(20):
        key = jr.PRNGKey(100 + seed)
        boxes = P.random_resized_crop_boxes(key, SIZES, scale, ratio)
        _, won = A.rrc_boxes(_uniforms(key, len(SIZES)), SIZES, scale, ratio)
        for (H, W), (top, left, h, w), ok in zip(SIZES, boxes.tolist(), won):
            assert h >= 1 and w >= 1 and top >= 0 and left >= 0 and top + h <= H and left + w <= W, ((H, W), (top, left, h, w))
            if ok:
                winners += 1
                assert (w - 0.5) / (h + 0.5) <= ratio[1] and (w + 0.5) / max(h - 0.5, 1e-9) >= ratio[0], ((H, W), h, w)
                assert (w - 0.5) * (h - 0.5) <= scale[1] * H * W and (w + 0.5) * (h + 0.5) >= scale[0] * H * W, ((H, W), h, w)
    assert winners > 100


def test_extreme_aspects_take_the_fallback():
    """10 x 400 (W / H = 40 > 4/3): h = H = 10, w = round(10 * 4/3) = 13, centred: left = (400 - 13) // 2 = 193.
    400 x 10 (W / H = 0.025 < 3/4): w = W = 10, h = round(10 / 0.75) = 13, top = 193.  No attempt can fit: with an aspect inside
    [3/4, 4/3] and 8 % of the area, the shorter side of the box would have to be at least sqrt(320 * 3/4) = 15.5 > 10."""
    for seed in range(5):
        got = P.random_resized_crop_boxes(jr.PRNGKey(seed), [(10, 400), (400, 10)])
        assert got.tolist() == [[0, 193, 10, 13], [193, 0, 13, 10]], got.tolist()
    # an aspect inside the range with no attempt that fits cannot happen at scale <= 1; scale > 1 forces it: the whole image
    got = P.random_resized_crop_boxes(jr.PRNGKey(0), [(30, 30)], scale=(4.0, 5.0))
    assert got.tolist() == [[0, 0, 30, 30]]


def test_sampler_refuses_bad_ranges():
    with pytest.raises(ValueError, match="scale"):
        P.random_resized_crop_boxes(jr.PRNGKey(0), [(8, 8)], scale=(0.5, 0.1))
    with pytest.raises(ValueError, match="ratio"):
        P.random_resized_crop_boxes(jr.PRNGKey(0), [(8, 8)], ratio=(0.0, 1.0))
    with pytest.raises(ValueError, match="image 1"):
        P.random_resized_crop_boxes(jr.PRNGKey(0), [(8, 8), (0, 8)])


def test_random_flips():
    key = jr.PRNGKey(3)
    never, always, half = P.random_flips(key, 64, 0.0), P.random_flips(key, 64, 1.0), P.random_flips(key, 64)
    assert never.dtype == bool and never.shape == (64,) and not never.any() and always.all()
    assert np.array_equal(half, jr.uniform(key, (64,)) < 0.5) and 8 < int(half.sum()) < 56
    assert not np.array_equal(half, P.random_flips(jr.PRNGKey(4), 64))


# ---- the core: records and refusals -------------------------------------------------------------------------------------------

def test_record_is_the_headers_struct():
    assert P.BOX.itemsize == 40
    assert [P.BOX.fields[n][1] for n in P.BOX.names] == [0, 8, 12, 16, 20, 24, 28, 32, 36]


def _images(sizes, chw=False):
    out = [R.images(hw, 1)[0] for hw in sizes]
    return [np.ascontiguousarray(im.transpose(2, 0, 1)) for im in out] if chw else out


@pytest.mark.parametrize("chw", [False, True])
def test_every_form_of_input_becomes_records_of_the_one_entry(on_host, chw):
    ims = _images(A.SIZES[:5], chw)
    boxes = A.BOX_SETS["ends"][:5]
    y = P.crop_resize_normalize(ims, boxes, 32, A.FLIPS[:5], dtype="bf16")
    assert tuple(y.shape) == (5, 3, 32, 32) and y.dtype == torch.bfloat16
    arr = np.stack(_images([A.ARRAY_SHAPE] * 2, chw))
    y = P.crop_resize_normalize(arr, np.asarray(A.ARRAY_BOXES), (32, 40), layout="nhwc")
    assert tuple(y.shape) == (2, 32, 40, 3) and y.dtype == torch.float32
    y = P.crop_resize_normalize(torch.from_numpy(arr[1]), A.ARRAY_BOXES[0], 40, True)
    assert tuple(y.shape) == (3, 40, 40)
    lst, batch, one = on_host
    assert (lst["B"], lst["hout"], lst["wout"], lst["chw"], lst["dtype"], lst["nhwc"]) == (5, 32, 32, int(chw), _lib.BF16, 0)
    assert (batch["B"], batch["hout"], batch["wout"], batch["chw"], batch["dtype"], batch["nhwc"]) == (2, 32, 40, int(chw), _lib.F32, 1)
    assert (one["B"], one["hout"], one["wout"]) == (1, 40, 40)
    offset = 0
    for i, (hw, im) in enumerate(zip(A.SIZES, ims)):
        g = lst["rec_host"][i]
        assert tuple(int(v) for v in g) == (offset, hw[0], hw[1]) + tuple(boxes[i]) + (int(A.FLIPS[i]), 0), i
        assert np.array_equal(lst["x"][offset:offset + im.size], im.reshape(-1)), i
        offset += im.size
    assert offset == lst["x"].size
    H, W = A.ARRAY_SHAPE
    assert [tuple(int(v) for v in g) for g in batch["rec_host"]] == [(i * H * W * 3, H, W) + tuple(A.ARRAY_BOXES[i]) + (0, 0) for i in range(2)]
    assert np.array_equal(batch["x"], arr.reshape(-1))
    assert tuple(int(v) for v in one["rec_host"][0]) == (0, H, W) + tuple(A.ARRAY_BOXES[0]) + (1, 0)
    for c in on_host:
        assert c["rec_host"].tobytes() == c["rec_dev"].tobytes()
    a, b = P.affine(P.IMAGENET_MEAN, P.IMAGENET_STD)
    assert np.array_equal(lst["a"], a) and np.array_equal(lst["b"], b)


def test_imagenet_train_is_the_core_on_the_boxes_and_flips_of_the_split_key(on_host):
    ims = _images(A.SIZES[:5])
    key = jr.PRNGKey(11)
    y = P.imagenet_train(ims, key, size=32, dtype="bf16")
    assert tuple(y.shape) == (5, 3, 32, 32) and y.dtype == torch.bfloat16
    k_box, k_flip = jr.split(key, 2)
    boxes, flips = P.random_resized_crop_boxes(k_box, A.SIZES[:5]), P.random_flips(k_flip, 5)
    P.crop_resize_normalize(ims, boxes, 32, flips, dtype="bf16")
    P.imagenet_train(ims, key, size=32, dtype="bf16")
    first, core, again = on_host
    assert first["rec_host"].tobytes() == core["rec_host"].tobytes() == again["rec_host"].tobytes()
    assert [int(g["flip"]) for g in first["rec_host"]] == [int(f) for f in flips]
    y = P.imagenet_train(np.stack(_images([A.ARRAY_SHAPE] * 2)), key, size=24, scale=(0.5, 1.0), flip_p=1.0)
    assert tuple(y.shape) == (2, 3, 24, 24) and [int(g["flip"]) for g in on_host[-1]["rec_host"]] == [1, 1]


def test_every_refusal_of_the_core_names_the_image_before_any_call(no_launch):
    ok = _images([(40, 30), (30, 40)])
    full = [(0, 0, 40, 30), (0, 0, 30, 40)]
    for bad, word in (((0, 0, 31, 40), "image 1.*does not lie inside"), ((0, 1, 30, 40), "image 1.*does not lie inside"),
                      ((-1, 0, 5, 5), "image 1.*does not lie inside"), ((0, 0, 0, 5), "image 1.*does not lie inside"),
                      ((29, 39, 1, 2), "image 1.*does not lie inside")):
        with pytest.raises(ValueError, match=word):
            P.crop_resize_normalize(ok, [full[0], bad], 16)
    with pytest.raises(ValueError, match="one box per image"):
        P.crop_resize_normalize(ok, full + full[:1], 16)
    with pytest.raises(ValueError, match="one box per image"):
        P.crop_resize_normalize(ok, full[:1], 16)
    with pytest.raises(ValueError, match="integers"):
        P.crop_resize_normalize(ok, np.asarray(full, np.float32), 16)
    with pytest.raises(ValueError, match="one flag per image"):
        P.crop_resize_normalize(ok, full, 16, [True])
    with pytest.raises(ValueError, match="one flag per image"):
        P.crop_resize_normalize(np.stack([ok[0], ok[0]]), [full[0]] * 2, 16, [True, False, True])
    big = [ok[0], np.zeros((400, 400, 3), np.uint8)]
    with pytest.raises(ValueError, match="image 1.*25 filter taps"):
        P.crop_resize_normalize(big, [full[0], (0, 0, 384, 30)], 32)          # 384 / 32 = 12: int(2 * 12 + 1) = 25
    with pytest.raises(ValueError, match="image 1.*filter taps"):
        P.crop_resize_normalize(big, [full[0], (0, 0, 30, 390)], 32)
    with pytest.raises(ValueError, match="output size"):
        P.crop_resize_normalize(ok, full, 0)
    with pytest.raises(ValueError, match="empty"):
        P.crop_resize_normalize([], [], 16)
    with pytest.raises(ValueError, match="image 1.*uint8"):
        P.crop_resize_normalize([ok[0], ok[1].astype(np.float32)], full, 16)
    with pytest.raises(ValueError, match="uint8"):
        P.crop_resize_normalize(np.zeros((2, 8, 8, 3), np.float32), [(0, 0, 8, 8)] * 2, 16)
    with pytest.raises(ValueError, match="dtype"):
        P.crop_resize_normalize(ok, full, 16, dtype="fp16")
    with pytest.raises(ValueError, match="layout"):
        P.crop_resize_normalize(ok, full, 16, layout="hwc")
    with pytest.raises(ValueError, match="std"):
        P.crop_resize_normalize(ok, full, 16, std=(1.0, 0.0, 1.0))
    # a box of 368 down to 32 needs exactly 24 taps and is NOT refused by the plan
    rec, size = P.boxes_plan([(400, 380)], [(16, 6, 368, 368)], None, 32)
    assert size == (32, 32) and int(rec[0]["h"]) == 368 and A.taps_needed(368, 32) == P.MAX_TAPS


def test_the_core_inside_a_recording_is_refused(no_launch):
    ims = _images([(40, 30), (30, 40)])
    with _act.keep_alive([]):
        with pytest.raises(ValueError, match="filter_jit"):
            P.crop_resize_normalize(ims, [(0, 0, 40, 30), (0, 0, 30, 40)], 16)
        with pytest.raises(ValueError, match="filter_jit"):
            P.crop_resize_normalize(np.stack([ims[0], ims[0]]), [(0, 0, 40, 30)] * 2, 16)
        with pytest.raises(ValueError, match="filter_jit"):
            P.imagenet_train(ims, jr.PRNGKey(0), size=16)


def test_entry_validates_the_host_records_before_any_device_call(built_lib):
    """`mv_preprocess_u8_boxes_fwd` checks the host copy of the records before it touches the device: made-up (never
    dereferenced) device addresses, a real host record array.  Each message names the image."""
    rec, (hout, wout) = P.boxes_plan([(40, 30), (400, 44)], [(1, 2, 20, 24), (0, 4, 300, 40)], [False, True], 32)
    x_bytes, X, Y, REC, AB = 40 * 30 * 3 + 400 * 44 * 3, 1 << 20, 2 << 20, 3 << 20, 5 << 20

    def call(r, x_bytes=x_bytes, y=Y, B=2):
        r = np.ascontiguousarray(r)
        return built_lib.mv_preprocess_u8_boxes_fwd(X, x_bytes, y, r.ctypes.data, REC, AB, AB, B, hout, wout, 0, _lib.F32, 0,
                                                    None), built_lib.mv_last_error()

    def changed(i, **kw):
        r = rec.copy()
        for k, v in kw.items():
            r[k][i] = v
        return r

    invalid, unsupported = -1, -2
    for r, kw, rc_want, word in ((changed(1, offset=rec["offset"][1] + 1), {}, invalid, b"image 1: 52800 bytes at offset 3601"),
                                 (changed(0, offset=-1), {}, invalid, b"image 0"),
                                 (rec, {"x_bytes": x_bytes - 1}, invalid, b"image 1"),
                                 (changed(0, Win=0), {}, invalid, b"image 0: bad sizes"),
                                 (changed(1, top=101), {}, invalid, b"image 1: box 300x40 at (101, 4)"),
                                 (changed(0, left=7), {}, invalid, b"image 0: box"),
                                 (changed(0, top=-1), {}, invalid, b"image 0: box"),
                                 (changed(1, w=0), {}, invalid, b"image 1: box"),
                                 (changed(1, h=384, top=0), {}, unsupported, b"image 1: box 384x40 -> 32x32 needs up to 25 x 3 taps"),
                                 (rec, {"y": X + 100}, unsupported, b"overlap")):
        rc, msg = call(r, **kw)
        assert rc == rc_want and word in msg, (rc, msg, word)
    assert call(rec, B=0)[0] == invalid and call(rec, B=70000)[0] == invalid


# ---- the kernel's weight recipe -----------------------------------------------------------------------------------------------

def test_kernel_weight_recipe_is_within_one_ulp_of_axis_table_on_every_axis_of_the_gpu_file():
    """float64, sequential sum in tap order, one rounding to fp32 (tests/_augment_ref.kernel_axis) against `axis_table`, whose
    float64 sum numpy adds in another order: same taps, every weight within one fp32 ulp, and both within one rounding of the
    dense float64 filter of tests/_preprocess_ref.weights64."""
    axes = A.axes_used()
    assert (368, 32) in axes and (1, 32) in axes and (3, 40) in axes and (30, 32) in axes and len(axes) > 20
    worst = 0.0
    for n_box, n_out in axes:
        first, taps, weights = A.kernel_axis(n_box, n_out)
        f, t, w = P.axis_table(n_box, n_out)
        assert np.array_equal(first, f) and np.array_equal(taps, t), (n_box, n_out)
        assert taps.max() <= A.taps_needed(n_box, n_out) <= P.MAX_TAPS, (n_box, n_out)
        exact = R.weights64(n_box, n_out)
        for o in range(n_out):
            got, want = weights[o], w[o, :taps[o]]
            ulp = np.spacing(np.maximum(np.abs(got), np.abs(want)))
            assert np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp), (n_box, n_out, o)
            e = exact[o, first[o]:first[o] + taps[o]]
            assert np.all(np.abs(got.astype(np.float64) - e) <= 2.0 ** -24 * e * (1 + 2.0 ** -20) + 2.0 ** -150), (n_box, n_out, o)
            assert np.count_nonzero(exact[o]) == np.count_nonzero(e)          # nothing outside the taps
            worst = max(worst, float(np.max(np.abs(got.astype(np.float64) - want) / ulp)))
    print(f"worst |kernel recipe - axis_table| = {worst:.2f} ulp over {len(axes)} axes")
