"""CPU: the host half of `eqxvision_amd.preprocess` -- geometry, tap tables, refusals -- and the float64 restatement the GPU tests
compare the kernel with (tests/_preprocess_ref.py) against torch's own antialiased bilinear resize."""
import numpy as np
import pytest
import torch

import eqxvision_amd as eqv
from eqxvision_amd import preprocess as P
from tests import _preprocess_ref as R


@pytest.mark.parametrize("name", list(R.CASES))
def test_reference_agrees_with_torch(name):
    """The restatement in float64 (weights NOT rounded) against interpolate(mode="bilinear", antialias=True, align_corners=False) on
    float64 CPU tensors, then crop and normalise.  Both evaluate the same filter in float64; they differ by summation order only:
    a few 2^-53 per tap relative to values <= 1, so 1e-12 on the [0, 1] scale is three orders of slack, and the same divided by
    the smallest std (0.224) after normalising."""
    (hin, win), resized, box = R.CASES[name]
    u8 = R.images((hin, win))
    r01, norm = R.torch_pipeline(u8, resized, box, R.IMAGENET_MEAN, R.IMAGENET_STD)
    a, b = R.affine64(R.IMAGENET_MEAN, R.IMAGENET_STD)
    y, _ = R.reference(u8, resized, box, a, b, round_weights=False)
    y01, _ = R.reference(u8, resized, box, np.full(3, 1.0 / 255.0), np.zeros(3), round_weights=False)
    e01, en = float(np.abs(y01 - r01).max()), float(np.abs(y - norm).max())
    print(f"{name}: |ref - torch| = {e01:.3e} on [0, 1], {en:.3e} normalised")
    assert e01 <= 1e-12
    assert en <= 1e-12 / 0.224


@pytest.mark.parametrize("hw", [(500, 375), (375, 500), (256, 256), (224, 224), (257, 1000)])
def test_geometry_is_torchvisions(hw):
    """torchvision.transforms.Resize(256) / CenterCrop(224), written out: the short side becomes 256, the long one
    int(256 * long / short); the crop starts at int(round((resized - 224) / 2.0))."""
    h, w = hw
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = 256, int(256 * long / short)
    want = (new_long, new_short) if w <= h else (new_short, new_long)
    assert P.resized_size(h, w, 256) == want
    hr, wr = want
    assert P.center_crop_box(hr, wr, 224) == (int(round((hr - 224) / 2.0)), int(round((wr - 224) / 2.0)), 224, 224)


def test_preset_case_is_the_preset():
    (hin, win), resized, box = R.CASES["preset"]
    assert P.resized_size(hin, win, 256) == resized
    assert P.center_crop_box(resized[0], resized[1], 224) == box


@pytest.mark.parametrize("name", list(R.CASES))
def test_tables(name):
    """Rows sum to 1 within 2^-22, taps inside [0, in), tap count within the declared maximum, padding zero; and the tables are
    the dense filter of the reference rounded once to fp32 (2^-24 relative; the two normalise in float64 with sums taken in a
    different order, which moves the value before rounding by parts in 1e16, and a tap
    on the very edge of the support may carry 1e-17 in one and be left out of the other)."""
    (hin, win), (hr, wr), (top, left, hout, wout) = R.CASES[name]
    for n_in, n_out, start, count in ((hin, hr, top, hout), (win, wr, left, wout)):
        first, taps, w = P.axis_table(n_in, n_out, start, count)
        assert first.dtype == np.int32 and taps.dtype == np.int32 and w.dtype == np.float32
        assert w.shape == (count, int(taps.max())) and w.shape[1] <= P.MAX_TAPS == R.MAX_TAPS
        assert np.all(np.abs(w.astype(np.float64).sum(1) - 1.0) <= 2.0 ** -22)
        assert np.all(first >= 0) and np.all(taps >= 1) and np.all(first + taps <= n_in)
        assert all(np.all(w[i, taps[i]:] == 0) for i in range(count))
        want = R.weights64(n_in, n_out)[start:start + count]
        got = R.dense(first, taps, w, n_in)
        assert np.all(np.abs(got - want) <= 2.0 ** -24 * want + 1e-15)
        packed = P.pack_table(first, taps, w)
        assert packed.dtype == np.int32 and packed.shape == (count * (2 + w.shape[1]),)
        assert np.array_equal(packed[2 * count:].view(np.float32).reshape(w.shape), w)


@pytest.mark.parametrize("n", [1, 7, 224])
def test_table_of_equal_sizes_is_the_identity(n):
    first, taps, w = P.axis_table(n, n)
    assert np.array_equal(first, np.arange(n)) and np.all(taps == 1) and w.shape == (n, 1) and np.all(w == 1.0)


def test_affine_vectors():
    a, b = P.affine(P.IMAGENET_MEAN, P.IMAGENET_STD)
    a64, b64 = R.affine64(R.IMAGENET_MEAN, R.IMAGENET_STD)
    assert a.dtype == np.float32 and np.array_equal(a, a64.astype(np.float32)) and np.array_equal(b, b64.astype(np.float32))


def test_refusals_before_any_launch(monkeypatch):
    """Each raises ValueError on the host; `_lib.call` and the device are never reached (this machine has neither)."""
    from eqxvision_amd import _lib

    def no_launch(*a, **k):
        raise AssertionError("a refused call reached the library")
    monkeypatch.setattr(_lib, "call", no_launch)
    monkeypatch.setattr(P, "device", no_launch)
    ok = np.zeros((2, 40, 30, 3), np.uint8)
    with pytest.raises(ValueError, match="uint8"):
        P.imagenet_eval(ok.astype(np.float32))
    with pytest.raises(ValueError, match="uint8"):
        P.imagenet_eval(torch.zeros((2, 3, 40, 30)))
    with pytest.raises(ValueError, match="3 channels"):
        P.imagenet_eval(np.zeros((2, 40, 30, 4), np.uint8))
    with pytest.raises(ValueError, match="3 channels"):
        P.imagenet_eval(np.zeros((2, 40, 3, 30), np.uint8), channels_last=True)
    with pytest.raises(ValueError, match="does not lie inside"):
        P.imagenet_eval(ok, resize=16, crop=24)                     # resized to 21 x 16: a 24 x 24 crop is larger
    with pytest.raises(ValueError, match="does not lie inside"):
        P.resize_crop_normalize(ok, (20, 20), (4, 0, 17, 20))
    with pytest.raises(ValueError, match="filter taps"):
        P.resize_crop_normalize(np.zeros((1, 260, 8, 3), np.uint8), (20, 8), (0, 0, 20, 8))     # 13x: 27 taps
    with pytest.raises(ValueError, match="layout"):
        P.imagenet_eval(ok, resize=16, crop=8, layout="nhwc")
    with pytest.raises(ValueError, match="dtype"):
        P.imagenet_eval(ok, resize=16, crop=8, dtype="fp16")


def test_exported():
    assert eqv.preprocess is P and callable(eqv.preprocess.imagenet_eval) and callable(eqv.preprocess.resize_crop_normalize)
