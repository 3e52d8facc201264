"""GPU: `mv_preprocess_u8_boxes_fwd` and `eqxvision_amd.preprocess.crop_resize_normalize` / `imagenet_train` -- crop a box out of
each image, resize it, mirror it, normalise, one launch, the filter generated in the kernel.

Images, boxes and output sizes are those of tests/_augment_ref.py (the host file checks the kernel's weight recipe on the same
axes).  By the entry's tile rule a batch without the 368 x 368 box takes the 32 x 32 tile, a batch with it the 4 x 8 tile when the
output is 32 (11.5x, 24 taps: 59 x 105 staged pixels) and the 8 x 16 tile when it is 40, so the small images are computed in
different tiles with and without it; output 32 is exactly one 32 x 32 tile, output 40 has partial edge tiles."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from eqxvision_amd import _lib
from eqxvision_amd import preprocess as P
from eqxvision_amd import random as jr
from tests import _augment_ref as A
from tests import _preprocess_ref as R
from tests._slices import GUARD, SENTINEL, _stream

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -2


@functools.lru_cache(maxsize=None)
def _images():
    out = tuple(R.images(hw, 1)[0] for hw in A.SIZES)            # HWC; every image holds 0 and 255
    for im in out:
        im.setflags(write=False)
    return out


def _as(im, chw):
    return np.ascontiguousarray(im.transpose(2, 0, 1)) if chw else im


def _crop(im, box):
    top, left, h, w = box
    return im[top:top + h, left:left + w].copy()


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu().numpy()


def _read_status():
    """status word, cleared -- synchronises."""
    v = ctypes.c_uint(0)
    assert _lib.load().mv_device_status(1, ctypes.byref(v)) == 0
    return v.value


def _cases():
    """(name, size, image indices, boxes) for every box set and output size."""
    for name, boxes in A.BOX_SETS.items():
        for size in A.OUT:
            idx = A.usable(boxes, size)
            assert len(idx) == len(boxes), (name, size)
            yield name, size, idx, [boxes[i] for i in idx]


@pytest.mark.parametrize("nhwc", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("chw", [False, True], ids=["hwc_in", "chw_in"])
def test_box_equals_the_physical_crop_bit_for_bit(chw, dtype, nhwc):
    """The core on the whole images with boxes == the core on the boxes copied out as images of their own with full boxes: the
    taps stop at the box, wherever it lies in its image and at whatever byte it starts."""
    kw = dict(dtype=dtype, layout="nhwc" if nhwc else "nchw")
    for name, size, idx, boxes in _cases():
        ims = [_images()[i] for i in idx]
        boxed = _bits(P.crop_resize_normalize([_as(im, chw) for im in ims], boxes, size, A.FLIPS, **kw))
        assert _lib.last_kernel() == "preprocess_u8_boxes"
        crops = [_crop(im, b) for im, b in zip(ims, boxes)]
        full = [(0, 0) + c.shape[:2] for c in crops]
        alone = _bits(P.crop_resize_normalize([_as(c, chw) for c in crops], full, size, A.FLIPS, **kw))
        assert boxed.shape == ((len(ims), size, size, 3) if nhwc else (len(ims), 3, size, size))
        assert np.array_equal(boxed, alone), (name, size, np.argwhere(boxed != alone)[:8].tolist())
    assert _lib.check_device_status() == 0


@pytest.mark.parametrize("nhwc", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_flip_is_torch_flip_of_the_unflipped_output(dtype, nhwc):
    """Flags mixed within one batch: a flagged image is the unflagged result mirrored along W bit for bit, the others are
    untouched -- on one full tile (32) and on partial edge tiles (40), for 32 x 32 and for small tiles."""
    kw = dict(dtype=dtype, layout="nhwc" if nhwc else "nchw")
    flips = torch.tensor(A.FLIPS)
    for name, size, idx, boxes in _cases():
        ims = [_images()[i] for i in idx]
        plain = P.crop_resize_normalize(ims, boxes, size, None, **kw)
        mixed = P.crop_resize_normalize(ims, boxes, size, A.FLIPS, **kw)
        every = P.crop_resize_normalize(ims, boxes, size, [True] * len(ims), **kw)
        mirrored = torch.flip(plain, dims=[2 if nhwc else 3])
        want = torch.where(flips.view(-1, 1, 1, 1).to(plain.device), mirrored, plain)
        assert np.array_equal(_bits(mixed), _bits(want)), (name, size)
        assert np.array_equal(_bits(every), _bits(mirrored)), (name, size)
    assert _lib.check_device_status() == 0


def test_an_image_gives_the_bits_it_gives_alone_and_an_array_those_of_the_list():
    for name, size, idx, boxes in _cases():
        ims = [_images()[i] for i in idx]
        together = _bits(P.crop_resize_normalize(ims, boxes, size, A.FLIPS, dtype="bf16"))
        for i, (im, box) in enumerate(zip(ims, boxes)):
            alone = _bits(P.crop_resize_normalize([im], [box], size, [A.FLIPS[i]], dtype="bf16"))
            assert np.array_equal(alone[0], together[i]), (name, size, i)
    arr = R.images(A.ARRAY_SHAPE, 2)
    for chw in (False, True):
        batch = np.ascontiguousarray(arr.transpose(0, 3, 1, 2)) if chw else arr
        for size in A.OUT:
            as_array = P.crop_resize_normalize(batch, A.ARRAY_BOXES, size, [False, True])
            assert _lib.last_kernel() == "preprocess_u8_boxes" and tuple(as_array.shape) == (2, 3, size, size)
            as_list = P.crop_resize_normalize([batch[0], batch[1]], A.ARRAY_BOXES, size, [False, True])
            on_device = P.crop_resize_normalize(torch.from_numpy(batch).cuda(), A.ARRAY_BOXES, size, [False, True])
            single = P.crop_resize_normalize(batch[1], A.ARRAY_BOXES[1], size, True)
            assert np.array_equal(_bits(as_array), _bits(as_list)) and np.array_equal(_bits(as_array), _bits(on_device))
            assert tuple(single.shape) == (3, size, size) and np.array_equal(_bits(single), _bits(as_array[1]))
    assert _lib.check_device_status() == 0


@functools.lru_cache(maxsize=None)
def _reference(name, size):
    """(y, bound) float64 [B, 3, size, size] of one box set with the flips of A.FLIPS, once: torch on the CPU in float64 on the
    physical crop, then the mirror, then the fp32 a and b of the kernel.  bound = (n_h + n_w + 5) 2^-24 (S |a| + |b|): the
    (n_h + n_w + 3) of tests/_preprocess_ref.reference for the kernel's arithmetic, and 2 x 2^-24 S for the two weight vectors,
    each weight within 2^-24 relative of its float64 value (nothing is negative, so each axis contributes at most 2^-24 S)."""
    a, b = P.affine(P.IMAGENET_MEAN, P.IMAGENET_STD)
    a64, b64 = a.astype(np.float64).reshape(3, 1, 1), b.astype(np.float64).reshape(3, 1, 1)
    ys, bounds = [], []
    for i, box in enumerate(A.BOX_SETS[name]):
        crop = torch.from_numpy(_crop(_images()[i], box)).permute(2, 0, 1)[None].double()
        s = F.interpolate(crop, size=(size, size), mode="bilinear", antialias=True, align_corners=False)[0].numpy()
        nh = A.nonzero_taps(box[2], size).reshape(1, size, 1)
        nw = A.nonzero_taps(box[3], size).reshape(1, 1, size)
        if A.FLIPS[i]:
            s, nw = s[:, :, ::-1], nw[:, :, ::-1]
        ys.append(s * a64 + b64)
        bounds.append((nh + nw + 5) * 2.0 ** -24 * (np.abs(s) * np.abs(a64) + np.abs(b64)))
    y, bound = np.stack(ys), np.stack(bounds)
    y.setflags(write=False)
    bound.setflags(write=False)
    return y, bound


def _entry(ims_hwc, boxes, flips, size, dtype="fp32", rec_dev=None):
    """The C entry on a sentinel-filled output with a guard behind it; returns (float64 [B, 3, size, size] with unwritten
    elements still SENTINEL, the host records).  rec_dev: what to upload instead of the host records."""
    rec, _ = P.boxes_plan([im.shape[:2] for im in ims_hwc], boxes, flips, size)
    a, b = P.affine(P.IMAGENET_MEAN, P.IMAGENET_STD)
    x = torch.from_numpy(np.concatenate([im.reshape(-1) for im in ims_hwc])).cuda()
    dev = [torch.from_numpy(v).cuda() for v in ((rec if rec_dev is None else rec_dev).view(np.uint8), a, b)]
    B = len(ims_hwc)
    n = B * 3 * size * size
    y = torch.full((n + GUARD,), SENTINEL, dtype=P.TORCH_DT[dtype], device="cuda")
    _lib.call("mv_preprocess_u8_boxes_fwd", x.data_ptr(), x.numel(), y.data_ptr(), rec.ctypes.data, dev[0].data_ptr(),
              dev[1].data_ptr(), dev[2].data_ptr(), B, size, size, 0, P.DT[dtype], 0, _stream())
    torch.cuda.synchronize()
    host = y.float().cpu().numpy().astype(np.float64)
    assert np.all(host[n:] == SENTINEL), "guard overwritten"
    return host[:n].reshape(B, 3, size, size), rec


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("size", A.OUT)
@pytest.mark.parametrize("name", list(A.BOX_SETS))
def test_per_element_bound_of_the_float64_torch_reference(name, size, dtype):
    """Every element of every image within the derived bound of `_reference`, plus half a bf16 ulp for the bf16 store.  No element
    is left out, every element was written, the guard is intact."""
    y, bound = _reference(name, size)
    got, _ = _entry(list(_images()), A.BOX_SETS[name], A.FLIPS, size, dtype)
    assert not np.any(got == SENTINEL) and np.isfinite(got).all(), "elements left unwritten"
    if dtype == "bf16":
        bound = bound + R.bf16_half_ulp(np.abs(y) + bound)
    err = np.abs(got - y)
    for i, box in enumerate(A.BOX_SETS[name]):
        print(f"{name} {box} -> {size} {dtype}: worst |got - ref| / bound = {float((err[i] / bound[i]).max()):.3f} "
              f"(max err {err[i].max():.3e})")
    assert np.all(err <= bound), np.argwhere(err > bound)[:8].tolist()
    assert _lib.check_device_status() == 0


def test_constant_images():
    """A flat image gives fma(v, a[c], b[c]) exactly for every box and both flips, however the generated weights round.  v a + b
    is exact in float64 (8 + 24 bits of product, at most 33 after the sum), so `astype(float32)` is the fma's one rounding."""
    a, b = P.affine(P.IMAGENET_MEAN, P.IMAGENET_STD)
    for v in (0, 255, 128):
        ims = [np.full(hw + (3,), v, np.uint8) for hw in A.SIZES]
        want = (v * a.astype(np.float64) + b.astype(np.float64)).astype(np.float32)
        for name, size, idx, boxes in _cases():
            for flips in (None, [True] * len(ims), A.FLIPS):
                got = P.crop_resize_normalize(ims, boxes, size, flips).cpu().numpy()
                full = np.ascontiguousarray(np.broadcast_to(want.reshape(1, 3, 1, 1), got.shape))
                assert np.array_equal(got.view(np.int32), full.view(np.int32)), (v, name, size, np.argwhere(got != full)[:8].tolist())
    assert _lib.check_device_status() == 0


def test_imagenet_train_preset():
    """Shapes and dtypes, == the core on the boxes and flips the two host functions return for the split key, same key same bits."""
    ims = list(_images()[:5])
    key = jr.PRNGKey(5)
    k_box, k_flip = jr.split(key, 2)
    boxes, flips = P.random_resized_crop_boxes(k_box, A.SIZES[:5]), P.random_flips(k_flip, 5)
    assert flips.any() and not flips.all()
    for dtype, tdt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        out = P.imagenet_train(ims, key, size=32, dtype=dtype)
        assert out.is_cuda and out.dtype == tdt and tuple(out.shape) == (5, 3, 32, 32)
        assert np.array_equal(_bits(out), _bits(P.crop_resize_normalize(ims, boxes, 32, flips, dtype=dtype)))
        assert np.array_equal(_bits(out), _bits(P.imagenet_train(ims, key, size=32, dtype=dtype)))
        assert not np.array_equal(_bits(out), _bits(P.imagenet_train(ims, jr.PRNGKey(6), size=32, dtype=dtype)))
    arr = R.images((300, 260), 2)                                                   # the default 224: 7 x 7 tiles of 32 x 32
    out = P.imagenet_train(arr, key)
    assert tuple(out.shape) == (2, 3, 224, 224) and out.dtype == torch.float32
    ab, af = P.random_resized_crop_boxes(k_box, [(300, 260)] * 2), P.random_flips(k_flip, 2)
    assert np.array_equal(_bits(out), _bits(P.crop_resize_normalize(arr, ab, 224, af)))
    assert _lib.check_device_status() == 0


def test_entry_refuses_bad_host_records_without_launching():
    """A box that leaves its image: MV_E_INVALID; 25 taps: MV_E_UNSUPPORTED; x overlapping y: refused.  Nothing is launched -- the
    output keeps its sentinel -- and the device status stays clean."""
    lib = _lib.load()
    ims = [_images()[0], _images()[5]]
    boxes = [(0, 0, 50, 37), (16, 6, 368, 368)]
    rec, _ = P.boxes_plan([im.shape[:2] for im in ims], boxes, None, 32)
    a, b = P.affine(P.IMAGENET_MEAN, P.IMAGENET_STD)
    x = torch.from_numpy(np.concatenate([im.reshape(-1) for im in ims])).cuda()
    dev = [torch.from_numpy(v).cuda() for v in (a, b)]
    y = torch.full((2 * 3 * 32 * 32 + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")

    def call(r, y_ptr=y.data_ptr()):
        r = np.ascontiguousarray(r)
        rd = torch.from_numpy(r.view(np.uint8)).cuda()
        return lib.mv_preprocess_u8_boxes_fwd(x.data_ptr(), x.numel(), y_ptr, r.ctypes.data, rd.data_ptr(), dev[0].data_ptr(),
                                              dev[1].data_ptr(), 2, 32, 32, 0, _lib.F32, 0, _stream())

    def changed(i, **kw):
        r = rec.copy()
        for k, v in kw.items():
            r[k][i] = v
        return r

    for r, kw, rc, word in ((changed(0, h=51), {}, INVALID, b"image 0: box 51x37"),
                            (changed(1, left=13), {}, INVALID, b"image 1: box 368x368 at (16, 13)"),
                            (changed(1, top=0, h=384), {}, UNSUPPORTED, b"image 1: box 384x368 -> 32x32 needs up to 25 x 24 taps"),
                            (rec, {"y_ptr": x.data_ptr() + 64}, UNSUPPORTED, b"overlap")):
        assert call(r, **kw) == rc
        assert word in lib.mv_last_error(), lib.mv_last_error()
    with pytest.raises(_lib.MVError, match="image 0"):
        r = changed(0, top=1)
        _lib.call("mv_preprocess_u8_boxes_fwd", x.data_ptr(), x.numel(), y.data_ptr(), r.ctypes.data, x.data_ptr(), dev[0].data_ptr(),
                  dev[1].data_ptr(), 2, 32, 32, 0, _lib.F32, 0, _stream())
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all())
    assert _lib.check_device_status() == 0


def test_device_record_that_differs_from_the_host_copy_is_clamped_not_followed():
    """Two images packed; the host records are the whole images.  The DEVICE copy of record 0 has h 13 rows larger than its image:
    followed literally the box would read into image 1 (allocated, inside x).  The kernel clamps the box into its image -- the
    output of image 0 is that of the whole image, the clean run -- and raises bit 2 of the status word; image 1 is unaffected."""
    ims = [_images()[0], _images()[1]]
    boxes = [(0, 0, 50, 37), (0, 0, 37, 50)]
    for size in A.OUT:
        clean, rec = _entry(ims, boxes, [False, True], size)
        assert _read_status() == 0 and not np.any(clean == SENTINEL)
        rec_dev = rec.copy()
        rec_dev["h"][0] = 50 + 13
        got, _ = _entry(ims, boxes, [False, True], size, rec_dev=rec_dev)
        assert _read_status() & 4
        assert np.array_equal(got[0], clean[0]) and np.array_equal(got[1], clean[1])
        assert _read_status() == 0
        rec_dev = rec.copy()
        rec_dev["top"][1], rec_dev["left"][1], rec_dev["w"][1] = -3, -2, 52          # clamped to (0, 0) and to the 50 columns there are
        got, _ = _entry(ims, boxes, [False, True], size, rec_dev=rec_dev)
        assert _read_status() & 4
        assert np.array_equal(got, clean)
        assert _read_status() == 0
