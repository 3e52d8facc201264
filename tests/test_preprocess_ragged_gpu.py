"""GPU: `mv_preprocess_u8_ragged_fwd` and the list path of `eqxvision_amd.preprocess` -- one launch for a batch of differently
sized images -- bit for bit against the single-size entry, against the float64 restatement of tests/_preprocess_ref.py within its
derived per-element bound, and the entry's refusals and clamps.

The batch (shorter side to 36, centre crop 32):
    50x37, 37x50    the two orientations
    36x36           identity resize
    20x31           up-sampling, two taps, clamped at the edges
    53x47           odd sizes: the images behind it start on odd byte offsets (the last one at byte 24321)
    400x380         down-sampling by 10.8 / 10.6: 22 taps per axis by the entry's check, int(2 * 380 / 36 + 1), limit 24
By the entry's tile rule each of the first five alone, and the five together, take the 32 x 32 tile (45 x 45 staged pixels at most,
25.2 KiB of LDS for HWC input), the steep image alone takes 4 x 8 (56 x 97 staged pixels, 23.8 KiB; 8 x 16 would need 74.9 KiB),
and so does any batch that holds it: the same five images are computed in 32 x 32 tiles in one run and in 4 x 8 tiles in the other."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from eqxvision_amd import _lib
from eqxvision_amd import preprocess as P
from tests import _preprocess_ref as R
from tests._slices import GUARD, SENTINEL, _stream

pytestmark = pytest.mark.gpu

SIZES = [(50, 37), (37, 50), (36, 36), (20, 31), (53, 47), (400, 380)]
RESIZE, CROP = 36, 32


def _geometry(sizes, resize=RESIZE, crop=CROP):
    resized = [P.resized_size(h, w, resize) for h, w in sizes]
    return resized, [P.center_crop_box(hr, wr, crop) for hr, wr in resized]


@functools.lru_cache(maxsize=None)
def _images(sizes=tuple(SIZES)):
    out = tuple(R.images(hw, 1)[0] for hw in sizes)            # HWC; every image holds 0 and 255
    for im in out:
        im.setflags(write=False)
    return out


def _as(im, chw):
    return np.ascontiguousarray(im.transpose(2, 0, 1)) if chw else im


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu().numpy()


def _read_status():
    """(status word, cleared) -- synchronises."""
    v = ctypes.c_uint(0)
    assert _lib.load().mv_device_status(1, ctypes.byref(v)) == 0
    return v.value


@pytest.mark.parametrize("nhwc", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("chw", [False, True], ids=["hwc_in", "chw_in"])
def test_list_call_equals_the_single_image_calls_bit_for_bit(chw, dtype, nhwc):
    """One list call == the stack of single-image calls through `mv_preprocess_u8_fwd`, with and without the steep image in the
    batch; the five shared images have the same bits in both runs (32 x 32 tiles in one, 4 x 8 in the other; other neighbours)."""
    ims = [_as(im, chw) for im in _images()]
    resized, boxes = _geometry(SIZES)
    kw = dict(dtype=dtype, layout="nhwc" if nhwc else "nchw")
    single = np.stack([_bits(P.resize_crop_normalize(im, r, b, **kw)) for im, r, b in zip(ims, resized, boxes)])
    with_steep = _bits(P.resize_crop_normalize(ims, resized, boxes, **kw))
    assert _lib.last_kernel() == "preprocess_u8_ragged"
    without = _bits(P.resize_crop_normalize(ims[:5], resized[:5], boxes[:5], **kw))
    assert with_steep.shape == single.shape == ((6, CROP, CROP, 3) if nhwc else (6, 3, CROP, CROP))
    assert np.array_equal(with_steep, single), np.argwhere(with_steep != single)[:8].tolist()
    assert np.array_equal(without, single[:5]), np.argwhere(without != single[:5])[:8].tolist()
    assert np.array_equal(without, with_steep[:5])
    assert _lib.check_device_status() == 0


def _entry(ims_hwc, resized, boxes, dtype="fp32", rec_dev=None, tables=None, runs=2):
    """The C entry on sentinel-filled outputs with a guard behind them, `runs` times; returns (float64 [B, 3, Hout, Wout] of the
    first run with unwritten elements still SENTINEL, the plan).  rec_dev / tables: what to upload instead of the plan's own."""
    sizes = [im.shape[:2] for im in ims_hwc]
    rec, tab, (hout, wout) = P.ragged_plan(sizes, resized, boxes)
    a, b = P.affine(P.IMAGENET_MEAN, P.IMAGENET_STD)
    x = torch.from_numpy(np.concatenate([im.reshape(-1) for im in ims_hwc])).cuda()
    tab_host = tab if tables is None else tables
    dev = [torch.from_numpy(v).cuda() for v in (tab_host, (rec if rec_dev is None else rec_dev).view(np.uint8), a, b)]
    B = len(ims_hwc)
    n = B * 3 * hout * wout
    outs = []
    for _ in range(runs):
        y = torch.full((n + GUARD,), SENTINEL, dtype=P.TORCH_DT[dtype], device="cuda")
        _lib.call("mv_preprocess_u8_ragged_fwd", x.data_ptr(), x.numel(), y.data_ptr(), rec.ctypes.data, dev[1].data_ptr(),
                  dev[0].data_ptr(), tab_host.size, dev[2].data_ptr(), dev[3].data_ptr(), B, hout, wout, 0, P.DT[dtype], 0, _stream())
        outs.append(y)
    torch.cuda.synchronize()
    for o in outs[1:]:
        assert np.array_equal(_bits(outs[0]), _bits(o)), "two runs differ"
    host = outs[0].float().cpu().numpy().astype(np.float64)
    assert np.all(host[n:] == SENTINEL), "guard overwritten"
    return host[:n].reshape(B, 3, hout, wout), (rec, tab)


@functools.lru_cache(maxsize=None)
def _reference():
    """(y, bound) float64 [6, 3, 32, 32] of the batch, once: per image the float64 reference on the dense form of the table words
    the plan uploads (read back out of the packed buffer through the record's offsets) and the fp32 affine vectors."""
    resized, boxes = _geometry(SIZES)
    rec, tab, _ = P.ragged_plan(SIZES, resized, boxes)
    a, b = P.affine(P.IMAGENET_MEAN, P.IMAGENET_STD)

    def dense(at, n, m, n_in):
        w = tab[at + 2 * n:at + n * (2 + m)].view(np.float32).reshape(n, m)
        return R.dense(tab[at:at + n], tab[at + n:at + 2 * n], w, n_in)

    ys, bounds = [], []
    for im, g, r, box in zip(_images(), rec, resized, boxes):
        y, bound = R.reference(im[None], r, box, a, b, wh=dense(int(g["tab_h"]), CROP, int(g["mh"]), im.shape[0]),
                               ww=dense(int(g["tab_w"]), CROP, int(g["mw"]), im.shape[1]))
        ys.append(y[0])
        bounds.append(bound[0])
    y, bound = np.stack(ys), np.stack(bounds)
    y.setflags(write=False)
    bound.setflags(write=False)
    return y, bound


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_per_element_bound_of_the_reference(dtype):
    """Independent of the single-size kernel: every element of the batch within the bound `_preprocess_ref.reference` derives from
    the kernel's arithmetic ((n_h + n_w + 3) 2^-24 (S |a| + |b|)), plus half a bf16 ulp for the bf16 store.  No element is left
    out, every element was written, the guard is intact, two runs give the same bits."""
    y, bound = _reference()
    resized, boxes = _geometry(SIZES)
    got, _ = _entry(list(_images()), resized, boxes, dtype)
    assert not np.any(got == SENTINEL) and np.isfinite(got).all(), "elements left unwritten"
    if dtype == "bf16":
        bound = bound + R.bf16_half_ulp(np.abs(y) + bound)
    err = np.abs(got - y)
    for i, hw in enumerate(SIZES):
        print(f"{hw} {dtype}: worst |got - ref| / bound = {float((err[i] / bound[i]).max()):.3f} (max err {err[i].max():.3e})")
    assert np.all(err <= bound), np.argwhere(err > bound)[:8].tolist()
    assert _lib.check_device_status() == 0


def test_constant_images():
    """A flat image gives fma(v, a[c], b[c]) exactly, at every output of every image, whatever its resize ratio.  v a + b is exact
    in float64 (8 + 24 bits of product, at most 33 bits after the sum, as in test_preprocess_gpu's identity test), so
    `astype(float32)` is the fma's one rounding."""
    values = [0, 255, 128, 1, 77, 254]
    ims = [np.full((h, w, 3), v, np.uint8) for (h, w), v in zip(SIZES, values)]
    a, b = P.affine(P.IMAGENET_MEAN, P.IMAGENET_STD)
    got = P.imagenet_eval(ims, resize=RESIZE, crop=CROP).cpu().numpy()
    want = (np.asarray(values, np.float64)[:, None] * a.astype(np.float64)[None] + b.astype(np.float64)[None]).astype(np.float32)
    want = np.ascontiguousarray(np.broadcast_to(want[:, :, None, None], got.shape))
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), np.argwhere(got != want)[:8].tolist()
    assert _lib.check_device_status() == 0


def test_imagenet_preset_on_two_photograph_sizes():
    """The real preset, once: imagenet_eval([500x375, 375x500]) at 256 / 224 == the two single-image calls (7 x 7 tiles each)."""
    ims = [R.images(hw, 1)[0] for hw in ((500, 375), (375, 500))]
    out = P.imagenet_eval(ims)
    assert out.is_cuda and out.dtype == torch.float32 and tuple(out.shape) == (2, 3, 224, 224)
    for i, im in enumerate(ims):
        assert np.array_equal(_bits(out[i]), _bits(P.imagenet_eval(im))), i
    dev = P.imagenet_eval([torch.from_numpy(im).cuda() for im in ims], dtype="bf16")        # device-resident images, one device cat
    mixed = P.imagenet_eval([ims[0], torch.from_numpy(ims[1]).cuda()], dtype="bf16")
    for i, im in enumerate(ims):
        single = _bits(P.imagenet_eval(im, dtype="bf16"))
        assert np.array_equal(_bits(dev[i]), single) and np.array_equal(_bits(mixed[i]), single), i
    assert _lib.check_device_status() == 0


def test_list_of_one_image_equals_the_array_path():
    im = _images()[4]
    for chw in (False, True):
        one = P.imagenet_eval([_as(im, chw)], resize=RESIZE, crop=CROP)
        assert _lib.last_kernel() == "preprocess_u8_ragged" and tuple(one.shape) == (1, 3, CROP, CROP)
        arr = P.imagenet_eval(_as(im, chw)[None], resize=RESIZE, crop=CROP)
        assert _lib.last_kernel() == "preprocess_u8"
        assert np.array_equal(_bits(one), _bits(arr))
    assert _lib.check_device_status() == 0


def test_entry_refuses_records_that_leave_their_buffers():
    """Host records whose image or tables lie outside the buffers: non-zero return, a message that names the image, nothing
    launched -- the output keeps its sentinel -- and the device status stays clean."""
    lib = _lib.load()
    ims = list(_images()[:3])
    resized, boxes = _geometry(SIZES[:3])
    rec, tab, (hout, wout) = P.ragged_plan(SIZES[:3], resized, boxes)
    a, b = P.affine(P.IMAGENET_MEAN, P.IMAGENET_STD)
    x = torch.from_numpy(np.concatenate([im.reshape(-1) for im in ims])).cuda()
    dev = [torch.from_numpy(v).cuda() for v in (tab, rec.view(np.uint8), a, b)]
    y = torch.full((3 * 3 * hout * wout + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")

    def call(r, x_bytes=x.numel(), tab_words=tab.size):
        r = np.ascontiguousarray(r)
        rd = torch.from_numpy(r.view(np.uint8)).cuda()
        return lib.mv_preprocess_u8_ragged_fwd(x.data_ptr(), x_bytes, y.data_ptr(), r.ctypes.data, rd.data_ptr(), dev[0].data_ptr(),
                                               tab_words, dev[2].data_ptr(), dev[3].data_ptr(), 3, hout, wout, 0, _lib.F32, 0, _stream())

    def changed(i, **kw):
        r = rec.copy()
        for k, v in kw.items():
            r[k][i] = v
        return r

    for r, kw, word in ((changed(2, offset=int(rec["offset"][2]) + 1), {}, b"image 2"),
                        (changed(1, offset=-1), {}, b"image 1"),
                        (changed(0, offset=x.numel()), {}, b"image 0"),
                        (rec, {"x_bytes": x.numel() - 1}, b"image 2"),
                        (changed(2, tab_w=int(rec["tab_w"][2]) + 1), {}, b"image 2"),
                        (changed(1, tab_h=tab.size), {}, b"image 1"),
                        (changed(0, tab_h=-1), {}, b"image 0"),
                        (rec, {"tab_words": tab.size - 1}, b"image 2")):
        assert call(r, **kw) != 0
        assert word in lib.mv_last_error() and b"lie inside" in lib.mv_last_error(), lib.mv_last_error()
    with pytest.raises(_lib.MVError, match="image 2"):
        _lib.call("mv_preprocess_u8_ragged_fwd", x.data_ptr(), x.numel() - 1, y.data_ptr(), rec.ctypes.data, dev[1].data_ptr(),
                  dev[0].data_ptr(), tab.size, dev[2].data_ptr(), dev[3].data_ptr(), 3, hout, wout, 0, _lib.F32, 0, _stream())
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all())
    assert _lib.check_device_status() == 0


def test_device_copy_that_differs_from_the_host_copy_is_clamped_not_followed():
    """The kernel reads the DEVICE records and tables, which the host cannot see at launch time; it forms no address from them
    without the cuts the single-size kernel makes, and raises bit 2 of the status word.  Two cases, each valid on the host copy:
    (a) the device record of image 0 points at a row table (inside the table buffer) whose `first` lies 5 rows beyond the image:
        the rows are clamped to the last row of the image (the staged rectangle is cut to [Hin - 1, Hin), tap indices to it);
    (b) the device record of image 1 puts the image at the very end of the buffer, so that it would leave it: that record forms
        no address at all, its image is not written.
    In both the other images have the bits of the clean run."""
    ims = list(_images()[:3])
    resized, boxes = _geometry(SIZES[:3])
    clean, (rec, tab) = _entry(ims, resized, boxes, runs=1)
    assert _read_status() == 0 and not np.any(clean == SENTINEL)

    g = rec[0]
    n, m = CROP, int(g["mh"])
    rows = tab[int(g["tab_h"]):int(g["tab_h"]) + n * (2 + m)].copy()
    rows[:n] = int(g["Hin"]) + 5                                               # first[] beyond the image; counts and weights kept
    rec_dev = rec.copy()
    rec_dev["tab_h"][0] = tab.size
    got, _ = _entry(ims, resized, boxes, rec_dev=rec_dev, tables=np.concatenate([tab, rows]), runs=1)
    assert _read_status() & 4
    assert np.array_equal(got[1:], clean[1:]) and not np.any(got[0] == SENTINEL) and np.isfinite(got).all()
    assert np.all(got[0] == got[0][:, :1])                                    # every output row: the filtered LAST input row

    rec_dev = rec.copy()
    rec_dev["offset"][1] = sum(im.size for im in ims) - 1
    got, _ = _entry(ims, resized, boxes, rec_dev=rec_dev, runs=1)
    assert _read_status() & 4
    assert np.all(got[1] == SENTINEL) and np.array_equal(got[0], clean[0]) and np.array_equal(got[2], clean[2])
    assert _read_status() == 0
