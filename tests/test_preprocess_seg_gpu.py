"""GPU: `mv_preprocess_u8_seg_fwd` and `eqxvision_amd.preprocess.resize_pad_crop_pair` / `segmentation_train` /
`segmentation_eval` -- resize the whole image, mirror it, pad it, keep a window; the image and its label map in one launch.

Images, masks and geometry sets are those of tests/_seg_augment_ref.py (the host file checks their preconditions).  The crop is
32 x 40: one full 32 x 32 tile and a partial one when the batch takes the large tile; every set holds the 400 x 380 image resized
by more than 10x, so the launches of whole sets run on the small tiles and those of single small images on the 32 x 32 one."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import eqxvision_amd as eqv
from eqxvision_amd import _lib
from eqxvision_amd import preprocess as P
from eqxvision_amd import random as jr
from tests import _augment_ref as A
from tests import _preprocess_ref as R
from tests import _seg_augment_ref as S
from tests._slices import GUARD, SENTINEL, _stream

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -2
HC, WC = S.CROP


def _as(im, chw):
    return np.ascontiguousarray(im.transpose(2, 0, 1)) if chw else im


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu().numpy()


def _nchw(bits, nhwc):
    return bits.transpose(0, 3, 1, 2) if nhwc else bits


def _geo(name):
    g = np.asarray(S.GEOMETRY[name])
    return g[:, :2], g[:, 2:]


def _read_status():
    """status word, cleared -- synchronises."""
    v = ctypes.c_uint(0)
    assert _lib.load().mv_device_status(1, ctypes.byref(v)) == 0
    return v.value


def _pair(name, masks=True, chw=False, **kw):
    rs, og = _geo(name)
    return P.resize_pad_crop_pair([_as(im, chw) for im in S.images(name)], list(S.masks(name)) if masks else None, rs, og, S.CROP,
                                  S.flips(name), **kw)


def _fill_values(fill, dtype):
    """fma(fill, a[c], b[c]): fill a + b is exact in float64 (8 + 24 bits of product), so `astype(float32)` is the fma's one
    rounding; bf16 is the store's rounding of that."""
    a, b = P.affine(P.IMAGENET_MEAN, P.IMAGENET_STD)
    v = torch.from_numpy((fill * a.astype(np.float64) + b.astype(np.float64)).astype(np.float32))
    return _bits(v.to(P.TORCH_DT[dtype]).cuda())


# ---- 1, 2: the image against the boxes entry on the whole image, and the fill ----------------------------------------------------

@pytest.mark.parametrize("nhwc", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("chw", [False, True], ids=["hwc_in", "chw_in"])
def test_valid_region_has_the_bits_of_the_boxes_entry_and_the_rest_is_the_fill(chw, dtype, nhwc):
    """y[n, :, :hv, :wv] == crop_resize_normalize(image n, its full box, (Hr, Wr), flip n)[:, top:top + hv, left:left + wv]: the
    yardstick is the existing entry.  Every other element is fma(fill, a[c], b[c]) exactly, for image_fill 0 and 114."""
    kw = dict(dtype=dtype, layout="nhwc" if nhwc else "nchw")
    for name, geos in S.GEOMETRY.items():
        for fill in (0, 114):
            y, lab = _pair(name, chw=chw, image_fill=fill, **kw)
            assert _lib.last_kernel() == "preprocess_u8_seg"
            assert tuple(y.shape) == ((len(geos), HC, WC, 3) if nhwc else (len(geos), 3, HC, WC)) and y.dtype == P.TORCH_DT[dtype]
            got = _nchw(_bits(y), nhwc)
            want_fill = _fill_values(fill, dtype)
            for n, (im, geo, flip) in enumerate(zip(S.images(name), geos, S.flips(name))):
                Hr, Wr, top, left = geo
                hv, wv = S.valid_extent(geo)
                whole = P.crop_resize_normalize(_as(im, chw), (0, 0) + im.shape[:2], (Hr, Wr), flip, **kw)
                whole = _nchw(_bits(whole[None]), nhwc)[0]
                assert np.array_equal(got[n, :, :hv, :wv], whole[:, top:top + hv, left:left + wv]), (name, n, fill)
                outside = np.ones((HC, WC), bool)
                outside[:hv, :wv] = False
                for c in range(3):
                    assert np.all(got[n, c][outside] == want_fill[c]), (name, n, c, fill)
    assert _lib.check_device_status() == 0


# ---- 3: the image against float64 torch on the CPU --------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _reference(name):
    """(y, bound, valid) [B, 3, Hc, Wc] of one set, once: torch on the CPU in float64 resizes the WHOLE image to (Hr, Wr), then the
    mirror, then the window, then the fp32 a and b of the kernel.  bound = (n_h + n_w + 5) 2^-24 (S |a| + |b|), the derived bound
    of tests/test_preprocess_train_gpu.py: n_h, n_w the non-zero taps of the resized row / unmirrored column."""
    a, b = P.affine(P.IMAGENET_MEAN, P.IMAGENET_STD)
    a64, b64 = a.astype(np.float64).reshape(3, 1, 1), b.astype(np.float64).reshape(3, 1, 1)
    ys, bounds, valids = [], [], []
    for im, geo, flip in zip(S.images(name), S.GEOMETRY[name], S.flips(name)):
        Hr, Wr, top, left = geo
        hv, wv = S.valid_extent(geo)
        t = torch.from_numpy(np.array(im)).permute(2, 0, 1)[None].double()
        s = F.interpolate(t, size=(Hr, Wr), mode="bilinear", antialias=True, align_corners=False)[0].numpy()
        nh = A.nonzero_taps(im.shape[0], Hr).reshape(1, Hr, 1)
        nw = A.nonzero_taps(im.shape[1], Wr).reshape(1, 1, Wr)
        if flip:
            s, nw = s[:, :, ::-1], nw[:, :, ::-1]
        y, bound, valid = np.zeros((3, HC, WC)), np.zeros((3, HC, WC)), np.zeros((3, HC, WC), bool)
        sw = s[:, top:top + hv, left:left + wv]
        y[:, :hv, :wv] = sw * a64 + b64
        bound[:, :hv, :wv] = (nh[:, top:top + hv] + nw[:, :, left:left + wv] + 5) * 2.0 ** -24 * (np.abs(sw) * np.abs(a64) + np.abs(b64))
        valid[:, :hv, :wv] = True
        ys.append(y), bounds.append(bound), valids.append(valid)
    out = np.stack(ys), np.stack(bounds), np.stack(valids)
    for v in out:
        v.setflags(write=False)
    return out


def _entry(name, dtype="fp32", rec_dev=None, masks=True, mask_fill=S.VOID):
    """The C entry on sentinel-filled outputs with guards behind them; returns (y float64 [B, 3, Hc, Wc], labels int64 [B, Hc, Wc]
    or None, the host records), unwritten elements still SENTINEL.  rec_dev: what to upload instead of the host records."""
    ims, ms = S.images(name), S.masks(name)
    rs, og = _geo(name)
    rec, _ = P.seg_plan([im.shape[:2] for im in ims], rs, og, S.flips(name), S.CROP)
    a, b = P.affine(P.IMAGENET_MEAN, P.IMAGENET_STD)
    x = torch.from_numpy(np.concatenate([im.reshape(-1) for im in ims])).cuda()
    m = torch.from_numpy(np.concatenate([mk.reshape(-1) for mk in ms])).cuda()
    dev = [torch.from_numpy(v).cuda() for v in ((rec if rec_dev is None else rec_dev).view(np.uint8), a, b)]
    B = len(ims)
    n = B * 3 * HC * WC
    y = torch.full((n + GUARD,), SENTINEL, dtype=P.TORCH_DT[dtype], device="cuda")
    lab = torch.full((B * HC * WC + GUARD,), int(SENTINEL), dtype=torch.int32, device="cuda")
    _lib.call("mv_preprocess_u8_seg_fwd", x.data_ptr(), x.numel(), m.data_ptr() if masks else None, m.numel() if masks else 0, y.data_ptr(),
              lab.data_ptr() if masks else None, rec.ctypes.data, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), B, HC, WC, 0,
              mask_fill, 0, P.DT[dtype], 0, _stream())
    torch.cuda.synchronize()
    host, lh = y.float().cpu().numpy().astype(np.float64), lab.cpu().numpy().astype(np.int64)
    assert np.all(host[n:] == SENTINEL) and np.all(lh[B * HC * WC:] == int(SENTINEL)), "guard overwritten"
    if not masks:
        assert np.all(lh == int(SENTINEL))
    return host[:n].reshape(B, 3, HC, WC), lh[:B * HC * WC].reshape(B, HC, WC) if masks else None, rec


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(S.GEOMETRY))
def test_per_element_bound_of_the_float64_torch_reference(name, dtype):
    """Every valid element within the derived bound of `_reference`, plus half a bf16 ulp for the bf16 store; every element was
    written, the guards are intact."""
    y, bound, valid = _reference(name)
    got, lab, _ = _entry(name, dtype)
    assert not np.any(got == SENTINEL) and np.isfinite(got).all() and not np.any(lab == int(SENTINEL)), "elements left unwritten"
    if dtype == "bf16":
        bound = bound + R.bf16_half_ulp(np.abs(y) + bound)
    err = np.abs(got - y)
    for n, geo in enumerate(S.GEOMETRY[name]):
        if valid[n].any():
            print(f"{name} image {n} -> {geo} {dtype}: worst |got - ref| / bound = {float((err[n][valid[n]] / bound[n][valid[n]]).max()):.3f} "
                  f"(max err {err[n][valid[n]].max():.3e})")
    assert np.all(err[valid] <= bound[valid]), np.argwhere(valid & (err > bound))[:8].tolist()
    assert _lib.check_device_status() == 0


# ---- 4, 5: labels ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mask_fill", [255, 0])
def test_labels_equal_the_scalar_restatement_at_every_pixel(mask_fill):
    for name, geos in S.GEOMETRY.items():
        _, lab = _pair(name, mask_fill=mask_fill, dtype="bf16")
        assert lab.dtype == torch.int32 and lab.is_cuda and tuple(lab.shape) == (len(geos), HC, WC)
        got = lab.cpu().numpy()
        for n, (mask, geo, flip) in enumerate(zip(S.masks(name), geos, S.flips(name))):
            want = S.labels_ref(mask, geo, flip, fill=mask_fill)
            assert np.array_equal(got[n], want), (name, n, np.argwhere(got[n] != want)[:8].tolist())
    assert _lib.check_device_status() == 0


def test_labels_and_image_describe_the_same_picture():
    """Images whose three channels are 12 x their mask (labels 0 .. 20, no void), not resized (Hr = Hin, Wr = Win: one tap of weight
    1), mean 0 and std 1 / 255 (a = 1, b = 0): y is the pixel value itself, so y == 12 labels at every pixel, under the flips, at
    origins off zero and in the padding (image_fill 252 = 12 x 21, mask_fill 21)."""
    ms = [np.where(m == S.VOID, 20, m).astype(np.uint8) for m in S.masks("inside")]
    ims = [np.repeat((12 * m)[:, :, None], 3, axis=2) for m in ms]
    rs = np.asarray(A.SIZES)
    og = np.asarray([(18, 0), (5, 10), (4, 0), (0, 0), (21, 7), (300, 200)])
    a, b = P.affine((0.0, 0.0, 0.0), (1 / 255,) * 3)
    assert np.all(a == 1.0) and np.all(b == 0.0)
    for flips in (A.FLIPS, [not f for f in A.FLIPS]):
        y, lab = P.resize_pad_crop_pair(ims, ms, rs, og, S.CROP, flips, mean=(0.0, 0.0, 0.0), std=(1 / 255,) * 3, image_fill=252, mask_fill=21)
        y, lab = y.cpu().numpy(), lab.cpu().numpy()
        assert np.array_equal(y, np.broadcast_to(12.0 * lab[:, None].astype(np.float32), y.shape))
        assert (lab == 21).any() and len(np.unique(lab)) == 22
        for n, (m, flip) in enumerate(zip(ms, flips)):
            assert np.array_equal(lab[n], S.labels_ref(m, tuple(rs[n]) + tuple(og[n]), flip, fill=21)), n
    assert _lib.check_device_status() == 0


# ---- 6: independence of the launch ---------------------------------------------------------------------------------------------

def test_an_image_gives_the_bits_it_gives_alone_and_an_array_those_of_the_list():
    for name, geos in S.GEOMETRY.items():
        rs, og = _geo(name)
        y, lab = _pair(name, dtype="bf16")
        y_only, none = _pair(name, masks=False, dtype="bf16")
        assert none is None and np.array_equal(_bits(y), _bits(y_only)), name
        for n, (im, mk, flip) in enumerate(zip(S.images(name), S.masks(name), S.flips(name))):
            ya, la = P.resize_pad_crop_pair([im], [mk], rs[n:n + 1], og[n:n + 1], S.CROP, [flip], dtype="bf16")
            assert np.array_equal(_bits(ya)[0], _bits(y)[n]) and np.array_equal(la.cpu().numpy()[0], lab.cpu().numpy()[n]), (name, n)
        again, lab2 = _pair(name, dtype="bf16")
        assert np.array_equal(_bits(y), _bits(again)) and torch.equal(lab, lab2)
    arr = R.images(A.ARRAY_SHAPE, 2)
    marr = np.stack([S.masks("pad")[0], S.masks("pad")[0][::-1].copy()])
    rs, og = np.asarray([(40, 44), (24, 18)]), np.asarray([(8, 4), (0, 0)])
    for chw in (False, True):
        batch = np.ascontiguousarray(arr.transpose(0, 3, 1, 2)) if chw else arr
        as_array = P.resize_pad_crop_pair(batch, marr, rs, og, S.CROP, [False, True])
        as_list = P.resize_pad_crop_pair([batch[0], batch[1]], [marr[0], marr[1]], rs, og, S.CROP, [False, True])
        on_device = P.resize_pad_crop_pair(torch.from_numpy(batch).cuda(), torch.from_numpy(marr).cuda(), rs, og, S.CROP, [False, True])
        single = P.resize_pad_crop_pair(batch[1], marr[1], rs[1], og[1], S.CROP, True)
        for other in (as_list, on_device):
            assert np.array_equal(_bits(as_array[0]), _bits(other[0])) and torch.equal(as_array[1], other[1])
        assert tuple(single[0].shape) == (3, HC, WC) and tuple(single[1].shape) == (HC, WC)
        assert np.array_equal(_bits(single[0]), _bits(as_array[0][1])) and torch.equal(single[1], as_array[1][1])
    assert _lib.check_device_status() == 0


# ---- 7: refusals ------------------------------------------------------------------------------------------------------------------

def test_entry_refuses_bad_host_records_without_launching():
    lib = _lib.load()
    ims, ms = S.images("pad")[:2], S.masks("pad")[:2]
    rec, _ = P.seg_plan(A.SIZES[:2], [(60, 44), (16, 22)], [(28, 4), (0, 0)], None, S.CROP)
    a, b = P.affine(P.IMAGENET_MEAN, P.IMAGENET_STD)
    x = torch.from_numpy(np.concatenate([im.reshape(-1) for im in ims])).cuda()
    m = torch.from_numpy(np.concatenate([mk.reshape(-1) for mk in ms])).cuda()
    dev = [torch.from_numpy(v).cuda() for v in (a, b)]
    y = torch.full((2 * 3 * HC * WC + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    lab = torch.full((2 * HC * WC + GUARD,), int(SENTINEL), dtype=torch.int32, device="cuda")

    def call(r, y_ptr=y.data_ptr(), m_ptr=m.data_ptr(), lab_ptr=lab.data_ptr(), fills=(0, 255)):
        r = np.ascontiguousarray(r)
        rd = torch.from_numpy(r.view(np.uint8)).cuda()
        return lib.mv_preprocess_u8_seg_fwd(x.data_ptr(), x.numel(), m_ptr, m.numel(), y_ptr, lab_ptr, r.ctypes.data, rd.data_ptr(),
                                            dev[0].data_ptr(), dev[1].data_ptr(), 2, HC, WC, fills[0], fills[1], 0, _lib.F32, 0, _stream())

    def changed(i, **kw):
        r = rec.copy()
        for k, v in kw.items():
            r[k][i] = v
        return r

    for r, kw, rc, word in ((changed(1, offset=rec["offset"][1] + 1), {}, INVALID, b"image 1: 5550 bytes at offset 5551"),
                            (changed(1, mask_offset=1851), {}, INVALID, b"image 1: mask of 1850 bytes at offset 1851"),
                            (changed(0, Hr=0), {}, INVALID, b"image 0: bad sizes"),
                            (changed(0, top=29), {}, INVALID, b"image 0: window 32x40 at (29, 4)"),
                            (changed(1, left=1), {}, INVALID, b"image 1: window 32x40 at (0, 1) does not lie inside the padded image 32x40"),
                            (rec, {"m_ptr": None}, INVALID, b"labels without masks"),
                            (rec, {"lab_ptr": None}, INVALID, b"masks without labels"),
                            (rec, {"fills": (300, 255)}, INVALID, b"image_fill 300"),
                            (changed(0, Hr=4, top=0), {}, UNSUPPORTED, b"image 0: 50x37 -> 4x44 needs up to 26 x 3 taps"),
                            (rec, {"y_ptr": x.data_ptr() + 64}, UNSUPPORTED, b"images and output overlap"),
                            (rec, {"lab_ptr": y.data_ptr() + 64}, UNSUPPORTED, b"output and labels overlap")):
        assert call(r, **kw) == rc
        assert word in lib.mv_last_error(), lib.mv_last_error()
    with pytest.raises(_lib.MVError, match="image 0"):
        r = changed(0, left=5)
        _lib.call("mv_preprocess_u8_seg_fwd", x.data_ptr(), x.numel(), m.data_ptr(), m.numel(), y.data_ptr(), lab.data_ptr(), r.ctypes.data,
                  x.data_ptr(), dev[0].data_ptr(), dev[1].data_ptr(), 2, HC, WC, 0, 255, 0, _lib.F32, 0, _stream())
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all()) and bool((lab == int(SENTINEL)).all())
    assert _lib.check_device_status() == 0


def test_device_record_that_differs_from_the_host_copy_is_checked_not_followed():
    """The host records are those of the "pad" set.  The DEVICE copy of record 0 has a larger Hr (a finer resize: fewer taps and
    shorter spans than the launch was sized for, so it is simply carried out), that of record 1 an offset past the buffer: image 1
    stores nothing -- its rows keep the sentinel, image and labels -- bit 2 of the status word is raised and every other image has
    the bits of the clean run.  Then an origin outside the padded image and a resized size of 0: clamped, bit 2, everything
    written, the other images untouched."""
    clean, clean_lab, rec = _entry("pad")
    assert _read_status() == 0 and not np.any(clean == SENTINEL)
    rec_dev = rec.copy()
    rec_dev["Hr"][0] = 48
    rec_dev["offset"][1] = rec["offset"][5] + 3 * 400 * 380 - 10            # 10 bytes before the end: the image leaves the buffer
    got, lab, _ = _entry("pad", rec_dev=rec_dev)
    assert _read_status() & 4
    assert np.all(got[1] == SENTINEL) and np.all(lab[1] == int(SENTINEL))
    assert not np.any(got[0] == SENTINEL) and not np.array_equal(got[0], clean[0])
    assert np.array_equal(got[2:], clean[2:]) and np.array_equal(lab[2:], clean_lab[2:])
    assert _read_status() == 0
    rec_dev = rec.copy()
    rec_dev["mask_offset"][2] = -1
    got, lab, _ = _entry("pad", rec_dev=rec_dev)
    assert _read_status() & 4
    assert np.all(got[2] == SENTINEL) and np.all(lab[2] == int(SENTINEL))
    keep = [0, 1, 3, 4, 5]
    assert np.array_equal(got[keep], clean[keep]) and np.array_equal(lab[keep], clean_lab[keep])
    got, _, _ = _entry("pad", rec_dev=rec_dev, masks=False)                  # without masks the mask offset is not looked at
    assert _read_status() == 0 and np.array_equal(got, clean)
    rec_dev = rec.copy()
    rec_dev["top"][0], rec_dev["left"][3], rec_dev["Wr"][4] = 7, -3, 0      # all clamped: (0, 0) origins, Wr = 1
    got, lab, _ = _entry("pad", rec_dev=rec_dev)
    assert _read_status() & 4
    assert not np.any(got == SENTINEL) and not np.any(lab == int(SENTINEL))
    keep = [0, 1, 2, 3, 5]
    assert np.array_equal(got[keep], clean[keep]) and np.array_equal(lab[keep], clean_lab[keep])
    assert np.array_equal(lab[4], S.labels_ref(S.masks("pad")[4], (31, 1, 0, 0), False))      # one resized column, the rest fill
    assert _read_status() == 0


# ---- 8: presets -------------------------------------------------------------------------------------------------------------------

def test_segmentation_train_preset():
    """== the core on the draws the three host functions return for the split key; same key same bits, another key other bits."""
    ims, ms = list(S.images("pad")[:5]), list(S.masks("pad")[:5])
    key = jr.PRNGKey(5)
    k_size, k_flip, k_origin = jr.split(key, 3)
    rs = P.random_resize_sizes(k_size, A.SIZES[:5], 20, 80)
    fl, og = P.random_flips(k_flip, 5), P.random_crop_origins(k_origin, rs, 32)
    assert fl.any() and not fl.all()
    for dtype, tdt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        x, lab = P.segmentation_train(ims, ms, key, base_size=40, crop_size=32, dtype=dtype)
        assert x.is_cuda and x.dtype == tdt and tuple(x.shape) == (5, 3, 32, 32) and lab.dtype == torch.int32 and tuple(lab.shape) == (5, 32, 32)
        cx, cl = P.resize_pad_crop_pair(ims, ms, rs, og, 32, fl, dtype=dtype)
        assert np.array_equal(_bits(x), _bits(cx)) and torch.equal(lab, cl)
        ax, al = P.segmentation_train(ims, ms, key, base_size=40, crop_size=32, dtype=dtype)
        assert np.array_equal(_bits(x), _bits(ax)) and torch.equal(lab, al)
        ox, ol = P.segmentation_train(ims, ms, jr.PRNGKey(6), base_size=40, crop_size=32, dtype=dtype)
        assert not np.array_equal(_bits(x), _bits(ox)) and not torch.equal(lab, ol)
    arr, marr = R.images((300, 260), 2), np.stack([S.masks("pad")[5][:300, :260]] * 2)          # the defaults: 480 x 480, 15 x 15 tiles
    x, lab = P.segmentation_train(arr, marr, key)
    assert tuple(x.shape) == (2, 3, 480, 480) and x.dtype == torch.float32 and tuple(lab.shape) == (2, 480, 480)
    rs = P.random_resize_sizes(k_size, [(300, 260)] * 2, 260, 1040)
    cx, cl = P.resize_pad_crop_pair(arr, marr, rs, P.random_crop_origins(k_origin, rs, 480), 480, P.random_flips(k_flip, 2))
    assert np.array_equal(_bits(x), _bits(cx)) and torch.equal(lab, cl)
    assert _lib.check_device_status() == 0


def test_segmentation_eval_preset():
    """The image == `resize_crop_normalize` with the full box (the table entry: the host file holds its weights on these two axes
    equal to the generated ones), the labels == the restatement; no flip, no fill."""
    im, mk = S.images("pad")[0], S.masks("pad")[0]
    for dtype in ("fp32", "bf16"):
        x, lab = P.segmentation_eval(np.array(im), np.array(mk), base_size=24, dtype=dtype)
        assert tuple(x.shape) == (3, 32, 24) and tuple(lab.shape) == (32, 24)
        want = P.resize_crop_normalize(np.array(im), (32, 24), (0, 0, 32, 24), dtype=dtype)
        assert np.array_equal(_bits(x), _bits(want))
        assert np.array_equal(lab.cpu().numpy(), S.labels_ref(mk, (32, 24, 0, 0), False, crop=(32, 24)))
    x, lab = P.segmentation_eval(np.stack([im, im]), base_size=24)
    assert lab is None and tuple(x.shape) == (2, 3, 32, 24) and np.array_equal(_bits(x[0]), _bits(x[1]))
    assert _lib.check_device_status() == 0


# ---- 9: end to end ----------------------------------------------------------------------------------------------------------------

def test_one_training_step_of_fcn_resnet50_on_the_pipeline_output():
    """2 images of 64 x 48 -> segmentation_train(base_size=40, crop_size=32) -> fcn on ResNet-50, 21 classes, loss on `out` plus
    0.4 x the loss on `aux`, void and padding masked by a DEVICE `where`: finite, and bit for bit the loss of the same x, labels
    and mask given as host arrays (the device-`where` path against the host one); an sgd update runs.  The step itself is
    taken on batch statistics with Dropout live; the comparison of bits is then made on the same network with BatchNorm on the
    statistics that step left and Dropout off, because on batch statistics two runs of the SAME operands already differ in the last
    bits of the loss (measured: 2.5550008 / 2.5550013 / 2.5550003), so there no comparison of bits could tell the two paths apart."""
    from eqxvision_amd.models.classification import resnet as RN
    rng = np.random.default_rng(3)
    ims = rng.integers(0, 256, (2, 64, 48, 3), dtype=np.uint8)
    ms = rng.integers(0, S.CLASSES, (2, 64, 48), dtype=np.uint8)
    ms[rng.random(ms.shape) < 0.1] = S.VOID
    x, labels = P.segmentation_train(ims, ms, jr.PRNGKey(2), base_size=40, crop_size=32)
    where = labels != S.VOID
    assert where.is_cuda and 0 < int(where.sum()) < where.numel()
    bb = RN._resnet(RN._ResNetBottleneck, [3, 4, 6, 3], None, replace_stride_with_dilation=[False, True, True])
    net = eqv.models.fcn(num_classes=S.CLASSES, backbone=bb, intermediate_layers=lambda m: [m.layer3, m.layer4], aux_in_channels=1024,
                         key=jr.PRNGKey(0))
    keys = jr.split(jr.PRNGKey(1), 2)
    xent = eqv.optim.softmax_cross_entropy_with_integer_labels

    @eqv.filter_value_and_grad
    def compute_loss(model, xx, yy, ww):
        aux, out = eqv.vmap(model, axis_name="batch")(xx, key=keys)
        return xent(out, yy, axis=1, where=ww).mean() + 0.4 * xent(aux, yy, axis=1, where=ww).mean()

    loss, grads = compute_loss(net, x, labels, where)
    assert np.isfinite(loss)
    frozen = eqv.tree_inference(net, True)
    dev_loss, _ = compute_loss(frozen, x, labels, where)
    host_loss, _ = compute_loss(frozen, x.cpu().numpy(), labels.cpu().numpy(), where.cpu().numpy())
    print("training-mode loss", loss, "stored statistics: device operands", dev_loss, "host arrays", host_loss)
    assert np.isfinite(dev_loss) and dev_loss == host_loss
    logits = rng.normal(0.0, 3.0, (2, S.CLASSES, 32, 32)).astype(np.float32)                   # the loss kernel alone, per pixel
    on_dev = xent(logits, labels, axis=1, where=where)
    on_host = xent(logits, labels.cpu().numpy(), axis=1, where=where.cpu().numpy())
    assert torch.equal(on_dev.losses, on_host.losses) and on_dev.counted == on_host.counted == int(where.sum())
    opt = eqv.optim.sgd(learning_rate=0.01)
    st = opt.init(eqv.filter(net, eqv.is_array))
    updates, st = opt.update(grads, st)
    new = eqv.apply_updates(net, updates)
    moved = [not np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(eqv.tree_leaves(net), eqv.tree_leaves(new))
             if eqv.is_array(a) and a.dtype.kind == "f"]
    assert any(moved)
    assert _lib.check_device_status() == 0
