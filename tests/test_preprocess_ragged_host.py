"""CPU: the host half of a ragged call (`eqxvision_amd.preprocess` given a LIST of differently sized images) -- per-image
geometry, the packed image buffer, the records and the packed tables exactly as `mv_preprocess_u8_ragged_fwd` would receive them,
the refusals, the bounded cache.  The library call is replaced by one that copies what its pointers point to; "the device" is
host memory, so the whole path runs without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

from eqxvision_amd import _act, _lib
from eqxvision_amd import preprocess as P
from tests import _preprocess_ref as R

SIZES = [(50, 37), (37, 50), (36, 36), (20, 31), (53, 47), (400, 380)]      # the batch of tests/test_preprocess_ragged_gpu.py
RESIZE, CROP = 36, 32


def _images(sizes, chw=False):
    out = [R.images(hw, 1)[0] for hw in sizes]
    return [np.ascontiguousarray(im.transpose(2, 0, 1)) for im in out] if chw else out


def _bytes_at(ptr, n):
    return np.ctypeslib.as_array((ctypes.c_uint8 * n).from_address(ptr)).copy()


@pytest.fixture
def on_host(monkeypatch):
    """Runs the list path with host memory for the device; returns the list of captured calls, each a dict of what the entry was
    handed: x, rec_host, rec_dev, tab as arrays and the scalar arguments."""
    calls = []

    def fake_call(name, *a):
        assert name == "mv_preprocess_u8_ragged_fwd" and len(a) == len(_lib.PROTOTYPES[name])
        x, x_bytes, y, rec_host, rec_dev, tab, tab_words, ca, cb, B, hout, wout, chw, dt, nhwc, stream = a
        calls.append({
            "x": _bytes_at(x, x_bytes), "rec_host": _bytes_at(rec_host, B * P.RECORD.itemsize).view(P.RECORD),
            "rec_dev": _bytes_at(rec_dev, B * P.RECORD.itemsize).view(P.RECORD), "tab": _bytes_at(tab, 4 * tab_words).view(np.int32),
            "a": _bytes_at(ca, 12).view(np.float32), "b": _bytes_at(cb, 12).view(np.float32),
            "B": B, "hout": hout, "wout": wout, "chw": chw, "dtype": dt, "nhwc": nhwc})
        return 0

    monkeypatch.setattr(_lib, "call", fake_call)
    monkeypatch.setattr(P, "device", lambda: torch.device("cpu"))
    monkeypatch.setattr(P, "empty", lambda shape, dtype: torch.empty(tuple(shape), dtype=dtype))
    monkeypatch.setattr(P, "stream_ptr", lambda: 0)
    monkeypatch.setattr(P, "_affines", {})
    return calls


def test_record_is_the_headers_struct():
    assert P.RECORD.itemsize == 48
    assert [P.RECORD.fields[n][1] for n in P.RECORD.names] == [0, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44]


@pytest.mark.parametrize("chw", [False, True])
def test_packed_buffer_records_and_tables_describe_each_image(on_host, chw):
    """imagenet_eval(list) at 36 / 32: the geometry of record i is resized_size / center_crop_box of image i, its bytes in the
    packed buffer are the image, and the table words at its offsets are pack_table(axis_table(...)) of its axes -- rebuilt here
    from the packed words and compared field by field.  Host copy and device copy of the records are equal."""
    ims = _images(SIZES, chw)
    tables_before = dict(P._tables)
    y = P.imagenet_eval(ims, resize=RESIZE, crop=CROP)
    assert tuple(y.shape) == (len(SIZES), 3, CROP, CROP) and y.dtype == torch.float32
    (c,) = on_host
    assert (c["B"], c["hout"], c["wout"], c["chw"], c["dtype"], c["nhwc"]) == (len(SIZES), CROP, CROP, int(chw), _lib.F32, 0)
    assert c["rec_host"].tobytes() == c["rec_dev"].tobytes()
    a, b = P.affine(P.IMAGENET_MEAN, P.IMAGENET_STD)
    assert np.array_equal(c["a"], a) and np.array_equal(c["b"], b)
    rec, tab, offset, word = c["rec_host"], c["tab"], 0, 0
    for i, ((hin, win), im) in enumerate(zip(SIZES, ims)):
        g = rec[i]
        hr, wr = P.resized_size(hin, win, RESIZE)
        top, left, hout, wout = P.center_crop_box(hr, wr, CROP)
        assert (g["Hin"], g["Win"], g["Hr"], g["Wr"], g["top"], g["left"]) == (hin, win, hr, wr, top, left), i
        assert g["offset"] == offset, i                                       # tightly packed, in list order
        assert np.array_equal(c["x"][offset:offset + hin * win * 3], im.reshape(-1)), i
        offset += hin * win * 3
        for n_in, n_out, start, count, at, m in ((hin, hr, top, hout, g["tab_h"], g["mh"]), (win, wr, left, wout, g["tab_w"], g["mw"])):
            assert at == word, i                                              # tables back to back: rows, then columns
            first, taps, w = P.axis_table(n_in, n_out, start, count)
            assert m == w.shape[1] <= P.MAX_TAPS
            words = tab[at:at + count * (2 + m)]
            assert np.array_equal(words[:count], first) and np.array_equal(words[count:2 * count], taps), i
            assert np.array_equal(words[2 * count:].view(np.float32).reshape(count, m), w), i
            word += count * (2 + m)
    assert offset == c["x"].size and word == tab.size
    assert P._tables == tables_before                                         # nothing kept on the device
    assert SIZES[3] == (20, 31) and SIZES[4] == (53, 47) and rec[5]["offset"] % 2 == 1       # the steep image starts on an odd byte
    # the steep image: what the entry's tap check computes for it is 22 per axis, under the limit of 24; the rows / columns of
    # the crop happen to need 21 or 22 of them
    assert int(2 * 380 / 36 + 1) == 22 and int(2 * 400 / 37 + 1) == 22 and P.MAX_TAPS == 24
    assert rec[5]["mh"] in (21, 22) and rec[5]["mw"] in (21, 22)


def test_one_geometry_or_one_per_image(on_host):
    ims = _images([(40, 30), (30, 44)])
    P.resize_crop_normalize(ims, (24, 24), (2, 3, 16, 20), dtype="bf16", layout="nhwc")
    P.resize_crop_normalize(ims, [(24, 24), (20, 30)], [(2, 3, 16, 20), (0, 10, 16, 20)])
    one, per = on_host
    assert (one["dtype"], one["nhwc"], one["hout"], one["wout"]) == (_lib.BF16, 1, 16, 20)
    assert [tuple(int(v) for v in r)[1:7] for r in one["rec_host"]] == [(40, 30, 24, 24, 2, 3), (30, 44, 24, 24, 2, 3)]
    assert [tuple(int(v) for v in r)[1:7] for r in per["rec_host"]] == [(40, 30, 24, 24, 2, 3), (30, 44, 20, 30, 0, 10)]


def test_torch_and_numpy_images_pack_alike(on_host):
    ims = _images(SIZES[:3])
    P.imagenet_eval(ims, resize=RESIZE, crop=CROP)
    P.imagenet_eval(tuple(torch.from_numpy(im) for im in ims), resize=RESIZE, crop=CROP)
    P.imagenet_eval([ims[0], torch.from_numpy(ims[1]), np.asfortranarray(ims[2])], resize=RESIZE, crop=CROP)      # not C-contiguous
    a, b, c = on_host
    for other in (b, c):
        assert np.array_equal(a["x"], other["x"]) and a["rec_host"].tobytes() == other["rec_host"].tobytes()
        assert np.array_equal(a["tab"], other["tab"])


def test_refusals_name_the_image_before_any_call(monkeypatch):
    def no_launch(*a, **k):
        raise AssertionError("a refused call reached the library or the device")
    monkeypatch.setattr(_lib, "call", no_launch)
    monkeypatch.setattr(P, "device", no_launch)
    ok = _images([(40, 30), (30, 40)])
    ev = dict(resize=RESIZE, crop=CROP)
    with pytest.raises(ValueError, match="empty"):
        P.imagenet_eval([], **ev)
    with pytest.raises(ValueError, match="image 1.*uint8"):
        P.imagenet_eval([ok[0], ok[1].astype(np.float32)], **ev)
    with pytest.raises(ValueError, match="image 1.*shape"):
        P.imagenet_eval([ok[0], np.zeros((2, 40, 30, 3), np.uint8)], **ev)             # a batch inside the list
    with pytest.raises(ValueError, match="image 1.*shape"):
        P.imagenet_eval([ok[0], np.zeros((40, 30), np.uint8)], **ev)
    with pytest.raises(ValueError, match="image 1.*3 channels"):
        P.imagenet_eval([ok[0], np.zeros((40, 30, 4), np.uint8)], **ev)
    with pytest.raises(ValueError, match="image 1.*mixed layouts"):
        P.imagenet_eval([ok[0], np.zeros((3, 40, 30), np.uint8)], **ev)
    with pytest.raises(ValueError, match="image 0.*3 channels"):
        P.imagenet_eval([ok[0], np.zeros((3, 40, 30), np.uint8)], channels_last=False, **ev)
    with pytest.raises(ValueError, match="image 1.*mixed crop sizes"):
        P.resize_crop_normalize(ok, (36, 36), [(0, 0, 32, 32), (0, 0, 32, 30)])
    with pytest.raises(ValueError, match="image 1.*filter taps"):
        P.imagenet_eval([ok[0], np.zeros((470, 480, 3), np.uint8)], **ev)              # 13.06x: 27 taps
    with pytest.raises(ValueError, match="image 1.*does not lie inside"):
        P.resize_crop_normalize(ok, [(36, 36), (36, 30)], (0, 0, 32, 32))
    with pytest.raises(ValueError, match="image 0.*does not lie inside"):
        P.imagenet_eval(ok, resize=16, crop=24)
    with pytest.raises(ValueError, match="one such entry per image"):
        P.resize_crop_normalize(ok, [(36, 36)] * 3, (0, 0, 32, 32))
    with pytest.raises(ValueError, match="dtype"):
        P.imagenet_eval(ok, dtype="fp16", **ev)
    with pytest.raises(ValueError, match="layout"):
        P.imagenet_eval(ok, layout="nhwc", **ev)


def test_ambiguous_shapes_follow_the_list_or_channels_last(on_host):
    """[3, N, 3] could be either layout: alone it is HWC as in the array path, next to an image that leaves no doubt it follows
    that image, and `channels_last` decides over both."""
    amb, chw_im, hwc_im = np.zeros((3, 6, 3), np.uint8), np.zeros((3, 8, 6), np.uint8), np.zeros((8, 6, 3), np.uint8)
    geo = ((4, 4), (0, 0, 2, 2))
    P.resize_crop_normalize([amb], *geo)
    P.resize_crop_normalize([amb, chw_im], *geo)
    P.resize_crop_normalize([hwc_im, amb], *geo)
    P.resize_crop_normalize([amb], *geo, channels_last=False)
    assert [c["chw"] for c in on_host] == [0, 1, 0, 1]
    assert [(int(c["rec_host"][0]["Hin"]), int(c["rec_host"][0]["Win"])) for c in on_host] == [(3, 6), (6, 3), (8, 6), (6, 3)]


def test_list_inside_a_recording_is_refused(monkeypatch):
    def no_launch(*a, **k):
        raise AssertionError("a refused call reached the library or the device")
    monkeypatch.setattr(_lib, "call", no_launch)
    monkeypatch.setattr(P, "device", no_launch)
    ims = _images([(40, 30), (30, 40)])
    with _act.keep_alive([]):
        with pytest.raises(ValueError, match="filter_jit"):
            P.imagenet_eval(ims, resize=RESIZE, crop=CROP)
        with pytest.raises(ValueError, match="filter_jit"):
            P.resize_crop_normalize(ims, (36, 36), (0, 0, 32, 32))


def test_axis_cache_is_bounded_and_tables_stay_off_the_device(on_host):
    """More distinct geometries than the cache holds: its size stops at its bound, later calls still get the right tables, and
    the per-geometry device cache of the array path never grows."""
    tables_before = dict(P._tables)
    P._axis_words.cache_clear()
    assert P._axis_words.cache_info().maxsize == P.AXIS_CACHE
    for n in range(2, P.AXIS_CACHE + 300):
        P._axis_words(n + 1, n, 0, 1)
    assert P._axis_words.cache_info().currsize == P.AXIS_CACHE
    ims = _images([(40, 30), (30, 44)])
    P.imagenet_eval(ims, resize=RESIZE, crop=CROP)
    assert P._axis_words.cache_info().currsize == P.AXIS_CACHE
    (c,) = on_host
    g = c["rec_host"][1]
    first, taps, w = P.axis_table(44, int(g["Wr"]), int(g["left"]), CROP)
    assert np.array_equal(c["tab"][g["tab_w"]:g["tab_w"] + CROP], first)
    words, m = P._axis_words(44, int(g["Wr"]), int(g["left"]), CROP)
    assert not words.flags.writeable and m == w.shape[1]                      # cached arrays cannot be changed behind the cache
    assert P._tables == tables_before
    P._axis_words.cache_clear()


def test_entry_validates_the_host_records_before_any_device_call(built_lib):
    """`mv_preprocess_u8_ragged_fwd` checks the host copy of the records before it touches the device, so its refusals can be
    seen without one: made-up (never dereferenced) device addresses, a real host record array.  Each message names the image."""
    rec, tables, (hout, wout) = P.ragged_plan([(40, 30), (30, 44)], [(36, 27), (24, 36)], (1, 2, 20, 24))
    x_bytes, X, Y, REC, TAB, AB = 40 * 30 * 3 + 30 * 44 * 3, 1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20

    def call(r, x_bytes=x_bytes, tab_words=tables.size, y=Y, B=2):
        r = np.ascontiguousarray(r)
        return built_lib.mv_preprocess_u8_ragged_fwd(X, x_bytes, y, r.ctypes.data, REC, TAB, tab_words, AB, AB, B, hout, wout, 0, _lib.F32,
                                                     0, None), built_lib.mv_last_error()

    def changed(i, **kw):
        r = rec.copy()
        for k, v in kw.items():
            r[k][i] = v
        return r

    for r, kw, word in ((changed(1, offset=rec["offset"][1] + 1), {}, b"image 1: 3960 bytes at offset 3601"),
                        (changed(0, offset=-1), {}, b"image 0"),
                        (rec, {"x_bytes": x_bytes - 1}, b"image 1"),
                        (changed(1, tab_w=tables.size - 1), {}, b"image 1: tables"),
                        (changed(0, tab_h=-4), {}, b"image 0: tables"),
                        (rec, {"tab_words": tables.size - 1}, b"image 1: tables"),
                        (changed(1, mw=rec["mw"][1] + 1), {}, b"image 1: tables"),
                        (changed(1, top=5), {}, b"image 1: crop"),
                        (changed(0, left=-1), {}, b"image 0: crop"),
                        (changed(1, Hr=2, mh=P.MAX_TAPS), {"tab_words": 1 << 20}, b"image 1: crop"),
                        (changed(0, mh=P.MAX_TAPS + 1), {"tab_words": 1 << 20}, b"image 0: 40x30 -> 36x27 needs"),
                        (changed(1, Hin=300, Hr=24, offset=0), {"x_bytes": 1 << 20}, b"image 1: 300x44 -> 24x36 needs up to 26"),
                        (changed(0, Win=0), {}, b"image 0: bad sizes"),
                        (rec, {"y": X + 100}, b"overlap")):
        rc, msg = call(r, **kw)
        assert rc in (-1, -2) and word in msg, (rc, msg, word)
    assert call(rec, B=0)[0] == -1 and call(rec, B=70000)[0] == -1
