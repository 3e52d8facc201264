"""CPU: the host half of the segmentation input pipeline of `eqxvision_amd.preprocess` -- the two samplers against plain-Python
restatements fed the same uniforms, the records `mv_preprocess_u8_seg_fwd` receives, every refusal before the library is reached,
the integer label rule against its float64 restatement on every axis the GPU file uses, the preconditions of the GPU file, and
the entry's host-side validation and tile sizing in a stand-alone sanitised program (tests/seg_validate.cpp)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

from eqxvision_amd import _act, _lib
from eqxvision_amd import preprocess as P
from eqxvision_amd import random as jr
from eqxvision_amd.build import HIPCC
from tests import _augment_ref as A
from tests import _seg_augment_ref as S

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = A.SIZES + [(224, 224), (500, 375), (375, 500), (10, 400), (400, 10), (1, 1)]


@pytest.fixture
def no_launch(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a refused call reached the library or the device")
    monkeypatch.setattr(_lib, "call", refuse)
    monkeypatch.setattr(P, "device", refuse)


def _bytes_at(ptr, n):
    return np.ctypeslib.as_array((ctypes.c_uint8 * n).from_address(ptr)).copy()


@pytest.fixture
def on_host(monkeypatch):
    calls = []

    def fake_call(name, *a):
        assert name == "mv_preprocess_u8_seg_fwd" and len(a) == len(_lib.PROTOTYPES[name])
        x, x_bytes, m, m_bytes, y, labels, rec_host, rec_dev, ca, cb, B, hout, wout, ifill, mfill, chw, dt, nhwc, stream = a
        assert (m is None) == (labels is None) and (m is not None or m_bytes == 0)
        calls.append({"x": _bytes_at(x, x_bytes), "m": None if m is None else _bytes_at(m, m_bytes),
                      "rec_host": _bytes_at(rec_host, B * P.SEG.itemsize).view(P.SEG),
                      "rec_dev": _bytes_at(rec_dev, B * P.SEG.itemsize).view(P.SEG), "B": B, "hout": hout, "wout": wout,
                      "fills": (ifill, mfill), "chw": chw, "dtype": dt, "nhwc": nhwc})
        return 0

    monkeypatch.setattr(_lib, "call", fake_call)
    monkeypatch.setattr(P, "device", lambda: torch.device("cpu"))
    monkeypatch.setattr(P, "empty", lambda shape, dtype: torch.empty(tuple(shape), dtype=dtype))
    monkeypatch.setattr(P, "stream_ptr", lambda: 0)
    monkeypatch.setattr(P, "_affines", {})
    return calls


# ---- samplers -----------------------------------------------------------------------------------------------------------------

def test_samplers_equal_the_restatements_on_the_same_uniforms_and_are_deterministic():
    for seed in range(6):
        key = jr.PRNGKey(seed)
        keys = jr.split(key, len(SIZES))
        got = P.random_resize_sizes(key, SIZES, 260, 1040)
        want = S.resize_sizes([jr.uniform(k, ()) for k in keys], SIZES, 260, 1040)
        assert got.dtype == np.int32 and got.shape == (len(SIZES), 2) and np.array_equal(got, want), (seed, got.tolist())
        assert np.array_equal(got, P.random_resize_sizes(key, SIZES, 260, 1040))
        for crop in (480, (32, 40), (2000, 100)):
            o = P.random_crop_origins(key, got, crop)
            c = (crop, crop) if isinstance(crop, int) else crop
            assert o.dtype == np.int32 and np.array_equal(o, S.crop_origins([jr.uniform(k, (2,)) for k in keys], got, c))
            assert np.array_equal(o, P.random_crop_origins(key, got, crop))
    a, b = P.random_resize_sizes(jr.PRNGKey(1), SIZES, 260, 1040), P.random_resize_sizes(jr.PRNGKey(2), SIZES, 260, 1040)
    assert not np.array_equal(a, b)
    two = P.random_resize_sizes(jr.PRNGKey(1), [(224, 224)] * 2, 260, 1040)      # image i draws from split(key, B)[i]
    assert not np.array_equal(two[0], two[1])


def test_samplers_stay_in_range_and_reach_both_ends_over_2000_keys():
    lo, hi, crop = 20, 27, (32, 40)
    sizes = [(50, 37), (37, 50)]
    seen_s, seen_top, seen_left = set(), set(), set()
    for seed in range(2000):
        key = jr.PRNGKey(seed)
        rs = P.random_resize_sizes(key, sizes, lo, hi)
        for (h, w), (hr, wr) in zip(sizes, rs.tolist()):
            s = min(hr, wr)
            assert lo <= s <= hi and (hr, wr) == P.resized_size(h, w, s)
            seen_s.add(s)
        resized = [(36, 44), (20, 30)]                  # 5 x 5 origins; padded on both axes: the origin (0, 0) only
        og = P.random_crop_origins(key, resized, crop)
        assert 0 <= og[0, 0] <= 4 and 0 <= og[0, 1] <= 4 and og[1].tolist() == [0, 0]
        seen_top.add(int(og[0, 0]))
        seen_left.add(int(og[0, 1]))
    assert seen_s == set(range(lo, hi + 1)) and seen_top == set(range(5)) and seen_left == set(range(5))


def test_samplers_refuse_bad_ranges():
    with pytest.raises(ValueError, match="min_size"):
        P.random_resize_sizes(jr.PRNGKey(0), [(8, 8)], 10, 9)
    with pytest.raises(ValueError, match="min_size"):
        P.random_resize_sizes(jr.PRNGKey(0), [(8, 8)], 0, 9)
    with pytest.raises(ValueError, match="image 1"):
        P.random_resize_sizes(jr.PRNGKey(0), [(8, 8), (0, 8)], 4, 9)
    with pytest.raises(ValueError, match="crop"):
        P.random_crop_origins(jr.PRNGKey(0), [(8, 8)], 0)
    with pytest.raises(ValueError, match="image 0"):
        P.random_crop_origins(jr.PRNGKey(0), [(0, 8)], 4)


# ---- records and refusals -----------------------------------------------------------------------------------------------------

class _Seg(ctypes.Structure):
    _fields_ = [("offset", ctypes.c_int64), ("mask_offset", ctypes.c_int64), ("Hin", ctypes.c_int32), ("Win", ctypes.c_int32),
                ("Hr", ctypes.c_int32), ("Wr", ctypes.c_int32), ("top", ctypes.c_int32), ("left", ctypes.c_int32),
                ("flip", ctypes.c_int32), ("pad", ctypes.c_int32)]


def test_record_is_the_headers_struct():
    assert P.SEG.itemsize == ctypes.sizeof(_Seg) == 48
    assert list(P.SEG.names) == [f[0] for f in _Seg._fields_]
    for name, ctype in _Seg._fields_:
        assert P.SEG.fields[name][1] == getattr(_Seg, name).offset and P.SEG.fields[name][0].itemsize == ctypes.sizeof(ctype), name


def _geo(name):
    g = np.asarray(S.GEOMETRY[name])
    return g[:, :2], g[:, 2:]


@pytest.mark.parametrize("chw", [False, True])
def test_every_form_of_input_becomes_records_of_the_one_entry(on_host, chw):
    ims = [np.ascontiguousarray(im.transpose(2, 0, 1)) if chw else im for im in S.images("pad")]
    ms = list(S.masks("pad"))
    rs, og = _geo("pad")
    x, lab = P.resize_pad_crop_pair(ims, ms, rs, og, S.CROP, A.FLIPS, dtype="bf16", image_fill=114, mask_fill=0)
    assert tuple(x.shape) == (6, 3, 32, 40) and x.dtype == torch.bfloat16 and tuple(lab.shape) == (6, 32, 40) and lab.dtype == torch.int32
    arr, marr = np.stack([ims[0], ims[0]]), np.stack([ms[0], ms[0]])
    x, lab = P.resize_pad_crop_pair(arr, None, rs[:2], og[:2], 24, layout="nhwc")
    assert tuple(x.shape) == (2, 24, 24, 3) and lab is None
    x, lab = P.resize_pad_crop_pair(torch.from_numpy(arr[1]), torch.from_numpy(marr[1]), rs[0], og[0], S.CROP, True)
    assert tuple(x.shape) == (3, 32, 40) and tuple(lab.shape) == (32, 40)
    lst, batch, one = on_host
    assert (lst["B"], lst["hout"], lst["wout"], lst["fills"], lst["chw"], lst["dtype"], lst["nhwc"]) == (6, 32, 40, (114, 0), int(chw), _lib.BF16, 0)
    assert (batch["B"], batch["hout"], batch["wout"], batch["fills"], batch["nhwc"], batch["m"]) == (2, 24, 24, (0, 255), 1, None)
    at = 0
    for i, (hw, im, m) in enumerate(zip(A.SIZES, ims, ms)):
        g = lst["rec_host"][i]
        assert tuple(int(v) for v in g) == (3 * at, at, hw[0], hw[1]) + tuple(S.GEOMETRY["pad"][i]) + (int(A.FLIPS[i]), 0), i
        assert np.array_equal(lst["x"][3 * at:3 * at + im.size], im.reshape(-1)) and np.array_equal(lst["m"][at:at + m.size], m.reshape(-1))
        at += m.size
    assert 3 * at == lst["x"].size and at == lst["m"].size
    assert tuple(int(v) for v in one["rec_host"][0]) == (0, 0, 50, 37) + tuple(S.GEOMETRY["pad"][0]) + (1, 0)
    assert np.array_equal(one["m"], ms[0].reshape(-1))
    for c in on_host:
        assert c["rec_host"].tobytes() == c["rec_dev"].tobytes()


def test_presets_are_the_core_on_the_draws_of_the_split_key(on_host):
    ims, ms = list(S.images("pad")), list(S.masks("pad"))
    key = jr.PRNGKey(11)
    x, lab = P.segmentation_train(ims, ms, key, base_size=40, crop_size=32)
    assert tuple(x.shape) == (6, 3, 32, 32) and tuple(lab.shape) == (6, 32, 32)
    k_size, k_flip, k_origin = jr.split(key, 3)
    rs = P.random_resize_sizes(k_size, A.SIZES, 20, 80)
    fl, og = P.random_flips(k_flip, 6), P.random_crop_origins(k_origin, rs, 32)
    P.resize_pad_crop_pair(ims, ms, rs, og, 32, fl)
    P.segmentation_train(ims, ms, key, base_size=40, crop_size=32)
    P.segmentation_train(ims, ms, jr.PRNGKey(12), base_size=40, crop_size=32)
    first, core, again, other = on_host
    assert first["rec_host"].tobytes() == core["rec_host"].tobytes() == again["rec_host"].tobytes() != other["rec_host"].tobytes()
    assert first["fills"] == (0, 255)
    x, lab = P.segmentation_eval(ims[0].copy(), ms[0].copy(), base_size=24)
    assert tuple(x.shape) == (3, 32, 24) and tuple(lab.shape) == (32, 24)
    assert tuple(int(v) for v in on_host[-1]["rec_host"][0]) == (0, 0, 50, 37, 32, 24, 0, 0, 0, 0)
    x, lab = P.segmentation_eval(np.stack([ims[0]] * 2), base_size=24)
    assert tuple(x.shape) == (2, 3, 32, 24) and lab is None


def test_every_refusal_names_the_image_before_any_call(no_launch):
    ok = [np.zeros((40, 30, 3), np.uint8), np.zeros((30, 40, 3), np.uint8)]
    mk = [np.zeros((40, 30), np.uint8), np.zeros((30, 40), np.uint8)]
    rs, og = [(40, 30), (30, 40)], [(0, 0), (0, 0)]
    for bad_rs, bad_og, word in (([(40, 30), (0, 40)], og, "image 1.*positive"), (rs, [(0, 0), (1, 0)], "image 1.*padded image 32x40"),
                                 (rs, [(9, 0), (0, 0)], "image 0.*window 32x32 at \\(9, 0\\)"), (rs, [(0, 0), (0, 9)], "image 1.*does not lie"),
                                 (rs, [(0, -1), (0, 0)], "image 0.*does not lie"), ([(40, 30), (30, 3)], og, "image 1.*27 filter taps")):
        with pytest.raises(ValueError, match=word):
            P.resize_pad_crop_pair(ok, mk, bad_rs, bad_og, 32)
    assert P.seg_plan([(40, 30)], [(40, 30)], [(8, 0)], None, 32)[1] == (32, 32)          # the last valid origin is not refused
    for kw, word in ((dict(resized=rs[:1]), "one size per image"), (dict(origins=og + og), "one origin per image"),
                     (dict(resized=np.asarray(rs, np.float32)), "integers"), (dict(flip=[True]), "one flag per image"),
                     (dict(crop=0), "crop"), (dict(crop=(32, 0)), "crop"), (dict(image_fill=256), "image_fill"),
                     (dict(mask_fill=-1), "mask_fill"), (dict(image_fill=0.5), "image_fill"), (dict(dtype="fp16"), "dtype"),
                     (dict(layout="hwc"), "layout"), (dict(std=(1.0, 0.0, 1.0)), "std")):
        args = dict(resized=rs, origins=og, crop=32)
        args.update(kw)
        with pytest.raises(ValueError, match=word):
            P.resize_pad_crop_pair(ok, mk, **args)
    for bad, word in ((mk[:1], "2 masks"), ([mk[0], mk[0]], "image 1: mask of shape"), ([mk[0], mk[1].astype(np.int32)], "image 1.*uint8"),
                      (np.zeros((2, 40, 30), np.uint8), "list of 2 masks")):
        with pytest.raises(ValueError, match=word):
            P.resize_pad_crop_pair(ok, bad, rs, og, 32)
    arr = np.stack([ok[0], ok[0]])
    for bad, word in ((mk[0], r"\[B, H, W\]"), (np.zeros((3, 40, 30), np.uint8), "3 masks for 2"), (np.zeros((2, 30, 40), np.uint8), "image 0: mask")):
        with pytest.raises(ValueError, match=word):
            P.resize_pad_crop_pair(arr, bad, [rs[0]] * 2, og, 32)
    with pytest.raises(ValueError, match="empty"):
        P.resize_pad_crop_pair([], [], [], [], 32)
    with pytest.raises(ValueError, match="image 1.*uint8"):
        P.resize_pad_crop_pair([ok[0], ok[1].astype(np.float32)], mk, rs, og, 32)
    with pytest.raises(ValueError, match="image 1.*one by one"):
        P.segmentation_eval(ok, mk, base_size=20)
    with pytest.raises(ValueError, match="image 0.*filter taps"):
        P.segmentation_train([np.zeros((400, 380, 3), np.uint8)], None, jr.PRNGKey(0), base_size=10, crop_size=16)   # 380 -> 5 .. 20


def test_the_core_inside_a_recording_is_refused(no_launch):
    ims, ms = list(S.images("pad"))[:2], list(S.masks("pad"))[:2]
    rs, og = _geo("pad")
    with _act.keep_alive([]):
        with pytest.raises(ValueError, match="filter_jit"):
            P.resize_pad_crop_pair(ims, ms, rs[:2], og[:2], S.CROP)
        with pytest.raises(ValueError, match="filter_jit"):
            P.segmentation_train(ims, ms, jr.PRNGKey(0), base_size=40, crop_size=32)
        with pytest.raises(ValueError, match="filter_jit"):
            P.segmentation_eval(ims[0], ms[0], base_size=24)


# ---- the label rule and the preconditions of the GPU file -------------------------------------------------------------------------

def test_integer_label_rule_is_the_float64_centre_rule_on_every_axis_of_the_gpu_file():
    rows, cols = S.axes_used()
    assert (9, 1) in rows and (400, 36) in rows and (20, 40) in rows and (380, 33) in cols and (50, 50) in cols
    for n_in, n_out in rows + cols + [(500, 260), (375, 1040), (3, 1000), (1000, 3), (1, 7)]:
        for o in range(n_out):
            want = ((2 * o + 1) * n_in) // (2 * n_out)
            assert S.label_index(o, n_in, n_out) == want and 0 <= want < n_in, (n_in, n_out, o)
            assert abs((want + 0.5) - (o + 0.5) * n_in / n_out) <= 0.5 + 1e-9                   # the source pixel that holds the centre


def test_preconditions_of_the_gpu_file():
    """Conditions, not measurements: fill and non-fill both well represented, enough distinct labels to tell a shifted or mirrored
    gather, and on each axis at least one resize on which torch's default `nearest` picks other pixels than the centre rule.
    The distinct-labels condition is asked of every image that keeps at least 9 resized pixels: TINY_FIRST keeps one."""
    differs = {"rows": 0, "cols": 0}
    for name, geos in S.GEOMETRY.items():
        fill = total = 0
        assert len(geos) == len(S.sizes(name)) == len(S.flips(name))
        for mask, geo, flip in zip(S.masks(name), geos, S.flips(name)):
            Hr, Wr, top, left = geo
            assert top >= 0 and left >= 0 and top + S.CROP[0] <= max(Hr, S.CROP[0]) and left + S.CROP[1] <= max(Wr, S.CROP[1])
            assert A.taps_needed(mask.shape[0], Hr) <= P.MAX_TAPS and A.taps_needed(mask.shape[1], Wr) <= P.MAX_TAPS
            lab = S.labels_ref(mask, geo, flip, fill=-1)
            hv, wv = S.valid_extent(geo)
            assert int((lab == -1).sum()) == lab.size - hv * wv and not (lab[:hv, :wv] == -1).any()
            fill += lab.size - hv * wv
            total += lab.size
            if Hr * Wr >= 9:
                assert len(np.unique(lab[:hv, :wv])) >= 3, (name, geo)
            for axis, n_in, n_out in (("rows", mask.shape[0], Hr), ("cols", mask.shape[1], Wr)):
                differs[axis] += any(S.label_index(o, n_in, n_out) != S.torch_default_nearest(o, n_in, n_out) for o in range(n_out))
        if name == "inside":
            assert fill == 0
            assert any((Hr - S.CROP[0], Wr - S.CROP[1]) == (top, left) for Hr, Wr, top, left in geos)
        else:
            assert fill >= 0.1 * total and total - fill >= 0.1 * total, (name, fill, total)
    assert differs["rows"] >= 1 and differs["cols"] >= 1, differs
    for name in S.GEOMETRY:                              # ... and in every set on some axis
        assert any(S.label_index(o, n, Hr) != S.torch_default_nearest(o, n, Hr) for m, (Hr, _, _, _) in zip(S.masks(name), S.GEOMETRY[name])
                   for n in [m.shape[0]] for o in range(Hr)), name
    assert sum(hw[0] * hw[1] for hw in S.sizes("tiny")[:2]) % 2 == 1 and S.sizes("tiny")[0] == S.TINY_FIRST


def test_eval_axes_of_the_gpu_file_have_the_same_weights_in_the_table_and_in_the_kernel():
    """tests/test_preprocess_seg_gpu.py compares `segmentation_eval` bit for bit with `resize_crop_normalize`, whose weights come
    from `axis_table` (numpy's sum) and not from the kernel's recipe (sequential sum): on the axes it uses, 50 -> 32 and 37 -> 24,
    the two give the same fp32 weights, so the comparison is one of arithmetic, not of weight rounding."""
    for n_in, n_out in ((50, 32), (37, 24)):
        first, taps, weights = A.kernel_axis(n_in, n_out)
        f, t, w = P.axis_table(n_in, n_out)
        assert np.array_equal(first, f) and np.array_equal(taps, t)
        for o in range(n_out):
            assert np.array_equal(weights[o], w[o, :taps[o]]), (n_in, n_out, o)


# ---- the entry's own host-side checks -------------------------------------------------------------------------------------------

def test_entry_validates_the_host_records_before_any_device_call(built_lib):
    """Made-up (never dereferenced) device addresses, a real host record array.  Each message names the image."""
    rec, (hout, wout) = P.seg_plan([(40, 30), (400, 44)], [(50, 20), (36, 48)], [(18, 0), (4, 8)], [False, True], (32, 40))
    x_bytes, m_bytes = 3 * (40 * 30 + 400 * 44), 40 * 30 + 400 * 44
    X, M, Y, L, REC, AB = 1 << 20, 2 << 20, 3 << 20, 4 << 20, 5 << 20, 6 << 20

    def call(r, x_bytes=x_bytes, m=M, m_bytes=m_bytes, y=Y, lab=L, B=2, fills=(0, 255)):
        r = np.ascontiguousarray(r)
        return built_lib.mv_preprocess_u8_seg_fwd(X, x_bytes, m, m_bytes, y, lab, r.ctypes.data, REC, AB, AB, B, hout, wout, fills[0],
                                                  fills[1], 0, _lib.F32, 0, None), built_lib.mv_last_error()

    def changed(i, **kw):
        r = rec.copy()
        for k, v in kw.items():
            r[k][i] = v
        return r

    invalid, unsupported = -1, -2
    for r, kw, rc_want, word in ((changed(1, offset=rec["offset"][1] + 1), {}, invalid, b"image 1: 52800 bytes at offset 3601"),
                                 (changed(0, offset=-1), {}, invalid, b"image 0"),
                                 (rec, {"x_bytes": x_bytes - 1}, invalid, b"image 1"),
                                 (changed(1, mask_offset=1201), {}, invalid, b"image 1: mask of 17600 bytes at offset 1201"),
                                 (rec, {"m_bytes": m_bytes - 1}, invalid, b"image 1: mask"),
                                 (changed(0, Win=0), {}, invalid, b"image 0: bad sizes"),
                                 (changed(1, Hr=0), {}, invalid, b"image 1: bad sizes"),
                                 (changed(0, top=19), {}, invalid, b"image 0: window 32x40 at (19, 0)"),
                                 (changed(0, left=1), {}, invalid, b"image 0: window"),
                                 (changed(1, top=-1), {}, invalid, b"image 1: window"),
                                 (changed(1, left=9), {}, invalid, b"image 1: window 32x40 at (4, 9) does not lie inside the padded image 36x48"),
                                 (rec, {"m": None}, invalid, b"labels without masks"),
                                 (rec, {"lab": None}, invalid, b"masks without labels"),
                                 (rec, {"fills": (256, 255)}, invalid, b"image_fill 256"),
                                 (rec, {"fills": (0, -1)}, invalid, b"mask_fill -1"),
                                 (changed(1, Hr=33, top=1), {}, unsupported, b"image 1: 400x44 -> 33x48 needs up to 25 x 3 taps"),
                                 (rec, {"y": X + 100}, unsupported, b"images and output overlap"),
                                 (rec, {"lab": M + 8}, unsupported, b"masks and labels overlap"),
                                 (rec, {"lab": Y + 64}, unsupported, b"output and labels overlap")):
        rc, msg = call(r, **kw)
        assert rc == rc_want and word in msg, (rc, msg, word)
    assert call(rec, B=0)[0] == invalid and call(rec, B=70000)[0] == invalid


def test_host_validation_and_tile_sizing_run_clean_under_asan_and_ubsan(tmp_path):
    """tests/seg_validate.cpp: the entry's host code (record checks, tile and LDS sizing) compiled for the host only with
    AddressSanitizer and UBSan, as a program of its own, over good and bad records; it has no device to reach."""
    exe = str(tmp_path / "seg_validate")
    san = [f for flag in ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all") for f in ("-Xarch_host", flag)]
    cmd = [HIPCC, "--offload-arch=gfx950", "-x", "hip", "-std=c++17", "-O1"] + san + ["-I", os.path.join(HERE, "..", "include"), "-I", os.path.join(HERE, "..", "eqxvision_amd", "csrc"),
           os.path.join(HERE, "seg_validate.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all records answered as expected" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
