"""Restatements and cases for the segmentation input pipeline (`eqxvision_amd.preprocess.segmentation_train` and what it is made
of), shared by tests/test_preprocess_seg_host.py and tests/test_preprocess_seg_gpu.py:
  * the label rule and the padded-window semantics of `mv_preprocess_u8_seg_fwd` as scalar Python in float64;
  * the two samplers as plain Python, fed the uniforms the code under test drew;
  * the images, masks and geometry sets of the GPU file, so that the host file can check its preconditions without a device."""
import functools
import math

import numpy as np

from tests import _augment_ref as A
from tests import _preprocess_ref as R

CROP = (32, 40)               # one full 32 x 32 tile and a partial one beside it
CLASSES = 21
VOID = 255
TINY_FIRST = (9, 5)           # 135 bytes of image, 45 of mask: every image behind it starts on an odd byte of both buffers

# name -> one (Hr, Wr, top, left) per image; every set runs with the flips of `flips(name)`
GEOMETRY = {
    # the resized image is larger than the crop on both axes: no padding.  Image 0 sits at the last valid origin (Hr - 32, Wr - 40),
    # image 1 is not resized at all, image 3 is up-sampled 2x, the large image goes down 11.1x to 36 rows (23 taps)
    "inside": [(60, 44, 28, 4), (37, 50, 3, 7), (45, 45, 0, 0), (40, 62, 5, 11), (48, 43, 10, 2), (36, 44, 2, 3)],
    # smaller than the crop on both axes: partly filled tiles, columns 32.. of nothing but fill, image 4 with one row and one column
    # of fill.  The large image cannot: below 34 rows it needs more than 24 taps, so it pads its columns only, at 24 taps per axis
    "pad": [(24, 18, 0, 0), (16, 22, 0, 0), (20, 20, 0, 0), (20, 31, 0, 0), (31, 39, 0, 0), (34, 33, 2, 0)],
    # padding on one axis only, origins off zero on the other; image 2 up-sampled 2x without padding
    "mixed": [(40, 30, 8, 0), (24, 60, 0, 20), (72, 72, 40, 32), (40, 31, 3, 0), (30, 47, 0, 7), (40, 38, 8, 0)],
    # resized to next to nothing: TINY_FIRST goes in front of the batch and becomes 1 x 1 (taps = the whole axis, so nothing larger
    # than 24 pixels can), image 3 becomes one row
    "tiny": [(1, 1, 0, 0), (5, 4, 0, 0), (4, 5, 0, 0), (4, 4, 0, 0), (1, 3, 0, 0), (5, 5, 0, 0), (35, 34, 3, 0)],
}


def sizes(name):
    return ([TINY_FIRST] if name == "tiny" else []) + list(A.SIZES)


def flips(name):
    return ([True] if name == "tiny" else []) + list(A.FLIPS)


@functools.lru_cache(maxsize=None)
def images(name):
    """uint8 HWC images of the set, read-only; those of A.SIZES are the ones of tests/test_preprocess_train_gpu.py."""
    out = tuple(R.images(hw, 1)[0] for hw in sizes(name))
    for im in out:
        im.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def masks(name):
    """uint8 [H, W] label maps of the set: labels in [0, CLASSES), about one pixel in eight VOID; read-only."""
    out = []
    for h, w in sizes(name):
        rng = np.random.default_rng(7000 + 1000 * h + w)
        m = rng.integers(0, CLASSES, (h, w), dtype=np.uint8)
        m[rng.random((h, w)) < 0.125] = VOID
        m.setflags(write=False)
        out.append(m)
    return tuple(out)


def label_index(o, n_in, n_out):
    """The source index of output o of an n_in -> n_out nearest resize by the centre rule, in float64: the centre of output o lies
    at (o + 0.5) n_in / n_out.  The product is an exact integer multiple of 0.5 below 2^53 and the quotient's floor is that of
    the exact ratio (a float64 division is correctly rounded and cannot cross an integer it does not reach: the exact quotient
    of two integers a / n that is below k lies at least 1 / n below it), so this is (2 o + 1) n_in // (2 n_out)."""
    return min(int(math.floor(((o + 0.5) * n_in) / n_out)), n_in - 1)


def torch_default_nearest(o, n_in, n_out):
    """torch's default mode="nearest": floor(o * scale) with the fp32 scale n_in / n_out -- the rule NOT to use."""
    return min(int(math.floor(np.float32(o) * (np.float32(n_in) / np.float32(n_out)))), n_in - 1)


def window(value_at, Hr, Wr, top, left, flip, fill, crop=CROP):
    """The padded-window semantics, one pixel at a time: output (i, j) is padded pixel (top + i, left + j); outside the resized
    Hr x Wr image that is `fill`, inside it `value_at(r, c)` with c the column BEFORE the mirror.  Returns a list of rows."""
    out = []
    for i in range(crop[0]):
        r, row = top + i, []
        for j in range(crop[1]):
            q = left + j
            row.append(fill if r >= Hr or q >= Wr else value_at(r, Wr - 1 - q if flip else q))
        out.append(row)
    return out


def labels_ref(mask, geo, flip, fill=VOID, crop=CROP):
    """int32 [Hc, Wc]: the label map the kernel must give for one mask."""
    Hr, Wr, top, left = geo
    hin, win = mask.shape
    rows = [label_index(r, hin, Hr) for r in range(Hr)]
    cols = [label_index(c, win, Wr) for c in range(Wr)]
    return np.asarray(window(lambda r, c: int(mask[rows[r], cols[c]]), Hr, Wr, top, left, flip, fill, crop), np.int32)


def valid_extent(geo, crop=CROP):
    """(hv, wv): the rows and columns of the window that lie inside the resized image."""
    Hr, Wr, top, left = geo
    return max(0, min(crop[0], Hr - top)), max(0, min(crop[1], Wr - left))


def axes_used():
    """Every (n_in, n_out) the GPU file resizes along the (H, W) axis: two sorted lists."""
    rows, cols = set(), set()
    for name, geos in GEOMETRY.items():
        for (h, w), (Hr, Wr, _, _) in zip(sizes(name), geos):
            rows.add((h, Hr))
            cols.add((w, Wr))
    return sorted(rows), sorted(cols)


def resize_sizes(u, sizes_hw, lo, hi):
    """RandomResize on given uniforms u [B]: the shorter side becomes lo + min(int(u (hi - lo + 1)), hi - lo)."""
    out = []
    for (h, w), ui in zip(sizes_hw, u):
        s = lo + min(int(float(ui) * (hi - lo + 1)), hi - lo)
        out.append((s, int(s * w / h)) if h <= w else (int(s * h / w), s))
    return np.asarray(out, np.int64)


def crop_origins(u, resized, crop):
    """RandomCrop.get_params on the padded size, on given uniforms u [B, 2]."""
    out = []
    for (hr, wr), ui in zip(resized, u):
        fh, fw = max(hr, crop[0]) - crop[0], max(wr, crop[1]) - crop[1]
        out.append((min(int(float(ui[0]) * (fh + 1)), fh), min(int(float(ui[1]) * (fw + 1)), fw)))
    return np.asarray(out, np.int64)
