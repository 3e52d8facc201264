"""Restatements for the training-time input pipeline (`eqxvision_amd.preprocess.imagenet_train` and what it is made of), shared by
tests/test_preprocess_train_host.py and tests/test_preprocess_train_gpu.py:
  * torchvision's RandomResizedCrop.get_params as plain numpy, fed the uniforms the code under test drew;
  * the weight recipe `mv_preprocess_u8_boxes_fwd` runs inside the kernel (float64, sequential sum, one rounding to fp32), one
    output at a time, as scalar Python -- no tables, no vector code shared with `preprocess.axis_table`;
  * the images, boxes and output sizes of the GPU file, so that the host file can check the recipe on exactly those axes."""
import math

import numpy as np

# the batch of tests/test_preprocess_ragged_gpu.py; the last image starts on an odd byte of the packed buffer
SIZES = [(50, 37), (37, 50), (36, 36), (20, 31), (53, 47), (400, 380)]
OUT = (32, 40)                # exactly one 32 x 32 tile; partial edge tiles

# name -> one (top, left, h, w) per image of SIZES, for either output size
BOX_SETS = {
    # the whole image; of the large one a 368 x 368 box: to 32 that is 11.5x, exactly 24 taps, the 4 x 8 tile, 4 x 8 tiles staged
    "whole": [(0, 0, 50, 37), (0, 0, 37, 50), (0, 0, 36, 36), (0, 0, 20, 31), (0, 0, 53, 47), (16, 6, 368, 368)],
    # 1 x 1: one tap, pure replication (the first and the last pixel of the buffer among them); 3 x 30: up-sampled on both axes
    # by different factors, at an odd byte offset (image 3 starts at byte 14988, (1 * 31 + 0) * 3 = 93 is odd); 3 x 36 and
    # 3 x 47: up-sampled on one axis, down-sampled on the other (3 x 36 only to 32)
    "small": [(49, 36, 1, 1), (0, 0, 1, 1), (17, 0, 3, 36), (1, 0, 3, 30), (9, 0, 3, 47), (399, 379, 1, 1)],
    # boxes that end at the last pixel of their image: the last one ends the packed buffer, its 16-byte chunks cross that end
    "ends": [(20, 7, 30, 30), (7, 20, 30, 30), (1, 1, 35, 35), (17, 0, 3, 31), (0, 44, 53, 3), (380, 347, 20, 33)],
}
FLIPS = [True, False, True, True, False, True]
ARRAY_SHAPE = (50, 37)        # the equal-size cases: [2, 50, 37, 3]
ARRAY_BOXES = [(3, 4, 40, 30), (0, 0, 50, 37)]


def axes_used():
    """Every (n_box, n_out) the GPU file resizes along an axis."""
    out = set()
    for size in OUT:
        for boxes in list(BOX_SETS.values()) + [ARRAY_BOXES]:
            for _, _, h, w in boxes:
                out.add((h, size))
                out.add((w, size))
    return sorted(out)


def taps_needed(n_box, n_out):
    return min(n_box, int(2.0 * max(1.0, n_box / n_out) + 1.0))


def usable(boxes, size):
    """The boxes of a set that an output size can take (at most 24 taps per axis); the others are the refusal tests' business."""
    return [i for i, (_, _, h, w) in enumerate(boxes) if taps_needed(h, size) <= 24 and taps_needed(w, size) <= 24]


def kernel_axis(n_box, n_out):
    """The filter the kernel generates for one axis of a box: (first int [n_out], taps int [n_out], weights: list of fp32 arrays).
    Output o: centre s = (o + 0.5) n_box / n_out - 0.5, support sup = max(1, n_box / n_out), taps floor(s - sup) + 1 ..
    ceil(s + sup) - 1 clipped to the box, weights 1 - |x - s| / sup in ascending order, summed in that order (float64), each
    quotient rounded once to fp32."""
    ratio = n_box / n_out
    sup = ratio if ratio > 1.0 else 1.0
    first, taps, weights = [], [], []
    for o in range(n_out):
        s = (o + 0.5) * ratio - 0.5
        lo = max(math.floor(s - sup) + 1, 0)
        hi = min(math.ceil(s + sup) - 1, n_box - 1)
        w = [max(0.0, 1.0 - abs(x - s) / sup) for x in range(lo, hi + 1)]
        total = 0.0
        for v in w:
            total += v
        first.append(lo)
        taps.append(hi - lo + 1)
        weights.append(np.asarray([np.float32(v / total) for v in w], np.float32))
    return np.asarray(first), np.asarray(taps), weights


def nonzero_taps(n_box, n_out):
    """int [n_out]: the non-zero weights of each output."""
    return np.asarray([int(np.count_nonzero(w)) for w in kernel_axis(n_box, n_out)[2]])


def rrc_boxes(u, sizes, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0)):
    """RandomResizedCrop.get_params on given uniforms u [B, 10, 4] -> (int [B, 4] of (top, left, h, w), bool [B]: an attempt won)."""
    u = np.asarray(u, np.float64)
    boxes, won = [], []
    for (H, W), ui in zip(sizes, u):
        area = H * W * (scale[0] + ui[:, 0] * (scale[1] - scale[0]))
        ar = np.exp(np.log(ratio[0]) + ui[:, 1] * (np.log(ratio[1]) - np.log(ratio[0])))
        w = np.rint(np.sqrt(area * ar)).astype(np.int64)              # rint and round() both round halves to even
        h = np.rint(np.sqrt(area / ar)).astype(np.int64)
        fits = (w > 0) & (w <= W) & (h > 0) & (h <= H)
        if fits.any():
            t = int(np.argmax(fits))
            hh, ww = int(h[t]), int(w[t])
            boxes.append((min(int(ui[t, 2] * (H - hh + 1)), H - hh), min(int(ui[t, 3] * (W - ww + 1)), W - ww), hh, ww))
        else:
            if W / H < ratio[0]:
                ww = W
                hh = int(round(ww / ratio[0]))
            elif W / H > ratio[1]:
                hh = H
                ww = int(round(hh * ratio[1]))
            else:
                hh, ww = H, W
            boxes.append(((H - hh) // 2, (W - ww) // 2, hh, ww))
        won.append(bool(fits.any()))
    return np.asarray(boxes, np.int64), np.asarray(won)
