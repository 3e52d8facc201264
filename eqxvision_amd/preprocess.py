"""Image preprocessing on the device: uint8 images -> the tensor the models read, one launch (csrc/preprocess.hip).

    x = eqv.preprocess.imagenet_eval(images_u8)            # Resize(256, antialias) -> CenterCrop(224) -> ToTensor -> Normalize
    logits = eqv.vmap(net)(x)

The transform is torchvision's evaluation preset, the one the `torch_weights=` checkpoints were evaluated under: the resized size
and the crop offsets follow torchvision's rounding, the filter is `torch.nn.functional.interpolate(mode="bilinear", antialias=True)`
(the triangle filter of `jax.image.resize` -- oracle/np_ops.py restates it -- widened by in / out when down-sampling, weights
normalised over the taps inside the image).  The host builds the filter as one tap table per axis in float64, rounds the weights
to fp32, uploads them once per geometry and keeps them; the kernel only applies them.

    x = eqv.preprocess.imagenet_eval([img0, img1, ...])    # images of different sizes, still one launch

A list of images takes `mv_preprocess_u8_ragged_fwd`: the images packed tightly into one uint8 buffer, every table into one int32
buffer, one record per image (`RECORD`) that says where they lie.  The geometry belongs to that call, so nothing is kept on the
device and only the per-axis tables are cached, on the host and bounded (`AXIS_CACHE`).

    x = eqv.preprocess.imagenet_train(images_u8, key)      # RandomResizedCrop(224) -> RandomHorizontalFlip -> ToTensor -> Normalize

The training preset crops FIRST and resizes the crop, with a fresh random box per image and step, so tables would be rebuilt and
uploaded on every call.  `mv_preprocess_u8_boxes_fwd` takes one 40-byte record per image (`BOX`: where the image lies, the box,
whether to mirror) and generates the filter of each tile in the kernel, in float64, by the formulas of `axis_table`; the host
only draws the boxes (`random_resized_crop_boxes`, `random_flips`).  `crop_resize_normalize` is the deterministic core.

    x, targets = eqv.preprocess.imagenet_train_mixed(images_u8, labels, key, num_classes)   # ... -> RandomErasing -> Mixup / CutMix

The rest of torchvision's classification recipe rides in the same launch.  `mv_preprocess_u8_mix_fwd` takes the box records and a
second 52-byte record per image (`MIX`: the partner mixed in, the two weights, a cut rectangle, an erase rectangle, the weights of
the two labels) and writes the batch and the smoothed soft targets [B, K]; a tile resamples its partner only where it needs it.
The host draws (`mixup_cutmix_draw`, `random_erasing_draw`); `crop_resize_normalize_mix` is the deterministic core.

    x, labels = eqv.preprocess.segmentation_train(images_u8, masks_u8, key)   # RandomResize -> flip -> RandomCrop(pad) -> Normalize

The segmentation preset resizes the WHOLE image to a random size, mirrors it, pads it on the right and bottom up to the crop and
keeps a random window, and the label map goes through the same geometry.  `mv_preprocess_u8_seg_fwd` takes one 48-byte record
per image (`SEG`) and writes both in one launch: the image through the generated filter above with `image_fill` in the padding,
the labels as int32 by the centre-based nearest rule with `mask_fill` (255, the void label) in the padding.  The host draws sizes,
flips and origins (`random_resize_sizes`, `random_flips`, `random_crop_origins`); `resize_pad_crop_pair` is the deterministic
core, `segmentation_eval` the evaluation preset.

Outputs: NCHW in fp32 or bf16 are what the models' entry kernels read without a conversion launch (`_act.wrap` takes a [B, 3, H, W]
tensor as the image batch; the entry convolutions read fp32 or bf16).  The models have no NHWC entry, so `imagenet_eval` does not
offer one; `resize_crop_normalize(layout="nhwc")` returns a plain tensor for other consumers.
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from . import random as _random
from ._act import DT, TORCH_DT, device, empty, stream_ptr
from ._act import _tls as _act_tls
from ._module import DevArray

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
MAX_TAPS = 24          # MV_PREPROCESS_MAX_TAPS of include/eqxvision_amd.h: down-sampling by up to 11.5 per axis


def resized_size(h: int, w: int, size: int):
    """torchvision `Resize(size)` with an int: the shorter side becomes `size`, the longer one int(size * long / short)."""
    h, w, size = int(h), int(w), int(size)
    if h <= w:
        return size, int(size * w / h)
    return int(size * h / w), size


def center_crop_box(hr: int, wr: int, crop):
    """torchvision `CenterCrop`: (top, left, height, width) with top = int(round((hr - height) / 2.0))."""
    ch, cw = (int(crop), int(crop)) if isinstance(crop, (int, np.integer)) else (int(crop[0]), int(crop[1]))
    return int(round((hr - ch) / 2.0)), int(round((wr - cw) / 2.0)), ch, cw


def axis_table(n_in: int, n_out: int, start: int = 0, count: int = None):
    """The filter of one axis for the outputs start .. start + count - 1 of an n_in -> n_out resize.
    Returns (first int32 [count], taps int32 [count], weight fp32 [count, m]) with m = max(taps): output i is
    sum_k weight[i, k] * input[first[i] + k] over k < taps[i]; weight[i, taps[i]:] is 0.
    Sample centre s = (o + 0.5) in / out - 0.5, support max(1, in / out), weight 1 - |x - s| / support over the x inside the
    support and the axis, divided by their sum (float64), rounded to fp32."""
    n_in, n_out = int(n_in), int(n_out)
    count = n_out - start if count is None else int(count)
    if n_in < 1 or n_out < 1 or start < 0 or count < 1 or start + count > n_out:
        raise ValueError(f"axis_table: outputs {start}..{start + count} of a {n_in} -> {n_out} resize")
    ratio = n_in / n_out
    sup = max(1.0, ratio)
    o = np.arange(start, start + count, dtype=np.float64)
    s = (o + 0.5) * ratio - 0.5
    first = np.maximum(np.floor(s - sup).astype(np.int64) + 1, 0)
    last = np.minimum(np.ceil(s + sup).astype(np.int64) - 1, n_in - 1)
    taps = last - first + 1
    m = int(taps.max())
    x = first[:, None] + np.arange(m)[None, :]
    w = np.maximum(0.0, 1.0 - np.abs(x - s[:, None]) / sup)
    w[np.arange(m)[None, :] >= taps[:, None]] = 0.0
    w /= w.sum(1, keepdims=True)
    return first.astype(np.int32), taps.astype(np.int32), w.astype(np.float32)


def pack_table(first, taps, weight) -> np.ndarray:
    """The device layout of `mv_preprocess_u8_fwd`: int32 first[n] | int32 taps[n] | fp32 weight[n][m] as one int32 array."""
    return np.concatenate([first.astype(np.int32), taps.astype(np.int32), np.ascontiguousarray(weight, np.float32).reshape(-1).view(np.int32)])


def affine(mean, std):
    """(a, b) fp32 [3] of the epilogue y = acc * a + b: a = 1 / (255 std), b = -mean / std, computed in float64."""
    mean, std = np.asarray(mean, np.float64).reshape(-1), np.asarray(std, np.float64).reshape(-1)
    if mean.shape != (3,) or std.shape != (3,) or not np.all(std != 0):
        raise ValueError("preprocess: mean and std must be three numbers each, std non-zero")
    return (1.0 / (255.0 * std)).astype(np.float32), (-mean / std).astype(np.float32)


_tables = {}        # (device, Hin, Win, Hr, Wr, top, left, Hout, Wout) -> (tab_h, tab_w, taps_h, taps_w) on the device
_affines = {}       # (device, mean, std) -> (a, b) on the device


def _geometry(hin, win, resized_hw, crop_box, who="preprocess"):
    hr, wr = int(resized_hw[0]), int(resized_hw[1])
    top, left, hout, wout = (int(v) for v in crop_box)
    if hr < 1 or wr < 1 or hout < 1 or wout < 1:
        raise ValueError(f"{who}: resized size {(hr, wr)} and crop {(hout, wout)} must be positive")
    if top < 0 or left < 0 or top + hout > hr or left + wout > wr:
        raise ValueError(f"{who}: crop {hout}x{wout} at ({top}, {left}) does not lie inside the resized image {hr}x{wr}")
    return hr, wr, top, left, hout, wout


def _check_taps(hin, win, hr, wr, who="preprocess"):
    for n_in, n_out in ((hin, hr), (win, wr)):               # refused on the host, before the device is touched
        need = min(n_in, int(2.0 * max(1.0, n_in / n_out) + 1.0))
        if need > MAX_TAPS:
            raise ValueError(f"{who}: {hin}x{win} -> {hr}x{wr} needs {need} filter taps on an axis, at most {MAX_TAPS} "
                             f"(down-sampling by up to {(MAX_TAPS - 1) / 2})")


def _device_tables(hin, win, hr, wr, top, left, hout, wout):
    geo = (hin, win, hr, wr, top, left, hout, wout)
    _check_taps(hin, win, hr, wr)
    key = (str(device()),) + geo
    hit = _tables.get(key)
    if hit is None:
        th, tw = axis_table(hin, hr, top, hout), axis_table(win, wr, left, wout)
        hit = (torch.from_numpy(pack_table(*th)).to(device()), torch.from_numpy(pack_table(*tw)).to(device()),
               th[2].shape[1], tw[2].shape[1])
        _tables[key] = hit
    return hit


def _device_affine(mean, std):
    key = (str(device()), tuple(float(v) for v in np.asarray(mean).reshape(-1)), tuple(float(v) for v in np.asarray(std).reshape(-1)))
    hit = _affines.get(key)
    if hit is None:
        a, b = affine(mean, std)
        hit = _affines[key] = (torch.from_numpy(a).to(device()), torch.from_numpy(b).to(device()))
    return hit


def _check_input(images_u8, channels_last, who="preprocess"):
    """-> (array, batched, chw, Hin, Win); raises ValueError before anything touches the device."""
    x = images_u8
    if not isinstance(x, (np.ndarray, torch.Tensor)):
        raise ValueError(f"{who}: images must be a uint8 numpy array or torch tensor, got {type(x).__name__}")
    if x.dtype != (torch.uint8 if isinstance(x, torch.Tensor) else np.uint8):
        raise ValueError(f"{who}: images must be uint8 (decoded pixels 0..255), got {x.dtype}")
    if x.ndim not in (3, 4):
        raise ValueError(f"{who}: images must be [H, W, 3] / [3, H, W] or a batch of them, got shape {tuple(x.shape)}")
    batched = x.ndim == 4
    s = tuple(int(v) for v in x.shape[-3:])
    if channels_last is None:
        if s[2] == 3:
            chw = False
        elif s[0] == 3:
            chw = True
        else:
            raise ValueError(f"{who}: images must have 3 channels first or last, got shape {tuple(x.shape)}")
    else:
        chw = not channels_last
        if s[0 if chw else 2] != 3:
            raise ValueError(f"{who}: images must have 3 channels, got shape {tuple(x.shape)} with channels_last={channels_last}")
    hin, win = (s[1], s[2]) if chw else (s[0], s[1])
    if hin < 1 or win < 1:
        raise ValueError(f"{who}: empty image, shape {tuple(x.shape)}")
    return x, batched, chw, hin, win


def _check_output(dtype, layout):
    if dtype not in DT:
        raise ValueError(f"preprocess: dtype must be 'fp32' or 'bf16', got {dtype!r}")
    if layout not in ("nchw", "nhwc"):
        raise ValueError(f"preprocess: layout must be 'nchw' or 'nhwc', got {layout!r}")


# ---- what the record calls share on the host: intake, refusals, the trip to the device ------------------------------------------

class _Intake(NamedTuple):
    """Any accepted form of input.  listed: a list of images, else one array `x`; batched: False for one image without the batch
    axis; sizes: [(Hin, Win)] per image; x: what `_one_buffer` uploads."""
    listed: bool
    batched: bool
    chw: bool
    sizes: list
    x: object


def _intake(images_u8, channels_last) -> _Intake:
    if isinstance(images_u8, (list, tuple)):
        chw, sizes = _check_list(images_u8, channels_last)
        return _Intake(True, True, chw, sizes, images_u8)
    x, batched, chw, hin, win = _check_input(images_u8, channels_last)
    sizes = [(hin, win)] * (int(x.shape[0]) if batched else 1)
    if len(sizes) == 0:
        raise ValueError("preprocess: the batch of images is empty")
    return _Intake(False, batched, chw, sizes, x)


def _refuse_recording(who, what_belongs, advice=""):
    """The geometry of a record call belongs to that call: inside a `filter_jit` recording it is refused."""
    if getattr(_act_tls, "keep", None) is not None:
        raise ValueError(f"preprocess: {who} cannot be recorded by filter_jit: its {what_belongs} belong to this one call, and a "
                         f"replay would apply them to other images; preprocess outside the recorded function{advice}")


def _rows_of_one(v, width):
    """A per-image argument of an un-batched image as a batch of one: a scalar (`width` 0) becomes [1], a row of `width` numbers
    [1, width]; None and an argument that already has its batch axis stay."""
    if v is None:
        return None
    a = np.asarray(v)
    return a.reshape(-1) if width == 0 else (a.reshape(1, -1) if a.ndim == 1 else a)


def _int_rows(v, B, width, what, fields):
    a = np.asarray(v)
    if a.dtype.kind not in "iu" or a.shape != (B, width):
        raise ValueError(f"preprocess: {what} must be integers [{B}, {width}] of {fields} per image, got {a.dtype} {tuple(a.shape)}")
    return a


def _flags(flip, B):
    fl = np.zeros(B, bool) if flip is None else np.asarray(flip)
    if fl.shape != (B,):
        raise ValueError(f"preprocess: flip must hold one flag per image ({B}), got shape {tuple(fl.shape)}")
    return fl


def _pair(v, what):
    hw = (int(v), int(v)) if isinstance(v, (int, np.integer)) else tuple(int(s) for s in v)
    if len(hw) != 2 or hw[0] < 1 or hw[1] < 1:
        raise ValueError(f"preprocess: {what} {v!r} must be a positive int or (height, width)")
    return hw


def _affine_on_device(mean, std):
    affine(mean, std)                                        # validates before the device is touched
    return _device_affine(mean, std)


def _one_buffer(v):
    """A list -> `pack_images` (which packs any uint8 arrays, planes included); an array -> itself on the device, contiguous."""
    if isinstance(v, (list, tuple)):
        return pack_images(v)
    t = v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v))
    return t.to(device(), non_blocking=True).contiguous()


def _records_to_device(rec):
    return torch.from_numpy(rec.view(np.uint8)).to(device())


def _new_output(B, h, w, dtype, layout):
    return empty((B, 3, h, w) if layout == "nchw" else (B, h, w, 3), TORCH_DT[dtype])


# ---- batches of differently sized images: a list of images -> mv_preprocess_u8_ragged_fwd, one launch ----------------------------

# `mv_preprocess_image` of include/eqxvision_amd.h, 48 bytes
RECORD = np.dtype([("offset", "<i8"), ("Hin", "<i4"), ("Win", "<i4"), ("Hr", "<i4"), ("Wr", "<i4"), ("top", "<i4"), ("left", "<i4"),
                   ("tab_h", "<i4"), ("tab_w", "<i4"), ("mh", "<i4"), ("mw", "<i4")])
AXIS_CACHE = 4096      # tables kept on the HOST, per axis; a ragged call keeps nothing on the device


@functools.lru_cache(maxsize=AXIS_CACHE)
def _axis_words(n_in, n_out, start, count):
    """(`pack_table(*axis_table(...))`, read-only; its pitch).  ImageNet's validation set has a few hundred distinct (size, resized
    size) pairs per axis, so a warm cache leaves a call the concatenation only."""
    first, taps, w = axis_table(n_in, n_out, start, count)
    words = pack_table(first, taps, w)
    words.setflags(write=False)
    return words, w.shape[1]


def _is_device_tensor(im):
    return isinstance(im, torch.Tensor) and im.device.type != "cpu"


def _check_list(images, channels_last):
    """-> (chw, [(Hin, Win), ...]); every refusal names the image."""
    if len(images) == 0:
        raise ValueError("preprocess: the list of images is empty")
    for i, im in enumerate(images):
        _check_input(im, channels_last, f"preprocess: image {i}")
        if im.ndim != 3:
            raise ValueError(f"preprocess: image {i}: a list holds single images [H, W, 3] / [3, H, W], got shape {tuple(im.shape)}")
    if channels_last is None:                                # read off the images that leave no doubt; [3, W, 3] follows them
        chw, decided_by = False, None
        for i, im in enumerate(images):
            first, last = int(im.shape[0]) == 3, int(im.shape[2]) == 3
            if first != last:
                if decided_by is not None and chw != first:
                    raise ValueError(f"preprocess: image {i}: mixed layouts, shape {tuple(im.shape)} has its channels "
                                     f"{'first' if first else 'last'} and image {decided_by}, shape {tuple(images[decided_by].shape)}, "
                                     "has not; give every image of a list in the same layout")
                if decided_by is None:
                    chw, decided_by = first, i
    else:
        chw = not channels_last
    sizes = []
    for i, im in enumerate(images):
        s = tuple(int(v) for v in im.shape)
        if s[0 if chw else 2] != 3:
            raise ValueError(f"preprocess: image {i}: mixed layouts, shape {s} has no 3 channels "
                             f"{'first' if chw else 'last'} like the rest of the list")
        sizes.append((s[1], s[2]) if chw else (s[0], s[1]))
    return chw, sizes


def _per_image(value, B, width, what):
    """`value`: one geometry (`width` numbers) for all images or a list of B of them -> a list of B."""
    if len(value) == width and all(isinstance(v, (int, np.integer)) for v in value):
        return [value] * B
    if len(value) != B:
        raise ValueError(f"preprocess: {what} must be {width} numbers or one such entry per image ({B}), got {len(value)} entries")
    return list(value)


def ragged_plan(sizes, resized_hw, crop_box):
    """Host half of a ragged call, no device involved.  `sizes`: [(Hin, Win)] per image; `resized_hw`, `crop_box`: one geometry or
    one per image.  Returns (records, tables, (Hout, Wout)): `records` a RECORD array [B] for tightly packed images in list
    order, `tables` the int32 buffer its tab_h / tab_w offsets point into (each image's row table, then its column table)."""
    B = len(sizes)
    resized, boxes = _per_image(resized_hw, B, 2, "resized_hw"), _per_image(crop_box, B, 4, "crop_box")
    rec = np.zeros(B, RECORD)
    parts, offset, word, crop = [], 0, 0, None
    for i, (hin, win) in enumerate(sizes):
        who = f"preprocess: image {i}"
        hr, wr, top, left, hout, wout = _geometry(hin, win, resized[i], boxes[i], who)
        crop = crop or (hout, wout)
        if (hout, wout) != crop:
            raise ValueError(f"{who}: mixed crop sizes, {hout}x{wout} here and {crop[0]}x{crop[1]} for image 0; the images of one "
                             "call share the output size")
        _check_taps(hin, win, hr, wr, who)
        (th, mh), (tw, mw) = _axis_words(hin, hr, top, hout), _axis_words(win, wr, left, wout)
        rec[i] = (offset, hin, win, hr, wr, top, left, word, word + th.size, mh, mw)
        parts += [th, tw]
        offset += hin * win * 3
        word += th.size + tw.size
    if word >= 2 ** 31:
        raise ValueError(f"preprocess: the tables of {B} images take {word} words, more than an int32 offset reaches")
    return rec, np.concatenate(parts), crop


def pack_images(images) -> torch.Tensor:
    """The images as one tightly packed uint8 buffer on the device, in list order.  Host images are concatenated in one staging
    array and cross in one copy; device images are joined by one device concatenation."""
    host = [i for i, im in enumerate(images) if not _is_device_tensor(im)]
    up = None
    if host:
        flat = [np.ascontiguousarray(images[i].numpy() if isinstance(images[i], torch.Tensor) else images[i]).reshape(-1) for i in host]
        up = torch.from_numpy(np.concatenate(flat)).to(device(), non_blocking=True)
        if len(host) == len(images):
            return up
    pieces, at = [], 0
    for im in images:
        if _is_device_tensor(im):
            pieces.append(im.to(device()).reshape(-1))
        else:
            n = int(np.prod(im.shape))
            pieces.append(up[at:at + n])
            at += n
    return torch.cat(pieces)


def _ragged(images, resized_hw, crop_box, mean, std, dtype, layout, channels_last):
    _refuse_recording("a list of differently sized images", "sizes and offsets", ", or give one array of equally sized images")
    chw, sizes = _check_list(images, channels_last)
    _check_output(dtype, layout)
    rec, tables, (hout, wout) = ragged_plan(sizes, resized_hw, crop_box)
    a, b = _affine_on_device(mean, std)
    x = _one_buffer(images)
    tab, rec_dev = torch.from_numpy(tables).to(device()), _records_to_device(rec)
    B = len(images)
    y = _new_output(B, hout, wout, dtype, layout)
    _lib.call("mv_preprocess_u8_ragged_fwd", x.data_ptr(), x.numel(), y.data_ptr(), rec.ctypes.data, rec_dev.data_ptr(),
              tab.data_ptr(), tab.numel(), a.data_ptr(), b.data_ptr(), B, hout, wout, int(chw), DT[dtype], int(layout == "nhwc"),
              stream_ptr())
    return y


def resize_crop_normalize(images_u8, resized_hw, crop_box, mean=IMAGENET_MEAN, std=IMAGENET_STD, dtype="fp32", layout="nchw",
                          channels_last=None) -> torch.Tensor:
    """Resize uint8 images to `resized_hw` (antialiased triangle filter), keep `crop_box` = (top, left, height, width) of the resized
    image, return (x / 255 - mean) / std as a device tensor [B, 3, height, width] (`layout="nchw"`) or [B, height, width, 3], fp32
    or bf16.  `images_u8`: [B, H, W, 3] or [B, 3, H, W] (or one image without the batch axis), numpy or torch, host or device; the
    layout is read off which axis is 3 unless `channels_last` says so.  One launch on the current stream; recorded by `filter_jit`
    like any other (a device-resident input is then read in place, a host array is staged as uint8 once per call).
    A list or tuple of images [H_i, W_i, 3] (or all [3, H_i, W_i]) of DIFFERENT sizes is one launch too: `resized_hw` and
    `crop_box` are then one geometry for all images or lists with one entry per image, the crop's height and width the same for
    all.  The images are packed tightly into one buffer (one upload for host images), tables and records are built per call from
    a bounded host-side cache; such a call cannot be recorded by `filter_jit`."""
    if isinstance(images_u8, (list, tuple)):
        return _ragged(images_u8, resized_hw, crop_box, mean, std, dtype, layout, channels_last)
    x, batched, chw, hin, win = _check_input(images_u8, channels_last)
    _check_output(dtype, layout)
    hr, wr, top, left, hout, wout = _geometry(hin, win, resized_hw, crop_box)
    affine(mean, std)                                        # validates before the device is touched
    tab_h, tab_w, mh, mw = _device_tables(hin, win, hr, wr, top, left, hout, wout)
    a, b = _device_affine(mean, std)
    t = _one_buffer(x)
    B = t.shape[0] if batched else 1
    y = _new_output(B, hout, wout, dtype, layout)
    _lib.call("mv_preprocess_u8_fwd", t.data_ptr(), y.data_ptr(), tab_h.data_ptr(), tab_w.data_ptr(), a.data_ptr(), b.data_ptr(),
              B, hin, win, hr, wr, top, left, hout, wout, mh, mw, int(chw), DT[dtype], int(layout == "nhwc"), stream_ptr())
    keep = getattr(_act_tls, "keep", None)
    if keep is not None and t is not x:                      # uploaded inside a recording: the replayed launch reads this buffer
        keep.append(t)
    return y if batched else y[0]


def imagenet_eval(images_u8, resize=256, crop=224, mean=IMAGENET_MEAN, std=IMAGENET_STD, dtype="fp32", layout="nchw",
                  channels_last=None) -> torch.Tensor:
    """torchvision's ImageNet evaluation preset on the device: shorter side to `resize` (antialiased bilinear), centre crop `crop`,
    scale by 1 / 255, subtract `mean`, divide by `std`.  Returns [B, 3, crop, crop], fp32 or bf16: what `eqv.vmap(net)` reads.
    A list of images of different sizes (decoded photographs) gets the preset's geometry per image, in one launch."""
    if layout != "nchw":
        raise ValueError(f"preprocess.imagenet_eval: the models read NCHW images; layout={layout!r} is not one of their entries "
                         "(resize_crop_normalize offers NHWC for other consumers)")
    if isinstance(images_u8, (list, tuple)):
        _, sizes = _check_list(images_u8, channels_last)
        resized = [resized_size(h, w, resize) for h, w in sizes]
        boxes = [center_crop_box(hr, wr, crop) for hr, wr in resized]
        return resize_crop_normalize(images_u8, resized, boxes, mean, std, dtype, layout, channels_last)
    _, _, _, hin, win = _check_input(images_u8, channels_last)
    hr, wr = resized_size(hin, win, resize)
    return resize_crop_normalize(images_u8, (hr, wr), center_crop_box(hr, wr, crop), mean, std, dtype, layout, channels_last)


# ---- the training transform: crop a box, resize it, mirror it -> mv_preprocess_u8_boxes_fwd, one launch, no tables --------------

# `mv_preprocess_box` of include/eqxvision_amd.h, 40 bytes
BOX = np.dtype([("offset", "<i8"), ("Hin", "<i4"), ("Win", "<i4"), ("top", "<i4"), ("left", "<i4"), ("h", "<i4"), ("w", "<i4"),
                ("flip", "<i4"), ("pad", "<i4")])
RRC_ATTEMPTS = 10      # torchvision's RandomResizedCrop.get_params tries ten boxes before it falls back


def random_resized_crop_boxes(key, sizes, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0)) -> np.ndarray:
    """torchvision's `RandomResizedCrop.get_params` for B images: `sizes` [(H, W)] -> int32 [B, 4] of (top, left, h, w) in source
    pixels.  Host only.  Image i draws from `random.split(key, B)[i]`: with u = random.uniform(k_i, (10, 4)), attempt t takes
    area = H W (scale0 + u[t, 0] (scale1 - scale0)), aspect = exp(log r0 + u[t, 1] (log r1 - log r0)),
    w = round(sqrt(area aspect)), h = round(sqrt(area / aspect)); the first attempt that fits the image wins and is placed at
    top = min(int(u[t, 2] (H - h + 1)), H - h), left likewise from u[t, 3].  If none fits: the largest centred box whose aspect
    lies inside `ratio` (torchvision's fallback).
    This is torchvision's DISTRIBUTION, not torch's random stream: the same seed gives other boxes than torchvision does."""
    sizes = [(int(h), int(w)) for h, w in sizes]
    s0, s1 = (float(v) for v in scale)
    r0, r1 = (float(v) for v in ratio)
    if not (0.0 < s0 <= s1) or not (0.0 < r0 <= r1):
        raise ValueError(f"preprocess: scale {scale} and ratio {ratio} must be positive (min, max) pairs")
    if len(sizes) == 0:
        raise ValueError("preprocess: no image sizes")
    out = np.zeros((len(sizes), 4), np.int32)
    keys = _random.split(key, len(sizes))
    log0, log1 = np.log(np.float64(r0)), np.log(np.float64(r1))
    for i, (H, W) in enumerate(sizes):
        if H < 1 or W < 1:
            raise ValueError(f"preprocess: image {i}: empty image {H}x{W}")
        u = np.asarray(_random.uniform(keys[i], (RRC_ATTEMPTS, 4)), np.float64)
        for t in range(RRC_ATTEMPTS):
            area = H * W * (s0 + u[t, 0] * (s1 - s0))
            ar = np.exp(log0 + u[t, 1] * (log1 - log0))
            w, h = int(round(float(np.sqrt(area * ar)))), int(round(float(np.sqrt(area / ar))))
            if 0 < w <= W and 0 < h <= H:
                out[i] = (min(int(u[t, 2] * (H - h + 1)), H - h), min(int(u[t, 3] * (W - w + 1)), W - w), h, w)
                break
        else:
            if W / H < r0:
                w = W
                h = int(round(w / r0))
            elif W / H > r1:
                h = H
                w = int(round(h * r1))
            else:
                h, w = H, W
            out[i] = ((H - h) // 2, (W - w) // 2, h, w)
    return out


def random_flips(key, B, p=0.5) -> np.ndarray:
    """bool [B]: `random.uniform(key, (B,)) < p` (torchvision's RandomHorizontalFlip, one draw per image)."""
    return np.asarray(_random.uniform(key, (int(B),)) < p, bool)


def boxes_plan(sizes, boxes, flip, size):
    """Host half of `crop_resize_normalize`, no device involved: `sizes` [(Hin, Win)] of tightly packed images in order, `boxes`
    [B, 4] of (top, left, h, w), `flip` None or [B].  Returns (records, (Hout, Wout)), `records` a BOX array [B]; every refusal is
    a ValueError that names the image."""
    B = len(sizes)
    hout, wout = _pair(size, "output size")
    bx, fl = _int_rows(boxes, B, 4, "boxes", "(top, left, h, w), one box"), _flags(flip, B)
    rec = np.zeros(B, BOX)
    offset = 0
    for i, (hin, win) in enumerate(sizes):
        who = f"preprocess: image {i}"
        top, left, h, w = (int(v) for v in bx[i])
        if h < 1 or w < 1 or top < 0 or left < 0 or top + h > hin or left + w > win:
            raise ValueError(f"{who}: box {h}x{w} at ({top}, {left}) does not lie inside the image {hin}x{win}")
        _check_taps(h, w, hout, wout, who)
        rec[i] = (offset, hin, win, top, left, h, w, int(bool(fl[i])), 0)
        offset += hin * win * 3
    return rec, (hout, wout)


def crop_resize_normalize(images_u8, boxes, size, flip=None, mean=IMAGENET_MEAN, std=IMAGENET_STD, dtype="fp32", layout="nchw",
                          channels_last=None) -> torch.Tensor:
    """Crop box i = (top, left, h, w) out of image i (source pixels), resize it to `size` (an int or (Hout, Wout)) with the
    antialiased triangle filter of `resize_crop_normalize` -- its taps stop at the edge of the BOX, as if the crop had been copied
    out first -- mirror it left-right where `flip[i]`, and return (x / 255 - mean) / std as a device tensor [B, 3, Hout, Wout]
    (`layout="nchw"`) or [B, Hout, Wout, 3], fp32 or bf16.  `images_u8`: [B, H, W, 3] or [B, 3, H, W], one image without the batch
    axis (then `boxes` is one box and the result has no batch axis), or a list of images of different sizes (packed with
    `pack_images`); numpy or torch, host or device.  One launch of `mv_preprocess_u8_boxes_fwd` on the current stream for every
    form: the kernel generates the filter of each box itself, so a fresh random box per image and step costs one 40-byte record.
    The call cannot be recorded by `filter_jit`: the boxes belong to this one call."""
    _refuse_recording("crop_resize_normalize", "boxes, flips and offsets")
    it = _intake(images_u8, channels_last)
    if not it.batched:
        boxes, flip = _rows_of_one(boxes, 4), _rows_of_one(flip, 0)
    _check_output(dtype, layout)
    rec, (hout, wout) = boxes_plan(it.sizes, boxes, flip, size)
    a, b = _affine_on_device(mean, std)
    t, rec_dev = _one_buffer(it.x), _records_to_device(rec)
    B = len(it.sizes)
    y = _new_output(B, hout, wout, dtype, layout)
    _lib.call("mv_preprocess_u8_boxes_fwd", t.data_ptr(), t.numel(), y.data_ptr(), rec.ctypes.data, rec_dev.data_ptr(),
              a.data_ptr(), b.data_ptr(), B, hout, wout, int(it.chw), DT[dtype], int(layout == "nhwc"), stream_ptr())
    return y if it.batched else y[0]


def imagenet_train(images_u8, key, size=224, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), flip_p=0.5, mean=IMAGENET_MEAN,
                   std=IMAGENET_STD, dtype="fp32", channels_last=None) -> torch.Tensor:
    """torchvision's ImageNet training preset on the device: RandomResizedCrop(size, scale, ratio) -> RandomHorizontalFlip(flip_p)
    -> ToTensor -> Normalize, one launch.  `key` is split in two: `random_resized_crop_boxes` draws the boxes from the first
    half, `random_flips` the flips from the second; the same key gives the same tensor.  Returns [B, 3, size, size], fp32 or
    bf16: what `eqv.vmap(net)` reads.  `images_u8`: as for `crop_resize_normalize`."""
    sizes, single = _sizes_of(images_u8, channels_last)
    k_box, k_flip = _random.split(key, 2)
    boxes = random_resized_crop_boxes(k_box, sizes, scale, ratio)
    flips = random_flips(k_flip, len(sizes), flip_p)
    return crop_resize_normalize(images_u8, boxes[0] if single else boxes, size, flips, mean, std, dtype, "nchw", channels_last)


# ---- the rest of the classification recipe: mixup / cutmix, random erasing, soft targets -> mv_preprocess_u8_mix_fwd, one launch ----

# `mv_preprocess_mix` of include/eqxvision_amd.h, 52 bytes
MIX = np.dtype([("partner", "<i4"), ("lam", "<f4"), ("oml", "<f4"), ("cy0", "<i4"), ("cx0", "<i4"), ("cy1", "<i4"), ("cx1", "<i4"),
                ("ey0", "<i4"), ("ex0", "<i4"), ("ey1", "<i4"), ("ex1", "<i4"), ("lam_t", "<f4"), ("oml_t", "<f4")])
ERASE_ATTEMPTS = 10    # torchvision's RandomErasing.get_params tries ten rectangles before it gives up


def mixup_cutmix_draw(key, B, size, mixup_alpha=0.2, cutmix_alpha=1.0, switch_p=0.5):
    """The batch-level draw of torchvision's reference `RandomMixup` / `RandomCutmix` (references/classification/transforms.py, one
    of the two chosen per batch) for B images of output `size` (an int or (H, W)).  Host only.  Returns per-image arrays
    (partner int32 [B], lam fp32 [B], cut_rect int32 [B, 4] of (y0, x0, y1, x1) in output pixels, lam_t fp32 [B]); the draw is
    one per batch, so every row holds the same numbers.  partner[i] = (i - 1) mod B, which is `batch.roll(1, 0)`.
    `key` is split in three.  The first decides the branch: cutmix iff random.uniform01 < switch_p when both alphas are positive;
    an alpha <= 0 disables its branch, both disabled or B == 1 give no mixing (partner[i] = i, lam = lam_t = 1, empty
    rectangle).  The second gives lam ~ Beta(alpha, alpha) from `random.generator`.  Mixup: no rectangle, lam_t = lam.  Cutmix:
    the third key gives the centre, r_x = min(int(u0 W), W - 1), r_y = min(int(u1 H), H - 1) from random.uniform01; with
    r = 0.5 sqrt(1 - lam) the half extents are int(r W), int(r H); the rectangle is clamped to the image,
    lam_t = 1 - area / (H W), and the pixel weight lam is 1: inside the rectangle the partner, outside the image itself.
    This is torchvision's DISTRIBUTION, not torch's random stream: the same seed gives other draws than torchvision does."""
    B = int(B)
    H, W = _pair(size, "size")
    if B < 1:
        raise ValueError(f"preprocess: a batch of {B} images")
    if not 0.0 <= float(switch_p) <= 1.0:
        raise ValueError(f"preprocess: switch_p = {switch_p} must lie in [0, 1]")
    k_choice, k_lam, k_box = _random.split(key, 3)
    mixup, cutmix = float(mixup_alpha) > 0.0, float(cutmix_alpha) > 0.0
    own = np.arange(B, dtype=np.int32)
    if B == 1 or not (mixup or cutmix):
        return own, np.ones(B, np.float32), np.zeros((B, 4), np.int32), np.ones(B, np.float32)
    use_cutmix = cutmix and (not mixup or float(_random.uniform01(k_choice, 1)[0]) < float(switch_p))
    alpha = float(cutmix_alpha if use_cutmix else mixup_alpha)
    lam = float(_random.generator(k_lam).beta(alpha, alpha))
    rect = (0, 0, 0, 0)
    if use_cutmix:
        u = np.asarray(_random.uniform01(k_box, 2), np.float64)
        r_x, r_y = min(int(u[0] * W), W - 1), min(int(u[1] * H), H - 1)
        r = 0.5 * float(np.sqrt(1.0 - lam))
        hw, hh = int(r * W), int(r * H)
        x0, y0, x1, y1 = max(r_x - hw, 0), max(r_y - hh, 0), min(r_x + hw, W), min(r_y + hh, H)
        rect = (y0, x0, y1, x1)
        lam_t, lam = 1.0 - (x1 - x0) * (y1 - y0) / (H * W), 1.0
    else:
        lam_t = lam
    return ((own - 1) % B).astype(np.int32), np.full(B, lam, np.float32), np.tile(np.asarray(rect, np.int32), (B, 1)), \
        np.full(B, lam_t, np.float32)


def random_erasing_draw(key, B, size, p=0.5, scale=(0.02, 0.33), ratio=(0.3, 3.3)) -> np.ndarray:
    """torchvision's `RandomErasing(p, scale, ratio, value=0)` for B images of output `size` (an int or (H, W)): int32 [B, 4] of
    (y0, x0, y1, x1) in output pixels, an empty rectangle (all zeros) where nothing is erased.  Host only.  Image i draws
    u = random.uniform(random.split(key, B)[i], (1 + 10 * 4,)): it is erased iff u[0] < p; attempt t reads u[1 + 4 t : 5 + 4 t] and
    takes area = H W (scale0 + u0 (scale1 - scale0)), aspect = exp(log r0 + u1 (log r1 - log r0)), h = int(round(sqrt(area aspect))),
    w = int(round(sqrt(area / aspect))); the first attempt with h < H and w < W wins and is placed at
    y0 = min(int(u2 (H - h + 1)), H - h), x0 likewise from u3.  If none fits, nothing is erased (`get_params` returns the image).
    This is torchvision's DISTRIBUTION, not torch's random stream: the same seed gives other rectangles than torchvision does."""
    B = int(B)
    H, W = _pair(size, "size")
    s0, s1 = (float(v) for v in scale)
    r0, r1 = (float(v) for v in ratio)
    if not (0.0 < s0 <= s1) or not (0.0 < r0 <= r1):
        raise ValueError(f"preprocess: scale {scale} and ratio {ratio} must be positive (min, max) pairs")
    if B < 1:
        raise ValueError(f"preprocess: a batch of {B} images")
    out = np.zeros((B, 4), np.int32)
    log0, log1 = np.log(np.float64(r0)), np.log(np.float64(r1))
    for i, k in enumerate(_random.split(key, B)):
        u = np.asarray(_random.uniform(k, (1 + ERASE_ATTEMPTS * 4,)), np.float64)
        if not u[0] < p:
            continue
        for t in range(ERASE_ATTEMPTS):
            u0, u1, u2, u3 = u[1 + 4 * t:5 + 4 * t]
            area = H * W * (s0 + u0 * (s1 - s0))
            ar = np.exp(log0 + u1 * (log1 - log0))
            h, w = int(round(float(np.sqrt(area * ar)))), int(round(float(np.sqrt(area / ar))))
            if h < H and w < W:
                y0, x0 = min(int(u2 * (H - h + 1)), H - h), min(int(u3 * (W - w + 1)), W - w)
                out[i] = (y0, x0, y0 + h, x0 + w)
                break
    return out


def _per_image_array(v, B, tail, kind, what, default):
    """`v` as an array [B] + tail of integers (kind "i") or floats ("f"); None -> `default`."""
    if v is None:
        return default
    a = np.asarray(v)
    if a.shape != (B,) + tail or a.dtype.kind not in ("iu" if kind == "i" else "iuf"):
        want = "integers" if kind == "i" else "numbers"
        raise ValueError(f"preprocess: {what} must be {want} {list((B,) + tail)}, one entry per image, got {a.dtype} {tuple(a.shape)}")
    return a.astype(np.int64 if kind == "i" else np.float64)


def mix_plan(B, size, partner=None, lam=None, cut=None, erase=None, lam_t=None):
    """Host half of `crop_resize_normalize_mix`, no device involved: the MIX records [B] of a batch with output `size`.  partner
    int [B] (None: nobody is mixed), lam [B] (None: 1), cut / erase int [B, 4] of (y0, x0, y1, x1) in output pixels, half-open (None
    or y1 <= y0 or x1 <= x0: none), lam_t [B] (None: lam).  oml and oml_t are 1 - lam and 1 - lam_t, taken in float64 from the fp32
    values and rounded once.  Every refusal is a ValueError that names the image."""
    hout, wout = _pair(size, "size")
    pa = _per_image_array(partner, B, (), "i", "partner", np.arange(B, dtype=np.int64))
    la = _per_image_array(lam, B, (), "f", "lam", np.ones(B))
    lt = _per_image_array(lam_t, B, (), "f", "lam_t", la)
    ct = _per_image_array(cut, B, (4,), "i", "cut", np.zeros((B, 4), np.int64))
    er = _per_image_array(erase, B, (4,), "i", "erase", np.zeros((B, 4), np.int64))
    rec = np.zeros(B, MIX)
    for i in range(B):
        who = f"preprocess: image {i}"
        if not 0 <= pa[i] < B:
            raise ValueError(f"{who}: partner {int(pa[i])} does not lie in [0, {B})")
        for name, v in (("lam", la[i]), ("lam_t", lt[i])):
            if not (np.isfinite(v) and 0.0 <= v <= 1.0):
                raise ValueError(f"{who}: {name} = {float(v)} must be finite and lie in [0, 1]")
        for name, (y0, x0, y1, x1) in (("cut", ct[i]), ("erase", er[i])):
            if not (0 <= y0 <= hout and 0 <= y1 <= hout and 0 <= x0 <= wout and 0 <= x1 <= wout):
                raise ValueError(f"{who}: {name} rectangle {(int(y0), int(x0), int(y1), int(x1))} does not lie inside the output "
                                 f"{hout}x{wout}")
        l32, t32 = np.float32(la[i]), np.float32(lt[i])
        rec[i] = (pa[i], l32, np.float32(1.0 - np.float64(l32))) + tuple(ct[i]) + tuple(er[i]) + (t32, np.float32(1.0 - np.float64(t32)))
    return rec


def smoothing_values(label_smoothing, num_classes):
    """(on, off) fp32 of a smoothed one-hot row: on = 1 - eps + eps / K, off = eps / K, computed in float64 and rounded once."""
    eps, K = float(label_smoothing), int(num_classes)
    if K < 1:
        raise ValueError(f"preprocess: num_classes = {num_classes} must be positive")
    if not 0.0 <= eps < 1.0:
        raise ValueError(f"preprocess: label_smoothing = {label_smoothing} must lie in [0, 1)")
    return np.float32(1.0 - eps + eps / K), np.float32(eps / K)


def crop_resize_normalize_mix(images_u8, boxes, size, flip=None, labels=None, num_classes=None, partner=None, lam=None, cut=None,
                              erase=None, lam_t=None, label_smoothing=0.0, mean=IMAGENET_MEAN, std=IMAGENET_STD, dtype="fp32",
                              layout="nchw", channels_last=None):
    """`crop_resize_normalize` with the rest of torchvision's classification recipe in the same launch
    (`mv_preprocess_u8_mix_fwd`).  With v_i the fp32 value `crop_resize_normalize` gives image i before the output is rounded:
    v_i is 0 inside `erase[i]` = (y0, x0, y1, x1) (output pixels, half-open: RandomErasing(value=0), after Normalize); then, with
    r = partner[i], the output is v_r inside `cut[i]`, v_i where r == i or lam[i] == 1, else lam[i] v_i + (1 - lam[i]) v_r as two
    rounded products and one rounded sum.  An image is erased before it is mixed, so its erase rectangle shows in every image it is
    the partner of.  `labels` (int [B], host or a device int32 tensor) and `num_classes` give soft targets fp32 [B, K],
    lam_t[i] s(labels[i]) + (1 - lam_t[i]) s(labels[r]) with s the one-hot row smoothed by `label_smoothing` (`smoothing_values`);
    `lam_t` defaults to `lam`.  Returns (x, targets): x as `crop_resize_normalize` returns it, targets a `DevArray` -- what
    `optim.softmax_cross_entropy(out, targets)` reads -- or None without labels.  Host labels outside [0, K) are refused; device
    labels are checked by the kernel (bit 3 of the device status).  `images_u8`: as for `crop_resize_normalize`; a single image
    has nobody to be mixed with and is refused when `partner` says otherwise.  One launch on the current stream.  The call cannot
    be recorded by `filter_jit`: the boxes and the draws belong to this one call."""
    _refuse_recording("crop_resize_normalize_mix", "boxes, flips, partners and rectangles")
    it = _intake(images_u8, channels_last)
    sizes, batched, chw = it.sizes, it.batched, it.chw
    if not batched:
        if partner is not None and np.any(np.asarray(partner).reshape(-1) != 0):
            raise ValueError("preprocess: a single image has no partner to be mixed with; give a batch, or partner=None")
        boxes, cut, erase = _rows_of_one(boxes, 4), _rows_of_one(cut, 4), _rows_of_one(erase, 4)
        flip, partner, lam, lam_t = _rows_of_one(flip, 0), _rows_of_one(partner, 0), _rows_of_one(lam, 0), _rows_of_one(lam_t, 0)
        if not isinstance(labels, torch.Tensor):
            labels = _rows_of_one(labels, 0)
    _check_output(dtype, layout)
    B = len(sizes)
    rec, (hout, wout) = boxes_plan(sizes, boxes, flip, size)
    mix = mix_plan(B, (hout, wout), partner, lam, cut, erase, lam_t)
    lab_host, lab_dev, K, on, off = None, None, 0, np.float32(1.0), np.float32(0.0)
    if labels is not None:
        if num_classes is None:
            raise ValueError("preprocess: labels need num_classes")
        K = int(num_classes)
        on, off = smoothing_values(label_smoothing, K)
        if _is_device_tensor(labels):
            if labels.dtype != torch.int32 or labels.numel() != B:
                raise ValueError(f"preprocess: device labels must be an int32 tensor [{B}], got {labels.dtype} {tuple(labels.shape)}")
        else:
            lab_host = np.asarray(labels.numpy() if isinstance(labels, torch.Tensor) else labels)
            if lab_host.dtype.kind not in "iu" or lab_host.shape != (B,):
                raise ValueError(f"preprocess: labels must be integers [{B}], one label per image, got {lab_host.dtype} "
                                 f"{tuple(lab_host.shape)}")
            for i, v in enumerate(lab_host):
                if not 0 <= int(v) < K:
                    raise ValueError(f"preprocess: image {i}: label {int(v)} does not lie in [0, {K})")
            lab_host = np.ascontiguousarray(lab_host, np.int32)
    a, b = _affine_on_device(mean, std)
    t, rec_dev, mix_dev = _one_buffer(it.x), _records_to_device(rec), _records_to_device(mix)
    y = _new_output(B, hout, wout, dtype, layout)
    targets = None
    if labels is not None:
        lab_dev = labels.to(device()).contiguous().reshape(B) if lab_host is None else torch.from_numpy(lab_host).to(device())
        targets = empty((B, K), torch.float32)
    _lib.call("mv_preprocess_u8_mix_fwd", t.data_ptr(), t.numel(), y.data_ptr(), rec.ctypes.data, rec_dev.data_ptr(), mix.ctypes.data,
              mix_dev.data_ptr(), a.data_ptr(), b.data_ptr(), None if lab_host is None else lab_host.ctypes.data,
              None if lab_dev is None else lab_dev.data_ptr(), None if targets is None else targets.data_ptr(), K, float(on), float(off),
              B, hout, wout, int(chw), DT[dtype], int(layout == "nhwc"), stream_ptr())
    if batched:
        return y, None if targets is None else DevArray(targets)
    return y[0], None if targets is None else DevArray(targets[0])


def imagenet_train_mixed(images_u8, labels, key, num_classes, size=224, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), flip_p=0.5,
                         mixup_alpha=0.2, cutmix_alpha=1.0, switch_p=0.5, erase_p=0.0, erase_scale=(0.02, 0.33),
                         erase_ratio=(0.3, 3.3), label_smoothing=0.0, mean=IMAGENET_MEAN, std=IMAGENET_STD, dtype="fp32",
                         channels_last=None):
    """torchvision's full classification training recipe on the device, one launch: `imagenet_train`'s RandomResizedCrop ->
    RandomHorizontalFlip -> ToTensor -> Normalize, then RandomErasing(erase_p, value=0) per image, then one of RandomMixup(mixup_alpha)
    / RandomCutmix(cutmix_alpha) on the batch, with label smoothing folded into the soft targets.  `key` is split in FOUR:
    `random_resized_crop_boxes` draws from the first, `random_flips` from the second, `mixup_cutmix_draw` from the third,
    `random_erasing_draw` from the fourth.  The first two are NOT the halves of `imagenet_train`'s two-way split: the same key gives
    other boxes and flips here than there.  The same key gives the same bits.  Returns (x [B, 3, size, size] fp32 or bf16, targets
    `DevArray` fp32 [B, num_classes]), ready for `optim.softmax_cross_entropy(out, targets).mean()`.  `images_u8`: a batch, as for
    `crop_resize_normalize`; `labels`: int [B], host or a device int32 tensor."""
    sizes, single = _sizes_of(images_u8, channels_last)
    if single:
        raise ValueError("preprocess: imagenet_train_mixed mixes the images of a batch; a single image has no partner to be mixed "
                         "with (imagenet_train takes one)")
    B = len(sizes)
    k_box, k_flip, k_mix, k_erase = _random.split(key, 4)
    boxes = random_resized_crop_boxes(k_box, sizes, scale, ratio)
    flips = random_flips(k_flip, B, flip_p)
    partner, lam, cut, lam_t = mixup_cutmix_draw(k_mix, B, size, mixup_alpha, cutmix_alpha, switch_p)
    erase = random_erasing_draw(k_erase, B, size, erase_p, erase_scale, erase_ratio) if erase_p > 0.0 else None
    return crop_resize_normalize_mix(images_u8, boxes, size, flips, labels, num_classes, partner, lam, cut, erase, lam_t,
                                     label_smoothing, mean, std, dtype, "nchw", channels_last)


# ---- segmentation training: resize the whole image, mirror, pad, take a window; image and label map -> mv_preprocess_u8_seg_fwd ----

# `mv_preprocess_seg` of include/eqxvision_amd.h, 48 bytes
SEG = np.dtype([("offset", "<i8"), ("mask_offset", "<i8"), ("Hin", "<i4"), ("Win", "<i4"), ("Hr", "<i4"), ("Wr", "<i4"),
                ("top", "<i4"), ("left", "<i4"), ("flip", "<i4"), ("pad", "<i4")])


def random_resize_sizes(key, sizes, min_size, max_size) -> np.ndarray:
    """torchvision's segmentation `RandomResize(min_size, max_size)` for B images: `sizes` [(H, W)] -> int32 [B, 2] of (Hr, Wr).
    Host only.  Image i draws u = random.uniform(random.split(key, B)[i], ()) and takes
    s = min_size + min(int(u (max_size - min_size + 1)), max_size - min_size), an integer uniform over [min_size, max_size] like
    torch.randint(min_size, max_size + 1), then (Hr, Wr) = resized_size(H, W, s): the shorter side becomes s.
    This is torchvision's DISTRIBUTION, not torch's random stream: the same seed gives other sizes than torchvision does."""
    sizes = [(int(h), int(w)) for h, w in sizes]
    lo, hi = int(min_size), int(max_size)
    if lo < 1 or hi < lo:
        raise ValueError(f"preprocess: min_size {min_size} and max_size {max_size} must satisfy 1 <= min_size <= max_size")
    if len(sizes) == 0:
        raise ValueError("preprocess: no image sizes")
    out = np.zeros((len(sizes), 2), np.int32)
    keys = _random.split(key, len(sizes))
    for i, (H, W) in enumerate(sizes):
        if H < 1 or W < 1:
            raise ValueError(f"preprocess: image {i}: empty image {H}x{W}")
        u = float(_random.uniform(keys[i], ()))
        out[i] = resized_size(H, W, lo + min(int(u * (hi - lo + 1)), hi - lo))
    return out


def random_crop_origins(key, resized, crop) -> np.ndarray:
    """torchvision's `RandomCrop.get_params` on the padded size, for B images: `resized` [(Hr, Wr)], `crop` an int or (Hc, Wc) ->
    int32 [B, 2] of (top, left) in the image padded to max(Hr, Hc) x max(Wr, Wc).  Host only.  Image i draws
    u = random.uniform(random.split(key, B)[i], (2,)): top = min(int(u[0] (max(Hr, Hc) - Hc + 1)), max(Hr, Hc) - Hc), left
    likewise from u[1]; an axis that had to be padded leaves only the origin 0.
    This is torchvision's DISTRIBUTION, not torch's random stream: the same seed gives other origins than torchvision does."""
    hc, wc = _pair(crop, "crop")
    resized = [(int(h), int(w)) for h, w in resized]
    if len(resized) == 0:
        raise ValueError("preprocess: no image sizes")
    out = np.zeros((len(resized), 2), np.int32)
    keys = _random.split(key, len(resized))
    for i, (hr, wr) in enumerate(resized):
        if hr < 1 or wr < 1:
            raise ValueError(f"preprocess: image {i}: empty resized image {hr}x{wr}")
        u = np.asarray(_random.uniform(keys[i], (2,)), np.float64)
        fh, fw = max(hr, hc) - hc, max(wr, wc) - wc
        out[i] = (min(int(u[0] * (fh + 1)), fh), min(int(u[1] * (fw + 1)), fw))
    return out


def seg_plan(sizes, resized, origins, flip, crop):
    """Host half of `resize_pad_crop_pair`, no device involved: `sizes` [(Hin, Win)] of tightly packed images (and, one plane
    each, masks) in order, `resized` [B, 2] of (Hr, Wr), `origins` [B, 2] of (top, left) in the padded image, `flip` None or [B],
    `crop` an int or (Hc, Wc).  Returns (records, (Hc, Wc)), `records` a SEG array [B]; every refusal is a ValueError that names
    the image."""
    B = len(sizes)
    hc, wc = _pair(crop, "crop")
    rs, og = _int_rows(resized, B, 2, "resized", "(Hr, Wr), one size"), _int_rows(origins, B, 2, "origins", "(top, left), one origin")
    fl = _flags(flip, B)
    rec = np.zeros(B, SEG)
    offset = 0
    for i, (hin, win) in enumerate(sizes):
        who = f"preprocess: image {i}"
        (hr, wr), (top, left) = (int(v) for v in rs[i]), (int(v) for v in og[i])
        if hr < 1 or wr < 1:
            raise ValueError(f"{who}: resized size {(hr, wr)} must be positive")
        hp, wp = max(hr, hc), max(wr, wc)
        if top < 0 or left < 0 or top + hc > hp or left + wc > wp:
            raise ValueError(f"{who}: window {hc}x{wc} at ({top}, {left}) does not lie inside the padded image {hp}x{wp}")
        _check_taps(hin, win, hr, wr, who)
        rec[i] = (3 * offset, offset, hin, win, hr, wr, top, left, int(bool(fl[i])), 0)
        offset += hin * win
    return rec, (hc, wc)


def _check_masks(masks, sizes, listed, batched):
    """Masks in the form of the images, without the channel axis and of matching sizes; every refusal names the image."""
    who = "preprocess: masks"
    if listed:
        if not isinstance(masks, (list, tuple)) or len(masks) != len(sizes):
            raise ValueError(f"{who}: a list of {len(sizes)} images needs a list of {len(sizes)} masks")
        planes = list(masks)
    else:
        if not isinstance(masks, (np.ndarray, torch.Tensor)) or masks.ndim != (3 if batched else 2):
            raise ValueError(f"{who}: must be an array {'[B, H, W]' if batched else '[H, W]'} like the images without their channel axis")
        if batched and int(masks.shape[0]) != len(sizes):
            raise ValueError(f"{who}: {int(masks.shape[0])} masks for {len(sizes)} images")
        planes = list(masks) if batched else [masks]
    for i, (m, hw) in enumerate(zip(planes, sizes)):
        if not isinstance(m, (np.ndarray, torch.Tensor)) or m.dtype != (torch.uint8 if isinstance(m, torch.Tensor) else np.uint8):
            raise ValueError(f"preprocess: image {i}: the mask must be a uint8 array of labels, got "
                             f"{getattr(m, 'dtype', type(m).__name__)}")
        if tuple(int(v) for v in m.shape) != tuple(hw):
            raise ValueError(f"preprocess: image {i}: mask of shape {tuple(m.shape)} for an image of {hw[0]}x{hw[1]}")


def resize_pad_crop_pair(images_u8, masks_u8, resized, origins, crop, flip=None, mean=IMAGENET_MEAN, std=IMAGENET_STD, dtype="fp32",
                         layout="nchw", image_fill=0, mask_fill=255, channels_last=None):
    """Resize image i WHOLE to `resized[i]` = (Hr, Wr) with the antialiased triangle filter of `crop_resize_normalize`, mirror it
    left-right where `flip[i]`, pad it on the right and bottom to max(Hr, Hc) x max(Wr, Wc), and keep the `crop` = (Hc, Wc) window
    at `origins[i]` = (top, left) of the padded image.  Returns (x, labels): x = (image / 255 - mean) / std as a device tensor
    [B, 3, Hc, Wc] (`layout="nchw"`) or [B, Hc, Wc, 3], fp32 or bf16, with `image_fill` (a pixel value 0..255, normalised like the
    rest) in the padding; labels int32 [B, Hc, Wc], the mask through the same geometry with the centre-based nearest rule,
    mask[(2 r + 1) Hin // (2 Hr)][(2 c + 1) Win // (2 Wr)] (PIL, torch's "nearest-exact": the half-pixel grid of the image
    filter), and `mask_fill` in the padding -- what `optim.softmax_cross_entropy_with_integer_labels(out, labels, axis=1,
    where=labels != 255)` reads.  `images_u8`: as for `crop_resize_normalize`; `masks_u8`: the same form without the channel
    axis, sizes matching, or None (then labels is None).  One launch of `mv_preprocess_u8_seg_fwd` on the current stream for
    every form; lists are packed with `pack_images`, one upload each.  The call cannot be recorded by `filter_jit`: the sizes and
    origins belong to this one call."""
    _refuse_recording("resize_pad_crop_pair", "sizes, origins, flips and offsets")
    it = _intake(images_u8, channels_last)
    sizes, batched = it.sizes, it.batched
    if not batched:
        resized, origins, flip = _rows_of_one(resized, 2), _rows_of_one(origins, 2), _rows_of_one(flip, 0)
    if masks_u8 is not None:
        _check_masks(masks_u8, sizes, it.listed, batched)
    _check_output(dtype, layout)
    for name, v in (("image_fill", image_fill), ("mask_fill", mask_fill)):
        if not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= 255:
            raise ValueError(f"preprocess: {name} must be an integer in [0, 255], got {v!r}")
    rec, (hc, wc) = seg_plan(sizes, resized, origins, flip, crop)
    a, b = _affine_on_device(mean, std)
    t = _one_buffer(it.x)
    m = None if masks_u8 is None else _one_buffer(masks_u8)
    rec_dev = _records_to_device(rec)
    B = len(sizes)
    y = _new_output(B, hc, wc, dtype, layout)
    labels = None if m is None else empty((B, hc, wc), torch.int32)
    _lib.call("mv_preprocess_u8_seg_fwd", t.data_ptr(), t.numel(), None if m is None else m.data_ptr(), 0 if m is None else m.numel(),
              y.data_ptr(), None if m is None else labels.data_ptr(), rec.ctypes.data, rec_dev.data_ptr(), a.data_ptr(), b.data_ptr(),
              B, hc, wc, int(image_fill), int(mask_fill), int(it.chw), DT[dtype], int(layout == "nhwc"), stream_ptr())
    if batched:
        return y, labels
    return y[0], None if labels is None else labels[0]


def _sizes_of(images_u8, channels_last):
    """-> ([(Hin, Win)] per image, single): the sizes of any accepted form of input."""
    it = _intake(images_u8, channels_last)
    return it.sizes, not it.batched


def segmentation_train(images_u8, masks_u8, key, base_size=520, crop_size=480, flip_p=0.5, mean=IMAGENET_MEAN, std=IMAGENET_STD,
                       dtype="fp32", image_fill=0, mask_fill=255, channels_last=None):
    """torchvision's segmentation training preset on the device: RandomResize(int(0.5 base_size), int(2 base_size)) -- image
    antialiased bilinear, mask nearest -- -> RandomHorizontalFlip(flip_p) -> RandomCrop(crop_size) with pad-if-smaller on the
    right and bottom (image 0, mask 255) -> ToTensor -> Normalize, image and label map in one launch.  `key` is split in three:
    `random_resize_sizes` draws from the first, `random_flips` from the second, `random_crop_origins` from the third; the same
    key gives the same bits.  Returns (x [B, 3, crop, crop] fp32 or bf16, labels int32 [B, crop, crop]).  `images_u8`,
    `masks_u8`: as for `resize_pad_crop_pair`."""
    sizes, single = _sizes_of(images_u8, channels_last)
    k_size, k_flip, k_origin = _random.split(key, 3)
    resized = random_resize_sizes(k_size, sizes, int(0.5 * base_size), int(2.0 * base_size))
    flips = random_flips(k_flip, len(sizes), flip_p)
    origins = random_crop_origins(k_origin, resized, crop_size)
    return resize_pad_crop_pair(images_u8, masks_u8, resized[0] if single else resized, origins[0] if single else origins, crop_size,
                                flips, mean, std, dtype, "nchw", image_fill, mask_fill, channels_last)


def segmentation_eval(images_u8, masks_u8=None, base_size=520, mean=IMAGENET_MEAN, std=IMAGENET_STD, dtype="fp32",
                      channels_last=None):
    """torchvision's segmentation evaluation preset on the device: the shorter side to `base_size` (image antialiased bilinear,
    mask nearest), no flip, no crop, ToTensor, Normalize; the core with crop = resized size and origin (0, 0).  Returns
    (x [B, 3, Hr, Wr], labels int32 [B, Hr, Wr] or None).  Images of different sizes give outputs of different sizes and are
    refused: evaluate them one by one."""
    sizes, single = _sizes_of(images_u8, channels_last)
    resized = [resized_size(h, w, base_size) for h, w in sizes]
    for i, hw in enumerate(resized):
        if hw != resized[0]:
            raise ValueError(f"preprocess: image {i}: segmentation_eval resizes it to {hw[0]}x{hw[1]} and image 0 to "
                             f"{resized[0][0]}x{resized[0][1]}; the outputs of one call share a size, evaluate such images one by one")
    rs, og = np.asarray(resized, np.int32), np.zeros((len(sizes), 2), np.int32)
    return resize_pad_crop_pair(images_u8, masks_u8, rs[0] if single else rs, og[0] if single else og, resized[0], None, mean, std,
                                dtype, "nchw", 0, 255, channels_last)
