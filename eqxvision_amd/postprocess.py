"""The back end of inference on the device: label maps for the segmentation models, top-k for the classifiers.

    labels = eqv.postprocess.segment(net, images)                 # uint8 [B, H, W], instead of argmax(vmap(net)(images)[1], 1)
    p, idx = eqv.postprocess.topk(eqv.vmap(net)(x), k=5)           # fp32 [B, 5] probabilities, int32 [B, 5] classes

A segmentation model ends in a bilinear resize of its [B, h, w, classes] logits to the input resolution, written as fp32
[B, classes, H, W]; the label map every inference caller takes from it is one byte per pixel.  `upsample_argmax` interpolates and
selects in registers (csrc/resize.hip: the same taps and the same interpolation expression as the resize kernel, so the labels
ARE the argmax of what that kernel would have written) and stores only the labels.  `topk` is softmax + top-k of a logit matrix
in one launch (csrc/postprocess.hip).  Ties go to the lower class in both, as in `jnp.argmax` and `jax.lax.top_k`.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, ops
from . import random as jr
from ._act import _tls as _act_tls
from ._act import device, empty, stream_ptr, wrap

MAX_CLASSES = 256      # a label is one byte
MAX_K = 16             # MV_TOPK_MAX_K of include/eqxvision_amd.h
MAX_ROW = 65536


def _check_array(x, who, dtypes):
    if not isinstance(x, (np.ndarray, torch.Tensor)):
        raise ValueError(f"{who}: expected a numpy array or torch tensor, got {type(x).__name__}")
    names = {torch.float32: "float32", torch.bfloat16: "bfloat16"}
    ok = [d for d in dtypes] if isinstance(x, torch.Tensor) else [np.float32]
    if x.dtype not in ok:
        raise ValueError(f"{who}: dtype must be {' or '.join(names[d] for d in dtypes)}, got {x.dtype}")
    return x


def _check_logits(logits, size, channels_last, who="postprocess.upsample_argmax"):
    """-> (batched, h, w, C, H, W); raises ValueError before anything touches the device."""
    x = _check_array(logits, who, (torch.float32, torch.bfloat16))
    if x.ndim not in (3, 4):
        raise ValueError(f"{who}: logits must be [h, w, C] / [C, h, w] or a batch of them, got shape {tuple(x.shape)}")
    s = tuple(int(v) for v in x.shape[-3:])
    h, w, C = s if channels_last else (s[1], s[2], s[0])
    try:
        H, W = (int(v) for v in size)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: size must be (H, W), got {size!r}") from None
    if min(h, w, C) < 1 or (x.ndim == 4 and x.shape[0] < 1):
        raise ValueError(f"{who}: empty logits, shape {tuple(x.shape)}")
    if C > MAX_CLASSES:
        raise ValueError(f"{who}: {C} classes do not fit a uint8 label (at most {MAX_CLASSES})")
    if H < h or W < w:
        raise ValueError(f"{who}: {h}x{w} -> {H}x{W} is down-sampling; only up-sampling is supported")
    return x.ndim == 4, h, w, C, H, W


def _to_device(x):
    """The array as a contiguous device tensor; an upload made inside a recording stays alive with it (the replayed launch reads it)."""
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    t = t.to(device(), non_blocking=True).contiguous()
    keep = getattr(_act_tls, "keep", None)
    if keep is not None and t is not x:
        keep.append(t)
    return t


def _labels(t: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """t: NHWC logits on the device -> uint8 [B, H, W], one launch."""
    B, h, w, C = (int(v) for v in t.shape)
    y = empty((B, H, W), torch.uint8)
    _lib.call("mv_resize_argmax_nhwc_fwd", t.data_ptr(), y.data_ptr(), B, h, w, C, H, W,
              _lib.BF16 if t.dtype == torch.bfloat16 else _lib.F32, stream_ptr())
    return y


def upsample_argmax(logits, size, channels_last=True) -> torch.Tensor:
    """argmax over the classes of `logits` resized bilinearly (half-pixel centres, `jax.image.resize`) to `size` = (H, W), as a
    uint8 device tensor [B, H, W] ([H, W] for one sample).  `logits`: [B, h, w, C] -- the layout the dense heads produce -- or,
    with `channels_last=False`, [B, C, h, w] (one layout launch more); fp32 or bf16, numpy or torch, host or device; C <= 256,
    H >= h, W >= w.  One launch on the current stream; recorded by `filter_jit` like any other."""
    batched, h, w, C, H, W = _check_logits(logits, size, channels_last)
    t = _to_device(logits)
    if not batched:
        t = t.unsqueeze(0)
    if not channels_last:
        n = empty((t.shape[0], h, w, C), t.dtype)
        dt = _lib.BF16 if t.dtype == torch.bfloat16 else _lib.F32
        _lib.call("mv_nchw_to_nhwc", t.data_ptr(), n.data_ptr(), int(t.shape[0]), C, h, w, dt, dt, stream_ptr())
        t = n
    y = _labels(t, H, W)
    return y if batched else y[0]


def _head_logits(net, images, key, who):
    """What `segment` and `metrics.evaluate_segmentation` share: the checks, then backbone and classifier exactly as in the model's
    own forward, the auxiliary head skipped.  -> (NHWC logits of the head on the device, H, W of the images)."""
    from .models.segmentation._utils import _SimpleSegmentationModel
    from .models.segmentation.lraspp import LRASPP
    from .transforms import _train_layers
    if not isinstance(net, (_SimpleSegmentationModel, LRASPP)):
        raise ValueError(f"{who}: net must be a segmentation model (fcn, deeplabv3, lraspp_mobilenet_v3_large), got "
                         f"{type(net).__name__}")
    bns, stochastic = _train_layers(net)
    if bns or stochastic:
        raise ValueError(f"{who}: the model is in training mode; label maps are an inference result "
                         "(use tree_inference(net, True))")
    x = _check_array(images, who, (torch.float32, torch.bfloat16))
    if x.ndim != 4 or x.shape[1] != 3 or min(int(v) for v in x.shape) < 1:
        raise ValueError(f"{who}: images must be [B, 3, H, W], got shape {tuple(x.shape)}")
    a = wrap(x, batched=True)
    H, W = (int(v) for v in a.shape[-2:])
    if isinstance(net, LRASPP):                  # its forward takes no key (lraspp.py), and its head reads both feature maps
        _, feats = net.backbone(a)
        logits = net.classifier(feats)
    else:                                        # _SimpleSegmentationModel._forward without the auxiliary head
        k_backbone, k_clf, _ = jr.split(jr.PRNGKey(0) if key is None else key, 3)
        _, feats = net.backbone(a, key=k_backbone)
        logits = net.classifier(feats[-1], key=k_clf)
    return ops.as_map(logits).t, H, W


def segment(net, images, *, key=None) -> torch.Tensor:
    """The label map of a segmentation model: argmax over the classes of what `vmap(net)(images, key=...)[1]` returns, uint8
    [B, H, W], without that tensor ever being written.  Backbone and classifier run exactly as in the model's own forward; the
    auxiliary head, whose result inference discards, is skipped; the final resize is `upsample_argmax`.  `net`: fcn / deeplabv3 /
    lraspp_mobilenet_v3_large in inference mode; `images`: [B, 3, H, W], fp32 or bf16; `key`: as for the model (None, one key, or
    [B, 2] keys -- dead values in inference)."""
    return _labels(*_head_logits(net, images, key, "postprocess.segment"))


def topk(logits, k: int = 5, probabilities: bool = True):
    """The k largest entries of every row of `logits` [B, K] (or [K]): (values fp32 [B, k], indices int32 [B, k]) on the device,
    sorted by value descending, equal values by ascending index (`jax.lax.top_k`).  `probabilities`: values are softmax
    probabilities (fp32 `exp`, sum over the whole row); otherwise the selected logits, bit for bit.  fp32 logits, numpy or torch,
    host or device -- the result of `vmap(net)(x)` as it is; K <= 65536, k <= min(K, 16).  One launch on the current stream."""
    x = _check_array(logits, "postprocess.topk", (torch.float32,))
    if x.ndim not in (1, 2):
        raise ValueError(f"postprocess.topk: logits must be [B, K] or [K], got shape {tuple(x.shape)}")
    try:
        k = int(k)
    except (TypeError, ValueError):
        raise ValueError(f"postprocess.topk: k must be an integer, got {k!r}") from None
    K = int(x.shape[-1])
    if K < 1 or K > MAX_ROW or (x.ndim == 2 and x.shape[0] < 1):
        raise ValueError(f"postprocess.topk: rows must have 1 .. {MAX_ROW} entries and there must be a row, got shape {tuple(x.shape)}")
    if k < 1 or k > K:
        raise ValueError(f"postprocess.topk: k={k} must be in 1 .. K={K}")
    if k > MAX_K:
        raise ValueError(f"postprocess.topk: k={k} is more than the {MAX_K} the selection kernel keeps")
    t = _to_device(logits)
    B = int(t.shape[0]) if t.dim() == 2 else 1
    values, indices = empty((B, k), torch.float32), empty((B, k), torch.int32)
    _lib.call("mv_softmax_topk_f32", t.data_ptr(), values.data_ptr(), indices.data_ptr(), B, K, k, int(bool(probabilities)),
              stream_ptr())
    return (values, indices) if t.dim() == 2 else (values[0], indices[0])
