"""Scoring on the device: the confusion matrix / mIoU of the segmentation models and top-k accuracy of the classifiers.

    cm = eqv.metrics.ConfusionMatrix(num_classes=21)
    for images, labels in validation:                              # preprocess.segmentation_eval: labels with 255 in the padding
        eqv.metrics.evaluate_segmentation(net, images, labels, cm)  # backbone, head, label map and counting: nothing is fetched
    cm.reduce_over_ranks()
    print(cm.compute()["mean_iou"])                                 # the one fetch: C x C integers

    acc = eqv.metrics.TopK(ks=(1, 5))
    acc.update(eqv.vmap(net)(x), labels); acc.compute()            # {"top1": ..., "top5": ..., "count": n}

`update_logits` is two launches: the label kernel of `postprocess.upsample_argmax`, then the counting kernel on its uint8 map.  The
one-launch form exists (`update_logits_fused`, csrc/resize.hip: the body of the label kernel feeding the counting stage, neither
logits nor labels at full resolution written) and counts the same, but measured 2.4 % slower at fcn, batch 32, 520 px (DESIGN.md
section 3.15), so it is not on the path.  Counters are int64 on the device and exact; every update ADDS, on the current stream,
and is recorded by `filter_jit` like any other launch (a replay adds again).  Inside `filter_jit` pass labels as uint8: it stages
other integer arrays as floats, which the checks here refuse.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from . import postprocess as P
from ._act import device, stream_ptr
from .postprocess import MAX_CLASSES, MAX_ROW, _to_device

MAX_KS = 8             # MV_TOPK_MAX_KS of include/eqxvision_amd.h


def _check_label_map(x, who, name):
    if not isinstance(x, (np.ndarray, torch.Tensor)):
        raise ValueError(f"{who}: {name}: expected a numpy array or torch tensor, got {type(x).__name__}")
    ok = (torch.uint8, torch.int32) if isinstance(x, torch.Tensor) else (np.uint8, np.int32)
    if x.dtype not in ok:
        raise ValueError(f"{who}: {name}: dtype must be uint8 or int32, got {x.dtype}")
    return x


def _bytes(t: torch.Tensor) -> int:
    return 1 if t.dtype == torch.uint8 else 4


def metrics_from_matrix(mat) -> dict:
    """The metrics of an integer confusion matrix (rows = target, columns = prediction), float64 on the host:
    pixel_accuracy = trace / sum, class_accuracy = diag / row sums, iou = diag / (row + column - diag).  A class with an empty
    denominator gives NaN.  mean_iou is the mean over the classes whose union is non-zero (NaN if there is none): torchvision's
    reference prints `iu.mean()`, which is NaN as soon as one class is absent from both maps."""
    m = np.asarray(mat).astype(np.int64)
    diag, rows, cols, total = np.diag(m), m.sum(1), m.sum(0), int(m.sum())
    union = rows + cols - diag
    with np.errstate(divide="ignore", invalid="ignore"):
        acc = diag.astype(np.float64) / rows.astype(np.float64)
        iou = diag.astype(np.float64) / union.astype(np.float64)
        pixel = np.float64(int(diag.sum())) / np.float64(total)
    seen = union > 0
    return {"pixel_accuracy": float(pixel), "class_accuracy": acc, "iou": iou,
            "mean_iou": float(iou[seen].mean()) if seen.any() else float("nan")}


def _reduce(t: torch.Tensor):
    from . import dist
    dist.all_reduce_sum_int64_(t)


class ConfusionMatrix:
    """int64 [C, C] counters on the device, rows = target, columns = prediction, C <= 256.  A pixel counts iff 0 <= label < C
    (the rule of torchvision's reference segmentation ConfusionMatrix): 255, any other value >= C and negative int32 labels do
    not.  `mat` is the device tensor itself."""

    def __init__(self, num_classes: int, *, device=None):
        try:
            C = int(num_classes)
        except (TypeError, ValueError):
            raise ValueError(f"metrics.ConfusionMatrix: num_classes must be an integer, got {num_classes!r}") from None
        if C < 1 or C > MAX_CLASSES:
            raise ValueError(f"metrics.ConfusionMatrix: num_classes={C} must be in 1 .. {MAX_CLASSES}")
        self.num_classes = C
        self._device = device          # None: the current HIP device, asked for when the counters are first needed
        self._mat = None

    @property
    def mat(self) -> torch.Tensor:
        if self._mat is None:
            self._mat = torch.zeros((self.num_classes, self.num_classes), dtype=torch.int64,
                                    device=device() if self._device is None else self._device)
        return self._mat

    def reset(self):
        self.mat.zero_()

    def _check_pair(self, who, a_shape, labels):
        if tuple(labels.shape) != tuple(a_shape):
            raise ValueError(f"{who}: labels have shape {tuple(labels.shape)}, expected {tuple(a_shape)}")

    def update_logits(self, logits, labels):
        """Counts argmax over the classes of `logits` resized bilinearly to the labels' resolution (`postprocess.upsample_argmax`
        of the same logits) against `labels`.  logits [B, h, w, C] (or [h, w, C]) fp32 / bf16, the layout the dense heads
        produce; labels [B, H, W] (or [H, W]) uint8 or int32; numpy or torch, host or device; H >= h, W >= w, C == num_classes.
        Two launches (label map, then counting): the faster of the two forms measured, see the module docstring."""
        self._from_logits(logits, labels, False, "metrics.ConfusionMatrix.update_logits")

    def update_logits_fused(self, logits, labels):
        """`update_logits` as ONE launch (mv_confusion_from_logits): interpolation, argmax and counting in registers, no label
        map.  The same counts; kept for measurement (tools/time_metrics.py), not the default."""
        self._from_logits(logits, labels, True, "metrics.ConfusionMatrix.update_logits_fused")

    def _from_logits(self, logits, labels, fused, who):
        lab = _check_label_map(labels, who, "labels")
        if lab.ndim not in (2, 3):
            raise ValueError(f"{who}: labels must be [B, H, W] or [H, W], got shape {tuple(lab.shape)}")
        batched, h, w, C, H, W = P._check_logits(logits, tuple(lab.shape[-2:]), True, who)
        if C != self.num_classes:
            raise ValueError(f"{who}: logits have {C} classes, the matrix {self.num_classes}")
        if batched != (lab.ndim == 3):
            raise ValueError(f"{who}: logits {tuple(logits.shape)} and labels {tuple(lab.shape)}: one is batched, the other is not")
        B = int(logits.shape[0]) if batched else 1
        self._check_pair(who, ((B, H, W) if batched else (H, W)), lab)
        t = _to_device(logits)
        self._launch_logits(t if batched else t.unsqueeze(0), _to_device(lab), B, h, w, H, W, fused)

    def _launch_logits(self, t, lab, B, h, w, H, W, fused):
        if not fused:
            self._launch_labels(P._labels(t, H, W), lab)
            return
        _lib.call("mv_confusion_from_logits", t.data_ptr(), lab.data_ptr(), self.mat.data_ptr(), B, h, w, self.num_classes, H, W,
                  _lib.BF16 if t.dtype == torch.bfloat16 else _lib.F32, _bytes(lab), stream_ptr())

    def update(self, pred, labels):
        """Counts two label maps of one shape against each other, uint8 or int32 each, numpy or torch, host or device.  One
        launch.  A pixel whose prediction is outside [0, C) has no cell in the matrix and is not counted."""
        who = "metrics.ConfusionMatrix.update"
        p, lab = _check_label_map(pred, who, "pred"), _check_label_map(labels, who, "labels")
        if p.ndim < 1 or min((int(v) for v in p.shape), default=0) < 1:
            raise ValueError(f"{who}: empty prediction, shape {tuple(p.shape)}")
        self._check_pair(who, p.shape, lab)
        self._launch_labels(_to_device(p), _to_device(lab))

    def _launch_labels(self, p, lab):
        _lib.call("mv_confusion_from_labels", p.data_ptr(), lab.data_ptr(), self.mat.data_ptr(), p.numel(), self.num_classes,
                  _bytes(p), _bytes(lab), stream_ptr())

    def reduce_over_ranks(self):
        """The exact sum of the matrices of the data-parallel ranks, on every rank (`dist.all_reduce_sum_int64_`: integers all the
        way, never the fp32 all-reduce).  A single process: nothing happens."""
        _reduce(self.mat)

    def compute(self) -> dict:
        """One fetch of the matrix -> {"pixel_accuracy", "class_accuracy" [C], "iou" [C], "mean_iou"}, float64 on the host:
        `metrics_from_matrix`.  mean_iou averages the classes whose union is non-zero."""
        return metrics_from_matrix(self.mat.cpu().numpy())


def evaluate_segmentation(net, images, labels, cm: ConfusionMatrix, *, key=None):
    """`cm.update_logits` on the head of a segmentation model: the model runs as in `postprocess.segment` (same checks, same
    refusals: inference mode, fcn / deeplabv3 / lraspp_mobilenet_v3_large), then the two launches of `update_logits`.  Equal to
    `cm.update(postprocess.segment(net, images), labels)`.  labels: [B, H, W] of the images' size."""
    who = "metrics.evaluate_segmentation"
    if not isinstance(cm, ConfusionMatrix):
        raise ValueError(f"{who}: cm must be a metrics.ConfusionMatrix, got {type(cm).__name__}")
    lab = _check_label_map(labels, who, "labels")
    if lab.ndim != 3:
        raise ValueError(f"{who}: labels must be [B, H, W], got shape {tuple(lab.shape)}")
    t, H, W = P._head_logits(net, images, key, who)
    B, h, w, C = (int(v) for v in t.shape)
    if C != cm.num_classes:
        raise ValueError(f"{who}: the model has {C} classes, the matrix {cm.num_classes}")
    cm._check_pair(who, (B, H, W), lab)
    cm._launch_logits(t, _to_device(lab), B, h, w, H, W, False)


class TopK:
    """Top-k accuracy counters: int64 [len(ks) + 1] on the device (correct at each k, then the number of rows).  A row with
    label l is correct at k iff rank < k, rank = #{j : x[j] > x[l] or (x[j] == x[l] and j < l)} -- the tie rule of
    `jax.lax.top_k` that `postprocess.topk` documents, so for rows without NaN this is "l is among topk(x, k)'s indices".  A row
    whose label is outside [0, K) or whose logit at the label is NaN is wrong for every k and still counted.  Any k >= 1
    (nothing is selected, `postprocess.MAX_K` does not apply); at most 8 values of k."""

    def __init__(self, ks=(1, 5), *, device=None):
        try:
            self.ks = tuple(int(k) for k in ks)
        except (TypeError, ValueError):
            raise ValueError(f"metrics.TopK: ks must be integers, got {ks!r}") from None
        if not 1 <= len(self.ks) <= MAX_KS or min(self.ks) < 1:
            raise ValueError(f"metrics.TopK: ks={self.ks} must be 1 .. {MAX_KS} values, each at least 1")
        self._ks = (ctypes.c_int * len(self.ks))(*self.ks)      # read by the entry during the call (and by every replay)
        self._device = device
        self._counts = None

    @property
    def counts(self) -> torch.Tensor:
        if self._counts is None:
            self._counts = torch.zeros((len(self.ks) + 1,), dtype=torch.int64, device=device() if self._device is None else self._device)
        return self._counts

    def reset(self):
        self.counts.zero_()

    def update(self, logits, labels):
        """logits [B, K] fp32 -- `vmap(net)(x)` as it is -- and labels [B] int32, numpy or torch, host or device; K <= 65536.
        One launch."""
        who = "metrics.TopK.update"
        x = P._check_array(logits, who, (torch.float32,))
        if x.ndim != 2:
            raise ValueError(f"{who}: logits must be [B, K], got shape {tuple(x.shape)}")
        B, K = int(x.shape[0]), int(x.shape[1])
        if B < 1 or K < 1 or K > MAX_ROW:
            raise ValueError(f"{who}: rows must have 1 .. {MAX_ROW} entries and there must be a row, got shape {tuple(x.shape)}")
        if not isinstance(labels, (np.ndarray, torch.Tensor)):
            raise ValueError(f"{who}: labels: expected a numpy array or torch tensor, got {type(labels).__name__}")
        if labels.dtype != (torch.int32 if isinstance(labels, torch.Tensor) else np.int32):
            raise ValueError(f"{who}: labels: dtype must be int32, got {labels.dtype}")
        if tuple(labels.shape) != (B,):
            raise ValueError(f"{who}: labels have shape {tuple(labels.shape)}, expected {(B,)}")
        t, lab = _to_device(logits), _to_device(labels)
        _lib.call("mv_topk_correct_f32", t.data_ptr(), lab.data_ptr(), self.counts.data_ptr(), B, K, self._ks, len(self.ks),
                  stream_ptr())

    def reduce_over_ranks(self):
        """The exact sum of the counters of the data-parallel ranks, as for `ConfusionMatrix`."""
        _reduce(self.counts)

    def compute(self) -> dict:
        """One fetch -> {"top<k>": correct / count for every k, "count": rows seen}; NaN accuracies before the first row."""
        c = self.counts.cpu().numpy()
        n = int(c[-1])
        out = {f"top{k}": (int(v) / n if n else float("nan")) for k, v in zip(self.ks, c[:-1])}
        out["count"] = n
        return out
