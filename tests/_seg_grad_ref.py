"""Reference side of the segmentation training tests (tests/test_seg_grad_host.py, tests/test_seg_grad_gpu.py): torch.autograd on the
CPU in fp32, the yardstick of tests/_grad_cases.py.

oracle/torch_ref.py: segmentation_forward / lraspp_forward run under `torch.no_grad()`, so they are restated here without it, on the
same un-decorated pieces (`_resnet_stages`, `_fcn_head_t`, `_deeplab_head_t`, `_mbv3_features_t`), with `F.interpolate(mode="bilinear",
align_corners=False)` and `F.cross_entropy`.  The host file pins these forwards to oracle/models.py and `resize` to
oracle/np_ops.resize_bilinear.  Also here: the float64 tap tables of the bilinear up-sampling, from which the kernel tests derive
their per-element bounds, and a copy of grad_parity_case's criterion."""
from __future__ import annotations

import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import state as S
from oracle import torch_grad as TG
from oracle import torch_ref as TR

U = 2.0 ** -24                                     # unit round-off of fp32

# (B, h, w, C) -> (H, W) of the kernel tests: exact (dyadic ratios 8, 2, a one-row source, identity) and general ratios
RESIZE_EXACT = (((2, 3, 5, 7), (24, 40)), ((1, 4, 4, 21), (8, 8)), ((2, 1, 2, 5), (8, 16)), ((1, 6, 6, 3), (6, 6)))
RESIZE_GENERAL = (((2, 4, 3, 21), (10, 7)), ((1, 5, 7, 70), (13, 9)))

B, SIZE, CLASSES, AUX_WEIGHT = 2, 64, 5, 0.4
LAYERS = (1, 1, 1, 1)
# name -> (model, has an auxiliary head, uses `where`)
CASES = {"fcn_aux": ("fcn", True, False), "fcn_no_aux_where_void255": ("fcn", False, True), "deeplabv3_aux": ("deeplabv3", True, False),
         "lraspp": ("lraspp", False, False)}


def resize(x: torch.Tensor, size) -> torch.Tensor:
    return F.interpolate(x, size=tuple(size), mode="bilinear", align_corners=False)


def segmentation_forward(t, x, kind, layers=LAYERS, aux=True):
    size = x.shape[-2:]
    feats = TR._resnet_stages(t, x, "bottleneck", layers, dilate=(False, True, True), prefix="backbone.")
    head = TR._fcn_head_t if kind == "fcn" else TR._deeplab_head_t
    out = resize(head(t, feats[3], "classifier"), size)
    return (resize(TR._fcn_head_t(t, feats[2], "aux_classifier"), size) if aux else None), out


def lraspp_forward(t, x, conf, taps=(4, 16)):
    size = x.shape[-2:]
    _, (low, high) = TR._mbv3_features_t(t, x, conf, taps, prefix="backbone.")
    y = F.relu(TR._bn(t, F.conv2d(high, t["classifier.cbr.0.weight"]), "classifier.cbr.1"))
    s = torch.sigmoid(F.conv2d(F.adaptive_avg_pool2d(high, 1), t["classifier.scale.1.weight"]))
    y = resize(y * s, low.shape[-2:])
    out = F.conv2d(low, t["classifier.low_classifier.weight"], t["classifier.low_classifier.bias"]) + \
        F.conv2d(y, t["classifier.high_classifier.weight"], t["classifier.high_classifier.bias"])
    return None, resize(out, size)


def pixel_losses(logits: torch.Tensor, labels, where=None) -> torch.Tensor:
    """optax.softmax_cross_entropy_with_integer_labels(axis=1, where=...): per pixel, 0 where masked (whatever the label there)."""
    lab = torch.as_tensor(np.asarray(labels), dtype=torch.long)
    if where is None:
        return F.cross_entropy(logits, lab, reduction="none")
    m = torch.as_tensor(np.asarray(where), dtype=torch.bool)
    return F.cross_entropy(logits, torch.where(m, lab, torch.zeros_like(lab)), reduction="none") * m.to(logits.dtype)


def lraspp_conf():
    return S.mobilenet_v3_conf("large", dilated=True)[0]


def case_state(name):
    model, aux, _ = CASES[name]
    if model == "lraspp":
        return S.lraspp_state(1, lraspp_conf(), (4, 16), CLASSES)
    return S.segmentation_state(1, model, LAYERS, CLASSES, aux)


def case_inputs(name):
    """(images, labels [B, H, W] int64, where [B, H, W] bool or None); masked pixels carry the void label 255."""
    _, _, use_where = CASES[name]
    rng = np.random.Generator(np.random.PCG64(7))
    x = S.synthetic_images(B, SIZE, seed=11)
    labels = rng.integers(0, CLASSES, (B, SIZE, SIZE))
    where = None
    if use_where:
        where = rng.random((B, SIZE, SIZE)) >= 0.25
        labels = np.where(where, labels, 255)
    return x, labels, where


def forward(name, t, x):
    model, aux, _ = CASES[name]
    if model == "lraspp":
        return lraspp_forward(t, x, lraspp_conf())
    return segmentation_forward(t, x, model, LAYERS, aux)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(loss, {state-dict name: gradient}) of mean(xent(out)) + 0.4 mean(xent(aux)) in inference mode; computed once, shared."""
    sd = case_state(name)
    x, labels, where = case_inputs(name)
    P = TG._params(sd)
    aux, out = forward(name, TR._t(P), torch.from_numpy(x))
    loss = pixel_losses(out, labels, where).mean()
    if aux is not None:
        loss = loss + AUX_WEIGHT * pixel_losses(aux, labels, where).mean()
    loss.backward()
    return float(loss.detach()), {k: v.grad.numpy() for k, v in P.items() if v.requires_grad and v.grad is not None}


def compare(got_l, ref_l, ref, loss, ref_loss, lim=1e-3):
    """tests/_grad_cases.py: grad_parity_case's criterion, copied: every tensor within `lim` of its own max |.|, or the ReLU-flip
    allowance (relative L2 <= 1e-4, none beyond 10 x lim, at most 3 % of the tensors beyond lim); the loss within 1e-4 relative."""
    if len(got_l) != len(ref_l):
        return {"ok": False, "err": f"{len(got_l)} gradient leaves vs {len(ref_l)} parameters"}
    errs = []
    for (gn, a), name in zip(got_l, ref_l):
        a = np.asarray(a, np.float64).reshape(-1)
        b = np.asarray(ref[name], np.float64).reshape(-1)
        if a.shape != b.shape:
            return {"ok": False, "err": f"{name} / {gn}: shape {a.shape} vs {b.shape}"}
        if not np.isfinite(a).all():
            return {"ok": False, "err": f"{name}: non-finite gradient"}
        errs.append((float(np.abs(a - b).max() / max(1e-12, np.abs(b).max())), name))
    errs.sort(reverse=True)
    worst, worst_name = errs[0]
    ga = np.concatenate([np.asarray(a, np.float64).reshape(-1) for _, a in got_l])
    gb = np.concatenate([np.asarray(ref[n], np.float64).reshape(-1) for n in ref_l])
    l2 = float(np.linalg.norm(ga - gb) / max(1e-30, np.linalg.norm(gb)))
    over = [n for e, n in errs if e > lim]
    strict = worst <= lim and l2 <= lim
    flips = l2 <= 1e-4 and worst <= 10 * lim and len(over) <= max(1, int(0.03 * len(errs)))
    return {"ok": bool((strict or flips) and abs(loss - ref_loss) <= 1e-4 * max(1.0, abs(ref_loss))), "err": worst, "rel_l2": l2,
            "strict": bool(strict), "over_lim": over, "worst": worst_name, "loss": loss, "ref_loss": ref_loss, "top": errs[:4]}


# ------------------------------------------------------------------------------------------------ tap tables (float64)
def taps(n_in: int, n_out: int):
    """Index arithmetic of the 2-tap up-sampling on one axis (half-pixel centres, edge clamp): (i0, i1, w0, w1) per output."""
    src = np.maximum((np.arange(n_out) + 0.5) * (n_in / n_out) - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    w1 = src - i0
    return i0, i1, 1.0 - w1, w1


def tap_matrix(n_in: int, n_out: int, count: bool = False, extra: float = 0.0) -> np.ndarray:
    """[n_out, n_in]: the weights (or, with `count`, the number of non-zero taps: a clamped output has two on the edge pixel);
    `extra` is added to every tap's weight (an allowance for the rounding of the fp32 source coordinate)."""
    i0, i1, w0, w1 = taps(n_in, n_out)
    M = np.zeros((n_out, n_in))
    o = np.arange(n_out)
    if count:
        np.add.at(M, (o, i0), (w0 != 0).astype(np.float64))
        np.add.at(M, (o, i1), (w1 != 0).astype(np.float64))
    else:
        np.add.at(M, (o, i0), w0 + extra)
        np.add.at(M, (o, i1), w1 + extra)
    return M


def resize_bwd_bound(dy_nchw: np.ndarray, h: int, w: int) -> np.ndarray:
    """Per element of dx [B, C, h, w]: (n + 2) 2^-24 sum_i |w_i dy_i|, n = the number of products w_i dy_i that reach the element."""
    H, W = dy_nchw.shape[-2:]
    a = np.abs(np.asarray(dy_nchw, np.float64))
    s = np.einsum("oi,bcop,pj->bcij", tap_matrix(h, H), a, tap_matrix(w, W))
    n = np.einsum("oi,pj->ij", tap_matrix(h, H, count=True), tap_matrix(w, W, count=True))
    return (n + 2.0) * U * s
