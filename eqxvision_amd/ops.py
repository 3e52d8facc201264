"""Host-side operator layer: Python wrappers that marshal `Act`s into the C ABI
(`include/eqxvision_amd.h`).  One function per fused op of the hot path; weight preparation
(BN folding, KRSC re-layout, bf16 conversion) happens once per module and is cached on it.

Everything here enqueues HIP kernels on torch's current stream; nothing computes on the host.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._act import (Act, is_act, DT, TORCH_DT, compute_dtype, device, empty, head_fp32, on_replay, residual_fp32, split_weights,
                   stream_ptr)

ACT = {None: _lib.ACT_NONE, "none": _lib.ACT_NONE, "relu": _lib.ACT_RELU, "gelu": _lib.ACT_GELU_TANH,
       "hard_swish": _lib.ACT_HARD_SWISH, "hard_sigmoid": _lib.ACT_HARD_SIGMOID, "sigmoid": _lib.ACT_SIGMOID, "silu": _lib.ACT_SILU}
UNFUSED_ACTS = ("hard_swish", "hard_sigmoid", "sigmoid", "silu")    # element-wise entries + depthwise conv only (header: MV_ACT_*)


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _dev(a: np.ndarray, dtype: torch.dtype) -> torch.Tensor:
    a = np.ascontiguousarray(a)
    if dtype == torch.bfloat16 and a.dtype == np.float32 and a.size < (1 << 20):
        # small per-call constants (DropPath noise, folded scales): round to bf16 with integer numpy -- a torch CPU cast wakes the
        # whole intra-op thread pool, 16 ms per call on a 100+-core host against microseconds here
        u = a.view(np.uint32)
        r = ((u >> np.uint32(16)) & np.uint32(1)) + np.uint32(0x7FFF)
        b = np.where(np.isnan(a), np.uint32(0x7FC0), (u + r) >> np.uint32(16)).astype(np.uint16)
        return torch.from_numpy(b.view(np.int16)).to(device()).view(torch.bfloat16)
    t = torch.from_numpy(a)
    if t.dtype != dtype:
        t = t.to(dtype)            # host-side RNE conversion of constants (weights)
    return t.to(device())


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


# ------------------------------------------------------------------ weight preparation (cached)
def bn_fold(bn) -> Tuple[np.ndarray, np.ndarray]:
    """BatchNorm inference as per-channel scale/shift:  (x-mean)/sqrt(var+eps)*w+b."""
    st = bn.state_index.value
    if st is None:
        raise RuntimeError(
            "BatchNorm has no running statistics (the reference's unloaded eqx.experimental.BatchNorm "
            "cannot run inference either); load weights or set them via load_torch_weights")
    mean, var = st
    inv = 1.0 / np.sqrt(np.asarray(var, np.float32) + np.float32(bn.eps))
    g = np.asarray(bn.weight, np.float32) if bn.weight is not None else np.ones_like(inv)
    b = np.asarray(bn.bias, np.float32) if bn.bias is not None else np.zeros_like(inv)
    scale = (g * inv).astype(np.float32)
    shift = (b - np.asarray(mean, np.float32) * scale).astype(np.float32)
    return scale, shift


def _bn_training(bn) -> bool:
    return bn is not None and not bn.inference


def _prepared(mod, tag, deps, build):
    """The operands `build()` prepares for `mod`, made once and kept in the module's cache under `tag` (a hashable: the static variant --
    layout, dtype, form).  `deps`: the foreign objects the operands are made from -- parameter leaves, sibling modules, BatchNorms
    (None where absent).  The entry holds them, and a later call is a hit only if it passes the very same objects (`is`; an id()
    alone could be a recycled one: tree_at shares untouched sub-modules between trees); another set of objects under the same tag
    gets an entry of its own.  A BatchNorm among them also has to be at the version of its running statistics the operands were
    folded with (the StateIndex is shared by every copy of the module, e.g. tree_inference's; a training-mode update bumps it):
    otherwise the entry is rebuilt in place, so the stale device tensors go."""
    entries = mod._cache().setdefault(tag, [])
    vers = [d.state_index.version for d in deps if hasattr(d, "state_index")]
    for e in entries:
        if len(e[0]) == len(deps) and all(a is b for a, b in zip(e[0], deps)):
            if e[1] != vers:
                e[1], e[2] = vers, build()
            return e[2]
    entries.append([tuple(deps), vers, build()])
    return entries[-1][2]


def _bias(m) -> Optional[np.ndarray]:
    """A module's bias as a flat fp32 vector, None where it has none."""
    return None if m.bias is None else np.asarray(m.bias, np.float32).reshape(-1)


def _dev_bias(m) -> Optional[torch.Tensor]:
    b = _bias(m)
    return None if b is None else _dev(b, torch.float32)


def _conv_fold(conv, bn):
    """fp32 (scale, shift) of a convolution's bias + BatchNorm(inference) epilogue; None for a part there is nothing to apply for."""
    bias = _bias(conv)
    if bn is None:
        return None, bias
    scale, shift = bn_fold(bn)
    return scale, shift if bias is None else shift + bias * scale


def _ln_fold(lin, ln, wide: bool = False):
    """A LayerNorm's affine folded into the Linear behind it, fp32: (W . diag(gamma), b + W . beta); `wide`: b + W . beta is formed
    in float64 and rounded once."""
    w = np.asarray(lin.weight, np.float32)
    g, beta = np.asarray(ln.weight, np.float32).reshape(-1), np.asarray(ln.bias, np.float32).reshape(-1)
    b = np.zeros(w.shape[0], np.float32) if lin.bias is None else _bias(lin)
    if wide:
        return w * g[None, :], (b.astype(np.float64) + w.astype(np.float64) @ beta.astype(np.float64)).astype(np.float32)
    return w * g[None, :], b + w @ beta


def bn_train_update(bn, y: Act):
    """The statistics half of eqx.experimental.BatchNorm's TRAINING branch (resnet.py:132-136 with the model
    not in inference mode): per-channel batch mean, then the mean of squared deviations from it -- two passes, each summed over
    the ranks of `axis_name`'s data-parallel group (RCCL all-reduce of C floats on the launch stream) --, then the running
    statistics: first call: running = batch; later: running = (1 - momentum) * batch + momentum * running.  Everything stays on
    the device and in stream order (no host round trip inside a step); the host `StateIndex.value` is fetched when asked for.
    Returns the (scale, shift) device vectors of the UPDATED running statistics: what the caller normalises with (reference
    semantics)."""
    from . import dist as _dist
    t = y.t
    C = t.shape[-1]
    if C != bn.input_size:
        raise ValueError(f"BatchNorm({bn.input_size}) applied to {C} channels")
    rows = t.numel() // C
    if not _lib.load().mv_channel_moments_supported(rows, C, y.dt):
        raise NotImplementedError(f"training-mode BatchNorm over {C} channels (multiples of 8 up to 2048 only)")
    ws = empty((int(_lib.load().mv_channel_moments_ws(C)),), torch.float32)
    s, q, mean = (empty((C,), torch.float32) for _ in range(3))
    reduce_ranks = bn.axis_name is not None and _dist.world_size() > 1
    cnt = None
    st = stream_ptr()
    if reduce_ranks:                       # rows of the GLOBAL batch (shards may be ragged): summed on the device
        mine, cnt = empty((1,), torch.float32), empty((1,), torch.float32)
        mine.fill_(float(rows))            # (a constant of the recording; the copy + in-place sum below are what a replay repeats)
        _lib.call("mv_cast", _ptr(mine), _ptr(cnt), 1, _lib.F32, _lib.F32, st)
        _dist.all_reduce_sum_(cnt)
    sidx = bn.state_index
    first = bool(bn.first_time_index.value) or (sidx._dev is None and sidx._value is None)
    if sidx._dev is None:                  # the running statistics move to the device once and stay there
        host = sidx._value
        run = (torch.zeros(C, dtype=torch.float32, device=device()), torch.ones(C, dtype=torch.float32, device=device())) \
            if host is None else tuple(_dev(np.asarray(a, np.float32), torch.float32) for a in host)
    else:
        run = sidx._dev
    w = prep_f32(bn, "weight", bn.weight) if bn.weight is not None else None
    b = prep_f32(bn, "bias", bn.bias) if bn.bias is not None else None
    scale, shift = empty((C,), torch.float32), empty((C,), torch.float32)
    if first or _lib.get_flag("bn_two_pass"):
        # the reference's literal two passes (mean, then squared deviations from it): nothing to centre a single pass on yet
        _lib.call("mv_channel_moments_fwd", _ptr(t), None, _ptr(s), _ptr(ws), rows, C, 0, y.dt, st)
        if reduce_ranks:
            _dist.all_reduce_sum_(s)
        _lib.call("mv_bn_mean_fwd", _ptr(s), _ptr(cnt), float(rows), _ptr(mean), C, st)
        _lib.call("mv_channel_moments_fwd", _ptr(t), _ptr(mean), _ptr(q), _ptr(ws), rows, C, 1, y.dt, st)
        if reduce_ranks:
            _dist.all_reduce_sum_(q)
        _lib.call("mv_bn_ema_fold_fwd", _ptr(q), _ptr(mean), _ptr(cnt), float(rows), _ptr(run[0]), _ptr(run[1]), _ptr(w), _ptr(b),
                  _ptr(scale), _ptr(shift), float(bn.momentum), float(bn.eps), 1 if first else 0, C, st)
    else:
        # steady state: both moments about the running mean in ONE pass, ONE all-reduce of 2 x C floats per layer
        ws2, sums = empty((2 * ws.numel(),), torch.float32), empty((2 * C,), torch.float32)
        _lib.call("mv_channel_moments2_fwd", _ptr(t), _ptr(run[0]), _ptr(sums), _ptr(ws2), rows, C, y.dt, st)
        if reduce_ranks:
            _dist.all_reduce_sum_(sums)
        _lib.call("mv_bn_ema_fold1_fwd", _ptr(sums), _ptr(cnt), float(rows), _ptr(run[0]), _ptr(run[1]), _ptr(w), _ptr(b),
                  _ptr(scale), _ptr(shift), float(bn.momentum), float(bn.eps), C, st)
    if first:
        bn.first_time_index.value = False
    # what the backward of THIS call needs (grad._bn_backward): the weight of the batch statistics in the statistics the layer
    # normalised with (running' = a * batch + (1 - a) * running), the row count of the data-parallel batch and whether the column
    # sums have to be summed over ranks
    sidx._last_update = dict(a=1.0 if first else 1.0 - float(bn.momentum), rows=float(rows), cnt=cnt, reduce=reduce_ranks)
    sidx.device_updated(run)               # bumps the version: every fold prepared with the old statistics is stale (_prepared)
    on_replay(lambda s=sidx, r=run: s.device_updated(r))     # ... and again after every replay of a recorded step
    return scale, shift


def _bn_affine(y: Act, scale: torch.Tensor, shift: torch.Tensor, act=None, residual: Optional[Act] = None) -> Act:
    C = y.t.shape[-1]
    out = empty(tuple(y.t.shape), y.t.dtype)
    if residual is not None and C % 8 == 0 and residual.t.dtype == y.t.dtype and tuple(residual.t.shape) == tuple(y.t.shape):
        _lib.call("mv_channel_affine_res_fwd", _ptr(y.t), _ptr(scale), _ptr(shift), _ptr(residual.t), _ptr(out), y.t.numel() // C, C,
                  ACT[act], y.dt, stream_ptr())
        return Act(out, y.kind, y.batched)
    _lib.call("mv_channel_affine_fwd", _ptr(y.t), _ptr(scale), _ptr(shift), _ptr(out), y.t.numel() // C, C,
              ACT[act if residual is None else None], y.dt, stream_ptr())
    z = Act(out, y.kind, y.batched)
    return z if residual is None else add(z, residual, act)


def prep_conv(conv, bn, layout: str, dtype: str):
    def build():
        w = np.asarray(conv.weight, np.float32)                      # (O, I/g, kh, kw)
        if layout == "krsc":
            w = np.ascontiguousarray(w.transpose(0, 2, 3, 1))
        scale, shift = _conv_fold(conv, bn)
        return (_dev(w, TORCH_DT[dtype]),
                None if scale is None else _dev(scale, torch.float32),
                None if shift is None else _dev(shift, torch.float32))
    return _prepared(conv, ("conv", layout, dtype), (bn,), build)


def prep_conv_grouped64(conv, bn):
    """Grouped filters (O, I/g, kh, kw) expanded to the per-tile input windows: [O][kh][kw][win] (the layout
    mv_conv2d_nhwc_grouped64_fwd documents; block-diagonal 64 x 64 tiles when the group width divides 64), bf16; BN folded to
    fp32 scale / shift as in prep_conv."""
    def build():
        w = np.asarray(conv.weight, np.float32)                      # (O, Cg, kh, kw)
        O_, cg, kh, kw = w.shape
        win = int(_lib.load().mv_conv2d_grouped64_window(O_, conv.groups))
        w64 = np.zeros((O_, kh, kw, win), np.float32)
        for k in range(O_):
            off = (k // cg) * cg - ((k // 64 * 64) // cg) * cg       # my group's first channel inside my tile's window
            w64[k, :, :, off:off + cg] = w[k].transpose(1, 2, 0)
        scale, shift = _conv_fold(conv, bn)
        return (_dev(w64, torch.bfloat16), None if scale is None else _dev(scale, torch.float32),
                None if shift is None else _dev(shift, torch.float32))
    return _prepared(conv, "conv_g64", (bn,), build)


def prep_linear(lin, dtype: str):
    return _prepared(lin, ("lin", dtype), (), lambda: (_dev(np.asarray(lin.weight, np.float32), TORCH_DT[dtype]), _dev_bias(lin)))


def _bf16_split(w: np.ndarray):
    """fp32 -> (hi, lo) bf16 tensors with hi + lo ~ w to ~16 mantissa bits (host, round-to-nearest-even)."""
    t = torch.from_numpy(np.ascontiguousarray(w.astype(np.float32)))
    hi = t.to(torch.bfloat16)
    lo = (t - hi.to(torch.float32)).to(torch.bfloat16)
    return hi, lo


def prep_linear_split(lin):
    """[N][2K] = [hi row | lo row] bf16 + fp32 bias (cached)."""
    def build():
        hi, lo = _bf16_split(np.asarray(lin.weight, np.float32))
        return torch.cat([hi, lo], dim=1).contiguous().to(device()), _dev_bias(lin)
    return _prepared(lin, "lin_split", (), build)


def prep_conv_split(conv):
    """OIHW weights as (hi, lo) bf16 + fp32 bias (cached); no BatchNorm on these call sites."""
    def build():
        hi, lo = _bf16_split(np.asarray(conv.weight, np.float32))
        return hi.to(device()), lo.to(device()), _dev_bias(conv)
    return _prepared(conv, "conv_split", (), build)


def prep_f32(mod, name: str, arr) -> Optional[torch.Tensor]:
    if arr is None:
        return None
    from ._module import DevArray
    return _prepared(mod, ("f32", name), (),
                     lambda: arr.dev.reshape(-1) if isinstance(arr, DevArray) else _dev(np.asarray(arr, np.float32), torch.float32))


# ------------------------------------------------------------------ layout plumbing
def as_map(x: Act) -> Act:
    """img (NCHW, user dtype) -> map (NHWC, compute dtype)."""
    if x.kind == "map":
        return x
    if x.kind != "img":
        raise ValueError(f"expected an image / feature map, got {x}")
    B, C, H, W = x.t.shape
    dt = compute_dtype()
    y = empty((B, H, W, C), TORCH_DT[dt])
    _lib.call("mv_nchw_to_nhwc", _ptr(x.t), _ptr(y), B, C, H, W, x.dt, DT[dt], stream_ptr())
    return Act(y, "map", x.batched)


def as_rows(x: Act, keep_fp32: bool = False) -> Act:
    """seq / vec in the compute dtype (fp32 rows pass through when `keep_fp32`: residual streams)."""
    dt = compute_dtype()
    if x.t.dtype == TORCH_DT[dt] or (keep_fp32 and x.t.dtype == torch.float32):
        return x
    y = empty(tuple(x.t.shape), TORCH_DT[dt])
    _lib.call("mv_cast", _ptr(x.t), _ptr(y), x.t.numel(), x.dt, DT[dt], stream_ptr())
    return Act(y, x.kind, x.batched)


def to_user(x: Act) -> torch.Tensor:
    """Act -> fp32 torch tensor in the reference's logical layout (batch axis kept iff batched)."""
    if x.ln is not None:            # a residual stream kept as two bf16 planes never leaves as its high plane alone
        x = stream_f32(x)
    if x.kind == "map":
        B, H, W, C = x.t.shape
        y = empty((B, C, H, W), torch.float32)
        _lib.call("mv_nhwc_to_nchw", _ptr(x.t), _ptr(y), B, C, H, W, x.dt, _lib.F32, stream_ptr())
    elif x.t.dtype == torch.float32:
        y = x.t
    else:
        y = empty(tuple(x.t.shape), torch.float32)
        _lib.call("mv_cast", _ptr(x.t), _ptr(y), x.t.numel(), x.dt, _lib.F32, stream_ptr())
    return y if x.batched else y[0]


def flatten(x: Act) -> Act:
    """jnp.ravel of the logical (C,H,W) sample -> vec, CHW order (alexnet.py:83, resnet.py:355)."""
    if x.kind == "vec":
        return x
    if x.kind == "seq":
        B = x.B
        return Act(x.t.reshape(B, -1), "vec", x.batched)
    x = as_map(x)
    B, H, W, C = x.t.shape
    if H * W == 1:
        return Act(x.t.reshape(B, C), "vec", x.batched)
    y = empty((B, C, H, W), x.t.dtype)
    _lib.call("mv_nhwc_to_nchw", _ptr(x.t), _ptr(y), B, C, H, W, x.dt, x.dt, stream_ptr())
    return Act(y.reshape(B, C * H * W), "vec", x.batched)


# ------------------------------------------------------------------ contractions
STEM_MAX_CIN = 4


def conv2d(x: Act, conv, bn=None, act=None, residual: Optional[Act] = None) -> Act:
    """Conv2d [+ BatchNorm(inference)] [+ residual] [+ relu/gelu], one launch.  A BatchNorm in TRAINING mode cannot be folded:
    convolution, batch statistics (+ cross-rank sum), running-statistics update, normalisation, (+ residual, activation)."""
    if _bn_training(bn):
        y = conv2d(x, conv, None, None, None)
        sc, sh = bn_train_update(bn, y)
        return _bn_affine(y, sc, sh, act, None if residual is None else as_map(residual))
    dt = compute_dtype()
    if act in UNFUSED_ACTS and (dt != "bf16" or (x.kind != "img" and conv.out_channels % 8) or
                                (conv.groups > 1 and not conv.groups == conv.in_channels == conv.out_channels)):
        # hard_swish & co. are fused by the NHWC bf16 convolution (dense: the streaming / one tile kernel have them; depthwise: in
        # the kernel) and by the image-entry kernels; the grouped / padded-width paths and fp32 mode take an element-wise pass
        return eltwise(conv2d(x, conv, bn, None, residual), act)
    kh, kw = conv.kernel_size
    sh, sw = conv.stride
    ph, pw = conv.padding
    dh, dw = conv.dilation
    K, Cin = conv.out_channels, conv.in_channels
    if x.kind == "img" and Cin <= STEM_MAX_CIN and conv.groups == 1 and dh == 1 and dw == 1 and residual is None:
        B, C, H, W = x.t.shape
        if C != Cin:
            raise ValueError(f"Conv2d expected {Cin} input channels, got {C}")
        w, scale, shift = prep_conv(conv, bn, "oihw", dt)
        Ho = (H + 2 * ph - (kh - 1) - 1) // sh + 1
        Wo = (W + 2 * pw - (kw - 1) - 1) // sw + 1
        y = empty((B, Ho, Wo, K), TORCH_DT[dt])
        _lib.call("mv_conv2d_nchw_fwd", _ptr(x.t), _ptr(w), _ptr(scale), _ptr(shift), _ptr(y),
                  B, C, H, W, K, kh, kw, sh, sw, ph, pw, ACT[act], x.dt, DT[dt], 0, 0, None, stream_ptr())
        return Act(y, "map", x.batched)
    x = as_map(x)
    B, H, W, C = x.t.shape
    if C != Cin:
        raise ValueError(f"Conv2d expected {Cin} input channels, got {C}")
    if x.t.dtype != TORCH_DT[dt]:
        raise ValueError(f"activation dtype {x.t.dtype} does not match compute dtype {dt}")
    Ho = (H + 2 * ph - dh * (kh - 1) - 1) // sh + 1
    Wo = (W + 2 * pw - dw * (kw - 1) - 1) // sw + 1

    def res_ptr():
        if residual is None:
            return None
        r = as_map(residual)
        if tuple(r.t.shape) != (B, Ho, Wo, K):
            raise ValueError(f"residual shape {tuple(r.t.shape)} != conv output {(B, Ho, Wo, K)}")
        return _ptr(r.t)

    if conv.groups > 1 and dt == "bf16" and residual is None and \
            _lib.load().mv_dwconv2d_supported(C, K, conv.groups, kh, kw, _lib.BF16, _lib.BF16):
        hit = prep_dw(conv, bn)
        y = empty((B, Ho, Wo, K), torch.bfloat16)
        _lib.call("mv_dwconv2d_nhwc_fwd", _ptr(x.t), _ptr(hit[0]), _ptr(hit[1]), _ptr(hit[2]), _ptr(y), B, H, W, C, kh, kw, sh, sw,
                  ph, pw, dh, dw, ACT[act], _lib.BF16, _lib.BF16, stream_ptr())
        return Act(y, "map", x.batched)
    if conv.groups > 1 and dt == "bf16" and _lib.load().mv_conv2d_grouped64_supported(C, K, kh, kw, conv.groups, _lib.BF16, _lib.BF16):
        w64, scale, shift = prep_conv_grouped64(conv, bn)
        y = empty((B, Ho, Wo, K), torch.bfloat16)
        _lib.call("mv_conv2d_nhwc_grouped64_fwd", _ptr(x.t), _ptr(w64), _ptr(scale), _ptr(shift), res_ptr(), _ptr(y),
                  B, H, W, C, K, kh, kw, sh, sw, ph, pw, dh, dw, conv.groups, ACT[act], _lib.BF16, _lib.BF16, stream_ptr())
        return Act(y, "map", x.batched)
    w, scale, shift = prep_conv(conv, bn, "krsc", dt)
    if K % 8 and dt == "bf16" and conv.groups == 1 and residual is None and C % 8 == 0:
        # an output width the MFMA kernels cannot store in 16-byte pieces (21-class segmentation heads, fcn.py:33): run the
        # convolution on zero-padded filters and compact the rows afterwards instead of dropping to the VALU kernel
        return _conv2d_padded_k(x, conv, bn, act, (w, scale, shift), (B, H, W, C, Ho, Wo))
    y = empty((B, Ho, Wo, K), TORCH_DT[dt])
    if conv.groups == 1 and dt == "bf16":
        _splitk_scratch(B * Ho * Wo, K, kh * kw * C)
    _lib.call("mv_conv2d_nhwc_fwd", _ptr(x.t), _ptr(w), _ptr(scale), _ptr(shift), res_ptr(), _ptr(y),
              B, H, W, C, K, kh, kw, sh, sw, ph, pw, dh, dw, conv.groups, ACT[act], DT[dt], DT[dt], stream_ptr())
    return Act(y, "map", x.batched)


def _conv2d_padded_k(x: Act, conv, bn, act, prep, dims) -> Act:
    w, scale, shift = prep
    B, H, W, C, Ho, Wo = dims
    K = conv.out_channels
    Kp = (K + 7) // 8 * 8

    def build():
        wp = torch.zeros((Kp,) + tuple(w.shape[1:]), dtype=w.dtype, device=w.device)
        wp[:K] = w
        pad1 = lambda v, fill: None if v is None else torch.cat([v, torch.full((Kp - K,), fill, dtype=v.dtype, device=v.device)])
        return wp, pad1(scale, 1.0), pad1(shift, 0.0)
    hit = _prepared(conv, "kpad", (bn,), build)
    kh, kw = conv.kernel_size
    sh, sw = conv.stride
    ph, pw = conv.padding
    dh, dw = conv.dilation
    yp = empty((B, Ho, Wo, Kp), torch.bfloat16)
    _lib.call("mv_conv2d_nhwc_fwd", _ptr(x.t), _ptr(hit[0]), _ptr(hit[1]), _ptr(hit[2]), None, _ptr(yp),
              B, H, W, C, Kp, kh, kw, sh, sw, ph, pw, dh, dw, 1, ACT[act], _lib.BF16, _lib.BF16, stream_ptr())
    y = empty((B, Ho, Wo, K), torch.bfloat16)
    _lib.call("mv_copy_rows", _ptr(yp), _ptr(y), B * Ho * Wo, K * 2, Kp * 2, K * 2, stream_ptr())
    return Act(y, "map", x.batched)


def _strided_pointwise(conv) -> bool:
    """1x1, no padding, no dilation, one group, the same stride along both axes."""
    s = tuple(conv.stride)
    return (tuple(conv.kernel_size) == (1, 1) and s[0] == s[1] and tuple(conv.padding) == (0, 0)
            and tuple(conv.dilation) == (1, 1) and conv.groups == 1)


def _pointwise(conv) -> bool:
    return _strided_pointwise(conv) and tuple(conv.stride) == (1, 1)


def _chained(y: torch.Tensor, conv1n, t1: torch.Tensor, batched, sub=None) -> Act:
    """What a chain entry returns: the block output y (`.sub`: written only at every sub-th row and column) with the next
    block's conv1 result attached as `.pre = (conv1n, Act)`."""
    out = Act(y, "map", batched)
    out.sub = sub
    out.pre = (conv1n, Act(t1, "map", batched))
    return out


def conv1x1_chain(x: Act, conv3, bn3, residual: Act, conv1n, bn1n, sub: int = 0) -> Optional[Act]:
    """relu(bn3(conv3(x)) + residual), and in the same launch relu(bn1n(conv1n(.))) of that result: the tail of one
    ResNet bottleneck and the head of the next (resnet.py:144-162).  Returns the first result with the second attached
    as `.pre = (conv1n, Act)`, or None when the library has no fused path for the shapes (caller falls back to conv2d).
    `sub` = 2: the caller guarantees that the only other consumer of the first result is a stride-2 pointwise convolution
    (the next stage's downsample branch); where the library can, only the pixels that convolution reads are written
    (`.sub = 2`, a quarter of the map); otherwise the full map is written as usual."""
    dt = compute_dtype()
    if dt != "bf16" or not (_pointwise(conv3) and _pointwise(conv1n)) or conv3.out_channels != conv1n.in_channels:
        return None
    if _bn_training(bn3) or _bn_training(bn1n):
        return None
    x, residual = as_map(x), as_map(residual)
    B, H, W, C = x.t.shape
    K, N2 = conv3.out_channels, conv1n.out_channels
    M = B * H * W
    if C != conv3.in_channels or tuple(residual.t.shape) != (B, H, W, K) or x.t.dtype != torch.bfloat16 \
            or residual.t.dtype != torch.bfloat16:
        return None
    lib = _lib.load()
    # the accumulator-layout kernels (csrc/chain_rc.hip: chain_res; csrc/chain_l2.hip for C = 128 / K = 512, which also serves N2 = 256,
    # a width mv_conv1x1_chain_supported refuses) where they have the shape
    for sb in ((2, 0) if sub == 2 else (0,)):
        if lib.mv_conv1x1_chain_res_supported(B, H, W, C, K, N2, sb, DT[dt]):
            wf, shf = chain_acc_operands(conv3, [[(conv3, bn3)]], conv1n, bn1n)
            y = empty((B, H // 2, W // 2, K) if sb else (B, H, W, K), torch.bfloat16)
            t1 = empty((B, H, W, N2), torch.bfloat16)
            _lib.call("mv_conv1x1_chain_res_fwd", _ptr(x.t), _ptr(residual.t), _ptr(wf), _ptr(shf), _ptr(y), _ptr(t1), B, H, W, C, K, N2,
                      sb, DT[dt], stream_ptr())
            return _chained(y, conv1n, t1, x.batched, sub=2 if sb else None)
    if not lib.mv_conv1x1_chain_supported(M, C, K, N2, DT[dt]):
        return None
    w3, s3, h3 = prep_conv(conv3, bn3, "krsc", dt)
    w1, s1, h1 = prep_conv(conv1n, bn1n, "krsc", dt)
    t1 = empty((B, H, W, N2), torch.bfloat16)
    if sub == 2 and _lib.load().mv_conv1x1_chain_sub_supported(B, H, W, C, K, N2, DT[dt]):
        y = empty((B, H // 2, W // 2, K), torch.bfloat16)
        _lib.call("mv_conv1x1_chain_sub_fwd", _ptr(x.t), _ptr(w3), _ptr(s3), _ptr(h3), _ptr(residual.t), _ptr(y), _ptr(w1), _ptr(s1),
                  _ptr(h1), _ptr(t1), B, H, W, C, K, N2, DT[dt], stream_ptr())
        return _chained(y, conv1n, t1, x.batched, sub=2)
    y = empty((B, H, W, K), torch.bfloat16)
    _lib.call("mv_conv1x1_chain_fwd", _ptr(x.t), _ptr(w3), _ptr(s3), _ptr(h3), _ptr(residual.t), _ptr(y), _ptr(w1), _ptr(s1),
              _ptr(h1), _ptr(t1), M, C, K, N2, DT[dt], stream_ptr())
    return _chained(y, conv1n, t1, x.batched)


def _rc_shift_rows(*vecs) -> np.ndarray:
    """The shift rows of mv_conv1x1_chain_rc*_fwd: per 32 values one row of 64 uint32 words, word r < 32 = bf16 hi(v) | bf16 lo(v) << 16
    (two bf16 terms: the shift goes through the matrix pipe as one more k-step), words 32 .. 63 zero."""
    rows = []
    for v in vecs:
        v = np.asarray(v, np.float32).reshape(-1, 32)
        hi = torch.from_numpy(v).to(torch.bfloat16)
        lo = (torch.from_numpy(v) - hi.to(torch.float32)).to(torch.bfloat16)
        w = hi.view(torch.int16).numpy().astype(np.uint16).astype(np.uint32) | (lo.view(torch.int16).numpy().astype(np.uint16).astype(np.uint32) << 16)
        out = np.zeros((v.shape[0], 64), np.uint32)
        out[:, :32] = w
        rows.append(out)
    return np.concatenate(rows, 0)


def chain_acc_operands(cache_on, y_blocks, conv1n, bn1n):
    """The (fragments, shift rows) of the accumulator-layout chain kernels (csrc/chain_acc.h; header:
    mv_conv1x1_chain_rc_fwd, _chain_rc0_fwd, _chain_res_fwd, _dual_chain_res_fwd), cached on `cache_on`.  `y_blocks` lists the
    pointwise (conv, bn) groups that produce y, in the order of the kernel's reduction: the groups of ONE inner list add into the
    same accumulation, so their shifts are summed into one block of shift rows; every inner list has a block of its own.  Per
    32-channel chunk of y: the k-step fragments of the groups' scaled weight rows side by side, then the next conv1's
    (_res_fragments); shift rows: one block per inner list, then the next conv1's (_rc_shift_rows)."""
    def build():
        blocks = [[_scaled_rows(c, b) for c, b in blk] for blk in y_blocks]
        wy = np.concatenate([w for blk in blocks for w, _ in blk], axis=1)
        w1n, hn = _scaled_rows(conv1n, bn1n)
        sh = _rc_shift_rows(*[np.add.reduce([h for _, h in blk]) for blk in blocks], hn)
        return _dev(_res_fragments(wy, w1n).reshape(-1), torch.bfloat16), torch.from_numpy(sh.view(np.int32)).to(device())
    # (the block sizes are part of the variant: the same modules grouped differently are different operands)
    return _prepared(cache_on, ("chain_acc",) + tuple(len(blk) for blk in y_blocks),
                     [m for blk in y_blocks for pair in blk for m in pair] + [conv1n, bn1n], build)


def _res_fragments(w3, w1n) -> np.ndarray:
    """(K / 32, C / 16 + 2 N2 / 32, 2, 32, 8): per 32-channel chunk c of y, the C / 16 fragments of w3[32 c .., :] (k-step kk), then those
    of the next conv1 w1n[:, 32 c ..] as (k-step s, row tile a2) with the reduction index in accumulator order.  A fragment is
    [lane = 32 fh + r][8] = W[row0 + r][k0 + 8 fh ..] (mv_conv1x1_chain_res_fwd, mv_conv1x1_dual_chain_res_fwd)."""
    K, KX, T2 = w3.shape[0], w3.shape[1] // 16, w1n.shape[0] // 32
    frags = np.empty((K // 32, KX + 2 * T2, 2, 32, 8), np.float32)
    e8 = np.arange(8)
    for c in range(K // 32):
        rows = slice(32 * c, 32 * c + 32)
        for fh in range(2):
            for kk in range(KX):
                frags[c, kk, fh] = w3[rows][:, 16 * kk + 8 * fh + e8]
            for s_ in range(2):
                cols = 32 * c + 16 * s_ + 4 * fh + np.array([0, 1, 2, 3, 8, 9, 10, 11])
                for a2 in range(T2):
                    frags[c, KX + T2 * s_ + a2, fh] = w1n[32 * a2:32 * a2 + 32][:, cols]
    return frags


def conv1x1_chain_rc(t2: Act, t2_prev: Act, x0: Act, conv3_0, bn3_0, ds_conv, ds_bn, conv3_1, bn3_1, conv1n, bn1n) -> Optional[Act]:
    """The boundary between the second and the third bottleneck of a stage whose FIRST block output was not written
    (ops.conv1x1_dual_chain(..., store_y=False)): y0 = relu(bn3_0(conv3_0(t2_prev)) + ds_bn(ds_conv(x0))) is recomputed from its
    two 64-channel sources, then y1 = relu(bn3_1(conv3_1(t2)) + y0) and relu(bn1n(conv1n(y1))) as ops.conv1x1_chain
    (resnet.py:144-162, 295-303).  Returns y1 with the next conv1's result attached as `.pre`, or None if unsupported."""
    dt = compute_dtype()
    if dt != "bf16" or not all(_pointwise(c) for c in (conv3_0, ds_conv, conv3_1, conv1n)):
        return None
    if any(_bn_training(b) for b in (bn3_0, ds_bn, bn3_1, bn1n)):
        return None
    t2, t2_prev, x0 = as_map(t2), as_map(t2_prev), as_map(x0)
    B, H, W, C = t2.t.shape
    K, N2 = conv3_1.out_channels, conv1n.out_channels
    M = B * H * W
    if tuple(t2_prev.t.shape) != (B, H, W, C) or tuple(x0.t.shape) != (B, H, W, C) or conv3_0.in_channels != C \
            or ds_conv.in_channels != C or conv3_1.in_channels != C or conv3_0.out_channels != K or ds_conv.out_channels != K \
            or conv1n.in_channels != K or any(a.t.dtype != torch.bfloat16 for a in (t2, t2_prev, x0)):
        return None
    if not _lib.load().mv_conv1x1_chain_rc_supported(M, C, K, N2, DT[dt]):
        return None
    # y0's two sources share an accumulation (one shift block, shift3_0 + shift_d); conv3_1 continues from bf16(y0) with its own
    wf, tab = chain_acc_operands(conv3_1, [[(conv3_0, bn3_0), (ds_conv, ds_bn)], [(conv3_1, bn3_1)]], conv1n, bn1n)
    y = empty((B, H, W, K), torch.bfloat16)
    t1 = empty((B, H, W, N2), torch.bfloat16)
    _lib.call("mv_conv1x1_chain_rc_fwd", _ptr(t2.t), _ptr(t2_prev.t), _ptr(x0.t), _ptr(wf), _ptr(tab), _ptr(y), _ptr(t1), M, C, K, N2,
              DT[dt], stream_ptr())
    return _chained(y, conv1n, t1, t2.batched)


def _fold(conv, bn):
    """fp32 (scale, shift) of a convolution's bias + BatchNorm(inference) epilogue (ones / zeros where absent)."""
    K = conv.out_channels
    scale, shift = _conv_fold(conv, bn)
    return (np.ones(K, np.float32) if scale is None else scale), (np.zeros(K, np.float32) if shift is None else shift)


def prep_bneck_tail(conv2, bn2, conv3, bn3):
    """Weights of a bottleneck's 3x3 and expansion convolutions in the FRAGMENT ORDER of mv_bottleneck_tail_fwd (header): a wave
    owns 32 output channels and fetches each k16-step of them as one contiguous 1 KB piece (cached on conv2)."""
    def build():
        w2 = np.ascontiguousarray(np.asarray(conv2.weight, np.float32).transpose(0, 2, 3, 1))     # [K][R][S][C]
        K, R, S, C = w2.shape
        w2f = w2.reshape(K // 32, 32, R * S, C // 16, 2, 8).transpose(0, 2, 3, 4, 1, 5)            # (wave, tap, j, h, m, e)
        w3 = np.asarray(conv3.weight, np.float32).reshape(conv3.out_channels, C)
        w3f = w3.reshape(conv3.out_channels // 256, 8, 32, C // 16, 2, 8).transpose(0, 1, 3, 4, 2, 5)   # (chunk, wave, j, h, m, e)
        s2, h2 = _fold(conv2, bn2)
        s3, h3 = _fold(conv3, bn3)
        return (_dev(w2f, torch.bfloat16), _dev(s2, torch.float32), _dev(h2, torch.float32),
                _dev(w3f, torch.bfloat16), _dev(s3, torch.float32), _dev(h3, torch.float32))
    return _prepared(conv2, "bneck_tail", (bn2, conv3, bn3), build)


def bottleneck_tail(t1: Act, conv2, bn2, conv3, bn3, identity: Act) -> Optional[Act]:
    """relu(bn3(conv3(relu(bn2(conv2(t1))))) + identity) in ONE launch with the `width`-channel intermediate resident in LDS,
    one workgroup per image (resnet.py:144-162, identity blocks).  None when the library has no such path for the shapes."""
    dt = compute_dtype()
    if dt != "bf16" or _bn_training(bn2) or _bn_training(bn3) or not _pointwise(conv3):
        return None
    if tuple(conv2.kernel_size) != (3, 3) or tuple(conv2.stride) != (1, 1) or tuple(conv2.padding) != (1, 1) \
            or tuple(conv2.dilation) != (1, 1) or conv2.groups != 1 or conv2.in_channels != conv2.out_channels \
            or conv3.in_channels != conv2.out_channels:
        return None
    t1, identity = as_map(t1), as_map(identity)
    B, H, W, C = t1.t.shape
    K = conv3.out_channels
    if C != conv2.in_channels or tuple(identity.t.shape) != (B, H, W, K) or t1.t.dtype != torch.bfloat16 \
            or identity.t.dtype != torch.bfloat16:
        return None
    if not _lib.load().mv_bottleneck_tail_supported(H, W, C, K, DT[dt]):
        return None
    w2f, s2, h2, w3f, s3, h3 = prep_bneck_tail(conv2, bn2, conv3, bn3)
    y = empty((B, H, W, K), torch.bfloat16)
    _lib.call("mv_bottleneck_tail_fwd", _ptr(t1.t), _ptr(w2f), _ptr(s2), _ptr(h2), _ptr(w3f), _ptr(s3), _ptr(h3),
              _ptr(identity.t), _ptr(y), B, H, W, C, K, DT[dt], stream_ptr())
    return Act(y, "map", t1.batched)


def _scaled_rows(conv, bn) -> Tuple[np.ndarray, np.ndarray]:
    """A pointwise conv + BatchNorm(inference) as (scale[k] * W[k, :], shift[k]) in fp32."""
    w = np.asarray(conv.weight, np.float32).reshape(conv.out_channels, -1)
    scale, shift = _fold(conv, bn)
    return w * scale[:, None], shift


def _dual_weights(conv3, bn3, ds_conv, ds_bn):
    """[scale3 * W3 | scale_d * W_d] as bf16 rows and shift3 + shift_d (cached on conv3)."""
    def build():
        w3, h3 = _scaled_rows(conv3, bn3)
        wd, hd = _scaled_rows(ds_conv, ds_bn)
        return _dev(np.concatenate([w3, wd], axis=1), torch.bfloat16), _dev((h3 + hd).astype(np.float32), torch.float32)
    return _prepared(conv3, "dual", (bn3, ds_conv, ds_bn), build)


def conv1x1_dual(x: Act, conv3, bn3, xin: Act, ds_conv, ds_bn, act="relu") -> Optional[Act]:
    """act(bn3(conv3(x)) + ds_bn(ds_conv(xin))): a bottleneck's last conv and its (possibly strided) pointwise downsample
    branch as one GEMM over the concatenated reduction (resnet.py:144-162, 295-303).  None when unsupported."""
    dt = compute_dtype()
    if dt != "bf16" or not _pointwise(conv3):
        return None
    sd = tuple(ds_conv.stride)
    if not _strided_pointwise(ds_conv) or conv3.out_channels != ds_conv.out_channels:
        return None
    if _bn_training(bn3) or _bn_training(ds_bn):
        return None
    x, xin = as_map(x), as_map(xin)
    B, Ho, Wo, C1 = x.t.shape
    B2, H2, W2, C2 = xin.t.shape
    K = conv3.out_channels
    if xin.sub is not None:             # the producer wrote only the pixels this convolution reads (ops.conv1x1_chain(..., sub=))
        if xin.sub != sd[0]:
            raise RuntimeError(f"conv1x1_dual: source sub-sampled by {xin.sub}, convolution stride {sd[0]}")
        sd = (1, 1)
    if B2 != B or (H2 - 1) // sd[0] + 1 != Ho or (W2 - 1) // sd[0] + 1 != Wo or C1 != conv3.in_channels \
            or C2 != ds_conv.in_channels or x.t.dtype != torch.bfloat16 or xin.t.dtype != torch.bfloat16:
        return None
    if not _lib.load().mv_conv1x1_dual_supported(B * Ho * Wo, C1, C2, K, DT[dt]):
        return None
    wcat, shift = _dual_weights(conv3, bn3, ds_conv, ds_bn)
    y = empty((B, Ho, Wo, K), torch.bfloat16)
    _splitk_scratch(B * Ho * Wo, K, C1 + C2)
    _lib.call("mv_conv1x1_dual_fwd", _ptr(x.t), _ptr(xin.t), _ptr(wcat), None, _ptr(shift), _ptr(y), B, Ho, Wo, C1, H2, W2, C2,
              sd[0], K, ACT[act], DT[dt], stream_ptr())
    return Act(y, "map", x.batched)


def conv1x1_dual_available(M: int, conv3, bn3, ds_conv, ds_bn) -> bool:
    """Would ops.conv1x1_dual run for M output pixels of these layers?  (Asked BEFORE a producer decides to write only the pixels
    a strided downsample branch reads.)"""
    if compute_dtype() != "bf16" or not _pointwise(conv3) or _bn_training(bn3) or _bn_training(ds_bn) \
            or conv3.out_channels != ds_conv.out_channels or _lib.get_flag("no_chain_sub"):
        return False
    return bool(_lib.load().mv_conv1x1_dual_supported(M, conv3.in_channels, ds_conv.in_channels, conv3.out_channels, DT["bf16"]))


def chain_rc_available(x: Act, b0, cd, b1, b2) -> bool:
    """Can a three-bottleneck stage run with its first block output un-written (models/classification/resnet.py: _stage_rc)?"""
    if compute_dtype() != "bf16" or _lib.get_flag("no_chain_rc"):
        return False
    convs = (b0.conv3, cd[0], b1.conv1, b1.conv3, b2.conv1)
    if not all(_pointwise(c) for c in convs) or any(_bn_training(b) for b in (b0.bn1, b0.bn2, b0.bn3, cd[1], b1.bn1, b1.bn2, b1.bn3, b2.bn1)):
        return False
    if x.kind != "map" or x.t.dtype != torch.bfloat16:
        return False
    B, H, W, C = x.t.shape
    M, K = B * H * W, b0.conv3.out_channels
    if b0.conv3.in_channels != C or cd[0].in_channels != C or b1.conv3.in_channels != C or cd[0].out_channels != K \
            or b1.conv3.out_channels != K or b1.conv1.in_channels != K or b2.conv1.in_channels != K \
            or tuple(b0.conv2.stride) != (1, 1) or tuple(b1.conv2.stride) != (1, 1) or b0.conv2.out_channels != C or b1.conv2.out_channels != C:
        return False
    lib = _lib.load()
    return bool(lib.mv_conv1x1_dual_chain_supported(M, C, C, K, b1.conv1.out_channels, DT["bf16"])
                and lib.mv_conv1x1_chain_rc_supported(M, C, K, b2.conv1.out_channels, DT["bf16"]))


def conv1x1_dual_chain(x: Act, conv3, bn3, xin: Act, ds_conv, ds_bn, conv1n, bn1n, store_y: bool = True) -> Optional[Act]:
    """relu(bn3(conv3(x)) + ds_bn(ds_conv(xin))) -- a bottleneck whose identity is a pointwise conv of the block input
    (resnet.py:295-303) -- and relu(bn1n(conv1n(.))) of that result, in ONE launch: the two convolutions that add into
    the same output run as one GEMM over the concatenated reduction [x | xin], the BatchNorm scales folded into the bf16
    weight rows.  Returns the block output with the next conv1's result attached (`.pre`), or None if unsupported."""
    dt = compute_dtype()
    if dt != "bf16" or not (_pointwise(conv3) and _pointwise(conv1n)) or not _strided_pointwise(ds_conv):
        return None
    if conv3.out_channels != ds_conv.out_channels or conv3.out_channels != conv1n.in_channels:
        return None
    if any(_bn_training(b) for b in (bn3, ds_bn, bn1n)):
        return None
    x, xin = as_map(x), as_map(xin)
    B, H, W, C1 = x.t.shape
    C2, K, N2 = xin.t.shape[-1], conv3.out_channels, conv1n.out_channels
    M = B * H * W
    if tuple(xin.t.shape[:3]) != (B, H, W) or C1 != conv3.in_channels or C2 != ds_conv.in_channels \
            or x.t.dtype != torch.bfloat16 or xin.t.dtype != torch.bfloat16:
        return None
    ds_stride = tuple(ds_conv.stride)
    if store_y and (ds_stride == (1, 1) or (xin.sub is not None and ds_stride == (xin.sub, xin.sub))) \
            and _lib.load().mv_conv1x1_dual_chain_res_supported(M, C1, C2, K, N2, DT[dt]):
        # C = 128 / K = 512 (layer 2 entry): y stored, weights streamed (csrc/chain_l2.hip); xin is the map the downsample branch reads
        wf, tab = chain_acc_operands(conv3, [[(conv3, bn3), (ds_conv, ds_bn)]], conv1n, bn1n)
        y = empty((B, H, W, K), torch.bfloat16)
        t1 = empty((B, H, W, N2), torch.bfloat16)
        _lib.call("mv_conv1x1_dual_chain_res_fwd", _ptr(x.t), _ptr(xin.t), _ptr(wf), _ptr(tab), _ptr(y), _ptr(t1), M, C1, C2, K, N2,
                  DT[dt], stream_ptr())
        return _chained(y, conv1n, t1, x.batched)
    if not _pointwise(ds_conv) or not _lib.load().mv_conv1x1_dual_chain_supported(M, C1, C2, K, N2, DT[dt]):
        return None
    if not store_y and not _lib.get_flag("no_chain_rc0") and _lib.load().mv_conv1x1_chain_rc_supported(M, C1, K, N2, DT[dt]):
        wf, tab = chain_acc_operands(conv3, [[(conv3, bn3), (ds_conv, ds_bn)]], conv1n, bn1n)   # the same function without its output map
        t1 = empty((B, H, W, N2), torch.bfloat16)
        _lib.call("mv_conv1x1_chain_rc0_fwd", _ptr(x.t), _ptr(xin.t), _ptr(wf), _ptr(tab), _ptr(t1), M, C1, K, N2, DT[dt], stream_ptr())
        return Act(t1, "map", x.batched)
    wcat, shift = _dual_weights(conv3, bn3, ds_conv, ds_bn)
    w1, s1, h1 = prep_conv(conv1n, bn1n, "krsc", dt)
    y = empty((B, H, W, K), torch.bfloat16) if store_y else None
    t1 = empty((B, H, W, N2), torch.bfloat16)
    _lib.call("mv_conv1x1_dual_chain_fwd", _ptr(x.t), _ptr(xin.t), _ptr(wcat), None, _ptr(shift), _ptr(y), _ptr(w1), _ptr(s1),
              _ptr(h1), _ptr(t1), M, C1, C2, K, N2, DT[dt], stream_ptr())
    if not store_y:                     # the block output stays un-written (the next boundary recomputes it: ops.conv1x1_chain_rc):
        return Act(t1, "map", x.batched)        # the caller gets the next block's conv1 output itself
    return _chained(y, conv1n, t1, x.batched)


def stem_conv_pool(x: Act, conv, bn, act, pool) -> Act:
    """ResNet entry (resnet.py:243-254): conv1 + bn1 + relu + maxpool.  One launch when the library has the fused
    path for this configuration (the 112x112x64 map then never reaches HBM), else conv2d followed by maxpool2d."""
    if _bn_training(bn):
        return maxpool2d(conv2d(x, conv, bn, act), pool.kernel_size, pool.stride, pool.padding)
    dt = compute_dtype()
    kh, kw = conv.kernel_size
    sh, sw = conv.stride
    ph, pw = conv.padding
    pk, ps, pp = _pair(pool.kernel_size), _pair(pool.stride), _pair(pool.padding)
    fused = (x.kind == "img" and conv.groups == 1 and tuple(conv.dilation) == (1, 1) and pk[0] == pk[1] and ps[0] == ps[1]
             and pp[0] == pp[1] and x.t.dim() == 4 and x.t.shape[1] == conv.in_channels)
    if fused:
        B, C, H, W = x.t.shape
        fused = bool(_lib.load().mv_stem_conv_pool_supported(C, conv.out_channels, kh, kw, sh, sw, ph, pw, pk[0], ps[0], pp[0],
                                                              ACT[act], x.dt, DT[dt], B * C * H * W))
    if not fused:
        return maxpool2d(conv2d(x, conv, bn, act), pool.kernel_size, pool.stride, pool.padding)
    w, scale, shift = prep_conv(conv, bn, "oihw", dt)
    Ho = (H + 2 * ph - kh) // sh + 1
    Wo = (W + 2 * pw - kw) // sw + 1
    Po = (Ho + 2 * pp[0] - pk[0]) // ps[0] + 1
    Qo = (Wo + 2 * pp[0] - pk[0]) // ps[0] + 1
    y = empty((B, Po, Qo, conv.out_channels), TORCH_DT[dt])
    _lib.call("mv_stem_conv_pool_fwd", _ptr(x.t), _ptr(w), _ptr(scale), _ptr(shift), _ptr(y), B, C, H, W, conv.out_channels,
              kh, kw, sh, sw, ph, pw, pk[0], ps[0], pp[0], ACT[act], x.dt, DT[dt], stream_ptr())
    return Act(y, "map", x.batched)


def linear(x: Act, lin, act=None, residual: Optional[Act] = None, out_fp32: bool = False) -> Act:
    """Linear over the last (feature) axis of rows: seq [B,N,D], vec [B,D] or map (Linear2d)."""
    dt = compute_dtype()
    if act in UNFUSED_ACTS:
        return eltwise(linear(x, lin, None, residual, out_fp32), act)
    x = as_map(x) if x.kind in ("img", "map") else as_rows(x)
    if x.t.dtype != TORCH_DT[dt]:
        x = cast(x, dt)
    N, K = lin.out_features, lin.in_features
    if x.t.shape[-1] != K:
        raise ValueError(f"Linear expected {K} input features, got {x.t.shape[-1]}")
    M = x.t.numel() // K
    if residual is not None and residual.t.dtype == torch.float32:
        out_fp32 = True                 # fp32 residual stream: add and store in fp32
    odt = torch.float32 if out_fp32 else TORCH_DT[dt]
    y = empty(tuple(x.t.shape[:-1]) + (N,), odt)
    res = None
    if residual is not None:
        if tuple(residual.t.shape) != tuple(y.shape) or residual.t.dtype != odt:
            raise ValueError(f"residual shape/dtype mismatch in linear: {residual} vs {tuple(y.shape)} {odt}")
        res = residual.t
    odc = _lib.F32 if out_fp32 else DT[dt]
    if res is None and dt == "bf16" and _lib.load().mv_fc_stream_supported(M, N, K, DT[dt], odc):
        # few rows, a big weight matrix (AlexNet / VGG classifiers): the layer is bound by streaming W -- fragment-ordered weights,
        # split-K over the CUs, fixed-order reduction (csrc/fc_stream.hip)
        # (decided BEFORE prep_linear: the row-major bf16 copy of a 9216 x 4096 weight would only double the device memory)
        wf = fc_fragments(lin)
        b = prep_f32(lin, "bias", _bias(lin))
        nbytes = int(_lib.load().mv_fc_stream_workspace(M, N, K))
        ws = _fc_workspace(nbytes)
        _lib.call("mv_fc_stream_fwd", _ptr(x.t), _ptr(wf), _ptr(b), _ptr(y), _ptr(ws), nbytes, M, N, K, ACT[act], DT[dt], odc, stream_ptr())
        return Act(y, x.kind, x.batched)
    w, b = prep_linear(lin, dt)
    if dt == "bf16":
        _splitk_scratch(M, N, K)
    _lib.call("mv_linear_fwd", _ptr(x.t), _ptr(w), None, _ptr(b), _ptr(res), _ptr(y), M, N, K, ACT[act],
              DT[dt], odc, stream_ptr())
    return Act(y, x.kind, x.batched)


_FC_WS = {}


def _fc_workspace(nbytes: int) -> torch.Tensor:
    """The split-K workspace of an eager call: ONE per stream instead of a fresh allocation per call (launches on a stream are
    ordered, so consecutive layers share it).  While a forward is being RECORDED every call keeps its own: the lanes of a recording
    become parallel branches of the hipGraph, and two branches must not share scratch memory."""
    from . import _act
    if getattr(_act._tls, "keep", None) is not None:
        return empty(((nbytes + 3) // 4,), torch.float32)
    key = (stream_ptr(), torch.cuda.current_device())
    ws = _FC_WS.get(key)
    if ws is None or ws.numel() * 4 < nbytes:
        ws = torch.empty(((nbytes + 3) // 4,), dtype=torch.float32, device=device())
        _FC_WS[key] = ws
    return ws


_SPLITK_WS = {}


def _splitk_scratch(M: int, N: int, kred: int):
    """Hand the next launch on this stream room for split-K partial sums (include/eqxvision_amd.h: mv_set_scratch) when its shape
    is one the library would split: [M] x [N] output, `kred` reduction elements.  Same ownership rule as `_fc_workspace`: while
    a forward is being recorded every launch keeps its own (lanes become parallel graph branches), an eager call shares one per
    stream.  The first 4096 bytes (the tiles' arrival words) are zeroed once; the kernel leaves them zero."""
    nbytes = int(_lib.load().mv_splitk_scratch_bytes(M, N, kred))
    if not nbytes:
        _lib.call("mv_set_scratch", None, 0, stream_ptr())       # withdraw whatever an earlier entry left pending on this thread
        return
    from . import _act
    if getattr(_act._tls, "keep", None) is not None:
        ws = empty((nbytes,), torch.uint8)
        ws[:4096].zero_()
    else:
        key = (stream_ptr(), torch.cuda.current_device())
        ws = _SPLITK_WS.get(key)
        if ws is None or ws.numel() < nbytes:
            ws = torch.zeros((nbytes,), dtype=torch.uint8, device=device())
            _SPLITK_WS[key] = ws
    _lib.call("mv_set_scratch", _ptr(ws), nbytes, stream_ptr())


def fc_fragments(lin) -> torch.Tensor:
    """Linear weight [N][K] in MFMA fragment order for csrc/fc_stream.hip: [N / 32 tiles][K / 16 steps][64 lanes][8] bf16, lane
    (n = l % 32, h = l / 32) holds W[32 tile + n][16 step + 8 h .. + 7]; N is padded to a multiple of 32 with zero rows (cached)."""
    def build():
        w = torch.from_numpy(np.ascontiguousarray(np.asarray(lin.weight, np.float32))).to(torch.bfloat16)
        N, K = w.shape
        NT = (N + 31) // 32
        if NT * 32 != N:
            w = torch.cat([w, torch.zeros((NT * 32 - N, K), dtype=torch.bfloat16)], dim=0)
        # [NT][32 n][K/16][2 h][8] -> [NT][K/16][2 h][32 n][8]
        return w.view(NT, 32, K // 16, 2, 8).permute(0, 2, 3, 1, 4).contiguous().to(device())
    return _prepared(lin, "fc_frag", (), build)


def linear_head(x: Act, lin) -> Act:
    """The classifier head -> fp32 logits.  With `head_fp32()` (default in bf16 mode) features and weights stay fp32 and the
    product runs on the exact-fp32 MFMA; otherwise the bf16 Linear with an fp32 store."""
    if not head_fp32():
        return linear(x, lin, out_fp32=True)
    if x.t.dtype != torch.float32:
        x = cast(x, "fp32")
    w, b = prep_linear(lin, "fp32")
    N, K = lin.out_features, lin.in_features
    if x.t.shape[-1] != K:
        raise ValueError(f"Linear expected {K} input features, got {x.t.shape[-1]}")
    M = x.t.numel() // K
    y = empty(tuple(x.t.shape[:-1]) + (N,), torch.float32)
    _lib.call("mv_linear_fwd", _ptr(x.t), _ptr(w), None, _ptr(b), None, _ptr(y), M, N, K, _lib.ACT_NONE, _lib.F32, _lib.F32,
              stream_ptr())
    return Act(y, x.kind, x.batched)


def linear_split(x: Act, lin, out_fp32: bool = False, act=None, residual: Optional[Act] = None) -> Act:
    """Linear with split-precision (hi + lo bf16) weights where the library has the path, else the plain Linear."""
    dt = compute_dtype()
    x = as_map(x) if x.kind in ("img", "map") else as_rows(x)
    N, K = lin.out_features, lin.in_features
    M = x.t.numel() // K
    if not split_weights() or act in UNFUSED_ACTS or x.t.dtype != torch.bfloat16 or x.t.shape[-1] != K or \
            not _lib.load().mv_linear_split_supported(M, N, K, DT[dt]):
        return linear(x, lin, act=act, residual=residual, out_fp32=out_fp32)
    if residual is not None and residual.t.dtype == torch.float32:
        out_fp32 = True
    w, b = prep_linear_split(lin)
    odt = torch.float32 if out_fp32 else TORCH_DT[dt]
    y = empty(tuple(x.t.shape[:-1]) + (N,), odt)
    res = None
    if residual is not None:
        if tuple(residual.t.shape) != tuple(y.shape) or residual.t.dtype != odt:
            raise ValueError(f"residual shape/dtype mismatch in linear_split: {residual} vs {tuple(y.shape)} {odt}")
        res = residual.t
    _splitk_scratch(M, N, 2 * K)
    _lib.call("mv_linear_split_fwd", _ptr(x.t), _ptr(w), None, _ptr(b), _ptr(res), _ptr(y), M, N, K, ACT[act], DT[dt],
              _lib.F32 if out_fp32 else DT[dt], stream_ptr())
    return Act(y, x.kind, x.batched)


_SWIN_FUSED_WIDTHS = (96, 192, 384, 768)


def swin_precise(C: int) -> bool:
    """Swin widths outside swin_t / swin_s's (swin_b: 128 / 256 / 512 / 1024) take the un-fused block path; there the bf16 rounding
    of the block Linears' WEIGHTS alone is 1.16e-2 of absolute logit error over 24 blocks (tests/attrib_swin_bf16.py: weights
    bf16 / activations fp32 1.16e-2, weights fp32 / activations bf16 2.2e-3), past north_star's 1e-2 -- so those Linears run with
    split-precision weights (two products per layer; swin_b is not a measured config, swin_t's kernels are untouched)."""
    return split_weights() and C not in _SWIN_FUSED_WIDTHS and not _lib.get_flag("no_swin_precise")


def conv2d_entry_split(x: Act, conv) -> Optional[Act]:
    """The network-entry convolution (raw NCHW image, no norm) with split-precision weights; None if not applicable."""
    dt = compute_dtype()
    if not split_weights() or x.kind != "img" or conv.groups != 1 or tuple(conv.dilation) != (1, 1) or \
            conv.in_channels > STEM_MAX_CIN or x.t.shape[1] != conv.in_channels:
        return None
    B, C, H, W = x.t.shape
    kh, kw = conv.kernel_size
    sh, sw = conv.stride
    ph, pw = conv.padding
    K = conv.out_channels
    hi, lo, b = prep_conv_split(conv)
    Ho = (H + 2 * ph - kh) // sh + 1
    Wo = (W + 2 * pw - kw) // sw + 1
    y = empty((B, Ho, Wo, K), TORCH_DT[dt])
    try:
        _lib.call("mv_conv2d_nchw_split_fwd", _ptr(x.t), _ptr(hi), _ptr(lo), None, _ptr(b), _ptr(y), B, C, H, W, K, kh, kw, sh, sw,
                  ph, pw, _lib.ACT_NONE, x.dt, DT[dt], stream_ptr())
    except _lib.MVError:
        return None
    return Act(y, "map", x.batched)


def patch4_ln(x: Act, conv, ln) -> Optional[Act]:
    """LayerNorm2d(Conv2d(3, K, 4, 4)(x)) -- Swin's patch embedding and its norm (swin.py:705-711) -- in one launch from the raw
    NCHW image to the fp32 NHWC residual stream, split-precision weights; None when the library has no such path."""
    if compute_dtype() != "bf16" or x.kind != "img" or x.t.dtype != torch.float32 or conv.groups != 1 or ln.weight is None or ln.bias is None:
        return None
    B, C, H, W = x.t.shape
    K = conv.out_channels
    if tuple(conv.kernel_size) != (4, 4) or tuple(conv.stride) != (4, 4) or tuple(conv.padding) != (0, 0) or tuple(conv.dilation) != (1, 1) \
            or conv.in_channels != C or int(np.prod(ln.shape)) != K:
        return None
    if not _lib.load().mv_patch4_ln_supported(C, H, W, K, _lib.F32):
        return None
    hi, lo, b = prep_conv_split(conv)
    if not split_weights():
        lo = None
    y = empty((B, H // 4, W // 4, K), torch.float32)
    _lib.call("mv_patch4_ln_fwd", _ptr(x.t), _ptr(hi), _ptr(lo), _ptr(b), _ptr(prep_f32(ln, "weight", ln.weight)),
              _ptr(prep_f32(ln, "bias", ln.bias)), _ptr(y), B, C, H, W, K, float(ln.eps), _lib.F32, stream_ptr())
    return Act(y, "map", x.batched)


def patch_embed_tokens(x: Act, conv, cls: Optional[torch.Tensor], pos: Optional[torch.Tensor], n_extra: int, out_fp32: bool = False) -> Act:
    """PatchEmbed conv (k = s = patch) straight from the NCHW image into token rows
    [B, n_extra + P, D]; with `pos` the position embedding is added in the epilogue and row 0 gets
    cls + pos[0] (vit.py:268-269).  `out_fp32` (bf16 mode with the fp32 residual stream): the rows are written in fp32 where the
    library has that epilogue, else in the compute dtype (the caller casts)."""
    dt = compute_dtype()
    if x.kind != "img":
        raise ValueError("patch_embed expects a raw (C,H,W) image")
    B, C, H, W = x.t.shape
    kh, kw = conv.kernel_size
    sh, sw = conv.stride
    ph, pw = conv.padding
    K = conv.out_channels
    w, scale, shift = prep_conv(conv, None, "oihw", dt)
    Ho = (H + 2 * ph - kh) // sh + 1
    Wo = (W + 2 * pw - kw) // sw + 1
    T = n_extra + Ho * Wo
    if out_fp32 and dt == "bf16" and _lib.load().mv_conv2d_nchw_f32out_supported(C, H, W, K, kh, kw, sh, sw, ph, pw, x.dt):
        y = empty((B, T, K), torch.float32)
        _lib.call("mv_conv2d_nchw_f32out_fwd", _ptr(x.t), _ptr(w), _ptr(scale), _ptr(shift), _ptr(y),
                  B, C, H, W, K, kh, kw, sh, sw, ph, pw, _lib.ACT_NONE, x.dt, T, n_extra, _ptr(pos), stream_ptr())
        if n_extra:
            _lib.call("mv_vit_cls_pos_fwd", _ptr(cls), _ptr(pos), _ptr(y), B, T, K, _lib.F32, stream_ptr())
        return Act(y, "seq", x.batched)
    y = empty((B, T, K), TORCH_DT[dt])
    _lib.call("mv_conv2d_nchw_fwd", _ptr(x.t), _ptr(w), _ptr(scale), _ptr(shift), _ptr(y),
              B, C, H, W, K, kh, kw, sh, sw, ph, pw, _lib.ACT_NONE, x.dt, DT[dt], T, n_extra, _ptr(pos), stream_ptr())
    if n_extra:
        _lib.call("mv_vit_cls_pos_fwd", _ptr(cls), _ptr(pos), _ptr(y), B, T, K, DT[dt], stream_ptr())
    return Act(y, "seq", x.batched)


# ------------------------------------------------------------------ normalisation / pooling
def layernorm(x: Act, ln, out_fp32: bool = False) -> Act:
    """Rows of the last axis; reads the input in its own dtype (bf16, or the fp32 residual stream) and
    writes the compute dtype (what the next GEMM consumes) unless `out_fp32`."""
    if x.kind == "img":
        x = as_map(x)
    dt = compute_dtype()
    C = x.t.shape[-1]
    if int(np.prod(ln.shape)) != C:
        raise ValueError(f"LayerNorm over {ln.shape} applied to rows of {C}")
    g = prep_f32(ln, "weight", ln.weight)
    b = prep_f32(ln, "bias", ln.bias)
    odt = torch.float32 if out_fp32 else TORCH_DT[dt]
    y = empty(tuple(x.t.shape), odt)
    _lib.call("mv_layernorm_fwd", _ptr(x.t), _ptr(g), _ptr(b), _ptr(y), x.t.numel() // C, C, 0, float(ln.eps),
              x.dt, _lib.F32 if out_fp32 else DT[dt], stream_ptr())
    return Act(y, x.kind, x.batched)


def _ln_folded(lin, ln):
    """(W . diag(gamma) as bf16, b + W . beta as fp32) on the device, cached on the Linear."""
    def build():
        w, b = _ln_fold(lin, ln)
        return _dev(w, torch.bfloat16), _dev(b, torch.float32)
    return _prepared(lin, "ln_fold", (ln.weight, ln.bias), build)


def _ln_folded_cs(lin, ln):
    """For mv_linear_lnin_fwd: (W' = bf16(W . diag(gamma)), colsum[n] = sum_k W'[n][k] of the ROUNDED values, b' = b + W . beta),
    on the device, cached on the Linear."""
    def build():
        w, bf = _ln_fold(lin, ln, wide=True)
        wf = torch.from_numpy(np.ascontiguousarray(w)).to(torch.bfloat16)
        cs = wf.to(torch.float64).sum(dim=1).to(torch.float32).numpy()
        return wf.to(device()), _dev(cs, torch.float32), _dev(bf, torch.float32)
    return _prepared(lin, "ln_fold_cs", (ln.weight, ln.bias), build)


def _ln_foldable(ln, C: int) -> bool:
    from . import nn
    return (type(ln) is nn.LayerNorm and ln.weight is not None and ln.bias is not None and int(np.prod(ln.shape)) == C)


def linear_lnout_available(M: int, lin) -> bool:
    return (compute_dtype() == "bf16" and residual_fp32()
            and bool(_lib.load().mv_linear_lnout_supported(M, lin.out_features, lin.in_features, _lib.BF16)))


def linear_lnin_available(M: int, ln, lin, tokens: int = 0, dh: int = 0) -> bool:
    return (compute_dtype() == "bf16" and _ln_foldable(ln, lin.in_features)
            and bool(_lib.load().mv_linear_lnin_supported(M, lin.out_features, lin.in_features, tokens, dh, _lib.BF16)))


def is_split_stream(x: Act) -> bool:
    """The residual stream as two bf16 planes: `x.t` = hi = bf16(y), `x.ln` = (lo = bf16(y - hi), row-statistics pieces)."""
    return x.ln is not None and x.t.dtype == torch.bfloat16


def stream_f32(x: Act) -> Act:
    """Split stream -> fp32 rows (hi + lo), for a consumer that has no folded form (three element-wise launches: not the hot path)."""
    if not is_split_stream(x):
        return x
    hi = Act(x.t, x.kind, x.batched)
    lo = Act(x.ln[0], x.kind, x.batched)
    return add(cast(hi, "fp32"), cast(lo, "fp32"))


def linear_lnout(x: Act, lin, residual: Act, out_split: bool = True) -> Act:
    """residual + lin(x) on the residual STREAM of a block whose LayerNorms are folded into the GEMM epilogues (header:
    mv_linear_lnout_fwd).  `residual`: fp32 rows or a split stream; result: a split stream (`Act.t` = the high plane = the operand of
    the LayerNorm + Linear pair behind it, `Act.ln` = (low plane, statistics pieces) -> `linear_lnin`), or fp32 rows
    (`out_split=False`, from a split residual).  Ask `linear_lnout_available` first."""
    x = as_rows(x)
    if x.t.dtype != torch.bfloat16:
        x = cast(x, "bf16")
    N, K = lin.out_features, lin.in_features
    M = x.t.numel() // K
    split_in = is_split_stream(residual)
    if tuple(residual.t.shape) != tuple(x.t.shape[:-1]) + (N,) or not (split_in or residual.t.dtype == torch.float32):
        raise ValueError(f"linear_lnout: residual {residual} does not match {tuple(x.t.shape[:-1]) + (N,)} (fp32 rows or a split stream)")
    if not out_split and not split_in:
        raise ValueError("linear_lnout: fp32 rows in and out is ops.linear")
    w, b = prep_linear(lin, "bf16")
    res_lo = residual.ln[0] if split_in else None
    if out_split:
        y = empty(tuple(residual.t.shape), torch.bfloat16)
        y_lo = empty(tuple(residual.t.shape), torch.bfloat16)
        st = empty(((N + 255) // 256, M, 2), torch.float32)
    else:
        y, y_lo, st = empty(tuple(residual.t.shape), torch.float32), None, None
    _lib.call("mv_linear_lnout_fwd", _ptr(x.t), _ptr(w), _ptr(b), _ptr(residual.t), _ptr(res_lo), _ptr(y), _ptr(y_lo), _ptr(st), M, N, K,
              _lib.BF16, stream_ptr())
    out = Act(y, x.kind, x.batched)
    if out_split:
        out.ln = (y_lo, st)
    return out


def linear_lnin(x: Act, ln, lin, act=None, heads: int = 0):
    """lin(ln(x)) (+ activation) for a split stream x (header: mv_linear_lnin_fwd).  heads > 0: the qkv projection, written
    head-major [B, 3*heads, N, dh] (as `qkv_attention` does).  Ask `linear_lnin_available` first."""
    hi, st = x.t, x.ln[1]
    N, K = lin.out_features, lin.in_features
    M = hi.numel() // K
    w, cs, b = _ln_folded_cs(lin, ln)
    if heads:
        B, T, D = hi.shape
        y = empty((B, 3 * heads, T, D // heads), torch.bfloat16)
        tok, dh = T, D // heads
    else:
        y = empty(tuple(hi.shape[:-1]) + (N,), torch.bfloat16)
        tok, dh = 0, 0
    _lib.call("mv_linear_lnin_fwd", _ptr(hi), _ptr(st), _ptr(w), _ptr(cs), _ptr(b), _ptr(y), M, N, K, float(ln.eps), ACT[act], tok, dh,
              _lib.BF16, stream_ptr())
    return y if heads else Act(y, x.kind, x.batched)


def ln_linear(x: Act, ln, lin, act=None) -> Act:
    """lin(ln(x)) (+ activation): ONE launch where the library folds the LayerNorm into the Linear's operand path (short rows:
    Swin stages 0-1), else LayerNorm launch + Linear launch."""
    from . import nn
    C = lin.in_features
    ok = (compute_dtype() == "bf16" and x.kind in ("map", "seq") and x.t.dtype in (torch.float32, torch.bfloat16)
          and isinstance(ln, nn.LayerNorm) and ln.weight is not None and ln.bias is not None
          and x.t.shape[-1] == C and int(np.prod(ln.shape)) == C)
    if ok:
        M = x.t.numel() // C
        xdt = _lib.F32 if x.t.dtype == torch.float32 else _lib.BF16
        ok = bool(_lib.load().mv_ln_linear_supported(M, lin.out_features, C, xdt, _lib.BF16))
    if not ok:
        return linear(layernorm(x, ln), lin, act=act)
    w, b = _ln_folded(lin, ln)
    y = empty(tuple(x.t.shape[:-1]) + (lin.out_features,), torch.bfloat16)
    _lib.call("mv_ln_linear_fwd", _ptr(x.t), _ptr(w), _ptr(b), _ptr(y), M, lin.out_features, C, float(ln.eps), ACT[act], xdt,
              _lib.BF16, stream_ptr())
    return Act(y, x.kind, x.batched)


def ln_mlp(x: Act, ln, mlp) -> Optional[Act]:
    """x + mlp(ln(x)) in ONE launch where the library has the fused kernel (narrow rows: Swin stage 0), else None.
    The LayerNorm affine is folded into fc1 on the host (fp32, then one bf16 rounding of the product)."""
    from . import nn
    if compute_dtype() != "bf16" or x.kind not in ("map", "seq") or x.t.dtype not in (torch.float32, torch.bfloat16):
        return None
    fc1, fc2 = mlp.fc1, mlp.fc2
    if not (isinstance(fc1, nn.Linear) and isinstance(fc2, nn.Linear) and isinstance(ln, nn.LayerNorm)):
        return None
    if any(not (d.inference or d.p == 0.0) for d in (mlp.drop1, mlp.drop2) if isinstance(d, nn.Dropout)):
        return None
    if nn.act_name(mlp.act) != "gelu" or fc1.bias is None or fc2.bias is None or ln.weight is None or ln.bias is None:
        return None
    C, Hd = fc1.in_features, fc1.out_features
    if x.t.shape[-1] != C or fc2.in_features != Hd or fc2.out_features != C or int(np.prod(ln.shape)) != C:
        return None
    M = x.t.numel() // C
    xdt = _lib.F32 if x.t.dtype == torch.float32 else _lib.BF16
    if not _lib.load().mv_ln_mlp_supported(M, C, Hd, xdt):
        if _lib.load().mv_ln_mlp_stream_supported(M, C, Hd, xdt):
            return _ln_mlp_stream(x, ln, mlp, M, C, Hd, xdt)
        return None

    def build():
        w1, b1 = _ln_fold(fc1, ln)
        return (_dev(w1, torch.bfloat16), _dev(b1, torch.float32), _dev(np.asarray(fc2.weight, np.float32), torch.bfloat16),
                _dev_bias(fc2))
    hit = _prepared(mlp, "ln_mlp", (ln.weight, ln.bias), build)
    y = empty(tuple(x.t.shape), x.t.dtype)
    _lib.call("mv_ln_mlp_fwd", _ptr(x.t), _ptr(hit[0]), _ptr(hit[1]), _ptr(hit[2]), _ptr(hit[3]), _ptr(y), M, C, Hd,
              float(ln.eps), xdt, stream_ptr())
    return Act(y, x.kind, x.batched)


def ln_mlp_fragments(w1: np.ndarray, w2: np.ndarray):
    """fc1 [hidden][C] / fc2 [C][hidden] -> the fragment order of mv_ln_mlp_stream_fwd (header)."""
    Hd, C = w1.shape
    w1f = w1.reshape(Hd // 256, 8, 32, C // 16, 2, 8).transpose(0, 1, 3, 4, 2, 5)            # (chunk, wave, j, h, m, e)
    w2f = w2.reshape(C // 32, 32, Hd // 256, 16, 2, 8).transpose(2, 0, 3, 4, 1, 5)           # (chunk, tile, j, h, m, e)
    return np.ascontiguousarray(w1f), np.ascontiguousarray(w2f)


def _ln_mlp_stream(x: Act, ln, mlp, M, C, Hd, xdt) -> Act:
    """ln_mlp's wide-row variant: weights streamed from L2 in fragment order (LayerNorm affine folded into fc1 on the host)."""
    fc1, fc2 = mlp.fc1, mlp.fc2

    def build():
        w1, b1 = _ln_fold(fc1, ln)
        w1f, w2f = ln_mlp_fragments(w1, np.asarray(fc2.weight, np.float32))
        return _dev(w1f, torch.bfloat16), _dev(b1, torch.float32), _dev(w2f, torch.bfloat16), _dev_bias(fc2)
    hit = _prepared(mlp, "ln_mlp_stream", (ln.weight, ln.bias), build)
    y = empty(tuple(x.t.shape), x.t.dtype)
    _lib.call("mv_ln_mlp_stream_fwd", _ptr(x.t), _ptr(hit[0]), _ptr(hit[1]), _ptr(hit[2]), _ptr(hit[3]), _ptr(y), M, C, Hd,
              float(ln.eps), xdt, stream_ptr())
    return Act(y, x.kind, x.batched)


def cast(x: Act, dtype: str) -> Act:
    if x.t.dtype == TORCH_DT[dtype]:
        return x
    y = empty(tuple(x.t.shape), TORCH_DT[dtype])
    _lib.call("mv_cast", _ptr(x.t), _ptr(y), x.t.numel(), x.dt, DT[dtype], stream_ptr())
    return Act(y, x.kind, x.batched)


def layernorm_first_row(x: Act, ln, out_fp32: bool = False) -> Act:
    """LayerNorm of row 0 of every sample of a seq [B,N,D] -> vec [B,D] (vit.py:272-273: only
    `x[0]` of the normalised tokens is used), via the kernel's row-stride argument."""
    dt = compute_dtype()
    B, N, D = x.t.shape
    g = prep_f32(ln, "weight", ln.weight)
    b = prep_f32(ln, "bias", ln.bias)
    y = empty((B, D), torch.float32 if out_fp32 else TORCH_DT[dt])
    _lib.call("mv_layernorm_fwd", _ptr(x.t), _ptr(g), _ptr(b), _ptr(y), B, D, N * D, float(ln.eps),
              x.dt, _lib.F32 if out_fp32 else DT[dt], stream_ptr())
    return Act(y, "vec", x.batched)


def batchnorm(x: Act, bn, act=None) -> Act:
    """Stand-alone BatchNorm (unfused call sites): per-channel affine with the running statistics -- after updating them from
    this batch when the module is in training mode (reference semantics)."""
    if x.kind == "seq":
        # eqx.experimental.BatchNorm treats AXIS 0 of the single-sample array as channels; a (tokens, features) array would be
        # normalised per token there, per feature here -- refuse instead of returning different numbers (round-1 advice)
        raise NotImplementedError("BatchNorm on a (tokens, features) array: the reference normalises axis 0; not on the hot path")
    x = as_map(x) if x.kind in ("img", "map") else as_rows(x)
    if _bn_training(bn):
        sc, sh = bn_train_update(bn, x)
        return _bn_affine(x, sc, sh, act)
    hit = _prepared(bn, "fold", (bn,), lambda: tuple(_dev(v, torch.float32) for v in bn_fold(bn)))
    C = x.t.shape[-1]
    y = empty(tuple(x.t.shape), x.t.dtype)
    _lib.call("mv_channel_affine_fwd", _ptr(x.t), _ptr(hit[0]), _ptr(hit[1]), _ptr(y), x.t.numel() // C, C,
              ACT[act], x.dt, stream_ptr())
    return Act(y, x.kind, x.batched)


def maxpool2d(x: Act, kernel_size, stride, padding) -> Act:
    x = as_map(x)
    B, H, W, C = x.t.shape
    kh, kw = _pair(kernel_size)
    sh, sw = _pair(stride)
    ph, pw = _pair(padding)
    Ho = (H + 2 * ph - kh) // sh + 1
    Wo = (W + 2 * pw - kw) // sw + 1
    y = empty((B, Ho, Wo, C), x.t.dtype)
    _lib.call("mv_maxpool2d_nhwc_fwd", _ptr(x.t), _ptr(y), B, H, W, C, kh, kw, sh, sw, ph, pw, x.dt, stream_ptr())
    return Act(y, "map", x.batched)


def maxpool2d_ceil(x: Act, pool) -> Act:
    """nn.MaxPool2d(use_ceil=True) (squeezenet.py:88-112): the output size is the module's (equinox's rule), the taps of the last
    window that fall outside the map do not take part (mv_maxpool2d_out_nhwc_fwd)."""
    x = as_map(x)
    B, H, W, C = x.t.shape
    kh, kw = _pair(pool.kernel_size)
    sh, sw = _pair(pool.stride)
    ph, pw = _pair(pool.padding)
    Ho, Wo = pool.output_size(H, W)
    y = empty((B, Ho, Wo, C), x.t.dtype)
    _lib.call("mv_maxpool2d_out_nhwc_fwd", _ptr(x.t), _ptr(y), B, H, W, C, kh, kw, sh, sw, ph, pw, Ho, Wo, x.dt, stream_ptr())
    return Act(y, "map", x.batched)


def avgpool2d(x: Act, kernel_size, stride) -> Act:
    """nn.AvgPool2d: floor-mode output size, no padding (mv_avgpool2d_nhwc_fwd)."""
    x = as_map(x)
    B, H, W, C = x.t.shape
    kh, kw = _pair(kernel_size)
    sh, sw = _pair(stride)
    if H < kh or W < kw:
        raise ValueError(f"avgpool2d: a {kh} x {kw} window on a {H} x {W} map")
    y = empty((B, (H - kh) // sh + 1, (W - kw) // sw + 1, C), x.t.dtype)
    _lib.call("mv_avgpool2d_nhwc_fwd", _ptr(x.t), _ptr(y), B, H, W, C, kh, kw, sh, sw, x.dt, stream_ptr())
    return Act(y, "map", x.batched)


def adaptive_avgpool2d(x: Act, target, out_fp32: bool = False) -> Act:
    x = as_map(x)
    B, H, W, C = x.t.shape
    oh, ow = _pair(target)
    if oh == H and ow == W and not (out_fp32 and x.t.dtype != torch.float32):
        return x
    odt = torch.float32 if out_fp32 else x.t.dtype
    y = empty((B, oh, ow, C), odt)
    _lib.call("mv_adaptive_avgpool2d_nhwc_fwd", _ptr(x.t), _ptr(y), B, H, W, C, oh, ow, x.dt,
              _lib.F32 if odt == torch.float32 else _lib.BF16, stream_ptr())
    return Act(y, "map", x.batched)


# ------------------------------------------------------------------ attention
def _mha_call(qkv_t, head_major: bool, out, probs, B, N, heads, dh, scale, dt, drop):
    """The attention core; `drop` = (p, keys) runs the reference's live attention dropout inside the kernel (vit.py:71)."""
    if drop is None:
        _lib.call("mv_mha_heads_fwd" if head_major else "mv_mha_fwd", _ptr(qkv_t), _ptr(out), _ptr(probs), B, N, heads, dh,
                  float(scale), dt, stream_ptr())
        return
    p, key = drop
    if not 0.0 < float(p) < 1.0:
        raise NotImplementedError(f"attention Dropout(p={p})")
    keys = _keys_dev(key, B)
    _lib.call("mv_mha_dropout_fwd", _ptr(qkv_t), 1 if head_major else 0, _ptr(out), _ptr(probs), _ptr(keys), float(1.0 - p),
              B, N, heads, dh, float(scale), dt, stream_ptr())


def mha(qkv: Act, heads: int, scale: float, need_probs: bool, drop=None):
    """qkv rows [B,N,3D] -> ([B,N,D], probs fp32 [B,heads,N,N] or None)   (vit.py:65-73)."""
    qkv = cast(qkv, compute_dtype())
    B, N, D3 = qkv.t.shape
    D = D3 // 3
    dh = D // heads
    out = empty((B, N, D), qkv.t.dtype)
    probs = empty((B, heads, N, N), torch.float32) if need_probs else None
    _mha_call(qkv.t, False, out, probs, B, N, heads, dh, scale, qkv.dt, drop)
    return Act(out, "seq", qkv.batched), probs


def qkv_attention_ln(x: Act, ln, lin, heads: int, scale: float):
    """`qkv_attention(ln(x), lin, ...)` for a split stream x (inference, no probabilities): the LayerNorm is folded into the qkv
    projection's epilogue (vit.py:142 norm1 -> :64 qkv)."""
    B, N, D = x.t.shape
    qkv = linear_lnin(x, ln, lin, heads=heads)
    out = empty((B, N, D), torch.bfloat16)
    _mha_call(qkv, True, out, None, B, N, heads, D // heads, scale, _lib.BF16, None)
    return Act(out, "seq", x.batched)


def qkv_attention(x: Act, lin, heads: int, scale: float, need_probs: bool, drop=None):
    """qkv Linear + attention core of `_VitAttention` (vit.py:64-73): rows [B,N,D] -> ([B,N,D], probs or None).
    When the library has the path for this shape the projection writes q/k/v head-major
    ([B, 3*heads, N, dh]: what the reference's reshape + transpose produce) and the attention kernel reads
    contiguous heads; otherwise Linear -> [B,N,3D] -> strided attention.  Both are the HIP path.
    `drop` = (p, per-sample keys): training-mode attention dropout, applied to the probabilities inside the kernel."""
    dt = compute_dtype()
    x = as_rows(x)
    if x.t.dtype != TORCH_DT[dt]:
        x = cast(x, dt)
    B, N, D = x.t.shape
    if lin.in_features != D or lin.out_features != 3 * D or D % heads:
        raise ValueError(f"qkv projection {lin.in_features}->{lin.out_features} does not fit rows of {D} / {heads} heads")
    dh = D // heads
    if not _lib.load().mv_linear_heads_supported(B * N, 3 * D, D, N, dh, DT[dt]):
        return mha(linear(x, lin), heads, scale, need_probs, drop)
    w, b = prep_linear(lin, dt)
    qkv = empty((B, 3 * heads, N, dh), TORCH_DT[dt])
    _lib.call("mv_linear_heads_fwd", _ptr(x.t), _ptr(w), None, _ptr(b), _ptr(qkv), B * N, 3 * D, D, N, dh, DT[dt],
              stream_ptr())
    out = empty((B, N, D), TORCH_DT[dt])
    probs = empty((B, heads, N, N), torch.float32) if need_probs else None
    _mha_call(qkv, True, out, probs, B, N, heads, dh, scale, DT[dt], drop)
    return Act(out, "seq", x.batched), probs


def swin_rel_bias(attn) -> torch.Tensor:
    """The relative-position bias [heads][n][n] of a _ShiftedWindowAttention on the device: table[index] gathered on the host
    (swin.py:34-43), cached on the module."""
    return _prepared(attn, "bias", (), lambda: _dev(attn.get_relative_position_bias(), torch.float32))


def swin_window_attention(qkv: Act, bias: torch.Tensor, heads: int, window, shift, drop=None) -> Act:
    """`drop` = (p, per-sample keys): the reference's `_func_dropout(attn, attention_dropout, key)` (swin.py:227) inside the kernel."""
    B, Hf, Wf, C3 = qkv.t.shape
    C = C3 // 3
    out = empty((B, Hf, Wf, C), qkv.t.dtype)
    if drop is None:
        _lib.call("mv_swin_window_attn_fwd", _ptr(qkv.t), _ptr(bias), _ptr(out), B, Hf, Wf, C, heads,
                  int(window[0]), int(window[1]), int(shift[0]), int(shift[1]), qkv.dt, stream_ptr())
    else:
        p, key = drop
        if not 0.0 < float(p) < 1.0:
            raise NotImplementedError(f"Swin attention_dropout = {p}")
        _lib.call("mv_swin_window_attn_dropout_fwd", _ptr(qkv.t), _ptr(bias), _ptr(out), _ptr(_keys_dev(key, B)), float(1.0 - p),
                  B, Hf, Wf, C, heads, int(window[0]), int(window[1]), int(shift[0]), int(shift[1]), qkv.dt, stream_ptr())
    return Act(out, "map", qkv.batched)


def swin_block_attn_fragments(wqkv: np.ndarray, bqkv: np.ndarray, wp: np.ndarray, bias: np.ndarray):
    """qkv weight [3C][C] (LayerNorm already folded) / bias [3C], proj weight [C][C], relative-position bias [heads][n][n] ->
    the operand layouts of mv_swin_block_attn_fwd (header), or None for a width the kernel is not instantiated for (swin_b's
    128 / 256 / 512 / 1024: the caller takes the un-fused path)."""
    C = wp.shape[0]
    heads = C // 32
    if C not in (384, 192, 96):                           # the widths the kernel is instantiated for (NWIN / NWV templates)
        return None
    HG = {384: 4, 192: 2, 96: 1}[C]                       # heads per group (x windows per workgroup = 4)
    G, GT = heads // HG, 3 * HG                            # always 3 groups; tiles per group: q heads, k heads, v heads
    rows = np.array([[(t // HG) * C + 32 * (HG * g + t % HG) for t in range(GT)] for g in range(G)])              # [G][GT]
    w = wqkv[(rows[:, :, None] + np.arange(32)[None, None, :])]                                                   # [G][GT][32][C]
    wf = w.reshape(G, GT, 32, C // 16, 2, 8).transpose(0, 1, 3, 4, 2, 5)                                           # (g, t, j, h, m, e)
    bf_ = bqkv[(rows[:, :, None] + np.arange(32)[None, None, :])]                                                  # [G][GT][32]
    wpf = wp.reshape(C // 32, 32, C // 16, 2, 8).transpose(0, 2, 3, 1, 4)                                          # (t, j, h, m, e)
    n = bias.shape[1]
    b64 = np.zeros((heads, 64, 64), np.float32)
    b64[:, :, n:] = -1e30
    b64[:, :n, :n] = bias
    return (np.ascontiguousarray(wf, np.float32), np.ascontiguousarray(bf_, np.float32), np.ascontiguousarray(wpf, np.float32), b64)


def swin_block_attention(x: Act, norm, attn) -> Optional[Act]:
    """x + attn(norm(x)) of a Swin block (swin.py:572-578, first line) in ONE launch where the library has the fused per-window
    kernel (stage 2 of swin_t / swin_s), else None."""
    from . import nn
    if compute_dtype() != "bf16" or x.kind != "map" or x.t.dtype != torch.float32 or not isinstance(norm, nn.LayerNorm):
        return None
    if norm.weight is None or norm.bias is None or attn.qkv.bias is None or attn.proj.bias is None:
        return None
    B, Hf, Wf, C = x.t.shape
    ws, sh = attn.window_size, list(attn.shift_size)
    if ws[0] >= Hf:                                                   # reference :116-120: no shift when the window covers the map
        sh[0] = 0
    if ws[1] >= Wf:
        sh[1] = 0
    if attn.qkv.in_features != C or not _lib.load().mv_swin_block_attn_supported(Hf, Wf, C, attn.num_heads, ws[0], ws[1], _lib.F32):
        return None

    def build():
        frags = swin_block_attn_fragments(*_ln_fold(attn.qkv, norm), np.asarray(attn.proj.weight, np.float32),
                                          attn.get_relative_position_bias())
        if frags is None:
            return None
        wf, bq, wpf, b64 = frags
        return (_dev(wf, torch.bfloat16), _dev(bq, torch.float32), _dev(wpf, torch.bfloat16), _dev_bias(attn.proj),
                _dev(b64, torch.float32))
    hit = _prepared(attn, "block_attn", (norm.weight, norm.bias), build)
    if hit is None:
        return None
    y = empty(tuple(x.t.shape), torch.float32)
    _lib.call("mv_swin_block_attn_fwd", _ptr(x.t), _ptr(hit[0]), _ptr(hit[1]), _ptr(hit[2]), _ptr(hit[3]), _ptr(hit[4]), _ptr(y),
              B, Hf, Wf, C, attn.num_heads, ws[0], ws[1], sh[0], sh[1], float(norm.eps), _lib.F32, stream_ptr())
    return Act(y, "map", x.batched)


def dropout_windows(x: Act, p: float, key, window, shift) -> Act:
    """`_func_dropout(x, dropout, key)` on the projection output of `_shifted_window_attention` (swin.py:233): the mask is drawn
    for the (num_windows, tokens, C) layout the reference holds there; x is the NHWC map of the same values."""
    x = as_map(x)
    if not 0.0 < float(p) < 1.0:
        raise NotImplementedError(f"Swin dropout = {p}")
    B, Hf, Wf, C = x.t.shape
    y = empty(tuple(x.t.shape), x.t.dtype)
    _lib.call("mv_dropout_windows_fwd", _ptr(x.t), _ptr(_keys_dev(key, B)), _ptr(y), B, Hf, Wf, C, int(window[0]), int(window[1]),
              int(shift[0]), int(shift[1]), float(1.0 - p), x.dt, stream_ptr())
    return Act(y, "map", x.batched)


# ------------------------------------------------------------------ Swin V2 (models/classification/swin.py, reference :68-87, :144-168, :369-522, :581-635)
def swin_v2_fused() -> bool:
    """Library switch "no_swin_v2_fused": V2 blocks and patch merging on the literal composition (LayerNorm, add and cast launches
    instead of mv_layernorm_add_fwd) -- the A/B of tools/ab_flag.py / tools/time_swin_v2.py and the tests' cross-check."""
    return not _lib.get_flag("no_swin_v2_fused")


def swin_v2_rel_bias_host(table, index, w1, b1, w2, heads: int, window) -> np.ndarray:
    """`_ShiftedWindowAttentionV2.get_relative_position_bias` (reference :486-495) on the host, fp32 numpy: the cpb_mlp
    (transpose, Linear2d(2, 512), relu, Linear2d(512, heads, no bias): :418-426) on the log-spaced coordinate table gives
    (heads, 2Wh-1, 2Ww-1); that array is reshaped RAW to (-1, heads) -- not transposed: the reference mixes heads and positions,
    and so does this -- gathered by the index (negative entries wrap), laid out (heads, n, n) and mapped through 16 * sigmoid."""
    t = np.asarray(table, np.float32).reshape(-1, 2)
    hid = np.maximum(t @ np.asarray(w1, np.float32).T + np.asarray(b1, np.float32).reshape(1, -1), np.float32(0))
    out = np.ascontiguousarray((hid @ np.asarray(w2, np.float32).T).T)          # (heads, (2Wh-1)(2Ww-1)): the MLP's output layout
    raw = out.reshape(-1, heads)                                                # reference :488-490
    n = int(window[0]) * int(window[1])
    idx = np.asarray(index).reshape(-1).astype(np.int64)
    b = np.ascontiguousarray(raw[idx].reshape(n, n, heads).transpose(2, 0, 1))  # reference :34-43
    return (np.float32(16) / (np.float32(1) + np.exp(-b))).astype(np.float32)


def _cpb_linears(attn):
    lins = [m for m in attn.cpb_mlp.layers if hasattr(m, "weight")]
    if len(lins) != 2 or lins[0].bias is None or lins[1].bias is not None:
        raise ValueError("cpb_mlp must be Linear2d(2, hidden) -> relu -> Linear2d(hidden, heads, use_bias=False) (reference :418-426)")
    return lins


def swin_v2_operands(attn):
    """(bias [heads][n][n], logit_mul [heads]) of a _ShiftedWindowAttentionV2 on the device -- weight preprocessing like the
    LayerNorm folding of swin_block_attention -- cached on the module, keyed by the identities of the leaves they are made of."""
    l1, l2 = _cpb_linears(attn)
    leaves = (l1.weight, l1.bias, l2.weight, attn.logit_scale, attn.relative_position_index, attn.relative_position_bias_table)

    def build():
        bias = swin_v2_rel_bias_host(attn.relative_position_bias_table, attn.relative_position_index, l1.weight, l1.bias, l2.weight,
                                     attn.num_heads, attn.window_size)
        ls = np.asarray(attn.logit_scale, np.float32).reshape(-1)
        mul = np.exp(np.minimum(ls, np.float32(np.log(100.0)))).astype(np.float32)       # reference :165-167
        return _dev(bias, torch.float32), _dev(mul, torch.float32)
    return _prepared(attn, "v2_operands", leaves, build)


def swin_v2_rel_bias(attn) -> torch.Tensor:
    return swin_v2_operands(attn)[0]


def swin_v2_qkv(attn):
    """The qkv Linear2d as the reference applies it in the V2 attention: the key third of the bias is zeroed on EVERY call
    (:144-150), whatever the leaf holds (a checkpoint may carry a non-zero one).  A shadow layer sharing the weight, cached on the
    module; the module's own leaf stays as it is."""
    lin = attn.qkv
    if lin.bias is None:
        return lin

    def build():
        from ._module import tree_at
        b = np.array(np.asarray(lin.bias, np.float32))
        n = b.size // 3
        b.reshape(-1)[n:2 * n] = 0
        return tree_at(lambda l: l.bias, lin, b)
    return _prepared(attn, "v2_qkv", (lin.weight, lin.bias), build)


def swin_qk_rnorm(qkv: Act, window, shift) -> torch.Tensor:
    """fp32 [B][2][n][C]: 1 / norm of q and k over the windows of each image (reference :161-163, axis 0)."""
    B, Hf, Wf, C3 = qkv.t.shape
    C = C3 // 3
    rn = empty((B, 2, int(window[0]) * int(window[1]), C), torch.float32)
    _lib.call("mv_swin_qk_rnorm_fwd", _ptr(qkv.t), _ptr(rn), B, Hf, Wf, C, int(window[0]), int(window[1]), int(shift[0]), int(shift[1]),
              qkv.dt, stream_ptr())
    return rn


def swin_window_attention_cos(qkv: Act, rnorm: torch.Tensor, logit_mul: torch.Tensor, bias: torch.Tensor, heads: int, window, shift,
                              drop=None) -> Act:
    """The V2 attention core (reference :159-173, then as V1).  `drop` = (p, per-sample keys): the attention dropout of :227."""
    B, Hf, Wf, C3 = qkv.t.shape
    C = C3 // 3
    out = empty((B, Hf, Wf, C), qkv.t.dtype)
    keys, keep = None, 1.0
    if drop is not None:
        p, key = drop
        if not 0.0 < float(p) < 1.0:
            raise NotImplementedError(f"Swin attention_dropout = {p}")
        keys, keep = _keys_dev(key, B), float(1.0 - p)
    _lib.call("mv_swin_window_attn_cos_fwd", _ptr(qkv.t), _ptr(rnorm), _ptr(logit_mul), _ptr(bias), _ptr(out), _ptr(keys), keep,
              B, Hf, Wf, C, heads, int(window[0]), int(window[1]), int(shift[0]), int(shift[1]), qkv.dt, stream_ptr())
    return Act(out, "map", qkv.batched)


_LO = object()      # Act.pre = (_LO, plane): `plane` holds the same rows rounded once to the compute dtype (mv_layernorm_add_fwd's y_lo)


def stream_plane(x: Act) -> Act:
    """The fp32 stream's rows in the compute dtype: the plane written next to them, or one cast launch."""
    if x.pre is not None and x.pre[0] is _LO:
        return x.pre[1]
    return cast(x, compute_dtype())


def layernorm_add(z: Act, ln, res: Optional[Act] = None) -> Act:
    """res + ln(z) as the fp32 stream (reference :629-635, :83-87), one launch; in bf16 mode the bf16 plane the next Linear reads is
    written by the same launch (`stream_plane`).  With "no_swin_v2_fused": LayerNorm, add, and the consumer's cast."""
    z = as_map(z)
    C = z.t.shape[-1]
    if int(np.prod(ln.shape)) != C or ln.weight is None or ln.bias is None:
        raise ValueError(f"layernorm_add: an affine LayerNorm over {C} channels is required, got {ln.shape}")
    if res is not None and (tuple(res.t.shape) != tuple(z.t.shape) or res.t.dtype != torch.float32):
        raise ValueError(f"layernorm_add: the residual must be the fp32 stream of z's shape: {res} vs {z}")
    if not swin_v2_fused():
        y = layernorm(z, ln, out_fp32=True)
        return y if res is None else add(res, y)
    dt = compute_dtype()
    y = empty(tuple(z.t.shape), torch.float32)
    lo = empty(tuple(z.t.shape), TORCH_DT[dt]) if dt != "fp32" else None
    _lib.call("mv_layernorm_add_fwd", _ptr(z.t), _ptr(None if res is None else res.t), _ptr(prep_f32(ln, "weight", ln.weight)),
              _ptr(prep_f32(ln, "bias", ln.bias)), _ptr(y), _ptr(lo), z.t.numel() // C, C, float(ln.eps), z.dt, DT[dt], stream_ptr())
    out = Act(y, "map", z.batched)
    if lo is not None:
        out.pre = (_LO, Act(lo, "map", z.batched))
    return out


def resize_bilinear(x: Act, size, final: bool = False) -> Act:
    """jax.image.resize(x, (C,) + size, "bilinear") of a feature map (up-sampling).  `final`: the result is what the caller of the
    model receives -> written directly as fp32 NCHW; otherwise an NHWC map in the compute dtype for further layers."""
    x = as_map(x)
    B, h, w, C = x.t.shape
    H, W = int(size[0]), int(size[1])
    if final:
        y = empty((B, C, H, W), torch.float32)
        _lib.call("mv_resize_bilinear_nhwc_fwd", _ptr(x.t), _ptr(y), B, h, w, C, H, W, x.dt, _lib.F32, 1, stream_ptr())
        return Act(y, "img", x.batched)
    if (H, W) == (h, w):
        return x
    y = empty((B, H, W, C), x.t.dtype)
    _lib.call("mv_resize_bilinear_nhwc_fwd", _ptr(x.t), _ptr(y), B, h, w, C, H, W, x.dt, x.dt, 0, stream_ptr())
    return Act(y, "map", x.batched)


def concat_channels(xs) -> Act:
    """jnp.concatenate(maps, axis=0) of (C,H,W) samples == channel concatenation of NHWC maps (deeplabv3.py:132-136)."""
    maps = [as_map(x) for x in xs]
    B, H, W, _ = maps[0].t.shape
    dt = maps[0].t.dtype
    for m in maps:
        if tuple(m.t.shape[:3]) != (B, H, W) or m.t.dtype != dt:
            raise ValueError(f"concat_channels: mismatched maps {[tuple(m.t.shape) for m in maps]}")
    ctot = sum(m.t.shape[3] for m in maps)
    y = empty((B, H, W, ctot), dt)
    es = y.element_size()
    off = 0
    for m in maps:
        c = m.t.shape[3]
        _lib.call("mv_copy_rows", _ptr(m.t), y.data_ptr() + off * es, B * H * W, c * es, c * es, ctot * es, stream_ptr())
        off += c
    return Act(y, "map", maps[0].batched)


def se_scale(x: Act, fc1, fc2, act1, act2) -> Optional[Act]:
    """SqueezeExcitation's scale vector [B, C] (layers/squeeze.py:47-60: mean -> fc1 -> activation -> fc2 -> scale activation) in
    ONE launch, or None when the library has no fused path (caller: avgpool + two convolutions + activations)."""
    x = as_map(x)
    B, H, W, C = x.t.shape
    S = fc1.out_channels
    plain = all(tuple(c.kernel_size) == (1, 1) and tuple(c.stride) == (1, 1) and tuple(c.padding) == (0, 0) and c.groups == 1
                for c in (fc1, fc2))
    if (compute_dtype() != "bf16" or x.t.dtype != torch.bfloat16 or not plain or fc1.in_channels != C or fc2.in_channels != S
            or fc2.out_channels != C or act1 not in ACT or act2 not in ACT or not _lib.load().mv_se_scale_supported(C, S, _lib.BF16)):
        return None
    w1, _, b1 = prep_conv(fc1, None, "krsc", "bf16")
    # [S][C]: the kernel's threads read consecutive channels of a row
    w2, b2 = _prepared(fc2, "se_w2t", (), lambda: (
        _dev(np.ascontiguousarray(np.asarray(fc2.weight, np.float32).reshape(C, S).T), torch.bfloat16), _dev_bias(fc2)))
    s = empty((B, C), torch.bfloat16)
    _lib.call("mv_se_scale_fwd", _ptr(x.t), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(s), B, H * W, C, S, ACT[act1], ACT[act2],
              _lib.BF16, stream_ptr())
    return Act(s, "vec", x.batched)


def channel_scale(x: Act, s: Act) -> Act:
    """x * s with s one value per (image, channel): SqueezeExcitation's last line (layers/squeeze.py:60)."""
    x = as_map(x)
    B, H, W, C = x.t.shape
    st = s.t.reshape(B, -1)
    if st.shape[1] != C:
        raise ValueError(f"channel_scale: scale has {st.shape[1]} channels, the map {C}")
    if st.dtype != x.t.dtype:
        s = cast(Act(st, "vec", s.batched), "bf16" if x.t.dtype == torch.bfloat16 else "fp32")
        st = s.t
    if not st.is_contiguous():          # a temporary copy would not be pinned for the recorded launch list
        raise ValueError("channel_scale: the scale must be a contiguous [B, C] tensor")
    y = empty(tuple(x.t.shape), x.t.dtype)
    _lib.call("mv_channel_scale_nhwc_fwd", _ptr(x.t), _ptr(st), _ptr(y), B, H * W, C, x.dt, stream_ptr())
    return Act(y, "map", x.batched)


def _batched_keys(key, B: int) -> np.ndarray:
    """uint32 [B, 2]: the per-sample keys of a vmapped call; one key [2] serves an un-batched call (B == 1)."""
    k = np.asarray(key, np.uint32)
    if k.ndim == 1 and k.shape[0] == 2 and B == 1:
        k = k[None]
    if k.shape != (B, 2):
        raise ValueError(f"expected one PRNG key per sample, uint32 [{B}, 2]; got {k.shape}")
    return np.ascontiguousarray(k)


def _keys_dev(key, B: int) -> torch.Tensor:
    """int32 [B, 2] on the device: host keys (numpy, one per sample) are uploaded, keys derived on the device pass through."""
    if isinstance(key, torch.Tensor):
        if tuple(key.shape) != (B, 2) or key.dtype != torch.int32 or not key.is_contiguous():
            raise ValueError(f"expected device keys int32 [{B}, 2], got {key.dtype} {tuple(key.shape)}")
        return key
    return torch.from_numpy(_batched_keys(key, B).view(np.int32)).to(device())


def split_keys(keys, num: int):
    """jax.random.split of batched keys [R, 2] -> [num, R, 2] (child i of every key): numpy in, numpy out (random.split); a
    device tensor in, a device tensor out (mv_prng_split) -- what the per-token keys of a transformer MLP go through."""
    if not isinstance(keys, torch.Tensor):
        from . import random as jr
        return jr.split(np.asarray(keys, np.uint32), num)
    R = keys.shape[0]
    out = empty((num, R, 2), torch.int32)
    _lib.call("mv_prng_split", _ptr(_keys_dev(keys, R)), _ptr(out), R, int(num), 1, stream_ptr())
    return out


def token_keys(key, B: int, N: int) -> torch.Tensor:
    """int32 [B*N, 2] on the device: jax.random.split(key, N) of every sample's key, rows in (sample, token) order -- the keys
    `jax.vmap(self.mlp)(y, key=jrandom.split(keys[2], x.shape[0]))` hands the tokens (vit.py:155)."""
    out = empty((B * N, 2), torch.int32)
    _lib.call("mv_prng_split", _ptr(_keys_dev(key, B)), _ptr(out), B, int(N), 0, stream_ptr())
    return out


def dropout(x: Act, p: float, key, per_row: bool = False) -> Act:
    """eqx.nn.Dropout's training branch: where(bernoulli(key, 1 - p, x.shape), x / (1 - p), 0) per sample, the mask from the
    sample's key in JAX's bit stream (generated on the device, rng.hip).  `per_row`: x is (tokens, features) rows and `key`
    holds one key per ROW (uint32 [B*N, 2], `token_keys`): the reference vmaps the layer over the tokens.  A map is always the
    reference's (C, H, W) array (also behind Swin's Linear2d layers, extensions_2d.py:46-50): the kernel maps NHWC positions to it."""
    if x.kind == "img":
        x = as_map(x)
    B = x.t.shape[0]
    C = x.t.shape[-1]
    if per_row:
        if x.kind != "seq":
            raise ValueError(f"per-row dropout expects (tokens, features) rows, got {x.kind} {tuple(x.t.shape)}")
        B = x.t.numel() // C
    keys = _keys_dev(key, B)
    per = x.t.numel() // B
    y = empty(tuple(x.t.shape), x.t.dtype)
    _lib.call("mv_dropout_fwd", _ptr(x.t), _ptr(keys), _ptr(y), B, per, C, 1 if x.kind == "map" else 0,
              float(1.0 - p), x.dt, stream_ptr())
    return Act(y, x.kind, x.batched)


def drop_path(x: Act, p: float, mode: str, key) -> Act:
    """DropPath's training branch (drop_path.py:51-61): noise = bernoulli(key, 1 - p) for the whole sample (mode "global") or one
    draw per entry of the sample's FIRST logical axis (mode "local": channels of a (C,H,W) map, tokens of an (N,D) matrix),
    divided by 1 - p when that is positive; x * noise.  The draws are made on the device from the samples' keys (JAX's bit stream,
    mv_drop_path_noise -> a [B, C] scale); the multiply is the broadcast-scale kernel."""
    if x.kind == "img":
        x = as_map(x)
    B = x.t.shape[0]
    keep = 1.0 - float(p)
    if x.kind == "seq" and mode != "global":
        raise NotImplementedError("DropPath(mode='local') on a (tokens, features) array is not on any model's path")
    C = x.t.shape[-1]
    if keep <= 0.0:                    # p = 1: bernoulli(key, 0) is all False and the reference skips the division
        _keys_dev(key, B)
        s = torch.zeros((B, C), dtype=x.t.dtype, device=device())
    else:
        s = empty((B, C), x.t.dtype)
        _lib.call("mv_drop_path_noise", _ptr(_keys_dev(key, B)), _ptr(s), B, C, 0 if mode == "global" else 1,
                  float(np.float32(keep)), x.dt, stream_ptr())
    xm = x if x.kind == "map" else Act(x.t.reshape(B, -1, 1, C), "map", x.batched)
    y = channel_scale(xm, Act(s, "vec", x.batched))
    return y if x.kind == "map" else Act(y.t.reshape(x.t.shape), x.kind, x.batched)


def patch_merge_ln(x: Act, ln) -> Optional[Act]:
    """norm(_patch_merging_pad(x)) (swin.py:61-65) in one pass over the fp32 map -- the gathered 4C map is never written; None when
    the library has no such path (odd sizes, bf16 stream)."""
    x = as_map(x)
    B, H, W, C = x.t.shape
    dt = compute_dtype()
    if dt != "bf16" or x.t.dtype != torch.float32 or int(np.prod(ln.shape)) != 4 * C or ln.weight is None or ln.bias is None:
        return None
    if not _lib.load().mv_patch_merge_ln_supported(H, W, C, _lib.F32):
        return None
    y = empty((B, H // 2, W // 2, 4 * C), TORCH_DT[dt])
    _lib.call("mv_patch_merge_ln_fwd", _ptr(x.t), _ptr(prep_f32(ln, "weight", ln.weight)), _ptr(prep_f32(ln, "bias", ln.bias)), _ptr(y),
              B, H, W, C, float(ln.eps), _lib.F32, DT[dt], stream_ptr())
    return Act(y, "map", x.batched)


def patch_merge_gather(x: Act) -> Act:
    x = as_map(x)
    B, H, W, C = x.t.shape
    y = empty((B, (H + 1) // 2, (W + 1) // 2, 4 * C), x.t.dtype)
    _lib.call("mv_patch_merge_gather_nhwc", _ptr(x.t), _ptr(y), B, H, W, C, x.dt, stream_ptr())
    return Act(y, "map", x.batched)


# ------------------------------------------------------------------ ConvNeXt block (models/classification/convnext.py)
def prep_dw(conv, bn=None):
    """Depthwise filters (C, 1, R, S) re-laid to [R][S][C] bf16 + folded scale / shift (cached: the "dw" entry conv2d uses)."""
    def build():
        _, scale, shift = prep_conv(conv, bn, "oihw", "bf16")
        wr = np.ascontiguousarray(np.asarray(conv.weight, np.float32)[:, 0].transpose(1, 2, 0))     # (C,1,R,S) -> [R][S][C]
        return _dev(wr, torch.bfloat16), scale, shift
    return _prepared(conv, "dw", (bn,), build)


def _cnblock_layers(blk):
    """(dwconv, norm, fc1, fc2) when the block is the reference's Sequential[Conv2d 7x7 depthwise, LayerNorm, Linear, gelu, Linear]
    with every bias / affine present, else None."""
    from . import nn
    L = getattr(blk.block, "layers", None)
    if L is None or len(L) != 5:
        return None
    dw, ln, fc1, act, fc2 = L
    C = getattr(dw, "in_channels", -1)
    ok = (isinstance(dw, nn.Conv2d) and type(dw) is nn.Conv2d and dw.groups == C == dw.out_channels and tuple(dw.kernel_size) == (7, 7)
          and tuple(dw.stride) == (1, 1) and tuple(dw.padding) == (3, 3) and tuple(dw.dilation) == (1, 1) and dw.bias is not None
          and isinstance(ln, nn.LayerNorm) and ln.weight is not None and ln.bias is not None and int(np.prod(ln.shape)) == C
          and isinstance(fc1, nn.Linear) and isinstance(fc2, nn.Linear) and fc1.bias is not None and fc2.bias is not None
          and fc1.in_features == C and fc2.out_features == C and fc2.in_features == fc1.out_features
          and isinstance(act, nn.Lambda) and nn.act_name(act.fn) == "gelu")
    return (dw, ln, fc1, fc2) if ok else None


def _cnblock_mlp(blk, ln, fc1, fc2, form: str):
    """The block's MLP with the LayerNorm affine folded into fc1 (W1 diag(g), b1 + W1 beta) and layer_scale into fc2 (diag(ls) W2 in
    fp32, then one bf16 rounding; ls * b2).  form "lds" / "lin": row-major; "stream": mv_ln_mlp_stream_fwd's fragment order."""
    def build():
        ls = np.asarray(blk.layer_scale, np.float32).reshape(-1)
        w1f, b1 = _ln_fold(fc1, ln)
        w2f = np.asarray(fc2.weight, np.float32) * ls[:, None]
        if form == "stream":
            w1f, w2f = ln_mlp_fragments(w1f, w2f)
        return _dev(w1f, torch.bfloat16), _dev(b1, torch.float32), _dev(w2f, torch.bfloat16), _dev(_bias(fc2) * ls, torch.float32)
    return _prepared(blk, ("cnb_mlp", form), (ln.weight, ln.bias, fc1.weight, fc1.bias, fc2.weight, fc2.bias, blk.layer_scale), build)


def _cnblock_dw(x: Act, dw, ln, normalize: int, y_dt: str) -> Act:
    B, H, W, C = x.t.shape
    w, _, bias = prep_dw(dw)
    y = empty((B, H, W, C), TORCH_DT[y_dt])
    _lib.call("mv_cnblock_dw_fwd", _ptr(x.t), _ptr(w), _ptr(bias), _ptr(y), B, H, W, C, float(ln.eps), normalize, x.dt, DT[y_dt],
              stream_ptr())
    return Act(y, "map", x.batched)


def convnext_downsample(x: Act, ln, conv) -> Act:
    """conv2x2/2(LayerNorm2d(x)) between ConvNeXt stages (convnext.py:179-193) back onto the fp32 stream.  Even maps: the 2x2 patches
    do not overlap, so the convolution is patch gather + a Linear over 4C, run with split-precision weights and an fp32 store like
    Swin's patch merging (its weight rounding is not damped by a residual add); odd maps: the convolution, then a cast."""
    x = as_map(x)
    B, H, W, C = x.t.shape
    n = layernorm(x, ln)
    if H % 2 or W % 2 or x.t.dtype != torch.float32 or tuple(conv.kernel_size) != (2, 2) or tuple(conv.stride) != (2, 2) \
            or tuple(conv.padding) != (0, 0) or conv.groups != 1:
        return cast(conv2d(n, conv), "fp32") if x.t.dtype == torch.float32 else conv2d(n, conv)

    def build():
        from . import nn
        K = conv.out_channels
        lin = nn.Linear.__new__(nn.Linear)
        w = np.asarray(conv.weight, np.float32)                  # (K, C, dh, dw) -> [K][dw][dh][C]: the gather's (dh, dw) order
        for f, v in (("weight", np.ascontiguousarray(w.transpose(0, 3, 2, 1).reshape(K, 4 * C))), ("bias", _bias(conv)),
                     ("in_features", 4 * C), ("out_features", K), ("use_bias", conv.bias is not None)):
            object.__setattr__(lin, f, v)
        return lin
    return linear_split(patch_merge_gather(n), _prepared(conv, "patch_linear", (), build), out_fp32=True)


def cnblock(x: Act, blk, drop=None) -> Act:
    """x + layer_scale * block(x) (convnext.py:62-72).  `drop` = (DropPath, keys): the training-mode branch (stochastic depth
    between the scale and the residual add), always on the composition of the generic entries.
    Inference, bf16, the fp32 stream:  C = 96 / 192 / 384: mv_cnblock_dw_fwd (normalize 0) + mv_ln_mlp[_stream]_res_fwd (2 launches);
    other widths: mv_cnblock_dw_fwd (normalize 1) + two mv_linear_fwd (3 launches)."""
    x = as_map(x)
    B, H, W, C = x.t.shape
    parts = _cnblock_layers(blk)
    lib = _lib.load()
    if parts is not None and drop is None and compute_dtype() == "bf16" and x.t.dtype in (torch.float32, torch.bfloat16):
        dw, ln, fc1, fc2 = parts
        M, Hd = B * H * W, fc1.out_features
        if x.t.dtype == torch.float32 and lib.mv_ln_mlp_res_supported(M, C, Hd, _lib.BF16) and \
                lib.mv_cnblock_dw_supported(C, H, W, x.dt, _lib.BF16, 0):
            d = _cnblock_dw(x, dw, ln, 0, "bf16")
            w1, b1, w2, b2 = _cnblock_mlp(blk, ln, fc1, fc2, "lds")
            y = empty((B, H, W, C), torch.float32)
            _lib.call("mv_ln_mlp_res_fwd", _ptr(d.t), _ptr(x.t), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(y), M, C, Hd,
                      float(ln.eps), _lib.BF16, stream_ptr())
            return Act(y, "map", x.batched)
        if x.t.dtype == torch.float32 and lib.mv_ln_mlp_stream_res_supported(M, C, Hd, _lib.F32) and \
                lib.mv_cnblock_dw_supported(C, H, W, x.dt, _lib.F32, 0):
            # the stream kernel reads fp32 rows: d is written in fp32 (+8 B per element of d against bf16, in exchange for keeping
            # the 577-line kernel single-typed)
            d = _cnblock_dw(x, dw, ln, 0, "fp32")
            w1, b1, w2, b2 = _cnblock_mlp(blk, ln, fc1, fc2, "stream")
            y = empty((B, H, W, C), torch.float32)
            _lib.call("mv_ln_mlp_stream_res_fwd", _ptr(d.t), _ptr(x.t), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2), _ptr(y), M, C, Hd,
                      float(ln.eps), _lib.F32, stream_ptr())
            return Act(y, "map", x.batched)
        if lib.mv_cnblock_dw_supported(C, H, W, x.dt, _lib.BF16, 1):
            n = _cnblock_dw(x, dw, ln, 1, "bf16")
            w1, b1, w2, b2 = _cnblock_mlp(blk, ln, fc1, fc2, "lin")
            h = empty((B, H, W, Hd), torch.bfloat16)
            _splitk_scratch(M, Hd, C)
            _lib.call("mv_linear_fwd", _ptr(n.t), _ptr(w1), None, _ptr(b1), None, _ptr(h), M, Hd, C, _lib.ACT_GELU_TANH, _lib.BF16,
                      _lib.BF16, stream_ptr())
            y = empty((B, H, W, C), x.t.dtype)
            _splitk_scratch(M, C, Hd)
            _lib.call("mv_linear_fwd", _ptr(h), _ptr(w2), None, _ptr(b2), _ptr(x.t), _ptr(y), M, C, Hd, _lib.ACT_NONE, _lib.BF16,
                      x.dt, stream_ptr())
            return Act(y, "map", x.batched)
    # the composition of the generic entries (the cross-check of the paths above)
    dt = compute_dtype()
    h = blk.block(x if x.t.dtype == TORCH_DT[dt] else cast(x, dt))
    ls = np.broadcast_to(np.asarray(blk.layer_scale, np.float32).reshape(1, -1), (B, C))
    h = channel_scale(h, Act(_dev(ls, h.t.dtype), "vec", x.batched))
    if drop is not None:
        sd, keys = drop
        h = sd(h, key=keys)
    return add(x, h)


# ------------------------------------------------------------------ ShuffleNetV2 unit (models/classification/shufflenetv2.py)
# The FOLDED layout of a unit output with branch width bf: one bf16 NHWC tensor [B, H, W, 2P], P = bf rounded up to SHUFFLE_GRANULE.
# Channels [0, bf) hold the left half L (branch1's output / the pass-through), [P, P + bf) the right half R (branch2's output), every
# other channel is an exact zero.  The reference's tensor after its channel shuffle is logical[2i] = L[i], logical[2i + 1] = R[i], so
# logical channel j sits at physical channel j // 2 (even j) or P + j // 2 (odd j): the shuffle, the split and the concatenation
# become permutations of the NEXT unit's weight columns and nothing is launched for them.  A layout is None (plain channels) or the
# pair (bf, P).
# The granule is 8: the kernel needs 16-byte channel chunks, and pads its own operands further on the inside (the k-step 32 and the
# 16-row tile of v_mfma_f32_16x16x32_bf16: zeros in LDS and in the packed weight, never in HBM).
SHUFFLE_GRANULE = 8


def shuffle_layout(bf: int):
    return (int(bf), (int(bf) + SHUFFLE_GRANULE - 1) // SHUFFLE_GRANULE * SHUFFLE_GRANULE)


def shuffle_phys_index(C: int, layout) -> np.ndarray:
    """The physical channel of every logical channel of a C-channel tensor kept in `layout`."""
    j = np.arange(C)
    if layout is None:
        return j
    bf, P = layout
    if C != 2 * bf:
        raise ValueError(f"a folded tensor of branch width {bf} has {2 * bf} logical channels, not {C}")
    return np.where(j % 2 == 0, j // 2, P + j // 2)


def _shuffle_parts(unit):
    """((dw, bn, pw, bn) of branch1 or None, (pw1, bn, dw, bn, pw2, bn) of branch2) when the unit is the reference's pair of
    Sequentials (shufflenetv2.py:44-112), else None."""
    from . import nn

    def conv_bn(L, i, dw):
        c, b = L[i], L[i + 1]
        ok = type(c) is nn.Conv2d and isinstance(b, nn.BatchNorm) and c.bias is None and tuple(c.dilation) == (1, 1)
        if dw:
            return ok and c.groups == c.in_channels == c.out_channels and tuple(c.kernel_size) == (3, 3) and tuple(c.padding) == (1, 1) \
                and tuple(c.stride) == (unit.stride, unit.stride)
        return ok and _pointwise(c)

    def relu(L, i):
        return isinstance(L[i], nn.Lambda) and nn.act_name(L[i].fn) == "relu"

    L1, L2 = getattr(unit.branch1, "layers", None), getattr(unit.branch2, "layers", None)
    if L1 is None or L2 is None or len(L2) != 8 or unit.stride not in (1, 2):
        return None
    if not (conv_bn(L2, 0, False) and relu(L2, 2) and conv_bn(L2, 3, True) and conv_bn(L2, 5, False) and relu(L2, 7)):
        return None
    b2 = (L2[0], L2[1], L2[3], L2[4], L2[5], L2[6])
    if not (b2[0].out_channels == b2[2].in_channels == b2[4].in_channels == b2[4].out_channels):
        return None
    if unit.stride == 1:
        return (None, b2)
    if len(L1) != 5 or not (conv_bn(L1, 0, True) and conv_bn(L1, 2, False) and relu(L1, 4)) or L1[2].out_channels != b2[4].out_channels \
            or L1[0].out_channels != L1[2].in_channels:
        return None
    return ((L1[0], L1[1], L1[2], L1[3]), b2)


def _place(v: np.ndarray, pos: np.ndarray, size: int, axis: int = -1) -> np.ndarray:
    """zeros of `size` along `axis` with v's entries at `pos`."""
    v = np.moveaxis(np.asarray(v, np.float32), axis, -1)
    out = np.zeros(v.shape[:-1] + (size,), np.float32)
    out[..., pos] = v
    return np.moveaxis(out, -1, axis)


def _shuffle_tail_fold(dw, bn_d, pw, bn_p, pos: np.ndarray, Cx: int, P: int):
    """depthwise 3x3 + BN -> 1x1 + BN (+ relu) over a physical input of Cx channels whose logical channel j sits at pos[j]:
    (dw weight [3][3][Cx], dw scale, dw shift [Cx], 1x1 weight [P][Cx], scale, shift [P]); zeros at every pad."""
    wd = np.asarray(dw.weight, np.float32)[:, 0].transpose(1, 2, 0)                      # (C,1,3,3) -> [3][3][C]
    sd, hd = _fold(dw, bn_d)
    wp = np.asarray(pw.weight, np.float32).reshape(pw.out_channels, pw.in_channels)
    sp, hp = _fold(pw, bn_p)
    rows = np.arange(pw.out_channels)
    return (_place(wd, pos, Cx), _place(sd, pos, Cx), _place(hd, pos, Cx), _place(_place(wp, pos, Cx), rows, P, axis=0),
            _place(sp, rows, P), _place(hp, rows, P))


def shuffle_fold_unit(unit, layout_in, C_in: int):
    """One ShuffleNetV2 unit as fp32 numpy operands on the folded layout (no device): what ops.shuffle_unit uploads and what
    shuffle_unit_numpy applies.  `layout_in` / `C_in`: the layout and the LOGICAL channel count of the unit input.  None when the unit
    is not the reference's structure (or a stride-1 unit on a plain input, which the reference's networks never have)."""
    parts = _shuffle_parts(unit)
    if parts is None or (unit.stride == 1 and layout_in is None):
        return None
    b1, b2 = parts
    bf, P = shuffle_layout(b2[4].out_channels)
    idx = shuffle_phys_index(C_in, layout_in)
    Cp = C_in if layout_in is None else 2 * layout_in[1]
    pw1 = b2[0]
    if unit.stride == 1:
        if layout_in != (bf, P) or pw1.in_channels != bf or C_in != 2 * bf:
            return None
        cols = idx[bf:]                                    # branch2 reads logical[bf:2bf]
    else:
        if pw1.in_channels != C_in or b1[0].in_channels != C_in:
            return None
        cols = idx
    w1 = np.asarray(pw1.weight, np.float32).reshape(bf, -1)
    s1, h1 = _fold(pw1, b2[1])
    rows = np.arange(bf)
    F = dict(stride=unit.stride, bf=bf, P=P, Cp=Cp, layout_in=layout_in,
             pw1=(_place(_place(w1, cols, Cp), rows, P, axis=0), _place(s1, rows, P), _place(h1, rows, P)),
             tail2=_shuffle_tail_fold(b2[2], b2[3], b2[4], b2[5], rows, P, P),
             tail1=None if b1 is None else _shuffle_tail_fold(b1[0], b1[1], b1[2], b1[3], idx, Cp, P))
    return F


def shuffle_fold_head(conv, bn, layout_in):
    """conv5 (1x1 + BN + relu) on a folded input: (weight [K][Cp] with permuted columns, scale, shift), fp32 numpy."""
    C = conv.in_channels
    idx = shuffle_phys_index(C, layout_in)
    Cp = C if layout_in is None else 2 * layout_in[1]
    s, h = _fold(conv, bn)
    return _place(np.asarray(conv.weight, np.float32).reshape(conv.out_channels, C), idx, Cp), s, h


def _np_dw3x3(x: np.ndarray, w: np.ndarray, stride: int) -> np.ndarray:
    """[H][W][C] depthwise 3x3, pad 1, fp32 numpy."""
    H, W, C = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    xp = np.zeros((H + 2, W + 2, C), np.float32)
    xp[1:-1, 1:-1] = x
    y = np.zeros((Ho, Wo, C), np.float32)
    for r in range(3):
        for s in range(3):
            y += xp[r:r + stride * (Ho - 1) + 1:stride, s:s + stride * (Wo - 1) + 1:stride] * w[r, s]
    return y


def shuffle_unit_numpy(x: np.ndarray, F) -> np.ndarray:
    """A whole folded unit in fp32 numpy: physical [H][W][Cp] in, physical [Ho][Wo][2P] out -- the algebra of the device path
    (first 1x1 with permuted columns; depthwise + 1x1 tails; the pass-through as an index), launch for launch."""
    x = np.asarray(x, np.float32)
    P, bf, s = F["P"], F["bf"], F["stride"]

    def tail(t, T):
        d = _np_dw3x3(t, T[0], s) * T[1] + T[2]
        return np.maximum(d @ T[3].T * T[4] + T[5], 0.0).astype(np.float32)

    w1, s1, h1 = F["pw1"]
    t1 = np.maximum(x @ w1.T * s1 + h1, 0.0).astype(np.float32)
    y = np.zeros(((x.shape[0] - 1) // s + 1, (x.shape[1] - 1) // s + 1, 2 * P), np.float32)
    y[..., P:] = tail(t1, F["tail2"])
    if s == 1:
        y[..., :bf] = x[..., shuffle_phys_index(2 * bf, F["layout_in"])[:bf]]
    else:
        y[..., :P] = tail(x, F["tail1"])
    return y


def dwpw_fragments(w: np.ndarray) -> np.ndarray:
    """A [N][Cx] 1x1 weight in the A-fragment order of mv_shuffle_dwpw_fwd (header): [Np / 16][Kp / 32][lane 64][8], lane
    16 g + r = W[16 tile + r][32 step + 8 g ..], zero rows / columns up to Np = N rounded up to 16 and Kp = Cx rounded up to 32.
    (The packer of the boundary chains, _res_fragments, lays out 32-row tiles of TWO matrices per chunk for v_mfma_f32_32x32x16:
    16-row tiles keep the padding of the half-widths 24 .. 488 at 16 instead of 32.)"""
    N, K = w.shape
    Np, Kp = (N + 15) // 16 * 16, (K + 31) // 32 * 32
    wp = np.zeros((Np, Kp), np.float32)
    wp[:N, :K] = w
    return np.ascontiguousarray(wp.reshape(Np // 16, 16, Kp // 32, 4, 8).transpose(0, 2, 3, 1, 4))


def channel_gather(x: Act, idx: torch.Tensor) -> Act:
    """y[..., j] = x[..., idx[j]] over the channel (last) axis; idx: device int32.  bf16 / fp32, any channel count."""
    x = as_map(x) if x.kind in ("img", "map") else x
    C, Co = x.t.shape[-1], idx.numel()
    y = empty(tuple(x.t.shape[:-1]) + (Co,), x.t.dtype)
    _lib.call("mv_channel_gather_nhwc_fwd", _ptr(x.t), _ptr(idx), _ptr(y), x.t.numel() // C, C, Co, x.dt, stream_ptr())
    return Act(y, x.kind, x.batched)


def _gather_index(mod, name, idx: np.ndarray) -> torch.Tensor:
    return _prepared(mod, ("gather", name), (), lambda: _dev(np.asarray(idx, np.int32), torch.int32))


def _channel_slice(x: Act, c0: int, c1: int) -> Act:
    B, H, W, C = x.t.shape
    y = empty((B, H, W, c1 - c0), x.t.dtype)
    es = y.element_size()
    _lib.call("mv_copy_rows", x.t.data_ptr() + c0 * es, _ptr(y), B * H * W, (c1 - c0) * es, C * es, (c1 - c0) * es, stream_ptr())
    return Act(y, "map", x.batched)


def shuffle_unit_literal(x: Act, unit) -> Act:
    """The reference's unit on the logical layout (shufflenetv2.py:104-112): split, branches, concatenate, channel shuffle."""
    x = as_map(x)
    C = x.t.shape[-1]
    if unit.stride == 1:
        out = concat_channels([_channel_slice(x, 0, C // 2), unit.branch2(_channel_slice(x, C // 2, C))])
    else:
        out = concat_channels([unit.branch1(x), unit.branch2(x)])
    Co = out.t.shape[-1]
    j = np.arange(Co)
    return channel_gather(out, _gather_index(unit, "shuffle", (j % 2) * (Co // 2) + j // 2))     # _channel_shuffle(out, 2)


def _shuffle_operands(unit, layout_in, C_in: int):
    """shuffle_fold_unit's operands on the device (cached on the unit, keyed by its BatchNorms' statistics), or None."""
    parts = _shuffle_parts(unit)
    if parts is None:
        return None

    def build():
        F = shuffle_fold_unit(unit, layout_in, C_in)
        if F is None:
            return None

        def tail(T):
            return (_dev(T[0], torch.bfloat16), _dev(T[1], torch.float32), _dev(T[2], torch.float32),
                    _dev(dwpw_fragments(T[3]), torch.bfloat16), _dev(T[4], torch.float32), _dev(T[5], torch.float32))
        w1, s1, h1 = F["pw1"]
        return dict(F, pw1=(_dev(w1, torch.bfloat16), _dev(s1, torch.float32), _dev(h1, torch.float32)), tail2=tail(F["tail2"]),
                    tail1=None if F["tail1"] is None else tail(F["tail1"]))
    return _prepared(unit, ("shuffle_fold", layout_in, C_in), [m for br in parts if br is not None for m in br[1::2]], build)


def _conv1x1_folded(x: Act, w: torch.Tensor, scale: torch.Tensor, shift: torch.Tensor, K: int) -> Act:
    """relu(scale * (w . x) + shift) with a prepared [K][C] weight: the ordinary NHWC convolution entry."""
    B, H, W, C = x.t.shape
    y = empty((B, H, W, K), torch.bfloat16)
    _splitk_scratch(B * H * W, K, C)
    _lib.call("mv_conv2d_nhwc_fwd", _ptr(x.t), _ptr(w), _ptr(scale), _ptr(shift), None, _ptr(y), B, H, W, C, K, 1, 1, 1, 1, 0, 0, 1, 1, 1,
              _lib.ACT_RELU, _lib.BF16, _lib.BF16, stream_ptr())
    return Act(y, "map", x.batched)


def shuffle_unfold(x: Act, layout, mod) -> Act:
    """Folded -> logical channels (one gather); a plain tensor passes through."""
    if layout is None:
        return x
    return channel_gather(x, _gather_index(mod, ("unfold", layout), shuffle_phys_index(2 * layout[0], layout)))


def shuffle_unit(x: Act, unit, layout_in):
    """One ShuffleNetV2 unit -> (output, its layout).  bf16 inference where mv_shuffle_dwpw_fwd has the shapes: the folded layout,
    2 launches at stride 1 (first 1x1; depthwise + 1x1 + pass-through), 3 at stride 2 (branch1's depthwise + 1x1; first 1x1;
    branch2's depthwise + 1x1).  Otherwise (fp32 mode, training-mode BatchNorm, the switches "no_shuffle_dwpw" / "force_generic",
    shapes without a kernel): the literal composition on logical channels."""
    x = as_map(x)
    B, H, W, Cphys = x.t.shape
    C_in = Cphys if layout_in is None else 2 * layout_in[0]
    parts = _shuffle_parts(unit)
    F = None
    if compute_dtype() == "bf16" and x.t.dtype == torch.bfloat16 and parts is not None and \
            not any(_bn_training(m) for br in parts if br is not None for m in br[1::2]):
        s = unit.stride
        bf, P = shuffle_layout(parts[1][4].out_channels)
        lib = _lib.load()
        if lib.mv_shuffle_dwpw_supported(P, P, s, H, W, _lib.BF16, _lib.BF16) and \
                (s == 1 or lib.mv_shuffle_dwpw_supported(Cphys, P, s, H, W, _lib.BF16, _lib.BF16)):
            F = _shuffle_operands(unit, layout_in, C_in)
    if F is None:
        return shuffle_unit_literal(shuffle_unfold(x, layout_in, unit), unit), None
    s, bf, P = F["stride"], F["bf"], F["P"]
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    y = empty((B, Ho, Wo, 2 * P), torch.bfloat16)
    st = stream_ptr()
    if s == 2:
        T = F["tail1"]
        _lib.call("mv_shuffle_dwpw_fwd", _ptr(x.t), *[_ptr(t) for t in T], _ptr(y), 2 * P, 0, P, bf, None, 0, 0, 0, 0, 0,
                  B, H, W, Cphys, s, _lib.BF16, _lib.BF16, st)
    t1 = _conv1x1_folded(x, *F["pw1"], P)
    T = F["tail2"]
    src = (_ptr(x.t), Cphys, layout_in[1], bf, 0, P) if s == 1 else (None, 0, 0, 0, 0, 0)
    _lib.call("mv_shuffle_dwpw_fwd", _ptr(t1.t), *[_ptr(t) for t in T], _ptr(y), 2 * P, P, P, bf, *src, B, H, W, P, s, _lib.BF16,
              _lib.BF16, st)
    return Act(y, "map", x.batched), (bf, P)


def shuffle_head(x: Act, conv, bn, layout_in) -> Act:
    """conv5 + BatchNorm + relu (shufflenetv2.py:196-210) on a folded input: its weight columns permuted, the ordinary 1x1 path."""
    if layout_in is None:
        return conv2d(x, conv, bn, "relu")
    if compute_dtype() != "bf16" or _bn_training(bn) or not _pointwise(conv) or conv.out_channels % 8:
        return conv2d(shuffle_unfold(x, layout_in, conv), conv, bn, "relu")

    def build():
        w, s, h = shuffle_fold_head(conv, bn, layout_in)
        return _dev(w, torch.bfloat16), _dev(s, torch.float32), _dev(h, torch.float32)
    hit = _prepared(conv, ("shuffle_head", layout_in), (bn,), build)
    return _conv1x1_folded(as_map(x), *hit, conv.out_channels)


# ------------------------------------------------------------------ SqueezeNet Fire module (fire_expand.hip)
FIRE_S64_LITERAL_PIXELS = 256 * 512      # the pixel count from which mv_fire_expand_fwd uses its 256-pixel tile
FIRE_TILE_ROW = 16 * ((np.arange(32) >> 2) & 1) + 4 * (np.arange(32) >> 3) + (np.arange(32) & 3)     # csrc/flat3x3.h: mfma32_tile_row


def fire_fragments(w: np.ndarray) -> np.ndarray:
    """An [E][S][kh][kw] expand weight (1x1 or 3x3) in the A-fragment order of mv_fire_expand_fwd: with Wk[n][k],
    k = (3 r + s) * S + c, the array [E / 32][K / 16][lane 64][8] holds Wk[32 tile + chan(lane % 32)][16 step + 8 (lane / 32) + e],
    chan = FIRE_TILE_ROW (why: csrc/flat3x3.h).  E % 32 == 0 and S % 16 == 0: nothing is padded."""
    E, S, kh, kw = w.shape
    K = kh * kw * S
    if E % 32 or S % 16:
        raise ValueError(f"fire_fragments: E={E} (multiple of 32), S={S} (multiple of 16)")
    wk = np.asarray(w, np.float32).transpose(0, 2, 3, 1).reshape(E // 32, 32, K // 16, 2, 8)[:, FIRE_TILE_ROW]
    return np.ascontiguousarray(wk.transpose(0, 2, 3, 1, 4).reshape(E // 32, K // 16, 64, 8))


def _fire_conv(x: Act, conv, lam) -> Act:
    from .nn import act_name
    a = act_name(lam.fn)
    return conv2d(x, conv, None, a) if a is not None else lam(conv2d(x, conv))


def fire_literal(x: Act, fire) -> Act:
    """The reference's Fire (squeezenet.py:45-53): three convolutions with their activations and the concatenation."""
    t = _fire_conv(as_map(x), fire.squeeze, fire.squeeze_activation)
    return concat_channels([_fire_conv(t, fire.expand1x1, fire.expand1x1_activation),
                            _fire_conv(t, fire.expand3x3, fire.expand3x3_activation)])


def _fire_plain(fire) -> bool:
    """The module the fused kernel computes: 1x1 and 3x3 (pad 1) dense stride-1 convolutions on one input, ReLU after each."""
    from .nn import Conv2d, Lambda, act_name
    e1, e3 = fire.expand1x1, fire.expand3x3
    if not (type(fire.squeeze) is Conv2d and type(e1) is Conv2d and type(e3) is Conv2d):
        return False
    if not all(isinstance(a, Lambda) and act_name(a.fn) == "relu"
               for a in (fire.squeeze_activation, fire.expand1x1_activation, fire.expand3x3_activation)):
        return False
    one = (1, 1)
    return (e1.kernel_size == one and e1.padding == (0, 0) and e3.kernel_size == (3, 3) and e3.padding == one
            and all(c.stride == one and c.dilation == one and c.groups == 1 for c in (e1, e3))
            and e1.in_channels == e3.in_channels == fire.squeeze.out_channels)


def fire(x: Act, mod) -> Act:
    """One Fire module.  bf16 inference where mv_fire_expand_fwd has the shape: the squeeze as the ordinary fused convolution, then
    both expand convolutions, their ReLUs and the concatenation in one launch (2 launches).  Otherwise (fp32 mode, the switches
    "no_fire_expand" / "force_generic", other shapes or activations): the literal composition."""
    x = as_map(x)
    B, H, W, _ = x.t.shape
    if not (compute_dtype() == "bf16" and x.t.dtype == torch.bfloat16 and _fire_plain(mod)):
        return fire_literal(x, mod)
    S, E1, E3 = mod.squeeze.out_channels, mod.expand1x1.out_channels, mod.expand3x3.out_channels
    if not _lib.load().mv_fire_expand_supported(S, E1, E3, H, W, _lib.BF16, _lib.BF16):
        return fire_literal(x, mod)
    if S == 64 and B * H * W >= FIRE_S64_LITERAL_PIXELS and not _lib.get_flag("fire_expand_always"):
        # measured: 64 -> 256 + 256 on 27 x 27 maps at 256 images is the one Fire of both networks where the
        # composition beats the fused launch (by 5 - 8 %); it stays on the composition
        return fire_literal(x, mod)
    ops_ = _prepared(mod, "fire_expand", (), lambda: (
        _dev(fire_fragments(np.asarray(mod.expand1x1.weight, np.float32)), torch.bfloat16), _dev_bias(mod.expand1x1),
        _dev(fire_fragments(np.asarray(mod.expand3x3.weight, np.float32)), torch.bfloat16), _dev_bias(mod.expand3x3)))
    t = conv2d(x, mod.squeeze, None, "relu")
    y = empty((B, H, W, E1 + E3), torch.bfloat16)
    _lib.call("mv_fire_expand_fwd", _ptr(t.t), _ptr(ops_[0]), _ptr(ops_[1]), _ptr(ops_[2]), _ptr(ops_[3]), _ptr(y), B, H, W, S, E1, E3,
              _lib.BF16, _lib.BF16, stream_ptr())
    return Act(y, "map", x.batched)


# ------------------------------------------------------------------ GoogLeNet Inception module (conv1x1_split.hip, inception_pair.hip)
def inception_fragments(w: np.ndarray, s_pad: Optional[int] = None) -> np.ndarray:
    """An [N][S][3][3] filter in the A-fragment order of mv_conv3x3_pair_fwd (csrc/flat3x3.h): `fire_fragments` of the filter with its input
    channels padded by zero columns to `s_pad` (the reduce map's slice is 16-channel aligned) and its output rows padded by zero rows
    to a multiple of 32 (N is a multiple of 16: the upper half of the last tile may not exist)."""
    N, S, kh, kw = w.shape
    Sp = S if s_pad is None else int(s_pad)
    if N % 16 or Sp % 16 or Sp < S:
        raise ValueError(f"inception_fragments: N={N} (multiple of 16), S={S} padded to {Sp} (multiple of 16)")
    wp = np.zeros(((N + 31) // 32 * 32, Sp, kh, kw), np.float32)
    wp[:N, :S] = np.asarray(w, np.float32)
    return fire_fragments(wp)


def inception_stack(parts):
    """The merged pointwise convolution: `parts` = [(w [n][C][1][1], scale [n], shift [n])] -> (W [N][C], scale [N], shift [N], the
    parts' first rows), every part padded to a multiple of 16 rows with zero filters, zero scale and zero shift (a padded column
    computes relu(0 * acc + 0) = 0)."""
    C = parts[0][0].shape[1]
    rows, sc, sh, starts = [], [], [], []
    n = 0
    for w, s, h in parts:
        k = w.shape[0]
        kp = (k + 15) // 16 * 16
        wp, sp, hp = np.zeros((kp, C), np.float32), np.zeros((kp,), np.float32), np.zeros((kp,), np.float32)
        wp[:k], sp[:k], hp[:k] = np.asarray(w, np.float32).reshape(k, C), s, h
        rows.append(wp), sc.append(sp), sh.append(hp), starts.append(n)
        n += kp
    return np.concatenate(rows), np.concatenate(sc), np.concatenate(sh), starts


def _inception_units(mod):
    """(branch1, 3x3 reduce, 3x3, "5x5" reduce, "5x5", pool projection) when `mod` is the reference's module built from BasicConv2d
    units (1x1 / 3x3 pad 1, stride 1, dense) with the 3x3 stride-1 pad-1 max pool in branch 4, else None."""
    from .nn import Conv2d, BatchNorm, MaxPool2d, Sequential
    from .models.classification.googlenet import BasicConv2d
    b2, b3, b4 = mod.branch2, mod.branch3, mod.branch4
    if not all(isinstance(b, Sequential) and len(b.layers) == 2 for b in (b2, b3, b4)):
        return None
    pool = b4.layers[0]
    units = (mod.branch1, b2.layers[0], b2.layers[1], b3.layers[0], b3.layers[1], b4.layers[1])
    if not (type(pool) is MaxPool2d and pool.kernel_size == (3, 3) and pool.stride == (1, 1) and pool.padding == (1, 1)):
        return None
    one = (1, 1)
    for u, k in zip(units, (1, 1, 3, 1, 3, 1)):
        if not (type(u) is BasicConv2d and type(u.conv) is Conv2d and type(u.bn) is BatchNorm):
            return None
        c = u.conv
        if not (c.kernel_size == (k, k) and c.padding == (k // 2, k // 2) and c.stride == one and c.dilation == one and c.groups == 1
                and c.bias is None):
            return None
    C = units[0].conv.in_channels
    if not (units[1].conv.in_channels == units[3].conv.in_channels == units[5].conv.in_channels == C
            and units[2].conv.in_channels == units[1].conv.out_channels and units[4].conv.in_channels == units[3].conv.out_channels):
        return None
    return units


def _inception_pool(x: Act, pool) -> Act:
    from .nn import MaxPool2d
    if type(pool) is MaxPool2d and pool.stride == (1, 1):
        return maxpool2d(x, pool.kernel_size, pool.stride, pool.padding)    # at stride 1 ceil mode never grows the output
    return pool(x)


def inception_literal(x: Act, mod) -> Act:
    """The reference's module (googlenet.py:229-237): four branches and the concatenation.  BatchNorm ignores its key."""
    x = as_map(x)
    b4 = mod.branch4
    from .nn import Sequential
    p4 = b4.layers[1](_inception_pool(x, b4.layers[0])) if isinstance(b4, Sequential) and len(b4.layers) == 2 else b4(x)
    return concat_channels([mod.branch1(x), mod.branch2(x), mod.branch3(x), p4])


# (C_in, H) of module shapes kept on the composition because the 4-launch path measured slower there; the switch
# "inception_always" overrides it for measurements
INCEPTION_LITERAL_SHAPES = frozenset()


def inception(x: Act, mod) -> Act:
    """One Inception module.  bf16 inference where the two kernels have the shapes: 4 launches and no concatenation -- the merged
    1x1 (branch 1 into its slice of the output, the two reduce maps into the scratch map t), the stride-1 max pool, the pool
    projection into its slice, both 3x3 convolutions into theirs.  Otherwise (fp32 mode, training-mode BatchNorm, the switches
    "no_inception_fused" / "force_generic", other module structures or shapes): the literal composition."""
    x = as_map(x)
    B, H, W, C = x.t.shape
    units = _inception_units(mod) if compute_dtype() == "bf16" and x.t.dtype == torch.bfloat16 else None
    if units is None or any(_bn_training(u.bn) for u in units) or C != units[0].conv.in_channels:
        return inception_literal(x, mod)
    c1, c3r, c3, c5r, c5, cp = (u.conv.out_channels for u in units)
    c5p = (c5r + 15) // 16 * 16
    lt, Ct = c3r + c5p, c1 + c3 + c5 + cp
    lib, BF = _lib.load(), _lib.BF16
    if not (lib.mv_conv1x1_split_supported(C, c1 + lt, c1, Ct, 0, lt, 0, BF, BF)
            and lib.mv_conv1x1_split_supported(C, cp, cp, Ct, c1 + c3 + c5, 0, 0, BF, BF)
            and lib.mv_conv3x3_pair_supported(c3r, c5p, c3, c5, H, W, BF, BF)):
        return inception_literal(x, mod)
    if (C, H) in INCEPTION_LITERAL_SHAPES and H == W and not _lib.get_flag("inception_always"):
        return inception_literal(x, mod)

    def build():
        f = [(np.asarray(u.conv.weight, np.float32),) + bn_fold(u.bn) for u in units]
        wm, sm, hm, _ = inception_stack([f[0], f[1], f[3]])
        d32 = lambda a: _dev(a, torch.float32)
        return dict(merged=(_dev(wm, torch.bfloat16), d32(sm), d32(hm)),
                    proj=(_dev(f[5][0].reshape(cp, C), torch.bfloat16), d32(f[5][1]), d32(f[5][2])),
                    w3=(_dev(inception_fragments(f[2][0]), torch.bfloat16), d32(f[2][1]), d32(f[2][2])),
                    w5=(_dev(inception_fragments(f[4][0], c5p), torch.bfloat16), d32(f[4][1]), d32(f[4][2])))
    hit = _prepared(mod, "inception", [u.bn for u in units], build)
    M, st = B * H * W, stream_ptr()
    y = empty((B, H, W, Ct), torch.bfloat16)
    t = empty((B, H, W, lt), torch.bfloat16)
    w, s, h = hit["merged"]
    _lib.call("mv_conv1x1_split_fwd", _ptr(x.t), _ptr(w), _ptr(s), _ptr(h), _ptr(y), Ct, 0, _ptr(t), lt, 0, M, C, c1 + lt, c1, BF, BF, st)
    p = maxpool2d(x, 3, 1, 1)
    w, s, h = hit["proj"]
    _lib.call("mv_conv1x1_split_fwd", _ptr(p.t), _ptr(w), _ptr(s), _ptr(h), _ptr(y), Ct, c1 + c3 + c5, None, 0, 0, M, C, cp, cp, BF, BF, st)
    (w3, s3, h3), (w5, s5, h5) = hit["w3"], hit["w5"]
    _lib.call("mv_conv3x3_pair_fwd", _ptr(t), lt, 0, c3r, c3r, c5p, _ptr(w3), _ptr(s3), _ptr(h3), _ptr(w5), _ptr(s5), _ptr(h5), _ptr(y), Ct,
              c1, c3, c1 + c3, c5, B, H, W, BF, BF, st)
    return Act(y, "map", x.batched)


# ------------------------------------------------------------------ DenseNet dense blocks and transitions (preact1x1.hip, conv3x3_slice.hip)
def _bn_act(x: Act, bn, lam) -> Act:
    from .nn import act_name
    a = act_name(getattr(lam, "fn", None))
    return batchnorm(x, bn, a) if a is not None else lam(batchnorm(x, bn))


def dense_layer_literal(feats, layer, key=None) -> Act:
    """The reference's dense layer (densenet.py:55-67) on the list of earlier features: concatenate, BatchNorm + ReLU, 1x1, BatchNorm
    + ReLU (folded behind the 1x1 in inference: the ordinary fused convolution), 3x3, Dropout."""
    from .nn import act_name, dropout_live
    cat = as_map(feats[0]) if len(feats) == 1 else concat_channels(feats)
    a = _bn_act(cat, layer.norm1, layer.relu)
    if act_name(getattr(layer.relu, "fn", None)) == "relu":
        t = conv2d(a, layer.conv1, layer.norm2, "relu")
    else:
        t = layer.relu(conv2d(a, layer.conv1, layer.norm2))
    new = conv2d(t, layer.conv2)
    if dropout_live(layer.dropout):
        if key is None:
            raise RuntimeError("Dropout requires a key when running in non-deterministic mode.")
        new = layer.dropout(new, key=key)
    return new


def dense_block_literal(x: Act, block, key=None) -> Act:
    """The reference's block (densenet.py:97-103): every layer sees the concatenation of everything before it; the block's key is
    split over its layers and a layer's Dropout draws from its key as given."""
    from .nn import dropout_live
    from . import random as jr
    feats = [as_map(x)]
    n = len(block.layers)
    live = any(dropout_live(getattr(l, "dropout", None)) for l in block.layers)
    keys = jr.split(_batched_keys(key, feats[0].t.shape[0]), n) if live and key is not None else [None] * n
    for i, layer in enumerate(block.layers):
        feats.append(dense_layer_literal(feats, layer, keys[i]))
    return concat_channels(feats)


def _transition_parts(trans):
    """(BatchNorm, relu Lambda, 1x1 convolution, pool) of the reference's transition, else None."""
    from .nn import AvgPool2d, BatchNorm, Conv2d, Lambda, Sequential
    seq = getattr(trans, "layers", None)
    if not (isinstance(seq, Sequential) and len(seq.layers) == 4):
        return None
    bn, lam, conv, pool = seq.layers
    if not (type(bn) is BatchNorm and isinstance(lam, Lambda) and type(conv) is Conv2d and type(pool) is AvgPool2d):
        return None
    return bn, lam, conv, pool


def dense_transition_literal(x: Act, trans, key=None) -> Act:
    """The reference's transition (densenet.py:116-133): BatchNorm + ReLU, the 1x1 convolution, the 2 x 2 average."""
    parts = _transition_parts(trans)
    if parts is None:
        return trans.layers(as_map(x), key=key)
    bn, lam, conv, pool = parts
    return pool(conv2d(_bn_act(as_map(x), bn, lam), conv))


def _plain_conv(c, k: int) -> bool:
    one = (1, 1)
    return (c.kernel_size == (k, k) and c.padding == (k // 2, k // 2) and c.stride == one and c.dilation == one and c.groups == 1
            and c.bias is None)


# (C0, layers, growth, H) of blocks kept on the composition because the two-launch layers measured slower there; the
# switch "dense_always" overrides it for measurements
DENSE_LITERAL_SHAPES = frozenset()


def dense_block_plan(block, C0: int, H: int, W: int):
    """(mid, growth, total channels) when `block` is the reference's structure on C0 input channels, in bf16 inference, and both
    kernels have every layer's shape -- the block then runs as two launches per layer in one buffer; else None (the composition)."""
    from .nn import BatchNorm, Conv2d, Lambda, act_name, dropout_live
    layers = getattr(block, "layers", None)
    if compute_dtype() != "bf16" or not isinstance(layers, (list, tuple)) or not layers:
        return None
    mid, g = layers[0].conv1.out_channels if hasattr(layers[0], "conv1") else 0, 0
    for i, l in enumerate(layers):
        if not all(hasattr(l, f) for f in ("norm1", "relu", "conv1", "norm2", "conv2", "dropout")):
            return None
        if not (type(l.norm1) is BatchNorm and type(l.norm2) is BatchNorm and type(l.conv1) is Conv2d and type(l.conv2) is Conv2d
                and isinstance(l.relu, Lambda) and act_name(l.relu.fn) == "relu"):
            return None
        if _bn_training(l.norm1) or _bn_training(l.norm2) or dropout_live(l.dropout):
            return None
        g = g or l.conv2.out_channels
        if not (_plain_conv(l.conv1, 1) and _plain_conv(l.conv2, 3) and l.conv1.in_channels == C0 + i * g == l.norm1.input_size
                and l.conv1.out_channels == mid == l.conv2.in_channels == l.norm2.input_size and l.conv2.out_channels == g):
            return None
    Ct = C0 + len(layers) * g
    lib, BF = _lib.load(), _lib.BF16
    if not lib.mv_conv3x3_slice_supported(mid, g, H, W, BF, BF):
        return None
    if not all(lib.mv_preact_conv1x1_supported(C0 + i * g, mid, Ct, mid, 0, 1, BF, BF) for i in range(len(layers))):
        return None
    if (C0, len(layers), g, H) in DENSE_LITERAL_SHAPES and H == W and not _lib.get_flag("dense_always"):
        return None
    return mid, g, Ct


def _dense_layer_operands(layer):
    def build():
        s1, h1 = bn_fold(layer.norm1)
        s2, h2 = bn_fold(layer.norm2)
        w1 = np.asarray(layer.conv1.weight, np.float32)
        d32 = lambda a: _dev(a, torch.float32)
        return (d32(s1), d32(h1), _dev(w1.reshape(w1.shape[0], w1.shape[1]), torch.bfloat16), d32(s2), d32(h2),
                _dev(inception_fragments(np.asarray(layer.conv2.weight, np.float32)), torch.bfloat16))
    return _prepared(layer, "dense_layer", (layer.norm1, layer.norm2), build)


def dense_block(x: Act, block, filled: Optional[int] = None, key=None) -> Act:
    """One dense block.  bf16 inference where the two kernels have the shapes: ONE [B, H, W, C0 + L * growth] buffer with the input in
    channels [0, C0); per layer mv_preact_conv1x1_fwd (BatchNorm 1 + ReLU on the way into LDS, the 1x1, BatchNorm 2 + ReLU; buffer
    channels [0, C_i) -> the scratch map t, reused by every layer) and mv_conv3x3_slice_fwd (t -> buffer channels [C_i, C_i + growth)):
    two launches per layer, nothing is concatenated.  `filled` = C0 says that `x` already IS that buffer with its first C0 channels
    written (ops.dense_transition with `next_ld`), so there is nothing to place; otherwise one mv_copy_rows places the input.
    Everything else (fp32 mode, training-mode BatchNorm, live Dropout, the switches "no_dense_fused" / "force_generic", other
    structures or shapes): the literal composition."""
    x = as_map(x)
    B, H, W, Cx = x.t.shape
    C0 = Cx if filled is None else int(filled)
    plan = dense_block_plan(block, C0, H, W) if x.t.dtype == torch.bfloat16 else None
    if plan is None or (filled is not None and plan[2] != Cx):
        return dense_block_literal(x if filled is None else _channel_slice(x, 0, C0), block, key)
    mid, g, Ct = plan
    BF, st, es = _lib.BF16, stream_ptr(), 2
    if filled is None:
        buf = empty((B, H, W, Ct), torch.bfloat16)
        _lib.call("mv_copy_rows", _ptr(x.t), _ptr(buf), B * H * W, C0 * es, C0 * es, Ct * es, st)
    else:
        buf = x.t
    t = empty((B, H, W, mid), torch.bfloat16)
    for i, layer in enumerate(block.layers):
        s1, h1, w1, s2, h2, wf = _dense_layer_operands(layer)
        Ci = C0 + i * g
        _lib.call("mv_preact_conv1x1_fwd", _ptr(buf), Ct, _ptr(s1), _ptr(h1), _ptr(w1), _ptr(s2), _ptr(h2), _ptr(t), mid, 0, B, H, W, Ci,
                  mid, 1, BF, BF, st)
        _lib.call("mv_conv3x3_slice_fwd", _ptr(t), mid, mid, _ptr(wf), _ptr(buf), Ct, Ci, g, B, H, W, BF, BF, st)
    return Act(buf, "map", x.batched)


def dense_transition(x: Act, trans, next_ld: int = 0, key=None) -> Act:
    """One transition.  bf16 inference: ONE mv_preact_conv1x1_fwd with the 2 x 2 average in front of the product (exact: both are
    linear).  With `next_ld` > 0 the result is a [B, H/2, W/2, next_ld] map whose channels [0, C/2) are written -- the next block's
    buffer, handed to ops.dense_block with `filled` = C/2; the caller tells the two results apart by the channel count.  Otherwise,
    and wherever the kernel does not serve, the dense [.., C/2] map (the literal composition where the kernel does not serve)."""
    from .nn import act_name
    x = as_map(x)
    B, H, W, C = x.t.shape
    parts = _transition_parts(trans)
    ok = parts is not None and compute_dtype() == "bf16" and x.t.dtype == torch.bfloat16
    if ok:
        bn, lam, conv, pool = parts
        N = conv.out_channels
        ld = int(next_ld) if next_ld else N
        ok = (act_name(lam.fn) == "relu" and not _bn_training(bn) and _plain_conv(conv, 1) and conv.in_channels == C == bn.input_size
              and pool.kernel_size == (2, 2) and pool.stride == (2, 2) and H >= 2 and W >= 2 and ld >= N
              and bool(_lib.load().mv_preact_conv1x1_supported(C, N, C, ld, 0, 2, _lib.BF16, _lib.BF16)))
    if not ok:
        return dense_transition_literal(x, trans, key)
    hit = _prepared(trans, "dense_transition", (bn,), lambda: tuple(_dev(v, torch.float32) for v in bn_fold(bn)) + (
        _dev(np.asarray(conv.weight, np.float32).reshape(N, C), torch.bfloat16),))
    y = empty((B, H // 2, W // 2, ld), torch.bfloat16)
    _lib.call("mv_preact_conv1x1_fwd", _ptr(x.t), C, _ptr(hit[0]), _ptr(hit[1]), _ptr(hit[2]), None, None, _ptr(y), ld, 0, B, H, W, C, N, 2,
              _lib.BF16, _lib.BF16, stream_ptr())
    return Act(y, "map", x.batched)


# ------------------------------------------------------------------ element-wise (unfused call sites)
def _canon(x: Act) -> Act:
    return as_map(x) if x.kind == "img" else (x if x.kind == "map" else as_rows(x))


def eltwise(x: Act, act: str) -> Act:
    x = _canon(x)
    y = empty(tuple(x.t.shape), x.t.dtype)
    _lib.call("mv_eltwise_fwd", _ptr(x.t), _ptr(y), x.t.numel(), ACT[act], x.dt, stream_ptr())
    return Act(y, x.kind, x.batched)


def add(a: Act, b: Act, act=None) -> Act:
    a, b = _canon(a), _canon(b)
    if a.t.dtype != b.t.dtype and {a.t.dtype, b.t.dtype} == {torch.float32, torch.bfloat16}:
        # an fp32 residual stream + a compute-dtype branch (the un-fused x + drop_path(f(x)) of training mode): add in fp32
        a, b = (a if a.t.dtype == torch.float32 else cast(a, "fp32")), (b if b.t.dtype == torch.float32 else cast(b, "fp32"))
    if tuple(a.t.shape) != tuple(b.t.shape) or a.t.dtype != b.t.dtype:
        raise ValueError(f"add: mismatched operands {a} vs {b}")
    y = empty(tuple(a.t.shape), a.t.dtype)
    _lib.call("mv_add_fwd", _ptr(a.t), _ptr(b.t), _ptr(y), a.t.numel(), ACT[act], a.dt, stream_ptr())
    return Act(y, a.kind, a.batched)


def first_row(x: Act) -> Act:
    """x[0] of a seq [B,N,D] -> vec [B,D] (a strided gather done by the cast kernel per image)."""
    B, N, D = x.t.shape
    y = empty((B, D), x.t.dtype)
    for b in range(B):
        _lib.call("mv_cast", x.t[b].data_ptr(), y[b].data_ptr(), D, x.dt, x.dt, stream_ptr())
    return Act(y, "vec", x.batched)


# ------------------------------------------------------------------ gradients (eqxvision_amd/grad.py)
# Under `filter_value_and_grad` the entry points below run their differentiable fp32 twins; everywhere else they are untouched.
from . import grad as _grad  # noqa: E402

for _name in _grad.HOOKED:
    globals()[_name] = _grad.hook(_name, globals()[_name])
del _name
