"""Float64 restatement of `eqxvision_amd.preprocess` (resize with the antialiased triangle filter -> crop -> affine) and the
per-element error bound of the fp32 kernel, shared by tests/test_preprocess_host.py and tests/test_preprocess_gpu.py.
Written from the definition of the filter, not from the code under test: dense weight matrices, no tap tables."""
import numpy as np

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
MAX_TAPS = 24

# name -> ((Hin, Win), (Hr, Wr), (top, left, Hout, Wout)): the smallest shapes that exercise each way to go wrong
CASES = {
    "identity": ((8, 8), (8, 8), (0, 0, 8, 8)),                 # one tap of weight 1 per axis
    "down2": ((16, 24), (8, 12), (0, 0, 8, 12)),                # weights 1/8 3/8 3/8 1/8: every sum exact in fp32
    "ragged": ((37, 53), (23, 33), (3, 5, 17, 19)),             # rows no multiple of 16 bytes, odd crop offset, partial tile
    "up": ((5, 7), (11, 15), (1, 3, 9, 9)),                     # two taps, clamped at the edges
    "down8": ((64, 9), (8, 9), (0, 0, 8, 8)),                   # 16 taps on one axis, one on the other
    "preset": ((300, 260), (295, 256), (36, 16, 224, 224)),     # Resize(256) -> CenterCrop(224) of a 300 x 260 image: 7 x 7 tiles
    "multi": ((70, 90), (45, 70), (2, 1, 41, 67)),              # several tiles, the last ones partial on both axes
}


def weights64(n_in, n_out):
    """(n_out, n_in) float64: row o is the filter of output o.  Sample centre s = (o + 0.5) n_in / n_out - 0.5, triangle of
    half-width max(1, n_in / n_out) about it, restricted to the axis and divided by its sum."""
    ratio = n_in / n_out
    sup = max(1.0, ratio)
    s = (np.arange(n_out, dtype=np.float64) + 0.5) * ratio - 0.5
    x = np.arange(n_in, dtype=np.float64)
    w = np.maximum(0.0, 1.0 - np.abs(x[None, :] - s[:, None]) / sup)
    return w / w.sum(1, keepdims=True)


def affine64(mean, std):
    mean, std = np.asarray(mean, np.float64), np.asarray(std, np.float64)
    return 1.0 / (255.0 * std), -mean / std


def images(shape_hw, B=2, seed=0):
    """uint8 [B, H, W, 3] with the extremes present."""
    rng = np.random.default_rng(seed + 1000 * shape_hw[0] + shape_hw[1])
    x = rng.integers(0, 256, (B, shape_hw[0], shape_hw[1], 3), dtype=np.uint8)
    x[0, 0, 0] = (0, 255, 128)
    x[-1, -1, -1] = (255, 0, 1)
    return x


def dense(first, taps, w, n_in):
    """A tap table (first, taps, fp32 weights) as the dense (n_out, n_in) float64 matrix it stands for."""
    d = np.zeros((len(first), n_in), np.float64)
    for i in range(len(first)):
        d[i, first[i]:first[i] + taps[i]] = w[i, :taps[i]]
    return d


def reference(u8_hwc, resized_hw, box, a, b, round_weights=True, wh=None, ww=None):
    """u8_hwc uint8 [B, H, W, 3] -> (y, bound), float64 [B, 3, Hout, Wout].
    y = (sum_hw Wh[i, h] Ww[j, w] p[h, w, c]) a[c] + b[c] in float64, with the weights rounded to fp32 first when
    `round_weights` and a, b as passed (the tests pass the fp32 vectors of the kernel).  wh / ww: the dense fp32 weights of the
    box's rows / columns that the kernel was actually given (`dense` of the uploaded tables; test_preprocess_host.py holds those
    to one fp32 rounding of `weights64`), so that a weight whose float64 value sits on a rounding boundary cannot count as a
    kernel error.

    bound: the kernel forms, per pass, sum_k w_k (v_k - vmin) + vmin with one fma per tap.  Every term and partial sum lies
    between 0 and the pass's result, the tap that holds the minimum contributes an exact zero, so with u = 2^-24 the horizontal pass
    (uint8 differences are exact) is off by at most (n_w - 1 + 1) u of its result and the vertical pass (fp32 differences: one more
    rounding, shared by all terms) by (1 + n_h - 1 + 1) u; the epilogue fma rounds once.  The horizontal error passes through
    the vertical weights (which sum to 1) unchanged, so to first order |got - y| <= (n_h + n_w + 2) u (S |a| + |b|) with
    S = sum |Wh Ww p| (= the resized value: nothing is negative); the bound used is (n_h + n_w + 3) u (S |a| + |b|), the third
    unit covering the products of roundings (40 taps: 40^2 u^2 / 2 << u).  n_h, n_w: the non-zero taps of the output's row / column."""
    B, H, W, C = u8_hwc.shape
    assert C == 3 and u8_hwc.dtype == np.uint8
    top, left, hout, wout = box
    given = wh is not None
    wh = weights64(H, resized_hw[0])[top:top + hout] if wh is None else np.asarray(wh, np.float64)
    ww = weights64(W, resized_hw[1])[left:left + wout] if ww is None else np.asarray(ww, np.float64)
    assert wh.shape == (hout, H) and ww.shape == (wout, W)
    if round_weights and not given:
        wh, ww = wh.astype(np.float32).astype(np.float64), ww.astype(np.float32).astype(np.float64)
    acc = np.einsum("bhwc,ih,jw->bcij", u8_hwc.astype(np.float64), wh, ww, optimize=True)
    a = np.asarray(a, np.float64).reshape(1, 3, 1, 1)
    b = np.asarray(b, np.float64).reshape(1, 3, 1, 1)
    y = acc * a + b
    nh = (wh != 0).sum(1).reshape(1, 1, hout, 1)
    nw = (ww != 0).sum(1).reshape(1, 1, 1, wout)
    bound = (nh + nw + 3) * 2.0 ** -24 * (acc * np.abs(a) + np.abs(b))
    return y, bound


def bf16_half_ulp(v):
    """Half a bf16 ulp (8 significant bits) at magnitude |v|, float64."""
    v = np.maximum(np.abs(np.asarray(v, np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(v)) - 8)


def torch_pipeline(u8_hwc, resized_hw, box, mean, std):
    """The same transform through torch on float64 CPU tensors: interpolate(bilinear, antialias) -> crop -> / 255 -> normalise.
    Returns (resized and cropped image / 255, normalised), float64 [B, 3, Hout, Wout]."""
    import torch
    import torch.nn.functional as F
    x = torch.from_numpy(u8_hwc).permute(0, 3, 1, 2).double()
    r = F.interpolate(x, size=tuple(resized_hw), mode="bilinear", antialias=True, align_corners=False)
    top, left, hout, wout = box
    r = (r[:, :, top:top + hout, left:left + wout] / 255.0).numpy()
    m = np.asarray(mean, np.float64).reshape(1, 3, 1, 1)
    s = np.asarray(std, np.float64).reshape(1, 3, 1, 1)
    return r, (r - m) / s
