"""Float64 restatements for the tests of `eqxvision_amd.postprocess` (csrc/resize.hip: mv_resize_argmax_nhwc_fwd; csrc/postprocess.hip:
mv_softmax_topk_f32).  numpy only; nothing here knows how the kernels compute."""
import numpy as np

F64 = np.float64


def taps64(n_in, n_out):
    """jax.image.resize "bilinear" for n_out >= n_in, per output index: (i0, i1, w0, w1) with value = w0 x[i0] + w1 x[i1].  Sample
    centre s = (o + 0.5) n_in / n_out - 0.5; a tap outside the axis is dropped and the rest renormalised, which for two taps means
    the whole weight goes to the edge pixel."""
    o = np.arange(n_out, dtype=F64)
    s = (o + 0.5) * (F64(n_in) / F64(n_out)) - 0.5
    f = np.floor(s)
    i0, i1, w1 = f.astype(np.int64), f.astype(np.int64) + 1, s - f
    w0 = 1.0 - w1
    lo, hi = i0 < 0, i1 > n_in - 1
    w1 = np.where(lo, 1.0, np.where(hi, 0.0, w1))
    w0 = np.where(lo, 0.0, np.where(hi, 1.0, w0))
    return np.clip(i0, 0, n_in - 1), np.clip(i1, 0, n_in - 1), w0, w1


def weights64(n_in, n_out):
    """The (n_out, n_in) interpolation matrix of taps64."""
    i0, i1, w0, w1 = taps64(n_in, n_out)
    m = np.zeros((n_out, n_in))
    np.add.at(m, (np.arange(n_out), i0), w0)
    np.add.at(m, (np.arange(n_out), i1), w1)
    return m


def resize64(x, H, W):
    """x (N, h, w, C) -> (N, H, W, C) in float64."""
    x = np.asarray(x, F64)
    return np.einsum("nhwc,Hh,Ww->nHWc", x, weights64(x.shape[1], H), weights64(x.shape[2], W))


def argmax_first(v, axis=-1):
    """jnp.argmax: the first index of the maximum; a NaN beats every number and the first NaN wins (numpy's rule as well)."""
    return np.argmax(np.asarray(v), axis=axis)


def labels64(x, H, W):
    """uint8-valued (N, H, W) label map of NHWC logits: argmax over the classes of the float64 resize."""
    return argmax_first(resize64(x, H, W), -1)


def top2_gap(v):
    """(first, second, gap) over the last axis of a float64 array with at least two classes: the indices of the two largest
    values (first-index rule) and their difference."""
    v = np.asarray(v, F64)
    first = argmax_first(v, -1)
    masked = v.copy()
    np.put_along_axis(masked, first[..., None], -np.inf, -1)
    second = argmax_first(masked, -1)
    top = np.take_along_axis(v, first[..., None], -1)[..., 0]
    nxt = np.take_along_axis(v, second[..., None], -1)[..., 0]
    return first, second, top - nxt


def touched_by(n_in, n_out, i):
    """Boolean [n_out]: the outputs whose taps include input i with a non-zero weight."""
    return weights64(n_in, n_out)[:, i] > 0


def topk_indices(logits, k):
    """jax.lax.top_k's order: value descending, equal values by ascending index -- a stable sort of the negated row."""
    x = np.asarray(logits, F64)
    return np.argsort(-x, axis=-1, kind="stable")[..., :k]


def softmax64(logits):
    x = np.asarray(logits, F64)
    e = np.exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def topk64(logits, k):
    """(probabilities, logits, indices) of the k selected entries of every row, float64."""
    idx = topk_indices(logits, k)
    return (np.take_along_axis(softmax64(logits), idx, -1), np.take_along_axis(np.asarray(logits, F64), idx, -1), idx)


def prob_bound(p64, K):
    """|p - p64| <= (K + 48) 2^-24 p64: K for the worst summation order of the K-term fp32 sum, 48 for the rounded exponent
    argument (magnitude <= 16 for |logit| <= 8, so 16 ulp through exp in the numerator and as much in the sum) plus a few ulp of
    expf and the division."""
    return (K + 48) * 2.0 ** -24 * np.asarray(p64, F64)
