"""numpy restatement of `mv_preprocess_u8_mix_fwd`'s semantics in float32, on whatever fp32 v_i tensors it is given (the GPU file
gives it the outputs of the existing `crop_resize_normalize`), of the soft targets, of `eqv.optim.ema`, and -- independently of
eqxvision_amd/preprocess.py -- of the two draw functions on the package's random stream.

float32 numpy rounds every product and every sum once and never contracts them, which is what the kernel's fmul / fadd do."""
import numpy as np

from eqxvision_amd import random as jr

F = np.float32


def empty(rect):
    y0, x0, y1, x1 = (int(v) for v in rect)
    return y1 <= y0 or x1 <= x0


def erased(v, erase):
    """v fp32 [B, 3, H, W] with image i's own erase rectangle set to +0.0."""
    out = np.array(v, np.float32)
    for i, (y0, x0, y1, x1) in enumerate(np.asarray(erase)):
        if not empty((y0, x0, y1, x1)):
            out[i, :, y0:y1, x0:x1] = F(0.0)
    return out


def mix(v, partner, lam, oml, cut, erase):
    """fp32 [B, 3, H, W]: erase each image, then per image the partner inside the cut rectangle, the image itself where it has
    no partner or lam == 1, else fl(fl(lam v_i) + fl(oml v_r))."""
    ve = erased(v, erase)
    out = np.empty_like(ve)
    for i in range(ve.shape[0]):
        r = int(partner[i])
        if r == i:
            out[i] = ve[i]
            continue
        if F(lam[i]) == F(1.0):
            o = ve[i].copy()
        else:
            o = (F(lam[i]) * ve[i]).astype(np.float32) + (F(oml[i]) * ve[r]).astype(np.float32)
        if not empty(cut[i]):
            y0, x0, y1, x1 = (int(c) for c in cut[i])
            o[:, y0:y1, x0:x1] = ve[r][:, y0:y1, x0:x1]
        out[i] = o
    return out


def one_minus(v):
    """1 - v in float64 from the fp32 value, rounded once."""
    return (1.0 - np.asarray(v, np.float32).astype(np.float64)).astype(np.float32)


def bf16_bits(x):
    """fp32 -> bf16, round to nearest even, as uint16 bits (finite inputs)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def on_off(eps, K):
    return F(1.0 - eps + eps / K), F(eps / K)


def targets(labels, partner, lam_t, oml_t, K, eps):
    """fp32 [B, K]: fl(fl(lam_t s(y_i)) + fl(oml_t s(y_r))), s the smoothed one-hot row; a label outside [0, K) matches no class."""
    on, off = on_off(eps, K)
    labels = np.asarray(labels)
    s = np.full((len(labels), K), off, np.float32)
    for i, y in enumerate(labels):
        if 0 <= int(y) < K:
            s[i, int(y)] = on
    lt, ot = np.asarray(lam_t, np.float32)[:, None], np.asarray(oml_t, np.float32)[:, None]
    return (lt * s).astype(np.float32) + (ot * s[np.asarray(partner)]).astype(np.float32)


def ema(e, p, decay):
    """One update of the average in float32: fl(fl(d e) + fl((1 - d) p)), 1 - d from float64."""
    d, omd = F(decay), F(1.0 - float(decay))
    return (d * np.asarray(e, np.float32)).astype(np.float32) + (omd * np.asarray(p, np.float32)).astype(np.float32)


# ---- the draws, restated ---------------------------------------------------------------------------------------------------

def mixup_cutmix_draw(key, B, hw, mixup_alpha=0.2, cutmix_alpha=1.0, switch_p=0.5):
    """-> (branch, partner, lam, rect, lam_t) for the whole batch: branch "none" / "mixup" / "cutmix", scalars and one rectangle."""
    H, W = hw
    kc, kl, kb = jr.split(key, 3)
    if B == 1 or (mixup_alpha <= 0 and cutmix_alpha <= 0):
        return "none", np.arange(B), 1.0, (0, 0, 0, 0), 1.0
    if mixup_alpha > 0 and cutmix_alpha > 0:
        branch = "cutmix" if jr.uniform01(kc, 1)[0] < switch_p else "mixup"
    else:
        branch = "cutmix" if cutmix_alpha > 0 else "mixup"
    alpha = cutmix_alpha if branch == "cutmix" else mixup_alpha
    lam = float(jr.generator(kl).beta(alpha, alpha))
    partner = np.roll(np.arange(B), 1)
    if branch == "mixup":
        return branch, partner, lam, (0, 0, 0, 0), lam
    u = jr.uniform01(kb, 2).astype(np.float64)
    rx, ry = min(int(u[0] * W), W - 1), min(int(u[1] * H), H - 1)
    r = 0.5 * np.sqrt(1.0 - lam)
    rw, rh = int(r * W), int(r * H)
    x0, y0, x1, y1 = max(rx - rw, 0), max(ry - rh, 0), min(rx + rw, W), min(ry + rh, H)
    return branch, partner, 1.0, (y0, x0, y1, x1), 1.0 - (x1 - x0) * (y1 - y0) / (H * W)


def random_erasing_draw(key, B, hw, p=0.5, scale=(0.02, 0.33), ratio=(0.3, 3.3)):
    H, W = hw
    out = np.zeros((B, 4), np.int32)
    for i, k in enumerate(jr.split(key, B)):
        u = jr.uniform(k, (41,)).astype(np.float64)
        if u[0] >= p:
            continue
        for t in range(10):
            a = H * W * (scale[0] + u[1 + 4 * t] * (scale[1] - scale[0]))
            ar = np.exp(np.log(ratio[0]) + u[2 + 4 * t] * (np.log(ratio[1]) - np.log(ratio[0])))
            h, w = int(round(float(np.sqrt(a * ar)))), int(round(float(np.sqrt(a / ar))))
            if h < H and w < W:
                y0, x0 = min(int(u[3 + 4 * t] * (H - h + 1)), H - h), min(int(u[4 + 4 * t] * (W - w + 1)), W - w)
                out[i] = (y0, x0, y0 + h, x0 + w)
                break
    return out
