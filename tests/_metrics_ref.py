"""numpy restatements for the tests of `eqxvision_amd.metrics`, and the inputs the GPU tests use (tests/test_metrics_host.py checks
on the CPU that those inputs satisfy their own preconditions).

The counting rule is that of torchvision's reference segmentation ConfusionMatrix: a pixel counts iff 0 <= target < C, and adds
one to mat[target, prediction]."""
import numpy as np


def confusion(target, pred, C):
    """int64 [C, C], rows = target, columns = prediction."""
    t, p = np.asarray(target).astype(np.int64).ravel(), np.asarray(pred).astype(np.int64).ravel()
    k = (t >= 0) & (t < C)
    return np.bincount(C * t[k] + p[k], minlength=C * C).reshape(C, C)


def metrics(mat):
    """Class by class, in Python integers and one float64 division each."""
    m = [[int(v) for v in row] for row in np.asarray(mat)]
    C = len(m)
    total, trace = sum(map(sum, m)), sum(m[c][c] for c in range(C))
    nan = float("nan")
    acc, iou = [], []
    for c in range(C):
        row, col = sum(m[c]), sum(m[r][c] for r in range(C))
        acc.append(np.float64(m[c][c]) / np.float64(row) if row else nan)
        union = row + col - m[c][c]
        iou.append(np.float64(m[c][c]) / np.float64(union) if union else nan)
    seen = [v for v in iou if v == v]
    return {"pixel_accuracy": float(np.float64(trace) / np.float64(total)) if total else nan, "class_accuracy": np.array(acc, np.float64),
            "iou": np.array(iou, np.float64), "mean_iou": float(np.mean(np.array(seen, np.float64))) if seen else nan}


def same_metrics(a, b):
    """== on every figure, NaN matching NaN."""
    def eq(x, y):
        x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
        return x.shape == y.shape and bool(np.all((x == y) | ((x != x) & (y != y))))
    return set(a) == set(b) and all(eq(a[k], b[k]) for k in a)


def topk_counts(x, labels, ks):
    """[correct at k for k in ks] + [rows]: the label's position in the stable descending order of its row (equal values by
    ascending index); a label outside [0, K) or a NaN at the label's logit is wrong for every k."""
    x = np.asarray(x)
    B, K = x.shape
    out = [0] * len(ks)
    for r in range(B):
        l = int(labels[r])
        if l < 0 or l >= K or x[r, l] != x[r, l]:
            continue
        order = np.argsort(-x[r].astype(np.float64), kind="stable")
        pos = int(np.nonzero(order == l)[0][0])
        for i, k in enumerate(ks):
            out[i] += pos < k
    return out + [B]


# ------------------------------------------------------------------------------------------------ inputs of the GPU tests
IGNORED = 0.15                 # the share of pixels given a value that must not be counted


def targets(n, C, dtype, seed):
    """n targets: every class 0 .. C-1 occurs (n >= C), and IGNORED of the pixels hold a value the rule leaves out -- 255, values
    in [C, 255), and for int32 negatives and values above 255.  uint8 with C = 256 has no such value: every byte is a class."""
    assert n >= C
    rng = np.random.default_rng(seed)
    t = (np.arange(n) % C).astype(np.int64)
    out_of_range = [v for v in (255, C, (C + 255) // 2, 254) if C <= v <= 255]
    if dtype == np.int32:
        out_of_range += [-1, -7, -2 ** 31, 256, 1000, 2 ** 31 - 1]
    if out_of_range:
        where = C + rng.choice(n - C, size=int(round(IGNORED * n)), replace=False)       # the first C stay: one of every class
        t[where] = rng.choice(np.array(out_of_range, np.int64), size=where.size)
    return rng.permutation(t).astype(dtype)


def ignored_share(t, C):
    t = np.asarray(t).astype(np.int64)
    return float(((t < 0) | (t >= C)).mean())


def peaked_logits(shape, seed):
    """Standard-normal logits [B, h, w, C] with +6 on class (pixel index mod C): every class wins around some source pixel when
    there are at least C of them."""
    B, h, w, C = shape
    x = np.random.default_rng(seed).standard_normal(shape).astype(np.float32)
    idx = np.arange(B * h * w) % C
    x.reshape(-1, C)[np.arange(B * h * w), idx] += 6.0
    return x


def predictions(n, C, dtype, seed):
    """n predictions in [0, C), every class present (n >= C)."""
    assert n >= C
    return np.random.default_rng(seed).permutation(np.arange(n) % C).astype(dtype)


LOGIT_SHAPES = [((2, 5, 7), (17, 23)), ((1, 8, 8), (32, 32))]       # ragged W % 4 and an odd ratio; x4
CLASS_COUNTS = [1, 2, 21, 64, 65, 150, 256]                          # 64 | 65: the last class count with LDS counters, the first without
ALL_CLASSES_PREDICTED = (1, 2, 21)                                   # (many) fewer classes than source pixels: every class is predicted
