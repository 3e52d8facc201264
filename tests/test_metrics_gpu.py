"""`-m gpu`: `eqxvision_amd.metrics` on the MI355X -- the confusion-matrix kernels (mv_confusion_from_logits / _from_labels) and the
top-k accuracy kernel (mv_topk_correct_f32) through the public classes, at model level and under `filter_jit`.

Every comparison is exact integer equality; the float64 figures of `compute()` are compared with `==` to the numpy restatement on
the same integers."""
import functools

import numpy as np
import pytest
import torch

import eqxvision_amd as eqv
from eqxvision_amd import _lib
from eqxvision_amd import metrics as M
from eqxvision_amd import postprocess as P
from tests import _metrics_ref as R
from tests import _postprocess_ref as PR
from tests import _strict as S

pytestmark = pytest.mark.gpu


def _dev_logits(x, dtype):
    t = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
    return t.to(torch.bfloat16) if dtype == "bf16" else t


def _mat(cm):
    return cm.mat.cpu().numpy()


def _kernel_tail(C):
    return "_lds" if C <= 64 else "_global"


# ------------------------------------------------------------------------------------------------ update_logits
@pytest.mark.parametrize("C", R.CLASS_COUNTS)
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("ldtype", [np.uint8, np.int32], ids=["u8", "i32"])
def test_update_logits_counts_what_upsample_argmax_writes(C, dtype, ldtype):
    """update_logits(logits, labels) == bincount of (labels, fetched upsample_argmax(logits)) for both shapes, in its two-launch
    form (the default) and as one launch (update_logits_fused: the kernel resize_argmax_confusion); values that are not a class
    (255, [C, 255), negatives) are not counted: the sum is the number of valid pixels."""
    for si, ((b, h, w), (H, W)) in enumerate(R.LOGIT_SHAPES):
        x = R.peaked_logits((b, h, w, C), 6)
        t = _dev_logits(x, dtype)
        labels = R.targets(b * H * W, C, ldtype, 5).reshape(b, H, W)
        pred = P.upsample_argmax(t, (H, W)).cpu().numpy()
        want = R.confusion(labels, pred, C)
        two = M.ConfusionMatrix(C)
        two.update_logits(t, labels)
        assert _lib.last_kernel() == "label_confusion" + _kernel_tail(C)
        assert np.array_equal(_mat(two), want)
        cm = M.ConfusionMatrix(C)
        cm.update_logits_fused(t, labels)
        kern = _lib.last_kernel()
        vec = C % (8 if dtype == "bf16" else 4) == 0
        assert kern == "resize_argmax_confusion" + ("_v16" if vec else "") + _kernel_tail(C), kern
        got = _mat(cm)
        valid = int(((labels.astype(np.int64) >= 0) & (labels.astype(np.int64) < C)).sum())
        print(f"C={C} {dtype} {ldtype.__name__} shape {si} [{kern}]: {int((got != want).sum())} cells differ; {valid} of {labels.size} "
              f"pixels valid; classes predicted {np.unique(pred).size}")
        assert got.dtype == np.int64 and np.array_equal(got, want)
        assert int(got.sum()) == valid and (valid < labels.size or (C == 256 and ldtype == np.uint8))
        if C in R.ALL_CLASSES_PREDICTED:
            assert np.unique(pred).size == C
        assert R.same_metrics(cm.compute(), R.metrics(want))


@pytest.mark.parametrize("shape,ratio", [((2, 6, 5, 21), 2), ((1, 5, 6, 8), 4)], ids=["21_x2", "8_x4"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_integer_logits_count_exactly(shape, ratio, dtype):
    """Integer logits in [-2, 2] at x2 / x4: the interpolation is exact in fp32 (tests/test_postprocess_gpu.py:
    test_integer_logits_select_exactly), so the predictions are the float64 first-index argmax, ties to the lower class, and the
    matrix is the numpy one computed from exact arithmetic."""
    N, h, w, C = shape
    H, W = h * ratio, w * ratio
    x = S.rng_of(62).integers(-2, 3, shape).astype(np.float32)
    ref = PR.resize64(x, H, W)
    assert np.array_equal(ref * 64, np.rint(ref * 64)) and (PR.top2_gap(ref)[2] == 0).mean() > 0.05
    labels = R.targets(N * H * W, C, np.int32, 9).reshape(N, H, W)
    cm = M.ConfusionMatrix(C)
    cm.update_logits_fused(_dev_logits(x, dtype), labels)
    assert np.array_equal(_mat(cm), R.confusion(labels, PR.argmax_first(ref, -1), C))
    cm.reset()                                                   # a constant map: every class ties everywhere, class 0 is predicted
    cm.update_logits_fused(_dev_logits(np.full(shape, 1.5, np.float32), dtype), labels)
    got = _mat(cm)
    assert not got[:, 1:].any() and np.array_equal(got[:, 0], R.confusion(labels, np.zeros_like(labels), C)[:, 0])


@pytest.mark.parametrize("mode", [0, 1, 2, 3], ids=["default", "global", "lds", "lds_per_wave"])
def test_maximum_contention(mode):
    """[1, 64, 64, 21] -> 256 x 256 with one class winning everywhere and one target class: ONE cell holds 65 536 and every other
    is zero.  Then vertical stripes of two target classes, four pixels wide: a lane's four pixels agree, the lanes of a wave do
    not.  Run on every counter placement the kernel has (`confusion_mode`)."""
    x = S.rng_of(91).standard_normal((1, 64, 64, 21)).astype(np.float32)
    x[..., 7] = 9.0
    t = _dev_logits(x, "fp32")
    _lib.set_flag("confusion_mode", mode)
    try:
        cm = M.ConfusionMatrix(21)
        cm.update_logits_fused(t, np.full((1, 256, 256), 3, np.uint8))
        assert _lib.last_kernel() == "resize_argmax_confusion" + {0: "_lds", 1: "_global", 2: "_lds", 3: "_lds4"}[mode]
        want = np.zeros((21, 21), np.int64)
        want[3, 7] = 65536
        assert np.array_equal(_mat(cm), want)
        stripes = np.where((np.arange(256) // 4) % 2 == 0, 3, 5).astype(np.int32)
        cm.reset()
        cm.update_logits_fused(t, np.broadcast_to(stripes, (1, 256, 256)).copy())
        want[3, 7] = want[5, 7] = 32768
        assert np.array_equal(_mat(cm), want)
    finally:
        _lib.set_flag("confusion_mode", 0)


# ------------------------------------------------------------------------------------------------ update(pred, labels)
N_ODD = 4099                     # not a multiple of the four elements a lane takes


@pytest.mark.parametrize("C", [2, 21, 64, 65, 256])
@pytest.mark.parametrize("pdtype", [np.uint8, np.int32], ids=["pred_u8", "pred_i32"])
@pytest.mark.parametrize("ldtype", [np.uint8, np.int32], ids=["labels_u8", "labels_i32"])
def test_update_of_two_label_maps(C, pdtype, ldtype):
    pred, labels = R.predictions(N_ODD, C, pdtype, 7), R.targets(N_ODD, C, ldtype, 8)
    want = R.confusion(labels, pred, C)
    cm = M.ConfusionMatrix(C)
    cm.update(pred, labels)
    assert _lib.last_kernel() == "label_confusion" + _kernel_tail(C)
    assert np.array_equal(_mat(cm), want)
    cm.reset()
    cm.update(torch.from_numpy(pred).cuda().reshape(1, -1), torch.from_numpy(labels).reshape(1, -1))       # device / host, 2-D
    assert np.array_equal(_mat(cm), want)
    assert R.same_metrics(cm.compute(), R.metrics(want))


@pytest.mark.parametrize("C", [21, 150])
def test_label_buffers_offset_by_one_byte(C):
    """uint8 maps that start one byte behind the allocation's alignment take the byte loads: the same matrix."""
    pred, labels = R.predictions(N_ODD, C, np.uint8, 7), R.targets(N_ODD, C, np.uint8, 8)
    want = R.confusion(labels, pred, C)
    for skew_p, skew_l in ((1, 1), (0, 1), (1, 0), (3, 2)):
        p = torch.zeros((N_ODD + skew_p,), dtype=torch.uint8, device="cuda")
        l = torch.zeros((N_ODD + skew_l,), dtype=torch.uint8, device="cuda")
        p[skew_p:] = torch.from_numpy(pred).cuda()
        l[skew_l:] = torch.from_numpy(labels).cuda()
        assert p[skew_p:].data_ptr() % 4 == skew_p and l[skew_l:].data_ptr() % 4 == skew_l
        cm = M.ConfusionMatrix(C)
        cm.update(p[skew_p:], l[skew_l:])
        assert np.array_equal(_mat(cm), want), (skew_p, skew_l)
    # the fused kernel: a label map whose rows start off the 4-byte boundary
    x = R.peaked_logits((2, 4, 4, C), 3)
    t = _dev_logits(x, "fp32")
    lab = R.targets(2 * 8 * 8, C, np.uint8, 4) if C <= 128 else R.targets(2 * 8 * 8 + 100, C, np.uint8, 4)[:128]
    buf = torch.zeros((129,), dtype=torch.uint8, device="cuda")
    buf[1:] = torch.from_numpy(lab).cuda()
    cm = M.ConfusionMatrix(C)
    cm.update_logits_fused(t, buf[1:].reshape(2, 8, 8))
    assert np.array_equal(_mat(cm), R.confusion(lab, P.upsample_argmax(t, (8, 8)).cpu().numpy(), C))


def test_counters_are_flushed_before_they_can_wrap():
    """`confusion_flush_iters` = 1 makes every block flush its LDS counters after each step of its loop instead of after 2^20: a
    map long enough that the blocks loop (2048 blocks x 1024 pixels per step) still gives the exact matrix."""
    C, n = 21, 2048 * 1024 * 2 + 4099
    pred, labels = R.predictions(n, C, np.uint8, 11), R.targets(n, C, np.uint8, 12)
    want = R.confusion(labels, pred, C)
    p, l = torch.from_numpy(pred).cuda(), torch.from_numpy(labels).cuda()
    for flush in (0, 1):
        _lib.set_flag("confusion_flush_iters", flush)
        try:
            cm = M.ConfusionMatrix(C)
            cm.update(p, l)
            assert _lib.last_kernel() == "label_confusion_lds"
            assert np.array_equal(_mat(cm), want), flush
        finally:
            _lib.set_flag("confusion_flush_iters", 0)


# ------------------------------------------------------------------------------------------------ accumulate / reset / replay
def test_updates_accumulate_in_64_bits_and_reset_zeroes():
    C = 21
    pred, labels = R.predictions(N_ODD, C, np.uint8, 7), R.targets(N_ODD, C, np.int32, 8)
    labels[:50], pred[:50] = 0, 0                               # at least 50 counts in cell (0, 0)
    one = R.confusion(labels, pred, C)
    assert one[0, 0] >= 50
    cm = M.ConfusionMatrix(C)
    cm.update(pred, labels)
    cm.update(pred, labels)
    assert np.array_equal(_mat(cm), 2 * one)
    cm.reset()
    assert not _mat(cm).any()
    cm.mat[0, 0] = 2 ** 32 - 3
    cm.update(pred, labels)
    want = one.copy()
    want[0, 0] += 2 ** 32 - 3
    assert want[0, 0] > 2 ** 32 and np.array_equal(_mat(cm), want)
    x = R.peaked_logits((1, 8, 8, C), 6)                        # the fused kernel's flush, the same way
    lab = np.zeros((1, 32, 32), np.uint8)
    cm.reset()
    cm.mat[0, 0] = 2 ** 32 - 3
    cm.update_logits_fused(x, lab)
    want = R.confusion(lab, P.upsample_argmax(x, (32, 32)).cpu().numpy(), C)
    assert want[0, 0] >= 3
    want[0, 0] += 2 ** 32 - 3
    assert np.array_equal(_mat(cm), want)


def test_update_logits_under_filter_jit():
    """Recording call, capturing call, replays: every call adds the same counts once."""
    C = 21
    t = _dev_logits(R.peaked_logits((2, 5, 7, C), 6), "fp32")
    labels = torch.from_numpy(R.targets(2 * 17 * 23, C, np.uint8, 5).reshape(2, 17, 23)).cuda()
    one = R.confusion(labels.cpu().numpy(), P.upsample_argmax(t, (17, 23)).cpu().numpy(), C)
    cm = M.ConfusionMatrix(C)
    cm.reset()                                                  # the counters exist before the recording
    step = eqv.filter_jit(lambda lg, lb: cm.update_logits(lg, lb))
    for i in range(1, 5):
        step(t, labels)
        assert np.array_equal(_mat(cm), i * one), f"after call {i}"
    assert step._entries()[0].replays >= 2
    fused = eqv.filter_jit(lambda lg, lb: cm.update_logits_fused(lg, lb))
    for i in range(5, 9):
        fused(t, labels)
        assert np.array_equal(_mat(cm), i * one), f"after call {i}"
    assert fused._entries()[0].replays >= 2


# ------------------------------------------------------------------------------------------------ model level
SIZE, BATCH, CLASSES = 64, 2, 21


@functools.lru_cache(maxsize=None)
def _net(name):
    if name == "lraspp_mobilenet_v3_large":
        net = eqv.models.lraspp_mobilenet_v3_large(num_classes=CLASSES)
    else:
        net = getattr(eqv.models, name)(num_classes=CLASSES, intermediate_layers=lambda m: [m.layer3, m.layer4], aux_in_channels=1024)
    return eqv.tree_inference(eqv.utils.randomize_batchnorm(net, 1), True)


@pytest.mark.parametrize("name", ["fcn", "deeplabv3", "lraspp_mobilenet_v3_large"])
def test_evaluate_segmentation_is_update_of_segment(name):
    net = _net(name)
    x = torch.from_numpy(S.rng_of(71).random((BATCH, 3, SIZE, SIZE), dtype=np.float32)).cuda()
    keys = eqv.random.split(eqv.random.PRNGKey(0), BATCH)
    labels = R.targets(BATCH * SIZE * SIZE, CLASSES, np.int32, 13).reshape(BATCH, SIZE, SIZE)
    with eqv.precision("bf16"):
        a, b = M.ConfusionMatrix(CLASSES), M.ConfusionMatrix(CLASSES)
        M.evaluate_segmentation(net, x, labels, a, key=keys)
        seg = P.segment(net, x, key=keys)
        b.update(seg, labels)
    assert np.array_equal(_mat(a), _mat(b))
    assert np.array_equal(_mat(a), R.confusion(labels, seg.cpu().numpy(), CLASSES)) and int(_mat(a).sum()) > 0
    _lib.check_device_status()


def test_evaluate_segmentation_refuses_training_mode_and_classifiers():
    x = torch.from_numpy(S.rng_of(74).random((BATCH, 3, SIZE, SIZE), dtype=np.float32)).cuda()
    labels, cm = np.zeros((BATCH, SIZE, SIZE), np.uint8), M.ConfusionMatrix(CLASSES)
    with pytest.raises(ValueError, match="training mode"):
        M.evaluate_segmentation(eqv.tree_inference(_net("fcn"), False), x, labels, cm)
    with pytest.raises(ValueError, match="segmentation model"):
        M.evaluate_segmentation(eqv.tree_inference(eqv.models.alexnet(num_classes=10), True), x, labels, cm)
    with pytest.raises(ValueError, match="the model has 21 classes, the matrix 5"):
        M.evaluate_segmentation(_net("fcn"), x, labels, M.ConfusionMatrix(5))
    assert not _mat(cm).any()


# ------------------------------------------------------------------------------------------------ top-k accuracy
def _counts(acc):
    return acc.counts.cpu().numpy().tolist()


@pytest.mark.parametrize("B,K", [(3, 1000), (1, 1), (2, 65536), (5, 37)], ids=lambda v: str(v))
@pytest.mark.parametrize("ks", [(1, 5), (1, 3, 1000)], ids=["k1_5", "k1_3_1000"])
def test_topk_counts(B, K, ks):
    """Integer logits in [-8, 8] (many ties) and labels spread over the rows: the counters are those of a stable descending
    argsort; for k <= min(K, 16) they also equal membership of the label in postprocess.topk's indices.  Two updates add."""
    rng = S.rng_of(95)
    x = rng.integers(-8, 9, (B, K)).astype(np.float32)
    labels = rng.integers(0, K, (B,)).astype(np.int32)
    labels[0] = int(np.argmax(x[0]))                            # one row is right at k = 1
    want = R.topk_counts(x, labels, ks)
    acc = M.TopK(ks)
    acc.update(x, labels)
    assert _lib.last_kernel() == "topk_correct"
    assert _counts(acc) == want and want[0] >= 1
    for i, k in enumerate(ks):
        if k <= min(K, P.MAX_K):
            idx = P.topk(x, k, probabilities=False)[1].cpu().numpy()
            assert int((idx == labels[:, None]).any(1).sum()) == want[i]
    acc.update(torch.from_numpy(x).cuda(), torch.from_numpy(labels).cuda())
    assert _counts(acc) == [2 * v for v in want]
    res = acc.compute()
    assert res["count"] == 2 * B and all(res[f"top{k}"] == want[i] / B for i, k in enumerate(ks))
    acc.reset()
    assert _counts(acc) == [0] * (len(ks) + 1)


def test_topk_tie_rule_and_rows_that_cannot_be_right():
    """All-equal rows: the label at index 0 is first, the label at the last index is last.  A label outside [0, K) and a NaN at
    the label's logit are wrong for every k and still counted; a NaN elsewhere in the row does not outrank the label."""
    K = 300
    x = np.full((2, K), 3.0, np.float32)
    acc = M.TopK((1, K - 1, K))
    acc.update(x, np.array([0, K - 1], np.int32))
    assert _counts(acc) == [1, 1, 2, 2]
    assert _counts(acc) == R.topk_counts(x, [0, K - 1], (1, K - 1, K))
    z = np.array([[0.0, -0.0, -1.0]], np.float32)               # the two zeros tie: index decides
    acc = M.TopK((1, 2))
    acc.update(z, np.array([1], np.int32))
    assert _counts(acc) == [0, 1, 1]
    y = S.rng_of(96).standard_normal((5, 37)).astype(np.float32)
    labels = np.array([37, -1, 4, 2 ** 31 - 1, 6], np.int32)
    y[2, 4] = np.nan                                            # at the label
    y[4, 6], y[4, 9] = 50.0, np.nan                             # the label holds the maximum, a NaN sits elsewhere
    acc = M.TopK((1, 37, 1000))
    acc.update(y, labels)
    assert _counts(acc) == [1, 1, 1, 5]
    assert _counts(acc) == R.topk_counts(y, labels, (1, 37, 1000))


# ------------------------------------------------------------------------------------------------ refusal under the tape
def test_refused_inside_value_and_grad():
    x = S.rng_of(84).standard_normal((1, 4, 4, 5)).astype(np.float32)
    cm, acc = M.ConfusionMatrix(5), M.TopK((1,))
    cm.reset()
    acc.reset()

    @eqv.filter_value_and_grad
    def from_logits(model, im):
        return cm.update_logits_fused(im, np.zeros((1, 8, 8), np.uint8))

    @eqv.filter_value_and_grad
    def two_launches(model, im):
        return cm.update_logits(im, np.zeros((1, 8, 8), np.uint8))

    @eqv.filter_value_and_grad
    def from_labels(model, im):
        return cm.update(np.zeros((8, 8), np.uint8), np.zeros((8, 8), np.uint8))

    @eqv.filter_value_and_grad
    def topk(model, im):
        return acc.update(im.reshape(16, 5), np.zeros((16,), np.int32))
    with pytest.raises(NotImplementedError, match="mv_confusion_from_logits"):
        from_logits(None, x)
    with pytest.raises(NotImplementedError, match="mv_resize_argmax_nhwc_fwd"):
        two_launches(None, x)
    with pytest.raises(NotImplementedError, match="mv_confusion_from_labels"):
        from_labels(None, x)
    with pytest.raises(NotImplementedError, match="mv_topk_correct_f32"):
        topk(None, x)
    assert not _mat(cm).any() and not acc.counts.cpu().numpy().any()
