"""CPU: the host half of `eqxvision_amd.metrics` -- the numpy restatement against a hand-written example, the NaN / mean-IoU rules,
every refusal before the device is touched, the argument checks of the three C entries, and the preconditions of the inputs
the GPU tests use (tests/_metrics_ref.py)."""
import numpy as np
import pytest
import torch

import eqxvision_amd as eqv
from eqxvision_amd import _lib
from eqxvision_amd import metrics as M
from eqxvision_amd import postprocess as P
from tests import _metrics_ref as R
from tests import _postprocess_ref as PR


def test_module_is_exported():
    assert eqv.metrics is M and "metrics" in eqv.__all__


def test_reference_on_a_hand_written_example():
    #        pixel:  0  1  2  3    4  5  6  7   8  9
    target = [0, 0, 0, 1, 255, 1, 2, 2, -1, 3]                        # 255, -1 and 3 (= C) do not count
    pred = [0, 1, 0, 1, 0, 2, 2, 2, 1, 0]
    want = np.array([[2, 1, 0], [0, 1, 1], [0, 0, 2]])
    assert np.array_equal(R.confusion(np.array(target, np.int32), np.array(pred, np.uint8), 3), want)
    m = R.metrics(want)
    assert m["pixel_accuracy"] == 5 / 7
    assert m["class_accuracy"].tolist() == [2 / 3, 1 / 2, 1.0]
    assert m["iou"].tolist() == [2 / 3, 1 / 3, 2 / 3]
    assert m["mean_iou"] == float(np.mean(np.array([2 / 3, 1 / 3, 2 / 3])))
    assert R.same_metrics(M.metrics_from_matrix(want), m)


def test_absent_classes_give_nan_and_are_left_out_of_the_mean():
    mat = np.array([[3, 0, 1, 0], [0, 0, 0, 0], [2, 0, 4, 0], [0, 0, 0, 0]])      # class 1 and 3 occur nowhere
    for m in (R.metrics(mat), M.metrics_from_matrix(mat)):
        assert np.isnan(m["iou"][[1, 3]]).all() and np.isnan(m["class_accuracy"][[1, 3]]).all()
        assert m["iou"][0] == 3 / 6 and m["iou"][2] == 4 / 7
        assert m["mean_iou"] == float(np.mean(np.array([3 / 6, 4 / 7])))
        assert m["pixel_accuracy"] == 7 / 10
    mat[1, 0] = 1                                                                  # a target without a hit: accuracy 0, IoU 0, counted
    m = M.metrics_from_matrix(mat)
    assert m["class_accuracy"][1] == 0.0 and m["iou"][1] == 0.0 and R.same_metrics(m, R.metrics(mat))
    for m in (R.metrics(np.zeros((3, 3), np.int64)), M.metrics_from_matrix(np.zeros((3, 3), np.int64))):
        assert np.isnan(m["mean_iou"]) and np.isnan(m["pixel_accuracy"]) and np.isnan(m["iou"]).all()
    big = np.array([[2 ** 40 + 1, 3], [5, 2 ** 33]])                               # beyond float32 and int32
    assert R.same_metrics(M.metrics_from_matrix(big), R.metrics(big))


def test_topk_reference_rules():
    x = np.array([[1.0, 3.0, 3.0, 2.0], [5.0, 5.0, 5.0, 5.0], [0.0, np.nan, 1.0, 2.0], [1.0, 2.0, 3.0, 4.0]], np.float32)
    assert R.topk_counts(x, [2, 3, 1, 9], (1, 2, 4)) == [0, 1, 2, 4]                # second of a tie; last of a tie; NaN; out of range
    assert R.topk_counts(x[:2], [1, 0], (1,)) == [2, 2]


@pytest.fixture
def no_device(monkeypatch):
    def no_launch(*a, **k):
        raise AssertionError("a refused call reached the library or the device")
    monkeypatch.setattr(_lib, "call", no_launch)
    monkeypatch.setattr(M, "device", no_launch)
    monkeypatch.setattr(M, "_to_device", no_launch)
    monkeypatch.setattr(P, "wrap", no_launch)


def test_confusion_matrix_refusals_before_any_launch(no_device):
    for bad in (0, 257, -3):
        with pytest.raises(ValueError, match="must be in 1 .. 256"):
            M.ConfusionMatrix(bad)
    with pytest.raises(ValueError, match="must be an integer"):
        M.ConfusionMatrix("many")
    cm = M.ConfusionMatrix(21)
    lg, lab = np.zeros((2, 4, 5, 21), np.float32), np.zeros((2, 8, 10), np.uint8)
    with pytest.raises(ValueError, match="dtype must be float32 or bfloat16"):
        cm.update_logits(lg.astype(np.float64), lab)
    with pytest.raises(ValueError, match="labels: dtype must be uint8 or int32"):
        cm.update_logits(lg, lab.astype(np.int64))
    with pytest.raises(ValueError, match="labels: dtype must be uint8 or int32"):
        cm.update_logits(lg, torch.zeros((2, 8, 10), dtype=torch.float32))
    with pytest.raises(ValueError, match="labels: expected a numpy array or torch tensor"):
        cm.update_logits(lg, [[0]])
    with pytest.raises(ValueError, match="numpy array or torch tensor"):
        cm.update_logits([[0.0]], lab)
    with pytest.raises(ValueError, match=r"labels must be \[B, H, W\] or \[H, W\]"):
        cm.update_logits(lg, np.zeros((8,), np.uint8))
    with pytest.raises(ValueError, match="batch of them"):
        cm.update_logits(np.zeros((4, 21), np.float32), lab)
    with pytest.raises(ValueError, match="down-sampling"):
        cm.update_logits(lg, np.zeros((2, 3, 10), np.uint8))
    with pytest.raises(ValueError, match="down-sampling"):
        cm.update_logits(lg, np.zeros((2, 8, 4), np.uint8))
    with pytest.raises(ValueError, match="logits have 20 classes, the matrix 21"):
        cm.update_logits(lg[..., :20], lab)
    with pytest.raises(ValueError, match="257 classes"):
        cm.update_logits(np.zeros((1, 2, 2, 257), np.float32), np.zeros((1, 4, 4), np.uint8))
    with pytest.raises(ValueError, match="one is batched"):
        cm.update_logits(lg, lab[0])
    with pytest.raises(ValueError, match="one is batched"):
        cm.update_logits(lg[0], lab)
    with pytest.raises(ValueError, match=r"labels have shape \(3, 8, 10\), expected \(2, 8, 10\)"):
        cm.update_logits(lg, np.zeros((3, 8, 10), np.uint8))
    with pytest.raises(ValueError, match="empty"):
        cm.update_logits(lg[:0], lab[:0])
    # two label maps
    with pytest.raises(ValueError, match="pred: dtype must be uint8 or int32"):
        cm.update(np.zeros((4, 4), np.int16), np.zeros((4, 4), np.uint8))
    with pytest.raises(ValueError, match="labels: dtype must be uint8 or int32"):
        cm.update(np.zeros((4, 4), np.uint8), np.zeros((4, 4), np.float32))
    with pytest.raises(ValueError, match=r"labels have shape \(4, 5\), expected \(4, 4\)"):
        cm.update(np.zeros((4, 4), np.uint8), np.zeros((4, 5), np.int32))
    with pytest.raises(ValueError, match="empty prediction"):
        cm.update(np.zeros((0, 4), np.uint8), np.zeros((0, 4), np.uint8))
    with pytest.raises(ValueError, match="pred: expected a numpy array or torch tensor"):
        cm.update(3, np.zeros((4, 4), np.uint8))


def test_evaluate_segmentation_refusals_before_any_launch(no_device):
    class NotAModel:
        pass
    cm = M.ConfusionMatrix(21)
    x, lab = np.zeros((1, 3, 8, 8), np.float32), np.zeros((1, 8, 8), np.uint8)
    with pytest.raises(ValueError, match="segmentation model"):
        M.evaluate_segmentation(NotAModel(), x, lab, cm)
    with pytest.raises(ValueError, match="cm must be a metrics.ConfusionMatrix"):
        M.evaluate_segmentation(NotAModel(), x, lab, None)
    with pytest.raises(ValueError, match=r"labels must be \[B, H, W\]"):
        M.evaluate_segmentation(NotAModel(), x, lab[0], cm)
    with pytest.raises(ValueError, match="dtype must be uint8 or int32"):
        M.evaluate_segmentation(NotAModel(), x, lab.astype(np.int64), cm)


def test_topk_refusals_before_any_launch(no_device):
    for bad in ((), (0,), (1, -5), tuple(range(1, 10))):
        with pytest.raises(ValueError, match="must be 1 .. 8 values, each at least 1"):
            M.TopK(bad)
    with pytest.raises(ValueError, match="must be integers"):
        M.TopK(("one",))
    acc = M.TopK((1, 5))
    x, lab = np.zeros((3, 10), np.float32), np.zeros((3,), np.int32)
    with pytest.raises(ValueError, match="dtype must be float32"):
        acc.update(torch.zeros((3, 10), dtype=torch.bfloat16), lab)
    with pytest.raises(ValueError, match=r"logits must be \[B, K\]"):
        acc.update(x[0], lab)
    with pytest.raises(ValueError, match="65536"):
        acc.update(np.zeros((1, 65537), np.float32), lab[:1])
    with pytest.raises(ValueError, match="there must be a row"):
        acc.update(x[:0], lab[:0])
    with pytest.raises(ValueError, match="labels: dtype must be int32"):
        acc.update(x, lab.astype(np.int64))
    with pytest.raises(ValueError, match="labels: dtype must be int32"):
        acc.update(x, torch.zeros((3,), dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"labels have shape \(4,\), expected \(3,\)"):
        acc.update(x, np.zeros((4,), np.int32))
    with pytest.raises(ValueError, match="labels: expected a numpy array or torch tensor"):
        acc.update(x, [0, 1, 2])


def test_single_process_reduce_is_a_no_op():
    cm = M.ConfusionMatrix(3, device="cpu")
    cm.mat[1, 2] = 2 ** 40 + 1
    cm.reduce_over_ranks()
    assert int(cm.mat[1, 2]) == 2 ** 40 + 1 and int(cm.mat.sum()) == 2 ** 40 + 1
    assert cm.compute()["iou"][1] == 0.0
    cm.reset()
    assert not cm.mat.any()
    acc = M.TopK((1, 3), device="cpu")
    acc.counts.copy_(torch.tensor([1, 3, 4]))
    acc.reduce_over_ranks()
    assert acc.compute() == {"top1": 0.25, "top3": 0.75, "count": 4}
    acc.reset()
    assert np.isnan(acc.compute()["top1"]) and acc.compute()["count"] == 0


def test_confusion_entries_argument_errors_do_not_need_a_gpu(built_lib):
    f = built_lib.mv_confusion_from_logits
    ok = (1, 2, 2, 3, 4, 4, 0, 1)                                       # B, h, w, C, H, W, dtype, label bytes
    for ptrs in ((None, 4, 8), (4, None, 8), (4, 4, None)):
        assert f(*ptrs, *ok, None) == -1 and b"NULL" in built_lib.mv_last_error()
    for dims in ((0, 2, 2, 3, 4, 4), (1, 0, 2, 3, 4, 4), (1, 2, -1, 3, 4, 4), (1, 2, 2, 3, 0, 4), (1, 2, 2, 3, 4, -2)):
        assert f(4, 4, 8, *dims, 0, 1, None) == -1 and b"bad dimensions" in built_lib.mv_last_error()
    for C in (0, -1, 257):
        assert f(4, 4, 8, 1, 2, 2, C, 4, 4, 0, 1, None) == -1 and b"classes (1 .. 256)" in built_lib.mv_last_error()
    assert f(4, 4, 8, 1, 2, 2, 3, 4, 4, 2, 1, None) == -1 and b"dtype" in built_lib.mv_last_error()
    for lb in (0, 2, 8):
        assert f(4, 4, 8, 1, 2, 2, 3, 4, 4, 0, lb, None) == -1 and b"uint8 or int32" in built_lib.mv_last_error()
    assert f(4, 4, 8, 1, 5, 2, 3, 4, 4, 0, 1, None) == -1 and b"down-sampling" in built_lib.mv_last_error()
    assert f(4, 4, 8, 1, 2, 5, 3, 4, 4, 1, 4, None) == -1 and b"down-sampling" in built_lib.mv_last_error()
    assert f(4, 5, 8, 1, 2, 2, 3, 4, 4, 0, 4, None) == -1 and b"4-byte aligned" in built_lib.mv_last_error()
    g = built_lib.mv_confusion_from_labels
    for ptrs in ((None, 4, 8), (4, None, 8), (4, 4, None)):
        assert g(*ptrs, 16, 3, 1, 1, None) == -1 and b"NULL" in built_lib.mv_last_error()
    for n in (0, -4):
        assert g(4, 4, 8, n, 3, 1, 1, None) == -1 and b"bad size" in built_lib.mv_last_error()
    for C in (0, 257):
        assert g(4, 4, 8, 16, C, 1, 1, None) == -1 and b"classes (1 .. 256)" in built_lib.mv_last_error()
    for widths in ((2, 1), (1, 3), (0, 4)):
        assert g(4, 4, 8, 16, 3, *widths, None) == -1 and b"uint8 or int32" in built_lib.mv_last_error()
    assert g(5, 4, 8, 16, 3, 4, 1, None) == -1 and b"4-byte aligned" in built_lib.mv_last_error()
    assert g(4, 6, 8, 16, 3, 1, 4, None) == -1 and b"4-byte aligned" in built_lib.mv_last_error()


def test_topk_correct_entry_argument_errors_do_not_need_a_gpu(built_lib):
    import ctypes
    f = built_lib.mv_topk_correct_f32
    ks = (ctypes.c_int * 2)(1, 5)
    for ptrs in ((None, 4, 8), (4, None, 8), (4, 4, None)):
        assert f(*ptrs, 2, 10, ks, 2, None) == -1 and b"NULL" in built_lib.mv_last_error()
    assert f(4, 4, 8, 2, 10, None, 2, None) == -1 and b"NULL" in built_lib.mv_last_error()
    for B, K in ((0, 10), (2, 0), (2, 65537)):
        assert f(4, 4, 8, B, K, ks, 2, None) == -1 and b"bad dimensions" in built_lib.mv_last_error()
    for nk in (0, 9):
        assert f(4, 4, 8, 2, 10, ks, nk, None) == -1 and b"nk=" in built_lib.mv_last_error()
    assert f(4, 4, 8, 2, 10, (ctypes.c_int * 2)(1, 0), 2, None) == -1 and b"k=0" in built_lib.mv_last_error()


# ------------------------------------------------------------------------------------------------ the GPU tests' inputs
@pytest.mark.parametrize("C", R.CLASS_COUNTS)
@pytest.mark.parametrize("dtype", [np.uint8, np.int32])
def test_gpu_inputs_satisfy_their_preconditions(C, dtype):
    """Targets: every class occurs, and between 5 % and 30 % of the pixels hold a value that must not be counted (uint8 with 256
    classes is the one exception: every byte is a class, nothing can be ignored); int32 targets include negatives.  Predictions:
    every class where the case says so -- for the logits, judged on the float64 label map of the same logits."""
    for (b, h, w), (H, W) in R.LOGIT_SHAPES:
        t = R.targets(b * H * W, C, dtype, 5)
        tt = t.astype(np.int64)
        assert set(range(C)) <= set(tt.tolist())
        if C == 256 and dtype == np.uint8:
            assert R.ignored_share(t, C) == 0.0
        else:
            assert 0.05 <= R.ignored_share(t, C) <= 0.30
            assert (tt == 255).any() or C == 256
            assert ((tt >= C) & (tt < 255)).any() or C >= 255
        if dtype == np.int32:
            assert (tt < 0).any() and (tt > 255).any()
        if C in R.ALL_CLASSES_PREDICTED:
            pred = PR.labels64(R.peaked_logits((b, h, w, C), 6), H, W)
            assert set(range(C)) == set(np.unique(pred).tolist())
    n = 4099
    p, t = R.predictions(n, C, dtype, 7), R.targets(n, C, dtype, 8)
    assert set(range(C)) == set(p.astype(np.int64).tolist()) and set(range(C)) <= set(t.astype(np.int64).tolist())
    assert n % 4 and (R.ignored_share(t, C) == 0.0 if (C == 256 and dtype == np.uint8) else 0.05 <= R.ignored_share(t, C) <= 0.30)
