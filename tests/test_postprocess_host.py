"""CPU: the host half of `eqxvision_amd.postprocess` -- refusals before the device is touched, the argument checks of the two C
entries -- and the float64 restatements the GPU tests compare the kernels with (tests/_postprocess_ref.py) against torch's own
bilinear interpolation and a plain sort."""
import numpy as np
import pytest
import torch

from eqxvision_amd import _lib
from eqxvision_amd import postprocess as P
from tests import _postprocess_ref as R


@pytest.fixture
def no_device(monkeypatch):
    def no_launch(*a, **k):
        raise AssertionError("a refused call reached the library or the device")
    monkeypatch.setattr(_lib, "call", no_launch)
    monkeypatch.setattr(P, "device", no_launch)
    monkeypatch.setattr(P, "empty", no_launch)
    monkeypatch.setattr(P, "wrap", no_launch)


def test_upsample_argmax_refusals_before_any_launch(no_device):
    ok = np.zeros((2, 4, 5, 21), np.float32)
    with pytest.raises(ValueError, match="dtype"):
        P.upsample_argmax(ok.astype(np.float64), (8, 10))
    with pytest.raises(ValueError, match="dtype"):
        P.upsample_argmax(torch.zeros((2, 4, 5, 21), dtype=torch.float16), (8, 10))
    with pytest.raises(ValueError, match="dtype"):
        P.upsample_argmax(np.zeros((2, 4, 5, 21), np.uint8), (8, 10))
    with pytest.raises(ValueError, match="numpy array or torch tensor"):
        P.upsample_argmax([[1.0, 2.0]], (8, 10))
    with pytest.raises(ValueError, match="batch of them"):
        P.upsample_argmax(np.zeros((4, 21), np.float32), (8, 10))
    with pytest.raises(ValueError, match="batch of them"):
        P.upsample_argmax(np.zeros((1, 2, 4, 5, 21), np.float32), (8, 10))
    with pytest.raises(ValueError, match="257 classes"):
        P.upsample_argmax(np.zeros((1, 2, 3, 257), np.float32), (4, 6))
    with pytest.raises(ValueError, match="257 classes"):
        P.upsample_argmax(torch.zeros((257, 2, 3), dtype=torch.bfloat16), (4, 6), channels_last=False)
    with pytest.raises(ValueError, match="down-sampling"):
        P.upsample_argmax(ok, (3, 10))
    with pytest.raises(ValueError, match="down-sampling"):
        P.upsample_argmax(ok, (8, 4))
    with pytest.raises(ValueError, match="size must be"):
        P.upsample_argmax(ok, 8)
    with pytest.raises(ValueError, match="empty"):
        P.upsample_argmax(np.zeros((0, 4, 5, 21), np.float32), (8, 10))


def test_topk_refusals_before_any_launch(no_device):
    ok = np.zeros((2, 10), np.float32)
    with pytest.raises(ValueError, match="dtype"):
        P.topk(ok.astype(np.float64))
    with pytest.raises(ValueError, match="dtype"):
        P.topk(torch.zeros((2, 10), dtype=torch.bfloat16))          # bf16 logits are not taken
    with pytest.raises(ValueError, match=r"\[B, K\] or \[K\]"):
        P.topk(np.zeros((2, 3, 10), np.float32))
    with pytest.raises(ValueError, match=r"\[B, K\] or \[K\]"):
        P.topk(np.zeros((), np.float32))
    with pytest.raises(ValueError, match="k=11 must be in 1 .. K=10"):
        P.topk(ok, k=11)
    with pytest.raises(ValueError, match="k=0 must be"):
        P.topk(ok, k=0)
    with pytest.raises(ValueError, match="k=17 is more than the 16"):
        P.topk(np.zeros((2, 100), np.float32), k=17)
    with pytest.raises(ValueError, match="65536"):
        P.topk(np.zeros((1, 65537), np.float32), k=1)
    with pytest.raises(ValueError, match="there must be a row"):
        P.topk(np.zeros((0, 10), np.float32), k=1)


def test_segment_refuses_what_is_not_a_segmentation_model(no_device):
    class NotAModel:
        pass
    with pytest.raises(ValueError, match="segmentation model"):
        P.segment(NotAModel(), np.zeros((1, 3, 8, 8), np.float32))


def test_label_entry_argument_errors_do_not_need_a_gpu(built_lib):
    f = built_lib.mv_resize_argmax_nhwc_fwd
    assert f(None, 1, 1, 2, 2, 3, 4, 4, 0, None) == -1 and b"NULL" in built_lib.mv_last_error()
    assert f(1, None, 1, 2, 2, 3, 4, 4, 0, None) == -1 and b"NULL" in built_lib.mv_last_error()
    for dims in ((0, 2, 2, 3, 4, 4), (1, 0, 2, 3, 4, 4), (1, 2, 2, 0, 4, 4), (1, 2, 2, 3, 4, -1)):
        assert f(1, 1, *dims, 0, None) == -1 and b"bad dimensions" in built_lib.mv_last_error()
    assert f(1, 1, 1, 2, 2, 257, 4, 4, 0, None) == -1 and b"257 classes" in built_lib.mv_last_error()
    assert f(1, 1, 1, 2, 2, 3, 4, 4, 2, None) == -1 and b"dtype" in built_lib.mv_last_error()
    assert f(1, 1, 1, 5, 2, 3, 4, 4, 0, None) == -1 and b"down-sampling" in built_lib.mv_last_error()
    assert f(1, 1, 1, 2, 5, 3, 4, 4, 1, None) == -1 and b"down-sampling" in built_lib.mv_last_error()


def test_topk_entry_argument_errors_do_not_need_a_gpu(built_lib):
    f = built_lib.mv_softmax_topk_f32
    for ptrs in ((None, 1, 1), (1, None, 1), (1, 1, None)):
        assert f(*ptrs, 1, 10, 5, 1, None) == -1 and b"NULL" in built_lib.mv_last_error()
    assert f(1, 1, 1, 0, 10, 5, 1, None) == -1 and b"bad dimensions" in built_lib.mv_last_error()
    assert f(1, 1, 1, 1, 0, 1, 1, None) == -1 and b"bad dimensions" in built_lib.mv_last_error()
    assert f(1, 1, 1, 1, 65537, 1, 1, None) == -1 and b"bad dimensions" in built_lib.mv_last_error()
    assert f(1, 1, 1, 1, 10, 0, 1, None) == -1 and b"k=0" in built_lib.mv_last_error()
    assert f(1, 1, 1, 1, 10, 11, 1, None) == -1 and b"k=11" in built_lib.mv_last_error()
    assert f(1, 1, 1, 1, 100, 17, 1, None) == -1 and b"k=17" in built_lib.mv_last_error()
    assert f(1, 1, 1, 1, 10, 5, 2, None) == -1 and b"want_prob" in built_lib.mv_last_error()


@pytest.mark.parametrize("shape,size", [((2, 5, 7, 6), (13, 22)), ((1, 9, 4, 21), (9, 32))])
def test_resize_reference_agrees_with_torch(shape, size):
    """resize64 against interpolate(mode="bilinear", align_corners=False) on float64 CPU tensors.  Both evaluate the same two-tap
    filter in float64 and differ by the order of a handful of operations: a few 2^-53 relative to values below 8, so 1e-12 is four
    orders of slack.  The label maps must then be equal: with standard-normal logits the smallest top-two gap of these maps is far
    above 1e-12 (asserted)."""
    x = np.random.default_rng(5).standard_normal(shape)
    ref = R.resize64(x, *size)
    t = torch.nn.functional.interpolate(torch.from_numpy(x).permute(0, 3, 1, 2), size=size, mode="bilinear", align_corners=False)
    t = t.permute(0, 2, 3, 1).numpy()
    err = float(np.abs(ref - t).max())
    print(f"{shape} -> {size}: |ref - torch| = {err:.3e}")
    assert err <= 1e-12
    assert float(R.top2_gap(ref)[2].min()) > 1e-9
    assert np.array_equal(R.labels64(x, *size), t.argmax(-1))


def test_reference_argmax_rules():
    assert R.argmax_first(np.array([1.0, 3.0, 3.0, 2.0])) == 1                       # the first maximum
    assert R.argmax_first(np.array([1.0, np.nan, 5.0, np.nan])) == 1                 # a NaN beats every number, the first NaN wins
    assert R.argmax_first(np.array([-np.inf, -np.inf])) == 0
    first, second, gap = R.top2_gap(np.array([[1.0, 4.0, 4.0, 0.0], [2.0, 0.0, 1.0, -1.0]]))
    assert first.tolist() == [1, 0] and second.tolist() == [2, 2] and gap.tolist() == [0.0, 1.0]
    # weights: x2 of 3 pixels; rows sum to one, the outermost outputs read the edge pixel alone
    w = R.weights64(3, 6)
    assert np.allclose(w.sum(1), 1.0) and w[0].tolist() == [1.0, 0.0, 0.0] and w[5].tolist() == [0.0, 0.0, 1.0]
    assert np.array_equal(w[1], [0.75, 0.25, 0.0])
    assert R.touched_by(3, 6, 1).tolist() == [False, True, True, True, True, False]


@pytest.mark.parametrize("B,K,k", [(3, 50, 5), (2, 10, 10), (1, 1, 1), (2, 300, 16)])
def test_topk_reference_is_the_stable_descending_order(B, K, k):
    """topk_indices against a sort of (-value, index) pairs written out in Python, on integer logits with many ties; the selected
    probabilities sum to at most one and are those of the selected logits."""
    x = np.random.default_rng(7).integers(-3, 4, (B, K)).astype(np.float64)
    want = np.array([sorted(range(K), key=lambda i: (-row[i], i))[:k] for row in x])
    p, v, idx = R.topk64(x, k)
    assert np.array_equal(idx, want)
    assert np.array_equal(v, np.take_along_axis(x, want, -1)) and np.all(np.diff(v, axis=-1) <= 0)
    full = np.exp(x) / np.exp(x).sum(-1, keepdims=True)
    assert np.allclose(p, np.take_along_axis(full, want, -1), rtol=1e-13, atol=0) and np.all(p.sum(-1) <= 1.0 + 1e-12)
