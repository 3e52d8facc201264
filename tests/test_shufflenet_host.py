"""CPU: the ShuffleNetV2 surface (reference models/classification/shufflenetv2.py) -- structure, errors, checkpoint order, the two
restatements against each other, the folded layout's algebra in numpy, and which C-ABI entries the bf16 forward calls (launch
recorder, no GPU)."""
import os
import tempfile
import warnings

import numpy as np
import pytest

import eqxvision_amd as eqv
from eqxvision_amd import nn, ops, utils
from oracle import state as S
from tests import _shufflenet_ref as R
from tests.test_host import _launch_list as _host_launch_list

FACTORIES = {"shufflenet_v2_x0_5": eqv.models.shufflenet_v2_x0_5, "shufflenet_v2_x1_0": eqv.models.shufflenet_v2_x1_0,
             "shufflenet_v2_x1_5": eqv.models.shufflenet_v2_x1_5, "shufflenet_v2_x2_0": eqv.models.shufflenet_v2_x2_0}
PADDED = {"shufflenet_v2_x0_5": (24, 48, 96), "shufflenet_v2_x1_0": (64, 120, 232), "shufflenet_v2_x1_5": (88, 176, 352),
          "shufflenet_v2_x2_0": (128, 248, 488)}


@pytest.mark.parametrize("arch", list(FACTORIES))
def test_structure(arch):
    from eqxvision_amd.models.classification.shufflenetv2 import _InvertedResidual
    m = FACTORIES[arch]()
    repeats, widths = R.SETTINGS[arch]
    assert repeats == (4, 8, 4)
    c1 = m.conv1.layers
    assert (c1[0].in_channels, c1[0].out_channels, c1[0].kernel_size, c1[0].stride, c1[0].padding) == (3, widths[0], (3, 3), (2, 2), (1, 1))
    assert c1[0].bias is None and isinstance(c1[1], nn.BatchNorm) and nn.act_name(c1[2].fn) == "relu"
    assert (m.maxpool.kernel_size, m.maxpool.stride, m.maxpool.padding) == ((3, 3), (2, 2), (1, 1))
    cin = widths[0]
    for stage, n, cout, P in zip((m.stage2, m.stage3, m.stage4), repeats, widths[1:4], PADDED[arch]):
        assert len(stage) == n
        bf = cout // 2
        assert ops.shuffle_layout(bf) == (bf, P)
        for i, u in enumerate(stage):
            assert isinstance(u, _InvertedResidual) and u.stride == (2 if i == 0 else 1)
            b2 = u.branch2.layers
            assert len(b2) == 8
            assert (b2[0].in_channels, b2[0].out_channels, b2[0].kernel_size) == (cin if i == 0 else bf, bf, (1, 1))
            assert b2[3].groups == b2[3].in_channels == b2[3].out_channels == bf and b2[3].kernel_size == (3, 3)
            assert b2[3].stride == (u.stride, u.stride) and b2[3].padding == (1, 1)
            assert (b2[5].in_channels, b2[5].out_channels, b2[5].kernel_size) == (bf, bf, (1, 1))
            assert all(c.bias is None for c in (b2[0], b2[3], b2[5]))
            assert all(isinstance(b2[k], nn.BatchNorm) and b2[k].input_size == bf and b2[k].axis_name == "batch" for k in (1, 4, 6))
            b1 = u.branch1.layers
            if i == 0:
                assert len(b1) == 5 and b1[0].groups == b1[0].in_channels == b1[0].out_channels == cin and b1[0].stride == (2, 2)
                assert b1[0].kernel_size == (3, 3) and (b1[2].in_channels, b1[2].out_channels, b1[2].kernel_size) == (cin, bf, (1, 1))
            else:
                assert len(b1) == 1 and isinstance(b1[0], nn.Identity)
                assert not [k for k in utils.state_dict(u) if k.startswith("branch1")]      # no parameters
        cin = cout
    c5 = m.conv5.layers
    assert (c5[0].in_channels, c5[0].out_channels, c5[0].kernel_size) == (widths[3], widths[4], (1, 1))
    assert m.pool.target_shape == (1, 1) and (m.fc.in_features, m.fc.out_features) == (widths[4], 1000)


def test_urls():
    assert utils.CLASSIFICATION_URLS["shufflenetv2_x0.5"] == "https://download.pytorch.org/models/shufflenetv2_x0.5-f707e7126e.pth"
    assert utils.CLASSIFICATION_URLS["shufflenetv2_x1.0"] == "https://download.pytorch.org/models/shufflenetv2_x1-5666bf0f80.pth"
    from eqxvision_amd.models import classification as C
    assert C.shufflenet_v2_x2_0 is eqv.models.shufflenet_v2_x2_0 and C.ShuffleNetV2 is eqv.models.ShuffleNetV2


def test_reference_errors():
    from eqxvision_amd.models.classification.shufflenetv2 import ShuffleNetV2, _InvertedResidual
    with pytest.raises(ValueError, match="illegal stride value"):
        _InvertedResidual(8, 16, 4, key=eqv.random.PRNGKey(0))
    with pytest.raises(ValueError, match="illegal stride value"):
        _InvertedResidual(8, 16, 0, key=eqv.random.PRNGKey(0))
    with pytest.raises(AssertionError):
        _InvertedResidual(8, 20, 1, key=eqv.random.PRNGKey(0))
    with pytest.raises(ValueError, match="expected stages_repeats as list of 3 positive ints"):
        ShuffleNetV2([4, 8], [24, 48, 96, 192, 1024])
    with pytest.raises(ValueError, match="expected stages_out_channels as list of 5 positive ints"):
        ShuffleNetV2([4, 8, 4], [24, 48, 96, 192])
    assert eqv.models.shufflenet_v2_x0_5(num_classes=7).fc.out_features == 7


def test_checkpoint_order_and_roundtrip():
    sd = R.shufflenet_state(R.SETTINGS["shufflenet_v2_x0_5"])
    m = eqv.models.shufflenet_v2_x0_5()
    ours = [k for k in utils.state_dict(m)]
    want = [k for k in sd if "running" not in k and "num_batches" not in k]
    assert ours == want                                                 # an unloaded BatchNorm has no running statistics yet
    assert want[:3] == ["conv1.0.weight", "conv1.1.weight", "conv1.1.bias"] and want[3] == "stage2.0.branch1.0.weight"
    assert want[-3:] == ["conv5.1.bias", "fc.weight", "fc.bias"]
    with tempfile.TemporaryDirectory() as td:
        p = os.path.join(td, "w.pth")
        S.save_pth(sd, p)
        m = eqv.models.shufflenet_v2_x0_5(torch_weights=p)
    back = utils.state_dict(m)
    full = [k for k in sd if "num_batches" not in k]
    assert list(back) == full
    assert full[1:5] == ["conv1.1.weight", "conv1.1.bias", "conv1.1.running_mean", "conv1.1.running_var"]
    for k in full:
        np.testing.assert_array_equal(np.asarray(back[k]).reshape(-1), np.asarray(sd[k]).reshape(-1))


def test_two_restatements_agree():
    sd = R.shufflenet_state(R.SMALL, seed=3, num_classes=10)
    imgs = S.synthetic_images(2, 32, seed=1)
    t = R.forward_torch(sd, R.SMALL, imgs)
    n = np.stack([R.forward_numpy(sd, R.SMALL, im) for im in imgs])
    np.testing.assert_allclose(n, t, rtol=0, atol=1e-6 * max(1.0, np.abs(t).max()))


def _small_net(sd, num_classes=10):
    from eqxvision_amd.models.classification.shufflenetv2 import ShuffleNetV2
    with tempfile.TemporaryDirectory() as td:
        p = os.path.join(td, "w.pth")
        S.save_pth(sd, p)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            net = utils.load_torch_weights(ShuffleNetV2(list(R.SMALL[0]), list(R.SMALL[1]), num_classes=num_classes), p)
    return eqv.tree_inference(net, True)


def test_phys_index():
    assert ops.shuffle_phys_index(24, None).tolist() == list(range(24))
    idx = ops.shuffle_phys_index(20, (10, 16))
    assert idx.tolist() == [0, 16, 1, 17, 2, 18, 3, 19, 4, 20, 5, 21, 6, 22, 7, 23, 8, 24, 9, 25]
    with pytest.raises(ValueError):
        ops.shuffle_phys_index(24, (10, 16))


def test_folding_is_exact():
    """The folded layout end to end in fp32 numpy (ops.shuffle_fold_unit / shuffle_unit_numpy / shuffle_fold_head: the operands the
    device path uploads, no device): equal to the literal network, and every pad channel an exact zero after every unit."""
    sd = R.shufflenet_state(R.SMALL, seed=3, num_classes=10)
    net = _small_net(sd)
    imgs = S.synthetic_images(2, 32, seed=1)
    units = list(net.stage2.layers) + list(net.stage3.layers) + list(net.stage4.layers)
    got = []
    for im in imgs:
        x = R.np_stem(sd, im).transpose(1, 2, 0).astype(np.float32)          # [H][W][C], plain channels
        layout, C = None, x.shape[-1]
        for u in units:
            F = ops.shuffle_fold_unit(u, layout, C)
            assert F is not None
            x = ops.shuffle_unit_numpy(x, F)
            bf, P = F["bf"], F["P"]
            assert P % 8 == 0 and P >= bf and P - bf < 8 and x.shape[-1] == 2 * P
            assert P > bf                                                    # this setting has pads everywhere
            assert np.all(x[..., bf:P] == 0.0) and np.all(x[..., P + bf:] == 0.0)
            assert np.abs(x[..., :bf]).max() > 0 and np.abs(x[..., P:P + bf]).max() > 0
            layout, C = (bf, P), 2 * bf
        w, s, h = ops.shuffle_fold_head(net.conv5.layers[0], net.conv5.layers[1], layout)
        x = np.maximum(x @ w.T * s + h, 0.0)
        got.append(x.mean((0, 1)).astype(np.float64) @ np.asarray(sd["fc.weight"], np.float64).T + np.asarray(sd["fc.bias"], np.float64))
    got = np.stack(got)
    ref = np.stack([R.forward_numpy(sd, R.SMALL, im) for im in imgs])
    scale = max(1.0, float(np.abs(ref).max()))
    # fp32 arithmetic over 7 units against fp64: 1e-6 relative to the logit scale is ~8 ulp of fp32
    assert float(np.abs(got - ref).max()) <= 1e-6 * scale, float(np.abs(got - ref).max())


def test_fragment_packer():
    rng = np.random.default_rng(0)
    w = rng.standard_normal((24, 40)).astype(np.float32)
    f = ops.dwpw_fragments(w)
    assert f.shape == (2, 2, 4, 16, 8)
    for tile, step, g, r, e in ((0, 0, 0, 0, 0), (1, 0, 3, 7, 5), (0, 1, 0, 15, 7), (1, 1, 2, 3, 1)):
        n, k = 16 * tile + r, 32 * step + 8 * g + e
        assert f[tile, step, g, r, e] == (w[n, k] if n < 24 and k < 40 else 0.0)


def test_synthetic_state_window_and_shuffle_matters():
    setting = R.SETTINGS["shufflenet_v2_x0_5"]
    sd = R.shufflenet_state(setting, seed=1)
    x = S.synthetic_images(2, 224, seed=1)
    ref = R.forward_torch(sd, setting, x)
    assert 0.5 <= float(np.abs(ref).max()) <= 3.0
    plain = R.forward_torch(sd, setting, x, shuffle=False)
    assert float(np.abs(plain - ref).max()) > 10 * 1e-2


def test_supported_for_every_unit(built_lib):
    from eqxvision_amd import _lib
    for arch, (_, widths) in R.SETTINGS.items():
        hw, cin_phys = 56, widths[0]
        for cout, P in zip(widths[1:4], PADDED[arch]):
            assert built_lib.mv_shuffle_dwpw_supported(cin_phys, P, 2, hw, hw, _lib.BF16, _lib.BF16) == 1, (arch, cin_phys, P)
            assert built_lib.mv_shuffle_dwpw_supported(P, P, 2, hw, hw, _lib.BF16, _lib.BF16) == 1
            hw //= 2
            assert built_lib.mv_shuffle_dwpw_supported(P, P, 1, hw, hw, _lib.BF16, _lib.BF16) == 1
            cin_phys = 2 * P
    assert built_lib.mv_shuffle_dwpw_supported(58, 64, 1, 28, 28, _lib.BF16, _lib.BF16) == 0
    assert built_lib.mv_shuffle_dwpw_supported(64, 64, 3, 28, 28, _lib.BF16, _lib.BF16) == 0
    assert built_lib.mv_shuffle_dwpw_supported(64, 64, 1, 28, 28, _lib.F32, _lib.F32) == 0
    _lib.set_flag("no_shuffle_dwpw", 1)
    try:
        assert built_lib.mv_shuffle_dwpw_supported(64, 64, 1, 28, 28, _lib.BF16, _lib.BF16) == 0
    finally:
        _lib.set_flag("no_shuffle_dwpw", 0)


def test_argument_errors_do_not_need_a_gpu(built_lib):
    rc = built_lib.mv_shuffle_dwpw_fwd(None, None, None, None, None, None, None, None, 128, 64, 64, 58, None, 0, 0, 0, 0, 0,
                                       1, 28, 28, 64, 1, 1, 1, None)
    assert rc == -1 and b"NULL" in built_lib.mv_last_error()
    rc = built_lib.mv_shuffle_dwpw_fwd(1, 1, None, None, 1, None, None, 2, 128, 72, 64, 58, None, 0, 0, 0, 0, 0,
                                       1, 28, 28, 64, 1, 1, 1, None)
    assert rc == -1 and b"do not fit the pitch" in built_lib.mv_last_error()
    rc = built_lib.mv_shuffle_dwpw_fwd(1, 1, None, None, 1, None, None, 2, 128, 64, 64, 58, 3, 128, 64, 58, 0, 64,
                                       1, 28, 28, 64, 2, 1, 1, None)
    assert rc == -1 and b"stride 1" in built_lib.mv_last_error()
    rc = built_lib.mv_channel_gather_nhwc_fwd(None, None, None, 4, 4, 4, 1, None)
    assert rc == -1 and b"NULL" in built_lib.mv_last_error()


_launch_list = _host_launch_list        # tests/test_host.py's recorder


NEW = "mv_shuffle_dwpw_fwd"
ABSENT = ("mv_copy_rows", "mv_channel_gather_nhwc_fwd", "mv_dwconv2d_nhwc_fwd", "mv_add_fwd")


def _check_fused_list(names):
    assert names.count(NEW) == 19                      # 13 stride-1 units + 2 launches for each of the 3 stride-2 units
    heads = [i for i, n in enumerate(names) if n == "mv_conv2d_nhwc_fwd" and names[i + 1] == NEW]
    assert len(heads) == 16                            # every branch2 head: one 1x1 directly before its fused tail
    assert names.count("mv_conv2d_nhwc_fwd") == 16 + 1          # ... and conv5
    assert not any(n in names for n in ABSENT)
    i = [k for k, n in enumerate(names) if n == NEW]
    for stage_first in (i[0], i[5], i[14]):            # a stride-2 unit (stages of 4 / 8 / 4 units): dwpw, conv, dwpw
        assert names[stage_first:stage_first + 3] == [NEW, "mv_conv2d_nhwc_fwd", NEW]


@pytest.mark.parametrize("arch,B", [("shufflenet_v2_x1_0", 4), ("shufflenet_v2_x0_5", 1), ("shufflenet_v2_x2_0", 1)])
def test_launch_list_fused(monkeypatch, built_lib, arch, B):
    names = _launch_list(monkeypatch, FACTORIES[arch], lambda: R.shufflenet_state(R.SETTINGS[arch]), B)
    _check_fused_list(names)


def test_launch_list_switch_off(monkeypatch, built_lib):
    arch = "shufflenet_v2_x1_0"
    names = _launch_list(monkeypatch, FACTORIES[arch], lambda: R.shufflenet_state(R.SETTINGS[arch]), 4, flags=("no_shuffle_dwpw",))
    assert NEW not in names
    assert names.count("mv_channel_gather_nhwc_fwd") == 16
    # the split of every stride-1 unit and every concatenation (+ the compaction of convolutions whose output width is not a multiple of 8)
    assert names.count("mv_copy_rows") >= 13 * 2 + 16 * 2
