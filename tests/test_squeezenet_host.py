"""CPU: the SqueezeNet surface (reference models/classification/squeezenet.py) -- structure, defaults, checkpoint order, the ceil-mode
pooling size rule, the new C-ABI entries' argument checks, the fragment packer, and which entries the bf16 forward calls (launch
recorder, no GPU)."""
import os
import tempfile

import numpy as np
import pytest

import eqxvision_amd as eqv
from eqxvision_amd import nn, ops, utils
from oracle import state as S
from tests import _squeezenet_ref as R
from tests.test_host import _launch_list

FACTORIES = {"1_0": eqv.models.squeezenet1_0, "1_1": eqv.models.squeezenet1_1}


@pytest.mark.parametrize("version", ["1_0", "1_1"])
def test_structure_and_defaults(version):
    from eqxvision_amd.models.classification.squeezenet import SqueezeNet, _Fire
    m = FACTORIES[version]()
    assert SqueezeNet.__fields__ == ("features", "classifier")
    assert _Fire.__fields__ == ("inplanes", "squeeze", "squeeze_activation", "expand1x1", "expand1x1_activation", "expand3x3",
                                "expand3x3_activation")
    L = m.features.layers
    assert len(L) == 13
    k, width = R.PLANS[version][0]
    assert isinstance(L[0], nn.Conv2d) and L[0].kernel_size == (k, k) and L[0].stride == (2, 2) and L[0].out_channels == width
    assert L[0].padding == (0, 0) and L[0].bias is not None and nn.act_name(L[1].fn) == "relu"
    pools = [2] + [i for i, v in R.PLANS[version][1].items() if v == "pool"]
    for i in pools:
        assert type(L[i]) is nn.MaxPool2d and L[i].use_ceil and (L[i].kernel_size, L[i].stride, L[i].padding) == ((3, 3), (2, 2), (0, 0))
    for i, inp, s, e1, e3 in R.fires(version):
        f = L[i]
        assert isinstance(f, _Fire) and f.inplanes == inp
        assert (f.squeeze.in_channels, f.squeeze.out_channels, f.squeeze.kernel_size) == (inp, s, (1, 1))
        assert (f.expand1x1.in_channels, f.expand1x1.out_channels, f.expand1x1.kernel_size) == (s, e1, (1, 1))
        assert (f.expand3x3.in_channels, f.expand3x3.out_channels, f.expand3x3.kernel_size, f.expand3x3.padding) == (s, e3, (3, 3), (1, 1))
        assert all(nn.act_name(a.fn) == "relu" for a in (f.squeeze_activation, f.expand1x1_activation, f.expand3x3_activation))
    drop, conv, act, pool = m.classifier.layers
    assert isinstance(drop, nn.Dropout) and drop.p == 0.5 and not drop.inference
    assert (conv.in_channels, conv.out_channels, conv.kernel_size) == (512, 1000, (1, 1)) and nn.act_name(act.fn) == "relu"
    assert pool.target_shape == (1, 1)


def test_constructor_arguments():
    from eqxvision_amd.models.classification.squeezenet import SqueezeNet
    m = SqueezeNet()                                                   # version "1_0", 1000 classes, dropout 0.5, PRNGKey(0) split in 10
    assert m.features.layers[0].kernel_size == (7, 7) and m.classifier.layers[1].out_channels == 1000
    keys = eqv.random.split(eqv.random.PRNGKey(0), 10)
    np.testing.assert_array_equal(m.features.layers[0].weight, nn.Conv2d(3, 96, 7, 2, key=keys[0]).weight)
    np.testing.assert_array_equal(m.classifier.layers[1].weight, nn.Conv2d(512, 1000, 1, key=keys[9]).weight)
    fk = eqv.random.split(keys[1], 3)                                  # a Fire splits its key in 3
    np.testing.assert_array_equal(m.features.layers[3].expand3x3.weight, nn.Conv2d(16, 64, 3, padding=1, key=fk[2]).weight)
    m = eqv.models.squeezenet1_1(num_classes=7, dropout=0.25, key=eqv.random.PRNGKey(3))
    assert m.classifier.layers[0].p == 0.25 and m.classifier.layers[1].out_channels == 7
    assert utils.CLASSIFICATION_URLS["squeezenet1_1"].startswith("https://download.pytorch.org/models/squeezenet1_1-")


@pytest.mark.parametrize("version", ["1_0", "1_1"])
def test_checkpoint_order_and_roundtrip(version):
    sd = R.squeezenet_state(version)
    ours = utils.state_dict(FACTORIES[version]())
    assert list(ours) == list(sd)
    i = R.fires(version)[0][0]
    assert list(sd)[2:8] == [f"features.{i}.{c}.{p}" for c in ("squeeze", "expand1x1", "expand3x3") for p in ("weight", "bias")]
    assert list(sd)[-2:] == ["classifier.1.weight", "classifier.1.bias"]
    for k in sd:
        assert np.asarray(ours[k]).size == sd[k].size, k
        assert np.asarray(ours[k]).shape[:1] == sd[k].shape[:1], k
    with tempfile.TemporaryDirectory() as td:
        p = os.path.join(td, "w.pth")
        S.save_pth(sd, p)
        back = utils.state_dict(FACTORIES[version](torch_weights=p))
    for k in sd:
        np.testing.assert_array_equal(np.asarray(back[k]).reshape(-1), sd[k].reshape(-1))


def test_ceil_pool_size_rule():
    pool = nn.MaxPool2d(3, 2, use_ceil=True)
    for H in range(5, 17):
        assert pool.output_size(H, H + 1) == (-(-(H - 3) // 2) + 1, -(-(H - 2) // 2) + 1)
    assert nn.MaxPool2d(3, 2).output_size(6, 7) == (2, 3)
    assert nn.MaxPool2d(3, 2, 1, use_ceil=True).output_size(6, 7) == (4, 4)           # (6 + 2 - 3) % 2 != 0; (7 + 2 - 3) % 2 == 0
    # floor mode: the module is what it was before the argument existed, attribute for attribute and leaf for leaf
    plain = nn.MaxPool2d(3, 2, 1)
    assert nn.MaxPool2d.__fields__ == ("kernel_size", "stride", "padding")
    assert plain.__dict__ == {"kernel_size": (3, 3), "stride": (2, 2), "padding": (1, 1)}
    assert nn.MaxPool2d(3, 2, 1, use_ceil=False).__dict__ == plain.__dict__ and not plain.use_ceil
    assert eqv.tree_inference(nn.Sequential([pool]), True).layers[0].use_ceil          # survives a rebuild of the tree


def test_supported_for_every_fire(built_lib):
    from eqxvision_amd import _lib
    BF, F32 = _lib.BF16, _lib.F32
    seen = set()
    for version in ("1_0", "1_1"):
        h = R.feature_shape(version, 224)                              # walk the 224-pixel map sizes
        k = R.PLANS[version][0][0]
        hw = -(-((224 - k) // 2 + 1 - 3) // 2) + 1
        for i, spec in sorted(R.PLANS[version][1].items()):
            if spec == "pool":
                hw = -(-(hw - 3) // 2) + 1
                continue
            _, s, e1, e3 = spec
            seen.add((version, i))
            assert built_lib.mv_fire_expand_supported(s, e1, e3, hw, hw, BF, BF) == 1, (version, i, hw)
        assert hw == h[1] == 13
    assert len(seen) == 16
    for hw in (1, 2, 300):
        assert built_lib.mv_fire_expand_supported(16, 64, 64, hw, hw, BF, BF) == 1
    assert built_lib.mv_fire_expand_supported(24, 64, 64, 13, 13, BF, BF) == 0
    assert built_lib.mv_fire_expand_supported(16, 64, 128, 13, 13, BF, BF) == 0
    assert built_lib.mv_fire_expand_supported(16, 96, 96, 13, 13, BF, BF) == 0
    assert built_lib.mv_fire_expand_supported(16, 64, 64, 13, 13, F32, BF) == 0
    assert built_lib.mv_fire_expand_supported(16, 64, 64, 13, 13, F32, F32) == 0
    assert built_lib.mv_fire_expand_supported(16, 64, 64, 0, 13, BF, BF) == 0
    assert built_lib.mv_fire_expand_supported(64, 256, 256, 13, 1000, BF, BF) == 0     # the halo rows would not fit LDS
    for flag in ("no_fire_expand", "force_generic"):
        _lib.set_flag(flag, 1)
        try:
            assert built_lib.mv_fire_expand_supported(16, 64, 64, 13, 13, BF, BF) == 0
        finally:
            _lib.set_flag(flag, 0)


def test_argument_errors_do_not_need_a_gpu(built_lib):
    rc = built_lib.mv_fire_expand_fwd(None, None, None, None, None, None, 1, 13, 13, 16, 64, 64, 1, 1, None)
    assert rc == -1 and b"NULL" in built_lib.mv_last_error()
    rc = built_lib.mv_fire_expand_fwd(1, 1, None, 1, None, 1, 1, 13, 13, 16, 64, 64, 1, 1, None)
    assert rc == -1 and b"in place" in built_lib.mv_last_error()
    rc = built_lib.mv_fire_expand_fwd(1, 1, None, 1, None, 2, 0, 13, 13, 16, 64, 64, 1, 1, None)
    assert rc == -1 and b"B=0" in built_lib.mv_last_error()
    rc = built_lib.mv_fire_expand_fwd(1, 1, None, 1, None, 2, 1, 13, 13, 24, 64, 64, 1, 1, None)
    assert rc not in (0, -1) and b"unsupported S=24" in built_lib.mv_last_error()
    rc = built_lib.mv_fire_expand_fwd(1, 1, None, 1, None, 2, 1, 13, 13, 16, 64, 64, 0, 0, None)
    assert rc not in (0, -1) and b"unsupported" in built_lib.mv_last_error()
    pool = lambda *a: built_lib.mv_maxpool2d_out_nhwc_fwd(*a)
    assert pool(None, None, 1, 6, 6, 8, 3, 3, 2, 2, 0, 0, 3, 3, 1, None) == -1 and b"bad args" in built_lib.mv_last_error()
    assert pool(1, 2, 1, 6, 6, 8, 3, 3, 2, 2, 0, 0, 4, 3, 1, None) == -1 and b"neither the floor nor the ceil" in built_lib.mv_last_error()
    assert pool(1, 2, 1, 7, 7, 8, 3, 3, 2, 2, 0, 0, 4, 3, 1, None) == -1           # 7: floor == ceil == 3
    assert pool(1, 2, 1, 6, 6, 8, 3, 3, 2, 2, 0, 0, 3, 3, 7, None) == -1 and b"dtype" in built_lib.mv_last_error()
    # kernel 2, stride 3 on 6 rows: the ceil size 3 would start its last window at row 6, outside the map
    assert pool(1, 2, 1, 6, 6, 8, 2, 2, 3, 3, 0, 0, 3, 3, 1, None) == -1 and b"last window" in built_lib.mv_last_error()


def _unpack(f, E, K):
    """The documented index formula (header, mv_fire_expand_fwd), inverted element by element."""
    wk = np.full((E, K), np.nan, np.float32)
    for lane in range(64):
        p = lane % 32
        chan = 16 * ((p // 4) % 2) + 4 * (p // 8) + p % 4
        for tile in range(E // 32):
            for step in range(K // 16):
                for e in range(8):
                    n, k = 32 * tile + chan, 16 * step + 8 * (lane // 32) + e
                    assert np.isnan(wk[n, k])
                    wk[n, k] = f[tile, step, lane, e]
    return wk


@pytest.mark.parametrize("S_", [16, 32, 48, 64])
def test_fragment_packer_round_trip(S_):
    rng = np.random.default_rng(S_)
    E = 4 * S_
    for k in (1, 3):
        w = rng.standard_normal((E, S_, k, k)).astype(np.float32)
        f = ops.fire_fragments(w)
        assert f.shape == (E // 32, k * k * S_ // 16, 64, 8) and f.dtype == np.float32
        wk = _unpack(f, E, k * k * S_)                                  # Wk[n][(3 r + s) * S + c]
        np.testing.assert_array_equal(wk.reshape(E, k, k, S_).transpose(0, 3, 1, 2), w)
    # a lane's accumulator registers 0 .. 15 (tile rows (e % 4) + 8 (e / 4) + 4 half) are 16 consecutive channels
    for half in (0, 1):
        rows = [(e % 4) + 8 * (e // 4) + 4 * half for e in range(16)]
        assert list(ops.FIRE_TILE_ROW[rows]) == list(range(16 * half, 16 * half + 16))
    with pytest.raises(ValueError):
        ops.fire_fragments(np.zeros((64, 24, 1, 1), np.float32))


NEW = "mv_fire_expand_fwd"


def test_launch_list_fused(monkeypatch, built_lib):
    names = _launch_list(monkeypatch, eqv.models.squeezenet1_1, lambda: R.squeezenet_state("1_1"), 4)
    assert names.count(NEW) == 8 and "mv_copy_rows" not in names
    for i, n in enumerate(names):
        if n == NEW:
            assert names[i - 1] == "mv_conv2d_nhwc_fwd"                 # its squeeze
    assert names.count("mv_conv2d_nhwc_fwd") == 8 + 1                    # ... and the classifier's convolution
    assert names.count("mv_maxpool2d_out_nhwc_fwd") == 3 and "mv_maxpool2d_nhwc_fwd" not in names
    assert names[0] == "mv_conv2d_nchw_fwd" and "mv_dropout_fwd" not in names and "mv_eltwise_fwd" not in names
    assert names[-2:] == ["mv_conv2d_nhwc_fwd", "mv_adaptive_avgpool2d_nhwc_fwd"]
    assert len(names) == 1 + 3 + 16 + 2


def test_launch_list_1_0(monkeypatch, built_lib):
    names = _launch_list(monkeypatch, eqv.models.squeezenet1_0, lambda: R.squeezenet_state("1_0"), 2)
    assert names.count(NEW) == 8 and "mv_copy_rows" not in names and len(names) == 1 + 3 + 16 + 2


def test_launch_list_switch_off(monkeypatch, built_lib):
    names = _launch_list(monkeypatch, eqv.models.squeezenet1_1, lambda: R.squeezenet_state("1_1"), 4, flags=("no_fire_expand",))
    assert NEW not in names
    assert names.count("mv_conv2d_nhwc_fwd") == 24 + 1 and names.count("mv_copy_rows") == 16
    assert names.count("mv_maxpool2d_out_nhwc_fwd") == 3
