"""CPU: the ConvNeXt surface (reference models/classification/convnext.py) -- structure, errors, checkpoint order, the two
restatements against each other, and which C-ABI entries the bf16 forward calls (launch recorder, no GPU)."""
import os
import tempfile
import warnings

import numpy as np
import pytest

import eqxvision_amd as eqv
from eqxvision_amd import nn, utils
from oracle import state as S
from tests import _convnext_ref as R
from tests.test_host import _launch_list as _host_launch_list

FACTORIES = {"convnext_tiny": eqv.models.convnext_tiny, "convnext_small": eqv.models.convnext_small,
             "convnext_base": eqv.models.convnext_base, "convnext_large": eqv.models.convnext_large}


@pytest.mark.parametrize("arch", list(FACTORIES))
def test_structure(arch):
    from eqxvision_amd.models.classification.convnext import CNBlock
    m = FACTORIES[arch]()
    setting = R.SETTINGS[arch]
    L = m.features.layers
    assert len(L) == 8
    stem = L[0]
    assert isinstance(stem[0], nn.Conv2d) and stem[0].kernel_size == (4, 4) and stem[0].stride == (4, 4) and stem[0].bias is not None
    assert isinstance(stem[1], nn.LayerNorm) and stem[1].eps == 1e-6 and len(stem) == 2
    probs = R._sd_probs(R.DEFAULT_SD[arch], setting)
    bid = 0
    for si, (cin, cout, n) in enumerate(setting):
        stage = L[1 + 2 * si]
        assert len(stage) == n
        for blk in stage:
            assert isinstance(blk, CNBlock)
            dw, ln, fc1, act, fc2 = blk.block.layers
            assert dw.groups == cin == dw.in_channels == dw.out_channels and dw.kernel_size == (7, 7) and dw.padding == (3, 3)
            assert ln.eps == 1e-5 and ln.shape == (cin,)
            assert (fc1.in_features, fc1.out_features, fc2.in_features, fc2.out_features) == (cin, 4 * cin, 4 * cin, cin)
            assert nn.act_name(act.fn) == "gelu"
            assert blk.layer_scale.shape == (cin, 1, 1) and blk.layer_scale.dtype == np.float32
            assert np.all(blk.layer_scale == np.float32(1e-6))
            assert blk.stochastic_depth.mode == "local" and blk.stochastic_depth.p == pytest.approx(probs[bid])
            bid += 1
        if cout is not None:
            down = L[2 + 2 * si]
            assert down[0].eps == 1e-6 and down[1].kernel_size == (2, 2) and down[1].stride == (2, 2)
            assert (down[1].in_channels, down[1].out_channels) == (cin, cout)
    assert bid == sum(n for *_, n in setting)
    last = setting[-1][0]
    assert m.classifier[0].eps == 1e-6 and m.classifier[2].in_features == last and m.classifier[2].out_features == 1000
    assert utils.CLASSIFICATION_URLS[arch].startswith("https://download.pytorch.org/models/" + arch + "-")


def test_reference_errors():
    from eqxvision_amd.models.classification.convnext import ConvNeXt, _CNBlockConfig, _convnext
    with pytest.raises(ValueError):
        ConvNeXt([])
    with pytest.raises(TypeError):
        ConvNeXt([(96, 192, 3)])
    with pytest.raises(ValueError, match="No checkpoint"):
        _convnext("convnext_huge", [_CNBlockConfig(8, None, 2)], 0.0, "w.pth")
    assert eqv.models.convnext_tiny(layer_scale=0.5).features.layers[1][0].layer_scale[0, 0, 0] == np.float32(0.5)
    assert eqv.models.convnext_tiny(stochastic_depth_prob=0.0).features.layers[7][2].stochastic_depth.p == 0.0


def test_checkpoint_order_and_roundtrip():
    sd = R.convnext_state(R.SETTINGS["convnext_tiny"])
    keys = list(sd)
    assert keys.index("features.1.0.layer_scale") < keys.index("features.1.0.block.0.weight")
    m = eqv.models.convnext_tiny()
    ours = utils.state_dict(m)
    assert len(ours) == len(sd)
    for (k1, v1), (k2, v2) in zip(ours.items(), sd.items()):
        assert np.asarray(v1).size == np.asarray(v2).size, (k1, k2)
        assert k1.rsplit(".", 1)[-1] == k2.rsplit(".", 1)[-1], (k1, k2)
    with tempfile.TemporaryDirectory() as td:
        p = os.path.join(td, "w.pth")
        S.save_pth(sd, p)
        m = eqv.models.convnext_tiny(torch_weights=p)
    back = utils.state_dict(m)
    for (k1, v1), (k2, v2) in zip(back.items(), sd.items()):
        np.testing.assert_array_equal(np.asarray(v1).reshape(-1), np.asarray(v2).reshape(-1))


def test_two_restatements_agree():
    setting = ((16, 32, 2), (32, None, 2))
    sd = R.convnext_state(setting, seed=3, num_classes=10)
    imgs = S.synthetic_images(2, 32, seed=1)
    t = R.forward_torch(sd, setting, imgs)
    n = np.stack([R.forward_numpy(sd, setting, im) for im in imgs])
    np.testing.assert_allclose(n, t, rtol=0, atol=1e-6 * max(1.0, np.abs(t).max()))
    keys = eqv.random.split(eqv.random.PRNGKey(5), 2)
    masks = R.training_masks(setting, keys, 0.5)
    assert any(m is not None and (m == 0).any() for m in masks[0])
    t = R.forward_torch(sd, setting, imgs, masks)
    n = np.stack([R.forward_numpy(sd, setting, im, masks[i]) for i, im in enumerate(imgs)])
    np.testing.assert_allclose(n, t, rtol=0, atol=1e-6 * max(1.0, np.abs(t).max()))


_launch_list = _host_launch_list        # tests/test_host.py's recorder


NEW = ("mv_cnblock_dw_fwd", "mv_ln_mlp_res_fwd", "mv_ln_mlp_stream_res_fwd")


def _dw_to_mlp(names):
    """[(dw entry, the entry right after it)]."""
    return [(names[i], names[i + 1]) for i, n in enumerate(names) if n == "mv_cnblock_dw_fwd"]


def test_launch_list_tiny(monkeypatch, built_lib):
    names = _launch_list(monkeypatch, eqv.models.convnext_tiny, lambda: R.convnext_state(R.SETTINGS["convnext_tiny"]), 4)
    assert names.count("mv_cnblock_dw_fwd") == 18
    assert names.count("mv_ln_mlp_res_fwd") == 3 and names.count("mv_ln_mlp_stream_res_fwd") == 12
    pairs = _dw_to_mlp(names)
    assert [b for _, b in pairs] == ["mv_ln_mlp_res_fwd"] * 3 + ["mv_ln_mlp_stream_res_fwd"] * 12 + ["mv_linear_fwd"] * 3
    i = [k for k, n in enumerate(names) if n == "mv_cnblock_dw_fwd"][-1]
    assert names[i + 1:i + 3] == ["mv_linear_fwd", "mv_linear_fwd"]
    assert "mv_dwconv2d_nhwc_fwd" not in names and "mv_channel_scale_nhwc_fwd" not in names
    assert names.count("mv_layernorm_fwd") == 3 + 1          # the three downsamples and the head; none inside a block
    assert "mv_add_fwd" not in names and "mv_eltwise_fwd" not in names
    assert names.count("mv_patch_merge_gather_nhwc") == 3 and "mv_cast" not in names


def test_launch_list_switches_off(monkeypatch, built_lib):
    names = _launch_list(monkeypatch, eqv.models.convnext_tiny, lambda: R.convnext_state(R.SETTINGS["convnext_tiny"]), 4,
                         flags=("no_cnblock_dw", "no_ln_mlp", "no_ln_mlp_stream"))
    assert not any(n in names for n in NEW)
    assert names.count("mv_dwconv2d_nhwc_fwd") == 18 and names.count("mv_add_fwd") == 18
    assert names[-1] == "mv_linear_fwd"


def test_launch_list_base_three_launch_form(monkeypatch, built_lib):
    names = _launch_list(monkeypatch, eqv.models.convnext_base, lambda: R.convnext_state(R.SETTINGS["convnext_base"]), 1)
    assert names.count("mv_cnblock_dw_fwd") == 36
    assert "mv_ln_mlp_res_fwd" not in names and "mv_ln_mlp_stream_res_fwd" not in names
    for i, n in enumerate(names):
        if n == "mv_cnblock_dw_fwd":
            assert names[i + 1:i + 3] == ["mv_linear_fwd", "mv_linear_fwd"]
