"""CPU: the GoogLeNet surface (reference models/classification/googlenet.py) -- fields and their order, defaults, checkpoint order and
round trip, the weight packers of the two Inception kernels against plain numpy, the Dropout key schedule, the `_supported` answers for
the nine module shapes, which entries the bf16 forward calls (launch recorder, no GPU), and the refusal inside
filter_value_and_grad."""
import os
import tempfile
import warnings

import numpy as np
import pytest

import eqxvision_amd as eqv
from eqxvision_amd import nn, ops, utils
from oracle import np_ops as O
from oracle import state as S
from tests import _googlenet_ref as R
from tests._cpu_ops import cpu_ops
from tests.test_host import _launch_list

# read off the reference file (class annotations, in order)
GOOGLENET_FIELDS = ("aux_logits", "conv1", "maxpool1", "conv2", "conv3", "maxpool2", "inception3a", "inception3b", "maxpool3",
                    "inception4a", "inception4b", "inception4c", "inception4d", "inception4e", "maxpool4", "inception5a", "inception5b",
                    "aux1", "aux2", "avgpool", "dropout", "fc")
INCEPTION_FIELDS = ("branch1", "branch2", "branch3", "branch4")
AUX_FIELDS = ("conv", "fc1", "fc2", "dropout", "avgpool")
BASIC_FIELDS = ("conv", "bn")


def test_fields_and_defaults():
    import importlib
    G = importlib.import_module("eqxvision_amd.models.classification.googlenet")      # (the package attribute is the factory)
    assert G.GoogLeNet.__fields__ == GOOGLENET_FIELDS
    assert G._Inception.__fields__ == INCEPTION_FIELDS
    assert G.InceptionAux.__fields__ == AUX_FIELDS
    assert G.BasicConv2d.__fields__ == BASIC_FIELDS
    for name in ("GoogLeNet", "googlenet", "BasicConv2d", "_Inception", "InceptionAux"):
        assert getattr(eqv.models, name) is getattr(G, name)
    m = G.GoogLeNet()
    assert m.aux_logits is False and m.aux1 is None and m.aux2 is None
    assert m.dropout.p == 0.2 and m.fc.out_features == 1000 and m.fc.in_features == 1024 and m.avgpool.target_shape == (1, 1)
    c = m.conv1
    assert (c.conv.kernel_size, c.conv.stride, c.conv.padding, c.conv.bias) == ((7, 7), (2, 2), (3, 3), None)
    assert abs(c.bn.eps - 1e-3) < 1e-12 and c.bn.axis_name == "batch" and not c.bn.inference
    for p, k in ((m.maxpool1, 3), (m.maxpool2, 3), (m.maxpool3, 3), (m.maxpool4, 2)):
        assert p.use_ceil and (p.kernel_size, p.stride, p.padding) == ((k, k), (2, 2), (0, 0))
    for name, (cin, c1, c3r, c3, c5r, c5, cp) in R.INCEPTIONS.items():
        i = getattr(m, name)
        assert (i.branch1.conv.in_channels, i.branch1.conv.out_channels) == (cin, c1)
        assert [u.conv.out_channels for u in i.branch2.layers] == [c3r, c3]
        assert [u.conv.out_channels for u in i.branch3.layers] == [c5r, c5]
        assert i.branch3.layers[1].conv.kernel_size == (3, 3) and i.branch3.layers[1].conv.padding == (1, 1)      # the "5x5" bug
        pool, proj = i.branch4.layers
        assert (pool.kernel_size, pool.stride, pool.padding) == ((3, 3), (1, 1), (1, 1)) and pool.output_size(7, 9) == (7, 9)
        assert proj.conv.out_channels == cp and proj.conv.in_channels == cin
    a = G.GoogLeNet(num_classes=5, aux_logits=True, dropout=0.1, dropout_aux=0.6, key=eqv.random.PRNGKey(2))
    assert a.aux1.dropout.p == 0.6 and a.aux2.conv.conv.in_channels == 528 and a.aux1.conv.conv.in_channels == 512
    assert a.aux1.fc1.in_features == 2048 and a.aux1.fc2.out_features == 5 and a.aux1.avgpool.target_shape == (4, 4) and a.dropout.p == 0.1
    keys = eqv.random.split(eqv.random.PRNGKey(2), 20)
    np.testing.assert_array_equal(a.fc.weight, nn.Linear(1024, 5, key=keys[14]).weight)
    ik = eqv.random.split(keys[3], 5)                                  # a module splits its key in 5; index 5 is clamped to 4
    np.testing.assert_array_equal(a.inception3a.branch4.layers[1].conv.weight, nn.Conv2d(192, 32, 1, use_bias=False, key=ik[4]).weight)
    assert utils.CLASSIFICATION_URLS["googlenet"].startswith("https://download.pytorch.org/models/googlenet-")


def test_checkpoint_order_and_roundtrip():
    sd = R.googlenet_state()
    names = [k for k in sd if "num_batches" not in k]
    ours = utils.state_dict(eqv.tree_inference(eqv.utils.randomize_batchnorm(eqv.models.googlenet(aux_logits=True)), True))
    assert list(ours) == names
    heads = [k.split(".")[0] for k in names]
    order = ["conv1", "conv2", "conv3"] + list(R.INCEPTIONS) + ["aux1", "aux2", "fc"]
    assert [h for i, h in enumerate(heads) if i == 0 or heads[i - 1] != h] == order
    with tempfile.TemporaryDirectory() as td:
        p = os.path.join(td, "w.pth")
        S.save_pth(sd, p)
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            plain = eqv.models.googlenet(torch_weights=p)
            assert not [w for w in rec if "aux-branch" in str(w.message)]
        with pytest.warns(UserWarning, match="aux-branch weights are un-trained"):
            full = eqv.models.googlenet(torch_weights=p, aux_logits=True)
    assert plain.aux_logits is False and full.aux_logits is True and plain.aux1 is not None
    assert plain.fc.use_bias is True and plain.conv1.bn.channelwise_affine is True          # only `aux_logits` was switched
    for m in (plain, full):
        back = utils.state_dict(m)
        for k in names:
            np.testing.assert_array_equal(np.asarray(back[k]).reshape(-1), sd[k].reshape(-1))


def test_stacked_pointwise_packer():
    """Module 4b: branch 1 (160), the 3x3 reduce (112) and the "5x5" reduce (24 -> 32) of 512 inputs."""
    rng = np.random.default_rng(4)
    parts = [(rng.standard_normal((n, 512, 1, 1)).astype(np.float32), rng.standard_normal(n).astype(np.float32),
              rng.standard_normal(n).astype(np.float32)) for n in (160, 112, 24)]
    w, sc, sh, starts = ops.inception_stack(parts)
    assert w.shape == (160 + 112 + 32, 512) and sc.shape == sh.shape == (304,) and starts == [0, 160, 272]
    for (pw, ps, ph), s in zip(parts, starts):
        n = pw.shape[0]
        np.testing.assert_array_equal(w[s:s + n], pw[:, :, 0, 0])
        np.testing.assert_array_equal(sc[s:s + n], ps)
        np.testing.assert_array_equal(sh[s:s + n], ph)
    assert not w[296:].any() and not sc[296:].any() and not sh[296:].any()          # zero filters, zero scale, zero shift


def _unpack(f, tiles, K):
    """The documented index formula (header, mv_conv3x3_pair_fwd), inverted element by element."""
    wk = np.full((32 * tiles, K), np.nan, np.float32)
    for lane in range(64):
        p = lane % 32
        chan = 16 * ((p // 4) % 2) + 4 * (p // 8) + p % 4
        for tile in range(tiles):
            for step in range(K // 16):
                for e in range(8):
                    wk[32 * tile + chan, 16 * step + 8 * (lane // 32) + e] = f[tile, step, lane, e]
    assert not np.isnan(wk).any()
    return wk


@pytest.mark.parametrize("N,S_,Sp", [(48, 16, 16), (208, 96, 96), (64, 24, 32)])
def test_fragment_packer(N, S_, Sp):
    """N % 32 == 16 (48, 208): the upper half of the last tile is zero rows; c5r = 24: the input channels 24 .. 31 are zero columns."""
    rng = np.random.default_rng(N + S_)
    w = rng.standard_normal((N, S_, 3, 3)).astype(np.float32)
    f = ops.inception_fragments(w, Sp)
    tiles = (N + 31) // 32
    assert f.shape == (tiles, 9 * Sp // 16, 64, 8) and f.dtype == np.float32
    wk = _unpack(f, tiles, 9 * Sp).reshape(32 * tiles, 3, 3, Sp).transpose(0, 3, 1, 2)          # Wk[n][(3 r + s) * Sp + c]
    np.testing.assert_array_equal(wk[:N, :S_], w)
    assert not wk[N:].any() and not wk[:, S_:].any()
    with pytest.raises(ValueError):
        ops.inception_fragments(np.zeros((40, 16, 3, 3), np.float32))
    with pytest.raises(ValueError):
        ops.inception_fragments(np.zeros((48, 24, 3, 3), np.float32))


def test_dropout_key_schedule(monkeypatch):
    """The main Dropout is handed element 13 of the 14-way split of the sample's key (the reference indexes 15, jax clamps), an
    auxiliary head's Dropout element 1 of the 2-way split of elements 7 (aux1) / 11 (aux2)."""
    import torch
    seen = []

    def fake_dropout(x, p, key, per_row=False):
        seen.append((p, np.asarray(key, np.uint32).copy()))
        return x
    calls = cpu_ops(monkeypatch)
    monkeypatch.setattr(ops, "dropout", fake_dropout)
    monkeypatch.setattr(ops, "bn_train_update", lambda bn, y: (torch.ones(bn.input_size), torch.zeros(bn.input_size)))
    m = eqv.models.googlenet(aux_logits=True, num_classes=8)          # training mode: the Dropouts are live
    keys = eqv.random.split(eqv.random.PRNGKey(11), 2)
    with eqv.precision("bf16"):
        out = eqv.vmap(m, axis_name="batch")(torch.zeros(2, 3, 64, 64), key=keys)
    assert isinstance(out, tuple) and len(out) == 3
    assert [p for p, _ in seen] == [0.7, 0.7, 0.2]                     # aux1, aux2, main: the order of the forward
    for b in range(2):
        ks = eqv.random.split(keys[b], 14)
        np.testing.assert_array_equal(ks, O.jax_split(np.asarray(keys[b], np.uint32), 14))
        np.testing.assert_array_equal(seen[2][1][b], ks[13])
        np.testing.assert_array_equal(seen[0][1][b], eqv.random.split(ks[7], 2)[1])
        np.testing.assert_array_equal(seen[1][1][b], eqv.random.split(ks[11], 2)[1])
    masks = R.dropout_masks(keys)
    np.testing.assert_array_equal(masks["main"][1], O.jax_bernoulli(eqv.random.split(keys[1], 14)[13], 0.8, (1024,)))
    names = [c[0] for c in calls]
    assert "mv_copy_rows" in names and "mv_conv3x3_pair_fwd" not in names          # training mode is the literal composition


def test_supported_for_every_module(built_lib):
    from eqxvision_amd import _lib
    BF, F32 = _lib.BF16, _lib.F32
    assert len(R.INCEPTIONS) == 9
    for name, (C, c1, c3r, c3, c5r, c5, cp) in R.INCEPTIONS.items():
        hw = R.MAP_224[name]
        c5p = (c5r + 15) // 16 * 16
        lt, Ct = c3r + c5p, c1 + c3 + c5 + cp
        assert built_lib.mv_conv1x1_split_supported(C, c1 + lt, c1, Ct, 0, lt, 0, BF, BF) == 1, name
        assert built_lib.mv_conv1x1_split_supported(C, cp, cp, Ct, c1 + c3 + c5, 0, 0, BF, BF) == 1, name
        assert built_lib.mv_conv3x3_pair_supported(c3r, c5p, c3, c5, hw, hw, BF, BF) == 1, name
    assert R.map_sizes(224) == (28, 14, 7)
    ok1 = (192, 176, 64, 256, 0, 112, 0)
    assert built_lib.mv_conv1x1_split_supported(*ok1, BF, BF) == 1
    for i, bad in ((0, 200), (1, 168), (2, 72), (3, 264), (4, 8), (5, 120), (6, 8)):              # a width that is no multiple of 16
        args = list(ok1)
        args[i] = bad
        assert built_lib.mv_conv1x1_split_supported(*args, BF, BF) == 0, (i, bad)
    assert built_lib.mv_conv1x1_split_supported(192, 176, 64, 48, 0, 112, 0, BF, BF) == 0       # the slice does not fit the row
    assert built_lib.mv_conv1x1_split_supported(*ok1, F32, BF) == 0
    ok3 = (96, 16, 208, 48, 14, 14)
    assert built_lib.mv_conv3x3_pair_supported(*ok3, BF, BF) == 1
    for i, bad in ((0, 24), (1, 24), (2, 200), (3, 40), (4, 0)):
        args = list(ok3)
        args[i] = bad
        assert built_lib.mv_conv3x3_pair_supported(*args, BF, BF) == 0, (i, bad)
    assert built_lib.mv_conv3x3_pair_supported(*ok3, BF, F32) == 0
    assert built_lib.mv_conv3x3_pair_supported(192, 48, 384, 128, 7, 1000, BF, BF) == 0        # the halo rows would not fit LDS
    for flag in ("no_inception_fused", "force_generic"):
        _lib.set_flag(flag, 1)
        try:
            assert built_lib.mv_conv1x1_split_supported(*ok1, BF, BF) == 0 and built_lib.mv_conv3x3_pair_supported(*ok3, BF, BF) == 0
        finally:
            _lib.set_flag(flag, 0)


def test_argument_errors_do_not_need_a_gpu(built_lib):
    s = lambda *a: built_lib.mv_conv1x1_split_fwd(*a)
    assert s(None, None, None, None, None, 64, 0, None, 0, 0, 4, 16, 16, 16, 1, 1, None) == -1 and b"NULL" in built_lib.mv_last_error()
    assert s(1, 2, 3, 4, 1, 64, 0, None, 0, 0, 4, 16, 16, 16, 1, 1, None) == -1 and b"in place" in built_lib.mv_last_error()
    assert s(1, 2, 3, 4, 5, 64, 0, None, 0, 0, 0, 16, 16, 16, 1, 1, None) == -1 and b"M=0" in built_lib.mv_last_error()
    assert s(1, 2, 3, 4, 5, 64, 0, None, 0, 0, 4, 16, 32, 16, 1, 1, None) == -1 and b"dst1 goes with" in built_lib.mv_last_error()
    assert s(1, 2, 3, 4, 5, 64, 0, None, 0, 0, 4, 24, 16, 16, 1, 1, None) not in (0, -1) and b"unsupported C=24" in built_lib.mv_last_error()
    q = lambda *a: built_lib.mv_conv3x3_pair_fwd(*a)
    ok = [1, 64, 0, 32, 32, 16, 2, 3, 4, 5, 6, 7, 8, 112, 16, 48, 64, 16, 1, 5, 5, 1, 1, None]
    bad = list(ok); bad[0] = None
    assert q(*bad) == -1 and b"NULL" in built_lib.mv_last_error()
    bad = list(ok); bad[12] = 1
    assert q(*bad) == -1 and b"in place" in built_lib.mv_last_error()
    bad = list(ok); bad[3] = 24
    assert q(*bad) not in (0, -1) and b"unsupported S0=24" in built_lib.mv_last_error()
    bad = list(ok); bad[4] = 56
    assert q(*bad) == -1 and b"multiples of 16" in built_lib.mv_last_error()
    bad = list(ok); bad[1] = 32
    assert q(*bad) == -1 and b"slices" in built_lib.mv_last_error()
    bad = list(ok); bad[16] = 48
    assert q(*bad) == -1 and b"output slices" in built_lib.mv_last_error()          # [16, 64) and [48, 64) overlap


NEW = ("mv_conv1x1_split_fwd", "mv_conv3x3_pair_fwd")


def test_launch_list_fused(monkeypatch, built_lib):
    names = _launch_list(monkeypatch, eqv.models.googlenet, R.googlenet_state, 2)
    assert names.count(NEW[0]) == 18 and names.count(NEW[1]) == 9 and "mv_copy_rows" not in names
    assert names.count("mv_maxpool2d_nhwc_fwd") == 9 and names.count("mv_maxpool2d_out_nhwc_fwd") == 4
    i = names.index(NEW[0])
    assert names[i:i + 4] == [NEW[0], "mv_maxpool2d_nhwc_fwd", NEW[0], NEW[1]]
    assert names[0] == "mv_conv2d_nchw_fwd" and names.count("mv_conv2d_nhwc_fwd") == 2 and "mv_dropout_fwd" not in names
    assert names[-2:] == ["mv_adaptive_avgpool2d_nhwc_fwd", "mv_linear_fwd"]
    assert len(names) == 1 + 2 + 4 + 9 * 4 + 2


def test_launch_list_switch_off(monkeypatch, built_lib):
    names = _launch_list(monkeypatch, eqv.models.googlenet, R.googlenet_state, 2, flags=("no_inception_fused",))
    assert NEW[0] not in names and NEW[1] not in names
    assert names.count("mv_conv2d_nhwc_fwd") == 2 + 9 * 6 and names.count("mv_copy_rows") == 9 * 4
    assert names.count("mv_maxpool2d_nhwc_fwd") == 9 and names.count("mv_maxpool2d_out_nhwc_fwd") == 4


def test_grad_refuses(monkeypatch):
    """Inside filter_value_and_grad (grad.active()) the model, a module, an auxiliary head and a conv unit refuse before any launch."""
    import torch
    from eqxvision_amd import _lib, grad as _grad
    from eqxvision_amd._act import Act
    monkeypatch.setattr(_grad, "active", lambda: True)
    monkeypatch.setattr(_lib, "call", lambda name, *a: pytest.fail(f"{name} was launched"))
    m = eqv.models.googlenet(num_classes=3, aux_logits=True)
    x = Act(torch.zeros(1, 3, 32, 32), "img", True)
    for mod in (m, m.conv1, m.inception3a, m.aux1):
        with pytest.raises(NotImplementedError, match="without a backward"):
            mod(x, key=eqv.random.split(eqv.random.PRNGKey(0), 1))
