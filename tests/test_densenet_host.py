"""CPU: the DenseNet surface (reference models/classification/densenet.py) -- fields and their order, defaults, the constructor's key
indexing, checkpoint order and round trip, the `_supported` answers for every layer and transition shape of the four variants,
argument errors of the two kernels, which entries the bf16 forward calls (launch recorder, no GPU), the Dropout key schedule,
nn.AvgPool2d's output sizes and the refusal inside filter_value_and_grad."""
import os
import tempfile

import numpy as np
import pytest

import eqxvision_amd as eqv
from eqxvision_amd import nn, ops, utils
from oracle import np_ops as O
from oracle import state as S
from tests import _densenet_ref as R
from tests._cpu_ops import cpu_ops
from tests.test_host import _launch_list

NEW = ("mv_preact_conv1x1_fwd", "mv_conv3x3_slice_fwd")


def _mod():
    import importlib
    return importlib.import_module("eqxvision_amd.models.classification.densenet")


def test_fields_and_defaults():
    D = _mod()
    assert D.DenseNet.__fields__ == ("features", "classifier")
    assert D._DenseLayer.__fields__ == ("norm1", "relu", "conv1", "norm2", "conv2", "dropout")
    assert D._DenseBlock.__fields__ == ("layers", "num_layers")
    assert D._Transition.__fields__ == ("layers",)
    for name in ("DenseNet", "_DenseLayer", "_DenseBlock", "_Transition", "densenet121", "densenet161", "densenet169", "densenet201"):
        assert getattr(eqv.models, name) is getattr(D, name)
    m = D.DenseNet()
    assert [b.num_layers for b in m.features.layers[4:-3:2]] == [6, 12, 24, 16] and m.classifier.in_features == 1024
    for name, (g, cfg, c0) in R.VARIANTS.items():
        m = getattr(D, name)(num_classes=7)
        L = m.features.layers
        assert len(L) == 4 + 2 * len(cfg) - 1 + 3
        c = L[0]
        assert (c.in_channels, c.out_channels, c.kernel_size, c.stride, c.padding, c.bias) == (3, c0, (7, 7), (2, 2), (3, 3), None)
        assert abs(L[1].eps - 1e-5) < 1e-12 and L[1].axis_name == "batch" and not L[1].inference and L[1].momentum == 0.99
        assert (L[3].kernel_size, L[3].stride, L[3].padding) == ((3, 3), (2, 2), (1, 1)) and not L[3].use_ceil
        ch = c0
        for b, n in enumerate(cfg):
            blk = L[4 + 2 * b]
            assert type(blk) is D._DenseBlock and blk.num_layers == n == len(blk.layers)
            for i, l in enumerate(blk.layers):
                assert (l.norm1.input_size, l.conv1.in_channels, l.conv1.out_channels, l.conv1.kernel_size) == (ch, ch, 4 * g, (1, 1))
                assert (l.norm2.input_size, l.conv2.in_channels, l.conv2.out_channels) == (4 * g, 4 * g, g)
                assert (l.conv2.kernel_size, l.conv2.padding, l.conv2.bias, l.conv1.bias) == ((3, 3), (1, 1), None, None)
                assert l.dropout.p == 0.0 and nn.act_name(l.relu.fn) == "relu"
                ch += g
            if b != len(cfg) - 1:
                bn, lam, conv, pool = L[5 + 2 * b].layers.layers
                assert (bn.input_size, conv.in_channels, conv.out_channels, conv.bias) == (ch, ch, ch // 2, None)
                assert type(pool) is nn.AvgPool2d and (pool.kernel_size, pool.stride) == ((2, 2), (2, 2))
                ch //= 2
        assert L[-3].input_size == ch and L[-1].target_shape == (1, 1)
        assert (m.classifier.in_features, m.classifier.out_features) == (ch, 7) == (R.layer_shapes(name)[2], 7)
        assert utils.CLASSIFICATION_URLS[name].startswith(f"https://download.pytorch.org/models/{name}-")
    d = D.DenseNet(growth_rate=16, block_config=(2, 2), num_init_features=32, bn_size=2, drop_rate=0.2, num_classes=5)
    assert d.features.layers[4].layers[1].dropout.p == 0.2 and d.features.layers[4].layers[0].conv1.out_channels == 32


def test_constructor_key_indexing():
    """`keys` is re-bound to a 3-way split inside the block loop and jax clamps out-of-range indices: block 0 takes element 0 of
    split(keys10[1], 3) and transition 0 its element 2; from then on keys[2 i + 1] and keys[2 i + 2] are both the LAST element of the
    previous split; the classifier takes the last element of the last split."""
    D = _mod()
    key = eqv.random.PRNGKey(3)
    m = D.densenet121(num_classes=4, key=key)
    k10 = eqv.random.split(key, 10)
    np.testing.assert_array_equal(m.features.layers[0].weight, nn.Conv2d(3, 64, 7, 2, 3, use_bias=False, key=k10[0]).weight)
    ks = eqv.random.split(k10[1], 3)
    c, L = 64, m.features.layers
    for b, n in enumerate((6, 12, 24, 16)):
        if b:
            ks = eqv.random.split(ks[2], 3)
        np.testing.assert_array_equal(L[4 + 2 * b].layers[n - 1].conv2.weight,
                                      D._DenseBlock(n, c, 4, 32, 0.0, key=ks[0]).layers[n - 1].conv2.weight)
        c += 32 * n
        if b != 3:
            np.testing.assert_array_equal(L[5 + 2 * b].layers.layers[2].weight, nn.Conv2d(c, c // 2, 1, use_bias=False, key=ks[2]).weight)
            c //= 2
    np.testing.assert_array_equal(m.classifier.weight, nn.Linear(1024, 4, key=ks[2]).weight)


@pytest.mark.parametrize("variant", list(R.VARIANTS))
def test_checkpoint_order_and_roundtrip(variant):
    sd = R.densenet_state(variant, head_scale_=1.0)
    names = [k for k in sd if "num_batches" not in k]
    assert names[0] == "features.conv0.weight" and names[5] == "features.denseblock1.denselayer1.norm1.weight"
    assert names[9:11] == ["features.denseblock1.denselayer1.conv1.weight", "features.denseblock1.denselayer1.norm2.weight"]
    assert names[-6:] == ["features.norm5." + s for s in ("weight", "bias", "running_mean", "running_var")] + \
        ["classifier.weight", "classifier.bias"]
    with tempfile.TemporaryDirectory() as td:
        p = os.path.join(td, "w.pth")
        S.save_pth(sd, p)
        m = getattr(eqv.models, variant)(torch_weights=p)
    back = utils.state_dict(m)
    assert len(back) == len(names)
    for (ours, got), k in zip(back.items(), names):                    # same order; our names are attribute paths
        assert ours.rsplit(".", 1)[-1] == k.rsplit(".", 1)[-1], (ours, k)
        np.testing.assert_array_equal(np.asarray(got).reshape(-1), sd[k].reshape(-1))
    blk = m.features.layers[6]
    np.testing.assert_array_equal(blk.layers[3].conv2.weight, sd["features.denseblock2.denselayer4.conv2.weight"])
    np.testing.assert_array_equal(blk.layers[3].norm2.state_index.value[1], sd["features.denseblock2.denselayer4.norm2.running_var"])


def test_supported_for_every_shape(built_lib):
    from eqxvision_amd import _lib
    BF, F32 = _lib.BF16, _lib.F32
    for variant, (g, cfg, c0) in R.VARIANTS.items():
        layers, trans, _ = R.layer_shapes(variant)
        assert [h for _, _, h in trans] == [56, 28, 14] and layers[-1][2] == 7
        ends = {}
        for b, c, h in layers:
            ends[b] = c + g
        for b, c, h in layers:
            assert built_lib.mv_preact_conv1x1_supported(c, 4 * g, ends[b], 4 * g, 0, 1, BF, BF) == 1, (variant, b, c)
            assert built_lib.mv_conv3x3_slice_supported(4 * g, g, h, h, BF, BF) == 1, (variant, b)
        for b, c, h in trans:
            assert c == ends[b]
            assert built_lib.mv_preact_conv1x1_supported(c, c // 2, c, ends[b + 1], 0, 2, BF, BF) == 1, (variant, b, c)
    ok1 = (80, 128, 112, 128, 0, 1)
    assert built_lib.mv_preact_conv1x1_supported(*ok1, BF, BF) == 1
    for i, bad in ((0, 72), (1, 120), (2, 104), (2, 64), (3, 136), (3, 112), (4, 8), (5, 3)):      # no multiple of 16; ldx < C; ldy < N
        args = list(ok1)
        args[i] = bad
        assert built_lib.mv_preact_conv1x1_supported(*args, BF, BF) == 0, (i, bad)
    assert built_lib.mv_preact_conv1x1_supported(*ok1, F32, BF) == 0 and built_lib.mv_preact_conv1x1_supported(*ok1, BF, F32) == 0
    ok3 = (128, 32, 14, 14)
    assert built_lib.mv_conv3x3_slice_supported(*ok3, BF, BF) == 1 and built_lib.mv_conv3x3_slice_supported(192, 48, 7, 7, BF, BF) == 1
    for i, bad in ((0, 120), (1, 40), (2, 0), (3, 0)):
        args = list(ok3)
        args[i] = bad
        assert built_lib.mv_conv3x3_slice_supported(*args, BF, BF) == 0, (i, bad)
    assert built_lib.mv_conv3x3_slice_supported(*ok3, BF, F32) == 0
    assert built_lib.mv_conv3x3_slice_supported(192, 48, 7, 1000, BF, BF) == 0                  # the halo rows would not fit LDS
    for flag in ("no_dense_fused", "force_generic"):
        _lib.set_flag(flag, 1)
        try:
            assert built_lib.mv_preact_conv1x1_supported(*ok1, BF, BF) == 0 and built_lib.mv_conv3x3_slice_supported(*ok3, BF, BF) == 0
        finally:
            _lib.set_flag(flag, 0)


def test_argument_errors_do_not_need_a_gpu(built_lib):
    f = lambda *a: built_lib.mv_preact_conv1x1_fwd(*a)
    err = built_lib.mv_last_error
    #     x  ldx s1 h1 w  s2 h2 y  ldy cy B  H  W  C   N   pool
    ok = [1, 112, 2, 3, 4, 5, 6, 7, 128, 0, 1, 4, 4, 80, 128, 1, 1, 1, None]
    for i in (0, 2, 3, 4, 7):
        bad = list(ok); bad[i] = None
        assert f(*bad) == -1 and b"NULL" in err(), i
    bad = list(ok); bad[6] = None
    assert f(*bad) == -1 and b"go together" in err()
    bad = list(ok); bad[7] = 1
    assert f(*bad) == -1 and b"in place" in err()
    bad = list(ok); bad[13] = 72
    assert f(*bad) not in (0, -1) and b"unsupported C=72" in err()
    bad = list(ok); bad[9] = 16
    assert f(*bad) == -1 and b"output slice [16, +128) of rows of 128" in err()
    bad = list(ok); bad[15] = 2; bad[11] = 1
    assert f(*bad) == -1 and b"H=1 W=4 with pool=2" in err()
    bad = list(ok); bad[15] = 2; bad[12] = 1
    assert f(*bad) == -1 and b"with pool=2" in err()
    bad = list(ok); bad[15] = 3
    assert f(*bad) == -1 and b"pool=3" in err()
    q = lambda *a: built_lib.mv_conv3x3_slice_fwd(*a)
    #     t  ldt  S   wf y  ldy cy  N  B  H  W
    ok = [1, 128, 128, 2, 3, 96, 48, 32, 1, 5, 5, 1, 1, None]
    for i in (0, 3, 4):
        bad = list(ok); bad[i] = None
        assert q(*bad) == -1 and b"NULL" in err(), i
    bad = list(ok); bad[4] = 1
    assert q(*bad) == -1 and b"in place" in err()
    bad = list(ok); bad[2] = 120
    assert q(*bad) not in (0, -1) and b"unsupported S=120" in err()
    bad = list(ok); bad[6] = 40
    assert q(*bad) == -1 and b"multiples of 16" in err()
    bad = list(ok); bad[1] = 112
    assert q(*bad) == -1 and b"128 channels of rows of 112" in err()
    bad = list(ok); bad[6] = 80
    assert q(*bad) == -1 and b"output slice" in err()
    a = lambda *v: built_lib.mv_avgpool2d_nhwc_fwd(*v)
    assert a(None, 1, 1, 4, 4, 8, 2, 2, 2, 2, 1, None) == -1 and b"NULL" in err()
    assert a(1, 2, 1, 1, 4, 8, 2, 2, 2, 2, 1, None) == -1 and b"empty output" in err()


def _block_and_transition():
    D = _mod()
    blk = D._DenseBlock(3, 48, bn_size=2, growth_rate=16, drop_rate=0.0, key=eqv.random.PRNGKey(1))
    tr = D._Transition(96, 48, key=eqv.random.PRNGKey(2))
    return tuple(eqv.tree_inference(utils.randomize_batchnorm(m), True) for m in (blk, tr))


def test_launch_list_of_a_block_and_a_transition(monkeypatch, built_lib):
    """Fused: the placing copy, 2 launches per layer in ONE buffer (source rows of 96, slices [48, 64), [64, 80), [80, 96)), then one
    launch for the transition, written into a 112-wide buffer.  Under the switch: the composition."""
    import torch
    from eqxvision_amd import _lib
    from eqxvision_amd._act import Act
    calls = cpu_ops(monkeypatch)
    blk, tr = _block_and_transition()
    x = Act(torch.zeros(2, 5, 7, 48, dtype=torch.bfloat16), "map", True)
    with eqv.precision("bf16"):
        y = ops.dense_block(x, blk)
        z = ops.dense_transition(y, tr, next_ld=112)
    names = [c[0] for c in calls]
    assert names == ["mv_copy_rows"] + list(NEW) * 3 + [NEW[0]], names
    assert tuple(y.t.shape) == (2, 5, 7, 96) and tuple(z.t.shape) == (2, 2, 3, 112)
    pre = [c[1] for c in calls if c[0] == NEW[0]]
    assert [(a[1], a[8], a[9], a[13], a[14], a[15]) for a in pre] == [(96, 32, 0, 48, 32, 1), (96, 32, 0, 64, 32, 1), (96, 32, 0, 80, 32, 1),
                                                                       (96, 112, 0, 96, 48, 2)]
    assert all(a[0] == y.t.data_ptr() for a in pre) and pre[3][5] is None and pre[3][6] is None and pre[0][5] is not None
    assert len({a[7] for a in pre[:3]}) == 1                           # the scratch map is reused by every layer
    sl = [c[1] for c in calls if c[0] == NEW[1]]
    assert [(a[1], a[2], a[5], a[6], a[7]) for a in sl] == [(32, 32, 96, 48, 16), (32, 32, 96, 64, 16), (32, 32, 96, 80, 16)]
    assert all(a[4] == y.t.data_ptr() and a[0] == pre[0][7] for a in sl)
    # the block that follows takes the transition's buffer as it is: nothing is placed
    D = _mod()
    nxt = eqv.tree_inference(utils.randomize_batchnorm(D._DenseBlock(4, 48, 2, 16, 0.0, key=eqv.random.PRNGKey(3))), True)
    del calls[:]
    with eqv.precision("bf16"):
        assert ops.dense_block_plan(nxt, 48, 2, 3) == (32, 16, 112)
        w = ops.dense_block(z, nxt, filled=48)
    assert [c[0] for c in calls] == list(NEW) * 4 and w.t.data_ptr() == z.t.data_ptr()
    # the composition: per layer (a concatenation of i + 1 maps from the second layer on,) BatchNorm + ReLU, two convolutions; the
    # final concatenation; the transition's BatchNorm + ReLU, convolution and average pool
    del calls[:]
    _lib.load().mv_set_flag(b"no_dense_fused", 1)
    try:
        with eqv.precision("bf16"):
            y = ops.dense_block(x, blk)
            z = ops.dense_transition(y, tr, next_ld=112)
    finally:
        _lib.load().mv_set_flag(b"no_dense_fused", 0)
    names = [c[0] for c in calls]
    assert not any(n in names for n in NEW)
    assert names.count("mv_copy_rows") == 2 + 3 + 4 and names.count("mv_channel_affine_fwd") == 4
    assert names.count("mv_conv2d_nhwc_fwd") == 7 and names[-1] == "mv_avgpool2d_nhwc_fwd"
    assert tuple(y.t.shape) == (2, 5, 7, 96) and tuple(z.t.shape) == (2, 2, 3, 48)
    for mode in ("fp32",):                                             # fp32 mode is the composition as well
        del calls[:]
        with eqv.precision(mode):
            ops.dense_block(Act(torch.zeros(2, 5, 7, 48), "map", True), blk)
        assert not any(c[0] in NEW for c in calls)


def test_launch_list_of_the_network(monkeypatch, built_lib):
    sd_fn = lambda: R.densenet_state("densenet121", head_scale_=1.0)
    names = _launch_list(monkeypatch, eqv.models.densenet121, sd_fn, 2)
    assert names.count(NEW[0]) == 58 + 3 and names.count(NEW[1]) == 58 and names.count("mv_copy_rows") == 1
    assert names[:4] == ["mv_stem_conv_pool_fwd", "mv_copy_rows", NEW[0], NEW[1]]
    assert names[-3:] == ["mv_channel_affine_fwd", "mv_adaptive_avgpool2d_nhwc_fwd", "mv_linear_fwd"]
    assert len(names) == 1 + 1 + 2 * 58 + 3 + 3
    off = _launch_list(monkeypatch, eqv.models.densenet121, sd_fn, 2, flags=("no_dense_fused",))
    assert not any(n in off for n in NEW)
    assert off.count("mv_conv2d_nhwc_fwd") == 2 * 58 + 3 and off.count("mv_avgpool2d_nhwc_fwd") == 3
    assert off.count("mv_channel_affine_fwd") == 58 + 3 + 1
    assert off.count("mv_copy_rows") == sum(sum(range(2, n + 1)) + n + 1 for n in (6, 12, 24, 16))


def test_dropout_key_schedule(monkeypatch):
    """drop_rate = 0.2 in training mode: the composition runs, and the Dropout of layer l of the block at position p of `features` is
    handed element l of the split of element p of the split of the sample's key over the len(features) layers."""
    import torch
    D = _mod()
    calls = cpu_ops(monkeypatch)
    seen = []

    def fake_dropout(x, p, key, per_row=False):
        seen.append((p, np.asarray(key, np.uint32).copy()))
        return x
    monkeypatch.setattr(ops, "dropout", fake_dropout)
    monkeypatch.setattr(ops, "bn_train_update", lambda bn, y: (torch.ones(bn.input_size), torch.zeros(bn.input_size)))
    m = D.DenseNet(growth_rate=16, block_config=(2, 3), num_init_features=32, bn_size=2, drop_rate=0.2, num_classes=8)
    keys = eqv.random.split(eqv.random.PRNGKey(11), 2)
    with eqv.precision("bf16"):
        out = eqv.vmap(m, axis_name="batch")(torch.zeros(2, 3, 64, 64), key=keys)
    assert tuple(out.shape) == (2, 8)
    assert [p for p, _ in seen] == [0.2] * 5
    n_feat = len(m.features.layers)
    assert n_feat == 4 + 3 + 3
    want = [(4, 2, 0), (4, 2, 1), (6, 3, 0), (6, 3, 1), (6, 3, 2)]
    for (pos, n, l), (_, got) in zip(want, seen):
        for b in range(2):
            np.testing.assert_array_equal(got[b], R.dropout_keys(keys[b], n_feat, pos, n, l))
            np.testing.assert_array_equal(got[b], O.jax_split(O.jax_split(np.asarray(keys[b], np.uint32), n_feat)[pos], n)[l])
    names = [c[0] for c in calls]
    assert "mv_copy_rows" in names and not any(n in names for n in NEW)                # live Dropout is the literal composition


def test_avgpool2d_output_sizes(monkeypatch):
    import torch
    from eqxvision_amd._act import Act
    p = nn.AvgPool2d(kernel_size=2, stride=2)
    assert type(p).__fields__ == ("kernel_size", "stride") and (p.kernel_size, p.stride) == ((2, 2), (2, 2))
    assert p.output_size(5, 7) == (2, 3) and p.output_size(14, 14) == (7, 7) and p.output_size(15, 2) == (7, 1)
    assert nn.AvgPool2d(3, 2).output_size(7, 8) == (3, 3) and nn.AvgPool2d((2, 3), 1).output_size(5, 5) == (4, 3)
    with pytest.raises(NotImplementedError):
        nn.AvgPool2d(2, 2, padding=1)
    calls = cpu_ops(monkeypatch)
    y = p(Act(torch.zeros(2, 5, 7, 24, dtype=torch.bfloat16), "map", True))
    assert tuple(y.t.shape) == (2, 2, 3, 24) and calls[-1][0] == "mv_avgpool2d_nhwc_fwd" and calls[-1][1][2:10] == (2, 5, 7, 24, 2, 2, 2, 2)
    with pytest.raises(ValueError):
        p(Act(torch.zeros(1, 1, 4, 8), "map", True))


def test_grad_refuses(monkeypatch):
    """Inside filter_value_and_grad (grad.active()) the model, a block, a layer and a transition refuse before any launch."""
    import torch
    from eqxvision_amd import _lib, grad as _grad
    from eqxvision_amd._act import Act
    monkeypatch.setattr(_grad, "active", lambda: True)
    monkeypatch.setattr(_lib, "call", lambda name, *a: pytest.fail(f"{name} was launched"))
    m = eqv.models.densenet121(num_classes=3)
    L = m.features.layers
    key = eqv.random.split(eqv.random.PRNGKey(0), 1)
    with pytest.raises(NotImplementedError, match="without a backward"):
        m(Act(torch.zeros(1, 3, 32, 32), "img", True), key=key)
    for mod, c in ((L[4], 64), (L[4].layers[0], 64), (L[5], 256)):
        with pytest.raises(NotImplementedError, match="without a backward"):
            mod(Act(torch.zeros(1, 4, 4, c, dtype=torch.bfloat16), "map", True), key=key)
