"""CPU (`-m "not gpu"`): the Swin V2 surface and the reference's quirks (models/classification/swin.py:68-87, :369-522, :581-635,
:874-946) -- exports, field order, the coordinate table, the index, the zeroed key bias, errors, the host-side continuous position
bias against the restatement of tests/_swin_v2_ref.py (and against the transposed reading it must NOT equal), what the cosine
normalisation over axis 0 does at one and at four windows, and a torchvision-ordered checkpoint through `torch_weights=`."""
import math
import os
import tempfile
import warnings

import numpy as np
import pytest
import torch

import eqxvision_amd as eqv
from eqxvision_amd import ops
from eqxvision_amd import random as jr
from eqxvision_amd.models.classification import swin as S
from oracle import state as OS
from tests import _swin_v2_ref as R


def _reduced(**kw):
    return S.SwinTransformer([4, 4], 32, [2, 2], [1, 2], [8, 8], num_classes=5, block=S._SwinTransformerBlockV2,
                             downsample_layer=S._PatchMergingV2, key=jr.PRNGKey(1), **kw)


def test_exports_and_field_order():
    for name in ("swin_v2_t", "swin_v2_s", "swin_v2_b"):
        assert callable(getattr(eqv.models, name))
    assert S._ShiftedWindowAttentionV2.__fields__ == ("window_size", "shift_size", "num_heads", "attention_dropout", "dropout", "logit_scale",
                                                      "relative_position_bias_table", "relative_position_index", "qkv", "proj", "cpb_mlp")
    assert S._SwinTransformerBlockV2.__fields__ == ("norm1", "attn", "stochastic_depth", "norm2", "mlp")
    assert S._PatchMergingV2.__fields__ == ("reduction", "norm")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = eqv.models.swin_v2_t()
    stages = m.features.layers[1::2]
    assert [len(s.layers) for s in stages] == [2, 2, 6, 2]
    assert [s.layers[0].attn.num_heads for s in stages] == [3, 6, 12, 24]
    assert all(type(b) is S._SwinTransformerBlockV2 and b.attn.window_size == [8, 8] for s in stages for b in s.layers)
    assert [b.attn.shift_size for b in stages[2].layers[:2]] == [[0, 0], [4, 4]]
    assert all(type(d) is S._PatchMergingV2 for d in m.features.layers[2::2])
    assert m.features.layers[2].norm.shape == (192,)                        # norm_layer(2 * dim), after the reduction
    assert abs(stages[3].layers[1].stochastic_depth.p - 0.2) < 1e-12 and stages[0].layers[0].stochastic_depth.mode == "local"


@pytest.mark.parametrize("window", [(8, 8), (4, 8)])
def test_table_index_and_logit_scale(window):
    a = S._ShiftedWindowAttentionV2(64, list(window), [0, 0], 2, key=jr.PRNGKey(0))
    wh, ww = window
    assert a.logit_scale.shape == (2, 1, 1) and np.allclose(a.logit_scale, math.log(10.0))
    assert a.relative_position_bias_table.shape == (2 * wh - 1, 2 * ww - 1, 2)
    assert np.abs(a.relative_position_bias_table - R.coords_table(window)).max() < 1e-6
    idx = np.asarray(a.relative_position_index)
    assert idx.shape == ((wh * ww) ** 2,) and np.array_equal(idx, R.rel_index(window))
    assert idx.min() == -(wh + ww - 2) and idx.max() == wh + ww - 2
    if window == (8, 8):
        assert (idx.min(), idx.max()) == (-14, 14)
    b = np.asarray(a.qkv.bias)
    assert not b[64:128].any() and b[:64].any() and b[128:].any()           # the key third starts at zero (:427-433)
    l1, l2 = ops._cpb_linears(a)
    assert l1.weight.shape == (512, 2) and l1.bias.shape == (512,) and l2.weight.shape == (2, 512) and l2.bias is None


def test_errors():
    with pytest.raises(ValueError, match="length 2"):
        S._ShiftedWindowAttentionV2(32, [8], [0, 0], 1, key=jr.PRNGKey(0))
    with pytest.raises(ValueError, match="length 2"):
        S._ShiftedWindowAttentionV2(32, [8, 8], [0], 1, key=jr.PRNGKey(0))


@pytest.mark.parametrize("heads", [3, 4])
@pytest.mark.parametrize("window", [(8, 8), (4, 8)])
def test_host_bias_is_the_raw_reshape(window, heads):
    rng = np.random.Generator(np.random.PCG64(heads * 10 + window[0]))
    w1 = rng.standard_normal((512, 2)).astype(np.float32)
    b1 = rng.standard_normal(512).astype(np.float32)
    w2 = (rng.standard_normal((heads, 512)) / 16).astype(np.float32)
    table, index = R.coords_table(window).astype(np.float32), R.rel_index(window)
    got = ops.swin_v2_rel_bias_host(table, index, w1, b1, w2, heads, window)
    n = window[0] * window[1]
    assert got.shape == (heads, n, n) and got.dtype == np.float32
    ref = R.rel_bias(table, index, w1, b1, w2, heads, window)
    assert np.abs(got - ref).max() / np.abs(ref).max() <= 1e-6
    other = R.rel_bias_transposed(table, index, w1, b1, w2, heads, window)
    assert np.abs(got - other).max() > 0.1                                   # NOT the torchvision-style (positions, heads) reading


def test_cosine_normalisation_axis():
    """Pins the RESTATEMENT (tests/_swin_v2_ref.py), not the engine: the reference the GPU tests compare against normalises over
    axis 0.  It touches no package code, so it is the one test of this file that does not depend on the feature."""
    g = torch.Generator().manual_seed(0)
    ls = torch.tensor([math.log(3.0), math.log(100.0) + 1.0], dtype=torch.float64).reshape(2, 1, 1)
    mul = torch.exp(torch.clamp(ls, max=math.log(100.0)))
    q, k = torch.randn(1, 2, 16, 8, generator=g).double(), torch.randn(1, 2, 16, 8, generator=g).double()
    one = R.cos_logits(q, k, ls)                                            # nW = 1: q / |q| = sign(q), exactly
    assert torch.equal(one, torch.sign(q) @ torch.sign(k).transpose(-2, -1) * mul)
    q, k = torch.randn(4, 2, 16, 8, generator=g).double(), torch.randn(4, 2, 16, 8, generator=g).double()
    feat = (q / q.norm(dim=-1, keepdim=True)) @ (k / k.norm(dim=-1, keepdim=True)).transpose(-2, -1) * mul
    assert float((R.cos_logits(q, k, ls) - feat).abs().max()) > 0.5          # axis 0 (the windows), not the feature axis
    assert float((q / torch.linalg.norm(q, ord=2, dim=0)).abs().max()) <= 1.0


def test_shadow_qkv_zeroes_the_key_bias_only_in_the_operand():
    a = S._ShiftedWindowAttentionV2(32, [8, 8], [0, 0], 1, key=jr.PRNGKey(0))
    b = np.arange(96, dtype=np.float32) + 1
    a2 = eqv.tree_at(lambda m: m.qkv.bias, a, b)                             # a checkpoint may carry a non-zero key bias
    sh = ops.swin_v2_qkv(a2)
    assert np.array_equal(np.asarray(a2.qkv.bias), b)                        # the leaf is untouched
    assert not np.asarray(sh.bias)[32:64].any() and np.array_equal(np.asarray(sh.bias)[:32], b[:32]) and sh.weight is a2.qkv.weight
    assert ops.swin_v2_qkv(a2) is sh                                         # cached


def test_checkpoint_loads_every_leaf_in_torchvision_order():
    m = _reduced()
    leaves = [l for l in eqv.tree_leaves(m) if eqv.is_array(l)]
    rng = np.random.Generator(np.random.PCG64(7))
    sd, vals = {}, []
    for i, l in enumerate(leaves):
        v = rng.integers(-3, 4, l.shape).astype(np.int64) if np.issubdtype(l.dtype, np.integer) else rng.standard_normal(l.shape).astype(np.float32)
        if l.ndim == 3 and l.shape[-1] == 2:                                # torchvision stores the table as (1, 2Wh-1, 2Ww-1, 2)
            sd[f"t{i:04d}"] = torch.from_numpy(v[None].copy())
        else:
            sd[f"t{i:04d}"] = torch.from_numpy(v.copy())
        vals.append(v)
    with tempfile.TemporaryDirectory() as td:
        p = os.path.join(td, "w.pth")
        OS.save_pth(sd, p)
        m2 = eqv.utils.load_torch_weights(m, torch_weights=p)
    got = [l for l in eqv.tree_leaves(m2) if eqv.is_array(l)]
    assert len(got) == len(vals)
    names = {"logit_scale": 0, "index": 0, "table": 0}
    for g, v in zip(got, vals):
        assert g.shape == v.shape and np.array_equal(np.asarray(g), v.astype(g.dtype))
        names["logit_scale"] += g.ndim == 3 and g.shape[1:] == (1, 1) and g.shape[0] <= 2        # (heads, 1, 1); the conv bias is (32, 1, 1)
        names["index"] += bool(np.issubdtype(g.dtype, np.integer))
        names["table"] += g.ndim == 3 and g.shape[-1] == 2
    assert names == {"logit_scale": 4, "index": 4, "table": 4}               # the buffers and logit_scale of all four blocks


def test_map_not_a_multiple_of_the_window_and_no_backward():
    from eqxvision_amd._act import Act
    a = S._ShiftedWindowAttentionV2(32, [8, 8], [0, 0], 1, key=jr.PRNGKey(0))
    x = Act(torch.zeros(1, 12, 16, 32), "map", True)                        # raises before anything touches a device
    with pytest.raises(ValueError, match="not a multiple of the window"):
        a._forward(x)


def test_grad_refuses(monkeypatch):
    """Inside filter_value_and_grad (grad.active()) the model, a block, the attention and the patch merging refuse before any
    launch, like the other families without a backward."""
    from eqxvision_amd import _lib, grad as _grad
    from eqxvision_amd._act import Act
    monkeypatch.setattr(_grad, "active", lambda: True)
    monkeypatch.setattr(_lib, "call", lambda name, *a: pytest.fail(f"{name} was launched"))
    m = _reduced()
    key = jr.split(jr.PRNGKey(0), 1)
    with pytest.raises(NotImplementedError, match="without a backward"):
        m(Act(torch.zeros(1, 3, 64, 64), "img", True), key=key)
    blk = m.features.layers[1].layers[0]
    for mod, c in ((blk, 32), (blk.attn, 32), (m.features.layers[2], 32)):
        with pytest.raises(NotImplementedError, match="without a backward"):
            mod(Act(torch.zeros(1, 16, 16, c), "map", True), key=key)
