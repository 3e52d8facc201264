"""CPU: the operand-and-launch digest.  For one forward per model family that eqxvision_amd/ops.py serves, every launch's entry name
and scalar arguments and a SHA-256 (bytes, dtype, shape) of the tensor behind every pointer argument are compared with a golden
recorded BEFORE ops.py's prepared-operand cache and fold arithmetic were put into one helper each (tests/data/operand_digest.json):
no prepared operand may differ by a bit, no launch may move.  Host-side bytes: no tolerance.  The same run pins the cache itself:
a second forward builds nothing, and every tag that ops.py prepares operands under is reached by some case."""
import hashlib
import json
import os
import re
import tempfile
import warnings

import numpy as np
import torch

import eqxvision_amd as eqv
from eqxvision_amd import _lib, ops
from oracle import state as S
from tests._cpu_ops import cpu_ops
from tests import _convnext_ref, _densenet_ref, _googlenet_ref, _shufflenet_ref, _squeezenet_ref

GOLDEN = os.path.join(os.path.dirname(__file__), "data", "operand_digest.json")

# Tags no case reaches, each with its reason (at most five): none.
UNREACHED = {}


def _loaded(factory, sd_fn, **kw):
    with tempfile.TemporaryDirectory() as td:
        p = os.path.join(td, "w.pth")
        S.save_pth(sd_fn(), p)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return eqv.tree_inference(factory(torch_weights=p, **kw), True)


def _vit(torch_weights=None):
    return eqv.utils.load_torch_weights(
        eqv.models.VisionTransformer(img_size=224, patch_size=16, embed_dim=768, depth=3, num_heads=12, num_classes=10), torch_weights)


def _fcn(torch_weights=None):
    from eqxvision_amd.models.classification import resnet as R
    bb = R._resnet(R._ResNetBottleneck, [1, 1, 1, 1], None, replace_stride_with_dilation=[False, True, True])
    return eqv.models.fcn(num_classes=21, backbone=bb, intermediate_layers=lambda m: [m.layer3, m.layer4], aux_in_channels=1024,
                          torch_weights=torch_weights)


def _swin_v2(torch_weights=None):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return eqv.models.swin_v2_t(key=eqv.random.PRNGKey(3))       # no state builder: the constructor's own (keyed) initialisation


def _swin_b_like(torch_weights=None):
    # widths outside swin_t's (ops.swin_precise): the split-precision Linears
    return eqv.utils.load_torch_weights(eqv.models.SwinTransformer(patch_size=[4, 4], embed_dim=64, depths=[2, 2], num_heads=[2, 4],
                                                                   window_size=[7, 7], num_classes=10), torch_weights)


# name -> (factory, state builder or None, batch, image size, precisions[, library switches])
CASES = {
    "resnet50_b4": (eqv.models.resnet50, lambda: S.resnet_state(1), 4, 224, ("bf16", "fp32")),
    "resnet50_b2": (eqv.models.resnet50, lambda: S.resnet_state(1), 2, 224, ("bf16",)),
    "resnet50_b32": (eqv.models.resnet50, lambda: S.resnet_state(1), 32, 224, ("bf16",)),
    "fcn": (_fcn, lambda: S.segmentation_state(1, "fcn", (1, 1, 1, 1), 21, True), 2, 64, ("bf16",)),
    "regnet_y_400mf": (eqv.models.regnet_y_400mf, lambda: S.regnet_state(1), 2, 224, ("bf16",)),
    "mobilenet_v3_small": (eqv.models.mobilenet_v3_small, lambda: S.mobilenet_v3_state(1, *S.mobilenet_v3_conf("small")), 2, 224, ("bf16",)),
    "efficientnet_b0": (eqv.models.efficientnet_b0, lambda: S.efficientnet_state(1), 2, 224, ("bf16",)),
    "alexnet": (eqv.models.alexnet, lambda: S.alexnet_state(1), 2, 224, ("bf16",)),
    "vit_b64": (_vit, lambda: S.vit_state(1, 224, 16, 768, 3, 12, 4, 10), 64, 224, ("bf16",)),
    "vit_b2": (_vit, lambda: S.vit_state(1, 224, 16, 768, 3, 12, 4, 10), 2, 224, ("bf16", "fp32")),
    "swin_t": (eqv.models.swin_t, lambda: S.swin_state(1), 2, 224, ("bf16", "fp32")),
    # without the block kernels, and 4 x 3136 rows in stage 0: the LayerNorm + Linear launch (ops.ln_linear)
    "swin_t_ln_linear": (eqv.models.swin_t, lambda: S.swin_state(1), 4, 224, ("bf16",), ("no_swin_block_attn", "no_ln_mlp")),
    "swin_w64": (_swin_b_like, lambda: S.swin_state(1, (4, 4), 64, (2, 2), (2, 4), (7, 7), 4.0, 10), 2, 56, ("bf16",)),
    "swin_v2_t": (_swin_v2, None, 2, 256, ("bf16", "fp32")),
    "convnext_tiny": (eqv.models.convnext_tiny, lambda: _convnext_ref.convnext_state(_convnext_ref.SETTINGS["convnext_tiny"]), 4, 224,
                      ("bf16",)),
    "shufflenet_v2_x0_5": (eqv.models.shufflenet_v2_x0_5,
                           lambda: _shufflenet_ref.shufflenet_state(_shufflenet_ref.SETTINGS["shufflenet_v2_x0_5"]), 1, 224, ("bf16", "fp32")),
    "squeezenet1_1": (eqv.models.squeezenet1_1, lambda: _squeezenet_ref.squeezenet_state("1_1"), 4, 224, ("bf16",)),
    "googlenet": (eqv.models.googlenet, _googlenet_ref.googlenet_state, 2, 224, ("bf16",)),
    "densenet121": (eqv.models.densenet121, lambda: _densenet_ref.densenet_state("densenet121", head_scale_=1.0), 2, 224, ("bf16",)),
}


class _Hasher:
    """SHA-256 of (dtype, shape, bytes) per tensor.  The buffers of the fake `empty` are big and all zero bytes: those are not fed
    through the hash (their digest says so); everything else is, once per (object, version)."""

    def __init__(self):
        self.memo = {}

    def tensor(self, t):
        key = (id(t), t._version)
        hit = self.memo.get(key)
        if hit is not None:
            return hit[0]
        h = hashlib.sha256(f"{t.dtype}{tuple(t.shape)}".encode())
        raw = t.detach().contiguous().reshape(-1).view(torch.uint8)
        if not bool(raw.any()):
            h.update(b"zero bytes")
            return h.hexdigest()
        h.update(raw.numpy().tobytes())
        self.memo[key] = (h.hexdigest(), t)          # t: keeps the id alive
        return self.memo[key][0]

    def arg(self, a):
        if isinstance(a, torch.Tensor):
            return self.tensor(a)
        if isinstance(a, int) and not isinstance(a, bool) and a >= 1 << 40:
            return "ptr"                             # a raw data_ptr() (an offset into a buffer): no tensor to trace it back to
        return a if a is None or isinstance(a, (int, str)) else repr(a)

    def launches(self, calls):
        out = []
        for name, args in calls:
            h = hashlib.sha256(json.dumps([self.arg(a) for a in args]).encode()).hexdigest()[:16]
            out.append(f"{name}:{h}")
        return out


def _forward(net, B, size, dt):
    with eqv.precision(dt):
        eqv.vmap(net, axis_name="batch")(torch.zeros(B, 3, size, size), key=eqv.random.split(eqv.random.PRNGKey(0), B))


def _version_rule_net():
    return _loaded(eqv.models.resnet18, lambda: S.resnet_state(1, "basic", (2, 2, 2, 2), 10), num_classes=10)


def _bump_batchnorms(net):
    """What a training-mode step does to the shared state: new statistics, a new version."""
    from eqxvision_amd import nn
    from eqxvision_amd._module import Module

    def rec(n):
        if isinstance(n, nn.BatchNorm):
            mean, var = n.state_index.value
            n.state_index.value = (np.asarray(mean, np.float32) + np.float32(0.25), np.asarray(var, np.float32) * np.float32(2))
        elif isinstance(n, Module):
            for f in n.__fields__:
                rec(getattr(n, f, None))
        elif isinstance(n, (list, tuple)):
            for c in n:
                rec(c)
    rec(net)


def run_cases(monkeypatch):
    """-> ({case: [launch digests]}, {case: builds during the repeated forward}, tags reached)."""
    calls = cpu_ops(monkeypatch)
    monkeypatch.setattr(ops, "_fc_workspace", lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8))
    monkeypatch.setattr(ops, "_ptr", lambda t: t)               # hand the tensor itself to the recorder
    builds, tags = [0], set()
    helper = getattr(ops, "_prepared", None)
    if helper is not None:
        def counted(mod, tag, deps, build):
            tags.add(tag if isinstance(tag, str) else tag[0])

            def b():
                builds[0] += 1
                return build()
            return helper(mod, tag, deps, b)
        monkeypatch.setattr(ops, "_prepared", counted)
    digests, rebuilt = {}, {}

    def record(name, *forwards):
        H = _Hasher()
        del calls[:]
        for f in forwards:
            f()
        digests[name] = H.launches(calls)
        builds[0] = 0
        del calls[:]
        forwards[-1]()
        rebuilt[name] = builds[0]
        assert H.launches(calls) == digests[name][-len(calls):], f"{name}: the repeated forward differs"

    for name, (factory, sd_fn, B, size, dts, *flags) in CASES.items():
        net = eqv.tree_inference(factory(), True) if sd_fn is None else _loaded(factory, sd_fn)
        flags = flags[0] if flags else ()
        for f in flags:
            _lib.load().mv_set_flag(f.encode(), 1)
        try:
            for dt in dts:
                record(f"{name}/{dt}", lambda: _forward(net, B, size, dt))
        finally:
            for f in flags:
                _lib.load().mv_set_flag(f.encode(), 0)
    net = _version_rule_net()
    record("resnet18_bn_version/bf16", lambda: _forward(net, 2, 64, "bf16"), lambda: _bump_batchnorms(net), lambda: _forward(net, 2, 64, "bf16"))
    return digests, rebuilt, tags


def _tags_in_source():
    src = open(ops.__file__.replace(".pyc", ".py")).read()
    return set(re.findall(r'_prepared\(\s*[\w.\[\]]+,\s*\(?"(\w+)"', src))


def test_operand_digest(monkeypatch, built_lib):
    digests, rebuilt, tags = run_cases(monkeypatch)
    golden = json.load(open(GOLDEN))
    assert sorted(digests) == sorted(golden)
    for name in golden:
        assert len(digests[name]) == len(golden[name]), name
        diff = [(i, a, b) for i, (a, b) in enumerate(zip(digests[name], golden[name])) if a != b]
        assert not diff, f"{name}: launch {diff[0][0]} is {diff[0][1]}, recorded {diff[0][2]} ({len(diff)} launches differ)"
    assert not any(rebuilt.values()), {k: v for k, v in rebuilt.items() if v}
    assert len(UNREACHED) <= 5
    assert tags == _tags_in_source() - set(UNREACHED), (sorted(_tags_in_source() - tags), sorted(tags - _tags_in_source()))
