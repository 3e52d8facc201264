"""`eqxvision.utils` for the hot path: the ordered torch-checkpoint loader and the URL table.

`load_torch_weights` reproduces the reference's contract (eqxvision/utils.py:120-219, SURVEY
Appendix C): iterate the torch `state_dict` in file order, skip keys containing "running" /
"num_batches", and hand the remaining tensors one-per-array-leaf to the model in pytree-flatten
order (reshaped to the leaf's shape); BatchNorm running statistics are consumed in the same file
order by the `StateIndex` leaves.
"""
from __future__ import annotations

import logging
import os
from typing import Optional

import numpy as np

from ._module import Module, StateIndex, is_array, tree_leaves, tree_map

_TEMP_DIR = "/tmp/.eqx"          # same cache dir as the reference (utils.py:17)

_PT = "https://download.pytorch.org/models/"
_DINO = "https://dl.fbaipublicfiles.com/dino/"
# key -> checkpoint file stem; keys are the reference's (including its "sim_b" typo, utils.py:79)
_STEMS = {
    "alexnet": "alexnet-owt-7be5be79",
    "convnext_tiny": "convnext_tiny-983f1562", "convnext_small": "convnext_small-0c510722",
    "convnext_base": "convnext_base-6075fbad", "convnext_large": "convnext_large-ea097f82",
    "resnet18": "resnet18-5c106cde", "resnet34": "resnet34-333f7ec4", "resnet50": "resnet50-19c8e357",
    "resnet101": "resnet101-5d3b4d8f", "resnet152": "resnet152-b121ed2d",
    "resnext50_32x4d": "resnext50_32x4d-7cdf4587", "resnext101_32x8d": "resnext101_32x8d-8ba56ff5",
    "wide_resnet50_2": "wide_resnet50_2-95faca4d", "wide_resnet101_2": "wide_resnet101_2-32ee1156",
    "vgg11": "vgg11-8a719046", "vgg13": "vgg13-19584684", "vgg16": "vgg16-397923af", "vgg19": "vgg19-dcbb9e9d",
    "vgg11_bn": "vgg11_bn-6002323d", "vgg13_bn": "vgg13_bn-abd245e5", "vgg16_bn": "vgg16_bn-6c64b313",
    "vgg19_bn": "vgg19_bn-c79401a0",
    "efficientnet_b0": "efficientnet_b0_rwightman-3dd342df", "efficientnet_b1": "efficientnet_b1_rwightman-533bc792",
    "efficientnet_b2": "efficientnet_b2_rwightman-bcdf34b7", "efficientnet_b3": "efficientnet_b3_rwightman-cf984f9c",
    "efficientnet_b4": "efficientnet_b4_rwightman-7eb33cd5", "efficientnet_b5": "efficientnet_b5_lukemelas-b6417697",
    "efficientnet_b6": "efficientnet_b6_lukemelas-c76e70fd", "efficientnet_b7": "efficientnet_b7_lukemelas-dcc49843",
    "efficientnet_v2_s": "efficientnet_v2_s-dd5fe13b", "efficientnet_v2_m": "efficientnet_v2_m-dc08266a",
    "efficientnet_v2_l": "efficientnet_v2_l-59c71312",
    "regnet_y_400mf": "regnet_y_400mf-e6988f5f", "regnet_y_800mf": "regnet_y_800mf-58fc7688", "regnet_y_1_6gf": "regnet_y_1_6gf-0d7bc02a",
    "regnet_y_3_2gf": "regnet_y_3_2gf-9180c971", "regnet_y_8gf": "regnet_y_8gf-dc2b1b54", "regnet_y_16gf": "regnet_y_16gf-3e4a00f9",
    "regnet_y_32gf": "regnet_y_32gf-8db6d4b5", "regnet_y_128gf": "regnet_y_128gf_swag-c8ce3e52",
    "regnet_x_400mf": "regnet_x_400mf-62229a5f", "regnet_x_800mf": "regnet_x_800mf-94a99ebd", "regnet_x_1_6gf": "regnet_x_1_6gf-a12f2b72",
    "regnet_x_3_2gf": "regnet_x_3_2gf-7071aa85", "regnet_x_8gf": "regnet_x_8gf-2b70d774", "regnet_x_16gf": "regnet_x_16gf-ba3796d7",
    "regnet_x_32gf": "regnet_x_32gf-6eb8fdc6",
    "mobilenet_v2": "mobilenet_v2-b0353104", "mobilenet_v3_small": "mobilenet_v3_small-047dcff4",
    "mobilenet_v3_large": "mobilenet_v3_large-8738ca79",
    "shufflenetv2_x0.5": "shufflenetv2_x0.5-f707e7126e", "shufflenetv2_x1.0": "shufflenetv2_x1-5666bf0f80",
    "squeezenet1_0": "squeezenet1_0-b66bff10", "squeezenet1_1": "squeezenet1_1-b8a52dc0",
    "googlenet": "googlenet-1378be20",
    "densenet121": "densenet121-a639ec97", "densenet169": "densenet169-b2777c0a", "densenet201": "densenet201-c1103571",
    "densenet161": "densenet161-8d451a50",
    "swin_t": "swin_t-704ceda3", "swin_s": "swin_s-5e29d889", "sim_b": "swin_b-68c6b09e",
}
SEGMENTATION_URLS = {      # reference utils.py:20-24
    "deeplabv3_resnet50": _PT + "deeplabv3_resnet50_coco-cd0a2569.pth",
    "fcn_resnet50": _PT + "fcn_resnet50_coco-1167a1af.pth",
    "lraspp_mobilenetv3_large": _PT + "lraspp_mobilenet_v3_large-d234d4ea.pth",
}
CLASSIFICATION_URLS = {k: f"{_PT}{v}.pth" for k, v in _STEMS.items()}
for _arch, _dir in (("small", "deitsmall"), ("base", "vitbase")):
    for _p in (16, 8):
        CLASSIFICATION_URLS[f"vit_{_arch}_patch{_p}_224_dino"] = (
            f"{_DINO}dino_{_dir}{_p}_pretrain/dino_{_dir}{_p}_pretrain.pth")


def _make_divisible(v: float, divisor: int, min_value: Optional[int] = None) -> int:
    """Channel rounding of the MobileNet family (reference utils.py:104-117): nearest multiple of `divisor`, never more than
    10% below `v`."""
    floor = divisor if min_value is None else min_value
    rounded = max(floor, int(v + divisor / 2) // divisor * divisor)
    return rounded + divisor if rounded < 0.9 * v else rounded


def _resolve(torch_weights: str) -> str:
    if os.path.exists(torch_weights):
        return torch_weights
    cached = os.path.join(_TEMP_DIR, os.path.basename(torch_weights))
    if os.path.exists(cached):
        logging.info(f"Downloaded file exists at {cached}. Using the cached file!")
        return cached
    import torch
    os.makedirs(_TEMP_DIR, exist_ok=True)
    torch.hub.download_url_to_file(torch_weights, cached)     # network boundary (reference :159-170)
    return cached


def _is_param_leaf(leaf) -> bool:
    # reference :192-199: every array leaf that is not a size-1 bool takes the next checkpoint tensor
    return is_array(leaf) and not (leaf.size == 1 and leaf.dtype == np.bool_)


def load_torch_weights(model: Module, torch_weights: Optional[str] = None) -> Module:
    """Return a copy of `model` whose array leaves are replaced, in order, by the tensors of a
    PyTorch checkpoint (path or URL)."""
    if torch_weights is None:
        raise ValueError("torch_weights parameter cannot be empty!")
    path = _resolve(torch_weights)
    import zipfile
    if zipfile.is_zipfile(path):           # own zip + restricted-pickle reader: no torch needed, nothing in the file is executed
        from .pth import load_state_dict   # (eqxvision_amd/pth.py); its errors are final -- no fallback to an unrestricted loader
        saved = load_state_dict(path)
    else:                                  # legacy (pre-1.6, non-zip) container: torch's own loader, tensors only
        try:
            import torch
        except ImportError as e:  # pragma: no cover
            raise RuntimeError(" Torch package not found! Legacy-format checkpoints need the torch package.") from e
        saved = torch.load(path, map_location="cpu", weights_only=True)
    params, stats = [], []
    for name, w in saved.items():
        arr = w.detach().cpu().numpy() if hasattr(w, "detach") else np.asarray(w)
        if "running_mean" in name:
            stats.append([arr.astype(np.float32), None])
        elif "running_var" in name:
            stats[-1][1] = arr.astype(np.float32)
        elif "num_batches" not in name:
            params.append((name, arr))
    it_p = iter(params)
    it_s = iter(stats)
    n_state = [0]

    def replace(leaf):
        if _is_param_leaf(leaf):
            try:
                name, arr = next(it_p)
            except StopIteration:
                raise ValueError("checkpoint has fewer tensors than the model has array leaves") from None
            if arr.size != leaf.size:
                raise ValueError(f"checkpoint tensor {name} {arr.shape} cannot fill a leaf of shape {leaf.shape}")
            dt = leaf.dtype if np.issubdtype(leaf.dtype, np.integer) else np.float32
            return np.ascontiguousarray(arr.reshape(leaf.shape).astype(dt))
        if isinstance(leaf, StateIndex):
            # leaves come in pairs per BatchNorm: first_time_index <- False, state_index <- (mean, var)
            n_state[0] += 1
            if n_state[0] % 2 == 1:
                return StateIndex(False)
            try:
                mean, var = next(it_s)
            except StopIteration:
                raise ValueError("checkpoint has fewer BatchNorm statistics than the model has BatchNorm layers") from None
            return StateIndex((mean, var))
        return leaf

    new = tree_map(replace, model)
    leftover = sum(1 for _ in it_p)
    if leftover:
        raise ValueError(f"checkpoint has {leftover} more tensors than the model has array leaves")
    return new


def state_dict(model: Module) -> "OrderedDict[str, np.ndarray]":
    """Export a torch-style ordered `state_dict` from a model tree: names are attribute paths with
    `nn.Sequential.layers[i]` / list entries flattened to their index ("layer1.0.conv1.weight"), which
    is torchvision's naming for the ported families; BatchNorm running statistics are emitted as
    `running_mean` / `running_var`.  The inverse of `load_torch_weights` (same order)."""
    from collections import OrderedDict

    from . import nn
    out = OrderedDict()

    def rec(node, prefix):
        if isinstance(node, nn.BatchNorm):
            if node.weight is not None:
                out[prefix + "weight"] = node.weight
                out[prefix + "bias"] = node.bias
            st = node.state_index.value
            if st is not None:
                out[prefix + "running_mean"], out[prefix + "running_var"] = st
            return
        if isinstance(node, Module):
            for f in node.__fields__:
                if not hasattr(node, f):
                    continue
                v = getattr(node, f)
                if isinstance(node, nn.Sequential) and f == "layers":
                    rec(v, prefix)
                else:
                    rec(v, prefix + f + ".")
            return
        if isinstance(node, (list, tuple)):
            for i, v in enumerate(node):
                rec(v, prefix + f"{i}.")
            return
        if is_array(node):                         # a device-resident leaf (DevArray) is fetched here, once
            out[prefix[:-1]] = np.asarray(node)

    rec(model, "")
    return out


def randomize_batchnorm(model: Module, seed: int = 1) -> Module:
    """Give every BatchNorm non-trivial affine parameters and running statistics
    (gamma~U[0.5,1.5], beta~N(0,0.1), mean~N(0,0.1), var~U[0.5,1.5]) so that a randomly initialised
    model can run inference (the reference's unloaded BatchNorm has no state at all) and the BN
    folding is exercised.  Used for synthetic benchmarks."""
    from . import nn
    rng = np.random.Generator(np.random.PCG64(seed))

    def rec(n):
        if isinstance(n, nn.BatchNorm):
            c = n.input_size
            new = object.__new__(type(n))
            new.__dict__.update({k: v for k, v in n.__dict__.items() if k != "_dev_cache"})
            object.__setattr__(new, "weight", rng.uniform(0.5, 1.5, c).astype(np.float32))
            object.__setattr__(new, "bias", (0.1 * rng.standard_normal(c)).astype(np.float32))
            object.__setattr__(new, "first_time_index", StateIndex(False))
            object.__setattr__(new, "state_index", StateIndex(((0.1 * rng.standard_normal(c)).astype(np.float32),
                                                                rng.uniform(0.5, 1.5, c).astype(np.float32))))
            return new
        if isinstance(n, Module):
            from ._module import _rebuild
            return _rebuild(n, rec)
        if isinstance(n, list):
            return [rec(c) for c in n]
        if isinstance(n, tuple):
            return tuple(rec(c) for c in n)
        return n

    return rec(model)
