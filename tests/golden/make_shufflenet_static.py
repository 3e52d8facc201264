"""Converts the reference's ShuffleNetV2 known-answer fixture (a data file of its test-suite) into a torch-free array, as
make_reference_static.py does for the other families:

    <reference>/tests/static/shufflenet_v2_x0_5.pred.pth  ->  tests/golden/reference_static/shufflenet_v2_x0_5_logits.npy

torchvision's logits for `img.png` with the pretrained shufflenetv2_x0.5 checkpoint (reference tests/test_models/test_shufflenetv2.py).
usage: python tests/golden/make_shufflenet_static.py <reference>/tests/static
"""
import os
import sys

import numpy as np
import torch

SRC = sys.argv[1]
DST = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_static")
t = torch.load(os.path.join(SRC, "shufflenet_v2_x0_5.pred.pth"), map_location="cpu")
a = (t["output"] if isinstance(t, dict) else t).detach().numpy().astype(np.float32).reshape(1, -1)
np.save(os.path.join(DST, "shufflenet_v2_x0_5_logits.npy"), a)
print("shufflenet_v2_x0_5_logits", a.shape, a.dtype, float(np.abs(a).max()))
