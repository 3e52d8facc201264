"""The reference's own ShuffleNetV2 known-answer test (tests/test_models/test_shufflenetv2.py), armed as tests/test_reference_goldens.py
arms the others: `tests/golden/reference_static/shufflenet_v2_x0_5_logits.npy` is torchvision's output for the reference's `img.png`
with the pretrained shufflenetv2_x0.5 checkpoint (converted by tests/golden/make_shufflenet_static.py).  The checkpoint cannot be
downloaded here, so the comparison SKIPS unless `shufflenetv2_x0.5-f707e7126e.pth` is found in `$EQXVISION_WEIGHTS` or
`~/.eqxvision/models`; the fixture itself is tested unconditionally."""
import os

import numpy as np
import pytest

from tests.test_reference_goldens import STATIC, demo_image

CKPT = "shufflenetv2_x0.5-f707e7126e.pth"


def test_fixture():
    a = np.load(os.path.join(STATIC, "shufflenet_v2_x0_5_logits.npy"))
    assert a.shape == (1, 1000) and a.dtype == np.float32 and np.isfinite(a).all()
    r = np.load(os.path.join(STATIC, "resnet18_logits.npy"))
    top5 = set(np.argsort(-r[0])[:5].tolist())
    assert len(top5 & set(np.argsort(-a[0])[:5].tolist())) >= 2          # the same bird


@pytest.mark.gpu
def test_hip_path_vs_reference_golden():
    """The HIP path in fp32 mode against the reference's golden (atol 1e-3, as for the other families)."""
    import torch
    import eqxvision_amd as eqv
    path = None
    for d in (os.environ.get("EQXVISION_WEIGHTS"), os.path.expanduser("~/.eqxvision/models")):
        if d and os.path.exists(os.path.join(d, CKPT)):
            path = os.path.join(d, CKPT)
    if path is None:
        pytest.skip(f"{CKPT} not present (no network in this environment): reference known-answer test armed, not run")
    eqv.set_compute_dtype("fp32")
    try:
        net = eqv.tree_inference(eqv.models.shufflenet_v2_x0_5(torch_weights=path), True)
        x = torch.from_numpy(demo_image(224)).cuda()
        got = eqv.vmap(net, axis_name="batch")(x, key=eqv.random.split(eqv.random.PRNGKey(0), 1)).float().cpu().numpy()
    finally:
        eqv.set_compute_dtype("bf16")
    assert np.allclose(got, np.load(os.path.join(STATIC, "shufflenet_v2_x0_5_logits.npy")), atol=1e-3)
