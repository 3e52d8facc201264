"""`-m gpu`: the layer-2 streamed boundaries (csrc/chain_l2.hip) against fp64 references of their function, and ResNet-50 / 101 with
them on and off ("no_chain_l2").  Margins are printed (`pytest -s`)."""
import numpy as np
import pytest
import torch

from eqxvision_amd import _lib, ops
from tests import _model_cases as MC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    _lib.load()
    _lib.check_device_status()
    yield
    _lib.check_device_status()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return t.data_ptr()


def _operands(rng, K, Cin, N2):
    """fp32 scales / shifts folded into the weight rows as the host does; the kernel sees bf16 rows."""
    w3 = (rng.standard_normal((K, Cin)) / np.sqrt(Cin)).astype(np.float32) * rng.uniform(0.5, 1.5, (K, 1)).astype(np.float32)
    h3 = (0.3 * rng.standard_normal(K)).astype(np.float32)
    w1n = (rng.standard_normal((N2, K)) / np.sqrt(K / 2)).astype(np.float32) * rng.uniform(0.5, 1.5, (N2, 1)).astype(np.float32)
    hn = (0.3 * rng.standard_normal(N2)).astype(np.float32)
    wf = torch.from_numpy(ops._res_fragments(w3, w1n).reshape(-1)).to(torch.bfloat16).cuda()
    sh = torch.from_numpy(ops._rc_shift_rows(h3, hn).view(np.int32)).cuda()
    bf = lambda a: torch.from_numpy(a).to(torch.bfloat16).double()
    return wf, sh, bf(w3), torch.from_numpy(h3).double(), bf(w1n), torch.from_numpy(hn).double()


def _reference(xcat, res, w3, h3, w1n, hn):
    """fp64 of the bf16 operands; y rounded to bf16 before the next conv1, as the next layer would read it."""
    y = xcat.double() @ w3.T + h3
    if res is not None:
        y = y + res.double()
    y = torch.relu(y).to(torch.bfloat16)
    t1 = torch.relu(y.double() @ w1n.T + hn)
    return y.double(), t1


def _err(got, ref):
    return float((got.double().cpu() - ref).abs().max()) / max(float(ref.abs().max()), 1e-6)


RES_CASES = [(N, H, W, N2, sub) for (N, H, W) in ((32, 28, 28), (37, 28, 30)) for N2 in (128, 256) for sub in (0, 2)] + \
            [(1, 128, 128, 256, 2), (1, 128, 128, 128, 0)]


@pytest.mark.parametrize("N,H,W,N2,sub", RES_CASES)
def test_chain_l2_res(N, H, W, N2, sub):
    """middle (N2 = 128) and exit (N2 = 256) boundaries, y whole or sub-sampled; ragged pixel counts; M = 16 384 exactly."""
    C, K, M = 128, 512, N * H * W
    lib = _lib.load()
    assert lib.mv_conv1x1_chain_res_supported(N, H, W, C, K, N2, sub, _lib.BF16)
    rng = np.random.default_rng(N * 7 + W + N2 + sub)
    wf, sh, w3, h3, w1n, hn = _operands(rng, K, C, N2)
    t2 = torch.relu(torch.randn(M, C, device="cuda")).to(torch.bfloat16)
    res = torch.relu(torch.randn(M, K, device="cuda")).to(torch.bfloat16)
    y = torch.full(((N * (H // 2) * (W // 2)) if sub else M, K), float("nan"), device="cuda", dtype=torch.bfloat16)
    t1 = torch.empty(M, N2, device="cuda", dtype=torch.bfloat16)
    _lib.call("mv_conv1x1_chain_res_fwd", _p(t2), _p(res), _p(wf), _p(sh), _p(y), _p(t1), N, H, W, C, K, N2, sub, _lib.BF16, _stream())
    torch.cuda.synchronize()
    ry, rt = _reference(t2.cpu(), res.cpu(), w3, h3, w1n, hn)
    if sub:
        ry = ry.reshape(N, H, W, K)[:, ::2, ::2].reshape(-1, K)
    ey, et = _err(y, ry), _err(t1, rt)
    print(f"chain_l2 res N={N} H={H} W={W} N2={N2} sub={sub}: y {ey:.2e} t1 {et:.2e}")
    assert ey <= 1e-2 and et <= 1e-2


@pytest.mark.parametrize("M", [25088, 16384, 37 * 28 * 30])
def test_chain_l2_entry(M):
    C1, C2, K, N2 = 128, 256, 512, 128
    rng = np.random.default_rng(M)
    wf, sh, w3, h3, w1n, hn = _operands(rng, K, C1 + C2, N2)
    t2 = torch.relu(torch.randn(M, C1, device="cuda")).to(torch.bfloat16)
    x = torch.relu(torch.randn(M, C2, device="cuda")).to(torch.bfloat16)
    y = torch.empty(M, K, device="cuda", dtype=torch.bfloat16)
    t1 = torch.empty(M, N2, device="cuda", dtype=torch.bfloat16)
    _lib.call("mv_conv1x1_dual_chain_res_fwd", _p(t2), _p(x), _p(wf), _p(sh), _p(y), _p(t1), M, C1, C2, K, N2, _lib.BF16, _stream())
    torch.cuda.synchronize()
    ry, rt = _reference(torch.cat([t2, x], 1).cpu(), None, w3, h3, w1n, hn)
    ey, et = _err(y, ry), _err(t1, rt)
    print(f"chain_l2 entry M={M}: y {ey:.2e} t1 {et:.2e}")
    assert ey <= 1e-2 and et <= 1e-2


def test_chain_l2_aliases_refused():
    M, lib = 25088, _lib.load()
    a = torch.zeros(M, 512, device="cuda", dtype=torch.bfloat16)
    b = torch.zeros(M, 256, device="cuda", dtype=torch.bfloat16)
    w = torch.zeros(1, device="cuda")
    rc = lib.mv_conv1x1_dual_chain_res_fwd(_p(b), _p(b), _p(w), _p(w), _p(b), _p(a), M, 128, 256, 512, 128, _lib.BF16, None)
    assert rc == -1
    rc = lib.mv_conv1x1_chain_res_fwd(_p(b), _p(a), _p(w), _p(w), _p(a), _p(b), 32, 28, 28, 128, 512, 256, 0, _lib.BF16, None)
    assert rc == -1


def _plan_vs_off(factory, sd, layers, B=32):
    import eqxvision_amd as eqv
    from oracle import state as S
    from oracle import torch_ref as TR
    x = S.synthetic_images(B, 224, seed=0)
    ref = TR.resnet_forward(sd, x, layers=layers).numpy()
    rec = []
    old = _lib.set_recording(rec)
    try:
        got = MC._run(MC._load(factory, sd), x, "bf16").cpu().numpy()
    finally:
        _lib.set_recording(old)
    _lib.set_flag("no_chain_l2", 1)
    rec2 = []
    try:
        old = _lib.set_recording(rec2)
        try:
            plain = MC._run(MC._load(factory, sd), x, "bf16").cpu().numpy()
        finally:
            _lib.set_recording(old)
    finally:
        _lib.set_flag("no_chain_l2", 0)
    names, names2 = [n for _, _, n in rec], [n for _, _, n in rec2]
    info, info2 = MC._cmp(got, ref, 1e-2), MC._cmp(plain, ref, 1e-2)
    d = float(np.abs(got - plain).max())
    print(f"plan {info['err']:.2e} off {info2['err']:.2e} plan-vs-off {d:.2e}, launches {len(names)} / {len(names2)}")
    assert info["ok"] and info2["ok"] and d <= 2e-3
    assert "mv_conv1x1_dual_chain_res_fwd" in names and "mv_conv1x1_dual_chain_res_fwd" not in names2


def test_resnet50_b32_plan_vs_off():
    import eqxvision_amd as eqv
    from oracle import state as S
    _plan_vs_off(eqv.models.resnet50, S.resnet_state(1), (3, 4, 6, 3))


def test_resnet101_b32_plan_vs_off():
    import eqxvision_amd as eqv
    from oracle import state as S
    _plan_vs_off(eqv.models.resnet101, S.resnet_state(1, "bottleneck", (3, 4, 23, 3), 1000), (3, 4, 23, 3))
