"""`-m gpu`: the ResNet entry kernel with its weight fragments in registers and 8 x 7 pooled tiles (csrc/stem_pool.hip) against
the kernel it replaced, which stays compiled in behind the library switch `no_stem_wreg`.  Both bodies feed the same operands to
the same MFMAs in the same k order and share the epilogue and the pooling, so the outputs are the same bits: `torch.equal`, no
tolerance.  The shapes sit on the edges of the new tiling, not at the workload's size."""
import pytest
import torch

from tests import _cases

pytestmark = pytest.mark.gpu

FLAG = "no_stem_wreg"
F32, BF = 0, 1
SENTINEL = -7.0


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from eqxvision_amd import _lib
    _lib.load()
    _lib.check_device_status()
    yield
    _lib.set_flag(FLAG, 0)
    _lib.check_device_status()


def _run(x, w, sc, sh, old):
    """One launch of the entry with the switch at `old`, into an output pre-filled with a sentinel."""
    from eqxvision_amd import _lib
    N, C, H, W = x.shape
    Ho, Wo = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    Po, Qo = (Ho + 2 - 3) // 2 + 1, (Wo + 2 - 3) // 2 + 1
    y = torch.full((N, Po, Qo, 64), SENTINEL, dtype=torch.bfloat16, device="cuda")
    _lib.set_flag(FLAG, int(old))
    try:
        _lib.call("mv_stem_conv_pool_fwd", x.data_ptr(), w.data_ptr(), sc.data_ptr(), sh.data_ptr(), y.data_ptr(),
                  N, 3, H, W, 64, 7, 7, 2, 2, 3, 3, 3, 2, 1, 1, BF if x.dtype == torch.bfloat16 else F32, BF,
                  torch.cuda.current_stream().cuda_stream)
        kern = _lib.last_kernel()
        torch.cuda.synchronize()
    finally:
        _lib.set_flag(FLAG, 0)
    return y, kern


def _operands(seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    w = (torch.randn((64, 3, 7, 7), generator=g, device="cuda") / 12).to(torch.bfloat16)
    sc = torch.rand(64, generator=g, device="cuda") + 0.5
    sc[::3] *= -1.0
    sh = torch.randn(64, generator=g, device="cuda") * 0.1
    return g, w, sc, sh


def _check(x, w, sc, sh, name):
    y_old, k_old = _run(x, w, sc, sh, True)
    y_new, k_new = _run(x, w, sc, sh, False)
    assert k_old == name and k_new == name, (k_old, k_new)
    assert not (y_new == SENTINEL).any(), "the new body left output elements unwritten"
    b_old, b_new = y_old.view(torch.int16), y_new.view(torch.int16)
    assert torch.equal(b_old, b_new), f"{int((b_old != b_new).sum())} of {b_old.numel()} elements differ"


# (N, H, W): full tiles at an exact multiple | odd sizes, partial tile row and column, no 4-pixel loads | one tile row, nine tile
# columns, the last one partial | one partial tile, fewer than 8 blocks (plain tile order) | many tiles per block: the persistent
# loop, LDS reuse from tile to tile, the per-XCD tile ranges
@pytest.mark.parametrize("N,H,W", [(2, 224, 224), (3, 75, 93), (2, 30, 228), (1, 20, 20), (40, 128, 128)])
def test_bits_f32in(N, H, W):
    g, w, sc, sh = _operands(N * 1000 + H)
    x = torch.rand((N, 3, H, W), generator=g, device="cuda") * 2 - 0.7
    _check(x, w, sc, sh, "stem_pool_mfma_f32in")


@pytest.mark.parametrize("N,H,W", [(2, 64, 64), (3, 61, 70)])
def test_bits_bf16in(N, H, W):
    g, w, sc, sh = _operands(N * 1000 + H)
    x = (torch.rand((N, 3, H, W), generator=g, device="cuda") * 2 - 0.7).to(torch.bfloat16)
    _check(x, w, sc, sh, "stem_pool_mfma_bf16in")


def test_bits_f32in_base_off_by_4_bytes():
    """W % 4 == 0, but the image starts 4 bytes into an allocation: the aligned 4-pixel loads are off, the scalar path runs."""
    g, w, sc, sh = _operands(5)
    N, H, W = 2, 64, 64
    buf = torch.rand(N * 3 * H * W + 1, generator=g, device="cuda") * 2 - 0.7
    x = buf[1:].view(N, 3, H, W)
    assert x.data_ptr() % 16 == 4 and x.is_contiguous()
    _check(x, w, sc, sh, "stem_pool_mfma_f32in")


def test_negative_gamma_against_the_oracle():
    """BN gamma < 0 on every third channel: scale / shift are applied before the max.  Against the oracle chain conv2d ->
    scale / shift -> relu -> bf16 -> maxpool2d, with the suite's bf16 tolerance (tests/_cases.py: _cmp, TOL_BF16)."""
    from eqxvision_amd import _lib
    _lib.set_flag(FLAG, 0)
    info = _cases.stem_pool_case(2, 75, 93, seed=21, neg_scale=True)()
    print(info)
    assert info["ok"] and info["kernel"] == "stem_pool_mfma_f32in", info
