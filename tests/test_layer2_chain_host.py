"""Host side of the accumulator-layout boundary kernels (csrc/chain_rc.hip, csrc/chain_l2.hip): operand layouts and which C-ABI entries
a forward calls.  No GPU."""
import numpy as np
import pytest

from oracle import state as S
from tests._cpu_ops import cpu_ops
from tests.test_host import _launch_list

NEW_ENTRY = "mv_conv1x1_dual_chain_res_fwd"


def _restated_fragments(w3, w1n):
    """mv_conv1x1_chain_res_fwd's fragment order written out element by element from the header's description: fragment f of chunk c
    is [lane = 32 fh + r][8]; f < C / 16: w3[32 c + r][16 f + 8 fh + e]; else f = C / 16 + T2 s + a2:
    w1n[32 a2 + r][slot 8 fh + e of k-step s], slot 8 fh + i <-> channel 32 c + 8 (2 s + i / 4) + 4 fh + i % 4."""
    K, C = w3.shape
    N2 = w1n.shape[0]
    KX, T2 = C // 16, N2 // 32
    out = np.zeros((K // 32, KX + 2 * T2, 64, 8), np.float32)
    for c in range(K // 32):
        for lane in range(64):
            r, fh = lane % 32, lane // 32
            for e in range(8):
                for f in range(KX):
                    out[c, f, lane, e] = w3[32 * c + r, 16 * f + 8 * fh + e]
                for s in range(2):
                    for a2 in range(T2):
                        ch = 32 * c + 8 * (2 * s + e // 4) + 4 * fh + e % 4
                        out[c, KX + T2 * s + a2, lane, e] = w1n[32 * a2 + r, ch]
    return out


@pytest.mark.parametrize("C,N2", [(128, 128), (128, 256), (384, 128)])
def test_l2_fragment_order(C, N2):
    from eqxvision_amd import ops
    rng = np.random.default_rng(7)
    K = 512
    w3 = rng.standard_normal((K, C)).astype(np.float32)
    w1n = rng.standard_normal((N2, K)).astype(np.float32)
    got = ops._res_fragments(w3, w1n).reshape(K // 32, C // 16 + N2 // 16, 64, 8)
    np.testing.assert_array_equal(got, _restated_fragments(w3, w1n))


def _conv_bn(rng, cin, cout, bias):
    """A pointwise Conv2d + inference BatchNorm with random parameters and statistics, and its fp32 (scaled rows, shift) restated."""
    import eqxvision_amd as eqv
    conv = eqv.nn.Conv2d(cin, cout, 1, use_bias=bias, key=eqv.random.PRNGKey(0))
    conv.weight = (rng.standard_normal((cout, cin, 1, 1)) / np.sqrt(cin)).astype(np.float32)
    if bias:
        conv.bias = (0.3 * rng.standard_normal((cout, 1, 1))).astype(np.float32)
    bn = eqv.nn.BatchNorm(cout, inference=True)
    bn.weight = rng.uniform(0.5, 1.5, cout).astype(np.float32)
    bn.weight[::7] *= -1.0
    bn.bias = (0.2 * rng.standard_normal(cout)).astype(np.float32)
    mean, var = (0.3 * rng.standard_normal(cout)).astype(np.float32), rng.uniform(0.3, 2.0, cout).astype(np.float32)
    bn.state_index.value = (mean, var)
    scale = bn.weight * (np.float32(1.0) / np.sqrt(var + np.float32(bn.eps)))
    shift = bn.bias - mean * scale
    if bias:
        shift = shift + conv.bias.reshape(-1) * scale
    return conv, bn, conv.weight.reshape(cout, cin) * scale[:, None], shift


@pytest.mark.parametrize("bias", [False, True])
def test_rc_operands_from_modules(monkeypatch, bias):
    """The operands of mv_conv1x1_chain_rc_fwd (16 fragments per chunk, 18 shift rows) and mv_conv1x1_chain_rc0_fwd (12 and 10) as
    ops.chain_acc_operands packs them from Conv2d / BatchNorm modules, against the header's layouts restated in tests/_cases.py
    (the ones the GPU cases hand to the kernels); rc0 is rc without conv3_1's fragments and shift rows, as chain_rc_case takes it."""
    import torch
    from eqxvision_amd import ops
    from tests._cases import _rc_fragments, _rc_shifts
    cpu_ops(monkeypatch)
    rng = np.random.default_rng(5)
    C, K, N2 = 64, 256, 64
    c30, b30, w30, h30 = _conv_bn(rng, C, K, bias)
    cd, bd, wd, hd = _conv_bn(rng, C, K, bias)
    c31, b31, w31, h31 = _conv_bn(rng, C, K, bias)
    c1n, b1n, w1n, h1n = _conv_bn(rng, K, N2, bias)
    bits = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).view(torch.int16).numpy()
    ref_f = _rc_fragments(np.concatenate([w30, wd], axis=1), w31, w1n).reshape(K // 32, 16, 64 * 8)
    ref_s = _rc_shifts(h30 + hd, h31, h1n)

    wf, sh = ops.chain_acc_operands(c31, [[(c30, b30), (cd, bd)], [(c31, b31)]], c1n, b1n)
    assert wf.dtype == torch.bfloat16 and sh.dtype == torch.int32 and tuple(sh.shape) == (18, 64)
    np.testing.assert_array_equal(wf.view(torch.int16).numpy().reshape(K // 32, 16, 64 * 8), bits(ref_f))
    np.testing.assert_array_equal(sh.numpy().view(np.uint32), ref_s)

    wf0, sh0 = ops.chain_acc_operands(c30, [[(c30, b30), (cd, bd)]], c1n, b1n)
    assert tuple(sh0.shape) == (10, 64)
    np.testing.assert_array_equal(wf0.view(torch.int16).numpy().reshape(K // 32, 12, 64 * 8),
                                  bits(np.concatenate([ref_f[:, :8], ref_f[:, 12:]], axis=1)))
    np.testing.assert_array_equal(sh0.numpy().view(np.uint32), np.concatenate([ref_s[:8], ref_s[16:]], axis=0))


def _r50(monkeypatch, B, flags=()):
    import eqxvision_amd as eqv
    return _launch_list(monkeypatch, eqv.models.resnet50, lambda: S.resnet_state(1), B, flags=flags)


def test_resnet50_layer2_launch_list(monkeypatch, built_lib):
    """B = 32 (25 088 pixels at 28 x 28): layer 2 opens with the dual entry (y stored), its middle boundaries and its exit (sub-sampled
    y, N2 = 256 into layer 3's conv1) are mv_conv1x1_chain_res_fwd; with no_chain_l2 it is today's list exactly."""
    on = _r50(monkeypatch, 32)
    off = _r50(monkeypatch, 32, ("no_chain_l2",))
    assert on.count(NEW_ENTRY) == 1 and NEW_ENTRY not in off
    # layer 1's exit + layer 2's two middle boundaries + its exit
    assert off.count("mv_conv1x1_chain_res_fwd") == 1 and on.count("mv_conv1x1_chain_res_fwd") == 4
    assert off.count("mv_conv1x1_dual_fwd") - on.count("mv_conv1x1_dual_fwd") == 1
    assert off.count("mv_conv2d_nhwc_fwd") - on.count("mv_conv2d_nhwc_fwd") == 3
    assert off.count("mv_conv1x1_chain_fwd") == 2 and on.count("mv_conv1x1_chain_fwd") == 0
    assert len(off) - len(on) == 2
    e = on.index(NEW_ENTRY)
    assert on[e:].count("mv_conv1x1_chain_res_fwd") == 3


def test_layer2_exit_writes_subsampled(monkeypatch, built_lib):
    """The exit's y reaches layer 3 only through its stride-2 downsample branch: chain_res is asked with sub = 2."""
    from eqxvision_amd import _lib
    seen = []
    real_lib = _lib.load()
    real = real_lib.mv_conv1x1_chain_res_supported

    def spy(N, H, W, C, K, N2, sub, dt):
        r = real(N, H, W, C, K, N2, sub, dt)
        if r:
            seen.append((C, K, N2, sub))
        return r
    monkeypatch.setattr(real_lib, "mv_conv1x1_chain_res_supported", spy, raising=False)
    _r50(monkeypatch, 32)
    assert (128, 512, 256, 2) in seen and (128, 512, 128, 0) in seen


def test_no_chain_l2_is_todays_list(monkeypatch, built_lib):
    """no_chain_l2 restores the layer-2 launches of the older dispatch (the off switches of every other path give the same list)."""
    off = _r50(monkeypatch, 32, ("no_chain_l2",))
    names = set(off)
    assert NEW_ENTRY not in names and "mv_conv1x1_chain_fwd" in names and "mv_conv1x1_dual_fwd" in names


def test_small_batch_and_other_widths_unchanged(monkeypatch, built_lib):
    """Below 16 384 pixels (B = 16 at 28 x 28 is 12 544) and for other stage widths the flag changes nothing."""
    import eqxvision_amd as eqv
    assert _r50(monkeypatch, 16) == _r50(monkeypatch, 16, ("no_chain_l2",))
    wide = lambda fl: _launch_list(monkeypatch, eqv.models.wide_resnet50_2,
                                   lambda: S.resnet_state(1, "bottleneck", (3, 4, 6, 3), 1000, width_per_group=128), 32, flags=fl)
    assert wide(()) == wide(("no_chain_l2",))
    rx = lambda fl: _launch_list(monkeypatch, eqv.models.resnext50_32x4d,
                                 lambda: S.resnet_state(1, "bottleneck", (3, 4, 6, 3), 1000, groups=32, width_per_group=4), 32, flags=fl)
    assert rx(()) == rx(("no_chain_l2",))


def test_resnet101_takes_the_path(monkeypatch, built_lib):
    import eqxvision_amd as eqv
    r101 = _launch_list(monkeypatch, eqv.models.resnet101, lambda: S.resnet_state(1, "bottleneck", (3, 4, 23, 3), 1000), 32)
    assert r101.count(NEW_ENTRY) == 1 and "mv_conv1x1_chain_fwd" not in r101
