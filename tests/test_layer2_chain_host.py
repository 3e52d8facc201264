"""Host side of the layer-2 streamed boundaries (csrc/chain_l2.hip): fragment order and which C-ABI entries a forward calls.  No GPU."""
import numpy as np
import pytest

from oracle import state as S
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
