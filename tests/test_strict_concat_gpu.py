"""`-m gpu`: exact, rounding-visible exact and per-element checks of the concat-free conv kernels -- mv_fire_expand_fwd,
mv_conv3x3_pair_fwd, mv_conv3x3_slice_fwd, mv_conv1x1_split_fwd, mv_preact_conv1x1_fwd.  Instruments, derivations, case tables and the
defect table: tests/_strict_concat.py; the CPU proof that the instruments see each seeded defect: tests/test_strict_concat_host.py.

Every test names the kernel it must reach (`_lib.last_kernel()`), writes into sentinel-filled strided destinations with a guard
behind them (tests/_slices.py), puts NaN (preact: NaN and 2^14) into every source channel the kernel must not read, and prints its
figures (`pytest -s`): the number of wrong elements, or the worst |got - ref| / bound and the rounding bias.  Worst ratio per kernel
on an MI355X (fire 0.999, split 0.996, slice 0.989, pair 0.988, preact 0.700: the same as the CPU emulations') is recorded in
tests/_strict_concat.py's docstring."""
import numpy as np
import pytest
import torch

from eqxvision_amd import _lib
from tests import _strict_concat as C
from tests._slices import GUARD, SENTINEL, _check_slice, _dest, _read
from tests._strict_gpu import _dev, _Flags, _need_gpu, _p, _stream  # noqa: F401  (_need_gpu: the module fixture)

pytestmark = pytest.mark.gpu

BF = _lib.BF16
assert (C.SENTINEL, C.GUARD) == (SENTINEL, GUARD)
MODES = ["int", "gauss"]


def _f32(a):
    return None if a is None else _dev(np.array(a, np.float32), "fp32")


def _judge(tag, d, ys, kern, expect, mode):
    """The guard, the sentinel outside the slices, the kernel's name, then the mode's instrument (C.verdict, as on the CPU)."""
    torch.cuda.synchronize()
    bufs = []
    for i, (y, (M, ld)) in enumerate(zip(ys, d["dests"])):
        body, guard = _read(y, M, ld)
        assert guard.numel() == GUARD and bool((guard == SENTINEL).all()), f"{tag}: guard behind the destination overwritten"
        bufs.append(np.concatenate([body.numpy().reshape(-1), guard.numpy()]))
        own = [(c, ref) for j, c, ref, _ in d["slices"] if j == i]
        if len(own) == 1:                                           # one slice: tests/_slices.py's own check of sentinel, guard and NaN
            _check_slice(body, guard, own[0][0], torch.from_numpy(np.ascontiguousarray(own[0][1])), np.inf, tag)
    v = C.verdict(d, bufs, mode)
    print(f"{tag} [{kern}]: ok {v['ok']}, wrong {v['wrong']}, worst |got-ref|/bound {v['worst']:.3f}, bias {v['bias']}")
    assert kern == expect, f"{tag}: served by {kern!r}, expected {expect!r}"
    assert v["ok"], f"{tag}: {v['why']}"


# ================================================================================================ mv_conv3x3_slice_fwd
def _slice(case, mode, flag):
    d = C.slice_data(case, mode)
    H, W, B, S_, N, pad, cy, ldy = case
    tag = f"slice/{mode}/{C.case_id(case)}/{flag}"
    assert _lib.load().mv_conv3x3_slice_supported(S_, N, H, W, BF, BF) == 1, tag
    td, fd = _dev(d["t"]), _dev(d["frag"])
    y = _dest(*d["dests"][0])
    with _Flags((flag,)):
        _lib.call("mv_conv3x3_slice_fwd", _p(td), S_ + pad, S_, _p(fd), _p(y), ldy, cy, N, B, H, W, BF, BF, _stream())
        kern = _lib.last_kernel()
    _judge(tag, d, [y], kern, C.SLICE_FLAGS[flag], mode)


@pytest.mark.parametrize("flag", list(C.SLICE_FLAGS))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", C.SLICE_CASES, ids=C.case_id)
def test_slice(case, mode, flag):
    _slice(case, mode, flag)


@pytest.mark.parametrize("flag", list(C.SLICE_FLAGS))
def test_slice_round(flag):
    _slice(C.SLICE_ROUND, "round", flag)


@pytest.mark.parametrize("flag", list(C.SLICE_FLAGS))
def test_slice_at_the_gate_edge(flag):
    """S = 512 on a 2 x 13 map: the largest LDS the gate admits (163280 of 163840 bytes with the 128-pixel tile).  Bound only."""
    _slice(C.SLICE_EDGE, "gauss", flag)


def test_slice_past_the_gate_is_refused():
    """W = 14 at S = 512: _supported says 0, the entry answers MV_E_UNSUPPORTED and leaves the destination untouched."""
    H, W, B, S_, N = 2, 14, 1, 512, 16
    assert _lib.load().mv_conv3x3_slice_supported(S_, N, H, W, BF, BF) == 0
    t = _dev(np.zeros((B * H * W, S_), np.float32))
    f = _dev(np.zeros((1, 9 * S_ // 16, 64, 8), np.float32))
    y = _dest(B * H * W, 32)
    with pytest.raises(_lib.MVError, match="unsupported"):
        _lib.call("mv_conv3x3_slice_fwd", _p(t), S_, S_, _p(f), _p(y), 32, 16, N, B, H, W, BF, BF, _stream())
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all())


# ================================================================================================ mv_conv3x3_pair_fwd
def _pair(case, mode):
    d = C.pair_data(case, mode)
    H, W, B, SS, NN, ct, ldt, cy, ldy = case
    tag = f"pair/{mode}/{C.case_id(case)}"
    assert _lib.load().mv_conv3x3_pair_supported(SS[0], SS[1], NN[0], NN[1], H, W, BF, BF) == 1, tag
    td, f0, f1 = _dev(d["t"]), _dev(d["frag"][0]), _dev(d["frag"][1])
    sc0, sh0, sc1, sh1 = _f32(d["scale"][0]), _f32(d["shift"][0]), _f32(d["scale"][1]), _f32(d["shift"][1])
    y = _dest(*d["dests"][0])
    _lib.call("mv_conv3x3_pair_fwd", _p(td), ldt, ct[0], SS[0], ct[1], SS[1], _p(f0), _p(sc0), _p(sh0), _p(f1), _p(sc1), _p(sh1), _p(y), ldy,
              cy[0], NN[0], cy[1], NN[1], B, H, W, BF, BF, _stream())
    _judge(tag, d, [y], _lib.last_kernel(), "conv3x3_pair", mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", C.PAIR_CASES, ids=C.case_id)
def test_pair(case, mode):
    _pair(case, mode)


def test_pair_round():
    _pair(C.PAIR_ROUND, "round")


# ================================================================================================ mv_fire_expand_fwd
def _fire(case, mode, flag, expect):
    d = C.fire_data(case, mode)
    H, W, B, S_, E = case[:5]
    tag = f"fire/{mode}/{C.case_id(case)}/{flag or 'default'}"
    assert _lib.load().mv_fire_expand_supported(S_, E, E, H, W, BF, BF) == 1, tag
    td, f1, f3, b1, b3 = _dev(d["t"]), _dev(d["f1"]), _dev(d["f3"]), _f32(d["b1"]), _f32(d["b3"])
    y = _dest(*d["dests"][0])
    with _Flags((flag,) if flag else ()):
        _lib.call("mv_fire_expand_fwd", _p(td), _p(f1), _p(b1), _p(f3), _p(b3), _p(y), B, H, W, S_, E, E, BF, BF, _stream())
        kern = _lib.last_kernel()
    _judge(tag, d, [y], kern, expect, mode)


@pytest.mark.parametrize("flag", list(C.FIRE_FLAGS))
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", C.FIRE_CASES, ids=C.case_id)
def test_fire(case, mode, flag):
    _fire(case, mode, flag, C.FIRE_FLAGS[flag])


@pytest.mark.parametrize("flag", list(C.FIRE_FLAGS))
def test_fire_round(flag):
    _fire(C.FIRE_ROUND, "round", flag, C.FIRE_FLAGS[flag])


def test_fire_wide_tile_falls_back_on_a_wide_map():
    """S = 64 on a 2 x 300 map with "fire_expand_m256": the 256-pixel tile would need more than 64 KB, so the entry serves the call
    with the 128-pixel tile and says so."""
    _fire(C.FIRE_FALLBACK, "int", "fire_expand_m256", "fire_expand_m128")


# ================================================================================================ mv_conv1x1_split_fwd
def _split(case, mode):
    d = C.split_data(case, mode)
    M, Cc, N, n0, c0, ld0, c1, ld1 = case
    tag = f"split/{mode}/{C.case_id(case)}"
    assert _lib.load().mv_conv1x1_split_supported(Cc, N, n0, ld0, c0, ld1, c1, BF, BF) == 1, tag
    xd, wd, sc, sh = _dev(d["x"]), _dev(d["w"]), _f32(d["scale"]), _f32(d["shift"])
    ys = [_dest(*dm) for dm in d["dests"]]
    _lib.call("mv_conv1x1_split_fwd", _p(xd), _p(wd), _p(sc), _p(sh), _p(ys[0]), ld0, c0, _p(ys[1]) if n0 < N else None, ld1, c1, M, Cc, N, n0,
              BF, BF, _stream())
    _judge(tag, d, ys, _lib.last_kernel(), "conv1x1_split2" if n0 < N else "conv1x1_split1", mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", C.SPLIT_CASES, ids=C.case_id)
def test_split(case, mode):
    _split(case, mode)


def test_split_round():
    _split(C.SPLIT_ROUND, "round")


# ================================================================================================ mv_preact_conv1x1_fwd
def _preact(case, d, mode, tag):
    H, W, B, pool, Cc, N, post, pad, cy, ldy = case
    assert _lib.load().mv_preact_conv1x1_supported(Cc, N, Cc + pad, ldy, cy, pool, BF, BF) == 1, tag
    xd, wd, s1, h1, s2, h2 = _dev(d["x"]), _dev(d["w"]), _f32(d["s1"]), _f32(d["h1"]), _f32(d["s2"]), _f32(d["h2"])
    y = _dest(*d["dests"][0])
    _lib.call("mv_preact_conv1x1_fwd", _p(xd), Cc + pad, _p(s1), _p(h1), _p(wd), _p(s2), _p(h2), _p(y), ldy, cy, B, H, W, Cc, N, pool, BF, BF,
              _stream())
    _judge(tag, d, [y], _lib.last_kernel(), C.preact_kernel(case), mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", C.PREACT_CASES, ids=C.case_id)
def test_preact(case, mode):
    _preact(case, C.preact_data(case, mode), mode, f"preact/{mode}/{C.case_id(case)}")


def test_preact_round():
    _preact(C.PREACT_ROUND, C.preact_data(C.PREACT_ROUND, "round"), "round", "preact/round")


def test_preact_mean_before_rounding():
    """Windows whose four pre-activated values each round UP in bf16 while their mean is a bf16 value: the mean is taken in fp32
    before the one rounding, so the output is exact; rounded first it would be two off everywhere (tests/_strict_concat.py)."""
    _preact(C.PREACT_MEAN, C.preact_mean_case(), "int", "preact/mean")
