"""`-m gpu`: exact and per-element parity checks of the LayerNorm family (csrc/layernorm.hip) and of the batch-moment and BatchNorm
fold kernels (csrc/moments.hip).  Case tables, float64 references, bounds with their derivations and the emulations:
tests/_strict_norm.py; CPU proof that the instruments see each defect: tests/test_strict_norm_host.py.

Every destination is filled with the sentinel and has a guard behind it (tests/_slices.py); the guard must be intact (the clamped
re-read rows of a ragged row group never store) and no sentinel may survive.  Operands are rounded to their storage type before both
sides see them; the reference is float64.  Every case names the kernel it must reach and prints kernel, worst |got - ref| / bound
ratio and rounding bias (`pytest -s`).

Exact: the moments of integers (three entries, NaN-filled workspace, two calls bitwise equal); y_lo of mv_layernorm_add_fwd against
bf16_round(y) / y; row-position invariance (three base rows in a shuffled order: equal input rows give bitwise-equal output rows at
every sub-row, in the ragged last group and in both register sets) and isolation (a NaN row stays in its row; NaN in the gaps of a
strided input is never read) for every LayerNorm kernel; the guards; constant channels through mv_bn_ema_fold1_fwd's clamp.
Bound and bias: every case of the tables on Gaussian operands.

rsqrtf: R = 2 ulp is assumed in the bound (no installed ROCm document states its accuracy; nobody has measured it).

The `else GOS(4)` branch of mv_layernorm_fwd's slim dispatch cannot be reached (its gate admits C = 256, 512, 768 only; C = 1024 is
served by layernorm_vec, which test_layernorm_fwd's C1024_not_slim case pins).  It stays in this change because the change adds
tests only and leaves the library as it was; it can go with the next edit of that entry.

Worst |got - ref| / bound per kernel name, measured on an MI355X against the float64 reference (a bf16 output sits near 1 by
construction: its bound is little more than the store's half ulp):
    layernorm             fp32 out 0.053 (C = 22)                       bf16 out 0.995   bias -0.0042
    layernorm_vec         fp32 out 0.095 (65937 x 32, grid stride)      bf16 out 0.999   bias -0.0089 at the worst case
    layernorm_slim                                                      bf16 out 0.998   bias -0.0002
    layernorm_add         fp32 out 0.071 (nch 13, fp32 z, res); y_lo bit-equal to the rounded y in every case
    patch_merge_ln_f32in  fp32 out 0.051 (182 x 182 x 16)               bf16 out 0.999   bias -0.0026
    channel_sum 0.075 (37 x 1032 fp32)   channel_sqdev, channel_moments2 0.931 (1 x 2040 bf16: one row, so the bound is the three
                          roundings of (x - shift)^2 and nothing else); exact on integers at every shape, two calls bitwise equal
    bn_mean 0.262   bn_ema_fold 0.265 (run_var, first call)   bn_ema_fold1 0.419 (run_var of the constant channels)
No case violated its bound, no row differed from an equal row elsewhere, and no kernel had to be changed.
"""
import numpy as np
import pytest
import torch

from eqxvision_amd import _lib
from tests import _strict as S
from tests import _strict_norm as N
from tests._slices import GUARD, SENTINEL, _dest, _read
from tests._strict_gpu import DT, _dev, _Flags, _need_gpu, _p, _stream  # noqa: F401  (_need_gpu: the module fixture)

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
TT = {"bf16": torch.bfloat16, "fp32": torch.float32}
MV_E_UNSUPPORTED = -2
assert N.SENTINEL == SENTINEL and N.GUARD == GUARD


def _opt(a):
    return None if a is None else _dev(a, "fp32")


def _take(y, M, C, tag):
    torch.cuda.synchronize()
    body, guard = _read(y, M, C)
    assert guard.numel() == GUARD and bool((guard == SENTINEL).all()), f"{tag}: guard behind the destination overwritten"
    return body.numpy().astype(F64)


def _report(tag, kern, expect, got, ref, bound, out):
    """Prints the figures, then asserts the kernel name, the sentinel, the bound and the bias."""
    a, b = N.judge(got, ref, bound, out)
    print(f"{tag} [{kern}]: worst |got-ref|/bound {a.get('worst', float('nan')):.3f} over {a.get('n')} elements, "
          f"violations {a.get('nviol')} | bias {b['bias']:+.4f} over {b['n_bias']}")
    assert kern == expect, f"{tag}: served by {kern!r}, expected {expect!r}"
    # a sentinel survives where the output equals it and the reference is further from it than the bound allows a result to be
    left = int(((got == SENTINEL) & (np.abs(np.asarray(ref) - SENTINEL) > bound)).sum())
    assert left == 0, f"{tag}: {left} sentinel values left inside the output"
    assert a["ok"], f"{tag} bound: {a}"
    assert b["ok"], f"{tag} bias: {b}"


def _report_rep(tag, kern, expect, got, idx, ref, bound, out):
    bad = N.judge_rep(got, idx, ref, bound, out)
    print(f"{tag} [{kern}]: row invariance / isolation over {len(idx)} rows: {'ok' if not bad else bad}")
    assert kern == expect and not bad, (tag, kern, bad)


# ================================================================================================ mv_layernorm_fwd
def _ln_fwd(c, x, g, b):
    xd, gd, bd = _dev(N.strided(x, c.xs) if c.stride else np.array(x), c.din), _opt(g), _opt(b)
    y = _dest(c.M, c.C, TT[c.dout])
    with _Flags(c.flags):
        _lib.call("mv_layernorm_fwd", _p(xd), _p(gd), _p(bd), _p(y), c.M, c.C, c.stride, N.EPS, DT[c.din], DT[c.dout], _stream())
        kern = _lib.last_kernel()
    return _take(y, c.M, c.C, c.id), kern


@pytest.mark.parametrize("i", range(len(N.LN_CASES)), ids=[c.id for c in N.LN_CASES])
def test_layernorm_fwd(i):
    """Gaussian (or offset / small-sigma / constant) rows: bound and bias; then the three-base-row input with a NaN row: invariance
    and isolation.  A strided case carries NaN in its gap columns in both launches."""
    c, x, g, b, ref, bound = N.ln_case_data(i)
    got, kern = _ln_fwd(c, x, g, b)
    _report("layernorm/" + c.id, kern, c.expect, got, ref, bound, c.dout)
    xr, idx = N.rep_rows(c.M, c.C, c.din)
    refr, boundr = N.ln_ref_bound(xr, g, b, None, N.EPS, c.dout, k_mean=c.k_mean)
    gotr, kern = _ln_fwd(c, xr, g, b)
    _report_rep("layernorm/" + c.id, kern, c.expect, gotr, idx, refr, boundr, c.dout)


# ================================================================================================ mv_layernorm_add_fwd
def _ln_add(M, C, zd, z, res, g, b, lo):
    zdv, rd, gd, bd = _dev(z, zd), _opt(res), _opt(g), _opt(b)
    y = _dest(M, C, torch.float32)
    ylo = None if lo is None else _dest(M, C, TT[lo])
    _lib.call("mv_layernorm_add_fwd", _p(zdv), _p(rd), _p(gd), _p(bd), _p(y), _p(ylo), M, C, N.EPS, DT[zd], DT[lo or "bf16"], _stream())
    kern = _lib.last_kernel()
    tag = f"layernorm_add/{M}x{C}/{zd}"
    return _take(y, M, C, tag), (None if lo is None else _take(ylo, M, C, tag + "/lo")), kern


def _add_case(M, C, zd, with_res, lo):
    z, res, g, b, ref, bound = N.add_data(M, C, zd, with_res)
    y, ylo, kern = _ln_add(M, C, zd, z, res, g, b, lo)
    tag = f"layernorm_add/nch{C // N.EPC[zd]}_ch%dw%d_M{M}_{zd}_res{int(with_res)}_lo{lo}" % N.vec_shape(C // N.EPC[zd])
    _report(tag, kern, "layernorm_add", y, ref, bound, "fp32")
    if lo is not None:
        info = S.check_exact(ylo, S.store(y.astype(F32), lo))
        print(f"{tag} [{kern}]: y_lo == round_{lo}(y) exact {info['ok']} wrong {info.get('nbad')} of {info.get('n')}")
        assert info["ok"], info
    zr, idx = N.rep_rows(M, C, zd)
    refr, boundr = N.ln_ref_bound(zr, g, b, None, N.EPS, "fp32")
    yr, ylor, kern = _ln_add(M, C, zd, zr, None, g, b, lo)
    _report_rep(tag, kern, "layernorm_add", yr, idx, refr, boundr, "fp32")
    if lo is not None:
        keep = idx >= 0
        assert S.check_exact(ylor[keep], S.store(yr[keep].astype(F32), lo))["ok"] and np.isnan(ylor[~keep]).all()


@pytest.mark.parametrize("nch,zd,with_res,lo", N.ADD_CASES)
def test_layernorm_add(nch, zd, with_res, lo):
    _add_case(37, nch * N.EPC[zd], zd, with_res, lo)


def test_layernorm_add_gridstride():
    """16485 row groups on 8192 waves: the first 101 waves take a third trip."""
    _add_case(*N.ADD_GRIDSTRIDE)


def test_layernorm_add_ragged_width_unsupported():
    """C = 100 with bf16 z is 12.5 chunks: MV_E_UNSUPPORTED, nothing written."""
    M, C = 37, 100
    z, g, b = _dev(N.rows_data(M, C, "bf16"), "bf16"), _dev(np.ones(C, F32), "fp32"), _dev(np.zeros(C, F32), "fp32")
    y, ylo = _dest(M, C, torch.float32), _dest(M, C, torch.bfloat16)
    rc = _lib.load().mv_layernorm_add_fwd(_p(z), None, _p(g), _p(b), _p(y), _p(ylo), M, C, N.EPS, DT["bf16"], DT["bf16"], _stream())
    torch.cuda.synchronize()
    assert rc == MV_E_UNSUPPORTED, rc
    assert bool((y == SENTINEL).all()) and bool((ylo == SENTINEL).all()), "an unsupported call wrote to its destination"


# ================================================================================================ mv_patch_merge_ln_fwd
def _unmerge(rows, B, H, W, C):
    """The inverse of N.merge_rows: (B Ho Wo, 4 C) -> (B, H, W, C)."""
    m = rows.reshape(B, H // 2, W // 2, 4, C)
    x = np.empty((B, H, W, C), rows.dtype)
    x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2] = m[..., 0, :], m[..., 1, :], m[..., 2, :], m[..., 3, :]
    return x


def _pm(x, g, b, out):
    B, H, W, C = x.shape
    rows = B * (H // 2) * (W // 2)
    xd, gd, bd = _dev(x, "fp32"), _dev(g, "fp32"), _dev(b, "fp32")
    y = _dest(rows, 4 * C, TT[out])
    _lib.call("mv_patch_merge_ln_fwd", _p(xd), _p(gd), _p(bd), _p(y), B, H, W, C, N.EPS, DT["fp32"], DT[out], _stream())
    kern = _lib.last_kernel()
    return _take(y, rows, 4 * C, f"patch_merge_ln/C{C}"), kern


@pytest.mark.parametrize("out", ["bf16", "fp32"])
@pytest.mark.parametrize("B,H,W,C", N.PM_CASES + [N.PM_GRIDSTRIDE], ids=lambda v: str(v))
def test_patch_merge_ln(B, H, W, C, out):
    assert _lib.load().mv_patch_merge_ln_supported(H, W, C, DT["fp32"]) == 1
    x, g, b = N.pm_data(B, H, W, C)
    assert np.array_equal(_unmerge(N.merge_rows(x), B, H, W, C), x)
    ref, bound = N.ln_ref_bound(N.merge_rows(x), g, b, None, N.EPS, out, k_mean=1, k_mul=2, k_add=1)
    got, kern = _pm(x, g, b, out)
    tag = f"patch_merge_ln/{B}x{H}x{W}x{C}_nv{N.pm_nv(C)}_{out}"
    _report(tag, kern, "patch_merge_ln_f32in", got, ref, bound, out)
    rows, idx = N.rep_rows(ref.shape[0], 4 * C, "fp32")
    refr, boundr = N.ln_ref_bound(rows, g, b, None, N.EPS, out, k_mean=1, k_mul=2, k_add=1)
    gotr, kern = _pm(_unmerge(rows, B, H, W, C), g, b, out)
    _report_rep(tag, kern, "patch_merge_ln_f32in", gotr, idx, refr, boundr, out)


def test_patch_merge_ln_refusals():
    lib = _lib.load()
    assert lib.mv_patch_merge_ln_supported(4, 6, 12, DT["fp32"]) == 0
    assert lib.mv_patch_merge_ln_supported(5, 6, 16, DT["fp32"]) == 0
    x, g, b = _dev(np.zeros((1, 4, 6, 12), F32), "fp32"), _dev(np.ones(48, F32), "fp32"), _dev(np.zeros(48, F32), "fp32")
    y = _dest(6, 48)
    rc = lib.mv_patch_merge_ln_fwd(_p(x), _p(g), _p(b), _p(y), 1, 4, 6, 12, N.EPS, DT["fp32"], DT["bf16"], _stream())
    torch.cuda.synchronize()
    assert rc == MV_E_UNSUPPORTED and bool((y == SENTINEL).all())


# ================================================================================================ moments
def _moments(entry, x, shift, dtype, squared=None):
    """Two calls on a NaN-filled workspace and a sentinel-filled guarded destination; the results must be bitwise equal."""
    rows, C = x.shape
    both = entry == "mv_channel_moments2_fwd"
    n_out = 2 * C if both else C
    xd, sd = _dev(x, dtype), _opt(shift)
    n_ws = _lib.load().mv_channel_moments_ws(C) * (2 if both else 1)
    outs = []
    for _ in range(2):
        ws = torch.full((n_ws + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
        y = _dest(1, n_out, torch.float32)
        if both:
            _lib.call(entry, _p(xd), _p(sd), _p(y), _p(ws), rows, C, DT[dtype], _stream())
        else:
            _lib.call(entry, _p(xd), _p(sd), _p(y), _p(ws), rows, C, squared, DT[dtype], _stream())
        kern = _lib.last_kernel()
        outs.append(_take(y, 1, n_out, entry)[0])
    assert np.array_equal(outs[0].view(np.uint64), outs[1].view(np.uint64)), f"{entry}: two calls differ"
    return outs[0], kern


MOM = [(r, c, d) for r, c in N.MOM_CASES for d in ("bf16", "fp32")] + [N.MOM_CAP + ("bf16",)]


def _mom_line(tag, kern, info):
    print(f"{tag} [{kern}]: exact {info['ok']} wrong {info.get('nbad')} of {info.get('n')} | bound n/a | bias n/a")


@pytest.mark.parametrize("rows,C,dtype", MOM, ids=[f"{r}x{c}_{d}" for r, c, d in MOM])
def test_moments_exact(rows, C, dtype):
    x, shift = N.mom_data(rows, C, dtype, "int")
    N.prove_mom_exact(f"{rows}x{C}", x, shift, rows)
    (s1, _), (d1, _), (d2, _) = N.mom_ref(x, None, 1), N.mom_ref(x, shift, 1), N.mom_ref(x, shift, 2)
    tag = f"moments/{rows}x{C}/{dtype}/G{N.mom_geometry(rows, C)[3]}"
    for entry, sh, sq, ref, expect in (("mv_channel_moments_fwd", None, 0, s1, "channel_sum"),
                                       ("mv_channel_moments_fwd", shift, 1, d2, "channel_sqdev"),
                                       ("mv_channel_moments2_fwd", shift, None, np.concatenate([d1, d2]), "channel_moments2")):
        got, kern = _moments(entry, x, sh, dtype, sq)
        info = S.check_exact(got, ref)
        _mom_line(tag, kern, info)
        assert kern == expect and info["ok"], (kern, info)


@pytest.mark.parametrize("rows,C,dtype", MOM, ids=[f"{r}x{c}_{d}" for r, c, d in MOM])
def test_moments_bound(rows, C, dtype):
    x, shift = N.mom_data(rows, C, dtype, "gauss")
    (r1, m1), (r2, m2) = N.mom_ref(x, shift, 1), N.mom_ref(x, shift, 2)
    tag = f"moments/{rows}x{C}/{dtype}/G{N.mom_geometry(rows, C)[3]}"
    got, kern = _moments("mv_channel_moments2_fwd", x, shift, dtype)
    _report(tag, kern, "channel_moments2", got, np.concatenate([r1, r2]), N.mom_bound(rows, np.concatenate([m1, m2])), "fp32")
    got, kern = _moments("mv_channel_moments_fwd", x, shift, dtype, 1)
    _report(tag, kern, "channel_sqdev", got, r2, N.mom_bound(rows, m2), "fp32")
    if rows * C <= 1 << 22:
        r0, m0 = N.mom_ref(x, None, 1)
        got, kern = _moments("mv_channel_moments_fwd", x, None, dtype, 0)
        _report(tag, kern, "channel_sum", got, r0, N.mom_bound(rows, m0), "fp32")


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("sigmas", [0.0, 0.3, 3.0])
@pytest.mark.parametrize("rows,C", [(1000, 96), (37, 2048)])
def test_moments2_shift(rows, C, sigmas, dtype):
    """The shift at the mean, at 0.3 sigma and at 3 sigma from it: the bound is computed per case from sum |x - shift|^p."""
    x, shift = N.mom_data(rows, C, dtype, "gauss", sigmas)
    (r1, m1), (r2, m2) = N.mom_ref(x, shift, 1), N.mom_ref(x, shift, 2)
    got, kern = _moments("mv_channel_moments2_fwd", x, shift, dtype)
    _report(f"moments2/{rows}x{C}/{dtype}/shift{sigmas}", kern, "channel_moments2", got, np.concatenate([r1, r2]),
            N.mom_bound(rows, np.concatenate([m1, m2])), "fp32")


@pytest.mark.parametrize("C", [12, 2056])
def test_moments_refusals(C):
    lib = _lib.load()
    assert lib.mv_channel_moments_supported(64, C, DT["fp32"]) == 0
    x, sh = _dev(np.zeros((64, C), F32), "fp32"), _dev(np.zeros(C, F32), "fp32")
    ws = torch.zeros(2 * 1024 * C, dtype=torch.float32, device="cuda")
    y = _dest(1, 2 * C, torch.float32)
    rc1 = lib.mv_channel_moments_fwd(_p(x), None, _p(y), _p(ws), 64, C, 0, DT["fp32"], _stream())
    rc2 = lib.mv_channel_moments2_fwd(_p(x), _p(sh), _p(y), _p(ws), 64, C, DT["fp32"], _stream())
    torch.cuda.synchronize()
    assert rc1 == MV_E_UNSUPPORTED and rc2 == MV_E_UNSUPPORTED and bool((y == SENTINEL).all())


# ================================================================================================ fold kernels
def _guarded(a):
    """A device copy of the fp32 vector `a` with the sentinel guard behind it (for the values a kernel updates in place)."""
    t = _dest(1, a.size, torch.float32)
    t[:a.size] = torch.from_numpy(np.ascontiguousarray(a, F32)).cuda()
    return t


def _fold_outputs(C, tag, **bufs):
    return {k: _take(t, 1, C, f"{tag}/{k}")[0] for k, t in bufs.items()}


def _count(n, on_device):
    return (_dev(np.array([n], F32), "fp32"), 0.0) if on_device else (None, float(n))


@pytest.mark.parametrize("count_on_device", [False, True], ids=["host_count", "device_count"])
@pytest.mark.parametrize("C", [8, 264])
def test_bn_mean(C, count_on_device):
    d = N.fold_data(C)
    cd, ch = _count(d["n"], count_on_device)
    sd, y = _dev(d["sum"], "fp32"), _dest(1, C, torch.float32)
    _lib.call("mv_bn_mean_fwd", _p(sd), _p(cd), ch, _p(y), C, _stream())
    kern = _lib.last_kernel()
    ref, mag, n_ops = N.bn_mean_ref(d["sum"], d["n"])
    _report(f"bn_mean/C{C}", kern, "bn_mean", _take(y, 1, C, "bn_mean")[0], ref, S.ops_bound(ref, mag, n_ops, "fp32"), "fp32")


@pytest.mark.parametrize("affine", [True, False], ids=["affine", "no_affine"])
@pytest.mark.parametrize("first_time", [0, 1])
@pytest.mark.parametrize("count_on_device", [False, True], ids=["host_count", "device_count"])
@pytest.mark.parametrize("C", [8, 264])
def test_bn_ema_fold(C, count_on_device, first_time, affine):
    """run_mean / run_var are updated in place: compared with the float64 update of the values they held before the call."""
    d = N.fold_data(C)
    w, b = (d["weight"], d["bias"]) if affine else (None, None)
    cd, ch = _count(d["n"], count_on_device)
    rm, rv, sc, sh = _guarded(d["run_mean"]), _guarded(d["run_var"]), _dest(1, C, torch.float32), _dest(1, C, torch.float32)
    sq, mn, wd, bd = _dev(d["sqdev"], "fp32"), _dev(d["mean"], "fp32"), _opt(w), _opt(b)
    _lib.call("mv_bn_ema_fold_fwd", _p(sq), _p(mn), _p(cd), ch, _p(rm), _p(rv), _p(wd), _p(bd), _p(sc), _p(sh), float(d["momentum"]),
              float(d["eps"]), first_time, C, _stream())
    kern = _lib.last_kernel()
    got = _fold_outputs(C, "bn_ema_fold", run_mean=rm, run_var=rv, scale=sc, shift=sh)
    refs = N.fold_ref(d["sqdev"], d["mean"], d["n"], d["run_mean"], d["run_var"], w, b, d["momentum"], d["eps"], first_time)
    for k, (ref, mag, n_ops) in refs.items():
        _report(f"bn_ema_fold/C{C}/first{first_time}/{k}", kern, "bn_ema_fold", got[k], ref, S.ops_bound(ref, mag, n_ops, "fp32"), "fp32")


def _fold1(C, sums, n, run_mean, run_var, w, b, momentum, eps, count_on_device):
    cd, ch = _count(n, count_on_device)
    rm, rv, sc, sh = _guarded(run_mean), _guarded(run_var), _dest(1, C, torch.float32), _dest(1, C, torch.float32)
    sd, wd, bd = _dev(sums, "fp32"), _opt(w), _opt(b)
    _lib.call("mv_bn_ema_fold1_fwd", _p(sd), _p(cd), ch, _p(rm), _p(rv), _p(wd), _p(bd), _p(sc), _p(sh), float(momentum), float(eps), C,
              _stream())
    kern = _lib.last_kernel()
    return _fold_outputs(C, "bn_ema_fold1", run_mean=rm, run_var=rv, scale=sc, shift=sh), kern


@pytest.mark.parametrize("affine", [True, False], ids=["affine", "no_affine"])
@pytest.mark.parametrize("count_on_device", [False, True], ids=["host_count", "device_count"])
@pytest.mark.parametrize("C", [8, 264])
def test_bn_ema_fold1(C, count_on_device, affine):
    d = N.fold_data(C)
    w, b = (d["weight"], d["bias"]) if affine else (None, None)
    got, kern = _fold1(C, d["sums"], d["n"], d["run_mean"], d["run_var"], w, b, d["momentum"], d["eps"], count_on_device)
    refs = N.fold1_ref(d["sums"], d["n"], d["run_mean"], d["run_var"], w, b, d["momentum"], d["eps"])
    for k, (ref, bound) in refs.items():
        _report(f"bn_ema_fold1/C{C}/{k}", kern, "bn_ema_fold1", got[k], ref, bound, "fp32")


@pytest.mark.parametrize("zero_run_var", [False, True], ids=["run_var_old", "run_var_0"])
@pytest.mark.parametrize("C", [8, 264])
def test_bn_ema_fold1_constant_channels(C, zero_run_var):
    """sums of a constant input: variance 0 through the fmaxf clamp, run_var = momentum * run_var_old within the counted
    operations, never negative, never NaN -- also when run_var_old is 0 and a negative residue would show."""
    sums, _ = N.const_sums(C)
    d = N.fold_data(C)
    rv0 = np.zeros(C, F32) if zero_run_var else d["run_var"]
    got, kern = _fold1(C, sums, 1568.0, d["run_mean"], rv0, None, None, d["momentum"], d["eps"], False)
    refs = N.fold1_ref(sums, 1568.0, d["run_mean"], rv0, None, None, d["momentum"], d["eps"])
    rv, bound = refs["run_var"]
    assert np.isfinite(got["run_var"]).all() and (got["run_var"] >= 0).all(), got["run_var"]
    for k, (ref, bnd) in refs.items():
        _report(f"bn_ema_fold1_const/C{C}/{k}", kern, "bn_ema_fold1", got[k], ref, bnd, "fp32")
    target = float(d["momentum"]) * rv0.astype(F64)
    assert (np.abs(got["run_var"] - target) <= bound + np.abs(rv - target)).all()
