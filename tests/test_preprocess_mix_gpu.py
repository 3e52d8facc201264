"""GPU: `mv_preprocess_u8_mix_fwd`, `eqxvision_amd.preprocess.crop_resize_normalize_mix` / `imagenet_train_mixed` and
`eqv.optim.ema`.  Every comparison is of BITS: the reference is tests/_mix_ref.py applied to the fp32 outputs of the EXISTING
`crop_resize_normalize` on the same boxes and flips.

Tiles (`pick_tile`): with these small sources every launch takes the 32 x 32 tile (at most 64 x 71 staged pixels, 24.5 KiB of
horizontal sums, 12 KiB of kept partner values: under 64 KiB).  The 24 x 40 output is one row of two tiles, columns [0, 32) and
[32, 40); the 72 x 72 output is 3 x 3 tiles with edges at 32 and 64.  The scenarios place rectangles strictly inside a tile, across
tile edges, and exactly on them (a whole tile inside a cut or an erase rectangle takes the paths that skip a resample)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import eqxvision_amd as eqv
from eqxvision_amd import _lib, _optim
from eqxvision_amd import preprocess as P
from eqxvision_amd import random as jr
from eqxvision_amd._module import DevArray
from tests import _mix_ref as M
from tests import _preprocess_ref as R
from tests._slices import _stream

pytestmark = pytest.mark.gpu

SIZES5 = [(37, 53), (64, 48), (40, 40), (33, 71), (50, 34)]
BOXES5 = [(2, 3, 30, 44), (0, 0, 64, 48), (5, 5, 30, 30), (1, 0, 32, 71), (10, 4, 40, 30)]
FLIPS5 = [False, True, False, True, True]
ROLL5 = [4, 0, 1, 2, 3]
NONE = (0, 0, 0, 0)
SIZES3 = [(64, 48), (50, 34), (40, 40)]
BOXES3 = [(0, 0, 64, 48), (3, 2, 45, 30), (0, 0, 40, 40)]
FLIPS3 = [True, False, False]


def _scn(partner, lam, cut=None, erase=None):
    B = len(partner)
    return dict(partner=partner, lam=np.asarray(lam, np.float32), cut=[NONE] * B if cut is None else cut,
                erase=[NONE] * B if erase is None else erase)


# name -> (which batch, scenario).  24 x 40 unless "72".
SCENARIOS = {
    "mixup_025": ("5", _scn(ROLL5, [0.25] * 5)),
    # image 0 erased inside the first tile, image 2 wholly, image 4 in the corner across the tile edge at 32: each shows in its own
    # output and in the image it is the partner of (1, 3, 0)
    "mixup_07309_erase": ("5", _scn(ROLL5, [0.7309] * 5, erase=[(3, 5, 10, 20), NONE, (0, 0, 24, 40), NONE, (20, 30, 24, 40)])),
    # cut: interior of the first tile / touching two borders / the full image / empty / exactly the second tile; erase rectangles
    # overlapping the cut (image 0), of the partner under the cut (image 4 is image 0's partner)
    "cutmix": ("5", _scn(ROLL5, [1.0] * 5, cut=[(5, 7, 20, 29), (0, 0, 10, 12), (0, 0, 24, 40), NONE, (0, 32, 24, 40)],
                         erase=[(10, 20, 22, 35), NONE, NONE, (0, 0, 24, 32), (0, 0, 12, 12)])),
    # no partner with lam < 1 / a partner with lam == 1 and no cut / lam == 0 / a mix with a cut and both erased / lam == 1, empty cut
    "bag": ("5", _scn([0, 3, 4, 1, 2], [0.3, 1.0, 0.0, 0.5, 1.0], cut=[(1, 1, 9, 9), NONE, NONE, (4, 30, 20, 36), (7, 7, 7, 30)],
                      erase=[(2, 2, 5, 39), (0, 0, 24, 40), (1, 33, 23, 39), (10, 10, 15, 34), NONE])),
    # 72 x 72, tile edges at 32 and 64: cut exactly tile (1, 0) / across every edge / none; erase exactly tile (0, 1) / strictly
    # inside tile (1, 1) / the full image
    "72": ("3", _scn([2, 0, 1], [0.25, 1.0, 0.7309], cut=[(32, 0, 64, 32), (10, 20, 70, 50), NONE],
                     erase=[(0, 32, 32, 64), (33, 33, 63, 63), (0, 0, 72, 72)])),
}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    _lib.load()
    _lib.check_device_status()
    yield
    _lib.check_device_status()


@functools.lru_cache(maxsize=None)
def _batch(which):
    """(images HWC, boxes, flips, size, v): v the fp32 [B, 3, H, W] output of the existing core, computed once, read-only."""
    sizes, boxes, flips, size = (SIZES5, BOXES5, FLIPS5, (24, 40)) if which == "5" else (SIZES3, BOXES3, FLIPS3, (72, 72))
    ims = tuple(R.images(hw, 1)[0] for hw in sizes)
    v = P.crop_resize_normalize(list(ims), boxes, size, flips).cpu().numpy()
    assert _lib.last_kernel() == "preprocess_u8_boxes"
    v.setflags(write=False)
    return ims, boxes, flips, size, v


@functools.lru_cache(maxsize=None)
def _want(name):
    which, s = SCENARIOS[name]
    out = M.mix(_batch(which)[4], s["partner"], s["lam"], M.one_minus(s["lam"]), s["cut"], s["erase"])
    out.setflags(write=False)
    return out


def _bits(t, nhwc=False):
    t = t.permute(0, 3, 1, 2) if nhwc else t
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu().numpy()


def _want_bits(want, dtype):
    return want.view(np.int32) if dtype == "fp32" else M.bf16_bits(want).view(np.int16)


def _read_status():
    v = ctypes.c_uint(0)
    assert _lib.load().mv_device_status(1, ctypes.byref(v)) == 0
    return v.value


@pytest.mark.parametrize("nhwc", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("chw", [False, True], ids=["hwc_in", "chw_in"])
def test_every_scenario_bit_for_bit(chw, dtype, nhwc):
    for name, (which, s) in SCENARIOS.items():
        ims, boxes, flips, size, _ = _batch(which)
        src = [np.ascontiguousarray(im.transpose(2, 0, 1)) if chw else im for im in ims]
        x, t = P.crop_resize_normalize_mix(src, boxes, size, flips, partner=s["partner"], lam=s["lam"], cut=s["cut"], erase=s["erase"],
                                           dtype=dtype, layout="nhwc" if nhwc else "nchw")
        assert _lib.last_kernel() == "preprocess_u8_mix" and t is None
        got, want = _bits(x, nhwc), _want_bits(_want(name), dtype)
        assert got.shape == want.shape
        assert np.array_equal(got, want), (name, np.argwhere(got != want)[:8].tolist())
    assert _lib.check_device_status() == 0


def test_the_scenarios_exercise_what_they_claim():
    """The references differ from the unmixed output where they should, hold zeros of both signs' worth of care (lam == 0 gives
    fadd(fmul(0, v_i), v_r): the reference decides the sign), and no partner / lam == 1 / empty cut leave the image as it is."""
    v5 = _batch("5")[4]
    bag = _want("bag")
    assert np.array_equal(bag[1].view(np.int32), np.zeros_like(bag[1]).view(np.int32))           # lam == 1, own erase = the image
    assert np.array_equal(bag[4].view(np.int32), v5[4].view(np.int32))                           # lam == 1, empty cut
    own0 = M.erased(v5, SCENARIOS["bag"][1]["erase"])[0]
    assert np.array_equal(bag[0].view(np.int32), own0.view(np.int32))                            # no partner: cut and lam ignored
    part = M.erased(v5, SCENARIOS["bag"][1]["erase"])[4]
    zero_own = (np.float32(0.0) * M.erased(v5, SCENARIOS["bag"][1]["erase"])[2]) + part
    assert np.array_equal(bag[2].view(np.int32), zero_own.view(np.int32))
    cm = _want("cutmix")
    assert not cm[0, :, 5:12, 7:12].any() and np.array_equal(cm[0, :, 12:20, 7:20], v5[4][:, 12:20, 7:20])   # the partner, erased
    assert np.array_equal(cm[2], v5[1]) and np.array_equal(cm[4, :, :, 32:], v5[3][:, :, 32:]) and not cm[4, :, :12, :12].any()
    assert np.array_equal(cm[3, :, :, 32:], v5[3][:, :, 32:]) and not cm[3, :, :, :32].any()
    for name in SCENARIOS:
        assert not np.array_equal(_want(name), _batch(SCENARIOS[name][0])[4])


def test_array_input_single_image_and_partner_free_batch():
    """An array of equally sized images == the list of them; no mixing at all == the existing core bit for bit (bf16 too); a single
    image goes through with an erase rectangle."""
    arr = R.images((45, 52), 3)
    boxes, flips = [(0, 0, 45, 52), (3, 4, 40, 40), (5, 0, 30, 52)], [False, True, False]
    kw = dict(partner=[1, 2, 0], lam=[0.7309, 0.25, 1.0], cut=[NONE, (3, 3, 20, 38), (0, 0, 24, 10)], erase=[(1, 1, 9, 9), NONE, (0, 30, 24, 40)])
    for chw in (False, True):
        batch = np.ascontiguousarray(arr.transpose(0, 3, 1, 2)) if chw else arr
        a, _ = P.crop_resize_normalize_mix(batch, boxes, (24, 40), flips, **kw)
        b, _ = P.crop_resize_normalize_mix(list(batch), boxes, (24, 40), flips, **kw)
        c, _ = P.crop_resize_normalize_mix(torch.from_numpy(batch).cuda(), boxes, (24, 40), flips, **kw)
        v = P.crop_resize_normalize(batch, boxes, (24, 40), flips).cpu().numpy()
        want = M.mix(v, kw["partner"], np.float32(kw["lam"]), M.one_minus(kw["lam"]), kw["cut"], kw["erase"])
        assert np.array_equal(_bits(a), want.view(np.int32)) and np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(c))
    for dtype in ("fp32", "bf16"):
        plain, t = P.crop_resize_normalize_mix(arr, boxes, (24, 40), flips, dtype=dtype)
        assert t is None and np.array_equal(_bits(plain), _bits(P.crop_resize_normalize(arr, boxes, (24, 40), flips, dtype=dtype)))
    one, t = P.crop_resize_normalize_mix(arr[1], boxes[1], (24, 40), True, labels=3, num_classes=7, erase=(2, 2, 20, 20))
    v = P.crop_resize_normalize(arr[1], boxes[1], (24, 40), True).cpu().numpy()
    assert tuple(one.shape) == (3, 24, 40) and np.array_equal(one.cpu().numpy().view(np.int32), M.erased(v[None], [(2, 2, 20, 20)])[0].view(np.int32))
    assert np.asarray(t).tolist() == [0, 0, 0, 1, 0, 0, 0]
    assert _lib.check_device_status() == 0


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("K", [7, 1000])
def test_targets(K, eps):
    """Bits of the reference; every row sums to 1 within 2^-20 (summed in float64)."""
    ims, boxes, flips, size, _ = _batch("5")
    labels = np.array([0, K - 1, 3, K - 1, 5], np.int64)
    for lam_t in ([0.25] * 5, [0.7309, 1.0, 0.0, 0.5, 0.123]):
        for labs in (labels, torch.from_numpy(labels.astype(np.int32)).cuda()):
            x, t = P.crop_resize_normalize_mix(list(ims), boxes, size, flips, labs, K, partner=ROLL5, lam=[0.5] * 5, lam_t=lam_t,
                                               label_smoothing=eps)
            assert isinstance(t, DevArray) and t.shape == (5, K)
            got = np.asarray(t)
            want = M.targets(labels, ROLL5, np.float32(lam_t), M.one_minus(lam_t), K, eps)
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), np.argwhere(got != want)[:8].tolist()
            sums = got.astype(np.float64).sum(1)
            print(f"K {K} eps {eps}: worst |row sum - 1| = {np.abs(sums - 1).max():.3e}")
            assert np.all(np.abs(sums - 1.0) <= 2.0 ** -20)
    assert _lib.check_device_status() == 0


def _entry(scenario, which="5", dtype="fp32", labels=None, K=7, lam_t=None, mix_dev=None, labels_dev=None, with_targets=True):
    """The C entry with y and targets allocated INSIDE larger NaN-filled buffers; returns (y fp32 [B, 3, H, W], targets or None),
    after checking that everything around them is still NaN (and the targets buffer too, when no labels were given)."""
    ims, boxes, flips, size, _ = _batch(which)
    B, (H, W) = len(ims), size
    rec, _ = P.boxes_plan([im.shape[:2] for im in ims], boxes, flips, size)
    mix = P.mix_plan(B, size, scenario["partner"], scenario["lam"], scenario["cut"], scenario["erase"], lam_t)
    a, b = P.affine(P.IMAGENET_MEAN, P.IMAGENET_STD)
    x = torch.from_numpy(np.concatenate([im.reshape(-1) for im in ims])).cuda()
    dev = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (rec.view(np.uint8), (mix if mix_dev is None else mix_dev).view(np.uint8), a, b)]
    pad, n, nt = 256, B * 3 * H * W, B * K
    ybuf = torch.full((pad + n + pad,), float("nan"), dtype=P.TORCH_DT[dtype], device="cuda")
    tbuf = torch.full((pad + nt + pad,), float("nan"), dtype=torch.float32, device="cuda")
    lab_host = None if labels is None else np.ascontiguousarray(labels, np.int32)
    lab_dev = None
    if labels_dev is not None or labels is not None:
        lab_dev = torch.from_numpy(np.ascontiguousarray(labels if labels_dev is None else labels_dev, np.int32)).cuda()
    on, off = P.smoothing_values(0.0, K)
    esz = ybuf.element_size()
    _lib.call("mv_preprocess_u8_mix_fwd", x.data_ptr(), x.numel(), ybuf.data_ptr() + pad * esz, rec.ctypes.data, dev[0].data_ptr(),
              mix.ctypes.data, dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), None if lab_host is None else lab_host.ctypes.data,
              None if lab_dev is None else lab_dev.data_ptr(), None if lab_dev is None else tbuf.data_ptr() + pad * 4, K, float(on),
              float(off), B, H, W, 0, P.DT[dtype], 0, _stream())
    torch.cuda.synchronize()
    yh, th = ybuf.float().cpu().numpy(), tbuf.cpu().numpy()
    assert np.isnan(yh[:pad]).all() and np.isnan(yh[pad + n:]).all(), "written outside y"
    assert np.isnan(th[:pad]).all() and np.isnan(th[pad + nt:]).all(), "written outside the targets"
    assert not np.isnan(yh[pad:pad + n]).any(), "elements of y left unwritten"
    if lab_dev is None:
        assert np.isnan(th).all(), "targets written without labels"
        return yh[pad:pad + n].reshape(B, 3, H, W), None
    assert not np.isnan(th[pad:pad + nt]).any(), "targets left unwritten"
    return yh[pad:pad + n].reshape(B, 3, H, W), th[pad:pad + nt].reshape(B, K)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_nothing_outside_the_outputs_is_written(dtype):
    for name in ("cutmix", "72"):
        which, s = SCENARIOS[name]
        B = len(s["partner"])
        y, t = _entry(s, which, dtype, labels=list(range(B)), K=7, lam_t=[0.5] * B)
        want = _want(name) if dtype == "fp32" else (M.bf16_bits(_want(name)).astype(np.uint32) << 16).view(np.float32)
        assert np.array_equal(y.view(np.int32), want.view(np.int32)), name
        assert np.array_equal(t.view(np.int32), M.targets(list(range(B)), s["partner"], [0.5] * B, [0.5] * B, 7, 0.0).view(np.int32))
        y, t = _entry(s, which, dtype)                                                  # labels == NULL: no target block
        assert t is None and np.array_equal(y.view(np.int32), want.view(np.int32))
    assert _read_status() == 0


def test_device_records_that_differ_from_the_host_copy_are_clamped_not_followed():
    """The DEVICE copy of the mix records says something else than the validated host copy: a partner outside [0, B) is treated as
    none, a rectangle beyond the output is clamped to it, each raising bit 2; a device label of K matches no class and raises bit
    3.  Every run completes and the status reads clean after it was cleared."""
    which, s = SCENARIOS["cutmix"]
    ims, boxes, flips, size, v = _batch(which)
    host = P.mix_plan(5, size, s["partner"], s["lam"], s["cut"], s["erase"], [0.25] * 5)
    clean, _ = _entry(s)
    assert _read_status() == 0 and np.array_equal(clean.view(np.int32), _want("cutmix").view(np.int32))

    bad = host.copy()
    bad["partner"][1] = 99
    bad["partner"][3] = -1
    got, t = _entry(s, mix_dev=bad, labels=[0, 1, 2, 3, 4], lam_t=[0.25] * 5)
    assert _read_status() & 4
    partner = [4, 1, 1, 3, 3]
    want = M.mix(v, partner, s["lam"], M.one_minus(s["lam"]), s["cut"], s["erase"])
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert np.array_equal(t.view(np.int32), M.targets([0, 1, 2, 3, 4], partner, [0.25] * 5, [0.75] * 5, 7, 0.0).view(np.int32))
    assert _read_status() == 0

    bad = host.copy()
    bad["cy1"][0], bad["cx1"][0] = 200, 290                      # (5, 7, 20, 29) -> clamped to (5, 7, 24, 40)
    bad["ey0"][4], bad["ex0"][4] = -3, -1000                     # (0, 0, 12, 12) as it is after the clamp
    got, _ = _entry(s, mix_dev=bad)
    assert _read_status() & 4
    cut = list(s["cut"])
    cut[0] = (5, 7, 24, 40)
    want = M.mix(v, s["partner"], s["lam"], M.one_minus(s["lam"]), cut, s["erase"])
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert _read_status() == 0

    got, t = _entry(s, labels_dev=[0, 7, 2, -1, 6], lam_t=[0.25] * 5)
    assert _read_status() == 8
    assert np.array_equal(got.view(np.int32), clean.view(np.int32))
    assert np.array_equal(t.view(np.int32), M.targets([0, 7, 2, -1, 6], s["partner"], [0.25] * 5, [0.75] * 5, 7, 0.0).view(np.int32))
    assert t[1].tolist() == [0.75, 0, 0, 0, 0, 0, 0] and t[3].tolist() == [0, 0, 0.75, 0, 0, 0, 0]      # their own labels matched nothing
    assert _read_status() == 0


def test_imagenet_train_mixed_preset():
    """== the core on the draws of the four-way split; the same key gives the same bits, another key other bits; both branches."""
    ims = [R.images(hw, 1)[0] for hw in SIZES5]
    labels = np.array([0, 6, 3, 2, 6])
    seen = set()
    for seed in (0, 1, 4, 6):
        key = jr.PRNGKey(seed)
        kb, kf, km, ke = jr.split(key, 4)
        boxes, flips = P.random_resized_crop_boxes(kb, SIZES5), P.random_flips(kf, 5)
        partner, lam, cut, lam_t = P.mixup_cutmix_draw(km, 5, 40)
        erase = P.random_erasing_draw(ke, 5, 40, 0.5)
        seen.add(bool(cut.any()))
        for dtype in ("fp32", "bf16"):
            x, t = P.imagenet_train_mixed(ims, labels, key, 7, size=40, erase_p=0.5, label_smoothing=0.1, dtype=dtype)
            assert x.is_cuda and tuple(x.shape) == (5, 3, 40, 40) and x.dtype == P.TORCH_DT[dtype] and t.shape == (5, 7)
            cx, ct = P.crop_resize_normalize_mix(ims, boxes, 40, flips, labels, 7, partner, lam, cut, erase, lam_t, 0.1, dtype=dtype)
            x2, t2 = P.imagenet_train_mixed(ims, labels, key, 7, size=40, erase_p=0.5, label_smoothing=0.1, dtype=dtype)
            assert np.array_equal(_bits(x), _bits(cx)) and np.array_equal(_bits(x), _bits(x2))
            assert np.array_equal(np.asarray(t), np.asarray(ct)) and np.array_equal(np.asarray(t), np.asarray(t2))
        v = P.crop_resize_normalize(ims, boxes, 40, flips).cpu().numpy()
        want = M.mix(v, partner, lam, M.one_minus(lam), cut, erase)
        x, t = P.imagenet_train_mixed(ims, labels, key, 7, size=40, erase_p=0.5, label_smoothing=0.1)
        assert np.array_equal(_bits(x), want.view(np.int32))
        assert np.array_equal(np.asarray(t).view(np.int32), M.targets(labels, partner, lam_t, M.one_minus(lam_t), 7, 0.1).view(np.int32))
        other, _ = P.imagenet_train_mixed(ims, labels, jr.PRNGKey(seed + 100), 7, size=40, erase_p=0.5)
        assert not np.array_equal(_bits(x), _bits(other))
    assert seen == {False, True}, "the four keys should draw both mixup and cutmix"
    assert _lib.check_device_status() == 0


def test_inside_value_and_grad():
    """Under the tape the launch is allowed; the soft targets it returns give the loss that the same targets give after a round
    trip through numpy.  alexnet, num_classes = 7, B = 4, at 224 px: its AdaptiveAvgPool2d((6, 6)) has a backward only where the
    map already is 6 x 6, which a 64 px input (a 1 x 1 map) is not -- `filter_value_and_grad` refuses that, by design."""
    net = eqv.tree_inference(eqv.models.alexnet(num_classes=7), True)
    arr = R.images((80, 72), 4)
    labels = np.array([0, 6, 2, 2])
    keys = jr.split(jr.PRNGKey(0), 4)
    key = jr.PRNGKey(9)
    held = {}

    @eqv.filter_value_and_grad
    def inside(model, im, y):
        x, t = P.imagenet_train_mixed(im, y, key, 7, size=224, erase_p=0.5, label_smoothing=0.1)
        held["t"] = np.asarray(t).copy()
        out = eqv.vmap(model, axis_name="batch")(x, key=keys)
        return eqv.optim.softmax_cross_entropy(out, t).mean()

    @eqv.filter_value_and_grad
    def outside(model, x, t):
        out = eqv.vmap(model, axis_name="batch")(x, key=keys)
        return eqv.optim.softmax_cross_entropy(out, t).mean()

    with eqv.precision("fp32"):
        a, ga = inside(net, arr, labels)
        x, _ = P.imagenet_train_mixed(arr, labels, key, 7, size=224, erase_p=0.5, label_smoothing=0.1)
        b, gb = outside(net, x, held["t"])
    assert np.isfinite(float(a)) and float(a) == float(b)
    assert held["t"].shape == (4, 7) and np.all(np.abs(held["t"].astype(np.float64).sum(1) - 1) <= 2.0 ** -20)
    _lib.check_device_status()


# ---- eqv.optim.ema --------------------------------------------------------------------------------------------------------------

def test_ema_three_updates_bit_for_bit_in_one_launch_each():
    """Leaves of 1, 4097 and 70000 elements (one block, two, eighteen: the CHUNK boundaries of `_optim.plan`), a frozen leaf and
    a non-float leaf between them.  The first update copies; the next two are float32 numpy bit for bit; one launch per update."""
    assert _optim.plan([1, 4097, 70000]) == ([0, 1, 3], 21)
    rng = np.random.default_rng(7)
    sizes = [(1,), (4097,), (280, 250)]
    steps = [[rng.standard_normal(s).astype(np.float32) for s in sizes] for _ in range(4)]
    steps[1][0][0] = np.float32(-0.0)

    def tree(leaves, frozen=False):
        d = [DevArray(torch.from_numpy(a).cuda()) for a in leaves]
        return {"a": d[0], "n": 3, "frozen": None if frozen else d[1], "b": d[1], "c": [d[2], None]}

    e = eqv.optim.ema(0.999)
    st = e.init(tree(steps[0]))
    assert st["count"] == 0 and len(st["ema"]) == 4
    avg = [a.copy() for a in steps[0]]
    frozen0 = steps[0][1].copy()
    for k in (1, 2, 3):
        calls = []
        orig = _lib.call
        _lib.call = lambda name, *a: (calls.append(name), orig(name, *a))[1]
        try:
            st = e.update(tree(steps[k], frozen=True), st)
        finally:
            _lib.call = orig
        assert calls == ["mv_optim_step_f32"] and _lib.last_kernel() == "optim_ema_f32" and st["count"] == k
        avg = [p.copy() for p in steps[k]] if k == 1 else [M.ema(a, p, 0.999) for a, p in zip(avg, steps[k])]
        got = e.state_params(st, tree(steps[0]))
        assert got["n"] == 3 and got["c"][1] is None and all(isinstance(got[n], DevArray) for n in ("a", "b", "frozen"))
        for name, want in (("a", avg[0]), ("b", avg[1])):
            assert np.array_equal(np.asarray(got[name]).view(np.int32), want.view(np.int32)), (k, name)
        assert got["c"][0].shape == (280, 250) and np.array_equal(np.asarray(got["c"][0]).view(np.int32), avg[2].view(np.int32)), k
        assert np.array_equal(np.asarray(got["frozen"]), frozen0), "the slot of a leaf that arrives as None is left alone"
    like = tree(steps[0], frozen=True)
    assert e.state_params(st, like)["frozen"] is None
    with pytest.raises(ValueError, match="structure"):
        e.update([DevArray(torch.zeros(3, device="cuda"))], st)
    with pytest.raises(ValueError, match="decay"):
        eqv.optim.ema(1.5)
    _lib.check_device_status()
