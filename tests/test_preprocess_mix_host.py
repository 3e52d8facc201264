"""CPU: the host half of mixup / cutmix / random erasing / soft targets in `eqxvision_amd.preprocess` -- the two draw functions
against the independent restatement of tests/_mix_ref.py and against their distributions, every refusal of the core (Python and
the C entry, both before any device call), the record against the header's struct, and `_mix_ref` itself against a float64
formulation."""
import os
import re

import numpy as np
import pytest

from eqxvision_amd import _act, _lib
from eqxvision_amd import preprocess as P
from eqxvision_amd import random as jr
from tests import _mix_ref as M

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "eqxvision_amd.h")
N_KEYS = 2000


@pytest.fixture
def no_launch(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a refused call reached the library or the device")
    monkeypatch.setattr(_lib, "call", refuse)
    monkeypatch.setattr(P, "device", refuse)


# ---- draws --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hw", [(24, 40), (224, 224)])
def test_mix_draw_is_the_restatement_and_respects_its_invariants(hw):
    H, W = hw
    seen = set()
    for seed in range(200):
        key = jr.PRNGKey(seed)
        partner, lam, cut, lam_t = P.mixup_cutmix_draw(key, 5, hw)
        again = P.mixup_cutmix_draw(key, 5, hw)
        assert all(np.array_equal(a, b) for a, b in zip((partner, lam, cut, lam_t), again))
        assert partner.dtype == np.int32 and lam.dtype == np.float32 and cut.dtype == np.int32 and lam_t.dtype == np.float32
        assert partner.tolist() == [4, 0, 1, 2, 3] == np.roll(np.arange(5), 1).tolist()
        branch, rp, rlam, rrect, rlam_t = M.mixup_cutmix_draw(key, 5, hw)
        seen.add(branch)
        assert np.array_equal(partner, rp) and np.all(lam == np.float32(rlam)) and np.all(lam_t == np.float32(rlam_t))
        assert np.all(cut == np.asarray(rrect))
        y0, x0, y1, x1 = (int(v) for v in cut[0])
        if branch == "cutmix":
            assert 0 <= y0 <= y1 <= H and 0 <= x0 <= x1 <= W and np.all(lam == 1.0)
            assert np.all(lam_t == np.float32(1.0 - (y1 - y0) * (x1 - x0) / (H * W)))
        else:
            assert (y0, x0, y1, x1) == (0, 0, 0, 0) and np.array_equal(lam_t, lam) and 0.0 <= lam[0] <= 1.0
    assert seen == {"mixup", "cutmix"}


def test_mix_draw_frequencies():
    """Over 2000 keys: the branch is cutmix with probability switch_p (binomial, 4 sigma); the mean of lam ~ Beta(0.2, 0.2), drawn
    with cutmix disabled, is 0.5 within 4 sigma, var = a b / ((a + b)^2 (a + b + 1)) = 0.04 / (0.16 x 1.4)."""
    for switch_p in (0.5, 0.2):
        n_cut = 0
        for s in range(N_KEYS):
            branch, _, rlam, rrect, rlam_t = M.mixup_cutmix_draw(jr.PRNGKey(s), 4, (32, 32), switch_p=switch_p)
            _, lam, cut, lam_t = P.mixup_cutmix_draw(jr.PRNGKey(s), 4, 32, switch_p=switch_p)
            assert lam[0] == np.float32(rlam) and lam_t[0] == np.float32(rlam_t) and cut[0].tolist() == list(rrect)
            n_cut += branch == "cutmix"
        sigma = np.sqrt(switch_p * (1 - switch_p) / N_KEYS)
        print(f"switch_p {switch_p}: cutmix {n_cut / N_KEYS:.4f}, 4 sigma {4 * sigma:.4f}")
        assert abs(n_cut / N_KEYS - switch_p) <= 4 * sigma
    lams = np.array([P.mixup_cutmix_draw(jr.PRNGKey(s), 4, 32, cutmix_alpha=0.0)[1][0] for s in range(N_KEYS)], np.float64)
    sigma = np.sqrt(0.04 / (0.16 * 1.4) / N_KEYS)
    print(f"mean lam {lams.mean():.4f}, 4 sigma {4 * sigma:.4f}")
    assert abs(lams.mean() - 0.5) <= 4 * sigma


def test_mix_draw_noops():
    for kw in (dict(mixup_alpha=0.0, cutmix_alpha=0.0), dict(mixup_alpha=-1.0, cutmix_alpha=0.0)):
        partner, lam, cut, lam_t = P.mixup_cutmix_draw(jr.PRNGKey(3), 6, 32, **kw)
        assert partner.tolist() == list(range(6)) and np.all(lam == 1) and np.all(lam_t == 1) and not cut.any()
    partner, lam, cut, lam_t = P.mixup_cutmix_draw(jr.PRNGKey(3), 1, 32)
    assert partner.tolist() == [0] and lam.tolist() == [1.0] and lam_t.tolist() == [1.0] and not cut.any()
    for s in range(50):                                       # one branch disabled: always the other
        assert np.all(P.mixup_cutmix_draw(jr.PRNGKey(s), 4, 32, mixup_alpha=0.0)[1] == 1.0)
        assert not P.mixup_cutmix_draw(jr.PRNGKey(s), 4, 32, cutmix_alpha=0.0)[2].any()


@pytest.mark.parametrize("hw", [(24, 40), (224, 224)])
def test_erasing_draw(hw):
    """== the restatement; h < H and w < W; area and aspect inside their ranges once the rounding of h and w (half a pixel each way)
    is allowed for; the fraction of erased images within 4 sigma of p."""
    H, W = hw
    s0, s1, r0, r1 = 0.02, 0.33, 0.3, 3.3
    B, n_keys, p = 20, 100, 0.5
    n_erased = 0
    for seed in range(n_keys):
        key = jr.PRNGKey(seed)
        rects = P.random_erasing_draw(key, B, hw, p)
        assert rects.dtype == np.int32 and rects.shape == (B, 4)
        assert np.array_equal(rects, P.random_erasing_draw(key, B, hw, p)) and np.array_equal(rects, M.random_erasing_draw(key, B, hw, p))
        for y0, x0, y1, x1 in rects.tolist():
            h, w = y1 - y0, x1 - x0
            if (y0, x0, y1, x1) == (0, 0, 0, 0):
                continue
            n_erased += 1
            assert 0 <= y0 and 0 <= x0 and y1 <= H and x1 <= W and 0 <= h < H and 0 <= w < W
            assert max(h - 0.5, 0) * max(w - 0.5, 0) <= s1 * H * W and (h + 0.5) * (w + 0.5) >= s0 * H * W
            assert max(h - 0.5, 0) / (w + 0.5) <= r1 and (w <= 0.5 or (h + 0.5) / (w - 0.5) >= r0)
    n = B * n_keys
    sigma = np.sqrt(p * (1 - p) / n)
    print(f"{hw}: erased {n_erased / n:.4f}, 4 sigma {4 * sigma:.4f}")
    assert abs(n_erased / n - p) <= 4 * sigma                # at these sizes an attempt fits almost surely: ten misses are < 1e-6
    assert not P.random_erasing_draw(jr.PRNGKey(0), B, hw, 0.0).any()
    assert np.count_nonzero(P.random_erasing_draw(jr.PRNGKey(0), B, hw, 1.0).any(axis=1)) == B


# ---- records and refusals -------------------------------------------------------------------------------------------------------

def test_record_is_the_headers_struct():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    body = re.search(r"typedef struct mv_preprocess_mix \{(.*?)\} mv_preprocess_mix;", src, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), {"int32_t": "<i4", "float": "<f4"}[ctype]) for n in names.split(",")]
    assert fields == [(n, P.MIX[n].str) for n in P.MIX.names]
    assert P.MIX.itemsize == 4 * len(fields) == 52
    assert [P.MIX.fields[n][1] for n in P.MIX.names] == list(range(0, 52, 4))
    assert "52 bytes, no padding" in open(HDR).read()


def test_mix_plan_fills_the_record():
    rec = P.mix_plan(3, (24, 40), [2, 0, 1], [0.25, 1.0, 0.0], [(0, 0, 0, 0), (1, 2, 24, 40), (0, 0, 0, 0)],
                     [(3, 4, 5, 6), (0, 0, 0, 0), (0, 0, 24, 40)], [0.25, 0.5, 0.0])
    assert rec["partner"].tolist() == [2, 0, 1] and rec["lam"].tolist() == [0.25, 1.0, 0.0] and rec["oml"].tolist() == [0.75, 0.0, 1.0]
    assert rec["lam_t"].tolist() == [0.25, 0.5, 0.0] and rec["oml_t"].tolist() == [0.75, 0.5, 1.0]
    assert [rec[n][1] for n in ("cy0", "cx0", "cy1", "cx1")] == [1, 2, 24, 40] and [rec[n][0] for n in ("ey0", "ex0", "ey1", "ex1")] == [3, 4, 5, 6]
    lam = np.float32(0.7309)
    rec = P.mix_plan(2, 8, [1, 0], [lam, lam])
    assert rec["oml"][0] == np.float32(1.0 - np.float64(lam)) == M.one_minus(lam) and rec["lam_t"][0] == lam
    none = P.mix_plan(2, 8)
    assert none["partner"].tolist() == [0, 1] and none["lam"].tolist() == [1, 1] and none["oml_t"].tolist() == [0, 0]


def test_every_refusal_of_the_core_names_the_image_before_any_call(no_launch):
    ims = [np.zeros((40, 30, 3), np.uint8), np.zeros((30, 40, 3), np.uint8)]
    full = [(0, 0, 40, 30), (0, 0, 30, 40)]

    def core(**kw):
        args = dict(flip=None, labels=[0, 6], num_classes=7, partner=[1, 0], lam=[0.5, 0.5])
        args.update(kw)
        return P.crop_resize_normalize_mix(ims, full, (16, 24), **args)

    for kw, word in ((dict(partner=[1, 2]), r"image 1: partner 2 does not lie in \[0, 2\)"),
                     (dict(partner=[-1, 0]), r"image 0: partner -1 does not lie"),
                     (dict(cut=[(0, 0, 16, 24), (0, 0, 17, 24)]), r"image 1: cut rectangle \(0, 0, 17, 24\) does not lie inside the output 16x24"),
                     (dict(erase=[(0, -1, 4, 4), (0, 0, 0, 0)]), r"image 0: erase rectangle \(0, -1, 4, 4\) does not lie inside"),
                     (dict(erase=[(0, 0, 4, 25), (0, 0, 0, 0)]), r"image 0: erase rectangle"),
                     (dict(lam=[0.5, 1.5]), r"image 1: lam = 1.5 must be finite and lie in \[0, 1\]"),
                     (dict(lam=[-0.1, 0.5]), r"image 0: lam = -0.1"),
                     (dict(lam=[np.nan, 0.5]), r"image 0: lam = nan"),
                     (dict(lam_t=[0.5, 2.0]), r"image 1: lam_t = 2.0"),
                     (dict(labels=[0, 7]), r"image 1: label 7 does not lie in \[0, 7\)"),
                     (dict(labels=[-1, 3]), r"image 0: label -1 does not lie"),
                     (dict(labels=[0.5, 1.0]), "labels must be integers"),
                     (dict(labels=[0, 1, 2]), "one label per image"),
                     (dict(num_classes=None), "num_classes"),
                     (dict(label_smoothing=1.0), "label_smoothing"),
                     (dict(partner=[1]), "partner must be integers"),
                     (dict(cut=[(0, 0, 1, 1)]), "cut must be integers")):
        with pytest.raises(ValueError, match=word):
            core(**kw)
    with pytest.raises(ValueError, match="image 1.*does not lie inside the image"):
        P.crop_resize_normalize_mix(ims, [full[0], (0, 0, 31, 40)], 16)
    with pytest.raises(ValueError, match="single image has no partner"):
        P.crop_resize_normalize_mix(ims[0], full[0], 16, partner=[1])
    with pytest.raises(ValueError, match="single image has no partner"):
        P.imagenet_train_mixed(ims[0], [0], jr.PRNGKey(0), 7, size=16)
    with _act.keep_alive([]):
        with pytest.raises(ValueError, match="filter_jit"):
            core()
        with pytest.raises(ValueError, match="filter_jit"):
            P.imagenet_train_mixed(ims, [0, 1], jr.PRNGKey(0), 7, size=16)


def test_entry_validates_the_host_records_before_any_device_call(built_lib):
    """`mv_preprocess_u8_mix_fwd` checks the host copies before it touches the device: made-up (never dereferenced) device
    addresses, real host arrays.  Each message names the image."""
    rec, (hout, wout) = P.boxes_plan([(40, 30), (400, 44)], [(1, 2, 20, 24), (0, 4, 300, 40)], [False, True], (32, 24))
    mix = P.mix_plan(2, (32, 24), [1, 0], [0.5, 1.0], [(0, 0, 0, 0), (2, 3, 32, 24)], [(0, 0, 5, 5), (0, 0, 0, 0)], [0.5, 0.25])
    labels = np.array([0, 6], np.int32)
    x_bytes, X, Y, T, DEV = 40 * 30 * 3 + 400 * 44 * 3, 1 << 20, 2 << 20, 3 << 20, 5 << 20

    def call(r=rec, m=mix, lab=labels, y=Y, t=T, lab_dev=DEV, K=7):
        r, m = np.ascontiguousarray(r), np.ascontiguousarray(m)
        rc = built_lib.mv_preprocess_u8_mix_fwd(X, x_bytes, y, r.ctypes.data, DEV, m.ctypes.data, DEV, DEV, DEV,
                                                None if lab is None else lab.ctypes.data, lab_dev, t, K, 1.0, 0.0, 2, hout, wout, 0,
                                                _lib.F32, 0, None)
        return rc, built_lib.mv_last_error()

    def changed(a, i, **kw):
        a = a.copy()
        for k, v in kw.items():
            a[k][i] = v
        return a

    invalid, unsupported = -1, -2
    for kw, rc_want, word in ((dict(m=changed(mix, 1, partner=2)), invalid, b"image 1: partner 2 does not lie in [0, 2)"),
                              (dict(m=changed(mix, 0, partner=-1)), invalid, b"image 0: partner -1"),
                              (dict(m=changed(mix, 1, cy1=33)), invalid, b"image 1: cut rectangle (2, 3, 33, 24) does not lie inside the output 32x24"),
                              (dict(m=changed(mix, 0, ex0=-1)), invalid, b"image 0: erase rectangle (0, -1, 5, 5)"),
                              (dict(m=changed(mix, 0, lam=1.5)), invalid, b"image 0: lam 1.5"),
                              (dict(m=changed(mix, 1, oml=np.nan)), invalid, b"image 1: lam 1, oml nan"),
                              (dict(m=changed(mix, 1, lam_t=-0.25)), invalid, b"image 1"),
                              (dict(m=changed(mix, 0, oml_t=np.inf)), invalid, b"image 0"),
                              (dict(lab=np.array([0, 7], np.int32)), invalid, b"image 1: label 7 does not lie in [0, 7)"),
                              (dict(lab=np.array([-1, 0], np.int32)), invalid, b"image 0: label -1"),
                              (dict(r=changed(rec, 1, top=101)), invalid, b"image 1: box 300x40 at (101, 4)"),
                              (dict(r=changed(rec, 1, h=400, top=0)), unsupported, b"image 1: box 400x40 -> 32x24 needs up to 26 x 4 taps"),
                              (dict(t=None), invalid, b"labels without targets"),
                              (dict(lab=None, lab_dev=None), invalid, b"targets without labels"),
                              (dict(K=0), invalid, b"0 classes"),
                              (dict(y=X + 100), unsupported, b"images and output overlap"),
                              (dict(t=X + 100), unsupported, b"images and targets overlap"),
                              (dict(t=Y + 8), unsupported, b"output and targets overlap")):
        rc, msg = call(**kw)
        assert rc == rc_want and word in msg, (rc, msg, word)


# ---- the reference against float64 ----------------------------------------------------------------------------------------------

def test_mix_ref_against_float64():
    """fl32(lam v_i) is the one rounding of a product that float64 holds exactly (24 + 24 bits).  Where float64 also holds the sum
    of the two rounded products exactly, one rounding of it is the reference bit for bit; elsewhere (the float64 sum was itself
    rounded: double rounding) the two differ by at most one fp32 ulp."""
    rng = np.random.default_rng(0)
    v = (rng.standard_normal((4, 3, 9, 11)) * np.exp(rng.uniform(-12, 12, (4, 3, 9, 11)))).astype(np.float32)
    partner = np.array([3, 0, 1, 2])
    for lam in (np.float32(0.25), np.float32(0.7309), np.float32(0.0), np.float32(1e-7)):
        lams, omls = np.full(4, lam), np.full(4, M.one_minus(lam))
        got = M.mix(v, partner, lams, omls, np.zeros((4, 4), int), np.zeros((4, 4), int))
        p1 = (np.float64(lam) * v.astype(np.float64)).astype(np.float32).astype(np.float64)
        p2 = (np.float64(omls[0]) * v[partner].astype(np.float64)).astype(np.float32).astype(np.float64)
        s = p1 + p2
        exact = ((s - p1) == p2) & ((s - p2) == p1)
        want = s.astype(np.float32)
        assert exact.mean() > 0.5
        assert np.array_equal(got[exact].view(np.int32), want[exact].view(np.int32))
        assert np.all(np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want)))
    # erase, then cut, then the targets on a hand-made case
    v = np.arange(2 * 3 * 4 * 4, dtype=np.float32).reshape(2, 3, 4, 4) + 1
    out = M.mix(v, [1, 0], [0.5, 1.0], [0.5, 0.0], [(0, 0, 2, 2), (0, 0, 0, 0)], [(0, 0, 0, 0), (1, 1, 4, 4)])
    assert np.array_equal(out[0, :, :2, :2], v[1, :, :2, :2] * np.array([[1, 1], [1, 0]], np.float32))      # the partner, erased at (1, 1)
    assert np.array_equal(out[0, :, 2:, 2:], 0.5 * v[0, :, 2:, 2:]) and np.array_equal(out[1, :, 0, :], v[1, :, 0, :])
    assert not out[1, :, 1:, 1:].any()
    t = M.targets([0, 6], [1, 0], [0.25, 1.0], [0.75, 0.0], 7, 0.0)
    assert t[0].tolist() == [0.25, 0, 0, 0, 0, 0, 0.75] and t[1].tolist() == [0, 0, 0, 0, 0, 0, 1.0]
    assert M.bf16_bits(np.array([1.0, 1.00390625, 1.01171875, -2.0], np.float32)).tolist() == [0x3F80, 0x3F80, 0x3F82, 0xC000]
