"""CPU proofs for tests/test_strict_bwd_gpu.py: the float32 emulations of tests/_strict.py for the two conv backward contracts, the
column sum and the attention backward go through the checkers the GPU module uses, at its shapes.  The correct emulation passes the
exact-integer and the per-element instrument; each of eight defects, one switch each, fails:

    conv dgrad   the last k dropped at odd K; the upper half-wave's four k kept at K % 8 == 4 (reads past K); a tap accepted where
                 the stride does not divide
    conv wgrad   the last position of an odd P dropped; the position walk wrapping once only at Wo = 1; a chunk boundary counted twice
    colsum       the rows m >= 4 (M / 4) dropped
    mha_bwd      the keys j >= 64 dropped

The last test records why the module exists: the lost rows of a 100352 x 64 column sum pass `_cases._cmp` at colsum_case's tolerance."""
import functools

import numpy as np
import pytest

from tests import _strict as S

SHAPES = S.CONV_BWD_SHAPES
IDS = [g.tag for g in SHAPES]
BY_NOTE = {"odd_k": SHAPES[0], "k12": SHAPES[1], "asym": SHAPES[3], "wo1": SHAPES[5], "two_chunks": SHAPES[9], "clamp": SHAPES[10]}


@functools.lru_cache(maxsize=None)
def _case(i, kind):
    g = SHAPES[i]
    x, w, dy = S.conv_bwd_data(g, kind)
    return (g, x, w, dy) + S.conv_bwd_ref(x, w, dy, g)


def _of(g, kind):
    return _case(SHAPES.index(g), kind)


def _kred_dx(g):
    return g.Kg * g.R * g.S


def _splits(g):
    """The splits the GPU module's scratch regimes reach: none, the entry's own, and the clamp to two."""
    want = g.wgrad_split()[0]
    return sorted({1, want, min(want, 2)})


# ================================================================================================ the case list itself
def test_case_list_reaches_what_it_claims():
    g = SHAPES
    assert g[0].K % 2 == 1 and g[0].K % 4 and 32 < g[0].C and g[0].C % 32 and g[0].N * g[0].H * g[0].W == 99 and g[0].P % 2 == 1
    assert g[1].K % 8 == 4 and g[2].K % 4 == 2 and g[2].dh == 2
    assert g[3].R != g[3].S and g[3].sh != g[3].sw and g[3].ph != g[3].pw and g[3].C == 8 and g[4].C == 7
    assert g[5].Wo == 1 and g[5].P % 2 == 1 and 32 < g[5].Kg and g[5].Kg % 32 and g[6].Wo == 2
    assert g[7].groups == g[7].C == g[7].K and (g[8].Kg, g[8].Cg) == (5, 3)
    assert g[9].N * g[9].H * g[9].W == 132 and -(-g[9].C // 32) == 3
    # the split of the weight gradient as the entry's comment states it: only the eleventh shape wants more than two chunks
    assert [s.wgrad_split()[0] for s in g] == [1, 1, 1, 1, 1, 1, 1, 1, 1, 2, 4]
    c = S.CONV_BWD_CLAMP
    assert c.wgrad_split()[0] > 2
    assert c.wgrad_split(8 << 20) == (4, 4)
    assert c.wgrad_split(4096 + int(2.5 * c.out_elems * 4)) == (4, 2)          # the `split > fit` clamp
    assert c.wgrad_split(4096 + int(1.5 * c.out_elems * 4)) == (4, 1)          # the `fit < 2` fallback
    assert c.wgrad_split(None) == (4, 1)


# ================================================================================================ correct emulations pass
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_conv_bwd_emulation_passes_both_instruments(i):
    g, x, w, dy, dx, mx, dw, mw = _case(i, "int")
    wd, ww = S.conv_bwd_weights(x, w, dy, g)
    S.prove_exact(g.tag + "/dgrad", dx, mx, wd, out="fp32")
    S.prove_exact(g.tag + "/wgrad", dw, mw, ww, out="fp32")
    assert S.check_exact(S.emu_conv_dgrad(dy, w, g), dx)["ok"]
    for split in _splits(g):
        assert S.check_exact(S.emu_conv_wgrad(x, dy, g, split), dw)["ok"], split
    g, x, w, dy, dx, mx, dw, mw = _case(i, "gauss")
    a = S.check_bound(S.emu_conv_dgrad(dy, w, g), dx, mx, _kred_dx(g), "fp32")
    assert a["ok"], a
    for split in _splits(g):
        b = S.check_bound(S.emu_conv_wgrad(x, dy, g, split), dw, mw, g.P, "fp32")
        assert b["ok"], (split, b)


# ================================================================================================ conv dgrad defects
def _dgrad_both(g, defect):
    out = []
    for kind in ("int", "gauss"):
        _, x, w, dy, dx, mx, _, _ = _of(g, kind)
        bad = S.emu_conv_dgrad(dy, w, g, defect)
        out.append(S.check_exact(bad, dx) if kind == "int" else S.check_bound(bad, dx, mx, _kred_dx(g), "fp32"))
    return out


def test_mutant_dgrad_last_k_dropped_at_odd_k():
    e, b = _dgrad_both(BY_NOTE["odd_k"], "drop_last_odd_k")
    assert not e["ok"] and e["nbad"] > e["n"] // 2 and not b["ok"]
    # an even K has no lone last k: the shapes of _cases.py (K % 4 == 0) cannot see this defect
    e, b = _dgrad_both(BY_NOTE["k12"], "drop_last_odd_k")
    assert e["ok"] and b["ok"]


def test_mutant_dgrad_reads_past_k_at_k_mod_8_eq_4():
    e, b = _dgrad_both(BY_NOTE["k12"], "read_past_k")
    assert not e["ok"] and e["nbad"] > e["n"] // 2 and not b["ok"]
    e, b = _dgrad_both(BY_NOTE["asym"], "read_past_k")          # K = 8: the upper half-wave is in range
    assert e["ok"] and b["ok"]


def test_mutant_dgrad_tap_accepted_where_stride_does_not_divide():
    for note in ("k12", "asym"):                                 # stride 2 on both axes; stride 2 on the rows only
        e, b = _dgrad_both(BY_NOTE[note], "stride_any")
        assert not e["ok"] and not b["ok"], note
    e, b = _dgrad_both(BY_NOTE["odd_k"], "stride_any")          # stride 1: nothing to get wrong
    assert e["ok"] and b["ok"]


# ================================================================================================ conv wgrad defects
def _wgrad_both(g, split, defect):
    out = []
    for kind in ("int", "gauss"):
        _, x, w, dy, _, _, dw, mw = _of(g, kind)
        bad = S.emu_conv_wgrad(x, dy, g, split, defect)
        out.append(S.check_exact(bad, dw) if kind == "int" else S.check_bound(bad, dw, mw, g.P, "fp32"))
    return out


def test_mutant_wgrad_last_position_of_odd_p_dropped():
    for note in ("odd_k", "wo1"):                                # P = 99 and P = 9
        e, b = _wgrad_both(BY_NOTE[note], 1, "drop_last_odd_p")
        assert not e["ok"] and not b["ok"], note
    e, b = _wgrad_both(BY_NOTE["k12"], 1, "drop_last_odd_p")    # P = 40
    assert e["ok"] and b["ok"]


def test_mutant_wgrad_walk_wraps_once_at_wo_1():
    e, b = _wgrad_both(BY_NOTE["wo1"], 1, "wrap_once")
    assert not e["ok"] and not b["ok"]
    e, b = _wgrad_both(SHAPES[6], 1, "wrap_once")               # Wo = 2: a step of two wraps exactly once
    assert e["ok"] and b["ok"]


def test_mutant_wgrad_chunk_boundary_counted_twice():
    for note, split in (("two_chunks", 2), ("clamp", 4), ("clamp", 2)):
        e, b = _wgrad_both(BY_NOTE[note], split, "chunk_twice")
        assert not e["ok"] and not b["ok"], (note, split)
    e, b = _wgrad_both(BY_NOTE["clamp"], 1, "chunk_twice")      # one chunk has no boundary
    assert e["ok"] and b["ok"]


# ================================================================================================ colsum
COLSUM = [(3, 5), (515, 70), (1029, 64)]


@pytest.mark.parametrize("M,C", COLSUM, ids=[f"{m}x{c}" for m, c in COLSUM])
@pytest.mark.parametrize("product", [False, True], ids=["sum", "product"])
def test_colsum_emulation_and_lost_tail_rows(M, C, product):
    want = S.colsum_split(M)[0]
    assert (want > 1) == (M >= 512)
    for kind in ("int", "gauss"):
        rng = S.rng_of(61)
        a, b = ((S.int_tensor(rng, (M, C), 2) if kind == "int" else rng.standard_normal((M, C)).astype(np.float32)) for _ in range(2))
        b = b if product else None
        ref, mag = S.colsum_ref(a, b)
        for split in sorted({1, want}):
            n_ops = S.colsum_n_ops(M, split)
            good, bad = S.emu_colsum(a, b, split), S.emu_colsum(a, b, split, drop_tail_rows=True)
            lost = M % 4 or any((min((c + 1) * -(-M // split), M) - c * -(-M // split)) % 4 for c in range(split))
            assert lost, "every case of the list has rows behind the last whole group of four"
            if kind == "int":
                S.prove_exact(f"colsum/{M}x{C}", ref, mag, [a.T] + ([b.T] if product else []), out="fp32")
                assert S.check_exact(good, ref)["ok"] and not S.check_exact(bad, ref)["ok"]
            else:
                assert S.check_bound(good, ref, mag, 0, "fp32", n_ops=n_ops)["ok"]
                assert not S.check_bound(bad, ref, mag, 0, "fp32", n_ops=n_ops)["ok"]


def test_colsum_lost_rows_pass_the_old_criterion():
    """colsum_case(100352, 64) allows 2e-5 sqrt(M) max(1, max|ref|): about 5 on its Gaussian data, more than one whole row can
    move a column sum by.  M is a multiple of four there, so the tail switch of the emulation loses nothing; the defect shown is the
    matrix's last row lost (a loop bound one short).  On Gaussian data and on integers in [-2, 2] it passes the old criterion; on
    the integers it fails check_exact."""
    from tests._cases import _cmp
    M, C = 100352, 64
    tol = 2e-5 * np.sqrt(M)
    rng = S.rng_of(62)
    for kind in ("gauss", "int"):
        a = rng.standard_normal((M, C)).astype(np.float32) if kind == "gauss" else S.int_tensor(rng, (M, C), 2)
        ref, mag = S.colsum_ref(a, None)
        bad = S.emu_colsum(a[:M - 1], None, 1)
        old = _cmp(bad, ref, tol)
        print(f"colsum {kind}: the lost row moves a sum by {old['err']:.3f}, the old criterion allows {old['lim']:.3f}")
        assert old["ok"] and old["err"] >= 1.0
        if kind == "int":
            assert not S.check_exact(bad, ref)["ok"]
            assert S.check_exact(S.emu_colsum(a, None, 1), ref)["ok"]
        else:           # 25091 roundings of sum |a| allow more than a row as well: why the GPU module's column sums are short
            assert S.check_bound(bad, ref, mag, 0, "fp32", n_ops=S.colsum_n_ops(M, 1))["ok"]
            short = S.emu_colsum(a[:1028], None, 1)
            assert not S.check_bound(short, *S.colsum_ref(a[:1029], None), 0, "fp32", n_ops=S.colsum_n_ops(1029, 1))["ok"]


# ================================================================================================ mha_bwd
MHA = [(2, 65, 2, 8), (1, 5, 3, 72), (1, 64, 1, 16)]


def _mha_scaled(r):
    """dS is a multiple of 2^-8 (scale 1/4, two factors of 1/8): the exact-integer preconditions are checked on 2^8 times the values."""
    return [np.asarray(v, np.float64) * 256.0 for v in r[:2]]


@pytest.mark.parametrize("B,N,H,dh", MHA, ids=[f"B{b}_N{n}_H{h}_dh{d}" for b, n, h, d in MHA])
def test_mha_bwd_emulation_and_lost_key_tail(B, N, H, dh):
    for kind in ("int", "gauss"):
        qkv, probs, dout = S.mha_bwd_data(B, N, H, dh, kind)
        scale = 0.25 if kind == "int" else dh ** -0.5
        r = S.mha_bwd_ref(qkv, probs, dout, scale, H, dh)
        ds, dq = S.emu_mha_bwd(qkv, probs, dout, scale, H, dh)
        ds_bad, dq_bad = S.emu_mha_bwd(qkv, probs, dout, scale, H, dh, drop_j_tail=True)
        if kind == "int":
            for key in ("ds", "dqkv"):
                S.prove_exact(f"mha_bwd/{key}", *_mha_scaled(r[key]), [qkv.reshape(B * N, -1).T], out="fp32")
            assert S.check_exact(ds, r["ds"][0])["ok"] and S.check_exact(dq, r["dqkv"][0])["ok"]
            seen = not S.check_exact(ds_bad, r["ds"][0])["ok"], not S.check_exact(dq_bad, r["dqkv"][0])["ok"]
        else:
            a = S.check_bound(ds, *r["ds"][:2], 0, "fp32", n_ops=r["ds"][2])
            b = S.check_bound(dq, *r["dqkv"][:2], 0, "fp32", n_ops=r["dqkv"][2])
            assert a["ok"] and b["ok"], (a, b)
            seen = (not S.check_bound(ds_bad, *r["ds"][:2], 0, "fp32", n_ops=r["ds"][2])["ok"],
                    not S.check_bound(dq_bad, *r["dqkv"][:2], 0, "fp32", n_ops=r["dqkv"][2])["ok"])
        assert seen == ((True, True) if N > 64 else (False, False)), (kind, seen)          # only N = 65 has a second trip


# ================================================================================================ the other references
def test_references_agree_with_autograd_and_definitions():
    """The hand-written float64 references against torch.autograd in double, where one exists."""
    import torch
    rng = S.rng_of(63)
    x = S.act_input(rng, 1031, "fp32")
    for act, fn in (("relu", torch.relu), ("gelu_tanh", lambda t: torch.nn.functional.gelu(t, approximate="tanh")),
                    ("hard_swish", torch.nn.functional.hardswish), ("hard_sigmoid", torch.nn.functional.hardsigmoid),
                    ("sigmoid", torch.sigmoid), ("silu", torch.nn.functional.silu)):
        t = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
        fn(t).sum().backward()
        corner = np.isin(x, (-3.0, 0.0, 3.0)) & (act in ("relu", "hard_swish", "hard_sigmoid"))
        assert np.allclose(S.act_grad64(x, act)[~corner], t.grad.numpy()[~corner], rtol=1e-6, atol=1e-14), act          # torch's 1/6 is a float
    assert S.act_grad64(np.array([-3.0, 3.0]), "hard_swish").tolist() == [0.0, 1.0]
    assert S.act_grad64(np.array([-3.0, 0.0, 3.0]), "hard_sigmoid").tolist() == [0.0, 1.0 / 6.0, 0.0]
    assert S.act_grad64(np.array([0.0]), "relu").tolist() == [0.0]
    xs, gam, dy = rng.standard_normal((5, 33)), rng.uniform(0.5, 1.5, 33), rng.standard_normal((5, 33))
    t = torch.from_numpy(xs).requires_grad_(True)
    torch.nn.functional.layer_norm(t, (33,), torch.from_numpy(gam), None, 1e-5).backward(torch.from_numpy(dy))
    assert np.allclose(S.layernorm_bwd64(xs, gam, dy, 1e-5)[0], t.grad.numpy(), rtol=1e-10, atol=1e-12)
    lg, lab = 3 * rng.standard_normal((7, 10)), rng.integers(0, 10, 7)
    t = torch.from_numpy(lg).requires_grad_(True)
    loss = torch.nn.functional.cross_entropy(t, torch.from_numpy(lab))
    loss.backward()
    rows, mean, dl = S.xent64(lg, np.eye(10)[lab])
    assert abs(mean - float(loss.detach())) < 1e-12 and np.allclose(dl, t.grad.numpy(), rtol=1e-10, atol=1e-14)
    dyp = rng.standard_normal((2, 3, 4, 24))
    t = torch.from_numpy(rng.standard_normal((2, 5, 7, 6))).requires_grad_(True)
    tp = torch.nn.functional.pad(t, (0, 0, 0, 1, 0, 1))
    torch.cat([tp[:, 0::2, 0::2], tp[:, 1::2, 0::2], tp[:, 0::2, 1::2], tp[:, 1::2, 1::2]], -1).backward(torch.from_numpy(dyp))
    assert np.array_equal(S.patch_merge_bwd_ref(dyp, 5, 7), t.grad.numpy())
