"""_post_cases.py checked on its own, without a GPU: the restatements against torch on the CPU, the data against the conditions
the derivations need, every bound against a plain fp32 emulation of the kernel's arithmetic (sequential sums, K rounded to bf16
where the kernel rounds it) -- and, so that the suite is known to be able to fail, a list of wrong variants of the emulation,
each of which must leave at least one element outside TWICE the bound in every case that reaches the affected path."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _post_cases as pc


def _ids(cases):
    return [c["id"] for c in cases]


def _inside(what, got, ref, bound):
    r, at = pc.worst_ratio(got, ref, bound)
    assert r <= 1.0, "%s: the fp32 emulation is at %.3f of the bound at %s" % (what, r, at)


def _outside(what, got, ref, bound):
    assert pc.fraction_outside(got, ref, bound, 2.0) > 0, "%s: the wrong variant stays inside twice the bound everywhere" % what


# ============================================================================================================ part A
def test_bilateral_tables_and_data():
    assert sorted({c["reach"] for c in pc.BILATERAL_CASES}) == pc.BILATERAL_INSTANTIATIONS
    assert {c["N"] for c in pc.BILATERAL_CASES if c["Cp"] in (32, 64)} >= {1, 63, 64, 65, 135, 273}
    assert any(c["ldq"] == (c["N"] + 63) // 64 * 64 + 64 for c in pc.BILATERAL_CASES) and any(c["signed"] for c in pc.BILATERAL_CASES)
    for c in pc.BILATERAL_CASES:
        q = pc.bilateral_qn(c["Cp"], c["N"], c["signed"])
        assert pc.is_bf16(q) and not q[c["C"]:].any() and q[:c["C"]].any(1).all() and (q.min() < 0) == c["signed"]
        assert c["H"] * c["W"] == c["N"] and (c["H"] != c["W"] or c["N"] == 1)
        d2 = pc._bilateral_k64(c["N"])[1]
        assert d2.max() <= 90.0
        if c["N"] > 64:     # the colour term neither vanishes nor kills everything
            assert (d2 < 2).mean() > 0.1 and (d2 > 8).mean() > 0.1


@pytest.mark.parametrize("case", pc.BILATERAL_CASES, ids=_ids(pc.BILATERAL_CASES))
def test_bilateral_bound_and_wrong_variants(case):
    key = (case["Cp"], case["N"], case["signed"])
    ref, bound = pc.bilateral_ref(*key)
    _inside("bilateral " + case["id"], pc.bilateral_emul(*key), ref, bound)
    assert not ref[case["C"]:].any()
    if case["N"] % 64:
        _outside("last ragged j tile left out, " + case["id"], pc.bilateral_emul(*key, wrong="tile"), ref, bound)
    if case["N"] > 1:
        _outside("gx and gy swapped, " + case["id"], pc.bilateral_emul(*key, wrong="swap"), ref, bound)
    if case["Cp"] >= 64:
        _outside("class rows 0..31 and 32..63 exchanged, " + case["id"], pc.bilateral_emul(*key, wrong="rows"), ref, bound)


def test_spatial_data_is_exact():
    assert all((c["C"] * c["H"] * c["W"]) % 256 for c in pc.SPATIAL_CASES)
    for c in pc.SPATIAL_CASES:
        s = pc.spatial_case(c["R"], c["H"], c["W"], c["C"])
        assert np.abs(s["q"]).max() <= 8 and np.array_equal(s["g"], 2.0 ** -np.arange(c["R"] + 1))
        assert np.array_equal(np.round(s["ref"] * 1024), s["ref"] * 1024) and np.abs(s["ref"]).max() < 2048      # 21 bits
    # the (3, 4) window of radius 5 overhangs every side at once: every output is the full weighted sum
    s = pc.spatial_case(5, 3, 4, 1)
    g, q = s["g"].astype(np.float64), s["q"].reshape(3, 4).astype(np.float64)
    gy = np.array([[g[abs(a - b)] for b in range(3)] for a in range(3)])
    gx = np.array([[g[abs(a - b)] for b in range(4)] for a in range(4)])
    assert np.array_equal((gy @ q @ gx.T).reshape(-1), s["ref"][0])


@pytest.mark.parametrize("case", pc.UPDATE_CASES, ids=_ids(pc.UPDATE_CASES))
def test_update_bound(case):
    prob = pc.update_inputs(case["C"], case["N"])[0]
    if prob.size >= len(pc.PROB_SPECIALS):
        assert np.array_equal(prob.reshape(-1)[:5], np.array(pc.PROB_SPECIALS, dtype=np.float32))
    ref = pc.update_ref(case)
    assert np.allclose(ref["Q"].sum(0), 1.0, atol=1e-12)
    for name, got in zip(("Q", "qpos", "qbi"), pc.update_emul(case)):
        _inside("update %s %s" % (case["id"], name), got, ref[name], ref[name + "_b"])
    # a class row that takes its neighbour's message is seen
    if case["msg"] and case["C"] > 1:
        Q = pc.update_emul(case)[0]
        _outside("update, rows rolled " + case["id"], np.roll(Q, 1, axis=0), ref["Q"], ref["Q_b"])


def test_norm_bound():
    k1, ref, bound = pc.norm_case()
    assert (k1 == 0).sum() == 3 and ref[0] == pytest.approx(1e10, rel=1e-6)
    _inside("norm", pc.norm_emul(k1), ref, bound)


@pytest.mark.parametrize("case", pc.CRF_CASES, ids=_ids(pc.CRF_CASES))
def test_crf_cases_are_decided(case):
    """at most MARGIN_CAP of the pixels have an oracle top-2 gap below twice the value tolerance"""
    import crf_ref
    image, probs = pc.crf_inputs(case["h"], case["w"], case["c"], case["seed"])
    assert (case["h"] * case["w"]) % 64 and (case["c"] + 31) // 32 in (2, 5)
    want = crf_ref.rgb_dense_crf_exact(np.array(image), np.array(probs), max_iter=case["iters"]).double()
    top2 = want.topk(2, dim=0).values
    share = ((top2[0] - top2[1]) < pc.CRF_GAP).double().mean().item()
    changed = (want.argmax(0) != torch.from_numpy(np.array(probs)).argmax(0)).double().mean().item()
    print("%s: %.2f %% of the pixels undecided, the CRF changes %.1f %% of the labels" % (case["id"], 100 * share, 100 * changed))
    assert share <= pc.MARGIN_CAP and pc.CRF_GAP == 2 * pc.CRF_TOL
    assert changed > 0.05                       # the pairwise terms matter on this fixture


# ============================================================================================================ part B
@pytest.mark.parametrize("sn,dn", pc.INTERP_PAIRS)
def test_taps_restatement_against_interpolate(sn, dn):
    x = torch.from_numpy(np.random.default_rng(sn * 100 + dn).standard_normal((3, sn)))
    want = F.interpolate(x.view(1, 3, sn, 1), size=(dn, 1), mode="bilinear", align_corners=False).view(3, dn).numpy()
    assert np.allclose(x.numpy() @ pc.interp_matrix(dn, sn).T, want, rtol=0, atol=1e-13)
    for fma in (False, True):                   # the fp32 taps: the same or the neighbouring cell, the position within 4 u max(1, src)
        i0, i1, w1 = pc.taps1d_f32(dn, sn, fma)
        src = pc.taps1d(dn, sn)[3]
        assert (np.abs((i0 + w1.astype(np.float64)) - src) <= 4 * pc.U * np.maximum(1.0, src)).all()


@pytest.mark.parametrize("src,dst", pc.GRIDS + (((65, 65), (2, 2)), ((4, 4), (46, 46)), ((8, 8), (12, 6))))
def test_interp2d_against_interpolate(src, dst):
    x = torch.from_numpy(np.random.default_rng(7).standard_normal((2,) + src))
    want = F.interpolate(x[None], size=dst, mode="bilinear", align_corners=False)[0].reshape(2, -1).numpy()
    assert np.allclose(x.reshape(2, -1).numpy() @ pc.interp2d(dst[0], dst[1], src[0], src[1])[0].T, want, rtol=0, atol=1e-13)


@pytest.mark.parametrize("case", pc.ROWS_CASES, ids=_ids(pc.ROWS_CASES))
def test_rows_bound_and_wrong_variant(case):
    ref, bound = pc.rows_ref(case)
    assert pc.is_bf16(pc.rows_grid(case))
    for fma in (False, True):
        got = pc.rows_emul(case, fma)
        _inside("resize_rows %s fma %s" % (case["id"], fma), got, ref, bound)
        if case["exact"]:
            assert pc.is_bf16(ref) and np.array_equal(got.astype(np.float64), ref), case["id"]
    _outside("src_off ignored, " + case["id"], pc.rows_emul(case, use_off=False), ref, bound)


def test_rows_and_bias_tables_cover_the_issue():
    assert {(c["oh"], c["ow"], c["h"], c["w"]) for c in pc.ROWS_CASES} == {s + d for s, d in pc.GRIDS}
    assert {c["C"] for c in pc.ROWS_CASES} == {8, 264, 768} and any(c["ld_src"] > c["C"] for c in pc.ROWS_CASES)
    grids = {(c["oh"], c["ow"], c["h"], c["w"]) for c in pc.BIAS_CASES}
    assert grids >= {s + d for s, d in pc.GRIDS} | {(65, 65, 2, 2), (4, 4, 46, 46)}
    assert {c["H"] for c in pc.BIAS_CASES} == {1, 3} and {c["Lt"] for c in pc.BIAS_CASES} == {0, 1, 5}
    assert {(c["tails"], c["causal"], c["pad"]) for c in pc.BIAS_CASES if c["Lt"]} >= {(a, b, d) for a in (False, True) for b in (False, True) for d in (True,)}
    assert (2 * 65 - 1) ** 2 * 4 == 66564 > 64 * 1024 and (2 * 101 - 1) ** 2 * 4 == 161604
    assert 46 * 46 > pc.BIAS_LOOP_EDGE == 8 * 256


@pytest.mark.parametrize("case", pc.BIAS_CASES, ids=_ids(pc.BIAS_CASES))
def test_bias_bound_and_wrong_variants(case):
    from ifseg_amd.models.segofa import resized
    P, Lt, T = case["h"] * case["w"], case["Lt"], case["h"] * case["w"] + case["Lt"]
    big = T > 1024
    heads = [0] if big else None
    ref, bound = pc.bias_ref(case)
    hidden = np.isinf(ref)
    if case["causal"]:
        assert (hidden == pc.causal_hidden(P, Lt)[None]).all()
        if Lt == 1:
            assert np.array_equal(pc.causal_hidden(P, 1), resized.causal_mask(P, torch.device("cpu")).numpy())
    else:
        assert not hidden.any()
    fin = np.where(hidden, 0.0, ref)

    def cmp(got):
        assert np.array_equal(np.isneginf(got), hidden)
        return np.where(hidden, 0.0, got)

    for fma in ((False,) if big else (False, True)):
        got = cmp(pc.bias_emul(case, fma, heads=heads))
        _inside("resized_rel_bias %s fma %s" % (case["id"], fma), got, fin, bound)
        assert np.array_equal(got[:, :P, P:], fin[:, :P, P:]) and np.array_equal(got[:, P:], fin[:, P:])       # the tails are copies
        if case["exact"]:
            assert np.array_equal(got.astype(np.float64), fin), case["id"]
    vis = ~hidden
    if P > 1 and case["oh"] * case["ow"] > 1 and vis[:, :P, :P].sum() > P:
        got = pc.bias_emul(case, wrong="qk", heads=heads)
        _outside("query taps from the key position, " + case["id"], np.where(hidden, 0.0, got), fin, bound)
    if case["tails"]:
        got = pc.bias_emul(case, wrong="relx", heads=heads)
        _outside("relx[0] and relx[1] exchanged, " + case["id"], np.where(hidden, 0.0, got), fin, bound)
    if T > pc.BIAS_LOOP_EDGE:
        got = pc.bias_emul(case, wrong="loop", heads=heads)
        _outside("columns j >= 2048 unwritten, " + case["id"], got, fin, bound)


# ============================================================================================================ part C
@pytest.mark.parametrize("D", pc.L2_WIDTHS)
def test_l2norm_bound(D):
    x, ref, bound = pc.l2norm_case(D)
    assert not x[3].any() and not ref[3].any() and pc.is_bf16(x)
    got = pc.l2norm_emul(x)
    _inside("l2norm %d" % D, got, ref, bound)
    _outside("l2norm %d, rows rolled" % D, np.roll(got, 1, axis=0), ref, bound)


@pytest.mark.parametrize("N,k", pc.TOPK_CASES)
def test_topk_reference(N, k):
    rows = pc.topk_rows(N)
    ref = pc.topk_ref(rows, k)
    t = torch.from_numpy(rows.copy())
    for r in range(pc.TOPK_ROWS):
        assert len(set(ref[r])) == k and ref[r].min() >= 0 and ref[r].max() < N
        # torch.topk agrees on the values (NaN first); the order among equal values is this module's rule
        want = torch.topk(t[r], k).values.numpy()
        assert np.array_equal(np.isnan(want), np.isnan(rows[r][ref[r]])) and np.array_equal(np.nan_to_num(want, nan=9), np.nan_to_num(rows[r][ref[r]], nan=9))
        v = rows[r][ref[r]]
        for a in range(k - 1):
            if v[a] == v[a + 1] or (np.isnan(v[a]) and np.isnan(v[a + 1])):
                assert ref[r][a] < ref[r][a + 1]
    if N > 1:
        assert np.isnan(rows[3]).any() and np.isnan(rows[4]).sum() > N // 2 and np.isneginf(rows[2]).any()
        assert not np.array_equal(pc.topk_ref(rows, k, higher_on_ties=True), ref), "ties towards the higher index go unnoticed"


@pytest.mark.parametrize("case", pc.SOFTMAX_CASES, ids=_ids(pc.SOFTMAX_CASES))
def test_softmax_bound(case):
    x = pc.softmax_rows_of(case["n"], case["rows"])
    assert pc.is_bf16(x) and np.abs(x).max() <= 1.25 and x.shape == (case["rows"], case["n"])
    ref, bound = pc.softmax_ref(case)
    if not case["softmax"]:
        assert np.array_equal(ref, x.astype(np.float64))
        return
    a = x.astype(np.float64) / case["temp"]
    assert (a.max(1, keepdims=True) - a).max() <= 5.0
    got = pc.softmax_emul(case)
    _inside("softmax " + case["id"], got, ref, bound)
    if case["rows"] > 1 and case["n"] > 1:
        _outside("softmax, the second batch read without its gap, " + case["id"], np.roll(got, pc.SOFTMAX_T - pc.SOFTMAX_RPB, axis=0), ref, bound)


@pytest.mark.parametrize("k", pc.GATHER_KS)
def test_gather_mean_data(k):
    x, idx, ref = pc.gather_case(k)
    assert idx.min() >= 0 and idx.max() < pc.GATHER_BPN[1] and pc.is_f32(x)
    B, P, n = pc.GATHER_BPN
    s = np.array([[[sum(float(x[b, idx[b, p, j], c]) for j in range(k)) for c in range(n)] for p in range(P)] for b in range(B)])
    assert np.array_equal(ref, (s.astype(np.float32) / np.float32(k)))
    if k == 3:
        assert (ref.astype(np.float64) != s / 3).any()          # some quotients are rounded


@pytest.mark.parametrize("case", pc.EVAL_CASES, ids=_ids(pc.EVAL_CASES))
def test_seg_eval_case(case):
    hp, wp, h, w, n = (case[k] for k in ("hp", "wp", "h", "w", "n"))
    c = pc.seg_eval_case(hp, wp, h, w, n, case["all_ignored"])
    assert c["undecided"] <= c["cap"] == pc.MARGIN_CAP
    assert np.abs(c["scores"]).max() <= 2.0
    t = c["target"]
    if case["all_ignored"]:
        assert not c["valid"].any() and not c["hist"].any()
        return
    for val in (pc.SEG0 + n, pc.PAD_ID, pc.EOS_ID, pc.SEG0 - 1, 5):
        assert (t == val).any() or h * w < 64, val
    assert c["valid_share"] > 0.4 and c["hist"][1].sum() == c["hist"][2].sum() == c["valid"].sum() >= c["hist"][0].sum() > 0
    loss, v = pc.seg_eval_emul(c, hp, wp, h, w, n)
    _inside("seg_eval loss " + case["id"], loss, c["loss"], c["bound"])
    arg = v.argmax(1)
    assert np.array_equal(pc.seg_eval_hist(arg, t, n), c["hist"])          # the fp32 values name the same class on every counted pixel
    if (t == pc.SEG0 + n).any():
        assert not np.array_equal(pc.seg_eval_hist(arg, t, n, ignore_as_last=True), c["hist"]), "the ignore label counted as class n - 1 goes unnoticed"
    sums, bounds, cnt = pc.seg_eval_block_sums(c)
    assert cnt.sum() == c["valid"].sum() and (bounds >= 0).all() and sums.size == (h * w + 255) // 256
