"""_loss_cases.py checked alone, without a GPU: the numpy fp64 references against the torch fp64 composition (F.interpolate,
F.cross_entropy(weight=, label_smoothing=), autograd) and against the `*_reference` functions of criterions/seg_criterion.py; the
margin rule on every pixel of every case; and the two conditions every bound must meet:
  1. the fp32 restatement of each kernel, in the kernel's order of operations, sits inside its bound on every case;
  2. each of the fourteen wrong variants, applied to that restatement, lands outside TWICE the bound on a case the GPU file runs.
`report()` prints the worst ratios and the wrong-variant table of profiles/loss_conformance.txt (what the older rel-L2 / 2e-4 /
1e-6 assertions make of each variant included): python tests/test_loss_conformance_cpu.py
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _loss_cases as lc
from _loss_cases import U, worst_ratio

IDS = [c["id"] for c in lc.TILE_CASES]


def _torch_inputs(c):
    d = lc.tile_data(c["id"])
    B, hp, wp, n = c["B"], c["hp"], c["wp"], c["nseg"]
    L = torch.tensor(d["logits"], dtype=torch.float64, requires_grad=True)
    Tt = torch.tensor(d["teacher"], dtype=torch.float64)
    up = lambda x: F.interpolate(x.view(B, hp, wp, n).permute(0, 3, 1, 2), scale_factor=16, mode="bilinear", align_corners=False)
    tg = torch.tensor(d["target"])
    return L, up(L), up(Tt), tg


def _torch_ce(c, up, tg):
    """F.cross_entropy on the upsampled scores [B, n, H, W]; a label that is no class becomes the ignore index"""
    B, n = c["B"], c["nseg"]
    o = lc.ce_options(c)
    valid = torch.tensor(lc.is_class(lc.tile_data(c["id"])["target"], n))
    t = torch.where(valid, tg - lc.SEG0, torch.full_like(tg, -100)).view(B, up.shape[2], up.shape[3])
    cw = torch.tensor(o["cw"], dtype=torch.float64)
    l = F.cross_entropy(up, t, weight=cw, ignore_index=-100, reduction="none", label_smoothing=o["eps"]).reshape(B, -1)
    q = torch.ones_like(l) if o["q"] is None else torch.tensor(o["q"])
    q = q * valid
    if o["norm_pixels"]:
        Z = valid.sum() * (255.0 if o["has_plane"] else 1.0)
    else:
        Z = (q * cw[torch.where(valid, tg - lc.SEG0, torch.zeros_like(tg))]).sum() if o["weighted"] else valid.sum().double()
    return ((q * l).sum() / Z if float(Z) > 0 else (q * l).sum() * 0.0), float(Z)


# ------------------------------------------------------------------------------------------------ the references
@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_interpolation_matrix_is_f_interpolate(n):
    x = torch.randn(1, 1, n, 1, dtype=torch.float64, generator=torch.Generator().manual_seed(n))
    want = F.interpolate(x, size=(16 * n, 1), mode="bilinear", align_corners=False)[0, 0, :, 0].numpy()
    got = lc.interp_matrix(n) @ x[0, 0, :, 0].numpy()
    assert np.abs(got - want).max() < 1e-14
    assert np.abs(lc.local_weights(n).sum(1) - 1).max() < 1e-15


@pytest.mark.parametrize("cid", IDS)
def test_ce_reference_is_the_torch_composition(cid):
    c = lc.CASE[cid]
    L, up, _, tg = _torch_inputs(c)
    loss, Z = _torch_ce(c, up, tg)
    r = lc.ce_ref(cid)
    assert abs(Z - r["Z"]) <= 1e-9 * max(1.0, abs(Z))
    assert abs(float(loss.detach()) - r["loss"]) <= 1e-12 * max(1.0, abs(float(loss.detach())))
    ref, _, _, _ = lc.gather_ref(cid, True, False, False)
    if Z > 0:
        loss.backward()
        g = L.grad.numpy().reshape(ref.shape)
        assert np.abs(g - ref).max() <= 1e-12 * max(1.0, np.abs(g).max())
    else:
        assert not ref.any() and r["loss"] == 0.0 and not r["tp"].any()
    assert np.isfinite(r["tp_bound"]).all() and np.isfinite(r["sp0_bound"]).all()


@pytest.mark.parametrize("cid", IDS)
def test_references_are_the_criterion_specifications(cid):
    from ifseg_amd.criterions import seg_criterion as sc
    c = lc.CASE[cid]
    n, B = c["nseg"], c["B"]
    assert (sc.PAD, sc.EOS) == (lc.PAD_ID, lc.EOS_ID)
    L, up, upt, tg = _torch_inputs(c)
    s, t = up.permute(0, 2, 3, 1).reshape(B, -1, n), upt.permute(0, 2, 3, 1).reshape(B, -1, n)
    valid = torch.tensor(lc.is_class(tg.numpy(), n))
    clean = torch.where(valid | (tg == lc.PAD_ID) | (tg == lc.EOS_ID), tg, torch.full_like(tg, lc.SEG0 + n))    # bad labels: dropped
    o = lc.ce_options(c)
    cw = class_w = None
    if c["weighted"] and lc.class_weights(c) is not None:
        cw = torch.tensor(lc.class_weights(c))
    plane = lc.pixel_plane(c) if c["weighted"] else None
    ce = sc.weighted_loss_reference(s, clean, lc.SEG0, n, cw, None if plane is None else torch.tensor(plane), o["eps"],
                                    "pixels" if o["norm_pixels"] else "weights")
    assert abs(float(ce.detach()) - lc.ce_ref(cid)["loss"]) <= 1e-6 * max(1.0, abs(float(ce.detach())))       # (the specification keeps cw in fp32)
    dw = lc.class_weights(c, dice=True)
    class_w = None if dw is None else torch.tensor(dw)
    dice = lc.DICE_WEIGHT * sc.dice_loss_reference(s, tg, lc.SEG0, n, float(np.float32(c["smooth"])), class_w)
    rd = lc.dice_ref(cid)
    assert abs(float(dice.detach()) - rd["value"]) <= 1e-6 * max(1.0, abs(float(dice.detach())))
    sums = sc.dice_sums_reference(s, tg, lc.SEG0, n).numpy()
    assert np.abs(sums - rd["sums"]).max() <= 1e-10 * max(1.0, np.abs(sums).max())
    Tk = float(np.float32(c["T"]))
    kd = sc.distill_loss_reference(s, t, tg, lc.SEG0, n, Tk, "all" if c["mask_all"] else "valid")
    rk = lc.kd_ref(cid)
    N = rk["count"].sum()
    # (1 / T is the fp32 reciprocal the entry point forms: the specification divides by T in double)
    assert abs(float(kd.detach()) - (Tk * Tk * rk["kl"].sum() / max(N, 1.0))) <= 1e-6 * max(1.0, abs(float(kd.detach())))
    total = ce + dice + lc.KD_W * kd
    total.backward()
    ref, _, loss, _ = lc.gather_ref(cid, True, True, True)
    g = L.grad.numpy().reshape(ref.shape)
    assert np.abs(g - ref).max() <= 2e-6 * max(1e-30, np.abs(g).max())
    assert abs(loss[0] - float(total.detach())) <= 2e-6 * max(1.0, abs(float(total.detach())))
    h = sc.hardness_reference(s.detach(), tg, lc.SEG0, n).numpy()
    assert np.abs(h - lc.hardness_ref(cid)[0]).max() <= 1e-12


@pytest.mark.parametrize("cid", [c["id"] for c in lc.OHEM_CASES if c["N"] < 10 ** 5])
def test_ohem_expectation_is_the_specification(cid):
    from ifseg_amd.criterions.seg_criterion import ohem_reference
    c = next(x for x in lc.OHEM_CASES if x["id"] == cid)
    h, w = lc.ohem_plane(cid)
    plane, info = lc.ohem_expected(h, c["B"], c["thresh"], c["min_kept"], w)
    p2, i2 = ohem_reference(torch.tensor(h), c["thresh"], c["min_kept"], None if w is None else torch.tensor(w))
    assert np.array_equal(plane, p2.numpy()) and np.array_equal(info, i2.numpy())


def test_ohem_cases_reach_what_they_name():
    info = {}
    for c in lc.OHEM_CASES:
        h, w = lc.ohem_plane(c["id"])
        info[c["id"]] = lc.ohem_expected(h, c["B"], c["thresh"], c["min_kept"], w)[1]
    tb = lambda x: int(np.array([x], dtype=np.float32).view(np.uint32)[0])
    assert info["nvalid0"][0] == 0 and info["all-equal"][1] == 0 and info["all-equal"][0] > 0
    assert info["thresh-above-kth"][2] == tb(0.9) > info["thresh-above-kth"][3]
    assert info["thresh-below-kth"][2] == info["thresh-below-kth"][3] > tb(0.05)
    assert info["thresh-equal-kth"][3] == tb(0.5) == info["kth-many-ties"][3]
    c = next(x for x in lc.OHEM_CASES if x["id"] == "minkept-ge-nvalid")
    assert c["min_kept"] * c["B"] >= info["minkept-ge-nvalid"][0]
    assert lc.OHEM_BIG <= 8 * 2 ** 20 and lc.OHEM_BIG > 512 * 1024


# ------------------------------------------------------------------------------------------------ the margin rule
@pytest.mark.parametrize("cid", IDS)
def test_every_valid_pixel_has_a_top2_margin_above_the_value_bound(cid):
    c = lc.CASE[cid]
    d = lc.tile_data(cid)
    gap, need = lc.margins(d["logits"], d["target"], c["hp"], c["wp"])
    valid = lc.is_class(d["target"], c["nseg"])
    if c["regime"] == "ties":
        assert not gap.any()                   # exact ties, in fp32 as in fp64: `if (v > m)` keeps the lowest index
        assert not lc.ce_ref(cid)["pred"].any()
        return
    assert bool((gap > need)[valid].all()), "margin rule broken on %d pixels" % int((gap <= need)[valid].sum())


def test_case_tables_reach_the_listed_paths():
    grids = {(c["hp"], c["wp"]) for c in lc.TILE_CASES}
    assert {(1, 1), (1, 3), (3, 1), (2, 2), (3, 4)} <= grids
    assert {1, 2, 15, 16, 17, 150, 171, 257, 512} <= {c["nseg"] for c in lc.TILE_CASES}
    assert {1, 2, 3} <= {c["B"] for c in lc.TILE_CASES}
    assert {0.0, 0.1, 1.0} <= {c["eps"] for c in lc.TILE_CASES}
    assert all(c["B"] * c["hp"] * c["wp"] <= 3 * 12 * 16 and c["nseg"] <= 512 for c in lc.TILE_CASES)
    for c in lc.TILE_CASES:
        if c["plane"]:
            assert {0, 1, 128, 255} <= set(np.unique(lc.pixel_plane(c)).tolist())
    assert lc.bad_label(lc.CASE["g2x2-n17-bad"]) == 1 and lc.bad_label(lc.CASE["g3x4-n150"]) == 0
    r = lc.ce_ref("g3x4-n150")
    assert not r["valid"][2].any() and r["valid"][0].any() and not r["valid"][0, :16, :16].any()
    assert not lc.ce_ref("g2x2-n17-invalid")["valid"].any()
    assert (lc.dice_ref("g3x4-n150")["sums"][1, 2, 1] == 0)                # a class absent from a sample


# ------------------------------------------------------------------------------------------------ condition 1
def _ratios():
    """worst |restatement - reference| / bound per case and quantity"""
    out = {}
    for c in lc.TILE_CASES:
        cid = c["id"]
        r, e = lc.ce_ref(cid), lc.ce_emulate(cid)
        out["A %s tile_partial" % cid] = worst_ratio(e["tp"], r["tp"], r["tp_bound"])[0]
        out["A %s stats_part[0]" % cid] = worst_ratio(e["sp0"], r["sp0"], r["sp0_bound"])[0]
        out["A %s stats_part[1]" % cid] = worst_ratio(e["sp1"], r["sp1"], r["sp1_bound"])[0]
        out["A %s histograms" % cid] = float((e["hist"] != r["hist"]).any()) * np.inf if (e["hist"] != r["hist"]).any() else 0.0
        h, hb = lc.hardness_ref(cid)
        out["E %s hardness" % cid] = worst_ratio(lc.hardness_emulate(cid), h, hb)[0]
    for c in lc.DICE_CASES:
        cid = c["id"]
        r = lc.dice_ref(cid)
        tp, val = lc.dice_tile_emulate(cid)
        out["B %s sums" % cid] = worst_ratio(lc.dice_sums_emulate(cid), r["sums"], r["sums_bound"])[0]
        out["B %s tile_partial" % cid] = worst_ratio(tp, r["tp"], r["tp_bound"])[0]
        out["B %s dice_out" % cid] = worst_ratio(np.array([val]), np.array([r["value"]]), np.array([r["value_bound"]]))[0]
    for c in lc.KD_CASES:
        cid = c["id"]
        r = lc.kd_ref(cid)
        tp, kl, cnt = lc.kd_emulate(cid)
        out["C %s tile_partial" % cid] = worst_ratio(tp, r["tp"], r["tp_bound"])[0]
        out["C %s kd_part[0]" % cid] = worst_ratio(kl, r["kl"], r["kl_bound"])[0]
        assert np.array_equal(cnt, r["count"])
    for c in lc.GATHER_CASES:
        for sub in range(1, 8):
            use = (bool(sub & 1), bool(sub & 2), bool(sub & 4))
            ref, bound, loss, lb = lc.gather_ref(c["id"], *use)
            dl, lo = lc.end_to_end_emulate(c["id"], *use)
            out["D %s sources %d dlogits" % (c["id"], sub)] = worst_ratio(dl, ref, bound)[0]
            out["D %s sources %d loss_out" % (c["id"], sub)] = worst_ratio(lo, loss, lb)[0]
    for c in lc.SUMSQ_CASES:
        if c["n"]:
            ref, b = lc.sumsq_ref(c["n"], c["data"])
            out["F sumsq %s" % c["id"]] = abs(lc.sumsq_emulate(c["n"], c["data"]) - ref) / b
    for c in lc.ADAM_CASES:
        r, e = lc.adam_ref(c["id"]), lc.adam_emulate(c["id"])
        for k in "pmv":
            out["F adam %s %s" % (c["id"], k)] = worst_ratio(e[k], r[k], r["d" + k])[0]
    return out


def test_condition_1_every_restatement_sits_inside_its_bound():
    bad = {k: v for k, v in _ratios().items() if not v <= 1.0}
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ condition 2
def _old_rules(dl, ref, loss, loss_ref):
    """what test_fused_seg_loss / test_weighted_loss_gpu / test_dice_gpu / test_distill_gpu assert: rel-L2 < 6e-3 on the gradient,
    |loss - ref| <= 2e-4 max(1, |ref|)"""
    rel = float(np.linalg.norm(dl - ref) / max(np.linalg.norm(ref), 1e-30))
    return rel, rel < 6e-3 and abs(loss - loss_ref) <= 2e-4 * max(1.0, abs(loss_ref))


def _tile_variant(v, cid, part):
    """-> (worst ratio of the variant's tile partials, the old rules' verdict on the end-to-end gradient)"""
    if part == "S":             # exact on the synthetic partials: any difference is outside a bound of zero
        hp, wp, B = cid
        args = [lc.stencil_partials(B, hp, wp, 5, 1), np.float32([3.0, 4.0]), lc.stencil_partials(B, hp, wp, 5, 2),
                lc.stencil_partials(B, hp, wp, 5, 3), np.float32([1.0, 8.0]), 2.0, 2.0]
        ratio = float("inf") if not np.array_equal(lc.gather_emulate(*args), lc.gather_emulate(*args, variant=v)) else 0.0
        part, cid = "D", "g3x4-n150"
        ref, bound, loss, _ = lc.gather_ref(cid, True, False, False)
        dl, lo = lc.end_to_end_emulate(cid, True, False, False, variant=v)
        return (ratio,) + _old_rules(dl, ref, lo[0], loss[0])
    use = dict(A=(True, False, False), B=(False, True, False), D=(True, False, False), K=(True, False, True))[part]
    if part == "A":
        r, e = lc.ce_ref(cid), lc.ce_emulate(cid, variant=v)
        ratio = worst_ratio(e["tp"], r["tp"], r["tp_bound"])[0]
    elif part == "B":
        r = lc.dice_ref(cid)
        ratio = worst_ratio(lc.dice_tile_emulate(cid, variant=v)[0], r["tp"], r["tp_bound"])[0]
    ref, bound, loss, _ = lc.gather_ref(cid, *use)
    dl, lo = lc.end_to_end_emulate(cid, *use, variant=v)
    if part in "DK":
        ratio = worst_ratio(dl, ref, bound)[0]
    rel, old_pass = _old_rules(dl, ref, lo[0], loss[0])
    return ratio, rel, old_pass


def _adam_variant(v, cid):
    r, e = lc.adam_ref(cid), lc.adam_emulate(cid, variant=v)
    ratio = max(worst_ratio(e[k], r[k], r["d" + k])[0] for k in "pmv")
    err = float(np.abs(e["p"] - r["p"]).max())
    return ratio, err, err < 1e-6          # test_adam_and_gradnorm: |p32 - ref| < 1e-6; m and v are compared with nothing


VARIANTS = [
    (1, "the top clamp fmaxf(src, 0) dropped", "A", "g3x4-n150"),
    (2, "i1 = i0 + 1 without the clamp (reads the zero cell)", "A", "g3x4-n150"),
    (3, "the last ragged class chunk's final class lost", "A", "g2x2-n17-bad"),
    (4, "class c >= 256 staged from c - 256", "A", "g2x2-n257"),
    (5, "ky and kx swapped in the gather", "D", "g3x4-n150"),
    # (a real tile's partial towards a cell outside the grid is an exact zero, so this one shows on the synthetic partials only)
    (6, "the corner cell sums a partial from outside the grid", "S", (3, 4, 2)),
    (7, "hot without (1 - eps)", "A", "g2x2-n17-bad"),
    (8, "unif * sCw[c] dropped from the weighted gradient", "A", "g2x2-n17-bad"),
    (9, "the normaliser taken per sample instead of per batch", "D", "g3x4-n150"),
    (10, "Dice e built with Q instead of Q^2", "B", "g3x4-n150"),
    (11, "the KD gradient scaled by T^2 instead of T", "K", "g2x2-n17-bad"),
    (12, "Adam's v built from the unclipped gradient", "F", "n1027-step10-value"),
    (13, "the weight-decay term applied after the step", "F", "n1027-step1000-value"),
    (14, "m bias-corrected with bc2", "F", "n1027-step10-value"),
]


@pytest.mark.parametrize("v,what,part,cid", VARIANTS, ids=["variant%d" % x[0] for x in VARIANTS])
def test_condition_2_wrong_variant_lands_outside_twice_the_bound(v, what, part, cid):
    ratio = _adam_variant(v, cid)[0] if part == "F" else _tile_variant(v, cid, part)[0]
    print("[loss] variant %d (%s) on %s: %.3g of the bound" % (v, what, cid, ratio))
    assert ratio > 2.0, "variant %d (%s) stays within %.3f of the bound on %s" % (v, what, ratio, cid)


def test_stencil_partials_are_exact_and_pin_the_layout():
    """the synthetic gather: every operation exact, so the fp32 restatement equals the fp64 stencil; variants 5 and 6 do not"""
    for hp, wp, B in lc.STENCIL_GRIDS:
        n = 5
        ce, di, kd = (lc.stencil_partials(B, hp, wp, n, s) for s in (1, 2, 3))
        want = lc.stencil_gather(ce.astype(np.float64)) / 4 + lc.stencil_gather(di.astype(np.float64)) \
            + lc.stencil_gather(kd.astype(np.float64)) * (2.0 * 2.0 / 8.0)
        got = lc.gather_emulate(ce, np.float32([3.0, 4.0]), di, kd, np.float32([1.0, 8.0]), 2.0, 2.0)
        assert np.array_equal(got.astype(np.float64), lc.bf16_round(want).astype(np.float64))
        if hp * wp > 1:
            for v in (5, 6):
                bad = lc.gather_emulate(ce, np.float32([3.0, 4.0]), di, kd, np.float32([1.0, 8.0]), 2.0, 2.0, variant=v)
                assert not np.array_equal(bad, got), (hp, wp, v)


# ------------------------------------------------------------------------------------------------ the profile's CPU half
def report():
    lines = ["worst |fp32 restatement - fp64 reference| / bound (condition 1)"]
    for k, v in _ratios().items():
        lines.append("  %-52s %.3f" % (k, v))
    lines.append("")
    lines.append("wrong variants (condition 2: outside twice the bound); old: the rel-L2 < 6e-3 + 2e-4 loss rule of the older tests")
    lines.append("(Adam: |p32 - ref| < 1e-6 of test_adam_and_gradnorm) applied to the same restatement")
    for v, what, part, cid in VARIANTS:
        if part == "F":
            ratio, err, ok = _adam_variant(v, cid)
            lines.append("  %2d %-55s %-22s %10.3g x bound   old: max |dp| %.2e -> %s" % (v, what, cid, ratio, err, "PASSES" if ok else "fails"))
        else:
            ratio, rel, ok = _tile_variant(v, cid, part)
            lines.append("  %2d %-55s %-22s %10.3g x bound   old: rel-L2 %.2e -> %s" % (v, what, "stencil %dx%d B%d" % cid if part == "S" else cid, ratio, rel, "PASSES" if ok else "fails"))
    return "\n".join(lines)


if __name__ == "__main__":
    print(report())
