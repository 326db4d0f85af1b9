"""CPU: the specification of the distillation term (`distill_loss_reference`) against a literal per-pixel F.kl_div and against a
transcription of mmrazor's KLDivergence, the closed-form gradient the kernel computes against fp64 autograd, the criterion's
reference path with and without `distill_weight`, the refusals, `reduce_metrics`, the C ABI surface and the op's fake kernel."""
import ctypes
import os
import re
import types

import pytest
import torch
import torch.nn.functional as F

import _dice_cases as DC
import _distill_cases as KC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG0 = KC.SEG0
TRAINING = types.SimpleNamespace(training=True)
EVAL = types.SimpleNamespace(training=False)
KW = dict(unsupervised_segmentation=False, init_seg_with_text=False, seg_id_offset=SEG0)
SMALL = [(2, 2, 3, 4), (5, 2, 3, 4), (17, 2, 3, 4), (15, 3, 1, 1)]


def _both(nseg, B, hp, wp, kind, dtype=torch.float64):
    lp, tgt, _ = DC.dice_inputs(nseg, B, hp, wp)
    return KC.scores(lp, nseg, hp, wp, dtype), KC.scores(KC.teacher(nseg, B, hp, wp, kind), nseg, hp, wp, dtype), tgt


@pytest.mark.parametrize("nseg,B,hp,wp", SMALL)
def test_reference_is_the_literal_per_pixel_kl(nseg, B, hp, wp):
    """pixel by pixel: T^2 / N times the sum over M of F.kl_div(log_softmax(s / T), softmax(t / T), reduction="none").sum(-1)"""
    from ifseg_amd.criterions.seg_criterion import distill_loss_reference, distill_sums_reference
    for kind in KC.TEACHERS + ("same",):
        s, t, tgt = _both(nseg, B, hp, wp, kind)
        valid = DC.valid_mask(tgt, nseg)
        for T in KC.TEMPERATURES:
            kl = F.kl_div(F.log_softmax(s / T, -1), F.softmax(t / T, -1), reduction="none").sum(-1)          # [B, H*W]
            for mask in KC.MASKS:
                m = valid if mask == "valid" else torch.ones_like(valid)
                want = T * T * sum(float(kl[b, i]) for b, i in m.nonzero().tolist()) / int(m.sum())
                got = distill_loss_reference(s, t, tgt, SEG0, nseg, T, mask)
                sums = distill_sums_reference(s, t, tgt, SEG0, nseg, T, mask)
                assert abs(float(got) - want) <= 1e-12 * max(1.0, abs(want)), (kind, T, mask, float(got), want)
                assert int(sums[1]) == int(m.sum()) and (kind != "same" or abs(float(got)) <= 1e-15)
    assert float(distill_loss_reference(*_both(nseg, B, hp, wp, "far"), SEG0, nseg)) > 0.1          # the defaults: T = 1, "valid"


@pytest.mark.parametrize("nseg,B,hp,wp", SMALL)
def test_reference_with_every_pixel_is_mmrazors_batchmean_over_the_pixels(nseg, B, hp, wp):
    """the only relation to upstream claimed: mask="all" == KLDivergence(tau=T, reduction="batchmean") / (H W)"""
    from ifseg_amd.criterions.seg_criterion import distill_loss_reference
    H, W = 16 * hp, 16 * wp
    s, t, tgt = _both(nseg, B, hp, wp, "far")
    to_map = lambda x: x.transpose(1, 2).reshape(B, nseg, H, W)
    for T in KC.TEMPERATURES:
        want = float(KC.mmrazor_kl_divergence(to_map(s), to_map(t), tau=T)) / (H * W)
        for target in (tgt, None):
            got = float(distill_loss_reference(s, t, target, SEG0, nseg, T, "all"))
            assert abs(got - want) <= 1e-12 * max(1.0, abs(want)), (T, got, want)


@pytest.mark.parametrize("nseg,B,hp,wp", KC.SHAPES)
def test_closed_form_gradient_is_autograd(nseg, B, hp, wp):
    """fp64: d L_kd / d s_ic = (T / N) (p_ic - q_ic) on M, zero elsewhere, to 1e-12"""
    from ifseg_amd.criterions.seg_criterion import distill_grad_closed_form, distill_loss_reference
    s, t, tgt = _both(nseg, B, hp, wp, "far")
    valid = DC.valid_mask(tgt, nseg)
    for T in KC.TEMPERATURES:
        for mask in KC.MASKS:
            x = s.clone().requires_grad_(True)
            distill_loss_reference(x, t, tgt, SEG0, nseg, T, mask).backward()
            got = distill_grad_closed_form(s, t, tgt, SEG0, nseg, T, mask)
            err = float((got - x.grad).abs().max())
            assert tuple(got.shape) == tuple(s.shape) and float(x.grad.abs().max()) > 0.0
            assert err <= 1e-12, (T, mask, err)
            if mask == "valid":
                assert float(got[~valid].abs().max()) == 0.0
            elif B == 3:
                assert float(got[2].abs().max()) > 0.0                        # the all-ignore sample is distilled under "all"


def test_no_masked_pixel_gives_zero():
    from ifseg_amd.criterions.seg_criterion import distill_grad_closed_form, distill_loss_reference, distill_sums_reference
    nseg, B, hp, wp = 15, 3, 1, 1
    s, t, tgt = _both(nseg, B, hp, wp, "far")
    s, t, tgt = s[2:], t[2:], tgt[2:]                                         # the all-ignore sample alone
    x = s.clone().requires_grad_(True)
    loss = distill_loss_reference(x, t, tgt, SEG0, nseg, 2.0, "valid")
    loss.backward()
    assert float(loss.detach()) == 0.0 and float(x.grad.abs().max()) == 0.0
    assert distill_sums_reference(s, t, tgt, SEG0, nseg, 2.0, "valid").tolist() == [0.0, 0.0]
    assert float(distill_grad_closed_form(s, t, tgt, SEG0, nseg, 2.0, "valid").abs().max()) == 0.0
    assert float(distill_loss_reference(s, t, tgt, SEG0, nseg, 2.0, "all")) > 0.0


def _net_output(nseg, B, hp, wp, kind="far"):
    lp, tgt, cw = DC.dice_inputs(nseg, B, hp, wp)
    tgt = DC.clean_target(tgt, nseg)
    H, W = 16 * hp, 16 * wp
    extra = {"encoder_returns": {"image_embed_shape": [(hp, wp)]}}
    sample = {"target": tgt, "net_input": {"patch_images": torch.zeros(B, 3, H, W)}, "ntokens": 1, "nsentences": B,
              "teacher_logits": KC.teacher(nseg, B, hp, wp, kind)}
    return (lp[:, :, :nseg].float(), extra), sample, cw


def test_criterion_reference_path_and_the_default():
    from ifseg_amd.criterions import SegCriterion
    from ifseg_amd.criterions.seg_criterion import dice_loss_reference, distill_loss_reference, distill_sums_reference
    nseg, B, hp, wp = 17, 2, 3, 4
    H, W = 16 * hp, 16 * wp
    net_output, sample, cw = _net_output(nseg, B, hp, wp)
    plain_sample = {k: v for k, v in sample.items() if k != "teacher_logits"}
    scores = SegCriterion.upsample_logits(net_output[0], hp, wp, H, W)
    tgt = sample["target"]
    mask = (tgt == 1) | (tgt == SEG0 + nseg) | (tgt == 2)
    plain = F.cross_entropy(scores[~mask], tgt[~mask] - SEG0)
    # distill_weight=None: today's bits and keys, whether or not the sample carries teacher logits
    base = SegCriterion(num_seg_tokens=nseg, **KW)
    assert base.distill_weight is None and base.distill_temperature == 1.0 and base.distill_mask == "valid" and base.distill_stats is None
    for smp in (plain_sample, sample):
        loss0, metrics0, one = base.compute_loss_torch(TRAINING, net_output, smp, 0)
        assert torch.equal(loss0, plain) and one == 1 and base.distill_stats is None
        assert sorted(metrics0) == ["area_intersect", "area_label", "area_pred_label", "area_union", "nll_loss"]
    log0 = dict({"loss": loss0, "imfree_loss": loss0 * 0, "seg_loss": loss0, "ntokens": 1, "nsentences": B, "sample_size": 1}, **metrics0)
    red0 = SegCriterion.reduce_metrics([log0, log0])
    assert sorted(red0) == ["aAcc", "imfree_loss", "loss", "mAcc", "mIoU", "nll_loss", "nsentences", "ntokens", "sample_size", "seg_loss"]
    # distill_weight: CE + weight * reference, nll_loss stays the CE term
    t_up = KC.scores(sample["teacher_logits"], nseg, hp, wp, torch.float32)
    for T, m in ((1.0, "valid"), (2.0, "all")):
        crit = SegCriterion(num_seg_tokens=nseg, distill_weight=1.5, distill_temperature=T, distill_mask=m, **KW)
        loss, metrics, _ = crit.compute_loss_torch(TRAINING, net_output, sample, 0)
        kd = 1.5 * distill_loss_reference(scores[:, :H * W], t_up, tgt, SEG0, nseg, T, m)
        assert torch.equal(metrics["nll_loss"], plain) and torch.equal(metrics["kd_loss"], kd) and torch.equal(loss, plain + kd)
        assert float(kd) > 0.0 and torch.equal(crit.distill_stats, distill_sums_reference(scores[:, :H * W], t_up, tgt, SEG0, nseg, T, m))
        assert sorted(set(metrics) - set(metrics0)) == ["kd_loss"]
        for k in metrics0:
            assert torch.equal(metrics[k], metrics0[k]), k
        log = dict(log0, loss=loss, seg_loss=loss, **metrics)
        red = SegCriterion.reduce_metrics([log, log])
        assert sorted(set(red) - set(red0)) == ["kd_loss"] and abs(red["kd_loss"] - float(kd)) < 1e-6
        assert all(red[k] == red0[k] for k in red0 if k not in ("loss", "seg_loss"))
        # a call that trains nothing skips the term when the key is missing
        for mdl, ctx in ((EVAL, torch.enable_grad()), (TRAINING, torch.no_grad())):
            with ctx:
                l2, m2, _ = crit.compute_loss_torch(mdl, net_output, plain_sample, 0)
            assert torch.equal(l2, plain) and "kd_loss" not in m2
    # composes with Dice and the CE options: the KD term sees neither the pixel nor the class weights
    pw = DC.pixel_plane(B, H * W)
    both = SegCriterion(num_seg_tokens=nseg, distill_weight=1.5, dice_weight=3.0, class_weight=cw, weight_norm="pixels", **KW)
    only = SegCriterion(num_seg_tokens=nseg, class_weight=cw, weight_norm="pixels", **KW)
    lb, mb, _ = both.compute_loss_torch(TRAINING, net_output, dict(sample, target_weight=pw), 0)
    lo, _, _ = only.compute_loss_torch(TRAINING, net_output, dict(sample, target_weight=pw), 0)
    dice = 3.0 * dice_loss_reference(scores[:, :H * W], tgt, SEG0, nseg)
    kd = 1.5 * distill_loss_reference(scores[:, :H * W], t_up, tgt, SEG0, nseg)
    assert torch.equal(mb["nll_loss"], lo) and torch.equal(mb["dice_loss"], dice) and torch.equal(mb["kd_loss"], kd)
    assert torch.equal(lb, lo + dice + kd)


def test_refusals():
    from ifseg_amd import hip
    from ifseg_amd.criterions import SegCriterion
    from ifseg_amd.criterions.seg_criterion import distill_loss_reference
    kw = dict(num_seg_tokens=5, **KW)
    for bad in (0, -1.0, float("nan"), float("inf"), "3", True):
        with pytest.raises(ValueError, match="distill_weight"):
            SegCriterion(distill_weight=bad, **kw)
        with pytest.raises(ValueError, match="distill_weight"):
            hip.check_distill(bad, 1.0, "valid", "t")
    for bad in (0, -1.0, float("nan"), float("inf"), "1", None, False):
        with pytest.raises(ValueError, match="distill_temperature"):
            SegCriterion(distill_weight=1.0, distill_temperature=bad, **kw)
        with pytest.raises(ValueError, match="distill_temperature"):
            SegCriterion(distill_temperature=bad, **kw)
        with pytest.raises(ValueError, match="distill_temperature"):
            distill_loss_reference(torch.zeros(1, 4, 5), torch.zeros(1, 4, 5), torch.full((1, 4), SEG0), SEG0, 5, temperature=bad)
    for bad in ("none", "ALL", None, 1, True):
        with pytest.raises(ValueError, match="distill_mask"):
            SegCriterion(distill_weight=1.0, distill_mask=bad, **kw)
        with pytest.raises(ValueError, match="distill_mask"):
            hip.check_distill(None, 1.0, bad, "t")
    assert hip.check_distill(None, 2, "all", "t") == (None, 2.0, True) and hip.check_distill(3, 1.0, "valid", "t") == (3.0, 1.0, False)
    with pytest.raises(ValueError, match="scores_up"):
        distill_loss_reference(torch.zeros(1, 4, 6), torch.zeros(1, 4, 5), torch.full((1, 4), SEG0), SEG0, 5)
    with pytest.raises(ValueError, match="teacher_up"):
        distill_loss_reference(torch.zeros(1, 4, 5), torch.zeros(1, 4, 6), torch.full((1, 4), SEG0), SEG0, 5)
    with pytest.raises(ValueError, match="teacher_up"):
        distill_loss_reference(torch.zeros(1, 4, 5), torch.zeros(2, 4, 5), torch.full((1, 4), SEG0), SEG0, 5)
    with pytest.raises(ValueError, match="target"):
        distill_loss_reference(torch.zeros(1, 4, 5), torch.zeros(1, 4, 5), torch.full((1, 7), SEG0), SEG0, 5)
    with pytest.raises(ValueError, match="target"):
        distill_loss_reference(torch.zeros(1, 4, 5), torch.zeros(1, 4, 5), None, SEG0, 5)
    # the sample
    nseg, B, hp, wp = 5, 2, 3, 4
    net_output, sample, _ = _net_output(nseg, B, hp, wp)
    crit = SegCriterion(num_seg_tokens=nseg, distill_weight=2, distill_temperature=2, distill_mask="all", **KW)
    assert (crit.distill_weight, crit.distill_temperature, crit.distill_mask) == (2.0, 2.0, "all")
    te = sample["teacher_logits"]
    with pytest.raises(ValueError, match="teacher_logits"):
        crit.compute_loss_torch(TRAINING, net_output, {k: v for k, v in sample.items() if k != "teacher_logits"}, 0)
    for bad, what in ((te.float(), "bf16"), (te[:1], "shape"), (te[:, :-1], "shape"), (te[:, :, :nseg - 1], "shape"),
                      (te[0], "shape"), ("x", "bf16"), (te.to("meta"), "device")):
        with pytest.raises(ValueError, match=what):
            crit.compute_loss_torch(TRAINING, net_output, dict(sample, teacher_logits=bad), 0)
    # the task
    from ifseg_amd.tasks.mm_tasks import SegmentationTask
    task = SegmentationTask(num_seg_tokens=5, patch_image_size=32, n_base_vocab=100, category_token_ids=[[31], [32, 33], [34], [35], [36]])
    model = types.SimpleNamespace(training=True)
    with pytest.raises(ValueError, match="teacher"):
        task.distill_sample(sample, model)
    with pytest.raises(ValueError, match="store_ema"):
        task.distill_sample(sample, model, trainer=types.SimpleNamespace(store_ema=False, model=model))
    with pytest.raises(ValueError, match="another model"):
        task.distill_sample(sample, model, trainer=types.SimpleNamespace(store_ema=True, model=object()))


def test_reduce_metrics_reports_kd_loss_only_when_present():
    from ifseg_amd.criterions import SegCriterion
    one = torch.tensor(2.0)
    area = torch.ones(3)
    log = {"loss": one, "imfree_loss": one * 0, "seg_loss": one, "nll_loss": one, "ntokens": 1, "nsentences": 2, "sample_size": 1,
           "area_intersect": area, "area_pred_label": area, "area_label": area, "area_union": area}
    assert "kd_loss" not in SegCriterion.reduce_metrics([log, log])
    red = SegCriterion.reduce_metrics([dict(log, kd_loss=torch.tensor(0.5)), dict(log, kd_loss=torch.tensor(1.5))])
    assert red["kd_loss"] == 1.0 and "dice_loss" not in red
    red = SegCriterion.reduce_metrics([dict(log, kd_loss=torch.tensor(0.5), dice_loss=one), log])
    assert red["kd_loss"] == 0.25 and red["dice_loss"] == 1.0


def test_abi_declares_and_exports_the_entry_points():
    from ifseg_amd import hip
    hdr = open(os.path.join(ROOT, "include", "ifseg_hip.h")).read()
    names = set(re.findall(r"\bint\s+(ifseg_\w+)\s*\(", hdr))
    new = {"ifseg_seg_distill_tiles", "ifseg_seg_loss_gather3"}
    assert new <= names
    assert int(re.search(r"#define IFSEG_ABI_VERSION (\d+)", hdr).group(1)) == 21 == hip.ABI_VERSION
    if not os.path.exists(hip.LIB_PATH):
        from ifseg_amd.build import build
        build(verbose=False)
    lib = hip.lib()
    assert all(hasattr(lib, n) for n in new)
    lib.ifseg_abi_version.restype = ctypes.c_int
    assert lib.ifseg_abi_version() == 21
    assert callable(hip.seg_distill) and callable(hip.seg_loss_distill) and callable(hip.check_distill)


def test_op_has_a_fake_kernel():
    import ifseg_amd.ops  # noqa: F401
    B, hp, wp, nseg = 2, 3, 4, 15
    H, W = 16 * hp, 16 * wp
    logits = torch.empty(B, hp * wp + 1, nseg, dtype=torch.bfloat16, device="meta")
    teacher = torch.empty(B, hp * wp + 1, 16, dtype=torch.bfloat16, device="meta")
    tgt = torch.empty(B, H * W + 1, dtype=torch.int64, device="meta")
    for target, mask_all in ((tgt, False), (tgt, True), (None, True)):
        loss, stats, dl = torch.ops.ifseg.seg_distill(logits, teacher, target, hp, wp, H, W, SEG0, 1.5, 2.0, mask_all)
        assert loss.dtype == torch.float32 and tuple(loss.shape) == () and loss.device.type == "meta"
        assert stats.dtype == torch.float32 and tuple(stats.shape) == (2,)
        assert dl.dtype == torch.bfloat16 and tuple(dl.shape) == (B, hp * wp + 1, 16)
    with pytest.raises(ValueError, match="distill_weight"):
        torch.ops.ifseg.seg_distill(logits, teacher, tgt, hp, wp, H, W, SEG0, 0.0, 1.0, False)
    with pytest.raises(ValueError, match="distill_temperature"):
        torch.ops.ifseg.seg_distill(logits, teacher, tgt, hp, wp, H, W, SEG0, 1.5, -1.0, False)
    with pytest.raises(ValueError, match="mask_all"):
        torch.ops.ifseg.seg_distill(logits, teacher, None, hp, wp, H, W, SEG0, 1.5, 1.0, False)
    with pytest.raises(ValueError, match="teacher_logits"):
        torch.ops.ifseg.seg_distill(logits, teacher[:, :-1], tgt, hp, wp, H, W, SEG0, 1.5, 1.0, False)
    with pytest.raises(ValueError, match="teacher_logits"):
        torch.ops.ifseg.seg_distill(logits, teacher.float(), tgt, hp, wp, H, W, SEG0, 1.5, 1.0, False)
    with pytest.raises(ValueError, match="x16"):
        torch.ops.ifseg.seg_distill(logits, teacher, tgt, hp, wp, H + 16, W, SEG0, 1.5, 1.0, False)
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.ifseg.seg_distill(torch.zeros(B, hp * wp + 1, nseg, dtype=torch.bfloat16), torch.zeros(B, hp * wp + 1, 16, dtype=torch.bfloat16),
                                    torch.zeros(B, H * W + 1, dtype=torch.int64), hp, wp, H, W, SEG0, 1.5, 1.0, False)
