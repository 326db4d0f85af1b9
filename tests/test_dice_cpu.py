"""CPU: the specifications of the Dice auxiliary loss (`dice_sums_reference`, `dice_loss_reference`) against a literal
transcription of the upstream loss, the closed-form gradient the kernel computes against autograd, the criterion's reference
path with and without `dice_weight`, the refusals, the C ABI surface and the dispatcher op's fake kernel."""
import ctypes
import os
import re
import types

import pytest
import torch

import _dice_cases as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG0 = DC.SEG0
TRAINING = types.SimpleNamespace(training=True)
KW = dict(unsupervised_segmentation=False, init_seg_with_text=False, seg_id_offset=SEG0)


def _every_pixel_a_class(tgt, nseg):
    """the case's targets with pad / ignore / out-of-range labels replaced by classes: upstream and the rule agree exactly here"""
    t = tgt.clone()
    body = t[:, :-1]
    bad = ~((body >= SEG0) & (body < SEG0 + nseg))
    body[bad] = SEG0 + (torch.arange(body.numel()).reshape(body.shape)[bad] % nseg)
    return t


@pytest.mark.parametrize("nseg,B,hp,wp", [(2, 2, 3, 4), (5, 2, 3, 4), (17, 2, 3, 4), (15, 3, 1, 1)])
def test_reference_is_the_upstream_loss(nseg, B, hp, wp):
    """fp64, no ignored pixel: one binary_dice_loss per class, per sample, mean over the batch, sum over classes / num_classes"""
    from ifseg_amd.criterions.seg_criterion import dice_loss_reference
    lp, tgt, cw = DC.dice_inputs(nseg, B, hp, wp)
    tgt = _every_pixel_a_class(tgt, nseg)
    H, W = 16 * hp, 16 * wp
    scores = DC._scores(lp, nseg, hp, wp, torch.float64)
    pred = scores[:, :-1].transpose(1, 2).reshape(B, nseg, H, W)
    labels = (tgt[:, :-1] - SEG0).reshape(B, H, W)
    for smooth, w in ((1.0, None), (1.0, cw.double()), (0.25, cw.double())):
        got = dice_loss_reference(scores, tgt, SEG0, nseg, smooth, w)
        want = DC.upstream_dice_loss(pred, labels, smooth=smooth, exponent=2, class_weight=w)
        assert got.dtype == torch.float64 and 0.0 < float(want) < 2.0     # the class weights reach 2
        assert abs(float(got) - float(want)) <= 1e-13 * float(want), (float(got), float(want))
    # with ignored pixels the two differ (upstream masks the numerator only): the README says so, this shows it
    lp, tgt, cw = DC.dice_inputs(nseg, B, hp, wp)
    clean = DC.clean_target(tgt, nseg)
    lab = torch.where(clean[:, :-1] == SEG0 + nseg, torch.full_like(clean[:, :-1], 255), clean[:, :-1] - SEG0)
    lab = torch.where(clean[:, :-1] == 1, torch.full_like(lab, 255), lab).reshape(B, H, W)
    ours = dice_loss_reference(scores, tgt, SEG0, nseg)
    assert abs(float(ours) - float(DC.upstream_dice_loss(pred, lab))) > 1e-6


@pytest.mark.parametrize("nseg,B,hp,wp", [(5, 2, 3, 4), (17, 2, 3, 4), (15, 3, 1, 1)])
def test_closed_form_gradient_is_autograd(nseg, B, hp, wp):
    """the kernel's arithmetic (a_bc, e_bc, S_i) in fp64 against autograd of the rule: the entries are below 1e-2, so 1e-15 is a
    few units of fp64 rounding"""
    from ifseg_amd.criterions.seg_criterion import dice_grad_closed_form, dice_loss_reference
    lp, tgt, cw = DC.dice_inputs(nseg, B, hp, wp)
    HW = 256 * hp * wp
    for smooth, w in ((1.0, None), (0.5, cw.double())):
        scores = DC._scores(lp, nseg, hp, wp, torch.float64).requires_grad_(True)
        dice_loss_reference(scores, tgt, SEG0, nseg, smooth, w).backward()
        got = dice_grad_closed_form(scores, tgt, SEG0, nseg, smooth, w)
        assert tuple(got.shape) == (B, HW, nseg) and float(scores.grad.abs().max()) > 0.0
        err = float((got - scores.grad[:, :HW]).abs().max())
        assert err <= 1e-15, err
        assert float(scores.grad[:, HW:].abs().max()) == 0.0
        assert float(got[~DC.valid_mask(tgt, nseg)].abs().max()) == 0.0


def test_sums_are_per_sample_and_skip_the_eos_row():
    from ifseg_amd.criterions.seg_criterion import dice_sums_reference
    nseg, B, hp, wp = 5, 2, 3, 4
    lp, tgt, _ = DC.dice_inputs(nseg, B, hp, wp)
    scores = DC._scores(lp, nseg, hp, wp, torch.float32)
    s = dice_sums_reference(scores, tgt, SEG0, nseg)
    assert s.dtype == torch.float32 and tuple(s.shape) == (B, 3, nseg)
    assert dice_sums_reference(scores.double(), tgt, SEG0, nseg).dtype == torch.float64
    assert torch.equal(dice_sums_reference(scores[:, :-1], tgt, SEG0, nseg), s)
    assert torch.equal(dice_sums_reference(scores, tgt[:, :-1], SEG0, nseg), s)
    for b in range(B):
        assert torch.equal(dice_sums_reference(scores[b:b + 1], tgt[b:b + 1], SEG0, nseg)[0], s[b])
    valid = DC.valid_mask(tgt, nseg)
    assert torch.equal(s[:, 2].sum(1).long(), valid.sum(1))
    gone = int((s[1, 2] == 0).nonzero()[0])
    assert float(s[0, 2, gone]) > 0.0 and float(s[1, 0, gone]) == 0.0 and float(s[1, 1, gone]) > 0.0


def test_a_sample_without_a_valid_pixel_gives_zero():
    from ifseg_amd.criterions.seg_criterion import dice_loss_reference, dice_sums_reference
    nseg, B, hp, wp = 15, 3, 1, 1
    lp, tgt, cw = DC.dice_inputs(nseg, B, hp, wp)
    scores = DC._scores(lp[2:], nseg, hp, wp, torch.float64).requires_grad_(True)
    loss = dice_loss_reference(scores, tgt[2:], SEG0, nseg, 1.0, cw)
    loss.backward()
    assert float(loss.detach()) == 0.0 and float(scores.grad.abs().max()) == 0.0
    assert float(dice_sums_reference(scores, tgt[2:], SEG0, nseg).abs().max()) == 0.0
    # in the batch it contributes nothing but the 1 / B
    full = dice_loss_reference(DC._scores(lp, nseg, hp, wp, torch.float64), tgt, SEG0, nseg, 1.0, cw)
    two = dice_loss_reference(DC._scores(lp[:2], nseg, hp, wp, torch.float64), tgt[:2], SEG0, nseg, 1.0, cw)
    assert abs(float(full) - float(two) * 2 / 3) <= 1e-15


def _net_output(nseg, B, hp, wp):
    lp, tgt, cw = DC.dice_inputs(nseg, B, hp, wp)
    tgt = DC.clean_target(tgt, nseg)
    H, W = 16 * hp, 16 * wp
    extra = {"encoder_returns": {"image_embed_shape": [(hp, wp)]}}
    sample = {"target": tgt, "net_input": {"patch_images": torch.zeros(B, 3, H, W)}, "ntokens": 1, "nsentences": B}
    return (lp[:, :, :nseg].float(), extra), sample, cw


def test_criterion_reference_path_and_the_default():
    from ifseg_amd.criterions import SegCriterion
    from ifseg_amd.criterions.seg_criterion import dice_loss_reference, dice_sums_reference
    nseg, B, hp, wp = 17, 2, 3, 4
    H, W = 16 * hp, 16 * wp
    net_output, sample, cw = _net_output(nseg, B, hp, wp)
    scores = SegCriterion.upsample_logits(net_output[0], hp, wp, H, W)
    tgt = sample["target"]
    mask = (tgt == 1) | (tgt == SEG0 + nseg) | (tgt == 2)
    plain = torch.nn.functional.cross_entropy(scores[~mask], tgt[~mask] - SEG0)
    # dice_weight=None: what compute_loss_torch and reduce_metrics return today -- same keys, same bits
    base = SegCriterion(num_seg_tokens=nseg, **KW)
    assert base.dice_weight is None and base.dice_sums is None
    loss0, metrics0, one = base.compute_loss_torch(TRAINING, net_output, sample, 0)
    assert torch.equal(loss0, plain) and one == 1 and base.dice_sums is None
    assert sorted(metrics0) == ["area_intersect", "area_label", "area_pred_label", "area_union", "nll_loss"]
    assert torch.equal(metrics0["nll_loss"], plain)
    log0 = dict({"loss": loss0, "imfree_loss": loss0 * 0, "seg_loss": loss0, "ntokens": 1, "nsentences": B, "sample_size": 1}, **metrics0)
    red0 = SegCriterion.reduce_metrics([log0, log0])
    assert sorted(red0) == ["aAcc", "imfree_loss", "loss", "mAcc", "mIoU", "nll_loss", "nsentences", "ntokens", "sample_size", "seg_loss"]
    assert red0["loss"] == float(plain + plain) / 2 and red0["nll_loss"] == red0["loss"]
    # dice_weight=3: CE + 3 Dice, nll_loss stays the CE term
    crit = SegCriterion(num_seg_tokens=nseg, dice_weight=3, dice_smooth=0.5, dice_class_weight=cw.tolist(), **KW)
    loss, metrics, _ = crit.compute_loss_torch(TRAINING, net_output, sample, 0)
    dice = 3.0 * dice_loss_reference(scores[:, :H * W], tgt, SEG0, nseg, 0.5, cw)
    assert torch.equal(metrics["nll_loss"], plain) and torch.equal(metrics["dice_loss"], dice) and torch.equal(loss, plain + dice)
    assert float(dice) > 0.0 and torch.equal(crit.dice_sums, dice_sums_reference(scores, tgt, SEG0, nseg))
    assert sorted(set(metrics) - set(metrics0)) == ["dice_loss"]
    for k in metrics0:
        assert torch.equal(metrics[k], metrics0[k]), k
    log = dict(log0, loss=loss, seg_loss=loss, **metrics)
    red = SegCriterion.reduce_metrics([log, log])
    assert sorted(set(red) - set(red0)) == ["dice_loss"] and abs(red["dice_loss"] - float(dice)) < 1e-6
    assert all(red[k] == red0[k] for k in red0 if k not in ("loss", "seg_loss"))
    # composes with the CE options: the Dice term does not see the pixel weights
    pw = DC.pixel_plane(B, H * W)
    both = SegCriterion(num_seg_tokens=nseg, dice_weight=3.0, dice_smooth=0.5, dice_class_weight=cw, class_weight=cw, weight_norm="pixels", **KW)
    only = SegCriterion(num_seg_tokens=nseg, class_weight=cw, weight_norm="pixels", **KW)
    lb, mb, _ = both.compute_loss_torch(TRAINING, net_output, dict(sample, target_weight=pw), 0)
    lo, _, _ = only.compute_loss_torch(TRAINING, net_output, dict(sample, target_weight=pw), 0)
    assert torch.equal(mb["nll_loss"], lo) and torch.equal(mb["dice_loss"], dice) and torch.equal(lb, lo + dice)


def test_refusals():
    from ifseg_amd import hip
    from ifseg_amd.criterions import SegCriterion
    from ifseg_amd.criterions.seg_criterion import dice_loss_reference, dice_sums_reference
    kw = dict(num_seg_tokens=5, **KW)
    for bad in (0, -1.0, float("nan"), float("inf"), "3", True):
        with pytest.raises(ValueError, match="dice_weight"):
            SegCriterion(dice_weight=bad, **kw)
        with pytest.raises(ValueError, match="dice_weight"):
            hip.check_dice(bad, 1.0)
    for bad in (0, -1.0, float("nan"), float("inf"), "1", None):
        with pytest.raises(ValueError, match="dice_smooth"):
            SegCriterion(dice_weight=3.0, dice_smooth=bad, **kw)
        with pytest.raises(ValueError, match="dice_smooth"):
            SegCriterion(dice_smooth=bad, **kw)
        with pytest.raises(ValueError, match="dice_smooth"):
            dice_loss_reference(torch.zeros(1, 4, 5), torch.full((1, 4), SEG0), SEG0, 5, smooth=bad)
    for bad in ([1.0] * 4, [1.0, -1.0, 1.0, 1.0, 1.0], [float("nan")] * 5):
        with pytest.raises(ValueError, match="class_weight"):
            SegCriterion(dice_weight=3.0, dice_class_weight=bad, **kw)
    with pytest.raises(ValueError, match="scores_up"):
        dice_sums_reference(torch.zeros(1, 4, 6), torch.full((1, 4), SEG0), SEG0, 5)
    with pytest.raises(ValueError, match="target"):
        dice_sums_reference(torch.zeros(1, 4, 5), torch.full((1, 7), SEG0), SEG0, 5)
    c = SegCriterion(dice_weight=3, dice_smooth=2, dice_class_weight=[1, 0, 2, 1, 1], **kw)
    assert c.dice_weight == 3.0 and c.dice_smooth == 2.0 and c.dice_class_weight.dtype == torch.float32
    d = SegCriterion(**kw)
    assert d.dice_weight is None and d.dice_smooth == 1.0 and d.dice_class_weight is None


def test_abi_declares_and_exports_the_entry_points():
    from ifseg_amd import hip
    hdr = open(os.path.join(ROOT, "include", "ifseg_hip.h")).read()
    names = set(re.findall(r"\bint\s+(ifseg_\w+)\s*\(", hdr))
    new = {"ifseg_seg_dice_sums", "ifseg_seg_dice_tiles", "ifseg_seg_loss_gather_sum"}
    assert new <= names
    assert int(re.search(r"#define IFSEG_ABI_VERSION (\d+)", hdr).group(1)) == 21 == hip.ABI_VERSION
    if not os.path.exists(hip.LIB_PATH):
        from ifseg_amd.build import build
        build(verbose=False)
    lib = hip.lib()
    assert all(hasattr(lib, n) for n in new)
    lib.ifseg_abi_version.restype = ctypes.c_int
    assert lib.ifseg_abi_version() == 21


def test_op_has_a_fake_kernel():
    import ifseg_amd.ops  # noqa: F401
    B, hp, wp, nseg = 2, 3, 4, 15
    H, W = 16 * hp, 16 * wp
    logits = torch.empty(B, hp * wp + 1, nseg, dtype=torch.bfloat16, device="meta")
    tgt = torch.empty(B, H * W + 1, dtype=torch.int64, device="meta")
    cw = torch.empty(nseg, device="meta")
    for w in (None, cw):
        loss, sums, dl = torch.ops.ifseg.seg_dice(logits, tgt, w, hp, wp, H, W, SEG0, 3.0, 1.0)
        assert loss.dtype == torch.float32 and tuple(loss.shape) == () and loss.device.type == "meta"
        assert sums.dtype == torch.float32 and tuple(sums.shape) == (B, 3, nseg)
        assert dl.dtype == torch.bfloat16 and tuple(dl.shape) == (B, hp * wp + 1, 16)
    with pytest.raises(ValueError, match="dice_weight"):
        torch.ops.ifseg.seg_dice(logits, tgt, None, hp, wp, H, W, SEG0, 0.0, 1.0)
    with pytest.raises(ValueError, match="dice_smooth"):
        torch.ops.ifseg.seg_dice(logits, tgt, None, hp, wp, H, W, SEG0, 3.0, -1.0)
    with pytest.raises(ValueError, match="class_weight"):
        torch.ops.ifseg.seg_dice(logits, tgt, cw[:-1], hp, wp, H, W, SEG0, 3.0, 1.0)
    with pytest.raises(ValueError, match="x16"):
        torch.ops.ifseg.seg_dice(logits, tgt, None, hp, wp, H + 16, W, SEG0, 3.0, 1.0)
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.ifseg.seg_dice(torch.zeros(B, hp * wp + 1, nseg, dtype=torch.bfloat16), torch.zeros(B, H * W + 1, dtype=torch.int64),
                                 None, hp, wp, H, W, SEG0, 3.0, 1.0)
