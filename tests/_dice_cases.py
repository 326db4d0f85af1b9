"""Shared cases of the Dice tests (test_dice_cpu.py, test_dice_gpu.py): the logits / targets of `_ohem_cases.hard_inputs` with what
a per-sample loss has to get right added and asserted, a literal transcription of the upstream loss's lines, and the
specifications' values in fp32 and fp64.  Everything is made on the host, once per shape (lru_cache); nobody writes to what these
functions return."""
import functools

import torch

import _ohem_cases as OC

SEG0 = OC.SEG0

# (n, B, hp, wp): smallest class count; small, unaligned; one class past a chunk of 16; the 150-class configuration; the LDS
# maximum; interior cells with all nine partials; a single cell, every tap clamped (and B = 3); many tiles per sample
SHAPES = [(2, 2, 3, 4), (5, 2, 3, 4), (17, 2, 3, 4), (150, 1, 2, 3), (512, 1, 2, 3), (171, 1, 4, 6), (15, 3, 1, 1), (15, 2, 8, 8)]


@functools.lru_cache(maxsize=None)
def dice_inputs(nseg, B, hp, wp):
    """`_ohem_cases.hard_inputs` (bf16 logits at scale 2, the ignore label among the targets, a pad, a below-range and an
    above-range target poisoned in) plus: for B >= 2 a class present in sample 0 and absent from sample 1 (batch-wide sums taken
    for per-sample ones), for B = 3 a last sample whose targets are all the ignore label, and a class weight vector with one
    zero -> (logits_pad bf16 [B, P+1, npad], target int64 [B, H*W+1], class_weight fp32 [n]).  All of it is asserted here."""
    lp, tgt = OC.hard_inputs(nseg, B, hp, wp)
    tgt = tgt.clone()
    HW = 256 * hp * wp
    body = tgt[:, :HW]
    gone = None
    if B >= 2:
        gone = int(body[0][(body[0] >= SEG0) & (body[0] < SEG0 + nseg)][0]) - SEG0      # a class sample 0 certainly has
        body[1][body[1] == SEG0 + gone] = SEG0 + (gone + 1) % nseg
    if B == 3:
        body[2] = SEG0 + nseg
        body[0, HW - 7] = SEG0 + nseg + 5                                    # the above-range target sat in the last sample
    g = torch.Generator().manual_seed(11 + nseg)
    cw = torch.rand(nseg, generator=g) * 1.5 + 0.5
    cw[nseg // 2] = 0.0
    # the properties the tests rely on
    assert bool((body == 1).any()) and bool(((body < SEG0) & (body > 2)).any()) and bool((body > SEG0 + nseg).any())
    assert bool((body == SEG0 + nseg).any()) and bool((tgt[:, HW] == 2).all())
    if B >= 2:
        assert bool((body[0] == SEG0 + gone).any()) and not bool((body[1] == SEG0 + gone).any())
        assert bool(((body[1] >= SEG0) & (body[1] < SEG0 + nseg)).any())
    if B == 3:
        assert bool((body[2] == SEG0 + nseg).all())
    assert int((cw == 0).sum()) == 1 and bool((cw >= 0).all())
    return lp, tgt, cw


def valid_mask(tgt, nseg):
    body = tgt[:, :-1]
    return (body >= SEG0) & (body < SEG0 + nseg)


def clean_target(tgt, nseg):
    """the out-of-range labels (the kernels drop and flag them; F.cross_entropy raises on them) turned into the ignore label"""
    t = tgt.clone()
    t[(t < SEG0) & (t > 2)] = SEG0 + nseg
    t[t > SEG0 + nseg] = SEG0 + nseg
    return t


def _scores(lp, nseg, hp, wp, dtype):
    from ifseg_amd.criterions import SegCriterion
    return SegCriterion.upsample_logits(lp[:, :, :nseg].to(dtype), hp, wp, 16 * hp, 16 * wp)


@functools.lru_cache(maxsize=None)
def sums_specs(nseg, B, hp, wp):
    """-> (fp32 specification [B, 3, n], fp64 one, N_b = valid pixels per sample int64 [B], e_pix = max |fp32 - fp64| over the
    softmax probabilities (every class) of the case's valid pixels)"""
    from ifseg_amd.criterions.seg_criterion import dice_sums_reference
    lp, tgt, _ = dice_inputs(nseg, B, hp, wp)
    s32, s64 = _scores(lp, nseg, hp, wp, torch.float32), _scores(lp, nseg, hp, wp, torch.float64)
    valid = valid_mask(tgt, nseg)
    p32, p64 = torch.softmax(s32[:, :-1], -1), torch.softmax(s64[:, :-1], -1)
    e_pix = float((p32.double() - p64)[valid].abs().max())
    return dice_sums_reference(s32, tgt, SEG0, nseg), dice_sums_reference(s64, tgt, SEG0, nseg), valid.sum(1), e_pix


@functools.lru_cache(maxsize=None)
def dice_reference(nseg, B, hp, wp, use_cw, dice_weight=3.0, smooth=1.0):
    """dice_weight * `dice_loss_reference` on `upsample_logits` in fp32 with autograd -> (loss [], d loss / d logits [B, P+1, n])"""
    from ifseg_amd.criterions.seg_criterion import dice_loss_reference
    lp, tgt, cw = dice_inputs(nseg, B, hp, wp)
    lf = lp[:, :, :nseg].float().clone().requires_grad_(True)
    from ifseg_amd.criterions import SegCriterion
    scores = SegCriterion.upsample_logits(lf, hp, wp, 16 * hp, 16 * wp)
    loss = dice_weight * dice_loss_reference(scores, tgt, SEG0, nseg, smooth, cw if use_cw else None)
    loss.backward()
    return loss.detach(), lf.grad.detach()


def pixel_plane(B, HW, seed=5):
    return OC.weight_plane(B, HW, seed)


@functools.lru_cache(maxsize=None)
def combined_reference(nseg, B, hp, wp, weighted, dice_weight=3.0, smooth=1.0):
    """CE reference + Dice reference in fp32 with autograd.  weighted: CE with the case's class weights, `pixel_plane` and
    weight_norm="pixels"; else the plain mean.  The Dice term carries the class weights in both.
    -> (total, ce, dice, d total / d logits [B, P+1, n])"""
    from ifseg_amd.criterions import SegCriterion
    from ifseg_amd.criterions.seg_criterion import dice_loss_reference, weighted_loss_reference
    lp, tgt, cw = dice_inputs(nseg, B, hp, wp)
    H, W = 16 * hp, 16 * wp
    lf = lp[:, :, :nseg].float().clone().requires_grad_(True)
    scores = SegCriterion.upsample_logits(lf, hp, wp, H, W)
    clean = clean_target(tgt, nseg)
    if weighted:
        ce = weighted_loss_reference(scores, clean, SEG0, nseg, cw, pixel_plane(B, H * W), 0.0, "pixels")
    else:
        ce = weighted_loss_reference(scores, clean, SEG0, nseg)
    dice = dice_weight * dice_loss_reference(scores, tgt, SEG0, nseg, smooth, cw)
    total = ce + dice
    total.backward()
    return total.detach(), ce.detach(), dice.detach(), lf.grad.detach()


def upstream_dice_loss(pred, target, smooth=1, exponent=2, class_weight=None, ignore_index=255, loss_weight=1.0):
    """The lines of mmseg 0.x's DiceLoss.forward / dice_loss / binary_dice_loss with reduction='mean', transcribed: pred [B, n, ...]
    logits, target int64 [B, ...] with `ignore_index` among the labels -> loss [].
        pred = F.softmax(pred, dim=1)
        one_hot_target = F.one_hot(torch.clamp(target.long(), 0, num_classes - 1), num_classes=num_classes)
        valid_mask = (target != ignore_index).long()
        for i in range(num_classes):
            if i != ignore_index:
                dice_loss = binary_dice_loss(pred[:, i], one_hot_target[..., i], valid_mask)      # mean over the batch
                if class_weight is not None: dice_loss *= class_weight[i]
                total_loss += dice_loss
        return loss_weight * total_loss / num_classes
    binary_dice_loss, per sample:
        num = torch.sum(torch.mul(pred, target) * valid_mask, dim=1) * 2 + smooth
        den = torch.sum(pred.pow(exponent) + target.pow(exponent), dim=1) + smooth
        return 1 - num / den"""
    import torch.nn.functional as F

    def binary_dice_loss(pred, target, valid_mask):
        assert pred.shape[0] == target.shape[0]
        pred = pred.reshape(pred.shape[0], -1)
        target = target.reshape(target.shape[0], -1)
        valid_mask = valid_mask.reshape(valid_mask.shape[0], -1)
        num = torch.sum(torch.mul(pred, target) * valid_mask, dim=1) * 2 + smooth
        den = torch.sum(pred.pow(exponent) + target.pow(exponent), dim=1) + smooth
        return (1 - num / den).mean()

    pred = F.softmax(pred, dim=1)
    num_classes = pred.shape[1]
    one_hot_target = F.one_hot(torch.clamp(target.long(), 0, num_classes - 1), num_classes=num_classes)
    valid_mask = (target != ignore_index).long()
    total_loss = 0
    for i in range(num_classes):
        if i != ignore_index:
            dice_loss = binary_dice_loss(pred[:, i], one_hot_target[..., i], valid_mask)
            if class_weight is not None:
                dice_loss = dice_loss * class_weight[i]
            total_loss = total_loss + dice_loss
    return loss_weight * total_loss / num_classes
