"""seg_criterion -- caller of the hot path (mirror of criterions/seg_criterion.py).

Supervised branch of the reference criterion (seg_criterion.py:188-192 ->
compute_loss :269-347 -> upsample_logits :237-244, compute_metric :349-362,
reduce_metrics mIoU :533-572): bilinear upsample of the per-patch logits to pixel
resolution, masked cross entropy, per-class area histograms.  ``sample_size`` is 1 per
rank (``ntokens = 1``, :345) exactly like the reference, so after the trainer's
``multiply_grads(world / sum(sample_size))`` the gradient is the mean over ranks.

The loss math is one fused HIP kernel pair (csrc/loss.hip: upsample + CE + gradient +
histograms) whenever the image is exactly 16x the feature grid and
label smoothing is off; otherwise the same math runs as stock PyTorch ops (eval on odd
image sizes).  ``compute_loss_torch`` is kept as the in-framework reference of the kernel.

Opt-in weights (self-training on pseudo-labels): ``SegCriterion(class_weight=, weight_norm=)`` and a sample's
``"target_weight"`` (uint8 per pixel) select the weighted instantiation of the same kernel; ``weighted_loss_reference``
states the rule.  Without them every call is the unweighted one.

Opt-in online hard example mining: ``SegCriterion(ohem_thresh=, ohem_min_kept=)`` builds that plane on the device
(csrc/ohem.hip: the probability of every pixel's own label, then an exact radix select over the batch);
``hardness_reference`` and ``ohem_reference`` state the rule.

Opt-in Dice auxiliary loss: ``SegCriterion(dice_weight=, dice_smooth=, dice_class_weight=)`` adds ``dice_weight`` times the
per-sample soft Dice loss of the same upsampled logits (csrc/dice.hip: two tile passes with a device-side reduction between
them, one gradient); ``dice_sums_reference`` and ``dice_loss_reference`` state the rule.  Without it every call is as before.

Opt-in distillation: ``SegCriterion(distill_weight=, distill_temperature=, distill_mask=)`` adds ``distill_weight`` times the
per-pixel KL divergence from a teacher's upsampled logits (the sample's ``"teacher_logits"``) to the student's, at a temperature
(csrc/distill.hip: one tile pass over both logits, one gradient); ``distill_loss_reference`` states the rule.  Without it every
call is as before.
"""
from dataclasses import dataclass, field
from typing import Optional

import torch
import torch.nn.functional as F

from .. import hip
from ..registry import CriterionBase, DataclassBase, register_criterion, str_bool


def _f(default, help=""):
    return field(default=default, metadata={"help": help})


@dataclass
class SegCriterionConfig(DataclassBase):
    """criterions/seg_criterion.py:32-101 (the 'true' / 'false' string flags included)."""
    label_smoothing: float = _f(0.0, "epsilon for label smoothing, 0 means no label smoothing")
    report_accuracy: bool = _f(False, "report accuracy metric")
    ignore_prefix_size: int = _f(0, "Ignore first N tokens")
    ignore_eos: bool = _f(True, "Ignore eos token")
    sentence_avg: bool = _f(False, "optimization.sentence_avg")
    drop_worst_ratio: float = _f(0.0, "ratio for discarding bad samples")
    drop_worst_after: int = _f(0, "steps for discarding bad samples")
    use_rdrop: bool = _f(False, "use R-Drop")
    reg_alpha: float = _f(1.0, "weight for R-Drop")
    sample_patch_num: int = _f(196, "sample patches for v1")
    constraint_range: Optional[str] = _f(None, "constraint range")
    upscale_lprobs: str = _f("true", "true | false")
    unsupervised_segmentation: str = _f("true", "true | false")
    criterion_update_freq: int = _f(1, "update frequency used in this criterion")
    freeze_embedding_iter: int = _f(-1, "Freeze the token embedding after this iteration (ignored if -1)")
    full_context_alignment: str = _f("false", "whether to apply full attention in decoder")
    init_seg_with_text: str = _f("true", "whether to lazy initialize the segmentation with text embedding bags")
    resnet_topk: int = _f(3, "filtering with topk adjacent resnet features")
    resnet_prob_temperature: float = _f(1.0, "resnet softmax temperature")
    resnet_iters: int = _f(0, "resnet filtering iterations")


PAD, EOS = 1, 2
WEIGHT_NORMS = ("weights", "pixels")


def check_weight_norm(weight_norm):
    if weight_norm not in WEIGHT_NORMS:
        raise ValueError("weight_norm must be one of %s, got %r" % (WEIGHT_NORMS, weight_norm))
    return weight_norm == "pixels"


def check_class_weight(class_weight, nseg):
    """-> fp32 (fp64 stays fp64) [nseg] on the device it was given on (or the CPU), or None.  Negative, NaN or infinite entries, another length:
    ValueError.  Reads the values: one host round trip for a device tensor, so callers check once, not per step."""
    if class_weight is None:
        return None
    cw = torch.as_tensor(class_weight)
    if cw.dtype == torch.bool or cw.dtype.is_complex or tuple(cw.shape) != (nseg,):
        raise ValueError("class_weight must be %d real numbers, got %s %s" % (nseg, cw.dtype, tuple(cw.shape)))
    cw = cw.detach()
    if cw.dtype != torch.float64:
        cw = cw.to(torch.float32)
    if not bool((torch.isfinite(cw) & (cw >= 0)).all()):
        raise ValueError("class_weight must be finite and non-negative (zeros allowed)")
    return cw.contiguous()


def check_pixel_weight(pixel_weight, B, npix):
    """the per-pixel weight plane: uint8 [B, npix], q in 0 .. 255 (ValueError otherwise); None passes"""
    if pixel_weight is None:
        return None
    if not torch.is_tensor(pixel_weight) or pixel_weight.dtype != torch.uint8 or tuple(pixel_weight.shape) != (B, npix):
        raise ValueError("pixel_weight must be uint8 [%d, %d], got %s" % (
            B, npix, (pixel_weight.dtype, tuple(pixel_weight.shape)) if torch.is_tensor(pixel_weight) else type(pixel_weight)))
    return pixel_weight


def weighted_loss_reference(scores_up, target, seg_id_offset, nseg, class_weight=None, pixel_weight=None, label_smoothing=0.0,
                            weight_norm="weights"):
    """Specification of the weighted fused criterion (csrc/loss.hip, ifseg_seg_loss_tiles_weighted), runs on any device and is
    differentiable in scores_up.  scores_up [B, H*W, n] (already upsampled; a trailing eos row is ignored), target int64
    [B, H*W (+1)], pixel_weight uint8 [B, H*W] (q_i in 0 .. 255; None: 1), class_weight fp32 [n] >= 0 (None: ones).
    A pixel is valid iff its target is a class (not pad / eos / <seg_n>: `compute_loss_torch`'s mask).  With
      l_i = F.cross_entropy(v_i, y_i, weight=cw, reduction="none", label_smoothing=eps)
          = (1 - eps) cw[y_i] (lse_i - v_i[y_i]) + (eps / n) sum_c cw[c] (lse_i - v_i[c]):
      loss = sum_valid q_i l_i / Z,   Z = sum_valid q_i cw[y_i]             weight_norm="weights": torch's weighted mean, so the
                                                                           loss does not depend on the scale of q
                                      Z = qmax N_valid, qmax = 255 | 1      weight_norm="pixels": with | without a plane; a batch
                                                                           of unsure pixels gives a smaller gradient
    and loss = 0 (with a zero gradient) when Z = 0."""
    norm_pixels = check_weight_norm(weight_norm)
    B, n = scores_up.shape[0], int(nseg)
    if scores_up.dim() != 3 or scores_up.shape[2] != n:
        raise ValueError("weighted_loss_reference: scores_up must be [B, H*W, %d], got %s" % (n, tuple(scores_up.shape)))
    npix = min(scores_up.shape[1], target.shape[1])
    if torch.is_tensor(pixel_weight) and pixel_weight.dim() == 2 and pixel_weight.shape[1] == npix - 1:
        npix -= 1                                   # scores and target both carry the eos row: the plane says so
    if target.dtype != torch.int64 or target.dim() != 2 or target.shape[0] != B or target.shape[1] - npix not in (0, 1) \
            or scores_up.shape[1] - npix not in (0, 1):
        raise ValueError("weighted_loss_reference: target must be int64 [B, H*W (+1)], got %s %s for scores %s"
                         % (target.dtype, tuple(target.shape), tuple(scores_up.shape)))
    check_pixel_weight(pixel_weight, B, npix)
    cw = check_class_weight(class_weight, n)
    dev, dt = scores_up.device, scores_up.dtype
    tgt = target[:, :npix].to(dev)
    mask = ~((tgt == PAD) | (tgt == seg_id_offset + n) | (tgt == EOS))
    s, t = scores_up[:, :npix][mask], tgt[mask] - seg_id_offset
    cw = cw.to(dev, dt) if cw is not None else None
    l = F.cross_entropy(s, t, weight=cw, reduction="none", label_smoothing=float(label_smoothing))
    q = pixel_weight.to(dev)[mask].to(dt) if pixel_weight is not None else torch.ones_like(l)
    if norm_pixels:
        Z = (255.0 if pixel_weight is not None else 1.0) * l.new_tensor(float(t.numel()))
    else:
        Z = (q * cw[t]).sum() if cw is not None else q.sum()
    num = (q * l).sum()
    return torch.where(Z > 0, num / torch.where(Z > 0, Z, torch.ones_like(Z)), num * 0.0)


OHEM_MIN_KEPT = 100000         # mmseg's default
OHEM_ONE_BITS = 0x3F800000     # the bits of 1.0f: the largest candidate


def check_ohem(thresh, min_kept=OHEM_MIN_KEPT):
    """the sampler's two numbers -> (thresh or None, min_kept).  thresh=None switches the sampler off; with a min_kept of its own
    that would be mmseg's loss-ranked variant, which is not built: ValueError, as thresh outside [0, 1] and a negative min_kept."""
    if thresh is None:
        if min_kept != OHEM_MIN_KEPT:
            raise ValueError("ohem_thresh=None with ohem_min_kept=%r: mmseg's loss-ranked OHEMPixelSampler (thresh=None) is not "
                             "built; give ohem_thresh" % (min_kept,))
        return None, OHEM_MIN_KEPT
    return hip.check_ohem(thresh, min_kept)


def check_dice(dice_weight, dice_smooth=1.0):
    """the Dice term's two numbers -> (dice_weight or None, dice_smooth).  dice_weight=None switches the term off; a number
    > 0 switches it on; dice_smooth is a number > 0 either way (a bad one is a mistake in the configuration whether or not the
    term is on).  Anything else: ValueError naming the keyword."""
    smooth = hip.check_dice_number("dice_smooth", dice_smooth, "seg_criterion")
    if dice_weight is None:
        return None, smooth
    return hip.check_dice_number("dice_weight", dice_weight, "seg_criterion"), smooth


def hardness_reference(scores_up, target, seg_id_offset, nseg):
    """Specification of `hip.seg_hardness` (csrc/ohem.hip), runs on any device.  scores_up fp32 or fp64 [B, H*W (+1), n] (already
    upsampled), target int64 [B, H*W (+1)] -> [B, H*W] in the dtype of the scores: softmax(scores_up)[y], clamped to <= 1, where
    the target is a class (seg_id_offset <= t < seg_id_offset + n and not pad / eos: the loss kernel's predicate), -1 elsewhere.
    A trailing row that scores and target both carry and whose targets are all eos is the eos row and is left out."""
    n = int(nseg)
    if scores_up.dim() != 3 or scores_up.shape[2] != n or not scores_up.dtype.is_floating_point:
        raise ValueError("hardness_reference: scores_up must be floating point [B, H*W, %d], got %s %s"
                         % (n, scores_up.dtype, tuple(scores_up.shape)))
    B = scores_up.shape[0]
    npix = min(scores_up.shape[1], target.shape[1]) if target.dim() == 2 else -1
    if target.dtype != torch.int64 or target.dim() != 2 or target.shape[0] != B or target.shape[1] - npix not in (0, 1) \
            or scores_up.shape[1] - npix not in (0, 1):
        raise ValueError("hardness_reference: target must be int64 [B, H*W (+1)], got %s %s for scores %s"
                         % (target.dtype, tuple(target.shape), tuple(scores_up.shape)))
    if target.shape[1] == scores_up.shape[1] and bool((target[:, -1] == EOS).all()):
        npix -= 1                                   # scores and target both carry the eos row
    s = scores_up.detach()[:, :npix]
    if s.dtype not in (torch.float32, torch.float64):
        s = s.float()
    tgt = target[:, :npix].to(s.device)
    valid = (tgt >= seg_id_offset) & (tgt < seg_id_offset + n) & (tgt != PAD) & (tgt != EOS)
    label = torch.where(valid, tgt - seg_id_offset, torch.zeros_like(tgt))
    p = torch.softmax(s, dim=-1).gather(2, label.unsqueeze(-1)).squeeze(-1).clamp(max=1.0)
    return torch.where(valid, p, torch.full_like(p, -1.0))


def ohem_reference(hardness, thresh, min_kept, weight=None):
    """Specification of `hip.ohem_select` (csrc/ohem.hip) -- mmseg's OHEMPixelSampler.sample with `thresh` given, restated from
    upstream's behaviour (sort, min(batch_kept, numel - 1), max, <) -- runs on any device.  hardness [B, N] (rounded to fp32),
    weight None or uint8 [B, N] -> (plane uint8 [B, N], info int64 [4]).  Integer from here on: a value is the uint32 bit
    pattern of its fp32, and an entry is a candidate iff bits <= 0x3F800000 (0 <= v <= 1 with the sign bit clear; -1, -0.0, NaN
    and anything above 1 are none).  With k = min(min_kept * B, #candidates - 1):
      kth = the k-th smallest candidate, counted from 0 (0 without a candidate),   tau = max(bits(fp32(thresh)), kth)
      plane = weight[i] (None: 255) where the entry is a candidate and bits < tau -- strictly, so the entries that tie with the
      k-th value are dropped -- and 0 elsewhere;   info = [#candidates, #kept, tau, kth]."""
    thresh, min_kept = hip.check_ohem(thresh, min_kept)
    if not torch.is_tensor(hardness) or hardness.dim() != 2 or not hardness.dtype.is_floating_point:
        raise ValueError("ohem_reference: hardness must be a floating-point [B, N] tensor")
    B, N = hardness.shape
    if weight is not None and (weight.dtype != torch.uint8 or tuple(weight.shape) != (B, N)):
        raise ValueError("ohem_reference: weight must be uint8 [%d, %d], got %s %s" % (B, N, weight.dtype, tuple(weight.shape)))
    dev = hardness.device
    bits = hardness.detach().to(torch.float32).contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    cand = bits <= OHEM_ONE_BITS
    tb = int(torch.tensor(thresh, dtype=torch.float32).view(torch.int32))
    nv = int(cand.sum())
    kth = int(bits[cand].sort().values[min(min_kept * B, nv - 1)]) if nv else 0
    tau = max(tb, kth)
    keep = cand & (bits < tau)
    full = weight.to(dev) if weight is not None else torch.full((B, N), 255, dtype=torch.uint8, device=dev)
    plane = torch.where(keep, full, torch.zeros_like(full))
    return plane, torch.tensor([nv, int(keep.sum()), tau, kth], dtype=torch.int64, device=dev)


def _dice_terms(scores_up, target, seg_id_offset, nseg, what):
    """-> (p [B, npix, n] with zeros on the invalid pixels, onehot of the same shape and dtype): the two factors of the sums"""
    n = int(nseg)
    if scores_up.dim() != 3 or scores_up.shape[2] != n or not scores_up.dtype.is_floating_point:
        raise ValueError("%s: scores_up must be floating point [B, H*W, %d], got %s %s"
                         % (what, n, scores_up.dtype, tuple(scores_up.shape)))
    B = scores_up.shape[0]
    npix = min(scores_up.shape[1], target.shape[1]) if target.dim() == 2 else -1
    if target.dtype != torch.int64 or target.dim() != 2 or target.shape[0] != B or target.shape[1] - npix not in (0, 1) \
            or scores_up.shape[1] - npix not in (0, 1):
        raise ValueError("%s: target must be int64 [B, H*W (+1)], got %s %s for scores %s"
                         % (what, target.dtype, tuple(target.shape), tuple(scores_up.shape)))
    if target.shape[1] == scores_up.shape[1] and bool((target[:, -1] == EOS).all()):
        npix -= 1                                   # scores and target both carry the eos row
    s = scores_up[:, :npix]
    if s.dtype not in (torch.float32, torch.float64):
        s = s.float()
    tgt = target[:, :npix].to(s.device)
    valid = (tgt >= seg_id_offset) & (tgt < seg_id_offset + n) & (tgt != PAD) & (tgt != EOS)
    label = torch.where(valid, tgt - seg_id_offset, torch.zeros_like(tgt))
    v = valid.unsqueeze(-1).to(s.dtype)
    return torch.softmax(s, dim=-1) * v, F.one_hot(label, n).to(s.dtype) * v


def dice_sums_reference(scores_up, target, seg_id_offset, nseg):
    """Specification of `hip.seg_dice_sums` (csrc/dice.hip, pass A and the reduction), runs on any device.  scores_up fp32 or fp64
    [B, H*W (+1), n] (already upsampled), target int64 [B, H*W (+1)] -> [B, 3, n] in the dtype of the scores.  A pixel is valid iff
    its target is a class (seg_id_offset <= t < seg_id_offset + n and not pad / eos: the loss kernel's predicate); with
    p_ic = softmax_c(v_i), over the valid pixels i of sample b only:
      [b, 0, c] = I_bc = sum_i p_ic [y_i = c]     [b, 1, c] = P_bc = sum_i p_ic^2     [b, 2, c] = Y_bc = sum_i [y_i = c]
    A trailing row that scores and target both carry and whose targets are all eos is the eos row and is left out."""
    p, onehot = _dice_terms(scores_up.detach(), target, seg_id_offset, nseg, "dice_sums_reference")
    return torch.stack([(p * onehot).sum(1), (p * p).sum(1), onehot.sum(1)], dim=1)


def dice_loss_reference(scores_up, target, seg_id_offset, nseg, smooth=1.0, class_weight=None):
    """Specification of the Dice term of the fused criterion (csrc/dice.hip; `hip.seg_dice` computes dice_weight times this and its
    gradient), unscaled, runs on any device and dtype and is differentiable in scores_up.  Inputs as `dice_sums_reference`;
    smooth = s > 0, class_weight fp32 / fp64 [n] >= 0 (None: ones).  With I, P, Y of `dice_sums_reference`:
      N_bc = 2 I_bc + s       Q_bc = P_bc + Y_bc + s
      L_dice = (1 / B) sum_b (1 / n) sum_c w_c (1 - N_bc / Q_bc)
    This is mmseg 0.x's DiceLoss(smooth=1, exponent=2) in form -- one binary_dice_loss per class, taken per sample, averaged over
    the batch, summed over the classes and divided by num_classes -- restated from upstream's behaviour (mmseg is no dependency:
    the rule is not checked against its code).  Upstream applies the valid mask to the numerator only and clamps ignored labels
    into class n - 1 in the denominator; this rule masks all three sums, so the two agree exactly only on samples without ignored
    pixels.  mmseg 1.x's flattened variant, exponent=1 and naive_dice are not built.
    A sample without a valid pixel has I = P = Y = 0: every class gives 1 - s / s = 0 with a zero gradient.  The sums run per
    sample, so under data parallelism the term needs no reduction across ranks: a rank's value is the mean over its own samples.
    Gradient in closed form (what the kernel computes), with k_c = w_c / (B n), a_bc = -2 k_c / Q_bc, e_bc = k_c N_bc / Q_bc^2:
      g_ic = a_bc [y_i = c] + 2 p_ic e_bc on a valid pixel,  S_i = sum_k p_ik g_ik,  d L_dice / d v_ic = p_ic (g_ic - S_i)."""
    if isinstance(smooth, bool) or not isinstance(smooth, (int, float)) or not 0 < smooth < float("inf"):
        raise ValueError("dice_loss_reference: dice_smooth must be a finite number > 0, got %r" % (smooth,))
    p, onehot = _dice_terms(scores_up, target, seg_id_offset, nseg, "dice_loss_reference")
    cw = check_class_weight(class_weight, int(nseg))
    num = 2.0 * (p * onehot).sum(1) + smooth
    den = (p * p).sum(1) + onehot.sum(1) + smooth
    per_class = 1.0 - num / den                                             # [B, n]
    if cw is not None:
        per_class = per_class * cw.to(p.device, p.dtype)
    return per_class.sum(1).div(int(nseg)).mean()


def dice_grad_closed_form(scores_up, target, seg_id_offset, nseg, smooth=1.0, class_weight=None):
    """d `dice_loss_reference` / d scores_up by the closed form of its docstring (the arithmetic of csrc/dice.hip's pass B), no
    autograd -> the shape of scores_up's pixel rows (the eos row, when carried, left out)"""
    p, onehot = _dice_terms(scores_up.detach(), target, seg_id_offset, nseg, "dice_grad_closed_form")
    B, n = p.shape[0], int(nseg)
    cw = check_class_weight(class_weight, n)
    k = (cw.to(p.device, p.dtype) if cw is not None else p.new_ones(n)) / (B * n)
    N = 2.0 * (p * onehot).sum(1) + smooth
    Q = (p * p).sum(1) + onehot.sum(1) + smooth
    a, e = (-2.0 * k / Q).unsqueeze(1), (k * N / (Q * Q)).unsqueeze(1)      # [B, 1, n]
    g = a * onehot + 2.0 * p * e                                            # zero where p and onehot are (invalid pixels)
    return p * (g - (p * g).sum(-1, keepdim=True))


def check_distill(distill_weight, distill_temperature=1.0, distill_mask="valid"):
    """the distillation term's three settings -> (distill_weight or None, temperature, mask).  distill_weight=None switches the
    term off; the temperature (a finite number > 0) and the mask ("valid" | "all") are checked either way.  Anything else:
    ValueError naming the keyword."""
    w, T, _ = hip.check_distill(distill_weight, distill_temperature, distill_mask, "seg_criterion")
    return w, T, distill_mask


def _distill_terms(scores_up, teacher_up, target, seg_id_offset, nseg, temperature, mask, what):
    """-> (p, q [B, npix, n], m bool [B, npix], T): the two tempered softmaxes and the mask M of the rule"""
    _, T, mask_all = hip.check_distill(None, temperature, mask, what)
    n = int(nseg)
    for nm, x in (("scores_up", scores_up), ("teacher_up", teacher_up)):
        if not torch.is_tensor(x) or x.dim() != 3 or x.shape[2] != n or not x.dtype.is_floating_point:
            raise ValueError("%s: %s must be floating point [B, H*W, %d], got %s" % (
                what, nm, n, (x.dtype, tuple(x.shape)) if torch.is_tensor(x) else type(x)))
    B = scores_up.shape[0]
    if target is None:
        if not mask_all:
            raise ValueError("%s: distill_mask=\"valid\" needs the target" % what)
        npix = scores_up.shape[1]                    # every row is a pixel: the caller leaves the eos row out
    else:
        npix = min(scores_up.shape[1], target.shape[1]) if target.dim() == 2 else -1
        if target.dtype != torch.int64 or target.dim() != 2 or target.shape[0] != B or target.shape[1] - npix not in (0, 1) \
                or scores_up.shape[1] - npix not in (0, 1):
            raise ValueError("%s: target must be int64 [B, H*W (+1)], got %s %s for scores %s"
                             % (what, target.dtype, tuple(target.shape), tuple(scores_up.shape)))
        if target.shape[1] == scores_up.shape[1] and bool((target[:, -1] == EOS).all()):
            npix -= 1                                   # scores and target both carry the eos row
    if teacher_up.shape[0] != B or teacher_up.shape[1] - npix not in (0, 1) or teacher_up.device != scores_up.device:
        raise ValueError("%s: teacher_up must be [%d, %d (+1), %d] on %s, got %s on %s"
                         % (what, B, npix, n, scores_up.device, tuple(teacher_up.shape), teacher_up.device))
    s = scores_up[:, :npix]
    if s.dtype not in (torch.float32, torch.float64):
        s = s.float()
    t = teacher_up.detach()[:, :npix].to(s.dtype)
    if mask_all:
        m = torch.ones(B, npix, dtype=torch.bool, device=s.device)
    else:
        tgt = target[:, :npix].to(s.device)
        m = (tgt >= seg_id_offset) & (tgt < seg_id_offset + n) & (tgt != PAD) & (tgt != EOS)
    return s / T, t / T, m, T


def distill_sums_reference(scores_up, teacher_up, target, seg_id_offset, nseg, temperature=1.0, mask="valid"):
    """-> ([sum_{i in M} KL(q_i || p_i), N = |M|] in the dtype of the scores, differentiable in scores_up): the two numbers
    `distill_loss_reference` is made of, and what `hip.seg_distill` leaves in bufs["kd_stats"]"""
    s, t, m, _ = _distill_terms(scores_up, teacher_up, target, seg_id_offset, nseg, temperature, mask, "distill_sums_reference")
    kl = F.kl_div(F.log_softmax(s, dim=-1), F.softmax(t, dim=-1), reduction="none").sum(-1)
    return torch.stack([torch.where(m, kl, torch.zeros_like(kl)).sum(), m.sum().to(kl.dtype)])


def distill_loss_reference(scores_up, teacher_up, target, seg_id_offset, nseg, temperature=1.0, mask="valid"):
    """Specification of the distillation term of the fused criterion (csrc/distill.hip; `hip.seg_distill` computes distill_weight
    times this and its gradient), unscaled, runs on any device and dtype and is differentiable in scores_up only.  scores_up /
    teacher_up fp32 or fp64 [B, H*W (+1), n] (already upsampled: `SegCriterion.upsample_logits` of the student's and the teacher's
    per-patch logits), target int64 [B, H*W (+1)] (None with mask="all": every row of the scores is then a pixel).  With
    p_i = softmax(s_i / T), q_i = softmax(t_i / T):
      L_kd = T^2 (1 / N) sum_{i in M} sum_c q_ic (log q_ic - log p_ic),   N = |M| over the WHOLE batch
    built on F.kl_div(log_softmax(s / T), softmax(t / T)).  M is, with mask="valid", the pixels whose target is a class
    (seg_id_offset <= y < seg_id_offset + n and not pad / eos: the loss kernel's predicate); with mask="all" every pixel -- the
    usual choice on unlabelled or pseudo-labelled batches, a poisoned or out-of-range target is then irrelevant.  N = 0 gives
    exactly 0 with a zero gradient.  A trailing row that scores and target both carry and whose targets are all eos is the eos
    row and is left out.  With mask="all" this is mmrazor's KLDivergence(tau=T, reduction="batchmean") on [B, n, H, W] scores
    divided by H*W (its batchmean divides by B only); no other relation to upstream is claimed.
    Gradient in closed form (what the kernel computes, `distill_grad_closed_form`): d L_kd / d s_ic = (T / N) (p_ic - q_ic) on M."""
    T = hip.check_distill(None, temperature, mask, "distill_loss_reference")[1]
    kl_sum, N = distill_sums_reference(scores_up, teacher_up, target, seg_id_offset, nseg, temperature, mask)
    return (T * T) * kl_sum / N.clamp(min=1.0)


def distill_grad_closed_form(scores_up, teacher_up, target, seg_id_offset, nseg, temperature=1.0, mask="valid"):
    """d `distill_loss_reference` / d scores_up by the closed form of its docstring (the arithmetic of csrc/distill.hip and its
    gather), no autograd -> the shape of scores_up's pixel rows (the eos row, when carried, left out)"""
    s, t, m, T = _distill_terms(scores_up.detach(), teacher_up, target, seg_id_offset, nseg, temperature, mask,
                                "distill_grad_closed_form")
    N = m.sum().to(s.dtype).clamp(min=1.0)
    return (torch.softmax(s, dim=-1) - torch.softmax(t, dim=-1)) * m.unsqueeze(-1).to(s.dtype) * (T / N)


class _FusedSegLossFn(torch.autograd.Function):
    """loss = mean CE(bilinear_x16(logits[:, :P]), target) (+ dice_weight * Dice) (+ distill_weight * KD) of the same upsampled
    logits; backward hands out the gradient the forward kernels already produced.  pixel_weight / class_weight / norm_pixels: the
    weighted CE kernel (`weighted_loss_reference`); all of them None / False: the unweighted launch, as before they existed.
    dice = (dice_weight, dice_smooth, dice_class_weight) adds csrc/dice.hip's two passes (`hip.seg_loss_dice`),
    kd = (teacher_pad, distill_weight, temperature, mask) csrc/distill.hip's tile pass (`hip.seg_loss_distill`); one gather sums
    the gradients.  -> (total, CE, weighted Dice, weighted KD, stats), None for a term that is absent (CE too when it is the
    total); only the total is differentiable, and only in the student."""

    @staticmethod
    def forward(ctx, logits, logits_pad, target, hp, wp, H, W, nseg, seg0, bufs, eps=0.0, pixel_weight=None,
                class_weight=None, norm_pixels=False, dice=None, kd=None):
        B = logits_pad.shape[0]
        dev = logits_pad.device
        key = (B, hp, wp, nseg, logits_pad.shape[2], dev, dice is not None, kd is not None)
        fresh = bufs.get("key") != key
        if fresh:
            bufs.clear()
            bufs["key"] = key
        weights = dict(pixel_weight=pixel_weight, class_weight=class_weight, norm_pixels=norm_pixels, label_smoothing=float(eps))
        ce = dice_loss = kd_loss = None
        if kd is not None:
            dw, ds, dcw = dice if dice is not None else (None, 1.0, None)
            loss4, dl = hip.seg_loss_distill(logits_pad, kd[0], target, hp, wp, H, W, nseg, seg0, kd[1], kd[2], kd[3], dice_weight=dw,
                                             dice_smooth=ds, dice_class_weight=dcw, bufs=bufs, **weights)
            total, ce, kd_loss = loss4[0].clone(), loss4[1].clone(), loss4[3].clone()
            if dice is not None:
                dice_loss = loss4[2].clone()
        elif dice is not None:
            loss3, dl = hip.seg_loss_dice(logits_pad, target, hp, wp, H, W, nseg, seg0, *dice, bufs=bufs, **weights)
            total, ce, dice_loss = loss3[0].clone(), loss3[1].clone(), loss3[2].clone()
        else:
            if fresh:
                n_tiles, nstat = B * hp * wp, 2 + 3 * nseg
                bufs["tile"] = torch.empty(n_tiles * 9 * nseg, dtype=torch.float32, device=dev)
                bufs["sp"] = torch.empty(n_tiles * nstat, dtype=torch.float32, device=dev)
                bufs["stats"] = torch.empty(nstat, dtype=torch.float32, device=dev)
                bufs["dl"] = torch.empty_like(logits_pad)
                bufs["loss"] = torch.empty(1, dtype=torch.float32, device=dev)
                bufs["bad"] = torch.zeros(1, dtype=torch.int32, device=dev)
            dl = bufs["dl"]
            args = (logits_pad, target, hp, wp, H, W, nseg, seg0, bufs["tile"], bufs["sp"], bufs["stats"], dl, bufs["loss"])
            if pixel_weight is None and class_weight is None and not norm_pixels:
                hip.seg_loss(*args, bad_label=bufs["bad"], label_smoothing=float(eps))
            else:
                hip.seg_loss_weighted(*args, bad_label=bufs["bad"], **weights)
            total = bufs["loss"][0].clone()
        ctx.dl = dl
        ctx.nseg = nseg
        # fresh tensors: callers keep them in logging outputs across calls (update_freq > 1, validation loops)
        out = (total, ce, dice_loss, kd_loss, bufs["stats"].clone())
        ctx.mark_non_differentiable(*(t for t in out[1:] if t is not None))
        return out

    @staticmethod
    def backward(ctx, gloss, *_):
        g = ctx.dl[:, :, : ctx.nseg]
        return (g * gloss.to(g.dtype),) + (None,) * 15


FUSED_MAX_CLASSES = 512      # csrc/loss.hip NS_MAX


@register_criterion("seg_criterion", dataclass=SegCriterionConfig)
class SegCriterion(CriterionBase):
    def __init__(self, task=None, sentence_avg=False, label_smoothing=0.0, ignore_prefix_size=0, ignore_eos=True,
                 report_accuracy=False, drop_worst_ratio=0, drop_worst_after=0, use_rdrop=False, reg_alpha=1.0,
                 sample_patch_num=196, constraint_range=None, upscale_lprobs="true", unsupervised_segmentation="true",
                 criterion_update_freq=1, freeze_embedding_iter=-1, full_context_alignment="false",
                 init_seg_with_text="true", resnet_topk=3, resnet_prob_temperature=1.0, resnet_iters=0,
                 num_seg_tokens=None, seg_id_offset=None, class_weight=None, weight_norm="weights", ohem_thresh=None,
                 ohem_min_kept=OHEM_MIN_KEPT, dice_weight=None, dice_smooth=1.0, dice_class_weight=None, distill_weight=None,
                 distill_temperature=1.0, distill_mask="valid"):
        """Signature of the reference (seg_criterion.py:115-161; fairseq's `build_criterion` fills it from
        SegCriterionConfig by name).  `num_seg_tokens` / `seg_id_offset` stand in for `task.cfg.num_seg_tokens` and
        `task.target_dictionary.index("<seg_0>")` when the criterion is used without a task.  `class_weight` (n numbers >= 0,
        F.cross_entropy's `weight`) and `weight_norm` ("weights" | "pixels": the normaliser of `weighted_loss_reference`) are
        constructor keywords only as well; a sample that carries `"target_weight"` (uint8 [B, H*W]) is weighted per pixel.
        `ohem_thresh` (0 .. 1) / `ohem_min_kept` (constructor keywords only): mmseg's `OHEMPixelSampler(thresh, min_kept)` on the
        supervised loss while the model trains -- `ohem_reference` states the rule; the kept pixels carry the sample's
        `target_weight` (or 255), the dropped ones 0, and the plane goes to the weighted kernel.  weight_norm="weights" is then the
        mean over the kept pixels, weight_norm="pixels" divides by 255 N_valid (mmseg's `avg_non_ignore=True` under a sampler).
        `self.ohem_info` holds the last call's int64 [4] on the device: valid pixels, kept pixels, the bits of tau and of the
        k-th value.  Not built: `ohem_thresh=None` with a min_kept (the loss-ranked sampler), OHEM in the image-free loss and in
        evaluation.
        `dice_weight` (> 0; None: off) / `dice_smooth` (> 0) / `dice_class_weight` (n numbers >= 0), constructor keywords only:
        mmseg's second decode loss, `DiceLoss(loss_weight=dice_weight, smooth=dice_smooth, class_weight=dice_class_weight)` --
        `dice_loss_reference` states the rule.  The returned loss is CE + dice_weight * Dice, `metrics["nll_loss"]` stays the CE
        term, `metrics["dice_loss"]` is the weighted Dice term and `self.dice_sums` holds the last call's fp32 [B, 3, n] on the
        device.  Pixel weights and the OHEM plane do not enter the Dice term.  It applies wherever `compute_loss` runs.  That
        includes the no-grad pass over the real images of image-free training (`unsupervised_segmentation`): there
        `seg_loss`, `nll_loss` and `dice_loss` are logged monitors of the real images and nothing of them is trained, as `seg_loss`
        and `nll_loss` always were in that mode; the trained image-free loss has no Dice term.  Not built: Dice in the image-free
        loss and in the `ori_semantic_seg` evaluation.
        `distill_weight` (> 0; None: off) / `distill_temperature` (> 0) / `distill_mask` ("valid" | "all"), constructor keywords
        only: distillation from a teacher's whole output -- `distill_loss_reference` states the rule.  The term is computed when
        the sample carries `"teacher_logits"`: bf16 [B, P+1, >= n] on the logits' device, the teacher's per-patch logits on the
        same grid and classes (`task.distill_sample` attaches them); anything else is a ValueError that names what differs.  The
        returned loss is CE (+ dice_weight * Dice) + distill_weight * KD, `metrics["kd_loss"]` is the weighted KD term and
        `self.distill_stats` holds the last call's fp32 [sum KL, N] on the device.  Pixel weights, class weights and the OHEM
        plane do not enter the term.  A supervised training call (`model.training`, gradients enabled) whose sample lacks the
        key is a ValueError; under `torch.no_grad()` and in evaluation a missing key just skips the term (the no-grad monitor
        pass of image-free training is such a case).  Not built: KD in the image-free loss and in the `ori_semantic_seg`
        evaluation."""
        super().__init__(task)
        self.sentence_avg = sentence_avg
        self.eps = label_smoothing
        self.sample_patch_num = sample_patch_num
        self.iter = -1
        self.effective_iter = -1
        self.criterion_update_freq = criterion_update_freq
        self.upscale_lprobs = str_bool(upscale_lprobs)
        self.unsupervised_segmentation = str_bool(unsupervised_segmentation)
        self.full_context_alignment = str_bool(full_context_alignment)
        self.init_seg_with_text = str_bool(init_seg_with_text)
        # eval-time top-k neighbour smoothing on the trunk features (seg_criterion.py:93-101,197-213)
        self.resnet_topk, self.resnet_prob_temperature, self.resnet_iters = resnet_topk, resnet_prob_temperature, resnet_iters
        cfg = getattr(task, "cfg", None)
        self.num_seg = num_seg_tokens if num_seg_tokens is not None else cfg.num_seg_tokens
        self.seg_id_offset = seg_id_offset if seg_id_offset is not None else task.target_dictionary.index("<seg_0>")
        cats = getattr(cfg, "category_list", "") or ""
        self.id2rawtext = [x.strip() for x in cats.split(",")] if cats else []
        if self.id2rawtext and len(self.id2rawtext) != self.num_seg:
            raise AssertionError("category_list names %d classes, num_seg_tokens is %d" % (len(self.id2rawtext), self.num_seg))
        self.padding_idx = PAD
        self.class_weight = check_class_weight(class_weight, self.num_seg)
        if self.class_weight is not None:
            self.class_weight = self.class_weight.float()          # what the kernel reads
        self.norm_pixels = check_weight_norm(weight_norm)
        self.weight_norm = weight_norm
        self.ohem_thresh, self.ohem_min_kept = check_ohem(ohem_thresh, ohem_min_kept)
        self.ohem_info = None
        self.dice_weight, self.dice_smooth = check_dice(dice_weight, dice_smooth)
        self.dice_class_weight = check_class_weight(dice_class_weight, self.num_seg)
        if self.dice_class_weight is not None:
            self.dice_class_weight = self.dice_class_weight.float()          # what the kernel reads
        self.dice_sums = None
        self.distill_weight, self.distill_temperature, self.distill_mask = check_distill(distill_weight, distill_temperature,
                                                                                         distill_mask)
        self.distill_stats = None
        # image-free samples drawn on the device (ifseg_amd/artificial.py).  The trainer sets the seed and, before every
        # micro-batch, the ordinal of its first sample (an int, or a device int64 word inside a captured step); without a
        # trainer the criterion counts the samples it has drawn.
        self.imfree_seed, self.imfree_first_ordinal = 1, None
        self._imfree_sampler, self._imfree_drawn = None, 0

    def _lazy_initialization(self, sample, model, ema_model=None):
        """seg_criterion.py:373-407: every <seg_i> embedding := mean token embedding of its category name
        (EmbeddingBag over the frozen token table), written into encoder/decoder.seg_embed_tokens (and the untied
        projection).  On the device: `ifseg_embed_bag_mean` on the bf16 token table of the engine's arena."""
        if not self.init_seg_with_text:
            return
        task = self.task
        ids = getattr(task, "category_token_ids", None)
        if ids is None:
            if not self.id2rawtext:
                raise RuntimeError("init_seg_with_text: the task carries neither category_list (+ BPE) nor category_token_ids")
            ids = [task.encode_category(" %s" % x) for x in self.id2rawtext]
        ids = [torch.as_tensor(x, dtype=torch.long).reshape(-1) for x in ids]
        if len(ids) != self.num_seg:
            raise AssertionError("%d category names for %d seg tokens" % (len(ids), self.num_seg))
        avg = model.seg_tokens_from_text(ids)
        model.encoder.seg_embed_tokens.weight.data = avg
        model.decoder.seg_embed_tokens.weight.data = avg
        if ema_model is not None:
            ema_model.encoder.seg_embed_tokens.weight.data = avg
            ema_model.decoder.seg_embed_tokens.weight.data = avg
        if not model.decoder.tie_seg_projection:
            model.decoder.seg_projection.weight.data = avg
            if ema_model is not None:
                ema_model.decoder.seg_projection.weight.data = avg

    def _artificial_sample(self, sample):
        """aux_input / text2seg_target of this batch from the device sampler; the prompt is the real image's prompt"""
        net = sample["net_input"]
        src = net["src_tokens"]
        if self._imfree_sampler is None:
            if self.task is None or not hasattr(self.task, "build_artificial_sampler"):
                raise RuntimeError("seg_criterion: the sample carries no aux_input and there is no task to build the "
                                   "artificial-image sampler from")
            self._imfree_sampler = self.task.build_artificial_sampler(src.device, seed=self.imfree_seed)
        B = src.shape[0]
        first = self.imfree_first_ordinal
        if first is None:
            first = self._imfree_drawn
            self._imfree_drawn += B
        return self._imfree_sampler.sample(B, first, src, net.get("src_lengths"))

    def forward(self, model, sample, update_num=0, reduce=True, ema_model=None):
        """seg_criterion.py:165-235 (lazy init on the first call, image-free / supervised train branches, eval branch)."""
        if self.iter == -1:
            self.iter = self.criterion_update_freq * update_num - 1
            self._lazy_initialization(sample, model, ema_model)
        self.iter += 1
        self.effective_iter = self.iter // self.criterion_update_freq
        if self.unsupervised_segmentation and model.training:
            # image-free training (seg_criterion.py:179-186): the loss comes from the artificial image; the real
            # images are only evaluated (no grad) for the logged metrics
            if getattr(getattr(self.task, "cfg", None), "artificial_image_on_device", False) or sample.get("aux_input") is None:
                sample = dict(sample, **self._artificial_sample(sample))
            net_output = model(full_context_alignment=self.full_context_alignment, aux_input=sample["aux_input"])
            imfree_loss = self.compute_imfree_loss(model, net_output[1]["aux_output"], sample, update_num, reduce=reduce)
            loss = imfree_loss
            with torch.no_grad():
                seg_output = model(**sample["net_input"], full_context_alignment=self.full_context_alignment)
                seg_loss, metrics, ntokens = self.compute_loss(model, seg_output, sample, update_num, reduce=reduce,
                                                               bufs_name="_bufs_metrics")
        elif not model.training and sample.get("ori_semantic_seg") is not None:
            # evaluation at the original image resolution (seg_criterion.py:194-217,289-347); batch 1 like the
            # reference (`ori_semantic_seg[0]`)
            with torch.no_grad():
                net_output = model(**sample["net_input"], full_context_alignment=self.full_context_alignment)
                seg_loss, metrics, ntokens = self.compute_loss_eval(model, net_output, sample)
            loss, imfree_loss = seg_loss, seg_loss.data.new_zeros(1)
        else:
            net_output = model(**sample["net_input"], full_context_alignment=self.full_context_alignment)
            seg_loss, metrics, ntokens = self.compute_loss(model, net_output, sample, update_num, reduce=reduce)
            loss, imfree_loss = seg_loss, seg_loss.data.new_zeros(1)
        sample_size = sample["target"].size(0) if self.sentence_avg else ntokens
        logging_output = {"loss": loss.data, "imfree_loss": imfree_loss.data, "seg_loss": seg_loss.data,
                          "ntokens": sample["ntokens"], "nsentences": sample["nsentences"],
                          "sample_size": sample_size}
        logging_output.update({k: (v.data if isinstance(v, torch.Tensor) else v) for k, v in metrics.items()})
        return loss, sample_size, logging_output

    @staticmethod
    def upsample_logits(logits, hp=32, wp=32, h=512, w=512):
        """seg_criterion.py:237-244 (mmseg.ops.resize == F.interpolate)."""
        lo = logits[:, :-1]
        B, _, n = lo.shape
        lo = lo.transpose(1, 2).reshape(B, n, hp, wp)
        lo = F.interpolate(lo, size=(h, w), mode="bilinear", align_corners=False)
        lo = lo.reshape(B, n, h * w).transpose(1, 2)
        return torch.cat([lo, logits[:, -1:]], dim=1)

    def compute_imfree_loss(self, model, net_output, sample, update_num, reduce=True):
        """seg_criterion.py:246-267: CE of the bilinear-upsampled (32x32 -> 512x512 in the reference; here the
        model's grid x16) logits of the artificial image against ``text2seg_target``; eos / pad / ignore dropped."""
        scores_low, extra = net_output
        target = sample["text2seg_target"]
        hp, wp = extra["encoder_returns"]["image_embed_shape"][0]
        h, w = 16 * hp, 16 * wp
        pad = extra.get("logits_padded")
        if (pad is not None and self.num_seg <= FUSED_MAX_CLASSES and target.shape[1] == h * w + 1):
            if not hasattr(self, "_bufs_imfree"):
                self._bufs_imfree = {}
            return _FusedSegLossFn.apply(scores_low, pad, target.contiguous(), hp, wp, h, w, self.num_seg,
                                         self.seg_id_offset, self._bufs_imfree, self.eps)[0]
        scores = self.upsample_logits(scores_low.float(), hp, wp, h, w)[:, :-1]
        tgt = target[:, :-1]
        scores = scores.reshape(-1, scores.shape[-1])
        tgt = tgt.reshape(-1)
        mask = (tgt != self.padding_idx) & (tgt != self.seg_id_offset + self.num_seg)
        return F.cross_entropy(scores[mask], tgt[mask] - self.seg_id_offset, label_smoothing=self.eps)

    def compute_loss_eval(self, model, net_output, sample):
        """compute_loss, ``not model.training`` (seg_criterion.py:289-347) + the top-k neighbour smoothing of
        :197-213: per-patch scores resized bilinearly to the ORIGINAL image shape, argmax, area histograms, display
        CE -- all on the device (csrc/evalops.hip), the [h*w, n] score tensor is never built."""
        scores_low, extra = net_output
        pad = extra["logits_padded"]
        hp, wp = extra["encoder_returns"]["image_embed_shape"][0]
        P, n, dev = hp * wp, self.num_seg, pad.device
        ori = sample["ori_semantic_seg"][0]
        ori = torch.as_tensor(ori)
        h, w = ori.shape[:2]
        target = ori.reshape(-1).long().to(dev) + self.seg_id_offset
        scores = hip.rows_to_f32(pad[:1], n, P)[0]
        loss, hist = hip.seg_eval(scores, hp, wp, target, h, w, self.seg_id_offset)
        f = lambda t: t.float()
        metrics = {"area_intersect": f(hist[0]), "area_pred_label": f(hist[1]), "area_label": f(hist[2]),
                   "area_union": f(hist[1] + hist[2] - hist[0]), "nll_loss": loss}
        if self.resnet_iters > 0:
            feat = extra["encoder_returns"]["image_embed_before_proj"][0]
            prob = hip.neighbour_smoothing(pad[:1], n, feat[:1], self.resnet_iters, self.resnet_topk,
                                           self.resnet_prob_temperature)
            extra["resnet_postprocess_probability"] = torch.cat([prob, prob.new_zeros(1, 1, n)], dim=1)
            _, hpp = hip.seg_eval(prob[0], hp, wp, target, h, w, self.seg_id_offset)
            metrics.update({"area_intersect_resnet_postprocess": f(hpp[0]), "area_pred_label_resnet_postprocess": f(hpp[1]),
                            "area_label_resnet_postprocess": f(hpp[2]),
                            "area_union_resnet_postprocess": f(hpp[1] + hpp[2] - hpp[0])})
        return loss, metrics, 1

    def compute_loss(self, model, net_output, sample, update_num, reduce=True, bufs_name="_bufs"):
        scores_low, extra = net_output
        target = sample["target"]
        hp, wp = extra["encoder_returns"]["image_embed_shape"][0]
        h, w = sample["net_input"]["patch_images"].shape[-2:]
        pad = extra.get("logits_padded")
        pw = check_pixel_weight(sample.get("target_weight"), target.shape[0], h * w)
        if (pad is not None and self.upscale_lprobs and h == 16 * hp and w == 16 * wp
                and self.num_seg <= FUSED_MAX_CLASSES and target.shape[1] == h * w + 1):
            if not hasattr(self, bufs_name):
                setattr(self, bufs_name, {})
            if self.ohem_thresh is not None and model.training:
                pw = self._ohem_plane(pad, target.contiguous(), pw, hp, wp, h, w, bufs_name + "_ohem")
            bufs = getattr(self, bufs_name)
            teacher = self._teacher_logits(model, sample, scores_low, hp * wp)
            weighted = pw is not None or self.class_weight is not None
            loss, ce, dice, kd, stats = _FusedSegLossFn.apply(
                scores_low, pad, target.contiguous(), hp, wp, h, w, self.num_seg, self.seg_id_offset, bufs, self.eps,
                pw.contiguous() if pw is not None else None, self._weight_on("class_weight", pad.device) if weighted else None,
                self.norm_pixels and weighted,
                None if self.dice_weight is None else (self.dice_weight, self.dice_smooth, self._weight_on("dice_class_weight", pad.device)),
                None if teacher is None else (teacher, self.distill_weight, self.distill_temperature, self.distill_mask))
            if kd is not None:
                self.distill_stats = bufs["kd_stats"]
            if dice is not None:
                self.dice_sums = bufs["dice_sums"]
            # the loss kernel flags labels that are neither a class nor pad / eos / ignore (read back without a sync)
            model.engine.deferred_check(
                bufs["bad"], lambda t: ((t[0] != 0).clone(), t.zero_())[0],
                "seg_criterion: target label outside [<seg_0>, <seg_%d>] (F.cross_entropy: target out of bounds)" % self.num_seg,
                exc=IndexError, native=(hip.CHECK_FLAG, 0, 1))
            n = self.num_seg
            ai, ap, al = stats[2:2 + n], stats[2 + n:2 + 2 * n], stats[2 + 2 * n:2 + 3 * n]
            metrics = {"area_intersect": ai, "area_pred_label": ap, "area_label": al, "area_union": ap + al - ai,
                       "nll_loss": loss}
            if dice is not None:
                metrics.update(nll_loss=ce, dice_loss=dice)
            if kd is not None:
                metrics.update(nll_loss=ce, kd_loss=kd)
            return loss, metrics, 1
        return self.compute_loss_torch(model, net_output, sample, update_num, reduce)

    def compute_loss_torch(self, model, net_output, sample, update_num, reduce=True):
        scores_low, extra = net_output
        scores_low = scores_low.float()
        target = sample["target"]
        hp, wp = extra["encoder_returns"]["image_embed_shape"][0]
        h, w = sample["net_input"]["patch_images"].shape[-2:]
        scores = self.upsample_logits(scores_low, hp, wp, h, w)
        mask = (target == self.padding_idx) | (target == self.seg_id_offset + self.num_seg) | (target == EOS)
        t = target[~mask] - self.seg_id_offset
        s = scores[~mask]
        metrics = dict(zip(("area_intersect", "area_pred_label", "area_label", "area_union"),
                           self.compute_metric(s.detach(), t.detach())))
        pw = check_pixel_weight(sample.get("target_weight"), target.shape[0], h * w)
        if self.ohem_thresh is not None and model.training:
            hard = hardness_reference(scores[:, :h * w], target, self.seg_id_offset, self.num_seg)
            pw, self.ohem_info = ohem_reference(hard, self.ohem_thresh, self.ohem_min_kept, pw)
        if pw is None and self.class_weight is None:
            loss = F.cross_entropy(s, t, label_smoothing=self.eps)
        else:
            loss = weighted_loss_reference(scores[:, :h * w], target, self.seg_id_offset, self.num_seg,
                                           self._weight_on("class_weight", scores.device), pw, self.eps, self.weight_norm)
        metrics["nll_loss"] = loss
        if self.dice_weight is not None:
            self.dice_sums = dice_sums_reference(scores[:, :h * w], target, self.seg_id_offset, self.num_seg)
            dice = self.dice_weight * dice_loss_reference(scores[:, :h * w], target, self.seg_id_offset, self.num_seg,
                                                          self.dice_smooth, self._weight_on("dice_class_weight", scores.device))
            metrics["dice_loss"] = dice
            loss = loss + dice
        teacher = self._teacher_logits(model, sample, scores_low, hp * wp)
        if teacher is not None:
            teacher_up = self.upsample_logits(teacher[:, :, :self.num_seg].float(), hp, wp, h, w)
            args = (scores[:, :h * w], teacher_up[:, :h * w], target, self.seg_id_offset, self.num_seg, self.distill_temperature,
                    self.distill_mask)
            self.distill_stats = distill_sums_reference(*args).detach()
            kd = self.distill_weight * distill_loss_reference(*args)
            metrics["kd_loss"] = kd
            loss = loss + kd
        return loss, metrics, 1

    def _teacher_logits(self, model, sample, scores_low, P):
        """the sample's `"teacher_logits"` when the distillation term applies to this call, checked against the student's logits
        (ValueError naming what differs), or None: the term is off, or the key is missing in a call that trains nothing"""
        if self.distill_weight is None:
            return None
        teacher = sample.get("teacher_logits")
        if teacher is None:
            if model.training and torch.is_grad_enabled():
                raise ValueError("seg_criterion: distill_weight is set and the sample carries no \"teacher_logits\" "
                                 "(task.distill_sample attaches them)")
            return None
        B, n = scores_low.shape[0], self.num_seg
        if not torch.is_tensor(teacher) or teacher.dtype != torch.bfloat16:
            raise ValueError("seg_criterion: teacher_logits must be a bf16 tensor, got %s"
                             % (teacher.dtype if torch.is_tensor(teacher) else type(teacher)))
        if teacher.dim() != 3 or teacher.shape[0] != B or teacher.shape[1] != P + 1 or teacher.shape[2] < n:
            raise ValueError("seg_criterion: teacher_logits must have the shape [B, P+1, >= n] = [%d, %d, >= %d] of the student's "
                             "grid and classes, got %s" % (B, P + 1, n, tuple(teacher.shape)))
        if teacher.device != scores_low.device:
            raise ValueError("seg_criterion: teacher_logits are on device %s, the logits on %s" % (teacher.device, scores_low.device))
        return teacher if teacher.stride(2) == 1 else teacher.contiguous()

    def _ohem_plane(self, pad, target, pw, hp, wp, h, w, name):
        """the sampler's two stages on the device (hip.seg_hardness, hip.ohem_select), no gradient and no read-back -> the
        weight plane of this call, in buffers kept under `name` and re-allocated only when the shape changes"""
        B, dev = pad.shape[0], pad.device
        ob = getattr(self, name, None)
        key = (B, h * w, dev)
        if ob is None or ob["key"] != key:
            ob = {"key": key, "hard": torch.empty(B, h * w, dtype=torch.float32, device=dev),
                  "plane": torch.empty(B, h * w, dtype=torch.uint8, device=dev),
                  "info": torch.zeros(4, dtype=torch.int64, device=dev), "work": hip.ohem_workspace(dev)}
            setattr(self, name, ob)
        with torch.no_grad():
            hip.seg_hardness(pad, target, hp, wp, h, w, self.num_seg, self.seg_id_offset, out=ob["hard"])
            hip.ohem_select(ob["hard"], self.ohem_thresh, self.ohem_min_kept, weight=pw.contiguous() if pw is not None else None,
                            out=ob["plane"], info=ob["info"], work=ob["work"])
        self.ohem_info = ob["info"]
        return ob["plane"]

    def _weight_on(self, name, dev):
        """the class weights kept as `self.<name>` (class_weight, dice_class_weight) on `dev` (moved there once), or None"""
        cw = getattr(self, name)
        if cw is not None and cw.device != dev:
            cw = cw.to(dev)
            setattr(self, name, cw)
        return cw

    @staticmethod
    def compute_metric(lprobs, target):
        """seg_criterion.py:349-362."""
        n = lprobs.size(-1)
        pred = lprobs.argmax(-1)
        inter = pred[pred == target]
        a_i = torch.histc(inter.float(), bins=n, min=0, max=n - 1)
        a_p = torch.histc(pred.float(), bins=n, min=0, max=n - 1)
        a_l = torch.histc(target.float(), bins=n, min=0, max=n - 1)
        return a_i, a_p, a_l, a_p + a_l - a_i

    @classmethod
    def reduce_metrics(cls, logging_outputs):
        """seg_criterion.py:414-572: sums over workers / micro-batches, losses per sample_size, aAcc / mIoU / mAcc from
        the summed area histograms (nanmean over classes).  Logged through fairseq's `metrics` when it is importable
        (same keys); the aggregate is also returned as a dict for the bundled harness."""
        tot = lambda k: sum(l.get(k, 0) for l in logging_outputs)
        ss = tot("sample_size")
        out = {k: float(tot(k)) / max(float(ss), 1e-9) for k in ("loss", "imfree_loss", "seg_loss", "nll_loss")}
        out.update(ntokens=tot("ntokens"), nsentences=tot("nsentences"), sample_size=ss)
        has_dice = any("dice_loss" in l for l in logging_outputs)             # only a criterion with dice_weight logs it
        if has_dice:
            out["dice_loss"] = float(tot("dice_loss")) / max(float(ss), 1e-9)
        has_kd = any("kd_loss" in l for l in logging_outputs)                 # only a criterion with distill_weight logs it
        if has_kd:
            out["kd_loss"] = float(tot("kd_loss")) / max(float(ss), 1e-9)
        areas = {}
        for suf in ("", "_resnet_postprocess", "_lowres"):
            if "area_intersect" + suf not in logging_outputs[0]:
                continue
            ai, ap, al, au = (tot("area_%s%s" % (k, suf)) for k in ("intersect", "pred_label", "label", "union"))
            areas[suf] = (ai, ap, al, au)
            out["aAcc" + suf] = round(float(ai.sum() / ap.sum()), 4)
            out["mIoU" + suf] = round(float(torch.nanmean(ai / au)), 4)
            out["mAcc" + suf] = round(float(torch.nanmean(ai / al)), 4)
        try:
            from fairseq import metrics
        except ImportError:
            return out
        ntok = out["ntokens"]
        metrics.log_scalar("loss", out["loss"], ss, round=3)
        for k in ("imfree_loss", "seg_loss", "nll_loss") + (("dice_loss",) if has_dice else ()) + (("kd_loss",) if has_kd else ()):
            metrics.log_scalar(k, out[k], ntok, round=3)
        for k in ("ntokens", "nsentences", "sample_size"):
            metrics.log_scalar(k, out[k], 1, round=3)
        for suf, (ai, ap, al, au) in areas.items():
            for k, v in (("intersect", ai), ("pred_label", ap), ("label", al), ("union", au)):
                metrics.log_scalar_sum("_area_%s%s" % (k, suf), v, 1)
            f = lambda a, b, s=suf: (lambda m: round(float(torch.nanmean(m["_area_%s%s" % (a, s)].sum / m["_area_%s%s" % (b, s)].sum)), 4))
            metrics.log_derived("aAcc" + suf, lambda m, s=suf: round(float(m["_area_intersect" + s].sum.sum() / m["_area_pred_label" + s].sum.sum()), 4))
            metrics.log_derived("mIoU" + suf, f("intersect", "union"))
            metrics.log_derived("mAcc" + suf, f("intersect", "label"))
        return out

    @staticmethod
    def logging_outputs_can_be_summed():
        return True
