"""Shared cases of the distillation tests (test_distill_cpu.py, test_distill_gpu.py): `_dice_cases.dice_inputs` as the student, the
teachers of the issue made on the host with a seeded generator, the specification's values in fp64 and its fp32 autograd
gradient, and a transcription of mmrazor's KLDivergence.  Everything is made once per case (lru_cache); nobody writes to what
these functions return."""
import functools

import torch

import _dice_cases as DC

SEG0 = DC.SEG0
SHAPES = DC.SHAPES
TEACHERS = ("far", "near")
TEMPERATURES = (1.0, 2.0)
MASKS = ("valid", "all")
LAMBDA = 1.5


@functools.lru_cache(maxsize=None)
def teacher(nseg, B, hp, wp, kind):
    """far: bf16(3 randn); near: bf16(student + 0.5 randn); same: the student's own bits.  The padding columns [n:npad] and the eos
    row are NaN: a kernel that reads them shows up as a non-finite result -> bf16 [B, P+1, npad]"""
    lp, _, _ = DC.dice_inputs(nseg, B, hp, wp)
    P, npad = hp * wp, lp.shape[2]
    g = torch.Generator().manual_seed(23 + nseg)
    noise = torch.randn(B, P, nseg, generator=g)
    student = lp[:, :P, :nseg].float()
    body = {"far": 3.0 * noise, "near": student + 0.5 * noise, "same": student}[kind].to(torch.bfloat16)
    t = torch.full((B, P + 1, npad), float("nan"), dtype=torch.bfloat16)
    t[:, :P, :nseg] = body
    if kind == "same":
        assert torch.equal(t[:, :P, :nseg].view(torch.int16), lp[:, :P, :nseg].view(torch.int16))
    assert bool(t[:, P].isnan().all()) and bool(t[:, :, nseg:].isnan().all()) and bool(t[:, :P, :nseg].isfinite().all())
    return t


def widen(t, device):
    """the teacher `t` on `device` as a view with a row stride and a batch stride of its own: 16 columns and 3 rows of NaN more"""
    B, rows, cols = t.shape
    big = torch.full((B, rows + 3, cols + 16), float("nan"), dtype=t.dtype, device=device)
    big[:, :rows, :cols] = t.to(device)
    v = big[:, :rows, :cols]
    assert v.stride(1) == cols + 16 and v.stride(0) > rows * v.stride(1) and not v.is_contiguous()
    return v


def scores(x, nseg, hp, wp, dtype):
    """the x16 upsample of the class columns of the pixel rows -> [B, H*W, n] (the eos row, NaN in a teacher, is left out)"""
    from ifseg_amd.criterions import SegCriterion
    return SegCriterion.upsample_logits(x[:, :, :nseg].to(dtype), hp, wp, 16 * hp, 16 * wp)[:, :-1]


@functools.lru_cache(maxsize=None)
def spec(nseg, B, hp, wp, kind, T, mask):
    """-> (L_kd of the fp64 specification, the fp32 one, N, d (LAMBDA L_kd) / d logits [B, P+1, n] by fp32 autograd of the
    specification through `upsample_logits`)"""
    from ifseg_amd.criterions import SegCriterion
    from ifseg_amd.criterions.seg_criterion import distill_loss_reference, distill_sums_reference
    lp, tgt, _ = DC.dice_inputs(nseg, B, hp, wp)
    te = teacher(nseg, B, hp, wp, kind)
    l64 = distill_loss_reference(scores(lp, nseg, hp, wp, torch.float64), scores(te, nseg, hp, wp, torch.float64), tgt, SEG0,
                                 nseg, T, mask)
    lf = lp[:, :, :nseg].float().clone().requires_grad_(True)
    s32 = SegCriterion.upsample_logits(lf, hp, wp, 16 * hp, 16 * wp)[:, :-1]
    t32 = scores(te, nseg, hp, wp, torch.float32)
    l32 = distill_loss_reference(s32, t32, tgt, SEG0, nseg, T, mask)
    (LAMBDA * l32).backward()
    N = int(distill_sums_reference(s32.detach(), t32, tgt, SEG0, nseg, T, mask)[1])
    return float(l64), float(l32.detach()), N, lf.grad.detach()


def mmrazor_kl_divergence(preds_S, preds_T, tau=1.0, reduction="batchmean", loss_weight=1.0):
    """The lines of mmrazor's KLDivergence.forward, transcribed (mmrazor is no dependency): preds [B, n, H, W]
        preds_T = preds_T.detach()
        softmax_pred_T = F.softmax(preds_T / self.tau, dim=1)
        logsoftmax_preds_S = F.log_softmax(preds_S / self.tau, dim=1)
        loss = (self.tau**2) * F.kl_div(logsoftmax_preds_S, softmax_pred_T, reduction=self.reduction)
        return self.loss_weight * loss"""
    import torch.nn.functional as F
    preds_T = preds_T.detach()
    softmax_pred_T = F.softmax(preds_T / tau, dim=1)
    logsoftmax_preds_S = F.log_softmax(preds_S / tau, dim=1)
    loss = (tau ** 2) * F.kl_div(logsoftmax_preds_S, softmax_pred_T, reduction=reduction)
    return loss_weight * loss
