"""Shared cases of the OHEM tests (test_ohem_cpu.py, test_ohem_gpu.py): synthetic hardness planes of every kind the select has
to get right, the regimes of (thresh, min_kept), a literal transcription of the upstream sampler's lines, and the logits /
targets of the hardness kernel with their fp32 and fp64 specifications.  Everything is made on the host, once per shape
(lru_cache); nobody writes to what these functions return."""
import functools

import torch

SEG0 = 1000
ONE_BITS = 0x3F800000

KINDS = ("uniform", "seven", "shared", "half", "special", "none", "equal")


def _bits_to_f32(bits):
    return bits.to(torch.int32).view(torch.float32)


@functools.lru_cache(maxsize=None)
def plane(kind, B, N, seed=3):
    """fp32 [B, N]:
    uniform   random values in [0, 1)
    seven     seven distinct values: heavy ties, the k-th value is always shared
    shared    half of the entries share their top 20 key bits (only the last digit tells them apart), the others their top 10
    half      uniform, every second entry -1 (an invalid pixel)
    special   -1, -0.0, NaN, 1.0, the float above 1.0, 0, a denormal, +inf, 2.0 among uniform values
    none      no candidate at all (-1 everywhere)
    equal     one value everywhere"""
    g = torch.Generator().manual_seed(seed + 17 * B + N)
    u = torch.rand(B, N, generator=g)
    if kind == "uniform":
        return u
    if kind == "seven":
        vals = torch.tensor([0.0, 0.03, 0.25, 0.5, 0.69999, 0.7, 1.0])
        return vals[torch.randint(0, 7, (B, N), generator=g)]
    if kind == "shared":
        low = torch.randint(0, 1 << 10, (B, N), generator=g)
        mid = torch.randint(0, 1 << 20, (B, N), generator=g)
        pick = torch.rand(B, N, generator=g) < 0.5
        return _bits_to_f32(torch.where(pick, 0x3F000000 | (0x155 << 10) | low, 0x3F000000 | mid))
    if kind == "half":
        h = u.clone().reshape(-1)
        h[::2] = -1.0
        return h.reshape(B, N)
    if kind == "special":
        sp = torch.tensor([-1.0, -0.0, float("nan"), 1.0, 0.0, 1e-40, float("inf"), 2.0, 0.0])
        sp[4] = _bits_to_f32(torch.tensor([ONE_BITS + 1]))[0]               # 1.0000001
        h = u.clone().reshape(-1)
        idx = torch.randperm(B * N, generator=g)[: max(1, min(B * N, max(len(sp), B * N // 3)))]
        h[idx] = sp[torch.arange(len(idx)) % len(sp)]
        return h.reshape(B, N)
    if kind == "none":
        return torch.full((B, N), -1.0)
    if kind == "equal":
        return torch.full((B, N), 0.4)
    raise KeyError(kind)


def weight_plane(B, N, seed=5):
    g = torch.Generator().manual_seed(seed + B + N)
    w = torch.randint(0, 256, (B, N), generator=g, dtype=torch.uint8)
    w.reshape(-1)[::5] = 0                                                   # kept pixels of weight 0 among them
    return w


def regimes(B, N):
    """(thresh, min_kept), one per regime: thresh decides (k = 0: the k-th value is the minimum); min_kept decides; both
    in play; min_kept * B >= |V| (everything below the maximum); min_kept = 0 and thresh = 0 (nothing below the minimum);
    thresh = 1 (every candidate below 1.0)"""
    return [(0.7, 0), (0.0, max(N // 4, 1)), (0.3, max(N // 2, 1)), (0.5, N + 1), (0.0, 0), (1.0, 3)]


def upstream_sample(prob, valid, thresh, min_kept):
    """The lines of mmseg's OHEMPixelSampler.sample with `thresh` given, transcribed: prob fp32 [B, N] (the probability of
    every pixel's own label), valid bool [B, N] -> the kept pixels, bool [B, N].
        batch_kept = min_kept * batch size
        sort_prob = prob[valid].sort()
        min_threshold = sort_prob[min(batch_kept, sort_prob.numel() - 1)] if sort_prob.numel() > 0 else 0.0
        threshold = max(min_threshold, thresh)
        kept[valid][prob[valid] < threshold] = 1"""
    batch_kept = min_kept * prob.shape[0]
    sort_prob, _ = prob[valid].sort()
    thr32 = torch.tensor(thresh, dtype=torch.float32)                       # the comparison below is an fp32 one
    if sort_prob.numel() > 0:
        min_threshold = sort_prob[min(batch_kept, sort_prob.numel() - 1)]
    else:
        min_threshold = torch.tensor(0.0)
    threshold = max(min_threshold, thr32)
    kept = torch.zeros_like(valid)
    kept[valid] = prob[valid] < threshold
    return kept


# ------------------------------------------------------------------------------------------------- the hardness plane
HARD_CASES = [(2, 2, 3, 4), (5, 2, 3, 4), (17, 2, 3, 4), (150, 1, 2, 3), (512, 1, 2, 3), (15, 2, 8, 8)]


@functools.lru_cache(maxsize=None)
def hard_inputs(nseg, B, hp, wp):
    """test_weighted_loss_gpu._inputs' logits and targets (bf16, scale 2, the ignore label among the targets), one pad and one
    out-of-range target poisoned in, and for 15 classes or more a bonus of +4 at the label of each cell's centre pixel, so that
    p spreads over (0, 1) -> (logits_pad bf16 [B, P+1, npad], target int64 [B, H*W+1])"""
    P, H, W = hp * wp, hp * 16, wp * 16
    npad = (nseg + 7) // 8 * 8
    g = torch.Generator().manual_seed(7)
    logits = torch.randn(B, P + 1, nseg, generator=g) * 2
    tgt = torch.randint(0, nseg + 1, (B, H * W), generator=g) + SEG0        # includes the ignore label seg0 + nseg
    if nseg >= 15:
        t2 = tgt.reshape(B, hp, 16, wp, 16)[:, :, 8, :, 8].reshape(B, P) - SEG0
        ok = t2 < nseg
        b, c = torch.nonzero(ok, as_tuple=True)
        logits[b, c, t2[ok]] += 4.0
    tgt[0, 5] = 1                                                            # pad
    tgt[B - 1, H * W - 7] = SEG0 + nseg + 5                                   # neither a class nor pad / eos / ignore
    tgt[0, 40] = SEG0 - 3
    tgt = torch.cat([tgt, torch.full((B, 1), 2)], 1)
    lp = torch.zeros(B, P + 1, npad, dtype=torch.bfloat16)
    lp[:, :, :nseg] = logits
    return lp, tgt


@functools.lru_cache(maxsize=None)
def hard_specs(nseg, B, hp, wp):
    """-> (the fp32 specification, the fp64 one, valid bool [B, H*W], e = max |fp32 - fp64| over the valid pixels)"""
    from ifseg_amd.criterions import SegCriterion
    from ifseg_amd.criterions.seg_criterion import hardness_reference
    lp, tgt = hard_inputs(nseg, B, hp, wp)
    H, W = hp * 16, wp * 16
    s32 = hardness_reference(SegCriterion.upsample_logits(lp[:, :, :nseg].float(), hp, wp, H, W), tgt, SEG0, nseg)
    s64 = hardness_reference(SegCriterion.upsample_logits(lp[:, :, :nseg].double(), hp, wp, H, W), tgt, SEG0, nseg)
    body = tgt[:, :-1]
    valid = (body >= SEG0) & (body < SEG0 + nseg)
    e = float((s32.double() - s64)[valid].abs().max())
    return s32, s64, valid, e
