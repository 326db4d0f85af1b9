"""Shared makers of the temperature-sweep tests (test_temperature_sweep_cpu.py, test_temperature_sweep_gpu.py): K grids of
probabilities of one set of logits, a piecewise-constant ground truth, three doctored pixels, a literal per-pixel transcription
of the rule, and the per-pixel terms of the two proper scores."""
import math

import torch

from ifseg_amd.predict import FLT_MIN, _scored_mask, default_temperatures

# (hp, wp, h, w, n, K, B): the smallest shapes at which each part of the kernel can go wrong
SHAPES = {
    "ragged_k1": (2, 3, 33, 70, 3, 1, 1),               # ragged tile edges, K = 1
    "x16_two_images": (4, 4, 64, 64, 15, 4, 2),         # x16 upsampling, two images
    "k16_odd_ratios": (8, 5, 37, 129, 150, 16, 1),      # K at its limit, odd ratios
    "downscale": (32, 32, 20, 20, 19, 3, 1),            # downscaling, footprint larger than the tile
    "n512": (3, 3, 48, 64, 512, 2, 1),                  # n at its limit
    "identity": (6, 6, 6, 6, 2, 2, 1),                  # identity
}
# per shape: (the ground truth's dtype, raw_labels, whether one pixel holds a class out of range)
KINDS = {
    "ragged_k1": (torch.uint8, True, False),
    "x16_two_images": (torch.int16, False, True),
    "k16_odd_ratios": (torch.uint8, True, True),
    "downscale": (torch.uint8, False, False),
    "n512": (torch.int16, True, True),
    "identity": (torch.uint8, True, False),
}
# smaller cases of the same maker for the literal transcription on the CPU (Python loops per pixel)
SMALL = {
    "small_ids_i16_oor": (3, 4, 13, 22, 5, 3, 2),
    "small_raw_u8_oor": (5, 2, 9, 30, 7, 2, 1),
    "small_down_ids_u8": (9, 11, 6, 5, 4, 2, 1),
    "n1": (2, 2, 7, 9, 1, 2, 1),
}
SMALL_KINDS = {
    "small_ids_i16_oor": (torch.int16, False, True),
    "small_raw_u8_oor": (torch.uint8, True, True),
    "small_down_ids_u8": (torch.uint8, False, False),
    "n1": (torch.int16, True, True),
}


def temperatures(K):
    """K of the default temperatures, around 1.0"""
    d = default_temperatures()
    return d[(len(d) - K) // 2:][:K]


def _axis(d, n_in, n_out):
    """the source samples of destination sample d that carry weight (float64 evaluation of the coordinate rule; the doctored
    pixels sit where it is far from a rounding boundary)"""
    s = max((d + 0.5) * n_in / n_out - 0.5, 0.0)
    i0 = min(int(s), n_in - 1)
    i1 = min(i0 + 1, n_in - 1)
    return sorted({i0} | ({i1} if s - i0 > 0 else set()))


def doctored_pixels(h, w):
    """-> {kind: (y, x)} of image 0: three corners, whose source patches do not overlap on any of SHAPES"""
    return {"one": (0, 0), "zero": (0, w - 1), "tie": (h - 1, 0)}


def make(name, seed=0):
    """-> (grids fp32 [K, B, hp*wp, n], gt [B, h, w], (hp, wp, n, raw_labels), {kind: (y, x, true class)}), on the host.
    grids[k] = softmax(z / T_k) of one z = 3 randn.  Grid 0 is doctored at the patches under three scored pixels of image 0:
    'tie': two classes share the maximum exactly (the lower one must win; the true class is the higher one), 'zero': the true
    class's value is exactly 0 (NLL 87.3...), 'one': the true class's value is a one-hot 1 (bin 255; exactly 1.0 where the
    pixel's weights are 1, 0, 0, 0: every shape but the downscaling ones).  n = 1 has no doctored pixel."""
    hp, wp, h, w, n, K, B = {**SHAPES, **SMALL}[name]
    dtype, raw, oor = {**KINDS, **SMALL_KINDS}[name]
    g = torch.Generator().manual_seed(9100 + seed + 13 * n + K)
    z = 3.0 * torch.randn(B, hp * wp, n, generator=g)
    grids = torch.stack([torch.softmax(z.double() / T, -1).float() for T in temperatures(K)]).contiguous()
    # the ground truth: blocks of 5 x 7 pixels of one class each, a share of them an ignore value
    shift = 1 if raw else 0
    by, bx = -(-h // 5), -(-w // 7)
    blocks = torch.randint(0, n, (B, by, bx), generator=g) + shift
    if dtype == torch.uint8:
        blocks = torch.where(blocks == 255, torch.full_like(blocks, shift), blocks)
    ign = torch.tensor([0, 255] if raw else [n, 255])
    drop = torch.rand(B, by, bx, generator=g) < 0.2
    blocks = torch.where(drop, ign[torch.randint(0, 2, (B, by, bx), generator=g)], blocks)
    gt = blocks.repeat_interleave(5, 1).repeat_interleave(7, 2)[:, :h, :w].contiguous()
    if oor:
        gt[B - 1, h // 2, w // 2] = 600 if dtype == torch.int16 else 254       # class 599 / 253 (254 with ids): outside [0, n)
        assert dtype == torch.int16 or n < 253
    where = {}
    hi, lo = n - 1, max(n - 2, 0)
    for kind, (y, x) in (doctored_pixels(h, w) if n > 1 else {}).items():
        vec = torch.zeros(n)
        if kind == "one":
            t = lo
            vec[t] = 1.0
        elif kind == "zero":
            t = hi
            vec[:] = 1.0 / (n - 1)
            vec[t] = 0.0
        else:
            t = hi
            vec[:] = 0.2 / max(n - 2, 1) if n > 2 else 0.0
            vec[lo] = vec[hi] = 0.4 if n > 2 else 0.5
        for py in _axis(y, hp, h):
            for px in _axis(x, wp, w):
                grids[0, 0, py * wp + px] = vec
        gt[0, y, x] = t + shift
        where[kind] = (y, x, t)
    return grids, gt.to(dtype), (hp, wp, n, raw), where


def literal(grids, hp, wp, gt, raw_labels, interp=torch.float64):
    """The rule of `temperature_sweep_reference`, transcribed pixel by pixel with Python loops and scalars (small cases only):
    -> (hist int64 [K, 256, 2], sums float64 [K, 2], tally int64 [2])"""
    K, B, P, n = grids.shape
    h, w = gt.shape[1:]
    hist = torch.zeros(K, 256, 2, dtype=torch.int64)
    sums = [[0.0, 0.0] for _ in range(K)]
    tally = [0, 0]

    def coord(d, n_in, n_out):
        s = max((d + 0.5) * (n_in / n_out) - 0.5, 0.0)
        i0 = min(int(s), n_in - 1)
        return i0, min(i0 + 1, n_in - 1), s - i0

    for b in range(B):
        for y in range(h):
            for x in range(w):
                v = int(gt[b, y, x])
                if raw_labels:
                    if v in (0, 255):
                        continue
                    t = v - 1
                else:
                    if v in (n, 255):
                        continue
                    t = v
                if not 0 <= t < n:
                    tally[1] += 1
                    continue
                tally[0] += 1
                y0, y1, ly = coord(y, hp, h)
                x0, x1, lx = coord(x, wp, w)
                for k in range(K):
                    gk = grids[k, b].to(interp)
                    p = ((1 - ly) * ((1 - lx) * gk[y0 * wp + x0] + lx * gk[y0 * wp + x1])
                         + ly * ((1 - lx) * gk[y1 * wp + x0] + lx * gk[y1 * wp + x1])).tolist()
                    best = max(range(n), key=lambda c: p[c])              # max keeps the first of equal values
                    q = math.floor(float(torch.tensor(p[best], dtype=torch.float32)) * 256.0)
                    hist[k, min(max(q, 0), 255), 1 if best == t else 0] += 1
                    sums[k][0] += -math.log(max(p[t], FLT_MIN))
                    sums[k][1] += sum(c * c for c in p) - 2.0 * p[t] + 1.0
    return hist, torch.tensor(sums, dtype=torch.float64), torch.tensor(tally)


def terms(probs, gt, n, raw_labels):
    """probs floating [B, n, h, w] -> per SCORED pixel, float64: (the NLL term, the Brier term, the Brier term with every sign
    positive: sum_c p^2 + 2 p_t + 1, the scale of its rounding), and the scored mask over all pixels"""
    _, cls, scored, _ = _scored_mask("terms", probs.argmax(1), gt, n, raw_labels)
    p = probs.permute(0, 2, 3, 1).reshape(-1, n)[scored].double()
    pt = p.gather(1, cls[scored][:, None])[:, 0]
    sq = (p * p).sum(1)
    return -pt.clamp_min(FLT_MIN).log(), sq - 2.0 * pt + 1.0, sq + 2.0 * pt + 1.0, scored
