"""Shared makers of the bias-sweep tests (test_bias_sweep_cpu.py, test_bias_sweep_gpu.py): K logit-like grids z - g_k d of one
set of logits, _tsweep_cases' piecewise-constant ground truth, three doctored pixels, and a literal per-pixel transcription of
the rule."""
import torch

import _tsweep_cases as TC

# (hp, wp, h, w, n, K, B): _tsweep_cases' shapes, and n at its limit together with K at its limit
SHAPES = {**TC.SHAPES, "n512_k16": (3, 3, 48, 64, 512, 16, 1)}
KINDS = {**TC.KINDS, "n512_k16": TC.KINDS["n512"]}
SMALL, SMALL_KINDS = TC.SMALL, TC.SMALL_KINDS
_GT_OF = {"n512_k16": "n512"}           # the case of _tsweep_cases whose ground truth a case takes


def strengths(K):
    """K strengths around 0 in steps of 1 / 4, zero and negative ones among them for K > 1"""
    return tuple((j - K // 3) / 4 for j in range(K))


def make(name, seed=0):
    """-> (grids fp32 [K, B, hp*wp, n], gt [B, h, w], (hp, wp, n, raw_labels), {kind: (y, x, true class)}), on the host.
    grids[k] = z - g_k d for one z = 3 randn, a random direction d and g = strengths(K): logit-like, negative values among
    them.  The ground truth is `_tsweep_cases.make`'s (blocks, ignore values, uint8 raw / int16 ids, one pixel out of range).
    Every grid is doctored at the patches under three scored pixels of image 0, placed as `_tsweep_cases.doctored_pixels`
    places them: 'tie': two classes share the maximum exactly (the lower one must win; the true class is the higher one),
    'nan': the true class's value is NaN and every other one is far below what a NaN would have to beat (a NaN never wins: the
    pixel is a miss), 'allnan': every value is NaN (the label is class 0, and the true class is 0: a hit).  n = 1 has no
    doctored pixel."""
    hp, wp, h, w, n, K, B = {**SHAPES, **SMALL}[name]
    dtype, raw, _ = {**KINDS, **SMALL_KINDS}[name]
    _, gt, (hp2, wp2, n2, raw2), _ = TC.make(_GT_OF.get(name, name), seed)
    assert (hp2, wp2, n2, raw2) == (hp, wp, n, raw) and tuple(gt.shape) == (B, h, w) and gt.dtype == dtype
    g = torch.Generator().manual_seed(7300 + seed + 13 * n + K)
    z = 3.0 * torch.randn(B, hp * wp, n, generator=g)
    d = torch.randn(n, generator=g)
    grids = torch.stack([z - gk * d for gk in strengths(K)]).contiguous()
    gt = gt.clone()
    shift = 1 if raw else 0
    where = {}
    hi, lo = n - 1, max(n - 2, 0)
    spots = TC.doctored_pixels(h, w) if n > 1 else {}
    for kind, at in (("allnan", "one"), ("nan", "zero"), ("tie", "tie")):
        if at not in spots:
            continue
        y, x = spots[at]
        vec = torch.full((n,), -20.0)
        if kind == "allnan":
            t = 0
            vec[:] = float("nan")
        elif kind == "nan":
            t = hi
            vec[t] = float("nan")
            vec[0] = -5.0
        else:
            t = hi
            vec[lo] = vec[hi] = 7.5
        for py in TC._axis(y, hp, h):
            for px in TC._axis(x, wp, w):
                grids[:, 0, py * wp + px] = vec
        gt[0, y, x] = t + shift
        where[kind] = (y, x, t)
    return grids, gt, (hp, wp, n, raw), where


def literal(grids, hp, wp, gt, raw_labels, interp=torch.float64):
    """The rule of `bias_sweep_reference`, transcribed pixel by pixel with Python loops and scalars (small cases only):
    -> (areas int64 [K, 3, n], tally int64 [2])"""
    K, B, P, n = grids.shape
    h, w = gt.shape[1:]
    areas = torch.zeros(K, 3, n, dtype=torch.int64)
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
                    best, bv = 0, float("-inf")
                    for c in range(n):                  # the running first maximum: a NaN compares false and never wins
                        if p[c] > bv:
                            best, bv = c, p[c]
                    areas[k, 1, best] += 1
                    areas[k, 2, t] += 1
                    if best == t:
                        areas[k, 0, t] += 1
    return areas, torch.tensor(tally)
