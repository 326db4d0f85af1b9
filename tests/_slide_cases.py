"""Inputs, references and the comparison rule shared by test_slide_cpu.py and test_slide_gpu.py.

The rule and its constants are those of tests/_predict_cases.py (VALUE_FACTOR, MARGIN_FACTOR, MARGIN_CAP), on the specification
`ifseg_amd.predict.slide_reference`: e = max |fp32 specification - fp64 specification| of the case, values within 4 e, labels
equal wherever the fp64 top-2 margin is >= 32 e, and the pixels left out at most 1 % of the case.

Exact family: integer scores in [-8, 8]; crop = 16 x the window grid, so a window's bilinear weights are multiples of 1/32 per
axis and its values multiples of 1/1024; (o - crop) % stride == 0 and stride >= crop / 2, so a pixel is covered by 1, 2 or 4
windows and the division is by a power of two; the second stage is the identity or exactly x2 (weights in quarters).  Every
sum, quotient and product is exact in fp32: fp32 == fp64 bit for bit, whatever the order of the additions.

General family: randn scores (raw, and softmaxed) on windows whose number per pixel reaches 3 and 9, with up- and downscaling
second stages, a non-square crop, a short axis and a single window.
"""
import torch

from _predict_cases import MARGIN_CAP, MARGIN_FACTOR, VALUE_FACTOR
from ifseg_amd.imageio import slide_windows
from ifseg_amd.predict import slide_reference

# name -> (B, hpw, wpw, n, oh, ow, crop, stride, h, w)
EXACT_CASES = {
    "A": (2, 4, 4, 15, 64, 96, 64, 32, 64, 96),
    "B": (1, 2, 2, 150, 32, 64, 32, (16, 32), 64, 128),
    "C": (1, 4, 4, 257, 64, 128, 64, 64, 64, 128),
    "D": (1, 2, 4, 512, 32, 128, 64, 32, 32, 128),             # a short axis (32 < 64), int16 labels
}
# (hpw, wpw, n, oh, ow, crop, stride, h, w)
GENERAL_CASES = [
    (8, 8, 15, 128, 171, 128, 85, 150, 200),                   # the ADE shape scaled down
    (4, 4, 150, 64, 120, 64, 48, 64, 120),                     # count 3
    (4, 4, 5, 100, 90, 64, 21, 133, 77),                       # 9 windows, count up to 9
    (6, 6, 150, 96, 250, 96, 64, 37, 91),                      # downscaling second stage, odd width
    (3, 5, 257, 40, 200, (48, 80), (30, 50), 40, 200),         # non-square crop, short axis
    (4, 6, 15, 60, 90, (64, 96), 43, 100, 75),                 # one window, non-identity second stage
]
SEEDS = (1, 2)
BATCH_CASE = (3, 4, 4, 150, 64, 120, 64, 48, 37, 91)           # (B, hpw, wpw, n, oh, ow, crop, stride, h, w): w % 4 != 0
# one covering window, identity second stage: (hp, wp, n, h, w), crop >= the image
ONE_WINDOW_CASES = [(4, 6, 150, 37, 91), (8, 12, 5, 127, 200)]


def n_windows(oh, ow, crop, stride):
    ys, xs, _, _ = slide_windows(oh, ow, crop, stride)
    return len(ys) * len(xs)


def exact_scores(name):
    B, hpw, wpw, n, oh, ow, crop, stride, h, w = EXACT_CASES[name]
    g = torch.Generator().manual_seed(3000 + 7 * n + hpw)
    return torch.randint(-8, 9, (B, n_windows(oh, ow, crop, stride), hpw * wpw, n), generator=g).float()


def general_scores(case, seed, softmaxed, batch=1):
    hpw, wpw, n, oh, ow, crop, stride, h, w = case
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(batch, n_windows(oh, ow, crop, stride), hpw * wpw, n, generator=g)
    return s.softmax(-1) if softmaxed else s


class Reference:
    """fp64 specification of one case + the error scale e and the mask of the pixels whose label is decided"""

    def __init__(self, scores, hpw, wpw, oh, ow, crop, stride, h, w):
        scores = scores.detach().float().cpu()
        self.labels, self.conf, self.probs = slide_reference(scores, hpw, wpw, oh, ow, crop, stride, h, w, torch.float64)
        p32 = slide_reference(scores, hpw, wpw, oh, ow, crop, stride, h, w, torch.float32)[2]
        self.e = (p32.double() - self.probs).abs().max().item()
        if self.probs.shape[1] > 1:
            top2 = self.probs.topk(2, dim=1).values
            self.decided = (top2[:, 0] - top2[:, 1]) >= MARGIN_FACTOR * self.e
        else:
            self.decided = torch.ones_like(self.labels, dtype=torch.bool)
        self.undecided_share = 1.0 - self.decided.float().mean().item()

    def check(self, labels, conf=None, probs=None, what=""):
        """asserts the comparison rule on device results"""
        assert self.undecided_share <= MARGIN_CAP, (what, self.undecided_share)
        tol = VALUE_FACTOR * self.e
        lab = labels.cpu().long()
        assert lab.shape == self.labels.shape, (what, lab.shape, self.labels.shape)
        bad = (lab != self.labels) & self.decided
        assert not bad.any(), (what, int(bad.sum()), "label mismatches on decided pixels")
        if probs is not None:
            d = (probs.cpu().double() - self.probs).abs().max().item()
            print(what, "probs: max |d| = %.3e, 4 e = %.3e" % (d, tol))
            assert d <= tol, (what, "probs", d, tol)
        if conf is not None:
            # against the reference value of the class the device named (see _predict_cases.Reference.check)
            ref = self.probs.gather(1, lab[:, None]).squeeze(1)
            d = (conf.cpu().double() - ref).abs().max().item()
            assert d <= tol, (what, "conf", d, tol)


_references = {}


def reference(key, scores, *geometry):
    """one Reference per case, computed once and shared by the tests of a session"""
    if key not in _references:
        _references[key] = Reference(scores, *geometry)
    return _references[key]
