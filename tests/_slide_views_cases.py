"""Inputs, references and the comparison rule shared by test_slide_views_cpu.py and test_slide_views_gpu.py.

The rule and its constants are those of tests/_predict_cases.py (VALUE_FACTOR, MARGIN_FACTOR, MARGIN_CAP), on the specification
`ifseg_amd.predict.slide_views_reference`: e = max |fp32 specification - fp64 specification| of the case, values within 4 e,
labels equal wherever the fp64 top-2 margin is >= 32 e, and the pixels left out at most 1 % of the case.

Exact family (linear mode): the geometries EXACT_CASES A-D of tests/_slide_cases.py with integer scores in [-8, 8], K = 2 and
K = 4 views on the same plane, flips alternating, a fresh score tensor per view.  Every view's value is exact in fp32 (see
_slide_cases.py: a multiple of 2^-16 of magnitude at most 8), so is the sum of up to four of them, and 1 / K is a power of
two: fp32 == fp64 bit for bit, whatever the order of the views.

General family, both modes: per-patch softmaxed randn scores in linear mode (the "probs" order), raw randn scores in softmax
mode (the "logits" order, mmseg's).
"""
import torch

import _slide_cases as SC
from _predict_cases import MARGIN_CAP, MARGIN_FACTOR, VALUE_FACTOR  # noqa: F401
from ifseg_amd.predict import slide_views_reference

EXACT_VIEWS = (2, 4)
# (hpw, wpw, n, crop, stride, h, w, [(oh, ow, flip), ...])
GENERAL_CASES = [
    (4, 4, 15, 64, 42, 75, 100, [(32, 43, 0), (32, 43, 1), (64, 85, 0), (64, 85, 1), (96, 128, 0), (96, 128, 1)]),  # an ADE shape
    (4, 4, 150, 64, 48, 64, 120, [(64, 120, 0), (64, 120, 1), (96, 180, 0)]),                                        # scaled down
    (2, 2, 5, 32, 21, 37, 91, [(32 + 8 * i, 80 + 20 * i, j) for i in range(8) for j in (0, 1)]),   # 16 views, up to 40 windows
    (3, 5, 257, (48, 80), (30, 50), 40, 200, [(40, 200, 0), (60, 300, 1)]),                        # non-square crop, int16 labels
    (2, 4, 512, 64, 32, 32, 128, [(32, 128, 1), (64, 256, 0)]),
    (4, 4, 15, 64, 42, 75, 100, [(64, 85, 1)]),                                                    # one flipped view
]
SEEDS = (1, 2)
# (B, case): the second case's geometry at h, w = 37, 91 (w % 4 != 0)
BATCH_CASE = (3, (4, 4, 150, 64, 48, 37, 91, [(64, 120, 0), (64, 120, 1), (96, 180, 0)]))


def exact_views(name, K):
    """-> (views, crop, stride, h, w) of exact case `name` with K views on its plane, flips alternating"""
    B, hpw, wpw, n, oh, ow, crop, stride, h, w = SC.EXACT_CASES[name]
    nw = SC.n_windows(oh, ow, crop, stride)
    views = []
    for k in range(K):
        g = torch.Generator().manual_seed(5000 + 7 * n + hpw + 101 * k)
        views.append((torch.randint(-8, 9, (B, nw, hpw * wpw, n), generator=g).float(), hpw, wpw, oh, ow, bool(k % 2)))
    return views, crop, stride, h, w


def general_views(case, seed, softmax, batch=1):
    """-> (views, crop, stride, h, w): raw randn scores in softmax mode, per-patch softmaxed ones in linear mode"""
    hpw, wpw, n, crop, stride, h, w, planes = case
    views = []
    for k, (oh, ow, flip) in enumerate(planes):
        g = torch.Generator().manual_seed(1000 * seed + k)
        s = torch.randn(batch, SC.n_windows(oh, ow, crop, stride), hpw * wpw, n, generator=g)
        views.append((s if softmax else s.softmax(-1), hpw, wpw, oh, ow, bool(flip)))
    return views, crop, stride, h, w


def to_device(views, dev):
    return [(s.to(dev), *rest) for s, *rest in views]


class Reference(SC.Reference):
    """fp64 specification of one case + the error scale e and the mask of the pixels whose label is decided; `check` is
    _slide_cases.Reference's"""

    def __init__(self, views, crop, stride, h, w, softmax):
        views = [(s.detach().float().cpu(), *rest) for s, *rest in views]
        self.labels, self.conf, self.probs = slide_views_reference(views, crop, stride, h, w, softmax, torch.float64)
        self.labels32, _, p32 = slide_views_reference(views, crop, stride, h, w, softmax, torch.float32)
        self.e = (p32.double() - self.probs).abs().max().item()
        if self.probs.shape[1] > 1:
            top2 = self.probs.topk(2, dim=1).values
            self.decided = (top2[:, 0] - top2[:, 1]) >= MARGIN_FACTOR * self.e
        else:
            self.decided = torch.ones_like(self.labels, dtype=torch.bool)
        self.undecided_share = 1.0 - self.decided.float().mean().item()


_references = {}


def reference(key, *args):
    """one Reference per case, computed once and shared by the tests of a session"""
    if key not in _references:
        _references[key] = Reference(*args)
    return _references[key]
