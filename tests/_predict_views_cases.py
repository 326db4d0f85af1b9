"""Inputs, references and the comparison rule shared by test_predict_views_cpu.py and test_predict_views_gpu.py.

The rule and its constants are those of tests/_predict_cases.py (VALUE_FACTOR, MARGIN_FACTOR, MARGIN_CAP), on the specification
`ifseg_amd.predict.upsample_views_reference`: e = max |fp32 specification - fp64 specification| of the case, values within
4 e, labels equal wherever the fp64 top-2 margin is >= 32 e, and the pixels left out at most 1 % of the case.

Exact family: integer scores in [-8, 8], output 16 g, view grids g/2, g and 2g.  The bilinear weights are multiples of 1/64,
1/32 and 1/16 per axis, so every product is a multiple of 1/4096 and every sum of at most four views of them is exact in fp32;
1/K is a power of two for K in {1, 2, 4}.  fp32 == fp64 bit for bit, whatever the order of the additions.

General family: randn scores (raw, and softmaxed) on the grids of GRIDS, taken in turn, flips alternating.
"""
import torch

from _predict_cases import MARGIN_CAP, MARGIN_FACTOR, VALUE_FACTOR
from ifseg_amd.predict import upsample_views_reference

# (B, g_h, g_w, n): output (16 g_h, 16 g_w)
EXACT_SHAPES = [(2, 4, 6, 15), (1, 2, 2, 150), (1, 2, 4, 257), (1, 2, 2, 512)]
EXACT_KS = (1, 2, 4)
# per K, (numerator, denominator) of the grid against g and the flip of every view: all three grids, flips mixed
EXACT_VIEWS = {1: [(1, 1, False)], 2: [(1, 2, True), (2, 1, False)], 4: [(1, 1, False), (1, 2, True), (2, 1, True), (1, 2, False)]}

GRIDS = [(4, 6), (8, 12), (12, 18), (7, 5)]
# (K, n, h, w): every K, n and output of the family; K = 12 is six ratios x two flips
GENERAL_CASES = [(3, 15, 100, 75), (5, 150, 100, 75), (12, 5, 33, 31), (5, 15, 127, 200), (3, 150, 5, 3), (12, 150, 33, 31)]
SEEDS = (1, 2)
# footprints beyond any staging buffer: a 40 x 40 grid of 512 classes down to 20 x 20, and a 20 x 20 grid beside it
DIRECT_CASE = (2, 512, 20, 20, [(40, 40), (20, 20)])
BATCH_CASE = (3, 3, 150, 37, 91)                # (B, K, n, h, w): w % 4 != 0


def exact_views(shape, K):
    B, gh, gw, n = shape
    g = torch.Generator().manual_seed(2000 + 7 * n + gh + K)
    out = []
    for num, den, flip in EXACT_VIEWS[K]:
        hp, wp = gh * num // den, gw * num // den
        out.append((torch.randint(-8, 9, (B, hp * wp, n), generator=g).float(), hp, wp, flip))
    return out


def general_views(K, n, seed, softmaxed, batch=1, grids=GRIDS):
    g = torch.Generator().manual_seed(seed)
    out = []
    for k in range(K):
        hp, wp = grids[k % len(grids)]
        s = torch.randn(batch, hp * wp, n, generator=g)
        out.append((s.softmax(-1) if softmaxed else s, hp, wp, k % 2 == 1))
    return out


def to_device(views, dev):
    return [(s.to(dev), hp, wp, flip) for s, hp, wp, flip in views]


class Reference:
    """fp64 specification of one case + the error scale e and the mask of the pixels whose label is decided"""

    def __init__(self, views, h, w):
        views = [(s.detach().float().cpu(), hp, wp, flip) for s, hp, wp, flip in views]
        self.labels, self.conf, self.probs = upsample_views_reference(views, h, w, torch.float64)
        p32 = upsample_views_reference(views, h, w, torch.float32)[2]
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
            assert d <= tol, (what, "probs", d, tol)
        if conf is not None:
            # against the reference value of the class the device named (see _predict_cases.Reference.check)
            ref = self.probs.gather(1, lab[:, None]).squeeze(1)
            d = (conf.cpu().double() - ref).abs().max().item()
            assert d <= tol, (what, "conf", d, tol)


_references = {}


def reference(key, views, h, w):
    """one Reference per case, computed once and shared by the tests of a session"""
    if key not in _references:
        _references[key] = Reference(views, h, w)
    return _references[key]
