"""Inputs, references and the comparison rule shared by test_pamr_cpu.py and test_pamr_gpu.py (pixel-adaptive mask refinement,
csrc/pamr.hip; `predict.pamr_reference` is the specification).

The image of a case is 16-pixel blocks of random colours plus uniform noise of +-6 grey levels: flat regions whose contrast is
the noise, and edges of every strength and direction.  The values are F.interpolate(bilinear, align_corners=False) of
softmax(3 randn) on an (H // 16 + 1) x (W // 16 + 1) grid: what `seg_predict(probs=True)` hands over.  The shapes are the
smallest at which the kernels can still go wrong (CASES says what each one exercises).

The comparison rule is the project's (tests/_predict_cases.py): the reference is the fp64 specification; e is
max |fp32 specification - fp64 specification| over the case, floored at 2^-23 (a weight or a probability can be 1, and no fp32
result is better than half a unit there).  Values must agree within 4 e; labels must agree wherever the fp64 specification's
top-2 margin is >= 32 e; the pixels below that margin are left out and must be at most 1 % of the case -- the CPU file asserts
that for every case."""
import functools

import torch
import torch.nn.functional as F

from ifseg_amd.predict import PAMR_DILATIONS, pamr_affinity_reference, pamr_iterate_reference, pamr_reference

VALUE_FACTOR, MARGIN_FACTOR, MARGIN_CAP = 4.0, 32.0, 0.01
E_FLOOR = 2.0 ** -23

# name: (H, W, n, dilations, iters)
CASES = {
    "tiny": (5, 7, 4, PAMR_DILATIONS, 2),                 # image smaller than most dilations, clamped on both sides
    "one_tile": (16, 64, 1, (1,), 1),                     # one exact tile, one class
    "thin_last_tile": (16, 129, 15, PAMR_DILATIONS, 1),   # last tile one pixel wide
    "int16": (17, 65, 260, (1, 2), 2),                    # int16 labels, one-pixel tile row and column
    "ten_iters": (20, 37, 3, PAMR_DILATIONS, 10),
    "one_wide_ring": (48, 48, 15, (24,), 2),
    "many_classes": (33, 70, 150, PAMR_DILATIONS, 3),
    "odd": (37, 131, 19, PAMR_DILATIONS, 10),
    "blocks": (64, 200, 15, PAMR_DILATIONS, 10),
}


def make_image(H, W, seed):
    g = torch.Generator().manual_seed(9000 + seed)
    blocks = torch.randint(0, 256, ((H + 15) // 16, (W + 15) // 16, 3), generator=g)
    img = blocks.repeat_interleave(16, 0).repeat_interleave(16, 1)[:H, :W]
    return (img + torch.randint(-6, 7, (H, W, 3), generator=g)).clamp(0, 255).to(torch.uint8).contiguous()


def make_values(H, W, n, seed):
    g = torch.Generator().manual_seed(9500 + seed)
    grid = (3.0 * torch.randn(1, n, H // 16 + 1, W // 16 + 1, generator=g)).softmax(1)
    return F.interpolate(grid, size=(H, W), mode="bilinear", align_corners=False)[0].contiguous()


def _e(a32, a64):
    return max((a32.double() - a64).abs().max().item(), E_FLOOR)


class Case:
    """one case: its inputs, the fp64 specification of every stage, the error scales and the decided pixels"""

    def __init__(self, name):
        self.name = name
        self.H, self.W, self.n, self.dilations, self.iters = CASES[name]
        seed = list(CASES).index(name)
        self.image, self.values = make_image(self.H, self.W, seed), make_values(self.H, self.W, self.n, seed)
        # the weights
        self.w64 = pamr_affinity_reference(self.image, self.dilations, torch.float64)
        self.w32 = pamr_affinity_reference(self.image, self.dilations, torch.float32)
        self.e_w = _e(self.w32, self.w64)
        # the iteration alone, on the fp32 weights: the gather and the dot product
        m64, m32 = self.values.double(), self.values
        for _ in range(self.iters):
            m64, m32 = pamr_iterate_reference(self.w32.double(), m64, self.dilations), pamr_iterate_reference(self.w32, m32, self.dilations)
        self.iter64, self.e_iter = m64, _e(m32, m64)
        # end to end
        self.labels, self.conf, self.probs = pamr_reference(self.image, self.values, self.dilations, self.iters, torch.float64)
        self.e = _e(pamr_reference(self.image, self.values, self.dilations, self.iters, torch.float32)[2], self.probs)
        if self.n > 1:
            top2 = self.probs.topk(2, dim=0).values
            self.decided = (top2[0] - top2[1]) >= MARGIN_FACTOR * self.e
        else:
            self.decided = torch.ones_like(self.labels, dtype=torch.bool)
        self.undecided_share = 1.0 - self.decided.float().mean().item()

    def check(self, labels, conf=None, probs=None, what=""):
        """asserts the comparison rule on device results -> the largest |value - specification| / e it saw (0 without values)"""
        what = what or self.name
        assert self.undecided_share <= MARGIN_CAP, (what, self.undecided_share)
        tol, worst = VALUE_FACTOR * self.e, 0.0
        lab = labels.cpu().long()
        assert lab.shape == self.labels.shape, (what, lab.shape, self.labels.shape)
        bad = (lab != self.labels) & self.decided
        assert not bad.any(), (what, int(bad.sum()), "label mismatches on decided pixels")
        if probs is not None:
            d = (probs.cpu().double() - self.probs).abs().max().item()
            print("%s: values |kernel - specification| = %.3g = %.2f e (e = %.3g)" % (what, d, d / self.e, self.e))
            assert d <= tol, (what, "probs", d, tol)
            worst = d / self.e
        if conf is not None:
            # the winning value, against the specification's value OF THE NAMED class (tests/_predict_cases.py)
            ref = self.probs.gather(0, lab[None]).squeeze(0)
            d = (conf.cpu().double() - ref).abs().max().item()
            assert d <= tol, (what, "conf", d, tol)
        return worst


@functools.lru_cache(maxsize=None)
def case(name):
    """the case, computed once per process and shared by the tests that need it"""
    return Case(name)


def upstream_pamr(x, mask, dilations, iters):
    """A literal transcription of the published module (Araslanov & Roth, "Single-Stage Semantic Segmentation from Image
    Labels", CVPR 2020: PAMR with LocalAffinityAbs, LocalStDev and LocalAffinityCopy) without its resize of the mask:
    x [B, 3, H, W] the image, mask [B, C, H, W] -> (the refined mask [B, C, H, W], the weights [B, 1, 8 D, H, W]).
    Every affinity is a dilated 3 x 3 convolution on the replicate-padded input with a fixed kernel bank."""
    def local(x, kernel):
        B, K, H, W = x.size()
        x = x.view(B * K, 1, H, W)
        affs = []
        for d in dilations:
            x_pad = F.pad(x, [d] * 4, mode="replicate")
            affs.append(F.conv2d(x_pad, kernel.type_as(x), dilation=d))
        return torch.cat(affs, 1).view(B, K, -1, H, W)

    ring = [(0, 0), (0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1), (2, 2)]
    k_abs, k_copy, k_std = torch.zeros(8, 1, 3, 3), torch.zeros(8, 1, 3, 3), torch.zeros(9, 1, 3, 3)
    for i, (r, c) in enumerate(ring):
        k_abs[i, 0, 1, 1], k_abs[i, 0, r, c] = 1, -1        # centre minus neighbour
        k_copy[i, 0, r, c] = 1                              # the neighbour
    for i in range(9):
        k_std[i, 0, i // 3, i % 3] = 1                      # the nine taps
    x_std = local(x, k_std).std(2, keepdim=True)
    a = -local(x, k_abs).abs() / (1e-8 + 0.1 * x_std)
    a = a.mean(1, keepdim=True)
    a = F.softmax(a, 2)
    for _ in range(iters):
        m = local(mask, k_copy)
        mask = (m * a).sum(2)
    return mask, a
