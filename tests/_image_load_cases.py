"""Inputs, references and the comparison rule shared by test_image_load_cpu.py and test_image_load_gpu.py.

Exact family: seeded random uint8 images upscaled by an integer factor f in both axes (and one 60 x 90 -> 128 x 192 ratio
case).  Every bilinear weight is a multiple of 1/(2f) per axis (1/64 for the ratio case), so every product of two weights
and a grey level and every sum is exact in fp32: the fp32 and fp64 specifications are identical and any summation order or
FMA contraction gives the same bits.  The device's grey level q and its normalised output must equal the fp32
specification bit for bit.

General family: arbitrary ratios, destination size from `eval_size`.  The reference is the fp64 specification; `e` is
max |v of the fp32 specification - v of the fp64 specification| on the same input, computed here.  The device's q must equal
the reference's wherever the reference's v lies at least 32 e from a rounding boundary (k + 0.5), |q_dev - q_ref| <= 1
everywhere, and where q agrees the normalised output equals the table entry bit for bit.  The pixels inside the margin are
left out and may be at most 1 % of a case (MARGIN_CAP) -- the CPU file asserts that for every case.  The factor 32 is the
one _predict_cases.py uses, for the same reason: FMA contraction and summation order.

The device's q is read through the kernel's own table: with mean 0 and std 1/255 the table entry of grey level k rounds to k.
"""
import functools

import torch

from ifseg_amd.imageio import eval_size, image_load_reference, normalisation_table

EXACT_CASES = [(2, 8, 12, 2), (1, 7, 5, 4), (3, 3, 3, 8), (1, 16, 16, 16), (1, 1, 1, 16)]          # (B, H0, W0, f)
EXACT_RATIO = (1, 60, 90, 128, 192)                                                                  # (B, H0, W0, oh, ow)
GENERAL_CASES = [(97, 61, 128), (33, 250, 128), (200, 131, 128), (5, 3, 128), (700, 300, 128), (61, 47, 128),
                 (375, 500, 512)]                                                                    # (H0, W0, P)
SEEDS = (1, 2, 3)
MARGIN_FACTOR, MARGIN_CAP = 32.0, 0.01
Q_MEAN, Q_STD = (0.0, 0.0, 0.0), (1.0 / 255,) * 3            # the table that carries q itself


def exact_shapes():
    """-> [(B, H0, W0, oh, ow)]"""
    return [(B, H0, W0, f * H0, f * W0) for B, H0, W0, f in EXACT_CASES] + [EXACT_RATIO]


def images(B, H0, W0, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (B, H0, W0, 3), generator=g, dtype=torch.uint8)


def exact_images(shape):
    B, H0, W0, oh, ow = shape
    return images(B, H0, W0, 5000 + 31 * H0 + W0)


def q_of(out_q_table):
    """the grey level from an fp32 output produced with (Q_MEAN, Q_STD)"""
    return out_q_table.float().round().clamp(0, 255).to(torch.uint8)


class Reference:
    """fp64 specification of one case + the error scale e and the mask of the pixels whose grey level is decided"""

    def __init__(self, img, oh, ow, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5), reverse_channels=False):
        img = img.cpu()
        self.norm, self.q, self.v = image_load_reference(img, oh, ow, mean, std, reverse_channels, torch.float64)
        v32 = image_load_reference(img, oh, ow, mean, std, reverse_channels, torch.float32)[2]
        self.e = (v32.double() - self.v).abs().max().item()
        frac = self.v - self.v.floor()
        self.decided = (frac - 0.5).abs() >= MARGIN_FACTOR * self.e
        self.undecided_share = 1.0 - self.decided.float().mean().item()
        self.lut = normalisation_table(mean, std)

    def check(self, q_dev, out_dev, what=""):
        """asserts the comparison rule: q_dev uint8 [B, 3, oh, ow], out_dev the normalised output (fp32 or bf16)"""
        assert self.undecided_share <= MARGIN_CAP, (what, self.undecided_share)
        q_dev, out_dev = q_dev.cpu(), out_dev.cpu()
        assert q_dev.shape == self.q.shape and out_dev.shape == self.q.shape, (what, q_dev.shape, out_dev.shape, self.q.shape)
        bad = (q_dev != self.q) & self.decided
        assert not bad.any(), (what, int(bad.sum()), "grey-level mismatches on decided pixels")
        d = (q_dev.int() - self.q.int()).abs().max().item()
        assert d <= 1, (what, "max |q_dev - q_ref|", d)
        # the normalised output is the table entry of the DEVICE's grey level, everywhere (so also where q agrees)
        own = torch.stack([self.lut[c][q_dev[:, c].long()] for c in range(3)], 1).to(out_dev.dtype)
        assert torch.equal(out_dev, own), (what, "normalised output is not the table entry of q")
        agree = q_dev == self.q
        assert torch.equal(out_dev[agree], self.norm.to(out_dev.dtype)[agree]), (what, "normalised output where q agrees")


@functools.lru_cache(maxsize=None)
def general_reference(case, seed):
    """computed once per (case, seed) and shared; nobody writes to it"""
    H0, W0, P = case
    oh, ow = eval_size(H0, W0, P)
    img = images(1, H0, W0, seed)
    return img, oh, ow, Reference(img, oh, ow)
