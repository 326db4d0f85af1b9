"""Inputs, records and comparison helpers shared by test_train_load_cpu.py and test_train_load_gpu.py.

Label maps (raw uint8, the dataset's convention: 0 and 255 are 'unknown', x is class x - 1):
  checker   a 1-pixel checkerboard of two classes: every window is half / half, so crop candidate 0 is always taken;
  flat      one class: no window passes, candidate 10 is always taken;
  mixed     the left 70 % one class, the right 30 % horizontal stripes of two others: a window passes only where it reaches far
            enough into the stripes.

Exact family: sources upscaled by the factor 4 (16 x 24 -> 64 x 96 at P = 64, 36 x 24 -> 144 x 96 at P = 96; a factor that is
no power of two, such as 24 x 16 -> 144 x 96, has weights in twelfths, which fp32 does not hold).  Every bilinear weight is a
multiple of 1/8 per axis, so every product of two weights and a grey level and every sum is exact in fp32: the fp32 and the fp64
specification are identical and any summation order or FMA contraction gives the same bits (the argument of
_image_load_cases.py).  The records are written by hand and cover both modes, every stage on and off, both ends of delta,
beta and alpha, flip on and off and the offsets 0 and maximal.

General family: arbitrary ratios, records drawn.  The resize obeys the rule of `_image_load_cases.Reference` (MARGIN_FACTOR 32,
MARGIN_CAP 1 %) on the whole resized image, read on the window; behind it everything is integer and must be exact.
"""
import functools

import numpy as np
import torch

import _image_load_cases as IC
from ifseg_amd import augment as A

NSEG, SEG0 = 5, 1000
GENERAL_SOURCES = [(97, 61), (33, 250), (300, 200), (1500, 1000)]          # the last one: the direct-global path on its own
RAGGED = [(37, 29), (16, 24), (64, 160), (90, 41), (50, 120)]              # the draw test's batch
DRAW_ORDINALS = (0, 2 ** 32 - 5)
CROP_SEED = 3                                                              # test_train_load_cpu asserts what it has to deliver


def image(H0, W0, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (H0, W0, 3), generator=g, dtype=torch.uint8)


def label(kind, H0, W0):
    y, x = torch.meshgrid(torch.arange(H0), torch.arange(W0), indexing="ij")
    if kind == "checker":
        m = 1 + (y + x) % 2
    elif kind == "flat":
        m = torch.full((H0, W0), 3)
    elif kind == "mixed":
        m = torch.where(x < (7 * W0) // 10, torch.full_like(x, 1), 2 + (y // 2) % 2)
    elif kind == "random":                      # every raw value, 0 and 255 among them
        g = torch.Generator().manual_seed(H0 * 1000 + W0)
        m = torch.randint(0, 256, (H0, W0), generator=g)
        m = torch.where(m > NSEG + 2, m % 2 * 255, m)
    else:
        raise ValueError(kind)
    return m.to(torch.uint8).contiguous()


KINDS = ("checker", "flat", "mixed", "random", "mixed")


def ragged_batch():
    """-> (images, labels) of the RAGGED shapes, one label kind each"""
    return ([image(h, w, 100 + i) for i, (h, w) in enumerate(RAGGED)], [label(KINDS[i], h, w) for i, (h, w) in enumerate(RAGGED)])


def record(new_h, new_w, off_h, off_w, flip=0, bright=0, contrast=0, sat=0, hue=0, mode=0, beta=0.0, alpha_c=1.0, alpha_s=1.0,
           delta=0, k=0):
    return [new_h, new_w, off_h, off_w, k, flip, bright, contrast, sat, hue, mode, A.f32_bits(beta), A.f32_bits(alpha_c),
            A.f32_bits(alpha_s), delta, 0]


LO, HI = 0.5, 1.5 - 2.0 ** -23                    # the ends of alpha's grid
BLO, BHI = -32.0, 32.0 - 2.0 ** -17               # the ends of beta's grid


def exact_family(which):
    """-> (P, images, labels, params int32 [8, 16]): eight samples of one exact-family source under hand-written records"""
    H0, W0, new_h, new_w, P = (16, 24, 64, 96, 64) if which == 0 else (36, 24, 144, 96, 96)
    mh, mw = new_h - P, new_w - P
    recs = [
        record(new_h, new_w, 0, 0),                                                                    # identity chain
        record(new_h, new_w, mh, mw, 1, 1, 1, 1, 1, 0, BLO, LO, LO, -18),                              # all on, mode 0, low ends
        record(new_h, new_w, mh, mw, 0, 1, 1, 1, 1, 1, BHI, HI, HI, 17),                               # all on, mode 1, high ends
        record(new_h, new_w, 0, mw, 1, bright=1, beta=32.0),                                           # one stage at a time
        record(new_h, new_w, mh, 0, 0, contrast=1, mode=1, alpha_c=HI),
        record(new_h, new_w, mh // 2, mw // 2, 1, sat=1, alpha_s=LO),
        record(new_h, new_w, min(1, mh), min(1, mw), 0, hue=1, delta=17, sat=1, alpha_s=HI),
        record(new_h, new_w, 0, 0, 1, hue=1, delta=-18, contrast=1, mode=0, alpha_c=LO),
    ]
    imgs = [image(H0, W0, 7000 + 10 * which + i) for i in range(len(recs))]
    labs = [label(KINDS[i % len(KINDS)], H0, W0) for i in range(len(recs))]
    return P, imgs, labs, torch.tensor(recs, dtype=torch.int32)


@functools.lru_cache(maxsize=None)
def exact_reference(which, out_dtype=torch.float32, reverse_channels=False):
    """the specification's (patch_images, target, q, q0) of an exact family, computed once and shared; nobody writes to it"""
    P, imgs, labs, params = exact_family(which)
    return A.train_load_reference(imgs, labs, params, P, NSEG, SEG0, reverse_channels=reverse_channels, dtype=torch.float32,
                                  out_dtype=out_dtype)


@functools.lru_cache(maxsize=None)
def general_case(i, P=64, seed=11):
    """source i of GENERAL_SOURCES under a drawn record -> (image, label, record [16] with the photometric stage on, the
    `_image_load_cases.Reference` of the whole resized image, window rows, window columns)"""
    H0, W0 = GENERAL_SOURCES[i]
    img, lab = image(H0, W0, 300 + i), label("random", H0, W0)
    rec = A.draw_params([(H0, W0)], [lab], P, NSEG, seed, 40 + i)[0]
    rec[A.R_BRIGHT:A.R_HUE + 1] = 1                                  # every photometric stage, whatever the bits were
    new_h, new_w, off_h, off_w = rec[:4].tolist()
    ref = IC.Reference(img[None], new_h, new_w)
    ys = off_h + torch.arange(P)
    xs = off_w + (torch.arange(P - 1, -1, -1) if int(rec[A.R_FLIP]) else torch.arange(P))
    return img, lab, rec, ref, ys, xs


def check_resize(ref, ys, xs, q_dev, what=""):
    """`_image_load_cases.Reference`'s rule on the window: q_dev uint8 [P, P, 3] (RGB) against the fp64 specification of the
    whole resized image"""
    assert ref.undecided_share <= IC.MARGIN_CAP, (what, ref.undecided_share)
    want = ref.q[0][:, ys][:, :, xs].permute(1, 2, 0)
    decided = ref.decided[0][:, ys][:, :, xs].permute(1, 2, 0)
    q_dev = q_dev.cpu()
    bad = (q_dev != want) & decided
    assert not bad.any(), (what, int(bad.sum()), "grey-level mismatches on decided pixels")
    d = (q_dev.int() - want.int()).abs().max().item()
    assert d <= 1, (what, "max |q_dev - q_ref|", d)


def target_of(lab, rec, P):
    """the expected target of one sample, written out independently of train_load_reference: raw remap, nearest resize by the
    integer rule, window, flip, offset, EOS"""
    new_h, new_w, off_h, off_w = (int(v) for v in rec[:4])
    H0, W0 = lab.shape
    raw = lab.long().numpy()
    cls = np.where((raw == 0) | (raw == 255), NSEG, np.minimum(raw - 1, NSEG))
    out = np.empty((P, P), dtype=np.int64)
    for y in range(P):
        sy = min((off_h + y) * H0 // new_h, H0 - 1)
        for x in range(P):
            xs = off_w + (P - 1 - x if int(rec[A.R_FLIP]) else x)
            out[y, x] = cls[sy, min(xs * W0 // new_w, W0 - 1)]
    return torch.cat([torch.from_numpy(out).reshape(-1) + SEG0, torch.tensor([2])])
