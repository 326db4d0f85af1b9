"""Inputs shared by test_strong_cpu.py and test_strong_gpu.py: image batches [B, 3, P, P] and records int32 [B, 16] for the
strong augmentation (`ifseg_amd.augment`: strong_draw_reference / strong_apply_reference; csrc/strong.hip), built on the host
from a seed, computed once per case and never written to.

The shapes are the smallest at which the kernel can go wrong on its 16 x 64 tile with a halo of 4: (1, 16) is one tile whose
halo is reflected on all four sides, (3, 16) adds the sample stride, (3, 48) three tile rows and a ragged tile column, (2, 80)
two tile columns -- a halo that crosses the tile boundary at x = 64 and a 16-wide last tile whose right halo reflects."""
import functools

import numpy as np
import torch

from ifseg_amd import augment as A
from ifseg_amd.imageio import HALF, IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD, normalisation_table

SHAPES = [(1, 16), (3, 16), (3, 48), (2, 80)]   # (B, P)
DTYPES = [torch.float32, torch.bfloat16]
STATS = {"half": (HALF, HALF), "imagenet": (IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD)}
KINDS = ("levels", "wild")
SEED = 5
IDENTITY = (4096, 0, 0, 0, 0)
BOX = (456, 455, 455, 455, 455)                 # a caller's box filter: 456 + 8 * 455 = 4096


def f32_bits(x):
    return A.f32_bits(x)


@functools.lru_cache(maxsize=None)
def grey(B, P, seed=0):
    """int64 [B, 3, P, P]: independent random grey levels per pixel (blocks would hide blur errors), the extremes included"""
    g = torch.Generator().manual_seed(1000 * P + 10 * B + seed)
    q = torch.randint(0, 256, (B, 3, P, P), generator=g)
    q[:, :, 0, 0] = 255
    q[:, :, P - 1, P - 1] = 0
    return q


@functools.lru_cache(maxsize=None)
def level_images(B, P, dtype, stats="half", reverse=False, seed=0):
    """[B, 3, P, P]: the grey levels of `grey` sent through the table, as `train_load` writes them (plane c holds colour
    2 - c under `reverse`); every value is a table value"""
    mean, std = STATS[stats]
    lut = normalisation_table(mean, std)
    q = grey(B, P, seed)
    if reverse:
        q = q.flip(1)
    return torch.stack([lut[c][q[:, c]] for c in range(3)], 1).to(dtype)


@functools.lru_cache(maxsize=None)
def wild_images(B, P, dtype, seed=0):
    """[B, 3, P, P] in the style of `_mix_cases.images`: NaNs of several payloads, -0.0, both infinities and values far off
    the table among random values that lie between its levels"""
    g = torch.Generator().manual_seed(7 * P + B + 1000 * seed)
    x = torch.randn(B, 3, P, P, generator=g)
    bits = x.view(torch.int32)
    flat = bits.view(-1)
    flat[0::97] = 0x7fc00000 + seed                 # quiet NaNs
    flat[1::101] = -0x00400000 + 0x10000 * seed     # 0xffc.....: negative NaNs with a payload in the upper half (survives bf16)
    flat[2::89] = -0x80000000                       # -0.0
    flat[3::83] = 0x7f800000                        # +inf
    flat[4::79] = -0x00800000                       # 0xff800000: -inf
    flat[5::73] = 0x42c80000                        # 100.0: off the table
    flat[6::71] = -0x3d380000                       # 0xc2c80000: -100.0
    if dtype == torch.bfloat16:
        return (bits >> 16).to(torch.int16).view(torch.bfloat16)
    return x


def images(kind, B, P, dtype):
    return level_images(B, P, dtype) if kind == "levels" else wild_images(B, P, dtype)


def as_int(img):
    """the integer view images are compared through"""
    return img.contiguous().view(torch.int32 if img.dtype == torch.float32 else torch.int16)


def record(bright=0, contrast=0, sat=0, hue=0, mode=0, beta=0.0, alpha_c=1.0, alpha_s=1.0, delta=0, sigma=-1, w=IDENTITY):
    return [bright, contrast, sat, hue, mode, f32_bits(beta), f32_bits(alpha_c), f32_bits(alpha_s), delta, sigma] + list(w) + [0]


def records_of(B, rec):
    """the same record for every sample -> int32 [B, 16]"""
    return torch.tensor([list(rec)] * B, dtype=torch.int32)


ALL_OFF = record()


@functools.lru_cache(maxsize=None)
def drawn(B, want_jitter, want_blur, seed=SEED):
    """(first_ordinal, records int32 [B, 16]): the first ordinal from which B consecutive drawn records all have the jitter
    gate and the blur gate as asked (the jitter gate counts as on when any of the four operations is)"""
    first = 0
    while True:
        rec = A.strong_draw_reference(B, seed, first)
        jit = (rec[:, :4].sum(1) > 0)
        blur = rec[:, A.S_SIGMA] >= 0
        if bool((jit == want_jitter).all()) and bool((blur == want_blur).all()):
            return first, rec
        first += 1
        assert first < 4096


def record_kinds(B):
    """name -> records int32 [B, 16]: what the apply kernel is run under at every shape"""
    kinds = {"drawn, both on": drawn(B, True, True)[1], "drawn, both off": drawn(B, False, False)[1]}
    ops = {"brightness": dict(bright=1, beta=-17.3125), "contrast": dict(contrast=1, alpha_c=1.37), "saturation": dict(sat=1, alpha_s=0.61),
           "hue": dict(hue=1, delta=-11)}
    for name, kw in ops.items():
        for mode in (0, 1):
            kinds["%s, mode %d" % (name, mode)] = records_of(B, record(mode=mode, **kw))
    kinds["blur, sigma 63"] = records_of(B, record(sigma=63, w=A.BLUR_WEIGHTS[63].tolist()))
    kinds["box filter"] = records_of(B, record(w=BOX))
    kinds["invalid"] = invalid_records(B)
    return kinds


def invalid_ways():
    """the four ways a record is invalid, two variants each: (name, record)"""
    nan, inf = 0x7fc00001, f32_bits(float("inf"))
    full = dict(bright=1, contrast=1, sat=1, hue=1, beta=3.0, alpha_c=1.1, alpha_s=0.9, delta=7)
    ways = [("flag 2", record(**dict(full, sat=2))), ("mode -1", record(**dict(full, mode=-1))),
            ("beta NaN", record(**full)[:5] + [nan] + record(**full)[6:]), ("alpha_s inf", record(**full)[:7] + [inf] + record(**full)[8:]),
            ("negative weight", record(w=(4098, -1, 0, 0, 0))), ("negative w0", record(w=(-4, 1025, 1025, 0, 0))),
            ("sum 4095", record(w=(4095, 0, 0, 0, 0))), ("sum wraps", record(w=(4096, 2 ** 30, 2 ** 30, 0, 0)))]
    return ways


def invalid_records(B):
    """int32 [B, 16]: sample b invalid in way b (cycling), except sample B - 1 of a batch of more than one, which is a valid
    record with everything on -- it must come out untouched by its neighbours"""
    ways = invalid_ways()
    rows = [ways[(3 * b) % len(ways)][1] for b in range(B)]
    if B > 1:
        rows[B - 1] = record(bright=1, contrast=1, sat=1, hue=1, beta=9.5, alpha_c=0.8, alpha_s=1.3, delta=200, sigma=40,
                             w=A.BLUR_WEIGHTS[40].tolist())
    return torch.tensor(rows, dtype=torch.int32)


@functools.lru_cache(maxsize=None)
def literal_levels(dtype, stats):
    """(values [3, N] of `dtype`, int64 [3, N]): every table value, the values around every midpoint and the specials, with
    the grey level counted literally: #{k : fp32(x) >= mid[c][k]}"""
    mean, std = STATS[stats]
    lut = normalisation_table(mean, std)
    mid = torch.from_numpy(A.strong_midpoints(lut.numpy()))
    special = torch.tensor([float("nan"), float("inf"), -float("inf"), 0.0, -0.0, 100.0, -100.0, 1e-40])
    rows, counts = [], []
    for c in range(3):
        around = torch.cat([torch.nextafter(mid[c], torch.tensor(-1e9)), mid[c], torch.nextafter(mid[c], torch.tensor(1e9))])
        x = torch.cat([lut[c], around, special]).to(dtype)
        rows.append(x)
        counts.append((x.float()[:, None] >= mid[c][None, :]).sum(1))
    return torch.stack(rows), torch.stack(counts)


def np_levels(images_t, stats="half", reverse=False):
    """[B, P, P, 3] true colours of a batch by `A.grey_levels`"""
    mean, std = STATS[stats]
    q = A.grey_levels(images_t, mean, std)
    if reverse:
        q = q[:, ::-1]
    return np.moveaxis(q, 1, -1)
