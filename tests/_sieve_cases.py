"""The label maps of the sieve tests (tests/test_sieve_cpu.py, tests/test_sieve_gpu.py) and the specification's answers on them,
computed once per process and shared.

The maps are the patterns of tests/_regions_cases.py plus one:
  speckled      16 x 50 blocks of constant value with 5 % of the pixels flipped to another value: what a sieve is for
Shapes: the smallest at which the kernels can still go wrong -- one pixel, one row, a map smaller than a wave, a single 16 x 64
tile, four tiles meeting in a corner, partial last tiles, several tiles each way -- and `batch()`'s [3, 17, 65], whose images
touch in equal rows.  int16 maps carry negative values."""
import functools

import torch

import _regions_cases as C

SHAPES = ((1, 1), (1, 65), (3, 2), (16, 64), (17, 65), (33, 129), (48, 200))
PATTERNS = C.PATTERNS + ("speckled",)
INT16_PATTERNS = C.INT16_PATTERNS + ("speckled",)
CONNECTIVITIES = C.CONNECTIVITIES
MIN_REGIONS = (2, 9, 10 ** 6)
BATCHES = ("batch", "batch_short", "batch_speckled")
N = 7                                           # the classes of the moved counter: some values of every pattern lie outside


def clean_blocks(H, W):
    """the 16 x 50 blocks under `speckled`, int64"""
    y = torch.arange(H).reshape(H, 1).expand(H, W)
    x = torch.arange(W).reshape(1, W).expand(H, W)
    return ((y // 16) * 3 + (x // 50) * 2) % 5


def speckled(H, W, dtype=torch.uint8, seed=0):
    g = torch.Generator().manual_seed(77 * H + W + seed)
    base = clean_blocks(H, W)
    flip = torch.rand(H, W, generator=g) < 0.05
    lab = torch.where(flip, (base + torch.randint(1, 5, (H, W), generator=g)) % 5, base)
    return (lab - (2 if dtype == torch.int16 else 0)).to(dtype)


@functools.lru_cache(maxsize=None)
def labels_of(key):
    """key: (pattern, H, W, short) or one of BATCHES"""
    if key == "batch_speckled":
        lab = torch.stack([speckled(17, 65, seed=b) for b in range(3)])
        for b in range(1, 3):
            lab[b, 0] = lab[b - 1, 16]
        return lab
    if isinstance(key, str):
        return C.labels_of(key)
    name, H, W, short = key
    if name == "speckled":
        return speckled(H, W, torch.int16 if short else torch.uint8)
    return C.case(name, H, W, short)


def case_keys(patterns=PATTERNS):
    return [(p, H, W, s) for p in patterns for H, W in SHAPES for s in ((False, True) if p in INT16_PATTERNS else (False,))]


def present_value(key):
    """a value the map holds: its middle pixel's"""
    lab = labels_of(key)
    return int(lab.reshape(-1)[lab.numel() // 2])


def conf_of(key):
    """a confidence plane without a zero in it"""
    lab = labels_of(key)
    g = torch.Generator().manual_seed(5 + lab.numel())
    return torch.rand(lab.shape, generator=g) * 0.5 + 0.25


@functools.lru_cache(maxsize=None)
def reference(key, connectivity, min_region, passes, ignore, raw_labels=False):
    """sieve_reference of a case on the CPU -> (out, moved, conf), computed once and never changed"""
    from ifseg_amd.predict import sieve_reference
    return sieve_reference(labels_of(key), min_region, connectivity, passes, ignore, n=N, raw_labels=raw_labels, conf=conf_of(key))
