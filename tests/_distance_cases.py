"""Inputs shared by test_distance_cpu.py and test_distance_gpu.py: label maps for the distance transform, the specification's
answer for each (computed once per process), a brute-force minimum, a Python transcription of the two kernel passes, and the
trimap cases on tests/_boundary_cases.py's block maps.

A key is (pattern, H, W).  The uint8 map of a key holds small values; its int16 twin holds the same map shifted by -3 (negative
values among them): a bijection on the values, so both have the same distances and share one reference."""
import functools

import torch

import _boundary_cases as BC

SHAPES = [(1, 1), (1, 65), (65, 1), (3, 2), (16, 64), (17, 65), (33, 129), (48, 200)]
PATTERNS = ("constant", "checkerboard", "hstripes", "vstripes", "random2", "random5", "blocks")
RADII = (1, 4, 17, 128)
FAR = 65535
SHIFT = 3                                       # the int16 twin: value - SHIFT


def case_keys(patterns=PATTERNS, shapes=SHAPES):
    return [(p, H, W) for p in patterns for H, W in shapes]


@functools.lru_cache(maxsize=None)
def labels_of(key):
    """-> the uint8 map of a key ([H, W]), or of a named special case"""
    if key == "disc":                           # one pixel of another value in a constant map: a disc cut by the clamp
        lab = torch.full((300, 400), 7, dtype=torch.uint8)
        lab[150, 200] = 2
        return lab
    if key == "table7":                         # 140 x 180 blocks in 300 x 400: pixels farther than 64 exist
        return BC.maps(BC.TABLE[7])[1]
    if key == "batch":                          # three images whose touching rows hold equal values
        top = torch.full((20, 70), 4, dtype=torch.uint8)
        top[:6] = 9                             # image b ends with 4s, image b + 1 begins with 9s ...
        mid = torch.full((20, 70), 4, dtype=torch.uint8)
        mid[:, 40:] = 1
        low = torch.full((20, 70), 4, dtype=torch.uint8)    # ... and a constant image between maps that are not
        return torch.stack([top, low, mid])
    pattern, H, W = key
    g = torch.Generator().manual_seed(1000 * H + W)
    y, x = torch.arange(H)[:, None], torch.arange(W)[None, :]
    if pattern == "constant":
        lab = torch.full((H, W), 5)
    elif pattern == "checkerboard":
        lab = (y + x) % 2 + 1
    elif pattern == "hstripes":
        lab = (y // 3) % 2 + 0 * x
    elif pattern == "vstripes":
        lab = (x // 5) % 3 + 0 * y
    elif pattern == "random2":
        lab = torch.randint(0, 2, (H, W), generator=g)
    elif pattern == "random5":
        lab = torch.randint(0, 5, (H, W), generator=g)
    elif pattern == "blocks":                   # blocks of 11 x 23 with 2 % of the pixels flipped to 255
        lab = 1 + (y // 11) * 10 + x // 23
        lab = torch.where(torch.rand((H, W), generator=g) < 0.02, torch.full_like(lab, 255), lab)
    else:
        raise KeyError(pattern)
    return lab.to(torch.uint8).contiguous()


def labels_as(key, short):
    lab = labels_of(key)
    return (lab.to(torch.int16) - SHIFT).contiguous() if short else lab


@functools.lru_cache(maxsize=None)
def reference(key, R, border):
    from ifseg_amd.predict import distance_reference
    return distance_reference(labels_of(key), R, border)


def clamp(d2, R):
    """exact squared distances (int64, a huge value for none) -> the output at max_distance R, int64"""
    return torch.where(d2 <= R * R, d2, torch.full_like(d2, FAR))


@functools.lru_cache(maxsize=None)
def brute(key, border):
    """the minimum over every pixel of another value, literally, row by row -> int64 [H, W], 2^40 where there is none"""
    lab = labels_of(key).long()
    H, W = lab.shape
    NONE = 1 << 40
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    qy, qx, qv = yy.reshape(-1), xx.reshape(-1), lab.reshape(-1)
    out = torch.empty(H, W, dtype=torch.int64)
    for y in range(H):
        d2 = (qy[None, :] - y) ** 2 + (qx[None, :] - xx[y][:, None]) ** 2
        d2 = torch.where(qv[None, :] != lab[y][:, None], d2, torch.full_like(d2, NONE))
        out[y] = d2.min(1).values
    if border:
        edge = torch.minimum(torch.minimum(xx + 1, W - xx), torch.minimum(yy + 1, H - yy))
        out = torch.minimum(out, edge * edge)
    return out


def two_passes(lab, R, border):
    """A transcription of csrc/distance.hip's two launches, pixel by pixel: (a) v = the clamped vertical distance to another
    value of the column (1 .. R, 255 for none), (b) the scan of the row on both sides, bounded by the pixel's own best
    -> (v, out) as lists of lists"""
    H, W = lab.shape
    L = lab.tolist()
    v = [[255] * W for _ in range(H)]
    for x in range(W):
        for y in range(H):
            for k in range(1, R + 1):
                up = (y - k >= 0 and L[y - k][x] != L[y][x]) or (border and y - k < 0)
                down = (y + k < H and L[y + k][x] != L[y][x]) or (border and y + k >= H)
                if up or down:
                    v[y][x] = k
                    break
    out = [[FAR] * W for _ in range(H)]
    for y in range(H):
        for x in range(W):
            own, best = L[y][x], v[y][x] ** 2
            open_side = {-1: True, 1: True}
            k = 1
            while k <= R and k * k < best and (open_side[-1] or open_side[1]):
                for s in (-1, 1):
                    if not open_side[s]:
                        continue
                    xx = x + s * k
                    if xx < 0 or xx >= W:
                        open_side[s] = False
                        if border:
                            best = min(best, k * k)
                    elif L[y][xx] != own:
                        open_side[s] = False
                        best = min(best, k * k)
                    else:
                        best = min(best, k * k + v[y][xx] ** 2)
                k += 1
            if best <= R * R:
                out[y][x] = best
    return v, out


# ------------------------------------------------------------------------------------------------- the trimap
# entry k of BC.TABLE is counted with TRIMAP_RADII[k]: every ring has pixels in all three rows and scored pixels remain beyond the
# last radius (`trimap_nonempty` states that, and the tests assert it on the reference before they compare anything)
TRIMAP_RADII = [(1, 2, 3), (1, 2, 4), (1, 3, 8), (2, 5, 12), (1, 4, 16, 24), (3, 17, 24), (2, 8, 33, 37), (1, 2, 4, 8, 16, 32, 64, 70)]


@functools.lru_cache(maxsize=None)
def gt_distance(k, raw):
    """the distance plane of entry k's ground truth at its last radius, shared by the entry's label maps"""
    from ifseg_amd.predict import distance_reference
    return distance_reference(BC.maps(BC.TABLE[k], torch.uint8, torch.int16, raw)[1], TRIMAP_RADII[k][-1])


@functools.lru_cache(maxsize=None)
def trimap_reference(k, ldt="u8", raw=True, outside=False):
    """entry k of BC.TABLE -> (trimap, areas) of the specifications; the ground truth's dtype does not change the values"""
    from ifseg_amd.predict import areas_reference, trimap_areas_reference
    labels, gt, n = BC.maps(BC.TABLE[k], BC.DTYPES[ldt], torch.int16, raw, outside)
    return (trimap_areas_reference(labels, gt, n, TRIMAP_RADII[k], raw, dist=gt_distance(k, raw)),
            areas_reference(labels, gt, n, raw)[0])


def trimap_nonempty(k, ldt="u8", raw=True, outside=False):
    """the condition on the inputs: every ring has pixels in all three rows, and scored pixels remain beyond the last radius"""
    trimap, areas = trimap_reference(k, ldt, raw, outside)
    return bool((trimap.sum(2) > 0).all()) and int(trimap[:, 2].sum()) < int(areas[2].sum())
