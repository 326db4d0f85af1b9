"""The cases of the region-table tests (tests/test_region_table_cpu.py, tests/test_region_table_gpu.py): tests/_regions_cases.py's
label maps (its shapes x its seven patterns, uint8 and int16 with negative values, its batches whose images touch in equal rows)
under both connectivities, min_region in {1, 9}, ignore in {None, a present value}, max_regions in {1, 7, 4096} and conf in
{None, a random fp32 plane with NaN, a negative value, 1.0 and +inf planted}; a brute-force flood fill that yields the table
region by region in plain Python; and a Python transcription of csrc/regiontab.hip's decomposition.

The regions of a (map, connectivity) come from `_regions_cases.reference`, computed once per process and shared; the table of a
parameter setting is made from them on request and not kept (a table of 4096 rows for every setting would be gigabytes)."""
import functools
import itertools
import random

import numpy as np
import torch

import _regions_cases as C

CONNECTIVITIES = C.CONNECTIVITIES
PATTERNS = C.PATTERNS
BATCHES = ("batch", "batch_constant", "batch_short")
MIN_REGIONS = (1, 9)
MAX_REGIONS = (1, 7, 4096)
# (min_region, ignore a present value, max_regions, with conf): the full product, 24 settings
SETTINGS = tuple(itertools.product(MIN_REGIONS, (False, True), MAX_REGIONS, (False, True)))
TILE_ROWS, TILE_COLS, BLOCK = 16, 64, 1024
SLOTS, PROBES = 512, 8                                                # csrc/regiontab.hip: RT_SLOTS, RT_PROBES


def case_keys(patterns=PATTERNS):
    return C.case_keys(patterns)


def labels_of(key):
    return C.labels_of(key)


def present_value(key):
    """a value the map holds: its first pixel's"""
    return int(labels_of(key).reshape(-1)[0])


@functools.lru_cache(maxsize=None)
def conf_of(key):
    """fp32 in [0, 1) of the labels' shape with NaN, a negative value, 1.0 and +inf planted (as many as the map has pixels for)"""
    lab = labels_of(key)
    g = torch.Generator().manual_seed(7 + lab.numel() + 31 * lab.shape[-1])
    conf = torch.rand(lab.shape, generator=g, dtype=torch.float32)
    flat = conf.reshape(-1)
    n = flat.numel()
    for k, v in enumerate((float("nan"), -0.25, 1.0, float("inf"))):
        flat[(k * 7 + n // 2) % n] = v
    return conf


def arguments(key, setting):
    """-> (conf or None, min_region, ignore, max_regions) of a setting on a case"""
    K, ign, R, with_conf = setting
    return (conf_of(key) if with_conf else None), K, (present_value(key) if ign else None), R


def reference(key, conn, setting):
    """region_table_reference of a case under a setting, its regions shared through `_regions_cases.reference`"""
    from ifseg_amd.predict import region_table_reference
    conf, K, ignore, R = arguments(key, setting)
    return region_table_reference(labels_of(key), conf, conn, K, ignore, R, regions=C.reference(key, conn))


def written(rows, sums, count, R):
    """the written rows of a table as [B, R, .] tensors -> per image (rows[:k], sums[:k]), k = min(count, R)"""
    rows, sums, count = rows.reshape(-1, R, 8), sums.reshape(-1, R, 3), count.reshape(-1)
    return [(rows[b, :min(int(count[b]), R)], sums[b, :min(int(count[b]), R)]) for b in range(rows.shape[0])]


# ------------------------------------------------------------------------------------------ brute force: a flood fill per region
def q16(conf):
    """the 16-bit fixed point of fp32 confidences, in numpy: clamp(floor(c * 65536), 0, 65535) in fp32, NaN -> 0"""
    c = np.asarray(conf, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.floor(c * np.float32(65536.0))
    q = np.where(np.isnan(q), np.float32(0.0), q)
    return np.clip(q, 0.0, 65535.0).astype(np.int64)


@functools.lru_cache(maxsize=None)
def flood(key, conn):
    """per image the regions of a case found by flood fill from every unvisited pixel in raster order -> a list (per image) of
    lists of dicts(value, root, size, x0, y0, x1, y1, sx, sy, sq, pixels); sq from `conf_of(key)`"""
    lab = labels_of(key)
    H, W = lab.shape[-2:]
    maps = lab.reshape(-1, H, W).tolist()
    qs = q16(conf_of(key).numpy()).reshape(-1, H, W).tolist()
    steps = [(0, 1), (1, 0), (0, -1), (-1, 0)] + ([(1, 1), (1, -1), (-1, 1), (-1, -1)] if conn == 8 else [])
    out = []
    for m, q in zip(maps, qs):
        seen = [[False] * W for _ in range(H)]
        regions = []
        for y0 in range(H):
            for x0 in range(W):
                if seen[y0][x0]:
                    continue
                v, stack, pixels = m[y0][x0], [(y0, x0)], []
                seen[y0][x0] = True
                while stack:
                    y, x = stack.pop()
                    pixels.append((y, x))
                    for dy, dx in steps:
                        yy, xx = y + dy, x + dx
                        if 0 <= yy < H and 0 <= xx < W and not seen[yy][xx] and m[yy][xx] == v:
                            seen[yy][xx] = True
                            stack.append((yy, xx))
                ys, xs = [p[0] for p in pixels], [p[1] for p in pixels]
                regions.append(dict(value=v, root=y0 * W + x0, size=len(pixels), x0=min(xs), y0=min(ys), x1=max(xs), y1=max(ys),
                                    sx=sum(xs), sy=sum(ys), sq=sum(q[y][x] for y, x in pixels), pixels=pixels))
        out.append(regions)                                                         # raster discovery: ascending root
    return out


def flood_table(key, conn, setting):
    """the table of a case from `flood`'s regions, in plain Python -> per image (rows, sums, count, slot) as lists"""
    _, K, ignore, R = arguments(key, setting)
    with_conf = setting[3]
    H, W = labels_of(key).shape[-2:]
    out = []
    for regions in flood(key, conn):
        listed = [r for r in regions if r["size"] >= K and (ignore is None or r["value"] != ignore)]
        assert [r["root"] for r in listed] == sorted(r["root"] for r in listed)
        slot = [[-1] * W for _ in range(H)]
        rows, sums = [], []
        for s, r in enumerate(listed[:R]):
            rows.append([r["value"], r["root"], r["size"], r["x0"], r["y0"], r["x1"], r["y1"], 0])
            sums.append([r["sx"], r["sy"], r["sq"] if with_conf else 0])
            for y, x in r["pixels"]:
                slot[y][x] = s
        out.append((rows, sums, len(listed), slot))
    return out


# ------------------------------------------------------------------------------------ the kernels' decomposition, in Python
def decomposition(labels, root, size, conf, min_region, ignore, R, seed):
    """labels / root / size [H, W] (one image; root and size as hip.seg_regions gives them) -> (rows, sums, count, slot, direct)
    as csrc/regiontab.hip computes them: the listed roots counted per block of 1024 flat pixels, the blocks' counts scanned, the
    ranks from the block's offset and the flags in front, and per 16 x 64 tile the row runs reduced into a table of SLOTS
    entries with PROBES linear probes -- the runs of a tile in a shuffled order, the tiles in a shuffled order, every entry's
    flush and every direct run applied to the rows as min / max / add in a shuffled order.  rows beyond min(count, R) stay
    None.  direct: how many runs found no entry and went to their row themselves"""
    H, W = labels.shape
    HW = H * W
    lab, rt, sz = labels.reshape(-1).tolist(), root.reshape(-1).tolist(), size.reshape(-1).tolist()
    q = q16(conf.numpy()).reshape(-1).tolist() if conf is not None else None
    rng = random.Random(seed)
    flagged = [rt[p] == p and sz[p] >= min_region and (ignore is None or lab[p] != ignore) for p in range(HW)]
    # (a) block counts
    nblk = -(-HW // BLOCK)
    blk = [sum(flagged[k * BLOCK:min((k + 1) * BLOCK, HW)]) for k in range(nblk)]
    # (b) scan, 256 blocks at a time with a carried total
    carry, offs = 0, []
    for base in range(0, nblk, 256):
        part = blk[base:base + 256]
        run = 0
        for v in part:
            offs.append(carry + run)
            run += v
        carry += run
    count = carry
    # (c) rows: the rank of a flagged root = its block's offset + the flags in front of it inside the block
    rows, sums, slot = [None] * R, [None] * R, [None] * HW
    for k in rng.sample(range(nblk), nblk):
        first = k * BLOCK
        groups = [sum(flagged[first + 64 * g:min(first + 64 * g + 64, HW)]) for g in range(BLOCK // 64)]
        in_front = [sum(groups[:g]) for g in range(BLOCK // 64)]
        below = 0                                                                   # the ballot's bits below the lane
        for p in range(first, min(first + BLOCK, HW)):
            g, lane = (p - first) // 64, (p - first) % 64
            if lane == 0:
                below = 0
            mine = below
            below += flagged[p]
            if rt[p] != p:
                continue
            s = -1
            if flagged[p]:
                s = offs[k] + in_front[g] + mine
                if s < R:
                    rows[s] = [lab[p], p, sz[p], 2 ** 31 - 1, 2 ** 31 - 1, -1, -1, 0]
                    sums[s] = [0, 0, 0]
                else:
                    s = -1
            slot[p] = s
    # (d) statistics
    updates, direct = [], 0            # (slot, x0, y0, x1, y1, sx, sy, sq) on a row
    tiles = [(Y0, X0) for Y0 in range(0, H, TILE_ROWS) for X0 in range(0, W, TILE_COLS)]
    final = list(slot)
    for Y0, X0 in tiles:
        runs = []
        for y in range(Y0, min(Y0 + TILE_ROWS, H)):
            x = X0
            xend = min(X0 + TILE_COLS, W)
            while x < xend:
                r = rt[y * W + x]
                e = x
                while e + 1 < xend and rt[y * W + e + 1] == r:
                    e += 1
                s = slot[r]
                assert s is not None                                                # the rows launch wrote every root's word
                for xx in range(x, e + 1):
                    final[y * W + xx] = s
                if s >= 0:
                    length = e - x + 1
                    sq = sum(q[y * W + xx] for xx in range(x, e + 1)) if q is not None else 0
                    runs.append((s, x - X0, y - Y0, e - X0, length, (x - X0 + e - X0) * length // 2, (y - Y0) * length, sq))
                x = e + 1
        rng.shuffle(runs)
        keys, table = [None] * SLOTS, {}
        for s, lx0, ly, lx1, length, sx, sy, sq in runs:
            e = ((s * 2654435761) & 0xffffffff) >> (32 - 9)
            for _ in range(PROBES):
                if keys[e] is None or keys[e] == s:
                    break
                e = (e + 1) & (SLOTS - 1)
            else:
                e = None
            if e is None:
                direct += 1
                updates.append((s, X0 + lx0, Y0 + ly, X0 + lx1, Y0 + ly, sx + length * X0, sy + length * Y0, sq))
                continue
            keys[e] = s
            t = table.setdefault(e, [2 ** 31 - 1, 2 ** 31 - 1, 0, 0, 0, 0, 0, 0])
            t[0], t[1], t[2], t[3] = min(t[0], lx0), min(t[1], ly), max(t[2], lx1), max(t[3], ly)
            t[4], t[5], t[6], t[7] = t[4] + length, t[5] + sx, t[6] + sy, t[7] + sq
            assert max(t[4:]) < 2 ** 32                                             # the entries are uint32
        for e, t in table.items():
            updates.append((keys[e], X0 + t[0], Y0 + t[1], X0 + t[2], Y0 + t[3], t[5] + t[4] * X0, t[6] + t[4] * Y0, t[7]))
    rng.shuffle(updates)
    for s, x0, y0, x1, y1, sx, sy, sq in updates:
        assert 0 <= s < R and rows[s] is not None
        r = rows[s]
        r[3], r[4], r[5], r[6] = min(r[3], x0), min(r[4], y0), max(r[5], x1), max(r[6], y1)
        sums[s][0] += sx
        sums[s][1] += sy
        sums[s][2] += sq
    return rows, sums, count, final, direct
