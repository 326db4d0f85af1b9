"""The label maps of the region tests (tests/test_regions_cpu.py, tests/test_regions_gpu.py), the specification's answers on them
(computed once per process and shared), and a Python transcription of csrc/regions.hip's decomposition.

Shapes: the smallest at which the kernels can still go wrong -- one pixel, one row, one column, a single 16 x 64 tile, both seams,
a corner where four tiles meet, partial last tiles.  Patterns:
  constant      one region across every seam
  checkerboard  H W single-pixel regions at connectivity 4; two regions that span the image through tile corners only at 8
  serpentine    full even rows joined alternately at the right and the left end: one chain through every tile, the long chase
  rings         nested rings of alternating values: a region enclosing another of the same value without touching it
  random2 / random5   per-pixel random maps over 2 and over 5 values
  blocks        test_render_gpu.make_labels: edges on both seams, single pixels beside them, values outside [0, n)
int16 maps carry negative values."""
import functools
import random

import torch

HS = (1, 3, 16, 17, 33, 48)
WS = (1, 2, 63, 64, 65, 129, 200)
PATTERNS = ("constant", "checkerboard", "serpentine", "rings", "random2", "random5", "blocks")
INT16_PATTERNS = ("checkerboard", "rings", "random5", "blocks")      # where another dtype means other values
CONNECTIVITIES = (4, 8)
TILE_ROWS, TILE_COLS = 16, 64


def pattern(name, H, W, dtype=torch.uint8, seed=0):
    """-> labels [H, W] of `dtype` (uint8 or int16)"""
    short = dtype == torch.int16
    lo, hi = (-5, 300) if short else (0, 1)
    y = torch.arange(H).reshape(H, 1).expand(H, W)
    x = torch.arange(W).reshape(1, W).expand(H, W)
    g = torch.Generator().manual_seed(1000 * H + W + seed)
    if name == "constant":
        lab = torch.full((H, W), -3 if short else 7)
    elif name == "checkerboard":
        lab = torch.where((y + x) % 2 == 0, lo, hi)
    elif name == "serpentine":
        joint = torch.where(y % 4 == 1, x == W - 1, x == 0)           # odd rows: one pixel, right end, then left end, ...
        lab = torch.where((y % 2 == 0) | joint, hi, lo)
    elif name == "rings":
        d = torch.minimum(torch.minimum(y, H - 1 - y), torch.minimum(x, W - 1 - x))
        lab = torch.where(d % 2 == 0, lo, hi)
    elif name in ("random2", "random5"):
        k = int(name[-1])
        lab = torch.randint(0, k, (H, W), generator=g) - (2 if short else 0)
    elif name == "blocks":
        from test_render_gpu import make_labels
        return make_labels(H, W, 5, dtype, 1000 * H + W + seed)
    else:
        raise KeyError(name)
    return lab.to(dtype)


def batch(H=17, W=65, B=3, name="random5", dtype=torch.uint8):
    """[B, H, W]: the last row of one image equals the first row of the next, so regions that joined across images would show"""
    lab = torch.stack([pattern(name, H, W, dtype, seed=b) for b in range(B)])
    for b in range(1, B):
        lab[b, 0] = lab[b - 1, H - 1]
    return lab


@functools.lru_cache(maxsize=None)
def case(name, H, W, short=False):
    return pattern(name, H, W, torch.int16 if short else torch.uint8)


def case_keys(patterns=PATTERNS):
    """every (pattern, H, W, short) of the suite"""
    return [(p, H, W, s) for p in patterns for H in HS for W in WS for s in ((False, True) if p in INT16_PATTERNS else (False,))]


@functools.lru_cache(maxsize=None)
def reference(key, connectivity):
    """regions_reference of a case (or of "batch" / "batch_constant"), on the CPU, computed once and never changed"""
    from ifseg_amd.predict import regions_reference
    root, size = regions_reference(labels_of(key), connectivity)
    return root, size


def labels_of(key):
    if key == "batch":
        return _batches()[0]
    if key == "batch_constant":
        return _batches()[1]
    if key == "batch_short":
        return _batches()[2]
    return case(*key)


@functools.lru_cache(maxsize=None)
def _batches():
    return batch(), batch(16, 64, 3, "constant"), batch(33, 130, 3, "random2", torch.int16)


# ------------------------------------------------------------------------------------ the kernels' decomposition, in Python
def _find(par, a):
    while par[a] != a:
        a = par[a]
    return a


def _tile_pass(lab, H, W, conn):
    """regions_tile_kernel: per tile the runs of a row, the edges to the row above that nothing else implies, a union-find over
    the tile alone -> (root plane of local roots as flat image indices, count plane: the local region's pixels at its root)"""
    root = list(range(H * W))
    for Y0 in range(0, H, TILE_ROWS):
        for X0 in range(0, W, TILE_COLS):
            rows, cols = min(TILE_ROWS, H - Y0), min(TILE_COLS, W - X0)
            at = lambda ry, lx: lab[Y0 + ry][X0 + lx]
            idx = lambda ry, lx: (Y0 + ry) * W + X0 + lx
            edges = []
            for ry in range(rows):
                for lx in range(cols):
                    l = at(ry, lx)
                    hasl, hasr = lx > 0, lx + 1 < cols
                    if hasl and at(ry, lx - 1) == l:
                        edges.append((idx(ry, lx), idx(ry, lx - 1)))            # the row's run
                    if ry < 1:
                        continue
                    up = at(ry - 1, lx)
                    lf = at(ry, lx - 1) if hasl else None
                    ul = at(ry - 1, lx - 1) if hasl else None
                    if up == l:
                        if not (hasl and lf == l and ul == l):
                            edges.append((idx(ry, lx), idx(ry - 1, lx)))
                    elif conn == 8:
                        if hasl and ul == l and lf != l:
                            edges.append((idx(ry, lx), idx(ry - 1, lx - 1)))
                        if hasr and at(ry - 1, lx + 1) == l and at(ry, lx + 1) != l:
                            edges.append((idx(ry, lx), idx(ry - 1, lx + 1)))
            for a, b in edges:
                a, b = _find(root, a), _find(root, b)
                if a != b:
                    root[max(a, b)] = min(a, b)
    count = [0] * (H * W)
    for p in range(H * W):
        root[p] = _find(root, p)            # flat inside a tile, and raster order in a tile is monotone in the flat index
        count[root[p]] += 1
    return root, count


def _seam_pairs(lab, H, W, conn):
    """regions_seam_kernel: the (pixel, neighbour) pairs its threads unite, tile by tile"""
    at = lambda y, x: lab[y][x]
    pairs = []
    for Y0 in range(0, H, TILE_ROWS):
        for X0 in range(0, W, TILE_COLS):
            for k in range(TILE_COLS):                                          # the first row
                x, y = X0 + k, Y0
                if y < 1 or x >= W:
                    continue
                l, up, p = at(y, x), at(y - 1, x), y * W + x
                hasl, hasr = x > 0, x + 1 < W
                lf = at(y, x - 1) if hasl else None
                ul = at(y - 1, x - 1) if hasl else None
                if up == l:
                    if not (hasl and lf == l and ul == l):
                        pairs.append((p, p - W))
                elif conn == 8:
                    if hasl and ul == l and lf != l:
                        pairs.append((p, p - W - 1))
                    if hasr and at(y - 1, x + 1) == l and at(y, x + 1) != l:
                        pairs.append((p, p - W + 1))
            for k in range(TILE_ROWS):                                          # the first column
                x, y = X0, Y0 + k
                if x < 1 or y >= H:
                    continue
                l, lf, p = at(y, x), at(y, x - 1), y * W + x
                if lf == l:
                    pairs.append((p, p - 1))
                elif conn == 8:
                    if y > Y0 and at(y - 1, x - 1) == l and at(y - 1, x) != l:
                        pairs.append((p, p - W - 1))
                    if y + 1 < min(Y0 + TILE_ROWS, H) and at(y + 1, x - 1) == l and at(y + 1, x) != l:
                        pairs.append((p, p + W - 1))
    return pairs


def _union_steps(par, a, b, atomics):
    """seam_union as a generator that yields after every access to the plane, so that a scheduler can interleave many of them
    the way the device's threads interleave: each access is atomic, nothing else is"""
    def find(a):
        while True:
            p = par[a]
            yield
            if p == a:
                return a
            a = p
    a = yield from find(a)
    b = yield from find(b)
    while a != b:
        if a < b:
            a, b = b, a
        old = par[a]                        # atomicMin: the read and the write are one step
        par[a] = min(old, b)
        atomics[0] += 1
        yield
        if old == a:
            return
        a = yield from find(old)
        b = yield from find(b)


def decomposition(labels, connectivity, seed, threads=32):
    """labels [H, W] -> (root, size, atomics) as csrc/regions.hip computes them: tile-local roots, the seam unions in a
    shuffled order with up to `threads` of them in flight and interleaved step by step, the flatten, and the sizes summed from
    the per-tile local counts.  atomics: how many atomicMins the seam pass issued"""
    H, W = labels.shape
    lab = labels.tolist()
    root, count = _tile_pass(lab, H, W, connectivity)
    assert all(root[p] <= p for p in range(H * W))
    pairs = _seam_pairs(lab, H, W, connectivity)
    rng = random.Random(seed)
    rng.shuffle(pairs)
    atomics = [0]
    live, nxt = [], 0
    while live or nxt < len(pairs):
        while len(live) < threads and nxt < len(pairs):
            live.append(_union_steps(root, *pairs[nxt], atomics))
            nxt += 1
        i = rng.randrange(len(live))
        try:
            next(live[i])
        except StopIteration:
            live[i] = live[-1]
            live.pop()
    assert all(root[p] <= p for p in range(H * W))
    out = [_find(root, p) for p in range(H * W)]                                # regions_flatten_kernel
    for p in range(H * W):
        if count[p] > 0 and out[p] != p:
            count[out[p]] += count[p]
    size = [count[out[p]] for p in range(H * W)]                                # regions_gather_kernel
    return (torch.tensor(out, dtype=torch.int32).reshape(H, W), torch.tensor(size, dtype=torch.int32).reshape(H, W), atomics[0])
