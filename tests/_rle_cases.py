"""The cases of the run-length tests (tests/test_rle_cpu.py, tests/test_rle_gpu.py): small label maps whose rows and columns are
no multiples of the chunk (32 rows) or of a workgroup's 64 columns, H = 1 (every step crosses a column boundary), a single
column; the specification's answers on them (computed once per process and shared); a literal loop over f; and Python
transcriptions of csrc/rle.hip's three encode launches and of its decoder's search-and-walk.

Patterns:
  constant      one run
  checkerboard  961 runs at 16 x 64 (H even: the run goes on across each of the 63 column seams), 1105 at 17 x 65 (one per pixel)
  hstripes      rows of alternating values: a run per pixel of a column
  vstripes      columns of alternating values: a run per column
  random5       per-pixel random over 5 values
  blocks        the region tests' make_labels: edges on the seams, single pixels, values outside [0, n)
int16 maps carry negative values."""
import functools

import torch

import _regions_cases as C

SHAPES = ((1, 1), (1, 65), (65, 1), (3, 2), (16, 64), (17, 65), (33, 129), (48, 200))
PATTERNS = ("constant", "checkerboard", "hstripes", "vstripes", "random5", "blocks")
INT16_PATTERNS = ("checkerboard", "hstripes", "random5", "blocks")
BATCHES = ("batch", "batch_constant", "batch_short")
MAX_RUNS = (1, 7, 16384)                                              # 16384 >= 48 x 200: at or above every count
CHUNK, COLS, ROWS = 32, 64, 8                                         # csrc/rle.hip: RL_CHUNK, RL_COLS, RL_ROWS


def pattern(name, H, W, dtype=torch.uint8, seed=0):
    short = dtype == torch.int16
    lo, hi = (-5, 300) if short else (0, 255)
    y = torch.arange(H).reshape(H, 1).expand(H, W)
    x = torch.arange(W).reshape(1, W).expand(H, W)
    if name == "hstripes":
        return torch.where(y % 2 == 0, lo, hi).to(dtype)
    if name == "vstripes":
        return torch.where(x % 2 == 0, lo, hi).to(dtype)
    return C.pattern(name, H, W, dtype, seed)


@functools.lru_cache(maxsize=None)
def case(name, H, W, short=False):
    return pattern(name, H, W, torch.int16 if short else torch.uint8)


def case_keys(patterns=PATTERNS):
    return [(p, H, W, s) for p in patterns for H, W in SHAPES for s in ((False, True) if p in INT16_PATTERNS else (False,))]


@functools.lru_cache(maxsize=None)
def _batches():
    """[3, H, W]: the last position of one image (its bottom right pixel) equals the first of the next (its top left one)"""
    out = []
    for H, W, name, dtype in ((17, 65, "random5", torch.uint8), (16, 64, "constant", torch.uint8), (33, 130, "random5", torch.int16)):
        lab = torch.stack([pattern(name, H, W, dtype, seed=b) for b in range(3)])
        for b in range(1, 3):
            lab[b, 0, 0] = lab[b - 1, H - 1, W - 1]
        out.append(lab)
    return tuple(out)


def labels_of(key):
    if key in BATCHES:
        return _batches()[BATCHES.index(key)]
    return case(*key)


@functools.lru_cache(maxsize=None)
def reference(key, R):
    """rle_encode_reference of a case, on the CPU, computed once and never changed -> (runs, count)"""
    from ifseg_amd.predict import rle_encode_reference
    return rle_encode_reference(labels_of(key), R)


def written(runs, count, R):
    """[B, R, 2] / [B] (or without B) -> per image runs[:min(count, R)]"""
    runs, count = runs.reshape(-1, R, 2), count.reshape(-1)
    return [runs[b, :min(int(count[b]), R)] for b in range(runs.shape[0])]


# ------------------------------------------------------------------------------------------ the rule, literally
def literal(lab2d):
    """one image [H, W] -> the list of (start, value) from a plain loop over f[i] = labels[i % H][i // H]"""
    H, W = lab2d.shape
    rows = lab2d.tolist()
    out, prev = [], None
    for i in range(H * W):
        v = rows[i % H][i // H]
        if i == 0 or v != prev:
            out.append([i, v])
        prev = v
    return out


# ------------------------------------------------------------------------------------ the encode launches, in Python
def encode_decomposition(lab2d, R):
    """one image [H, W] -> (runs as a list of R entries, None where never written; count) as csrc/rle.hip computes them: per
    (64 columns x 32 rows) workgroup the four waves' per-column counts of run starts, one count per segment (x, chunk) at
    x nchunk + chunk; the scan, 256 segments at a time with a carried total; and the ranks = the segment's offset + the counts
    of the waves above in the same column + the thread's running count"""
    H, W = lab2d.shape
    rows = lab2d.tolist()
    nchunk, ncg = -(-H // CHUNK), -(-W // COLS)

    def walk(x, y0):
        """the thread of column x from row y0: -> [(j, value)] of the rows that start a run"""
        if x >= W or y0 >= H:
            return []
        none = False
        prev = None
        if y0 > 0:
            prev = rows[y0 - 1][x]
        elif x > 0:
            prev = rows[H - 1][x - 1]
        else:
            none = True
        out = []
        for j in range(ROWS):
            if y0 + j >= H:
                break
            v = rows[y0 + j][x]
            if (j == 0 and none) or v != prev:
                out.append((j, v))
            prev = v
        return out

    # (a) the count launch
    seg = [None] * (W * nchunk)
    cnt = {}
    for cg in range(ncg):
        for ck in range(nchunk):
            for lane in range(COLS):
                x = cg * COLS + lane
                per_wave = [len(walk(x, ck * CHUNK + w * ROWS)) for w in range(4)]
                cnt[(cg, ck, lane)] = per_wave
                if x < W:
                    seg[x * nchunk + ck] = sum(per_wave)
    assert all(s is not None for s in seg)
    # (b) the scan
    carry, offs = 0, []
    for base in range(0, len(seg), 256):
        run = 0
        for v in seg[base:base + 256]:
            offs.append(carry + run)
            run += v
        carry += run
    count = carry
    # (c) the write launch
    runs = [None] * R
    for cg in reversed(range(ncg)):                                                 # any order of workgroups
        for ck in range(nchunk):
            for w in (2, 0, 3, 1):
                for lane in range(COLS):
                    x, y0 = cg * COLS + lane, ck * CHUNK + w * ROWS
                    starts = walk(x, y0)
                    if not starts:
                        continue
                    s = offs[x * nchunk + ck] + sum(cnt[(cg, ck, lane)][:w])
                    for j, v in starts:
                        if s < R:
                            assert runs[s] is None                                  # one writer per entry
                            runs[s] = [x * H + y0 + j, v]
                        s += 1
    return runs, count


# ------------------------------------------------------------------------------------ the decoder's search and walk, in Python
def decode_decomposition(runs, count, H, W, fill=255):
    """runs: a list of [start, value] of length R, count -> (the map as rows of ints, flag, reads) as rle_decode_kernel computes
    it: per thread (column x, eight rows from y0) a binary search of start[0 .. m) for x H + y0, then the walk down.  reads:
    every index the threads read of the table, which must lie in [0, m)"""
    R = len(runs)
    m = min(count, R)
    flag = (1 if count > R else 0) | (2 if m <= 0 or runs[0][0] != 0 else 0)
    out = [[None] * W for _ in range(H)]
    reads = set()
    if m > 0:
        reads.add(0)
    big = 2 ** 31 - 1

    def entry(s):
        assert 0 <= s < m, (s, m)
        reads.add(s)
        return runs[s]

    for x in range(W):
        for y0 in range(0, H, ROWS):
            if m <= 0:
                for j in range(min(ROWS, H - y0)):
                    out[y0 + j][x] = fill
                continue
            first = x * H + y0
            lo, hi = 0, m
            while hi - lo > 1:
                mid = lo + ((hi - lo) >> 1)
                if entry(mid)[0] <= first:
                    lo = mid
                else:
                    hi = mid
            s, val = lo, entry(lo)[1]
            nxt = entry(s + 1) if s + 1 < m else [big, 0]
            steps = 0
            for j in range(min(ROWS, H - y0)):
                while nxt[0] <= first + j:
                    val = nxt[1]
                    s += 1
                    steps += 1
                    nxt = entry(s + 1) if s + 1 < m else [big, 0]
                out[y0 + j][x] = val
            assert steps <= m
    return out, flag, reads
