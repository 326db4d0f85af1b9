"""Data, fp64 references, derived bounds, fp32 restatements and case tables of the stem / FFN-LayerNorm-fold conformance suite
(test_stem_ffn_conformance_cpu.py checks them without a GPU, test_stem_ffn_conformance_gpu.py holds the kernels of csrc/conv.hip,
csrc/ffn_ln.hip and nchw_to_nhwc of csrc/rowops.hip to them through the C ABI).  Plain numpy; nothing here imports ifseg_amd.

u = 2^-24 is one fp32 rounding; a bf16 store is 2^-8 |ref|.  Every bound is a formula of the reference's own magnitudes.
Four things below are not the issue's starting forms as written, each by derivation and none by observation (DESIGN.md lists the
same four): the chain length d of coef, d and the extra u of rowstats, the zero-addition argument behind param_grads' (J + 4) u at
small J, and the floor 2^-102 of the three-term weight identity (test_stem_weights_three_terms draws its weights above it).

Layout (nchw_to_nhwc): exact.  bf16(x) to nearest even, pad channels +0, -0 / inf / NaN kept: compared as bits.

Stem, out = bf16(relu(conv7x7/2(x, w) + shift)), 64 channels, x NHWC(4) bf16:
  exact    integer images in [-4, 4], weights odd multiples of 2^-10 in (1/2, 1) (10 significant bits: two bf16 terms, the third
           is zero), integer shifts in [40, 48] (so that fewer than 10 % of the outputs vanish behind the ReLU; the sums have a
           standard deviation of about 24).  Every partial sum is a multiple of 2^-10 below 2^10: 20 bits, exact in any order.
  isolate  one pixel of value 1 per image, w = 1 + 2^-9 + q 2^-23 (1 <= q < 64, a different q for every tap and channel), shift
           -(1 + 2^-9): the three bf16 terms are 1, 2^-9 and q 2^-23, and the output where the tap meets the pixel is q 2^-23.
  random   bf16 randn images, 0.1 randn fp32 weights and shifts:  |out - relu(ref)| <= 2^-8 |ref| + (K + 4) 2^-23 mag,
           K = 147, mag = sum |w x| + |shift| (direct kernel);  K = 3 * 224, mag = sum (|t0| + |t1| + |t2|) |x| + |shift| (matrix
           cores: 14 k-steps of 16 for each of the three terms).
  nonfinite  torch's contract: an output whose 7 x 7 window holds a NaN is NaN, relu(+inf) = +inf, relu(-inf) = +0 (the kernels' ReLU is
           the IEEE maximum, which keeps NaN).  The matrix-core kernel multiplies the zero weights of its padded tap kx = 7 (input
           column 2 ox + 4) with real pixels: a non-finite value there makes the output NaN as well (0 * NaN, 0 * inf) --
           include/ifseg_hip.h documents it, `stem_nonfinite_expect` states it.

Max-pool 3x3/2 pad 1: exact against the fp64 window maximum (NaN in the window -> NaN; compared as values, so -0 == +0).

ffn_ln_coef, one wave per row of W2 [J, N]: a lane sums `sa += w0 g0 + ... + w7 g7` once per trip of 512 columns, then six
  DPP steps.  The longest chain of additions a product passes through: 7 inside the expression, 1 into sa, trips - 1 further
  trips, 6 steps:  d = ceil(N / 512) + 13.   |a_j - ref| <= (d + 1) u sum_k |w gamma| (the product's own rounding is the + 1);
  wb_j: (d + 2) u (sum_k |w beta| + |b2_j|).
ffn_ln_rowstats, one wave per row: `s1 += d[e] * a[e]` element by element, 8 per trip of 512, then six steps: d = 8 ceil(J / 512) + 6.
  The starting form (d + 2) counts the product and the multiplication by 1 / N; the kernel multiplies by inv_n = 1.f / N, which
  is itself rounded unless N is a power of two: one more u there (`rowstats_extra`).
      c1: (d + 2 + x) u sum_j |dY_j a_j| / N      c2: [u sum_j |dY_j| |t_j - wb_j| + (d + 2 + x) u sum_j |dY_j (t_j - wb_j)|] / N
ffn_ln_param_grads (no rescue): a column's J products are summed over 8 slabs x 16 row lanes in a fixed order; additions of the
  exact zeros of idle lanes and slabs cost nothing, so J terms cost at most J - 1 roundings however they are grouped:
      E_wd = (J + 4) u sum_j |w dW2|, E_db = (J + 4) u sum_j |w db2|,   dbeta: 2^-8 |ref| + E_db,
      dgamma: 2^-8 |ref| + [E_wd + |beta| E_db + 3 u (|swd| + |beta sdb|)] / |gamma|;  gamma == 0 -> +0.
  semantic check: dW2, db2 the bf16 roundings of the fp64 weight gradient of LN(gelu(u)) W2^T + b2, reference the dgamma of the
  definition; the bound above plus the inputs' own rounding 2^-8 (sum_j |W2 dW2| + |beta| sum_j |W2 db2|) / |gamma|.
rescue kernel, per flagged column k: dz_m = sum_j dY[m][j] w[j] sequentially (J + 2 with the product), gelu by erf_as (4 u |uv| + 8 u,
  _rowops_cases), (g - mean) rstd and the product with dz three roundings, a thread's ceil(M / 256) terms and an 8-level tree:
      2^-8 |ref| + sum_m [(J + 2) u sum_j |dY w| |xhat| + |dz| (4 u |uv| + 8 u) rstd + 3 u |dz xhat|] + (ceil(M / 256) + 8) u sum_m |dz xhat|
"""
import functools
import math

import numpy as np

from _rowops_cases import F32, U, U_BF16, bf16_round, erf_as, gelu_f32, is_bf16, is_f32, worst_ratio  # noqa: F401

F64 = np.float64
ST_TH, ST_TW, GRID_CAP = 8, 32, 1024


def rng(seed):
    return np.random.default_rng(seed)


def bf(a):
    """nearest bf16 values as float64"""
    return bf16_round(np.asarray(a, dtype=F32)).astype(F64)


def bits16(a):
    """bf16 bit patterns (uint16) of float32 values that are bf16-representable"""
    return (np.ascontiguousarray(a, dtype=F32).view(np.uint32) >> 16).astype(np.uint16)


def within(got, ref, bound):
    return worst_ratio(got, ref, bound)[0]


# ===================================================================================================== layout
LAYOUT_SHAPES = ((1, 3, 1, 1, 4), (2, 3, 5, 7, 4), (3, 1, 9, 2, 8), (1, 4, 3, 3, 4))      # (B, C, H, W, Cpad)
# fp32 bit patterns: ties of the bf16 rounding (low half 0x8000) over an even and an odd upper half, both signs, next to a
# carry into the exponent and into infinity, just off the tie, -0, infinities, a quiet and a signalling-pattern NaN, denormals
TIE_BITS = (0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3FFF8000, 0x7F7F8000, 0x3F808001, 0x3F817FFF, 0x80000000, 0x00000000,
            0x7F800000, 0xFF800000, 0x7FC00000, 0x7F800001, 0x00008000, 0x00018000, 0x807F8000, 0x3F800000)
TIE_WANT = (0x3F80, 0x3F82, 0xBF80, 0xBF82, 0x4000, 0x7F80, 0x3F81, 0x3F81, 0x8000, 0x0000,
            0x7F80, 0xFF80, 0x7FC0, 0x7FC0, 0x0000, 0x0002, 0x8080, 0x3F80)


def layout_input(shape, f32, seed=3):
    """NCHW values (float32; bf16-representable unless f32) that start with the tie vector"""
    B, C, H, W, _ = shape
    n = B * C * H * W
    v = (rng(seed).standard_normal(n) * 3).astype(F32)
    t = np.array(TIE_BITS, dtype=np.uint32).view(F32)
    if not f32:
        v, t = bf16_round(v), bf16_round(t)
    k = min(n, t.size)
    v[:k] = t[:k]
    return v.reshape(B, C, H, W)


def layout_ref_bits(x, Cpad):
    B, C, H, W = x.shape
    out = np.zeros((B, H, W, Cpad), dtype=np.uint16)
    out[..., :C] = bits16(bf16_round(x)).reshape(B, C, H, W).transpose(0, 2, 3, 1)
    return out


# ======================================================================================================= stem
STEM_SHAPES = ((1, 1, 1), (1, 7, 7), (2, 13, 70), (1, 16, 64), (3, 33, 65), (1, 64, 96))
STEM_WRAP = (1030, 16, 64)          # 1030 tiles on 1024 workgroups: six workgroups walk a second tile; image b = pattern b mod 7
WRAP_PERIOD = 7


def out_hw(H, W):
    return (H - 1) // 2 + 1, (W - 1) // 2 + 1


def stem_tiles(B, H, W):
    OH, OW = out_hw(H, W)
    return B * ((OH + ST_TH - 1) // ST_TH) * ((OW + ST_TW - 1) // ST_TW)


def stem_terms(w):
    """the three bf16 terms of fp32 weights, as float32 arrays: t0 = bf16(w), t1 = bf16(w - t0), t2 = bf16(w - t0 - t1)"""
    w = np.asarray(w, dtype=F32)
    t0 = bf16_round(w)
    t1 = bf16_round(w - t0)
    t2 = bf16_round(w - t0 - t1)
    return t0, t1, t2


def stem_wt(w):
    """the matrix-core kernel's weights, restated: float32 [3][64][224] of bf16 values, k = ky*32 + kx*4 + ci"""
    wp = np.zeros((64, 7, 8, 4), dtype=F32)
    wp[:, :, :7, :3] = np.asarray(w, dtype=F32).transpose(3, 0, 1, 2)
    return np.stack(stem_terms(wp.reshape(64, 224)))


@functools.lru_cache(maxsize=None)
def stem_data(kind, B, H, W, period=None):
    """-> x float64 [B, H, W, 3] (bf16 values), w float32 [7, 7, 3, 64], shift float32 [64]; with `period`, image b is a copy of
    image b mod period (only `period` images are drawn)"""
    g = rng(1000 + 7 * H + W + {"exact": 0, "random": 1}[kind])
    nb = B if period is None else min(B, period)
    if kind == "exact":
        x = g.integers(-4, 5, (nb, H, W, 3)).astype(F64)
        m = 2 * g.integers(256, 512, (7, 7, 3, 64)) + 1                       # odd, 513 .. 1023
        w = (m * g.choice([-1, 1], m.shape) / 1024.0).astype(F32)
        shift = g.integers(40, 49, 64).astype(F32)
    else:
        x = bf(g.standard_normal((nb, H, W, 3)))
        w = (0.1 * g.standard_normal((7, 7, 3, 64))).astype(F32)
        shift = (0.1 * g.standard_normal(64)).astype(F32)
    if nb != B:
        x = x[np.arange(B) % period]
    for a in (x, w, shift):
        a.setflags(write=False)
    return x, w, shift


def _taps(x, H, W):
    """yields (ky, kx, window [B, OH, OW, 3]) over the zero-padded image; kx runs to 7 (the matrix-core kernel's padded tap)"""
    OH, OW = out_hw(H, W)
    xp = np.zeros((x.shape[0], H + 6 + 2, W + 6 + 2, x.shape[3]), dtype=x.dtype)
    xp[:, 3:3 + H, 3:3 + W] = x
    for ky in range(7):
        for kx in range(8):
            yield ky, kx, xp[:, ky:ky + 2 * OH:2, kx:kx + 2 * OW:2]


def stem_ref(x, w, shift, terms=False, period=None):
    """fp64: (pre-ReLU ref, mag).  mag = sum |w x| + |shift|, or with `terms` sum (|t0| + |t1| + |t2|) |x| + |shift|.  `period`: the
    caller states that image b equals image b mod period (asserted), and only `period` convolutions are computed"""
    B, H, W, _ = x.shape
    nb = B
    if period is not None and period < B:
        assert np.array_equal(x, x[np.arange(B) % period]), "the batch does not have the stated period"
        x, nb = x[:period], period
    w64 = np.asarray(w, dtype=F64)
    wa = sum(np.abs(t.astype(F64)) for t in stem_terms(w)) if terms else np.abs(w64)
    OH, OW = out_hw(H, W)
    ref, mag = np.zeros((nb, OH, OW, 64)), np.zeros((nb, OH, OW, 64))
    for ky, kx, win in _taps(x, H, W):
        if kx < 7:
            ref += win @ w64[ky, kx]
            mag += np.abs(win) @ wa[ky, kx]
    ref += np.asarray(shift, dtype=F64)
    mag += np.abs(np.asarray(shift, dtype=F64))
    if nb != B:
        idx = np.arange(B) % period
        ref, mag = ref[idx], mag[idx]
    return ref, mag


def relu(a):
    return np.where(a > 0, a, np.where(np.isnan(a), a, 0.0))


def stem_bound(ref, mag, K):
    return U_BF16 * np.abs(ref) + (K + 4) * 2.0 ** -23 * mag


K_DIRECT, K_MFMA = 147, 3 * 224


def stem_direct_emul(x, w, shift):
    """stem_conv_kernel in fp32: taps in the order ky, kx, ci, one product and one addition each"""
    B, H, W, _ = x.shape
    acc = np.zeros((B,) + out_hw(H, W) + (64,), dtype=F32)
    w = np.asarray(w, dtype=F32)
    for ky, kx, win in _taps(x.astype(F32), H, W):
        if kx < 7:
            for ci in range(3):
                acc = acc + win[..., ci:ci + 1] * w[ky, kx, ci]
    return bf16_round(relu(acc + np.asarray(shift, dtype=F32)))


def stem_mfma_emul(x, wt, shift, variant=None):
    """stem_conv_mfma_kernel from its own weight layout wt [3][64][224]: per k-step of 16 (ky, kx 4g .. 4g + 3, 4 channels) the
    three terms in turn, a k-step's 16 products summed in fp64 and added to the fp32 accumulator (the order inside one MFMA is
    the hardware's).  x [B, H, W, 3]; channel 3 of the NHWC(4) input is zero.
    variants: 'term2_dropped', 'term1_dropped', 'terms12_swapped_pitch' (term 2 read where term 1 lies), 'pw_off' (patch row
    pitch one pixel short: row ky is read ky pixels to the left)"""
    B, H, W, _ = x.shape
    x4 = np.concatenate([x, np.zeros(x.shape[:3] + (1,), dtype=x.dtype)], axis=3).astype(F32)
    wt = np.asarray(wt, dtype=F32).reshape(3, 64, 7, 8, 4)
    acc = np.zeros((B,) + out_hw(H, W) + (64,), dtype=F32)
    wins = {}
    OH, OW = out_hw(H, W)
    xp = np.zeros((B, H + 8, W + 8 + 8, 4), dtype=F32)
    xp[:, 3:3 + H, 3 + 8:3 + 8 + W] = x4
    for ky in range(7):
        for kx in range(8):
            off = kx + 8 - (ky if variant == "pw_off" else 0)
            wins[ky, kx] = xp[:, ky:ky + 2 * OH:2, off:off + 2 * OW:2]
    use = {None: (0, 1, 2), "term2_dropped": (0, 1), "term1_dropped": (0, 2), "terms12_swapped_pitch": (0, 2, 2), "pw_off": (0, 1, 2)}[variant]
    for ky in range(7):
        for g in range(2):
            for tm in use:
                s = np.zeros(acc.shape, dtype=F64)
                for kx in range(4 * g, 4 * g + 4):
                    s += wins[ky, kx].astype(F64) @ wt[tm, :, ky, kx, :].T.astype(F64)
                acc = (acc.astype(F64) + s).astype(F32)
    return bf16_round(relu(acc + np.asarray(shift, dtype=F32)))


# ---- term isolation
ISO_B, ISO_H, ISO_W = 12, 14, 14


def iso_q(ky, kx, ci, c):
    return (7 * (ky * 21 + kx * 3 + ci) + 3 * c) % 63 + 1


@functools.lru_cache(maxsize=None)
def iso_data():
    """-> x [12, 14, 14, 3], w [7, 7, 3, 64] fp32, shift, expected output (float64, exact), q table"""
    ky, kx, ci, c = np.meshgrid(np.arange(7), np.arange(7), np.arange(3), np.arange(64), indexing="ij")
    q = iso_q(ky, kx, ci, c)
    w = (1.0 + 2.0 ** -9 + q * 2.0 ** -23).astype(F32)
    assert np.array_equal(w.astype(F64), 1.0 + 2.0 ** -9 + q * 2.0 ** -23)
    shift = np.full(64, -(1.0 + 2.0 ** -9), dtype=F32)
    x = np.zeros((ISO_B, ISO_H, ISO_W, 3))
    want = np.zeros((ISO_B,) + out_hw(ISO_H, ISO_W) + (64,))
    for b in range(ISO_B):
        chan, py, px = b % 3, 6 + (b // 3) % 2, 7 - (b // 6) % 2           # both parities of the row and of the column
        x[b, py, px, chan] = 1.0
        for oy in range(want.shape[1]):
            for ox in range(want.shape[2]):
                ty, tx = py + 3 - 2 * oy, px + 3 - 2 * ox
                if 0 <= ty < 7 and 0 <= tx < 7:
                    want[b, oy, ox] = q[ty, tx, chan] * 2.0 ** -23
    return x, w, shift, want, q


# ---- non-finite inputs
NONFINITE_SHAPE = (3, 20, 40)


@functools.lru_cache(maxsize=None)
def nonfinite_data():
    """image 0: one NaN, one +inf and one -inf pixel far apart in a field of small integers; image 1: all NaN (the poisoned
    sample); image 2: finite.  Weights 1 + 2^-9 + 2^-18 (three positive terms), shifts 0: relu(+inf) = +inf, relu(-inf) = 0"""
    B, H, W = NONFINITE_SHAPE
    x = rng(77).integers(-2, 3, (B, H, W, 3)).astype(F64)
    x[0, 5, 6, 1], x[0, 10, 21, 0], x[0, 15, 34, 2] = np.nan, np.inf, -np.inf
    x[1] = np.nan
    w = np.full((7, 7, 3, 64), 1.0 + 2.0 ** -9 + 2.0 ** -18, dtype=F32)
    return x, w, np.zeros(64, dtype=F32)


def window_any(m):
    """pixel mask [B, H, W] -> [B, OH, OW]: the 7 x 7 window of the output holds a marked pixel"""
    B, H, W = m.shape
    out = np.zeros((B,) + out_hw(H, W), dtype=bool)
    for ky, kx, win in _taps(m[..., None], H, W):
        if kx < 7:
            out |= win[..., 0]
    return out


def stem_nonfinite_expect(x, w, shift, mfma):
    """bf16(relu(conv)) in fp64 with IEEE propagation (torch's contract); with `mfma` the padded tap kx = 7 enters with weight zero (0 * NaN and
    0 * inf are NaN).  Also returns the mask of torch's contract: the 7 x 7 window holds a NaN"""
    B, H, W, _ = x.shape
    out = np.zeros((B,) + out_hw(H, W) + (64,))
    nan7 = np.zeros(out.shape[:3], dtype=bool)
    w64 = np.asarray(w, dtype=F64)
    with np.errstate(invalid="ignore"):
        for ky, kx, win in _taps(x, H, W):
            if kx < 7:
                out += (win[..., None] * w64[ky, kx]).sum(axis=3)
                nan7 |= np.isnan(win).any(axis=3)
            elif mfma:
                out += (win * 0.0).sum(axis=3)[..., None]
        out = relu(out + np.asarray(shift, dtype=F64))
    return bf16_round(out).astype(F64), nan7


# ===================================================================================================== max-pool
POOL_SHAPES = ((1, 1, 1, 8), (2, 7, 9, 64), (1, 8, 32, 64), (3, 33, 17, 72))
BF16_LOWEST = -3.3895313892515355e38


@functools.lru_cache(maxsize=None)
def pool_data(shape, nan=False):
    B, H, W, C = shape
    g = rng(500 + H * W + C)
    x = bf(g.standard_normal(shape) * 2)
    pick = g.integers(0, 12, shape)
    x = np.where(pick == 0, 0.0, np.where(pick == 1, -0.0, np.where(pick == 2, BF16_LOWEST, np.where(pick == 3, -np.inf, x))))
    if H * W > 1:                       # a whole window of -inf, one of the lowest finite value next to -inf, one of -0 only
        x[0, :2, :2, 0], x[0, :2, :2, 1], x[0, :2, :2, 2] = -np.inf, BF16_LOWEST, -0.0
        x[0, 0, 0, 1] = -np.inf
    if nan:
        x[0, H // 2, W // 2, :] = np.nan
        x[-1, 0, 0, 3] = np.nan
    x.setflags(write=False)
    return x


def pool_ref(x):
    B, H, W, C = x.shape
    OH, OW = out_hw(H, W)
    xp = np.full((B, H + 2, W + 2, C), -np.inf)
    xp[:, 1:1 + H, 1:1 + W] = x
    out = np.full((B, OH, OW, C), -np.inf)
    for ky in range(3):
        for kx in range(3):
            out = np.maximum(out, xp[:, ky:ky + 2 * OH:2, kx:kx + 2 * OW:2])      # np.maximum propagates NaN
    return out


# ================================================================================================== wave sums
def warp_sum_f32(v):
    """common.h warp_sum on float32 [..., 64]: row_shr 1, 2, 4, 8 inside rows of 16 lanes (a lane without a source adds 0), then
    row_bcast:15 into rows 1 and 3 and row_bcast:31 into rows 2 and 3; the total is lane 63"""
    v = np.asarray(v, dtype=F32).copy()
    r = v.reshape(v.shape[:-1] + (4, 16))
    for s in (1, 2, 4, 8):
        sh = np.zeros_like(r)
        sh[..., s:] = r[..., :-s]
        r = (r + sh).astype(F32)
    r[..., 1, :] = r[..., 1, :] + r[..., 0, 15:16]
    r[..., 3, :] = r[..., 3, :] + r[..., 2, 15:16]
    r[..., 2, :] = r[..., 2, :] + r[..., 1, 15:16]
    r[..., 3, :] = r[..., 3, :] + r[..., 1, 15:16]
    return r[..., 3, 15]


def _lanes(p):
    """[rows, n] -> [rows, trips, 64, 8] (zeros where a lane has no column: adding a zero product changes nothing)"""
    rows, n = p.shape
    trips = -(-n // 512)
    q = np.zeros((rows, trips * 512), dtype=F32)
    q[:, :n] = p
    return q.reshape(rows, trips, 64, 8)


# ======================================================================================================= coef
COEF_SHAPES = ((1, 8), (3, 504), (4, 512), (5, 520), (72, 1032), (9, 3072))        # (J, N)
COEF_LAYERS = (1, 3, 32)


def coef_d(N):
    return -(-N // 512) + 13


@functools.lru_cache(maxsize=None)
def coef_data(J, N, L, kind):
    """-> w2 [L, J, N] (bf16 values), gamma, beta float32 [L, N], b2 [L, J] (bf16 values); layers differ"""
    g = rng(2000 + J * 31 + N + L + (0 if kind == "exact" else 1))
    if kind == "exact":
        w2 = g.integers(-1, 2, (L, J, N)).astype(F64)
        gamma, beta = g.integers(-4, 5, (L, N)).astype(F32), g.integers(-4, 5, (L, N)).astype(F32)
        b2 = g.integers(-4, 5, (L, J)).astype(F64)
    else:
        w2 = bf(g.standard_normal((L, J, N)) * 0.05)
        gamma, beta = (1 + 0.3 * g.standard_normal((L, N))).astype(F32), (0.2 * g.standard_normal((L, N))).astype(F32)
        b2 = bf(g.standard_normal((L, J)) * 0.1)
    return w2, gamma, beta, b2


def coef_ref(w2, gamma, beta, b2):
    """fp64 -> coef [L, 2, J], bound [L, 2, J]; b2 None: without the bias"""
    N = w2.shape[2]
    ga, be = gamma.astype(F64)[:, None, :], beta.astype(F64)[:, None, :]
    a, wb = (w2 * ga).sum(2), (w2 * be).sum(2)
    ma, mb = np.abs(w2 * ga).sum(2), np.abs(w2 * be).sum(2)
    d = coef_d(N)
    if b2 is not None:
        wb, mb = wb + b2, mb + np.abs(b2)
    return np.stack([a, wb], 1), np.stack([(d + 1) * U * ma, (d + 2) * U * mb], 1)


def coef_emul(w2, gamma, beta, b2, variant=None):
    """ffn_ln_coef_kernel in fp32, layer by layer.  variants: 'no_b2' (the bias forgotten), 'beta_is_gamma', 'last_trip_lost'"""
    L, J, N = w2.shape
    out = np.zeros((L, 2, J), dtype=F32)
    for l in range(L):
        w = w2[l].astype(F32)
        for which, vec in ((0, gamma[l]), (1, gamma[l] if variant == "beta_is_gamma" else beta[l])):
            p = _lanes(w * vec.astype(F32)[None, :])
            if variant == "last_trip_lost" and p.shape[1] > 1:
                p = p[:, :-1]
            e = p[..., 0]
            for i in range(1, 8):
                e = (e + p[..., i]).astype(F32)
            s = np.zeros(e.shape[:1] + e.shape[2:], dtype=F32)
            for t in range(e.shape[1]):
                s = (s + e[:, t]).astype(F32)
            out[l, which] = warp_sum_f32(s)
        if b2 is not None and variant != "no_b2":
            out[l, 1] = out[l, 1] + b2[l].astype(F32)
    return out


# =================================================================================================== rowstats
ROWSTATS_ROWS = (1, 3, 4, 5, 9)
ROWSTATS_J = (8, 504, 512, 520)
ROWSTATS_N = (8, 3072)


def rowstats_d(J):
    return 8 * (-(-J // 512)) + 6


def rowstats_extra(N):
    """inv_n = 1.f / N is exact only for a power of two"""
    return 0 if N & (N - 1) == 0 else 1


@functools.lru_cache(maxsize=None)
def rowstats_data(rows, J, kind):
    """-> dy, t [rows, J] (bf16 values), coef float32 [2, J].  kind 'cancel': t within a few bf16 ulps of wb"""
    g = rng(3000 + rows * 17 + J + {"exact": 0, "random": 1, "cancel": 2}[kind])
    if kind == "exact":
        dy, t = g.integers(-2, 3, (rows, J)).astype(F64), g.integers(-4, 5, (rows, J)).astype(F64)
        coef = g.integers(-4, 5, (2, J)).astype(F32)
    else:
        dy = bf(g.standard_normal((rows, J)))
        coef = np.stack([g.standard_normal(J) * 2, g.standard_normal(J) * 0.5 + 1]).astype(F32)
        t = bf(g.standard_normal((rows, J))) if kind == "random" else bf(coef[1].astype(F64)[None, :] * (1 + 2.0 ** -7 * g.integers(-2, 3, (rows, J))))
    return dy, t, coef


def rowstats_ref(dy, t, coef, N):
    J = dy.shape[1]
    a, wb = coef[0].astype(F64), coef[1].astype(F64)
    k = rowstats_d(J) + 2 + rowstats_extra(N)
    c1, c2 = (dy * a).sum(1) / N, (dy * (t - wb)).sum(1) / N
    b1 = k * U * np.abs(dy * a).sum(1) / N
    b2 = (U * (np.abs(dy) * np.abs(t - wb)).sum(1) + k * U * np.abs(dy * (t - wb)).sum(1)) / N
    return np.stack([c1, c2], 1), np.stack([b1, b2], 1)


def rowstats_emul(dy, t, coef, N, variant=None):
    """ffn_ln_rowstats_kernel in fp32.  variants: 'inv_from_J' (1 / N taken from J), 'wb_not_subtracted', 'a_for_wb'"""
    J = dy.shape[1]
    d32, t32 = dy.astype(F32), t.astype(F32)
    a, wb = coef[0][None, :], (coef[0] if variant == "a_for_wb" else coef[1])[None, :]
    sub = t32 if variant == "wb_not_subtracted" else (t32 - wb).astype(F32)
    out = []
    for p in (_lanes((d32 * a).astype(F32)), _lanes((d32 * sub).astype(F32))):
        s = np.zeros(p.shape[:1] + (64,), dtype=F32)
        for tr in range(p.shape[1]):
            for e in range(8):
                s = (s + p[:, tr, :, e]).astype(F32)
        out.append(warp_sum_f32(s))
    inv = F32(1) / F32(J if variant == "inv_from_J" else N)
    return np.stack([out[0] * inv, out[1] * inv], 1).astype(F32)


# ================================================================================================ param_grads
PG_J = (1, 7, 8, 9, 129, 136)
PG_N = (8, 120, 128, 136, 256, 264)
PG_SLABS = 8
GAIN_THRESHOLD = 0.05


def gain_is_small(gamma, beta):
    g, b = np.asarray(gamma, dtype=F32), np.asarray(beta, dtype=F32)
    return np.abs(g) < F32(GAIN_THRESHOLD) * np.maximum(F32(1), np.abs(b))


@functools.lru_cache(maxsize=None)
def pg_data(J, N, kind):
    """-> w2, dw2 [J, N], db2 [J] (bf16 values), gamma, beta float32 [N]; column 1 (and N - 2) has gamma == 0"""
    g = rng(4000 + J * 13 + N + (0 if kind == "exact" else 1))
    if kind == "exact":
        w2, dw2 = g.integers(-1, 2, (J, N)).astype(F64), g.integers(-1, 2, (J, N)).astype(F64)
        db2, beta = g.integers(-2, 3, J).astype(F64), g.integers(-2, 3, N).astype(F32)      # (sums stay below 2^8: bf16 holds them)
        gamma = (g.choice([-1.0, 1.0], N) * 2.0 ** g.integers(-2, 3, N)).astype(F32)
    else:
        w2, dw2 = bf(g.standard_normal((J, N)) * 0.05), bf(g.standard_normal((J, N)))
        db2, beta = bf(g.standard_normal(J)), (0.5 * g.standard_normal(N)).astype(F32)
        gamma = (1 + 0.3 * g.standard_normal(N)).astype(F32)
    gamma[1] = gamma[N - 2] = 0.0
    return w2, dw2, db2, gamma, beta


def pg_ref(w2, dw2, db2, gamma, beta, input_terms=False):
    """fp64 -> (dgamma, dbeta, bound_dgamma, bound_dbeta); gamma == 0 -> dgamma 0, bound 0 (the kernel writes +0)"""
    J = w2.shape[0]
    ga, be = gamma.astype(F64), beta.astype(F64)
    swd, sdb = (w2 * dw2).sum(0), (w2 * db2[:, None]).sum(0)
    mwd, mdb = np.abs(w2 * dw2).sum(0), np.abs(w2 * db2[:, None]).sum(0)
    E_wd, E_db = (J + 4) * U * mwd, (J + 4) * U * mdb
    nz = ga != 0
    gs = np.where(nz, ga, 1.0)
    dgamma = np.where(nz, (swd - be * sdb) / gs, 0.0)
    num = E_wd + np.abs(be) * E_db + 3 * U * (np.abs(swd) + np.abs(be * sdb))
    if input_terms:
        num = num + U_BF16 * (mwd + np.abs(be) * mdb)
    bg = np.where(nz, U_BF16 * np.abs(dgamma) + num / np.abs(gs), 0.0)
    return dgamma, sdb, bg, U_BF16 * np.abs(sdb) + E_db


def pg_emul(w2, dw2, db2, gamma, beta, variant=None):
    """the partial and final kernels in fp32 and in their order -> (dgamma, dbeta) as bf16 values.  variants: 'slab_off_by_one'
    (j0 one row late), 'beta_dbeta_kept' (not subtracted), 'no_division', 'ragged_block_lost' (the last partial 128-column block)"""
    J, N = w2.shape
    w, d, b = w2.astype(F32), dw2.astype(F32), db2.astype(F32)
    rows_per = -(-J // PG_SLABS)
    part = np.zeros((PG_SLABS, 2, N), dtype=F32)
    for sl in range(PG_SLABS):
        j0 = sl * rows_per + (1 if variant == "slab_off_by_one" else 0)
        j1 = min(J, sl * rows_per + rows_per)
        red = np.zeros((2, 16, N), dtype=F32)
        for ry in range(16):
            for j in range(j0 + ry, j1, 16):
                red[0, ry] = red[0, ry] + w[j] * d[j]
                red[1, ry] = red[1, ry] + w[j] * b[j]
        for r in range(16):
            part[sl] = part[sl] + red[:, r]
    if variant == "ragged_block_lost" and N % 128:
        part[:, :, N - N % 128:] = 0
    swd, sdb = np.zeros(N, dtype=F32), np.zeros(N, dtype=F32)
    for sl in range(PG_SLABS):
        swd, sdb = swd + part[sl, 0], sdb + part[sl, 1]
    num = swd if variant == "beta_dbeta_kept" else (swd - (beta * sdb).astype(F32)).astype(F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = num if variant == "no_division" else (num / gamma).astype(F32)
    return bf16_round(np.where(gamma != 0, q, F32(0))), bf16_round(sdb)


# ---- the division against the definition
SEM_M, SEM_J, SEM_N = 300, 64, 256


def gelu64(x):
    return 0.5 * x * (1.0 + np.vectorize(math.erf)(x / math.sqrt(2.0)))


@functools.lru_cache(maxsize=None)
def semantic_data():
    """a real LN(gelu(u)) W2^T + b2 and the fp64 gradients of its parameters.  Gains: 0, +-1e-4, +-0.04 (flagged), 0.0501 (just
    above the threshold), 0.08 with beta 4 and 0.3 with beta -3 (flagged through beta: below 0.05 |beta| resp. above), O(1)"""
    g = rng(5150)
    M, J, N = SEM_M, SEM_J, SEM_N
    u = bf(g.standard_normal((M, N)) * 1.5)
    w2 = bf(g.standard_normal((J, N)) * 0.06)
    dy = bf(g.standard_normal((M, J)))
    gamma = (1 + 0.3 * g.standard_normal(N)).astype(F32)
    beta = (0.3 * g.standard_normal(N)).astype(F32)
    special = [(0.0, 0.1), (1e-4, 0.2), (-1e-4, -0.1), (0.04, 0.3), (-0.04, 0.2), (0.0501, 0.5), (0.08, 4.0), (0.3, -3.0), (0.0501, -0.9)]
    for i, (gv, bv) in enumerate(special):
        for k in (3 + 11 * i, 130 + 11 * i):
            gamma[k], beta[k] = gv, bv
    a = gelu64(u)
    mean, var = a.mean(1, keepdims=True), a.var(1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + 1e-5)
    xhat = (a - mean) * rstd
    z = gamma.astype(F64) * xhat + beta.astype(F64)
    dw2, db2 = dy.T @ z, dy.sum(0)
    dz = dy @ w2
    return dict(u=u, w2=w2, dy=dy, gamma=gamma, beta=beta, dw2=bf(dw2), db2=bf(db2), dgamma=(dz * xhat).sum(0), dbeta=dz.sum(0),
                mean=mean[:, 0].astype(F32), rstd=rstd[:, 0].astype(F32), flagged=gain_is_small(gamma, beta))


SEM_FLAGGED = 2 * 6          # 0, +-1e-4, +-0.04 and 0.08 with beta 4, twice each


# ===================================================================================================== rescue
RESCUE_N = 520
RESCUE_FLAGGED = (0, 100, 101, 255, 256, RESCUE_N - 1)      # block edges, two neighbours, the ragged third block's last column
RESCUE_CASES = ((1, 8), (255, 8), (256, 1024), (257, 8), (600, 1024))      # (M, J)


def rescue_depth(M):
    return -(-M // 256) + 8


@functools.lru_cache(maxsize=None)
def rescue_data(M, J, flagged=RESCUE_FLAGGED):
    g = rng(6000 + M + J)
    N = RESCUE_N
    w2, dw2 = bf(g.standard_normal((J, N)) * 0.05), bf(g.standard_normal((J, N)))
    db2, dy, u = bf(g.standard_normal(J)), bf(g.standard_normal((M, J))), bf(g.standard_normal((M, N)) * 1.5)
    gamma = (g.choice([-1.0, 1.0], N) * (0.5 + g.random(N))).astype(F32)
    beta = (0.5 * g.standard_normal(N)).astype(F32)
    small = [(0.0, 0.3), (1e-3, -0.2), (-0.04, 0.9), (0.19, 4.0), (0.049, 0.0), (-0.0499, 1.0)]
    for k, (gv, bv) in zip(flagged, small):
        gamma[k], beta[k] = gv, bv
    a = gelu_f32(u).astype(F64)
    mean = a.mean(1).astype(F32)
    rstd = (1.0 / np.sqrt(a.var(1) + 1e-5)).astype(F32)
    return dict(w2=w2, dw2=dw2, db2=db2, dy=dy, u=u, gamma=gamma, beta=beta, mean=mean, rstd=rstd)


def rescue_ref(d, cols):
    """fp64 dgamma of the definition on `cols` and its bound; gelu is the fp32 restatement (erf_as), widened"""
    M, J = d["dy"].shape
    w = d["w2"][:, cols]
    dz = d["dy"] @ w
    mdz = np.abs(d["dy"]) @ np.abs(w)
    uv = d["u"][:, cols]
    rstd = d["rstd"].astype(F64)[:, None]
    xhat = (gelu_f32(uv).astype(F64) - d["mean"].astype(F64)[:, None]) * rstd
    ref = (dz * xhat).sum(0)
    per = (J + 2) * U * mdz * np.abs(xhat) + np.abs(dz) * (4 * U * np.abs(uv) + 8 * U) * rstd + 3 * U * np.abs(dz * xhat)
    return ref, U_BF16 * np.abs(ref) + per.sum(0) + rescue_depth(M) * U * np.abs(dz * xhat).sum(0)


def rescue_emul(d, cols, variant=None):
    """ffn_ln_dgamma_exact_kernel in fp32 on `cols` -> bf16 values.  variants: 'u_pitch_N' (u read with ldu = N although its rows
    are ldu apart: pass the wrongly strided u as d['u_wrong']), 'mean_dropped', 'rows_beyond_256_lost'"""
    M, J = d["dy"].shape
    dy, w = d["dy"].astype(F32), d["w2"][:, cols].astype(F32)
    dz = np.zeros((M, len(cols)), dtype=F32)
    for j in range(J):
        dz = dz + dy[:, j:j + 1] * w[j][None, :]
    uv = (d["u_wrong"] if variant == "u_pitch_N" else d["u"])[:, cols]
    gl = gelu_f32(uv)
    mean = 0 if variant == "mean_dropped" else d["mean"][:, None]
    term = (dz * (gl - mean).astype(F32)).astype(F32) * d["rstd"][:, None]
    Mu = min(M, 256) if variant == "rows_beyond_256_lost" else M
    red = np.zeros((256, len(cols)), dtype=F32)
    for m in range(Mu):
        red[m % 256] = red[m % 256] + term[m]
    o = 128
    while o:
        red[:o] = red[:o] + red[o:2 * o]
        o >>= 1
    return bf16_round(red[0])
