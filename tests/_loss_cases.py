"""Cases, data, fp64 references, derived bounds and fp32 restatements for the conformance suite of the training-loss and optimizer
kernels: csrc/loss.hip, csrc/dice.hip, csrc/distill.hip, csrc/ohem.hip (all on csrc/seg_tile.h) and csrc/optim.hip.
test_loss_conformance_cpu.py checks this module alone, test_loss_conformance_gpu.py the kernels against it.  numpy only: nothing
here touches the GPU, torch or the library, and nothing calls ifseg_amd.criterions.*_reference (the CPU file compares with them).

u = 2^-24 (fp32 unit roundoff; "1 ulp" of a device intrinsic is 2 u).  A bf16 store adds 2^-8 |ref| and scales the fp32 error in
front of it by 1 + 2^-8 (the post-processing suite established 2^-8).  TINY = 2^-126 stands for a flushed or denormal result.
Every bound below is a function of the fp64 reference's own magnitudes; nothing is measured or fitted.

The tile (seg_tile.h).  Pixel i of a tile reads four taps: v_c = ((wA xA + wB xB) + wC xC) + wD xD.  The weights are products of
two multiples of 1/32 (exact), the logits are bf16, so every product is exact in fp32; three additions round:
      vb_c = 3 u sum_taps |w x_c|,      Vb = max_c vb_c   (the running maximum m is one of the v_c).
The margin rule: the predicted class of a pixel is exact when the fp64 top-2 gap exceeds 2 Vb; tile_data() draws until every valid
pixel of a case has such a gap (the exact-tie case excepted, where all classes are equal in fp32 as well and `if (v > m)` keeps 0).

Online softmax in fp32 (loss.hip, pass B of dice.hip).  a'_c = v_c - m, a_c = v_c - lse.  __expf(x) = v_exp_f32(x log2 e): the
product rounds the exponent by u |x log2 e|, a relative u |x| of the result, the instruction is 1 ulp: (|x| + 2) u.  A term of the
denominator carries the error of its argument (vb_c + Vb + u |a'_c|), its own exponential and the chain of rescalings
exp(m_old - m_new) it went through, whose arguments add up to at most |a'_c|, one exponential and one product each (3 u per
update, K updates: K counts the classes within 2 Vb of the running maximum in fp64); n additions of positive terms cost n u:
      R_sum = sum_c p_c (vb_c + Vb + (3 |a'_c| + 2) u) + (n + 3 K) u          (p-weighted: the error of a sum of positive terms)
      d_lse = Vb + R_sum + 3 u log S + u |lse|          (__logf: v_log_f32 1 ulp and the product with ln 2; m + log S one rounding)
      E_c   = vb_c + d_lse + (2 |a_c| + 2) u            (relative error of p_c = __expf(v_c - lse); + TINY absolutely)
The issue's starting form u_exp(|v - lse|) p A is the last term of E_c alone; vb_c and d_lse enter the argument of the
exponential and are not smaller than it, hence the longer form.

Part A -- loss.hip, one form for both instantiations (cw = 1, q = 1, A = 1 unweighted):
      d_c = q (p_c A - [c = y] hot - unif cw_c),   hot = (1 - eps) cw_y,  unif = eps / n,  A = hot + unif sum cw
      dd_c = q (p_c A (E_c + 16 u) + 2 u (p_c A + [c = y] hot + unif cw_c)) + 2 u |d_c| + TINY
             (A: sum cw through a 6 + 3 step tree after <= 2 sequential terms, one product, one addition: under 16 u)
      tile_partial[k][c]: bound = sum_pix |wy wx| dd_c + 34 u sum_pix |wy wx d_c|     (16 products + additions over x, then over y)
      loss  l = q (hot (lse - v_y) + unif (scw lse - sum cw v)):
      dl = q (hot (d_lse + vb_y + 2 u |lse - v_y|) + unif (scw d_lse + 13 u scw |lse| + sum cw vb + (n + 2) u sum cw |v|))
           + 4 u q (hot |lse - v_y| + unif (scw |lse| + |sum cw v|))
      stats_part[0]: sum_pix dl + 9 u sum |l| (warp tree 6, four waves 3).  stats_part[1]: counts (and 255 per pixel) are integers
      below 2^24: exact; sum q cw_y: 10 u of itself.  Histograms: exact under the margin rule.
Part B -- dice.hip.  Pass A keeps the denominator and the tile sums in fp64 and uses the accurate expf (1 ulp): a probability is
      e_c = p_c (vb_c + Vb + u |a'_c| + 3 u + sum_k p_k (vb_k + Vb + u |a'_k| + 2 u)) off.  This e is DERIVED per pixel and class
      and replaces the measured e of the "4 e N_b" rule of test_dice_gpu.py (a measured constant is not acceptable here):
      sI = sum_{y = c} e + (T + 1) u I,  sP = sum 2 p e + (T + 1) u P   (one rounding per tile, T tiles added in fp32),  Y exact.
      Pass B consumes its own fp32 sums: N = 2 I + s, Q = P + Y + s, k = kscale w_c, a = -2 k / Q, e = k N / Q^2:
      dN = 2 sI + 2 u N,  dQ = sP + 2 u Q,  da = |a| (dQ / Q + 6 u),  de = |e| (dN / N + 2 dQ / Q + 8 u)
      S = a_y p_y + 2 sum_k p_k^2 e_k:  dS = |a_y| p_y (E_y + 2 u) + p_y da_y + 2 sum_k p_k^2 (|e_k| (2 E_k + 2 R_sum + (n + 8) u) + de_k)
      d_c = p_c (a_c [y = c] + 2 p_c e_c - S):
      dd_c = |d_c| (E_c + u) + p_c ([y = c] da_c + 2 p_c (|e_c| (E_c + 2 u) + de_c) + dS + 3 u (|a_c| [y = c] + 2 p_c |e_c| + |S|)) + TINY
      dice_out: sum_{b,c} k (1 - N / Q):  sum k ((N / Q) (dN / N + dQ / Q + 2 u) + 5 u) + (ceil(B n / 256) + 9) u sum |term|
Part C -- distill.hip.  s = v_s / T in fp32: ds_c = vb_c / T + u |s_c|; Sb = max ds.  Denominators, A and KL in fp64 with the
      accurate expf:  eps_c = ds_c + Sb + u |s_c - ms| + 2 u (and the teacher's likewise),  R = sum_c p_c eps_c
      dKL = sum_c q_c (ds_c + dt_c) + 2 sum_c q_c epst_c |t_c - s_c| + (Sb + Rs) + (Tb + Rt);  kd_part[0]: sum dKL + u |sum KL|
      d_c = p_c - q_c in fp32:  dd_c = p_c (eps_c + Rs + 3 u) + q_c (epst_c + Rt + 3 u) + u |d_c| + TINY;  the adjoint as in A.
      Equal student and teacher: every term is the same bit pattern on both sides, KL and d are exactly 0.
Part D -- the gather.  g = ce_sum (1 / Z) + dice_sum + kd_sum ((w T) (1 / N)), rounded to bf16 once.  Each sum takes <= 9
      partials (8 additions), then 1 / Z, two products and two additions: 11 operations.
      bound = 2^-8 |ref| + (1 + 2^-8) (sum_9 bounds(partials) scaled like the partials + 11 u (|ce| + |dice| + |kd|)),
      |ce| etc. the sums of the ABSOLUTE partials in final scale; Z sums T tile shares in fp32: |ce| (T + 1) u more when it is no integer.
      Synthetic partials (small integers, powers of two for Z, N, w, T) make every operation exact: bit equality.
Part E -- ohem.hip.  hardness p = exp(v_y - m) / sum in fp64 from the fp32 values, rounded once:
      bound = p (vb_y + Vb + u |a'_y| + u + sum_k p_k (vb_k + Vb + u |a'_k| + 2 u)) + TINY
      (the kernel's comment claims 4 e of a MEASURED e; this is the same quantity derived).  The select is integer: exact.
Part F -- optim.hip.  sumsq: a thread adds, per trip, four terms a a + b b (products exact: bf16 squares; one rounding for the
      pair, one for the accumulation): 8 roundings per trip; then the wave tree (6), four waves (3), 16 sequential parts per lane
      and the tree again (6):  bound = (8 trips + 31) u sum g^2.
      Adam against fairseq's arithmetic with Python-double scalars (beta, 1 - beta, bc1, bc2 formed in double):
      the kernel takes beta as fp32 and forms 1.f - beta in fp32: R1(beta) = u (beta / (1 - beta) + 1) relative on (1 - beta)
      (216 u at beta2 = 0.999: the LARGEST term of v after one step); coef = gscale min(1, max_norm / (sqrt(ss) gscale + 1e-6)): 6 u.
      dm' = 2 u beta1 |m| + |g'| (1 - beta1) (R1(beta1) + 10 u) + u |m'|
      dv' = 2 u beta2 v + g'^2 (1 - beta2) (R1(beta2) + 18 u) + u v' + TINY
      denom = sqrt(v') + eps:  dden = min(dv' / (2 sqrt v'), sqrt(dv')) + u sqrt(v') + u denom
      bc = 1 - powf(beta, step) by value: beta^step is off by (step + 3) u of itself (beta's rounding step times, powf 1 ulp, the
      store), the subtraction cancels: Rbc = (step + 3) u beta^step / bc + u; through `hyper` the caller rounds the double: Rbc = u.
      step_size = lr sqrt(bc2) / bc1:  Rss = Rbc2 / 2 + Rbc1 + 5 u.   At steps 1 .. 100 by value Rbc2 is about (1 + 3 / step) 1000 u:
      the cancellation dominates every other relative error of the update (tens of u).
      p' = (p - wd lr p) - ss m' / denom = pa - t:
      dp = 3 u wd lr |p| + u |pa| + |t| (Rss + 3 u) + ss dm' / denom + |t| dden / denom + u |p'|
      p16 == bf16(p32 of the kernel) exactly, and within 2^-8 |ref| + (1 + 2^-8) dp of fp64.
"""
import functools
import math

import numpy as np

from _rowops_cases import F32, U, U_BF16, bf16_round, worst_ratio  # noqa: F401

TINY = 2.0 ** -126
TS, CH, NS_MAX = 16, 16, 512
SEG0, PAD_ID, EOS_ID = 59, 1, 2
F64 = np.float64


def _ro(*arrs):
    for a in arrs:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)


# ================================================================================================ geometry, fp64
@functools.lru_cache(maxsize=None)
def interp_matrix(n):
    """dense fp64 matrix [16 n, n] of the x16 bilinear upsample of one axis (F.interpolate, align_corners=False)"""
    d = np.arange(TS * n)
    src = np.maximum((d + 0.5) / TS - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), n - 1)
    i1 = np.minimum(i0 + 1, n - 1)
    w1 = src - i0
    M = np.zeros((TS * n, n))
    np.add.at(M, (d, i0), 1.0 - w1)
    np.add.at(M, (d, i1), w1)
    _ro(M)
    return M


@functools.lru_cache(maxsize=None)
def local_weights(n):
    """[16 n, 3] fp64: the weight of pixel d on the cells c0 - 1, c0, c0 + 1 of its own tile's stencil (0 outside the grid)"""
    M = interp_matrix(n)
    w = np.zeros((TS * n, 3))
    for d in range(TS * n):
        for k in range(3):
            c = d // TS - 1 + k
            if 0 <= c < n:
                w[d, k] = M[d, c]
    _ro(w)
    return w


def upsample(L, hp, wp, absolute=False):
    """L [B, hp wp, n] -> [B, 16 hp, 16 wp, n] in fp64 (absolute: sum |w| |x|, the magnitude the value bound needs)"""
    B, P, n = L.shape
    G = np.asarray(L, dtype=F64).reshape(B, hp, wp, n)
    if absolute:
        G = np.abs(G)
    return np.einsum("yi,xj,bijc->byxc", interp_matrix(hp), interp_matrix(wp), G, optimize=True)


def adjoint(D, hp, wp, absolute=False):
    """D [B, H, W, n] -> tile partials [B, hp, wp, 9, n] in fp64: G[ky kx] = sum_pix wy[py][ky] wx[px][kx] D (absolute: of |D|)"""
    B, H, W, n = D.shape
    D6 = (np.abs(D) if absolute else D).reshape(B, hp, TS, wp, TS, n)
    wy = local_weights(hp).reshape(hp, TS, 3)
    wx = local_weights(wp).reshape(wp, TS, 3)
    return np.einsum("ypk,xql,bypxqc->byxklc", wy, wx, D6, optimize=True).reshape(B, hp, wp, 9, n)


def stencil_gather(tp, order="yx", clip=True):
    """tile partials [B, hp, wp, 9, n] -> per-cell sums [B, hp, wp, n]: cell (cy, cx) takes partial ky * 3 + kx of tile
    (cy - (ky - 1), cx - (kx - 1)) where that tile exists.  fp64 in, fp64 out; float32 in: float32, summed in the kernel's order.
    order / clip restate two wrong variants (k = kx * 3 + ky; a tile index outside the row wraps into the flat array)."""
    B, hp, wp, _, n = tp.shape
    out = np.zeros((B, hp, wp, n), dtype=tp.dtype)
    flat = tp.reshape(B * hp * wp, 9, n)
    for cy in range(hp):
        for cx in range(wp):
            for ky in range(3):
                ty = cy - (ky - 1)
                if ty < 0 or ty >= hp:
                    continue
                for kx in range(3):
                    tx = cx - (kx - 1)
                    if clip and (tx < 0 or tx >= wp):
                        continue
                    k = ky * 3 + kx if order == "yx" else kx * 3 + ky
                    if clip:
                        out[:, cy, cx] = out[:, cy, cx] + tp[:, ty, tx, k]
                    else:
                        idx = np.clip(np.arange(B) * hp * wp + ty * wp + tx, 0, B * hp * wp - 1)
                        out[:, cy, cx] = out[:, cy, cx] + flat[idx, k]
    return out


# ================================================================================================ cases and data
def _tc(id, B, hp, wp, nseg, regime="n2", ldx=0, targets="mixed", **kw):
    c = dict(id=id, B=B, hp=hp, wp=wp, nseg=nseg, regime=regime, ldx=ldx, targets=targets, eps=0.0, cw=None, plane=None,
             norm_pixels=0, weighted=False, smooth=1.0, dcw=False, T=1.0, mask_all=False, teacher="rand", why="")
    c.update(kw)
    c["weighted"] = c["weighted"] or c["cw"] is not None or c["plane"] is not None or bool(c["norm_pixels"])
    return c


# every row says which path it is there for; ldl = nseg rounded up to 8, plus ldx
TILE_CASES = [
    _tc("g1x1-n1", 1, 1, 1, 1, why="p = 1, loss 0, gradient 0; every tap clamped"),
    _tc("g1x1-n2-s30", 2, 1, 1, 2, "s30", why="smallest softmax, saturated", eps=0.1, T=0.5),
    _tc("g1x3-n15", 1, 1, 3, 15, why="y axis fully clamped; ragged chunk 15", eps=0.1, cw="rand0", smooth=1e-3, T=4.0, mask_all=True),
    _tc("g3x1-n16", 1, 3, 1, 16, why="x axis fully clamped; exactly one chunk", plane="levels", dcw=True),
    _tc("g2x2-n17-bad", 2, 2, 2, 17, targets="mixed+bad", why="all corners; ragged chunk 17; bad labels", eps=0.1, cw="rand0",
        plane="levels", ldx=8, T=4.0, teacher="strided"),
    _tc("g3x4-n150", 3, 3, 4, 150, ldx=8, why="interior cell; shipped recipe; third sample invalid; lbs, tbs padded", cw="rand0",
        plane="levels", norm_pixels=1, dcw=True, teacher="strided"),
    _tc("g3x4-n171-s30", 1, 3, 4, 171, "s30", why="shipped recipe, saturated, eps = 1", eps=1.0, smooth=1e-3),
    _tc("g2x2-n257", 1, 2, 2, 257, why="second class per thread; odd ls == nseg", eps=0.1, cw="rand0", T=0.5),
    _tc("g1x1-n512-const", 1, 1, 1, 512, "const", why="NS_MAX; every pixel rounds alike", cw="zero", weighted=True, dcw=True),
    _tc("g3x4-n512", 1, 3, 4, 512, why="NS_MAX on a full grid", eps=0.1, plane="levels", norm_pixels=1, mask_all=True),
    _tc("g2x2-n150-const", 2, 2, 2, 150, "const", why="constant field over several cells", eps=0.1),
    _tc("g2x2-n17-invalid", 2, 2, 2, 17, targets="invalid", why="no valid pixel in the batch: loss 0, gradient 0, no NaN", eps=0.1,
        cw="rand0", plane="levels"),
    _tc("g2x2-n16-ties", 1, 2, 2, 16, "ties", why="equal logits everywhere: pred is the lowest index", weighted=True),
    _tc("g3x4-n17-same", 1, 3, 4, 17, why="teacher identical to the student: KL exactly 0", teacher="same", T=4.0),
    _tc("g2x2-n17-flat", 1, 2, 2, 17, "flat", why="a saturated teacher against a flat student", teacher="saturated"),
]
CASE = {c["id"]: c for c in TILE_CASES}
COSTLY = ("g1x1-n2-s30", "g2x2-n17-bad", "g3x4-n150", "g2x2-n257", "g1x1-n512-const", "g2x2-n17-invalid", "g1x1-n1", "g3x4-n171-s30",
          "g1x3-n15", "g3x1-n16")
DICE_CASES = [CASE[k] for k in COSTLY]
KD_CASES = [CASE[k] for k in COSTLY + ("g3x4-n17-same", "g2x2-n17-flat")]
GATHER_CASES = [CASE[k] for k in ("g2x2-n17-bad", "g3x4-n150", "g1x1-n2-s30")]
STENCIL_GRIDS = [(1, 1, 1), (1, 3, 2), (3, 1, 1), (2, 2, 3), (3, 4, 2)]          # (hp, wp, B)


def ldl_of(c):
    return (c["nseg"] + 7) // 8 * 8 + c["ldx"]


def _targets(rng, B, hp, wp, nseg, kind):
    H, W = TS * hp, TS * wp
    tg = rng.integers(0, nseg, (B, H, W)) + SEG0
    flat = tg.reshape(-1)
    cover = rng.permutation(flat.size)[:min(nseg, flat.size // 2)]
    flat[cover] = SEG0 + np.arange(cover.size)                                  # every class (where the pixels suffice)
    r = rng.random((B, H, W))
    tg[r < 0.04] = SEG0 + nseg
    tg[(r >= 0.04) & (r < 0.06)] = PAD_ID
    tg[(r >= 0.06) & (r < 0.08)] = EOS_ID
    if kind == "mixed+bad":
        tg[(r >= 0.08) & (r < 0.09)] = SEG0 - 3
        tg[(r >= 0.09) & (r < 0.10)] = SEG0 + nseg + 5
        tg[0, 0, 0], tg[-1, -1, -1] = 0, SEG0 + nseg + 1
    if hp * wp > 1:
        tg[0, :TS, :TS] = np.where(r[0, :TS, :TS] < 0.5, SEG0 + nseg, PAD_ID)   # one tile without a valid pixel
    if nseg > 2 and B >= 2:
        tg[1][tg[1] == SEG0 + 1] = SEG0                                         # a class absent from a sample
    if B == 3 or kind == "invalid":
        inv = np.where(r < 0.4, SEG0 + nseg, np.where(r < 0.7, PAD_ID, EOS_ID))
        if kind == "invalid":
            tg = inv
        else:
            tg[2] = inv[2]
    return tg.reshape(B, H * W).astype(np.int64)


def _logits(rng, B, P, nseg, regime):
    if regime == "ties":
        return np.full((B, P, nseg), 1.5, dtype=F32)
    if regime == "const":
        return np.broadcast_to(bf16_round(rng.standard_normal(nseg) * 2.0), (B, P, nseg)).copy()
    return bf16_round(rng.standard_normal((B, P, nseg)) * {"s30": 30.0, "flat": 2.0 ** -5}.get(regime, 2.0))


def is_class(tg, nseg):
    return ~((tg == PAD_ID) | (tg == EOS_ID) | (tg == SEG0 + nseg)) & (tg >= SEG0) & (tg < SEG0 + nseg)


def margins(L, tg, hp, wp):
    """(fp64 top-2 gap, 2 Vb) per pixel [B, H W]; the gap of a single class is inf"""
    V = upsample(L, hp, wp)
    Vb = 3 * U * upsample(L, hp, wp, absolute=True).max(-1)
    if V.shape[-1] == 1:
        gap = np.full(V.shape[:3], np.inf)
    else:
        top = np.partition(V, -2, axis=-1)
        gap = top[..., -1] - top[..., -2]
    return gap.reshape(L.shape[0], -1), (2 * Vb).reshape(L.shape[0], -1)


@functools.lru_cache(maxsize=None)
def tile_data(cid):
    """-> dict(logits [B, P, n] (bf16 values in fp32), target int64 [B, H W], teacher [B, P, n]); drawn until the margin rule holds"""
    c = CASE[cid]
    B, hp, wp, nseg = c["B"], c["hp"], c["wp"], c["nseg"]
    seed = 1000 + 7919 * TILE_CASES.index(c)
    for attempt in range(64):
        rng = np.random.default_rng(seed + attempt)
        L = _logits(rng, B, hp * wp, nseg, c["regime"])
        tg = _targets(rng, B, hp, wp, nseg, c["targets"])
        if c["regime"] == "ties":
            break
        gap, need = margins(L, tg, hp, wp)
        if bool((gap > need)[is_class(tg, nseg)].all()):
            break
    else:
        raise AssertionError("no draw of %s satisfies the margin rule" % cid)
    if c["teacher"] == "same":
        Tt = L.copy()
    elif c["teacher"] == "saturated":
        Tt = bf16_round(rng.standard_normal(L.shape) * 30.0)
    else:
        Tt = bf16_round(L + rng.standard_normal(L.shape) * (8.0 if c["regime"] == "s30" else 1.0))
    _ro(L, tg, Tt)
    return dict(logits=L, target=tg, teacher=Tt)


def class_weights(c, dice=False):
    """fp32 [n] or None"""
    n = c["nseg"]
    kind = ("rand" if c["dcw"] else None) if dice else c["cw"]
    if kind is None:
        return None
    if kind == "zero":
        return np.zeros(n, dtype=F32)
    w = (np.random.default_rng(5 + n + (3 if dice else 0)).random(n) * 1.5 + 0.5).astype(F32)
    if kind == "rand0" and n > 1:
        w[n // 2] = 0.0
    return w


def pixel_plane(c):
    """uint8 [B, H W] with the levels 0, 1, 128, 255 (and others), or None"""
    if c["plane"] is None:
        return None
    rng = np.random.default_rng(77 + c["nseg"])
    shape = (c["B"], 256 * c["hp"] * c["wp"])
    lv = rng.choice(np.array([0, 1, 128, 255, 37, 200], dtype=np.uint8), size=shape)
    return lv.astype(np.uint8)


# ================================================================================================ fp64 softmax pieces
class Pix:
    """the per-pixel fp64 quantities every part shares, for logits L [B, P, n] on an hp x wp grid"""

    def __init__(self, L, hp, wp, scale=1.0):
        self.V = upsample(L, hp, wp) * scale
        raw = 3 * U * upsample(L, hp, wp, absolute=True)
        self.vb = raw * scale + (U * np.abs(self.V) if scale != 1.0 else 0.0)         # ds_c of part C when scaled by 1 / T
        self.Vb = self.vb.max(-1)
        V = self.V
        self.m = V.max(-1)
        ap = V - self.m[..., None]
        ex = np.exp(ap)
        S = ex.sum(-1)
        self.lse = self.m + np.log(S)
        self.a = V - self.lse[..., None]
        self.p = ex / S[..., None]
        self.ap = ap
        n = V.shape[-1]
        run = np.maximum.accumulate(V, axis=-1)
        prev = np.concatenate([np.full(V.shape[:-1] + (1,), -np.inf), run[..., :-1]], axis=-1)
        K = (V >= prev - 2 * self.Vb[..., None]).sum(-1)
        self.R_sum = (self.p * (self.vb + self.Vb[..., None] + (3 * np.abs(ap) + 2) * U)).sum(-1) + (n + 3 * K) * U
        self.d_lse = self.Vb + self.R_sum + 3 * U * np.log(S) + U * np.abs(self.lse)
        self.E = self.vb + self.d_lse[..., None] + (2 * np.abs(self.a) + 2) * U
        # the fp64-denominator kernels (dice pass A, hardness, distill): accurate expf, 1 ulp
        self.eps64 = self.vb + self.Vb[..., None] + U * np.abs(ap) + 2 * U
        self.R64 = (self.p * self.eps64).sum(-1)


@functools.lru_cache(maxsize=None)
def pix(cid):
    c = CASE[cid]
    return Pix(tile_data(cid)["logits"], c["hp"], c["wp"])


def _labels(c):
    tg = tile_data(c["id"])["target"].reshape(c["B"], TS * c["hp"], TS * c["wp"])
    valid = is_class(tg, c["nseg"])
    return tg, valid, np.where(valid, tg - SEG0, 0)


def bad_label(c):
    tg, valid, _ = _labels(c)
    return int((~valid & ~((tg == PAD_ID) | (tg == EOS_ID) | (tg == SEG0 + c["nseg"]))).any())


def _tiles(x, hp, wp):
    """[B, H, W, ...] -> [B, hp, wp, 256, ...] (pixel tid = py * 16 + px)"""
    B = x.shape[0]
    rest = x.shape[3:]
    y = x.reshape((B, hp, TS, wp, TS) + rest)
    return np.moveaxis(y, 3, 2).reshape((B, hp, wp, 256) + rest)


# ================================================================================================ part A: reference
def ce_options(c, weighted=None):
    w = c["weighted"] if weighted is None else weighted
    n = c["nseg"]
    cw = class_weights(c) if w else None
    plane = pixel_plane(c) if w else None
    return dict(cw=np.ones(n) if cw is None else cw.astype(F64), q=None if plane is None else plane.astype(F64),
                eps=float(F32(c["eps"])), norm_pixels=c["norm_pixels"] if w else 0, weighted=w, has_plane=plane is not None)


@functools.lru_cache(maxsize=None)
def ce_ref(cid, weighted=None):
    """fp64 reference and bounds of one CE tile launch -> dict: tp, tp_bound [B, hp, wp, 9, n]; sp0, sp0_bound, sp1, sp1_bound
    [B, hp, wp]; hist [B, hp, wp, 3, n] (intersect | pred | label); d [B, H, W, n] (per-pixel derivative); loss, Z scalars"""
    c = CASE[cid]
    B, hp, wp, n = c["B"], c["hp"], c["wp"], c["nseg"]
    o = ce_options(c, weighted)
    px = pix(cid)
    tg, valid, label = _labels(c)
    V, p, lse = px.V, px.p, px.lse
    cw, eps = o["cw"], o["eps"]
    q = np.ones(valid.shape) if o["q"] is None else o["q"].reshape(valid.shape)
    q = q * valid
    scw = cw.sum()
    cwy = cw[label]
    hot, unif = (1.0 - eps) * cwy, eps / n
    A = hot + unif * scw
    onehot = np.zeros(V.shape)
    np.put_along_axis(onehot, label[..., None], 1.0, axis=-1)
    vy = np.take_along_axis(V, label[..., None], -1)[..., 0]
    vall = (cw * V).sum(-1)
    l = q * (hot * (lse - vy) + unif * (scw * lse - vall))
    d = q[..., None] * (p * A[..., None] - onehot * hot[..., None] - unif * cw)
    if o["norm_pixels"]:
        cnt = valid * (255.0 if o["has_plane"] else 1.0)
    else:
        cnt = q * cwy if o["weighted"] else valid * 1.0
    # bounds
    E = px.E
    dd = q[..., None] * (p * A[..., None] * (E + 16 * U) + 2 * U * (p * A[..., None] + onehot * hot[..., None] + unif * cw)) \
        + 2 * U * np.abs(d) + TINY * valid[..., None]
    vby = np.take_along_axis(px.vb, label[..., None], -1)[..., 0]
    dl = q * (hot * (px.d_lse + vby + 2 * U * np.abs(lse - vy))
              + unif * (scw * px.d_lse + 13 * U * scw * np.abs(lse) + (cw * px.vb).sum(-1) + (n + 2) * U * (cw * np.abs(V)).sum(-1))) \
        + 4 * U * q * (hot * np.abs(lse - vy) + unif * (scw * np.abs(lse) + np.abs(vall)))
    tp = adjoint(d, hp, wp)
    tp_bound = adjoint(dd, hp, wp) + 34 * U * adjoint(d, hp, wp, absolute=True)
    sp0 = _tiles(l, hp, wp).sum(-1)
    sp0_bound = _tiles(dl, hp, wp).sum(-1) + 9 * U * _tiles(np.abs(l), hp, wp).sum(-1)
    sp1 = _tiles(cnt, hp, wp).sum(-1)
    exact1 = (not o["weighted"]) or bool(o["norm_pixels"])
    sp1_bound = np.zeros_like(sp1) if exact1 else 10 * U * sp1
    pred = V.argmax(-1)
    hist = np.zeros((B, hp, wp, 3, n))
    tv, tpred, tlab = _tiles(valid, hp, wp), _tiles(pred, hp, wp), _tiles(label, hp, wp)
    for b in range(B):
        for y in range(hp):
            for x in range(wp):
                v = tv[b, y, x]
                pr, lb = tpred[b, y, x][v], tlab[b, y, x][v]
                hist[b, y, x, 0] = np.bincount(lb[pr == lb], minlength=n)
                hist[b, y, x, 1] = np.bincount(pr, minlength=n)
                hist[b, y, x, 2] = np.bincount(lb, minlength=n)
    Z = sp1.sum()
    T = B * hp * wp
    out = dict(tp=tp, tp_bound=tp_bound, sp0=sp0, sp0_bound=sp0_bound, sp1=sp1, sp1_bound=sp1_bound, hist=hist, d=d, dd=dd,
               Z=Z, Z_rel=0.0 if exact1 else (T + 11) * U, loss=(sp0.sum() / Z if Z > 0 else 0.0),
               loss_bound=((sp0_bound.sum() + (T + 1) * U * np.abs(sp0).sum()) / Z + (T + 13) * U * abs(sp0.sum() / Z)) if Z > 0 else 0.0,
               valid=valid, label=label, pred=pred, exact1=exact1)
    _ro(*[v for v in out.values() if isinstance(v, np.ndarray)])
    return out


# ================================================================================================ fp32 restatements (the tile)
def f32(x):
    return np.asarray(x, dtype=F32)


def axis_taps(n, variant=0):
    """stage_weights + Taps for one axis, every operation in fp32 -> (w3 [16 n, 3], ia [16 n] index of the first tap's cell with
    -1 / n for the zero cells around the grid, wa, wb).  variant 1: the top clamp fmaxf(src, 0) dropped; 2: i1 without its clamp"""
    d = np.arange(TS * n)
    c0, t = d // TS, d % TS
    src = f32(f32(f32(c0 * TS + t) + F32(0.5)) * F32(1.0 / TS)) - F32(0.5)
    if variant != 1:
        src = np.maximum(src, F32(0))
    i0 = np.trunc(src).astype(np.int64)
    i1 = i0 + 1 if variant == 2 else np.minimum(i0 + 1, n - 1)
    l1 = f32(src - f32(i0))
    l0 = f32(F32(1) - l1)
    s0, s1 = i0 - (c0 - 1), i1 - (c0 - 1)
    w3 = np.zeros((TS * n, 3), dtype=F32)
    for k in range(3):
        w3[:, k] = f32(np.where(k == s0, l0, F32(0)) + np.where(k == s1, l1, F32(0)))
    kl = np.where(w3[:, 0] != 0, 0, 1)
    wa = np.where(kl == 1, w3[:, 1], w3[:, 0])
    wb = np.where(kl == 1, w3[:, 2], w3[:, 1])
    return w3, c0 - 1 + kl, f32(wa), f32(wb)


def emu_values(L, hp, wp, variant=0):
    """value(c) of every pixel in the kernel's order [B, H, W, n] fp32.  variant 4: class c >= 256 staged from c - 256"""
    B, P, n = L.shape
    G = f32(L).reshape(B, hp, wp, n)
    if variant == 4 and n > 256:
        G = G.copy()
        G[..., 256:] = G[..., :n - 256]
    Lp = np.zeros((B, hp + 2, wp + 2, n), dtype=F32)
    Lp[:, 1:-1, 1:-1] = G
    _, ya, wya, wyb = axis_taps(hp, variant)
    _, xa, wxa, wxb = axis_taps(wp, variant)
    ya, xa = ya + 1, xa + 1
    wA, wB = f32(wya[:, None] * wxa[None, :]), f32(wya[:, None] * wxb[None, :])
    wC, wD = f32(wyb[:, None] * wxa[None, :]), f32(wyb[:, None] * wxb[None, :])
    Y, X = ya[:, None], xa[None, :]
    v = f32(wA[None, :, :, None] * Lp[:, Y, X])
    v = f32(v + f32(wB[None, :, :, None] * Lp[:, Y, X + 1]))
    v = f32(v + f32(wC[None, :, :, None] * Lp[:, Y + 1, X]))
    v = f32(v + f32(wD[None, :, :, None] * Lp[:, Y + 1, X + 1]))
    return v


def emu_adjoint(D, hp, wp, variant=0):
    """adjoint_chunk in fp32, xx then yy ascending -> [B, hp, wp, 9, n].  variant 3: the last class of a ragged last chunk lost"""
    B, H, W, n = D.shape
    wy = axis_taps(hp, variant)[0].reshape(hp, TS, 3)
    wx = axis_taps(wp, variant)[0].reshape(wp, TS, 3)
    D6 = f32(D).reshape(B, hp, TS, wp, TS, n)
    E = np.zeros((B, hp, TS, wp, 3, n), dtype=F32)
    for xx in range(TS):
        E = f32(E + f32(wx[None, None, None, :, xx, :, None] * D6[:, :, :, :, xx, None, :]))
    G = np.zeros((B, hp, wp, 3, 3, n), dtype=F32)
    for yy in range(TS):
        G = f32(G + f32(wy[None, :, yy, None, :, None, None] * E[:, :, yy, :, None, :, :]))
    G = G.reshape(B, hp, wp, 9, n)
    if variant == 3 and n % CH:
        G[..., n - 1] = 0
    return G


def wave_sum(x):
    """common.h warp_sum on [..., 64] fp32: the value lane 63 ends with"""
    v = f32(x).copy()
    rows = v.reshape(v.shape[:-1] + (4, 16))
    for s in (1, 2, 4, 8):
        sh = np.zeros_like(rows)
        sh[..., s:] = rows[..., :-s]
        rows = f32(rows + sh)
    r = rows[..., 15]
    r1 = f32(r[..., 1] + r[..., 0])
    r3 = f32(r[..., 3] + r[..., 2])
    return f32(r3 + r1)


def tile_sum(x, hp, wp):
    """the tile's fp32 sum of a per-pixel quantity [B, H, W]: warp_sum per wave, then red[0] + red[1] + red[2] + red[3]"""
    w = wave_sum(_tiles(f32(x), hp, wp).reshape(x.shape[0], hp, wp, 4, 64))
    return f32(f32(f32(w[..., 0] + w[..., 1]) + w[..., 2]) + w[..., 3])


def _online_softmax32(v, extra=None):
    """the fp32 online softmax walk -> (m, sum, pred); extra(c, is_new_max, r_or_x) lets a caller carry a second accumulator"""
    m = np.full(v.shape[:-1], -np.inf, dtype=F32)
    s = np.zeros(v.shape[:-1], dtype=F32)
    pred = np.zeros(v.shape[:-1], dtype=np.int64)
    with np.errstate(under="ignore", invalid="ignore", over="ignore"):
        for c in range(v.shape[-1]):
            vc = v[..., c]
            up = vc > m
            r = np.exp(f32(np.where(up, m - vc, vc - m))).astype(F32)
            if extra is not None:
                extra(c, up, r)
            s = np.where(up, f32(f32(s * r) + F32(1)), f32(s + r))
            pred = np.where(up, c, pred)
            m = np.where(up, vc, m)
    return m, s, pred


def ce_emulate(cid, weighted=None, variant=0):
    """seg_loss_tile_kernel in fp32, in its order of operations -> dict(tp, sp0, sp1, hist).  Variants: 1, 2 (tap weights), 3
    (ragged chunk), 4 (staging), 7 (hot without (1 - eps)), 8 (unif * cw[c] dropped from the weighted gradient)"""
    c = CASE[cid]
    B, hp, wp, n = c["B"], c["hp"], c["wp"], c["nseg"]
    o = ce_options(c, weighted)
    tg, valid, label = _labels(c)
    v = emu_values(tile_data(cid)["logits"], hp, wp, variant)
    m, s, pred = _online_softmax32(v)
    lse = f32(m + f32(np.log(s)))
    vl = np.take_along_axis(v, label[..., None], -1)[..., 0]
    eps = F32(c["eps"])
    unif = f32(eps / F32(n))
    hot = f32(F32(1) - eps)
    cw = f32(o["cw"])
    if o["weighted"]:
        vall = np.zeros(vl.shape, dtype=F32)
        for k in range(n):
            vall = f32(vall + f32(cw[k] * v[..., k]))
        part = np.zeros(256, dtype=F32)
        for i in range(n):
            part[i % 256] = f32(part[i % 256] + cw[i])
        ws = wave_sum(part.reshape(4, 64))
        scw = f32(f32(ws[0] + ws[1]) + f32(ws[2] + ws[3]))
        cwy = np.where(valid, cw[label], F32(0))
        q = np.where(valid, F32(1) if o["q"] is None else f32(o["q"].reshape(valid.shape)), F32(0))
        hotw = f32(hot * cwy)
        soft = f32(hotw + f32(unif * scw))
        lpix = f32(q * f32(f32(hotw * f32(lse - vl)) + f32(unif * f32(f32(scw * lse) - vall))))
        cnt = np.where(~valid, F32(0), (F32(255) if o["has_plane"] else F32(1)) if o["norm_pixels"] else f32(q * cwy))
        hotg = hotw if variant != 7 else cwy
        with np.errstate(under="ignore"):
            pe = np.exp(f32(v - lse[..., None])).astype(F32)
        onehot = np.arange(n) == label[..., None]
        d = f32(f32(pe * soft[..., None]) - np.where(onehot, hotg[..., None], F32(0)))
        if variant != 8:
            d = f32(d - f32(unif * cw))
        d = f32(q[..., None] * d)
    else:
        vall = np.zeros(vl.shape, dtype=F32)
        for k in range(n):
            vall = f32(vall + v[..., k])
        lpix = np.where(valid, f32(lse - vl), F32(0))
        if eps != 0:
            lpix = np.where(valid, f32(f32(f32(F32(1) - eps) * f32(lse - vl)) + f32(eps * f32(lse - f32(vall / F32(n))))), F32(0))
        cnt = np.where(valid, F32(1), F32(0))
        with np.errstate(under="ignore"):
            pe = np.exp(f32(v - lse[..., None])).astype(F32)
        onehot = np.arange(n) == label[..., None]
        hotg = hot if variant != 7 else F32(1)
        d = f32(f32(pe - np.where(onehot, hotg, F32(0))) - unif)
    d = np.where(valid[..., None], d, F32(0))
    lpix = np.where(valid, lpix, F32(0))
    hist = np.zeros((B, hp, wp, 3, n))
    tv, tpred, tlab = _tiles(valid, hp, wp), _tiles(pred, hp, wp), _tiles(label, hp, wp)
    for idx in np.ndindex(B, hp, wp):
        vv = tv[idx]
        pr, lb = tpred[idx][vv], tlab[idx][vv]
        hist[idx][0] = np.bincount(lb[pr == lb], minlength=n)
        hist[idx][1] = np.bincount(pr, minlength=n)
        hist[idx][2] = np.bincount(lb, minlength=n)
    return dict(tp=emu_adjoint(d, hp, wp, variant), sp0=tile_sum(lpix, hp, wp), sp1=tile_sum(cnt, hp, wp), hist=hist)


# ================================================================================================ part B: Dice
DICE_WEIGHT = 0.5


@functools.lru_cache(maxsize=None)
def dice_ref(cid):
    """-> dict(sums [B, 3, n], sums_bound; tp, tp_bound [B, hp, wp, 9, n]; value, value_bound; g [B, H, W, n])"""
    c = CASE[cid]
    B, hp, wp, n = c["B"], c["hp"], c["wp"], c["nseg"]
    T = hp * wp
    px = pix(cid)
    tg, valid, label = _labels(c)
    p = px.p * valid[..., None]
    onehot = np.zeros(p.shape)
    np.put_along_axis(onehot, label[..., None], 1.0, axis=-1)
    onehot *= valid[..., None]
    e = p * (px.eps64 + U + px.R64[..., None])
    I, Pq, Y = (p * onehot).sum((1, 2)), (p * p).sum((1, 2)), onehot.sum((1, 2))
    sI = (e * onehot).sum((1, 2)) + (T + 1) * U * I
    sP = (2 * p * e).sum((1, 2)) + (T + 1) * U * Pq
    sums = np.stack([I, Pq, Y], 1)
    sums_bound = np.stack([sI, sP, np.zeros_like(Y)], 1)
    w = class_weights(c, dice=True)
    w = np.ones(n) if w is None else w.astype(F64)
    s = float(F32(c["smooth"]))
    k = float(F32(DICE_WEIGHT)) * w / (B * n)
    N, Q = 2 * I + s, Pq + Y + s
    a, ee = -2 * k / Q, k * N / (Q * Q)
    dN, dQ = 2 * sI + 2 * U * N, sP + 2 * U * Q
    da, de = np.abs(a) * (dQ / Q + 6 * U), np.abs(ee) * (dN / N + 2 * dQ / Q + 8 * U)
    ab, eb, dab, deb = (x[:, None, None, :] for x in (a, ee, da, de))
    S = (onehot * ab * p).sum(-1) + 2 * (p * p * eb).sum(-1)
    g = p * (ab * onehot + 2 * p * eb - S[..., None])
    E = px.E
    Ey = (E * onehot).sum(-1)
    dS = (np.abs(ab) * onehot * p).sum(-1) * (Ey + 2 * U) + (onehot * p * dab).sum(-1) \
        + 2 * (p * p * (np.abs(eb) * (2 * E + 2 * px.R_sum[..., None] + (n + 8) * U) + deb)).sum(-1)
    dg = np.abs(g) * (E + U) + p * (onehot * dab + 2 * p * (np.abs(eb) * (E + 2 * U) + deb) + dS[..., None]
                                    + 3 * U * (np.abs(ab) * onehot + 2 * p * np.abs(eb) + np.abs(S)[..., None])) \
        + TINY * valid[..., None]
    term = k * (1 - N / Q)
    value = term.sum()
    value_bound = (k * ((N / Q) * (dN / N + dQ / Q + 2 * U) + 5 * U)).sum() + (math.ceil(B * n / 256) + 9) * U * np.abs(term).sum()
    out = dict(sums=sums, sums_bound=sums_bound, tp=adjoint(g, hp, wp),
               tp_bound=adjoint(dg, hp, wp) + 34 * U * adjoint(g, hp, wp, absolute=True), value=value, value_bound=value_bound, g=g,
               cw=w, valid=valid)
    _ro(*[v for v in out.values() if isinstance(v, np.ndarray)])
    return out


def dice_sums_emulate(cid):
    """pass A and the reduction over a sample's tiles -> [B, 3, n] fp32 (fp64 where the kernel is)"""
    c = CASE[cid]
    B, hp, wp, n = c["B"], c["hp"], c["wp"], c["nseg"]
    tg, valid, label = _labels(c)
    v = emu_values(tile_data(cid)["logits"], hp, wp)
    m = v.max(-1)
    with np.errstate(under="ignore"):
        x = np.exp(f32(v - m[..., None])).astype(F32).astype(F64)
    p = f32(x * (1.0 / x.sum(-1))[..., None]).astype(F64) * valid[..., None]
    onehot = (np.arange(n) == label[..., None]) & valid[..., None]
    parts = [f32(_tiles(t, hp, wp).sum(3)) for t in (p * onehot, p * p, onehot * 1.0)]           # [B, hp, wp, n], one rounding
    out = np.zeros((B, 3, n), dtype=F32)
    for q, t in enumerate(parts):
        for tile in t.reshape(B, hp * wp, n).transpose(1, 0, 2):
            out[:, q] = f32(out[:, q] + tile)
    return out


def dice_tile_emulate(cid, sums=None, variant=0):
    """pass B in fp32 from `sums` (default: the emulated pass A) -> (tp [B, hp, wp, 9, n], value).  variant 10: e with Q, not Q^2"""
    c = CASE[cid]
    B, hp, wp, n = c["B"], c["hp"], c["wp"], c["nseg"]
    sums = f32(dice_sums_emulate(cid) if sums is None else sums)
    tg, valid, label = _labels(c)
    w = class_weights(c, dice=True)
    w = np.ones(n, dtype=F32) if w is None else w
    smooth = F32(c["smooth"])
    kscale = f32(F32(DICE_WEIGHT) / f32(F32(B) * F32(n)))
    N = f32(f32(F32(2) * sums[:, 0]) + smooth)
    Q = f32(f32(sums[:, 1] + sums[:, 2]) + smooth)
    k = f32(kscale * w)
    a = f32(f32(F32(-2) * k) / Q)
    e = f32(f32(k * N) / (Q if variant == 10 else f32(Q * Q)))
    term = f32(k * f32(F32(1) - f32(N / Q))).reshape(-1)
    part = np.zeros(256, dtype=F32)
    for i in range(B * n):
        part[i % 256] = f32(part[i % 256] + term[i])
    wdt = 128
    while wdt:
        part[:wdt] = f32(part[:wdt] + part[wdt:2 * wdt])
        wdt //= 2
    v = emu_values(tile_data(cid)["logits"], hp, wp)
    eb = e[:, None, None, :]
    tt = [np.zeros(v.shape[:-1], dtype=F32)]

    def carry(cidx, up, r):
        ec = eb[..., cidx]
        tt[0] = np.where(up, f32(f32(tt[0] * f32(r * r)) + ec), f32(tt[0] + f32(f32(r * r) * ec)))

    m, s, _ = _online_softmax32(v, carry)
    lse = f32(m + f32(np.log(s)))
    rs = f32(F32(1) / s)
    vl = np.take_along_axis(v, label[..., None], -1)[..., 0]
    ay = np.take_along_axis(np.broadcast_to(a[:, None, None, :], v.shape), label[..., None], -1)[..., 0]
    with np.errstate(under="ignore"):
        S = f32(f32(ay * np.exp(f32(vl - lse)).astype(F32)) + f32(f32(F32(2) * tt[0]) * f32(rs * rs)))
        p = np.exp(f32(v - lse[..., None])).astype(F32)
    onehot = np.arange(n) == label[..., None]
    d = f32(p * f32(f32(np.where(onehot, a[:, None, None, :], F32(0)) + f32(f32(F32(2) * p) * eb)) - S[..., None]))
    d = np.where(valid[..., None], d, F32(0))
    return emu_adjoint(d, hp, wp), part[0]


# ================================================================================================ part C: distillation
@functools.lru_cache(maxsize=None)
def kd_ref(cid):
    """-> dict(tp, tp_bound [B, hp, wp, 9, n] (unnormalised p - q); kl, kl_bound [B, hp, wp]; count [B, hp, wp]; g [B, H, W, n])"""
    c = CASE[cid]
    B, hp, wp, n = c["B"], c["hp"], c["wp"], c["nseg"]
    inv_t = float(F32(1.0) / F32(c["T"]))
    dat = tile_data(cid)
    ps, pt = Pix(dat["logits"], hp, wp, inv_t), Pix(dat["teacher"], hp, wp, inv_t)
    tg, valid, _ = _labels(c)
    M = np.ones_like(valid) if c["mask_all"] else valid
    p, q = ps.p, pt.p
    with np.errstate(divide="ignore", invalid="ignore"):
        kl = (q * (pt.a - ps.a)).sum(-1)
    kl = np.where(M, kl, 0.0)
    g = (p - q) * M[..., None]
    dkl = (q * (ps.vb + pt.vb)).sum(-1) + 2 * (q * pt.eps64 * np.abs(pt.V - ps.V)).sum(-1) + (ps.Vb + ps.R64) + (pt.Vb + pt.R64)
    dg = (p * (ps.eps64 + ps.R64[..., None] + 3 * U) + q * (pt.eps64 + pt.R64[..., None] + 3 * U) + U * np.abs(g) + TINY) * M[..., None]
    klt = _tiles(kl, hp, wp).sum(-1)
    out = dict(tp=adjoint(g, hp, wp), tp_bound=adjoint(dg, hp, wp) + 34 * U * adjoint(g, hp, wp, absolute=True), kl=klt,
               kl_bound=_tiles(dkl * M, hp, wp).sum(-1) + U * np.abs(klt), count=_tiles(M * 1.0, hp, wp).sum(-1), g=g, M=M)
    _ro(*[v for v in out.values() if isinstance(v, np.ndarray)])
    return out


def kd_emulate(cid):
    """seg_distill_tile_kernel, fp32 where it is fp32 -> (tp fp32, kl fp32 [B, hp, wp], count)"""
    c = CASE[cid]
    B, hp, wp, n = c["B"], c["hp"], c["wp"], c["nseg"]
    inv_t = f32(F32(1.0) / F32(c["T"]))
    dat = tile_data(cid)
    tg, valid, _ = _labels(c)
    M = np.ones_like(valid) if c["mask_all"] else valid
    s = f32(emu_values(dat["logits"], hp, wp) * inv_t)
    t = f32(emu_values(dat["teacher"], hp, wp) * inv_t)
    ms, mt = s.max(-1), t.max(-1)
    with np.errstate(under="ignore"):
        xs = np.exp(f32(s - ms[..., None])).astype(F32)
        xt = np.exp(f32(t - mt[..., None])).astype(F32)
    sum_s, sum_t = xs.astype(F64).sum(-1), xt.astype(F64).sum(-1)
    acc = (xt.astype(F64) * (t.astype(F64) - s.astype(F64))).sum(-1)
    kl = acc / sum_t - (mt.astype(F64) + np.log(sum_t)) + (ms.astype(F64) + np.log(sum_s))
    rs, rt = f32(1.0 / sum_s), f32(1.0 / sum_t)
    d = f32(f32(xs * rs[..., None]) - f32(xt * rt[..., None]))
    d = np.where(M[..., None], d, F32(0))
    return emu_adjoint(d, hp, wp), f32(_tiles(np.where(M, kl, 0.0), hp, wp).sum(-1)), _tiles(M * 1.0, hp, wp).sum(-1)


# ================================================================================================ part D: the gather
KD_W = 2.0          # the distillation weight of the gather cases


def gather_emulate(ce=None, stats=None, dice=None, kd=None, kd_stats=None, kd_w=0.0, kd_t=0.0, variant=0):
    """seg_loss_gather_kernel in fp32 from fp32 partials [B, hp, wp, 9, n] -> bf16 values [B, hp, wp, n].  variant 5: ky / kx
    swapped; 6: no clipping in x; 9: stats [B, 2], the normaliser taken per sample; 11: KD scaled by T^2"""
    kw = dict(order="xy" if variant == 5 else "yx", clip=variant != 6)
    g = None
    if ce is not None:
        z = f32(stats)[..., 1]
        rz = np.where(z > 0, f32(F32(1) / np.where(z > 0, z, F32(1))), F32(0))
        g = f32(stencil_gather(f32(ce), **kw) * (rz[:, None, None, None] if variant == 9 else rz))
    if dice is not None:
        gd = stencil_gather(f32(dice), **kw)
        g = gd if g is None else f32(g + gd)
    if kd is not None:
        nk = F32(kd_stats[1])
        rn = f32(F32(1) / nk) if nk > 0 else F32(0)
        scale = f32(F32(kd_w) * F32(kd_t))
        if variant == 11:
            scale = f32(scale * F32(kd_t))
        gk = f32(stencil_gather(f32(kd), **kw) * f32(scale * rn))
        g = gk if g is None else f32(g + gk)
    return bf16_round(g)


def gather_ref(cid, use_ce, use_dice, use_kd):
    """fp64 end-to-end gradient of CE + Dice + w KD w.r.t. the logits [B, hp, wp, n], its bound, and loss_out [total, ce, dice, kd]
    with bounds"""
    c = CASE[cid]
    B, hp, wp = c["B"], c["hp"], c["wp"]
    T = B * hp * wp
    ref = np.zeros((B, hp, wp, c["nseg"]))
    fb = np.zeros_like(ref)
    loss, lb = np.zeros(4), np.zeros(4)
    if use_ce:
        r = ce_ref(cid)
        if r["Z"] > 0:
            ref += stencil_gather(r["tp"]) / r["Z"]
            mag = stencil_gather(np.abs(r["tp"])) / r["Z"]
            fb += stencil_gather(r["tp_bound"]) / r["Z"] + (11 * U + r["Z_rel"]) * mag
        loss[1], lb[1] = r["loss"], r["loss_bound"]
    if use_dice:
        r = dice_ref(cid)
        ref += stencil_gather(r["tp"])
        fb += stencil_gather(r["tp_bound"]) + 11 * U * stencil_gather(np.abs(r["tp"]))
        loss[2], lb[2] = r["value"], r["value_bound"]
    if use_kd:
        r = kd_ref(cid)
        N = r["count"].sum()
        Tk = float(F32(c["T"]))
        if N > 0:
            sc = KD_W * Tk / N
            ref += sc * stencil_gather(r["tp"])
            fb += sc * (stencil_gather(r["tp_bound"]) + 11 * U * stencil_gather(np.abs(r["tp"])))
            loss[3] = KD_W * Tk * Tk * r["kl"].sum() / N
            lb[3] = KD_W * Tk * Tk / N * (r["kl_bound"].sum() + (T + 1) * U * np.abs(r["kl"]).sum()) + 6 * U * abs(loss[3])
    loss[0] = loss[1:].sum()
    lb[0] = lb[1:].sum() + 3 * U * np.abs(loss[1:]).sum()
    bound = U_BF16 * np.abs(ref) + (1 + U_BF16) * fb
    return ref, bound, loss, lb


def stencil_partials(B, hp, wp, n, salt):
    """small distinct integers [B, hp, wp, 9, n] fp32"""
    i = np.arange(B * hp * wp * 9 * n, dtype=np.int64)
    return f32(((i * 37 + salt * 101) % 251 - 125).reshape(B, hp, wp, 9, n))


# ================================================================================================ part E: OHEM
@functools.lru_cache(maxsize=None)
def hardness_ref(cid):
    """-> (plane [B, H W] fp64 with -1 on invalid pixels, bound)"""
    c = CASE[cid]
    px = pix(cid)
    tg, valid, label = _labels(c)
    pick = lambda x: np.take_along_axis(x, label[..., None], -1)[..., 0]
    p = np.minimum(pick(px.p), 1.0)
    bound = p * (pick(px.vb) + px.Vb + U * np.abs(pick(px.ap)) + U + px.R64) + TINY
    B = c["B"]
    return np.where(valid, p, -1.0).reshape(B, -1), np.where(valid, bound, 0.0).reshape(B, -1)


def hardness_emulate(cid):
    c = CASE[cid]
    tg, valid, label = _labels(c)
    v = emu_values(tile_data(cid)["logits"], c["hp"], c["wp"])
    m = v.max(-1)
    with np.errstate(under="ignore"):
        s = np.exp(f32(v - m[..., None])).astype(F32).astype(F64).sum(-1)
    vl = np.take_along_axis(v, label[..., None], -1)[..., 0]
    p = np.minimum(f32(np.exp((vl - m).astype(F64)) / s), F32(1))
    return np.where(valid, p, F32(-1)).reshape(c["B"], -1)


KEY_MAX = 0x3F800000
OHEM_BIG = 512 * 1024 + 65          # count.h MAX_BLOCKS * 1024 + 65: the grid-stride second trip (at most 8 M elements)


def ohem_expected(h, B, thresh, min_kept, weight=None):
    """the select by a numpy sort -> (plane uint8, info [nvalid, kept, tau, kth])"""
    bits = f32(h).reshape(-1).view(np.uint32).astype(np.int64)
    cand = bits <= KEY_MAX
    nv = int(cand.sum())
    kth = int(np.sort(bits[cand])[min(min_kept * B, nv - 1)]) if nv else 0
    tb = int(np.array([thresh + 0.0], dtype=F32).view(np.uint32)[0])
    tau = max(tb, kth)
    keep = cand & (bits < tau)
    full = np.full(bits.shape, 255, dtype=np.uint8) if weight is None else weight.reshape(-1)
    return np.where(keep, full, 0).astype(np.uint8).reshape(np.shape(h)), np.array([nv, int(keep.sum()), tau, kth], dtype=np.int64)


def _oc(id, B, N, kind, thresh, min_kept, weight=False):
    return dict(id=id, B=B, N=N, kind=kind, thresh=thresh, min_kept=min_kept, weight=weight)


OHEM_CASES = ([_oc("total%d" % t, 1, t, "rand", 0.7, max(t // 3, 1)) for t in (1, 63, 64, 65, 255, 257)] + [
    _oc("second-trip", 1, OHEM_BIG, "rand", 0.6, 1000),
    _oc("nvalid0", 2, 130, "none", 0.7, 10),
    _oc("all-equal", 2, 130, "equal", 0.2, 50),
    _oc("kth-many-ties", 2, 257, "ties", 0.1, 100),
    _oc("thresh-above-kth", 2, 257, "rand", 0.9, 20),
    _oc("thresh-below-kth", 2, 257, "rand", 0.05, 100),
    _oc("thresh-equal-kth", 2, 257, "ties", 0.5, 100),
    _oc("minkept-ge-nvalid", 3, 100, "rand", 0.3, 1000),
    _oc("digits-0-and-1016", 1, 300, "zeroone", 0.5, 100),
    _oc("non-candidates", 2, 257, "junk", 0.7, 40),
    _oc("weight-plane", 2, 257, "rand", 0.7, 40, weight=True),
])


@functools.lru_cache(maxsize=None)
def ohem_plane(cid):
    """-> (hardness fp32 [B, N], weight uint8 [B, N] or None)"""
    c = next(x for x in OHEM_CASES if x["id"] == cid)
    B, N = c["B"], c["N"]
    rng = np.random.default_rng(31 + B * N)
    h = rng.random((B, N)).astype(F32)
    kind = c["kind"]
    if kind != "junk" and N > 4:
        h[rng.random((B, N)) < 0.1] = -1.0                    # invalid pixels
    if kind == "none":
        h[:] = -1.0
    elif kind == "equal":
        h[h >= 0] = 0.375
    elif kind == "ties":
        h[(h >= 0) & (rng.random((B, N)) < 0.5)] = 0.5         # half the candidates share one value, the k-th falls among them
    elif kind == "zeroone":
        h[:] = np.where(rng.random((B, N)) < 0.5, 0.0, 1.0)
    elif kind == "junk":
        junk = np.array([-0.0, -1.0, np.nan, 1.0000001, 2.0, np.inf, -np.inf], dtype=F32)
        sel = rng.random((B, N)) < 0.4
        h[sel] = rng.choice(junk, size=int(sel.sum()))
    w = rng.integers(0, 256, (B, N)).astype(np.uint8) if c["weight"] else None
    _ro(h, w)
    return h, w


# ================================================================================================ part F: optimizer
SUMSQ_SIZES = (1, 7, 8, 9, 2047, 1024 * 256 * 8 + 13)
SUMSQ_CASES = [dict(id="n%d" % n, n=n, data="normal") for n in SUMSQ_SIZES] + [dict(id="spike-n2047", n=2047, data="spike"),
                                                                               dict(id="n0", n=0, data="normal")]


@functools.lru_cache(maxsize=None)
def sumsq_data(n, data):
    if data == "spike":
        g = np.full(n, 1e-4)
        g[n // 3] = 1e4
    else:
        g = np.random.default_rng(900 + n % 1000).standard_normal(n) * 0.01
    g = bf16_round(g)
    _ro(g)
    return g


def sumsq_ref(n, data):
    g = sumsq_data(n, data).astype(F64)
    s = float((g * g).sum())
    trips = max(1, -(-n // (1024 * 256 * 8)))
    return s, (8 * trips + 31) * U * s


def sumsq_emulate(n, data):
    """sumsq_bf16_kernel + finish_norm_kernel in fp32, in their order"""
    g = sumsq_data(n, data)
    stride = 1024 * 256 * 8
    trips = max(1, -(-n // stride))
    full = np.zeros(trips * stride, dtype=F32)
    full[:n] = g
    grp = full.reshape(trips, 1024, 256, 4, 2)
    acc = np.zeros((1024, 256), dtype=F32)
    for t in range(trips):
        for e in range(4):
            a, b = grp[t, :, :, e, 0], grp[t, :, :, e, 1]
            acc = f32(acc + f32(f32(a * a) + f32(b * b)))
    if n % 8:                       # the thread that owns the ragged group adds its elements one by one
        i = n - n % 8
        t, r = divmod(i, stride)
        blk, th = divmod(r // 8, 256)
        a = np.zeros((), dtype=F32)
        for tt in range(t):
            for e in range(4):
                x, y = grp[tt, blk, th, e, 0], grp[tt, blk, th, e, 1]
                a = f32(a + f32(f32(x * x) + f32(y * y)))
        for k in range(i, n):
            a = f32(a + f32(g[k] * g[k]))
        acc[blk, th] = a
    w = wave_sum(acc.reshape(1024, 4, 64))
    part = f32(f32(f32(w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3])
    lane = np.zeros(64, dtype=F32)
    for i in range(0, 1024, 64):
        lane = f32(lane + part[i:i + 64])
    return float(wave_sum(lane))


ADAM_SIZES = (1, 3, 4, 5, 1027, 512 * 256 * 4 + 7)
ADAM_STEPS = (1, 2, 10, 1000, 100000)
B1, B2, ADAM_EPS = 0.9, 0.999, 1e-8


def _ac(id, n, step, clip="off", hyper=False, wd=0.1, lr=1e-2, ema=False, data="wide"):
    return dict(id=id, n=n, step=step, clip=clip, hyper=hyper, wd=wd, lr=lr, ema=ema, data=data)


ADAM_CASES = ([_ac("n%d-step%d" % (n, s), n, s, clip=("off", "active", "zero")[i % 3], hyper=bool(i % 2), wd=(0.1, 0.0)[i % 2],
                   ema=(i % 4 == 3))
               for i, (n, s) in enumerate(zip(ADAM_SIZES, (1, 2, 10, 1000, 100000, 2)))]
              + [_ac("n1027-step%d-value" % s, 1027, s, clip="active") for s in ADAM_STEPS]
              + [_ac("n1027-step%d-hyper" % s, 1027, s, clip="active", hyper=True) for s in (1, 1000)]
              + [_ac("n1027-zero-over-eps", 1027, 1, data="zeros"), _ac("n1027-underflow", 1027, 10, data="tiny"),
                 _ac("n1027-inactive-ema", 1027, 10, clip="inactive", ema=True)])
GSCALE = 0.5


@functools.lru_cache(maxsize=None)
def adam_data(cid):
    c = next(x for x in ADAM_CASES if x["id"] == cid)
    n = c["n"]
    rng = np.random.default_rng(4000 + n + c["step"] % 97)
    p = f32(rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n))
    p[0] = F32(1e3)
    g = bf16_round(rng.standard_normal(n))
    m = f32(rng.standard_normal(n) * 0.1)
    v = f32(rng.random(n) * 0.01)
    if c["data"] == "zeros":
        g[: n // 2], v[: n // 2], m[: n // 4] = 0, 0, 0
    if c["data"] == "tiny":
        g = bf16_round(g * 1e-25)
        v[: n // 2] = 0
    # the norm the clip sees: active: coef < 1; inactive: a large max_norm; zero: max_norm = 0 (no clipping at all)
    sumsq = F32(1e4) if c["clip"] == "active" else F32(1e-4)
    max_norm = {"off": 0.0, "zero": 0.0, "active": 1.0, "inactive": 1.0}[c["clip"]]
    _ro(p, g, m, v)
    return dict(p=p, g=g, m=m, v=v, sumsq=sumsq, max_norm=max_norm, use_sumsq=c["clip"] != "off")


def adam_scalars(c):
    """(bc1, bc2) in Python double, as fairseq forms them; the fp32 `hyper` words a caller uploads"""
    bc1, bc2 = 1.0 - B1 ** c["step"], 1.0 - B2 ** c["step"]
    return bc1, bc2, f32([c["lr"], bc1, bc2, GSCALE])


def adam_ref(cid):
    """fp64 Adam with double scalars -> dict(p, m, v, and their bounds)"""
    c = next(x for x in ADAM_CASES if x["id"] == cid)
    d = adam_data(cid)
    p, g, m, v = (d[k].astype(F64) for k in "pgmv")
    lr, wd, eps = float(F32(c["lr"])), float(F32(c["wd"])), float(F32(ADAM_EPS))
    bc1, bc2, _ = adam_scalars(c)
    coef = GSCALE
    if d["max_norm"] > 0 and d["use_sumsq"]:
        coef *= min(1.0, d["max_norm"] / (math.sqrt(float(d["sumsq"])) * GSCALE + float(F32(1e-6))))
    gg = g * coef
    m2 = m * B1 + gg * (1 - B1)
    v2 = v * B2 + gg * gg * (1 - B2)
    den = np.sqrt(v2) + eps
    ss = lr * math.sqrt(bc2) / bc1
    pa = p - wd * lr * p
    t = ss * m2 / den
    p2 = pa - t
    R1 = lambda b: U * (b / (1 - b) + 1)
    if c["hyper"]:
        Rb1 = Rb2 = U
    else:
        Rb1 = (c["step"] + 3) * U * B1 ** c["step"] / bc1 + U
        Rb2 = (c["step"] + 3) * U * B2 ** c["step"] / bc2 + U
    Rss = Rb2 / 2 + Rb1 + 5 * U
    dm = 2 * U * B1 * np.abs(m) + np.abs(gg) * (1 - B1) * (R1(B1) + 10 * U) + U * np.abs(m2)
    dv = 2 * U * B2 * v + gg * gg * (1 - B2) * (R1(B2) + 18 * U) + U * v2 + TINY
    with np.errstate(divide="ignore", invalid="ignore"):
        dsq = np.minimum(np.where(v2 > 0, dv / (2 * np.sqrt(v2)), np.inf), np.sqrt(dv))
    dden = dsq + U * np.sqrt(v2) + U * den
    dp = 3 * U * wd * lr * np.abs(p) + U * np.abs(pa) + np.abs(t) * (Rss + 3 * U) + ss * dm / den + np.abs(t) * dden / den + U * np.abs(p2)
    return dict(p=p2, m=m2, v=v2, dp=dp, dm=dm, dv=dv, Rss=Rss, t=t)


def adam_emulate(cid, variant=0):
    """adam_kernel in fp32 (scalars by value: bc = 1 - powf(beta, step) in fp32; through hyper: the uploaded words).
    variant 12: v from the unclipped gradient; 13: weight decay after the step; 14: m corrected with bc2"""
    c = next(x for x in ADAM_CASES if x["id"] == cid)
    d = adam_data(cid)
    p, g, m, v = d["p"], d["g"], d["m"], d["v"]
    lr, wd, eps, b1, b2, gs = F32(c["lr"]), F32(c["wd"]), F32(ADAM_EPS), F32(B1), F32(B2), F32(GSCALE)
    if c["hyper"]:
        _, _, h = adam_scalars(c)
        lr, bc1, bc2, gs = h
    else:
        bc1 = f32(F32(1) - F32(float(b1) ** c["step"]))
        bc2 = f32(F32(1) - F32(float(b2) ** c["step"]))
    coef = gs
    if d["max_norm"] > 0 and d["use_sumsq"]:
        norm = f32(np.sqrt(d["sumsq"]) * gs)
        coef = f32(coef * min(F32(1), f32(F32(d["max_norm"]) / f32(norm + F32(1e-6)))))
    ss = f32(f32(lr * np.sqrt(f32(bc2))) / (bc2 if variant == 14 else bc1))
    gg = f32(g * coef)
    gv = f32(g * gs) if variant == 12 else gg
    with np.errstate(under="ignore"):
        m2 = f32(f32(m * b1) + f32(gg * f32(F32(1) - b1)))
        v2 = f32(f32(v * b2) + f32(f32(gv * gv) * f32(F32(1) - b2)))
        den = f32(np.sqrt(v2) + eps)
        if variant == 13:
            p2 = f32(p - f32(f32(ss * m2) / den))
            p2 = f32(p2 - f32(f32(wd * lr) * p2))
        else:
            pa = f32(p - f32(f32(wd * lr) * p))
            p2 = f32(pa - f32(f32(ss * m2) / den))
    return dict(p=p2, m=m2, v=v2)


# ================================================================================================ end to end, restated
def _seq_tiles(x):
    """a per-tile quantity [B, hp, wp] summed over the tiles in fp32, one after the other (ifseg_reduce_parts)"""
    acc = F32(0)
    for t in f32(x).reshape(-1):
        acc = f32(acc + t)
    return acc


def end_to_end_emulate(cid, use_ce=True, use_dice=False, use_kd=False, variant=0):
    """the tile kernels, the reductions and the gather, all restated in fp32 -> (dlogits values [B, hp, wp, n], loss_out [4]).
    `variant` reaches the restatement it belongs to (see the wrong-variant table of the CPU file)"""
    c = CASE[cid]
    B = c["B"]
    kw, loss = {}, np.zeros(4)
    if use_ce:
        e = ce_emulate(cid, variant=variant)
        s0, s1 = _seq_tiles(e["sp0"]), _seq_tiles(e["sp1"])
        kw.update(ce=e["tp"], stats=f32([s0, s1]))
        if variant == 9:
            kw["stats"] = f32([[_seq_tiles(e["sp0"][b]), _seq_tiles(e["sp1"][b])] for b in range(B)])
        loss[1] = f32(s0 / s1) if s1 > 0 else 0.0
    if use_dice:
        tp, val = dice_tile_emulate(cid, variant=variant)
        kw.update(dice=tp)
        loss[2] = val
    if use_kd:
        tp, kl, cnt = kd_emulate(cid)
        ks = f32([_seq_tiles(kl), _seq_tiles(cnt)])
        kw.update(kd=tp, kd_stats=ks, kd_w=KD_W, kd_t=c["T"])
        if ks[1] > 0:
            loss[3] = f32(f32(F32(KD_W) * F32(c["T"]) * F32(c["T"])) * f32(ks[0] * f32(F32(1) / ks[1])))
    loss[0] = loss[1:].sum()
    return gather_emulate(variant=variant, **kw), loss
