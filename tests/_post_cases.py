"""Cases, data, fp64 references, derived bounds and CPU restatements for the conformance suite of the post-processing kernels:
csrc/crf.hip, csrc/resize.hip and csrc/evalops.hip (test_post_conformance_cpu.py checks this module alone,
test_post_conformance_gpu.py the kernels against it).  numpy only: nothing here touches the GPU or the library (the one
exception, `seg_eval_case`, borrows the margin rule of _predict_cases.py and imports it when it is called).

u = 2^-24 (fp32 unit roundoff; "1 ulp" of a device intrinsic is 2 u).  A bf16 output adds 2^-8 |ref| for its single rounding: bfloat16 has 8
significant bits, so half a unit in the last place of a value just above a power of two is 2^-8 of it (2^-9 |ref| is what a
correctly rounded value just below a power of two is off by at most; the fp32 emulation of the CPU file leaves it at 2^-8
values); the fp32 error in front of the rounding grows by 1 + 2^-8.  Nothing below is measured.

Part A -- crf.hip
  bilateral   out[c][i] = sum_j k(i, j) qn[c][j],  k = 2^-d2 gx[|dx|] gy[|dy|],  d2 = |f_i - f_j|^2 from the fp32 features.
              S = sum_j k |qn|.   bound = S (2^-8 + (8 + 4 max_j d2) u) + (N + 16) u S
              d2: three differences (u each), three squares and two additions: 4 u d2 absolutely, which v_exp_f32 turns into a
              relative 4 u d2 ln 2 of k; v_exp_f32 itself 1 ulp, two products one rounding each: 8 u covers them; the K tile is
              rounded to bf16 once (2^-8).  qn is bf16 and the products bf16 x bf16 are exact in fp32; N additions in any order
              (the MFMA's own order included) cost (N - 1) u S.  The colours of the data stay within d2 <= 90: no k is subnormal.
  spatial     integer qn (|q| <= 8), g = 2^-d: every product and every partial sum is a multiple of 2^-10 below 2^11: exact.
  update      v_c = log(clip(p_c, 1e-5f, 1)) + wp np mpos_c + wb nb mbi_c,  Q = softmax_c v.   V = max_c (|log| + |pos| + |bi|).
              bound(Q) = (16 + C + 16 V) u Q.   The form (16 + 4 max|v|) u Q needs two more terms, hence this one:
              * the unary is negative and the messages positive, so v_c can cancel: the roundings scale with V, not |v_c|;
                v_log_f32 1 ulp and the product with ln 2: 2 u |log|; each message two products and one addition: 4 u V for v_c;
                a_c = v_c - m: u |a| <= 2 u V; __expf = v_exp_f32(a log2 e): the product costs u |a| <= 2 u V relatively, the
                instruction 1 ulp: e_c is off by (8 V + 2) u relatively (the error of m is common to all c and cancels);
                the ratio e_c / sum e doubles that: 16 u V + 4 u;
              * the sum of C positive terms: (C - 1) u -- 16 does not cover C = 40; 1 / s and the product: 3 u more.
              qpos = Q np: one more rounding (u);  qbi = bf16(Q nb): 2^-8 |ref| + (1 + 2^-8) (bound + u |ref|).
  norm        rsqrtf(k1 + 1e-20f): the addition u (halved by the root), v_rsq_f32 1 ulp = 2 u:  4 u relative.
  rgb_dense_crf   end to end against oracle/crf_ref.py at the tolerances of test_dense_crf_meanfield_vs_exact_oracle
              (max |dQ| <= 3e-2, argmax agreement >= 0.99), the argmax compared on the pixels whose oracle top-2 gap is >= 6e-2
              = 2 x 3e-2 (a smaller gap can flip inside the value tolerance); the seeds of CRF_CASES keep those pixels below MARGIN_CAP = 1 %.

Part B -- resize.hip.  taps1d restated in fp64: src = max(0, (d + 0.5) sn / dn - 0.5), i0 = min(floor src, sn - 1), i1 = min(i0 + 1,
  sn - 1), w1 = src - i0.  In fp32 the quotient, the product and the subtraction are one rounding each of a value <= src + 1/2:
  |d src| <= 3 u src + u <= 4 u max(1, src); w1 = src - i0 is exact.  A weight that is off ABSOLUTELY by that much moves the result
  by that much times the difference of two table entries, which may not be among the four exact taps when the floor flips (the
  result is continuous there, the neighbour one further enters with weight <= d src): with A = max |table entry| of the column
  (rows) or head (bias) the weight term is   2 A 4 u (max(1, src_y) + max(1, src_x)) <= 16 u max(1, src_y, src_x) A.
  (The form 8 u max(1, src_y, src_x) sum |w v| underestimates it where a large entry carries an exact weight of 0.)
  The weights' products, the product with the value and the four additions:  8 u sum |w v|.
  rows    bound = 2^-8 |ref| + (1 + 2^-8) (16 u max(1, src_y, src_x) A + 8 u sum_taps |w v|)
  bias    the same on the key side (values: table entries), then on the query side (values: the inner sums, |inner| <= A):
          bound = 16 u (mk + mq) A + 16 u sum_q sum_k |wq wk B0|,   m = max(1, src_y, src_x) of the key / query position.
  Grids whose weights are dyadic (x1, x2, x1/2) with integer tables are bit-exact; x1 is bit-exact with any table (w1 = 0).

Part C -- evalops.hip
  l2norm    bound = 2^-8 |ref| + (D + 16) u |ref|:  D squares summed in any order (D u on the sum, halved by the root), sqrtf,
            1 / max(.), the product: under 16 u.
  top-k     exact: stable descending order, NaN first (torch.topk), lower index first on ties.
  softmax   (16 + 2 n) u relative holds for |x / T - max| <= 5, which the data guarantees (|x| <= 1.25, T in {1, 1/2, 2}: x / T and
            the difference from the maximum are exact): e_c off by (|a| + 2) u <= 7 u, the ratio doubles it, the sum (n - 1) u,
            1 / s and the product 2 u:  (15 + n) u.
  gather_mean   integers: the sum is exact, s / k one correctly rounded division.
  seg_eval  histograms exact on the pixels the margin rule of _predict_cases.Reference calls decided; the undecided ones (at most
            MARGIN_CAP of a case) get the ignore label, so that the three histograms of the kernel are exact as a whole.
            loss per pixel: (n + 32) u (1 + |loss|) for the online softmax (n exponentials and additions, __logf, m + log s - v_t)
            + 2 (16 max(1, src_y, src_x) + 8) u A for the interpolated values themselves (the Part B terms with |w v| <= A, on
            the maximum and on v_t; A = max |score|).  A block's partial sum adds 16 u sum |loss| (butterfly of 6 + 2 additions).
"""
import functools

import numpy as np

from _rowops_cases import F32, U, bf16_round, fraction_outside, is_bf16, is_f32, worst_ratio  # noqa: F401

U_BF16 = 2.0 ** -8        # unit roundoff of bf16 (8 significant bits)
SENTINEL = -12352.0
MARGIN_CAP = 0.01


def _ro(*arrs):
    for a in arrs:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)


def _seq(v, axis=-1):
    """strictly sequential fp32 sums along an axis"""
    v = np.asarray(v, dtype=F32)
    return np.take(np.cumsum(v, axis=axis, dtype=F32), -1, axis=axis)


# =================================================================================================== part A: bilateral
BI_SHAPES = {1: (1, 1), 63: (7, 9), 64: (4, 16), 65: (5, 13), 135: (9, 15), 273: (13, 21)}      # N -> (H, W), H != W
BI_SX, BI_SY = 3.0, 6.0                                                                       # gx != gy


def _bi(Cp, N, extra_ld=0, signed=False):
    H, W = BI_SHAPES[N]
    return dict(Cp=Cp, C=Cp - 3, N=N, H=H, W=W, ldq=(N + 63) // 64 * 64 + extra_ld, signed=signed, reach="crf_bilateral_kernel<%d>" % (Cp // 32),
                id="Cp%d-N%d%s%s" % (Cp, N, "-ld+64" if extra_ld else "", "-signed" if signed else ""))


BILATERAL_CASES = ([_bi(Cp, 135) for Cp in (32, 64, 96, 128, 160, 192)] + [_bi(Cp, N) for Cp in (32, 64) for N in (1, 63, 64, 65, 273)]
                   + [_bi(64, 65, extra_ld=64), _bi(64, 135, signed=True)])
BILATERAL_INSTANTIATIONS = ["crf_bilateral_kernel<%d>" % k for k in range(1, 7)]


@functools.lru_cache(maxsize=None)
def bilateral_geometry(N):
    """feat [N, 4] fp32 (colours pre-scaled as crf.py does, x | y << 16 in the bits of .w), gx [W], gy [H] fp32"""
    H, W = BI_SHAPES[N]
    rng = np.random.default_rng(100 + N)
    base = 100.0 + rng.integers(0, 14, size=(4, 3))
    ys, xs = np.divmod(np.arange(N), W)
    region = (ys * 2 // max(H, 1)) * 2 + (xs * 2 // max(W, 1))
    img = base[region] + np.clip(np.round(rng.standard_normal((N, 3)) * 1.5), -3, 3)
    feat = np.zeros((N, 4), dtype=F32)
    feat[:, :3] = (img * np.sqrt(np.log2(np.e) / (2.0 * 3.0 ** 2))).astype(F32)
    feat[:, 3] = (xs | (ys << 16)).astype(np.int32).view(F32)
    gx = np.exp(-np.arange(W) ** 2 / (2.0 * BI_SX ** 2)).astype(F32)
    gy = np.exp(-np.arange(H) ** 2 / (2.0 * BI_SY ** 2)).astype(F32)
    _ro(feat, gx, gy)
    return feat, gx, gy, xs, ys


@functools.lru_cache(maxsize=None)
def bilateral_qn(Cp, N, signed):
    """qn [Cp, N] bf16 values: class c scaled by 2^(c mod 5), rows >= C = Cp - 3 zero"""
    rng = np.random.default_rng(200 + Cp + N)
    q = rng.standard_normal((Cp, N)) if signed else rng.uniform(0.05, 1.0, (Cp, N))
    q = bf16_round(q * (2.0 ** (np.arange(Cp) % 5))[:, None])
    q[Cp - 3:] = 0
    _ro(q)
    return q


def _bilateral_k64(N):
    feat, gx, gy, xs, ys = bilateral_geometry(N)
    f = feat[:, :3].astype(np.float64)
    d2 = ((f[:, None, :] - f[None, :, :]) ** 2).sum(-1)
    k = 2.0 ** (-d2) * gx.astype(np.float64)[np.abs(xs[:, None] - xs[None, :])] * gy.astype(np.float64)[np.abs(ys[:, None] - ys[None, :])]
    return k, d2


@functools.lru_cache(maxsize=None)
def bilateral_ref(Cp, N, signed):
    """(out [Cp, N] fp64, bound [Cp, N])"""
    k, d2 = _bilateral_k64(N)
    q = bilateral_qn(Cp, N, signed).astype(np.float64)
    out, S = q @ k.T, np.abs(q) @ k.T
    bound = S * (U_BF16 + (8 + 4 * d2.max(1))[None, :] * U) + (N + 16) * U * S
    _ro(out, bound)
    return out, bound


def bilateral_emul(Cp, N, signed, wrong=None):
    """crf_bilateral_kernel in numpy fp32: K rounded to bf16, sums over j sequential.  wrong: "tile" (the last ragged j tile
    left out), "swap" (gx and gy exchanged), "rows" (class rows 0..31 and 32..63 exchanged)"""
    feat, gx, gy, xs, ys = bilateral_geometry(N)
    if wrong == "swap":
        gx = np.exp(-np.arange(gx.size) ** 2 / (2.0 * BI_SY ** 2)).astype(F32)
        gy = np.exp(-np.arange(gy.size) ** 2 / (2.0 * BI_SX ** 2)).astype(F32)
    d = feat[:, None, :3] - feat[None, :, :3]
    d2 = (d[..., 0] * d[..., 0] + (d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])).astype(F32)
    k = bf16_round(np.exp2(-d2).astype(F32) * gx[np.abs(xs[:, None] - xs[None, :])] * gy[np.abs(ys[:, None] - ys[None, :])])
    if wrong == "tile" and N % 64:
        k[:, N // 64 * 64:] = 0
    q = bilateral_qn(Cp, N, signed)
    out = np.stack([_seq(k * q[c][None, :]) for c in range(Cp)])
    if wrong == "rows" and Cp >= 64:
        out[:64] = np.concatenate([out[32:64], out[:32]])
    return out


# ===================================================================================================== part A: spatial
SPATIAL_CASES = [dict(R=R, H=H, W=W, C=C, id="R%d-%dx%d-C%d" % (R, H, W, C)) for R in (0, 1, 5) for (H, W) in ((1, 1), (3, 4), (12, 7)) for C in (1, 5)]


@functools.lru_cache(maxsize=None)
def spatial_case(R, H, W, C):
    rng = np.random.default_rng(300 + R + 7 * H + C)
    q = rng.integers(-8, 9, size=(C, H, W)).astype(F32)
    g = (2.0 ** -np.arange(R + 1)).astype(F32)
    ref, q64 = np.zeros((C, H, W)), q.astype(np.float64)
    for dy in range(-min(R, H - 1), min(R, H - 1) + 1):
        for dx in range(-min(R, W - 1), min(R, W - 1) + 1):
            ya, yb, xa, xb = max(0, -dy), min(H, H - dy), max(0, -dx), min(W, W - dx)      # out[y, x] += g g q[y + dy, x + dx]
            ref[:, ya:yb, xa:xb] += float(g[abs(dy)]) * float(g[abs(dx)]) * q64[:, ya + dy:yb + dy, xa + dx:xb + dx]
    _ro(q, g, ref)
    return dict(q=q.reshape(C, H * W), g=g, ref=ref.reshape(C, H * W))


# ====================================================================================================== part A: update
WPOS, WBI = 3.0, 4.0
CLIP_LO = F32(1e-5)
UPDATE_CASES = [dict(C=C, N=N, msg=msg, norm=norm, extra_ld=64 * ((C + N + msg) % 2), id="C%d-N%d-%s-%s" % (C, N, "msg" if msg else "init", "norm" if norm else "nonorm"))
                for C in (1, 5, 40) for N in (1, 255, 257) for msg in (False, True) for norm in (False, True)]
PROB_SPECIALS = (0.0, 1e-6, 1e-5, 1.0, 1.5)


@functools.lru_cache(maxsize=None)
def update_inputs(C, N):
    rng = np.random.default_rng(400 + C + N)
    prob = np.ascontiguousarray(rng.dirichlet(np.ones(max(C, 2)) * 0.5, size=N).T[:C], dtype=F32)
    sp = np.array(PROB_SPECIALS, dtype=F32)
    flat = prob.reshape(-1)
    flat[:min(flat.size, sp.size)] = sp[:flat.size]
    mpos, mbi = rng.uniform(0, 1.5, (C, N)).astype(F32), rng.uniform(0, 2.5, (C, N)).astype(F32)
    npos, nbi = rng.uniform(0.3, 1.0, N).astype(F32), rng.uniform(0.1, 0.8, N).astype(F32)
    _ro(prob, mpos, mbi, npos, nbi)
    return prob, mpos, mbi, npos, nbi


def update_ref(case):
    """fp64 reference and bounds: Q, qpos [C, N] (fp32 outputs), qbi [C, N] (bf16 output)"""
    C, N = case["C"], case["N"]
    prob, mpos, mbi, npos, nbi = (a.astype(np.float64) for a in update_inputs(C, N))
    np_, nb_ = (npos, nbi) if case["norm"] else (np.ones(N), np.ones(N))
    lg = np.log(np.clip(prob, float(CLIP_LO), 1.0))
    pos = WPOS * np_ * mpos if case["msg"] else np.zeros_like(lg)
    bi = WBI * nb_ * mbi if case["msg"] else np.zeros_like(lg)
    v = lg + pos + bi
    V = (np.abs(lg) + np.abs(pos) + np.abs(bi)).max(0)
    e = np.exp(v - v.max(0))
    Q = e / e.sum(0)
    Qb = (16 + C + 16 * V)[None, :] * U * Q
    qpos, qbi = Q * np_, Q * nb_
    return dict(Q=Q, Q_b=Qb, qpos=qpos, qpos_b=Qb * np_ + U * qpos, qbi=qbi, qbi_b=U_BF16 * qbi + (1 + U_BF16) * (Qb * nb_ + U * qbi))


def update_emul(case):
    """crf_update_kernel in numpy fp32, sequential sum over the classes: (Q, qpos, qbi as bf16 values)"""
    C, N = case["C"], case["N"]
    prob, mpos, mbi, npos, nbi = update_inputs(C, N)
    np_, nb_ = (npos, nbi) if case["norm"] else (np.ones(N, dtype=F32), np.ones(N, dtype=F32))
    v = np.log(np.minimum(np.maximum(prob, CLIP_LO), F32(1))).astype(F32)
    if case["msg"]:
        v = (v + F32(WPOS) * np_ * mpos).astype(F32)
        v = (v + F32(WBI) * nb_ * mbi).astype(F32)
    e = np.exp(v - v.max(0)).astype(F32)
    inv = F32(1) / _seq(e, axis=0)
    Q = (e * inv).astype(F32)
    return Q, (Q * np_).astype(F32), bf16_round(Q * nb_)


@functools.lru_cache(maxsize=None)
def norm_case():
    rng = np.random.default_rng(450)
    k1 = (10.0 ** rng.uniform(-12, 3, 257)).astype(F32)
    k1[[0, 100, 256]] = 0.0
    k1[1] = F32(1e-30)
    ref = (k1.astype(np.float64) + float(F32(1e-20))) ** -0.5
    _ro(k1, ref)
    return k1, ref, 4 * U * ref


def norm_emul(k1):
    return (F32(1) / np.sqrt((k1 + F32(1e-20)).astype(F32))).astype(F32)


# ================================================================================================ part A: end to end
CRF_CASES = [dict(h=13, w=21, c=40, iters=10, seed=1, id="13x21-c40-10it"), dict(h=13, w=21, c=150, iters=2, seed=1, id="13x21-c150-2it")]
CRF_GAP, CRF_TOL, CRF_AGREE = 6e-2, 3e-2, 0.99


@functools.lru_cache(maxsize=None)
def crf_inputs(h, w, c, seed):
    """(image uint8 [h, w, 3]: four flat regions + noise; probs fp32 [c, h, w]: a softmax with one favoured class per region)"""
    rng = np.random.default_rng(9000 + seed + c)
    base = rng.integers(0, 256, size=(4, 3)).astype(np.float64)
    region = (np.arange(h)[:, None] * 2 // h) * 2 + (np.arange(w)[None, :] * 2 // w)
    image = np.clip(np.round(base[region] + rng.standard_normal((h, w, 3)) * 2.0), 0, 255).astype(np.uint8)
    z = rng.standard_normal((c, h, w)) * 1.5
    fav = rng.permutation(c)[:4][region]
    np.put_along_axis(z, fav[None], np.take_along_axis(z, fav[None], 0) + 5.0, 0)
    z -= z.max(0)
    p = np.exp(z)
    probs = (p / p.sum(0)).astype(F32)
    _ro(image, probs)
    return image, probs


# ============================================================================================================ part B
def taps1d(dn, sn):
    """-> (i0, i1 int [dn], w1 fp64 [dn], src fp64 [dn])"""
    src = np.maximum(0.0, (np.arange(dn) + 0.5) * (sn / dn) - 0.5)
    i0 = np.minimum(np.floor(src).astype(np.int64), sn - 1)
    return i0, np.minimum(i0 + 1, sn - 1), src - i0, src


def taps1d_f32(dn, sn, fma):
    """the kernel's expression in fp32; fma: the product and the subtraction contracted into one rounding"""
    scale = F32(sn) / F32(dn)
    d = (np.arange(dn, dtype=F32) + F32(0.5))
    src = (d.astype(np.float64) * float(scale) - 0.5).astype(F32) if fma else ((d * scale).astype(F32) - F32(0.5)).astype(F32)
    src = np.where(src < 0, F32(0), src).astype(F32)
    i0 = np.minimum(src.astype(np.int64), sn - 1)
    return i0, np.minimum(i0 + 1, sn - 1), (src - i0.astype(F32)).astype(F32)


def interp_matrix(dn, sn):
    """dense [dn, sn] fp64"""
    i0, i1, w1, _ = taps1d(dn, sn)
    M = np.zeros((dn, sn))
    np.add.at(M, (np.arange(dn), i0), 1.0 - w1)
    np.add.at(M, (np.arange(dn), i1), w1)
    return M


def interp2d(h, w, oh, ow):
    """[h*w, oh*ow] fp64 and max(1, src_y, src_x) per destination position"""
    M = np.kron(interp_matrix(h, oh), interp_matrix(w, ow))
    m = np.maximum(1.0, np.maximum(taps1d(h, oh)[3][:, None], taps1d(w, ow)[3][None, :])).reshape(-1)
    return M, m


def taps2d_f32(h, w, oh, ow, fma):
    """per destination position: y [P, 2], x [P, 2] int, wy [P, 2], wx [P, 2] fp32 (taps2d of resize.hip)"""
    y0, y1, a = taps1d_f32(h, oh, fma)
    x0, x1, b = taps1d_f32(w, ow, fma)
    py, px = np.divmod(np.arange(h * w), w)
    return (np.stack([y0[py], y1[py]], 1), np.stack([x0[px], x1[px]], 1),
            np.stack([F32(1) - a[py], a[py]], 1).astype(F32), np.stack([F32(1) - b[px], b[px]], 1).astype(F32))


GRIDS = (((8, 8), (8, 8)), ((8, 8), (16, 16)), ((8, 8), (4, 4)), ((8, 8), (13, 5)), ((8, 8), (5, 11)), ((1, 1), (3, 2)), ((8, 8), (1, 7)), ((6, 10), (9, 4)))
DYADIC = (((8, 8), (8, 8)), ((8, 8), (16, 16)), ((8, 8), (4, 4)))
INTERP_PAIRS = sorted({(s, d) for (src, dst) in GRIDS for s, d in zip(src, dst)} | {(65, 2), (4, 46), (8, 12), (8, 6)})


def _rows(src, dst, C, ld_extra=0, ints=False):
    return dict(oh=src[0], ow=src[1], h=dst[0], w=dst[1], C=C, ld_src=C + ld_extra, stride=src[1] + 3, off=1, ints=ints,
                exact=ints or src == dst, id="%dx%d-%dx%d-C%d%s%s" % (src + dst + (C, "-ld+%d" % ld_extra if ld_extra else "", "-int" if ints else "")))


ROWS_CASES = ([_rows(s, d, 264) for s, d in GRIDS] + [_rows(s, d, 264, ints=True) for s, d in DYADIC[1:]]
              + [_rows((8, 8), (13, 5), 8), _rows((8, 8), (13, 5), 768), _rows((6, 10), (9, 4), 8, ld_extra=8), _rows((8, 8), (5, 11), 768, ld_extra=24),
                 _rows((8, 8), (8, 8), 8, ld_extra=8), _rows((1, 1), (3, 2), 768)])


@functools.lru_cache(maxsize=None)
def rows_table(oh, ow, C, stride, off, ints):
    """the bf16 table [(oh - 1) stride + ow + off + 2, C]: the grid rows y stride + x + off; every other row holds values too"""
    rng = np.random.default_rng(500 + oh + ow + C)
    n = (oh - 1) * stride + ow + off + 2
    t = rng.integers(-8, 9, size=(n, C)).astype(F32) if ints else bf16_round(rng.standard_normal((n, C)) * (2.0 ** (np.arange(C) % 4))[None, :])
    _ro(t)
    return t


def rows_grid(case, use_off=True):
    t = rows_table(case["oh"], case["ow"], case["C"], case["stride"], case["off"], case["ints"])
    ys, xs = np.divmod(np.arange(case["oh"] * case["ow"]), case["ow"])
    return t[ys * case["stride"] + xs + (case["off"] if use_off else 0)]


def rows_ref(case):
    g = rows_grid(case).astype(np.float64)
    M, m = interp2d(case["h"], case["w"], case["oh"], case["ow"])
    ref, mag = M @ g, np.abs(M) @ np.abs(g)
    A = np.abs(g).max(0)
    return ref, U_BF16 * np.abs(ref) + (1 + U_BF16) * (16 * U * m[:, None] * A[None, :] + 8 * U * mag)


def rows_emul(case, fma=False, use_off=True):
    """resize_rows_kernel in fp32 (tap order of the kernel), rounded to bf16"""
    g = rows_grid(case, use_off).astype(F32)
    y, x, wy, wx = taps2d_f32(case["h"], case["w"], case["oh"], case["ow"], fma)
    v = np.zeros((case["h"] * case["w"], case["C"]), dtype=F32)
    for t in range(4):
        v = (v + ((wy[:, t >> 1] * wx[:, t & 1]).astype(F32)[:, None] * g[y[:, t >> 1] * case["ow"] + x[:, t & 1]]).astype(F32)).astype(F32)
    return bf16_round(v)


def _bias(src, dst, H, Lt, tails=True, causal=False, pad=False, ints=False):
    return dict(oh=src[0], ow=src[1], h=dst[0], w=dst[1], H=H, Lt=Lt, tails=tails and Lt > 0, causal=causal, pad=pad, ints=ints,
                exact=ints or src == dst, id="%dx%d-%dx%d-H%d-Lt%d%s%s%s%s" % (src + dst + (H, Lt, "-tails" if tails and Lt > 0 else "", "-causal" if causal else "",
                                                                                 "-ld4" if pad else "", "-int" if ints else "")))


BIAS_CASES = [_bias((8, 8), (8, 8), 3, 5, pad=True), _bias((8, 8), (8, 8), 1, 1, causal=True), _bias((8, 8), (16, 16), 1, 1, ints=True, causal=True),
              _bias((8, 8), (4, 4), 3, 5, ints=True, pad=True), _bias((8, 8), (4, 4), 1, 0, ints=True),
              _bias((8, 8), (13, 5), 3, 5, pad=True), _bias((8, 8), (13, 5), 1, 1, causal=True), _bias((8, 8), (13, 5), 1, 5, tails=False, causal=True, pad=True),
              _bias((8, 8), (5, 11), 3, 1, causal=True, pad=True), _bias((8, 8), (5, 11), 1, 0, pad=True), _bias((8, 8), (5, 11), 3, 5, causal=True),
              _bias((1, 1), (3, 2), 3, 1, causal=True, pad=True), _bias((1, 1), (3, 2), 1, 5), _bias((8, 8), (1, 7), 3, 0), _bias((8, 8), (1, 7), 1, 1, tails=False, pad=True),
              _bias((6, 10), (9, 4), 3, 5, pad=True), _bias((6, 10), (9, 4), 1, 1, causal=True),
              _bias((65, 65), (2, 2), 1, 1, pad=True),            # delta table 129 x 129 x 4 = 66 564 bytes: the dynamic-LDS opt-in
              _bias((4, 4), (46, 46), 1, 0)]                      # T = 2116 > 8 x 256: the second trip of the j loop
BIAS_LOOP_EDGE = 2048


@functools.lru_cache(maxsize=None)
def bias_tables(oh, ow, H, Lt, ints):
    rng = np.random.default_rng(600 + oh + 3 * ow + H + Lt)
    n2d = (2 * oh - 1) * (2 * ow - 1)
    draw = (lambda s: rng.integers(-8, 9, size=s).astype(F32)) if ints else (lambda s: rng.standard_normal(s).astype(F32))
    t2, r1, rx = draw((H, n2d)), draw((H, max(2 * Lt - 1, 1))), draw((H, 2))
    _ro(t2, r1, rx)
    return t2, r1, rx


def causal_hidden(P, Lt):
    """True where the kernel writes -inf under `causal` (internal order [grid | tail], the reference's is [tail, grid])"""
    T = P + Lt
    i, j = np.arange(T)[:, None], np.arange(T)[None, :]
    return np.where(i < P, (j < P) & (j > i), (j < P) | (j > i))


def bias_ref(case):
    """(ref [H, T, T] fp64 with -inf under the mask, bound [H, T, T] (0 outside the grid block: those are copies))"""
    oh, ow, h, w, H, Lt = (case[k] for k in ("oh", "ow", "h", "w", "H", "Lt"))
    P, T = h * w, h * w + Lt
    t2, r1, rx = bias_tables(oh, ow, H, Lt, case["ints"])
    M, m = interp2d(h, w, oh, ow)
    used = np.flatnonzero(np.abs(M).sum(0) > 0)
    Mu = M[:, used]
    ys, xs = np.divmod(used, ow)
    s0 = 2 * ow - 1
    code = ys * s0 + xs
    idx = code[:, None] - code[None, :] + (oh - 1) * s0 + (ow - 1)
    ref, bound = np.zeros((H, T, T)), np.zeros((H, T, T))
    for hd in range(H):
        B0 = t2[hd].astype(np.float64)[idx]
        ref[hd, :P, :P] = Mu @ B0 @ Mu.T
        A = float(np.abs(t2[hd]).max())
        bound[hd, :P, :P] = 16 * U * (m[:, None] + m[None, :]) * A + 16 * U * (np.abs(Mu) @ np.abs(B0) @ np.abs(Mu).T)
        if Lt:
            d = np.arange(Lt)[:, None] - np.arange(Lt)[None, :] + Lt - 1
            ref[hd, P:, P:] = r1[hd].astype(np.float64)[d] if case["tails"] else 0.0
            ref[hd, :P, P:] = float(rx[hd, 0]) if case["tails"] else 0.0
            ref[hd, P:, :P] = float(rx[hd, 1]) if case["tails"] else 0.0
    if case["causal"]:
        ref[:, causal_hidden(P, Lt)] = -np.inf
    return ref, bound


def bias_emul(case, fma=False, wrong=None, heads=None):
    """resized_bias_kernel in fp32, sums in the kernel's order.  wrong: "qk" (the query taps taken from the key position),
    "relx" (relx[0] and relx[1] exchanged), "loop" (the columns j >= 2048 left unwritten: they keep the sentinel)"""
    oh, ow, h, w, H, Lt = (case[k] for k in ("oh", "ow", "h", "w", "H", "Lt"))
    P, T = h * w, h * w + Lt
    t2, r1, rx = bias_tables(oh, ow, H, Lt, case["ints"])
    y, x, wy, wx = taps2d_f32(h, w, oh, ow, fma)
    s0 = 2 * ow - 1
    bias0 = (oh - 1) * s0 + (ow - 1)
    code = [y[:, t >> 1] * s0 + x[:, t & 1] for t in range(4)]
    wt = [(wy[:, t >> 1] * wx[:, t & 1]).astype(F32) for t in range(4)]
    heads = range(H) if heads is None else heads
    out = np.zeros((len(heads), T, T), dtype=F32)
    for n, hd in enumerate(heads):
        v = np.zeros((P, P), dtype=F32)
        for t in range(4):
            inner = np.zeros((P, P), dtype=F32)
            ca = (code[t][None, :] if wrong == "qk" else code[t][:, None]) + bias0
            for u in range(4):
                inner = (inner + (wt[u][None, :] * t2[hd][ca - code[u][None, :]]).astype(F32)).astype(F32)
            v = (v + ((wt[t][None, :] if wrong == "qk" else wt[t][:, None]) * inner).astype(F32)).astype(F32)
        out[n, :P, :P] = v
        if Lt:
            a, b = (1, 0) if wrong == "relx" else (0, 1)
            d = np.arange(Lt)[:, None] - np.arange(Lt)[None, :] + Lt - 1
            out[n, P:, P:] = r1[hd][d] if case["tails"] else 0
            out[n, :P, P:] = rx[hd, a] if case["tails"] else 0
            out[n, P:, :P] = rx[hd, b] if case["tails"] else 0
    if case["causal"]:
        out[:, causal_hidden(P, Lt)] = -np.inf
    if wrong == "loop":
        out[:, :, BIAS_LOOP_EDGE:] = SENTINEL
    return out


# ============================================================================================================ part C
L2_WIDTHS, L2_ROWS = (8, 504, 512, 520, 1024), 5


@functools.lru_cache(maxsize=None)
def l2norm_case(D):
    rng = np.random.default_rng(700 + D)
    x = bf16_round(rng.standard_normal((L2_ROWS, D)) * (2.0 ** (np.arange(L2_ROWS) - 2))[:, None])
    x[3] = 0.0
    x64 = x.astype(np.float64)
    ref = x64 / np.maximum(np.sqrt((x64 ** 2).sum(1, keepdims=True)), 1e-12)
    _ro(x, ref)
    return x, ref, U_BF16 * np.abs(ref) + (D + 16) * U * np.abs(ref)


def l2norm_emul(x):
    ss = _seq(x.astype(F32) * x.astype(F32), axis=1)[:, None]
    return bf16_round(x * (F32(1) / np.maximum(np.sqrt(ss), F32(1e-12))).astype(F32))


TOPK_NS, TOPK_ROWS = (1, 63, 64, 65, 130), 5
TOPK_CASES = [(N, k) for N in TOPK_NS for k in (1, 3, 8) if k <= N]


@functools.lru_cache(maxsize=None)
def topk_rows(N):
    """five rows: few distinct values (duplicates across lanes), all equal, mostly -inf, some NaN among +-inf, mostly NaN"""
    rng = np.random.default_rng(800 + N)
    r = np.zeros((TOPK_ROWS, N), dtype=F32)
    r[0] = rng.integers(-2, 3, N)
    r[1] = 0.5
    r[2] = np.where(rng.random(N) < 0.9, -np.inf, rng.integers(-2, 3, N))
    r[3] = rng.integers(-2, 3, N)
    r[3, rng.random(N) < 0.1] = np.nan
    r[3, rng.random(N) < 0.1] = np.inf
    r[3, N - 1] = np.nan
    r[4] = np.where(rng.random(N) < 0.95, np.nan, np.where(rng.random(N) < 0.5, np.inf, -np.inf))
    _ro(r)
    return r


def topk_ref(rows, k, higher_on_ties=False):
    """stable descending order, NaN first, the lower index first on ties (higher_on_ties: the wrong variant)"""
    out = np.zeros((rows.shape[0], k), dtype=np.int64)
    for n, r in enumerate(rows):
        idx = np.arange(r.size)
        val = np.where(np.isnan(r), np.inf, r.astype(np.float64))
        order = np.lexsort((-idx if higher_on_ties else idx, -val, ~np.isnan(r)))
        out[n] = order[:k]
    return out


SOFTMAX_NS, SOFTMAX_ROWS, SOFTMAX_RPB, SOFTMAX_T = (1, 5, 171), (1, 127, 129), 65, 70
SOFTMAX_CASES = ([dict(n=n, rows=r, softmax=False, temp=1.0) for n in SOFTMAX_NS for r in SOFTMAX_ROWS]
                 + [dict(n=n, rows=r, softmax=True, temp=(1.0, 0.5, 2.0)[(i + j) % 3]) for i, n in enumerate(SOFTMAX_NS) for j, r in enumerate(SOFTMAX_ROWS)]
                 + [dict(n=171, rows=129, softmax=True, temp=t) for t in (1.0, 0.5)] + [dict(n=5, rows=127, softmax=True, temp=2.0)])
for _c in SOFTMAX_CASES:
    _c["id"] = "n%d-r%d-%s" % (_c["n"], _c["rows"], "T%g" % _c["temp"] if _c["softmax"] else "copy")


@functools.lru_cache(maxsize=None)
def softmax_logits(n):
    """bf16 logits [2, SOFTMAX_T, n + 5] with |x| <= 1.25; the kernel reads rows [0, SOFTMAX_RPB) of a batch, columns [0, n)"""
    x = bf16_round(np.random.default_rng(850 + n).uniform(-1.25, 1.25, (2, SOFTMAX_T, n + 5)))
    _ro(x)
    return x


def softmax_rows_of(n, rows):
    x = softmax_logits(n)
    r = np.arange(rows)
    return x[r // SOFTMAX_RPB, r % SOFTMAX_RPB, :n]


def softmax_ref(case):
    x = softmax_rows_of(case["n"], case["rows"]).astype(np.float64)
    if not case["softmax"]:
        return x, np.zeros_like(x)
    a = x / case["temp"]
    e = np.exp(a - a.max(1, keepdims=True))
    ref = e / e.sum(1, keepdims=True)
    return ref, (16 + 2 * case["n"]) * U * ref


def softmax_emul(case):
    x = softmax_rows_of(case["n"], case["rows"]).astype(F32)
    a = (x * F32(1.0 / case["temp"])).astype(F32)
    e = np.exp(a - a.max(1, keepdims=True)).astype(F32)
    return (e * (F32(1) / _seq(e, axis=1))[:, None]).astype(F32)


GATHER_KS, GATHER_BPN = (1, 2, 3, 8), (2, 7, 5)


@functools.lru_cache(maxsize=None)
def gather_case(k):
    B, P, n = GATHER_BPN
    rng = np.random.default_rng(870 + k)
    x = rng.integers(-50, 51, size=(B, P, n)).astype(F32)
    idx = rng.integers(0, P, size=(B, P, k)).astype(np.int32)
    s = np.stack([x[b][idx[b]].astype(np.float64).sum(1) for b in range(B)])
    ref = (s.astype(F32) / F32(k)).astype(F32)          # the sum is an integer below 2^24; one correctly rounded division
    _ro(x, idx, ref)
    return x, idx, ref


SEG0, PAD_ID, EOS_ID = 1000, 1, 2
EVAL_SHAPES = ((3, 5, 37, 23), (4, 4, 64, 64), (8, 6, 5, 9), (1, 1, 4, 4))
EVAL_CASES = [dict(hp=s[0], wp=s[1], h=s[2], w=s[3], n=n, all_ignored=False, id="%dx%d-%dx%d-n%d" % (s + (n,))) for s in EVAL_SHAPES for n in (1, 5, 171)]
EVAL_CASES.append(dict(hp=3, wp=5, h=37, w=23, n=5, all_ignored=True, id="3x5-37x23-n5-ignored"))


@functools.lru_cache(maxsize=None)
def seg_eval_case(hp, wp, h, w, n, all_ignored=False):
    """scores fp32 [hp*wp, n] (|score| <= 2), target int64 [h*w] (valid labels, ignore = SEG0 + n, pad, eos, values below SEG0;
    the undecided pixels of the margin rule get the ignore label), the fp64 values, per-pixel loss and bound, the histograms"""
    from _predict_cases import MARGIN_CAP as CAP, Reference
    import torch
    rng = np.random.default_rng(900 + hp + 3 * wp + h + n)
    scores = rng.uniform(-2, 2, (hp * wp, n)).astype(F32)
    rule = Reference(torch.from_numpy(scores.copy())[None], hp, wp, h, w)
    decided = rule.decided[0].numpy().reshape(-1)
    My, Mx = interp_matrix(h, hp), interp_matrix(w, wp)
    v = np.kron(My, Mx) @ scores.astype(np.float64)                     # [h*w, n]
    assert np.array_equal(v.argmax(1), rule.labels[0].numpy().reshape(-1))
    m = np.maximum(1.0, np.maximum(taps1d(h, hp)[3][:, None], taps1d(w, wp)[3][None, :])).reshape(-1)
    kind = rng.random(h * w)
    lab = rng.integers(0, n, h * w)
    lab = np.where(rng.random(h * w) < 0.5, v.argmax(1), lab)            # half of the labels agree with the prediction
    target = SEG0 + lab
    for lo, val in ((0.70, SEG0 + n), (0.78, PAD_ID), (0.84, EOS_ID), (0.90, SEG0 - 1), (0.95, 5)):
        target = np.where(kind >= lo, val, target)
    target = np.where(decided, target, SEG0 + n)
    if all_ignored:
        target = np.where(np.arange(h * w) % 2 == 0, SEG0 + n, PAD_ID)
    target = target.astype(np.int64)
    t = target - SEG0
    valid = (t >= 0) & (t < n)
    tv = np.where(valid, t, 0)
    mx = v.max(1)
    loss = np.where(valid, mx + np.log(np.exp(v - mx[:, None]).sum(1)) - v[np.arange(h * w), tv], 0.0)
    A = float(np.abs(scores).max())
    bound = np.where(valid, (n + 32) * U * (1 + np.abs(loss)) + 2 * (16 * m + 8) * U * A, 0.0)
    hist = seg_eval_hist(v.argmax(1), target, n)
    _ro(scores, target, v, loss, bound, hist)
    return dict(scores=scores, target=target, v=v, valid=valid, loss=loss, bound=bound, hist=hist, undecided=float(1 - decided.mean()), cap=CAP,
                valid_share=float(valid.mean()))


def seg_eval_hist(arg, target, n, ignore_as_last=False):
    """[3, n]: intersection, predicted area, label area over the pixels whose target lies in [SEG0, SEG0 + n)
    (ignore_as_last: the wrong variant that counts the ignore label as class n - 1)"""
    t = target - SEG0
    if ignore_as_last:
        t = np.where(t == n, n - 1, t)
    valid = (t >= 0) & (t < n)
    a, t = arg[valid], t[valid]
    return np.stack([np.bincount(a[a == t], minlength=n), np.bincount(a, minlength=n), np.bincount(t, minlength=n)]).astype(np.int64)


def seg_eval_block_sums(case):
    """per block of 256 pixels: (sum of the fp64 losses, bound on the fp32 partial sum, count)"""
    nb = (case["loss"].size + 255) // 256
    pad = nb * 256 - case["loss"].size
    L, Bd, cnt = (np.pad(a.astype(np.float64), (0, pad)).reshape(nb, 256) for a in (case["loss"], case["bound"], case["valid"]))
    return L.sum(1), Bd.sum(1) + 16 * U * np.abs(L).sum(1), cnt.sum(1)


def seg_eval_emul(case, hp, wp, h, w, n):
    """the per-pixel loss of seg_eval_kernel in fp32 (online softmax in class order); 0 on the pixels that are not counted"""
    s = case["scores"]
    y0, y1, ly = taps1d_f32(h, hp, False)
    x0, x1, lx = taps1d_f32(w, wp, False)
    py, px = np.divmod(np.arange(h * w), w)
    ly, lx = ly[py], lx[px]
    one = F32(1)
    ws = [((one - ly) * (one - lx)).astype(F32), ((one - ly) * lx).astype(F32), (ly * (one - lx)).astype(F32), (ly * lx).astype(F32)]
    ps = [s[y0[py] * wp + x0[px]], s[y0[py] * wp + x1[px]], s[y1[py] * wp + x0[px]], s[y1[py] * wp + x1[px]]]
    v = np.zeros((h * w, n), dtype=F32)
    for wt, p in zip(ws, ps):
        v = (v + (wt[:, None] * p).astype(F32)).astype(F32)
    m, ssum = np.full(h * w, -np.inf, dtype=F32), np.zeros(h * w, dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(n):
            up = v[:, c] > m
            ssum = np.where(up, ssum * np.exp(np.where(up, m - v[:, c], 0)).astype(F32) + one, ssum + np.exp(np.where(up, 0, v[:, c] - m)).astype(F32)).astype(F32)
            m = np.where(up, v[:, c], m)
    tv = np.where(case["valid"], case["target"] - SEG0, 0)
    loss = ((m + np.log(ssum).astype(F32)).astype(F32) - v[np.arange(h * w), tv]).astype(F32)
    return np.where(case["valid"], loss, F32(0)), v
