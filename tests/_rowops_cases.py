"""Cases, data, fp64 references, derived bounds and CPU restatements for the conformance suite of csrc/rowops.hip
(test_rowops_conformance_cpu.py checks this module alone, test_rowops_conformance_gpu.py the kernels against it).
numpy only: nothing here touches the GPU or the library.

Part A -- the LayerNorm family against an fp64 reference computed from the bf16 inputs.  u = 2^-24 (fp32 unit roundoff).
Every bound has the form   2^-8 |ref| + (1 + 2^-8) u (k_acc A + k_loc L)   for a bf16 output (one round-to-nearest of the
computed value: bfloat16 has 8 significant bits) and   u (k_acc A)   for an fp32 output.  Nothing in them is measured.

Forward, a = x or gelu(x), mu = mean(a), rstd = (var(a) + eps)^-1/2, y = [resid +] ks (a - mu) rstd gamma + beta:
  mean:  C fp32 additions in any order are off by at most (C - 1) u sum|a_i|, the division adds one rounding; with GELU each
         summand carries 4 u |x| of its own (below):               |d mu| <= (C + 16) u mean(max(|a|, |x|)) =: (C + 16) u am
  rstd:  the C squares are positive, their sum is off by (C + 2) u relatively, the mean's error enters in second order
         only (sum (a - mu) = 0), the inverse square root halves it, rsqrtf adds 2 ulp: |d rstd| <= (C + 16) u rstd
  y:     d mu moves y by d mu rstd |gamma|, d rstd by |a - mu| d rstd |gamma|:       k_acc = C + 16,
         A = (am + |a - mu|) rstd |gamma| ks;   the subtraction, two multiplications, the addition of beta, the dropout scale
         and the residual add are one rounding each of a value no larger than L = (|xhat gamma| + |beta|) ks + |resid| + |y|
         (+ |x| rstd |gamma| ks with GELU),  k_loc = 16.
  GELU:  the reference applies the restatement of gelu_f / erf_as (common.h) below in numpy fp32 and widens it, so the
         polynomial's own 1.5e-7 is inside the reference; what remains between the kernel and the restatement is the ulp-level
         difference of __expf, v_rcp_f32 and fused multiply-adds: erf is off by at most 8 u absolutely (poly e <= 1, and an
         exponent error of |t| u costs |t| e^-|t| u <= 0.37 u), a = x (1 + erf) / 2 by 4 u |x|, the derivative by 16 u.
Backward, d = ks dy, g = d gamma, xhat = (a - mean) rstd with the fp32 mean / rstd THE FORWARD KERNEL produced (widened: the
backward is tested on its own), s1 = mean(g), s2 = mean(g xhat), dx = [dx_add +] act'(x) rstd (g - s1 - xhat s2):
  s1 is off by (C + 16) u mean|g|, s2 by (C + 16) u mean(|g| xe), xe = |xhat| (+ |x| rstd with GELU: the local error of xhat):
         k_acc = C + 16,  A = rstd (mean|g| + |xhat| mean(|g| xe)) max(1, |act'|);
         L = rstd (|g| + |s1| + xe |s2|) max(1, |act'|) + |dx_add| + |dx|,  k_loc = 32 (16 of it the derivative's 16 u).
  dgamma = sum_rows d xhat, dbeta = sum_rows d (fp32, through ifseg_reduce_parts): rows additions (idle blocks add zeros):
         (rows + 16) u sum_rows |d| xe   and   (rows + 16) u sum_rows |d|.
The CPU file asserts, for every case, that an fp32 emulation with strictly sequential row sums stays inside these bounds and
that a row which takes its neighbour's statistics leaves at least 80 % of its elements outside TWICE the bound.  Elements
that cannot depend on the statistics are not counted there: columns whose gain is zero and elements the mask drops (forward),
rows DropPath has zeroed and, with GELU, elements the activation gates off (act'(x) < 1/2: their dx is dx_add and little else).

Data is row-sensitive: row r has offset 0.5 ((r mod 7) - 3) and scale 2^((r mod 5) - 2), dy its own scale 2^(((r + 2) mod 4) - 2);
gamma has negative entries (every 4th) and zeros (5 mod 64, from C = 64 on); rows 1 .. n carry a spike (x = 64, dy = 16) in element 1
of the k-th designated chunk: chunk 0, lane 63's chunk, the first chunk of every further slice of the row (64 i for a wave per row,
256 for four waves per row), the last chunk.  A chunk that never enters a row sum then shows in the fp32 mean / rstd.

Part B -- splitmix64, drop8 and the DropPath uniform restated with numpy uint64 wrap-around arithmetic.
Part C -- integer-valued data for the side kernels: one correct value per element.
"""
import functools
import math

import numpy as np

U = 2.0 ** -24
U_BF16 = 2.0 ** -8
F32 = np.float32
EPS = F32(1e-5)
K_LOC_FWD, K_LOC_BWD = 16, 32
LN_WIDTHS = (8, 64, 504, 512, 520, 1016, 1024, 1032, 2048, 2056, 3072, 3080, 4096)
LN_MAX_C, LN_BWD_DROP_MAX_C = 4096, 1024


# ------------------------------------------------------------------------------------------------- bf16
def bf16_round(a):
    """float array -> float32 array of the nearest bf16 values (ties to even; NaN stays NaN): f2bf of common.h"""
    f = np.ascontiguousarray(a, dtype=F32)
    u = f.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = np.where(nan, (u & 0xFFFF0000) | 0x400000, r)
    return (r & 0xFFFFFFFF).astype(np.uint32).view(F32).reshape(f.shape)


def is_bf16(a):
    a = np.asarray(a, dtype=np.float64)
    return bool(np.all(bf16_round(a).astype(np.float64) == a))


def is_f32(a):
    a = np.asarray(a, dtype=np.float64)
    return bool(np.all(a.astype(F32).astype(np.float64) == a))


# ------------------------------------------------------------------------------- GELU, restated (common.h, rowops.hip)
def erf_as(x, e):
    """erf(x / sqrt 2) by Abramowitz-Stegun 7.1.26, every operation in fp32; e = exp(-x^2 / 2)"""
    x = np.asarray(x, dtype=F32)
    z = np.abs(x) * F32(0.70710678118654752)
    t = F32(1) / (F32(1) + F32(0.3275911) * z)
    poly = t * (F32(0.254829592) + t * (F32(-0.284496736) + t * (F32(1.421413741) + t * (F32(-1.453152027) + t * F32(1.061405429)))))
    r = F32(1) - poly * e
    return np.where(x < 0, -r, r).astype(F32)


def gelu_f32(x):
    x = np.asarray(x, dtype=F32)
    with np.errstate(under="ignore"):
        e = np.exp(F32(-0.5) * x * x).astype(F32)
    return (F32(0.5) * x * (F32(1) + erf_as(x, e))).astype(F32)


def gelu_grad_f32(x):
    """the derivative as ln_bwd_kernel<*, true, *> computes it (the forward's erf and exponential)"""
    x = np.asarray(x, dtype=F32)
    with np.errstate(under="ignore"):
        e = np.exp(F32(-0.5) * x * x).astype(F32)
    return (F32(0.5) * (F32(1) + erf_as(x, e)) + x * F32(0.39894228040143268) * e).astype(F32)


def finite_bf16_in(lo, hi):
    """every finite bf16 value in [lo, hi] as float32"""
    v = (np.arange(1 << 16, dtype=np.uint32) << 16).view(F32)
    v = v[np.isfinite(v)]
    return np.unique(v[(v >= lo) & (v <= hi)])


# ------------------------------------------------------------------------------------ dispatch, restated
def _b(flag):
    return "true" if flag else "false"


def fwd_reach(C, gelu):
    """ln_fwd_impl: chunks per lane by width"""
    return "ln_fwd_kernel<%d,%s>" % (2 if C <= 1024 else (6 if C <= 3072 else 8), _b(gelu))


def bwd_reach(C, gelu):
    """ifseg_ln_bwd: the lean kernel for narrow rows without GELU, a wave per row up to 1024, four waves per row above"""
    if C <= 1024 and not gelu:
        return "ln_bwd_lean_kernel<2,false>"
    return "ln_bwd_kernel<2,%s,%d>" % (_b(gelu), 1 if C <= 1024 else 4)


def bwd_drop_reach(C):
    """ifseg_ln_bwd_drop: one instantiation, narrow rows only"""
    return "ln_bwd_lean_kernel<2,true>" if C <= LN_BWD_DROP_MAX_C else None


def bwd_waves_per_row(C, gelu):
    return 4 if C > 1024 else 1


def reduce_reach(outer, parts, n):
    """ifseg_reduce_parts"""
    total = outer * n
    if parts >= 2048 and total <= 4096:
        return "reduce_parts_tall_kernel"
    return "reduce_parts2d_kernel" if parts >= 32 else "reduce_parts_kernel"


def designated_chunks(C, stride):
    """chunks a spike goes into: the first, lane 63's, the first of every further slice (`stride` chunks apart), the last"""
    nch = C // 8
    want = [0, 63] + list(range(stride, nch, stride)) + [nch - 1]
    out = []
    for c in want:
        if c < nch and c not in out:
            out.append(c)
    return out


# ---------------------------------------------------------------------------------------------- case tables
def _fwd(C, reach, rows=13, gelu=False, resid=False, drop=False, pf32=False, strided=False):
    tags = [t for t, on in (("gelu", gelu), ("resid", resid), ("drop", drop), ("pf32", pf32), ("strided", strided)) if on]
    return dict(C=C, reach=reach, rows=rows, gelu=gelu, resid=resid, drop=drop, pf32=pf32, strided=strided,
                id="fwd-%dx%d-%s" % (rows, C, "+".join(tags) or "plain"), seed=7000 + C + 17 * rows)


def _fwd_options(C, nch):
    """the options crossed over one instantiation pair (GELU off / on) at width C; every forward row count"""
    k0, k1 = "ln_fwd_kernel<%d,false>" % nch, "ln_fwd_kernel<%d,true>" % nch
    return [_fwd(C, k1, 13, gelu=True, resid=True, strided=True), _fwd(C, k0, 13, resid=True, drop=True, pf32=True, strided=True),
            _fwd(C, k1, 3, gelu=True, drop=True), _fwd(C, k0, 1, pf32=True), _fwd(C, k0, 4, resid=True, strided=True),
            _fwd(C, k1, 5, gelu=True, pf32=True, strided=True), _fwd(C, k0, 5, drop=True)]


# every width once plain (13 rows: four blocks, the last with one row), then the options per instantiation
FWD_CASES = ([_fwd(C, "ln_fwd_kernel<%d,false>" % (2 if C <= 1024 else 6 if C <= 3072 else 8)) for C in LN_WIDTHS]
             + _fwd_options(520, 2) + _fwd_options(1024, 2) + _fwd_options(1032, 6) + _fwd_options(3072, 6)
             + _fwd_options(3080, 8) + _fwd_options(4096, 8) + [_fwd(8, "ln_fwd_kernel<2,true>", 5, gelu=True, drop=True)])


def _bwd(C, reach, rows, nblocks, gelu=False, add=False, drop=False, pf32=False, strided=False):
    tags = [t for t, on in (("gelu", gelu), ("add", add), ("drop", drop), ("pf32", pf32), ("strided", strided)) if on]
    return dict(C=C, reach=reach, rows=rows, nblocks=nblocks, gelu=gelu, add=add, drop=drop, pf32=pf32, strided=strided,
                id="bwd-%dx%d-b%d-%s" % (rows, C, nblocks, "+".join(tags) or "plain"), seed=9000 + C + 17 * rows + nblocks)


def _bwd_trips(C, gelu):
    """rows of the multi-trip case with 3 blocks: 25 for a wave per row (12 rows a trip: two trips and a ragged third), 7 for
    four waves per row (3 rows a trip: two trips and one block with a third)"""
    return 25 if C <= 1024 else 7


def _bwd_options(C, gelu):
    k = bwd_reach(C, gelu)
    return [_bwd(C, k, _bwd_trips(C, gelu), 3, gelu, add=True, strided=True), _bwd(C, k, _bwd_trips(C, gelu), 3, gelu, drop=True, pf32=True),
            _bwd(C, k, 1, 3, gelu), _bwd(C, k, 12, 3, gelu, add=True, pf32=True, strided=True),
            _bwd(C, k, 5, 768, gelu, add=True, drop=True)]


BWD_CASES = ([_bwd(C, bwd_reach(C, False), _bwd_trips(C, False), 3) for C in LN_WIDTHS]
             + [_bwd(C, bwd_reach(C, True), _bwd_trips(C, True), 3, gelu=True) for C in LN_WIDTHS if C >= 504]
             + _bwd_options(520, False) + _bwd_options(1024, True) + _bwd_options(1032, False) + _bwd_options(4096, True)
             + [_bwd(8, "ln_bwd_kernel<2,true,1>", 5, 768, gelu=True, add=True)])

# ifseg_ln_bwd_drop (lean<2,true>): every narrow width, dx_add / layouts / fp32 gains crossed at 520 and 1024
BWD_DROP_CASES = ([_bwd(C, "ln_bwd_lean_kernel<2,true>", 25, 3, drop=True) for C in LN_WIDTHS if C <= 1024]
                  + [_bwd(520, "ln_bwd_lean_kernel<2,true>", 25, 3, add=True, drop=True, strided=True),
                     _bwd(1024, "ln_bwd_lean_kernel<2,true>", 12, 3, add=True, drop=True, pf32=True),
                     _bwd(520, "ln_bwd_lean_kernel<2,true>", 1, 3, drop=True, pf32=True, strided=True),
                     _bwd(1024, "ln_bwd_lean_kernel<2,true>", 5, 768, add=True, drop=True, strided=True)])

LN_INSTANTIATIONS = (["ln_fwd_kernel<%d,%s>" % (n, g) for n in (2, 6, 8) for g in ("false", "true")]
                     + ["ln_bwd_lean_kernel<2,false>", "ln_bwd_lean_kernel<2,true>", "ln_bwd_kernel<2,true,1>",
                        "ln_bwd_kernel<2,false,4>", "ln_bwd_kernel<2,true,4>"])
# (ln_bwd_kernel<2,false,1> is not instantiated: narrow rows without GELU always take the lean kernel, so nothing could reach
# it through the C ABI.  The bit-identity "lean partials == ln_bwd_kernel<2,false,1> partials" therefore has no case.)

DROP_P, DROP_SEED, DROP_RPB = 0.1, 0x9E3779B97F4A7C15 ^ 0x1234567, 2      # (the seed has bit 63 set)
DROP_DPSCALE = (1.25, 0.0, 2.0, 1.0, 0.5, 1.25, 0.0, 2.0, 1.0, 0.5, 1.25, 0.0, 2.0)   # per batch of DROP_RPB rows; DropPath zeros included


# ---------------------------------------------------------------------------------------------------- data
@functools.lru_cache(maxsize=None)
def ln_inputs(rows, C, seed, stride=64):
    """the bf16-representable operands of a case as float32 arrays (never written to): x, dy, resid, add [rows, C];
    gamma / beta as bf16 values and as fp32 values"""
    rng = np.random.default_rng(seed)
    r = np.arange(rows)
    off, sc = 0.5 * ((r % 7) - 3.0), 2.0 ** ((r % 5) - 2.0)
    dsc = 2.0 ** (((r + 2) % 4) - 2.0)
    x = rng.standard_normal((rows, C)) * sc[:, None] + off[:, None]
    dy = rng.standard_normal((rows, C)) * dsc[:, None]
    resid = rng.standard_normal((rows, C)) * sc[:, None]
    add = rng.standard_normal((rows, C)) * dsc[:, None]
    gamma = 1.0 + 0.25 * rng.standard_normal(C)
    gamma[::4] *= -1.0
    if C >= 64:
        gamma[5::64] = 0.0
    beta = 0.5 * rng.standard_normal(C)
    for k, c in enumerate(designated_chunks(C, stride)):
        if k + 1 < rows:
            x[k + 1, 8 * c + 1], dy[k + 1, 8 * c + 1] = 64.0, 16.0
    out = dict(x=bf16_round(x), dy=bf16_round(dy), resid=bf16_round(resid), add=bf16_round(add),
               gamma16=bf16_round(gamma), beta16=bf16_round(beta), gamma32=gamma.astype(F32), beta32=beta.astype(F32))
    for v in out.values():
        v.setflags(write=False)
    return out


def case_inputs(case, backward=False):
    stride = 256 if (backward and case["C"] > 1024) else 64
    d = dict(ln_inputs(case["rows"], case["C"], case["seed"], stride))
    d["gamma"], d["beta"] = (d["gamma32"], d["beta32"]) if case["pf32"] else (d["gamma16"], d["beta16"])
    return d


def case_keepscale(case):
    """keep * scale [rows, C] (fp32 values) of a case's fused dropout, or None"""
    if not case["drop"]:
        return None
    return drop_keepscale(case["rows"], case["C"], DROP_P, DROP_SEED, DROP_DPSCALE, DROP_RPB)


# ---------------------------------------------------------------------------------- references and bounds
def _act(x, gelu):
    x64 = x.astype(np.float64)
    if not gelu:
        return x64, np.ones_like(x64), np.zeros_like(x64)
    return gelu_f32(x).astype(np.float64), gelu_grad_f32(x).astype(np.float64), np.abs(x64)


def ln_fwd_ref(x, gamma, beta, gelu=False, resid=None, ks=None, stats=None, eps=EPS):
    """fp64 reference of ifseg_ln_fwd with its bounds; gamma None: the identity first stage of ifseg_ln_fwd_pair.
    `stats` = (mean, rstd) replaces the row statistics (the neighbour-swap check)."""
    C = x.shape[1]
    a, _, xloc = _act(x, gelu)
    ks64 = np.ones_like(a) if ks is None else ks.astype(np.float64)
    r64 = np.zeros_like(a) if resid is None else resid.astype(np.float64)
    if gamma is None:
        y = a * ks64 + r64
        return dict(y=y, y_b=U_BF16 * np.abs(y) + (1 + U_BF16) * U * 4 * (np.abs(a * ks64) + np.abs(r64) + np.abs(y)))
    g, b = gamma.astype(np.float64)[None, :], beta.astype(np.float64)[None, :]
    mean = a.mean(1, keepdims=True)
    rstd = 1.0 / np.sqrt(((a - mean) ** 2).mean(1, keepdims=True) + float(eps))
    am = np.maximum(np.abs(a), xloc).mean(1, keepdims=True)
    out = dict(mean=mean[:, 0], rstd=rstd[:, 0], mean_b=U * (C + 16) * am[:, 0], rstd_b=U * (C + 16) * rstd[:, 0])
    if stats is not None:
        mean, rstd = stats[0][:, None], stats[1][:, None]
    xh = (a - mean) * rstd
    y = (xh * g + b) * ks64 + r64
    A = (am + np.abs(a - mean)) * rstd * np.abs(g) * ks64
    L = (np.abs(xh * g) + np.abs(b) + xloc * rstd * np.abs(g)) * ks64 + np.abs(r64) + np.abs(y)
    out.update(y=y, y_b=U_BF16 * np.abs(y) + (1 + U_BF16) * U * ((C + 16) * A + K_LOC_FWD * L))
    return out


def ln_bwd_ref(dy, x, gamma, mean, rstd, gelu=False, add=None, ks=None):
    """fp64 reference of ifseg_ln_bwd (+ the reduced dgamma / dbeta) from the fp32 mean / rstd given, with its bounds"""
    rows, C = x.shape
    a, dact, xloc = _act(x, gelu)
    d = dy.astype(np.float64) * (1.0 if ks is None else ks.astype(np.float64))
    g = d * gamma.astype(np.float64)[None, :]
    mu, rs = mean.astype(np.float64)[:, None], rstd.astype(np.float64)[:, None]
    xh = (a - mu) * rs
    xe = np.abs(xh) + xloc * rs
    s1, s2 = g.mean(1, keepdims=True), (g * xh).mean(1, keepdims=True)
    a64 = np.zeros_like(a) if add is None else add.astype(np.float64)
    dx = rs * (g - s1 - xh * s2) * dact + a64
    dm = np.maximum(1.0, np.abs(dact))
    A = rs * (np.abs(g).mean(1, keepdims=True) + np.abs(xh) * (np.abs(g) * xe).mean(1, keepdims=True)) * dm
    L = rs * (np.abs(g) + np.abs(s1) + xe * np.abs(s2)) * dm + np.abs(a64) + np.abs(dx)
    return dict(dx=dx, dx_b=U_BF16 * np.abs(dx) + (1 + U_BF16) * U * ((C + 16) * A + K_LOC_BWD * L),
                dgamma=(d * xh).sum(0), dgamma_b=U * (rows + 16) * (np.abs(d) * xe).sum(0),
                dbeta=d.sum(0), dbeta_b=U * (rows + 16) * np.abs(d).sum(0))


def _seq_sum(v):
    """strictly sequential fp32 row sums (np.cumsum accumulates left to right in the array's type)"""
    return np.cumsum(v.astype(F32), axis=1, dtype=F32)[:, -1:]


def ln_fwd_emul(x, gamma, beta, gelu=False, resid=None, ks=None, eps=EPS):
    """ln_fwd_kernel in numpy fp32, row sums in sequential order: (y as bf16 values, mean, rstd)"""
    C = F32(x.shape[1])
    a = gelu_f32(x) if gelu else x.astype(F32)
    mu = _seq_sum(a) / C
    dd = a - mu
    rs = (F32(1) / np.sqrt(_seq_sum(dd * dd) / C + eps)).astype(F32)
    o = (a - mu) * rs * gamma.astype(F32)[None, :] + beta.astype(F32)[None, :]
    if ks is not None:
        o = o * ks.astype(F32)
    if resid is not None:
        o = o + resid.astype(F32)
    return bf16_round(o), mu[:, 0], rs[:, 0]


def ln_bwd_emul(dy, x, gamma, mean, rstd, gelu=False, add=None, ks=None):
    """ln_bwd_kernel in numpy fp32, sequential sums: (dx as bf16 values, dgamma, dbeta)"""
    C = F32(x.shape[1])
    a = gelu_f32(x) if gelu else x.astype(F32)
    da = gelu_grad_f32(x) if gelu else np.ones_like(a)
    d = dy.astype(F32) if ks is None else dy.astype(F32) * ks.astype(F32)
    mu, rs = mean.astype(F32)[:, None], rstd.astype(F32)[:, None]
    xh = (a - mu) * rs
    g = d * gamma.astype(F32)[None, :]
    s1, s2 = _seq_sum(g) / C, _seq_sum(g * xh) / C
    o = rs * (g - s1 - xh * s2) * da
    if add is not None:
        o = o + add.astype(F32)
    dg = np.cumsum((d * xh).astype(F32), axis=0, dtype=F32)[-1]
    db = np.cumsum(d.astype(F32), axis=0, dtype=F32)[-1]
    return bf16_round(o), dg, db


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound (0 where both vanish, inf where only the bound does)"""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, err / bound)
    ratio = np.nan_to_num(ratio, nan=np.inf)
    k = int(np.argmax(ratio)) if ratio.size else 0
    return (float(ratio.reshape(-1)[k]) if ratio.size else 0.0), np.unravel_index(k, ratio.shape) if ratio.size else ()


def fraction_outside(got, ref, bound, factor=2.0):
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    return float((err > factor * bound).mean())


# ----------------------------------------------------------------------------- masks, restated (part B)
M64 = (1 << 64) - 1


def splitmix64(z):
    """common.h: splitmix64 on uint64 arrays (wrap-around arithmetic)"""
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def splitmix64_int(z):
    """the same with python integers (the hand-checkable form)"""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def drop_threshold(p):
    return int(F32(p) * F32(65536.0))


def drop_keep(rows, C, p, seed, seed_add=0):
    """drop8: keep pattern [rows, C] (bool).  Chunk c8 = row * C/8 + chunk draws splitmix64(sd + 2 c8) for its elements 0..3 and
    splitmix64(sd + 2 c8 + 1) for 4..7, 16 bits per element from the low end; keep: bits >= uint(p * 65536)"""
    nch = C // 8
    sd = np.uint64((seed + seed_add) & M64)
    c8 = np.arange(rows * nch, dtype=np.uint64)
    with np.errstate(over="ignore"):
        r = [splitmix64(sd + np.uint64(2) * c8), splitmix64(sd + np.uint64(2) * c8 + np.uint64(1))]
    bits = np.stack([(r[e // 4] >> np.uint64(16 * (e % 4))) & np.uint64(0xFFFF) for e in range(8)], axis=1)
    return (bits >= np.uint64(drop_threshold(p))).reshape(rows, C)


def drop_scale(rows, p, dpscale=None, rows_per_batch=1):
    """the fp32 factor of a kept element, per row: dpscale[row / rows_per_batch] * (1 / (1 - p))"""
    inv = F32(1) / (F32(1) - F32(p)) if p > 0 else F32(1)
    dps = np.ones(rows, dtype=F32) if dpscale is None else np.asarray(dpscale, dtype=F32)[np.arange(rows) // rows_per_batch]
    return (dps * inv).astype(F32)


def drop_keepscale(rows, C, p, seed, dpscale=None, rows_per_batch=1, seed_add=0):
    return (drop_keep(rows, C, p, seed, seed_add) * drop_scale(rows, p, dpscale, rows_per_batch)[:, None]).astype(F32)


def droppath_uniform(n, B, seed, seed_add=0):
    """droppath_scale_kernel: the 24-bit uniform of element gid = i * B + b"""
    sd = np.uint64((seed + seed_add) & M64)
    gid = np.arange(n * B, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = splitmix64(sd + np.uint64(0x5851F42D4C957F2D) * (gid + np.uint64(1)))
    return ((z >> np.uint64(40)).astype(np.float64) * 2.0 ** -24).astype(F32).reshape(n, B)


def droppath_scale(keep, B, seed, seed_add=0):
    keep = np.asarray(keep, dtype=F32)
    u = droppath_uniform(keep.size, B, seed, seed_add)
    with np.errstate(divide="ignore"):
        return np.where(u < keep[:, None], F32(1) / keep[:, None], F32(0)).astype(F32)


# ------------------------------------------------------------------------------- side kernels (part C)
def ints(shape, seed, lim):
    return np.random.default_rng(seed).integers(-lim, lim + 1, size=shape).astype(F32)


@functools.lru_cache(maxsize=None)
def segment_sum_case(C, weighted, ends=False):
    """rows_segment_sum: sorted ids with runs of 1, 2, 33 and 300 equal ids; ids equal to skip_id, negative and >= V mixed in
    (sorted: the negative ones come first, those >= V last); `ends`: a valid run at j = 0 and one ending at m - 1 instead.
    Values in [-4, 4] (even where weights from {0.5, 1, 2} apply), thinned so that every |sum| stays <= 256"""
    if ends:
        V, skip, runs = 9, 4, [(0, 2), (1, 1), (4, 3), (5, 300), (7, 1), (8, 33)]
    else:
        V, skip, runs = 12, 5, [(-3, 2), (-1, 1), (0, 2), (2, 1), (3, 33), (5, 4), (6, 300), (7, 1), (9, 2), (12, 3), (16, 1)]
    ids = np.concatenate([np.full(n, i, dtype=np.int64) for i, n in runs])
    return _segment_sum_build(ids, V, skip, C, weighted, 11 + int(ends))


def _segment_sum_build(ids, V, skip, C, weighted, seed):
    rng = np.random.default_rng(seed + C)
    m, S = ids.size, 400
    src = (2 * rng.integers(-2, 3, size=(S, C)) if weighted else rng.integers(-4, 5, size=(S, C))).astype(F32)
    src[rng.random((S, C)) < 0.75] = 0.0
    src_row = rng.integers(0, S, size=m).astype(np.int64)
    w = rng.choice(np.array([0.5, 1.0, 2.0], dtype=F32), size=m) if weighted else None
    prior = rng.integers(-3, 4, size=(V, C)).astype(F32)
    ref = prior.astype(np.float64).copy()
    touched = np.zeros(V, dtype=bool)
    for j in range(m):
        i = int(ids[j])
        if 0 <= i < V and i != skip:
            ref[i] += (1.0 if w is None else float(w[j])) * src[src_row[j]].astype(np.float64)
            touched[i] = True
    partial = np.zeros((V, C))
    worst = 0.0
    for j in range(m):                                   # every prefix of a run's sum stays exact in fp32 and small
        i = int(ids[j])
        if 0 <= i < V and i != skip:
            partial[i] += (1.0 if w is None else float(w[j])) * src[src_row[j]].astype(np.float64)
            worst = max(worst, float(np.abs(partial[i]).max()))
    return dict(ids=ids, V=V, skip=skip, src=src, src_row=src_row, w=w, prior=prior, ref=ref, touched=touched, worst_partial=worst)


MASK_WIDTHS = (8, 520)
MASK_ROWS, MASK_PS = 5, (0.0, 0.1, 0.999)


MASK_DPSCALE = (1.25, 2.0, 0.5)           # per batch of DROP_RPB rows: none zero, so that a zero output is a dropped element


@functools.lru_cache(maxsize=None)
def mask_ln_inputs(C):
    """operands whose LayerNorm output is never near zero: gains in [0.75, 1.25], every bias 12"""
    rng = np.random.default_rng(4000 + C)
    x = bf16_round(rng.standard_normal((MASK_ROWS, C)) * (2.0 ** (np.arange(MASK_ROWS) % 3))[:, None])
    dy = bf16_round(rng.standard_normal((MASK_ROWS, C)))
    gamma = bf16_round(1.0 + 0.25 * rng.uniform(-1, 1, C))
    return dict(x=x, dy=dy, gamma=gamma, beta=np.full(C, 12.0, dtype=F32))


def _red(outer, parts, n, reach, **kw):
    c = dict(outer=outer, parts=parts, n=n, reach=reach, bf16=False, acc=False, scale=1.0)
    c.update(kw)
    c["id"] = "%dx%dx%d-%s%s-s%g" % (outer, parts, n, "bf16" if c["bf16"] else "f32", "+acc" if c["acc"] else "", c["scale"])
    return c


def _red_variants(outer, parts, n, reach):
    return [_red(outer, parts, n, reach), _red(outer, parts, n, reach, bf16=True, acc=True, scale=0.5),
            _red(outer, parts, n, reach, acc=True, scale=2.0), _red(outer, parts, n, reach, bf16=True, scale=2.0)]


# ifseg_reduce_parts: one block of rows per kernel, both sides of parts = 31 / 32 and 2047 / 2048 and of total = 4096 / 4097;
# n = 45 is no multiple of 32
REDUCE_CASES = (_red_variants(2, 31, 45, "reduce_parts_kernel") + _red_variants(1, 1, 300, "reduce_parts_kernel")
                + _red_variants(2, 32, 45, "reduce_parts2d_kernel") + _red_variants(1, 2047, 45, "reduce_parts2d_kernel")
                + [_red(1, 2048, 4097, "reduce_parts2d_kernel"), _red(1, 2048, 4097, "reduce_parts2d_kernel", bf16=True, acc=True, scale=0.5)]
                + _red_variants(2, 2048, 45, "reduce_parts_tall_kernel")
                + [_red(1, 2048, 4096, "reduce_parts_tall_kernel"), _red(1, 2048, 4096, "reduce_parts_tall_kernel", bf16=True, acc=True, scale=2.0)])


@functools.lru_cache(maxsize=4)
def _reduce_draw(outer, parts, n):
    rng = np.random.default_rng(outer * 7 + parts * 13 + n)
    v = rng.integers(-1, 2, size=(outer, parts, n)).astype(F32)
    if parts > 64:
        v[rng.random((outer, parts, n)) < 0.75] = 0.0
    prev = rng.integers(-4, 5, size=(outer, n)).astype(F32)
    v.setflags(write=False)
    prev.setflags(write=False)
    return v, prev, v.astype(np.float64).sum(1)


def reduce_case(c):
    v, prev, s = _reduce_draw(c["outer"], c["parts"], c["n"])
    return dict(inp=v, prev=prev, ref=s * c["scale"] + (prev if c["acc"] else 0.0), absmax=float(np.abs(s).max()))


EMBED_WIDTHS = (8, 264)
BAG_SIZES_EXACT = ((0, 1, 2, 4, 8, 1), (8, 0, 4, 2, 1, 1))     # per sample; both end exactly at maxlen = 16
BAG_SIZES_ROUNDED = ((3, 5, 1, 0, 2, 5), (5, 3, 3, 5, 0, 0))


@functools.lru_cache(maxsize=None)
def embed_case(C, sizes=BAG_SIZES_EXACT, with_add=True):
    rng = np.random.default_rng(300 + C)
    V = 37
    table = rng.integers(-8, 9, size=(V, C)).astype(F32)
    add = rng.integers(-4, 5, size=C).astype(F32) if with_add else None
    sizes = np.array(sizes, dtype=np.int64)
    ends = sizes.cumsum(1)
    maxlen = int(ends.max())
    ids = rng.integers(0, V, size=(sizes.shape[0], maxlen)).astype(np.int64)
    a64 = np.zeros(C) if add is None else add.astype(np.float64)
    rows_ref = table[ids].astype(np.float64) + a64
    bag = np.zeros((sizes.shape[0], sizes.shape[1], C))
    mag = np.zeros_like(bag)
    for b in range(sizes.shape[0]):
        for p in range(sizes.shape[1]):
            lo, hi = (int(ends[b, p - 1]) if p else 0), int(ends[b, p])
            if hi > lo:
                bag[b, p] = table[ids[b, lo:hi]].astype(np.float64).sum(0) / (hi - lo)
            mag[b, p] = np.abs(bag[b, p]) + np.abs(a64)
            bag[b, p] += a64
    return dict(table=table, add=add, ids=ids, ends=ends, maxlen=maxlen, rows_ref=rows_ref, bag_ref=bag, bag_mag=mag,
                ends_at_maxlen=bool((ends[:, -1] == maxlen).all()))


REL_SHAPES = ((1, 1), (85, 3), (64, 4), (257, 1))        # (n, H): n H = 1, 255, 256, 257


@functools.lru_cache(maxsize=None)
def rel_case(n, H, L=1):
    rng = np.random.default_rng(500 + n * H + L)
    nb = 19
    tables = rng.integers(-100, 101, size=(L, nb, H)).astype(F32)
    idx = rng.integers(-3, nb, size=n).astype(np.int32)        # negative indices and duplicates
    if n > 2:
        idx[0], idx[n - 1] = -1, idx[1] if idx[1] >= 0 else 0
    gathered = np.where(idx[None, None, :] >= 0, tables[:, np.maximum(idx, 0), :].transpose(0, 2, 1), 0.0).astype(np.float64)
    d = rng.integers(-8, 9, size=(H, n)).astype(F32)
    prior = rng.integers(-5, 6, size=(nb, H)).astype(F32)
    acc = prior.astype(np.float64).copy()
    for i in range(n):
        if idx[i] >= 0:
            acc[idx[i]] += d[:, i]
    return dict(tables=tables, idx=idx, gathered=gathered, d=d, prior=prior, acc=acc, nb=nb)


KPROJ_SHAPES = ((255, 8), (32, 64), (257, 8))            # N C / 8 = 255, 256, 257 threads


@functools.lru_cache(maxsize=None)
def kproj_case(N, C):
    rng = np.random.default_rng(700 + N + C)
    gw, db, xm = rng.integers(-8, 9, size=(N, C)).astype(F32), rng.integers(-3, 4, size=N).astype(F32), rng.integers(-4, 5, size=C).astype(F32)
    return dict(gw=gw, db=db, xmean=xm, ref=gw.astype(np.float64) - db.astype(np.float64)[:, None] * xm.astype(np.float64)[None, :])


@functools.lru_cache(maxsize=None)
def colsum_case(M, N):
    rng = np.random.default_rng(800 + M + N)
    x = rng.integers(-1, 2, size=(M, N)).astype(F32)
    return dict(x=x, sum=x.astype(np.float64).sum(0))


COLSUM_SHAPES = ((512, 8), (504, 8), (512, 2056), (5, 264), (256, 8), (520, 8))     # 64 * 8 rows, just below, just above


def EXACT_CASES():
    """(what, ok): every expected value of an exact comparison is representable in its output type"""
    for c in REDUCE_CASES:
        r = reduce_case(c)
        yield dict(what="reduce " + c["id"], ok=(is_bf16 if c["bf16"] else is_f32)(r["ref"]) and r["absmax"] <= 128 and is_bf16(r["prev"]))
    for C in EMBED_WIDTHS:
        for add in (True, False):
            e = embed_case(C, BAG_SIZES_EXACT, add)
            yield dict(what="embed %d" % C, ok=is_bf16(e["rows_ref"]) and is_bf16(e["bag_ref"]) and e["ends_at_maxlen"])
        yield dict(what="embed %d (bags of 3 and 5)" % C, ok=embed_case(C, BAG_SIZES_ROUNDED)["ends_at_maxlen"])
    for n, H in REL_SHAPES:
        for L in (1, 16):
            r = rel_case(n, H, L)
            yield dict(what="rel %dx%d L%d" % (n, H, L), ok=is_bf16(r["tables"]) and is_f32(r["acc"]) and (r["idx"] < 0).any() == (n > 2 or bool((r["idx"] < 0).any())))
    for N, C in KPROJ_SHAPES:
        yield dict(what="kproj %dx%d" % (N, C), ok=is_bf16(kproj_case(N, C)["ref"]))
    for M, N in COLSUM_SHAPES:
        yield dict(what="colsum %dx%d" % (M, N), ok=is_f32(colsum_case(M, N)["sum"] / (2 ** int(math.log2(M)) if M & (M - 1) == 0 else 1)))
