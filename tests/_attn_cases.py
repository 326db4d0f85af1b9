"""Data, fp64 references, bounds and case tables of the attention conformance suite (test_attn_conformance_cpu.py checks
them without a GPU, test_attn_conformance_gpu.py runs the kernels of csrc/attention.hip, attention_bi.hip and attention_ops.hip
against them).  numpy only.

Regimes of part A (nothing in them is measured)
------------------------------------------------
select   q (or q and pos_q) carries the +-CQ sign code of ONE key index sel(b, h, t), k (or k and pos_k) the +-CK code of its own
         index: NBITS bits, DPB columns per bit, so score(t, j) = CQ CK DPB (NBITS - 2 hamming(sel, j)) + bias.  The winner beats
         every other key by 2 CQ CK DPB = 320 minus the spread of the (small integer) bias, at least 256 in natural units = 369 in
         log2 units.  exp2(-369) is 0 in fp32, so every other probability is exactly 0; the winner's exponent is
         fma(s, log2 e, -fl(s log2 e)), at most an ulp of s log2 e < 2^12, i.e. |exponent| < 2^-11 and p in 1 +- 2^-11, which rounds
         to bf16 1.0 (round to nearest even).  With v, dout small integers and gains in {0, +-0.5, 1, 2}:
             out[t] == gain v[sel(t)]  bit for bit (gain v (1 +- 2^-11) rounds back to the bf16 value gain v),
             dv[j]  == gain sum_{t: sel(t) = j} dout[t], dq == dk == dbias == 0 exactly (dP == delta exactly: integers),
             dgain_rows == dout . v[sel] within 2^-12 relative (the fp32 p of the backward is exp2(fma(s, log2 e, -lse)): the
                 product is exact, lse < 2^12 carries half an ulp from fl(s log2 e) and half an ulp from its own store, 2^-12
                 together, and p - 1 = ln 2 times that),
             lse == s log2 e within 4 fp32 ulps of its magnitude.
         With dropout p = 0.5 the scale 1 / (1 - p) is exactly 2: out == 2 gain v[sel] keep[t, sel], the same for dv.
poison   the same, and every key a row must not see scores HIGHER than any winner (POISON = 4096 > 1920 + bias): rows of the K
         allocation outside [0, S) (guard rows before and after each batch element), keys >= kv_len[b], causal-masked pairs (the
         rel-pos table entries of negative code difference and relx[1] hold POISON_REL), the tiles ifseg_attn_dense_bias leaves
         unwritten under causal (D is pre-filled with POISON_REL).  -inf entries of a dense fp32 bias sit where sel never points.
         The V rows of poisoned keys hold V_POISON.  All poison is finite.  A mask applied one key, one row or one tile off lets a
         poisoned key win and flips whole rows of out.  kv_len = 0 and fully masked rows are out of scope: every row of every
         case has at least one allowed key (checked on the CPU).
uniform  q = 0, zero bias: every allowed key has p = 1 / n_t.  v is a +-1 code of the key index, dout is a POSITIVE integer code
         (no cancellation in dv, see below).  out[t] = gain mean_{allowed} v: the unnormalised p is exp2(0) = 1 = bf16 1.0, the
         sums are exact integers, l = n_t exactly, so the only roundings are 1 / l and the product in fp32 (2^-23 together) and
         the bf16 store: |err| <= 2^-8 |ref| + 2^-20 |ref|.
         dv[j] = gain sum_t dout[t] / n_t has the same bound where every n_t is a power of two (p = exp2(-lse) = 1 / n_t is a
         bf16 value).  Any other 1 / n_t is rounded to bf16 on its way into the MFMA, up to 2^-8 relative (8 significant bits:
         1 / 30 -> 137 * 2^-12, +0.34 %).  That adds 2^-8 |g| sum_{t: n_t not a power of two} dout[t] / n_t (dout > 0: no
         cancellation).  A kernel within format exceeded the first bound alone by up to 1.56x at such elements; the term is
         the rounding of P that part B counts as well.  T, S <= 256: one missing or extra (t, j) pair moves some element by >= twice the bound
         (proven by enumeration in the CPU file).

Bounds of part B (random values; from the rounding model of the kernels, not from observation)
-----------------------------------------------------------------------------------------------
u = 2^-8 bounds one round-to-nearest to bf16 (8 significant bits).  Scores are fp32 MFMA sums of D = 64 (128 with pos) exact
products plus an fp32 bias: |ds| <= es = (D + 2) 2^-24 max_j sum_d |q_d k_d| + 2^-23 max|bias| per row, and p = exp2(s log2 e - m)
carries the relative error el = 2 es + 2^-20 (numerator and normaliser, v_exp_f32 is good to 1 ulp).
  out   |out - ref| <= u |ref| + (2 u + el) |g| sum_j p_j |v_j|        one rounding of the result, one of each P (the forward
                                                                         normalises by the fp32 sum of the UNROUNDED p), the scores
  dv    |dv - ref|  <= u |ref| + (u + el) |g| sum_t p_tj ks_tj |dout_t|  (the gain is applied in fp32 at the store)
  dS    e_dS(i, j) = p ((u_g) |g| sum_d |dout_d v_d| + (D + 2) 2^-24 |g| sum_d |dout_d v_d| + 2^-23 (|dP| + |delta|)) + el |dS|
        with u_g = u in the dK/dV kernels of both files (dk, dpos_k, and the table partials of attention.hip): they hold the V rows
        as -gain v ROUNDED TO BF16 (scale_bf16x8; the dP accumulator is seeded with delta, so the MFMAs leave delta - gain dP),
        and u_g = 0 in the dQ kernels, which apply the gain in fp32.  The first derivation had u_g = 0 for attention.hip: every
        dk of part B exceeded it (2.9x - 19.5x, profiles/attn_conformance.txt); the term is this rounding, nothing is fitted.
  dgain_rows = sum_j p dP (fp32 fma chain over the keys): (el + (66 + S) 2^-24) sum_j p |dout|.|v|
  dq    |dq - ref|  <= u |ref| + |dq_scale| sum_j (u |dS_ij| + e_dS) |k_j|
  dk    |dk - ref|  <= u |ref| + sum_i (u |dS_ij| + e_dS) |q_i|          (dpq / dpk partials: the same with |pos_k| / |pos_q|)
  dbias |db - ref|  <= u |ref| + sum_b (u |dS| + e_dS)                   (bf16 slab per group of four batch elements)
  lse   |lse - ref| <= (es + el) log2 e + 2^-20 + 4 ulp(lse)             (lse_bound: the maximum and the normaliser, v_log_f32, the store)
  table partials (fp32, summed over the parts): table_refs_and_bounds -- e_dS with u_g, 2^-18 of the bin's own |dS|, and on
        row32 / rowseg grids 96 * 2^-24 of the block's column sums for d rel2d (the bins are differences of class sums there)
Every one of these bounds is asserted on emulate_forward / emulate_backward / emulate_table_bins by the CPU file.
`delta` is computed in fp64 from the kernel's own bf16 `out`, P from the kernel's own `lse` (both checked by the forward
tests), as the LayerNorm suite takes the kernel's own mean and rstd.
"""
import functools

import numpy as np

LOG2E = 1.4426950408889634
U = 2.0 ** -8                         # one rounding to bf16
NBITS, DPB, CQ, CK = 12, 5, 4.0, 8.0   # sign code: 12 bits x 5 columns = 60 of the 64 head columns
WIN = CQ * CK * DPB * NBITS            # 1920: the score of a matching code
GAP_MIN_LOG2 = 200.0
POISON_COL, POISON_K = 60, 256.0       # columns 60..63: q holds CQ everywhere, a poisoned key POISON_K -> 4 * 4 * 256 = 4096
POISON = 4 * CQ * POISON_K
POISON_REL = 8192.0                    # table entries / D tiles no row may see
V_POISON = 30720.0                     # 240 * 2^7: a bf16 value
GAINS = (1.0, -0.5, 2.0, 0.0)          # head h takes GAINS[h % 4]: exact products with small integers
DROP_SEED = 0x5DEECE66D1234567


def bf16_round(x):
    """float -> nearest bf16 value (ties to even), as float32"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    b = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) << 16
    return b.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def grid_codes(gh, gw):
    ys, xs = np.meshgrid(np.arange(gh), np.arange(gw), indexing="ij")
    return (ys * (2 * gw - 1) + xs).reshape(-1).astype(np.int32), (gh - 1) * (2 * gw - 1) + (gw - 1), (2 * gh - 1) * (2 * gw - 1)


def causal_mask(T, S, P):
    """True = hidden; the rule of test_kernels_gpu._causal_mask ("tail-first": grid rows see grid keys j <= i and every tail key,
    tail rows see tail keys j <= i only)"""
    i, j = np.arange(T)[:, None], np.arange(S)[None, :]
    gk = j < P
    return (gk & ((i >= P) | (j > i))) | (~gk & (i >= P) & (j > i))


# ------------------------------------------------------------------------------------------------ case tables
def _c(id, entry, B, H, T, S, reach, grid=None, Lt=0, causal=False, pos=False, dense=None, layout="fused", grid_w=None,
       kv_len=None, drop=False, P=None):
    gh, gw = grid if grid else (0, 0)
    Pg = gh * gw if grid else (P if P is not None else None)
    if grid:
        T = S = Pg + Lt
    return dict(id=id, entry=entry, B=B, H=H, T=T, S=S, reach=reach, gh=gh, gw=gw, P=Pg, Lt=Lt if grid else 0, causal=causal, pos=pos,
                dense=dense, layout=layout, grid_w=(gw if grid_w is None else grid_w), kv_len=kv_len, drop=drop)


# ifseg_attn_fwd / ifseg_attn_bwd.  reach = bias path / HAS_POS / dK-dV kernel; B * H: 4 (nq H B not a multiple of 8) and 8
GRID_CASES = [
    _c("row32-2x32+37-pos", "fwd", 2, 2, 0, 0, "row32/pos/dkv4", (2, 32), 37, pos=True),
    _c("row32-2x32+1-causal-bh8", "fwd", 2, 4, 0, 0, "row32/nopos/dkv4", (2, 32), 1, causal=True),
    _c("row32-2x32+1-causal-pos-dense", "fwd", 1, 2, 0, 0, "row32/pos/dkv4", (2, 32), 1, causal=True, pos=True, layout="dense"),
    _c("rowseg-8x40+37", "fwd", 1, 2, 0, 0, "rowseg/nopos/dkv4", (8, 40), 37),
    _c("rowseg-8x40+1-causal-pos", "fwd", 2, 2, 0, 0, "rowseg/pos/dkv4", (8, 40), 1, causal=True, pos=True),
    _c("rowseg-4x48+37-pos", "fwd", 1, 2, 0, 0, "rowseg/pos/dkv4", (4, 48), 37, pos=True),
    _c("rowseg-4x48+1-causal", "fwd", 2, 2, 0, 0, "rowseg/nopos/dkv4", (4, 48), 1, causal=True),
    _c("generic-8x8+37-pos", "fwd", 2, 2, 0, 0, "generic/pos/dkv4", (8, 8), 37, pos=True),
    _c("generic-16x12+1-causal", "fwd", 2, 2, 0, 0, "generic/nopos/dkv4", (16, 12), 1, causal=True),
    _c("generic-16x36+37", "fwd", 1, 2, 0, 0, "generic/nopos/dkv4", (16, 36), 37),
    _c("generic-8x16+37-gridw0-pos", "fwd", 2, 4, 0, 0, "generic/pos/dkv4", (8, 16), 37, pos=True, grid_w=0),
    _c("rowseg-40x40+37-pos", "fwd", 1, 2, 0, 0, "rowseg/pos/dkv8", (40, 40), 37, pos=True),
    _c("rowseg-40x40+1-causal", "fwd", 1, 2, 0, 0, "rowseg/nopos/dkv8", (40, 40), 1, causal=True),     # the other 8-wave instantiation
]
DENSE_CASES = [      # fp32 dense bias (forward only: ifseg_attn_bwd has no dense operand)
    _c("dense-ld4-165", "fwd", 2, 2, 165, 165, "dfast/nopos", dense="ld4", layout="dense"),
    _c("dense-ldodd-165", "fwd", 2, 2, 165, 165, "dslow/nopos", dense="ldodd", layout="dense"),
    _c("dense-ld4-100x130-pos", "fwd", 1, 2, 100, 130, "dfast/pos", dense="ld4", pos=True, layout="cross"),
]
_EDGES = [(1, 129), (129, 1), (65, 128), (1, 1), (31, 31), (64, 64), (65, 65), (127, 193), (128, 127), (129, 64), (193, 65)]
PLAIN_CASES = [_c("plain-%dx%d%s" % (T, S, "-pos" if n % 3 == 0 else ""), "fwd", 2 if n % 2 else 1, 4 if n % 4 == 1 else 2, T, S,
                  "plain/%s/dkv4" % ("pos" if n % 3 == 0 else "nopos"), pos=n % 3 == 0,
                  layout="dense" if n == 5 else ("fused" if T == S else "cross")) for n, (T, S) in enumerate(_EDGES)]
FWD_CASES = GRID_CASES + DENSE_CASES + PLAIN_CASES
BWD_CASES = GRID_CASES + PLAIN_CASES

# batch-inner kernels (ifseg_attn_fwd_bi / ifseg_attn_bwd_bi): groups of four batch elements, slabs of dbias per group
BI_CASES = [
    _c("bi-b1-31x33", "bi", 1, 2, 31, 33, "bi/g1", layout="cross"),
    _c("bi-b3-33x31-kvlen", "bi", 3, 2, 33, 31, "bi/g1/kvlen", layout="cross", kv_len=(31, 30, 1)),
    _c("bi-b4-63x65-drop", "bi", 4, 2, 63, 65, "bi/g1/drop", layout="cross", drop=True),
    _c("bi-b5-65x63-kvlen-drop", "bi", 5, 2, 65, 63, "bi/g2/kvlen/drop", layout="cross", kv_len=(63, 62, 32, 33, 1), drop=True),
    _c("bi-b9-64x64", "bi", 9, 1, 64, 64, "bi/g3", layout="fused"),
    _c("bi-b5-65x65-kvlen-dense", "bi", 5, 2, 65, 65, "bi/g2/kvlen", layout="dense", kv_len=(65, 64, 33, 32, 1)),
    _c("bi-b3-causal-p64", "bi", 3, 2, 65, 65, "bi/g1/causal", P=64, causal=True),
    _c("bi-b5-causal-p128-drop", "bi", 5, 2, 129, 129, "bi/g2/causal/drop", P=128, causal=True, drop=True),
]
UNIFORM_CASES = [c for c in FWD_CASES + BI_CASES if c["T"] <= 256 and c["S"] <= 256 and not c["drop"]
                 and c["id"] in ("row32-2x32+37-pos", "row32-2x32+1-causal-bh8", "generic-16x12+1-causal", "rowseg-4x48+1-causal",
                                 "dense-ld4-165", "plain-65x128", "plain-129x1", "plain-127x193", "bi-b3-33x31-kvlen", "bi-b9-64x64",
                                 "bi-b5-65x65-kvlen-dense", "bi-b3-causal-p64")]
# part B: one case per path at the same shapes, big_enc and the 40 x 40 grid
RANDOM_CASES = [c for c in FWD_CASES + BI_CASES
                if c["id"] in ("row32-2x32+37-pos", "row32-2x32+1-causal-bh8", "rowseg-8x40+1-causal-pos", "rowseg-4x48+37-pos",
                               "generic-8x8+37-pos", "generic-16x36+37", "dense-ld4-165", "dense-ldodd-165", "plain-65x128",
                               "plain-127x193", "rowseg-40x40+37-pos", "bi-b3-33x31-kvlen", "bi-b4-63x65-drop", "bi-b5-65x65-kvlen-dense",
                               "bi-b5-causal-p128-drop", "plain-65x65-pos", "dense-ld4-100x130-pos", "rowseg-8x40+37",
                               "generic-8x16+37-gridw0-pos")] + [
    _c("big_enc-32x32+36-pos", "fwd", 1, 2, 0, 0, "row32/pos/dkv4", (32, 32), 36, pos=True),
    _c("bi-big_enc-32x32+36", "bi", 2, 2, 1060, 1060, "bi/g1", layout="fused"),
]

KT_BYTES, VT_BYTES = 64 * 256, 64 * 128


def reach(c):
    """the dispatch of ifseg_attn_fwd / ifseg_attn_bwd (attention.hip: the kernels' row32 / rowseg / dfast predicates, the host's
    HAS_POS choice and its LDS formula for the 8-wave dK/dV kernel) and of the batch-inner entry points, restated"""
    if c["entry"] == "bi":
        r = "bi/g%d" % ((c["B"] + 3) // 4)
        return r + ("/kvlen" if c["kv_len"] else "") + ("/causal" if c["causal"] else "") + ("/drop" if c["drop"] else "")
    rel = c["gh"] > 0
    gw = c["grid_w"]
    if rel:
        path = "row32" if gw == 32 else ("rowseg" if gw >= 32 and gw % 8 == 0 else "generic")
    elif c["dense"]:
        path = "dfast" if dense_ld(c) % 4 == 0 else "dslow"
    else:
        path = "plain"
    r = path + ("/pos" if c["pos"] else "/nopos")
    if c["dense"]:
        return r
    return r + ("/dkv8" if dkv8(c) else "/dkv4")


def dkv8(c):
    if not c["gh"]:
        return False
    n2d = (2 * c["gh"] - 1) * (2 * c["gw"] - 1)
    n2dp, n1dp, Pp = (n2d + 3) & ~3, (2 * c["Lt"] - 1 + 3) & ~3, (c["P"] + 3) & ~3
    rowseg = c["grid_w"] != 32 and c["grid_w"] >= 32 and c["grid_w"] % 8 == 0

    def lds(nw):
        return KT_BYTES + VT_BYTES + 512 + (nw // 2) * VT_BYTES + (2 * n2dp + nw * n1dp + 2 * nw) * 4 + Pp * 4 + (2 * nw * (4 + 3 * 64) * 4 if rowseg else 0)
    return lds(4) > 80 * 1024 and lds(8) <= 160 * 1024


def dense_ld(c):
    return (c["S"] + 3) // 4 * 4 if c["dense"] == "ld4" else (c["S"] if c["S"] % 4 else c["S"] + 1)


def gains(H):
    return np.array([GAINS[h % 4] for h in range(H)], dtype=np.float64)


def kv_lens(c):
    return np.array(c["kv_len"] if c["kv_len"] else [c["S"]] * c["B"], dtype=np.int64)


def allowed(c, dense_bias=None):
    """[B, H, T, S] bool: the keys a row may see"""
    B, H, T, S = c["B"], c["H"], c["T"], c["S"]
    a = np.ones((B, H, T, S), dtype=bool)
    if c["causal"]:
        a &= ~causal_mask(T, S, c["P"])[None, None]
    a &= (np.arange(S)[None, :] < kv_lens(c)[:, None])[:, None, None, :]
    if dense_bias is not None:
        a &= np.isfinite(dense_bias)[None]
    return a


# ------------------------------------------------------------------------------------------------ operands
def _code(idx):
    """[..., 64] +-1 sign code of an index (0 in the four last columns)"""
    idx = np.asarray(idx, dtype=np.int64)
    bits = ((idx[..., None] >> np.arange(NBITS)) & 1) * 2 - 1
    out = np.zeros(idx.shape + (64,), dtype=np.float64)
    out[..., :NBITS * DPB] = np.repeat(bits, DPB, axis=-1)
    return out


def _vcode(B, S, H):
    """v[b, j, h, :]: small integers that identify (b, j, h): +-1 bits of j in columns 0..54, b and h in the rest"""
    v = np.zeros((B, S, H, 64))
    v[..., :55] = _code(np.arange(S))[None, :, None, :55]
    b, h, d = np.arange(B)[:, None, None, None], np.arange(H)[None, None, :, None], np.arange(55, 64)[None, None, None, :]
    v[..., 55:] = (b * 3 + h * 2 + d) % 5 - 2
    return v


def _bias_tables(c, rng, poison):
    """integer rel-pos tables of a grid case; with `poison` the entries only causal-masked pairs reach hold POISON_REL"""
    if not c["gh"]:
        return None
    H, Lt = c["H"], c["Lt"]
    gcode, code_bias, n2d = grid_codes(c["gh"], c["gw"])
    rel2d = rng.integers(-8, 9, (H, n2d)).astype(np.float64)
    rel1d = rng.integers(-8, 9, (H, 2 * Lt - 1)).astype(np.float64)
    relx = rng.integers(-8, 9, (H, 2)).astype(np.float64)
    if poison and c["causal"]:
        rel2d[:, :code_bias] = POISON_REL          # code_i - code_j < 0  <=>  j after i in raster order
        relx[:, 1] = POISON_REL                    # tail query x grid key
    return dict(gcode=gcode, code_bias=code_bias, n2d=n2d, rel2d=rel2d, rel1d=rel1d, relx=relx)


def dense_rel(c, tabs):
    """[H, T, S] bias of the tables (the construction of test_kernels_gpu._dense_rel)"""
    H, T, S, P, Lt = c["H"], c["T"], c["S"], c["P"], c["Lt"]
    bias = np.zeros((H, T, S))
    gc = tabs["gcode"].astype(np.int64)
    bias[:, :P, :P] = tabs["rel2d"][:, gc[:, None] - gc[None, :] + tabs["code_bias"]]
    t = np.arange(Lt)
    bias[:, P:, P:] = tabs["rel1d"][:, t[:, None] - t[None, :] + Lt - 1]
    bias[:, :P, P:] = tabs["relx"][:, 0][:, None, None]
    bias[:, P:, :P] = tabs["relx"][:, 1][:, None, None]
    return bias


def _sel(al, per_batch):
    """sel[b, h, t]: consecutive rows hit different 64-key tiles (stride 67) and other 32-blocks; every fifth row the last allowed
    key, every fifth + 1 the first (key 0 where it is allowed)"""
    B, H, T, S = al.shape
    sel = np.zeros((B, H, T), dtype=np.int64)
    for b in range(B):
        for h in range(H):
            for t in range(T):
                ok = np.flatnonzero(al[b, h, t])
                n = len(ok)
                assert n > 0, "fully masked row"
                r = n - 1 if t % 5 == 0 else (0 if t % 5 == 1 else (t * 67 + h * 31 + (b * 13 if per_batch else 0)) % n)
                sel[b, h, t] = ok[r]
    return sel


@functools.lru_cache(maxsize=4)
def _select_cached(cid, poison):
    c = by_id(cid)
    B, H, T, S = c["B"], c["H"], c["T"], c["S"]
    rng = np.random.default_rng(sum(map(ord, cid)))
    tabs = _bias_tables(c, rng, poison)
    dense = None
    if c["dense"]:
        dense = rng.integers(-8, 9, (H, T, S)).astype(np.float64)
        hide = rng.random((H, T, S)) < 0.3
        hide[:, :, 0] &= rng.random((H, T)) < 0.5
        hide[np.arange(H)[:, None], np.arange(T)[None, :], rng.integers(0, S, (H, T))] = False      # every row keeps a key
        dense[hide] = -np.inf
    bi_bias = rng.integers(-8, 9, (H, T, S)).astype(np.float64) if c["entry"] == "bi" else None
    al = allowed(c, dense)
    sel = _sel(al, per_batch=not c["pos"])
    kcode, qcode = _code(np.arange(S)), _code(sel)                             # [S, 64], [B, H, T, 64]
    # pos carries the high half of the bits (sel does not depend on b then), q / k the low half
    lo = np.zeros(64); lo[:NBITS * DPB // 2 if c["pos"] else NBITS * DPB] = 1
    hi = np.zeros(64); hi[NBITS * DPB // 2:NBITS * DPB] = 1
    q = np.transpose(qcode * lo * CQ, (0, 2, 1, 3)).copy()                    # [B, T, H, 64]
    q[..., POISON_COL:] = CQ
    k = np.broadcast_to((kcode * lo * CK)[None, :, None, :], (B, S, H, 64)).copy()
    pq = pk = None
    if c["pos"]:
        pq = np.transpose(qcode[0] * hi * CQ, (1, 0, 2)).copy()               # [T, H, 64]
        pk = np.broadcast_to((kcode * hi * CK)[:, None, :], (S, H, 64)).copy()
    v = _vcode(B, S, H)
    if poison:
        dead = np.arange(S)[None, :] >= kv_lens(c)[:, None]                    # [B, S]
        k[dead] = 0
        k[dead, :, POISON_COL:] = POISON_K
        v[dead] = V_POISON
    dout = rng.integers(-3, 4, (B, T, H, 64)).astype(np.float64)
    return dict(q=q, k=k, v=v, pq=pq, pk=pk, dout=dout, tabs=tabs, dense=dense, bi_bias=bi_bias, sel=sel, allowed=al, gain=gains(H))


def by_id(cid):
    for c in FWD_CASES + BI_CASES + RANDOM_CASES:
        if c["id"] == cid:
            return c
    raise KeyError(cid)


def select_inputs(c, poison=True):
    """operands of the select / poison regime (shared, read-only): q, k, v, dout [B, T|S, H, 64], pq / pk [T|S, H, 64]"""
    return _select_cached(c["id"], poison)


def select_expect(c, d, keep=None):
    """out, dv, dgain_rows, lse of the select regime.  keep: uint8 [B, H, T, S] of ifseg_attn_dropout_mask (p = 0.5) or None"""
    B, H, T, S = c["B"], c["H"], c["T"], c["S"]
    sel, g = d["sel"], d["gain"]
    bb, hh = np.arange(B)[:, None, None], np.arange(H)[None, :, None]
    ks = np.ones((B, H, T))
    if keep is not None:
        ks = 2.0 * keep[bb, hh, np.arange(T)[None, None, :], sel]
    vs = d["v"][bb, sel, hh]                                                     # [B, H, T, 64] = v[b, sel, h]
    out = np.transpose(g[None, :, None, None] * ks[..., None] * vs, (0, 2, 1, 3))
    do = np.transpose(d["dout"], (0, 2, 1, 3))                                   # [B, H, T, 64]
    dv = np.zeros((B, H, S, 64))
    w = g[None, :, None, None] * ks[..., None] * do
    for b in range(B):
        for h in range(H):
            np.add.at(dv[b, h], sel[b, h], w[b, h])
    dgr = ks * (do * vs).sum(-1)
    score = scores(c, d)[bb, hh, np.arange(T)[None, None, :], sel]
    return dict(out=out, dv=np.transpose(dv, (0, 2, 1, 3)), dgain_rows=dgr, lse=score * LOG2E)


def bias_of(c, d):
    """[H, T, S] fp64 bias of a case's operands (tables, dense fp32 bias or the batch-inner operand) or None"""
    if d.get("tabs") is not None:
        return dense_rel(c, d["tabs"])
    if d.get("dense") is not None:
        return d["dense"]
    return d.get("bi_bias")


def scores(c, d):
    """[B, H, T, S] fp64 scores in natural units, -inf where hidden"""
    s = np.einsum("bthd,bshd->bhts", d["q"], d["k"])
    if d.get("pq") is not None:
        s = s + np.einsum("thd,shd->hts", d["pq"], d["pk"])[None]
    b = bias_of(c, d)
    if b is not None:
        s = s + b[None]
    return np.where(d["allowed"], s, -np.inf)


def select_gap_log2(c, d):
    """per row: (winner - best other allowed key) in log2 units, and whether sel is the argmax"""
    s = scores(c, d)
    order = np.sort(s, axis=-1)
    top = order[..., -1]
    second = order[..., -2] if s.shape[-1] > 1 else np.full(top.shape, -np.inf)
    return (top - second) * LOG2E, s.argmax(-1)


# ------------------------------------------------------------------------------------------------ uniform regime
def uniform_inputs(c):
    B, H, T, S = c["B"], c["H"], c["T"], c["S"]
    v = np.zeros((B, S, H, 64))
    v[:] = np.repeat(((np.arange(S)[:, None] >> np.arange(8)) & 1) * 2 - 1, 8, axis=-1)[None, :, None, :]
    v *= np.where((np.arange(B)[:, None, None, None] + np.arange(H)[None, None, :, None]) % 2 == 0, 1.0, -1.0)
    t, h, dd = np.arange(T)[None, :, None, None], np.arange(H)[None, None, :, None], np.arange(64)[None, None, None, :]
    dout = ((t * 3 + h + dd + np.arange(B)[:, None, None, None]) % 4 + 1).astype(np.float64)
    dense = None
    if c["dense"]:
        rng = np.random.default_rng(5)
        dense = np.zeros((H, T, S))
        hide = rng.random((H, T, S)) < 0.3
        hide[np.arange(H)[:, None], np.arange(T)[None, :], rng.integers(0, S, (H, T))] = False
        dense[hide] = -np.inf
    return dict(v=v, dout=dout, dense=dense, allowed=allowed(c, dense), gain=np.where(gains(H) == 0, 1.0, gains(H)))


def uniform_expect(c, d, al=None):
    """out [B, T, H, 64], dv [B, S, H, 64] and the bound 2^-8 |ref| (1 + 2^-12) of each"""
    al = d["allowed"] if al is None else al
    n = al.sum(-1).astype(np.float64)                                            # [B, H, T]
    g = d["gain"][None, :, None, None]
    out = np.transpose(g * np.einsum("bhts,bshd->bhtd", al.astype(np.float64), d["v"]) / n[..., None], (0, 2, 1, 3))   # integer sums: exact
    dv = np.transpose(g * np.einsum("bhts,bthd->bhsd", al / n[..., None], d["dout"]), (0, 2, 1, 3))
    # dv: p_t = 1 / n_t is rounded to bf16 (u relative) unless n_t is a power of two; dout > 0: no cancellation
    odd = al * (n != 2.0 ** np.round(np.log2(n)))[..., None] / n[..., None]
    dv_p = np.transpose(np.abs(g) * np.einsum("bhts,bthd->bhsd", odd, d["dout"]), (0, 2, 1, 3))
    return dict(out=out, dv=dv, out_b=uniform_bound(out), dv_b=uniform_bound(dv) + U * dv_p)


def uniform_bound(ref):
    return (U + 2.0 ** -20) * np.abs(ref)


# ------------------------------------------------------------------------------------------------ random regime (part B)
def _randn(shape, seed, scale=1.0):
    """the values of test_kernels_gpu._rand, rounded to bf16"""
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(torch.bfloat16).double().numpy()


@functools.lru_cache(maxsize=2)
def _random_cached(cid):
    import torch
    c = by_id(cid)
    B, H, T, S = c["B"], c["H"], c["T"], c["S"]
    C = H * 64
    q, k, v = _randn((B, T, C), 20, 0.35), _randn((B, S, C), 21), _randn((B, S, C), 22)
    dout = _randn((B, T, C), 25)
    d = dict(q=q.reshape(B, T, H, 64), k=k.reshape(B, S, H, 64), v=v.reshape(B, S, H, 64), dout=dout.reshape(B, T, H, 64), pq=None, pk=None)
    if c["pos"]:
        d["pq"], d["pk"] = _randn((T, C), 23, 0.35).reshape(T, H, 64), _randn((S, C), 24).reshape(S, H, 64)
    g = torch.Generator().manual_seed(30)
    d["tabs"] = d["dense"] = d["bi_bias"] = None
    if c["gh"]:
        gcode, code_bias, n2d = grid_codes(c["gh"], c["gw"])
        r2, r1, rx = torch.randn(H, n2d, generator=g), torch.randn(H, 2 * c["Lt"] - 1, generator=g), torch.randn(H, 2, generator=g)
        d["tabs"] = dict(gcode=gcode, code_bias=code_bias, n2d=n2d, rel2d=r2.double().numpy(), rel1d=r1.double().numpy(), relx=rx.double().numpy())
    elif c["dense"] or c["entry"] == "bi":
        bias = torch.randn(H, T, S, generator=g)
        if c["dense"]:
            bias[:, :, 1:][torch.rand(H, T, S - 1, generator=g) < 0.3] = float("-inf")
            d["dense"] = bias.double().numpy()
        else:
            d["bi_bias"] = bias.to(torch.bfloat16).double().numpy()            # the bias as stored in dense.D
    gain = (1.0 + 0.2 * torch.randn(H, generator=torch.Generator().manual_seed(5))).double().numpy()
    gain[0] = 0.0
    gain[H - 1] = -0.7 if H > 1 else gain[H - 1]
    d["gain"] = gain.astype(np.float32).astype(np.float64)
    d["allowed"] = allowed(c, d["dense"])
    return d


def random_inputs(c):
    return _random_cached(c["id"])


def score_err(c, d):
    """es [B, H, T]: the bound on the fp32 error of a score of the row (see the module docstring)"""
    D = 130 if d["pq"] is not None else 66
    m = np.einsum("bthd,bshd->bhts", np.abs(d["q"]), np.abs(d["k"]))
    if d["pq"] is not None:
        m = m + np.einsum("thd,shd->hts", np.abs(d["pq"]), np.abs(d["pk"]))[None]
    b = bias_of(c, d)
    bmax = 0.0 if b is None else np.abs(np.where(np.isfinite(b), b, 0)).max()
    return D * 2.0 ** -24 * m.max(-1) + 2.0 ** -23 * bmax


def forward_ref(c, d, ks=None):
    """fp64 forward: out [B, T, H, 64], lse [B, H, T] (log2 units), p [B, H, T, S] and the part B bound of out.
    ks: keep / (1 - p) [B, H, T, S] or None"""
    s = scores(c, d)
    m = s.max(-1, keepdims=True)
    e = np.exp(s - m)
    l = e.sum(-1, keepdims=True)
    p = e / l
    lse = (m[..., 0] + np.log(l[..., 0])) * LOG2E
    pk_ = p if ks is None else p * ks
    g = d["gain"][None, :, None, None]
    out = g * np.einsum("bhts,bshd->bhtd", pk_, d["v"])
    mag = np.abs(g) * np.einsum("bhts,bshd->bhtd", pk_, np.abs(d["v"]))
    el = 2 * score_err(c, d)[..., None] + 2.0 ** -20
    bound = U * np.abs(out) + (2 * U + el) * mag + 1e-30
    tr = lambda x: np.transpose(x, (0, 2, 1, 3))
    return dict(out=tr(out), out_b=tr(bound), lse=lse, p=p)


def backward_ref(c, d, out_used, lse_used, ks=None, dq_scale=1.0):
    """fp64 backward from the kernel's own bf16 `out` [B, T, H, 64] and `lse` [B, H, T]: dq, dk, dv (layout of the operands),
    dbias [H, T, S] (sum over the batch), dS, dgain_rows, delta and the part B bounds `<name>_b`"""
    tr = lambda x: np.transpose(x, (0, 2, 1, 3))
    g = d["gain"][None, :, None, None]
    s = scores(c, d)
    p = np.where(np.isfinite(s), np.exp2(s * LOG2E - lse_used[..., None]), 0.0)
    kk = np.ones_like(p) if ks is None else ks
    do, vv, qq, kx = tr(d["dout"]), tr(d["v"]), tr(d["q"]), tr(d["k"])           # [B, H, T|S, 64]
    delta = (do * tr(out_used)).sum(-1)                                           # [B, H, T]
    dpraw = np.einsum("bhtd,bhsd->bhts", do, vv)
    dpmag = np.einsum("bhtd,bhsd->bhts", np.abs(do), np.abs(vv))
    dP = g * dpraw * kk
    dS = p * (dP - delta[..., None])
    el = 2 * score_err(c, d)[..., None] + 2.0 ** -20
    e_dS = p * kk * np.abs(g) * dpmag * 66 * 2.0 ** -24 + p * 2.0 ** -23 * (np.abs(dP) + np.abs(delta[..., None])) + el * np.abs(dS)
    w = U * np.abs(dS) + e_dS                                                     # the dQ kernels: dq, dbias, dpos_q
    wk = w + U * p * kk * np.abs(g) * dpmag                                       # the dK/dV kernels: dk, dpos_k (u_g, see above)
    r = dict(delta=delta, dS=dS, p=p)
    r["dv"] = tr(g * np.einsum("bhts,bhtd->bhsd", p * kk, do))
    r["dv_b"] = tr(U * np.abs(tr(r["dv"])) + (U + el.max()) * np.abs(g) * np.einsum("bhts,bhtd->bhsd", p * kk, np.abs(do))) + 1e-30
    r["dq"] = tr(dq_scale * np.einsum("bhts,bhsd->bhtd", dS, kx))
    r["dq_b"] = tr(U * np.abs(tr(r["dq"])) + abs(dq_scale) * np.einsum("bhts,bhsd->bhtd", w, np.abs(kx))) + 1e-30
    r["dk"] = tr(np.einsum("bhts,bhtd->bhsd", dS, qq))
    r["dk_b"] = tr(U * np.abs(tr(r["dk"])) + np.einsum("bhts,bhtd->bhsd", wk, np.abs(qq))) + 1e-30
    r["dbias"] = dS.sum(0)
    r["dgain_rows"] = (p * kk * dpraw).sum(-1)
    r["dgain_rows_b"] = (el[..., 0] + (66 + s.shape[-1]) * 2.0 ** -24) * (p * kk * dpmag).sum(-1) + 1e-30   # + the fma chain over the keys
    r["w"], r["wk"] = w, wk
    if d["pq"] is not None:
        r["dpq"] = np.einsum("bhts,shd->bthd", dS, d["pk"])                      # per batch element, before dpq_scale
        r["dpq_b"] = np.einsum("bhts,shd->bthd", w, np.abs(d["pk"]))
        r["dpk"] = np.einsum("bhts,thd->bshd", dS, d["pq"])
        r["dpk_b"] = np.einsum("bhts,thd->bshd", wk, np.abs(d["pq"]))
    return r


def table_grads(c, tabs, dSb):
    """d rel2d [H, n2d], d rel1d [H, 2 Lt - 1], d relx [H, 2] of dSb [H, T, S] (index_add over the construction of dense_rel)"""
    H, P, Lt = c["H"], c["P"], c["Lt"]
    gc = tabs["gcode"].astype(np.int64)
    g2, g1 = np.zeros((H, tabs["n2d"])), np.zeros((H, 2 * Lt - 1))
    idx = (gc[:, None] - gc[None, :] + tabs["code_bias"]).reshape(-1)
    t = np.arange(Lt)
    i1 = (t[:, None] - t[None, :] + Lt - 1).reshape(-1)
    for h in range(H):
        np.add.at(g2[h], idx, dSb[h, :P, :P].reshape(-1))
        np.add.at(g1[h], i1, dSb[h, P:, P:].reshape(-1))
    gx = np.stack([dSb[:, :P, P:].sum((1, 2)), dSb[:, P:, :P].sum((1, 2))], 1)
    return g2, g1, gx


def worst_ratio(got, ref, bound):
    r = np.abs(got - ref) / bound
    at = np.unravel_index(int(np.argmax(r)), r.shape)
    return float(r[at]), tuple(int(i) for i in at)


# ------------------------------------------------------------------------------------------------ emulation (CPU file)
def emulate_forward(c, d, ks=None):
    """the forward with the kernels' formats: fp32 scores, fp32 exp2 and normaliser, P rounded to bf16 for P V, fp32 sums, one
    rounding of the result"""
    f = np.float32
    s = np.einsum("bthd,bshd->bhts", d["q"].astype(f), d["k"].astype(f))
    if d["pq"] is not None:
        s = s + np.einsum("thd,shd->hts", d["pq"].astype(f), d["pk"].astype(f))[None]
    b = bias_of(c, d)
    if b is not None:
        s = s + b.astype(f)[None]
    s = np.where(d["allowed"], s, f(-np.inf)).astype(f)
    m = (s.max(-1, keepdims=True) * f(LOG2E)).astype(f)
    p = np.exp2((s * f(LOG2E) - m).astype(f)).astype(f)
    l = p.sum(-1, keepdims=True, dtype=f)
    pb = bf16_round(p if ks is None else (p * ks.astype(f)).astype(f))
    o = np.einsum("bhts,bshd->bhtd", pb, d["v"].astype(f)).astype(f)
    o = o * (d["gain"].astype(f)[None, :, None, None] / l).astype(f)
    lse = (m[..., 0] + np.log2(l[..., 0])).astype(f)
    return np.transpose(bf16_round(o), (0, 2, 1, 3)).astype(np.float64), lse.astype(np.float64)


def emulate_backward(c, d, out_used, lse_used, ks=None, dq_scale=1.0, dpq_scale=1.0):
    """the backward with the kernels' formats: fp32 p = exp2(s log2 e - lse), P and dS rounded to bf16 for the MFMAs, fp32 sums,
    one rounding of each result.  dS exists in two flavours: the dQ kernels apply the gain in fp32 (dq, dpos_q, dbias,
    dgain_rows), the dK/dV kernels hold -gain v in bf16 (dk, dpos_k, the table partials).  dbias: the fp32 dS of a group of four
    batch elements summed in fp32, one bf16 store per slab; the table bins: see emulate_table_bins"""
    f = np.float32
    tr = lambda x: np.transpose(x, (0, 2, 1, 3))
    s = np.einsum("bthd,bshd->bhts", d["q"].astype(f), d["k"].astype(f))
    if d["pq"] is not None:
        s = s + np.einsum("thd,shd->hts", d["pq"].astype(f), d["pk"].astype(f))[None]
    b = bias_of(c, d)
    if b is not None:
        s = s + b.astype(f)[None]
    with np.errstate(over="ignore"):                                              # poisoned keys overflow before the mask drops them
        p = np.where(d["allowed"], np.exp2((s * f(LOG2E)).astype(f) - lse_used.astype(f)[..., None]), f(0)).astype(f)
    kk = np.ones_like(p) if ks is None else ks.astype(f)
    g = d["gain"].astype(f)[None, :, None, None]
    do, vv = tr(d["dout"]).astype(f), tr(d["v"]).astype(f)
    delta = (do.astype(np.float64) * tr(out_used)).sum(-1).astype(f)
    dpe = (np.einsum("bhtd,bhsd->bhts", do, vv).astype(f) * kk).astype(f)        # dP before the gain
    dSq32 = (p * (g * dpe - delta[..., None])).astype(f)                          # the dQ kernels: the gain in fp32
    dpk_ = np.einsum("bhtd,bhsd->bhts", do, bf16_round(vv * g)).astype(f)         # the dK/dV kernels: -gain v in bf16
    dSk32 = (p * (dpk_ * kk - delta[..., None])).astype(f)
    dSq, dSk, pb = bf16_round(dSq32), bf16_round(dSk32), bf16_round(p * kk)
    r = dict(dv=tr(bf16_round(g * np.einsum("bhts,bhtd->bhsd", pb, do).astype(f))),
             dq=tr(bf16_round(f(dq_scale) * np.einsum("bhts,bhsd->bhtd", dSq, tr(d["k"]).astype(f)).astype(f))),
             dk=tr(bf16_round(np.einsum("bhts,bhtd->bhsd", dSk, tr(d["q"]).astype(f)).astype(f))))
    B = p.shape[0]
    r["dbias"] = np.stack([bf16_round(dSq32[4 * gi:4 * gi + 4].sum(0, dtype=f)) for gi in range((B + 3) // 4)])
    r["dgain_rows"] = np.cumsum((p * dpe).astype(f), axis=-1, dtype=f)[..., -1]     # a sequential fp32 chain over the keys
    if d["pq"] is not None:
        r["dpq"] = bf16_round(f(dpq_scale) * np.einsum("bhts,shd->bthd", dSq, d["pk"].astype(f)).astype(f))
        r["dpk"] = bf16_round(np.einsum("bhts,thd->bshd", dSk, d["pq"].astype(f)).astype(f))
    out = {k_: v_.astype(np.float64) for k_, v_ in r.items()}
    out["dSk32"] = dSk32
    return out


def emulate_table_bins(c, tabs, dS32):
    """d rel2d [H, n2d], d rel1d, d relx from the fp32 dS of the dK/dV kernel [B, H, T, S], binned in fp32 with the structure of
    attn_bwd_dkv_body.  generic grids: every term is added to its bin.  row32 / rowseg: per (32-query block, 32-key block,
    diagonal u = (key - query) mod 32 inside the blocks) the kernel forms the class sums T (all), W (wrapped: key position
    below query position), K (key in the block's second grid row), WK per query set (query in the block's first / second grid
    row) and takes the bins as DIFFERENCES of them (nw / wr of the kernel; on 32-wide grids the no-wrap sum A and T - A).
    The summation order inside a class is numpy's, not the kernel's: any order is a legitimate fp32 evaluation.  That every
    output of a group lands in ONE bin is asserted (it is what makes the restatement meaningful)."""
    f = np.float32
    B, H, P, gw = c["B"], c["H"], c["P"], c["gw"]
    path = reach(c).split("/")[0]
    gc = tabs["gcode"].astype(np.int64)
    binidx = gc[:, None] - gc[None, :] + tabs["code_bias"]
    g2 = np.zeros((H, tabs["n2d"]), dtype=f)
    dS32 = dS32.astype(f)
    if path == "generic":
        for b in range(B):
            for h in range(H):
                np.add.at(g2[h], binidx.ravel(), dS32[b, h, :P, :P].ravel())
    else:
        i, j = np.arange(P)[:, None], np.arange(P)[None, :]
        qb, kb, qp, kp = i // 32, j // 32, i % 32, j % 32
        nkb = P // 32
        grp = np.broadcast_to((qb * nkb + kb) * 32 + (kp - qp) % 32, (P, P))
        G = nkb * nkb * 32
        W = np.broadcast_to(kp < qp, (P, P))
        s2 = np.broadcast_to(i // gw != (32 * qb) // gw, (P, P))
        K2 = np.broadcast_to(j // gw != (32 * kb) // gw, (P, P))
        slot = grp * 6 + (s2.astype(np.int64) - K2 + 1) * 2 + W
        slotbin = np.full(G * 6, -1, dtype=np.int64)
        slotbin[slot.ravel()] = binidx.ravel()
        assert (slotbin[slot] == binidx).all(), "a class-sum output of the restatement feeds more than one bin"
        live = slotbin >= 0
        for b in range(B):
            for h in range(H):
                x = dS32[b, h, :P, :P]
                cls = np.zeros((2, 4, G), dtype=f)
                for st in (0, 1):
                    m0 = s2 == bool(st)
                    for k_, m in enumerate((m0, m0 & W, m0 & K2, m0 & W & K2)):
                        np.add.at(cls[st, k_], grp[m], x[m])
                c0, c1 = cls
                if path == "row32":
                    a_ = np.zeros(G, dtype=f)
                    np.add.at(a_, grp[~W], x[~W])
                    z = np.zeros(G, dtype=f)
                    nw, wr = [z, a_, z], [z, (c0[0] - a_).astype(f), z]
                else:
                    nw = [c0[2] - c0[3], (c0[0] - c0[1] - c0[2] + c0[3]) + (c1[2] - c1[3]), c1[0] - c1[1] - c1[2] + c1[3]]
                    wr = [c0[3], (c0[1] - c0[3]) + c1[3], c1[1] - c1[3]]
                vals = np.stack([nw[0], wr[0], nw[1], wr[1], nw[2], wr[2]], axis=1).astype(f).ravel()       # slot order
                np.add.at(g2[h], slotbin[live], vals[live])
    rest = dS32.sum(0, dtype=f).astype(np.float64)
    rest[:, :P, :P] = 0
    _, g1, gx = table_grads(c, tabs, rest)
    return g2.astype(np.float64), g1, gx


def table_refs_and_bounds(c, tabs, b):
    """references and bounds of the three fp32 table partials summed over the parts, from backward_ref's result.  The dK/dV
    kernel bins its fp32 dS (not rounded to bf16): e_dS with u_g, plus 2^-18 of the bin's own |dS| for the fp32 sums over
    blocks, workgroups and parts.  On row32 / rowseg grids (NOT on generic ones, and not for d rel1d / d relx) the grid x grid
    bins of a 32-query block are differences of class sums (emulate_table_bins), so a bin also carries the rounding of the
    other bins of its group: worst case nw[1] of `rowseg`, six class sums of up to 16 terms (15 u each) and five combining
    operations on up to four times the magnitude, 60 u + 20 u, the half swap and the exchange area on top -> 96 * 2^-24 times
    sum_{i in block} |dS_ij| per (block, key) pair that feeds the bin."""
    H, P, S = c["H"], c["P"], c["S"]
    e_dS = (b["wk"] - U * np.abs(b["dS"])).sum(0)
    mag = np.abs(b["dS"]).sum(0)
    refs = table_grads(c, tabs, b["dS"].sum(0))
    errs = list(table_grads(c, tabs, e_dS + 2.0 ** -18 * mag))
    if reach(c).split("/")[0] in ("row32", "rowseg"):
        blk = mag[:, :P].reshape(H, P // 32, 32, S).sum(2, keepdims=True)
        mexp = np.zeros_like(mag)
        mexp[:, :P, :P] = np.broadcast_to(blk, (H, P // 32, 32, S)).reshape(H, P, S)[:, :, :P]
        errs[0] = errs[0] + table_grads(c, tabs, 96 * 2.0 ** -24 * mexp)[0]
    return refs, [e + 1e-30 for e in errs]


def lse_bound(c, d, ref_lse):
    """|lse - ref| in log2 units: the score error es and the relative error el of the normaliser (both times log2 e), the
    v_log_f32 result (2^-20 covers 1 ulp of log2 l <= 2^11) and four fp32 ulps of the stored value"""
    es = score_err(c, d)
    return (es + 2 * es + 2.0 ** -20) * LOG2E + 2.0 ** -20 + 4 * np.spacing(np.abs(ref_lse).astype(np.float32)).astype(np.float64)
