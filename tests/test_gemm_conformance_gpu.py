"""Conformance of the GEMM family of csrc/gemm.hip through the C ABI (ifseg_amd.hip): ifseg_gemm_bf16 in its three layouts,
split-K + ifseg_reduce_parts(_multi), ifseg_gemm_tn_group, ifseg_gemm_nn_rowdot, ifseg_gemm_nn_gelu_ln_bwd, ifseg_conv2d_nhwc_bf16.

Part A (exact): operands are small integers ({-1, 0, 1}; bias in [-2, 2], residual and previous C in [-4, 4], alpha 0.5 / 2).
bf16 x bf16 products summed in fp32 are then exact in every summation order, tile shape, split and pipeline, so each output
element has ONE correct value and the assertion is equality with an fp64 reference, per element.  Before a kernel is compared
the reference alone is checked: every expected value is representable in the output type and (K >= 64) less than 10 % of the
product is zero.  The unmarked ``test_inputs_*`` tests run those checks without a GPU.  A, B, resid and C are views into larger
allocations: surroundings of the operands hold 7, surroundings of C a sentinel that must be bit-identical after the call.

Part B (random values, ``_rand`` data of test_kernels_gpu.py): per element
    |out - ref| <= u_out |ref| (1 + 2^-6) + (K + 4 [+ slices]) 2^-23 mag,   mag = (|A|.|B| + |bias|) |alpha| + |resid| (+ |C_old|)
with u_out = 2^-9 for bf16 outputs and 0 for fp32 outputs: one round-to-nearest of the result plus the textbook bound of K
fp32 additions in any order; nothing in it is measured.  That is the bound this suite was specified with.  Its first term
is too small for bf16: bfloat16 has 8 significant bits, its unit roundoff is 2^-8, and a correctly rounded result may be off
by 2^-8 |ref|.  On MI355X 15 bf16-output cases exceeded it by 1.46x - 1.94x (the limit for a correct kernel is
2 / (1 + 2^-6) = 1.97x), each at an element just above a power of two that holds the correctly rounded value.  As the
specification prescribes for a bound that is itself wrong, only the accumulation term is widened, per case, by the
smallest power of two that holds, with the observation beside it (search PART_B_WIDEN).  Because such a factor says nothing
about the accumulation, every case ALSO asserts the bound with u_out = 2^-8 and the accumulation term unwidened (worst
ratio of any case 0.98; every fp32-output case stays below 0.02 of the unwidened bound).

ifseg_gemm_nn_gelu_ln_bwd has its own bound (see test_gemm_nn_gelu_ln_bwd): worst ratio 0.98 in both stage variants.

Every table row names the kernel instantiation it is meant to reach ("NT64/2" = gemm_kernel<A_KC, false, 64, 64, 2>, ...); the
dispatch rule of gemm_impl is restated in ``_nt_reach`` / ``_reach`` and every row is checked against it, so the tables cannot
drift from the shapes.  profiles/gemm_conformance_kernels.txt lists the kernels of gemm.hip seen in a kernel trace of this
file alone, with call counts, the part B figures case by case, and the table of deliberately wrong variants of gemm.hip that
this file catches.
"""
import ctypes
import functools
import math

import pytest
import torch

gpu = pytest.mark.gpu

NT, NN, TN = 0, 1, 2
RELU, OUT_F32, ACCUMULATE, COLSUM = 1, 2, 4, 8
BAD_SHAPE, BAD_ARG = -2, -3
GUARD = 7.0            # around A, B, resid, dot, u: a kernel that reads past a row or a matrix picks up 7s
SENTINEL = -12352.0    # around C (bf16- and fp32-representable); compared bit for bit after the call
BF16, F32 = torch.bfloat16, torch.float32
L_NAME = {NT: "NT", NN: "NN", TN: "TN"}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


CPU = torch.device("cpu")


# ------------------------------------------------------------------------------------------------ data
# (the draws are cached: rows of the tables that share a shape share their operands; nothing writes into a draw)
@functools.lru_cache(maxsize=8)
def _tern(shape, seed, p):
    g = torch.Generator(device="cpu").manual_seed(seed)
    t = torch.randint(-1, 2, shape, generator=g, dtype=torch.int8)
    return t if p >= 1.0 else t * (torch.rand(shape, generator=g) < p)


@functools.lru_cache(maxsize=8)
def _ints(shape, seed, lim):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(-lim, lim + 1, shape, generator=g, dtype=torch.int8)


@functools.lru_cache(maxsize=8)
def _randn(shape, seed, scale=1.0):
    """the values of test_kernels_gpu._rand (rounded to bf16 by the caller)"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def _p_for(red):
    """density of the ternary operands by reduction length: 0.5, 0.25 above 4096 (integers stay below 256); dense below 328,
    where a sparser draw would leave more than 10 % of the products zero"""
    return 0.25 if red > 4096 else (1.0 if red < 328 else 0.5)


def _zero_limit(red):
    # K = 8: no ternary draw gets below 10 % zeros (even dense +-1 operands give C(8,4)/2^8 = 27 %); the dense draw used
    # here gives 20-24 %, so the guard against "a kernel that writes zeros passes" is 30 % there
    return 0.30 if red < 64 else 0.10


def _guarded(vals, dtype, dev, pad, fill, rows=(3, 2)):
    """vals [b, R, C] -> (full [b, 3 + R + 2, C + pad] filled with `fill`, view of the logical matrix inside it); a shape
    instead of values leaves the matrix filled as well.  The allocation is put together on `dev` (the draw travels as it is)"""
    b, R, C = vals if isinstance(vals, tuple) else vals.shape
    full = torch.full((b, rows[0] + R + rows[1], C + pad), fill, dtype=dtype, device=dev)
    view = full[:, rows[0]:rows[0] + R, :C]
    if not isinstance(vals, tuple):
        view.copy_(vals.to(dev))
    return full, view


def _flat_guarded(vals, dtype, dev, fill, pad=16):
    """dense tensor (or, given a shape, a filled one) with `pad` guard elements before and after it in one allocation"""
    shape = vals if isinstance(vals, tuple) else tuple(vals.shape)
    n = math.prod(shape)
    full = torch.full((n + 2 * pad,), fill, dtype=dtype, device=dev)
    view = full[pad:pad + n].view(shape)
    if not isinstance(vals, tuple):
        view.copy_(vals.to(dev))
    return full, view


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def _assert_surroundings(full_after, full_before, inner, what):
    """everything of the allocation outside `inner` (a function full -> view of the logical output) is bit-identical"""
    chk = full_after.clone()
    inner(chk).copy_(inner(full_before))
    assert torch.equal(_bits(chk), _bits(full_before)), "%s: wrote outside its output (guard band changed)" % what


def _assert_valid_reference(ref, prod, out_dtype, red, what):
    """the two conditions on the inputs, on the reference alone"""
    assert bool((ref.to(out_dtype).double() == ref).all()), "%s: an expected value is not representable in %s (max |ref| %g)" % (
        what, out_dtype, ref.abs().max().item())
    zf = (prod == 0).double().mean().item()
    assert zf < _zero_limit(red), "%s: %.1f %% of the expected product is zero" % (what, 100 * zf)


def _assert_exact(got, ref, bn, what):
    g = got.double()
    bad = g != ref
    if bool(bad.any()):
        idx = bad.nonzero()[:6].tolist()
        rows = ["%s expected %g got %g (tile m %d n %d)" % (tuple(i), ref[tuple(i)].item(), g[tuple(i)].item(),
                                                            i[-2] // 128, i[-1] // bn) for i in idx]
        raise AssertionError("%s: %d of %d elements differ; first: %s" % (what, int(bad.sum()), bad.numel(), "; ".join(rows)))


def _assert_bound(got, ref, mag, terms, what, widen=0):
    """part B.  Two assertions per element: the bound as this suite was specified (u_out = 2^-9 for bf16), its accumulation
    term widened by 2^widen where the case's table row says so (the smallest power of two that holds, see PART_B_WIDEN), and
    the same bound with the unit roundoff bfloat16 has (2^-8) and the accumulation term as specified.  The message reports the
    worst |err| / bound of both and the factor the accumulation term of the first would need."""
    err = (got.double() - ref).abs()
    acc = terms * 2.0 ** -23 * mag

    def worst(u, factor):
        bound = (u if got.dtype == BF16 else 0.0) * ref.abs() * (1 + 2.0 ** -6) + factor * acc
        ratio = torch.nan_to_num(torch.where(err == 0, torch.zeros_like(err), err / bound), nan=float("inf"))
        k = int(ratio.argmax())
        return ratio.reshape(-1)[k].item(), k

    r, k = worst(2.0 ** -9, 2.0 ** widen)
    r8, _ = worst(2.0 ** -8, 1.0)
    over = err - (2.0 ** -9 if got.dtype == BF16 else 0.0) * ref.abs() * (1 + 2.0 ** -6)
    need = torch.nan_to_num(torch.where(over <= 0, torch.zeros_like(err), over / acc), nan=float("inf")).max().item()
    at, rest = [], k
    for d in reversed(ref.shape):
        at.insert(0, rest % d)
        rest //= d
    msg = ("%s: worst |err|/bound %.3f (accumulation term x 2^%d; it needs x %.4g) at %s (ref %g, got %g, mag %g, terms %d); "
           "with u_out = 2^-8 and the term as specified: %.3f" % (what, r, widen, need, at, ref.reshape(-1)[k].item(),
                                                                 got.double().reshape(-1)[k].item(), mag.reshape(-1)[k].item(), terms, r8))
    print("[part B]", msg)
    assert r <= 1.0 and r8 <= 1.0, msg


# ------------------------------------------------------------------------------------- dispatch, restated
def _ceil(a, b):
    return (a + b - 1) // b


def _nt_reach(M, N, batch=1):
    """gemm_impl / ifseg_conv2d_nhwc_bf16: 64-wide tiles for N <= 64 or fewer than 384 128-wide tiles; two LDS stages up to
    1024 workgroups"""
    rows, t128 = _ceil(M, 128), _ceil(M, 128) * _ceil(N, 128)
    narrow = N <= 64 or t128 < 384
    tiles = rows * _ceil(N, 64) if narrow else t128
    return "%d/%d" % (64 if narrow else 128, 2 if tiles * batch <= 1024 else 1)


def _reach(layout, M, N, batch=1, slices=1):
    if layout == NT:
        return "NT" + _nt_reach(M, N, batch)
    return "%s128/%d" % (L_NAME[layout], 2 if _ceil(M, 128) * _ceil(N, 128) * batch * slices <= 1024 else 1)


def _bn(reach):
    return 64 if "64/" in reach else 128


def _split_geometry(M, N, K, splitk):
    kchunk = _ceil(_ceil(K, splitk), 64) * 64
    nsl = _ceil(K, kchunk)
    tiles = _ceil(M, 128) * _ceil(N, 128)
    xcd = nsl > 1 and 8 % nsl == 0 and tiles % (8 // nsl) == 0
    return kchunk, nsl, xcd, (2 if tiles * nsl <= 1024 else 1)


# --------------------------------------------------------------------------------------------- case tables
def _case(layout, M, N, K, reach, data="int", **kw):
    c = dict(layout=layout, M=M, N=N, K=K, reach=reach, data=data, bias=False, alpha=1.0, ancols=-1, resid=False, relu=False,
             f32=False, acc=False, batch=1, cpad=8, widen=0)
    c.update(kw)
    tags = [k for k in ("bias", "resid", "relu", "f32", "acc") if c[k]]
    if c["alpha"] != 1.0:
        tags.append("a%g@%d" % (c["alpha"], c["ancols"]))
    c["id"] = "%s-%dx%dx%d-b%d-%s%s" % (L_NAME[layout], M, N, K, c["batch"], "+".join(tags) or "plain", "" if data == "int" else "-rand")
    c["seed"] = 1000 + (M * 7 + N * 13 + K * 17 + c["batch"]) % 100000
    return c


_ALL = dict(bias=True, alpha=0.5, ancols=100, resid=True, relu=True, acc=True)


def _variants(layout, M, N, K, reach, **kw):
    """each epilogue term alone and all together; alpha_ncols strictly inside a tile (100 = 64 + 36; N - 28)"""
    v = [dict(bias=True), dict(alpha=0.5, ancols=100), dict(alpha=2.0, ancols=N - 28), dict(resid=True), dict(relu=True),
         dict(f32=True), dict(acc=True), dict(f32=True, acc=True), dict(_ALL), dict(_ALL, f32=True, cpad=4)]
    return [_case(layout, M, N, K, reach, **dict(kw, **x)) for x in v]


B3 = dict(batch=3)
# ifseg_gemm_bf16 NT.  Columns: M, N, K, instantiation reached.  Every M edge {1, 127, 128, 129, 333, 2120, 8480}, N edge {8, 64, 72,
# 128, 136, 768, 3072} and K edge {8, 64, 72, 328, 768, 3072} against each of NT64/2, NT64/1, NT128/2, NT128/1 that can take it
# (N <= 64 is narrow by rule; NT128/2 cannot have batch 3: 384 x 3 > 1024).  The other dimensions are whatever the dispatch
# rule needs for that instantiation (a 1 x 131208 product is a legal F.linear).
GEMM_CASES = [
    # ---- NT64/2
    _case(NT, 1, 72, 72, "NT64/2"), _case(NT, 127, 136, 64, "NT64/2"), _case(NT, 128, 128, 328, "NT64/2"),
    _case(NT, 129, 8, 8, "NT64/2"), _case(NT, 333, 64, 768, "NT64/2"), _case(NT, 2120, 768, 768, "NT64/2"),
    _case(NT, 8480, 72, 72, "NT64/2"), _case(NT, 333, 3072, 64, "NT64/2"), _case(NT, 1025, 768, 3072, "NT64/2"),
    _case(NT, 333, 136, 72, "NT64/2", **dict(_ALL, **B3)), _case(NT, 129, 72, 328, "NT64/2", f32=True, **B3),
    # ---- NT64/1 (more than 1024 narrow workgroups: batch 3, or N <= 64 with more than 1024 row tiles)
    _case(NT, 1, 32776, 8, "NT64/1", **B3), _case(NT, 127, 32776, 64, "NT64/1", **B3), _case(NT, 128, 32776, 72, "NT64/1", **B3),
    _case(NT, 129, 24440, 8, "NT64/1", **B3), _case(NT, 333, 16256, 64, "NT64/1", **B3),
    _case(NT, 2120, 2816, 72, "NT64/1", **dict(_ALL, **B3)), _case(NT, 8480, 384, 3072, "NT64/1", **B3),
    _case(NT, 131201, 8, 8, "NT64/1"), _case(NT, 131201, 64, 72, "NT64/1", bias=True, relu=True),
    _case(NT, 22000, 72, 8, "NT64/1", **B3), _case(NT, 22000, 128, 64, "NT64/1", **B3), _case(NT, 22000, 136, 72, "NT64/1", **B3),
    _case(NT, 8000, 768, 328, "NT64/1", **B3), _case(NT, 1900, 3072, 72, "NT64/1", **B3), _case(NT, 8480, 384, 768, "NT64/1", **B3),
    # ---- NT128/2
    _case(NT, 1, 49160, 8, "NT128/2"), _case(NT, 127, 49160, 64, "NT128/2"), _case(NT, 128, 49160, 72, "NT128/2"),
    _case(NT, 129, 24584, 8, "NT128/2"), _case(NT, 333, 16392, 328, "NT128/2"), _case(NT, 2120, 3072, 768, "NT128/2"),
    _case(NT, 8480, 768, 768, "NT128/2"), _case(NT, 49153, 72, 8, "NT128/2"), _case(NT, 49153, 128, 64, "NT128/2"),
    _case(NT, 24600, 136, 72, "NT128/2"), _case(NT, 2120, 3072, 3072, "NT128/2"),
    # ---- NT128/1
    _case(NT, 1, 131208, 8, "NT128/1"), _case(NT, 127, 131208, 64, "NT128/1"), _case(NT, 128, 131208, 72, "NT128/1"),
    _case(NT, 129, 65672, 8, "NT128/1"), _case(NT, 333, 43784, 328, "NT128/1"), _case(NT, 2120, 7816, 72, "NT128/1"),
    _case(NT, 8480, 3072, 768, "NT128/1"), _case(NT, 131201, 72, 8, "NT128/1"), _case(NT, 131201, 128, 64, "NT128/1"),
    _case(NT, 65700, 136, 72, "NT128/1"), _case(NT, 21900, 768, 8, "NT128/1"), _case(NT, 5500, 3072, 3072, "NT128/1"),
    _case(NT, 8480, 3072, 768, "NT128/1", **_ALL), _case(NT, 8480, 768, 768, "NT128/1", **dict(_ALL, f32=True, **B3)),
    # ---- NN (dX): one tile width, two stage counts; N, K from {8, 72, 128, 768, 2304, 3072}
    _case(NN, 1, 72, 8, "NN128/2"), _case(NN, 127, 128, 72, "NN128/2"), _case(NN, 128, 768, 128, "NN128/2"),
    _case(NN, 129, 8, 768, "NN128/2"), _case(NN, 333, 2304, 72, "NN128/2"), _case(NN, 2120, 3072, 128, "NN128/2"),
    _case(NN, 8480, 768, 2304, "NN128/2"), _case(NN, 333, 128, 3072, "NN128/2"), _case(NN, 333, 136, 72, "NN128/2", resid=True, **B3),
    _case(NN, 1, 131208, 8, "NN128/1"), _case(NN, 127, 131208, 72, "NN128/1"), _case(NN, 128, 131208, 8, "NN128/1"),
    _case(NN, 129, 65672, 72, "NN128/1"), _case(NN, 333, 43784, 128, "NN128/1"), _case(NN, 2120, 7816, 72, "NN128/1"),
    _case(NN, 8480, 3072, 768, "NN128/1"), _case(NN, 8480, 2304, 128, "NN128/1"), _case(NN, 2120, 3072, 3072, "NN128/1", **B3),
    _case(NN, 8480, 768, 768, "NN128/1", **dict(_ALL, **B3)),
    # ---- TN plain (dW without split): output [M = N_out, N], reduction K (> 4096: p = 0.25)
    _case(TN, 8, 8, 8, "TN128/2"), _case(TN, 136, 72, 72, "TN128/2"), _case(TN, 768, 768, 1000, "TN128/2"),
    _case(TN, 3072, 768, 2120, "TN128/2"), _case(TN, 768, 3072, 8480, "TN128/2"), _case(TN, 136, 136, 8480, "TN128/2", f32=True, acc=True),
    _case(TN, 8, 3072, 1000, "TN128/2", f32=True), _case(TN, 768, 136, 2120, "TN128/2", acc=True),
    _case(TN, 3072, 8200, 72, "TN128/1"), _case(TN, 3072, 8200, 8, "TN128/1", f32=True, acc=True),
    _case(TN, 136, 264, 1000, "TN128/2", f32=True, **B3),
]
GEMM_CASES += _variants(NT, 333, 264, 328, "NT64/2") + _variants(NT, 8480, 768, 768, "NT128/2")
GEMM_CASES += [_case(NN, 333, 2304, 72, "NN128/2", **x) for x in (dict(resid=True), dict(acc=True), dict(f32=True), dict(f32=True, acc=True), dict(_ALL))]
GEMM_CASES += [_case(NN, 8480, 3072, 768, "NN128/1", **x) for x in (dict(resid=True), dict(acc=True), dict(f32=True, acc=True, cpad=4))]
# part B: one or two random-valued cases per instantiation (fp32 outputs: the bound is the accumulation term alone).
# PART_B_WIDEN -- `widen=w` on a row (here, in GROUP_WIDEN, ROWDOT_CASES and CONV_CASES): the accumulation term of the
# specified bound is multiplied by 2^w for that case, the smallest power of two with which the bound holds on MI355X, as the
# specification of this suite prescribes when the bound itself is wrong.  Observed, on every row that carries one: the worst
# element is a bf16 output just above a power of two that holds the CORRECTLY ROUNDED value (NT-131201x64x72: ref 4.01563
# stored as 4.03125, an error of 2^-8 |ref|); the first term allows 2^-9 |ref| (1 + 2^-6), half of what one round-to-nearest
# to bfloat16 (8 significant bits, unit roundoff 2^-8) can cost, and the accumulation term (76 x 2^-23 mag there) has to
# make up the difference.  The factors the term needed (worst |err| / bound before widening in brackets): NT-333x264x328 all
# terms 9.7 (1.71), NT-131201x64x72 142.5 (1.94), NT-2120x3072x768 3.04 (1.48), NT-8480x3072x768 all terms 5.04 (1.63),
# NN-333x2304x72 123.4 (1.93), NN-8480x2304x128 56.4 (1.92), TN-3072x8200x72 acc 145 (1.94); fp32-output rows need no
# widening (worst ratio 0.012).  Nothing of this reflects the kernels' accumulation: _assert_bound asserts, beside the
# widened bound, the bound with u_out = 2^-8 and the accumulation term as specified (worst ratio of any case 0.98).
GEMM_CASES += [
    _case(NT, 333, 264, 328, "NT64/2", "rand", widen=4, **_ALL), _case(NT, 2120, 768, 768, "NT64/2", "rand", f32=True, bias=True, resid=True),
    _case(NT, 8480, 384, 768, "NT64/1", "rand", f32=True, **B3), _case(NT, 131201, 64, 72, "NT64/1", "rand", bias=True, widen=8),
    _case(NT, 8480, 768, 768, "NT128/2", "rand", f32=True, bias=True, alpha=0.37, ancols=100), _case(NT, 2120, 3072, 768, "NT128/2", "rand", widen=2),
    _case(NT, 8480, 3072, 768, "NT128/1", "rand", f32=True), _case(NT, 8480, 3072, 768, "NT128/1", "rand", widen=3, **_ALL),
    _case(NN, 2120, 3072, 128, "NN128/2", "rand", f32=True), _case(NN, 333, 2304, 72, "NN128/2", "rand", resid=True, widen=7),
    _case(NN, 8480, 3072, 768, "NN128/1", "rand", f32=True, acc=True), _case(NN, 8480, 2304, 128, "NN128/1", "rand", widen=6),
    _case(TN, 768, 768, 1000, "TN128/2", "rand", f32=True), _case(TN, 3072, 768, 2120, "TN128/2", "rand"),
    _case(TN, 3072, 8200, 72, "TN128/1", "rand", f32=True), _case(TN, 3072, 8200, 72, "TN128/1", "rand", acc=True, widen=8),
]


def _build_gemm(c, dev):
    """inputs in guarded allocations on `dev`, the fp64 reference, the product alone and (random data) the magnitude sum"""
    L, M, N, K, b, s = c["layout"], c["M"], c["N"], c["K"], c["batch"], c["seed"]
    shA = (b, K, M) if L == TN else (b, M, K)
    shB = (b, N, K) if L == NT else (b, K, N)
    exact = c["data"] == "int"
    p = c.get("p", _p_for(K))
    draw = (lambda sh, sd, lim: _tern(sh, sd, p) if lim == 0 else _ints(sh, sd, lim)) if exact else \
           (lambda sh, sd, lim: _randn(sh, sd, 0.5 if lim == 0 else 1.0))
    Af, A = _guarded(draw(shA, s, 0), BF16, dev, 8, GUARD)
    Bf, B = _guarded(draw(shB, s + 1, 0), BF16, dev, 16, GUARD)
    bias = draw((N,), s + 2, 2).to(BF16).to(dev) if c["bias"] else None
    Rf, R = _guarded(draw((b, M, N), s + 3, 4), BF16, dev, 16, GUARD) if c["resid"] else (None, None)
    odt = F32 if c["f32"] else BF16
    if c["acc"]:
        Cf, C = _guarded(draw((b, M, N), s + 4, 4), odt, dev, c["cpad"], SENTINEL)
    else:
        Cf, C = _guarded((b, M, N), odt, dev, c["cpad"], SENTINEL)
    a, bb = A.double(), B.double()
    mm = {NT: lambda x, y: x @ y.transpose(1, 2), NN: lambda x, y: x @ y, TN: lambda x, y: x.transpose(1, 2) @ y}[L]
    prod = mm(a, bb)
    mag = None if exact else mm(a.abs(), bb.abs())
    ref = prod.clone()
    alpha = 0.37 if (not exact and c["alpha"] != 1.0) else c["alpha"]
    if bias is not None:
        ref += bias.double()
        mag = None if exact else mag + bias.double().abs()
    if alpha != 1.0:
        nc = N if c["ancols"] < 0 else c["ancols"]
        ref[..., :nc] *= alpha
        if not exact:
            mag[..., :nc] *= abs(alpha)
    if R is not None:
        ref += R.double()
        mag = None if exact else mag + R.double().abs()
    if c["relu"]:
        ref.clamp_(min=0)
    if c["acc"]:
        ref += C.double()
        mag = None if exact else mag + C.double().abs()
    return dict(A=A, B=B, bias=bias, R=R, Cf=Cf, C=C, ref=ref, prod=prod, mag=mag, alpha=alpha, keep=(Af, Bf, Rf))


def _run_gemm(c, t):
    from ifseg_amd import hip
    A, B, C, R = t["A"], t["B"], t["C"], t["R"]
    flags = (RELU if c["relu"] else 0) | (OUT_F32 if c["f32"] else 0) | (ACCUMULATE if c["acc"] else 0)
    hip.gemm(c["layout"], A, B, C, c["M"], c["N"], c["K"], A.stride(1), B.stride(1), C.stride(1), t["bias"], t["alpha"], c["ancols"],
             R, R.stride(1) if R is not None else 0, flags, c["batch"], A.stride(0), B.stride(0), C.stride(0),
             R.stride(0) if R is not None else 0, 1)
    torch.cuda.synchronize()


def _ids(cases):
    return [c["id"] for c in cases]


def _exact_cases(cases):
    return [c for c in cases if c["data"] == "int"]


def test_tables_name_the_instantiation_the_dispatch_rule_picks():
    for c in GEMM_CASES:
        assert _reach(c["layout"], c["M"], c["N"], c["batch"]) == c["reach"], c["id"]
    assert {c["reach"] for c in GEMM_CASES} == {"NT64/1", "NT64/2", "NT128/1", "NT128/2", "NN128/1", "NN128/2", "TN128/1", "TN128/2"}
    for c in SPLIT_CASES:
        kchunk, nsl, xcd, st = _split_geometry(c["M"], c["N"], c["K"], c["splitk"])
        assert (xcd, st) == (c["grid"] == "xcd", c["stages"]), (c["id"], xcd, st)
        assert c["K"] % kchunk != 0 and nsl > 1, c["id"]          # a ragged last slice
    assert {(c["colsum"], c["stages"]) for c in SPLIT_CASES} == {(False, 1), (False, 2), (True, 1), (True, 2)}
    for c in CONV_CASES:
        OH, OW = _conv_out(c)
        if c["KH"] == 1 and c["stride"] == 1:
            assert c["reach"] == "NT" + _nt_reach(c["B"] * OH * OW, c["Cout"]), c["id"]
        else:
            assert c["reach"] == "CONV" + _nt_reach(c["B"] * OH * OW, c["Cout"]), c["id"]
    assert {c["reach"] for c in CONV_CASES} >= {"CONV64/1", "CONV64/2", "CONV128/1", "CONV128/2"}
    for M, N, K, T, reach, data in ROWDOT_CASES:
        assert _reach(NN, M, N) == reach
    for M, N, K, reach in GLN_CASES:
        assert _reach(NN, M, N) == reach.replace("GLN", "NN")


@pytest.mark.parametrize("c", _exact_cases(GEMM_CASES), ids=_ids(_exact_cases(GEMM_CASES)))
def test_inputs_gemm(c):
    """the conditions on the inputs of part A hold (no GPU needed)"""
    t = _build_gemm(c, CPU)
    _assert_valid_reference(t["ref"], t["prod"], F32 if c["f32"] else BF16, c["K"], c["id"])


@gpu
@pytest.mark.parametrize("c", GEMM_CASES, ids=_ids(GEMM_CASES))
def test_gemm(c):
    """ifseg_gemm_bf16, unsplit.  Part A rows: exact.  -rand rows: the part B bounds (PART_B_WIDEN at the table)."""
    dev = _dev()
    t = _build_gemm(c, dev)
    if c["data"] == "int":
        _assert_valid_reference(t["ref"], t["prod"], F32 if c["f32"] else BF16, c["K"], c["id"])
    before = t["Cf"].clone()
    _run_gemm(c, t)
    _assert_surroundings(t["Cf"], before, lambda f: f[:, 3:3 + c["M"], :c["N"]], c["id"])
    if c["data"] == "int":
        _assert_exact(t["C"], t["ref"], _bn(c["reach"]), c["id"])
    else:
        _assert_bound(t["C"], t["ref"], t["mag"], c["K"] + 4, c["id"], c["widen"])


# ------------------------------------------------------------------------------------- TN split-K + reductions
def _split(M, N, K, splitk, grid, stages, colsum=False, follow="parts", out=F32, acc=False, data="int"):
    return dict(M=M, N=N, K=K, splitk=splitk, grid=grid, stages=stages, colsum=colsum, follow=follow, out=out, acc=acc, data=data,
                id="TNsplit%d-%dx%dx%d-%s%s-%s-%s%s%s" % (splitk, M, N, K, grid, "-colsum" if colsum else "", follow,
                                                        "bf16" if out == BF16 else "f32", "+acc" if acc else "", "" if data == "int" else "-rand"))


# split-K in {2, 3, 4, 8, 16}, last slice ragged in every row; "xcd": the 1-D XCD-pinned grid (slice count divides 8 and
# 8 / slices divides the tile count), "3d": the plain grid; reaches TN128 and TN128+COLSUM with 2 and 1 stages
SPLIT_CASES = [
    _split(768, 768, 8480, 2, "xcd", 2), _split(768, 768, 8480, 4, "xcd", 2, colsum=True, out=BF16),
    _split(768, 768, 8480, 8, "xcd", 2, follow="multi", out=BF16, acc=True), _split(136, 136, 1000, 3, "3d", 2, follow="multi"),
    _split(768, 640, 2120, 16, "3d", 2, colsum=True, acc=True), _split(136, 72, 2120, 2, "3d", 2, out=BF16),
    _split(3072, 768, 8480, 4, "xcd", 2, colsum=True, follow="multi", out=BF16, acc=True),
    _split(3072, 3072, 2120, 2, "xcd", 1, out=BF16), _split(3072, 3072, 2120, 2, "xcd", 1, colsum=True, follow="multi"),
    _split(3080, 3072, 1000, 3, "3d", 1, colsum=True, out=BF16),
    _split(768, 768, 8480, 4, "xcd", 2, colsum=True, data="rand"), _split(3072, 3072, 2120, 2, "xcd", 1, data="rand"),
    _split(3080, 3072, 1000, 3, "3d", 1, colsum=True, data="rand"), _split(136, 136, 1000, 3, "3d", 2, data="rand"),
]


def _build_split(c, dev):
    M, N, K = c["M"], c["N"], c["K"]
    exact = c["data"] == "int"
    s = 5000 + M + 3 * N + 7 * K + c["splitk"]
    p = _p_for(K)
    Af, A = _guarded((_tern((1, K, M), s, p) if exact else _randn((1, K, M), s, 0.5)), BF16, dev, 8, GUARD)
    Bf, B = _guarded((_tern((1, K, N), s + 1, p) if exact else _randn((1, K, N), s + 1, 0.5)), BF16, dev, 16, GUARD)
    n = M * N + (M if c["colsum"] else 0)
    old = (_ints((n,), s + 2, 4) if exact else _randn((n,), s + 2)) if c["acc"] else (n,)
    Of, O = _flat_guarded(old, c["out"], dev, SENTINEL)
    a, b = A[0].double(), B[0].double()
    prod = a.t() @ b
    ref = torch.cat([prod.reshape(-1), a.sum(0)]) if c["colsum"] else prod.reshape(-1)
    mag = None
    if not exact:
        mag = a.abs().t() @ b.abs()
        mag = torch.cat([mag.reshape(-1), a.abs().sum(0)]) if c["colsum"] else mag.reshape(-1)
    if c["acc"]:
        ref = ref + O.double()
        mag = None if exact else mag + O.double().abs()
    return dict(A=A[0], B=B[0], Of=Of, O=O, ref=ref, prod=prod, mag=mag, keep=(Af, Bf))


@pytest.mark.parametrize("c", _exact_cases(SPLIT_CASES), ids=_ids(_exact_cases(SPLIT_CASES)))
def test_inputs_split(c):
    t = _build_split(c, CPU)
    _assert_valid_reference(t["ref"], t["prod"], c["out"], c["K"], c["id"])


@gpu
@pytest.mark.parametrize("c", SPLIT_CASES, ids=_ids(SPLIT_CASES))
def test_gemm_tn_splitk_and_reduction(c):
    """every k-slice slab [M x N | M] against the product over its own rows, the workspace around the slabs untouched, then
    the sum of the slabs by ifseg_reduce_parts / ifseg_reduce_parts_multi into a guarded bf16 / fp32 destination"""
    from ifseg_amd import hip
    dev = _dev()
    M, N, K = c["M"], c["N"], c["K"]
    exact = c["data"] == "int"
    t = _build_split(c, dev)
    if exact:
        _assert_valid_reference(t["ref"], t["prod"], c["out"], K, c["id"])
    kchunk, nsl, _, _ = _split_geometry(M, N, K, c["splitk"])
    slab = M * N + (M if c["colsum"] else 0)
    wsf, ws = _flat_guarded((nsl, slab), F32, dev, SENTINEL)
    before = wsf.clone()
    A, B = t["A"], t["B"]
    hip.gemm(TN, A, B, ws, M, N, K, A.stride(0), B.stride(0), N, flags=OUT_F32 | (COLSUM if c["colsum"] else 0), splitk=c["splitk"])
    torch.cuda.synchronize()
    _assert_surroundings(wsf, before, lambda f: f[16:16 + nsl * slab], c["id"] + " workspace")
    if exact:
        for z in range(nsl):
            a, b = A[z * kchunk:min(K, (z + 1) * kchunk)].double(), B[z * kchunk:min(K, (z + 1) * kchunk)].double()
            _assert_exact(ws[z, :M * N].view(1, M, N), (a.t() @ b).view(1, M, N), 128, "%s slab %d" % (c["id"], z))
            if c["colsum"]:
                _assert_exact(ws[z, M * N:].view(1, 1, M), a.sum(0).view(1, 1, M), 128, "%s slab %d column sums" % (c["id"], z))
    obefore = t["Of"].clone()
    if c["follow"] == "parts":
        hip.reduce_parts(ws, t["O"], 1, nsl, slab, accumulate=c["acc"])
    else:
        hip.reduce_parts_multi([(ws, t["O"], 1, nsl, slab, c["acc"])])
    torch.cuda.synchronize()
    _assert_surroundings(t["Of"], obefore, lambda f: f[16:16 + slab], c["id"] + " reduction")
    if exact:
        _assert_exact(t["O"].view(1, 1, slab), t["ref"].view(1, 1, slab), 128, c["id"] + " reduced")
    else:
        _assert_bound(t["O"], t["ref"], t["mag"], K + 4 + nsl, c["id"])


def _reduce_tasks(ntask, dev):
    """ntask reductions of different shapes over integer-valued fp32 parts"""
    out = []
    for i in range(ntask):
        outer, parts, n = 1 + i % 3, (1, 2, 7, 8, 9, 33)[i % 6], (1, 31, 32, 33, 100, 768)[(i * 5 + 1) % 6]
        inp = _ints((outer, parts, n), 7000 + i, 5)
        odt, acc = (BF16 if i % 2 else F32), i % 3 == 1
        old = _ints((outer, n), 7100 + i, 4) if acc else (outer, n)
        Of, O = _flat_guarded(old, odt, dev, SENTINEL)
        inp = inp.to(F32).to(dev)
        ref = inp.double().sum(1) + (O.double() if acc else 0)
        out.append(dict(inp=inp, Of=Of, O=O, outer=outer, parts=parts, n=n, acc=acc, ref=ref, odt=odt))
    return out


@pytest.mark.parametrize("ntask", [1, 16, 17])
def test_inputs_reduce(ntask):
    for t in _reduce_tasks(ntask, CPU):
        assert bool((t["ref"].to(t["odt"]).double() == t["ref"]).all())


@gpu
@pytest.mark.parametrize("ntask", [1, 16, 17])
def test_reduce_parts_multi(ntask):
    """1, 16 (one full launch) and 17 (the binding cuts it into 16 + 1) tasks; ifseg_reduce_parts on the same tasks agrees"""
    from ifseg_amd import hip
    dev = _dev()
    ts = _reduce_tasks(ntask, dev)
    befores = [t["Of"].clone() for t in ts]
    hip.reduce_parts_multi([(t["inp"], t["O"], t["outer"], t["parts"], t["n"], t["acc"]) for t in ts])
    torch.cuda.synchronize()
    for i, (t, b) in enumerate(zip(ts, befores)):
        _assert_surroundings(t["Of"], b, lambda f: f[16:16 + t["outer"] * t["n"]], "task %d" % i)
        _assert_exact(t["O"].view(1, t["outer"], t["n"]), t["ref"].view(1, t["outer"], t["n"]), 128, "reduce_parts_multi task %d of %d" % (i, ntask))
        t["Of"].copy_(b)
        hip.reduce_parts(t["inp"], t["O"], t["outer"], t["parts"], t["n"], accumulate=t["acc"])
        torch.cuda.synchronize()
        _assert_surroundings(t["Of"], b, lambda f: f[16:16 + t["outer"] * t["n"]], "task %d (single)" % i)
        _assert_exact(t["O"].view(1, t["outer"], t["n"]), t["ref"].view(1, t["outer"], t["n"]), 128, "reduce_parts task %d" % i)


# ------------------------------------------------------------------------ TN + COLSUM without split; grouped dW
def _dw_problem(M, N, K, colsum, acc, dev, seed, data="int"):
    """dW [M, N] = A[K, M]^T B[K, N] as bf16 with db [M] right behind it, in one guarded allocation"""
    exact = data == "int"
    p = _p_for(K)
    Af, A = _guarded((_tern((1, K, M), seed, p) if exact else _randn((1, K, M), seed, 0.5)), BF16, dev, 8, GUARD)
    Bf, B = _guarded((_tern((1, K, N), seed + 1, p) if exact else _randn((1, K, N), seed + 1, 0.5)), BF16, dev, 16, GUARD)
    n = M * N + M
    old = torch.full((n,), SENTINEL)
    if acc:
        fresh = _ints((n,), seed + 2, 4) if exact else _randn((n,), seed + 2)
        old[:M * N + (M if colsum else 0)] = fresh[:M * N + (M if colsum else 0)].to(old.dtype)
    Of, O = _flat_guarded(old, BF16, dev, SENTINEL)
    a, b = A[0].double(), B[0].double()
    prod = a.t() @ b
    nout = M * N + (M if colsum else 0)
    ref = torch.cat([prod.reshape(-1), a.sum(0)])[:nout]
    mag = None if exact else torch.cat([(a.abs().t() @ b.abs()).reshape(-1), a.abs().sum(0)])[:nout]
    if acc:
        ref = ref + O[:nout].double()
        mag = None if exact else mag + O[:nout].double().abs()
    return dict(A=A[0], B=B[0], Of=Of, O=O, W=O[:M * N].view(M, N), db=O[M * N:] if colsum else None, nout=nout, ref=ref, prod=prod,
                mag=mag, M=M, N=N, K=K, colsum=colsum, acc=acc, keep=(Af, Bf))


def _check_dw(t, before, exact, what, widen=0):
    _assert_surroundings(t["Of"], before, lambda f: f[16:16 + t["nout"]], what)
    if exact:
        _assert_exact(t["O"][:t["nout"]].view(1, 1, -1), t["ref"].view(1, 1, -1), t["N"], what + " (flat index = m * N + n, then db[m])")
    else:
        _assert_bound(t["O"][:t["nout"]], t["ref"], t["mag"], t["K"] + 4, what, widen)


# M not a multiple of 32 (4 waves x 8): 136, 776; TN128+COLSUM/2 without split; db bf16 behind dW, ACCUMULATE on both
COLSUM_CASES = [(136, 72, 1000, True, "int"), (776, 768, 2120, False, "int"), (776, 264, 328, True, "int"), (776, 768, 2120, True, "rand")]


@pytest.mark.parametrize("M,N,K,acc,data", [c for c in COLSUM_CASES if c[4] == "int"])
def test_inputs_colsum(M, N, K, acc, data):
    t = _dw_problem(M, N, K, True, acc, CPU, 8000 + M + K)
    _assert_valid_reference(t["ref"], t["prod"], BF16, K, "colsum %dx%dx%d" % (M, N, K))


@gpu
@pytest.mark.parametrize("M,N,K,acc,data", COLSUM_CASES)
def test_gemm_tn_colsum_unsplit(M, N, K, acc, data):
    from ifseg_amd import hip
    dev = _dev()
    t = _dw_problem(M, N, K, True, acc, dev, 8000 + M + K, data)
    if data == "int":
        _assert_valid_reference(t["ref"], t["prod"], BF16, K, "colsum")
    before = t["Of"].clone()
    hip.gemm(TN, t["A"], t["B"], t["W"], M, N, K, t["A"].stride(0), t["B"].stride(0), N, flags=COLSUM | (ACCUMULATE if acc else 0))
    torch.cuda.synchronize()
    _check_dw(t, before, data == "int", "TN+COLSUM %dx%dx%d acc=%s" % (M, N, K, acc))


# (M, N, K, colsum, accumulate) per problem.  8: smaller than a tile (8 x 8), tiles_m < tiles_n (136 x 768: the row-fastest
# order), 648 tiles in all, so that the caps 8, 100 (-> 96) and 512 all make a workgroup walk several tiles
GROUPS = {
    1: [(136, 768, 328, True, True)],
    3: [(8, 8, 72, True, False), (768, 768, 2120, False, True), (264, 1536, 1000, True, False)],
    8: [(768, 768, 2120, True, False), (3072, 1536, 1000, True, True), (1536, 3072, 1000, False, False), (8, 8, 72, False, True),
        (136, 768, 328, True, False), (72, 136, 8, True, True), (768, 136, 8480, False, False), (264, 264, 1000, True, True)],
}


# PART_B_WIDEN per problem (needed factors 15.0; 57.1, 0.74, 2.65; 0.74, 3.00, 3.08, 51.6, 13.5, 1142 (K = 8), 0.09, 2.14)
GROUP_WIDEN = {1: [4], 3: [6, 0, 2], 8: [0, 2, 2, 6, 4, 11, 0, 2]}


def _group(n, dev, data="int"):
    return [_dw_problem(M, N, K, cs, acc, dev, 9000 + 10 * i + n, data) for i, (M, N, K, cs, acc) in enumerate(GROUPS[n])]


@pytest.mark.parametrize("n", [1, 3, 8])
def test_inputs_group(n):
    for t in _group(n, CPU):
        _assert_valid_reference(t["ref"], t["prod"], BF16, t["K"], "group of %d, %dx%dx%d" % (n, t["M"], t["N"], t["K"]))


@gpu
@pytest.mark.parametrize("data", ["int", "rand"])
@pytest.mark.parametrize("n", [1, 3, 8])
def test_gemm_tn_group(n, data):
    """exact (or within the part B bounds) for every workgroup cap, and the same bits for every cap"""
    from ifseg_amd import hip
    dev = _dev()
    ts = _group(n, dev, data)
    if data == "int":
        for t in ts:
            _assert_valid_reference(t["ref"], t["prod"], BF16, t["K"], "group")
    befores = [t["Of"].clone() for t in ts]
    first = None
    for cap in (0, 8, 512, 100):
        for t, b in zip(ts, befores):
            t["Of"].copy_(b)
        hip.linear_dw_group([(t["A"], t["B"], t["W"], t["db"], t["acc"]) for t in ts], wgs=cap)
        torch.cuda.synchronize()
        for i, (t, b) in enumerate(zip(ts, befores)):
            _check_dw(t, b, data == "int", "group of %d, problem %d (%dx%dx%d), cap %d" % (n, i, t["M"], t["N"], t["K"], cap),
                      GROUP_WIDEN[n][i])
        bits = [_bits(t["Of"]).clone() for t in ts]
        if first is None:
            first = bits
        assert all(torch.equal(x, y) for x, y in zip(first, bits)), "cap %d changes the result" % cap


# ------------------------------------------------------------------------------------------------ rowdot
# M, N, K, rows_per_batch, instantiation, data.  M is not a multiple of rows_per_batch: the last batch is short
ROWDOT_CASES = [(333, 64, 72, 100, "NN128/2", "int"), (2125, 768, 768, 1060, "NN128/2", "int"), (22000, 768, 72, 1000, "NN128/1", "int"),
                (2125, 768, 768, 1060, "NN128/2", "rand")]


def _build_rowdot(M, N, K, T, dev, data):
    exact = data == "int"
    s = 11000 + M + N + K
    p = _p_for(K)
    Af, A = _guarded((_tern((1, M, K), s, p) if exact else _randn((1, M, K), s, 0.5)), BF16, dev, 8, GUARD)
    Bf, B = _guarded((_tern((1, K, N), s + 1, p) if exact else _randn((1, K, N), s + 1, 0.5)), BF16, dev, 16, GUARD)
    Df, D = _guarded((_ints((1, M, N), s + 2, 2) if exact else _randn((1, M, N), s + 2)), BF16, dev, 24, GUARD)
    Cf, C = _guarded((1, M, N), BF16, dev, 8, SENTINEL)
    nb, H = _ceil(M, T), N // 64
    dof, do = _flat_guarded((nb, H, T), F32, dev, SENTINEL)
    a, b = A[0].double(), B[0].double()
    prod = a @ b
    mag = None if exact else a.abs() @ b.abs()
    return dict(A=A[0], B=B[0], D=D[0], Cf=Cf, C=C[0], dof=dof, do=do, prod=prod, mag=mag, nb=nb, H=H, keep=(Af, Bf, Df))


def _rowdot_expected(c_as_stored, D, M, N, T, nb, H):
    """dot_out[b, h, t] = sum_c C[b T + t][64 h + c] (as stored) * dot[b T + t][64 h + c]; rows past M keep the sentinel"""
    d = (c_as_stored.double() * D.double()).view(M, H, 64).sum(2)                    # [M, H]
    full = torch.full((nb * T, H), SENTINEL, dtype=torch.float64, device=d.device)
    full[:M] = d
    return full.view(nb, T, H).transpose(1, 2).contiguous()


@pytest.mark.parametrize("M,N,K,T,reach,data", [c for c in ROWDOT_CASES if c[5] == "int"])
def test_inputs_rowdot(M, N, K, T, reach, data):
    t = _build_rowdot(M, N, K, T, CPU, data)
    _assert_valid_reference(t["prod"], t["prod"], BF16, K, "rowdot dx")
    exp = _rowdot_expected(t["prod"], t["D"], M, N, T, t["nb"], t["H"])
    assert bool((exp.float().double() == exp).all())


@gpu
@pytest.mark.parametrize("M,N,K,T,reach,data", ROWDOT_CASES)
def test_gemm_nn_rowdot(M, N, K, T, reach, data):
    """exact dx and exact dot_out[b, h, t]; the -rand case: part B bounds on dot_out (fp32) and on dx (bf16)"""
    from ifseg_amd import hip
    dev = _dev()
    t = _build_rowdot(M, N, K, T, dev, data)
    cb, db = t["Cf"].clone(), t["dof"].clone()
    hip.linear_dx_rowdot(t["A"], t["B"], t["C"], t["D"], t["do"], T)
    torch.cuda.synchronize()
    _assert_surroundings(t["Cf"], cb, lambda f: f[:, 3:3 + M, :N], "rowdot dx")
    _assert_surroundings(t["dof"], db, lambda f: f[16:16 + t["nb"] * t["H"] * T], "rowdot dot_out")
    if data == "int":
        _assert_valid_reference(t["prod"], t["prod"], BF16, K, "rowdot dx")
        _assert_exact(t["C"].view(1, M, N), t["prod"].view(1, M, N), 128, "rowdot dx %dx%dx%d" % (M, N, K))
        exp = _rowdot_expected(t["prod"], t["D"], M, N, T, t["nb"], t["H"])
        _assert_exact(t["do"], exp, 1, "rowdot dot_out[b, h, t] %dx%dx%d T=%d" % (M, N, K, T))
    else:
        # the dots are taken of dx AS STORED (bf16): 64 exact fp32 products summed in fp32
        exp = _rowdot_expected(t["C"], t["D"], M, N, T, t["nb"], t["H"])
        dmag = _rowdot_expected(t["C"].double().abs(), t["D"].double().abs(), M, N, T, t["nb"], t["H"]).abs()
        _assert_bound(t["do"], exp, dmag, 64 + 4, "rowdot dot_out")
        _assert_bound(t["C"], t["prod"], t["mag"], K + 4, "rowdot dx", 2)        # PART_B_WIDEN: needed 3.96 (1.46 before)


# ---------------------------------------------------------------------------------- GELU + LayerNorm backward epilogue
GLN_CASES = [(2125, 1024, 256, "GLN128/2"), (8485, 2048, 256, "GLN128/1")]


@gpu
@pytest.mark.parametrize("M,N,K,reach", GLN_CASES)
def test_gemm_nn_gelu_ln_bwd(M, N, K, reach):
    """du = rstd (gamma dz - c1 - xh c2) gelu'(u), dz = A . B, xh = (gelu(u) - mean) rstd (include/ifseg_hip.h), in fp64 on the
    bf16 / fp32 inputs the kernel gets.  Bound per element: 4 x the error of the SAME formula evaluated with fp32 torch ops
    (taken as the largest |f32 - f64| / mag over the case, mag = rstd (|gamma| |A|.|B| + |c1| + |xh c2|) (1/2 + |erf| / 2 + |u| pdf(u)),
    the sum of the magnitudes of the formula's terms) plus one bf16 rounding of the result, 2^-8 |ref| (1 + 2^-6).  Measured fp32-torch figure on MI355X: see
    profiles/gemm_conformance_kernels.txt."""
    from ifseg_amd import hip
    dev = _dev()
    s = 12000 + M
    Af, A = _guarded(_randn((1, M, K), s, 0.1), BF16, dev, 8, GUARD)
    Bf, B = _guarded(_randn((1, K, N), s + 1, 0.05), BF16, dev, 16, GUARD)
    Uf, U = _guarded(_randn((1, M, N), s + 2), BF16, dev, 8, GUARD)
    Cf, C = _guarded((1, M, N), BF16, dev, 16, SENTINEL)
    gamma = (1 + 0.2 * _randn((N,), s + 3)).to(dev)
    A, B, U, C = A[0], B[0], U[0], C[0]

    def formula(dt, mean, rstd, cst):
        u = U.to(dt)
        er, pdf = torch.erf(u / math.sqrt(2.0)), torch.exp(-0.5 * u * u) / math.sqrt(2 * math.pi)
        cdf = 0.5 * (1 + er)
        act, dact = u * cdf, cdf + u * pdf
        xh = (act - mean.to(dt)[:, None]) * rstd.to(dt)[:, None]
        dz = A.to(dt) @ B.to(dt)
        core = gamma.to(dt) * dz - cst[:, 0].to(dt)[:, None] - xh * cst[:, 1].to(dt)[:, None]
        return rstd.to(dt)[:, None] * core * dact, xh, 0.5 + 0.5 * er.abs() + u.abs() * pdf      # gelu' = 1/2 + erf / 2 + u pdf, term by term

    with torch.no_grad():
        g64 = U.double() * 0.5 * (1 + torch.erf(U.double() / math.sqrt(2.0)))
        mean = g64.mean(1).float()
        rstd = (g64.var(1, unbiased=False) + 1e-5).rsqrt().float()
        dz64 = A.double() @ B.double()
        xh64 = (g64 - mean.double()[:, None]) * rstd.double()[:, None]
        cst = torch.stack([(dz64 * gamma.double()).mean(1), (dz64 * gamma.double() * xh64).mean(1)], 1).float().contiguous()
        ref, xh, dmag = formula(torch.float64, mean, rstd, cst)
        f32, _, _ = formula(torch.float32, mean, rstd, cst)
        mag = rstd.double()[:, None] * (gamma.double().abs() * (A.double().abs() @ B.double().abs()) + cst[:, 0].double().abs()[:, None]
                                        + (xh * cst[:, 1].double()[:, None]).abs()) * dmag
        e32 = ((f32.double() - ref).abs() / mag).max().item()
    before = Cf.clone()
    hip.linear_dx_gelu_ln_bwd(A, B, C, U, gamma, mean, rstd, cst)
    torch.cuda.synchronize()
    _assert_surroundings(Cf, before, lambda f: f[:, 3:3 + M, :N], "gelu_ln_bwd")
    err = (C.double() - ref).abs()
    bound = 2.0 ** -8 * ref.abs() * (1 + 2.0 ** -6) + 4 * e32 * mag
    ratio = torch.nan_to_num(torch.where(err == 0, torch.zeros_like(err), err / bound), nan=float("inf"))
    k = int(ratio.argmax())
    msg = "gelu_ln_bwd %dx%dx%d (%s): fp32-torch error %.3g of mag; worst |err|/bound %.3f at (m %d, n %d), ref %g got %g" % (
        M, N, K, reach, e32, ratio.reshape(-1)[k].item(), k // N, k % N, ref.reshape(-1)[k].item(), C.double().reshape(-1)[k].item())
    print("[part B]", msg)
    assert ratio.reshape(-1)[k].item() <= 1.0, msg


# -------------------------------------------------------------------------------------------------- conv
def _conv(B, H, W, Cin, Cout, KH, stride, reach, shift=False, resid=False, relu=False, data="int", widen=0):
    tags = ("s" if shift else "") + ("r" if resid else "") + ("relu" if relu else "")
    return dict(B=B, H=H, W=W, Cin=Cin, Cout=Cout, KH=KH, stride=stride, pad=KH // 2, reach=reach, shift=shift, resid=resid, relu=relu,
                data=data, widen=widen, id="conv%dx%ds%d-%dx%dx%dx%d-%d-%s%s" % (KH, KH, stride, B, H, W, Cin, Cout, tags or "plain",
                                                                   "" if data == "int" else "-rand"))


def _conv_out(c):
    return ((c["H"] + 2 * c["pad"] - c["KH"]) // c["stride"] + 1, (c["W"] + 2 * c["pad"] - c["KH"]) // c["stride"] + 1)


# 1x1 s1 is the NT route; the others the implicit-GEMM loader (CONV64 / CONV128, 2 / 1 stages); odd H and W under stride 2
CONV_CASES = [
    _conv(2, 16, 20, 64, 64, 1, 1, "NT64/2", shift=True, relu=True), _conv(2, 64, 64, 256, 1024, 1, 1, "NT128/2", shift=True, resid=True, relu=True),
    _conv(2, 17, 21, 256, 72, 1, 2, "CONV64/2", shift=True), _conv(2, 16, 20, 64, 8, 3, 1, "CONV64/2"),
    _conv(2, 17, 21, 128, 256, 3, 2, "CONV64/2", shift=True, resid=True, relu=True), _conv(1, 15, 15, 64, 64, 3, 2, "CONV64/2", resid=True),
    _conv(2, 16, 20, 128, 1024, 3, 1, "CONV64/2", relu=True),
    _conv(2, 64, 64, 64, 1024, 3, 1, "CONV128/2", shift=True, resid=True, relu=True), _conv(2, 127, 129, 256, 1024, 1, 2, "CONV128/2", shift=True),
    _conv(4, 130, 128, 128, 1024, 1, 2, "CONV128/1", shift=True, resid=True), _conv(2, 129, 131, 64, 1024, 3, 2, "CONV128/2", resid=True, relu=True),
    _conv(1, 725, 725, 64, 8, 3, 2, "CONV64/1", shift=True, relu=True), _conv(1, 727, 725, 64, 64, 1, 2, "CONV64/1", shift=True, resid=True, relu=True),
    _conv(2, 64, 64, 64, 1024, 3, 1, "CONV128/2", shift=True, resid=True, relu=True, data="rand", widen=4),
    _conv(4, 130, 128, 128, 1024, 1, 2, "CONV128/1", shift=True, data="rand", widen=7),
    _conv(2, 17, 21, 128, 256, 3, 2, "CONV64/2", shift=True, resid=True, data="rand", widen=2),
    _conv(1, 725, 725, 64, 8, 3, 2, "CONV64/1", shift=True, relu=True, data="rand", widen=3),
]  # PART_B_WIDEN, in this order: needed 12.5 (1.79 before), 64.2 (1.93), 3.73 (1.46), 7.14 (1.71)


def _conv_ref(x, w, stride, pad):
    """F.conv2d in fp64 on NHWC / [Cout, KH, KW, Cin] operands -> NHWC"""
    import torch.nn.functional as Fn
    xd, wd = x.double().permute(0, 3, 1, 2), w.double().permute(0, 3, 1, 2)
    try:
        y = Fn.conv2d(xd, wd, stride=stride, padding=pad)
    except RuntimeError:            # a backend without fp64 convolutions: the same call on the CPU
        y = Fn.conv2d(xd.cpu(), wd.cpu(), stride=stride, padding=pad).to(x.device)
    return y.permute(0, 2, 3, 1).contiguous()


def _build_conv(c, dev):
    exact = c["data"] == "int"
    B, H, W, Cin, Cout, KH = c["B"], c["H"], c["W"], c["Cin"], c["Cout"], c["KH"]
    OH, OW = _conv_out(c)
    red = KH * KH * Cin
    s = 13000 + H + W + Cin + Cout + KH
    p = _p_for(red)
    xf, x = _flat_guarded(_tern((B, H, W, Cin), s, p) if exact else _randn((B, H, W, Cin), s), BF16, dev, GUARD)
    wf, w = _flat_guarded(_tern((Cout, KH, KH, Cin), s + 1, p) if exact else _randn((Cout, KH, KH, Cin), s + 1, 1.0 / math.sqrt(red)), BF16, dev, GUARD)
    shift = (_ints((Cout,), s + 2, 2) if exact else _randn((Cout,), s + 2)).to(BF16).to(dev) if c["shift"] else None
    rf, r = (_flat_guarded(_ints((B, OH, OW, Cout), s + 3, 4) if exact else _randn((B, OH, OW, Cout), s + 3), BF16, dev, GUARD)
             if c["resid"] else (None, None))
    of, o = _flat_guarded((B, OH, OW, Cout), BF16, dev, SENTINEL)
    prod = _conv_ref(x, w, c["stride"], c["pad"])
    mag = None if exact else _conv_ref(x.abs(), w.abs(), c["stride"], c["pad"])
    ref = prod.clone()
    if shift is not None:
        ref += shift.double()
        mag = None if exact else mag + shift.double().abs()
    if r is not None:
        ref += r.double()
        mag = None if exact else mag + r.double().abs()
    if c["relu"]:
        ref.clamp_(min=0)
    return dict(x=x, w=w, shift=shift, r=r, of=of, o=o, ref=ref, prod=prod, mag=mag, red=red, keep=(xf, wf, rf))


@pytest.mark.parametrize("c", _exact_cases(CONV_CASES), ids=_ids(_exact_cases(CONV_CASES)))
def test_inputs_conv(c):
    t = _build_conv(c, CPU)
    _assert_valid_reference(t["ref"], t["prod"], BF16, t["red"], c["id"])


@gpu
@pytest.mark.parametrize("c", CONV_CASES, ids=_ids(CONV_CASES))
def test_conv2d_nhwc(c):
    """exact against F.conv2d in fp64; -rand cases: the part B bounds"""
    from ifseg_amd import hip
    dev = _dev()
    t = _build_conv(c, dev)
    if c["data"] == "int":
        _assert_valid_reference(t["ref"], t["prod"], BF16, t["red"], c["id"])
    before = t["of"].clone()
    hip.conv2d_nhwc(t["x"], t["w"], t["shift"], t["r"], t["o"], c["B"], c["H"], c["W"], c["Cin"], c["Cout"], c["KH"], c["KH"], c["stride"],
                    c["pad"], c["relu"])
    torch.cuda.synchronize()
    _assert_surroundings(t["of"], before, lambda f: f[16:16 + t["o"].numel()], c["id"])
    OH, OW = _conv_out(c)
    M = c["B"] * OH * OW
    if c["data"] == "int":
        _assert_exact(t["o"].view(1, M, c["Cout"]), t["ref"].view(1, M, c["Cout"]), _bn(c["reach"]), c["id"] + " (m = (b OH + oy) OW + ox)")
    else:
        _assert_bound(t["o"], t["ref"], t["mag"], t["red"] + 4, c["id"], c["widen"])


# ------------------------------------------------------------------------------------------ argument checks
def _raw_gemm(layout, A, B, C, M, N, K, lda, ldb, ldc, bias=None, alpha=1.0, ancols=-1, resid=None, ldr=0, flags=0, batch=1,
              strides=(0, 0, 0, 0), splitk=1):
    from ifseg_amd import hip
    i, f, ll, P = ctypes.c_int, ctypes.c_float, ctypes.c_longlong, hip._ptr
    return hip.lib().ifseg_gemm_bf16(i(layout), P(A), P(B), P(C), i(M), i(N), i(K), i(lda), i(ldb), i(ldc), P(bias), f(alpha), i(ancols),
                                     P(resid), i(ldr), i(flags), i(batch), ll(strides[0]), ll(strides[1]), ll(strides[2]), ll(strides[3]),
                                     i(splitk), hip._stream())


@gpu
def test_refusals_leave_the_output_alone():
    """every documented refusal returns its code, zero sizes return 0, and neither writes a byte of a sentinel-filled C"""
    from ifseg_amd import hip
    dev = _dev()
    i, P = ctypes.c_int, hip._ptr
    A = torch.ones(256, 256, dtype=BF16, device=dev)
    Bm = torch.ones(256, 256, dtype=BF16, device=dev)
    C = torch.full((4, 256, 256), SENTINEL, dtype=F32, device=dev)
    want = C.clone()
    calls = {
        "N % 8": (_raw_gemm(NT, A, Bm, C, 64, 60, 64, 256, 256, 256), BAD_SHAPE),
        "lda % 8": (_raw_gemm(NT, A, Bm, C, 64, 64, 64, 252, 256, 256), BAD_SHAPE),
        "ldb % 8": (_raw_gemm(NN, A, Bm, C, 64, 64, 64, 256, 252, 256), BAD_SHAPE),
        "ldc % 4": (_raw_gemm(NT, A, Bm, C, 64, 64, 64, 256, 256, 250), BAD_SHAPE),
        "ldr % 4": (_raw_gemm(NT, A, Bm, C, 64, 64, 64, 256, 256, 256, resid=A, ldr=250), BAD_SHAPE),
        "K % 8 (NT)": (_raw_gemm(NT, A, Bm, C, 64, 64, 60, 256, 256, 256), BAD_SHAPE),
        "TN with M % 8": (_raw_gemm(TN, A, Bm, C, 60, 64, 64, 256, 256, 256), BAD_SHAPE),
        "split-K without OUT_F32": (_raw_gemm(TN, A, Bm, C, 64, 64, 256, 256, 256, 64, splitk=2), BAD_ARG),
        "split-K with ACCUMULATE": (_raw_gemm(TN, A, Bm, C, 64, 64, 256, 256, 256, 64, flags=OUT_F32 | ACCUMULATE, splitk=2), BAD_ARG),
        "split-K with bias": (_raw_gemm(TN, A, Bm, C, 64, 64, 256, 256, 256, 64, bias=A, flags=OUT_F32, splitk=2), BAD_ARG),
        "split-K with resid": (_raw_gemm(TN, A, Bm, C, 64, 64, 256, 256, 256, 64, resid=A, ldr=256, flags=OUT_F32, splitk=2), BAD_ARG),
        "alpha_ncols % 4 inside the matrix": (_raw_gemm(NT, A, Bm, C, 64, 128, 64, 256, 256, 256, alpha=0.5, ancols=102), BAD_ARG),
        "split-K with alpha": (_raw_gemm(TN, A, Bm, C, 64, 64, 256, 256, 256, 64, alpha=0.5, flags=OUT_F32, splitk=2), BAD_ARG),
        "COLSUM on NT": (_raw_gemm(NT, A, Bm, C, 64, 64, 64, 256, 256, 64, flags=COLSUM), BAD_ARG),
        "COLSUM on NN": (_raw_gemm(NN, A, Bm, C, 64, 64, 64, 256, 256, 64, flags=COLSUM), BAD_ARG),
        "COLSUM with ldc != N": (_raw_gemm(TN, A, Bm, C, 64, 64, 64, 256, 256, 72, flags=COLSUM), BAD_ARG),
        "COLSUM with batch > 1": (_raw_gemm(TN, A, Bm, C, 64, 64, 64, 256, 256, 64, flags=COLSUM, batch=2, strides=(0, 0, 65536, 0)), BAD_ARG),
        "unsplit COLSUM with OUT_F32": (_raw_gemm(TN, A, Bm, C, 64, 64, 64, 256, 256, 64, flags=COLSUM | OUT_F32), BAD_ARG),
        "layout 3": (_raw_gemm(3, A, Bm, C, 64, 64, 64, 256, 256, 64), BAD_ARG),
        "M = 0": (_raw_gemm(NT, A, Bm, C, 0, 64, 64, 256, 256, 256), 0),
        "N = 0": (_raw_gemm(NN, A, Bm, C, 64, 0, 64, 256, 256, 256), 0),
        "K = 0": (_raw_gemm(TN, A, Bm, C, 64, 64, 0, 256, 256, 256), 0),
    }
    L = hip.lib()
    dot_out = torch.full((4, 256), SENTINEL, dtype=F32, device=dev)
    dwant = dot_out.clone()
    calls["rowdot with N % 64"] = (L.ifseg_gemm_nn_rowdot(P(A), P(Bm), P(C), i(64), i(72), i(64), i(256), i(256), i(256), P(A), i(256),
                                                          P(dot_out), i(64), hip._stream()), BAD_ARG)
    pr = (hip._TnProblem * 9)()
    for q in pr:
        q.A, q.B, q.C = A.data_ptr(), Bm.data_ptr(), C.data_ptr()
        q.M, q.N, q.K, q.lda, q.ldb, q.colsum, q.accumulate = 64, 64, 64, 256, 256, 1, 0
    calls["group with n = 9"] = (L.ifseg_gemm_tn_group(i(9), pr, i(0), hip._stream()), BAD_ARG)
    calls["group without problems"] = (L.ifseg_gemm_tn_group(i(2), None, i(0), hip._stream()), BAD_ARG)
    calls["group with n = 0"] = (L.ifseg_gemm_tn_group(i(0), pr, i(0), hip._stream()), 0)
    pr[1].B = None
    null_rc = L.ifseg_gemm_tn_group(i(2), pr, i(0), hip._stream())
    pr[1].B = Bm.data_ptr()
    pr[1].M = 60
    calls["group with M % 8"] = (L.ifseg_gemm_tn_group(i(2), pr, i(0), hip._stream()), BAD_SHAPE)
    x = torch.ones(1, 8, 8, 96, dtype=BF16, device=dev)
    calls["conv with Cin % 64"] = (L.ifseg_conv2d_nhwc_bf16(P(x), P(A), None, None, P(C), i(1), i(8), i(8), i(96), i(64), i(1), i(1), i(1), i(0),
                                                            i(0), hip._stream()), BAD_SHAPE)
    calls["conv with Cout % 8"] = (L.ifseg_conv2d_nhwc_bf16(P(x), P(A), None, None, P(C), i(1), i(8), i(8), i(64), i(60), i(3), i(3), i(1), i(1),
                                                            i(0), hip._stream()), BAD_SHAPE)
    tasks = (hip._ReduceTask * 17)()
    for q in tasks:
        q.inp, q.out, q.outer, q.parts, q.n, q.accumulate, q.out_bf16, q.scale = A.data_ptr(), C.data_ptr(), 1, 2, 8, 0, 0, 1.0
    calls["reduce_parts_multi with 17 tasks"] = (L.ifseg_reduce_parts_multi(i(17), tasks, hip._stream()), BAD_ARG)
    tasks[0].inp = None
    calls["reduce_parts_multi with a null input"] = (L.ifseg_reduce_parts_multi(i(2), tasks, hip._stream()), BAD_ARG)
    calls["reduce_parts_multi with 0 tasks"] = (L.ifseg_reduce_parts_multi(i(0), tasks, hip._stream()), 0)
    torch.cuda.synchronize()
    wrong = {k: v for k, v in calls.items() if v[0] != v[1]}
    assert not wrong, "return codes (got, expected): %s" % wrong
    assert null_rc in (BAD_SHAPE, BAD_ARG), null_rc
    assert torch.equal(_bits(C), _bits(want)) and torch.equal(_bits(dot_out), _bits(dwant)), "a refused call wrote to its output"


@gpu
def test_refused_call_leaves_the_profiler_alone():
    """a refusal comes before the profiler bracket: it counts no launch, no flops, no bytes and leaves no slot open, so the
    next valid call of the family is counted and timed as the one launch it is"""
    from ifseg_amd import hip
    dev = _dev()
    A = torch.ones(256, 256, dtype=BF16, device=dev)
    Bm = torch.ones(256, 256, dtype=BF16, device=dev)
    C = torch.zeros(256, 256, dtype=BF16, device=dev)
    kind = hip.PROF_KINDS.index("gemm_tn")
    hip.prof_enable(1 << kind)
    hip.prof_reset()
    try:
        assert _raw_gemm(TN, A, Bm, C, 64, 64, 64, 256, 256, 72, flags=COLSUM) == BAD_ARG      # COLSUM with ldc != N
        r = hip.prof_read(kind)
        assert (r["launches"], r["flops"], r["bytes"]) == (0, 0.0, 0.0), r
        assert _raw_gemm(TN, A, Bm, C, 64, 64, 64, 256, 256, 64) == 0
        r = hip.prof_read(kind)
        assert r["launches"] == 1 and math.isfinite(r["ms"]) and r["ms"] >= 0.0, r
        assert (r["flops"], r["bytes"]) == (2.0 * 64 ** 3, 2.0 * 3 * 64 * 64), r
    finally:
        hip.prof_enable(0)
        hip.prof_reset()
