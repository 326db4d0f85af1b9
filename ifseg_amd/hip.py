"""ctypes binding of libifseg_hip.so (C ABI: include/ifseg_hip.h).

PyTorch tensors are used only as owners of device memory and for the current
HIP stream; every call passes raw device pointers + sizes.  There is NO
fallback: a missing library or a non-zero return code raises RuntimeError.
"""
import contextlib
import ctypes
import os

import torch

from . import lab

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("IFSEG_LIB", os.path.join(_HERE, "lib", "libifseg_hip.so"))
_lib = None

GEMM_NT, GEMM_NN, GEMM_TN = 0, 1, 2
GEMM_RELU, GEMM_OUT_F32, GEMM_ACCUMULATE, GEMM_COLSUM = 1, 2, 4, 8

c_void_p, c_int, c_float, c_ll = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_longlong


ABI_VERSION = 21         # == IFSEG_ABI_VERSION of include/ifseg_hip.h (checked at load time and by __graft_entry__.build)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "ifseg_amd: %s not found -- build it with `python -m ifseg_amd.build` "
                "(there is no CPU/PyTorch fallback for the HIP path)" % LIB_PATH)
        # bind to the HIP runtime PyTorch uses (one runtime per process; see ifseg_amd/build.py)
        rt = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
        if not os.path.exists(rt):
            rt = "libamdhip64.so"
        ctypes.CDLL(rt, mode=ctypes.RTLD_GLOBAL)
        _lib = ctypes.CDLL(LIB_PATH)
        _lib.ifseg_abi_version.restype = c_int
        if _lib.ifseg_abi_version() != ABI_VERSION:
            raise RuntimeError("ifseg_amd: ABI version mismatch")
    return _lib


def _check(rc, what):
    if rc != 0:
        raise RuntimeError("ifseg_amd HIP call %s failed with code %d" % (what, rc))


def _ptr(t):
    if t is None:
        return None
    assert t.is_cuda, "device tensor required"
    return c_void_p(t.data_ptr())


_stream_handle = None     # set by the engine for the duration of a forward / backward (saves a torch lookup per launch)


def set_stream(handle):
    """Pin the HIP stream every following launch goes to (raw hipStream_t as int), or None to follow
    torch.cuda.current_stream() again.  Returns the previous setting."""
    global _stream_handle
    prev = _stream_handle
    _stream_handle = handle
    return prev


def _stream():
    if _stream_handle is not None:
        return c_void_p(_stream_handle)
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def _bf(t):
    assert t.dtype == torch.bfloat16, t.dtype
    return t


# --------------------------------------------------------------------------- GEMM
def gemm(layout, A, B, C, M, N, K, lda, ldb, ldc, bias=None, alpha=1.0, alpha_ncols=-1, resid=None, ldr=0,
         flags=0, batch=1, sA=0, sB=0, sC=0, sR=0, splitk=1):
    rc = lib().ifseg_gemm_bf16(c_int(layout), _ptr(A), _ptr(B), _ptr(C), c_int(M), c_int(N), c_int(K),
                               c_int(lda), c_int(ldb), c_int(ldc), _ptr(bias), c_float(alpha), c_int(alpha_ncols),
                               _ptr(resid), c_int(ldr), c_int(flags), c_int(batch), c_ll(sA), c_ll(sB), c_ll(sC),
                               c_ll(sR), c_int(splitk), _stream())
    _check(rc, "gemm")


def linear_fwd(x, w, bias=None, out=None, alpha=1.0, alpha_ncols=-1, resid=None):
    """out[M,N] = ((x[M,K] @ w[N,K]^T + bias) * alpha) + resid   (bf16)"""
    M, K = x.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty(M, N, dtype=torch.bfloat16, device=x.device)
    gemm(GEMM_NT, _bf(x), _bf(w), out, M, N, K, x.stride(0), w.stride(0), out.stride(0), bias, alpha, alpha_ncols,
         resid, resid.stride(0) if resid is not None else 0)
    return out


def linear_dx(dy, w, out=None, resid=None, accumulate=False):
    """dx[M,K] = dy[M,N] @ w[N,K]  (+ resid)"""
    M, N = dy.shape
    K = w.shape[1]
    if out is None:
        out = torch.empty(M, K, dtype=torch.bfloat16, device=dy.device)
    gemm(GEMM_NN, _bf(dy), _bf(w), out, M, K, N, dy.stride(0), w.stride(0), out.stride(0), None, 1.0, -1, resid,
         resid.stride(0) if resid is not None else 0, GEMM_ACCUMULATE if accumulate else 0)
    return out


def linear_dx_rowdot(dy, w, out, dot, dot_out, rows_per_batch):
    """dx[M,K] = dy[M,N] @ w[N,K] and dot_out[b, h, t] = sum_c dx[b*T+t, 64h+c] * dot[b*T+t, 64h+c] (attention delta)"""
    M, N = dy.shape
    K = w.shape[1]
    rc = lib().ifseg_gemm_nn_rowdot(_ptr(_bf(dy)), _ptr(_bf(w)), _ptr(out), c_int(M), c_int(K), c_int(N), c_int(dy.stride(0)),
                                    c_int(w.stride(0)), c_int(out.stride(0)), _ptr(dot), c_int(dot.stride(0)), _ptr(dot_out),
                                    c_int(rows_per_batch), _stream())
    _check(rc, "gemm_nn_rowdot")
    return out


def ffn_ln_coef(w2, gamma, beta, b2, coef):
    """coef fp32 [2, J]: row sums of W2 [J, N] against gamma / beta (+ b2) -- see include/ifseg_hip.h.  Lists of equally
    shaped tensors (one entry per layer, <= 32) go out in ONE launch."""
    if not isinstance(w2, (list, tuple)):
        w2, gamma, beta, b2, coef = [w2], [gamma], [beta], [b2], [coef]
    L = len(w2)
    J, N = w2[0].shape
    arr = lambda ts: (c_void_p * L)(*[t.data_ptr() for t in ts])
    _check(lib().ifseg_ffn_ln_coef(arr([_bf(t) for t in w2]), c_int(w2[0].stride(0)), arr(gamma), arr(beta), arr(b2), arr(coef),
                                   c_int(L), c_int(J), c_int(N), _stream()), "ffn_ln_coef")
    return coef


def ffn_ln_rowstats(dy, t, coef, c, N):
    """c fp32 [rows, 2]: the two row means of the ffn_layernorm backward from dY [rows, J] and the saved fc2 output t"""
    rows, J = dy.shape
    _check(lib().ifseg_ffn_ln_rowstats(_ptr(_bf(dy)), c_int(dy.stride(0)), _ptr(_bf(t)), c_int(t.stride(0)), _ptr(coef), _ptr(c),
                                       c_int(rows), c_int(J), c_int(N), _stream()), "ffn_ln_rowstats")
    return c


def linear_dx_gelu_ln_bwd(dy, w, out, u, gamma, mean, rstd, c):
    """du[M, N] = LayerNorm+GELU backward of dz = dy[M, K] @ w[K, N], in the GEMM epilogue (dz is not written)"""
    M, K = dy.shape
    N = w.shape[1]
    _check(lib().ifseg_gemm_nn_gelu_ln_bwd(_ptr(_bf(dy)), _ptr(_bf(w)), _ptr(out), c_int(M), c_int(N), c_int(K),
                                           c_int(dy.stride(0)), c_int(w.stride(0)), c_int(out.stride(0)), _ptr(_bf(u)),
                                           c_int(u.stride(0)), _ptr(gamma), _ptr(mean), _ptr(rstd), _ptr(c), _stream()),
           "gemm_nn_gelu_ln_bwd")
    return out


_pg_ws = {}


def ffn_ln_param_grads(w2, dw2, db2, gamma, beta, dgamma, dbeta, dy=None, u=None, mean=None, rstd=None):
    """dy [M, J], u [M, N], mean / rstd [M]: the operands of the rescue path for gains too small to divide by (csrc/ffn_ln.hip)"""
    J, N = w2.shape
    assert w2.is_contiguous() and dw2.is_contiguous()
    if J > 1024:
        # the rescue kernel stages one fc2.weight column (J values) in LDS: embed dims above 1024 (segofa_huge: 1280) run without
        # it -- a gain of exactly 0 then yields a zero gradient instead of the value from the definition
        if dy is not None and not _pg_ws.get("warned"):
            _pg_ws["warned"] = True
            import warnings
            warnings.warn("ifseg_amd: ffn_layernorm gradients run without the small-gain rescue path for embed dims above 1024 "
                          "(J = %d): a gain of exactly 0 yields a zero gradient there" % J)
        dy = None
    ws = _pg_ws.get((w2.device, N))
    if ws is None:
        ws = _pg_ws[(w2.device, N)] = torch.empty(16 * N, dtype=torch.float32, device=w2.device)
    _check(lib().ifseg_ffn_ln_param_grads(_ptr(_bf(w2)), _ptr(_bf(dw2)), _ptr(_bf(db2)), _ptr(gamma), _ptr(beta), _ptr(dgamma),
                                          _ptr(dbeta), _ptr(ws), c_int(J), c_int(N),
                                          _ptr(_bf(dy)) if dy is not None else None, c_int(dy.stride(0) if dy is not None else 0),
                                          _ptr(_bf(u)) if u is not None else None, c_int(u.stride(0) if u is not None else 0),
                                          _ptr(mean), _ptr(rstd), c_int(dy.shape[0] if dy is not None else 0), _stream()),
           "ffn_ln_param_grads")


_splitk_ws = {}


# workgroups a dW GEMM is split over: it runs on the side stream next to the dX chain, so filling the chip alone is not
# the goal (256 / 512 / 128 measured within 1% of each other; fewer slabs = less fp32 workspace traffic)
DW_TARGET_WGS = int(lab.get("DW_WGS", "256"))
# dW GEMMs with at least this many 128x128 tiles run without split-K (bf16 dW and db written once, no slabs, no
# reduction).  Off by default: measured on the Base step, 144-tile GEMMs that walk all 8480 tokens per workgroup make the
# weight-gradient stream lag (372-382 img/s vs 388 with split-K 2); the path is kept for models with wider layers.
DW_DIRECT_TILES = int(lab.get("DW_DIRECT", "1000000"))


def _db_follows(out, bias_out):
    """does db lie right behind dW in memory (a Linear's weight and bias in the gradient arena), in the same dtype?"""
    return (bias_out is not None and bias_out.dtype == out.dtype and bias_out.is_contiguous()
            and bias_out.data_ptr() == out.data_ptr() + out.numel() * out.element_size())


def linear_dw(dy, x, out, accumulate=False, bias_out=None):
    """dw[N,K] = dy[M,N]^T @ x[M,K]   (out bf16 or fp32 decided by out.dtype); with ``bias_out`` also
    db[N] = colsum(dy).  The reduction runs over the M tokens; with few output tiles it is split over
    workgroups (split-K into an fp32 workspace, then one reduction pass).  When ``bias_out`` sits right behind
    ``out`` in memory (a Linear's weight and bias in the gradient arena) the column sums ride on the same
    GEMM (one extra MFMA against an all-ones fragment) and the same reduction pass.
    Returns True if db was produced, False if the caller still has to compute it."""
    M, N = dy.shape
    K = x.shape[1]
    tiles = ((N + 127) // 128) * ((K + 127) // 128)
    splitk = max(1, min(16, DW_TARGET_WGS // max(1, tiles), M // 512))
    if M >= 4096:
        # k-slices pinned to XCDs (ifseg_gemm_bf16, TN): 8 slices for few-tile products, else 4 or 2; the count must divide
        # 8 and 8/splitk must divide the tile count
        for cand in (8, 4, 2):
            if tiles * cand <= max(DW_TARGET_WGS, 288) * (1 if cand == 8 else 2) and tiles % (8 // cand) == 0:
                splitk = cand
                break
    adjacent = N % 4 == 0 and out.is_contiguous() and _db_follows(out, bias_out)
    if tiles >= DW_DIRECT_TILES and out.dtype == torch.bfloat16 and out.is_contiguous():
        # enough tiles for a side-stream GEMM: one pass over all M tokens per workgroup, dW (and db) written once as bf16
        # -- no fp32 slabs, no reduction launch
        gemm(GEMM_TN, _bf(dy), _bf(x), out, N, K, M, dy.stride(0), x.stride(0), K,
             flags=(GEMM_ACCUMULATE if accumulate else 0) | (GEMM_COLSUM if adjacent else 0))
        return adjacent
    if bias_out is not None and M >= 1024:
        splitk = max(splitk, 2)      # the fused column sums ride on the split-K reduction
    if splitk > 1 and out.is_contiguous():
        kchunk = (((M + splitk - 1) // splitk) + 63) // 64 * 64
        nsl = (M + kchunk - 1) // kchunk
        fuse_b = N % 4 == 0 and _db_follows(out, bias_out)
        slab = N * K + (N if fuse_b else 0)
        ws = _splitk_ws.get(dy.device)
        if ws is None or ws.numel() < nsl * slab:
            ws = torch.empty(max(nsl * slab, 16 * (3072 * 768 + 3072)), dtype=torch.float32, device=dy.device)
            _splitk_ws[dy.device] = ws
        gemm(GEMM_TN, _bf(dy), _bf(x), ws, N, K, M, dy.stride(0), x.stride(0), K,
             flags=GEMM_OUT_F32 | (GEMM_COLSUM if fuse_b else 0), splitk=splitk)
        dst = out.as_strided((slab,), (1,)) if fuse_b else out       # dW followed by db, contiguous in the arena
        reduce_parts(ws, dst, 1, nsl, slab, accumulate=accumulate)
        return fuse_b
    flags = (GEMM_OUT_F32 if out.dtype == torch.float32 else 0) | (GEMM_ACCUMULATE if accumulate else 0)
    gemm(GEMM_TN, _bf(dy), _bf(x), out, N, K, M, dy.stride(0), x.stride(0), out.stride(0), flags=flags)
    return False


class _TnProblem(ctypes.Structure):
    _fields_ = [("A", c_void_p), ("B", c_void_p), ("C", c_void_p)] + [(n, c_int) for n in ("M", "N", "K", "lda", "ldb", "colsum", "accumulate")]


GEMM_GROUP_MAX = 8
DW_GROUP_WGS = int(lab.get("DW_GROUP_WGS", "512"))     # grid cap of the grouped dW GEMM: two workgroups per CU (in-step sweep, round 3: 256: 17.49, 384: 17.46, 512: 17.23 / 17.39, 768: 17.28, uncapped: 17.36 ms)


def dw_groupable(dy, x, out, bias_out):
    """can this dW = dy^T x (+ db) ride in a grouped launch?  bf16 dW contiguous in the arena, db right behind it"""
    if out.dtype != torch.bfloat16 or not out.is_contiguous() or dy.stride(1) != 1 or x.stride(1) != 1:
        return False
    if bias_out is not None and not _db_follows(out, bias_out):
        return False
    return dy.shape[1] % 8 == 0 and x.shape[1] % 8 == 0


def linear_dw_group(tasks, wgs=None):
    """tasks: list of (dy [M,N], x [M,K], out [N,K] bf16, bias_out or None[, accumulate]): every dW (+ db) in ONE launch
    (ifseg_gemm_tn_group), at most GEMM_GROUP_MAX per launch.  `wgs`: workgroup cap (default DW_GROUP_WGS; 0 = one workgroup per
    tile, for a launch with the GPU to itself).  The optional fifth element adds to what out / bias_out hold (the engine
    passes four: its grouped launches overwrite)"""
    for i in range(0, len(tasks), GEMM_GROUP_MAX):
        chunk = tasks[i:i + GEMM_GROUP_MAX]
        arr = (_TnProblem * len(chunk))()
        for q, (dy, x, out, bias_out, *acc) in zip(arr, chunk):
            M, N = dy.shape
            q.A, q.B, q.C = _p(_bf(dy)), _p(_bf(x)), _p(out)
            q.M, q.N, q.K, q.lda, q.ldb = N, x.shape[1], M, dy.stride(0), x.stride(0)
            q.colsum, q.accumulate = (1 if bias_out is not None else 0), (1 if acc and acc[0] else 0)
        _check(lib().ifseg_gemm_tn_group(c_int(len(chunk)), arr, c_int(DW_GROUP_WGS if wgs is None else wgs), _stream()), "gemm_tn_group")


def conv2d_nhwc(x, w, shift, resid, out, B, H, W, Cin, Cout, KH, KW, stride, pad, relu):
    rc = lib().ifseg_conv2d_nhwc_bf16(_ptr(x), _ptr(w), _ptr(shift), _ptr(resid), _ptr(out), c_int(B), c_int(H),
                                      c_int(W), c_int(Cin), c_int(Cout), c_int(KH), c_int(KW), c_int(stride),
                                      c_int(pad), c_int(1 if relu else 0), _stream())
    _check(rc, "conv2d_nhwc")
    return out


# ---------------------------------------------------------------------- attention
class RelBias:
    """Per-(layer) rel-pos bias operands of the attention kernels (all device tensors)."""

    def __init__(self, P, gcode, code_bias, rel2d, rel1d, relx, grid_w=0):
        self.P, self.gcode, self.code_bias, self.grid_w = P, gcode, code_bias, grid_w
        self.rel2d, self.rel1d, self.relx = rel2d, rel1d, relx   # fp32 [H,n2d], [H,2Lt-1], [H,2]


_F32_KEEP = []


def _f32(t):
    """[H] head gains are read as fp32 by the kernels; a bf16 tensor (tests) is converted (and kept alive until the next call)"""
    if t is None or t.dtype == torch.float32:
        return t
    c = t.float()
    _F32_KEEP[:] = [c]
    return c


class _AttnBwdArgs(ctypes.Structure):
    _fields_ = ([(n, c_void_p) for n in ("q", "k", "v", "pos_q", "pos_k", "out", "dout", "lse", "delta", "dq", "dk",
                                          "dv", "dpos_q_part", "dpos_k_part")]
                + [(n, c_int) for n in ("B", "H", "T", "S", "ldq", "ldk", "ldv", "ldpq", "ldpk", "ldout", "lddo",
                                        "lddq", "lddk", "lddv")]
                + [(n, c_ll) for n in ("q_bs", "k_bs", "v_bs", "out_bs", "do_bs", "dq_bs", "dk_bs", "dv_bs")]
                + [(n, c_int) for n in ("rel_mode", "P", "code_bias", "n2d", "causal", "nparts")]
                + [(n, c_void_p) for n in ("gcode", "rel2d", "rel1d", "relx", "gain", "drel2d_part", "drel1d_part",
                                           "drelx_part")]   # field order == ifseg_attn_bwd_args
                + [("dq_scale", c_float), ("dpq_scale", c_float), ("grid_w", c_int), ("phases", c_int), ("dgain_rows", c_void_p)])


def _p(t):
    return t.data_ptr() if t is not None else None


def _rel_fields(rel, P, S):
    """-> (rel_mode, P, gcode, code_bias, n2d, rel2d, rel1d, relx, grid_w) of the three entry points that take a RelBias:
    the grid size is the bias's, else the caller's P, else all S keys"""
    if rel is None:
        return 0, (S if P is None else P), None, 0, 0, None, None, None, 0
    return 1, rel.P, rel.gcode, rel.code_bias, rel.rel2d.shape[1], rel.rel2d, rel.rel1d, rel.relx, rel.grid_w


def attn_fwd(q, k, v, pos_q, pos_k, out, lse, B, H, T, S, rel=None, causal=False, P=None, dense_bias=None,
             gain=None):
    """q/k/v/out: [B, T|S, *] bf16 row-strided views (head h at cols h*64..); pos_q/pos_k: [T|S, H*64]."""
    rel_mode, P, gcode, code_bias, n2d, rel2d, rel1d, relx, grid_w = _rel_fields(rel, P, S)
    rc = lib().ifseg_attn_fwd(_ptr(q), _ptr(k), _ptr(v), _ptr(pos_q), _ptr(pos_k), _ptr(out), _ptr(lse), c_int(B),
                              c_int(H), c_int(T), c_int(S), c_int(q.stride(1)), c_int(k.stride(1)), c_int(v.stride(1)),
                              c_int(out.stride(1)), c_int(pos_q.stride(0) if pos_q is not None else 0),
                              c_int(pos_k.stride(0) if pos_k is not None else 0), c_ll(q.stride(0)), c_ll(k.stride(0)),
                              c_ll(v.stride(0)), c_ll(out.stride(0)), c_int(rel_mode), c_int(P), _ptr(gcode),
                              c_int(code_bias), c_int(n2d), _ptr(rel2d), _ptr(rel1d), _ptr(relx),
                              c_int(1 if causal else 0), _ptr(dense_bias), _ptr(_f32(gain)), c_int(grid_w),
                              c_int(dense_bias.stride(1) if dense_bias is not None else 0), _stream())
    _check(rc, "attn_fwd")
    return out


ATTN_BWD_DELTA, ATTN_BWD_DKV, ATTN_BWD_DQ = 1, 2, 4


def attn_bwd(q, k, v, pos_q, pos_k, out, dout, lse, delta, dq, dk, dv, dpq_part, dpk_part, B, H, T, S, rel=None,
             causal=False, P=None, gain=None, dq_scale=1.0, dpq_scale=1.0, drel2d_part=None, drel1d_part=None,
             drelx_part=None, nparts=0, phases=0, dgain_rows=None):
    a = _AttnBwdArgs()
    a.dgain_rows = _p(dgain_rows)
    assert all(t is None or t.dtype == torch.bfloat16 for t in (dpq_part, dpk_part)), "abs-pos partials are bf16"
    a.rel_mode, P, gcode, a.code_bias, a.n2d, rel2d, rel1d, relx, a.grid_w = _rel_fields(rel, P, S)
    for name, t in (("q", q), ("k", k), ("v", v), ("pos_q", pos_q), ("pos_k", pos_k), ("out", out), ("dout", dout),
                    ("lse", lse), ("delta", delta), ("dq", dq), ("dk", dk), ("dv", dv), ("dpos_q_part", dpq_part),
                    ("dpos_k_part", dpk_part), ("gain", _f32(gain)), ("drel2d_part", drel2d_part),
                    ("drel1d_part", drel1d_part), ("drelx_part", drelx_part), ("gcode", gcode), ("rel2d", rel2d),
                    ("rel1d", rel1d), ("relx", relx)):
        setattr(a, name, _p(t))
    a.B, a.H, a.T, a.S = B, H, T, S
    a.ldq, a.ldk, a.ldv = q.stride(1), k.stride(1), v.stride(1)
    a.ldpq = pos_q.stride(0) if pos_q is not None else 0
    a.ldpk = pos_k.stride(0) if pos_k is not None else 0
    a.ldout, a.lddo, a.lddq, a.lddk, a.lddv = out.stride(1), dout.stride(1), dq.stride(1), dk.stride(1), dv.stride(1)
    a.q_bs, a.k_bs, a.v_bs, a.out_bs = q.stride(0), k.stride(0), v.stride(0), out.stride(0)
    a.do_bs, a.dq_bs, a.dk_bs, a.dv_bs = dout.stride(0), dq.stride(0), dk.stride(0), dv.stride(0)
    a.P, a.causal, a.nparts = P, 1 if causal else 0, nparts
    a.dq_scale, a.dpq_scale = dq_scale, dpq_scale
    a.phases = phases
    rc = lib().ifseg_attn_bwd(ctypes.byref(a), _stream())
    _check(rc, "attn_bwd")


def attn_delta(out, dout, delta, B, H, T):
    """delta [B, H, T] fp32 = rowsum(dout * out) per head: the delta launch of ifseg_attn_bwd alone, for both kernel
    generations.  Only the fields that launch reads are filled; the others stay zero, which passes the entry point's checks."""
    a = _AttnBwdArgs()
    a.out, a.dout, a.delta = _p(out), _p(dout), _p(delta)
    a.B, a.H, a.T, a.S, a.P = B, H, T, T, T
    a.ldout, a.lddo, a.out_bs, a.do_bs = out.stride(1), dout.stride(1), out.stride(0), dout.stride(0)
    a.dq_scale, a.dpq_scale = 1.0, 1.0
    a.phases = ATTN_BWD_DELTA
    _check(lib().ifseg_attn_bwd(ctypes.byref(a), _stream()), "attn_bwd")


# ---- attention backward with the batch as a workgroup's inner dimension (csrc/attention_bi.hip)
def _pad32(n):
    return (n + 31) // 32 * 32


class DenseBias:
    """The batch-invariant attention bias of one layer as a dense bf16 operand D [H, Tp, Sp] (-inf = masked or padding),
    built from parameters only by ifseg_attn_dense_bias (fp32 arithmetic, one rounding)."""

    def __init__(self, H, T, S, device):
        self.H, self.T, self.S, self.Sp, self.Tp = H, T, S, _pad32(S), _pad32(T)
        self.D = torch.empty(H, self.Tp, self.Sp, dtype=torch.bfloat16, device=device)


def attn_dense_bias(dense, pos_q, pos_k, rel=None, causal=False, P=None):
    rel_mode, P, gcode, code_bias, n2d, rel2d, rel1d, relx, _ = _rel_fields(rel, P, dense.S)
    rc = lib().ifseg_attn_dense_bias(
        _ptr(pos_q), _ptr(pos_k), c_int(pos_q.stride(0) if pos_q is not None else 0),
        c_int(pos_k.stride(0) if pos_k is not None else 0), c_int(dense.H), c_int(dense.T), c_int(dense.S),
        c_int(rel_mode), c_int(P), _ptr(gcode), c_int(code_bias), c_int(n2d), _ptr(rel2d), _ptr(rel1d), _ptr(relx),
        c_int(1 if causal else 0), _ptr(dense.D), c_int(dense.Sp), c_int(dense.Tp), _stream())
    _check(rc, "attn_dense_bias")
    return dense


class _AttnBiArgs(ctypes.Structure):
    _fields_ = ([(n, c_void_p) for n in ("q", "k", "v", "dout", "lse", "delta", "D", "gain", "dq", "dk", "dv", "dbias")]
                + [(n, c_int) for n in ("B", "H", "T", "S", "Sp", "Tp", "ldq", "ldk", "ldv", "lddo", "lddq", "lddk", "lddv")]
                + [(n, c_ll) for n in ("q_bs", "k_bs", "v_bs", "do_bs", "dq_bs", "dk_bs", "dv_bs")]
                + [("causal", c_int), ("P", c_int), ("dq_scale", c_float), ("phases", c_int), ("dgain_rows", c_void_p),
                   ("out", c_void_p), ("ldout", c_int), ("out_bs", c_ll), ("kv_len", c_void_p), ("drop_p", c_float),
                   ("drop_seed", ctypes.c_uint64), ("drop_seed_add", c_void_p)])   # == ifseg_attn_bi_args


def _attn_drop(a, drop):
    """drop = (p, seed) or None: attention dropout of the batch-inner kernels (the per-update seed word is the global seed_add)"""
    if drop is not None and drop[0] > 0:
        a.drop_p, a.drop_seed, a.drop_seed_add = float(drop[0]), drop[1] & 0xFFFFFFFFFFFFFFFF, _seed_add_ptr()


def attn_dropout_mask(B, H, T, S, p, seed, device):
    """uint8 [B, H, T, S]: the keep mask the attention kernels apply for (p, seed) and the current seed_add"""
    out = torch.empty(B, H, T, S, dtype=torch.uint8, device=device)
    _check(lib().ifseg_attn_dropout_mask(_ptr(out), c_int(B), c_int(H), c_int(T), c_int(S), c_float(p),
                                         ctypes.c_uint64(seed & 0xFFFFFFFFFFFFFFFF), c_void_p(_seed_add_ptr()), _stream()), "attn_dropout_mask")
    return out


def _kvlen(kv_len, B):
    if kv_len is None:
        return None
    assert kv_len.dtype == torch.int32 and kv_len.is_cuda and kv_len.numel() == B and kv_len.is_contiguous()
    return kv_len


def _bi_args(q, k, v, dense, B, H, T, S, causal, P, gain, kv_len, drop):
    """the fields the two batch-inner entry points share"""
    a = _AttnBiArgs()
    a.q, a.k, a.v, a.D, a.gain = _p(q), _p(k), _p(v), _p(dense.D), _p(_f32(gain))
    a.B, a.H, a.T, a.S, a.Sp, a.Tp = B, H, T, S, dense.Sp, dense.Tp
    a.ldq, a.ldk, a.ldv = q.stride(1), k.stride(1), v.stride(1)
    a.q_bs, a.k_bs, a.v_bs = q.stride(0), k.stride(0), v.stride(0)
    a.causal, a.P = (1 if causal else 0), (P if P is not None else S)
    a.kv_len = _p(_kvlen(kv_len, B))
    _attn_drop(a, drop)
    return a


def attn_bwd_bi(q, k, v, dout, lse, delta, dense, dq, dk, dv, dbias, B, H, T, S, causal=False, P=None, gain=None,
                dq_scale=1.0, phases=0, dgain_rows=None, kv_len=None, drop=None):
    """dbias: bf16 [ceil(B/4), H, T, dense.Sp] -- zero-filled once by the caller when causal (skipped blocks are not written);
    kv_len: int32 [B] valid key counts (key padding), None = no padding"""
    a = _bi_args(q, k, v, dense, B, H, T, S, causal, P, gain, kv_len, drop)
    a.dout, a.lse, a.delta = _p(dout), _p(lse), _p(delta)
    a.dq, a.dk, a.dv, a.dbias = _p(dq), _p(dk), _p(dv), _p(dbias)
    assert dbias.dtype == torch.bfloat16 and tuple(dbias.shape) == ((B + 3) // 4, H, T, dense.Sp) and dbias.is_contiguous()
    a.lddo, a.lddq, a.lddk, a.lddv = dout.stride(1), dq.stride(1), dk.stride(1), dv.stride(1)
    a.do_bs, a.dq_bs, a.dk_bs, a.dv_bs = dout.stride(0), dq.stride(0), dk.stride(0), dv.stride(0)
    a.dq_scale, a.phases = dq_scale, phases
    a.dgain_rows = _p(dgain_rows)
    _check(lib().ifseg_attn_bwd_bi(ctypes.byref(a), _stream()), "attn_bwd_bi")


def dbias_nparts():
    return lib().ifseg_attn_dbias_nparts()


def attn_fwd_bi(q, k, v, dense, out, lse, B, H, T, S, causal=False, P=None, gain=None, kv_len=None, drop=None):
    """out = gain softmax(q k^T + dense.D) v, four batch elements per workgroup (csrc/attention_bi.hip)"""
    a = _bi_args(q, k, v, dense, B, H, T, S, causal, P, gain, kv_len, drop)
    a.lse, a.out, a.ldout, a.out_bs = _p(lse), _p(out), out.stride(1), out.stride(0)
    _check(lib().ifseg_attn_fwd_bi(ctypes.byref(a), _stream()), "attn_fwd_bi")
    return out


class _AttnDbiasArgs(ctypes.Structure):
    _fields_ = [("dbias", c_void_p), ("ng", c_int), ("H", c_int), ("T", c_int), ("S", c_int), ("Sp", c_int), ("C", c_int),
                ("pos_q", c_void_p), ("pos_k", c_void_p), ("ldpq", c_int), ("ldpk", c_int),
                ("dpos_q_acc", c_void_p), ("dpos_k_acc", c_void_p), ("accumulate_pos", c_int), ("dpq_scale", c_float),
                ("P", c_int), ("grid_h", c_int), ("grid_w", c_int),
                ("drel2d", c_void_p), ("drel1d", c_void_p), ("drelx", c_void_p), ("causal", c_int)]     # == ifseg_attn_dbias_args


def attn_dbias_grads(dbias, S, pos_q=None, pos_k=None, dpq_acc=None, dpk_acc=None, accumulate_pos=False, dpq_scale=1.0,
                     P=0, grid_h=0, grid_w=0, drel2d=None, drel1d=None, drelx=None, causal=False):
    """dbias [ng, H, T, Sp] bf16 -> abs-pos operand gradients (fp32 [T, C] / [S, C]) and delta-table gradients as
    NP = dbias_nparts() partial tables per head (fp32 [H, NP, (2gh-1)(2gw-1)], [H, NP, 2Lt-1], [H, NP, 2]) in one launch"""
    if drel2d is not None:
        assert all(t.shape[1] == dbias_nparts() and t.is_contiguous() for t in (drel2d, drel1d, drelx))
    a = _AttnDbiasArgs()
    ng, H, T, Sp = dbias.shape
    a.dbias, a.ng, a.H, a.T, a.S, a.Sp = _p(dbias), ng, H, T, S, Sp
    a.C = dpq_acc.shape[1] if dpq_acc is not None else 0
    a.pos_q, a.pos_k = _p(pos_q), _p(pos_k)
    a.ldpq = pos_q.stride(0) if pos_q is not None else 0
    a.ldpk = pos_k.stride(0) if pos_k is not None else 0
    a.dpos_q_acc, a.dpos_k_acc = _p(dpq_acc), _p(dpk_acc)
    a.accumulate_pos, a.dpq_scale = (1 if accumulate_pos else 0), dpq_scale
    a.P, a.grid_h, a.grid_w = P, grid_h, grid_w
    a.drel2d, a.drel1d, a.drelx = _p(drel2d), _p(drel1d), _p(drelx)
    a.causal = 1 if causal else 0
    _check(lib().ifseg_attn_dbias_grads(ctypes.byref(a), _stream()), "attn_dbias_grads")


# ---- attention with a bias the caller computed (csrc/attention_ops.hip)
def attn_bias_pack(dense, bias, causal=False, P=None):
    """dense.D = the operand of attn_fwd_bi / attn_bwd_bi for an ordinary bias tensor: bf16(bias) on [:, :T, :S], -inf on the
    padding and (causal) on the pairs attn_dense_bias masks; every element is written.  bias: fp32 / bf16 [H, T, S] with a
    contiguous last dimension (any head / row strides), or None for a zero bias"""
    f32, hs, rs = 0, 0, 0
    if bias is not None:
        assert bias.dtype in (torch.float32, torch.bfloat16) and tuple(bias.shape) == (dense.H, dense.T, dense.S), "bias: fp32 / bf16 [H, T, S]"
        assert bias.stride(2) == 1 or dense.S == 1, "bias: the last dimension must be contiguous"
        f32, hs, rs = int(bias.dtype == torch.float32), bias.stride(0), bias.stride(1)
    _check(lib().ifseg_attn_bias_pack(_ptr(bias), c_int(f32), c_ll(hs), c_ll(rs), c_int(dense.H), c_int(dense.T),
                                      c_int(dense.S), c_int(1 if causal else 0), c_int(P if P is not None else dense.S),
                                      _ptr(dense.D), c_int(dense.Sp), c_int(dense.Tp), _stream()), "attn_bias_pack")
    return dense


def attn_dbias_sum(dbias, S, out):
    """out [H, T, S] (fp32 / bf16, contiguous last dimension) = the sum over the slabs of dbias [ng, H, T, Sp] (bf16, as
    attn_bwd_bi writes them), in fp32 and in slab order"""
    ng, H, T, Sp = dbias.shape
    assert dbias.dtype == torch.bfloat16 and dbias.is_contiguous()
    assert out.dtype in (torch.float32, torch.bfloat16) and tuple(out.shape) == (H, T, S) and (out.stride(2) == 1 or S == 1)
    _check(lib().ifseg_attn_dbias_sum(_ptr(dbias), c_int(ng), c_int(H), c_int(T), c_int(S), c_int(Sp), _ptr(out),
                                      c_int(int(out.dtype == torch.float32)), c_ll(out.stride(0)), c_ll(out.stride(1)),
                                      _stream()), "attn_dbias_sum")
    return out


# ------------------------------------------------------------------------ row ops
def _map(t, rpb):
    """(bs, ld) of a [rows, C] or [B, rpb, C] view"""
    if t is None:
        return 0, 0
    if t.dim() == 3:
        return t.stride(0), t.stride(1)
    return 0, t.stride(0)


class _DropArgs(ctypes.Structure):
    _fields_ = [("p", c_float), ("seed", ctypes.c_ulonglong), ("drop_path_scale", c_void_p), ("rows_per_batch", c_int),
                ("seed_add", c_void_p)]


_seed_add = [None]


def set_seed_add(t):
    """device int64 / uint64 word added to every dropout / DropPath seed (the per-update part of the seed: the engine
    keeps it in device memory so that a captured step draws new masks on every replay); None: seeds are used as given"""
    prev = _seed_add[0]
    _seed_add[0] = t
    return prev


def _seed_add_ptr():
    t = _seed_add[0]
    return t.data_ptr() if t is not None else None


def _drop_ref(drop, rows):
    """drop = (p, seed, drop_path_scale tensor or None, rows_per_batch or None) -> byref(ifseg_drop_args) / None"""
    if drop is None:
        return None
    p, seed, dps, rpb = drop
    return ctypes.byref(_DropArgs(p, seed & 0xFFFFFFFFFFFFFFFF, dps.data_ptr() if dps is not None else None, rpb or rows,
                                  _seed_add_ptr()))


def _ln_flags(gamma, gelu=False, other=None):
    """IFSEG_LN_GELU | IFSEG_LN_PARAMS_F32 (gains / biases given as fp32 tensors: the master copy)"""
    f32 = gamma is not None and gamma.dtype == torch.float32
    if other is not None and gamma is not None:
        assert (other.dtype == torch.float32) == f32
    elif other is not None:
        f32 = other.dtype == torch.float32
    return (1 if gelu else 0) | (2 if f32 else 0)


def _ln_geom(x, *tensors):
    """(rows, C, rpb) of x, [rows, C] or [B, rpb, C], and the flattened (c_ll(bs), c_int(ld)) pairs of `tensors` in order"""
    C = x.shape[-1]
    rpb = x.shape[1] if x.dim() == 3 else 0
    maps = []
    for t in tensors:
        bs, ld = _map(t, rpb)
        maps += [c_ll(bs), c_int(ld)]
    return x.numel() // C, C, rpb, maps


def ln_fwd(x, gamma, beta, y, mean=None, rstd=None, resid=None, gelu=False, eps=1e-5, drop=None):
    """x, y, resid: [rows, C] or [B, rpb, C] (strided views allowed, last dim contiguous).
    drop: fused dropout/DropPath of the normalised output before the residual add (see _drop_ref)."""
    rows, C, rpb, maps = _ln_geom(x, x, y, resid)
    rc = lib().ifseg_ln_fwd(_ptr(x), _ptr(gamma), _ptr(beta), _ptr(resid), _ptr(y), _ptr(mean), _ptr(rstd),
                            c_int(rows), c_int(C), c_float(eps), c_int(_ln_flags(gamma, gelu)), c_int(rpb), *maps,
                            _drop_ref(drop, rpb or rows), _stream())
    _check(rc, "ln_fwd")
    return y


def ln_fwd_pair(x, gamma, beta, y, mean, rstd, gamma2, beta2, y2, mean2, rstd2, resid=None, eps=1e-5, drop=None):
    """y = [resid +] drop(LN(x)), y2 = LN2(y): the post-LN of a block and the pre-LN of the next in one launch"""
    rows, C, rpb, maps = _ln_geom(x, x, y, resid, y2)
    rc = lib().ifseg_ln_fwd_pair(_ptr(x), _ptr(gamma), _ptr(beta), _ptr(resid), _ptr(y), _ptr(mean), _ptr(rstd), _ptr(gamma2),
                                 _ptr(beta2), _ptr(y2), _ptr(mean2), _ptr(rstd2), c_int(rows), c_int(C), c_float(eps),
                                 c_int(_ln_flags(gamma, False, gamma2)), c_int(rpb), *maps, _drop_ref(drop, rpb or rows), _stream())
    _check(rc, "ln_fwd_pair")
    return y, y2


LN_BWD_BLOCKS = int(lab.get("LN_BWD_BLOCKS", "768"))   # three resident blocks per CU (146-162 VGPRs): best of a 256..2048 sweep on MI355X


def ln_bwd_drop(dy, x, gamma, mean, rstd, dx, dgamma_part, dbeta_part, dx2, dx_add=None, drop2=None):
    """dx = [dx_add +] LN'(x; gamma)(dy) and dx2 = drop2(dx): the pre-LN backward that closes a block of the backward and the
    fc2-dropout adjoint that opens the next one in one launch"""
    rows, C, rpb, maps = _ln_geom(x, dy, x, dx, dx_add, dx2)
    rc = lib().ifseg_ln_bwd_drop(_ptr(dy), _ptr(x), _ptr(gamma), _ptr(mean), _ptr(rstd), _ptr(dx_add), _ptr(dx),
                                 _ptr(dgamma_part), _ptr(dbeta_part), _ptr(dx2), c_int(LN_BWD_BLOCKS), c_int(rows), c_int(C),
                                 c_int(_ln_flags(gamma)), c_int(rpb), *maps, _drop_ref(drop2, rpb or rows), _stream())
    _check(rc, "ln_bwd_drop")
    return dx, dx2


def ln_bwd(dy, x, gamma, mean, rstd, dx, dgamma_part, dbeta_part, dx_add=None, gelu=False, drop=None):
    rows, C, rpb, maps = _ln_geom(x, dy, x, dx, dx_add)
    rc = lib().ifseg_ln_bwd(_ptr(dy), _ptr(x), _ptr(gamma), _ptr(mean), _ptr(rstd), _ptr(dx_add), _ptr(dx),
                            _ptr(dgamma_part), _ptr(dbeta_part), c_int(LN_BWD_BLOCKS), c_int(rows), c_int(C),
                            c_int(_ln_flags(gamma, gelu)), c_int(rpb), *maps, _drop_ref(drop, rpb or rows), _stream())
    _check(rc, "ln_bwd")
    return dx


CHECK_ANY_EQ, CHECK_SUFFIX, CHECK_ANY_ZERO_BYTE, CHECK_FLAG = 0, 1, 2, 3


def check_inputs(x, mode, verdict_pinned, slot, value=0, row_len=1):
    """one-launch input validation (ifseg_check_inputs): verdict_pinned[slot] <- 0 / 1 in stream order"""
    n = 1 if mode == CHECK_FLAG else x.numel()
    _check(lib().ifseg_check_inputs(_ptr(x), c_ll(n), c_int(mode), c_ll(value), c_ll(row_len),
                                    c_void_p(verdict_pinned.data_ptr() + slot), _stream()), "check_inputs")


def reduce_parts(inp, out, outer, parts, n, accumulate=False, scale=1.0):
    rc = lib().ifseg_reduce_parts(_ptr(inp), _ptr(out), c_int(outer), c_int(parts), c_ll(n),
                                  c_int(1 if accumulate else 0), c_int(1 if out.dtype == torch.bfloat16 else 0),
                                  c_float(scale), _stream())
    _check(rc, "reduce_parts")
    return out


class _ReduceTask(ctypes.Structure):
    _fields_ = [("inp", c_void_p), ("out", c_void_p), ("outer", c_int), ("parts", c_int), ("n", c_ll),
                ("accumulate", c_int), ("out_bf16", c_int), ("scale", c_float)]


def reduce_parts_multi(tasks):
    """tasks: list of (inp, out, outer, parts, n, accumulate) -- ifseg_reduce_parts for each, 16 per launch"""
    for i in range(0, len(tasks), 16):
        chunk = tasks[i:i + 16]
        arr = (_ReduceTask * len(chunk))()
        for q, (inp, out, outer, parts, n, accumulate) in zip(arr, chunk):
            q.inp, q.out, q.outer, q.parts, q.n = _p(inp), _p(out), outer, parts, n
            q.accumulate, q.out_bf16, q.scale = (1 if accumulate else 0), (1 if out.dtype == torch.bfloat16 else 0), 1.0
        _check(lib().ifseg_reduce_parts_multi(c_int(len(chunk)), arr, _stream()), "reduce_parts_multi")


COLSUM_BLOCKS = 256


def colsum(x, part):
    """x [M,N] (or [B,rpb,N]) bf16 -> part [COLSUM_BLOCKS, N] fp32 partial column sums"""
    N = x.shape[-1]
    M = x.numel() // N
    rpb = x.shape[1] if x.dim() == 3 else 0
    xb, xl = _map(x, rpb)
    rc = lib().ifseg_colsum_bf16(_ptr(x), _ptr(part), c_int(COLSUM_BLOCKS), c_int(M), c_int(N), c_int(rpb), c_ll(xb),
                                 c_int(xl), _stream())
    _check(rc, "colsum")
    return part


def col_mean(x, ws=None, every=1):
    """fp32 [C] column means of x [rows, C] bf16 (two launches: partial column sums, their sum); ws: a
    [COLSUM_BLOCKS + 1, C] fp32 workspace whose last row receives the result; every > 1: the mean over every `every`-th row"""
    C = x.shape[-1]
    if ws is None:
        ws = torch.empty(COLSUM_BLOCKS + 1, C, dtype=torch.float32, device=x.device)
    rows = x.numel() // C
    if every > 1 and x.dim() == 2 and x.is_contiguous() and rows >= 64 * every:
        x = x[: rows // every * every].view(rows // every, every * C)[:, :C]       # every `every`-th row (row stride every * C)
        rows = rows // every
    colsum(x, ws[:COLSUM_BLOCKS])
    reduce_parts(ws[:COLSUM_BLOCKS], ws[COLSUM_BLOCKS], 1, COLSUM_BLOCKS, C, scale=1.0 / rows)
    return ws[COLSUM_BLOCKS]


def kproj_common_mode(gw, db, xmean):
    """gw [N, C] -= db [N] (x) xmean [C]: the key-projection weight gradient without the product of dK's spurious column sum
    and the token-common component of its input (csrc/rowops.hip: ifseg_kproj_common_mode; xmean = col_mean(x))"""
    N, C = gw.shape
    assert gw.is_contiguous() and gw.dtype == torch.bfloat16 and db.dtype == torch.bfloat16 and db.is_contiguous()
    assert xmean.dtype == torch.float32 and xmean.numel() == C
    _check(lib().ifseg_kproj_common_mode(_ptr(gw), _ptr(db), _ptr(xmean), c_int(N), c_int(C), _stream()), "kproj_common_mode")


def embed_bag_mean(table, ids, ends, add, out):
    """table [V,C] bf16; ids int64 [B,maxlen]; ends int64 [B,P] (per-sample cumulative bag ends); add [C] bf16 or None;
    out [B*P, C] or [B, P, C] bf16 view"""
    B, maxlen = ids.shape
    P = ends.numel() // B
    C = table.shape[1]
    rpb = out.shape[1] if out.dim() == 3 else 0
    ob, ol = _map(out, rpb)
    assert ids.dtype == torch.int64 and ends.dtype == torch.int64 and ids.is_contiguous() and ends.is_contiguous()
    rc = lib().ifseg_embed_bag_mean(_ptr(table), _ptr(ids), _ptr(ends), _ptr(add), _ptr(out), c_int(B), c_int(P), c_int(C),
                                    c_int(maxlen), c_int(rpb), c_ll(ob), c_int(ol), _stream())
    _check(rc, "embed_bag_mean")
    return out


def imfree_draw(seed, first_ordinal, B, l, r, nseg, shapes, coarse):
    """shapes int32 [B, 2], coarse int32 [B, (r-1)^2] <- the artificial images of sample ordinals first_ordinal + b
    (csrc/imfree.hip); first_ordinal: a python int, or a device int64 word (read at execution time: graph replays)"""
    assert shapes.dtype == torch.int32 and coarse.dtype == torch.int32 and shapes.is_contiguous() and coarse.is_contiguous()
    assert tuple(shapes.shape) == (B, 2) and tuple(coarse.shape) == (B, (r - 1) * (r - 1))
    word = first_ordinal if isinstance(first_ordinal, torch.Tensor) else None
    if word is not None:
        assert word.dtype == torch.int64 and word.numel() == 1
    rc = lib().ifseg_imfree_draw(_seed64(seed), c_ll(0 if word is not None else int(first_ordinal)),
                                 _ptr(word), c_int(B), c_int(l), c_int(r), c_int(nseg), _ptr(shapes), _ptr(coarse), _stream())
    _check(rc, "imfree_draw")
    return shapes, coarse


def imfree_expand(shapes, coarse, name_ids, name_len, hp, wp, seg_id_offset, bos, eos, pad, ids, ends, prev, target):
    """the collater layout of the artificial images (csrc/imfree.hip): coarse int32 [B, max_side^2] -> ids int64 [B, P*Lmax],
    ends int64 [B*P], prev int64 [B, P+1], target int64 [B, 256*P + 1]"""
    B, P = shapes.shape[0], hp * wp
    nseg, Lmax = name_ids.shape[0] - 1, name_ids.shape[1]
    max_side = int(round(coarse.shape[1] ** 0.5))
    assert shapes.dtype == torch.int32 and coarse.dtype == torch.int32 and shapes.is_contiguous() and coarse.is_contiguous()
    assert tuple(shapes.shape) == (B, 2) and tuple(coarse.shape) == (B, max_side * max_side)
    assert name_ids.dtype == torch.int64 and name_len.dtype == torch.int32 and name_ids.is_contiguous() and name_len.is_contiguous()
    assert name_len.numel() == nseg + 1
    for t, n in ((ids, B * P * Lmax), (ends, B * P), (prev, B * (P + 1)), (target, B * (256 * P + 1))):
        assert t.dtype == torch.int64 and t.is_contiguous() and t.numel() == n, (tuple(t.shape), n)
    rc = lib().ifseg_imfree_expand(_ptr(shapes), _ptr(coarse), c_int(max_side), _ptr(name_ids), _ptr(name_len), c_int(nseg),
                                   c_int(Lmax), c_int(B), c_int(hp), c_int(wp), c_ll(seg_id_offset), c_ll(bos), c_ll(eos), c_ll(pad),
                                   _ptr(ids), _ptr(ends), _ptr(prev), _ptr(target), _stream())
    _check(rc, "imfree_expand")


def embed_rows(table, ids, add, out):
    C = table.shape[1]
    n = ids.numel()
    rpb = out.shape[1] if out.dim() == 3 else 0
    ob, ol = _map(out, rpb)
    rc = lib().ifseg_embed_rows(_ptr(table), _ptr(ids), _ptr(add), _ptr(out), c_int(n), c_int(C), c_int(rpb),
                                c_ll(ob), c_int(ol), _stream())
    _check(rc, "embed_rows")
    return out


def rows_segment_sum(src, src_row, weight, sorted_ids, table_grad, skip_id=-1):
    """table_grad[sorted_ids[j]] += weight[j] * src[src_row[j]] over runs of equal (sorted) ids; see csrc/rowops.hip"""
    C = src.shape[-1]
    assert src.is_contiguous() and table_grad.is_contiguous() and table_grad.shape[1] == C
    assert src_row.dtype == torch.int64 and sorted_ids.dtype == torch.int64 and (weight is None or weight.dtype == torch.float32)
    _check(lib().ifseg_rows_segment_sum(_ptr(src), _ptr(src_row), _ptr(weight), _ptr(sorted_ids), _ptr(table_grad),
                                        c_ll(sorted_ids.numel()), c_int(C), c_ll(table_grad.shape[0]), c_ll(skip_id), _stream()),
           "rows_segment_sum")


def sync_master(master, p16):
    _check(lib().ifseg_sync_master(_ptr(master), _ptr(p16), c_ll(master.numel()), _stream()), "sync_master")


def cast_f32_bf16(x, out, scale=1.0):
    _check(lib().ifseg_cast_f32_bf16(_ptr(x), _ptr(out), c_ll(x.numel()), c_float(scale), _stream()), "cast")
    return out


def add_bf16(a, b, out):
    _check(lib().ifseg_add_bf16(_ptr(a), _ptr(b), _ptr(out), c_ll(a.numel()), _stream()), "add")
    return out


def nchw_to_nhwc(x, out, Cpad):
    B, C, H, W = x.shape
    _check(lib().ifseg_nchw_to_nhwc_bf16(_ptr(x), c_int(1 if x.dtype == torch.float32 else 0), _ptr(out), c_int(B),
                                         c_int(C), c_int(H), c_int(W), c_int(Cpad), _stream()), "nchw_to_nhwc")
    return out


def stem_weights_mfma(w):
    """fp32 [7][7][3][64] (BN scale folded) -> bf16 [3][64][224] for ifseg_stem_conv7x7_mfma: k = ky*32 + kx*4 + ci, three bf16
    terms whose sum is the fp32 weight"""
    wt = torch.zeros(64, 7, 8, 4, dtype=torch.float32, device=w.device)
    wt[:, :, :7, :3] = w.permute(3, 0, 1, 2)
    wt = wt.reshape(64, 224)
    t0 = wt.to(torch.bfloat16)
    t1 = (wt - t0.float()).to(torch.bfloat16)
    t2 = (wt - t0.float() - t1.float()).to(torch.bfloat16)
    return torch.stack([t0, t1, t2]).contiguous()


def stem_conv(x4, w, shift, out, B, H, W):
    """w: fp32 [7][7][3][64] (direct kernel) or bf16 [3][64][224] from stem_weights_mfma (matrix cores)"""
    if w.dtype == torch.bfloat16:
        assert tuple(w.shape) == (3, 64, 224) and w.is_contiguous()
        _check(lib().ifseg_stem_conv7x7_mfma(_ptr(x4), _ptr(w), _ptr(shift), _ptr(out), c_int(B), c_int(H), c_int(W),
                                             _stream()), "stem_conv_mfma")
        return out
    _check(lib().ifseg_stem_conv7x7(_ptr(x4), _ptr(w), _ptr(shift), _ptr(out), c_int(B), c_int(H), c_int(W),
                                    _stream()), "stem_conv")
    return out


def maxpool(x, out, B, H, W, C):
    _check(lib().ifseg_maxpool3x3s2(_ptr(x), _ptr(out), c_int(B), c_int(H), c_int(W), c_int(C), _stream()), "maxpool")
    return out


def grad_sumsq(g, workspace, out):
    _check(lib().ifseg_grad_sumsq_bf16(_ptr(g), c_ll(g.numel()), _ptr(workspace), _ptr(out), _stream()), "sumsq")
    return out


def droppath_scale(out, keep, seed):
    """out fp32 [n, B] = Bernoulli(keep[i]) / keep[i]"""
    n, B = out.shape
    _check(lib().ifseg_droppath_scale(_ptr(out), _ptr(keep), c_int(n), c_int(B), ctypes.c_ulonglong(seed & 0xFFFFFFFFFFFFFFFF),
                                      c_void_p(_seed_add_ptr()), _stream()), "droppath_scale")


def adam_step(p32, g, m, v, p16, lr, beta1, beta2, eps, wd, step, grad_scale=1.0, max_norm=0.0, sumsq=None, overflow=None,
              hyper=None):
    _check(lib().ifseg_adam_step(_ptr(p32), _ptr(g), _ptr(m), _ptr(v), _ptr(p16), c_ll(p32.numel()), c_float(lr),
                                 c_float(beta1), c_float(beta2), c_float(eps), c_float(wd), c_int(step),
                                 c_float(grad_scale), c_float(max_norm), _ptr(sumsq), _ptr(overflow), _ptr(hyper), _stream()), "adam")


def adam_ema_step(p32, g, m, v, p16, e32, e16, lr, beta1, beta2, eps, wd, step, ema_decay, ema_rest, grad_scale=1.0,
                  max_norm=0.0, sumsq=None, overflow=None, hyper=None):
    """`adam_step` with the teacher (e32 fp32, e16 bf16) stepped towards the new bf16 weights in the same launch
    (ifseg_amd/ema.py: e32 = fma(ema_rest, p16, round32(e32 * ema_decay))); `hyper` has six floats here, the last two
    override (ema_decay, ema_rest); (1, 0) leaves the teacher alone"""
    from .ema import check_arenas
    check_arenas("adam_ema_step", p32, p16, e32, e16)
    if hyper is not None and hyper.numel() < 6:
        raise ValueError("adam_ema_step: hyper needs six floats, got %d" % hyper.numel())
    _check(lib().ifseg_adam_ema_step(_ptr(p32), _ptr(g), _ptr(m), _ptr(v), _ptr(p16), _ptr(e32), _ptr(e16), c_ll(p32.numel()),
                                     c_float(lr), c_float(beta1), c_float(beta2), c_float(eps), c_float(wd), c_int(step),
                                     c_float(grad_scale), c_float(max_norm), _ptr(sumsq), _ptr(overflow), _ptr(hyper),
                                     c_float(ema_decay), c_float(ema_rest), _stream()), "adam_ema")


def ema_swap(p32, p16, e32, e16):
    """p32 <-> e32 and p16 <-> e16 in place (one launch, no temporary); overlapping ranges, a wrong dtype or unequal lengths:
    ValueError"""
    from .ema import check_arenas
    n = check_arenas("ema_swap", p32, p16, e32, e16)
    _check(lib().ifseg_ema_swap(_ptr(p32), _ptr(p16), _ptr(e32), _ptr(e16), c_ll(n), _stream()), "ema_swap")


def rel_gather(table, idx, out):
    n, H = idx.numel(), table.shape[1]
    _check(lib().ifseg_rel_gather(_ptr(table), _ptr(idx), _ptr(out), c_int(n), c_int(H), _stream()), "rel_gather")
    return out


def resized_rel_bias(out, table2d, rel1d, relx, h, w, oh, ow, Lt, causal=False):
    """out fp32 [H, T, ld >= T] (T = h*w + Lt, rows `out.stride(1)` apart): the reference's doubly bilinear-resized rel-pos
    bias of a (h, w) grid from the delta table of the trained (oh, ow) grid; tail blocks from rel1d / relx (None: zero)"""
    H = out.shape[0]
    assert out.stride(2) == 1 and out.stride(0) == out.shape[1] * out.stride(1)
    _check(lib().ifseg_resized_rel_bias(_ptr(out), _ptr(table2d), _ptr(rel1d), _ptr(relx), c_int(H), c_int(h), c_int(w),
                                        c_int(oh), c_int(ow), c_int(Lt), c_int(1 if causal else 0), c_int(out.stride(1)),
                                        _stream()), "resized_rel_bias")
    return out


def resize_rows_bilinear(src, dst, h, w, oh, ow, src_stride, src_off):
    """dst bf16 [h*w, C] = bilinear resize of the oh x ow grid of rows src[y * src_stride + x + src_off]"""
    C = dst.shape[1]
    _check(lib().ifseg_resize_rows_bilinear(_ptr(src), _ptr(dst), c_int(C), c_int(h), c_int(w), c_int(oh), c_int(ow),
                                            c_int(src_stride), c_int(src_off), c_int(src.stride(0)), _stream()),
           "resize_rows_bilinear")
    return dst


def rel_gather_multi(tables, idx, out):
    """tables: list of L <= 16 bf16 [N, H] tensors of one shape; out fp32 [L, H, n]"""
    L, n, H = len(tables), idx.numel(), tables[0].shape[1]
    arr = (c_void_p * L)(*[t.data_ptr() for t in tables])
    _check(lib().ifseg_rel_gather_multi(arr, c_int(L), _ptr(idx), _ptr(out), c_int(n), c_int(H), _stream()), "rel_gather_multi")
    return out


class _AttnReduceArgs(ctypes.Structure):
    _fields_ = [("B", c_int), ("H", c_int), ("T", c_int), ("S", c_int), ("C", c_int), ("nparts", c_int),
                ("accumulate_pos", c_int),
                ("dpos_q_part", c_void_p), ("dpos_k_part", c_void_p), ("dpos_q_acc", c_void_p), ("dpos_k_acc", c_void_p),
                ("delta", c_void_p), ("gain", c_void_p), ("dgain", c_void_p), ("ntab", c_int),
                ("tab_part", c_void_p * 3), ("tab_idx", c_void_p * 3), ("tab_acc", c_void_p * 3), ("tab_n", c_int * 3),
                ("tab_nbucket", c_int * 3)]


def attn_bwd_reduce(B, H, T, S, C, dpq_part, dpk_part, dpq_acc, dpk_acc, accumulate_pos, delta, gain, dgain, nparts, tables):
    """every reduction behind attn_bwd's partial outputs in one launch (ifseg_attn_bwd_reduce); tables: list of
    (part [H,nparts,n] fp32, idx [n] int32, acc [n_bucket,H] fp32)"""
    assert all(t is None or t.dtype == torch.bfloat16 for t in (dpq_part, dpk_part)), "abs-pos partials are bf16"
    a = _AttnReduceArgs()
    a.B, a.H, a.T, a.S, a.C, a.nparts, a.accumulate_pos = B, H, T, S, C, nparts, 1 if accumulate_pos else 0
    a.dpos_q_part, a.dpos_k_part, a.dpos_q_acc, a.dpos_k_acc = _p(dpq_part), _p(dpk_part), _p(dpq_acc), _p(dpk_acc)
    a.delta, a.gain, a.dgain = _p(delta), _p(_f32(gain)), _p(dgain)
    a.ntab = len(tables)
    for i, (part, idx, acc) in enumerate(tables):
        assert part.dtype == torch.float32 and acc.dtype == torch.float32 and idx.dtype == torch.int32 and acc.shape[1] == H
        a.tab_part[i], a.tab_idx[i], a.tab_acc[i], a.tab_n[i], a.tab_nbucket[i] = _p(part), _p(idx), _p(acc), idx.numel(), acc.shape[0]
    _check(lib().ifseg_attn_bwd_reduce(ctypes.byref(a), _stream()), "attn_bwd_reduce")


def rel_scatter_add(d, idx, acc):
    n, H = idx.numel(), acc.shape[1]
    _check(lib().ifseg_rel_scatter_add(_ptr(d), _ptr(idx), _ptr(acc), c_int(n), c_int(H), _stream()), "rel_scatter")
    return acc


PROF_KINDS = ("gemm_nt", "gemm_nn", "gemm_tn", "conv", "attn_fwd", "attn_bwd_dkv", "attn_bwd_dq", "ln_fwd", "ln_bwd")


def prof_enable(mask, stride=1):
    lib().ifseg_prof_stride(c_int(stride))
    lib().ifseg_prof_enable(ctypes.c_uint(mask))


def prof_reset():
    lib().ifseg_prof_reset()


def prof_read(kind):
    ms, fl, by, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
    _check(lib().ifseg_prof_read(c_int(kind), ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by), ctypes.byref(n)), "prof_read")
    return {"kind": PROF_KINDS[kind], "ms": ms.value, "flops": fl.value, "bytes": by.value, "launches": n.value}


# ---------------------------------------------------------------------- the fused segmentation criterion (csrc/seg_tile.h)
# One 16 x 16 pixel tile per low-res cell, four sources of terms on it: cross entropy (csrc/loss.hip, plain or weighted), the OHEM
# hardness plane (csrc/ohem.hip), Dice (csrc/dice.hip), distillation (csrc/distill.hip); one gather (csrc/loss.hip) sums the
# gradients of the terms that are present.  The helpers below are what the public calls share.
def _span(t):
    """(first byte, one past the last byte) a view can touch, whatever its strides"""
    n = 1 + sum((s - 1) * st for s, st in zip(t.shape, t.stride())) if t.numel() else 0
    return t.data_ptr(), t.data_ptr() + n * t.element_size()


def _seg_geometry(logits_pad, target, hp, wp, H, W, nseg, teacher=None, target_optional=False):
    """what every tile call asserts of its logits, target (None allowed with target_optional) and teacher -> (B, device)"""
    assert logits_pad.dtype == torch.bfloat16 and logits_pad.dim() == 3 and logits_pad.stride(2) == 1 and logits_pad.is_cuda \
        and logits_pad.shape[1] >= hp * wp and logits_pad.stride(1) >= nseg, (logits_pad.dtype, tuple(logits_pad.shape), logits_pad.stride())
    B, dev = logits_pad.shape[0], logits_pad.device
    if teacher is not None:
        assert torch.is_tensor(teacher) and teacher.dtype == torch.bfloat16 and teacher.dim() == 3 \
            and teacher.device == dev and teacher.shape[0] == B and teacher.shape[1] >= hp * wp \
            and teacher.shape[2] >= nseg and teacher.stride(2) == 1 and teacher.stride(1) >= nseg \
            and (B == 1 or teacher.stride(0) >= hp * wp * teacher.stride(1)), \
            "distill: the teacher's logits must be bf16 [%d, >= %d, >= %d] on %s, got %s" % (
                B, hp * wp, nseg, dev, (teacher.dtype, tuple(teacher.shape), teacher.stride(), teacher.device)
                if torch.is_tensor(teacher) else type(teacher))
    if target is None:
        assert target_optional, "distill: mask=\"valid\" needs the target"
    else:
        assert target.dtype == torch.int64 and target.dim() == 2 and target.shape[0] == B and target.shape[1] >= H * W \
            and target.stride(1) == 1 and target.device == dev, (target.dtype, tuple(target.shape), target.stride(), target.device)
    assert B >= 1 and hp >= 1 and wp >= 1 and H == 16 * hp and W == 16 * wp and 1 <= nseg <= 512, (B, hp, wp, H, W, nseg)
    return B, dev


def _seg_tile_args(logits_pad, target, B, hp, wp, H, W, nseg, seg_id_offset, pad_id, eos_id):
    """the 14 leading arguments of every tile entry point; a single sample's batch stride is the sample's extent"""
    ld = logits_pad.stride(1)
    return (_ptr(logits_pad), c_int(ld), c_ll(logits_pad.stride(0) if B > 1 else hp * wp * ld), _ptr(target),
            c_ll(0 if target is None else target.stride(0) if B > 1 else H * W), c_int(B), c_int(hp), c_int(wp), c_int(H), c_int(W),
            c_int(nseg), c_ll(seg_id_offset), c_ll(pad_id), c_ll(eos_id))


def _seg_class_weight(class_weight, nseg, dev):
    if class_weight is not None:
        assert class_weight.dtype == torch.float32 and tuple(class_weight.shape) == (nseg,) and class_weight.is_contiguous() \
            and class_weight.device == dev, (class_weight.dtype, tuple(class_weight.shape), class_weight.device)
    return class_weight


def _seg_bufs(bufs, logits_pad, target, B, hp, wp, nseg, names, teacher=None):
    """the buffers `names` of a Dice / distillation call in `bufs` (a dict the caller keeps, or None): made on the first call,
    checked on every call, overlap with the logits, the target and the teacher refused"""
    bufs = {} if bufs is None else bufs
    dev, tiles, f32 = logits_pad.device, B * hp * wp, torch.float32
    shapes = {"dice_part": ((tiles * 3 * nseg,), f32), "dice_sums": ((B, 3, nseg), f32), "dice_tile": ((tiles * 9 * nseg,), f32),
              "dice_val": ((1,), f32), "loss3": ((3,), f32), "dl": (None, torch.bfloat16),
              "tile": ((tiles * 9 * nseg,), f32), "sp": ((tiles * (2 + 3 * nseg),), f32), "stats": ((2 + 3 * nseg,), f32),
              "bad": ((1,), torch.int32),
              "kd_tile": ((tiles * 9 * nseg,), f32), "kd_part": ((tiles * 2,), f32), "kd_stats": ((2,), f32), "loss4": ((4,), f32)}
    for k in names:
        shape, dt = shapes[k]
        if k == "dl":
            # the gradient has a layout of its own, whatever the logits' (a row-strided view [B, P+1, nseg] of a padded buffer
            # included): the gather writes whole rows of stride(1) elements, hp * wp + 1 of them per sample
            if k not in bufs:
                bufs[k] = torch.empty(B, hp * wp + 1, logits_pad.stride(1), dtype=dt, device=dev)
            t = bufs[k]
            assert t.dtype == dt and t.device == dev and t.dim() == 3 and t.shape[0] == B and t.shape[1] == hp * wp + 1 \
                and t.stride(2) == 1 and t.stride(1) == t.shape[2] >= nseg and (B == 1 or t.stride(0) >= t.shape[1] * t.stride(1)), \
                (k, t.dtype, tuple(t.shape), t.stride(), t.device)
        else:
            if k not in bufs:
                bufs[k] = (torch.zeros if k == "bad" else torch.empty)(shape, dtype=dt, device=dev)
            t = bufs[k]
            assert t.dtype == dt and tuple(t.shape) == shape and t.device == dev and t.is_contiguous(), \
                (k, t.dtype, tuple(t.shape), t.stride(), t.device)
        assert not _overlap(t, logits_pad) and (target is None or not _overlap(t, target)), \
            "dice: buffer %r overlaps the logits or the target" % k
    held = [bufs[k] for k in names]
    assert not any(_overlap(a, b) for i, a in enumerate(held) for b in held[i + 1:]), "dice: two buffers overlap"
    if teacher is not None:
        t0, t1 = _span(teacher)
        for k in names:
            b0, b1 = _span(bufs[k])
            assert not (b0 < t1 and t0 < b1), "distill: buffer %r overlaps the teacher's logits" % k
    return bufs


def _ce_tiles(logits_pad, target, B, hp, wp, H, W, nseg, seg_id_offset, pixel_weight, class_weight, norm_pixels, bufs, pad_id, eos_id,
              label_smoothing, weighted=None):
    """the CE tile launch (csrc/loss.hip: the weighted instantiation when pixel_weight, class_weight or norm_pixels is given, or
    for `seg_loss_weighted`, whatever it is given) and the reduction into bufs["tile"], bufs["sp"], bufs["stats"], bufs["bad"]"""
    dev = logits_pad.device
    if weighted is None:
        weighted = pixel_weight is not None or class_weight is not None or bool(norm_pixels)
    head = _seg_tile_args(logits_pad, target, B, hp, wp, H, W, nseg, seg_id_offset, pad_id, eos_id)
    tail = (_ptr(bufs["tile"]), _ptr(bufs["sp"]), _ptr(bufs["bad"]), c_float(label_smoothing), _stream())
    if not weighted:
        _check(lib().ifseg_seg_loss_tiles(*head, *tail), "seg_loss_tiles")
    else:
        pw_bs = 0
        if pixel_weight is not None:
            assert pixel_weight.dtype == torch.uint8 and tuple(pixel_weight.shape) == (B, H * W) and pixel_weight.stride(1) == 1 \
                and pixel_weight.device == dev, (pixel_weight.dtype, tuple(pixel_weight.shape), pixel_weight.stride(), pixel_weight.device)
            pw_bs = pixel_weight.stride(0) if B > 1 else H * W
        _seg_class_weight(class_weight, nseg, dev)
        _check(lib().ifseg_seg_loss_tiles_weighted(*head, _ptr(pixel_weight), c_ll(pw_bs), _ptr(class_weight),
                                                   c_int(1 if norm_pixels else 0), *tail), "seg_loss_tiles_weighted")
    reduce_parts(bufs["sp"], bufs["stats"], 1, B * hp * wp, 2 + 3 * nseg)


def _seg_gather(bufs, ce, dice, kd, B, hp, wp, nseg):
    """the one gather kernel through the entry point of the terms present: CE alone -> bufs["loss"] [1], with Dice ->
    bufs["loss3"], with distillation (kd = (weight, temperature, ..)) -> bufs["loss4"]; the gradient goes to bufs["dl"]"""
    dl = bufs["dl"]
    out = (_ptr(dl), c_int(dl.stride(1)), c_ll(dl.stride(0)), c_int(B), c_int(hp), c_int(wp), c_int(nseg))
    ce_src = (_ptr(bufs["tile"]), _ptr(bufs["stats"])) if ce else (None, None)
    dice_src = (_ptr(bufs["dice_tile"]), _ptr(bufs["dice_val"])) if dice else (None, None)
    if kd is not None:
        loss = bufs["loss4"]
        _check(lib().ifseg_seg_loss_gather3(*ce_src, *dice_src, _ptr(bufs["kd_tile"]), _ptr(bufs["kd_stats"]), c_float(kd[0]),
                                            c_float(kd[1]), *out, _ptr(loss), _stream()), "seg_loss_gather3")
    elif dice:
        loss = bufs["loss3"]
        _check(lib().ifseg_seg_loss_gather_sum(*ce_src, *dice_src, *out, _ptr(loss), _stream()), "seg_loss_gather_sum")
    else:
        loss = bufs["loss"]
        _check(lib().ifseg_seg_loss_gather(*ce_src, *out, _ptr(loss), _stream()), "seg_loss_gather")
    return loss, dl


def seg_loss(logits_pad, target, hp, wp, H, W, nseg, seg_id_offset, tile_partial, stats_part, stats, dlogits_pad,
             loss_out, pad_id=1, eos_id=2, bad_label=None, label_smoothing=0.0):
    """fused upsample + CE + grad + histograms; logits_pad / dlogits_pad: bf16 [B, P+1, ldl]"""
    B = logits_pad.shape[0]
    bufs = {"tile": tile_partial, "sp": stats_part, "stats": stats, "bad": bad_label, "dl": dlogits_pad, "loss": loss_out}
    _ce_tiles(logits_pad, target, B, hp, wp, H, W, nseg, seg_id_offset, None, None, False, bufs, pad_id, eos_id, label_smoothing)
    return _seg_gather(bufs, True, False, None, B, hp, wp, nseg)[0]


def seg_loss_weighted(logits_pad, target, hp, wp, H, W, nseg, seg_id_offset, tile_partial, stats_part, stats, dlogits_pad,
                      loss_out, pixel_weight=None, class_weight=None, norm_pixels=False, pad_id=1, eos_id=2, bad_label=None,
                      label_smoothing=0.0):
    """`seg_loss` with per-pixel and per-class weights (csrc/loss.hip, the weighted instantiation of the tile kernel;
    `criterions.seg_criterion.weighted_loss_reference` is the specification): pixel_weight uint8 [B, H*W] (rows H*W bytes
    apart or more) or None, class_weight fp32 [nseg] (non-negative and finite: the caller's duty) or None.  stats[0] is the
    weighted sum, stats[1] the normaliser Z (sum q cw[y], or qmax N_valid with norm_pixels), the histograms are the
    unweighted launch's; the reduction and the gather launch are `seg_loss`'s."""
    B = logits_pad.shape[0]
    bufs = {"tile": tile_partial, "sp": stats_part, "stats": stats, "bad": bad_label, "dl": dlogits_pad, "loss": loss_out}
    _ce_tiles(logits_pad, target, B, hp, wp, H, W, nseg, seg_id_offset, pixel_weight, class_weight, norm_pixels, bufs, pad_id, eos_id,
              label_smoothing, weighted=True)
    return _seg_gather(bufs, True, False, None, B, hp, wp, nseg)[0]


# ---------------------------------------------------------------------- online hard example mining
OHEM_WORK_WORDS = 3 * 1024 + 16     # == OHEM_WORK_WORDS (csrc/ohem.hip): three histograms of 1024 bins and the state words
OHEM_MAX_MIN_KEPT = 2 ** 40


def seg_hardness(logits_pad, target, hp, wp, H, W, nseg, seg_id_offset, out=None, pad_id=1, eos_id=2):
    """logits_pad bf16 [B, P+1, ldl], target int64 [B, H*W (+1)] -> fp32 [B, H*W] in one launch (csrc/ohem.hip, the front half of
    the loss tile kernel): the softmax probability of every pixel's own label under the x16 bilinear upsample, clamped to <= 1,
    and -1 where the target is no class (`seg_loss`'s predicate).  `criterions.seg_criterion.hardness_reference` is the
    specification.  out: written in place when given (contiguous)."""
    B, dev = _seg_geometry(logits_pad, target, hp, wp, H, W, nseg)
    if out is None:
        out = torch.empty(B, H * W, dtype=torch.float32, device=dev)
    assert out.dtype == torch.float32 and tuple(out.shape) == (B, H * W) and out.is_contiguous() and out.device == dev, \
        (out.dtype, tuple(out.shape), out.stride(), out.device)
    assert not _overlap(out, logits_pad) and not _overlap(out, target), "seg_hardness: out overlaps the logits or the target"
    _check(lib().ifseg_seg_hardness(*_seg_tile_args(logits_pad, target, B, hp, wp, H, W, nseg, seg_id_offset, pad_id, eos_id),
                                    _ptr(out), c_ll(H * W), _stream()), "seg_hardness")
    return out


def ohem_workspace(device):
    """the workspace of `ohem_select`: allocated (and zeroed) once, every call leaves it ready for the next"""
    return torch.zeros(OHEM_WORK_WORDS, dtype=torch.int64, device=device)


def check_ohem(thresh, min_kept):
    """0 <= thresh <= 1 and 0 <= min_kept < 2^40 (ValueError otherwise) -> (float, int); -0.0 becomes 0.0"""
    if isinstance(thresh, bool) or not isinstance(thresh, (int, float)) or not 0.0 <= thresh <= 1.0:
        raise ValueError("ohem: thresh must be a number in [0, 1], got %r" % (thresh,))
    if isinstance(min_kept, bool) or not isinstance(min_kept, int) or not 0 <= min_kept < OHEM_MAX_MIN_KEPT:
        raise ValueError("ohem: min_kept must be an integer in [0, 2**40), got %r" % (min_kept,))
    return float(thresh) + 0.0, min_kept


def ohem_select(hardness, thresh, min_kept, weight=None, out=None, info=None, work=None):
    """hardness fp32 [B, N] -> (plane uint8 [B, N], info int64 [4]) in four launches with no read-back (csrc/ohem.hip; an exact
    radix select over the batch; `criterions.seg_criterion.ohem_reference` is the specification, bit for bit): with
    k = min(min_kept * B, #candidates - 1) and tau = max(thresh, k-th smallest candidate), a candidate (0 <= v <= 1) strictly
    below tau gets weight[i] (uint8 [B, N]; None: 255), every other entry 0.  info = #candidates, #kept, the bits of tau and of
    the k-th value.  out / info: written in place when given; work: `ohem_workspace(device)`, kept by the caller between calls
    (a fresh one otherwise)."""
    thresh, min_kept = check_ohem(thresh, min_kept)
    assert hardness.dtype == torch.float32 and hardness.dim() == 2 and hardness.is_contiguous() and hardness.is_cuda, \
        (hardness.dtype, tuple(hardness.shape), hardness.stride(), hardness.device)
    B, N = hardness.shape
    dev = hardness.device
    assert B >= 1 and N >= 1 and B < 2 ** 20 and B * N < 2 ** 31, (B, N)
    if weight is not None:
        assert weight.dtype == torch.uint8 and tuple(weight.shape) == (B, N) and weight.is_contiguous() and weight.device == dev, \
            (weight.dtype, tuple(weight.shape), weight.stride(), weight.device)
    if out is None:
        out = torch.empty(B, N, dtype=torch.uint8, device=dev)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (B, N) and out.is_contiguous() and out.device == dev, \
        (out.dtype, tuple(out.shape), out.stride(), out.device)
    assert not _overlap(out, hardness) and (weight is None or not _overlap(out, weight)), "ohem_select: out overlaps its inputs"
    if info is None:
        info = torch.empty(4, dtype=torch.int64, device=dev)
    assert info.dtype == torch.int64 and tuple(info.shape) == (4,) and info.is_contiguous() and info.device == dev, \
        (info.dtype, tuple(info.shape), info.device)
    if work is None:
        work = ohem_workspace(dev)
    assert work.dtype == torch.int64 and tuple(work.shape) == (OHEM_WORK_WORDS,) and work.is_contiguous() and work.device == dev, \
        (work.dtype, tuple(work.shape), work.device)
    assert not any(_overlap(a, b) for a, b in ((info, out), (info, hardness), (work, out), (work, hardness), (work, info)))
    _check(lib().ifseg_ohem_select(_ptr(hardness), c_int(B), c_ll(N), c_float(thresh), c_ll(min_kept), _ptr(weight), _ptr(out),
                                   _ptr(info), _ptr(work), _stream()), "ohem_select")
    return out, info


# ---------------------------------------------------------------------- per-sample soft Dice
def check_dice_number(name, v, what="dice"):
    """a finite number > 0 (ValueError naming `name` otherwise) -> float"""
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0 < v < float("inf"):
        raise ValueError("%s: %s must be a finite number > 0, got %r" % (what, name, v))
    return float(v)


def check_dice(dice_weight, smooth, what="dice"):
    """dice_weight > 0 and smooth > 0, both finite numbers (ValueError otherwise) -> (float, float)"""
    return check_dice_number("dice_weight", dice_weight, what), check_dice_number("dice_smooth", smooth, what)


def seg_dice_sums(logits_pad, target, hp, wp, H, W, nseg, seg_id_offset, bufs=None, pad_id=1, eos_id=2):
    """logits_pad bf16 [B, P+1, ldl], target int64 [B, H*W (+1)] -> fp32 [B, 3, nseg] in two launches (csrc/dice.hip pass A, then
    `reduce_parts` over a sample's tiles, a fixed order): per sample and class I = sum p [y = c], P = sum p^2, Y = sum [y = c] over
    the valid pixels (`seg_loss`'s predicate), p the softmax of the x16 bilinear upsample.
    `criterions.seg_criterion.dice_sums_reference` is the specification.  bufs: a dict the caller keeps between calls (the result
    is bufs["dice_sums"]); nothing is allocated after the first call with it."""
    B, dev = _seg_geometry(logits_pad, target, hp, wp, H, W, nseg)
    bufs = _seg_bufs(bufs, logits_pad, target, B, hp, wp, nseg, ("dice_part", "dice_sums"))
    _check(lib().ifseg_seg_dice_sums(*_seg_tile_args(logits_pad, target, B, hp, wp, H, W, nseg, seg_id_offset, pad_id, eos_id),
                                     _ptr(bufs["dice_part"]), _stream()), "seg_dice_sums")
    reduce_parts(bufs["dice_part"], bufs["dice_sums"], B, hp * wp, 3 * nseg)
    return bufs["dice_sums"]


def _dice_tiles(logits_pad, target, B, hp, wp, H, W, nseg, seg_id_offset, dice_weight, smooth, class_weight, bufs, pad_id, eos_id):
    """pass A, the reduction and pass B into bufs["dice_sums"], bufs["dice_tile"], bufs["dice_val"]"""
    seg_dice_sums(logits_pad, target, hp, wp, H, W, nseg, seg_id_offset, bufs, pad_id, eos_id)
    _check(lib().ifseg_seg_dice_tiles(*_seg_tile_args(logits_pad, target, B, hp, wp, H, W, nseg, seg_id_offset, pad_id, eos_id),
                                      _ptr(bufs["dice_sums"]), _ptr(class_weight), c_float(dice_weight), c_float(smooth),
                                      _ptr(bufs["dice_tile"]), _ptr(bufs["dice_val"]), _stream()), "seg_dice_tiles")


def _distill_tiles(logits_pad, teacher_pad, target, B, hp, wp, H, W, nseg, seg_id_offset, temperature, mask_all, bufs, pad_id, eos_id):
    """the KD tile launch and the reduction into bufs["kd_tile"], bufs["kd_part"], bufs["kd_stats"]"""
    head = _seg_tile_args(logits_pad, target, B, hp, wp, H, W, nseg, seg_id_offset, pad_id, eos_id)
    ldt = teacher_pad.stride(1)
    _check(lib().ifseg_seg_distill_tiles(
        *head[:3], _ptr(teacher_pad), c_int(ldt), c_ll(teacher_pad.stride(0) if B > 1 else hp * wp * ldt), *head[3:],
        c_float(temperature), c_int(1 if mask_all else 0), _ptr(bufs["kd_tile"]), _ptr(bufs["kd_part"]), _stream()), "seg_distill_tiles")
    reduce_parts(bufs["kd_part"], bufs["kd_stats"], 1, B * hp * wp, 2)


_CE_BUFS = ("tile", "sp", "stats", "bad")
_DICE_BUFS = ("dice_part", "dice_sums", "dice_tile", "dice_val")
_KD_BUFS = ("kd_tile", "kd_part", "kd_stats")


def _seg_terms(logits_pad, teacher_pad, target, hp, wp, H, W, nseg, seg_id_offset, ce, dice, kd, bufs, pad_id, eos_id):
    """The terms that are present on one gradient: each term's own tile launches and reduction, in the order CE, Dice,
    distillation, then the gather entry of that set -> (bufs["loss4"] with distillation, else bufs["loss3"]; bufs["dl"]).
    ce: None or (pixel_weight, class_weight, norm_pixels, label_smoothing); dice: None or (dice_weight, smooth, class_weight);
    kd: None or (weight, temperature, mask_all) -- every number already validated by the caller."""
    B, dev = _seg_geometry(logits_pad, target, hp, wp, H, W, nseg, teacher=teacher_pad if kd is not None else None,
                           target_optional=kd is not None and kd[2] and ce is None and dice is None)
    if ce is not None:
        assert target.shape[1] == H * W + 1, tuple(target.shape)
    if dice is not None:
        _seg_class_weight(dice[2], nseg, dev)
    if kd is not None:
        names = _KD_BUFS + ("loss4", "dl") + (_CE_BUFS if ce is not None else ()) + (_DICE_BUFS if dice is not None else ())
    else:
        names = _DICE_BUFS + ("loss3", "dl") + (_CE_BUFS if ce is not None else ())
    bufs = _seg_bufs(bufs, logits_pad, target, B, hp, wp, nseg, names, teacher=teacher_pad if kd is not None else None)
    if ce is not None:
        _ce_tiles(logits_pad, target, B, hp, wp, H, W, nseg, seg_id_offset, ce[0], ce[1], ce[2], bufs, pad_id, eos_id, ce[3])
    if dice is not None:
        _dice_tiles(logits_pad, target, B, hp, wp, H, W, nseg, seg_id_offset, dice[0], dice[1], dice[2], bufs, pad_id, eos_id)
    if kd is not None:
        _distill_tiles(logits_pad, teacher_pad, target, B, hp, wp, H, W, nseg, seg_id_offset, kd[1], kd[2], bufs, pad_id, eos_id)
    return _seg_gather(bufs, ce is not None, dice is not None, kd, B, hp, wp, nseg)


def seg_dice(logits_pad, target, hp, wp, H, W, nseg, seg_id_offset, dice_weight, smooth=1.0, class_weight=None, bufs=None,
             pad_id=1, eos_id=2):
    """Dice alone (csrc/dice.hip): sums -> reduce -> tiles -> gather, four launches, nothing read back, no atomics.
    -> (loss fp32 [] = dice_weight * `criterions.seg_criterion.dice_loss_reference`, dlogits_pad bf16 [B, hp*wp+1, ld >= nseg] = its
    gradient, padding columns and the eos row zero).  class_weight fp32 [nseg] (non-negative and finite: the caller's duty) or
    None.  bufs as `seg_dice_sums` (loss is bufs["loss3"][0], the gradient bufs["dl"], the sums bufs["dice_sums"])."""
    dice = check_dice(dice_weight, smooth, "seg_dice") + (class_weight,)
    loss3, dl = _seg_terms(logits_pad, None, target, hp, wp, H, W, nseg, seg_id_offset, None, dice, None, bufs, pad_id, eos_id)
    return loss3[0], dl


def seg_loss_dice(logits_pad, target, hp, wp, H, W, nseg, seg_id_offset, dice_weight, smooth=1.0, dice_class_weight=None, bufs=None,
                  pixel_weight=None, class_weight=None, norm_pixels=False, pad_id=1, eos_id=2, label_smoothing=0.0):
    """cross entropy + dice_weight * Dice in one gradient: `seg_loss`'s tile launch and reduction (`seg_loss_weighted`'s when
    pixel_weight, class_weight or norm_pixels is given) as they are, then `seg_dice`'s launches and the
    two-source gather -> (loss_out fp32 [3] = total, CE, weighted Dice; dlogits_pad bf16 = d total / d logits, one rounding).
    loss_out[1] and bufs["stats"] are the bits the CE call gives alone.  bufs as `seg_dice_sums`; it also holds the CE call's
    tile / sp / stats / bad."""
    dice = check_dice(dice_weight, smooth, "seg_loss_dice") + (dice_class_weight,)
    return _seg_terms(logits_pad, None, target, hp, wp, H, W, nseg, seg_id_offset,
                      (pixel_weight, class_weight, norm_pixels, label_smoothing), dice, None, bufs, pad_id, eos_id)


# ---------------------------------------------------------------------- distillation: per-pixel KL to a teacher
DISTILL_MASKS = ("valid", "all")


def check_distill(weight, temperature=1.0, mask="valid", who="distill"):
    """the distillation term's three settings -> (weight or None, temperature, mask_all).  weight=None switches the term off; a
    finite number > 0 switches it on; the temperature is a finite number > 0 and the mask one of ("valid", "all") either way.
    Anything else (a bool, a string) is a ValueError naming distill_weight / distill_temperature / distill_mask."""
    temperature = check_dice_number("distill_temperature", temperature, who)
    if not isinstance(mask, str) or mask not in DISTILL_MASKS:
        raise ValueError("%s: distill_mask must be one of %s, got %r" % (who, DISTILL_MASKS, mask))
    if weight is not None:
        weight = check_dice_number("distill_weight", weight, who)
    return weight, temperature, mask == "all"


def seg_distill(logits_pad, teacher_pad, target, hp, wp, H, W, nseg, seg_id_offset, weight, temperature=1.0, mask="valid", bufs=None,
                pad_id=1, eos_id=2):
    """Distillation alone (csrc/distill.hip): tiles -> reduce -> gather, three launches, nothing read back, no atomics.
    logits_pad / teacher_pad bf16 [B, >= hp*wp, ld >= nseg] (row-strided views, each with strides of its own; the teacher's padding
    columns and eos row are never read), target int64 [B, H*W (+1)], or None with mask="all"
    -> (loss fp32 [] = weight * `criterions.seg_criterion.distill_loss_reference`, dlogits_pad bf16 [B, hp*wp+1, ld] = its gradient
    in the student's logits, padding columns and the eos row zero).  bufs: a dict the caller keeps between calls (the loss is
    bufs["loss4"][3], the gradient bufs["dl"], [sum KL, N] bufs["kd_stats"]); nothing is allocated after the first call with it."""
    kd = check_distill(weight, temperature, mask, "seg_distill")
    if kd[0] is None:
        raise ValueError("seg_distill: distill_weight must be a finite number > 0, got None")
    loss4, dl = _seg_terms(logits_pad, teacher_pad, target, hp, wp, H, W, nseg, seg_id_offset, None, None, kd, bufs, pad_id, eos_id)
    return loss4[3], dl


def seg_loss_distill(logits_pad, teacher_pad, target, hp, wp, H, W, nseg, seg_id_offset, weight, temperature=1.0, mask="valid",
                     dice_weight=None, dice_smooth=1.0, dice_class_weight=None, bufs=None, pixel_weight=None, class_weight=None,
                     norm_pixels=False, pad_id=1, eos_id=2, label_smoothing=0.0):
    """cross entropy (+ dice_weight * Dice) + weight * distillation in one gradient: `seg_loss`'s tile launch and reduction
    (`seg_loss_weighted`'s when pixel_weight, class_weight or norm_pixels is given) as they are, `seg_dice`'s launches when
    dice_weight is given, the KD tiles and reduction, and the three-source gather: five launches, eight with Dice
    -> (loss_out fp32 [4] = total, CE, weighted Dice, weighted KD; dlogits_pad bf16 = d total / d logits, one rounding).
    loss_out[1] and bufs["stats"] are the bits the CE call gives alone, loss_out[2] the bits `seg_loss_dice` gives, loss_out[3]
    the bits `seg_distill` gives.  bufs as `seg_distill`; it also holds the CE call's tile / sp / stats / bad and the Dice buffers."""
    kd = check_distill(weight, temperature, mask, "seg_loss_distill")
    if kd[0] is None:
        raise ValueError("seg_loss_distill: distill_weight must be a finite number > 0, got None")
    dice = None
    if dice_weight is not None:
        dice = check_dice(dice_weight, dice_smooth, "seg_loss_distill") + (dice_class_weight,)
    assert target is not None, "seg_loss_distill: the cross entropy needs the target"
    return _seg_terms(logits_pad, teacher_pad, target, hp, wp, H, W, nseg, seg_id_offset,
                      (pixel_weight, class_weight, norm_pixels, label_smoothing), dice, kd, bufs, pad_id, eos_id)


# ---------------------------------------------------------------------- eval post-processing
def rows_to_f32(logits_pad, nseg, rows_per_batch, softmax=False, temperature=1.0):
    """logits_pad bf16 [B, T, ld] -> fp32 [B, rows_per_batch, nseg] (first rows of every sample), optionally softmaxed"""
    B = logits_pad.shape[0]
    out = torch.empty(B, rows_per_batch, nseg, dtype=torch.float32, device=logits_pad.device)
    _check(lib().ifseg_softmax_rows(_ptr(logits_pad), c_ll(logits_pad.stride(0)), c_int(rows_per_batch),
                                    c_int(logits_pad.stride(1)), _ptr(out), c_int(B * rows_per_batch), c_int(nseg),
                                    c_float(1.0 / temperature), c_int(1 if softmax else 0), _stream()), "softmax_rows")
    return out


def rows_to_f32_biased(logits_pad, nseg, rows_per_batch, bias, softmax=False, temperature=1.0):
    """`rows_to_f32` with the per-class vector `bias` (fp32 [nseg], contiguous, on the logits' device) SUBTRACTED from the
    widened logits in front of the temperature: a_c = (z_c - bias[c]) * (1 / temperature), softmaxed or (softmax=False:
    no temperature) z_c - bias[c] itself, one fp32 subtraction (csrc/bsweep.hip).  bias = 0 gives `rows_to_f32`'s bits."""
    assert torch.is_tensor(bias) and bias.dtype == torch.float32 and tuple(bias.shape) == (nseg,) and bias.is_contiguous() \
        and bias.device == logits_pad.device, (getattr(bias, "dtype", type(bias)), tuple(getattr(bias, "shape", ())), nseg)
    B = logits_pad.shape[0]
    out = torch.empty(B, rows_per_batch, nseg, dtype=torch.float32, device=logits_pad.device)
    _check(lib().ifseg_softmax_rows_bias(_ptr(logits_pad), c_ll(logits_pad.stride(0)), c_int(rows_per_batch),
                                         c_int(logits_pad.stride(1)), _ptr(bias), _ptr(out), c_int(B * rows_per_batch),
                                         c_int(nseg), c_float(1.0 / temperature), c_int(1 if softmax else 0), _stream()),
           "softmax_rows_bias")
    return out


def neighbour_smoothing(logits_pad, nseg, feat, iters, topk, temperature=1.0, bias=None):
    """seg_criterion.py:197-213 on the device: logits_pad bf16 [B, P+1, ld], feat bf16 [B, P, D] (trunk features)
    -> smoothed class probabilities fp32 [B, P, nseg].  bias (fp32 [nseg]): the smoothing starts from
    `rows_to_f32_biased`'s probabilities; None: from `rows_to_f32`'s, as ever"""
    B, P, D = feat.shape
    dev = feat.device
    fn = torch.empty(B * P, D, dtype=torch.bfloat16, device=dev)
    _check(lib().ifseg_l2norm_rows_bf16(_ptr(feat.contiguous()), _ptr(fn), c_int(B * P), c_int(D), _stream()), "l2norm_rows")
    sim = torch.empty(B, P, P, dtype=torch.float32, device=dev)
    gemm(GEMM_NT, fn, fn, sim, P, P, D, D, D, P, flags=GEMM_OUT_F32, batch=B, sA=P * D, sB=P * D, sC=P * P)
    idx = torch.empty(B * P, topk, dtype=torch.int32, device=dev)
    _check(lib().ifseg_topk_rows_f32(_ptr(sim), _ptr(idx), c_int(B * P), c_int(P), c_int(topk), _stream()), "topk_rows")
    if bias is None:
        prob = rows_to_f32(logits_pad, nseg, P, softmax=True, temperature=temperature)
    else:
        prob = rows_to_f32_biased(logits_pad, nseg, P, bias, softmax=True, temperature=temperature)
    tmp = torch.empty_like(prob)
    for _ in range(iters):
        _check(lib().ifseg_gather_mean(_ptr(prob), _ptr(idx), _ptr(tmp), c_int(B), c_int(P), c_int(nseg), c_int(topk),
                                       _stream()), "gather_mean")
        prob, tmp = tmp, prob
    return prob


def seg_eval(scores, hp, wp, target, h, w, seg_id_offset):
    """scores fp32 [hp*wp, n] (one image), target int64 [h*w] -> (display CE loss tensor, int64 hist [3, n] =
    intersect / predicted / label pixel counts) at the original h x w resolution (seg_criterion.py:289-347)"""
    n = scores.shape[-1]
    dev = scores.device
    nblk = (h * w + 255) // 256
    hist = torch.zeros(3, n, dtype=torch.int64, device=dev)
    part = torch.empty(nblk, 2, dtype=torch.float32, device=dev)
    _check(lib().ifseg_seg_eval(_ptr(scores.contiguous()), c_int(hp), c_int(wp), c_int(n), _ptr(target.contiguous()), c_int(h),
                                c_int(w), c_ll(seg_id_offset), _ptr(hist), _ptr(part), c_int(nblk), _stream()), "seg_eval")
    tot = torch.empty(2, dtype=torch.float32, device=dev)
    reduce_parts(part, tot, 1, nblk, 2)
    return tot[0] / tot[1], hist


SEG_PREDICT_MAX_CLASSES = 512


@contextlib.contextmanager
def _staging(setter, staging_bytes):
    """the LDS staging limit of one kernel (an ifseg_*_staging setter) at staging_bytes for the calls inside; None: untouched"""
    prev = setter(c_int(staging_bytes)) if staging_bytes is not None else None
    try:
        yield
    finally:
        if prev is not None:
            setter(c_int(prev))


_UNSTAGED = contextlib.nullcontext()


def _staged(setter, staging_bytes):
    """`_staging` for the short launches: a call that leaves the limit alone (None) pays for no generator context"""
    return _staging(getattr(lib(), setter), staging_bytes) if staging_bytes is not None else _UNSTAGED


def _limits(symbol, count):
    """the first `count` values of one of the library's ifseg_*_limit(which) entry points"""
    return tuple(int(getattr(lib(), symbol)(c_int(k))) for k in range(count))


def _predict_outputs(B, n, h, w, dev, conf, probs, label_dtype, want_labels=True):
    """-> (labels [B, h, w] uint8 for n <= 256 else int16, or `label_dtype` (None without want_labels: the scoring calls); conf
    fp32 [B, h, w] or None; probs fp32 [B, n, h, w] or None), uninitialised"""
    if label_dtype is None:
        label_dtype = torch.uint8 if n <= 256 else torch.int16
    assert label_dtype in (torch.uint8, torch.int16) and (n <= 256 or label_dtype == torch.int16), (label_dtype, n)
    labels = torch.empty(B, h, w, dtype=label_dtype, device=dev) if want_labels else None
    cf = torch.empty(B, h, w, dtype=torch.float32, device=dev) if conf else None
    pr = torch.empty(B, n, h, w, dtype=torch.float32, device=dev) if probs else None
    return labels, cf, pr


def _seg_launch(checked, hw, gt, raw_labels=True, labels=True, conf=False, probs=False, areas=None, tally=None,
                staging_bytes=None, label_dtype=None):
    """The shared end of the seg_predict* / seg_score* bindings.  checked: what the pair's own checks of its inputs gave,
    (symbols, head, tail, B, n, device); symbols: the kernel's (predict, score, staging) entry points.  gt None: the predict
    call (head..., h, w, tail..., labels, their size, conf, probs, stream) at hw = (h, w) -> (labels, conf, probs).  gt given:
    the ground truth and the counters are checked, the output size is gt's own, and the score call takes the same arguments
    followed by gt and the counters -> (areas, tally, labels | None, conf | None, probs | None).  head: called behind every
    check -> the leading arguments (device pointers are taken there); tail: the ones behind h, w; both as ctypes values."""
    symbols, head, tail, B, n, dev = checked
    if gt is None:
        h, w = hw
        assert h >= 1 and w >= 1 and B * h * w < 2 ** 31, (B, h, w)
    else:
        h, w = _score_gt(gt, B, dev)
        assert B * h * w < 2 ** 31, (B, h, w)
        areas, tally = _score_counters(n, dev, areas, tally)
    lab, cf, pr = _predict_outputs(B, n, h, w, dev, conf, probs, label_dtype, labels)
    args = head() + (c_int(h), c_int(w)) + tail + (_ptr(lab), c_int(lab.element_size() if labels else 0), _ptr(cf), _ptr(pr))
    if gt is not None:
        args += (_ptr(gt), c_int(gt.element_size()), c_int(1 if raw_labels else 0), _ptr(areas), _ptr(tally))
    symbol = symbols[0] if gt is None else symbols[1]
    with _staged(symbols[2], staging_bytes):
        _check(getattr(lib(), symbol)(*args, _stream()), symbol[6:])
    return (lab, cf, pr) if gt is None else (areas, tally, lab, cf, pr)


def _seg_single(scores, hp, wp):
    """the inputs of seg_predict and seg_score, checked -> `_seg_launch`'s first argument"""
    assert scores.dtype == torch.float32 and scores.dim() == 3 and scores.is_contiguous(), (scores.dtype, tuple(scores.shape), scores.stride())
    B, P, n = scores.shape
    assert P == hp * wp and B >= 1 and hp >= 1 and wp >= 1, (tuple(scores.shape), hp, wp)
    assert 1 <= n <= SEG_PREDICT_MAX_CLASSES, n
    return (("ifseg_seg_predict", "ifseg_seg_score", "ifseg_seg_predict_staging"),
            lambda: (_ptr(scores), c_int(B), c_int(hp), c_int(wp), c_int(n)), (), B, n, scores.device)


def seg_predict(scores, hp, wp, h, w, conf=False, probs=False, staging_bytes=None, label_dtype=None):
    """scores fp32 [B, hp*wp, n] (class fastest: what rows_to_f32 / neighbour_smoothing return) -> (labels [B, h, w], uint8 for
    n <= 256 else int16; conf fp32 [B, h, w] or None; probs fp32 [B, n, h, w] or None): bilinear resize to h x w
    (align_corners=False), argmax, the winning value and every value in one pass (csrc/predict.hip).
    staging_bytes: size of the kernel's LDS staging buffer for this call (0: every tile reads global memory), None: the default;
    label_dtype: None, or torch.uint8 (n <= 256 only) / torch.int16 to choose the width"""
    return _seg_launch(_seg_single(scores, hp, wp), (h, w), None, conf=conf, probs=probs, staging_bytes=staging_bytes,
                       label_dtype=label_dtype)


SEG_PREDICT_MAX_VIEWS = 16


class _PredictView(ctypes.Structure):
    _fields_ = [("scores", c_void_p), ("hp", c_int), ("wp", c_int), ("flip", c_int)]


def seg_predict_views(views, h, w, conf=False, probs=False, staging_bytes=None, label_dtype=None):
    """views: a list of 1 .. 16 (scores fp32 [B, hp*wp, n], hp, wp, flip), one per forward of the same images at its own grid;
    flip: the network saw the image mirrored along its width -> (labels, conf, probs) as `seg_predict`, of the MEAN of the
    views: each is resized to h x w by seg_predict's rule (a flipped one on its mirrored columns), the values are added in
    fp32 in view order and multiplied by float(1 / K), in one launch (csrc/predict.hip); `predict.upsample_views_reference` is
    the specification.  One unflipped view gives seg_predict's outputs bit for bit.  The view table is a kernel argument:
    nothing is copied to the device.  staging_bytes, label_dtype: as in `seg_predict`."""
    return _seg_launch(_seg_views(views), (h, w), None, conf=conf, probs=probs, staging_bytes=staging_bytes,
                       label_dtype=label_dtype)


def _seg_views(views):
    """the inputs of seg_predict_views and seg_score_views, checked -> `_seg_launch`'s first argument"""
    views = list(views)
    assert 1 <= len(views) <= SEG_PREDICT_MAX_VIEWS, len(views)
    for k, (scores, hp, wp, flip) in enumerate(views):
        assert scores.dtype == torch.float32 and scores.dim() == 3 and scores.is_contiguous(), (k, scores.dtype, tuple(scores.shape), scores.stride())
    B, _, n = views[0][0].shape
    dev = views[0][0].device
    for k, (scores, hp, wp, flip) in enumerate(views):
        assert scores.shape[0] == B and scores.shape[2] == n and scores.device == dev, (k, tuple(scores.shape), B, n)
        assert scores.shape[1] == hp * wp and hp >= 1 and wp >= 1, (k, tuple(scores.shape), hp, wp)
    assert B >= 1 and 1 <= n <= SEG_PREDICT_MAX_CLASSES, (B, n)

    def head():
        table = (_PredictView * len(views))()
        for k, (scores, hp, wp, flip) in enumerate(views):
            table[k] = _PredictView(_ptr(scores), int(hp), int(wp), 1 if flip else 0)
        return table, c_int(len(views)), c_int(B), c_int(n)

    return ("ifseg_seg_predict_views", "ifseg_seg_score_views", "ifseg_seg_predict_views_staging"), head, (), B, n, dev


# --------------------------------------------------------------------------- scoring against ground truth
def _counter(t, shape, dev):
    """a counter a call adds to: the caller's `t` (int64 of `shape`, contiguous, on `dev`), checked, or fresh zeros"""
    if t is None:
        return torch.zeros(*shape, dtype=torch.int64, device=dev)
    assert t.dtype == torch.int64 and tuple(t.shape) == tuple(shape) and t.is_contiguous() and t.device == dev, \
        (t.dtype, tuple(t.shape), t.stride(), t.device, tuple(shape))
    return t


def _score_counters(n, dev, areas, tally):
    """the counters a scoring call adds to: the caller's (int64 [3, n] and [2], contiguous, on `dev`) or fresh zeroed ones"""
    return _counter(areas, (3, n), dev), _counter(tally, (2,), dev)


def _label_maps(what, labels, conf, gt, n=None):
    """what the kernels over a finished label map ask of it and of the maps beside it, its confidences and / or its ground
    truth (None: the kernel takes none): contiguous, of one shape on one device, 1 .. 2^31 - 1 pixels (and, where given,
    1 <= n <= SEG_PREDICT_MAX_CLASSES)"""
    assert labels.dtype in (torch.uint8, torch.int16) and labels.is_contiguous(), (what, labels.dtype, labels.stride())
    assert conf is None or (conf.dtype == torch.float32 and conf.is_contiguous() and conf.shape == labels.shape
                            and conf.device == labels.device), \
        (what, conf.dtype, tuple(conf.shape), conf.stride(), tuple(labels.shape), conf.device, labels.device)
    assert gt is None or (gt.dtype in (torch.uint8, torch.int16) and gt.is_contiguous() and gt.shape == labels.shape
                          and gt.device == labels.device), \
        (what, gt.dtype, tuple(gt.shape), gt.stride(), tuple(labels.shape), gt.device, labels.device)
    assert n is None or (isinstance(n, int) and 1 <= n <= SEG_PREDICT_MAX_CLASSES), (what, n)
    assert 1 <= labels.numel() < 2 ** 31, (what, tuple(labels.shape))


def _score_gt(gt, B, dev):
    assert gt.dtype in (torch.uint8, torch.int16) and gt.dim() == 3 and gt.is_contiguous(), (gt.dtype, tuple(gt.shape), gt.stride())
    assert gt.shape[0] == B and gt.device == dev and gt.shape[1] >= 1 and gt.shape[2] >= 1, (tuple(gt.shape), B, gt.device, dev)
    return int(gt.shape[1]), int(gt.shape[2])


def seg_areas(labels, gt, n, raw_labels=True, areas=None, tally=None):
    """labels uint8 / int16 [...] (predicted classes), gt uint8 / int16 of the same shape -> (areas int64 [3, n], tally int64 [2]):
    per class #(pred = gt = c), #(pred = c), #(gt = c) over the scored pixels; #scored pixels, #pixels with a ground truth out of
    range (csrc/predict.hip; `predict.areas_reference` is the specification and states the ground-truth rule).  `areas` / `tally`
    given: ACCUMULATED into, else fresh zeroed ones.  For label maps that do not come out of seg_score / seg_score_views."""
    _label_maps("seg_areas", labels, None, gt, n)
    areas, tally = _score_counters(n, labels.device, areas, tally)
    _check(lib().ifseg_seg_areas(_ptr(labels), c_int(labels.element_size()), _ptr(gt), c_int(gt.element_size()),
                                 c_ll(labels.numel()), c_int(n), c_int(1 if raw_labels else 0), _ptr(areas), _ptr(tally),
                                 _stream()), "seg_areas")
    return areas, tally


# the tables of seg_confusion_kernel (csrc/predict.hip, csrc/count.h), for callers and tests that size an input against them
SEG_CONFUSION_DIRECT_MAX = 16384    # == SC_DIRECT_MAX: n (n + 1) up to this (n <= 127) counts in a direct LDS table, else hashed
SEG_CONFUSION_SLOTS = 4096          # == count::SLOTS: the (class, label) pairs a workgroup's hashed table holds at most
SEG_CONFUSION_STEP_PIXELS = 4096    # the pixels a workgroup takes per step: 256 lanes of 16
SEG_CONFUSION_MAX_BLOCKS = 512      # == count::MAX_BLOCKS: the workgroups of a launch at most (grid-stride beyond)


def seg_confusion_limits():
    """-> (direct table entries, hashed slots, pixels per workgroup step, workgroups at most) as the loaded library states them
    (`ifseg_seg_confusion_limit`): the four constants above, which the tests hold against it"""
    return _limits("ifseg_seg_confusion_limit", 4)


def seg_confusion(labels, gt, n, raw_labels=True, confusion=None):
    """labels uint8 / int16 [...] (predicted classes), gt uint8 / int16 of the same shape -> confusion int64 [n, n + 1]: over the
    scored pixels of `seg_areas`, [c, p] = #(gt = c and pred = p), column n taking every predicted label outside [0, n)
    (csrc/predict.hip; `predict.confusion_reference` is the specification).  `confusion` given: ACCUMULATED into, else fresh
    zeros.  Its sum is seg_areas' tally[0], the diagonal / column sums of [:, :n] areas[0] / areas[1], its row sums areas[2]."""
    _label_maps("seg_confusion", labels, None, gt, n)
    confusion = _counter(confusion, (n, n + 1), labels.device)
    _check(lib().ifseg_seg_confusion(_ptr(labels), c_int(labels.element_size()), _ptr(gt), c_int(gt.element_size()),
                                     c_ll(labels.numel()), c_int(n), c_int(1 if raw_labels else 0), _ptr(confusion), _stream()),
           "seg_confusion")
    return confusion


# the limits of seg_boundary_kernel (csrc/boundary.hip)
SEG_BOUNDARY_MAX_D = 64             # == SEG_BOUNDARY_MAX_D there: the band's half width at most, 2 % of a 3200-pixel diagonal


def seg_boundary_limits():
    """-> (the largest d, the largest n) as the loaded library states them (`ifseg_seg_boundary_limit`): SEG_BOUNDARY_MAX_D and
    SEG_PREDICT_MAX_CLASSES, which the tests hold against it"""
    return _limits("ifseg_seg_boundary_limit", 2)


def seg_boundary_areas(labels, gt, n, d, raw_labels=True, bareas=None, band=False):
    """labels uint8 / int16 [B, h, w] or [h, w] (predicted classes), gt uint8 / int16 of the same shape, d an int in 1 ..
    SEG_BOUNDARY_MAX_D -> (bareas int64 [3, n], band uint8 of the maps' shape | None): Boundary IoU's band areas, `seg_areas`'
    three counters restricted to the pixels within d of a contour of the ground truth / of the labels / of both, and with
    `band` the two bands themselves, bit 0 the ground truth's and bit 1 the labels', for every pixel (csrc/boundary.hip;
    `predict.boundary_areas_reference` is the specification and states the rule).  `bareas` given: ACCUMULATED into, else fresh
    zeros.  One launch, nothing else allocated."""
    _label_maps("seg_boundary_areas", labels, None, gt, n)
    assert labels.dim() in (2, 3), tuple(labels.shape)
    assert isinstance(d, int) and not isinstance(d, bool) and 1 <= d <= SEG_BOUNDARY_MAX_D, d
    bareas = _counter(bareas, (3, n), labels.device)
    out = torch.empty(labels.shape, dtype=torch.uint8, device=labels.device) if band else None
    B = labels.shape[0] if labels.dim() == 3 else 1
    h, w = labels.shape[-2:]
    _check(lib().ifseg_seg_boundary_areas(_ptr(labels), c_int(labels.element_size()), _ptr(gt), c_int(gt.element_size()), c_int(B),
                                          c_int(h), c_int(w), c_int(n), c_int(d), c_int(1 if raw_labels else 0), _ptr(bareas),
                                          _ptr(out), _stream()), "seg_boundary_areas")
    return bareas, out


# the limits of csrc/distance.hip
SEG_DISTANCE_MAX = 128              # == SEG_DISTANCE_MAX there: the largest max_distance / radius; 128^2 fits the uint16
SEG_DISTANCE_FAR = 65535            # == SEG_DISTANCE_FAR: farther than max_distance, or no other value in the image
SEG_TRIMAP_MAX_RADII = 8            # == SEG_TRIMAP_MAX_RADII: the rings of one counting launch (K 3 n uint32 of LDS)


def seg_distance_limits():
    """-> (the largest max_distance, the "far" value, the largest number of radii, the largest n) as the loaded library states
    them (`ifseg_seg_distance_limit`): SEG_DISTANCE_MAX, SEG_DISTANCE_FAR, SEG_TRIMAP_MAX_RADII and SEG_PREDICT_MAX_CLASSES,
    which the tests hold against it"""
    return _limits("ifseg_seg_distance_limit", 4)


def _distance_map(what, name, t, like=None):
    """a label map of the distance kernels, as ValueErrors that name the argument -> (B, H, W)"""
    if not torch.is_tensor(t) or t.dtype not in (torch.uint8, torch.int16):
        raise ValueError("%s: %s must be a uint8 / int16 tensor, got %s" % (what, name, t.dtype if torch.is_tensor(t) else type(t)))
    if t.dim() not in (2, 3) or not t.is_contiguous() or not 1 <= t.numel() < 2 ** 31:
        raise ValueError("%s: %s must be contiguous [H, W] or [B, H, W] with 1 .. 2**31 - 1 pixels, got %s with strides %s"
                         % (what, name, tuple(t.shape), t.stride()))
    if like is not None and (t.shape != like.shape or t.device != like.device):
        raise ValueError("%s: %s must have the labels' shape %s on %s, got %s on %s"
                         % (what, name, tuple(like.shape), like.device, tuple(t.shape), t.device))
    H, W = t.shape[-2:]
    return t.numel() // (H * W), int(H), int(W)


def _distance_plane(what, name, t, like, others):
    """a distance plane: the caller's (contiguous uint16 of `like`'s shape on its device, sharing no byte with `others`)"""
    if not torch.is_tensor(t) or t.dtype != torch.uint16 or t.shape != like.shape or not t.is_contiguous() or t.device != like.device:
        raise ValueError("%s: %s must be a contiguous uint16 tensor of shape %s on %s, got %s" % (
            what, name, tuple(like.shape), like.device,
            (t.dtype, tuple(t.shape), t.stride(), t.device) if torch.is_tensor(t) else type(t)))
    for other_name, other in others:
        if _overlap(t, other):
            raise ValueError("%s: %s overlaps %s" % (what, name, other_name))
    return t


def _max_distance(what, max_distance):
    if not isinstance(max_distance, int) or isinstance(max_distance, bool) or not 1 <= max_distance <= SEG_DISTANCE_MAX:
        raise ValueError("%s: max_distance must be an int in 1 .. %d, got %r" % (what, SEG_DISTANCE_MAX, max_distance))
    return max_distance


def seg_distance(labels, max_distance, border=False, out=None):
    """labels uint8 / int16 [H, W] or [B, H, W], max_distance = R an int in 1 .. SEG_DISTANCE_MAX -> out uint16 of the labels'
    shape: per pixel the exact squared Euclidean distance to the nearest pixel of ANOTHER value of the same image where it is
    at most R^2, else SEG_DISTANCE_FAR = 65535 (csrc/distance.hip; `predict.distance_reference` is the specification and
    states the rule).  border: every position outside the image counts as another value too.  Two launches on the current
    stream, nothing synchronises; integers with one writer per element, so two calls give equal bits.  out: written in place
    when given.  The work plane (uint8 of the labels' shape, the clamped vertical distances) is allocated here.  Bad arguments:
    ValueError naming the argument, before anything is launched."""
    what = "seg_distance"
    B, H, W = _distance_map(what, "labels", labels)
    R = _max_distance(what, max_distance)
    if not isinstance(border, bool):
        raise ValueError("%s: border must be True or False, got %r" % (what, border))
    if out is None:
        out = torch.empty(labels.shape, dtype=torch.uint16, device=labels.device)
    else:
        _distance_plane(what, "out", out, labels, (("labels", labels),))
    work = torch.empty(labels.shape, dtype=torch.uint8, device=labels.device)
    _check(lib().ifseg_seg_distance(_ptr(labels), c_int(labels.element_size()), c_int(B), c_int(H), c_int(W), c_int(R),
                                    c_int(1 if border else 0), _ptr(work), _ptr(out), _stream()), what)
    return out


def _trimap_radii(what, radii):
    ok = isinstance(radii, (tuple, list)) and 1 <= len(radii) <= SEG_TRIMAP_MAX_RADII \
        and all(isinstance(r, int) and not isinstance(r, bool) and 1 <= r <= SEG_DISTANCE_MAX for r in radii) \
        and all(a < b for a, b in zip(radii, radii[1:]))
    if not ok:
        raise ValueError("%s: radii must be 1 .. %d strictly ascending ints in 1 .. %d, got %r"
                         % (what, SEG_TRIMAP_MAX_RADII, SEG_DISTANCE_MAX, radii))
    return tuple(radii)


def seg_trimap_areas(labels, gt, n, radii, raw_labels=True, border=False, trimap=None, dist=None):
    """labels uint8 / int16 [H, W] or [B, H, W] (predicted classes), gt uint8 / int16 of the same shape, radii a tuple of K
    strictly ascending ints in 1 .. SEG_DISTANCE_MAX, 1 <= K <= SEG_TRIMAP_MAX_RADII -> (trimap int64 [K, 3, n], the ground
    truth's distance plane uint16 of the maps' shape): `seg_areas`' three counters per ring of the trimap, ring k holding the
    scored pixels whose squared distance d2 to the nearest ground-truth pixel of another value has
    radii[k - 1]^2 < d2 <= radii[k]^2 (csrc/distance.hip; `predict.trimap_areas_reference` is the specification and states the
    rule).  dist: the plane of `seg_distance(gt, R, border)` with R >= radii[-1], where the caller has it; else it is computed
    here as `seg_distance(gt, radii[-1], border)` (two launches) and returned.  `trimap` given: ACCUMULATED into, else fresh
    zeros.  One counting launch behind the distance's, nothing synchronises.  Bad arguments: ValueError naming the argument,
    before anything is launched."""
    what = "seg_trimap_areas"
    B, H, W = _distance_map(what, "labels", labels)
    _distance_map(what, "gt", gt, labels)
    if not isinstance(n, int) or isinstance(n, bool) or not 1 <= n <= SEG_PREDICT_MAX_CLASSES:
        raise ValueError("%s: n must be an int in 1 .. %d, got %r" % (what, SEG_PREDICT_MAX_CLASSES, n))
    radii = _trimap_radii(what, radii)
    if not isinstance(border, bool):
        raise ValueError("%s: border must be True or False, got %r" % (what, border))
    K = len(radii)
    if trimap is None:
        trimap = torch.zeros(K, 3, n, dtype=torch.int64, device=labels.device)
    elif not torch.is_tensor(trimap) or trimap.dtype != torch.int64 or tuple(trimap.shape) != (K, 3, n) \
            or not trimap.is_contiguous() or trimap.device != labels.device:
        raise ValueError("%s: trimap must be a contiguous int64 tensor of shape %s on %s, got %s" % (
            what, (K, 3, n), labels.device,
            (trimap.dtype, tuple(trimap.shape), trimap.stride(), trimap.device) if torch.is_tensor(trimap) else type(trimap)))
    if dist is None:
        dist = seg_distance(gt, radii[-1], border)
    else:
        _distance_plane(what, "dist", dist, labels, (("trimap", trimap),))
    table = (c_int * K)(*radii)
    _check(lib().ifseg_seg_trimap_areas(_ptr(labels), c_int(labels.element_size()), _ptr(gt), c_int(gt.element_size()), _ptr(dist),
                                        c_int(B), c_int(H), c_int(W), c_int(n), table, c_int(K), c_int(1 if raw_labels else 0),
                                        _ptr(trimap), _stream()), what)
    return trimap, dist


def seg_score(scores, hp, wp, gt, raw_labels=True, labels=False, conf=False, probs=False, areas=None, tally=None,
              staging_bytes=None, label_dtype=None):
    """`seg_predict` at gt's own [B, h, w] with the scoring in the kernel's epilogue: -> (areas, tally, labels | None,
    conf | None, probs | None).  The counters are `seg_areas`' of the labels the launch decides on, whether it writes them or
    not; the three outputs are optional, and with none of them the launch writes nothing but counters.  What is written is
    `seg_predict`'s, bit for bit.  areas / tally given: accumulated into.  staging_bytes, label_dtype: as in `seg_predict`."""
    return _seg_launch(_seg_single(scores, hp, wp), None, gt, raw_labels=raw_labels, labels=labels, conf=conf, probs=probs,
                       areas=areas, tally=tally, staging_bytes=staging_bytes, label_dtype=label_dtype)


def seg_score_views(views, gt, raw_labels=True, labels=False, conf=False, probs=False, areas=None, tally=None,
                    staging_bytes=None, label_dtype=None):
    """`seg_predict_views` at gt's own [B, h, w] with the scoring in the kernel's epilogue; arguments and results as
    `seg_score`, `views` as in `seg_predict_views`."""
    return _seg_launch(_seg_views(views), None, gt, raw_labels=raw_labels, labels=labels, conf=conf, probs=probs, areas=areas,
                       tally=tally, staging_bytes=staging_bytes, label_dtype=label_dtype)


SLIDE_MAX_WINDOWS = 64       # == IFSEG_SLIDE_MAX_WINDOWS of include/ifseg_hip.h


def _slide_geometry(oh, ow, crop, stride):
    """-> (oh, ow, (crop_h, crop_w), (stride_h, stride_w), Nw, ch, cw) by `imageio.slide_windows`, whose refusals become
    assertions here as every other precondition of a binding"""
    from .imageio import _pair, slide_windows
    try:
        ys, xs, ch, cw = slide_windows(oh, ow, crop, stride)
    except ValueError as e:
        raise AssertionError(str(e))
    return int(oh), int(ow), _pair(crop, "crop"), _pair(stride, "stride"), len(ys) * len(xs), ch, cw


def _windows_scores(scores, hpw, wpw, nw):
    assert scores.dtype == torch.float32 and scores.dim() == 4 and scores.is_contiguous(), (scores.dtype, tuple(scores.shape), scores.stride())
    B, Nw, P, n = scores.shape
    assert Nw == nw, (tuple(scores.shape), "the window rule gives %d windows" % nw)
    assert P == hpw * wpw and B >= 1 and hpw >= 1 and wpw >= 1, (tuple(scores.shape), hpw, wpw)
    assert 1 <= n <= SEG_PREDICT_MAX_CLASSES, n
    assert Nw * P < 2 ** 22, (Nw, P)
    return B, n


def seg_predict_windows(scores, hpw, wpw, oh, ow, crop, stride, h, w, conf=False, probs=False, staging_bytes=None, label_dtype=None):
    """Sliding-window inference, the merge: scores fp32 [B, Nw, hpw*wpw, n], window k of `imageio.slide_windows(oh, ow, crop,
    stride)` having run the network on its own hpw x wpw grid -> (labels, conf, probs) at h x w as `seg_predict`: every window
    resized to its (ch, cw) by seg_predict's rule, the windows that cover a pixel of the [oh, ow] plane added in window order
    and divided by their number, the result resized to h x w, in ONE launch (csrc/predict.hip) that writes neither a window's
    [n, ch, cw] tensor nor the plane; `predict.slide_reference` is the specification.  One window that covers the plane and
    (h, w) == (oh, ow) give seg_predict's outputs bit for bit.  crop, stride: an int or an (h, w) pair each.
    staging_bytes, label_dtype: as in `seg_predict`."""
    return _seg_launch(_seg_windows(scores, hpw, wpw, oh, ow, crop, stride), (h, w), None, conf=conf, probs=probs,
                       staging_bytes=staging_bytes, label_dtype=label_dtype)


def _seg_windows(scores, hpw, wpw, oh, ow, crop, stride):
    """the inputs of seg_predict_windows and seg_score_windows, checked -> `_seg_launch`'s first argument"""
    oh, ow, crop, stride, nw, _, _ = _slide_geometry(oh, ow, crop, stride)
    B, n = _windows_scores(scores, hpw, wpw, nw)
    head = lambda: (_ptr(scores), c_int(B), c_int(hpw), c_int(wpw), c_int(n), c_int(oh), c_int(ow), c_int(crop[0]), c_int(crop[1]),
                    c_int(stride[0]), c_int(stride[1]))
    return (("ifseg_seg_predict_windows", "ifseg_seg_score_windows", "ifseg_seg_predict_windows_staging"), head, (), B, n,
            scores.device)


def seg_score_windows(scores, hpw, wpw, oh, ow, crop, stride, gt, raw_labels=True, labels=False, conf=False, probs=False,
                      areas=None, tally=None, staging_bytes=None, label_dtype=None):
    """`seg_predict_windows` at gt's own [B, h, w] with the scoring in the kernel's epilogue; results as `seg_score`."""
    return _seg_launch(_seg_windows(scores, hpw, wpw, oh, ow, crop, stride), None, gt, raw_labels=raw_labels, labels=labels,
                       conf=conf, probs=probs, areas=areas, tally=tally, staging_bytes=staging_bytes, label_dtype=label_dtype)


class _SlideView(ctypes.Structure):
    _fields_ = [("scores", c_void_p), ("hpw", c_int), ("wpw", c_int), ("oh", c_int), ("ow", c_int), ("flip", c_int)]


def _seg_slide_views(views, crop, stride, softmax):
    """the inputs of seg_predict_slide_views and seg_score_slide_views, checked -> `_seg_launch`'s first argument"""
    views = list(views)
    assert 1 <= len(views) <= SEG_PREDICT_MAX_VIEWS, len(views)
    B = n = dev = None
    planes = []
    for k, (scores, hpw, wpw, oh, ow, flip) in enumerate(views):
        oh, ow, cr, st, nw, _, _ = _slide_geometry(oh, ow, crop, stride)
        b, m = _windows_scores(scores, hpw, wpw, nw)
        if k == 0:
            B, n, dev = b, m, scores.device
        assert b == B and m == n and scores.device == dev, (k, tuple(scores.shape), B, n)
        planes.append((oh, ow))

    def head():
        table = (_SlideView * len(views))()
        for k, (scores, hpw, wpw, _, _, flip) in enumerate(views):
            table[k] = _SlideView(_ptr(scores), int(hpw), int(wpw), *planes[k], 1 if flip else 0)
        return table, c_int(len(views)), c_int(B), c_int(n), c_int(cr[0]), c_int(cr[1]), c_int(st[0]), c_int(st[1])

    return (("ifseg_seg_predict_slide_views", "ifseg_seg_score_slide_views", "ifseg_seg_predict_slide_views_staging"), head,
            (c_int(1 if softmax else 0),), B, n, dev)


def seg_predict_slide_views(views, crop, stride, h, w, softmax, conf=False, probs=False, staging_bytes=None, label_dtype=None):
    """Multi-scale + flip over sliding windows, the merge: views is a list of 1 .. 16 (scores fp32 [B, Nw, hpw*wpw, n], hpw, wpw,
    oh, ow, flip), each an input of `seg_predict_windows` at its own [oh, ow] plane under the call's crop and stride; flip: the
    network saw the resized image mirrored -> (labels, conf, probs) at h x w as `seg_predict`, of the MEAN of the views: every
    view merged and resized by seg_predict_windows' rule (a flipped one taken at the mirrored column), with `softmax`
    normalised over the classes per pixel (mmseg's order: logits merged, then softmax), the values added in fp32 in view order
    and multiplied by float(1 / K), in ONE launch (csrc/predict.hip); `predict.slide_views_reference` is the specification.
    One unflipped view without softmax gives seg_predict_windows' outputs bit for bit.  crop, stride: an int or an (h, w) pair
    each.  staging_bytes, label_dtype: as in `seg_predict`."""
    return _seg_launch(_seg_slide_views(views, crop, stride, softmax), (h, w), None, conf=conf, probs=probs,
                       staging_bytes=staging_bytes, label_dtype=label_dtype)


def seg_score_slide_views(views, crop, stride, gt, softmax, raw_labels=True, labels=False, conf=False, probs=False, areas=None,
                          tally=None, staging_bytes=None, label_dtype=None):
    """`seg_predict_slide_views` at gt's own [B, h, w] with the scoring in the kernel's epilogue; results as `seg_score`."""
    return _seg_launch(_seg_slide_views(views, crop, stride, softmax), None, gt, raw_labels=raw_labels, labels=labels,
                       conf=conf, probs=probs, areas=areas, tally=tally, staging_bytes=staging_bytes, label_dtype=label_dtype)


# --------------------------------------------------------------------------- the label map as a picture
SEG_RENDER_MAX_BOUNDARY = 4


def render_alpha(opacity):
    """the opacity in 256ths, floor(opacity * 256 + 0.5): the `alpha` of ifseg_seg_render"""
    assert 0.0 <= float(opacity) <= 1.0, opacity
    return int(float(opacity) * 256.0 + 0.5)


def _overlap(a, b):
    sa, sb = a.data_ptr(), b.data_ptr()
    return a.device == b.device and sa < sb + b.numel() * b.element_size() and sb < sa + a.numel() * a.element_size()


def seg_render(labels, image, palette, opacity=0.5, boundary=0, boundary_color=(255, 255, 255), conf=None, out=None):
    """labels uint8 / int16 [H, W] or [B, H, W], image uint8 [.., H, W, 3] (HWC), palette uint8 [n, 3], 1 <= n <= 512 -> the
    picture uint8 [.., H, W, 3] in one launch (csrc/render.hip): the palette's colour blended over the image at `opacity`
    (in 256ths, by `conf` fp32 [.., H, W] per pixel when given), a label outside the palette keeps the image's pixel, and with
    boundary = r in 1..4 every pixel with another label value within r pixels becomes `boundary_color`.
    `predict.render_reference` is the specification and states the rule; opacity 0.5 is the reference demo's "overlap" picture,
    1.0 its "segmentation" picture, bit for bit.  Every tensor contiguous, at any byte (labels: element) offset of its
    storage; out: written in place when given, it must not overlap image or labels."""
    assert labels.dtype in (torch.uint8, torch.int16) and labels.dim() in (2, 3) and labels.is_contiguous(), \
        (labels.dtype, tuple(labels.shape), labels.stride())
    assert image.dtype == torch.uint8 and image.is_contiguous() and tuple(image.shape) == tuple(labels.shape) + (3,) \
        and image.device == labels.device, (image.dtype, tuple(image.shape), image.stride(), tuple(labels.shape), image.device)
    assert palette.dtype == torch.uint8 and palette.dim() == 2 and palette.shape[1] == 3 and palette.is_contiguous() \
        and 1 <= palette.shape[0] <= SEG_PREDICT_MAX_CLASSES and palette.device == labels.device, \
        (palette.dtype, tuple(palette.shape), palette.stride(), palette.device)
    assert isinstance(boundary, int) and 0 <= boundary <= SEG_RENDER_MAX_BOUNDARY, boundary
    rgb = tuple(int(c) for c in boundary_color)
    assert len(rgb) == 3 and all(0 <= c <= 255 for c in rgb) and rgb == tuple(boundary_color), boundary_color
    alpha = render_alpha(opacity)
    assert 1 <= labels.numel() < 2 ** 31, tuple(labels.shape)
    if conf is not None:
        assert conf.dtype == torch.float32 and conf.shape == labels.shape and conf.is_contiguous() and conf.device == labels.device, \
            (conf.dtype, tuple(conf.shape), conf.stride(), conf.device)
    if out is None:
        out = torch.empty_like(image)
    assert out.dtype == torch.uint8 and out.shape == image.shape and out.is_contiguous() and out.device == image.device, \
        (out.dtype, tuple(out.shape), out.stride(), out.device)
    assert not _overlap(out, image) and not _overlap(out, labels), "seg_render: out overlaps the image or the labels"
    H, W = labels.shape[-2:]
    _check(lib().ifseg_seg_render(_ptr(labels), c_int(labels.element_size()), _ptr(image), _ptr(palette), c_int(palette.shape[0]),
                                  _ptr(conf), c_int(labels.numel() // (H * W)), c_int(H), c_int(W), c_int(alpha), c_int(boundary),
                                  c_int(rgb[0] | rgb[1] << 8 | rgb[2] << 16), _ptr(out), _stream()), "seg_render")
    return out


# --------------------------------------------------------------------------- confidence-filtered pseudo-labels
SEG_CONF_BINS = 256                 # bins of the confidence histogram: clamp(floor(conf * 256), 0, 255)
SEG_CONF_HIST_DIRECT_CLASSES = 64   # == HC_DIRECT_CLASSES (csrc/pseudo.hip): n up to this counts in a direct LDS table, else hashed
SEG_CONF_HIST_SLOTS = SEG_CONFUSION_SLOTS   # the same table (count::SLOTS): the (label, bin) pairs a workgroup's hashed table holds
SEG_PSEUDO_MAX_CLASSES = 255        # the uint8 output keeps 255 for "ignore"; with raw_labels class c is stored as c + 1: 254


def seg_pseudo_max_classes(raw_labels=True):
    return SEG_PSEUDO_MAX_CLASSES - 1 if raw_labels else SEG_PSEUDO_MAX_CLASSES


def seg_conf_hist(labels, conf, n, hist=None, tally=None):
    """labels uint8 / int16 [...] (predicted classes), conf fp32 of the same shape -> (hist int64 [n, 256], tally int64 [2]):
    hist[c, b] = #(label = c and clamp(floor(conf * 256), 0, 255) = b), tally = #labels in [0, n), #labels outside
    (csrc/pseudo.hip; `predict.confidence_histogram_reference` is the specification).  `hist` / `tally` given: ACCUMULATED
    into, else fresh zeroed ones.  1 <= n <= 512."""
    _label_maps("seg_conf_hist", labels, conf, None, n)
    hist, tally = _counter(hist, (n, SEG_CONF_BINS), labels.device), _counter(tally, (2,), labels.device)
    _check(lib().ifseg_seg_conf_hist(_ptr(labels), c_int(labels.element_size()), _ptr(conf), c_ll(labels.numel()), c_int(n),
                                     _ptr(hist), _ptr(tally), _stream()), "seg_conf_hist")
    return hist, tally


# the tables of seg_calibration_kernel (csrc/calib.hip, csrc/count.h)
SEG_CALIBRATION_DIRECT_CLASSES = 32             # == CB_DIRECT_CLASSES: n up to this counts in a direct LDS table (n * 512 dwords), else hashed
SEG_CALIBRATION_SLOTS = SEG_CONFUSION_SLOTS     # the same table (count::SLOTS): the (label, bin, hit) keys a workgroup's hashed table holds
SEG_CALIBRATION_STEP_PIXELS = SEG_CONFUSION_STEP_PIXELS
SEG_CALIBRATION_MAX_BLOCKS = SEG_CONFUSION_MAX_BLOCKS


def seg_calibration_limits():
    """-> (direct classes, hashed slots, pixels per workgroup step, workgroups at most) as the loaded library states them
    (`ifseg_seg_calibration_limit`): the four constants above, which the tests hold against it"""
    return _limits("ifseg_seg_calibration_limit", 4)


def seg_calibration(labels, conf, gt, n, raw_labels=True, calibration=None, tally=None):
    """labels uint8 / int16 [...] (predicted classes), conf fp32 and gt uint8 / int16 of the same shape -> (calibration int64
    [n, 256, 2], tally int64 [2]): over the scored pixels of `seg_areas`, calibration[l, b, hit] = #(label = l in [0, n),
    clamp(floor(conf * 256), 0, 255) = b, (l == gt class) = hit); tally = #scored pixels with a label in [0, n), #scored pixels
    with a label outside (csrc/calib.hip; `predict.calibration_reference` is the specification).  `calibration` / `tally`
    given: ACCUMULATED into and returned, else fresh zeroed ones.  One launch on the current stream.  1 <= n <= 512."""
    _label_maps("seg_calibration", labels, conf, gt, n)
    calibration = _counter(calibration, (n, SEG_CONF_BINS, 2), labels.device)
    tally = _counter(tally, (2,), labels.device)
    _check(lib().ifseg_seg_calibration(_ptr(labels), c_int(labels.element_size()), _ptr(conf), _ptr(gt), c_int(gt.element_size()),
                                       c_ll(labels.numel()), c_int(n), c_int(1 if raw_labels else 0), _ptr(calibration),
                                       _ptr(tally), _stream()), "seg_calibration")
    return calibration, tally


# the limits of seg_tsweep_kernel (csrc/tsweep.hip)
SEG_SWEEP_MAX_TEMPERATURES = 16     # == TS_MAX_K: the grids of one launch at most (2 KiB of LDS table each)
SEG_SWEEP_STAGING_BYTES = 31728     # == ts_stage_limit(16): what 16 tables and the waves' sums leave of 64 KiB for the footprint


def seg_temperature_sweep_limits():
    """-> (the largest K, the largest n, a tile's rows, a tile's columns, the staging bytes at the largest K) as the loaded
    library states them (`ifseg_seg_temperature_sweep_limit`): SEG_SWEEP_MAX_TEMPERATURES, SEG_PREDICT_MAX_CLASSES, 16, 64 and
    SEG_SWEEP_STAGING_BYTES, which the tests hold against it"""
    return _limits("ifseg_seg_temperature_sweep_limit", 5)


def seg_temperature_sweep(grids, hp, wp, gt, raw_labels=True, hist=None, sums=None, tally=None, staging_bytes=None):
    """grids fp32 [K, B, hp*wp, n], contiguous: K grids of class PROBABILITIES of the same images (what `rows_to_f32(softmax=True,
    temperature=T_k)` / `neighbour_smoothing(..., T_k)` return, stacked), 1 <= K <= SEG_SWEEP_MAX_TEMPERATURES; gt uint8 / int16
    [B, h, w] -> (hist int64 [K, 256, 2], sums float64 [K, 2], tally int64 [2]): every grid resized to gt's size by `seg_predict`'s
    rule, bit for bit, and over `seg_areas`' scored pixels hist[k, bin(conf_k), label_k == gt class] += 1,
    sums[k, 0] += -log(max(p_k[gt class], FLT_MIN)), sums[k, 1] += sum_c p_kc^2 - 2 p_k[gt class] + 1 (both in fp64 on the
    fp32 values); tally = #scored pixels, #pixels with a ground truth out of range (csrc/tsweep.hip;
    `predict.temperature_sweep_reference` is the specification).  One launch for all K and a small one that adds the tiles' sums
    in a fixed order: two calls give equal bits, nothing synchronises, and no [n, h, w] tensor exists.  `hist` / `sums` / `tally`
    given: ACCUMULATED into and returned, else fresh zeroed ones.  staging_bytes: as in `seg_predict`."""
    assert grids.dtype == torch.float32 and grids.dim() == 4 and grids.is_contiguous(), (grids.dtype, tuple(grids.shape), grids.stride())
    K, B, P, n = grids.shape
    assert 1 <= K <= SEG_SWEEP_MAX_TEMPERATURES and 1 <= n <= SEG_PREDICT_MAX_CLASSES, (K, n)
    assert P == hp * wp and B >= 1 and hp >= 1 and wp >= 1, (tuple(grids.shape), hp, wp)
    dev = grids.device
    h, w = _score_gt(gt, B, dev)
    assert B * h * w < 2 ** 31, (B, h, w)
    hist, tally = _counter(hist, (K, SEG_CONF_BINS, 2), dev), _counter(tally, (2,), dev)
    if sums is None:
        sums = torch.zeros(K, 2, dtype=torch.float64, device=dev)
    assert sums.dtype == torch.float64 and tuple(sums.shape) == (K, 2) and sums.is_contiguous() and sums.device == dev, \
        (sums.dtype, tuple(sums.shape), sums.stride(), sums.device)
    partials = torch.empty(B * ((h + 15) // 16) * ((w + 63) // 64), K, 2, dtype=torch.float64, device=dev)
    with _staged("ifseg_seg_temperature_sweep_staging", staging_bytes):
        _check(lib().ifseg_seg_temperature_sweep(_ptr(grids), c_int(K), c_int(B), c_int(hp), c_int(wp), c_int(n), c_int(h), c_int(w),
                                                 _ptr(gt), c_int(gt.element_size()), c_int(1 if raw_labels else 0), _ptr(hist),
                                                 _ptr(tally), _ptr(sums), _ptr(partials), _stream()), "seg_temperature_sweep")
    return hist, sums, tally


# the limits of seg_score_grids_kernel (csrc/bsweep.hip)
SEG_SCORE_GRIDS_MAX = 16                    # == BS_MAX_K: the grids of one launch at most
SEG_SCORE_GRIDS_STAGING_BYTES = 59376       # == bs_stage_limit(512): what the [3][512] table (+ tallies) leaves of 64 KiB


def seg_score_grids_limits():
    """-> (the largest K, the largest n, a tile's rows, a tile's columns, the staging bytes at the largest K and n) as the
    loaded library states them (`ifseg_seg_score_grids_limit`): SEG_SCORE_GRIDS_MAX, SEG_PREDICT_MAX_CLASSES, 16, 64 and
    SEG_SCORE_GRIDS_STAGING_BYTES, which the tests hold against it"""
    return _limits("ifseg_seg_score_grids_limit", 5)


def seg_score_grids(grids, hp, wp, gt, raw_labels=True, areas=None, tally=None, staging_bytes=None):
    """grids fp32 [K, B, hp*wp, n], contiguous: K score grids of the same images, ANY fp32 values (probabilities or logits:
    what `rows_to_f32_biased` / `neighbour_smoothing(bias=)` return for K biases, stacked), 1 <= K <= SEG_SCORE_GRIDS_MAX; gt
    uint8 / int16 [B, h, w] -> (areas int64 [K, 3, n], tally int64 [2]): every grid resized to gt's size by `seg_predict`'s
    rule and its label map counted against gt; row k is bit for bit `seg_score(grids[k], hp, wp, gt, raw_labels)`'s areas, and
    tally (#scored pixels, #pixels with a ground truth out of range) is added ONCE, not K times (csrc/bsweep.hip;
    `predict.bias_sweep_reference` is the specification).  One launch for all K, integers only: two calls give equal bits,
    nothing synchronises, and no [n, h, w] tensor exists.  `areas` / `tally` given: ACCUMULATED into and returned, else fresh
    zeroed ones.  staging_bytes: as in `seg_predict`."""
    assert grids.dtype == torch.float32 and grids.dim() == 4 and grids.is_contiguous(), (grids.dtype, tuple(grids.shape), grids.stride())
    K, B, P, n = grids.shape
    assert 1 <= K <= SEG_SCORE_GRIDS_MAX and 1 <= n <= SEG_PREDICT_MAX_CLASSES, (K, n)
    assert P == hp * wp and B >= 1 and hp >= 1 and wp >= 1, (tuple(grids.shape), hp, wp)
    dev = grids.device
    h, w = _score_gt(gt, B, dev)
    assert B * h * w < 2 ** 31, (B, h, w)
    areas, tally = _counter(areas, (K, 3, n), dev), _counter(tally, (2,), dev)
    with _staged("ifseg_seg_score_grids_staging", staging_bytes):
        _check(lib().ifseg_seg_score_grids(_ptr(grids), c_int(K), c_int(B), c_int(hp), c_int(wp), c_int(n), c_int(h), c_int(w),
                                           _ptr(gt), c_int(gt.element_size()), c_int(1 if raw_labels else 0), _ptr(areas),
                                           _ptr(tally), _stream()), "seg_score_grids")
    return areas, tally


def seg_pseudo(labels, conf, thresholds, n, boundary=0, raw_labels=True, kept=None, out=None, weight=False):
    """labels uint8 / int16 [H, W] or [B, H, W], conf fp32 of the same shape, thresholds int32 [n] (bins, 0 .. 256) ->
    (out uint8 of the labels' shape, kept int64 [2, n]) in one launch (csrc/pseudo.hip): a pixel of label l in [0, n) whose
    confidence bin is at least thresholds[l] and, with boundary = r in 1..4, that has no other label value within r pixels
    becomes l + 1 (raw_labels: the label-PNG convention `augment.remap_label` undoes) or l, every other pixel 255.
    kept[1, c] = #(label = c), kept[0, c] = those kept; `kept` given: ACCUMULATED into.  out: written in place when given
    (contiguous, at any byte offset of its storage; it must not overlap labels or conf).
    `predict.pseudo_label_reference` is the specification.  n <= 254 with raw_labels, 255 without.
    weight=True: the same launch also writes the loss weight of every pixel, and the call returns (out, kept, weight uint8 of
    the labels' shape): 0 where out is 255, max(conf_bin(conf), 1) where the pixel was kept."""
    assert labels.dim() in (2, 3), tuple(labels.shape)
    _label_maps("seg_pseudo", labels, conf, None)
    assert isinstance(n, int) and 1 <= n <= seg_pseudo_max_classes(raw_labels), (n, raw_labels)
    assert isinstance(boundary, int) and 0 <= boundary <= SEG_RENDER_MAX_BOUNDARY, boundary
    dev = labels.device
    assert thresholds.dtype == torch.int32 and tuple(thresholds.shape) == (n,) and thresholds.is_contiguous() \
        and thresholds.device == dev, (thresholds.dtype, tuple(thresholds.shape), thresholds.device, n)
    kept = _counter(kept, (2, n), dev)
    if out is None:
        out = torch.empty(labels.shape, dtype=torch.uint8, device=dev)
    assert out.dtype == torch.uint8 and out.shape == labels.shape and out.is_contiguous() and out.device == dev, \
        (out.dtype, tuple(out.shape), out.stride(), out.device)
    assert not _overlap(out, labels) and not _overlap(out, conf), "seg_pseudo: out overlaps the labels or conf"
    H, W = labels.shape[-2:]
    if weight:
        wt = torch.empty(labels.shape, dtype=torch.uint8, device=dev)
        _check(lib().ifseg_seg_pseudo_weighted(_ptr(labels), c_int(labels.element_size()), _ptr(conf), _ptr(thresholds), c_int(n),
                                               c_int(labels.numel() // (H * W)), c_int(H), c_int(W), c_int(boundary),
                                               c_int(1 if raw_labels else 0), _ptr(out), _ptr(wt), _ptr(kept), _stream()),
               "seg_pseudo_weighted")
        return out, kept, wt
    _check(lib().ifseg_seg_pseudo(_ptr(labels), c_int(labels.element_size()), _ptr(conf), _ptr(thresholds), c_int(n),
                                  c_int(labels.numel() // (H * W)), c_int(H), c_int(W), c_int(boundary),
                                  c_int(1 if raw_labels else 0), _ptr(out), _ptr(kept), _stream()), "seg_pseudo")
    return out, kept


# --------------------------------------------------------------------------- connected regions of a label map (csrc/regions.hip)
SEG_REGION_MAX_CLASSES = 255        # == RG_MAX_CLASSES: the classes of seg_region_drop's counter, the values of a uint8 map


def seg_regions_limits():
    """-> (a tile's rows, a tile's columns, the largest n of the drop) as the loaded library states them
    (`ifseg_seg_regions_limit`): 16, 64 and SEG_REGION_MAX_CLASSES, which the tests hold against it"""
    return _limits("ifseg_seg_regions_limit", 3)


def _region_maps(what, labels, connectivity, dtypes):
    """what the region kernels ask of a label map, as ValueErrors that name the argument -> (B, H, W)"""
    if not torch.is_tensor(labels) or labels.dtype not in dtypes:
        raise ValueError("%s: labels must be a %s tensor, got %s" % (
            what, " / ".join(str(d).replace("torch.", "") for d in dtypes), labels.dtype if torch.is_tensor(labels) else type(labels)))
    if labels.dim() not in (2, 3) or not labels.is_contiguous() or not 1 <= labels.numel() < 2 ** 31:
        raise ValueError("%s: labels must be contiguous [H, W] or [B, H, W] with 1 .. 2**31 - 1 pixels, got %s with strides %s"
                         % (what, tuple(labels.shape), labels.stride()))
    if not isinstance(connectivity, int) or isinstance(connectivity, bool) or connectivity not in (4, 8):
        raise ValueError("%s: connectivity must be the int 4 or 8, got %r" % (what, connectivity))
    H, W = labels.shape[-2:]
    return labels.numel() // (H * W), int(H), int(W)


def _region_plane(what, name, t, labels, dtype=torch.int32):
    """an output plane of the labels' shape: the caller's, checked, or a fresh one"""
    if t is None:
        return torch.empty(labels.shape, dtype=dtype, device=labels.device)
    if not torch.is_tensor(t) or t.dtype != dtype or t.shape != labels.shape or not t.is_contiguous() or t.device != labels.device:
        raise ValueError("%s: %s must be a contiguous %s tensor of the labels' shape %s on %s, got %s" % (
            what, name, str(dtype).replace("torch.", ""), tuple(labels.shape), labels.device,
            (t.dtype, tuple(t.shape), t.stride(), t.device) if torch.is_tensor(t) else type(t)))
    if _overlap(t, labels):
        raise ValueError("%s: %s overlaps the labels" % (what, name))
    return t


def _region_flag(what, flag, dev):
    if flag is None:
        return torch.zeros(1, dtype=torch.int32, device=dev)
    if not torch.is_tensor(flag) or flag.dtype != torch.int32 or flag.numel() != 1 or flag.device != dev:
        raise ValueError("%s: flag must be an int32 tensor of one element on %s, got %s" % (
            what, dev, (flag.dtype, tuple(flag.shape), flag.device) if torch.is_tensor(flag) else type(flag)))
    return flag


def seg_regions(labels, connectivity=4, root=None, size=None, flag=None):
    """labels uint8 / int16 [H, W] or [B, H, W] -> (root, size), both int32 of the labels' shape (csrc/regions.hip;
    `predict.regions_reference` is the specification and states the rule): root[p] = the smallest y W + x inside its image
    over the pixels of p's connected region of equal values (connectivity 4 or 8), size[p] = the region's pixel count.  Four
    launches on the current stream (three where an image is one 16 x 64 tile), nothing synchronises; the results are
    canonical, so two calls give equal bits.  root / size: written in place when given (contiguous int32).  flag: an int32
    word that a thread whose loop ran out of its step budget sets to 1 -- it stays 0; given: never cleared here, so one word
    can watch many calls (pass your own to read it), else a fresh zeroed one.
    The two int32 work planes of the labels' shape are allocated here.  Bad arguments: ValueError, before anything is
    launched."""
    what = "seg_regions"
    B, H, W = _region_maps(what, labels, connectivity, (torch.uint8, torch.int16))
    root, size = _region_plane(what, "root", root, labels), _region_plane(what, "size", size, labels)
    if root is size or _overlap(root, size):
        raise ValueError("%s: root and size overlap" % what)
    flag = _region_flag(what, flag, labels.device)
    work = torch.empty(2, B, H, W, dtype=torch.int32, device=labels.device)
    _check(lib().ifseg_seg_regions(_ptr(labels), c_int(labels.element_size()), c_int(B), c_int(H), c_int(W), c_int(connectivity),
                                   _ptr(work[0]), _ptr(work[1]), _ptr(root), _ptr(size), _ptr(flag), _stream()), "seg_regions")
    return root, size


def seg_region_drop(labels, connectivity=4, min_region=1, fill=255, n=None, raw_labels=True, weight=None, out=None, dropped=None,
                    flag=None):
    """labels uint8 [H, W] or [B, H, W] -> (out uint8 of the labels' shape, dropped int64 [n], size int32 of the labels'
    shape): `seg_regions` with the drop rule in its last launch (`predict.region_drop_reference` states it): a pixel whose
    value is not `fill` and whose region holds fewer than min_region pixels becomes `fill`, every other pixel is copied.
    weight uint8 of the labels' shape: its dropped pixels are set to 0 IN PLACE.  dropped[c] = the dropped pixels of class c
    (value - 1 with raw_labels, else the value; values outside [0, n) are dropped but not counted); given: ACCUMULATED into.
    n None: every class a uint8 map holds (254 with raw_labels, 255 without).  out: written in place when given; it must
    not overlap labels.  flag: as in `seg_regions`.  Bad arguments: ValueError, before anything is launched."""
    what = "seg_region_drop"
    B, H, W = _region_maps(what, labels, connectivity, (torch.uint8,))
    if not isinstance(min_region, int) or isinstance(min_region, bool) or not 1 <= min_region < 2 ** 31:
        raise ValueError("%s: min_region must be an int in 1 .. 2**31 - 1 (1 drops nothing), got %r" % (what, min_region))
    if not isinstance(fill, int) or isinstance(fill, bool) or not 0 <= fill <= 255:
        raise ValueError("%s: fill must be an int in 0 .. 255, got %r" % (what, fill))
    if n is None:
        n = seg_pseudo_max_classes(raw_labels)
    if not isinstance(n, int) or isinstance(n, bool) or not 1 <= n <= SEG_REGION_MAX_CLASSES:
        raise ValueError("%s: n must be an int in 1 .. %d, got %r" % (what, SEG_REGION_MAX_CLASSES, n))
    dev = labels.device
    out = _region_plane(what, "out", out, labels, torch.uint8)
    if weight is not None:
        _region_plane(what, "weight", weight, labels, torch.uint8)
        if _overlap(weight, out):
            raise ValueError("%s: weight overlaps out" % what)
    if dropped is None:
        dropped = torch.zeros(n, dtype=torch.int64, device=dev)
    elif not torch.is_tensor(dropped) or dropped.dtype != torch.int64 or tuple(dropped.shape) != (n,) \
            or not dropped.is_contiguous() or dropped.device != dev:
        raise ValueError("%s: dropped must be a contiguous int64 [%d] tensor on %s, got %s" % (
            what, n, dev, (dropped.dtype, tuple(dropped.shape), dropped.device) if torch.is_tensor(dropped) else type(dropped)))
    flag = _region_flag(what, flag, dev)
    work = torch.empty(3, B, H, W, dtype=torch.int32, device=dev)
    size = torch.empty(labels.shape, dtype=torch.int32, device=dev)
    _check(lib().ifseg_seg_region_drop(_ptr(labels), c_int(B), c_int(H), c_int(W), c_int(connectivity), c_int(min_region),
                                       c_int(fill), c_int(n), c_int(1 if raw_labels else 0), _ptr(work[0]), _ptr(work[1]),
                                       _ptr(work[2]), _ptr(size), _ptr(out), _ptr(weight), _ptr(dropped), _ptr(flag), _stream()),
           "seg_region_drop")
    return out, dropped, size


# --------------------------------------------------------------------------- the sieve of a label map (csrc/sieve.hip)
SEG_SIEVE_MAX_PASSES = 8            # == SV_MAX_PASSES: the passes of a call at most
SEG_SIEVE_MAX_CLASSES = 512         # == SV_MAX_CLASSES: the classes of the moved counter


def seg_sieve_limits():
    """-> (a tile's rows, a tile's columns, the passes of a call at most, the largest n) as the loaded library states them
    (`ifseg_seg_sieve_limit`): 16, 64, SEG_SIEVE_MAX_PASSES and SEG_SIEVE_MAX_CLASSES, which the tests hold against it"""
    return _limits("ifseg_seg_sieve_limit", 4)


def seg_sieve(labels, min_region, connectivity=4, passes=1, ignore=None, n=None, raw_labels=False, conf=None, out=None,
              moved=None, flag=None):
    """labels uint8 / int16 [H, W] or [B, H, W] -> (out of the labels' dtype and shape, moved int64 [2, n]): the sieve filter
    (csrc/sieve.hip; `predict.sieve_reference` is the specification and states the rule): per pass every connected region
    (connectivity 4 or 8) of fewer than min_region pixels whose value is not `ignore` takes the value of its 4-adjacent
    neighbour region with the largest key (size, -root), if that key exceeds its own; `passes` (1 .. SEG_SIEVE_MAX_PASSES)
    repeats it on the result.  Per pass `seg_regions`' launches and three more, on the current stream; nothing synchronises,
    and the result is canonical, so two calls give equal bits.
    conf fp32 of the labels' shape: set to 0 IN PLACE where out != labels.  moved[0, c] / moved[1, c]: the pixels that left /
    joined class c (value - 1 with raw_labels, else the value; values outside [0, n) are not counted); given: ACCUMULATED
    into.  n None: SEG_SIEVE_MAX_CLASSES.  out: written in place when given; it must not overlap labels.  flag: as in
    `seg_regions`.  The work planes are allocated here: four int32 and one uint64 of the labels' shape, and with passes > 1 one
    more map of the labels' dtype (about 25 bytes per pixel live during a call).  Bad arguments: ValueError, before anything is
    launched."""
    what = "seg_sieve"
    B, H, W = _region_maps(what, labels, connectivity, (torch.uint8, torch.int16))
    if not isinstance(min_region, int) or isinstance(min_region, bool) or not 1 <= min_region < 2 ** 31:
        raise ValueError("%s: min_region must be an int in 1 .. 2**31 - 1 (1 moves nothing), got %r" % (what, min_region))
    if not isinstance(passes, int) or isinstance(passes, bool) or not 1 <= passes <= SEG_SIEVE_MAX_PASSES:
        raise ValueError("%s: passes must be an int in 1 .. %d, got %r" % (what, SEG_SIEVE_MAX_PASSES, passes))
    if ignore is not None and (not isinstance(ignore, int) or isinstance(ignore, bool)):
        raise ValueError("%s: ignore must be None or an int, got %r" % (what, ignore))
    if n is None:
        n = SEG_SIEVE_MAX_CLASSES
    if not isinstance(n, int) or isinstance(n, bool) or not 1 <= n <= SEG_SIEVE_MAX_CLASSES:
        raise ValueError("%s: n must be an int in 1 .. %d, got %r" % (what, SEG_SIEVE_MAX_CLASSES, n))
    dev = labels.device
    out = _region_plane(what, "out", out, labels, labels.dtype)
    if conf is not None:
        _region_plane(what, "conf", conf, labels, torch.float32)
        if _overlap(conf, out):
            raise ValueError("%s: conf overlaps out" % what)
    if moved is None:
        moved = torch.zeros(2, n, dtype=torch.int64, device=dev)
    elif not torch.is_tensor(moved) or moved.dtype != torch.int64 or tuple(moved.shape) != (2, n) \
            or not moved.is_contiguous() or moved.device != dev:
        raise ValueError("%s: moved must be a contiguous int64 [2, %d] tensor on %s, got %s" % (
            what, n, dev, (moved.dtype, tuple(moved.shape), moved.device) if torch.is_tensor(moved) else type(moved)))
    flag = _region_flag(what, flag, dev)
    lo, hi = (0, 255) if labels.dtype == torch.uint8 else (-2 ** 15, 2 ** 15 - 1)
    has_ignore = ignore is not None and lo <= ignore <= hi      # a value the map cannot hold ignores nothing
    work = torch.empty(4, B, H, W, dtype=torch.int32, device=dev)
    best = torch.empty(B, H, W, dtype=torch.int64, device=dev)
    tmp = torch.empty_like(labels) if passes > 1 else None
    _check(lib().ifseg_seg_sieve(_ptr(labels), c_int(labels.element_size()), c_int(B), c_int(H), c_int(W), c_int(connectivity),
                                 c_int(min_region), c_int(passes), c_int(ignore if has_ignore else 0),
                                 c_int(1 if has_ignore else 0), c_int(n), c_int(1 if raw_labels else 0), _ptr(work[0]),
                                 _ptr(work[1]), _ptr(work[2]), _ptr(work[3]), _ptr(best), _ptr(tmp), _ptr(out), _ptr(conf),
                                 _ptr(moved), _ptr(flag), _stream()), "seg_sieve")
    return out, moved


# --------------------------------------------------------------------------- the region table of a label map (csrc/regiontab.hip)
SEG_REGION_TABLE_MAX = 1 << 20      # == RT_MAX_REGIONS: the largest max_regions
SEG_REGION_TABLE_BLOCK = 1024       # == RT_BLOCK: the flat pixels of a block of the counting launches


def seg_region_table_limits():
    """-> (a tile's rows, a tile's columns, the flat pixels of a block, the largest max_regions) as the loaded library states
    them (`ifseg_seg_region_table_limit`): 16, 64, SEG_REGION_TABLE_BLOCK and SEG_REGION_TABLE_MAX, which the tests hold
    against it"""
    return _limits("ifseg_seg_region_table_limit", 4)


def _region_table_out(what, name, t, shape, dtype, dev, others):
    """an output of the region table: the caller's, checked against `others` (name, tensor) for shared bytes, or None"""
    if t is None:
        return None
    if not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous() or t.device != dev:
        raise ValueError("%s: %s must be a contiguous %s tensor of shape %s on %s, got %s" % (
            what, name, str(dtype).replace("torch.", ""), tuple(shape), dev,
            (t.dtype, tuple(t.shape), t.stride(), t.device) if torch.is_tensor(t) else type(t)))
    for other_name, other in others:
        if other is not None and _overlap(t, other):
            raise ValueError("%s: %s overlaps %s" % (what, name, other_name))
    return t


def seg_region_table(labels, conf=None, connectivity=4, min_region=1, ignore=None, max_regions=1024, rows=None, sums=None,
                     count=None, slot=None, flag=None):
    """labels uint8 / int16 [H, W] or [B, H, W] -> (rows int32 [B, R, 8], sums int64 [B, R, 3], count int32 [B], slot int32 of
    the labels' shape), R = max_regions and the leading B absent for an [H, W] map: the table of the map's connected regions
    (csrc/regiontab.hip; `predict.region_table_reference` is the specification and states the rule).  A region of
    `seg_regions` (connectivity 4 or 8) is listed iff it holds at least min_region pixels and its value is not `ignore`; the
    listed regions of an image are numbered in ascending order of their roots.  rows[s] = (value, root, size, x0, y0, x1, y1,
    0), the box inclusive; sums[s] = (sum x, sum y, sum q) over the region's pixels, q = clamp(floor(conf * 65536), 0, 65535)
    of conf fp32 of the labels' shape (0 without conf); count = the listed regions, which may exceed R -- rows and sums from
    min(count, R) on are not written (fresh ones are zero there); slot[p] = the row of p's region, -1 where there is none.
    `seg_regions`' launches and four more on the current stream; nothing synchronises, and every output is an integer, so two
    calls give equal bits.  rows / sums / count / slot: written in place when given.  flag: as in `seg_regions`.
    The work planes are allocated here: `seg_regions`' four int32 planes of the labels' shape and the block counts, in one
    allocation; where neither rows nor sums is given, the two (and a fresh flag word) are views of one zero-filled allocation.
    Bad arguments: ValueError naming the argument, before anything is launched."""
    what = "seg_region_table"
    B, H, W = _region_maps(what, labels, connectivity, (torch.uint8, torch.int16))
    if not isinstance(min_region, int) or isinstance(min_region, bool) or not 1 <= min_region < 2 ** 31:
        raise ValueError("%s: min_region must be an int in 1 .. 2**31 - 1 (1 lists every region), got %r" % (what, min_region))
    if ignore is not None and (not isinstance(ignore, int) or isinstance(ignore, bool)):
        raise ValueError("%s: ignore must be None or an int, got %r" % (what, ignore))
    if not isinstance(max_regions, int) or isinstance(max_regions, bool) or not 1 <= max_regions <= SEG_REGION_TABLE_MAX:
        raise ValueError("%s: max_regions must be an int in 1 .. %d, got %r" % (what, SEG_REGION_TABLE_MAX, max_regions))
    dev, R = labels.device, max_regions
    if conf is not None:
        _region_plane(what, "conf", conf, labels, torch.float32)
    lead = tuple(labels.shape[:-2])
    given = [("labels", labels), ("conf", conf)]
    outs = {}
    for name, t, shape, dtype in (("rows", rows, lead + (R, 8), torch.int32), ("sums", sums, lead + (R, 3), torch.int64),
                                  ("count", count, lead, torch.int32), ("slot", slot, tuple(labels.shape), torch.int32)):
        outs[name] = _region_table_out(what, name, t, shape, dtype, dev, given)
        given.append((name, outs[name]))
    if flag is not None:
        _region_flag(what, flag, dev)
        for name, t in given[2:]:
            if t is not None and _overlap(t, flag):
                raise ValueError("%s: %s overlaps flag" % (what, name))
    rows, sums = outs["rows"], outs["sums"]
    if rows is None and sums is None:
        # ONE zero fill for everything the call must find zeroed: the table and, behind it, a fresh flag word
        nrow = B * R
        zeroed = torch.zeros(7 * nrow + 1, dtype=torch.int64, device=dev)
        rows = zeroed[:4 * nrow].view(torch.int32).view(lead + (R, 8))
        sums = zeroed[4 * nrow:7 * nrow].view(lead + (R, 3))
        if flag is None:
            flag = zeroed[7 * nrow:].view(torch.int32)[:1]
    elif rows is None:
        rows = torch.zeros(lead + (R, 8), dtype=torch.int32, device=dev)
    elif sums is None:
        sums = torch.zeros(lead + (R, 3), dtype=torch.int64, device=dev)
    flag = _region_flag(what, flag, dev)
    count = torch.empty(lead, dtype=torch.int32, device=dev) if outs["count"] is None else outs["count"]
    slot = torch.empty(labels.shape, dtype=torch.int32, device=dev) if outs["slot"] is None else outs["slot"]
    lo, hi = (0, 255) if labels.dtype == torch.uint8 else (-2 ** 15, 2 ** 15 - 1)
    has_ignore = ignore is not None and lo <= ignore <= hi      # a value the map cannot hold ignores nothing
    npix, nblk = B * H * W, B * -(-(H * W) // SEG_REGION_TABLE_BLOCK)
    scratch = torch.empty(4 * npix + nblk, dtype=torch.int32, device=dev)
    work, blk = scratch[:4 * npix].view(4, npix), scratch[4 * npix:]
    _check(lib().ifseg_seg_region_table(_ptr(labels), c_int(labels.element_size()), _ptr(conf), c_int(B), c_int(H), c_int(W),
                                        c_int(connectivity), c_int(min_region), c_int(ignore if has_ignore else 0),
                                        c_int(1 if has_ignore else 0), c_int(R), _ptr(work[0]), _ptr(work[1]), _ptr(work[2]),
                                        _ptr(work[3]), _ptr(blk), _ptr(rows), _ptr(sums), _ptr(count), _ptr(slot), _ptr(flag),
                                        _stream()), "seg_region_table")
    return rows, sums, count, slot


# --------------------------------------------------------------------------- run-length label maps (csrc/rle.hip)
SEG_RLE_MAX_RUNS = 1 << 24          # == RL_MAX_RUNS: the largest max_runs
SEG_RLE_CHUNK = 32                  # == RL_CHUNK: the rows of a column segment of the counting launches
SEG_RLE_COLS = 64                   # == RL_COLS: the columns of a workgroup


def seg_rle_limits():
    """-> (the rows of a chunk, the columns of a workgroup, the largest max_runs) as the loaded library states them
    (`ifseg_seg_rle_limit`): SEG_RLE_CHUNK, SEG_RLE_COLS and SEG_RLE_MAX_RUNS, which the tests hold against it"""
    return _limits("ifseg_seg_rle_limit", 3)


def _rle_max_runs(what, max_runs):
    if not isinstance(max_runs, int) or isinstance(max_runs, bool) or not 1 <= max_runs <= SEG_RLE_MAX_RUNS:
        raise ValueError("%s: max_runs must be an int in 1 .. %d, got %r" % (what, SEG_RLE_MAX_RUNS, max_runs))
    return max_runs


def _rle_runs(what, runs, shape, dev):
    """a run table: contiguous int32 of `shape` on `dev`, at an 8-byte aligned address (a run is one 8-byte word)"""
    if not torch.is_tensor(runs) or runs.dtype != torch.int32 or tuple(runs.shape) != tuple(shape) or not runs.is_contiguous() \
            or runs.device != dev or runs.data_ptr() % 8:
        raise ValueError("%s: runs must be a contiguous, 8-byte aligned int32 tensor of shape %s on %s, got %s" % (
            what, tuple(shape), dev, (runs.dtype, tuple(runs.shape), runs.stride(), runs.device, runs.data_ptr() % 8)
            if torch.is_tensor(runs) else type(runs)))
    return runs


def seg_rle_encode(labels, max_runs=65536, runs=None, count=None):
    """labels uint8 / int16 [H, W] or [B, H, W] -> (runs int32 [B, R, 2], count int32 [B]), R = max_runs and the leading B
    absent for an [H, W] map: the map's runs in COCO's run order (csrc/rle.hip; `predict.rle_encode_reference` is the
    specification and states the rule).  Per image f[i] = labels[i % H, i // H]; position i starts a run iff i == 0 or
    f[i] != f[i - 1]; runs[s] = (start, value) for s < min(count, R), in ascending order of start; count may exceed R -- entries
    from min(count, R) on are not written (a table allocated here is zero there).  Three launches on the current stream,
    nothing synchronises; integers with one writer per word, so two calls give equal bits.  runs / count: written in place when
    given.  The segment counts (int32, W ceil(H / 32) per image) are allocated here, and, where no runs is given, one zero-filled
    table.  Bad arguments: ValueError naming the argument, before anything is launched."""
    what = "seg_rle_encode"
    B, H, W = _region_maps(what, labels, 4, (torch.uint8, torch.int16))
    R = _rle_max_runs(what, max_runs)
    dev, lead = labels.device, tuple(labels.shape[:-2])
    if runs is not None:
        _rle_runs(what, runs, lead + (R, 2), dev)
        if _overlap(runs, labels):
            raise ValueError("%s: runs overlaps labels" % what)
    count = _region_table_out(what, "count", count, lead, torch.int32, dev, (("labels", labels), ("runs", runs)))
    if runs is None:
        runs = torch.zeros(lead + (R, 2), dtype=torch.int32, device=dev)
    if count is None:
        count = torch.empty(lead, dtype=torch.int32, device=dev)
    seg = torch.empty(B * W * -(-H // SEG_RLE_CHUNK), dtype=torch.int32, device=dev)
    _check(lib().ifseg_seg_rle_encode(_ptr(labels), c_int(labels.element_size()), c_int(B), c_int(H), c_int(W), c_int(R),
                                      _ptr(seg), _ptr(runs), _ptr(count), _stream()), what)
    return runs, count


def seg_rle_decode(runs, count, H, W, dtype=torch.uint8, fill=255, out=None, flag=None):
    """runs int32 [R, 2] or [B, R, 2], count int32 of the leading shape -> (out `dtype` [H, W] or [B, H, W], flag): the label
    map of a run table in one launch (csrc/rle.hip; `predict.rle_decode_reference` is the specification).  With
    m = min(count, R): out[y, x] = value[s], s the largest index below m with start[s] <= x H + y; with m <= 0 the image is
    `fill`.  flag: an int32 word that gets bit 0 where count > R (a truncated table: the tail carries the last written run's
    value) and bit 1 where m <= 0 or start[0] != 0; given: never cleared here, else a fresh zeroed one.  No index into the table
    leaves [0, m), whatever it holds.  `seg_rle_decode(*seg_rle_encode(x), H, W, x.dtype)[0]` is x wherever count <= R.  out:
    written in place when given.  Bad arguments: ValueError naming the argument, before anything is launched."""
    what = "seg_rle_decode"
    if not torch.is_tensor(runs) or runs.dim() not in (2, 3):
        raise ValueError("%s: runs must be an int32 tensor [R, 2] or [B, R, 2], got %s" % (
            what, tuple(runs.shape) if torch.is_tensor(runs) else type(runs)))
    dev, lead = runs.device, tuple(runs.shape[:-2])
    R = int(runs.shape[-2])
    if not 1 <= R <= SEG_RLE_MAX_RUNS:
        raise ValueError("%s: runs must hold 1 .. %d runs, got %d" % (what, SEG_RLE_MAX_RUNS, R))
    _rle_runs(what, runs, lead + (R, 2), dev)
    for name, v in (("H", H), ("W", W)):
        if not isinstance(v, int) or isinstance(v, bool) or v < 1:
            raise ValueError("%s: %s must be a positive int, got %r" % (what, name, v))
    B = runs.shape[0] if lead else 1
    if B < 1 or B * H * W >= 2 ** 31:
        raise ValueError("%s: H and W must give 1 .. 2**31 - 1 pixels in all, got B, H, W = %d, %d, %d" % (what, B, H, W))
    if dtype not in (torch.uint8, torch.int16):
        raise ValueError("%s: dtype must be torch.uint8 or torch.int16, got %r" % (what, dtype))
    lo, hi = (0, 255) if dtype == torch.uint8 else (-2 ** 15, 2 ** 15 - 1)
    if not isinstance(fill, int) or isinstance(fill, bool) or not lo <= fill <= hi:
        raise ValueError("%s: fill must be an int in %d .. %d, got %r" % (what, lo, hi, fill))
    given = [("runs", runs)]
    count = _region_table_out(what, "count", count, lead, torch.int32, dev, given)
    if count is None:
        raise ValueError("%s: count must be an int32 tensor of shape %s, got None" % (what, lead))
    given.append(("count", count))
    out = _region_table_out(what, "out", out, lead + (H, W), dtype, dev, given)
    if flag is not None:
        _region_flag(what, flag, dev)
        for name, t in given + [("out", out)]:
            if t is not None and _overlap(t, flag):
                raise ValueError("%s: %s overlaps flag" % (what, name))
    flag = _region_flag(what, flag, dev)
    if out is None:
        out = torch.empty(lead + (H, W), dtype=dtype, device=dev)
    _check(lib().ifseg_seg_rle_decode(_ptr(runs), _ptr(count), c_int(B), c_int(H), c_int(W), c_int(R), c_int(out.element_size()),
                                      c_int(fill), _ptr(out), _ptr(flag), _stream()), what)
    return out, flag


# --------------------------------------------------------------------------- pixel-adaptive mask refinement (csrc/pamr.hip)
SEG_PAMR_MAX_DILATIONS = 8          # == PM_MAX_D: the dilations of a call at most (8 neighbours each)
SEG_PAMR_MAX_DILATION = 32          # == PM_MAX_DILATION: the largest dilation (a tile's halo: 40 KiB of LDS)
SEG_PAMR_DILATIONS = (1, 2, 4, 8, 12, 24)       # the published defaults, with ten iterations


def seg_pamr_limits():
    """-> (dilations at most, the largest dilation, the largest n) as the loaded library states them (`ifseg_pamr_limit`):
    SEG_PAMR_MAX_DILATIONS, SEG_PAMR_MAX_DILATION and SEG_PREDICT_MAX_CLASSES, which the tests hold against it"""
    return _limits("ifseg_pamr_limit", 3)


def _pamr_dilations(dilations):
    """the dilations of a call, checked -> (a ctypes int array, D)"""
    d = tuple(dilations)
    assert 1 <= len(d) <= SEG_PAMR_MAX_DILATIONS and all(isinstance(v, int) and 1 <= v <= SEG_PAMR_MAX_DILATION for v in d), dilations
    return (c_int * len(d))(*d), len(d)


def pamr_affinity(image, dilations=SEG_PAMR_DILATIONS):
    """image uint8 [H, W, 3] (HWC, contiguous, at any byte offset of its storage), dilations: 1 .. 8 ints in 1 .. 32 -> w fp32
    [8 D, H, W] in one launch (csrc/pamr.hip): per pixel the softmax over its 8 D neighbours (every dilation's 3 x 3 ring,
    coordinates clamped to the image) of minus the mean over the channels of |difference| / (1e-8 + 0.1 local deviation).
    `predict.pamr_affinity_reference` is the specification and states the rule."""
    assert image.dtype == torch.uint8 and image.dim() == 3 and image.shape[2] == 3 and image.is_contiguous(), \
        (image.dtype, tuple(image.shape), image.stride())
    arr, D = _pamr_dilations(dilations)
    H, W = int(image.shape[0]), int(image.shape[1])
    assert H >= 1 and W >= 1 and 8 * D * H * W < 2 ** 31, (D, H, W)
    w = torch.empty(8 * D, H, W, dtype=torch.float32, device=image.device)
    _check(lib().ifseg_pamr_affinity(_ptr(image), c_int(H), c_int(W), arr, c_int(D), _ptr(w), _stream()), "pamr_affinity")
    return w


def pamr_iterate(w, src, dst, dilations=SEG_PAMR_DILATIONS, labels=None, conf=None):
    """One iteration in one launch (csrc/pamr.hip): w fp32 [8 D, H, W] (`pamr_affinity` of the same dilations), src fp32
    [n, H, W] -> dst fp32 [n, H, W], dst[c, p] = sum_k w[k, p] src[c, neighbour k of p]; dst must not overlap src or w.
    labels (uint8 for n <= 256, or int16) and conf (fp32) [H, W] given: also written, per pixel the first maximum of dst over
    the classes and its value -- the caller asks on its last iteration, there is no argmax pass.  Every tensor contiguous.
    `predict.pamr_iterate_reference` is the specification.  -> dst"""
    arr, D = _pamr_dilations(dilations)
    assert w.dtype == torch.float32 and w.dim() == 3 and w.shape[0] == 8 * D and w.is_contiguous(), \
        (w.dtype, tuple(w.shape), w.stride(), D)
    H, W = int(w.shape[1]), int(w.shape[2])
    for name, t in (("src", src), ("dst", dst)):
        assert t.dtype == torch.float32 and t.dim() == 3 and tuple(t.shape[1:]) == (H, W) and t.is_contiguous() \
            and t.device == w.device, (name, t.dtype, tuple(t.shape), t.stride(), t.device, (H, W))
    n = int(src.shape[0])
    assert dst.shape == src.shape and 1 <= n <= SEG_PREDICT_MAX_CLASSES and H >= 1 and W >= 1 and n * H * W < 2 ** 31 \
        and 8 * D * H * W < 2 ** 31, (tuple(src.shape), tuple(dst.shape))
    assert not _overlap(dst, src) and not _overlap(dst, w), "pamr_iterate: dst overlaps src or w"
    if labels is not None:
        assert labels.dtype in (torch.uint8, torch.int16) and (n <= 256 or labels.dtype == torch.int16) \
            and tuple(labels.shape) == (H, W) and labels.is_contiguous() and labels.device == w.device, \
            (labels.dtype, tuple(labels.shape), labels.stride(), labels.device, n)
    if conf is not None:
        assert conf.dtype == torch.float32 and tuple(conf.shape) == (H, W) and conf.is_contiguous() and conf.device == w.device, \
            (conf.dtype, tuple(conf.shape), conf.stride(), conf.device)
    _check(lib().ifseg_pamr_iterate(_ptr(w), _ptr(src), _ptr(dst), c_int(n), c_int(H), c_int(W), arr, c_int(D), _ptr(labels),
                                    c_int(labels.element_size() if labels is not None else 0), _ptr(conf), _stream()),
           "pamr_iterate")
    return dst


def seg_pamr(probs, image, iters=10, dilations=SEG_PAMR_DILATIONS, conf=False, probs_out=False, label_dtype=None):
    """Pixel-adaptive mask refinement (PAMR, Araslanov & Roth, CVPR 2020) of ONE image: probs fp32 [n, H, W] (what
    `seg_predict(probs=True)` hands over, one image of it), image uint8 [H, W, 3], the photograph at the same resolution ->
    (labels [H, W], uint8 for n <= 256 else int16 (or `label_dtype`); conf fp32 [H, W] or None; the refined values fp32
    [n, H, W] or None).  One `pamr_affinity` launch, `iters` >= 1 `pamr_iterate` launches over two ping-pong buffers, the last
    of which also writes the labels and conf; `probs` is not modified and nothing synchronises with the host.
    `predict.pamr_reference` is the specification.  Every value is a convex combination of `probs`' values: probabilities
    stay probabilities."""
    assert probs.dtype == torch.float32 and probs.dim() == 3 and probs.is_contiguous(), (probs.dtype, tuple(probs.shape), probs.stride())
    n, H, W = (int(v) for v in probs.shape)
    assert image.dim() == 3 and tuple(image.shape) == (H, W, 3) and image.device == probs.device, \
        (tuple(image.shape), image.device, (H, W), probs.device)
    assert isinstance(iters, int) and iters >= 1, iters
    w = pamr_affinity(image, dilations)
    labels, cf, _ = _predict_outputs(1, n, H, W, probs.device, conf, False, label_dtype)
    bufs = [torch.empty_like(probs), torch.empty_like(probs) if iters > 1 else None]
    src = probs
    for it in range(iters):
        last = it == iters - 1
        dst = bufs[it & 1]
        pamr_iterate(w, src, dst, dilations, labels[0] if last else None, cf[0] if last and conf else None)
        src = dst
    return labels[0], cf[0] if conf else None, src if probs_out else None


_image_luts = {}        # (mean, std, device) -> fp32 [3, 256] on the device; at most 16 entries


# ------------------- the front of the device-side input path (imgload.hip, trainload.hip, mix.hip, strong.hip): each rule once
def _hptr(t):                       # the address of a host tensor, or None
    return None if t is None else c_void_p(t.data_ptr())


def _seed64(seed):
    return ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF)


def _ordinals(first_ordinal, B):                    # -> the first of B ordinals as an int: the stream's ordinal has 32 bits
    first = int(first_ordinal)
    assert B >= 1 and 0 <= first and first + B <= 2 ** 32, (first, B)
    return first


def _out(out, shape, dtype, dev, align=1, like=None):
    """the tensor a wrapper writes into: allocated here (as `like`, a contiguous tensor of that shape, dtype and device,
    where the caller has one: the cheaper call; else with the sizes unpacked, cheaper than a tuple), or the caller's, checked"""
    if out is None:
        return torch.empty_like(like) if like is not None else torch.empty(*shape, dtype=dtype, device=dev)
    assert out.dtype == dtype and tuple(out.shape) == tuple(shape) and out.is_contiguous() and out.device == dev \
        and (align == 1 or out.data_ptr() % align == 0), (out.dtype, tuple(out.shape), out.stride(), out.device, align)
    return out


def _records(records, B, dev):
    assert records.is_cuda and records.device == dev and records.dtype == torch.int32 and tuple(records.shape) == (B, 16) \
        and records.is_contiguous(), (records.device, records.dtype, tuple(records.shape), records.stride())
    return records


def _records_in(params, B, dev):
    """records on the host or on the device -> (the device tensor, the host tensor the entry point checks first, or None)"""
    host = None
    if not params.is_cuda:
        host = params.contiguous()
        params = host.to(dev)
    return _records(params.contiguous(), B, dev), host


def _u8_batch(images_u8, dtype):
    """uint8 [B, H0, W0, 3] (HWC, contiguous) and the output dtype of a loader -> (B, H0, W0)"""
    assert images_u8.dtype == torch.uint8 and images_u8.dim() == 4 and images_u8.shape[-1] == 3 and images_u8.is_contiguous(), \
        (images_u8.dtype, tuple(images_u8.shape), images_u8.stride())
    B, H0, W0, _ = images_u8.shape
    assert B >= 1 and H0 >= 1 and W0 >= 1, tuple(images_u8.shape)
    assert dtype in (torch.float32, torch.bfloat16), dtype
    return B, H0, W0


def image_load(images_u8, oh, ow, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5), reverse_channels=False, dtype=torch.float32,
               staging_bytes=None, out=None):
    """uint8 [B, H0, W0, 3] (HWC, contiguous, on the device) -> patch_images [B, 3, oh, ow] in `dtype` (fp32 or bf16): the
    reference's evaluation transform in one kernel (csrc/imgload.hip) -- bilinear resize (align_corners=False, no antialiasing,
    integer source coordinates), rounding to a grey level, optional channel reversal (off by default: the reference's two
    reversals, segmentation_dataset.py:218 and :256, cancel, so the network sees RGB) and
    (x / 255 - mean) / std from a [3, 256] table built on the host.  `imageio.image_load_reference` is the specification.
    staging_bytes: size of the kernel's LDS staging buffer for this call (0: every tile reads global memory), None: the default;
    out: a contiguous [B, 3, oh, ow] tensor of `dtype` to write into."""
    B, H0, W0 = _u8_batch(images_u8, dtype)
    oh, ow = int(oh), int(ow)
    assert oh >= 1 and ow >= 1, (tuple(images_u8.shape), oh, ow)
    assert images_u8.is_cuda, "device tensor required"
    dev = images_u8.device
    lut = _image_lut(mean, std, dev)
    out = _out(out, (B, 3, oh, ow), dtype, dev)
    with _staging(lib().ifseg_image_load_staging, staging_bytes):
        _check(lib().ifseg_image_load(_ptr(images_u8), c_int(B), c_int(H0), c_int(W0), c_int(oh), c_int(ow), _ptr(lut),
                                      c_int(1 if reverse_channels else 0), _ptr(out), c_int(out.element_size()), _stream()),
               "image_load")
    return out


def image_load_windows(images_u8, oh, ow, crop, stride, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5), reverse_channels=False,
                       dtype=torch.float32, staging_bytes=None, flip=False):
    """uint8 [B, H0, W0, 3] -> the window batch [B Nw, 3, ch, cw] in `dtype` of sliding-window inference, written directly
    (csrc/imgload.hip): element (b Nw + k, c, y, x) is `image_load(..., oh, ow)`'s element (b, c, ys[k] + y, xs[k] + x), bit for
    bit, for the windows of `imageio.slide_windows(oh, ow, crop, stride)`; no [B, 3, oh, ow] image is written.
    `imageio.image_load_windows_reference` is the specification.  crop, stride: an int or an (h, w) pair each; the other
    arguments as in `image_load`.  flip: the windows of the MIRRORED resized image, bit for bit the `slide_windows` slices of
    `image_load(...).flip(-1)` (mirrored after the resize, as mmseg does; not the unmirrored windows flipped: the last window
    of an axis is pulled back inside, so the starts are not symmetric)."""
    B, H0, W0 = _u8_batch(images_u8, dtype)
    oh, ow, crop, stride, nw, ch, cw = _slide_geometry(oh, ow, crop, stride)
    assert images_u8.is_cuda, "device tensor required"
    dev = images_u8.device
    lut = _image_lut(mean, std, dev)
    out = torch.empty(B * nw, 3, ch, cw, dtype=dtype, device=dev)
    with _staging(lib().ifseg_image_load_staging, staging_bytes):
        entry = lib().ifseg_image_load_windows_mirrored if flip else lib().ifseg_image_load_windows
        _check(entry(_ptr(images_u8), c_int(B), c_int(H0), c_int(W0), c_int(oh), c_int(ow), c_int(crop[0]), c_int(crop[1]),
                     c_int(stride[0]), c_int(stride[1]), _ptr(lut), c_int(1 if reverse_channels else 0), _ptr(out),
                     c_int(out.element_size()), _stream()), "image_load_windows")
    return out


def _image_lut(mean, std, dev):
    from .imageio import normalisation_table
    key = (tuple(float(x) for x in mean), tuple(float(x) for x in std), dev)
    lut = _image_luts.get(key)
    if lut is None:
        # the first call per (mean, std, device) copies the table from the host: it blocks the host and cannot be captured
        if len(_image_luts) >= 16:
            _image_luts.clear()
        lut = _image_luts[key] = normalisation_table(mean, std).to(dev)
    return lut


def _train_table(images, labels):
    """the descriptor table of a batch (include/ifseg_hip.h ifseg_train_src: image pointer, label pointer, H0 | W0 << 32) ->
    (pinned host int64 [B, 3], its device copy): one small H2D copy on the current stream.  The sources are recorded on that
    stream, so their memory is not handed out again before the kernels have read it."""
    dev = labels[0].device
    rows = []
    stream = torch.cuda.current_stream(dev)
    for i, lab in enumerate(labels):
        assert lab.is_cuda and lab.device == dev and lab.dtype == torch.uint8 and lab.dim() == 2 and lab.is_contiguous(), \
            (lab.device, lab.dtype, tuple(lab.shape))
        H0, W0 = lab.shape
        assert 1 <= H0 < 2 ** 31 and 1 <= W0 < 2 ** 31, (H0, W0)
        img_ptr = 0
        if images is not None:
            img = images[i]
            assert img.is_cuda and img.device == dev and img.dtype == torch.uint8 and tuple(img.shape) == (H0, W0, 3) \
                and img.is_contiguous(), (img.device, img.dtype, tuple(img.shape), (H0, W0))
            img_ptr = img.data_ptr()
            img.record_stream(stream)
        lab.record_stream(stream)
        rows.append((img_ptr, lab.data_ptr(), H0 | (W0 << 32)))
    host = torch.tensor(rows, dtype=torch.int64).pin_memory()
    return host, host.to(dev, non_blocking=True)


def train_draw(labels, P, nseg, seed, first_ordinal, ratio_range=(0.5, 2.0), photometric=True, flip=True, raw_labels=True,
               out=None, table=None):
    """records int32 [B, 16] of the training transform for the samples at ordinals first_ordinal + b (csrc/trainload.hip;
    `augment.draw_params` is the specification).  labels: uint8 [H0, W0] device tensors of any sizes.  table: the batch's
    `_train_table(images, labels)` when the caller shares one between this call and `train_load`."""
    from .augment import ratio_halves
    lo2, span2 = ratio_halves(ratio_range)
    B = len(labels)
    assert B >= 1
    host, table = table if table is not None else _train_table(None, labels)
    out = _out(out, (B, 16), torch.int32, labels[0].device)
    _check(lib().ifseg_train_draw(_hptr(host), _ptr(table), c_int(B), c_int(P), c_int(nseg),
                                  c_int(1 if raw_labels else 0), _seed64(seed), c_ll(int(first_ordinal)), c_int(lo2), c_int(span2),
                                  c_int((1 if flip else 0) | (2 if photometric else 0)), _ptr(out), _stream()), "train_draw")
    return out


def train_load(images, labels, params, P, nseg, seg_id_offset, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5), reverse_channels=False,
               raw_labels=True, dtype=torch.float32, eos=2, staging_bytes=None, out=None, target=None, table=None):
    """the training transform under the given records, one launch (csrc/trainload.hip; `augment.train_load_reference` is the
    specification): uint8 images [H0, W0, 3] and label maps [H0, W0] of any sizes on the device ->
    (patch_images [B, 3, P, P] in `dtype`, target int64 [B, P*P + 1]).  params: int32 [B, 16]; records on the host are checked
    by the entry point before they are copied, records on the device are checked by the kernel (a bad one poisons its
    sample).  staging_bytes: the LDS staging buffer of this call (0: every tile reads global memory), None: the default."""
    B = len(images)
    assert B >= 1 and len(labels) == B and dtype in (torch.float32, torch.bfloat16), (B, len(labels), dtype)
    dev = labels[0].device
    params, params_host = _records_in(params, B, dev)
    lut = _image_lut(mean, std, dev)
    host, table = table if table is not None else _train_table(images, labels)
    out = _out(out, (B, 3, P, P), dtype, dev)
    target = _out(target, (B, P * P + 1), torch.int64, dev)
    with _staging(lib().ifseg_train_load_staging, staging_bytes):
        _check(lib().ifseg_train_load(_hptr(host), _ptr(table), _ptr(params), _hptr(params_host), c_int(B), c_int(P),
                                      c_int(nseg), c_int(1 if raw_labels else 0), c_ll(seg_id_offset), c_ll(eos), _ptr(lut),
                                      c_int(1 if reverse_channels else 0), _ptr(out), c_int(out.element_size()), _ptr(target),
                                      _stream()), "train_load")
    return out, target


def train_load_plane(planes, params, P, out=None, table=None):
    """uint8 planes [H0, W0] of any sizes on the device, under the records of `train_draw` / the caller -> uint8 [B, P*P]: the
    label tap of `train_load` on the plane's own bytes, one launch (csrc/trainload.hip; `augment.train_plane_reference` is the
    specification).  The planes travel in a descriptor table through its label pointers: table = `_train_table(None, planes)`
    when the caller already has it.  Records on the host are checked by the entry point, records on the device by the
    kernel (a bad one writes 0 for its sample).  Any 1 <= P <= 4096."""
    B = len(planes)
    assert B >= 1
    dev = planes[0].device
    params, params_host = _records_in(params, B, dev)
    host, table = table if table is not None else _train_table(None, planes)
    assert host.shape[0] == B, (tuple(host.shape), B)
    P = int(P)
    out = _out(out, (B, P * P), torch.uint8, dev)
    _check(lib().ifseg_train_load_plane(_hptr(host), _ptr(table), _ptr(params), _hptr(params_host), c_int(B), c_int(P),
                                        _ptr(out), _stream()), "train_load_plane")
    return out


# --------------------------------------------------------------------------- ClassMix / CutMix of two batches
MIX_MASKS = {"class": 0, "box": 1}
MIX_MAX_P = 4096             # == MX_MAX_P (csrc/mix.hip)


def _mix_target(t, what):
    """int64 [B, P*P + 1] on the device, contiguous -> (B, P)"""
    assert t.is_cuda and t.dtype == torch.int64 and t.dim() == 2 and t.is_contiguous() and t.data_ptr() % 8 == 0, \
        (what, t.device, t.dtype, tuple(t.shape), t.stride())
    B, P = t.shape[0], int(round((t.shape[1] - 1) ** 0.5))
    assert B >= 1 and P * P + 1 == t.shape[1] and P >= 16 and P % 16 == 0 and P <= MIX_MAX_P, (what, tuple(t.shape))
    return B, P


def mix_draw(src_target, nseg, seg_id_offset, seed, first_ordinal, mask="class", out=None):
    """records int32 [B, 16] of the batch mix for the samples at ordinals first_ordinal + b, one launch (csrc/mix.hip;
    `augment.mix_draw_reference` is the specification and states the rule).  src_target: int64 [B, P*P + 1], the labelled
    batch's targets; mask "class" (ClassMix: half of the classes present in each sample) or "box" (CutMix: a rectangle)."""
    B, P = _mix_target(src_target, "mix_draw")
    assert isinstance(nseg, int) and 1 <= nseg <= 255, nseg
    assert mask in MIX_MASKS, mask
    first = _ordinals(first_ordinal, B)
    assert out is None or not _overlap(out, src_target), (out.data_ptr(), src_target.data_ptr())
    out = _out(out, (B, 16), torch.int32, src_target.device)
    _check(lib().ifseg_mix_draw(_ptr(src_target), c_int(B), c_int(P), c_int(nseg), c_ll(int(seg_id_offset)), _seed64(seed),
                                c_ll(first), c_int(MIX_MASKS[mask]), _ptr(out), _stream()), "mix_draw")
    return out


def mix_apply(records, src_images, src_target, dst_images, dst_target, nseg, seg_id_offset, src_weight=None, dst_weight=None,
              out=None):
    """the batch mix under the given records, one launch (csrc/mix.hip; `augment.mix_apply_reference` is the specification):
    the pixels a record selects -- a chosen class of the SOURCE pixel, or the record's box -- take the source's image values,
    target and weight, the others keep the destination's -> (images [B, 3, P, P], target int64 [B, P*P + 1], weight uint8
    [B, P*P] or None).  Images fp32 or bf16, the same in both batches; weights uint8 [B, P*P] or None, a missing plane reads
    as 255 and no plane comes out if both are missing.  Everything contiguous.  out: (images, target, weight | None) to
    write into; each may be the destination's own tensor (in place), and must not overlap anything else."""
    B, P = _mix_target(src_target, "mix_apply")
    dev, n = src_target.device, P * P
    assert _mix_target(dst_target, "mix_apply") == (B, P) and dst_target.device == dev, (tuple(src_target.shape), tuple(dst_target.shape))
    assert isinstance(nseg, int) and 1 <= nseg <= 255, nseg
    _records(records, B, dev)
    assert src_images.dtype in (torch.float32, torch.bfloat16) and src_images.dtype == dst_images.dtype, (src_images.dtype, dst_images.dtype)
    assert B * 3 * n < 2 ** 31, (B, P)
    for t in (src_images, dst_images):
        assert t.device == dev and tuple(t.shape) == (B, 3, P, P) and t.is_contiguous() and t.data_ptr() % 16 == 0, \
            (t.device, tuple(t.shape), t.stride())
    for t in (src_weight, dst_weight):
        assert t is None or (t.device == dev and t.dtype == torch.uint8 and tuple(t.shape) == (B, n) and t.is_contiguous()
                             and t.data_ptr() % 8 == 0), (t.device, t.dtype, tuple(t.shape), t.stride())
    weighted = src_weight is not None or dst_weight is not None
    oi, ot, ow = out if out is not None else (None, None, None)
    assert out is None or (ow is not None) == weighted, "mix_apply: a weight plane comes out exactly when one goes in"
    oi = _out(oi, dst_images.shape, dst_images.dtype, dev, 16, dst_images)
    ot = _out(ot, dst_target.shape, torch.int64, dev, 8, dst_target)
    ow = _out(ow, (B, n), torch.uint8, dev, 8) if weighted else None
    outs, dsts = (oi, ot, ow), (dst_images, dst_target, dst_weight)
    for i, o in enumerate(outs):
        if o is None:
            continue
        for t in (records, src_images, src_target, src_weight) + outs[i + 1:]:
            assert t is None or not _overlap(o, t), "mix_apply: out overlaps the source, the records or another output"
        for j, t in enumerate(dsts):
            assert t is None or not _overlap(o, t) or (i == j and o.data_ptr() == t.data_ptr()), \
                "mix_apply: out may be the destination tensor it replaces, and overlaps the destination in no other way"
    _check(lib().ifseg_mix_apply(_ptr(records), _ptr(src_images), _ptr(src_target), _ptr(src_weight), _ptr(dst_images),
                                 _ptr(dst_target), _ptr(dst_weight), c_int(B), c_int(P), c_int(nseg), c_ll(int(seg_id_offset)),
                                 c_int(src_images.element_size()), _ptr(oi), _ptr(ot), _ptr(ow), _stream()), "mix_apply")
    return oi, ot, ow


# --------------------------------------------------------------------------- strong augmentation of a mixed batch
STRONG_MAX_P = 4096          # == SG_MAX_P (csrc/strong.hip)


def strong_blur_table():
    """the library's copy of `augment.BLUR_WEIGHTS`, int32 [64, 5] on the host; touches no device"""
    buf = (c_int * 320)()
    _check(lib().ifseg_strong_blur_table(buf), "strong_blur_table")
    return torch.tensor(list(buf), dtype=torch.int32).reshape(64, 5)


def strong_draw(B, seed, first_ordinal, jitter_p8=205, blur_p8=128, device=None, out=None):
    """records int32 [B, 16] of the strong augmentation for the samples at ordinals first_ordinal + b, one launch
    (csrc/strong.hip; `augment.strong_draw_reference` is the specification and states the rule).  jitter_p8 / blur_p8: the
    two gates in 256ths, 0 never fires and 256 always does."""
    B = int(B)
    first = _ordinals(first_ordinal, B)
    assert isinstance(jitter_p8, int) and isinstance(blur_p8, int) and 0 <= jitter_p8 <= 256 and 0 <= blur_p8 <= 256, (jitter_p8, blur_p8)
    here = out.device if out is not None else torch.device("cuda", torch.cuda.current_device())
    out = _out(out, (B, 16), torch.int32, here if device is None else torch.device(device))
    with torch.cuda.device(out.device):
        _check(lib().ifseg_strong_draw(c_int(B), _seed64(seed), c_ll(first), c_int(jitter_p8), c_int(blur_p8), _ptr(out),
                                       _stream()), "strong_draw")
    return out


def strong_apply(records, images, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5), reverse_channels=False, out=None, lut=None):
    """colour jitter and Gaussian blur of images [B, 3, P, P] (fp32 or bf16, the values of a normalised batch) under the
    given records, one launch (csrc/strong.hip; `augment.strong_apply_reference` is the specification): grey levels back
    from the values, the photometric chain, the 9-tap blur, the table -> images of the same shape and dtype.  An invalid
    record gives NaN for its sample.  out: a tensor to write into, sharing no byte with the images (the blur reads
    neighbours).  lut: the fp32 [3, 256] table on the device when the caller holds one, else cached per (mean, std, device)."""
    assert images.is_cuda and images.dtype in (torch.float32, torch.bfloat16) and images.dim() == 4 and images.shape[1] == 3 \
        and images.shape[2] == images.shape[3] and images.is_contiguous() and images.data_ptr() % 16 == 0, \
        (images.device, images.dtype, tuple(images.shape), images.stride())
    B, P, dev = images.shape[0], images.shape[2], images.device
    assert B >= 1 and P >= 16 and P % 16 == 0 and P <= STRONG_MAX_P and B * 3 * P * P < 2 ** 31, (B, P)
    _records(records, B, dev)
    assert len(tuple(std)) == 3 and all(float(s) > 0 for s in std), "strong_apply: std must be > 0 (the table must increase): %r" % (std,)
    if lut is None:
        lut = _image_lut(mean, std, dev)
    assert lut.device == dev and lut.dtype == torch.float32 and tuple(lut.shape) == (3, 256) and lut.is_contiguous(), \
        (lut.device, lut.dtype, tuple(lut.shape))
    for t in (images, records, lut):
        assert out is None or not _overlap(out, t), "strong_apply: out shares memory with the images, the records or the table (no in-place form)"
    out = _out(out, images.shape, images.dtype, dev, 16, images)
    _check(lib().ifseg_strong_apply(_ptr(records), _ptr(images), c_int(B), c_int(P), c_int(images.element_size()), _ptr(lut),
                                    c_int(1 if reverse_channels else 0), _ptr(out), _stream()), "strong_apply")
    return out


def dropout(x, resid, out, p, seed, drop_path_scale=None, rows_per_batch=None):
    """x / resid / out: [rows, C] or [B, rpb, C] bf16 views (last dim contiguous)"""
    C = x.shape[-1]
    rows = x.numel() // C
    rpb = x.shape[1] if x.dim() == 3 else 0
    xb, xl = _map(x, rpb)
    rb, rl = _map(resid, rpb)
    ob, ol = _map(out, rpb)
    rc = lib().ifseg_dropout(_ptr(x), _ptr(resid), _ptr(out), c_ll(rows), c_int(C), c_float(p),
                             ctypes.c_ulonglong(seed & 0xFFFFFFFFFFFFFFFF), _ptr(drop_path_scale),
                             c_int(rows_per_batch or (rpb if rpb else rows)), c_int(rpb), c_ll(xb), c_int(xl), c_ll(rb),
                             c_int(rl), c_ll(ob), c_int(ol), c_void_p(_seed_add_ptr()), _stream())
    _check(rc, "dropout")
    return out


def dropout_fill(x, out, p, seed, fill=-30.0):
    """out = keep ? x : fill (contiguous bf16, no rescaling; the activation dropout on the FFN pre-activation, see rowops.hip)"""
    assert x.is_contiguous() and out.is_contiguous() and x.dtype == torch.bfloat16 and out.shape == x.shape
    _check(lib().ifseg_dropout_fill(_ptr(x), _ptr(out), c_ll(x.numel()), c_float(p), ctypes.c_ulonglong(seed & 0xFFFFFFFFFFFFFFFF),
                                    c_void_p(_seed_add_ptr()), c_float(fill), _stream()), "dropout_fill")
    return out


# ---------------------------------------------------------------------- dense CRF (crf.py:19-37)
def crf_bilateral(feat4, gx, gy, qn, out, H, W):
    """out fp32 [Cp, N] = exact bilateral filter of qn bf16 [Cp, ldq]"""
    _check(lib().ifseg_crf_bilateral(_ptr(feat4), _ptr(gx), _ptr(gy), _ptr(qn), c_int(qn.stride(0)), _ptr(out),
                                     c_int(qn.shape[0]), c_int(H), c_int(W), _stream()), "crf_bilateral")


def crf_spatial(qn, g, R, out, H, W):
    _check(lib().ifseg_crf_spatial(_ptr(qn), _ptr(g), c_int(R), _ptr(out), c_int(qn.shape[0]), c_int(H), c_int(W), _stream()), "crf_spatial")


def crf_update(prob, mpos, mbi, npos, nbi, wpos, wbi, Q, qpos, qbi):
    C, N = prob.shape
    _check(lib().ifseg_crf_update(_ptr(prob), _ptr(mpos), _ptr(mbi), _ptr(npos), _ptr(nbi), c_float(wpos), c_float(wbi),
                                  _ptr(Q), _ptr(qpos), _ptr(qbi), c_int(qbi.stride(0) if qbi is not None else 0), c_int(C),
                                  c_int(N), _stream()), "crf_update")


def crf_norm(k1, n):
    _check(lib().ifseg_crf_norm(_ptr(k1), _ptr(n), c_int(n.numel()), _stream()), "crf_norm")
