"""torch.library registration of the hot-path kernels: `torch.ops.ifseg.*`.

BASELINE.json north_star asks for "Python host code calling hand-written HIP kernels for CDNA4 through PyTorch-ROCm custom
ops"; SURVEY 8b names torch.library.  The engine (models/segofa/engine.py) keeps calling the C ABI directly through
`ifseg_amd.hip` -- one ctypes call per launch, no dispatcher hop on a ~570-launch step -- and this module puts the same
kernels IN FRONT OF the dispatcher as functional ops with autograd and fake (meta) implementations, for callers that
compose them with other PyTorch code (`torch.compile`, `torch.autograd.gradcheck`-style tests, export).

  op                        csrc/              backward op             mirrors
  linear                    gemm.hip           linear_bwd              F.linear, unify_multihead_attention.py:327-346,513
  layer_norm                rowops.hip         layer_norm_bwd          LayerNorm (+ GELU in front), unify_transformer_layer.py:256-292
  bias_attention            attention.hip      bias_attention_bwd      unify_multihead_attention.py:459-512, encoder_module.py:757-809
  attention_bias            attention_bi.hip   attention_bias_bwd      unify_multihead_attention.py:459-512 (:130,464-465: the bias a tensor)
  bias_attention_bi         attention_bi.hip   bias_attention_bi_bwd   bias_attention + key counts + attention dropout
  seg_loss                  loss.hip           seg_loss_bwd            seg_criterion.py:237-244,269-347
  seg_loss_weighted         loss.hip           seg_loss_bwd            seg_loss with a weight per pixel and per class
  seg_dice                  dice.hip           seg_loss_bwd            per-sample soft Dice of the same upsampled logits
  seg_distill               distill.hip        seg_loss_bwd            per-pixel KL to a teacher (no gradient to the teacher)
  seg_ohem                  ohem.hip           -                       mmseg's OHEMPixelSampler: seg_loss_weighted's weight plane
  seg_predict               predict.hip        -                       label maps at image resolution
  seg_predict_views         predict.hip        -                       the mean of K views: multi-scale + flip inference
  seg_areas                 predict.hip        -                       label maps counted against ground truth: mIoU
  seg_confusion             predict.hip        -                       the class confusion matrix [n, n + 1]
  seg_boundary_areas        boundary.hip       -                       Boundary IoU's band areas and the two bands
  seg_score_views           predict.hip        -                       seg_areas in seg_predict_views' epilogue
  seg_render                render.hip         -                       the label map coloured over its image, with contours
  seg_conf_hist             pseudo.hip         -                       the per-class confidence histogram of a label map
  seg_pseudo                pseudo.hip         -                       pseudo-labels by thresholds and an ignore band
  seg_regions               regions.hip        -                       the connected regions of a label map
  seg_region_drop           regions.hip        -                       the map without its regions below a pixel count
  seg_calibration           calib.hip          -                       how often a confidence is right, per class and bin
  seg_temperature_sweep     tsweep.hip         -                       K temperatures of one forward: reliability, NLL, Brier
  seg_pamr                  pamr.hip           -                       pixel-adaptive mask refinement of one image
  image_load                imgload.hip        -                       the reference's evaluation transform
  image_load_windows        imgload.hip        -                       the window batch of sliding-window inference
  seg_predict_windows       predict.hip        -                       the windows' scores merged into one label map
  seg_score_windows         predict.hip        -                       seg_areas in seg_predict_windows' epilogue
  seg_predict_slide_views   predict.hip        -                       K views, each a set of windows (softmax per view: mmseg)
  seg_score_slide_views     predict.hip        -                       seg_areas in seg_predict_slide_views' epilogue
  train_load                trainload.hip      -                       the reference's training transform under given records
  mix_draw                  mix.hip            -                       ClassMix / CutMix: the choice of classes or of a box
  mix_apply                 mix.hip            -                       the paste of images, targets and weight planes (copies bits)
  strong_draw               strong.hip         -                       the records of colour jitter and Gaussian blur
  strong_apply              strong.hip         -                       a mixed batch's images under them (integer in between)

The backward ops are dispatcher-visible ops themselves; `ifseg_amd.modules.MultiheadAttention` composes `linear` and
`attention_bias` under the reference module's parameter names.  No CPU implementation is registered: on a CPU tensor the
dispatcher raises.

Every op has ONE check helper that its real and its fake implementation call first: tracing refuses what running refuses,
and nothing is launched (the library is not even loaded) before the arguments have passed.  Behind the check every real
body runs inside ONE stream scope, `with _on_stream(...)`: nowhere else is the stream of the launches set.
"""
from typing import Optional, Sequence, Tuple

import torch
from torch.library import custom_op

from . import hip

BF = torch.bfloat16


class _on_stream:
    """the kernels inside run on PyTorch's current stream of a tensor's device, or of the device itself; the handle that was
    pinned before comes back on every exit, a raised exception included"""
    __slots__ = ("where", "prev")

    def __init__(self, where):
        self.where = where

    def __enter__(self):
        where = self.where
        self.prev = hip.set_stream(torch.cuda.current_stream(where.device if torch.is_tensor(where) else where).cuda_stream)

    def __exit__(self, *exc):
        hip.set_stream(self.prev)


def _c(t):
    return None if t is None else t.contiguous()


def _or_empty(t, dtype, device):
    """an output that was not asked for (None) is an empty tensor of this dtype on this device"""
    return torch.empty(0, dtype=dtype, device=device) if t is None else t


# ----------------------------------------------------------------------------------------------- linear
@custom_op("ifseg::linear", mutates_args=(), device_types="cuda")
def linear(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    with _on_stream(x):
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        out = hip.linear_fwd(x2, w.contiguous(), bias)
        return out.view(*x.shape[:-1], w.shape[0])


@linear.register_fake
def _(x, w, bias):
    return x.new_empty(*x.shape[:-1], w.shape[0])


@custom_op("ifseg::linear_bwd", mutates_args=(), device_types="cuda")
def linear_bwd(g: torch.Tensor, x: torch.Tensor, w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """-> (dx, dw, db): dx = g w, dw = g^T x, db = column sums of g (one GEMM carries dw and db)"""
    with _on_stream(g):
        g2 = g.reshape(-1, g.shape[-1]).contiguous()
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        N, K = w.shape
        dx = hip.linear_dx(g2, w.contiguous())
        buf = torch.empty(N * K + N, dtype=BF, device=g.device)          # db right behind dw: rides on the dW GEMM
        dw, db = buf[: N * K].view(N, K), buf[N * K:]
        if not hip.linear_dw(g2, x2, dw, bias_out=db):
            db.copy_(g2.float().sum(0))
        return dx.view(x.shape), dw, db.clone()           # (returns of a custom op must not share storage)


@linear_bwd.register_fake
def _(g, x, w):
    return x.new_empty(x.shape), w.new_empty(w.shape), w.new_empty(w.shape[0])


def _linear_setup(ctx, inputs, output):
    x, w, bias = inputs
    ctx.save_for_backward(x, w)
    ctx.has_bias = bias is not None


def _linear_backward(ctx, g):
    x, w = ctx.saved_tensors
    dx, dw, db = torch.ops.ifseg.linear_bwd(g, x, w)
    return dx, dw, (db if ctx.has_bias else None)


linear.register_autograd(_linear_backward, setup_context=_linear_setup)


# ----------------------------------------------------------------------------------------------- layer norm
@custom_op("ifseg::layer_norm", mutates_args=(), device_types="cuda")
def layer_norm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, gelu: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """-> (y, mean, rstd); gelu: y = LN(GELU(x)) (the FFN's ffn_layernorm(gelu(fc1)), GELU evaluated in fp32)"""
    with _on_stream(x):
        C = x.shape[-1]
        x2 = x.reshape(-1, C).contiguous()
        y = torch.empty_like(x2)
        mean = torch.empty(x2.shape[0], dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
        hip.ln_fwd(x2, gamma, beta, y, mean, rstd, gelu=gelu, eps=eps)
        return y.view(x.shape), mean, rstd


@layer_norm.register_fake
def _(x, gamma, beta, eps, gelu):
    rows = x.numel() // x.shape[-1]
    return x.new_empty(x.shape), x.new_empty(rows, dtype=torch.float32), x.new_empty(rows, dtype=torch.float32)


@custom_op("ifseg::layer_norm_bwd", mutates_args=(), device_types="cuda")
def layer_norm_bwd(dy: torch.Tensor, x: torch.Tensor, gamma: torch.Tensor, mean: torch.Tensor, rstd: torch.Tensor,
                   gelu: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    with _on_stream(x):
        C = x.shape[-1]
        x2, dy2 = x.reshape(-1, C).contiguous(), dy.reshape(-1, C).contiguous()
        dx = torch.empty_like(x2)
        part = torch.empty(2, hip.LN_BWD_BLOCKS, C, dtype=torch.float32, device=x.device)
        hip.ln_bwd(dy2, x2, gamma, mean, rstd, dx, part[0], part[1], gelu=gelu)
        dgb = torch.empty(2, C, dtype=gamma.dtype if gamma.dtype in (BF, torch.float32) else torch.float32, device=x.device)
        hip.reduce_parts(part, dgb, 2, hip.LN_BWD_BLOCKS, C)
        return dx.view(x.shape), dgb[0].clone(), dgb[1].clone()


@layer_norm_bwd.register_fake
def _(dy, x, gamma, mean, rstd, gelu):
    return x.new_empty(x.shape), gamma.new_empty(gamma.shape), gamma.new_empty(gamma.shape)


def _ln_setup(ctx, inputs, output):
    x, gamma, beta, eps, gelu = inputs
    ctx.save_for_backward(x, gamma, output[1], output[2])
    ctx.gelu = gelu


def _ln_backward(ctx, gy, gmean, grstd):
    x, gamma, mean, rstd = ctx.saved_tensors
    dx, dg, db = torch.ops.ifseg.layer_norm_bwd(gy.contiguous(), x, gamma, mean, rstd, ctx.gelu)
    return dx, dg, db, None, None


layer_norm.register_autograd(_ln_backward, setup_context=_ln_setup)


# ----------------------------------------------------------------------------------------------- attention
def _rel(P, gcode, rel2d, rel1d, relx, code_bias, grid_w):
    return None if gcode is None else hip.RelBias(P, gcode, code_bias, rel2d, rel1d, relx, grid_w=grid_w)


def _attn_bwd_fake(q, k, v, pos_q, pos_k, gain, rel2d, rel1d, relx):
    """the nine of `bias_attention_bwd` and `bias_attention_bi_bwd`"""
    f = lambda t: q.new_empty(0, dtype=torch.float32) if t is None else t.new_empty(t.shape)
    return (q.new_empty(q.shape), k.new_empty(k.shape), v.new_empty(v.shape), pos_q.new_empty(pos_q.shape),
            pos_k.new_empty(pos_k.shape), gain.new_empty(gain.shape, dtype=torch.float32), f(rel2d), f(rel1d), f(relx))


def _attn_grads(nine, gcode, settings):
    """those nine as the gradients of the forward's inputs: none for gcode, the tables' only when there are tables, none for
    the `settings` arguments behind them"""
    has = gcode is not None
    return tuple(nine[:6]) + (None,) + tuple(d if has else None for d in nine[6:]) + (None,) * settings


@custom_op("ifseg::bias_attention", mutates_args=(), device_types="cuda")
def bias_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, pos_q: torch.Tensor, pos_k: torch.Tensor,
                   gain: torch.Tensor, gcode: Optional[torch.Tensor], rel2d: Optional[torch.Tensor],
                   rel1d: Optional[torch.Tensor], relx: Optional[torch.Tensor], P: int, code_bias: int, grid_w: int,
                   causal: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """q [B,T,H*64] (already scaled), k / v [B,S,H*64], pos_q [T,H*64] (scaled), pos_k [S,H*64], gain fp32 [H];
    gcode int32 [P] + fp32 delta tables rel2d [H,n2d] / rel1d [H,2Lt-1] / relx [H,2] (or all None: no relative bias).
    -> (out [B,T,H*64] = gain_h * softmax(q k^T + pos_q pos_k^T + rel) v, lse [B,H,T] in log2 units)"""
    with _on_stream(q):
        B, T, C = q.shape
        S, H = k.shape[1], C // 64
        out = torch.empty_like(q)
        lse = torch.empty(B, H, T, dtype=torch.float32, device=q.device)
        hip.attn_fwd(q, k, v, pos_q, pos_k, out, lse, B, H, T, S, rel=_rel(P, gcode, rel2d, rel1d, relx, code_bias, grid_w),
                     causal=causal, P=P, gain=gain)
        return out, lse


@bias_attention.register_fake
def _(q, k, v, pos_q, pos_k, gain, gcode, rel2d, rel1d, relx, P, code_bias, grid_w, causal):
    B, T, C = q.shape
    return q.new_empty(q.shape), q.new_empty(B, C // 64, T, dtype=torch.float32)


@custom_op("ifseg::bias_attention_bwd", mutates_args=(), device_types="cuda")
def bias_attention_bwd(dout: torch.Tensor, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, pos_q: torch.Tensor,
                       pos_k: torch.Tensor, gain: torch.Tensor, out: torch.Tensor, lse: torch.Tensor,
                       gcode: Optional[torch.Tensor], rel2d: Optional[torch.Tensor], rel1d: Optional[torch.Tensor],
                       relx: Optional[torch.Tensor], P: int, code_bias: int, grid_w: int, causal: bool
                       ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor,
                                  torch.Tensor, torch.Tensor, torch.Tensor]:
    """-> (dq, dk, dv, dpos_q, dpos_k, dgain, drel2d, drel1d, drelx); the three table gradients are empty tensors when the
    attention has no relative bias"""
    with _on_stream(q):
        B, T, C = q.shape
        S, H = k.shape[1], C // 64
        dev = q.device
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        delta = torch.empty(B, H, T, dtype=torch.float32, device=dev)
        dpq, dpk = torch.empty(B, T, C, dtype=BF, device=dev), torch.empty(B, S, C, dtype=BF, device=dev)
        rel = _rel(P, gcode, rel2d, rel1d, relx, code_bias, grid_w)
        nparts = B * ((S + 127) // 128)
        parts = [None, None, None]
        if rel is not None:
            parts = [torch.empty(H, nparts, t.shape[1], dtype=torch.float32, device=dev) for t in (rel2d, rel1d, relx)]
        # per-row terms of d c_attn = sum_j P dP from the dQ kernel (no division of delta by the gain: exact at c_attn = 0)
        dgr = torch.empty(B, H, T, dtype=torch.float32, device=dev)
        hip.attn_bwd(q, k, v, pos_q, pos_k, out, dout.contiguous(), lse, delta, dq, dk, dv, dpq, dpk, B, H, T, S, rel=rel,
                     causal=causal, P=P, gain=gain, drel2d_part=parts[0], drel1d_part=parts[1], drelx_part=parts[2],
                     nparts=nparts, dgain_rows=dgr)
        e = torch.empty(0, dtype=torch.float32, device=dev)
        tabs = [p.sum(1) if p is not None else e for p in parts]
        dgain = dgr.sum((0, 2))
        return dq, dk, dv, dpq.float().sum(0).to(pos_q.dtype), dpk.float().sum(0).to(pos_k.dtype), dgain, tabs[0], tabs[1], tabs[2]


@bias_attention_bwd.register_fake
def _(dout, q, k, v, pos_q, pos_k, gain, out, lse, gcode, rel2d, rel1d, relx, P, code_bias, grid_w, causal):
    return _attn_bwd_fake(q, k, v, pos_q, pos_k, gain, rel2d, rel1d, relx)


def _attn_setup(ctx, inputs, output):
    q, k, v, pos_q, pos_k, gain, gcode, rel2d, rel1d, relx, P, code_bias, grid_w, causal = inputs
    ctx.save_for_backward(q, k, v, pos_q, pos_k, gain, output[0], output[1], gcode, rel2d, rel1d, relx)
    ctx.meta = (P, code_bias, grid_w, causal)


def _attn_backward(ctx, gout, glse):
    q, k, v, pos_q, pos_k, gain, out, lse, gcode, rel2d, rel1d, relx = ctx.saved_tensors
    P, code_bias, grid_w, causal = ctx.meta
    nine = torch.ops.ifseg.bias_attention_bwd(gout, q, k, v, pos_q, pos_k, gain, out, lse, gcode, rel2d, rel1d, relx, P, code_bias,
                                              grid_w, causal)
    return _attn_grads(nine, gcode, 4)


bias_attention.register_autograd(_attn_backward, setup_context=_attn_setup)


# =============================================================================================== training-path ops
# The batch-inner attention kernels (csrc/attention_bi.hip: dense bf16 bias operand, four batch elements per workgroup,
# sum_b dS once per tile, per-sample key counts, in-kernel attention dropout) and the fused criterion kernel (csrc/loss.hip):
#
#   torch.ops.ifseg.attention_bias(q, k, v, bias, gain, kv_len, causal, P, dropout_p, seed)      the bias is a tensor with a gradient
#   torch.ops.ifseg.bias_attention_bi(q, k, v, pos_q, pos_k, gain, gcode, rel2d, rel1d, relx, P, code_bias, grid_w, causal,
#                                     kv_len, dropout_p, seed)                                   bias_attention + key counts + dropout
#   torch.ops.ifseg.seg_loss(logits, target, hp, wp, H, W, seg_id_offset, label_smoothing)       x16 upsample + CE + histograms
#   torch.ops.ifseg.seg_loss_weighted(logits, target, pixel_weight, class_weight, hp, wp, H, W, seg_id_offset, label_smoothing,
#                                     norm_pixels)                                               the same with per-pixel / per-class weights
#   torch.ops.ifseg.seg_dice(logits, target, class_weight, hp, wp, H, W, seg_id_offset, dice_weight, smooth)   per-sample soft Dice
#   torch.ops.ifseg.seg_distill(logits, teacher_logits, target, hp, wp, H, W, seg_id_offset, weight, temperature, mask_all)
#                                                                                                per-pixel KL to a teacher
_pad32 = hip._pad32


def _check_qkv(op, q, k, v):
    for name, t in (("q", q), ("k", k), ("v", v)):
        if t.dim() != 3 or t.dtype != BF:
            raise ValueError("%s: %s must be a bf16 [batch, tokens, heads * 64] tensor, got %s %s" % (op, name, t.dtype, tuple(t.shape)))
        if t.stride(2) != 1:
            raise ValueError("%s: %s must have a contiguous last dimension (stride %d)" % (op, name, t.stride(2)))
    B, T, C = q.shape
    if C % 64 != 0 or C == 0:
        raise ValueError("%s: the kernels take a head dimension of 64 only: q.shape[-1] = %d is not a multiple of 64" % (op, C))
    if k.shape[0] != B or k.shape[2] != C or tuple(v.shape) != tuple(k.shape):
        raise ValueError("%s: k / v must be [%d, S, %d], got %s / %s" % (op, B, C, tuple(k.shape), tuple(v.shape)))
    if B == 0 or T == 0 or k.shape[1] == 0:
        raise ValueError("%s: empty batch or sequence" % op)
    return B, T, k.shape[1], C // 64


def _check_common(op, q, k, v, gain, kv_len, causal, P, dropout_p):
    B, T, S, H = _check_qkv(op, q, k, v)
    if gain is not None and (gain.dtype != torch.float32 or tuple(gain.shape) != (H,)):
        raise ValueError("%s: gain must be fp32 [%d], got %s %s" % (op, H, gain.dtype, tuple(gain.shape)))
    if kv_len is not None and (kv_len.dtype != torch.int32 or tuple(kv_len.shape) != (B,)):
        raise ValueError("%s: kv_len must be int32 [%d] (valid key counts), got %s %s" % (op, B, kv_len.dtype, tuple(kv_len.shape)))
    if not (0.0 <= dropout_p < 1.0):
        raise ValueError("%s: dropout_p must lie in [0, 1), got %r" % (op, dropout_p))
    if causal and (P <= 0 or P % 64 != 0 or P > min(T, S)):
        raise ValueError("%s: causal needs P (grid tokens) > 0, P %% 64 == 0 and P <= min(T, S); got P = %d, T = %d, S = %d"
                         % (op, P, T, S))
    Tp, Sp = _pad32(T), _pad32(S)
    if Tp * Sp * 2 >= 2 ** 31:
        raise ValueError("%s: the padded bias of one head (T_p * S_p * 2 = %d bytes) must stay below 2**31" % (op, Tp * Sp * 2))
    return B, T, S, H, Tp, Sp


def _attention_bias_check(q, k, v, bias, gain, kv_len, causal, P, dropout_p):
    op = "ifseg::attention_bias"
    B, T, S, H, Tp, Sp = _check_common(op, q, k, v, gain, kv_len, causal, P, dropout_p)
    if bias is not None:
        if bias.dtype not in (torch.float32, BF) or tuple(bias.shape) != (H, T, S):
            raise ValueError("%s: bias must be fp32 or bf16 [H, T, S] = [%d, %d, %d] (batch-invariant), got %s %s"
                             % (op, H, T, S, bias.dtype, tuple(bias.shape)))
        if bias.stride(2) != 1:
            raise ValueError("%s: bias must have a contiguous last dimension (stride %d)" % (op, bias.stride(2)))
    return B, T, S, H, Tp, Sp


def _bias_attention_bi_check(q, k, v, pos_q, pos_k, gain, gcode, rel2d, rel1d, relx, P, code_bias, grid_w, causal, kv_len,
                             dropout_p):
    op = "ifseg::bias_attention_bi"
    B, T, S, H, Tp, Sp = _check_common(op, q, k, v, gain, kv_len, causal, P, dropout_p)
    C = H * 64
    for name, t, n in (("pos_q", pos_q, T), ("pos_k", pos_k, S)):
        if t.dtype != BF or tuple(t.shape) != (n, C):
            raise ValueError("%s: %s must be bf16 [%d, %d], got %s %s" % (op, name, n, C, t.dtype, tuple(t.shape)))
        if t.stride(1) != 1:
            raise ValueError("%s: %s must have a contiguous last dimension (stride %d)" % (op, name, t.stride(1)))
    tabs = (gcode, rel2d, rel1d, relx)
    if any(t is None for t in tabs) != all(t is None for t in tabs):
        raise ValueError("%s: gcode, rel2d, rel1d and relx come together or not at all" % op)
    if gcode is not None:
        # what ifseg_attn_dbias_grads needs for the table gradients
        if T != S:
            raise ValueError("%s: a relative-position bias needs T == S, got T = %d, S = %d" % (op, T, S))
        if grid_w <= 0 or grid_w > 64 or grid_w % 8 != 0:
            raise ValueError("%s: grid_w must be a multiple of 8 and at most 64, got %d" % (op, grid_w))
        if P <= 0 or P % grid_w != 0 or P > T:
            raise ValueError("%s: P = grid_h * grid_w grid tokens with P <= T; got P = %d, grid_w = %d, T = %d" % (op, P, grid_w, T))
        Lt = T - P
        if gcode.dtype != torch.int32 or tuple(gcode.shape) != (P,):
            raise ValueError("%s: gcode must be int32 [P] = [%d], got %s %s" % (op, P, gcode.dtype, tuple(gcode.shape)))
        for name, t, n in (("rel2d", rel2d, None), ("rel1d", rel1d, max(2 * Lt - 1, 0)), ("relx", relx, 2)):
            if t.dtype != torch.float32 or t.dim() != 2 or t.shape[0] != H or (n is not None and t.shape[1] != n):
                raise ValueError("%s: %s must be fp32 [%d, %s], got %s %s" % (op, name, H, n if n is not None else "n2d", t.dtype, tuple(t.shape)))
    return B, T, S, H, Tp, Sp


def _aligned(t):
    """the attention kernels read 16-byte row pieces: base 16-byte aligned, row and batch strides multiples of 8 elements
    (csrc/attention_bi.hip, the entry points' checks); anything else is copied, not refused"""
    if t.data_ptr() % 16 == 0 and all(s % 8 == 0 for s in t.stride()[:-1]):
        return t
    return t.contiguous()


class _seed_as_given:
    """the dropout seed of these ops is used as given: no per-update seed word (hip.set_seed_add) during their launches"""

    def __enter__(self):
        self.prev = hip.set_seed_add(None)

    def __exit__(self, *exc):
        hip.set_seed_add(self.prev)


def _dense_view(packed, H, T, S):
    d = hip.DenseBias.__new__(hip.DenseBias)
    d.H, d.T, d.S, d.Tp, d.Sp, d.D = H, T, S, packed.shape[1], packed.shape[2], packed
    return d


def _fwd_bi(q, k, v, dense, gain, kv_len, causal, P, dropout_p, seed):
    B, T, C = q.shape
    S, H = k.shape[1], C // 64
    out = torch.empty(B, T, C, dtype=BF, device=q.device)
    lse = torch.empty(B, H, T, dtype=torch.float32, device=q.device)
    with _seed_as_given():
        hip.attn_fwd_bi(_aligned(q), _aligned(k), _aligned(v), dense, out, lse, B, H, T, S, causal=causal, P=P, gain=gain,
                        kv_len=kv_len, drop=(dropout_p, seed) if dropout_p > 0 else None)
    return out, lse


def _bwd_bi(dout, q, k, v, gain, kv_len, out, lse, dense, causal, P, dropout_p, seed, zero_slabs):
    """delta, then dQ / dK|dV of the batch-inner kernels -> (dq, dk, dv, slabs of sum_b dS, per-row terms of d gain)"""
    B, T, C = q.shape
    S, H = k.shape[1], C // 64
    dev = q.device
    q, k, v, dout = _aligned(q), _aligned(k), _aligned(v), dout.contiguous()
    dq = torch.empty(B, T, C, dtype=BF, device=dev)
    dk, dv = torch.empty(B, S, C, dtype=BF, device=dev), torch.empty(B, S, C, dtype=BF, device=dev)
    delta = torch.empty(B, H, T, dtype=torch.float32, device=dev)
    dgr = torch.empty(B, H, T, dtype=torch.float32, device=dev)
    # causal launches skip the 32-blocks above the diagonal: those entries of the slabs are never written
    slabs = (torch.zeros if zero_slabs else torch.empty)((B + 3) // 4, H, T, dense.Sp, dtype=BF, device=dev)
    hip.attn_delta(out, dout, delta, B, H, T)
    with _seed_as_given():
        hip.attn_bwd_bi(q, k, v, dout, lse, delta, dense, dq, dk, dv, slabs, B, H, T, S, causal=causal, P=P, gain=gain,
                        dgain_rows=dgr, kv_len=kv_len, drop=(dropout_p, seed) if dropout_p > 0 else None)
    return dq, dk, dv, slabs, dgr


# ----------------------------------------------------------------------------------------------- attention_bias
@custom_op("ifseg::attention_bias", mutates_args=(), device_types="cuda")
def attention_bias(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, bias: Optional[torch.Tensor],
                   gain: Optional[torch.Tensor], kv_len: Optional[torch.Tensor], causal: bool, P: int, dropout_p: float,
                   seed: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """out = gain_h * dropout(softmax(q k^T + bias [+ masks])) v on the batch-inner kernels (unify_multihead_attention.py:459-512
    with `attn_bias` an ordinary tensor, :130,464-465).

    q [B,T,H*64] bf16, already scaled; k, v [B,S,H*64] bf16 (row-strided views such as slices of a fused QKV projection are
    fine; views that miss the kernels' 16-byte alignment are copied).
    bias: None or [H,T,S], fp32 or bf16, batch-invariant, -inf = masked, differentiable (the kernels see its bf16 rounding).
    gain: None or fp32 [H] (c_attn), differentiable.  kv_len: None or int32 [B], the valid key counts (key padding as a suffix).
    causal / P: the engine's decoder layout -- P grid tokens first (P % 64 == 0), the tail behind them; grid query i sees grid
    keys j <= i and EVERY tail key, tail query i sees tail keys j <= i and no grid key.  An ordinary causal mask goes into
    `bias` as -inf with causal=False.
    dropout_p, seed: the counter-based keep mask of the kernels, the seed used as given: hip.attn_dropout_mask(B, H, T, S,
    dropout_p, seed, device) reproduces it.
    Every query row must keep at least one visible key: a fully masked row is as undefined as in the reference's softmax.
    Whole leading key blocks of a row may be masked.
    -> (out [B,T,H*64] bf16, lse fp32 [B,H,T] in log2 units, the packed bias operand bf16 [H,T_p,S_p] (not differentiable))"""
    B, T, S, H, Tp, Sp = _attention_bias_check(q, k, v, bias, gain, kv_len, causal, P, dropout_p)
    with _on_stream(q):
        dense = hip.DenseBias(H, T, S, q.device)
        hip.attn_bias_pack(dense, bias, causal=causal, P=P)
        out, lse = _fwd_bi(q, k, v, dense, gain, kv_len, causal, P, dropout_p, seed)
        return out, lse, dense.D


@attention_bias.register_fake
def _(q, k, v, bias, gain, kv_len, causal, P, dropout_p, seed):
    B, T, S, H, Tp, Sp = _attention_bias_check(q, k, v, bias, gain, kv_len, causal, P, dropout_p)
    return q.new_empty(B, T, H * 64), q.new_empty(B, H, T, dtype=torch.float32), q.new_empty(H, Tp, Sp)


@custom_op("ifseg::attention_bias_bwd", mutates_args=(), device_types="cuda")
def attention_bias_bwd(dout: torch.Tensor, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, bias: Optional[torch.Tensor],
                       gain: Optional[torch.Tensor], kv_len: Optional[torch.Tensor], out: torch.Tensor, lse: torch.Tensor,
                       packed: torch.Tensor, causal: bool, P: int, dropout_p: float, seed: int
                       ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """-> (dq, dk, dv, dbias, dgain): dbias = sum_b dS in bias's dtype and shape (an empty tensor without a bias; exactly 0
    where the bias is -inf), dgain fp32 [H]"""
    B, T, S, H, Tp, Sp = _attention_bias_check(q, k, v, bias, gain, kv_len, causal, P, dropout_p)
    with _on_stream(q):
        dense = _dense_view(packed, H, T, S)
        dq, dk, dv, slabs, dgr = _bwd_bi(dout, q, k, v, gain, kv_len, out, lse, dense, causal, P, dropout_p, seed, causal)
        if bias is not None:
            dbias = torch.empty(H, T, S, dtype=bias.dtype, device=q.device)
            hip.attn_dbias_sum(slabs, S, dbias)
        else:
            dbias = torch.empty(0, dtype=torch.float32, device=q.device)
        return dq, dk, dv, dbias, dgr.sum((0, 2))


@attention_bias_bwd.register_fake
def _(dout, q, k, v, bias, gain, kv_len, out, lse, packed, causal, P, dropout_p, seed):
    B, T, S, H, Tp, Sp = _attention_bias_check(q, k, v, bias, gain, kv_len, causal, P, dropout_p)
    dbias = q.new_empty(0, dtype=torch.float32) if bias is None else q.new_empty(H, T, S, dtype=bias.dtype)
    return q.new_empty(B, T, H * 64), q.new_empty(B, S, H * 64), q.new_empty(B, S, H * 64), dbias, q.new_empty(H, dtype=torch.float32)


def _ab_setup(ctx, inputs, output):
    q, k, v, bias, gain, kv_len, causal, P, dropout_p, seed = inputs
    ctx.save_for_backward(q, k, v, bias, gain, kv_len, output[0], output[1], output[2])
    ctx.mark_non_differentiable(output[2])
    ctx.meta = (causal, P, dropout_p, seed)


def _ab_backward(ctx, gout, glse, gpacked):
    q, k, v, bias, gain, kv_len, out, lse, packed = ctx.saved_tensors
    causal, P, dropout_p, seed = ctx.meta
    dq, dk, dv, dbias, dgain = torch.ops.ifseg.attention_bias_bwd(gout, q, k, v, bias, gain, kv_len, out, lse, packed, causal,
                                                                  P, dropout_p, seed)
    return (dq, dk, dv, dbias if bias is not None else None, dgain if gain is not None else None, None, None, None, None, None)


attention_bias.register_autograd(_ab_backward, setup_context=_ab_setup)


# ----------------------------------------------------------------------------------------------- bias_attention_bi
@custom_op("ifseg::bias_attention_bi", mutates_args=(), device_types="cuda")
def bias_attention_bi(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, pos_q: torch.Tensor, pos_k: torch.Tensor,
                      gain: torch.Tensor, gcode: Optional[torch.Tensor], rel2d: Optional[torch.Tensor],
                      rel1d: Optional[torch.Tensor], relx: Optional[torch.Tensor], P: int, code_bias: int, grid_w: int,
                      causal: bool, kv_len: Optional[torch.Tensor], dropout_p: float, seed: int
                      ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """the arguments of bias_attention plus key counts and attention dropout (see attention_bias), on the batch-inner kernels:
    the bias pos_q pos_k^T + rel is built once as the dense bf16 operand (ifseg_attn_dense_bias) and shared by the batch.
    -> (out, lse, the dense operand bf16 [H,T_p,S_p] (not differentiable))"""
    B, T, S, H, Tp, Sp = _bias_attention_bi_check(q, k, v, pos_q, pos_k, gain, gcode, rel2d, rel1d, relx, P, code_bias, grid_w,
                                                  causal, kv_len, dropout_p)
    with _on_stream(q):
        dense = hip.DenseBias(H, T, S, q.device)
        if causal:
            dense.D.fill_(float("-inf"))       # the builder leaves masked tiles that no schedule reads unwritten
        hip.attn_dense_bias(dense, _aligned(pos_q), _aligned(pos_k), rel=_rel(P, gcode, rel2d, rel1d, relx, code_bias, grid_w), causal=causal, P=P)
        out, lse = _fwd_bi(q, k, v, dense, gain, kv_len, causal, P, dropout_p, seed)
        return out, lse, dense.D


@bias_attention_bi.register_fake
def _(q, k, v, pos_q, pos_k, gain, gcode, rel2d, rel1d, relx, P, code_bias, grid_w, causal, kv_len, dropout_p, seed):
    B, T, S, H, Tp, Sp = _bias_attention_bi_check(q, k, v, pos_q, pos_k, gain, gcode, rel2d, rel1d, relx, P, code_bias, grid_w,
                                                  causal, kv_len, dropout_p)
    return q.new_empty(B, T, H * 64), q.new_empty(B, H, T, dtype=torch.float32), q.new_empty(H, Tp, Sp)


@custom_op("ifseg::bias_attention_bi_bwd", mutates_args=(), device_types="cuda")
def bias_attention_bi_bwd(dout: torch.Tensor, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, pos_q: torch.Tensor,
                          pos_k: torch.Tensor, gain: torch.Tensor, out: torch.Tensor, lse: torch.Tensor, packed: torch.Tensor,
                          gcode: Optional[torch.Tensor], rel2d: Optional[torch.Tensor], rel1d: Optional[torch.Tensor],
                          relx: Optional[torch.Tensor], P: int, code_bias: int, grid_w: int, causal: bool,
                          kv_len: Optional[torch.Tensor], dropout_p: float, seed: int
                          ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor,
                                     torch.Tensor, torch.Tensor, torch.Tensor]:
    """-> (dq, dk, dv, dpos_q, dpos_k, dgain, drel2d, drel1d, drelx) as bias_attention_bwd; everything behind sum_b dS comes
    from ifseg_attn_dbias_grads, the partial tables summed in part order"""
    B, T, S, H, Tp, Sp = _bias_attention_bi_check(q, k, v, pos_q, pos_k, gain, gcode, rel2d, rel1d, relx, P, code_bias, grid_w,
                                                  causal, kv_len, dropout_p)
    with _on_stream(q):
        dev, C = q.device, H * 64
        dense = _dense_view(packed, H, T, S)
        # (zero-filled always: on grids that are not 32 wide the table kernel reads masked pairs of blocks a causal launch skips)
        dq, dk, dv, slabs, dgr = _bwd_bi(dout, q, k, v, gain, kv_len, out, lse, dense, causal, P, dropout_p, seed, True)
        dpq = torch.empty(T, C, dtype=torch.float32, device=dev)
        dpk = torch.empty(S, C, dtype=torch.float32, device=dev)
        kw, parts = {}, None
        if gcode is not None:
            NP = hip.dbias_nparts()
            parts = [torch.empty(H, NP, t.shape[1], dtype=torch.float32, device=dev) for t in (rel2d, rel1d, relx)]
            kw = dict(P=P, grid_h=P // grid_w, grid_w=grid_w, drel2d=parts[0], drel1d=parts[1], drelx=parts[2])
        hip.attn_dbias_grads(slabs, S, pos_q=_aligned(pos_q), pos_k=_aligned(pos_k), dpq_acc=dpq, dpk_acc=dpk, accumulate_pos=False, causal=causal, **kw)
        e = torch.empty(0, dtype=torch.float32, device=dev)
        tabs = [e, e.clone(), e.clone()]
        if parts is not None:
            tabs = []
            for p in parts:
                t = torch.empty(H, p.shape[2], dtype=torch.float32, device=dev)
                tabs.append(hip.reduce_parts(p, t, H, p.shape[1], p.shape[2]) if p.shape[2] else t)
        return dq, dk, dv, dpq.to(pos_q.dtype), dpk.to(pos_k.dtype), dgr.sum((0, 2)), tabs[0], tabs[1], tabs[2]


@bias_attention_bi_bwd.register_fake
def _(dout, q, k, v, pos_q, pos_k, gain, out, lse, packed, gcode, rel2d, rel1d, relx, P, code_bias, grid_w, causal, kv_len,
      dropout_p, seed):
    _bias_attention_bi_check(q, k, v, pos_q, pos_k, gain, gcode, rel2d, rel1d, relx, P, code_bias, grid_w, causal, kv_len, dropout_p)
    return _attn_bwd_fake(q, k, v, pos_q, pos_k, gain, rel2d, rel1d, relx)


def _abi_setup(ctx, inputs, output):
    q, k, v, pos_q, pos_k, gain, gcode, rel2d, rel1d, relx, P, code_bias, grid_w, causal, kv_len, dropout_p, seed = inputs
    ctx.save_for_backward(q, k, v, pos_q, pos_k, gain, output[0], output[1], output[2], gcode, rel2d, rel1d, relx, kv_len)
    ctx.mark_non_differentiable(output[2])
    ctx.meta = (P, code_bias, grid_w, causal, dropout_p, seed)


def _abi_backward(ctx, gout, glse, gpacked):
    q, k, v, pos_q, pos_k, gain, out, lse, packed, gcode, rel2d, rel1d, relx, kv_len = ctx.saved_tensors
    P, code_bias, grid_w, causal, dropout_p, seed = ctx.meta
    nine = torch.ops.ifseg.bias_attention_bi_bwd(gout, q, k, v, pos_q, pos_k, gain, out, lse, packed, gcode, rel2d, rel1d, relx, P,
                                                 code_bias, grid_w, causal, kv_len, dropout_p, seed)
    return _attn_grads(nine, gcode, 7)


bias_attention_bi.register_autograd(_abi_backward, setup_context=_abi_setup)


# ----------------------------------------------------------------------------------------------- the seg-loss family
SEG_LOSS_MAX_CLASSES = 512       # csrc/loss.hip NS_MAX (criterions.seg_criterion.FUSED_MAX_CLASSES)


def _fused_classes_check(op, n, name="n"):
    if n < 1 or n > SEG_LOSS_MAX_CLASSES:
        raise ValueError("%s: %s = %d classes, the kernel takes 1 .. FUSED_MAX_CLASSES = %d" % (op, name, n, SEG_LOSS_MAX_CLASSES))


def _seg_loss_check(logits, target, hp, wp, H, W):
    op = "ifseg::seg_loss"
    if logits.dim() != 3 or logits.dtype != BF:
        raise ValueError("%s: logits must be bf16 [B, hp*wp + 1, nseg], got %s %s" % (op, logits.dtype, tuple(logits.shape)))
    B, rows, nseg = logits.shape
    if hp <= 0 or wp <= 0 or rows != hp * wp + 1:
        raise ValueError("%s: logits.shape[1] = %d, expected hp * wp + 1 = %d" % (op, rows, hp * wp + 1))
    if H != 16 * hp or W != 16 * wp:
        raise ValueError("%s: the fused kernel upsamples x16: H = %d, W = %d, expected H == 16 * hp = %d and W == 16 * wp = %d"
                         % (op, H, W, 16 * hp, 16 * wp))
    _fused_classes_check(op, nseg, "nseg")
    if target.dtype != torch.int64 or target.dim() != 2 or target.shape[0] != B or target.shape[1] != H * W + 1:
        raise ValueError("%s: target must be int64 [B, H * W + 1] = [%d, %d], got %s %s"
                         % (op, B, H * W + 1, target.dtype, tuple(target.shape)))
    return B, nseg, (nseg + 7) // 8 * 8


def _pixel_weight_check(op, pixel_weight, B, H, W):
    if pixel_weight is not None and (pixel_weight.dtype != torch.uint8 or tuple(pixel_weight.shape) != (B, H * W)):
        raise ValueError("%s: pixel_weight must be uint8 [B, H * W] = [%d, %d], got %s %s"
                         % (op, B, H * W, pixel_weight.dtype, tuple(pixel_weight.shape)))


def _class_weight_check(op, class_weight, nseg):
    if class_weight is not None and (class_weight.dtype != torch.float32 or tuple(class_weight.shape) != (nseg,)):
        raise ValueError("%s: class_weight must be fp32 [nseg] = [%d], got %s %s"
                         % (op, nseg, class_weight.dtype, tuple(class_weight.shape)))


def _padded_logits(logits, B, P, nseg, npad):
    """the kernels read 16-byte pieces of a class axis padded to a multiple of 8: a view that already lies in such a buffer is
    taken as it is, anything else is copied into a zero-filled one"""
    lp = logits
    if not (lp.stride(2) == 1 and lp.stride(1) % 8 == 0 and lp.stride(1) >= npad and lp.stride(0) % 8 == 0
            and lp.data_ptr() % 16 == 0):
        lp = torch.zeros(B, P + 1, npad, dtype=BF, device=logits.device)
        lp[:, :, :nseg].copy_(logits)
    return lp


def _seg_loss_fwd(kernel, logits, target, hp, wp, H, W, seg_id_offset, label_smoothing, B, nseg, npad, **weights):
    """the body of `seg_loss` (kernel = hip.seg_loss) and of `seg_loss_weighted` (hip.seg_loss_weighted, with its weights)"""
    with _on_stream(logits):
        dev, P = logits.device, hp * wp
        lp = _padded_logits(logits, B, P, nseg, npad)
        n_tiles, nstat = B * P, 2 + 3 * nseg
        tile = torch.empty(n_tiles * 9 * nseg, dtype=torch.float32, device=dev)
        sp = torch.empty(n_tiles * nstat, dtype=torch.float32, device=dev)
        stats = torch.empty(nstat, dtype=torch.float32, device=dev)
        dl = torch.empty(B, P + 1, npad, dtype=BF, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        kernel(lp, target.contiguous(), hp, wp, H, W, nseg, seg_id_offset, tile, sp, stats, dl, loss, bad_label=bad,
               label_smoothing=float(label_smoothing), **weights)
        return loss, stats, dl, bad


def _seg_loss_fake(logits, hp, wp, B, nseg, npad):
    f32 = torch.float32
    return (logits.new_empty((), dtype=f32), logits.new_empty(2 + 3 * nseg, dtype=f32), logits.new_empty(B, hp * wp + 1, npad),
            logits.new_empty(1, dtype=torch.int32))


def _seg_setup(*constants):
    """setup_context of the family: dlogits is output 2 everywhere, `constants` are the outputs that carry no gradient"""
    def setup(ctx, inputs, output):
        ctx.save_for_backward(output[2])
        ctx.mark_non_differentiable(*(output[i] for i in constants))
        ctx.nseg = inputs[0].shape[2]
    return setup


def _seg_backward(n_inputs):
    """backward of the family: differentiable in logits, the first of the op's n_inputs arguments, only"""
    def backward(ctx, gloss, *rest):
        (dl,) = ctx.saved_tensors
        return (torch.ops.ifseg.seg_loss_bwd(gloss, dl, ctx.nseg),) + (None,) * (n_inputs - 1)
    return backward


@custom_op("ifseg::seg_loss", mutates_args=(), device_types="cuda")
def seg_loss(logits: torch.Tensor, target: torch.Tensor, hp: int, wp: int, H: int, W: int, seg_id_offset: int,
             label_smoothing: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """mean cross entropy of the x16 bilinear upsample of the per-patch logits (seg_criterion.py:237-244,269-347) in the fused
    kernel pair of csrc/loss.hip.  logits bf16 [B, hp*wp+1, nseg] (the last row is eos; a row-strided view is allowed),
    target int64 [B, H*W+1] dictionary ids (pad = 1, eos = 2 and seg_id_offset + nseg are ignored).
    -> (loss fp32 [], stats fp32 [2 + 3 nseg] = CE sum, pixel count, intersect / predicted / label areas,
        dlogits bf16 [B, hp*wp+1, nseg rounded up to 8] = d loss / d logits (padding columns zero),
        bad int32 [1]: non-zero when a label is neither a class nor pad / eos / ignore -- read it when convenient, the op
        does not synchronise).  Differentiable in logits only."""
    B, nseg, npad = _seg_loss_check(logits, target, hp, wp, H, W)
    return _seg_loss_fwd(hip.seg_loss, logits, target, hp, wp, H, W, seg_id_offset, label_smoothing, B, nseg, npad)


@seg_loss.register_fake
def _(logits, target, hp, wp, H, W, seg_id_offset, label_smoothing):
    B, nseg, npad = _seg_loss_check(logits, target, hp, wp, H, W)
    return _seg_loss_fake(logits, hp, wp, B, nseg, npad)


@custom_op("ifseg::seg_loss_bwd", mutates_args=(), device_types="cuda")
def seg_loss_bwd(grad_loss: torch.Tensor, dlogits: torch.Tensor, nseg: int) -> torch.Tensor:
    """the gradient the forward kernel already produced, times the upstream gradient of the loss -> bf16 [B, hp*wp+1, nseg]"""
    g = dlogits[:, :, :nseg]
    return g * grad_loss.to(g.dtype)


@seg_loss_bwd.register_fake
def _(grad_loss, dlogits, nseg):
    return dlogits.new_empty(dlogits.shape[0], dlogits.shape[1], nseg)


seg_loss.register_autograd(_seg_backward(8), setup_context=_seg_setup(1, 2, 3))


# ----------------------------------------------------------------------------------------------- seg_loss_weighted
def _seg_loss_weighted_check(logits, target, pixel_weight, class_weight, hp, wp, H, W, label_smoothing):
    op = "ifseg::seg_loss_weighted"
    B, nseg, npad = _seg_loss_check(logits, target, hp, wp, H, W)
    _pixel_weight_check(op, pixel_weight, B, H, W)
    _class_weight_check(op, class_weight, nseg)
    if not (0.0 <= label_smoothing <= 1.0):
        raise ValueError("%s: label_smoothing must lie in [0, 1], got %r" % (op, label_smoothing))
    return B, nseg, npad


@custom_op("ifseg::seg_loss_weighted", mutates_args=(), device_types="cuda")
def seg_loss_weighted(logits: torch.Tensor, target: torch.Tensor, pixel_weight: Optional[torch.Tensor],
                      class_weight: Optional[torch.Tensor], hp: int, wp: int, H: int, W: int, seg_id_offset: int,
                      label_smoothing: float, norm_pixels: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """`seg_loss` with a weight per pixel and per class, in the weighted instantiation of the same kernel
    (`criterions.seg_criterion.weighted_loss_reference` is the specification): pixel_weight None or uint8 [B, H*W]
    (q in 0 .. 255), class_weight None or fp32 [nseg], finite and non-negative (the caller's duty: the op reads no values).
    loss = sum q l / Z over the valid pixels, l = F.cross_entropy(weight=class_weight, reduction="none", label_smoothing);
    Z = sum q cw[y], or with norm_pixels qmax N_valid (qmax = 255 with a plane, else 1); 0 when Z = 0.
    -> (loss, stats, dlogits, bad) as `seg_loss`, with stats[0] the weighted sum, stats[1] = Z and the area histograms
    counted over the valid pixels whatever their weights.  Differentiable in logits only."""
    B, nseg, npad = _seg_loss_weighted_check(logits, target, pixel_weight, class_weight, hp, wp, H, W, label_smoothing)
    return _seg_loss_fwd(hip.seg_loss_weighted, logits, target, hp, wp, H, W, seg_id_offset, label_smoothing, B, nseg, npad,
                         pixel_weight=_c(pixel_weight), class_weight=_c(class_weight), norm_pixels=norm_pixels)


@seg_loss_weighted.register_fake
def _(logits, target, pixel_weight, class_weight, hp, wp, H, W, seg_id_offset, label_smoothing, norm_pixels):
    B, nseg, npad = _seg_loss_weighted_check(logits, target, pixel_weight, class_weight, hp, wp, H, W, label_smoothing)
    return _seg_loss_fake(logits, hp, wp, B, nseg, npad)


seg_loss_weighted.register_autograd(_seg_backward(11), setup_context=_seg_setup(1, 2, 3))


# ----------------------------------------------------------------------------------------------- seg_ohem
def _seg_ohem_check(logits, target, pixel_weight, hp, wp, H, W, thresh, min_kept):
    op = "ifseg::seg_ohem"
    B, nseg, npad = _seg_loss_check(logits, target, hp, wp, H, W)
    _pixel_weight_check(op, pixel_weight, B, H, W)
    hip.check_ohem(thresh, min_kept)
    return B, nseg, npad


@custom_op("ifseg::seg_ohem", mutates_args=(), device_types="cuda")
def seg_ohem(logits: torch.Tensor, target: torch.Tensor, pixel_weight: Optional[torch.Tensor], hp: int, wp: int, H: int, W: int,
             seg_id_offset: int, thresh: float, min_kept: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """mmseg's OHEMPixelSampler(thresh, min_kept) for `seg_loss_weighted` (csrc/ohem.hip: hip.seg_hardness, then
    hip.ohem_select; `criterions.seg_criterion.hardness_reference` / `ohem_reference` are the specifications).  logits and
    target as `seg_loss`, pixel_weight None or uint8 [B, H*W] -> (weight uint8 [B, H*W]: pixel_weight (None: 255) on the kept
    pixels, 0 on the others; info int64 [4]: valid pixels, kept pixels, the bits of tau and of the k-th value), fresh tensors.
    The selection is a constant of the step: not differentiable."""
    B, nseg, npad = _seg_ohem_check(logits, target, pixel_weight, hp, wp, H, W, thresh, min_kept)
    with _on_stream(logits):
        lp = logits if logits.stride(2) == 1 else logits.contiguous()
        hard = hip.seg_hardness(lp, target.contiguous(), hp, wp, H, W, nseg, seg_id_offset)
        return hip.ohem_select(hard, thresh, min_kept, weight=_c(pixel_weight))


@seg_ohem.register_fake
def _(logits, target, pixel_weight, hp, wp, H, W, seg_id_offset, thresh, min_kept):
    B, nseg, npad = _seg_ohem_check(logits, target, pixel_weight, hp, wp, H, W, thresh, min_kept)
    return logits.new_empty((B, H * W), dtype=torch.uint8), logits.new_empty((4,), dtype=torch.int64)


# ----------------------------------------------------------------------------------------------- seg_dice
def _seg_dice_check(logits, target, class_weight, hp, wp, H, W, dice_weight, smooth):
    op = "ifseg::seg_dice"
    B, nseg, npad = _seg_loss_check(logits, target, hp, wp, H, W)
    _class_weight_check(op, class_weight, nseg)
    hip.check_dice(dice_weight, smooth, op)
    return B, nseg, npad


@custom_op("ifseg::seg_dice", mutates_args=(), device_types="cuda")
def seg_dice(logits: torch.Tensor, target: torch.Tensor, class_weight: Optional[torch.Tensor], hp: int, wp: int, H: int, W: int,
             seg_id_offset: int, dice_weight: float, smooth: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """dice_weight times the per-sample soft Dice loss of the x16 bilinear upsample of the per-patch logits (csrc/dice.hip:
    hip.seg_dice; `criterions.seg_criterion.dice_loss_reference` is the specification).  logits and target as `seg_loss`,
    class_weight None or fp32 [nseg], finite and non-negative (the caller's duty: the op reads no values).
    -> (loss fp32 [], sums fp32 [B, 3, nseg] = I, P, Y of `dice_sums_reference`,
        dlogits bf16 [B, hp*wp+1, nseg rounded up to 8] = d loss / d logits, padding columns and the eos row zero), fresh tensors.
    Differentiable in logits only."""
    B, nseg, npad = _seg_dice_check(logits, target, class_weight, hp, wp, H, W, dice_weight, smooth)
    with _on_stream(logits):
        P = hp * wp
        lp = _padded_logits(logits, B, P, nseg, npad)
        bufs = {"dl": torch.empty(B, P + 1, npad, dtype=BF, device=logits.device)}
        loss, dl = hip.seg_dice(lp, target.contiguous(), hp, wp, H, W, nseg, seg_id_offset, dice_weight, smooth,
                                class_weight=_c(class_weight), bufs=bufs)
        return loss.clone(), bufs["dice_sums"], dl


@seg_dice.register_fake
def _(logits, target, class_weight, hp, wp, H, W, seg_id_offset, dice_weight, smooth):
    B, nseg, npad = _seg_dice_check(logits, target, class_weight, hp, wp, H, W, dice_weight, smooth)
    f32 = torch.float32
    return (logits.new_empty((), dtype=f32), logits.new_empty((B, 3, nseg), dtype=f32), logits.new_empty(B, hp * wp + 1, npad))


seg_dice.register_autograd(_seg_backward(10), setup_context=_seg_setup(1, 2))


# ----------------------------------------------------------------------------------------------- seg_distill
def _seg_distill_check(logits, teacher_logits, target, hp, wp, H, W, weight, temperature, mask_all):
    op = "ifseg::seg_distill"
    if target is None:
        if not mask_all:
            raise ValueError("%s: target=None needs mask_all=True (the valid pixels are read from the target)" % op)
        stand_in = torch.empty((logits.shape[0] if logits.dim() == 3 else 0, H * W + 1), dtype=torch.int64, device="meta")
        B, nseg, npad = _seg_loss_check(logits, stand_in, hp, wp, H, W)
    else:
        B, nseg, npad = _seg_loss_check(logits, target, hp, wp, H, W)
    if teacher_logits.dtype != BF or teacher_logits.dim() != 3 or teacher_logits.shape[0] != B \
            or teacher_logits.shape[1] != hp * wp + 1 or teacher_logits.shape[2] < nseg or teacher_logits.device != logits.device:
        raise ValueError("%s: teacher_logits must be bf16 [B, hp*wp + 1, >= nseg] = [%d, %d, >= %d] on %s, got %s %s on %s"
                         % (op, B, hp * wp + 1, nseg, logits.device, teacher_logits.dtype, tuple(teacher_logits.shape),
                            teacher_logits.device))
    hip.check_distill(weight, temperature, "all" if mask_all else "valid", op)
    return B, nseg, npad


@custom_op("ifseg::seg_distill", mutates_args=(), device_types="cuda")
def seg_distill(logits: torch.Tensor, teacher_logits: torch.Tensor, target: Optional[torch.Tensor], hp: int, wp: int, H: int, W: int,
                seg_id_offset: int, weight: float, temperature: float, mask_all: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """weight times the distillation loss of the x16 bilinear upsample of the per-patch logits against a teacher's (csrc/distill.hip:
    hip.seg_distill; `criterions.seg_criterion.distill_loss_reference` is the specification): T^2 times the mean over the masked
    pixels of KL(softmax(teacher / T) || softmax(student / T)).  logits and target as `seg_loss`; teacher_logits bf16
    [B, hp*wp+1, >= nseg], a row-strided view allowed; mask_all: every pixel instead of the pixels whose target is a class (the
    target may then be None).
    -> (loss fp32 [], stats fp32 [2] = sum KL and the number of masked pixels,
        dlogits bf16 [B, hp*wp+1, nseg rounded up to 8] = d loss / d logits, padding columns and the eos row zero), fresh tensors.
    Differentiable in logits only: the teacher gets no gradient."""
    B, nseg, npad = _seg_distill_check(logits, teacher_logits, target, hp, wp, H, W, weight, temperature, mask_all)
    with _on_stream(logits):
        P = hp * wp
        lp = _padded_logits(logits, B, P, nseg, npad)
        tp = teacher_logits.detach()
        if tp.stride(2) != 1:
            tp = tp.contiguous()
        bufs = {"dl": torch.empty(B, P + 1, npad, dtype=BF, device=logits.device)}
        loss, dl = hip.seg_distill(lp, tp, _c(target), hp, wp, H, W, nseg, seg_id_offset, weight, temperature,
                                   "all" if mask_all else "valid", bufs=bufs)
        return loss.clone(), bufs["kd_stats"], dl


@seg_distill.register_fake
def _(logits, teacher_logits, target, hp, wp, H, W, seg_id_offset, weight, temperature, mask_all):
    B, nseg, npad = _seg_distill_check(logits, teacher_logits, target, hp, wp, H, W, weight, temperature, mask_all)
    f32 = torch.float32
    return (logits.new_empty((), dtype=f32), logits.new_empty((2,), dtype=f32), logits.new_empty(B, hp * wp + 1, npad))


seg_distill.register_autograd(_seg_backward(11), setup_context=_seg_setup(1, 2))


# ------------------------------------------------------------------ the predict / score family: what its checks and outputs share
def _label_dtype(n):
    return torch.uint8 if n <= 256 else torch.int16


def _scores_f32_check(op, s, view=None):
    if s.dtype != torch.float32:
        raise ValueError("%s: scores must be fp32 (hip.rows_to_f32 / hip.neighbour_smoothing give it), %s dtype %s"
                         % (op, "got" if view is None else "view %d has" % view, s.dtype))


def _views_count_check(op, K):
    if K < 1 or K > hip.SEG_PREDICT_MAX_VIEWS:
        raise ValueError("%s: %d views, the kernel takes 1 .. %d" % (op, K, hip.SEG_PREDICT_MAX_VIEWS))


def _label_map_check(op, B, h, w):
    if h < 1 or w < 1 or B * h * w >= 2 ** 31:
        raise ValueError("%s: the label map [%d, %d, %d] must have 1 <= h, w and B * h * w < 2**31" % (op, B, h, w))


def _triple(labels, conf, probs, device):
    """(labels, conf, probs) of a predict kernel as an op returns them"""
    return labels, _or_empty(conf, torch.float32, device), _or_empty(probs, torch.float32, device)


def _five(scored, n, device):
    """(areas, tally, labels, conf, probs) of a score kernel as an op returns them"""
    areas, tally, labels, conf, probs = scored
    return (areas, tally) + _triple(_or_empty(labels, _label_dtype(n), device), conf, probs, device)


def _fake_triple(like, lead, n, h, w, ldt, want_conf, want_probs, want_labels=True):
    """the fake (labels, conf, probs); lead = (B,), or () for the single image of seg_pamr"""
    f32 = torch.float32
    return (like.new_empty(lead + (h, w) if want_labels else (0,), dtype=ldt),
            like.new_empty(lead + (h, w) if want_conf else (0,), dtype=f32),
            like.new_empty(lead + (n, h, w) if want_probs else (0,), dtype=f32))


def _fake_five(like, B, n, ldt, gt, want_labels, want_conf, want_probs):
    """the fake (areas, tally, labels, conf, probs) of a score op, at the ground truth's size"""
    return ((like.new_empty((3, n), dtype=torch.int64), like.new_empty((2,), dtype=torch.int64))
            + _fake_triple(like, (B,), n, gt.shape[1], gt.shape[2], ldt, want_conf, want_probs, want_labels))


# ----------------------------------------------------------------------------------------------- seg_predict
def _seg_predict_check(scores, hp, wp, h, w):
    op = "ifseg::seg_predict"
    _scores_f32_check(op, scores)
    if scores.dim() != 3:
        raise ValueError("%s: scores must be [B, hp*wp, n], got %s" % (op, tuple(scores.shape)))
    B, P, n = scores.shape
    if B == 0:
        raise ValueError("%s: empty batch" % op)
    if hp <= 0 or wp <= 0 or P != hp * wp:
        raise ValueError("%s: scores.shape[1] = %d, expected hp * wp = %d" % (op, P, hp * wp))
    _fused_classes_check(op, n)
    _label_map_check(op, B, h, w)
    return B, n, _label_dtype(n)


@custom_op("ifseg::seg_predict", mutates_args=(), device_types="cuda")
def seg_predict(scores: torch.Tensor, hp: int, wp: int, h: int, w: int, want_conf: bool, want_probs: bool
                ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """label map at h x w from per-patch class scores fp32 [B, hp*wp, n] (csrc/predict.hip): bilinear resize
    (align_corners=False, any ratio), argmax with torch.argmax's tie rule, in one pass.
    -> (labels [B, h, w] uint8 (n <= 256) or int16, conf fp32 [B, h, w] = the winning value, probs fp32 [B, n, h, w] = every
    interpolated value); an output that was not asked for is an empty tensor.  Not differentiable."""
    _seg_predict_check(scores, hp, wp, h, w)
    with _on_stream(scores):
        return _triple(*hip.seg_predict(scores.contiguous(), hp, wp, h, w, conf=want_conf, probs=want_probs), scores.device)


@seg_predict.register_fake
def _(scores, hp, wp, h, w, want_conf, want_probs):
    B, n, ldt = _seg_predict_check(scores, hp, wp, h, w)
    return _fake_triple(scores, (B,), n, h, w, ldt, want_conf, want_probs)


# ----------------------------------------------------------------------------------------------- seg_predict_views
def _seg_predict_views_check(scores, hps, wps, flips, h, w):
    op = "ifseg::seg_predict_views"
    K = len(scores)
    _views_count_check(op, K)
    if len(hps) != K or len(wps) != K or len(flips) != K:
        raise ValueError("%s: %d views with %d hps, %d wps and %d flips (one of each per view)" % (op, K, len(hps), len(wps), len(flips)))
    for k, (s, hp, wp) in enumerate(zip(scores, hps, wps)):
        _scores_f32_check(op, s, k)
        if s.dim() != 3:
            raise ValueError("%s: scores must be [B, hp*wp, n], view %d is %s" % (op, k, tuple(s.shape)))
        if s.shape[0] != scores[0].shape[0] or s.shape[2] != scores[0].shape[2]:
            raise ValueError("%s: all views share B and n, view %d is %s against %s" % (op, k, tuple(s.shape), tuple(scores[0].shape)))
        if hp <= 0 or wp <= 0 or s.shape[1] != hp * wp:
            raise ValueError("%s: view %d: scores.shape[1] = %d, expected hp * wp = %d" % (op, k, s.shape[1], hp * wp))
    B, _, n = scores[0].shape
    if B == 0:
        raise ValueError("%s: empty batch" % op)
    _fused_classes_check(op, n)
    _label_map_check(op, B, h, w)
    return B, n, _label_dtype(n)


def _views_list(scores, hps, wps, flips):
    return [(s.contiguous(), hp, wp, bool(f)) for s, hp, wp, f in zip(scores, hps, wps, flips)]


@custom_op("ifseg::seg_predict_views", mutates_args=(), device_types="cuda")
def seg_predict_views(scores: Sequence[torch.Tensor], hps: Sequence[int], wps: Sequence[int], flips: Sequence[bool], h: int, w: int,
                      want_conf: bool, want_probs: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """label map at h x w from K views of the same images (csrc/predict.hip): view k is fp32 [B, hps[k]*wps[k], n], mirrored
    along the width when flips[k]; every view is resized as `seg_predict` does, the mean over the views (fp32, in view order)
    is what labels, conf and probs are taken from, in one launch.  Outputs and conventions as `seg_predict`.  Not differentiable."""
    _seg_predict_views_check(scores, hps, wps, flips, h, w)
    with _on_stream(scores[0]):
        return _triple(*hip.seg_predict_views(_views_list(scores, hps, wps, flips), h, w, conf=want_conf, probs=want_probs),
                       scores[0].device)


@seg_predict_views.register_fake
def _(scores, hps, wps, flips, h, w, want_conf, want_probs):
    B, n, ldt = _seg_predict_views_check(scores, hps, wps, flips, h, w)
    return _fake_triple(scores[0], (B,), n, h, w, ldt, want_conf, want_probs)


# ----------------------------------------------------------------------------------------------- seg_areas
def _gt_check(op, gt):
    if gt.dtype not in (torch.uint8, torch.int16):
        raise ValueError("%s: ground truth must be uint8 or int16 (label PNG values or class ids), got dtype %s" % (op, gt.dtype))


def _score_check(op, gt, predict_check):
    """the check of a score op: the ground truth's dtype and [B, h, w], its predict op's check at that h x w (predict_check(h, w)
    -> (B, n, label dtype)), then the ground truth's batch"""
    _gt_check(op, gt)
    if gt.dim() != 3:
        raise ValueError("%s: ground truth must be [B, h, w], got %s" % (op, tuple(gt.shape)))
    B, n, ldt = predict_check(gt.shape[1], gt.shape[2])
    if gt.shape[0] != B:
        raise ValueError("%s: ground truth %s for a batch of %d" % (op, tuple(gt.shape), B))
    return B, n, ldt


def _labels_dtype_check(op, labels):
    if labels.dtype not in (torch.uint8, torch.int16):
        raise ValueError("%s: labels must be uint8 or int16 (what seg_predict gives), got dtype %s" % (op, labels.dtype))


def _conf_check(op, labels, conf):
    if conf is not None and (conf.dtype != torch.float32 or conf.shape != labels.shape):
        raise ValueError("%s: conf must be float32 of the labels' shape %s, got %s %s"
                         % (op, tuple(labels.shape), conf.dtype, tuple(conf.shape)))


def _map_shape_check(op, labels):
    if labels.dim() not in (2, 3) or labels.numel() < 1 or labels.numel() >= 2 ** 31:
        raise ValueError("%s: labels must be [H, W] or [B, H, W] with 1 <= pixels < 2**31, got %s" % (op, tuple(labels.shape)))


def _boundary_check(op, boundary):
    if not 0 <= boundary <= hip.SEG_RENDER_MAX_BOUNDARY:
        raise ValueError("%s: boundary must be in 0 .. %d, got %d" % (op, hip.SEG_RENDER_MAX_BOUNDARY, boundary))


def _classes_check(op, n):
    if n < 1 or n > hip.SEG_PREDICT_MAX_CLASSES:
        raise ValueError("%s: n = %d classes, the kernel takes 1 .. %d" % (op, n, hip.SEG_PREDICT_MAX_CLASSES))


def _maps_check(op, labels, conf=None, gt=None):
    """a predicted label map and what lies beside it, its confidences and / or its ground truth: one shape, 1 .. 2**31 - 1 pixels"""
    _labels_dtype_check(op, labels)
    _conf_check(op, labels, conf)
    if gt is not None:
        _gt_check(op, gt)
        if labels.shape != gt.shape:
            raise ValueError("%s: labels %s and ground truth %s must have one shape" % (op, tuple(labels.shape), tuple(gt.shape)))
    if labels.numel() < 1 or labels.numel() >= 2 ** 31:
        raise ValueError("%s: 1 <= pixels < 2**31, got %s" % (op, tuple(labels.shape)))


def _seg_areas_check(labels, gt, n, op="ifseg::seg_areas"):
    _maps_check(op, labels, gt=gt)
    _fused_classes_check(op, n)


@custom_op("ifseg::seg_areas", mutates_args=(), device_types="cuda")
def seg_areas(labels: torch.Tensor, gt: torch.Tensor, n: int, raw_labels: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """predicted labels (uint8 / int16) against ground truth (uint8 / int16) of the same shape (csrc/predict.hip) ->
    (areas int64 [3, n] = per class intersect / predicted / label pixel counts over the scored pixels, tally int64 [2] = scored
    pixels, pixels with a ground truth out of range), fresh tensors; `ifseg_amd.predict.areas_reference` is the specification.
    Integer inputs: not differentiable."""
    _seg_areas_check(labels, gt, n)
    with _on_stream(labels):
        return hip.seg_areas(labels.contiguous(), gt.contiguous(), n, raw_labels)


@seg_areas.register_fake
def _(labels, gt, n, raw_labels):
    _seg_areas_check(labels, gt, n)
    return labels.new_empty((3, n), dtype=torch.int64), labels.new_empty((2,), dtype=torch.int64)


# ----------------------------------------------------------------------------------------------- seg_confusion
@custom_op("ifseg::seg_confusion", mutates_args=(), device_types="cuda")
def seg_confusion(labels: torch.Tensor, gt: torch.Tensor, n: int, raw_labels: bool) -> torch.Tensor:
    """predicted labels (uint8 / int16) against ground truth (uint8 / int16) of the same shape (csrc/predict.hip) -> the
    confusion matrix int64 [n, n + 1] over `seg_areas`' scored pixels: [c, p] = #(gt = c and pred = p), column n = predicted
    labels outside [0, n); a fresh tensor.  `ifseg_amd.predict.confusion_reference` is the specification.  Integer inputs:
    not differentiable."""
    _seg_areas_check(labels, gt, n, "ifseg::seg_confusion")
    with _on_stream(labels):
        return hip.seg_confusion(labels.contiguous(), gt.contiguous(), n, raw_labels)


@seg_confusion.register_fake
def _(labels, gt, n, raw_labels):
    _seg_areas_check(labels, gt, n, "ifseg::seg_confusion")
    return labels.new_empty((n, n + 1), dtype=torch.int64)


# ----------------------------------------------------------------------------------------------- seg_boundary_areas
def _seg_boundary_check(labels, gt, n, d):
    op = "ifseg::seg_boundary_areas"
    _seg_areas_check(labels, gt, n, op)
    if labels.dim() not in (2, 3):
        raise ValueError("%s: the maps must be [B, h, w] or [h, w], got %s" % (op, tuple(labels.shape)))
    if d < 1 or d > hip.SEG_BOUNDARY_MAX_D:
        raise ValueError("%s: d = %d, the band's half width must be in 1 .. SEG_BOUNDARY_MAX_D = %d" % (op, d, hip.SEG_BOUNDARY_MAX_D))


@custom_op("ifseg::seg_boundary_areas", mutates_args=(), device_types="cuda")
def seg_boundary_areas(labels: torch.Tensor, gt: torch.Tensor, n: int, d: int, raw_labels: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """predicted labels (uint8 / int16) against ground truth (uint8 / int16), both [B, h, w] or [h, w] (csrc/boundary.hip) ->
    (bareas int64 [3, n] = `seg_areas`' counters over the scored pixels within d of a contour of both maps / the labels / the
    ground truth, band uint8 of the maps' shape = bit 0 in the ground truth's band, bit 1 in the labels'), fresh tensors;
    `ifseg_amd.predict.boundary_areas_reference` is the specification.  Integer inputs: not differentiable."""
    _seg_boundary_check(labels, gt, n, d)
    with _on_stream(labels):
        return hip.seg_boundary_areas(labels.contiguous(), gt.contiguous(), n, d, raw_labels, band=True)


@seg_boundary_areas.register_fake
def _(labels, gt, n, d, raw_labels):
    _seg_boundary_check(labels, gt, n, d)
    return labels.new_empty((3, n), dtype=torch.int64), labels.new_empty(labels.shape, dtype=torch.uint8)


# ----------------------------------------------------------------------------------------------- seg_score_views
def _seg_score_views_check(scores, hps, wps, flips, gt):
    return _score_check("ifseg::seg_score_views", gt, lambda h, w: _seg_predict_views_check(scores, hps, wps, flips, h, w))


@custom_op("ifseg::seg_score_views", mutates_args=(), device_types="cuda")
def seg_score_views(scores: Sequence[torch.Tensor], hps: Sequence[int], wps: Sequence[int], flips: Sequence[bool], gt: torch.Tensor,
                    raw_labels: bool, want_labels: bool, want_conf: bool, want_probs: bool
                    ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """`seg_predict_views` at the shape of the ground truth gt (uint8 / int16 [B, h, w]) with the label map counted against it
    in the kernel's epilogue (a single view is K = 1) -> (areas, tally, labels, conf, probs): the counters of `seg_areas`,
    fresh, and the outputs of `seg_predict_views`, each an empty tensor when it was not asked for.  Not differentiable."""
    _seg_score_views_check(scores, hps, wps, flips, gt)
    with _on_stream(scores[0]):
        return _five(hip.seg_score_views(_views_list(scores, hps, wps, flips), gt.contiguous(), raw_labels, labels=want_labels,
                                         conf=want_conf, probs=want_probs), scores[0].shape[2], gt.device)


@seg_score_views.register_fake
def _(scores, hps, wps, flips, gt, raw_labels, want_labels, want_conf, want_probs):
    B, n, ldt = _seg_score_views_check(scores, hps, wps, flips, gt)
    return _fake_five(scores[0], B, n, ldt, gt, want_labels, want_conf, want_probs)


# ----------------------------------------------------------------------------------------------- seg_render
def _seg_render_check(labels, image, palette, opacity, boundary, boundary_color, conf):
    op = "ifseg::seg_render"
    _labels_dtype_check(op, labels)
    _map_shape_check(op, labels)
    if image.dtype != torch.uint8 or tuple(image.shape) != tuple(labels.shape) + (3,):
        raise ValueError("%s: the image must be uint8 %s (HWC, the labels' shape), got %s %s"
                         % (op, tuple(labels.shape) + (3,), image.dtype, tuple(image.shape)))
    if palette.dtype != torch.uint8 or palette.dim() != 2 or palette.shape[1] != 3 or not 1 <= palette.shape[0] <= hip.SEG_PREDICT_MAX_CLASSES:
        raise ValueError("%s: the palette must be uint8 [n, 3], 1 <= n <= %d, got %s %s"
                         % (op, hip.SEG_PREDICT_MAX_CLASSES, palette.dtype, tuple(palette.shape)))
    if not 0.0 <= opacity <= 1.0:
        raise ValueError("%s: opacity must be in [0, 1], got %r" % (op, opacity))
    _boundary_check(op, boundary)
    if len(boundary_color) != 3 or any(not 0 <= c <= 255 for c in boundary_color):
        raise ValueError("%s: boundary_color must be three ints in 0 .. 255, got %s" % (op, list(boundary_color)))
    _conf_check(op, labels, conf)


@custom_op("ifseg::seg_render", mutates_args=(), device_types="cuda")
def seg_render(labels: torch.Tensor, image: torch.Tensor, palette: torch.Tensor, opacity: float, boundary: int,
               boundary_color: Sequence[int], conf: Optional[torch.Tensor]) -> torch.Tensor:
    """the label map as a picture (csrc/render.hip): labels uint8 / int16 [.., H, W] coloured by palette uint8 [n, 3] over image
    uint8 [.., H, W, 3] at `opacity` (scaled per pixel by conf fp32 [.., H, W] when given), contours of half width `boundary`
    in `boundary_color` -> uint8 [.., H, W, 3], a fresh tensor; `ifseg_amd.predict.render_reference` is the specification.
    Integer inputs: not differentiable."""
    _seg_render_check(labels, image, palette, opacity, boundary, boundary_color, conf)
    with _on_stream(labels):
        return hip.seg_render(labels.contiguous(), image.contiguous(), palette.contiguous(), opacity, boundary,
                              tuple(int(c) for c in boundary_color), conf=_c(conf))


@seg_render.register_fake
def _(labels, image, palette, opacity, boundary, boundary_color, conf):
    _seg_render_check(labels, image, palette, opacity, boundary, boundary_color, conf)
    return image.new_empty(tuple(labels.shape) + (3,), dtype=torch.uint8)


# ----------------------------------------------------------------------------------------------- seg_conf_hist, seg_pseudo
def _seg_conf_hist_check(labels, conf, n):
    op = "ifseg::seg_conf_hist"
    _maps_check(op, labels, conf)
    _classes_check(op, n)


@custom_op("ifseg::seg_conf_hist", mutates_args=(), device_types="cuda")
def seg_conf_hist(labels: torch.Tensor, conf: torch.Tensor, n: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """predicted labels (uint8 / int16) with their confidences (fp32, the same shape) (csrc/pseudo.hip) -> (hist int64 [n, 256] =
    pixels per (label, clamp(floor(conf * 256), 0, 255)), tally int64 [2] = labels inside / outside [0, n)), fresh tensors;
    `ifseg_amd.predict.confidence_histogram_reference` is the specification.  Counts: not differentiable."""
    _seg_conf_hist_check(labels, conf, n)
    with _on_stream(labels):
        return hip.seg_conf_hist(labels.contiguous(), conf.contiguous(), n)


@seg_conf_hist.register_fake
def _(labels, conf, n):
    _seg_conf_hist_check(labels, conf, n)
    return labels.new_empty((n, hip.SEG_CONF_BINS), dtype=torch.int64), labels.new_empty((2,), dtype=torch.int64)


def _seg_calibration_check(labels, conf, gt, n):
    op = "ifseg::seg_calibration"
    _maps_check(op, labels, conf, gt)
    _classes_check(op, n)


@custom_op("ifseg::seg_calibration", mutates_args=(), device_types="cuda")
def seg_calibration(labels: torch.Tensor, conf: torch.Tensor, gt: torch.Tensor, n: int,
                    raw_labels: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """predicted labels (uint8 / int16) with their confidences (fp32) against ground truth (uint8 / int16), one shape
    (csrc/calib.hip) -> (calibration int64 [n, 256, 2] = over `seg_areas`' scored pixels, pixels per (label in [0, n),
    clamp(floor(conf * 256), 0, 255), label == gt class), tally int64 [2] = scored pixels with a label inside / outside [0, n)),
    fresh tensors; `ifseg_amd.predict.calibration_reference` is the specification.  Counts: not differentiable."""
    _seg_calibration_check(labels, conf, gt, n)
    with _on_stream(labels):
        return hip.seg_calibration(labels.contiguous(), conf.contiguous(), gt.contiguous(), n, raw_labels)


@seg_calibration.register_fake
def _(labels, conf, gt, n, raw_labels):
    _seg_calibration_check(labels, conf, gt, n)
    return labels.new_empty((n, hip.SEG_CONF_BINS, 2), dtype=torch.int64), labels.new_empty((2,), dtype=torch.int64)


def _seg_temperature_sweep_check(grids, hp, wp, gt):
    op = "ifseg::seg_temperature_sweep"
    if grids.dtype != torch.float32 or grids.dim() != 4:
        raise ValueError("%s: grids must be float32 [K, B, hp*wp, n], got %s %s" % (op, grids.dtype, tuple(grids.shape)))
    K, B, P, n = grids.shape
    if not 1 <= K <= hip.SEG_SWEEP_MAX_TEMPERATURES:
        raise ValueError("%s: K = %d grids, the kernel takes 1 .. %d" % (op, K, hip.SEG_SWEEP_MAX_TEMPERATURES))
    _classes_check(op, n)
    if hp < 1 or wp < 1 or B < 1 or P != hp * wp:
        raise ValueError("%s: grids %s do not hold B >= 1 grids of %d x %d patches" % (op, tuple(grids.shape), hp, wp))
    _gt_check(op, gt)
    if gt.dim() != 3 or gt.shape[0] != B or gt.shape[1] < 1 or gt.shape[2] < 1 or gt.numel() >= 2 ** 31:
        raise ValueError("%s: the ground truth must be [%d, h, w] with fewer than 2**31 pixels, got %s" % (op, B, tuple(gt.shape)))
    return K


@custom_op("ifseg::seg_temperature_sweep", mutates_args=(), device_types="cuda")
def seg_temperature_sweep(grids: torch.Tensor, hp: int, wp: int, gt: torch.Tensor,
                          raw_labels: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """K grids of class probabilities fp32 [K, B, hp*wp, n] (one forward's logits softmaxed at K temperatures) against ground
    truth uint8 / int16 [B, h, w] in one launch (csrc/tsweep.hip) -> (hist int64 [K, 256, 2] = per grid the scored pixels per
    (confidence bin, hit), sums float64 [K, 2] = per grid the summed negative log likelihood and Brier score, tally int64 [2] =
    scored pixels, pixels with a ground truth out of range), fresh tensors; `ifseg_amd.predict.temperature_sweep_reference` is
    the specification.  Counts and sums for choosing a temperature: no autograd."""
    _seg_temperature_sweep_check(grids, hp, wp, gt)
    with _on_stream(grids):
        return hip.seg_temperature_sweep(grids.contiguous(), hp, wp, gt.contiguous(), raw_labels)


@seg_temperature_sweep.register_fake
def _(grids, hp, wp, gt, raw_labels):
    K = _seg_temperature_sweep_check(grids, hp, wp, gt)
    return (grids.new_empty((K, hip.SEG_CONF_BINS, 2), dtype=torch.int64), grids.new_empty((K, 2), dtype=torch.float64),
            grids.new_empty((2,), dtype=torch.int64))


def _seg_pseudo_check(labels, conf, thresholds, n, boundary, raw_labels):
    op = "ifseg::seg_pseudo"
    _maps_check(op, labels, conf)
    if labels.dim() not in (2, 3):
        raise ValueError("%s: labels must be [H, W] or [B, H, W], got %s" % (op, tuple(labels.shape)))
    if n < 1 or n > hip.seg_pseudo_max_classes(raw_labels):
        raise ValueError("%s: n = %d classes, the uint8 output holds 1 .. %d with raw_labels=%s"
                         % (op, n, hip.seg_pseudo_max_classes(raw_labels), raw_labels))
    if thresholds.dtype != torch.int32 or tuple(thresholds.shape) != (n,):
        raise ValueError("%s: thresholds must be int32 [%d], got %s %s" % (op, n, thresholds.dtype, tuple(thresholds.shape)))
    _boundary_check(op, boundary)


@custom_op("ifseg::seg_pseudo", mutates_args=(), device_types="cuda")
def seg_pseudo(labels: torch.Tensor, conf: torch.Tensor, thresholds: torch.Tensor, n: int, boundary: int,
               raw_labels: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """the confidence filter of self-training (csrc/pseudo.hip): labels uint8 / int16 [.., H, W], conf fp32 of that shape,
    thresholds int32 [n] in bins -> (the pseudo-label map uint8 [.., H, W]: class + 1 with raw_labels, else class, 255 where
    the pixel is not kept; kept int64 [2, n]: kept and predicted pixels per class), fresh tensors;
    `ifseg_amd.predict.pseudo_label_reference` is the specification.  Integer outputs: not differentiable."""
    _seg_pseudo_check(labels, conf, thresholds, n, boundary, raw_labels)
    with _on_stream(labels):
        return hip.seg_pseudo(labels.contiguous(), conf.contiguous(), thresholds.contiguous(), n, boundary, raw_labels)


@seg_pseudo.register_fake
def _(labels, conf, thresholds, n, boundary, raw_labels):
    _seg_pseudo_check(labels, conf, thresholds, n, boundary, raw_labels)
    return labels.new_empty(tuple(labels.shape), dtype=torch.uint8), labels.new_empty((2, n), dtype=torch.int64)


# ----------------------------------------------------------------------------------------------- seg_regions, seg_region_drop
def _seg_regions_check(labels, connectivity, op="ifseg::seg_regions", dtypes=(torch.uint8, torch.int16)):
    if labels.dtype not in dtypes:
        raise ValueError("%s: labels must be %s, got dtype %s" % (op, " or ".join(str(d).replace("torch.", "") for d in dtypes),
                                                                 labels.dtype))
    _map_shape_check(op, labels)
    if connectivity not in (4, 8):
        raise ValueError("%s: connectivity must be 4 or 8, got %d" % (op, connectivity))


@custom_op("ifseg::seg_regions", mutates_args=(), device_types="cuda")
def seg_regions(labels: torch.Tensor, connectivity: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """the connected regions of equal values of a label map uint8 / int16 [.., H, W] (csrc/regions.hip) -> (root int32 = per
    pixel the smallest y W + x of its region inside its image, size int32 = the region's pixel count), fresh tensors of the
    labels' shape; `ifseg_amd.predict.regions_reference` is the specification.  Integer outputs: not differentiable."""
    _seg_regions_check(labels, connectivity)
    with _on_stream(labels):
        return hip.seg_regions(labels.contiguous(), connectivity)


@seg_regions.register_fake
def _(labels, connectivity):
    _seg_regions_check(labels, connectivity)
    return labels.new_empty(tuple(labels.shape), dtype=torch.int32), labels.new_empty(tuple(labels.shape), dtype=torch.int32)


def _seg_region_drop_check(labels, connectivity, min_region, fill, n):
    op = "ifseg::seg_region_drop"
    _seg_regions_check(labels, connectivity, op, (torch.uint8,))
    if not 1 <= min_region < 2 ** 31:
        raise ValueError("%s: min_region must be in 1 .. 2**31 - 1 (1 drops nothing), got %d" % (op, min_region))
    if not 0 <= fill <= 255:
        raise ValueError("%s: fill must be in 0 .. 255, got %d" % (op, fill))
    if not 1 <= n <= hip.SEG_REGION_MAX_CLASSES:
        raise ValueError("%s: n = %d classes, the counter takes 1 .. %d" % (op, n, hip.SEG_REGION_MAX_CLASSES))


@custom_op("ifseg::seg_region_drop", mutates_args=(), device_types="cuda")
def seg_region_drop(labels: torch.Tensor, connectivity: int, min_region: int, fill: int, n: int,
                    raw_labels: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """the area filter of a pseudo-label map uint8 [.., H, W] (csrc/regions.hip): every connected region of a value other than
    `fill` with fewer than min_region pixels becomes `fill` -> (out uint8, dropped int64 [n] = the dropped pixels per class,
    size int32 = every pixel's region size), fresh tensors; `ifseg_amd.predict.region_drop_reference` on
    `regions_reference`'s sizes is the specification.  A weight plane goes through `hip.seg_region_drop`, which zeroes it in
    place.  Integer outputs: not differentiable."""
    _seg_region_drop_check(labels, connectivity, min_region, fill, n)
    with _on_stream(labels):
        return hip.seg_region_drop(labels.contiguous(), connectivity, min_region, fill, n, raw_labels)


@seg_region_drop.register_fake
def _(labels, connectivity, min_region, fill, n, raw_labels):
    _seg_region_drop_check(labels, connectivity, min_region, fill, n)
    return (labels.new_empty(tuple(labels.shape), dtype=torch.uint8), labels.new_empty((n,), dtype=torch.int64),
            labels.new_empty(tuple(labels.shape), dtype=torch.int32))


# ----------------------------------------------------------------------------------------------- seg_pamr
def _seg_pamr_check(probs, image, iters, dilations):
    op = "ifseg::seg_pamr"
    if probs.dtype != torch.float32 or probs.dim() != 3:
        raise ValueError("%s: probs must be float32 [n, H, W] (one image of seg_predict's probs), got %s %s"
                         % (op, probs.dtype, tuple(probs.shape)))
    n, H, W = probs.shape
    _classes_check(op, n)
    if image.dtype != torch.uint8 or tuple(image.shape) != (H, W, 3):
        raise ValueError("%s: the image must be uint8 %s (HWC, at the values' resolution), got %s %s"
                         % (op, (H, W, 3), image.dtype, tuple(image.shape)))
    if iters < 1:
        raise ValueError("%s: iters must be >= 1, got %d" % (op, iters))
    D = len(dilations)
    if not 1 <= D <= hip.SEG_PAMR_MAX_DILATIONS or any(not 1 <= d <= hip.SEG_PAMR_MAX_DILATION for d in dilations):
        raise ValueError("%s: dilations must be 1 .. %d ints in 1 .. %d, got %s"
                         % (op, hip.SEG_PAMR_MAX_DILATIONS, hip.SEG_PAMR_MAX_DILATION, list(dilations)))
    if H < 1 or W < 1 or n * H * W >= 2 ** 31 or 8 * D * H * W >= 2 ** 31:
        raise ValueError("%s: [%d, %d, %d] values under %d dilations: n H W and 8 D H W must stay below 2**31" % (op, n, H, W, D))
    return n, H, W, _label_dtype(n)


@custom_op("ifseg::seg_pamr", mutates_args=(), device_types="cuda")
def seg_pamr(probs: torch.Tensor, image: torch.Tensor, iters: int, dilations: Sequence[int], want_conf: bool, want_probs: bool
             ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """pixel-adaptive mask refinement of one image (csrc/pamr.hip): probs fp32 [n, H, W], image uint8 [H, W, 3] -> (labels [H, W]
    uint8 (n <= 256) or int16, conf fp32 [H, W], the refined values fp32 [n, H, W]), fresh tensors; an output that was not asked
    for is an empty tensor.  `ifseg_amd.predict.pamr_reference` is the specification.  No autograd."""
    _seg_pamr_check(probs, image, iters, dilations)
    with _on_stream(probs):
        return _triple(*hip.seg_pamr(probs.contiguous(), image.contiguous(), iters, tuple(int(d) for d in dilations),
                                     conf=want_conf, probs_out=want_probs), probs.device)


@seg_pamr.register_fake
def _(probs, image, iters, dilations, want_conf, want_probs):
    n, H, W, ldt = _seg_pamr_check(probs, image, iters, dilations)
    return _fake_triple(probs, (), n, H, W, ldt, want_conf, want_probs)


# ----------------------------------------------------------------------------------------------- image_load
def _norm_check(op, mean, std, dtype):
    if len(mean) != 3 or len(std) != 3:
        raise ValueError("%s: mean and std must have three entries, got %d and %d" % (op, len(mean), len(std)))
    if dtype not in (torch.float32, BF):
        raise ValueError("%s: the output dtype must be torch.float32 or torch.bfloat16, got %s" % (op, dtype))


def _image_load_check(images, oh, ow, mean, std, dtype, op="ifseg::image_load"):
    if images.dtype != torch.uint8:
        raise ValueError("%s: images must be uint8 (raw grey levels; normalised floats go to the model as they are), got dtype %s"
                         % (op, images.dtype))
    if images.dim() != 4 or images.shape[-1] != 3:
        raise ValueError("%s: images must be [B, H0, W0, 3] (HWC), got %s" % (op, tuple(images.shape)))
    B, H0, W0, _ = images.shape
    if B == 0 or H0 == 0 or W0 == 0:
        raise ValueError("%s: empty images %s" % (op, tuple(images.shape)))
    if oh < 1 or ow < 1:
        raise ValueError("%s: the destination size must be >= 1 x 1, got %d x %d" % (op, oh, ow))
    if B * H0 * W0 * 3 >= 2 ** 31 or B * 3 * oh * ow >= 2 ** 31 or 2 * H0 * oh >= 2 ** 31 or 2 * W0 * ow >= 2 ** 31:
        raise ValueError("%s: B * H0 * W0 * 3, B * 3 * oh * ow, 2 * H0 * oh and 2 * W0 * ow must stay below 2**31, got %s -> %d x %d"
                         % (op, tuple(images.shape), oh, ow))
    _norm_check(op, mean, std, dtype)
    return B


@custom_op("ifseg::image_load", mutates_args=(), device_types="cuda")
def image_load(images: torch.Tensor, oh: int, ow: int, mean: Sequence[float], std: Sequence[float], reverse_channels: bool,
               dtype: torch.dtype) -> torch.Tensor:
    """the reference's evaluation transform (csrc/imgload.hip): uint8 [B, H0, W0, 3] -> patch_images [B, 3, oh, ow] in `dtype`
    (fp32 / bf16) by bilinear resize (align_corners=False), rounding to a grey level, optional channel reversal and
    (x / 255 - mean) / std.  The input is integer: not differentiable."""
    _image_load_check(images, oh, ow, mean, std, dtype)
    with _on_stream(images):
        return hip.image_load(images.contiguous(), oh, ow, mean, std, reverse_channels, dtype)


@image_load.register_fake
def _(images, oh, ow, mean, std, reverse_channels, dtype):
    B = _image_load_check(images, oh, ow, mean, std, dtype)
    return images.new_empty((B, 3, oh, ow), dtype=dtype)


# ----------------------------------------------------------------------------------------------- sliding windows
def _slide_check(op, oh, ow, crop, stride):
    """-> (Nw, ch, cw) of `imageio.slide_windows`; crop and stride are (h, w) pairs here (the schema has no int-or-pair)"""
    from .imageio import slide_windows
    if len(crop) != 2 or len(stride) != 2:
        raise ValueError("%s: crop and stride must be (h, w) pairs, got %r and %r" % (op, list(crop), list(stride)))
    try:
        ys, xs, ch, cw = slide_windows(oh, ow, tuple(crop), tuple(stride))
    except ValueError as e:
        raise ValueError("%s: %s" % (op, e))
    return len(ys) * len(xs), ch, cw


def _seg_predict_windows_check(scores, hpw, wpw, oh, ow, crop, stride, h, w, op="ifseg::seg_predict_windows"):
    _scores_f32_check(op, scores)
    if scores.dim() != 4:
        raise ValueError("%s: scores must be [B, Nw, hpw*wpw, n], got %s" % (op, tuple(scores.shape)))
    B, Nw, P, n = scores.shape
    if B == 0:
        raise ValueError("%s: empty batch" % op)
    nw, _, _ = _slide_check(op, oh, ow, crop, stride)
    if Nw != nw:
        raise ValueError("%s: scores.shape[1] = %d, the window rule gives %d windows" % (op, Nw, nw))
    if hpw <= 0 or wpw <= 0 or P != hpw * wpw:
        raise ValueError("%s: scores.shape[2] = %d, expected hpw * wpw = %d" % (op, P, hpw * wpw))
    if Nw * P >= 2 ** 22:
        raise ValueError("%s: Nw * hpw * wpw = %d must stay below 2**22" % (op, Nw * P))
    _fused_classes_check(op, n)
    _label_map_check(op, B, h, w)
    return B, n, _label_dtype(n)


@custom_op("ifseg::seg_predict_windows", mutates_args=(), device_types="cuda")
def seg_predict_windows(scores: torch.Tensor, hpw: int, wpw: int, oh: int, ow: int, crop: Sequence[int], stride: Sequence[int],
                        h: int, w: int, want_conf: bool, want_probs: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """label map at h x w from the windows of sliding-window inference (csrc/predict.hip): scores fp32 [B, Nw, hpw*wpw, n],
    window k of `imageio.slide_windows(oh, ow, crop, stride)`; the windows are resized, averaged where they overlap and the
    result resized to h x w in one launch.  Outputs and conventions as `seg_predict`.  Not differentiable."""
    _seg_predict_windows_check(scores, hpw, wpw, oh, ow, crop, stride, h, w)
    with _on_stream(scores):
        return _triple(*hip.seg_predict_windows(scores.contiguous(), hpw, wpw, oh, ow, tuple(crop), tuple(stride), h, w,
                                                conf=want_conf, probs=want_probs), scores.device)


@seg_predict_windows.register_fake
def _(scores, hpw, wpw, oh, ow, crop, stride, h, w, want_conf, want_probs):
    B, n, ldt = _seg_predict_windows_check(scores, hpw, wpw, oh, ow, crop, stride, h, w)
    return _fake_triple(scores, (B,), n, h, w, ldt, want_conf, want_probs)


def _seg_score_windows_check(scores, hpw, wpw, oh, ow, crop, stride, gt):
    op = "ifseg::seg_score_windows"
    return _score_check(op, gt, lambda h, w: _seg_predict_windows_check(scores, hpw, wpw, oh, ow, crop, stride, h, w, op))


@custom_op("ifseg::seg_score_windows", mutates_args=(), device_types="cuda")
def seg_score_windows(scores: torch.Tensor, hpw: int, wpw: int, oh: int, ow: int, crop: Sequence[int], stride: Sequence[int],
                      gt: torch.Tensor, raw_labels: bool, want_labels: bool, want_conf: bool, want_probs: bool
                      ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """`seg_predict_windows` at the shape of the ground truth gt (uint8 / int16 [B, h, w]) with the label map counted against
    it in the kernel's epilogue -> (areas, tally, labels, conf, probs) as `seg_score_views`.  Not differentiable."""
    _seg_score_windows_check(scores, hpw, wpw, oh, ow, crop, stride, gt)
    with _on_stream(scores):
        return _five(hip.seg_score_windows(scores.contiguous(), hpw, wpw, oh, ow, tuple(crop), tuple(stride), gt.contiguous(),
                                           raw_labels, labels=want_labels, conf=want_conf, probs=want_probs),
                     scores.shape[3], gt.device)


@seg_score_windows.register_fake
def _(scores, hpw, wpw, oh, ow, crop, stride, gt, raw_labels, want_labels, want_conf, want_probs):
    B, n, ldt = _seg_score_windows_check(scores, hpw, wpw, oh, ow, crop, stride, gt)
    return _fake_five(scores, B, n, ldt, gt, want_labels, want_conf, want_probs)


def _image_load_windows_check(images, oh, ow, crop, stride, mean, std, dtype):
    op = "ifseg::image_load_windows"
    B = _image_load_check(images, oh, ow, mean, std, dtype, op)
    nw, ch, cw = _slide_check(op, oh, ow, crop, stride)
    if B * nw * 3 * ch * cw >= 2 ** 31:
        raise ValueError("%s: the window batch [%d, 3, %d, %d] must stay below 2**31 elements" % (op, B * nw, ch, cw))
    return B * nw, ch, cw


@custom_op("ifseg::image_load_windows", mutates_args=(), device_types="cuda")
def image_load_windows(images: torch.Tensor, oh: int, ow: int, crop: Sequence[int], stride: Sequence[int], mean: Sequence[float],
                       std: Sequence[float], reverse_channels: bool, dtype: torch.dtype) -> torch.Tensor:
    """the windows of sliding-window inference, written directly (csrc/imgload.hip): uint8 [B, H0, W0, 3] -> [B Nw, 3, ch, cw] in
    `dtype`, the slices of `image_load`'s [B, 3, oh, ow] at the windows of `imageio.slide_windows(oh, ow, crop, stride)`, bit
    for bit.  The input is integer: not differentiable."""
    _image_load_windows_check(images, oh, ow, crop, stride, mean, std, dtype)
    with _on_stream(images):
        return hip.image_load_windows(images.contiguous(), oh, ow, tuple(crop), tuple(stride), mean, std, reverse_channels, dtype)


@image_load_windows.register_fake
def _(images, oh, ow, crop, stride, mean, std, reverse_channels, dtype):
    nb, ch, cw = _image_load_windows_check(images, oh, ow, crop, stride, mean, std, dtype)
    return images.new_empty((nb, 3, ch, cw), dtype=dtype)


# ----------------------------------------------------------------------------------------------- views of sliding windows
def _seg_predict_slide_views_check(scores, hpws, wpws, ohs, ows, flips, crop, stride, h, w, op="ifseg::seg_predict_slide_views"):
    K = len(scores)
    _views_count_check(op, K)
    if any(len(x) != K for x in (hpws, wpws, ohs, ows, flips)):
        raise ValueError("%s: %d views with %d hpws, %d wpws, %d ohs, %d ows and %d flips (one of each per view)"
                         % (op, K, len(hpws), len(wpws), len(ohs), len(ows), len(flips)))
    for k, s in enumerate(scores):
        if s.dim() == 4 and scores[0].dim() == 4 and (s.shape[0] != scores[0].shape[0] or s.shape[3] != scores[0].shape[3]):
            raise ValueError("%s: all views share B and n, view %d is %s against %s" % (op, k, tuple(s.shape), tuple(scores[0].shape)))
        B, n, ldt = _seg_predict_windows_check(s, hpws[k], wpws[k], ohs[k], ows[k], crop, stride, h, w, "%s: view %d" % (op, k))
    return B, n, ldt


def _slide_views_list(scores, hpws, wpws, ohs, ows, flips):
    return [(s.contiguous(), hp, wp, oh, ow, bool(f)) for s, hp, wp, oh, ow, f in zip(scores, hpws, wpws, ohs, ows, flips)]


@custom_op("ifseg::seg_predict_slide_views", mutates_args=(), device_types="cuda")
def seg_predict_slide_views(scores: Sequence[torch.Tensor], hpws: Sequence[int], wpws: Sequence[int], ohs: Sequence[int],
                            ows: Sequence[int], flips: Sequence[bool], crop: Sequence[int], stride: Sequence[int], h: int, w: int,
                            softmax: bool, want_conf: bool, want_probs: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """label map at h x w from K views, each the windows of sliding-window inference at its own [ohs[k], ows[k]] plane
    (csrc/predict.hip): view k is fp32 [B, Nw_k, hpws[k]*wpws[k], n], mirrored when flips[k]; every view is merged and resized
    as `seg_predict_windows` does, normalised over the classes when `softmax` (mmseg's order), and the mean over the views is
    what labels, conf and probs are taken from, in one launch.  Outputs and conventions as `seg_predict`.  Not differentiable."""
    _seg_predict_slide_views_check(scores, hpws, wpws, ohs, ows, flips, crop, stride, h, w)
    with _on_stream(scores[0]):
        return _triple(*hip.seg_predict_slide_views(_slide_views_list(scores, hpws, wpws, ohs, ows, flips), tuple(crop),
                                                    tuple(stride), h, w, softmax, conf=want_conf, probs=want_probs),
                       scores[0].device)


@seg_predict_slide_views.register_fake
def _(scores, hpws, wpws, ohs, ows, flips, crop, stride, h, w, softmax, want_conf, want_probs):
    B, n, ldt = _seg_predict_slide_views_check(scores, hpws, wpws, ohs, ows, flips, crop, stride, h, w)
    return _fake_triple(scores[0], (B,), n, h, w, ldt, want_conf, want_probs)


def _seg_score_slide_views_check(scores, hpws, wpws, ohs, ows, flips, crop, stride, gt):
    op = "ifseg::seg_score_slide_views"
    return _score_check(op, gt, lambda h, w: _seg_predict_slide_views_check(scores, hpws, wpws, ohs, ows, flips, crop, stride, h, w, op))


@custom_op("ifseg::seg_score_slide_views", mutates_args=(), device_types="cuda")
def seg_score_slide_views(scores: Sequence[torch.Tensor], hpws: Sequence[int], wpws: Sequence[int], ohs: Sequence[int],
                          ows: Sequence[int], flips: Sequence[bool], crop: Sequence[int], stride: Sequence[int], gt: torch.Tensor,
                          softmax: bool, raw_labels: bool, want_labels: bool, want_conf: bool, want_probs: bool
                          ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """`seg_predict_slide_views` at the shape of the ground truth gt (uint8 / int16 [B, h, w]) with the label map counted
    against it in the kernel's epilogue -> (areas, tally, labels, conf, probs) as `seg_score_views`.  Not differentiable."""
    _seg_score_slide_views_check(scores, hpws, wpws, ohs, ows, flips, crop, stride, gt)
    with _on_stream(scores[0]):
        return _five(hip.seg_score_slide_views(_slide_views_list(scores, hpws, wpws, ohs, ows, flips), tuple(crop), tuple(stride),
                                               gt.contiguous(), softmax, raw_labels, labels=want_labels, conf=want_conf,
                                               probs=want_probs), scores[0].shape[3], gt.device)


@seg_score_slide_views.register_fake
def _(scores, hpws, wpws, ohs, ows, flips, crop, stride, gt, softmax, raw_labels, want_labels, want_conf, want_probs):
    B, n, ldt = _seg_score_slide_views_check(scores, hpws, wpws, ohs, ows, flips, crop, stride, gt)
    return _fake_five(scores[0], B, n, ldt, gt, want_labels, want_conf, want_probs)


# ----------------------------------------------------------------------------------------------- train_load
def _train_load_check(images, labels, params, P, nseg, mean, std, dtype):
    from .augment import check_records
    op = "ifseg::train_load"
    B = len(images)
    if B == 0 or len(labels) != B:
        raise ValueError("%s: %d images and %d label maps (one label map per image, at least one)" % (op, B, len(labels)))
    for img, lab in zip(images, labels):
        if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[-1] != 3 or img.numel() == 0:
            raise ValueError("%s: images must be non-empty uint8 [H0, W0, 3] (HWC), got %s %s" % (op, img.dtype, tuple(img.shape)))
        if lab.dtype != torch.uint8 or tuple(lab.shape) != tuple(img.shape[:2]):
            raise ValueError("%s: label maps must be uint8 [H0, W0] of the image's size, got %s %s for an image of %s"
                             % (op, lab.dtype, tuple(lab.shape), tuple(img.shape)))
        if img.shape[0] * img.shape[1] * 3 >= 2 ** 31:
            raise ValueError("%s: H0 * W0 * 3 must stay below 2**31, got %s" % (op, tuple(img.shape)))
    check_records(params, B, op, "params")
    if P < 16 or P % 16 or P > 4096 or B * 3 * P * P >= 2 ** 31:
        raise ValueError("%s: P must be a multiple of 16 in 16 .. 4096 with B * 3 * P * P < 2**31, got P = %d, B = %d" % (op, P, B))
    if not 1 <= nseg <= 255:
        raise ValueError("%s: nseg must lie in 1 .. 255 (uint8 label maps), got %d" % (op, nseg))
    _norm_check(op, mean, std, dtype)
    return B


@custom_op("ifseg::train_load", mutates_args=(), device_types="cuda")
def train_load(images: Sequence[torch.Tensor], labels: Sequence[torch.Tensor], params: torch.Tensor, P: int, nseg: int,
               seg_id_offset: int, mean: Sequence[float], std: Sequence[float], reverse_channels: bool, raw_labels: bool,
               dtype: torch.dtype) -> Tuple[torch.Tensor, torch.Tensor]:
    """the reference's training transform under the given records (csrc/trainload.hip; ifseg_amd/augment.py is the
    specification): uint8 images [H0, W0, 3] and label maps [H0, W0] of any sizes, params int32 [B, 16] ->
    (patch_images [B, 3, P, P] in `dtype`, target int64 [B, P*P + 1]).  Integer inputs: not differentiable."""
    _train_load_check(images, labels, params, P, nseg, mean, std, dtype)
    with _on_stream(params):
        return hip.train_load([t.contiguous() for t in images], [t.contiguous() for t in labels], params.contiguous(), P, nseg,
                              seg_id_offset, mean, std, reverse_channels, raw_labels, dtype)


@train_load.register_fake
def _(images, labels, params, P, nseg, seg_id_offset, mean, std, reverse_channels, raw_labels, dtype):
    B = _train_load_check(images, labels, params, P, nseg, mean, std, dtype)
    return params.new_empty((B, 3, P, P), dtype=dtype), params.new_empty((B, P * P + 1), dtype=torch.int64)


# ----------------------------------------------------------------------------------------------- mix_draw / mix_apply
def _mix_draw_check(src_target, nseg, first_ordinal, mask):
    from .augment import check_mix, check_ordinals, mix_patch_size
    op = "ifseg::mix_draw"
    P = mix_patch_size(src_target, op)
    check_mix(P, nseg, mask, op)
    B = src_target.shape[0]
    check_ordinals(first_ordinal, B, op)
    return B


@custom_op("ifseg::mix_draw", mutates_args=(), device_types="cuda")
def mix_draw(src_target: torch.Tensor, nseg: int, seg_id_offset: int, seed: int, first_ordinal: int, mask: str) -> torch.Tensor:
    """the records int32 [B, 16] of the batch mix (csrc/mix.hip; `augment.mix_draw_reference` is the specification):
    src_target int64 [B, P*P + 1], mask "class" (ClassMix) or "box" (CutMix); a pure function of (seed, first_ordinal + b) and,
    for "class", of the classes present in sample b.  Integer inputs: not differentiable."""
    _mix_draw_check(src_target, nseg, first_ordinal, mask)
    with _on_stream(src_target):
        return hip.mix_draw(src_target.contiguous(), nseg, seg_id_offset, seed, first_ordinal, mask)


@mix_draw.register_fake
def _(src_target, nseg, seg_id_offset, seed, first_ordinal, mask):
    B = _mix_draw_check(src_target, nseg, first_ordinal, mask)
    return src_target.new_empty((B, 16), dtype=torch.int32)


def _mix_apply_check(records, src_images, src_target, src_weight, dst_images, dst_target, dst_weight, nseg):
    from .augment import check_mix, check_mix_batches, check_records
    op = "ifseg::mix_apply"
    B, P = check_mix_batches(src_images, src_target, src_weight, dst_images, dst_target, dst_weight, op)
    check_mix(P, nseg, what=op)
    check_records(records, B, op)
    if B * 3 * P * P >= 2 ** 31:
        raise ValueError("%s: B * 3 * P * P must stay below 2**31, got B = %d, P = %d" % (op, B, P))
    return B, P


@custom_op("ifseg::mix_apply", mutates_args=(), device_types="cuda")
def mix_apply(records: torch.Tensor, src_images: torch.Tensor, src_target: torch.Tensor, src_weight: Optional[torch.Tensor],
              dst_images: torch.Tensor, dst_target: torch.Tensor, dst_weight: Optional[torch.Tensor], nseg: int,
              seg_id_offset: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """the batch mix under the given records (csrc/mix.hip; `augment.mix_apply_reference` is the specification): the pixels
    a record selects take the source's image values, target and weight, the others keep the destination's ->
    (images [B, 3, P, P], target int64 [B, P*P + 1], weight uint8 [B, P*P] -- an empty tensor when neither batch has a plane).
    A copy of bits: not differentiable."""
    _mix_apply_check(records, src_images, src_target, src_weight, dst_images, dst_target, dst_weight, nseg)
    with _on_stream(records):
        img, tgt, wgt = hip.mix_apply(records.contiguous(), _c(src_images), _c(src_target), _c(dst_images), _c(dst_target), nseg,
                                      seg_id_offset, src_weight=_c(src_weight), dst_weight=_c(dst_weight))
        return img, tgt, _or_empty(wgt, torch.uint8, records.device)


@mix_apply.register_fake
def _(records, src_images, src_target, src_weight, dst_images, dst_target, dst_weight, nseg, seg_id_offset):
    B, P = _mix_apply_check(records, src_images, src_target, src_weight, dst_images, dst_target, dst_weight, nseg)
    weighted = src_weight is not None or dst_weight is not None
    return (dst_images.new_empty((B, 3, P, P)), dst_target.new_empty((B, P * P + 1)),
            records.new_empty((B, P * P) if weighted else (0,), dtype=torch.uint8))


# ----------------------------------------------------------------------------------------------- strong_draw / strong_apply
def _strong_draw_check(B, first_ordinal, jitter_p8, blur_p8):
    from .augment import check_ordinals, check_strong
    op = "ifseg::strong_draw"
    check_strong(16, jitter_p8=jitter_p8, blur_p8=blur_p8, what=op)
    check_ordinals(first_ordinal, B, op)
    return B


@custom_op("ifseg::strong_draw", mutates_args=(), device_types="cuda")
def strong_draw(B: int, seed: int, first_ordinal: int, jitter_p8: int, blur_p8: int, device: torch.device) -> torch.Tensor:
    """the records int32 [B, 16] of the strong augmentation (csrc/strong.hip; `augment.strong_draw_reference` is the
    specification): a pure function of (seed, first_ordinal + b) and the two gates.  No tensor goes in: `device` says where
    the records are written.  Not differentiable."""
    _strong_draw_check(B, first_ordinal, jitter_p8, blur_p8)
    with _on_stream(device):
        return hip.strong_draw(B, seed, first_ordinal, jitter_p8, blur_p8, device=device)


@strong_draw.register_fake
def _(B, seed, first_ordinal, jitter_p8, blur_p8, device):
    B = _strong_draw_check(B, first_ordinal, jitter_p8, blur_p8)
    return torch.empty((B, 16), dtype=torch.int32, device=device)


def _strong_apply_check(records, images, mean, std):
    from .augment import check_records, check_strong, check_strong_images
    op = "ifseg::strong_apply"
    B, P = check_strong_images(images, op)
    check_strong(P, mean, std, what=op)
    check_records(records, B, op)
    return B, P


@custom_op("ifseg::strong_apply", mutates_args=(), device_types="cuda")
def strong_apply(records: torch.Tensor, images: torch.Tensor, mean: Sequence[float], std: Sequence[float],
                 reverse_channels: bool) -> torch.Tensor:
    """colour jitter and Gaussian blur of images [B, 3, P, P] (fp32 or bf16) under the given records (csrc/strong.hip;
    `augment.strong_apply_reference` is the specification) -> images of the same shape and dtype.  Integer between the
    input and the output: not differentiable."""
    _strong_apply_check(records, images, mean, std)
    with _on_stream(images):
        return hip.strong_apply(records.contiguous(), images.contiguous(), mean, std, reverse_channels)


@strong_apply.register_fake
def _(records, images, mean, std, reverse_channels):
    B, P = _strong_apply_check(records, images, mean, std)
    return images.new_empty((B, 3, P, P))
