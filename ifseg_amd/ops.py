"""torch.library registration of the hot-path kernels: `torch.ops.ifseg.*`.

BASELINE.json north_star asks for "Python host code calling hand-written HIP kernels for CDNA4 through PyTorch-ROCm custom
ops"; SURVEY 8b names torch.library.  The engine (models/segofa/engine.py) keeps calling the C ABI directly through
`ifseg_amd.hip` -- one ctypes call per launch, no dispatcher hop on a ~570-launch step -- and this module puts the same
kernels IN FRONT OF the dispatcher as functional ops with autograd and fake (meta) implementations, for callers that
compose them with other PyTorch code (`torch.compile`, `torch.autograd.gradcheck`-style tests, export):

  torch.ops.ifseg.linear(x, w, bias)                       F.linear                      unify_multihead_attention.py:327-346,513
  torch.ops.ifseg.layer_norm(x, gamma, beta, eps, gelu)    LayerNorm (+ GELU in front)   unify_transformer_layer.py:256-292
  torch.ops.ifseg.bias_attention(q, k, v, pos_q, pos_k, gain, gcode, rel2d, rel1d, relx, P, code_bias, grid_w, causal)
                                                           position-biased attention     unify_multihead_attention.py:459-512,
                                                                                         encoder_module.py:757-809
Each op has its backward registered as further ops (`linear_bwd`, `layer_norm_bwd`, `bias_attention_bwd`), so the backward
is dispatcher-visible too.  No CPU implementation is registered: on a CPU tensor the dispatcher raises.

The second half of the file puts the training-path kernels there as well (see the comment above `_check_qkv`):
`attention_bias` (the bias is an ordinary tensor with a gradient), `bias_attention_bi` (bias_attention on the batch-inner
kernels, with key counts and attention dropout), `seg_loss` (csrc/loss.hip) and `seg_loss_weighted` (the same kernel with a
weight per pixel and per class; it shares `seg_loss_bwd`), with `*_bwd` ops of their own, and `seg_ohem` (csrc/ohem.hip: the
online-hard-example sampler that makes that weight plane; a constant of the step, no backward) and `seg_dice` (csrc/dice.hip: the
per-sample soft Dice loss of the same upsampled logits, with `seg_loss_bwd` as its backward) and `seg_distill` (csrc/distill.hip:
the per-pixel KL divergence from a teacher's upsampled logits at a temperature, `seg_loss_bwd` again; no gradient to the teacher);
`ifseg_amd.modules.MultiheadAttention` composes `linear` and `attention_bias` under the reference module's parameter names.
`seg_predict` (csrc/predict.hip: label maps at image resolution), `seg_predict_views` (the same from the mean of K views of
differing grids, mirrored ones included: multi-scale + flip inference), `seg_areas` / `seg_score_views` (label maps counted
against ground truth, stand-alone and in the predict kernel's epilogue: mIoU on the device), `seg_confusion` (the class
confusion matrix of a label map against ground truth, [n, n + 1] with an "outside" column), `seg_boundary_areas` (csrc/boundary.hip: Boundary IoU's band areas and the two bands), `image_load` (csrc/imgload.hip: raw uint8 images to
normalised patch_images, the reference's evaluation transform) and the three ops of sliding-window inference (`image_load_windows`,
`seg_predict_windows`, `seg_score_windows`: the window batch written directly, and the windows' scores merged into one label
map in one launch), `seg_render` (csrc/render.hip: the label map coloured over its image, with class contours), `seg_conf_hist` / `seg_pseudo`
(csrc/pseudo.hip: the per-class confidence histogram of a label map, and the label map filtered by per-class thresholds and an
ignore band along class edges into pseudo-labels for self-training), `seg_regions` / `seg_region_drop` (csrc/regions.hip: the
connected regions of equal values of a label map, and the map with its regions below a pixel count dropped), `seg_calibration` (csrc/calib.hip: how often a confidence
is right, pixels per predicted class, confidence bin and hit against ground truth), `seg_temperature_sweep` (csrc/tsweep.hip: K
grids of one forward at K temperatures against one ground truth, per temperature the reliability counts, NLL and Brier),
`seg_pamr` (csrc/pamr.hip: pixel-adaptive mask refinement of one image's class values, guided by its photograph) and the two of multi-scale + flip over sliding windows (`seg_predict_slide_views`, `seg_score_slide_views`:
K views, each a set of windows, merged in one launch, optionally softmaxed per view as mmseg does) are inference only and
have no backward; `train_load`
(csrc/trainload.hip: raw images and label maps of any sizes to a training batch under given records, the reference's training
transform) has integer inputs and no backward either, and neither have `mix_draw` / `mix_apply` (csrc/mix.hip: ClassMix /
CutMix of a labelled batch into a pseudo-labelled one -- the choice of classes or of a box, and the paste of images, targets
and weight planes, which copies bits) and `strong_draw` / `strong_apply` (csrc/strong.hip: colour jitter and Gaussian blur of a
mixed batch's images, integer between input and output).
"""
import contextlib
from typing import Optional, Sequence, Tuple

import torch
from torch.library import custom_op

from . import hip

BF = torch.bfloat16


def _stream_scope(t):
    """the kernels run on PyTorch's current stream of the tensor's device"""
    return hip.set_stream(torch.cuda.current_stream(t.device).cuda_stream)


# ----------------------------------------------------------------------------------------------- linear
@custom_op("ifseg::linear", mutates_args=(), device_types="cuda")
def linear(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    prev = _stream_scope(x)
    try:
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        out = hip.linear_fwd(x2, w.contiguous(), bias)
        return out.view(*x.shape[:-1], w.shape[0])
    finally:
        hip.set_stream(prev)


@linear.register_fake
def _(x, w, bias):
    return x.new_empty(*x.shape[:-1], w.shape[0])


@custom_op("ifseg::linear_bwd", mutates_args=(), device_types="cuda")
def linear_bwd(g: torch.Tensor, x: torch.Tensor, w: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """-> (dx, dw, db): dx = g w, dw = g^T x, db = column sums of g (one GEMM carries dw and db)"""
    prev = _stream_scope(g)
    try:
        g2 = g.reshape(-1, g.shape[-1]).contiguous()
        x2 = x.reshape(-1, x.shape[-1]).contiguous()
        N, K = w.shape
        dx = hip.linear_dx(g2, w.contiguous())
        buf = torch.empty(N * K + N, dtype=BF, device=g.device)          # db right behind dw: rides on the dW GEMM
        dw, db = buf[: N * K].view(N, K), buf[N * K:]
        if not hip.linear_dw(g2, x2, dw, bias_out=db):
            db.copy_(g2.float().sum(0))
        return dx.view(x.shape), dw, db.clone()           # (returns of a custom op must not share storage)
    finally:
        hip.set_stream(prev)


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
    prev = _stream_scope(x)
    try:
        C = x.shape[-1]
        x2 = x.reshape(-1, C).contiguous()
        y = torch.empty_like(x2)
        mean = torch.empty(x2.shape[0], dtype=torch.float32, device=x.device)
        rstd = torch.empty_like(mean)
        hip.ln_fwd(x2, gamma, beta, y, mean, rstd, gelu=gelu, eps=eps)
        return y.view(x.shape), mean, rstd
    finally:
        hip.set_stream(prev)


@layer_norm.register_fake
def _(x, gamma, beta, eps, gelu):
    rows = x.numel() // x.shape[-1]
    return x.new_empty(x.shape), x.new_empty(rows, dtype=torch.float32), x.new_empty(rows, dtype=torch.float32)


@custom_op("ifseg::layer_norm_bwd", mutates_args=(), device_types="cuda")
def layer_norm_bwd(dy: torch.Tensor, x: torch.Tensor, gamma: torch.Tensor, mean: torch.Tensor, rstd: torch.Tensor,
                   gelu: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    prev = _stream_scope(x)
    try:
        C = x.shape[-1]
        x2, dy2 = x.reshape(-1, C).contiguous(), dy.reshape(-1, C).contiguous()
        dx = torch.empty_like(x2)
        part = torch.empty(2, hip.LN_BWD_BLOCKS, C, dtype=torch.float32, device=x.device)
        hip.ln_bwd(dy2, x2, gamma, mean, rstd, dx, part[0], part[1], gelu=gelu)
        dgb = torch.empty(2, C, dtype=gamma.dtype if gamma.dtype in (BF, torch.float32) else torch.float32, device=x.device)
        hip.reduce_parts(part, dgb, 2, hip.LN_BWD_BLOCKS, C)
        return dx.view(x.shape), dgb[0].clone(), dgb[1].clone()
    finally:
        hip.set_stream(prev)


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


@custom_op("ifseg::bias_attention", mutates_args=(), device_types="cuda")
def bias_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, pos_q: torch.Tensor, pos_k: torch.Tensor,
                   gain: torch.Tensor, gcode: Optional[torch.Tensor], rel2d: Optional[torch.Tensor],
                   rel1d: Optional[torch.Tensor], relx: Optional[torch.Tensor], P: int, code_bias: int, grid_w: int,
                   causal: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """q [B,T,H*64] (already scaled), k / v [B,S,H*64], pos_q [T,H*64] (scaled), pos_k [S,H*64], gain fp32 [H];
    gcode int32 [P] + fp32 delta tables rel2d [H,n2d] / rel1d [H,2Lt-1] / relx [H,2] (or all None: no relative bias).
    -> (out [B,T,H*64] = gain_h * softmax(q k^T + pos_q pos_k^T + rel) v, lse [B,H,T] in log2 units)"""
    prev = _stream_scope(q)
    try:
        B, T, C = q.shape
        S, H = k.shape[1], C // 64
        out = torch.empty_like(q)
        lse = torch.empty(B, H, T, dtype=torch.float32, device=q.device)
        hip.attn_fwd(q, k, v, pos_q, pos_k, out, lse, B, H, T, S, rel=_rel(P, gcode, rel2d, rel1d, relx, code_bias, grid_w),
                     causal=causal, P=P, gain=gain)
        return out, lse
    finally:
        hip.set_stream(prev)


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
    prev = _stream_scope(q)
    try:
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
    finally:
        hip.set_stream(prev)


@bias_attention_bwd.register_fake
def _(dout, q, k, v, pos_q, pos_k, gain, out, lse, gcode, rel2d, rel1d, relx, P, code_bias, grid_w, causal):
    e = q.new_empty(0, dtype=torch.float32)
    f = lambda t: e if t is None else t.new_empty(t.shape)
    return (q.new_empty(q.shape), k.new_empty(k.shape), v.new_empty(v.shape), pos_q.new_empty(pos_q.shape),
            pos_k.new_empty(pos_k.shape), gain.new_empty(gain.shape, dtype=torch.float32), f(rel2d), f(rel1d), f(relx))


def _attn_setup(ctx, inputs, output):
    q, k, v, pos_q, pos_k, gain, gcode, rel2d, rel1d, relx, P, code_bias, grid_w, causal = inputs
    ctx.save_for_backward(q, k, v, pos_q, pos_k, gain, output[0], output[1], gcode, rel2d, rel1d, relx)
    ctx.meta = (P, code_bias, grid_w, causal)


def _attn_backward(ctx, gout, glse):
    q, k, v, pos_q, pos_k, gain, out, lse, gcode, rel2d, rel1d, relx = ctx.saved_tensors
    P, code_bias, grid_w, causal = ctx.meta
    dq, dk, dv, dpq, dpk, dgain, d2, d1, dx = torch.ops.ifseg.bias_attention_bwd(
        gout, q, k, v, pos_q, pos_k, gain, out, lse, gcode, rel2d, rel1d, relx, P, code_bias, grid_w, causal)
    has = gcode is not None
    return (dq, dk, dv, dpq, dpk, dgain, None, d2 if has else None, d1 if has else None, dx if has else None,
            None, None, None, None)


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
#
# Every op has ONE check helper that its real and its fake implementation call first: tracing refuses what running refuses,
# and nothing is launched (the library is not even loaded) before the arguments have passed.
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
    prev = _stream_scope(q)
    try:
        dense = hip.DenseBias(H, T, S, q.device)
        hip.attn_bias_pack(dense, bias, causal=causal, P=P)
        out, lse = _fwd_bi(q, k, v, dense, gain, kv_len, causal, P, dropout_p, seed)
        return out, lse, dense.D
    finally:
        hip.set_stream(prev)


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
    prev = _stream_scope(q)
    try:
        dense = _dense_view(packed, H, T, S)
        dq, dk, dv, slabs, dgr = _bwd_bi(dout, q, k, v, gain, kv_len, out, lse, dense, causal, P, dropout_p, seed, causal)
        if bias is not None:
            dbias = torch.empty(H, T, S, dtype=bias.dtype, device=q.device)
            hip.attn_dbias_sum(slabs, S, dbias)
        else:
            dbias = torch.empty(0, dtype=torch.float32, device=q.device)
        return dq, dk, dv, dbias, dgr.sum((0, 2))
    finally:
        hip.set_stream(prev)


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
    prev = _stream_scope(q)
    try:
        dense = hip.DenseBias(H, T, S, q.device)
        if causal:
            dense.D.fill_(float("-inf"))       # the builder leaves masked tiles that no schedule reads unwritten
        hip.attn_dense_bias(dense, _aligned(pos_q), _aligned(pos_k), rel=_rel(P, gcode, rel2d, rel1d, relx, code_bias, grid_w), causal=causal, P=P)
        out, lse = _fwd_bi(q, k, v, dense, gain, kv_len, causal, P, dropout_p, seed)
        return out, lse, dense.D
    finally:
        hip.set_stream(prev)


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
    prev = _stream_scope(q)
    try:
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
    finally:
        hip.set_stream(prev)


@bias_attention_bi_bwd.register_fake
def _(dout, q, k, v, pos_q, pos_k, gain, out, lse, packed, gcode, rel2d, rel1d, relx, P, code_bias, grid_w, causal, kv_len,
      dropout_p, seed):
    _bias_attention_bi_check(q, k, v, pos_q, pos_k, gain, gcode, rel2d, rel1d, relx, P, code_bias, grid_w, causal, kv_len, dropout_p)
    f = lambda t: q.new_empty(0, dtype=torch.float32) if t is None else t.new_empty(t.shape)
    return (q.new_empty(q.shape), k.new_empty(k.shape), v.new_empty(v.shape), pos_q.new_empty(pos_q.shape),
            pos_k.new_empty(pos_k.shape), gain.new_empty(gain.shape, dtype=torch.float32), f(rel2d), f(rel1d), f(relx))


def _abi_setup(ctx, inputs, output):
    q, k, v, pos_q, pos_k, gain, gcode, rel2d, rel1d, relx, P, code_bias, grid_w, causal, kv_len, dropout_p, seed = inputs
    ctx.save_for_backward(q, k, v, pos_q, pos_k, gain, output[0], output[1], output[2], gcode, rel2d, rel1d, relx, kv_len)
    ctx.mark_non_differentiable(output[2])
    ctx.meta = (P, code_bias, grid_w, causal, dropout_p, seed)


def _abi_backward(ctx, gout, glse, gpacked):
    q, k, v, pos_q, pos_k, gain, out, lse, packed, gcode, rel2d, rel1d, relx, kv_len = ctx.saved_tensors
    P, code_bias, grid_w, causal, dropout_p, seed = ctx.meta
    dq, dk, dv, dpq, dpk, dgain, d2, d1, dx = torch.ops.ifseg.bias_attention_bi_bwd(
        gout, q, k, v, pos_q, pos_k, gain, out, lse, packed, gcode, rel2d, rel1d, relx, P, code_bias, grid_w, causal, kv_len,
        dropout_p, seed)
    has = gcode is not None
    return (dq, dk, dv, dpq, dpk, dgain, None, d2 if has else None, d1 if has else None, dx if has else None,
            None, None, None, None, None, None, None)


bias_attention_bi.register_autograd(_abi_backward, setup_context=_abi_setup)


# ----------------------------------------------------------------------------------------------- seg_loss
SEG_LOSS_MAX_CLASSES = 512       # csrc/loss.hip NS_MAX (criterions.seg_criterion.FUSED_MAX_CLASSES)


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
    if nseg < 1 or nseg > SEG_LOSS_MAX_CLASSES:
        raise ValueError("%s: nseg = %d classes, the kernel takes 1 .. FUSED_MAX_CLASSES = %d" % (op, nseg, SEG_LOSS_MAX_CLASSES))
    if target.dtype != torch.int64 or target.dim() != 2 or target.shape[0] != B or target.shape[1] != H * W + 1:
        raise ValueError("%s: target must be int64 [B, H * W + 1] = [%d, %d], got %s %s"
                         % (op, B, H * W + 1, target.dtype, tuple(target.shape)))
    return B, nseg, (nseg + 7) // 8 * 8


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
    prev = _stream_scope(logits)
    try:
        dev, P = logits.device, hp * wp
        # the kernel reads 16-byte pieces of a class axis padded to a multiple of 8: a view that already lies in such a
        # buffer is taken as it is
        lp = logits
        if not (lp.stride(2) == 1 and lp.stride(1) % 8 == 0 and lp.stride(1) >= npad and lp.stride(0) % 8 == 0
                and lp.data_ptr() % 16 == 0):
            lp = torch.zeros(B, P + 1, npad, dtype=BF, device=dev)
            lp[:, :, :nseg].copy_(logits)
        n_tiles, nstat = B * P, 2 + 3 * nseg
        tile = torch.empty(n_tiles * 9 * nseg, dtype=torch.float32, device=dev)
        sp = torch.empty(n_tiles * nstat, dtype=torch.float32, device=dev)
        stats = torch.empty(nstat, dtype=torch.float32, device=dev)
        dl = torch.empty(B, P + 1, npad, dtype=BF, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        hip.seg_loss(lp, target.contiguous(), hp, wp, H, W, nseg, seg_id_offset, tile, sp, stats, dl, loss, bad_label=bad,
                     label_smoothing=float(label_smoothing))
        return loss, stats, dl, bad
    finally:
        hip.set_stream(prev)


@seg_loss.register_fake
def _(logits, target, hp, wp, H, W, seg_id_offset, label_smoothing):
    B, nseg, npad = _seg_loss_check(logits, target, hp, wp, H, W)
    f32 = torch.float32
    return (logits.new_empty((), dtype=f32), logits.new_empty(2 + 3 * nseg, dtype=f32), logits.new_empty(B, hp * wp + 1, npad),
            logits.new_empty(1, dtype=torch.int32))


@custom_op("ifseg::seg_loss_bwd", mutates_args=(), device_types="cuda")
def seg_loss_bwd(grad_loss: torch.Tensor, dlogits: torch.Tensor, nseg: int) -> torch.Tensor:
    """the gradient the forward kernel already produced, times the upstream gradient of the loss -> bf16 [B, hp*wp+1, nseg]"""
    g = dlogits[:, :, :nseg]
    return g * grad_loss.to(g.dtype)


@seg_loss_bwd.register_fake
def _(grad_loss, dlogits, nseg):
    return dlogits.new_empty(dlogits.shape[0], dlogits.shape[1], nseg)


def _sl_setup(ctx, inputs, output):
    ctx.save_for_backward(output[2])
    ctx.mark_non_differentiable(output[1], output[2], output[3])
    ctx.nseg = inputs[0].shape[2]


def _sl_backward(ctx, gloss, gstats, gdl, gbad):
    (dl,) = ctx.saved_tensors
    return torch.ops.ifseg.seg_loss_bwd(gloss, dl, ctx.nseg), None, None, None, None, None, None, None


seg_loss.register_autograd(_sl_backward, setup_context=_sl_setup)


# ----------------------------------------------------------------------------------------------- seg_loss_weighted
def _seg_loss_weighted_check(logits, target, pixel_weight, class_weight, hp, wp, H, W, label_smoothing):
    op = "ifseg::seg_loss_weighted"
    B, nseg, npad = _seg_loss_check(logits, target, hp, wp, H, W)
    if pixel_weight is not None and (pixel_weight.dtype != torch.uint8 or tuple(pixel_weight.shape) != (B, H * W)):
        raise ValueError("%s: pixel_weight must be uint8 [B, H * W] = [%d, %d], got %s %s"
                         % (op, B, H * W, pixel_weight.dtype, tuple(pixel_weight.shape)))
    if class_weight is not None and (class_weight.dtype != torch.float32 or tuple(class_weight.shape) != (nseg,)):
        raise ValueError("%s: class_weight must be fp32 [nseg] = [%d], got %s %s"
                         % (op, nseg, class_weight.dtype, tuple(class_weight.shape)))
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
    prev = _stream_scope(logits)
    try:
        dev, P = logits.device, hp * wp
        lp = logits
        if not (lp.stride(2) == 1 and lp.stride(1) % 8 == 0 and lp.stride(1) >= npad and lp.stride(0) % 8 == 0
                and lp.data_ptr() % 16 == 0):
            lp = torch.zeros(B, P + 1, npad, dtype=BF, device=dev)
            lp[:, :, :nseg].copy_(logits)
        n_tiles, nstat = B * P, 2 + 3 * nseg
        tile = torch.empty(n_tiles * 9 * nseg, dtype=torch.float32, device=dev)
        sp = torch.empty(n_tiles * nstat, dtype=torch.float32, device=dev)
        stats = torch.empty(nstat, dtype=torch.float32, device=dev)
        dl = torch.empty(B, P + 1, npad, dtype=BF, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        hip.seg_loss_weighted(lp, target.contiguous(), hp, wp, H, W, nseg, seg_id_offset, tile, sp, stats, dl, loss,
                              pixel_weight=pixel_weight.contiguous() if pixel_weight is not None else None,
                              class_weight=class_weight.contiguous() if class_weight is not None else None,
                              norm_pixels=norm_pixels, bad_label=bad, label_smoothing=float(label_smoothing))
        return loss, stats, dl, bad
    finally:
        hip.set_stream(prev)


@seg_loss_weighted.register_fake
def _(logits, target, pixel_weight, class_weight, hp, wp, H, W, seg_id_offset, label_smoothing, norm_pixels):
    B, nseg, npad = _seg_loss_weighted_check(logits, target, pixel_weight, class_weight, hp, wp, H, W, label_smoothing)
    f32 = torch.float32
    return (logits.new_empty((), dtype=f32), logits.new_empty(2 + 3 * nseg, dtype=f32), logits.new_empty(B, hp * wp + 1, npad),
            logits.new_empty(1, dtype=torch.int32))


def _slw_backward(ctx, gloss, gstats, gdl, gbad):
    (dl,) = ctx.saved_tensors
    return (torch.ops.ifseg.seg_loss_bwd(gloss, dl, ctx.nseg),) + (None,) * 10


seg_loss_weighted.register_autograd(_slw_backward, setup_context=_sl_setup)


# ----------------------------------------------------------------------------------------------- seg_ohem
def _seg_ohem_check(logits, target, pixel_weight, hp, wp, H, W, thresh, min_kept):
    op = "ifseg::seg_ohem"
    B, nseg, npad = _seg_loss_check(logits, target, hp, wp, H, W)
    if pixel_weight is not None and (pixel_weight.dtype != torch.uint8 or tuple(pixel_weight.shape) != (B, H * W)):
        raise ValueError("%s: pixel_weight must be uint8 [B, H * W] = [%d, %d], got %s %s"
                         % (op, B, H * W, pixel_weight.dtype, tuple(pixel_weight.shape)))
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
    prev = _stream_scope(logits)
    try:
        lp = logits if logits.stride(2) == 1 else logits.contiguous()
        hard = hip.seg_hardness(lp, target.contiguous(), hp, wp, H, W, nseg, seg_id_offset)
        return hip.ohem_select(hard, thresh, min_kept, weight=pixel_weight.contiguous() if pixel_weight is not None else None)
    finally:
        hip.set_stream(prev)


@seg_ohem.register_fake
def _(logits, target, pixel_weight, hp, wp, H, W, seg_id_offset, thresh, min_kept):
    B, nseg, npad = _seg_ohem_check(logits, target, pixel_weight, hp, wp, H, W, thresh, min_kept)
    return logits.new_empty((B, H * W), dtype=torch.uint8), logits.new_empty((4,), dtype=torch.int64)


# ----------------------------------------------------------------------------------------------- seg_dice
def _seg_dice_check(logits, target, class_weight, hp, wp, H, W, dice_weight, smooth):
    op = "ifseg::seg_dice"
    B, nseg, npad = _seg_loss_check(logits, target, hp, wp, H, W)
    if class_weight is not None and (class_weight.dtype != torch.float32 or tuple(class_weight.shape) != (nseg,)):
        raise ValueError("%s: class_weight must be fp32 [nseg] = [%d], got %s %s"
                         % (op, nseg, class_weight.dtype, tuple(class_weight.shape)))
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
    prev = _stream_scope(logits)
    try:
        dev, P = logits.device, hp * wp
        lp = logits
        if not (lp.stride(2) == 1 and lp.stride(1) % 8 == 0 and lp.stride(1) >= npad and lp.stride(0) % 8 == 0
                and lp.data_ptr() % 16 == 0):
            lp = torch.zeros(B, P + 1, npad, dtype=BF, device=dev)
            lp[:, :, :nseg].copy_(logits)
        bufs = {"dl": torch.empty(B, P + 1, npad, dtype=BF, device=dev)}
        loss, dl = hip.seg_dice(lp, target.contiguous(), hp, wp, H, W, nseg, seg_id_offset, dice_weight, smooth,
                                class_weight=class_weight.contiguous() if class_weight is not None else None, bufs=bufs)
        return loss.clone(), bufs["dice_sums"], dl
    finally:
        hip.set_stream(prev)


@seg_dice.register_fake
def _(logits, target, class_weight, hp, wp, H, W, seg_id_offset, dice_weight, smooth):
    B, nseg, npad = _seg_dice_check(logits, target, class_weight, hp, wp, H, W, dice_weight, smooth)
    f32 = torch.float32
    return (logits.new_empty((), dtype=f32), logits.new_empty((B, 3, nseg), dtype=f32), logits.new_empty(B, hp * wp + 1, npad))


def _sd_setup(ctx, inputs, output):
    ctx.save_for_backward(output[2])
    ctx.mark_non_differentiable(output[1], output[2])
    ctx.nseg = inputs[0].shape[2]


def _sd_backward(ctx, gloss, gsums, gdl):
    (dl,) = ctx.saved_tensors
    return (torch.ops.ifseg.seg_loss_bwd(gloss, dl, ctx.nseg),) + (None,) * 9


seg_dice.register_autograd(_sd_backward, setup_context=_sd_setup)


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
    prev = _stream_scope(logits)
    try:
        dev, P = logits.device, hp * wp
        lp = logits
        if not (lp.stride(2) == 1 and lp.stride(1) % 8 == 0 and lp.stride(1) >= npad and lp.stride(0) % 8 == 0
                and lp.data_ptr() % 16 == 0):
            lp = torch.zeros(B, P + 1, npad, dtype=BF, device=dev)
            lp[:, :, :nseg].copy_(logits)
        tp = teacher_logits.detach()
        if tp.stride(2) != 1:
            tp = tp.contiguous()
        bufs = {"dl": torch.empty(B, P + 1, npad, dtype=BF, device=dev)}
        loss, dl = hip.seg_distill(lp, tp, target.contiguous() if target is not None else None, hp, wp, H, W, nseg, seg_id_offset,
                                   weight, temperature, "all" if mask_all else "valid", bufs=bufs)
        return loss.clone(), bufs["kd_stats"], dl
    finally:
        hip.set_stream(prev)


@seg_distill.register_fake
def _(logits, teacher_logits, target, hp, wp, H, W, seg_id_offset, weight, temperature, mask_all):
    B, nseg, npad = _seg_distill_check(logits, teacher_logits, target, hp, wp, H, W, weight, temperature, mask_all)
    f32 = torch.float32
    return (logits.new_empty((), dtype=f32), logits.new_empty((2,), dtype=f32), logits.new_empty(B, hp * wp + 1, npad))


def _skd_backward(ctx, gloss, gstats, gdl):
    (dl,) = ctx.saved_tensors
    return (torch.ops.ifseg.seg_loss_bwd(gloss, dl, ctx.nseg),) + (None,) * 10


seg_distill.register_autograd(_skd_backward, setup_context=_sd_setup)


# ----------------------------------------------------------------------------------------------- seg_predict
def _seg_predict_check(scores, hp, wp, h, w):
    op = "ifseg::seg_predict"
    if scores.dtype != torch.float32:
        raise ValueError("%s: scores must be fp32 (hip.rows_to_f32 / hip.neighbour_smoothing give it), got dtype %s" % (op, scores.dtype))
    if scores.dim() != 3:
        raise ValueError("%s: scores must be [B, hp*wp, n], got %s" % (op, tuple(scores.shape)))
    B, P, n = scores.shape
    if B == 0:
        raise ValueError("%s: empty batch" % op)
    if hp <= 0 or wp <= 0 or P != hp * wp:
        raise ValueError("%s: scores.shape[1] = %d, expected hp * wp = %d" % (op, P, hp * wp))
    if n < 1 or n > SEG_LOSS_MAX_CLASSES:
        raise ValueError("%s: n = %d classes, the kernel takes 1 .. FUSED_MAX_CLASSES = %d" % (op, n, SEG_LOSS_MAX_CLASSES))
    if h < 1 or w < 1 or B * h * w >= 2 ** 31:
        raise ValueError("%s: the label map [%d, %d, %d] must have 1 <= h, w and B * h * w < 2**31" % (op, B, h, w))
    return B, n, (torch.uint8 if n <= 256 else torch.int16)


@custom_op("ifseg::seg_predict", mutates_args=(), device_types="cuda")
def seg_predict(scores: torch.Tensor, hp: int, wp: int, h: int, w: int, want_conf: bool, want_probs: bool
                ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """label map at h x w from per-patch class scores fp32 [B, hp*wp, n] (csrc/predict.hip): bilinear resize
    (align_corners=False, any ratio), argmax with torch.argmax's tie rule, in one pass.
    -> (labels [B, h, w] uint8 (n <= 256) or int16, conf fp32 [B, h, w] = the winning value, probs fp32 [B, n, h, w] = every
    interpolated value); an output that was not asked for is an empty tensor.  Not differentiable."""
    _seg_predict_check(scores, hp, wp, h, w)
    prev = _stream_scope(scores)
    try:
        labels, conf, probs = hip.seg_predict(scores.contiguous(), hp, wp, h, w, conf=want_conf, probs=want_probs)
        e = lambda t: torch.empty(0, dtype=torch.float32, device=scores.device) if t is None else t
        return labels, e(conf), e(probs)
    finally:
        hip.set_stream(prev)


@seg_predict.register_fake
def _(scores, hp, wp, h, w, want_conf, want_probs):
    B, n, ldt = _seg_predict_check(scores, hp, wp, h, w)
    f32 = torch.float32
    return (scores.new_empty(B, h, w, dtype=ldt), scores.new_empty((B, h, w) if want_conf else (0,), dtype=f32),
            scores.new_empty((B, n, h, w) if want_probs else (0,), dtype=f32))


# ----------------------------------------------------------------------------------------------- seg_predict_views
def _seg_predict_views_check(scores, hps, wps, flips, h, w):
    op = "ifseg::seg_predict_views"
    K = len(scores)
    if K < 1 or K > hip.SEG_PREDICT_MAX_VIEWS:
        raise ValueError("%s: %d views, the kernel takes 1 .. %d" % (op, K, hip.SEG_PREDICT_MAX_VIEWS))
    if len(hps) != K or len(wps) != K or len(flips) != K:
        raise ValueError("%s: %d views with %d hps, %d wps and %d flips (one of each per view)" % (op, K, len(hps), len(wps), len(flips)))
    for k, (s, hp, wp) in enumerate(zip(scores, hps, wps)):
        if s.dtype != torch.float32:
            raise ValueError("%s: scores must be fp32 (hip.rows_to_f32 / hip.neighbour_smoothing give it), view %d has dtype %s" % (op, k, s.dtype))
        if s.dim() != 3:
            raise ValueError("%s: scores must be [B, hp*wp, n], view %d is %s" % (op, k, tuple(s.shape)))
        if s.shape[0] != scores[0].shape[0] or s.shape[2] != scores[0].shape[2]:
            raise ValueError("%s: all views share B and n, view %d is %s against %s" % (op, k, tuple(s.shape), tuple(scores[0].shape)))
        if hp <= 0 or wp <= 0 or s.shape[1] != hp * wp:
            raise ValueError("%s: view %d: scores.shape[1] = %d, expected hp * wp = %d" % (op, k, s.shape[1], hp * wp))
    B, _, n = scores[0].shape
    if B == 0:
        raise ValueError("%s: empty batch" % op)
    if n < 1 or n > SEG_LOSS_MAX_CLASSES:
        raise ValueError("%s: n = %d classes, the kernel takes 1 .. FUSED_MAX_CLASSES = %d" % (op, n, SEG_LOSS_MAX_CLASSES))
    if h < 1 or w < 1 or B * h * w >= 2 ** 31:
        raise ValueError("%s: the label map [%d, %d, %d] must have 1 <= h, w and B * h * w < 2**31" % (op, B, h, w))
    return B, n, (torch.uint8 if n <= 256 else torch.int16)


@custom_op("ifseg::seg_predict_views", mutates_args=(), device_types="cuda")
def seg_predict_views(scores: Sequence[torch.Tensor], hps: Sequence[int], wps: Sequence[int], flips: Sequence[bool], h: int, w: int,
                      want_conf: bool, want_probs: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """label map at h x w from K views of the same images (csrc/predict.hip): view k is fp32 [B, hps[k]*wps[k], n], mirrored
    along the width when flips[k]; every view is resized as `seg_predict` does, the mean over the views (fp32, in view order)
    is what labels, conf and probs are taken from, in one launch.  Outputs and conventions as `seg_predict`.  Not differentiable."""
    _seg_predict_views_check(scores, hps, wps, flips, h, w)
    prev = _stream_scope(scores[0])
    try:
        views = [(s.contiguous(), hp, wp, bool(f)) for s, hp, wp, f in zip(scores, hps, wps, flips)]
        labels, conf, probs = hip.seg_predict_views(views, h, w, conf=want_conf, probs=want_probs)
        e = lambda t: torch.empty(0, dtype=torch.float32, device=scores[0].device) if t is None else t
        return labels, e(conf), e(probs)
    finally:
        hip.set_stream(prev)


@seg_predict_views.register_fake
def _(scores, hps, wps, flips, h, w, want_conf, want_probs):
    B, n, ldt = _seg_predict_views_check(scores, hps, wps, flips, h, w)
    f32, s = torch.float32, scores[0]
    return (s.new_empty(B, h, w, dtype=ldt), s.new_empty((B, h, w) if want_conf else (0,), dtype=f32),
            s.new_empty((B, n, h, w) if want_probs else (0,), dtype=f32))


# ----------------------------------------------------------------------------------------------- seg_areas
def _gt_check(op, gt):
    if gt.dtype not in (torch.uint8, torch.int16):
        raise ValueError("%s: ground truth must be uint8 or int16 (label PNG values or class ids), got dtype %s" % (op, gt.dtype))


def _maps_check(op, labels, conf=None, gt=None):
    """a predicted label map and what lies beside it, its confidences and / or its ground truth: one shape, 1 .. 2**31 - 1 pixels"""
    if labels.dtype not in (torch.uint8, torch.int16):
        raise ValueError("%s: labels must be uint8 or int16 (what seg_predict gives), got dtype %s" % (op, labels.dtype))
    if conf is not None and (conf.dtype != torch.float32 or conf.shape != labels.shape):
        raise ValueError("%s: conf must be float32 of the labels' shape %s, got %s %s"
                         % (op, tuple(labels.shape), conf.dtype, tuple(conf.shape)))
    if gt is not None:
        _gt_check(op, gt)
        if labels.shape != gt.shape:
            raise ValueError("%s: labels %s and ground truth %s must have one shape" % (op, tuple(labels.shape), tuple(gt.shape)))
    if labels.numel() < 1 or labels.numel() >= 2 ** 31:
        raise ValueError("%s: 1 <= pixels < 2**31, got %s" % (op, tuple(labels.shape)))


def _seg_areas_check(labels, gt, n, op="ifseg::seg_areas"):
    _maps_check(op, labels, gt=gt)
    if n < 1 or n > SEG_LOSS_MAX_CLASSES:
        raise ValueError("%s: n = %d classes, the kernel takes 1 .. FUSED_MAX_CLASSES = %d" % (op, n, SEG_LOSS_MAX_CLASSES))


@custom_op("ifseg::seg_areas", mutates_args=(), device_types="cuda")
def seg_areas(labels: torch.Tensor, gt: torch.Tensor, n: int, raw_labels: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """predicted labels (uint8 / int16) against ground truth (uint8 / int16) of the same shape (csrc/predict.hip) ->
    (areas int64 [3, n] = per class intersect / predicted / label pixel counts over the scored pixels, tally int64 [2] = scored
    pixels, pixels with a ground truth out of range), fresh tensors; `ifseg_amd.predict.areas_reference` is the specification.
    Integer inputs: not differentiable."""
    _seg_areas_check(labels, gt, n)
    prev = _stream_scope(labels)
    try:
        return hip.seg_areas(labels.contiguous(), gt.contiguous(), n, raw_labels)
    finally:
        hip.set_stream(prev)


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
    prev = _stream_scope(labels)
    try:
        return hip.seg_confusion(labels.contiguous(), gt.contiguous(), n, raw_labels)
    finally:
        hip.set_stream(prev)


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
    prev = _stream_scope(labels)
    try:
        return hip.seg_boundary_areas(labels.contiguous(), gt.contiguous(), n, d, raw_labels, band=True)
    finally:
        hip.set_stream(prev)


@seg_boundary_areas.register_fake
def _(labels, gt, n, d, raw_labels):
    _seg_boundary_check(labels, gt, n, d)
    return labels.new_empty((3, n), dtype=torch.int64), labels.new_empty(labels.shape, dtype=torch.uint8)


# ----------------------------------------------------------------------------------------------- seg_score_views
def _seg_score_views_check(scores, hps, wps, flips, gt):
    op = "ifseg::seg_score_views"
    _gt_check(op, gt)
    if gt.dim() != 3:
        raise ValueError("%s: ground truth must be [B, h, w], got %s" % (op, tuple(gt.shape)))
    B, n, ldt = _seg_predict_views_check(scores, hps, wps, flips, gt.shape[1], gt.shape[2])
    if gt.shape[0] != B:
        raise ValueError("%s: ground truth %s for a batch of %d" % (op, tuple(gt.shape), B))
    return B, n, ldt


@custom_op("ifseg::seg_score_views", mutates_args=(), device_types="cuda")
def seg_score_views(scores: Sequence[torch.Tensor], hps: Sequence[int], wps: Sequence[int], flips: Sequence[bool], gt: torch.Tensor,
                    raw_labels: bool, want_labels: bool, want_conf: bool, want_probs: bool
                    ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """`seg_predict_views` at the shape of the ground truth gt (uint8 / int16 [B, h, w]) with the label map counted against it
    in the kernel's epilogue (a single view is K = 1) -> (areas, tally, labels, conf, probs): the counters of `seg_areas`,
    fresh, and the outputs of `seg_predict_views`, each an empty tensor when it was not asked for.  Not differentiable."""
    _seg_score_views_check(scores, hps, wps, flips, gt)
    prev = _stream_scope(scores[0])
    try:
        views = [(s.contiguous(), hp, wp, bool(f)) for s, hp, wp, f in zip(scores, hps, wps, flips)]
        areas, tally, labels, conf, probs = hip.seg_score_views(views, gt.contiguous(), raw_labels, labels=want_labels,
                                                                conf=want_conf, probs=want_probs)
        e = lambda t, dt: torch.empty(0, dtype=dt, device=gt.device) if t is None else t
        ldt = torch.uint8 if scores[0].shape[2] <= 256 else torch.int16
        return areas, tally, e(labels, ldt), e(conf, torch.float32), e(probs, torch.float32)
    finally:
        hip.set_stream(prev)


@seg_score_views.register_fake
def _(scores, hps, wps, flips, gt, raw_labels, want_labels, want_conf, want_probs):
    B, n, ldt = _seg_score_views_check(scores, hps, wps, flips, gt)
    f32, s, (h, w) = torch.float32, scores[0], gt.shape[1:]
    return (s.new_empty((3, n), dtype=torch.int64), s.new_empty((2,), dtype=torch.int64),
            s.new_empty((B, h, w) if want_labels else (0,), dtype=ldt), s.new_empty((B, h, w) if want_conf else (0,), dtype=f32),
            s.new_empty((B, n, h, w) if want_probs else (0,), dtype=f32))


# ----------------------------------------------------------------------------------------------- seg_render
def _seg_render_check(labels, image, palette, opacity, boundary, boundary_color, conf):
    op = "ifseg::seg_render"
    if labels.dtype not in (torch.uint8, torch.int16):
        raise ValueError("%s: labels must be uint8 or int16 (what seg_predict gives), got dtype %s" % (op, labels.dtype))
    if labels.dim() not in (2, 3) or labels.numel() < 1 or labels.numel() >= 2 ** 31:
        raise ValueError("%s: labels must be [H, W] or [B, H, W] with 1 <= pixels < 2**31, got %s" % (op, tuple(labels.shape)))
    if image.dtype != torch.uint8 or tuple(image.shape) != tuple(labels.shape) + (3,):
        raise ValueError("%s: the image must be uint8 %s (HWC, the labels' shape), got %s %s"
                         % (op, tuple(labels.shape) + (3,), image.dtype, tuple(image.shape)))
    if palette.dtype != torch.uint8 or palette.dim() != 2 or palette.shape[1] != 3 or not 1 <= palette.shape[0] <= hip.SEG_PREDICT_MAX_CLASSES:
        raise ValueError("%s: the palette must be uint8 [n, 3], 1 <= n <= %d, got %s %s"
                         % (op, hip.SEG_PREDICT_MAX_CLASSES, palette.dtype, tuple(palette.shape)))
    if not 0.0 <= opacity <= 1.0:
        raise ValueError("%s: opacity must be in [0, 1], got %r" % (op, opacity))
    if not 0 <= boundary <= hip.SEG_RENDER_MAX_BOUNDARY:
        raise ValueError("%s: boundary must be in 0 .. %d, got %d" % (op, hip.SEG_RENDER_MAX_BOUNDARY, boundary))
    if len(boundary_color) != 3 or any(not 0 <= c <= 255 for c in boundary_color):
        raise ValueError("%s: boundary_color must be three ints in 0 .. 255, got %s" % (op, list(boundary_color)))
    if conf is not None and (conf.dtype != torch.float32 or conf.shape != labels.shape):
        raise ValueError("%s: conf must be float32 of the labels' shape %s, got %s %s"
                         % (op, tuple(labels.shape), conf.dtype, tuple(conf.shape)))


@custom_op("ifseg::seg_render", mutates_args=(), device_types="cuda")
def seg_render(labels: torch.Tensor, image: torch.Tensor, palette: torch.Tensor, opacity: float, boundary: int,
               boundary_color: Sequence[int], conf: Optional[torch.Tensor]) -> torch.Tensor:
    """the label map as a picture (csrc/render.hip): labels uint8 / int16 [.., H, W] coloured by palette uint8 [n, 3] over image
    uint8 [.., H, W, 3] at `opacity` (scaled per pixel by conf fp32 [.., H, W] when given), contours of half width `boundary`
    in `boundary_color` -> uint8 [.., H, W, 3], a fresh tensor; `ifseg_amd.predict.render_reference` is the specification.
    Integer inputs: not differentiable."""
    _seg_render_check(labels, image, palette, opacity, boundary, boundary_color, conf)
    prev = _stream_scope(labels)
    try:
        return hip.seg_render(labels.contiguous(), image.contiguous(), palette.contiguous(), opacity, boundary,
                              tuple(int(c) for c in boundary_color), conf=None if conf is None else conf.contiguous())
    finally:
        hip.set_stream(prev)


@seg_render.register_fake
def _(labels, image, palette, opacity, boundary, boundary_color, conf):
    _seg_render_check(labels, image, palette, opacity, boundary, boundary_color, conf)
    return image.new_empty(tuple(labels.shape) + (3,), dtype=torch.uint8)


# ----------------------------------------------------------------------------------------------- seg_conf_hist, seg_pseudo
@custom_op("ifseg::seg_conf_hist", mutates_args=(), device_types="cuda")
def seg_conf_hist(labels: torch.Tensor, conf: torch.Tensor, n: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """predicted labels (uint8 / int16) with their confidences (fp32, the same shape) (csrc/pseudo.hip) -> (hist int64 [n, 256] =
    pixels per (label, clamp(floor(conf * 256), 0, 255)), tally int64 [2] = labels inside / outside [0, n)), fresh tensors;
    `ifseg_amd.predict.confidence_histogram_reference` is the specification.  Counts: not differentiable."""
    _maps_check("ifseg::seg_conf_hist", labels, conf)
    if n < 1 or n > hip.SEG_PREDICT_MAX_CLASSES:
        raise ValueError("ifseg::seg_conf_hist: n = %d classes, the kernel takes 1 .. %d" % (n, hip.SEG_PREDICT_MAX_CLASSES))
    prev = _stream_scope(labels)
    try:
        return hip.seg_conf_hist(labels.contiguous(), conf.contiguous(), n)
    finally:
        hip.set_stream(prev)


@seg_conf_hist.register_fake
def _(labels, conf, n):
    _maps_check("ifseg::seg_conf_hist", labels, conf)
    if n < 1 or n > hip.SEG_PREDICT_MAX_CLASSES:
        raise ValueError("ifseg::seg_conf_hist: n = %d classes, the kernel takes 1 .. %d" % (n, hip.SEG_PREDICT_MAX_CLASSES))
    return labels.new_empty((n, hip.SEG_CONF_BINS), dtype=torch.int64), labels.new_empty((2,), dtype=torch.int64)


def _seg_calibration_check(labels, conf, gt, n):
    op = "ifseg::seg_calibration"
    _maps_check(op, labels, conf, gt)
    if n < 1 or n > hip.SEG_PREDICT_MAX_CLASSES:
        raise ValueError("%s: n = %d classes, the kernel takes 1 .. %d" % (op, n, hip.SEG_PREDICT_MAX_CLASSES))


@custom_op("ifseg::seg_calibration", mutates_args=(), device_types="cuda")
def seg_calibration(labels: torch.Tensor, conf: torch.Tensor, gt: torch.Tensor, n: int,
                    raw_labels: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """predicted labels (uint8 / int16) with their confidences (fp32) against ground truth (uint8 / int16), one shape
    (csrc/calib.hip) -> (calibration int64 [n, 256, 2] = over `seg_areas`' scored pixels, pixels per (label in [0, n),
    clamp(floor(conf * 256), 0, 255), label == gt class), tally int64 [2] = scored pixels with a label inside / outside [0, n)),
    fresh tensors; `ifseg_amd.predict.calibration_reference` is the specification.  Counts: not differentiable."""
    _seg_calibration_check(labels, conf, gt, n)
    prev = _stream_scope(labels)
    try:
        return hip.seg_calibration(labels.contiguous(), conf.contiguous(), gt.contiguous(), n, raw_labels)
    finally:
        hip.set_stream(prev)


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
    if n < 1 or n > hip.SEG_PREDICT_MAX_CLASSES:
        raise ValueError("%s: n = %d classes, the kernel takes 1 .. %d" % (op, n, hip.SEG_PREDICT_MAX_CLASSES))
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
    prev = _stream_scope(grids)
    try:
        return hip.seg_temperature_sweep(grids.contiguous(), hp, wp, gt.contiguous(), raw_labels)
    finally:
        hip.set_stream(prev)


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
    if not 0 <= boundary <= hip.SEG_RENDER_MAX_BOUNDARY:
        raise ValueError("%s: boundary must be in 0 .. %d, got %d" % (op, hip.SEG_RENDER_MAX_BOUNDARY, boundary))


@custom_op("ifseg::seg_pseudo", mutates_args=(), device_types="cuda")
def seg_pseudo(labels: torch.Tensor, conf: torch.Tensor, thresholds: torch.Tensor, n: int, boundary: int,
               raw_labels: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """the confidence filter of self-training (csrc/pseudo.hip): labels uint8 / int16 [.., H, W], conf fp32 of that shape,
    thresholds int32 [n] in bins -> (the pseudo-label map uint8 [.., H, W]: class + 1 with raw_labels, else class, 255 where
    the pixel is not kept; kept int64 [2, n]: kept and predicted pixels per class), fresh tensors;
    `ifseg_amd.predict.pseudo_label_reference` is the specification.  Integer outputs: not differentiable."""
    _seg_pseudo_check(labels, conf, thresholds, n, boundary, raw_labels)
    prev = _stream_scope(labels)
    try:
        return hip.seg_pseudo(labels.contiguous(), conf.contiguous(), thresholds.contiguous(), n, boundary, raw_labels)
    finally:
        hip.set_stream(prev)


@seg_pseudo.register_fake
def _(labels, conf, thresholds, n, boundary, raw_labels):
    _seg_pseudo_check(labels, conf, thresholds, n, boundary, raw_labels)
    return labels.new_empty(tuple(labels.shape), dtype=torch.uint8), labels.new_empty((2, n), dtype=torch.int64)


# ----------------------------------------------------------------------------------------------- seg_regions, seg_region_drop
def _seg_regions_check(labels, connectivity, op="ifseg::seg_regions", dtypes=(torch.uint8, torch.int16)):
    if labels.dtype not in dtypes:
        raise ValueError("%s: labels must be %s, got dtype %s" % (op, " or ".join(str(d).replace("torch.", "") for d in dtypes),
                                                                 labels.dtype))
    if labels.dim() not in (2, 3) or labels.numel() < 1 or labels.numel() >= 2 ** 31:
        raise ValueError("%s: labels must be [H, W] or [B, H, W] with 1 <= pixels < 2**31, got %s" % (op, tuple(labels.shape)))
    if connectivity not in (4, 8):
        raise ValueError("%s: connectivity must be 4 or 8, got %d" % (op, connectivity))


@custom_op("ifseg::seg_regions", mutates_args=(), device_types="cuda")
def seg_regions(labels: torch.Tensor, connectivity: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """the connected regions of equal values of a label map uint8 / int16 [.., H, W] (csrc/regions.hip) -> (root int32 = per
    pixel the smallest y W + x of its region inside its image, size int32 = the region's pixel count), fresh tensors of the
    labels' shape; `ifseg_amd.predict.regions_reference` is the specification.  Integer outputs: not differentiable."""
    _seg_regions_check(labels, connectivity)
    prev = _stream_scope(labels)
    try:
        return hip.seg_regions(labels.contiguous(), connectivity)
    finally:
        hip.set_stream(prev)


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
    prev = _stream_scope(labels)
    try:
        return hip.seg_region_drop(labels.contiguous(), connectivity, min_region, fill, n, raw_labels)
    finally:
        hip.set_stream(prev)


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
    if n < 1 or n > hip.SEG_PREDICT_MAX_CLASSES:
        raise ValueError("%s: n = %d classes, the kernel takes 1 .. %d" % (op, n, hip.SEG_PREDICT_MAX_CLASSES))
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
    return n, H, W, (torch.uint8 if n <= 256 else torch.int16)


@custom_op("ifseg::seg_pamr", mutates_args=(), device_types="cuda")
def seg_pamr(probs: torch.Tensor, image: torch.Tensor, iters: int, dilations: Sequence[int], want_conf: bool, want_probs: bool
             ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """pixel-adaptive mask refinement of one image (csrc/pamr.hip): probs fp32 [n, H, W], image uint8 [H, W, 3] -> (labels [H, W]
    uint8 (n <= 256) or int16, conf fp32 [H, W], the refined values fp32 [n, H, W]), fresh tensors; an output that was not asked
    for is an empty tensor.  `ifseg_amd.predict.pamr_reference` is the specification.  No autograd."""
    _seg_pamr_check(probs, image, iters, dilations)
    prev = _stream_scope(probs)
    try:
        labels, conf, out = hip.seg_pamr(probs.contiguous(), image.contiguous(), iters, tuple(int(d) for d in dilations),
                                         conf=want_conf, probs_out=want_probs)
        e = lambda t: torch.empty(0, dtype=torch.float32, device=probs.device) if t is None else t
        return labels, e(conf), e(out)
    finally:
        hip.set_stream(prev)


@seg_pamr.register_fake
def _(probs, image, iters, dilations, want_conf, want_probs):
    n, H, W, ldt = _seg_pamr_check(probs, image, iters, dilations)
    f32 = torch.float32
    return (probs.new_empty((H, W), dtype=ldt), probs.new_empty((H, W) if want_conf else (0,), dtype=f32),
            probs.new_empty((n, H, W) if want_probs else (0,), dtype=f32))


# ----------------------------------------------------------------------------------------------- image_load
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
    if len(mean) != 3 or len(std) != 3:
        raise ValueError("%s: mean and std must have three entries, got %d and %d" % (op, len(mean), len(std)))
    if dtype not in (torch.float32, BF):
        raise ValueError("%s: the output dtype must be torch.float32 or torch.bfloat16, got %s" % (op, dtype))
    return B


@custom_op("ifseg::image_load", mutates_args=(), device_types="cuda")
def image_load(images: torch.Tensor, oh: int, ow: int, mean: Sequence[float], std: Sequence[float], reverse_channels: bool,
               dtype: torch.dtype) -> torch.Tensor:
    """the reference's evaluation transform (csrc/imgload.hip): uint8 [B, H0, W0, 3] -> patch_images [B, 3, oh, ow] in `dtype`
    (fp32 / bf16) by bilinear resize (align_corners=False), rounding to a grey level, optional channel reversal and
    (x / 255 - mean) / std.  The input is integer: not differentiable."""
    _image_load_check(images, oh, ow, mean, std, dtype)
    prev = _stream_scope(images)
    try:
        return hip.image_load(images.contiguous(), oh, ow, mean, std, reverse_channels, dtype)
    finally:
        hip.set_stream(prev)


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
    if scores.dtype != torch.float32:
        raise ValueError("%s: scores must be fp32 (hip.rows_to_f32 / hip.neighbour_smoothing give it), got dtype %s" % (op, scores.dtype))
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
    if n < 1 or n > SEG_LOSS_MAX_CLASSES:
        raise ValueError("%s: n = %d classes, the kernel takes 1 .. FUSED_MAX_CLASSES = %d" % (op, n, SEG_LOSS_MAX_CLASSES))
    if h < 1 or w < 1 or B * h * w >= 2 ** 31:
        raise ValueError("%s: the label map [%d, %d, %d] must have 1 <= h, w and B * h * w < 2**31" % (op, B, h, w))
    return B, n, (torch.uint8 if n <= 256 else torch.int16)


@custom_op("ifseg::seg_predict_windows", mutates_args=(), device_types="cuda")
def seg_predict_windows(scores: torch.Tensor, hpw: int, wpw: int, oh: int, ow: int, crop: Sequence[int], stride: Sequence[int],
                        h: int, w: int, want_conf: bool, want_probs: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """label map at h x w from the windows of sliding-window inference (csrc/predict.hip): scores fp32 [B, Nw, hpw*wpw, n],
    window k of `imageio.slide_windows(oh, ow, crop, stride)`; the windows are resized, averaged where they overlap and the
    result resized to h x w in one launch.  Outputs and conventions as `seg_predict`.  Not differentiable."""
    _seg_predict_windows_check(scores, hpw, wpw, oh, ow, crop, stride, h, w)
    prev = _stream_scope(scores)
    try:
        labels, conf, probs = hip.seg_predict_windows(scores.contiguous(), hpw, wpw, oh, ow, tuple(crop), tuple(stride), h, w,
                                                      conf=want_conf, probs=want_probs)
        e = lambda t: torch.empty(0, dtype=torch.float32, device=scores.device) if t is None else t
        return labels, e(conf), e(probs)
    finally:
        hip.set_stream(prev)


@seg_predict_windows.register_fake
def _(scores, hpw, wpw, oh, ow, crop, stride, h, w, want_conf, want_probs):
    B, n, ldt = _seg_predict_windows_check(scores, hpw, wpw, oh, ow, crop, stride, h, w)
    f32 = torch.float32
    return (scores.new_empty(B, h, w, dtype=ldt), scores.new_empty((B, h, w) if want_conf else (0,), dtype=f32),
            scores.new_empty((B, n, h, w) if want_probs else (0,), dtype=f32))


def _seg_score_windows_check(scores, hpw, wpw, oh, ow, crop, stride, gt):
    op = "ifseg::seg_score_windows"
    _gt_check(op, gt)
    if gt.dim() != 3:
        raise ValueError("%s: ground truth must be [B, h, w], got %s" % (op, tuple(gt.shape)))
    B, n, ldt = _seg_predict_windows_check(scores, hpw, wpw, oh, ow, crop, stride, gt.shape[1], gt.shape[2], op)
    if gt.shape[0] != B:
        raise ValueError("%s: ground truth %s for a batch of %d" % (op, tuple(gt.shape), B))
    return B, n, ldt


@custom_op("ifseg::seg_score_windows", mutates_args=(), device_types="cuda")
def seg_score_windows(scores: torch.Tensor, hpw: int, wpw: int, oh: int, ow: int, crop: Sequence[int], stride: Sequence[int],
                      gt: torch.Tensor, raw_labels: bool, want_labels: bool, want_conf: bool, want_probs: bool
                      ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """`seg_predict_windows` at the shape of the ground truth gt (uint8 / int16 [B, h, w]) with the label map counted against
    it in the kernel's epilogue -> (areas, tally, labels, conf, probs) as `seg_score_views`.  Not differentiable."""
    _seg_score_windows_check(scores, hpw, wpw, oh, ow, crop, stride, gt)
    prev = _stream_scope(scores)
    try:
        areas, tally, labels, conf, probs = hip.seg_score_windows(scores.contiguous(), hpw, wpw, oh, ow, tuple(crop), tuple(stride),
                                                                  gt.contiguous(), raw_labels, labels=want_labels, conf=want_conf,
                                                                  probs=want_probs)
        e = lambda t, dt: torch.empty(0, dtype=dt, device=gt.device) if t is None else t
        ldt = torch.uint8 if scores.shape[3] <= 256 else torch.int16
        return areas, tally, e(labels, ldt), e(conf, torch.float32), e(probs, torch.float32)
    finally:
        hip.set_stream(prev)


@seg_score_windows.register_fake
def _(scores, hpw, wpw, oh, ow, crop, stride, gt, raw_labels, want_labels, want_conf, want_probs):
    B, n, ldt = _seg_score_windows_check(scores, hpw, wpw, oh, ow, crop, stride, gt)
    f32, s, (h, w) = torch.float32, scores, gt.shape[1:]
    return (s.new_empty((3, n), dtype=torch.int64), s.new_empty((2,), dtype=torch.int64),
            s.new_empty((B, h, w) if want_labels else (0,), dtype=ldt), s.new_empty((B, h, w) if want_conf else (0,), dtype=f32),
            s.new_empty((B, n, h, w) if want_probs else (0,), dtype=f32))


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
    prev = _stream_scope(images)
    try:
        return hip.image_load_windows(images.contiguous(), oh, ow, tuple(crop), tuple(stride), mean, std, reverse_channels, dtype)
    finally:
        hip.set_stream(prev)


@image_load_windows.register_fake
def _(images, oh, ow, crop, stride, mean, std, reverse_channels, dtype):
    nb, ch, cw = _image_load_windows_check(images, oh, ow, crop, stride, mean, std, dtype)
    return images.new_empty((nb, 3, ch, cw), dtype=dtype)


# ----------------------------------------------------------------------------------------------- views of sliding windows
def _seg_predict_slide_views_check(scores, hpws, wpws, ohs, ows, flips, crop, stride, h, w, op="ifseg::seg_predict_slide_views"):
    K = len(scores)
    if K < 1 or K > hip.SEG_PREDICT_MAX_VIEWS:
        raise ValueError("%s: %d views, the kernel takes 1 .. %d" % (op, K, hip.SEG_PREDICT_MAX_VIEWS))
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
    prev = _stream_scope(scores[0])
    try:
        labels, conf, probs = hip.seg_predict_slide_views(_slide_views_list(scores, hpws, wpws, ohs, ows, flips), tuple(crop),
                                                          tuple(stride), h, w, softmax, conf=want_conf, probs=want_probs)
        e = lambda t: torch.empty(0, dtype=torch.float32, device=scores[0].device) if t is None else t
        return labels, e(conf), e(probs)
    finally:
        hip.set_stream(prev)


@seg_predict_slide_views.register_fake
def _(scores, hpws, wpws, ohs, ows, flips, crop, stride, h, w, softmax, want_conf, want_probs):
    B, n, ldt = _seg_predict_slide_views_check(scores, hpws, wpws, ohs, ows, flips, crop, stride, h, w)
    f32, s = torch.float32, scores[0]
    return (s.new_empty(B, h, w, dtype=ldt), s.new_empty((B, h, w) if want_conf else (0,), dtype=f32),
            s.new_empty((B, n, h, w) if want_probs else (0,), dtype=f32))


def _seg_score_slide_views_check(scores, hpws, wpws, ohs, ows, flips, crop, stride, gt):
    op = "ifseg::seg_score_slide_views"
    _gt_check(op, gt)
    if gt.dim() != 3:
        raise ValueError("%s: ground truth must be [B, h, w], got %s" % (op, tuple(gt.shape)))
    B, n, ldt = _seg_predict_slide_views_check(scores, hpws, wpws, ohs, ows, flips, crop, stride, gt.shape[1], gt.shape[2], op)
    if gt.shape[0] != B:
        raise ValueError("%s: ground truth %s for a batch of %d" % (op, tuple(gt.shape), B))
    return B, n, ldt


@custom_op("ifseg::seg_score_slide_views", mutates_args=(), device_types="cuda")
def seg_score_slide_views(scores: Sequence[torch.Tensor], hpws: Sequence[int], wpws: Sequence[int], ohs: Sequence[int],
                          ows: Sequence[int], flips: Sequence[bool], crop: Sequence[int], stride: Sequence[int], gt: torch.Tensor,
                          softmax: bool, raw_labels: bool, want_labels: bool, want_conf: bool, want_probs: bool
                          ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """`seg_predict_slide_views` at the shape of the ground truth gt (uint8 / int16 [B, h, w]) with the label map counted
    against it in the kernel's epilogue -> (areas, tally, labels, conf, probs) as `seg_score_views`.  Not differentiable."""
    _seg_score_slide_views_check(scores, hpws, wpws, ohs, ows, flips, crop, stride, gt)
    prev = _stream_scope(scores[0])
    try:
        areas, tally, labels, conf, probs = hip.seg_score_slide_views(_slide_views_list(scores, hpws, wpws, ohs, ows, flips),
                                                                      tuple(crop), tuple(stride), gt.contiguous(), softmax,
                                                                      raw_labels, labels=want_labels, conf=want_conf,
                                                                      probs=want_probs)
        e = lambda t, dt: torch.empty(0, dtype=dt, device=gt.device) if t is None else t
        ldt = torch.uint8 if scores[0].shape[3] <= 256 else torch.int16
        return areas, tally, e(labels, ldt), e(conf, torch.float32), e(probs, torch.float32)
    finally:
        hip.set_stream(prev)


@seg_score_slide_views.register_fake
def _(scores, hpws, wpws, ohs, ows, flips, crop, stride, gt, softmax, raw_labels, want_labels, want_conf, want_probs):
    B, n, ldt = _seg_score_slide_views_check(scores, hpws, wpws, ohs, ows, flips, crop, stride, gt)
    f32, s, (h, w) = torch.float32, scores[0], gt.shape[1:]
    return (s.new_empty((3, n), dtype=torch.int64), s.new_empty((2,), dtype=torch.int64),
            s.new_empty((B, h, w) if want_labels else (0,), dtype=ldt), s.new_empty((B, h, w) if want_conf else (0,), dtype=f32),
            s.new_empty((B, n, h, w) if want_probs else (0,), dtype=f32))


# --------------------------------------------- the training input path (train_load, mix_*, strong_*): what its ops share
@contextlib.contextmanager
def _on_stream(where):
    """the kernels inside run on PyTorch's current stream of a tensor's device, or of the device itself"""
    prev = hip.set_stream(torch.cuda.current_stream(where.device if torch.is_tensor(where) else where).cuda_stream)
    try:
        yield
    finally:
        hip.set_stream(prev)


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
    if len(mean) != 3 or len(std) != 3:
        raise ValueError("%s: mean and std must have three entries, got %d and %d" % (op, len(mean), len(std)))
    if dtype not in (torch.float32, BF):
        raise ValueError("%s: the output dtype must be torch.float32 or torch.bfloat16, got %s" % (op, dtype))
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
        c = lambda t: None if t is None else t.contiguous()
        img, tgt, wgt = hip.mix_apply(records.contiguous(), c(src_images), c(src_target), c(dst_images), c(dst_target), nseg,
                                      seg_id_offset, src_weight=c(src_weight), dst_weight=c(dst_weight))
        return img, tgt, torch.empty(0, dtype=torch.uint8, device=records.device) if wgt is None else wgt


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
