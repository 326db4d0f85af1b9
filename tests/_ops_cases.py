"""What `ifseg_amd/ops.py` shows the dispatcher, as data (tests/test_ops_pins_cpu.py): every `ifseg::*` op's schema, one good call
per op on fake tensors at the smallest legal shapes with the (shape, dtype) of each output, and refusal probes -- a good call
with arguments made wrong, and the complete message it raises.  Recorded from the file as it stood before its checks, fakes and
stream scopes were folded: a fold may move a check, it may not reword it or let another check fire first.

A tensor of a recipe is `t(*shape, dtype)`: a description, made real by `real()` inside the test's FakeTensorMode."""
import collections

import torch

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
U8, I16, I32, I64 = torch.uint8, torch.int16, torch.int32, torch.int64

T = collections.namedtuple("T", "shape dtype")


def t(*shape, dtype=BF):
    return T(tuple(shape), dtype)


def real(x):
    """a recipe's value as an argument: every `T` becomes an empty tensor on "cuda", inside lists too"""
    if isinstance(x, T):
        return torch.empty(x.shape, dtype=x.dtype, device="cuda")
    if isinstance(x, list):
        return [real(v) for v in x]
    return x


SCHEMAS = {
    "attention_bias": "ifseg::attention_bias(Tensor q, Tensor k, Tensor v, Tensor? bias, Tensor? gain, Tensor? kv_len, bool causal, SymInt P, float dropout_p, SymInt seed) -> (Tensor, Tensor, Tensor)",
    "attention_bias_bwd": "ifseg::attention_bias_bwd(Tensor dout, Tensor q, Tensor k, Tensor v, Tensor? bias, Tensor? gain, Tensor? kv_len, Tensor out, Tensor lse, Tensor packed, bool causal, SymInt P, float dropout_p, SymInt seed) -> (Tensor, Tensor, Tensor, Tensor, Tensor)",
    "bias_attention": "ifseg::bias_attention(Tensor q, Tensor k, Tensor v, Tensor pos_q, Tensor pos_k, Tensor gain, Tensor? gcode, Tensor? rel2d, Tensor? rel1d, Tensor? relx, SymInt P, SymInt code_bias, SymInt grid_w, bool causal) -> (Tensor, Tensor)",
    "bias_attention_bi": "ifseg::bias_attention_bi(Tensor q, Tensor k, Tensor v, Tensor pos_q, Tensor pos_k, Tensor gain, Tensor? gcode, Tensor? rel2d, Tensor? rel1d, Tensor? relx, SymInt P, SymInt code_bias, SymInt grid_w, bool causal, Tensor? kv_len, float dropout_p, SymInt seed) -> (Tensor, Tensor, Tensor)",
    "bias_attention_bi_bwd": "ifseg::bias_attention_bi_bwd(Tensor dout, Tensor q, Tensor k, Tensor v, Tensor pos_q, Tensor pos_k, Tensor gain, Tensor out, Tensor lse, Tensor packed, Tensor? gcode, Tensor? rel2d, Tensor? rel1d, Tensor? relx, SymInt P, SymInt code_bias, SymInt grid_w, bool causal, Tensor? kv_len, float dropout_p, SymInt seed) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)",
    "bias_attention_bwd": "ifseg::bias_attention_bwd(Tensor dout, Tensor q, Tensor k, Tensor v, Tensor pos_q, Tensor pos_k, Tensor gain, Tensor out, Tensor lse, Tensor? gcode, Tensor? rel2d, Tensor? rel1d, Tensor? relx, SymInt P, SymInt code_bias, SymInt grid_w, bool causal) -> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)",
    "image_load": "ifseg::image_load(Tensor images, SymInt oh, SymInt ow, float[] mean, float[] std, bool reverse_channels, ScalarType dtype) -> Tensor",
    "image_load_windows": "ifseg::image_load_windows(Tensor images, SymInt oh, SymInt ow, SymInt[] crop, SymInt[] stride, float[] mean, float[] std, bool reverse_channels, ScalarType dtype) -> Tensor",
    "layer_norm": "ifseg::layer_norm(Tensor x, Tensor gamma, Tensor beta, float eps, bool gelu) -> (Tensor, Tensor, Tensor)",
    "layer_norm_bwd": "ifseg::layer_norm_bwd(Tensor dy, Tensor x, Tensor gamma, Tensor mean, Tensor rstd, bool gelu) -> (Tensor, Tensor, Tensor)",
    "linear": "ifseg::linear(Tensor x, Tensor w, Tensor? bias) -> Tensor",
    "linear_bwd": "ifseg::linear_bwd(Tensor g, Tensor x, Tensor w) -> (Tensor, Tensor, Tensor)",
    "mix_apply": "ifseg::mix_apply(Tensor records, Tensor src_images, Tensor src_target, Tensor? src_weight, Tensor dst_images, Tensor dst_target, Tensor? dst_weight, SymInt nseg, SymInt seg_id_offset) -> (Tensor, Tensor, Tensor)",
    "mix_draw": "ifseg::mix_draw(Tensor src_target, SymInt nseg, SymInt seg_id_offset, SymInt seed, SymInt first_ordinal, str mask) -> Tensor",
    "seg_areas": "ifseg::seg_areas(Tensor labels, Tensor gt, SymInt n, bool raw_labels) -> (Tensor, Tensor)",
    "seg_boundary_areas": "ifseg::seg_boundary_areas(Tensor labels, Tensor gt, SymInt n, SymInt d, bool raw_labels) -> (Tensor, Tensor)",
    "seg_calibration": "ifseg::seg_calibration(Tensor labels, Tensor conf, Tensor gt, SymInt n, bool raw_labels) -> (Tensor, Tensor)",
    "seg_conf_hist": "ifseg::seg_conf_hist(Tensor labels, Tensor conf, SymInt n) -> (Tensor, Tensor)",
    "seg_confusion": "ifseg::seg_confusion(Tensor labels, Tensor gt, SymInt n, bool raw_labels) -> Tensor",
    "seg_dice": "ifseg::seg_dice(Tensor logits, Tensor target, Tensor? class_weight, SymInt hp, SymInt wp, SymInt H, SymInt W, SymInt seg_id_offset, float dice_weight, float smooth) -> (Tensor, Tensor, Tensor)",
    "seg_distill": "ifseg::seg_distill(Tensor logits, Tensor teacher_logits, Tensor? target, SymInt hp, SymInt wp, SymInt H, SymInt W, SymInt seg_id_offset, float weight, float temperature, bool mask_all) -> (Tensor, Tensor, Tensor)",
    "seg_loss": "ifseg::seg_loss(Tensor logits, Tensor target, SymInt hp, SymInt wp, SymInt H, SymInt W, SymInt seg_id_offset, float label_smoothing) -> (Tensor, Tensor, Tensor, Tensor)",
    "seg_loss_bwd": "ifseg::seg_loss_bwd(Tensor grad_loss, Tensor dlogits, SymInt nseg) -> Tensor",
    "seg_loss_weighted": "ifseg::seg_loss_weighted(Tensor logits, Tensor target, Tensor? pixel_weight, Tensor? class_weight, SymInt hp, SymInt wp, SymInt H, SymInt W, SymInt seg_id_offset, float label_smoothing, bool norm_pixels) -> (Tensor, Tensor, Tensor, Tensor)",
    "seg_ohem": "ifseg::seg_ohem(Tensor logits, Tensor target, Tensor? pixel_weight, SymInt hp, SymInt wp, SymInt H, SymInt W, SymInt seg_id_offset, float thresh, SymInt min_kept) -> (Tensor, Tensor)",
    "seg_pamr": "ifseg::seg_pamr(Tensor probs, Tensor image, SymInt iters, SymInt[] dilations, bool want_conf, bool want_probs) -> (Tensor, Tensor, Tensor)",
    "seg_predict": "ifseg::seg_predict(Tensor scores, SymInt hp, SymInt wp, SymInt h, SymInt w, bool want_conf, bool want_probs) -> (Tensor, Tensor, Tensor)",
    "seg_predict_slide_views": "ifseg::seg_predict_slide_views(Tensor[] scores, SymInt[] hpws, SymInt[] wpws, SymInt[] ohs, SymInt[] ows, bool[] flips, SymInt[] crop, SymInt[] stride, SymInt h, SymInt w, bool softmax, bool want_conf, bool want_probs) -> (Tensor, Tensor, Tensor)",
    "seg_predict_views": "ifseg::seg_predict_views(Tensor[] scores, SymInt[] hps, SymInt[] wps, bool[] flips, SymInt h, SymInt w, bool want_conf, bool want_probs) -> (Tensor, Tensor, Tensor)",
    "seg_predict_windows": "ifseg::seg_predict_windows(Tensor scores, SymInt hpw, SymInt wpw, SymInt oh, SymInt ow, SymInt[] crop, SymInt[] stride, SymInt h, SymInt w, bool want_conf, bool want_probs) -> (Tensor, Tensor, Tensor)",
    "seg_pseudo": "ifseg::seg_pseudo(Tensor labels, Tensor conf, Tensor thresholds, SymInt n, SymInt boundary, bool raw_labels) -> (Tensor, Tensor)",
    "seg_region_drop": "ifseg::seg_region_drop(Tensor labels, SymInt connectivity, SymInt min_region, SymInt fill, SymInt n, bool raw_labels) -> (Tensor, Tensor, Tensor)",
    "seg_regions": "ifseg::seg_regions(Tensor labels, SymInt connectivity) -> (Tensor, Tensor)",
    "seg_render": "ifseg::seg_render(Tensor labels, Tensor image, Tensor palette, float opacity, SymInt boundary, SymInt[] boundary_color, Tensor? conf) -> Tensor",
    "seg_score_slide_views": "ifseg::seg_score_slide_views(Tensor[] scores, SymInt[] hpws, SymInt[] wpws, SymInt[] ohs, SymInt[] ows, bool[] flips, SymInt[] crop, SymInt[] stride, Tensor gt, bool softmax, bool raw_labels, bool want_labels, bool want_conf, bool want_probs) -> (Tensor, Tensor, Tensor, Tensor, Tensor)",
    "seg_score_views": "ifseg::seg_score_views(Tensor[] scores, SymInt[] hps, SymInt[] wps, bool[] flips, Tensor gt, bool raw_labels, bool want_labels, bool want_conf, bool want_probs) -> (Tensor, Tensor, Tensor, Tensor, Tensor)",
    "seg_score_windows": "ifseg::seg_score_windows(Tensor scores, SymInt hpw, SymInt wpw, SymInt oh, SymInt ow, SymInt[] crop, SymInt[] stride, Tensor gt, bool raw_labels, bool want_labels, bool want_conf, bool want_probs) -> (Tensor, Tensor, Tensor, Tensor, Tensor)",
    "seg_temperature_sweep": "ifseg::seg_temperature_sweep(Tensor grids, SymInt hp, SymInt wp, Tensor gt, bool raw_labels) -> (Tensor, Tensor, Tensor)",
    "strong_apply": "ifseg::strong_apply(Tensor records, Tensor images, float[] mean, float[] std, bool reverse_channels) -> Tensor",
    "strong_draw": "ifseg::strong_draw(SymInt B, SymInt seed, SymInt first_ordinal, SymInt jitter_p8, SymInt blur_p8, Device device) -> Tensor",
    "train_load": "ifseg::train_load(Tensor[] images, Tensor[] labels, Tensor params, SymInt P, SymInt nseg, SymInt seg_id_offset, float[] mean, float[] std, bool reverse_channels, bool raw_labels, ScalarType dtype) -> (Tensor, Tensor)",
}

# ---------------------------------------------------------------------------------------------------------------- good calls
# op -> (arguments by the schema's names, [(shape, dtype) of each output])
_QKV = dict(q=t(1, 32, 64), k=t(1, 32, 64), v=t(1, 32, 64))
_POS = dict(pos_q=t(32, 64), pos_k=t(32, 64), gain=t(1, dtype=F32))
_NO_REL = dict(gcode=None, rel2d=None, rel1d=None, relx=None)
_REL_META = dict(P=0, code_bias=0, grid_w=0, causal=False)
_OUT_LSE = dict(out=t(1, 32, 64), lse=t(1, 1, 32, dtype=F32))
_DQKV = [((1, 32, 64), BF)] * 3
_NINE = _DQKV + [((32, 64), BF), ((32, 64), BF), ((1,), F32), ((0,), F32), ((0,), F32), ((0,), F32)]
# B 1, hp = wp = 1, nseg 3, H = W = 16
_LOGITS = dict(logits=t(1, 2, 3), target=t(1, 257, dtype=I64))
_GRID16 = dict(hp=1, wp=1, H=16, W=16, seg_id_offset=1000)
_LOSS4 = [((), F32), ((11,), F32), ((1, 2, 8), BF), ((1,), I32)]
# B 1, a 2 x 2 grid, n 3, 8 x 8 out
_SCORES = t(1, 4, 3, dtype=F32)
_VIEWS = dict(scores=[_SCORES], hps=[2], wps=[2], flips=[False])
_MAP, _CONF = t(1, 8, 8, dtype=U8), t(1, 8, 8, dtype=F32)
_AREAS = [((3, 3), I64), ((2,), I64)]
_TRIPLE = [((1, 8, 8), U8), ((1, 8, 8), F32), ((1, 3, 8, 8), F32)]
# two 16 x 16 windows of a 16 x 32 plane, a 2 x 2 grid each
_WIN_SCORES = t(1, 2, 4, 3, dtype=F32)
_WINDOWS = dict(crop=[16, 16], stride=[16, 16])
_SLIDE_VIEWS = dict(scores=[_WIN_SCORES], hpws=[2], wpws=[2], ohs=[16], ows=[32], flips=[False], **_WINDOWS)
_WANT = dict(raw_labels=True, want_labels=True, want_conf=False, want_probs=True)
_FIVE = _AREAS + [((1, 8, 8), U8), ((0,), F32), ((1, 3, 8, 8), F32)]
_NORM = dict(mean=[0.5, 0.5, 0.5], std=[0.5, 0.5, 0.5], reverse_channels=False)
_IMAGES = t(1, 8, 8, 3, dtype=U8)
_BATCH16 = t(1, 3, 16, 16, dtype=F32)
_TARGET16 = t(1, 257, dtype=I64)
_RECORDS = t(1, 16, dtype=I32)

GOOD = {
    "linear": (dict(x=t(1, 4, 64), w=t(32, 64), bias=None), [((1, 4, 32), BF)]),
    "linear_bwd": (dict(g=t(1, 4, 32), x=t(1, 4, 64), w=t(32, 64)), [((1, 4, 64), BF), ((32, 64), BF), ((32,), BF)]),
    "layer_norm": (dict(x=t(2, 3, 64), gamma=t(64), beta=t(64), eps=1e-5, gelu=False), [((2, 3, 64), BF), ((6,), F32), ((6,), F32)]),
    "layer_norm_bwd": (dict(dy=t(2, 3, 64), x=t(2, 3, 64), gamma=t(64), mean=t(6, dtype=F32), rstd=t(6, dtype=F32), gelu=False),
                       [((2, 3, 64), BF), ((64,), BF), ((64,), BF)]),
    "bias_attention": (dict(**_QKV, **_POS, **_NO_REL, **_REL_META), [((1, 32, 64), BF), ((1, 1, 32), F32)]),
    "bias_attention_bwd": (dict(dout=t(1, 32, 64), **_QKV, **_POS, **_OUT_LSE, **_NO_REL, **_REL_META), _NINE),
    "attention_bias": (dict(**_QKV, bias=None, gain=None, kv_len=None, causal=False, P=0, dropout_p=0.0, seed=0),
                       [((1, 32, 64), BF), ((1, 1, 32), F32), ((1, 32, 32), BF)]),
    "attention_bias_bwd": (dict(dout=t(1, 32, 64), **_QKV, bias=None, gain=None, kv_len=None, **_OUT_LSE, packed=t(1, 32, 32),
                                causal=False, P=0, dropout_p=0.0, seed=0), _DQKV + [((0,), F32), ((1,), F32)]),
    "bias_attention_bi": (dict(**_QKV, **_POS, **_NO_REL, **_REL_META, kv_len=None, dropout_p=0.0, seed=0),
                          [((1, 32, 64), BF), ((1, 1, 32), F32), ((1, 32, 32), BF)]),
    "bias_attention_bi_bwd": (dict(dout=t(1, 32, 64), **_QKV, **_POS, **_OUT_LSE, packed=t(1, 32, 32), **_NO_REL, **_REL_META,
                                   kv_len=None, dropout_p=0.0, seed=0), _NINE),
    "seg_loss": (dict(**_LOGITS, **_GRID16, label_smoothing=0.0), _LOSS4),
    "seg_loss_bwd": (dict(grad_loss=t(dtype=F32), dlogits=t(1, 2, 8), nseg=3), [((1, 2, 3), BF)]),
    "seg_loss_weighted": (dict(**_LOGITS, pixel_weight=t(1, 256, dtype=U8), class_weight=t(3, dtype=F32), **_GRID16,
                               label_smoothing=0.0, norm_pixels=False), _LOSS4),
    "seg_ohem": (dict(**_LOGITS, pixel_weight=None, **_GRID16, thresh=0.7, min_kept=1), [((1, 256), U8), ((4,), I64)]),
    "seg_dice": (dict(**_LOGITS, class_weight=None, **_GRID16, dice_weight=1.0, smooth=1.0),
                 [((), F32), ((1, 3, 3), F32), ((1, 2, 8), BF)]),
    "seg_distill": (dict(logits=t(1, 2, 3), teacher_logits=t(1, 2, 3), target=t(1, 257, dtype=I64), **_GRID16, weight=1.0,
                         temperature=1.0, mask_all=False), [((), F32), ((2,), F32), ((1, 2, 8), BF)]),
    "seg_predict": (dict(scores=_SCORES, hp=2, wp=2, h=8, w=8, want_conf=True, want_probs=True), _TRIPLE),
    "seg_predict_views": (dict(**_VIEWS, h=8, w=8, want_conf=True, want_probs=False), _TRIPLE[:2] + [((0,), F32)]),
    "seg_areas": (dict(labels=_MAP, gt=_MAP, n=3, raw_labels=True), _AREAS),
    "seg_confusion": (dict(labels=_MAP, gt=_MAP, n=3, raw_labels=True), [((3, 4), I64)]),
    "seg_boundary_areas": (dict(labels=_MAP, gt=_MAP, n=3, d=1, raw_labels=True), [((3, 3), I64), ((1, 8, 8), U8)]),
    "seg_score_views": (dict(**_VIEWS, gt=_MAP, **_WANT), _FIVE),
    "seg_render": (dict(labels=_MAP, image=t(1, 8, 8, 3, dtype=U8), palette=t(3, 3, dtype=U8), opacity=0.5, boundary=1,
                        boundary_color=[255, 255, 255], conf=None), [((1, 8, 8, 3), U8)]),
    "seg_conf_hist": (dict(labels=_MAP, conf=_CONF, n=3), [((3, 256), I64), ((2,), I64)]),
    "seg_calibration": (dict(labels=_MAP, conf=_CONF, gt=_MAP, n=3, raw_labels=True), [((3, 256, 2), I64), ((2,), I64)]),
    "seg_temperature_sweep": (dict(grids=t(2, 1, 4, 3, dtype=F32), hp=2, wp=2, gt=_MAP, raw_labels=True),
                              [((2, 256, 2), I64), ((2, 2), F64), ((2,), I64)]),
    "seg_pseudo": (dict(labels=_MAP, conf=_CONF, thresholds=t(3, dtype=I32), n=3, boundary=0, raw_labels=True),
                   [((1, 8, 8), U8), ((2, 3), I64)]),
    "seg_regions": (dict(labels=_MAP, connectivity=4), [((1, 8, 8), I32), ((1, 8, 8), I32)]),
    "seg_region_drop": (dict(labels=_MAP, connectivity=4, min_region=2, fill=255, n=3, raw_labels=True),
                        [((1, 8, 8), U8), ((3,), I64), ((1, 8, 8), I32)]),
    "seg_pamr": (dict(probs=t(3, 8, 8, dtype=F32), image=t(8, 8, 3, dtype=U8), iters=1, dilations=[1], want_conf=True,
                      want_probs=True), [((8, 8), U8), ((8, 8), F32), ((3, 8, 8), F32)]),
    "image_load": (dict(images=_IMAGES, oh=16, ow=16, **_NORM, dtype=F32), [((1, 3, 16, 16), F32)]),
    "seg_predict_windows": (dict(scores=_WIN_SCORES, hpw=2, wpw=2, oh=16, ow=32, **_WINDOWS, h=8, w=8, want_conf=True,
                                 want_probs=True), _TRIPLE),
    "seg_score_windows": (dict(scores=_WIN_SCORES, hpw=2, wpw=2, oh=16, ow=32, **_WINDOWS, gt=_MAP, **_WANT), _FIVE),
    "image_load_windows": (dict(images=_IMAGES, oh=16, ow=32, **_WINDOWS, **_NORM, dtype=BF), [((2, 3, 16, 16), BF)]),
    "seg_predict_slide_views": (dict(**_SLIDE_VIEWS, h=8, w=8, softmax=False, want_conf=True, want_probs=True), _TRIPLE),
    "seg_score_slide_views": (dict(**_SLIDE_VIEWS, gt=_MAP, softmax=True, **_WANT), _FIVE),
    "train_load": (dict(images=[t(8, 8, 3, dtype=U8)], labels=[t(8, 8, dtype=U8)], params=_RECORDS, P=16, nseg=3, seg_id_offset=1000,
                        **_NORM, raw_labels=True, dtype=F32), [((1, 3, 16, 16), F32), ((1, 257), I64)]),
    "mix_draw": (dict(src_target=_TARGET16, nseg=3, seg_id_offset=1000, seed=0, first_ordinal=0, mask="class"), [((1, 16), I32)]),
    "mix_apply": (dict(records=_RECORDS, src_images=_BATCH16, src_target=_TARGET16, src_weight=None, dst_images=_BATCH16,
                       dst_target=_TARGET16, dst_weight=None, nseg=3, seg_id_offset=1000),
                  [((1, 3, 16, 16), F32), ((1, 257), I64), ((0,), U8)]),
    "strong_draw": (dict(B=1, seed=0, first_ordinal=0, jitter_p8=205, blur_p8=128, device=torch.device("cuda")), [((1, 16), I32)]),
    "strong_apply": (dict(records=_RECORDS, images=_BATCH16, **_NORM), [((1, 3, 16, 16), F32)]),
}

# ------------------------------------------------------------------------------------------------------------ refusal probes
# (op, the arguments of its good call that are replaced, the complete message)
_BF_SCORES, _BF_WIN = t(1, 4, 3), t(1, 2, 4, 3)
_WIDE, _WIDE_WIN = t(1, 4, 513, dtype=F32), t(1, 2, 4, 513, dtype=F32)
_F32_GIVES = "scores must be fp32 (hip.rows_to_f32 / hip.neighbour_smoothing give it), "
_FUSED = "classes, the kernel takes 1 .. FUSED_MAX_CLASSES = 512"
_MAP_RULE = "must have 1 <= h, w and B * h * w < 2**31"
_GT_DTYPE = "ground truth must be uint8 or int16 (label PNG values or class ids), got dtype torch.int64"
_PIXELS = "labels must be [H, W] or [B, H, W] with 1 <= pixels < 2**31, got (8,)"
_SEVENTEEN = dict(scores=[_SCORES] * 17, hps=[2] * 17, wps=[2] * 17, flips=[False] * 17)
_SEVENTEEN_SLIDE = dict(scores=[_WIN_SCORES] * 17, hpws=[2] * 17, wpws=[2] * 17, ohs=[16] * 17, ows=[32] * 17, flips=[False] * 17)

PROBES = [
    # scores that are not fp32
    ("seg_predict", dict(scores=_BF_SCORES), "ifseg::seg_predict: " + _F32_GIVES + "got dtype torch.bfloat16"),
    ("seg_predict_views", dict(scores=[_BF_SCORES]), "ifseg::seg_predict_views: " + _F32_GIVES + "view 0 has dtype torch.bfloat16"),
    ("seg_score_views", dict(scores=[_BF_SCORES]), "ifseg::seg_predict_views: " + _F32_GIVES + "view 0 has dtype torch.bfloat16"),
    ("seg_predict_windows", dict(scores=_BF_WIN), "ifseg::seg_predict_windows: " + _F32_GIVES + "got dtype torch.bfloat16"),
    ("seg_score_windows", dict(scores=_BF_WIN), "ifseg::seg_score_windows: " + _F32_GIVES + "got dtype torch.bfloat16"),
    ("seg_predict_slide_views", dict(scores=[_BF_WIN]),
     "ifseg::seg_predict_slide_views: view 0: " + _F32_GIVES + "got dtype torch.bfloat16"),
    ("seg_score_slide_views", dict(scores=[_BF_WIN]), "ifseg::seg_score_slide_views: view 0: " + _F32_GIVES + "got dtype torch.bfloat16"),
    # more classes than the fused kernels take
    ("seg_loss", dict(logits=t(1, 2, 513)), "ifseg::seg_loss: nseg = 513 " + _FUSED),
    ("seg_loss_weighted", dict(logits=t(1, 2, 513)), "ifseg::seg_loss: nseg = 513 " + _FUSED),
    ("seg_ohem", dict(logits=t(1, 2, 513)), "ifseg::seg_loss: nseg = 513 " + _FUSED),
    ("seg_dice", dict(logits=t(1, 2, 513)), "ifseg::seg_loss: nseg = 513 " + _FUSED),
    ("seg_distill", dict(logits=t(1, 2, 513)), "ifseg::seg_loss: nseg = 513 " + _FUSED),
    ("seg_predict", dict(scores=_WIDE), "ifseg::seg_predict: n = 513 " + _FUSED),
    ("seg_predict_views", dict(scores=[_WIDE]), "ifseg::seg_predict_views: n = 513 " + _FUSED),
    ("seg_score_views", dict(scores=[_WIDE]), "ifseg::seg_predict_views: n = 513 " + _FUSED),
    ("seg_areas", dict(n=513), "ifseg::seg_areas: n = 513 " + _FUSED),
    ("seg_confusion", dict(n=0), "ifseg::seg_confusion: n = 0 " + _FUSED),
    ("seg_boundary_areas", dict(n=513), "ifseg::seg_boundary_areas: n = 513 " + _FUSED),
    ("seg_predict_windows", dict(scores=_WIDE_WIN), "ifseg::seg_predict_windows: n = 513 " + _FUSED),
    ("seg_score_windows", dict(scores=_WIDE_WIN), "ifseg::seg_score_windows: n = 513 " + _FUSED),
    ("seg_predict_slide_views", dict(scores=[_WIDE_WIN]), "ifseg::seg_predict_slide_views: view 0: n = 513 " + _FUSED),
    ("seg_score_slide_views", dict(scores=[_WIDE_WIN]), "ifseg::seg_score_slide_views: view 0: n = 513 " + _FUSED),
    # "the kernel takes 1 .. %d": views, classes, temperatures
    ("seg_predict_views", _SEVENTEEN, "ifseg::seg_predict_views: 17 views, the kernel takes 1 .. 16"),
    ("seg_score_views", _SEVENTEEN, "ifseg::seg_predict_views: 17 views, the kernel takes 1 .. 16"),
    ("seg_predict_slide_views", _SEVENTEEN_SLIDE, "ifseg::seg_predict_slide_views: 17 views, the kernel takes 1 .. 16"),
    ("seg_score_slide_views", _SEVENTEEN_SLIDE, "ifseg::seg_score_slide_views: 17 views, the kernel takes 1 .. 16"),
    ("seg_conf_hist", dict(n=513), "ifseg::seg_conf_hist: n = 513 classes, the kernel takes 1 .. 512"),
    ("seg_conf_hist", dict(conf=t(1, 8, 8)),
     "ifseg::seg_conf_hist: conf must be float32 of the labels' shape (1, 8, 8), got torch.bfloat16 (1, 8, 8)"),
    ("seg_calibration", dict(n=0), "ifseg::seg_calibration: n = 0 classes, the kernel takes 1 .. 512"),
    ("seg_temperature_sweep", dict(grids=t(2, 1, 4, 513, dtype=F32)),
     "ifseg::seg_temperature_sweep: n = 513 classes, the kernel takes 1 .. 512"),
    ("seg_temperature_sweep", dict(grids=t(17, 1, 4, 3, dtype=F32)), "ifseg::seg_temperature_sweep: K = 17 grids, the kernel takes 1 .. 16"),
    ("seg_pamr", dict(probs=t(513, 8, 8, dtype=F32)), "ifseg::seg_pamr: n = 513 classes, the kernel takes 1 .. 512"),
    # a label map without pixels
    ("seg_predict", dict(h=0), "ifseg::seg_predict: the label map [1, 0, 8] " + _MAP_RULE),
    ("seg_predict_views", dict(w=0), "ifseg::seg_predict_views: the label map [1, 8, 0] " + _MAP_RULE),
    ("seg_score_views", dict(gt=t(1, 0, 8, dtype=U8)), "ifseg::seg_predict_views: the label map [1, 0, 8] " + _MAP_RULE),
    ("seg_predict_windows", dict(h=0), "ifseg::seg_predict_windows: the label map [1, 0, 8] " + _MAP_RULE),
    ("seg_score_windows", dict(gt=t(1, 8, 0, dtype=U8)), "ifseg::seg_score_windows: the label map [1, 8, 0] " + _MAP_RULE),
    ("seg_predict_slide_views", dict(h=0), "ifseg::seg_predict_slide_views: view 0: the label map [1, 0, 8] " + _MAP_RULE),
    ("seg_score_slide_views", dict(gt=t(1, 0, 8, dtype=U8)), "ifseg::seg_score_slide_views: view 0: the label map [1, 0, 8] " + _MAP_RULE),
    # the ground truth of the score ops: dtype, [B, h, w], the batch
    ("seg_score_views", dict(gt=t(1, 8, 8, dtype=I64)), "ifseg::seg_score_views: " + _GT_DTYPE),
    ("seg_score_windows", dict(gt=t(1, 8, 8, dtype=I64)), "ifseg::seg_score_windows: " + _GT_DTYPE),
    ("seg_score_slide_views", dict(gt=t(1, 8, 8, dtype=I64)), "ifseg::seg_score_slide_views: " + _GT_DTYPE),
    ("seg_score_views", dict(gt=t(8, 8, dtype=U8)), "ifseg::seg_score_views: ground truth must be [B, h, w], got (8, 8)"),
    ("seg_score_windows", dict(gt=t(8, 8, dtype=U8)), "ifseg::seg_score_windows: ground truth must be [B, h, w], got (8, 8)"),
    ("seg_score_slide_views", dict(gt=t(8, 8, dtype=U8)), "ifseg::seg_score_slide_views: ground truth must be [B, h, w], got (8, 8)"),
    ("seg_score_views", dict(gt=t(2, 8, 8, dtype=U8)), "ifseg::seg_score_views: ground truth (2, 8, 8) for a batch of 1"),
    ("seg_score_windows", dict(gt=t(2, 8, 8, dtype=I16)), "ifseg::seg_score_windows: ground truth (2, 8, 8) for a batch of 1"),
    ("seg_score_slide_views", dict(gt=t(2, 8, 8, dtype=U8)), "ifseg::seg_score_slide_views: ground truth (2, 8, 8) for a batch of 1"),
    # the weights of the seg-loss family
    ("seg_loss_weighted", dict(pixel_weight=t(1, 256, dtype=F32)),
     "ifseg::seg_loss_weighted: pixel_weight must be uint8 [B, H * W] = [1, 256], got torch.float32 (1, 256)"),
    ("seg_ohem", dict(pixel_weight=t(1, 257, dtype=U8)),
     "ifseg::seg_ohem: pixel_weight must be uint8 [B, H * W] = [1, 256], got torch.uint8 (1, 257)"),
    ("seg_loss_weighted", dict(class_weight=t(4, dtype=F32)),
     "ifseg::seg_loss_weighted: class_weight must be fp32 [nseg] = [3], got torch.float32 (4,)"),
    ("seg_dice", dict(class_weight=t(3)), "ifseg::seg_dice: class_weight must be fp32 [nseg] = [3], got torch.bfloat16 (3,)"),
    ("seg_loss_weighted", dict(label_smoothing=1.5), "ifseg::seg_loss_weighted: label_smoothing must lie in [0, 1], got 1.5"),
    # the ignore band, the maps of render / pseudo / regions
    ("seg_render", dict(boundary=5), "ifseg::seg_render: boundary must be in 0 .. 4, got 5"),
    ("seg_pseudo", dict(boundary=-1), "ifseg::seg_pseudo: boundary must be in 0 .. 4, got -1"),
    ("seg_render", dict(labels=t(1, 8, 8, dtype=I64)),
     "ifseg::seg_render: labels must be uint8 or int16 (what seg_predict gives), got dtype torch.int64"),
    ("seg_areas", dict(labels=t(1, 8, 8, dtype=I64)),
     "ifseg::seg_areas: labels must be uint8 or int16 (what seg_predict gives), got dtype torch.int64"),
    ("seg_render", dict(conf=t(1, 8, dtype=F32)), "ifseg::seg_render: conf must be float32 of the labels' shape (1, 8, 8), got torch.float32 (1, 8)"),
    ("seg_pseudo", dict(conf=t(1, 8, dtype=F32)), "ifseg::seg_pseudo: conf must be float32 of the labels' shape (1, 8, 8), got torch.float32 (1, 8)"),
    ("seg_render", dict(labels=t(8, dtype=U8)), "ifseg::seg_render: " + _PIXELS),
    ("seg_regions", dict(labels=t(8, dtype=U8)), "ifseg::seg_regions: " + _PIXELS),
    ("seg_region_drop", dict(labels=t(8, dtype=U8)), "ifseg::seg_region_drop: " + _PIXELS),
    # normalisation and the output dtype of the image ops
    ("image_load", dict(mean=[0.5, 0.5]), "ifseg::image_load: mean and std must have three entries, got 2 and 3"),
    ("image_load_windows", dict(std=[0.5] * 4), "ifseg::image_load_windows: mean and std must have three entries, got 3 and 4"),
    ("train_load", dict(mean=[0.5]), "ifseg::train_load: mean and std must have three entries, got 1 and 3"),
    ("image_load", dict(dtype=torch.float16), "ifseg::image_load: the output dtype must be torch.float32 or torch.bfloat16, got torch.float16"),
    ("image_load_windows", dict(dtype=F64),
     "ifseg::image_load_windows: the output dtype must be torch.float32 or torch.bfloat16, got torch.float64"),
    ("train_load", dict(dtype=torch.float16), "ifseg::train_load: the output dtype must be torch.float32 or torch.bfloat16, got torch.float16"),
    # wrong in two ways: the order of the checks
    ("seg_predict", dict(scores=t(1, 4, 513)), "ifseg::seg_predict: " + _F32_GIVES + "got dtype torch.bfloat16"),
    ("seg_score_windows", dict(gt=t(2, 8, 8, dtype=I64)), "ifseg::seg_score_windows: " + _GT_DTYPE),
    ("seg_loss_weighted", dict(pixel_weight=t(1, 255, dtype=U8), label_smoothing=2.0),
     "ifseg::seg_loss_weighted: pixel_weight must be uint8 [B, H * W] = [1, 256], got torch.uint8 (1, 255)"),
]
