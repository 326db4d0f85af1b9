"""Inference entry point: images in, label maps at image resolution out.

The reference's user-facing demo is model forward -> softmax per patch -> optional top-k neighbour smoothing on the trunk
features -> bilinear resize of the class probabilities to the image shape -> optional dense CRF -> argmax.  Here the forward is
the HIP engine, the smoothing `hip.neighbour_smoothing`, the CRF `crf.rgb_dense_crf`, and softmax / resize / argmax at image
resolution one fused kernel (`hip.seg_predict`, csrc/predict.hip): the [B, n, h, w] probabilities are only written when the CRF
or the caller asks for them.

    seg = Segmenter(model, task)                      # or task.build_segmenter(model)
    res = seg(images)                                 # float [B, 3, H, W] (normalised) or uint8 RGB [B, H, W, 3] / [H, W, 3]
    res.labels                                        # uint8 (int16 above 256 classes) [B, H, W], on the device
    out = seg.segment_raw(photos)                     # uint8 RGB [H, W, 3] images of ANY size, one or a list: the reference's
    out[i].labels                                     # evaluation transform on the device (hip.image_load), labels [H_i, W_i]
    out = seg.segment_raw(photos, scales=(0.5, 0.75, 1.0, 1.25, 1.5, 1.75), flip=True)      # "ms+flip", see below

Multi-scale + flip (mmseg's `MultiScaleFlipAug(img_ratios=scales, flip=True)`, the setting mIoU tables call "ms+flip"): every
image is loaded once per ratio at `imageio.eval_size(H, W, P, ratio)`, mirrored views are the loaded tensor flipped, each view
runs the same forward (and smoothing), and ONE launch of `hip.seg_predict_views` resizes the K per-patch score grids to the
image's shape, un-mirrors, averages and takes the argmax: no [n, H, W] tensor per view is written or added.  The reference
never turns this on, so there is no golden for it: parity is to the specification `upsample_views_reference`.  Cost: every
distinct view size is one more entry of the engine's resized-bias cache (`engine.py:_resized_biases`), whose entries grow
with the square of the grid; the views are therefore run size by size (`imageio.plan_views`).

Sliding-window inference (mmseg's `test_cfg=dict(mode='slide', crop_size=(P, P), stride=(s, s))`, how fixed-grid transformer
segmenters are scored): `seg.segment_raw(photos, slide=True)` cuts the resized image into overlapping P x P windows
(`imageio.slide_windows`, written directly by `hip.image_load_windows`), runs every window at the trained grid -- one network
size for a whole data set, no resized-bias entry, the windows of all images in the same batches (`imageio.plan_slide_views`,
here with one view) -- and
ONE launch of `hip.seg_predict_windows` per image resizes the windows' scores, averages them where windows overlap and
resizes the result to the image's shape: no per-window [n, P, P] tensor, sum or count plane is written.  Limits: the
reference never slides, so there is no golden and parity is to the specification `slide_reference`; a single view only
(`slide` with several scales or `flip` is a ValueError) unless the Segmenter was built with `slide_views=True`.

Multi-scale + flip OVER sliding windows (mmseg's `MultiScaleFlipAug(img_ratios, flip=True)` over `test_cfg mode='slide'`, the
setting the mIoU tables of fixed-grid transformer segmenters report): `Segmenter(..., slide_views=True)` is the opt-in.  Every
view of every image is cut into windows (mirrored views from the mirrored resized image, `hip.image_load_windows(flip=True)`),
all windows of all views and images share batches (`imageio.plan_slide_views`; with crop = P one network size and no
resized-bias entry for the whole evaluation), and ONE launch of `hip.seg_predict_slide_views` per image merges every view's
windows, resizes, un-mirrors, and averages the views.  Two orders: upsample="logits" is mmseg's (the merged, resized logits
of a view are softmaxed per pixel inside the launch, then averaged); upsample="probs" and the neighbour smoothing hand over
probabilities, and everything behind them is linear.  Limits: 16 views, 64 windows per view, 512 classes; no golden (the
reference never slides): parity is to the specification `slide_views_reference`.

    seg = Segmenter(model, task, upsample="logits", slide_views=True)
    score = seg.evaluate_raw(photos, label_pngs, slide=True, scales=(0.5, 0.75, 1.0, 1.25, 1.5, 1.75), flip=True)

    out = seg.segment_raw(photos, slide=True)                                                # crop P, stride 2 P // 3
    score = seg.evaluate_raw(photos, label_pngs, slide=(512, 341))                           # (crop, stride), ints or (h, w)

Scoring against ground truth: `seg.evaluate_raw(photos, label_maps, ...)` is `segment_raw` with the same arguments whose last
launch per image also counts the label map against the image's ground truth (`hip.seg_score` / `hip.seg_score_views`: the
predict kernels with the counting in their epilogue; `hip.seg_areas` behind the CRF), into one `SegmentationScore` on the
device; `score.summary()` gives aAcc / mIoU / mAcc by `SegCriterion.reduce_metrics`' formulas and is the only host round trip.
`areas_reference` is the specification of the counters.  With upsample="logits" and one view this is the reference's
`valid_step` metric (seg_criterion.py:289-347); with the defaults it is the demo's order, probabilities resized.

    score = seg.evaluate_raw(photos, label_pngs, scales=(0.5, 0.75, 1.0, 1.25, 1.5, 1.75), flip=True)   # uint8 [H_i, W_i] maps
    for more in batches: seg.evaluate_raw(*more, into=score)                                             # a whole validation set
    score.summary()                                    # {"aAcc", "mIoU", "mAcc", "IoU": [n], "Acc": [n], "pixels"}

Which class is taken for which: `seg.evaluate_raw(..., confusion=True)` also fills `score.confusion`, int64 [n, n + 1] (row = the
ground truth's class, column = the predicted label, the last column for labels outside [0, n)): the scoring launch then
writes its label map and one launch of `hip.seg_confusion` per image counts the pairs, in every setting above.
`confusion_reference` is the specification; the matrix's sum, diagonal, column and row sums are `tally[0]` and `areas`.

    score = seg.evaluate_raw(photos, label_pngs, confusion=True)
    score.confusions(10)                               # [(gt class, predicted class, pixels, share of the gt class), ...]
    score.merged(class_to_super_category).summary()    # the same evaluation under a coarser label set, no second pass
    score.group_summary({"seen": seen_ids, "unseen": unseen_ids})   # per-group mIoU / mAcc and hIoU (needs `areas` only)

Whether the contours are in the right place: `seg.evaluate_raw(..., boundary_iou=True)` also fills `score.boundary`, int64
[3, n]: Boundary IoU's band areas (Cheng et al., CVPR 2021), the three rows of `areas` restricted to the pixels within d of a
contour of both maps / the labels / the ground truth, d = `boundary_distance(H_i, W_i)` = 2 % of the image's diagonal.  As for
the matrix, the scoring launch writes its label map and one launch of `hip.seg_boundary_areas` (csrc/boundary.hip) per image
counts it, behind `hip.seg_confusion` where both are asked for, in every setting above; `summary()` then carries "mBIoU" and
"BIoU".  `boundary_areas_reference` is the specification and says what is not pinned; d <= 64.

    score = seg.evaluate_raw(photos, label_pngs, boundary_iou=True)                # or a ratio: boundary_iou=0.01
    score.summary()["mBIoU"]

Whether the confidence means anything: `seg.evaluate_raw(..., calibration=True)` also fills `score.calibration`, int64
[n, 256, 2]: per predicted class and confidence bin (`conf_bin`, the pseudo-label path's) the scored pixels that were wrong and
right -- the reliability diagram and ECE (Guo et al., ICML 2017).  The scoring launch writes its labels and conf and one launch
of `hip.seg_calibration` (csrc/calib.hip) per image counts them against the ground truth, behind the other two, in every
setting above; `summary()` then carries "ECE", "MCE" and "cECE".  `calibration_reference` is the specification.

    score = seg.evaluate_raw(photos, label_pngs, calibration=True)                 # a labelled validation set
    score.summary()["ECE"];  score.reliability(bins=16)                            # (pixels, accuracy, confidence) per bin
    t = score.precision_thresholds(0.9)                                            # per class: the bin above which it is 90 % right
    seg.pseudo_label_raw(unlabelled_photos, thresholds=t)

Making the confidence mean something: `seg.calibrate_raw(photos, label_pngs)` is temperature scaling (the same paper's
one-parameter remedy) from a labelled validation set.  The network's logits do not depend on the temperature, so the forward
runs once per batch; `patch_scores_at` softmaxes its padded logits at K temperatures (`default_temperatures()`: 16 from 0.297
to 4.0) and ONE launch of `hip.seg_temperature_sweep` per image (csrc/tsweep.hip) scores all K grids against the ground truth:
per temperature the reliability counts, NLL and Brier -- the proper scores a temperature is fitted on, which need the true
class's probability at image resolution and are computed without an [n, H, W] tensor.  `temperature_sweep_reference` is the
specification.  One plain view only; the Segmenter's own `temperature` is not consulted.

    sweep = seg.calibrate_raw(photos, label_pngs)                                  # a `TemperatureSweep`; into=sweep for more batches
    sweep.summary()                                    # {"temperatures", "NLL", "Brier", "ECE", "MCE", "aAcc": [K] each, "pixels", "best"}
    seg.temperature = sweep.best()                     # lowest mean NLL; the confidences of every later call are calibrated

The label map as a picture: `seg.render_raw(photos, ...)` is `segment_raw` followed by one launch of `hip.seg_render`
(csrc/render.hip) per image, which blends the classes' colours over the original photo and draws class contours -- the demo's
`cmap[labels]` and `image * (1 - opacity) + cmap[labels] * opacity`, without the label map leaving the device.  The rule is
integer and `render_reference` states it; there is no reference golden (the notebook's figure goes through matplotlib and
PIL): parity is exact to `render_reference`, which equals the demo's formula at the demo's opacity.

    pics = seg.render_raw(photos, opacity=0.5, boundary=1)          # [RenderResult(picture uint8 [H_i, W_i, 3], labels, conf)]

Pseudo-labels for self-training (adapting the image-free model to unlabeled photographs of the target domain, the CBST /
MaskCLIP+ recipe): `seg.pseudo_label_raw(photos, keep=0.5, boundary=1)` is `segment_raw(return_conf=True)`, one launch of
`hip.seg_conf_hist` per image (csrc/pseudo.hip: the per-class histogram of the winning probability, into a
`ConfidenceHistogram` that can span a data set), the per-class thresholds from it on the device (`pseudo_thresholds`: a fixed
threshold, or the most confident share of every class) and one launch of `hip.seg_pseudo` per image, which writes the uint8
label map `task.train_sample` takes: kept pixels carry their class, everything else -- below its class's threshold, or within
`boundary` pixels of a class edge -- is 255.  `confidence_histogram_reference` and `pseudo_label_reference` are the
specifications, in integers.  `task.self_train_sample(model, photos, first_ordinal, keep=0.5)` is both steps.

    hist = ConfidenceHistogram(seg.n, device)
    for photos in batches: seg.pseudo_label_raw(photos, hist=hist)                 # pass 1: what "confident" means per class
    t = hist.thresholds(keep=0.5, floor=0.3)
    out = seg.pseudo_label_raw(photos, thresholds=t, boundary=1)                   # [PseudoLabelResult(labels, predicted, conf, kept)]

Those filters judge a pixel; what they leave behind is a matter of regions: speckles of a few confident but wrong pixels, and
the crumbs left where the filters cut a region apart.  `min_region=K` adds one `hip.seg_region_drop` per image on the filtered
map (csrc/regions.hip: connected regions of equal values by a block-based union-find, four launches): every region of fewer
than K pixels becomes 255 and its weights 0, and the result's `region_dropped` counts them per class.  `regions_reference`
and `region_drop_reference` are the specifications.

    out = seg.pseudo_label_raw(photos, thresholds=t, boundary=1, min_region=16, region_connectivity=8)

The list of objects -- what a robot, a counter or an annotation tool consumes -- is `regions_raw`: `segment_raw`, then one
`hip.seg_region_table` per image (csrc/regiontab.hip, four launches behind the regions'): one row per connected region with
its class value, area, bounding box, coordinate sums and summed confidence, numbered in ascending order of the regions' roots,
on the device.  `region_table_reference` is the specification; `RegionTable.to_list` is the one host round trip.

    for t in seg.regions_raw(photos, min_region=50):                # [RegionTable(rows, sums, count, slot, labels, conf)]
        print(t.to_list(names))                                     # [{"value", "name", "area", "box", "centroid", "confidence"}]

Label maps leave the device as run tables: `export_raw` is `segment_raw`, then one `hip.seg_rle_encode` per image
(csrc/rle.hip, three launches): the map's runs (start, value) in COCO's column-major run order, on the device.
`rle_encode_reference` / `rle_decode_reference` are the specifications; `RunLengthMap.to_coco` is the one host round trip and
gives COCO stuff results (`coco_counts`, `coco_rle_string`: cocoapi's RLE string, written here from its algorithm).

    for i, m in enumerate(seg.export_raw(photos)):                  # [RunLengthMap(runs, count, shape, dtype)]
        results += m.to_coco(image_id=i, category_ids=ids)          # [{"image_id", "category_id", "segmentation"}]

A cheap refinement that looks at the photograph: `Segmenter(..., pamr_iters=10)` runs pixel-adaptive mask refinement (PAMR,
Araslanov & Roth, CVPR 2020; what MaskCLIP applies to its pseudo-labels) on the resized values of every image, in the slot of
the CRF: `hip.seg_pamr` (csrc/pamr.hip), one affinity launch on the original uint8 photo and one launch per iteration.  Each
iteration replaces a pixel's class values by a convex combination of its neighbours' (8 per dilation, 1, 2, 4, 8, 12, 24 by
default), weighted by how alike the colours are against the local contrast.  Linear in the pixels, where the CRF's exact dense
kernels are quadratic, and probabilities stay probabilities: conf, the calibration counters, the pseudo-label thresholds and
`fade_by_conf` keep their meaning behind it.  `pamr_reference` is the specification; the reference has no counterpart, so
there is no golden.

    seg = Segmenter(model, task, pamr_iters=10)
    out = seg.pseudo_label_raw(unlabelled_photos, keep=0.5)         # the labels hug the photo's edges

How the four settings share their code: a front (`Segmenter._raw_views` without `slide`, `_raw_window_views` with it, for one
view or many) runs the loads and the forwards and hands back one `_Merge` per image -- the setting's last launch, as its
`hip.seg_predict*` and its `hip.seg_score*`, bound to the image's scores and geometry.  `Segmenter._label` finishes an image
from its merge (the predict launch, then the CRF) and `Segmenter._count` scores it (the scoring launch; with the CRF on
`_label` and `hip.seg_areas`; `hip.seg_confusion`, `hip.seg_boundary_areas` and `hip.seg_calibration` behind either); `__call__` and `evaluate` go through the same two with the
single-view merge of their batch.

Nothing in the call synchronises with the host; `labels`, `conf` and `probs` stay on the device.  There is no CPU fallback:
`upsample_argmax_reference` is the specification the tests compare against, not a second implementation of the path.
"""
import math
from typing import Callable, NamedTuple, Optional

import torch
import torch.nn.functional as F

from . import hip
from .imageio import HALF, eval_size, plan_slide_views, plan_views, slide_windows, view_list
from .tasks.mm_tasks.segmentation import BOS, EOS, PROMPT_IDS

MAX_CLASSES = hip.SEG_PREDICT_MAX_CLASSES


class SegmentationResult(NamedTuple):
    labels: torch.Tensor                       # [B, h, w] uint8 (n <= 256) or int16
    conf: Optional[torch.Tensor]               # [B, h, w] fp32: the value of the winning class
    probs: Optional[torch.Tensor]              # [B, n, h, w] fp32: every class


class _Merge(NamedTuple):
    """What a front of the Segmenter hands back per image (or batch): the last launch of its setting, bound to its scores and
    geometry.  Every setting is finished (`Segmenter._label`) and scored (`Segmenter._count`) through these two."""
    predict: Callable                          # (h, w, conf=, probs=, label_dtype=) -> what its hip.seg_predict* returns
    score: Callable                            # (gt, labels=, label_dtype=, raw_labels=, areas=, tally=) -> its hip.seg_score*'s


def upsample_argmax_reference(scores, hp, wp, h, w, dtype=torch.float64):
    """CPU specification of hip.seg_predict: scores [B, hp*wp, n] -> (labels int64 [B, h, w], conf [B, h, w], probs
    [B, n, h, w]) with F.interpolate(bilinear, align_corners=False) evaluated in `dtype`, then argmax (first maximum).
    Runs on any device."""
    B, P, n = scores.shape
    assert P == hp * wp, (tuple(scores.shape), hp, wp)
    grid = scores.to(dtype).transpose(1, 2).reshape(B, n, hp, wp)
    probs = F.interpolate(grid, size=(h, w), mode="bilinear", align_corners=False)
    labels = probs.argmax(dim=1)
    return labels, probs.gather(1, labels[:, None]).squeeze(1), probs


def upsample_views_reference(views, h, w, dtype=torch.float64):
    """CPU specification of hip.seg_predict_views: `views` is a list of (scores [B, hp*wp, n], hp, wp, flip).  View k is
    reshaped to [B, n, hp, wp], its columns reversed if `flip` (a permutation, in front of the resize: the network saw the
    mirrored image), resized with F.interpolate(bilinear, align_corners=False) in `dtype`; the K results are added in the
    order k = 0 .. K-1 and multiplied by 1 / K rounded to `dtype`; labels are the first maximum.
    -> (labels int64 [B, h, w], conf [B, h, w], probs [B, n, h, w]) as `upsample_argmax_reference`.  Runs on any device."""
    total = None
    for scores, hp, wp, flip in views:
        B, P, n = scores.shape
        assert P == hp * wp, (tuple(scores.shape), hp, wp)
        grid = scores.to(dtype).transpose(1, 2).reshape(B, n, hp, wp)
        if flip:
            grid = grid.flip(-1)
        up = F.interpolate(grid, size=(h, w), mode="bilinear", align_corners=False)
        total = up if total is None else total + up
    probs = total * torch.tensor(1.0 / len(views), dtype=dtype, device=total.device)
    labels = probs.argmax(dim=1)
    return labels, probs.gather(1, labels[:, None]).squeeze(1), probs


def slide_reference(scores, hpw, wpw, oh, ow, crop, stride, h, w, dtype=torch.float64):
    """CPU specification of hip.seg_predict_windows: scores [B, Nw, hpw*wpw, n], window k of `slide_windows(oh, ow, crop,
    stride)` having run the network on its own hpw x wpw grid.  Each window is reshaped to [B, n, hpw, wpw] and resized with
    F.interpolate(bilinear, align_corners=False) to the window's (ch, cw) in `dtype`; the results are added into a zero
    [B, n, oh, ow] plane at the windows' places, in window order, a count plane takes 1 per window, and the sum is divided by
    the count (mmseg's `slide_inference`); where (h, w) != (oh, ow) the quotient is resized to (h, w) the same way.  Labels are
    the first maximum.  -> (labels int64 [B, h, w], conf [B, h, w], probs [B, n, h, w]) as `upsample_argmax_reference`.
    Runs on any device."""
    ys, xs, ch, cw = slide_windows(oh, ow, crop, stride)
    B, Nw, P, n = scores.shape
    assert Nw == len(ys) * len(xs) and P == hpw * wpw, (tuple(scores.shape), len(ys), len(xs), hpw, wpw)
    total = torch.zeros(B, n, oh, ow, dtype=dtype, device=scores.device)
    count = torch.zeros(1, 1, oh, ow, dtype=dtype, device=scores.device)
    for k, (y, x) in enumerate((y, x) for y in ys for x in xs):
        grid = scores[:, k].to(dtype).transpose(1, 2).reshape(B, n, hpw, wpw)
        total[:, :, y:y + ch, x:x + cw] += F.interpolate(grid, size=(ch, cw), mode="bilinear", align_corners=False)
        count[:, :, y:y + ch, x:x + cw] += 1
    probs = total / count
    if (h, w) != (oh, ow):
        probs = F.interpolate(probs, size=(h, w), mode="bilinear", align_corners=False)
    labels = probs.argmax(dim=1)
    return labels, probs.gather(1, labels[:, None]).squeeze(1), probs


def slide_views_reference(views, crop, stride, h, w, softmax, dtype=torch.float64):
    """CPU specification of hip.seg_predict_slide_views: `views` is a list of K entries (scores [B, Nw_k, hpw_k*wpw_k, n], hpw_k,
    wpw_k, oh_k, ow_k, flip_k), view k being an input of `slide_reference` at its own [oh_k, ow_k] plane.  Per view, in order:
    p = slide_reference(...)[2], the window merge and the resize to (h, w), unchanged; if flip_k, p = p.flip(-1) (the network
    saw the resized image mirrored, and mmseg un-mirrors after the resize to the image's shape); if `softmax`,
    p = p.softmax(1).  The K results are added in view order and multiplied by 1 / K rounded to `dtype`; labels are the first
    maximum.  softmax=True is mmseg's order (`slide_inference` -> resize -> softmax -> un-flip, summed over the views, divided
    by K); softmax=False is this project's "probs" order, the per-patch softmax applied in front of the merge and everything
    behind it linear.  -> (labels int64 [B, h, w], conf [B, h, w], probs [B, n, h, w]) as `upsample_argmax_reference`.
    Runs on any device."""
    total = None
    for scores, hpw, wpw, oh, ow, flip in views:
        p = slide_reference(scores, hpw, wpw, oh, ow, crop, stride, h, w, dtype)[2]
        if flip:
            p = p.flip(-1)
        if softmax:
            p = p.softmax(1)
        total = p if total is None else total + p
    probs = total * torch.tensor(1.0 / len(views), dtype=dtype, device=total.device)
    labels = probs.argmax(dim=1)
    return labels, probs.gather(1, labels[:, None]).squeeze(1), probs


PAMR_TAPS = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))
PAMR_DILATIONS = hip.SEG_PAMR_DILATIONS


def _pamr_neighbours(H, W, dilations, device):
    """neighbour k = 8 i + t of every pixel, t over PAMR_TAPS at dilation i: (rows [H, 1], columns [1, W]), clamped to the image"""
    ys, xs = torch.arange(H, device=device), torch.arange(W, device=device)
    return [((ys + d * oy).clamp(0, H - 1)[:, None], (xs + d * ox).clamp(0, W - 1)[None, :]) for d in dilations for oy, ox in PAMR_TAPS]


def pamr_affinity_reference(image, dilations=PAMR_DILATIONS, dtype=torch.float64):
    """CPU specification of hip.pamr_affinity: image uint8 [H, W, 3] -> w [8 D, H, W] in `dtype`.  Per channel, in integers:
    S1, S2 = the sums of x and x^2 (grey levels) over the 9 taps of every dilation -- the 8 neighbours and the centre, which is
    thereby counted once per dilation -- M = 9 D, and the numerator M S2 - S1^2 of the unbiased variance, exact at every
    precision.  Then, in `dtype`: std = sqrt(numerator / (M (M - 1))), a_k = -((t_0 + t_1) + t_2) / 3 with
    t_ch = |x_ch(p) - x_ch(q_k)| / (1e-8 + 0.1 std_ch), and w = softmax_k a_k.  This is PAMR's affinity (Araslanov & Roth, CVPR
    2020: LocalStDev, LocalAffinityAbs, mean over the channels, softmax) on the grey levels in place of the normalised image:
    the ratio is scale-free per channel, so only the 1e-8 differs.  Runs on any device."""
    H, W = int(image.shape[0]), int(image.shape[1])
    D = len(dilations)
    M = 9 * D
    x = image.to(torch.int64)
    taps = [x[yy, xx] for yy, xx in _pamr_neighbours(H, W, dilations, image.device)]
    s1, s2 = D * x, D * x * x
    for t in taps:
        s1, s2 = s1 + t, s2 + t * t
    den = 1e-8 + 0.1 * ((M * s2 - s1 * s1).to(dtype) / (M * (M - 1))).sqrt()
    a = []
    for t in taps:
        q = (x - t).abs().to(dtype) / den
        a.append(-((q[..., 0] + q[..., 1]) + q[..., 2]) / 3)
    return torch.stack(a).softmax(0)


def pamr_iterate_reference(w, m, dilations=PAMR_DILATIONS):
    """CPU specification of hip.pamr_iterate: w [8 D, H, W], m [n, H, W] -> m' [n, H, W] in w's dtype,
    m'(c, p) = sum_k w(k, p) m(c, q_k(p)), added in the order k = 0 .. 8 D - 1.  Runs on any device."""
    H, W = int(m.shape[1]), int(m.shape[2])
    m, out = m.to(w.dtype), None
    for k, (yy, xx) in enumerate(_pamr_neighbours(H, W, dilations, m.device)):
        term = w[k] * m[:, yy, xx]
        out = term if out is None else out + term
    return out


def pamr_reference(image, m, dilations=PAMR_DILATIONS, iters=10, dtype=torch.float64):
    """CPU specification of hip.seg_pamr, pixel-adaptive mask refinement: image uint8 RGB [H, W, 3], m [n, H, W] (the values
    `seg_predict(probs=True)` hands over) -> (labels int64 [H, W], conf [H, W], the refined values [n, H, W]) in `dtype`:
    `pamr_affinity_reference` once, `pamr_iterate_reference` `iters` >= 1 times, then per pixel the first maximum over the
    classes and its value.  Upstream also resizes the mask to the image (align_corners=True); here the values arrive at image
    resolution by `seg_predict`'s own rule, so that step does not exist.  Runs on any device."""
    assert iters >= 1, iters
    w = pamr_affinity_reference(image, dilations, dtype)
    m = m.to(dtype)
    for _ in range(iters):
        m = pamr_iterate_reference(w, m, dilations)
    labels = m.argmax(dim=0)
    return labels, m.gather(0, labels[None]).squeeze(0), m


def areas_reference(labels, gt, n, raw_labels=True):
    """Specification of the scoring counters (hip.seg_areas, hip.seg_score, hip.seg_score_views): labels integer [..., h, w]
    (predicted classes), gt uint8 / int16 of the same shape -> (areas int64 [3, n], tally int64 [2]).

    Ground truth, raw_labels=True (augment.remap_label's rule, segmentation_dataset.py:231-233): raw 0 and raw 255 are ignored,
    any other x is class x - 1.  raw_labels=False: the value is the class id, n ('unknown') and 255 are ignored.  A class id
    outside [0, n) that is not an ignore value is out of range: not scored, counted in tally[1].  tally[0] is the number of
    scored pixels; over those only (seg_criterion.py:306-314 drops masked pixels from the prediction histogram too, :349-362)
    areas[0][c] = #(pred = c and gt = c), areas[1][c] = #(pred = c), areas[2][c] = #(gt = c).  A predicted label outside
    [0, n) on a scored pixel is in no bin of areas[0] and areas[1].  Runs on any device."""
    pred, cls, tally = _scored_pixels("areas_reference", labels, gt, n, raw_labels)
    known = (pred >= 0) & (pred < n)
    areas = torch.stack([torch.bincount(pred[known & (pred == cls)], minlength=n), torch.bincount(pred[known], minlength=n),
                         torch.bincount(cls, minlength=n)])
    return areas, tally


def _scored_pixels(what, labels, gt, n, raw_labels):
    """the ground-truth rule of `areas_reference` -> (the predicted labels and the classes of the scored pixels, int64
    [tally[0]] each, and tally)"""
    pred, cls, scored, tally = _scored_mask(what, labels, gt, n, raw_labels)
    return pred[scored], cls[scored], tally


def _scored_mask(what, labels, gt, n, raw_labels):
    """the ground-truth rule of `areas_reference`, its one statement -> (the predicted labels and the classes of ALL pixels,
    int64 [pixels] each, which of them are scored, bool [pixels], and tally)"""
    labels, gt = torch.as_tensor(labels), torch.as_tensor(gt)
    if gt.dtype not in (torch.uint8, torch.int16):
        raise ValueError("%s: ground truth must be uint8 or int16, got %s" % (what, gt.dtype))
    if labels.dtype.is_floating_point or labels.dtype == torch.bool or labels.shape != gt.shape:
        raise ValueError("%s: labels must be integer and of the ground truth's shape %s, got %s %s"
                         % (what, tuple(gt.shape), labels.dtype, tuple(labels.shape)))
    pred, g = labels.reshape(-1).long(), gt.reshape(-1).long().to(labels.device)
    ignored = (g == 0) | (g == 255) if raw_labels else (g == n) | (g == 255)
    cls = g - 1 if raw_labels else g
    in_range = (cls >= 0) & (cls < n)
    scored = ~ignored & in_range
    tally = torch.stack([scored.sum(), (~ignored & ~in_range).sum()])
    return pred, cls, scored, tally


def confusion_reference(labels, gt, n, raw_labels=True):
    """Specification of the confusion matrix (hip.seg_confusion): labels and gt as in `areas_reference`, whose ground-truth rule
    and set of scored pixels these are -> int64 [n, n + 1].  A scored pixel of ground-truth class c with predicted label p adds
    1 to C[c, p] where 0 <= p < n, else to C[c, n], the "outside" column (255 in a uint8 map of another source, a negative
    int16).  With (areas, tally) of the same inputs: C.sum() == tally[0], C[:, :n].diagonal() == areas[0],
    C[:, :n].sum(0) == areas[1], C.sum(1) == areas[2].  Runs on any device."""
    pred, cls, _ = _scored_pixels("confusion_reference", labels, gt, n, raw_labels)
    col = torch.where((pred >= 0) & (pred < n), pred, torch.full_like(pred, n))
    return torch.bincount(cls * (n + 1) + col, minlength=n * (n + 1)).reshape(n, n + 1)


def boundary_distance(h, w, ratio=0.02):
    """The half width of Boundary IoU's band for an h x w image: `ratio` of the diagonal, rounded, 1 at least -- upstream's
    line in `mask_to_boundary`.  Evaluated on the host in float64; the kernel only ever sees the integer."""
    return max(1, int(round(ratio * math.sqrt(h * h + w * w))))


def _in_band(v, d):
    """v int64 [N, h, w] -> bool [N, h, w]: some position within |dx| <= d and |dy| <= d lies outside the image or carries
    another value.  Separable: the window's minimum and maximum inside the image (a row pass, then a column pass; the pooling's
    padding is -inf, so positions outside the image take no part) differ, or the window leaves the image."""
    h, w = v.shape[-2:]
    f = v.double()[:, None]                       # exact up to 2^53

    def window_max(t):
        return F.max_pool2d(F.max_pool2d(t, (1, 2 * d + 1), 1, (0, d)), (2 * d + 1, 1), 1, (d, 0))

    differs = (window_max(f) != -window_max(-f))[:, 0]
    y, x = torch.arange(h, device=v.device)[:, None], torch.arange(w, device=v.device)[None, :]
    return differs | (y < d) | (y >= h - d) | (x < d) | (x >= w - d)


def boundary_areas_reference(labels, gt, n, d, raw_labels=True):
    """Specification of Boundary IoU's counters (hip.seg_boundary_areas; Cheng et al., CVPR 2021, in its semantic-segmentation
    form, per-class band areas summed over the data set): labels and gt [..., h, w] as in `areas_reference`, whose ground-truth
    rule and set of scored pixels these are; d an int >= 1 -> (bareas int64 [3, n], band uint8 of the maps' shape).

    A pixel p of a map is in the band of that map iff some position q with |dx| <= d and |dy| <= d either lies outside the
    image or carries a different value than p.  Values are compared as they are: the ground truth's raw values, so an ignore
    value is a value of its own, and the labels, so a label outside [0, n) is a value of its own.  That is upstream's
    `mask_to_boundary` (a zero border, d iterations of a 3 x 3 erosion, mask - eroded) applied to every class mask at once.
    Over the scored pixels only: bareas[2][c] = #(gt class c and in the gt band), bareas[1][c] = #(pred = c and in the pred
    band), bareas[0][c] = #(gt class = pred = c and in both bands); a predicted label outside [0, n) is in no bin of rows 0
    and 1.  band: bit 0 = in the gt band, bit 1 = in the pred band, for EVERY pixel, scored or not.  With d >= max(h, w)
    every pixel is in both bands and bareas is `areas_reference`'s areas.

    NOT pinned: upstream's code (`boundary_iou`, on `cv2`) is not available where this is tested, and its handling of ignore
    labels is not reproduced from it; the rule above is this project's statement, held against a literal transcription of
    `mask_to_boundary` class by class.  Runs on any device."""
    if not isinstance(d, int) or isinstance(d, bool) or d < 1:
        raise ValueError("boundary_areas_reference: d must be an int >= 1 (the band's half width in pixels), got %r" % (d,))
    pred, cls, scored, _ = _scored_mask("boundary_areas_reference", labels, gt, n, raw_labels)
    shape = torch.as_tensor(gt).shape
    if len(shape) < 2:
        raise ValueError("boundary_areas_reference: the maps must be [..., h, w], got %s" % (tuple(shape),))
    maps = (-1,) + tuple(shape[-2:])
    gb = _in_band(torch.as_tensor(gt).to(pred.device).long().reshape(maps), d).reshape(-1)
    pb = _in_band(pred.reshape(maps), d).reshape(-1)
    known = scored & (pred >= 0) & (pred < n)
    bareas = torch.stack([torch.bincount(pred[known & (pred == cls) & gb & pb], minlength=n),
                          torch.bincount(pred[known & pb], minlength=n), torch.bincount(cls[scored & gb], minlength=n)])
    return bareas, (gb.to(torch.uint8) | (pb.to(torch.uint8) << 1)).reshape(shape)


def default_trimap_radii():
    """the radii of the trimap curve where none are given: the band widths the DeepLab / PointRend / SegFix tables use, doubled
    up to 32 pixels"""
    return (1, 2, 4, 8, 16, 32)


def _max_distance(what, max_distance):
    if not isinstance(max_distance, int) or isinstance(max_distance, bool) or not 1 <= max_distance <= hip.SEG_DISTANCE_MAX:
        raise ValueError("%s: max_distance must be an int in 1 .. %d (the largest distance told apart, in pixels), got %r"
                         % (what, hip.SEG_DISTANCE_MAX, max_distance))
    return max_distance


def _trimap_radii(what, radii, name="radii"):
    """the radii of a trimap curve, checked -> a tuple of 1 .. 8 strictly ascending ints in 1 .. 128"""
    ok = isinstance(radii, (tuple, list)) and 1 <= len(radii) <= hip.SEG_TRIMAP_MAX_RADII \
        and all(isinstance(r, int) and not isinstance(r, bool) and 1 <= r <= hip.SEG_DISTANCE_MAX for r in radii) \
        and all(a < b for a, b in zip(radii, radii[1:]))
    if not ok:
        raise ValueError("%s: %s must be 1 .. %d strictly ascending ints in 1 .. %d (the trimap's band widths in pixels), got %r"
                         % (what, name, hip.SEG_TRIMAP_MAX_RADII, hip.SEG_DISTANCE_MAX, radii))
    return tuple(radii)


def distance_reference(labels, max_distance, border=False):
    """Specification of the exact squared Euclidean distance to the nearest pixel of another value (hip.seg_distance): labels
    uint8 / int16 [H, W] or [B, H, W], R = max_distance an int in 1 .. 128 -> uint16 of the labels' shape.

    With D2(p) = min over q of (px - qx)^2 + (py - qy)^2 over the pixels q of the SAME image with L(q) != L(p) -- values are
    compared as they are: 255, a negative int16, anything outside [0, n) is a value of its own, as in
    `boundary_areas_reference` and `regions_reference` -- and, with `border`, over every position q outside the image as
    well (so D2 <= min(x + 1, W - x, y + 1, H - y)^2): the output is D2(p) where D2(p) <= R^2 and 65535
    (`hip.SEG_DISTANCE_FAR`) where D2(p) > R^2 or no such q exists.  Distances never cross from one image of a batch into the
    next.  For border=False this is `scipy.ndimage.distance_transform_edt(L == c)` squared at the pixels of every value c.

    Evaluated one axis after the other, each by looking at every offset in -R .. R: v(x, y) = the least |dy| at which column
    x holds another value (or leaves the image, with `border`), then D2 = min over dx of dx^2 + (0 where row y holds another
    value at x + dx, or leaves the image with `border`; v(x + dx, y)^2 where it holds the same value).  An offset beyond the
    image's own extent on its axis reaches nothing new (every position there is outside) and is left out.  Runs on any
    device."""
    R = _max_distance("distance_reference", max_distance)
    labels = torch.as_tensor(labels)
    if labels.dtype not in (torch.uint8, torch.int16) or labels.dim() not in (2, 3) or labels.numel() == 0:
        raise ValueError("distance_reference: labels must be a uint8 or int16 map [H, W] or [B, H, W], got %s %s"
                         % (labels.dtype, tuple(labels.shape)))
    L = labels.long().reshape((-1,) + tuple(labels.shape[-2:]))
    H, W = L.shape[-2:]
    OUT, NONE = 1 << 20, 1 << 24                  # no label value; no distance (its square stays below 2^63)
    Ry, Rx = min(R, H), min(R, W)
    Lp = F.pad(L, (Rx, Rx, Ry, Ry), value=OUT)
    v = torch.full_like(L, NONE)
    for k in range(1, Ry + 1):
        for s in (-k, k):
            nb = Lp[:, Ry + s:Ry + s + H, Rx:Rx + W]
            differs = (nb != L) if border else (nb != L) & (nb != OUT)
            v = torch.where(differs & (v == NONE), torch.full_like(v, k), v)
    vp = F.pad(v, (Rx, Rx), value=NONE)
    best = v * v
    for k in range(1, Rx + 1):
        for s in (-k, k):
            nb = Lp[:, Ry:Ry + H, Rx + s:Rx + s + W]
            differs = (nb != L) if border else (nb != L) & (nb != OUT)
            side = vp[:, :, Rx + s:Rx + s + W]
            best = torch.minimum(best, torch.where(differs, torch.full_like(best, k * k), k * k + side * side))
    # 65535 as the int16 of the same bits: torch.uint16 holds it, int16 carries it there
    far = torch.where(best <= R * R, best, torch.full_like(best, hip.SEG_DISTANCE_FAR))
    return far.to(torch.int32).to(torch.uint16).reshape(labels.shape)


def trimap_areas_reference(labels, gt, n, radii, raw_labels=True, border=False, dist=None):
    """Specification of the trimap counters (hip.seg_trimap_areas): labels and gt [H, W] or [B, H, W] as in
    `areas_reference`, whose ground-truth rule and set of scored pixels these are; radii a tuple of 1 .. 8 strictly ascending
    ints in 1 .. 128 -> int64 [K, 3, n].

    With d2 = `distance_reference(gt, radii[-1], border)` of the GROUND TRUTH -- its raw values, so an ignore value is a value
    of its own for the distance, as for Boundary IoU's band, and is never scored -- ring k holds the pixels with
    r_{k-1}^2 < d2 <= r_k^2 (r_{-1} = 0), and out[k] is the three rows of `areas_reference` (intersect / predicted / label)
    restricted to ring k.  The rings are disjoint: the counters add across images, and the figures
    (`SegmentationScore.summary`) use their cumulative sum over k, the pixels within r_k of a ground-truth contour.
    dist: that plane where the caller has it -- as `hip.seg_trimap_areas` takes it, of any max_distance >= radii[-1], which
    puts the same pixels into the same rings.

    NOT pinned: no upstream trimap code is available where this is tested.  DeepLab's trimap is a dilation of VOC's void band;
    this rule is the Euclidean distance to a pixel of another ground-truth value.  Runs on any device."""
    radii = _trimap_radii("trimap_areas_reference", radii)
    pred, cls, scored, _ = _scored_mask("trimap_areas_reference", labels, gt, n, raw_labels)
    if dist is None:
        dist = distance_reference(torch.as_tensor(gt), radii[-1], border)
    elif not torch.is_tensor(dist) or dist.dtype != torch.uint16 or dist.shape != torch.as_tensor(gt).shape:
        raise ValueError("trimap_areas_reference: dist must be a uint16 plane of the ground truth's shape %s, got %s"
                         % (tuple(torch.as_tensor(gt).shape), (dist.dtype, tuple(dist.shape)) if torch.is_tensor(dist) else type(dist)))
    d2 = dist.to(pred.device).reshape(-1).long()
    known = scored & (pred >= 0) & (pred < n)
    out, lo = [], 0
    for r in radii:
        ring = (d2 > lo) & (d2 <= r * r)
        out.append(torch.stack([torch.bincount(pred[known & (pred == cls) & ring], minlength=n),
                                torch.bincount(pred[known & ring], minlength=n), torch.bincount(cls[scored & ring], minlength=n)]))
        lo = r * r
    return torch.stack(out)


class RenderResult(NamedTuple):
    picture: torch.Tensor                      # [H, W, 3] uint8: the labels' colours over the image, on the device
    labels: torch.Tensor                       # [H, W] uint8 / int16: what `segment_raw` gave
    conf: Optional[torch.Tensor]               # [H, W] fp32 with fade_by_conf, else None


def default_palette(n):
    """-> uint8 [n, 3]: the PASCAL-VOC colour map (bit 7 - j of red, green, blue from bits 3 j, 3 j + 1, 3 j + 2 of the index)
    with the loop run over all eight rounds of three index bits, so that it is one-to-one beyond 256 classes as well:
    0 -> (0, 0, 0), 1 -> (128, 0, 0), 255 -> (224, 224, 192), 256 -> (0, 0, 32)."""
    idx = torch.arange(int(n), dtype=torch.int64)
    rgb = torch.zeros(int(n), 3, dtype=torch.int64)
    for j in range(8):
        for c in range(3):
            rgb[:, c] |= ((idx >> (3 * j + c)) & 1) << (7 - j)
    return rgb.to(torch.uint8)


def _boundary_ratio(what, ratio):
    """the share of the diagonal that Boundary IoU's band is wide, checked -> float"""
    if isinstance(ratio, bool) or not isinstance(ratio, (int, float)) or not 0.0 < ratio < 1.0:
        raise ValueError("%s: the boundary ratio must be a number in (0, 1), the band's half width as a share of the image "
                         "diagonal, got %r" % (what, ratio))
    return float(ratio)


def _boundary_arg(what, boundary, band="ignore band"):
    if not isinstance(boundary, int) or isinstance(boundary, bool) or not 0 <= boundary <= hip.SEG_RENDER_MAX_BOUNDARY:
        raise ValueError("%s: boundary must be an int in 0 .. %d (the %s's half width in pixels), got %r"
                         % (what, hip.SEG_RENDER_MAX_BOUNDARY, band, boundary))
    return boundary


def _label_edges(lab, r):
    """labels [..., H, W] -> bool of the same shape: some pixel INSIDE the image with |dx| <= r and |dy| <= r carries a different
    label value (the contour of `render_reference`, the ignore band of `pseudo_label_reference`)"""
    H, W = lab.shape[-2:]
    edge = torch.zeros(lab.shape, dtype=torch.bool, device=lab.device)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if abs(dy) >= H or abs(dx) >= W:
                continue                                   # no pixel of the image has this neighbour
            here = (slice(max(-dy, 0), H - max(dy, 0)), slice(max(-dx, 0), W - max(dx, 0)))
            there = (slice(max(dy, 0), H - max(-dy, 0)), slice(max(dx, 0), W - max(-dx, 0)))
            edge[(..., *here)] |= lab[(..., *here)] != lab[(..., *there)]
    return edge


def _render_args(what, opacity, boundary, boundary_color):
    """the scalar arguments of a rendering call, checked on the host -> (alpha in 0..256, r, the contour colour as three ints)"""
    if not isinstance(opacity, (int, float)) or not 0.0 <= opacity <= 1.0:
        raise ValueError("%s: opacity must be a number in [0, 1], got %r" % (what, opacity))
    boundary = _boundary_arg(what, boundary, "contour")
    color = tuple(boundary_color)
    if len(color) != 3 or any(not isinstance(c, int) or not 0 <= c <= 255 for c in color):
        raise ValueError("%s: boundary_color must be three ints in 0 .. 255, got %r" % (what, boundary_color))
    return int(float(opacity) * 256.0 + 0.5), boundary, color


def render_reference(labels, image, palette, opacity=0.5, boundary=0, boundary_color=(255, 255, 255), conf=None):
    """CPU specification of hip.seg_render, in integers: labels integer [H, W] (or [B, H, W]), image uint8 [.., H, W, 3],
    palette uint8 [n, 3] -> the picture uint8 [.., H, W, 3].

      alpha = floor(opacity * 256 + 0.5), 0 .. 256 (opacity outside [0, 1]: ValueError); with conf (fp32, labels' shape) the
              pixel's own  a = (alpha q + 127) // 255,  q = clamp(floor(conf * 255 + 0.5), 0, 255) in fp32, NaN -> 0
      a pixel with 0 <= label < n:  (image (256 - a) + palette[label] a) >> 8  per channel
      any other label (255 "ignore", a negative int16):  the image's pixel
      boundary = r, 0 .. 4:  a pixel for which some pixel INSIDE the image with |dx| <= r and |dy| <= r carries a different
              raw label value becomes `boundary_color`, unblended, whatever its own label; r = 0: no contours

    opacity 0.5 is the reference demo's `(image * 0.5 + cmap[labels] * 0.5).astype(uint8)` bit for bit ("overlap"), 1.0 its
    `cmap[labels]` ("segmentation"); at any other opacity the rule is within one grey level of the float64 formula."""
    alpha, r, color = _render_args("render_reference", opacity, boundary, boundary_color)
    labels, image, palette = torch.as_tensor(labels), torch.as_tensor(image), torch.as_tensor(palette)
    if labels.dtype.is_floating_point or labels.dtype == torch.bool or labels.dim() not in (2, 3):
        raise ValueError("render_reference: labels must be integer [H, W] or [B, H, W], got %s %s" % (labels.dtype, tuple(labels.shape)))
    if image.dtype != torch.uint8 or tuple(image.shape) != tuple(labels.shape) + (3,):
        raise ValueError("render_reference: image must be uint8 %s, got %s %s"
                         % (tuple(labels.shape) + (3,), image.dtype, tuple(image.shape)))
    if palette.dtype != torch.uint8 or palette.dim() != 2 or palette.shape[1] != 3 or palette.shape[0] < 1:
        raise ValueError("render_reference: palette must be uint8 [n, 3], n >= 1, got %s %s" % (palette.dtype, tuple(palette.shape)))
    lab, img, n = labels.cpu().long(), image.cpu().int(), palette.shape[0]
    a = torch.full(lab.shape, alpha, dtype=torch.int32)
    if conf is not None:
        conf = torch.as_tensor(conf)
        if conf.dtype != torch.float32 or conf.shape != labels.shape:
            raise ValueError("render_reference: conf must be float32 %s, got %s %s" % (tuple(labels.shape), conf.dtype, tuple(conf.shape)))
        q = torch.floor(conf.cpu() * 255.0 + 0.5)
        q = torch.where(torch.isnan(q), torch.zeros_like(q), q).clamp(0.0, 255.0).int()
        a = (alpha * q + 127) // 255
    inside = (lab >= 0) & (lab < n)
    colour = palette.cpu().int()[lab.clamp(0, n - 1)]
    out = torch.where(inside[..., None], (img * (256 - a[..., None]) + colour * a[..., None]) >> 8, img)
    out = torch.where(_label_edges(lab, r)[..., None], torch.tensor(color, dtype=torch.int32), out)
    return out.to(torch.uint8)


CONF_BINS = hip.SEG_CONF_BINS


def conf_bin(conf):
    """fp32 confidences -> their histogram bin, int64 of the same shape: clamp(floor(conf * 256), 0, 255) evaluated in fp32
    (the product is exact), NaN -> 0 (the kernels' fmaxf(NaN, 0) = 0, as `render_reference`'s q), +inf -> 255.  Runs on any
    device."""
    conf = torch.as_tensor(conf)
    if conf.dtype != torch.float32:
        raise ValueError("conf_bin: conf must be float32, got %s" % conf.dtype)
    q = torch.floor(conf * 256.0)
    return torch.where(torch.isnan(q), torch.zeros_like(q), q).clamp(0.0, 255.0).long()


def _labels_conf(what, labels, conf, n):
    labels, conf = torch.as_tensor(labels), torch.as_tensor(conf)
    if labels.dtype.is_floating_point or labels.dtype == torch.bool:
        raise ValueError("%s: labels must be integer, got %s" % (what, labels.dtype))
    if conf.dtype != torch.float32 or conf.shape != labels.shape:
        raise ValueError("%s: conf must be float32 %s, got %s %s" % (what, tuple(labels.shape), conf.dtype, tuple(conf.shape)))
    if int(n) < 1:
        raise ValueError("%s: n = %d classes" % (what, n))
    return labels.long(), conf.to(labels.device)


def confidence_histogram_reference(labels, conf, n):
    """Specification of hip.seg_conf_hist: labels integer [...] (predicted classes), conf fp32 of the same shape ->
    (hist int64 [n, 256], tally int64 [2]): hist[c, b] = #(label = c and conf_bin(conf) = b), tally[0] = #labels in [0, n),
    tally[1] = #labels outside (255, a negative int16).  hist.sum() == tally[0].  Runs on any device."""
    lab, conf = _labels_conf("confidence_histogram_reference", labels, conf, n)
    lab, b = lab.reshape(-1), conf_bin(conf).reshape(-1)
    inside = (lab >= 0) & (lab < n)
    hist = torch.bincount(lab[inside] * CONF_BINS + b[inside], minlength=n * CONF_BINS).reshape(n, CONF_BINS)
    return hist, torch.stack([inside.sum(), (~inside).sum()])


def calibration_reference(labels, conf, gt, n, raw_labels=True):
    """Specification of hip.seg_calibration, the counts behind the reliability diagram and ECE (Guo et al., ICML 2017) per
    predicted class: labels integer [...] (predicted classes), conf fp32 and gt uint8 / int16 of the same shape ->
    (calibration int64 [n, 256, 2], tally int64 [2]).  The ground-truth rule and the set of scored pixels are
    `areas_reference`'s; over those only, calibration[l, b, hit] = #(label = l in [0, n), conf_bin(conf) = b,
    (l == gt class) = hit), tally[0] = #scored pixels with a label in [0, n), tally[1] = #scored pixels with a label outside.
    A pixel that is not scored (ignored ground truth, or ground truth outside the classes) is counted nowhere.  With (areas, _)
    of `areas_reference` on the same maps: calibration.sum((1, 2)) == areas[1], calibration[..., 1].sum(1) == areas[0],
    calibration.sum() == tally[0].  Runs on any device."""
    pred, cls, scored, _ = _scored_mask("calibration_reference", labels, gt, n, raw_labels)
    conf = torch.as_tensor(conf)
    if conf.dtype != torch.float32 or conf.shape != torch.as_tensor(labels).shape:
        raise ValueError("calibration_reference: conf must be float32 %s, got %s %s"
                         % (tuple(torch.as_tensor(labels).shape), conf.dtype, tuple(conf.shape)))
    if int(n) < 1:
        raise ValueError("calibration_reference: n = %d classes" % n)
    b = conf_bin(conf.to(pred.device)).reshape(-1)
    inside = scored & (pred >= 0) & (pred < n)
    key = (pred[inside] * CONF_BINS + b[inside]) * 2 + (pred[inside] == cls[inside]).long()
    calibration = torch.bincount(key, minlength=n * CONF_BINS * 2).reshape(n, CONF_BINS, 2)
    return calibration, torch.stack([inside.sum(), (scored & ~inside).sum()])


def _reliability_bins(cal, bins, per_class):
    """calibration counters int64 [n, 256, 2] -> (pixels, hits, confidence mass) float64 [n | 1, bins]: the fine bins summed
    in runs of 256 / bins, a fine bin's confidence being its midpoint (b + 0.5) / 256.  Exact: integers and multiples of 1/512
    far below 2^53"""
    c = cal.double() if per_class else cal.sum(0, keepdim=True).double()
    mid = (torch.arange(CONF_BINS, dtype=torch.float64, device=cal.device) + 0.5) / CONF_BINS
    fine = c.sum(-1)
    run = (c.shape[0], bins, CONF_BINS // bins)
    return fine.reshape(run).sum(-1), c[..., 1].reshape(run).sum(-1), (fine * mid).reshape(run).sum(-1)


def _calibration_errors(N, H, C):
    """(pixels, hits, confidence mass) [k, bins] -> (ECE, MCE) float64 [k]: sum_m (N_m / N) |acc_m - conf_m| and the largest
    gap over the non-empty bins; NaN without pixels"""
    total = N.sum(-1)
    gap = (H / N - C / N).abs()                                  # NaN where the bin is empty
    ece = torch.nansum(N * gap, -1) / total
    mce = torch.nan_to_num(gap, nan=-1.0).amax(-1)
    return ece, torch.where(total > 0, mce, torch.full_like(mce, float("nan")))


FLT_MIN = float(torch.finfo(torch.float32).tiny)          # 2^-126: the smallest normal fp32, C's FLT_MIN
MAX_TEMPERATURES = hip.SEG_SWEEP_MAX_TEMPERATURES


def default_temperatures():
    """the 16 temperatures a sweep tries by default: 2^(j/4), j = -7 .. 8 -- 0.297 to 4.0 in quarter octaves, with 1.0 (the
    model as it is) and 2.0 on the grid"""
    return tuple(2 ** (j / 4) for j in range(-7, 9))


def _check_temperatures(what, temperatures):
    """the temperature list of a sweep, checked -> a tuple of 1 .. 16 floats, each finite and > 0"""
    try:
        ts = tuple(temperatures)
    except TypeError:
        raise ValueError("%s: temperatures must be a sequence of numbers, got %r" % (what, temperatures))
    if not 1 <= len(ts) <= MAX_TEMPERATURES:
        raise ValueError("%s: temperatures must hold 1 .. %d values (one launch scores them all), got %d" % (what, MAX_TEMPERATURES, len(ts)))
    for t in ts:
        if isinstance(t, bool) or not isinstance(t, (int, float)) or not math.isfinite(t) or t <= 0:
            raise ValueError("%s: every one of temperatures must be a finite number > 0, got %r" % (what, t))
    return tuple(float(t) for t in ts)


def _check_label_maps(what, imgs, label_maps):
    """the ground truth of `evaluate_raw` / `calibrate_raw`, checked against the images [H_i, W_i, 3] -> the maps as a list"""
    gts = [label_maps] if torch.is_tensor(label_maps) else list(label_maps)
    if len(gts) != len(imgs):
        raise ValueError("%s: %d label maps for %d images" % (what, len(gts), len(imgs)))
    for i, (im, g) in enumerate(zip(imgs, gts)):
        if not torch.is_tensor(g) or g.dtype not in (torch.uint8, torch.int16) or tuple(g.shape) != tuple(im.shape[:2]):
            raise ValueError("%s: label map %d must be a uint8 or int16 tensor of its image's shape %s, got %s"
                             % (what, i, tuple(im.shape[:2]), (g.dtype, tuple(g.shape)) if torch.is_tensor(g) else type(g)))
    return gts


def _check_batch_gt(what, images, label_maps):
    """the ground truth of `evaluate` / `calibrate`, checked against the batch -> it as [B, h, w]"""
    gt = label_maps
    if not torch.is_tensor(gt) or gt.dtype not in (torch.uint8, torch.int16) or gt.dim() not in (2, 3) or gt.numel() == 0:
        raise ValueError("%s: label_maps must be a uint8 or int16 tensor [B, h, w], got %s"
                         % (what, (gt.dtype, tuple(gt.shape)) if torch.is_tensor(gt) else type(gt)))
    gt = gt[None] if gt.dim() == 2 else gt
    if torch.is_tensor(images) and images.dim() >= 3 and gt.shape[0] != (1 if images.dim() == 3 else images.shape[0]):
        raise ValueError("%s: %d label maps for images %s" % (what, gt.shape[0], tuple(images.shape)))
    return gt


def temperature_sweep_from_probs(probs_k, gt, n, raw_labels=True):
    """The scoring half of `temperature_sweep_reference`, starting from values at image resolution: probs_k a sequence of K
    floating tensors [B, n, h, w] (every class's value per pixel under temperature k: `upsample_argmax_reference`'s or
    `hip.seg_predict`'s `probs`), gt uint8 / int16 [B, h, w] -> (hist int64 [K, 256, 2], sums float64 [K, 2], tally int64 [2]).

    Per k: l = the first maximum over the classes, conf = its value.  The ground-truth rule and the set of scored pixels are
    `areas_reference`'s; tally[0] = #scored pixels, tally[1] = #pixels with a ground truth out of range; a pixel that is not
    scored contributes nowhere.  Over the scored pixels, t the true class and p the values AS GIVEN, taken to float64:
      hist[k, conf_bin(conf), l == t] += 1          (conf rounded to fp32 first where the values are wider)
      sums[k, 0] += -log(max(p_t, FLT_MIN))         NLL; a probability that underflowed to 0 costs 87.3, not infinity
      sums[k, 1] += sum_c p_c^2 - 2 p_t + 1         Brier, = sum_c (p_c - onehot_c)^2; every product and sum in float64
    Runs on any device."""
    what = "temperature_sweep_from_probs"
    probs_k = list(probs_k)
    if not probs_k:
        raise ValueError("%s: no temperatures" % what)
    gt = torch.as_tensor(gt)
    hist, sums, tally = [], [], None
    for k, probs in enumerate(probs_k):
        if not torch.is_tensor(probs) or not probs.dtype.is_floating_point or probs.dim() != 4 or probs.shape[1] != n \
                or (probs.shape[0],) + tuple(probs.shape[2:]) != tuple(gt.shape):
            raise ValueError("%s: values %d must be floating [B, %d, h, w] for a ground truth [B, h, w] = %s, got %s" % (
                what, k, n, tuple(gt.shape), (probs.dtype, tuple(probs.shape)) if torch.is_tensor(probs) else type(probs)))
        labels = probs.argmax(dim=1)
        lab, cls, scored, tally = _scored_mask(what, labels, gt, n, raw_labels)
        p = probs.permute(0, 2, 3, 1).reshape(-1, n)[scored]
        lab, t = lab[scored], cls[scored]
        conf = p.gather(1, lab[:, None])[:, 0]
        pt = p.gather(1, t[:, None])[:, 0].double()
        key = conf_bin(conf.float()) * 2 + (lab == t).long()
        hist.append(torch.bincount(key, minlength=CONF_BINS * 2).reshape(CONF_BINS, 2))
        pd = p.double()
        sums.append(torch.stack([-(pt.clamp_min(FLT_MIN).log()).sum(), ((pd * pd).sum(1) - 2.0 * pt + 1.0).sum()]))
    return torch.stack(hist), torch.stack(sums), tally


def temperature_sweep_reference(grids, hp, wp, gt, raw_labels=True, dtype=torch.float64):
    """Specification of hip.seg_temperature_sweep: grids [K, B, hp*wp, n] (or a sequence of K [B, hp*wp, n]), class fastest --
    K grids of class PROBABILITIES of the same images, one forward's logits softmaxed at K temperatures; gt uint8 / int16
    [B, h, w] -> (hist int64 [K, 256, 2], sums float64 [K, 2], tally int64 [2]).  Per k the grid is resized to gt's (h, w) by
    `upsample_argmax_reference` (bilinear, align_corners=False, evaluated in `dtype`), and `temperature_sweep_from_probs`
    scores the K results: per temperature the reliability counts of all classes together -- row k is
    `calibration_reference(labels_k, conf_k, gt, n)[0].sum(0)` -- and the two proper scores a temperature is fitted on (Guo et
    al., ICML 2017), summed over the scored pixels.  The kernel interpolates in fp32 (`hip.seg_predict`'s values, bit for
    bit); this is the fp64 statement it is held against.  Runs on any device."""
    gt = torch.as_tensor(gt)
    if gt.dim() != 3:
        raise ValueError("temperature_sweep_reference: the ground truth must be [B, h, w], got %s" % (tuple(gt.shape),))
    h, w = int(gt.shape[1]), int(gt.shape[2])
    grids = list(grids)
    if not grids:
        raise ValueError("temperature_sweep_reference: no temperatures")
    n = int(grids[0].shape[-1])
    return temperature_sweep_from_probs([upsample_argmax_reference(g, hp, wp, h, w, dtype)[2] for g in grids], gt, n, raw_labels)


class TemperatureSweep:
    """`temperature_sweep_reference`'s counters on the device, summed over everything swept into them: for the K temperatures
    `temperatures` (a tuple of floats), `hist` int64 [K, 256, 2] (confidence bin, hit), `sums` float64 [K, 2] (NLL, Brier;
    sums over the scored pixels) and `tally` int64 [2].  `hip.seg_temperature_sweep` adds to these tensors in place, so one
    sweep can span a validation set (`Segmenter.calibrate_raw(..., into=sweep)`).  n: the class count of what was swept
    (None: not known yet; `calibrate_raw` sets it)."""

    def __init__(self, temperatures, device=None, n=None):
        self.temperatures = _check_temperatures("TemperatureSweep", temperatures)
        K = len(self.temperatures)
        self.n = None if n is None else int(n)
        self.hist = torch.zeros(K, CONF_BINS, 2, dtype=torch.int64, device=device)
        self.sums = torch.zeros(K, 2, dtype=torch.float64, device=device)
        self.tally = torch.zeros(2, dtype=torch.int64, device=device)

    def add_(self, other):
        if tuple(other.temperatures) != self.temperatures:
            raise ValueError("TemperatureSweep.add_: temperatures %r against %r: sweeps of different lists do not add"
                             % (other.temperatures, self.temperatures))
        if self.n is not None and other.n is not None and self.n != other.n:
            raise ValueError("TemperatureSweep.add_: %d classes against %d" % (other.n, self.n))
        self.n = other.n if self.n is None else self.n
        self.hist += other.hist.to(self.hist.device)
        self.sums += other.sums.to(self.sums.device)
        self.tally += other.tally.to(self.tally.device)
        return self

    def _bins(self, what, bins):
        if not isinstance(bins, int) or isinstance(bins, bool) or bins < 1 or CONF_BINS % bins:
            raise ValueError("TemperatureSweep.%s: bins must be an int that divides %d, got %r" % (what, CONF_BINS, bins))
        return _reliability_bins(self.hist, bins, True)

    def reliability(self, k, bins=16):
        """row k's reliability diagram -> (pixels int64, accuracy float64, confidence float64), each [bins], as
        `SegmentationScore.reliability` gives them for all classes together.  Not synchronising."""
        if not isinstance(k, int) or isinstance(k, bool) or not 0 <= k < len(self.temperatures):
            raise ValueError("TemperatureSweep.reliability: k must be an int in 0 .. %d, got %r" % (len(self.temperatures) - 1, k))
        N, H, C = self._bins("reliability", bins)
        return N[k].long(), H[k] / N[k], C[k] / N[k]

    def summary(self):
        """-> {"temperatures": [K], "NLL": [K], "Brier": [K] (means per scored pixel), "ECE": [K], "MCE": [K] (16 bins, as
        `SegmentationScore.summary`), "aAcc": [K], "pixels", "best"}: float64 from the counters, not rounded; NaN (and best
        None) without pixels.  "best" is the temperature of lowest mean NLL, the first one on a tie.  The one place that
        synchronises with the host.  Ground truth out of range is an IndexError, as in `SegmentationScore.summary`."""
        K = len(self.temperatures)
        ece, mce = _calibration_errors(*self._bins("summary", 16))
        h = self.hist.double()
        flat = torch.cat([self.sums.reshape(-1), ece, mce, h[..., 1].sum(1) / h.sum((1, 2)), self.tally.double()]).tolist()
        pixels, bad = int(flat[5 * K]), int(flat[5 * K + 1])
        if bad != 0:
            raise IndexError("TemperatureSweep: tally[1] = %d ground-truth pixels hold a class outside [0, n) that is not an "
                             "ignore value (wrong raw_labels, or a label map of another dataset?)" % bad)
        nan = float("nan")
        nll = [flat[2 * k] / pixels if pixels else nan for k in range(K)]
        best = min(range(K), key=lambda k: nll[k]) if pixels else None          # min keeps the first of equal values
        return {"temperatures": list(self.temperatures), "NLL": nll,
                "Brier": [flat[2 * k + 1] / pixels if pixels else nan for k in range(K)],
                "ECE": flat[2 * K:3 * K], "MCE": flat[3 * K:4 * K], "aAcc": flat[4 * K:5 * K], "pixels": pixels,
                "best": None if best is None else self.temperatures[best]}

    def best(self):
        """the temperature of lowest mean NLL over what was swept, the first one on a tie (`summary()["best"]`: one host round
        trip, and `summary`'s IndexError); a ValueError without scored pixels.  Then: `seg.temperature = sweep.best()`."""
        best = self.summary()["best"]
        if best is None:
            raise ValueError("TemperatureSweep.best: no scored pixels have been swept")
        return best


MAX_BIAS_STRENGTHS = hip.SEG_SCORE_GRIDS_MAX


def default_bias_strengths():
    """the 16 strengths a bias sweep tries by default: j / 4, j = 0 .. 15 -- 0 (the Segmenter as it is) to 3.75 logit units per
    unit of the direction"""
    return tuple(j / 4 for j in range(16))


def _check_strengths(what, strengths):
    """the strength list of a bias sweep, checked -> a tuple of 1 .. 16 finite floats"""
    try:
        gs = tuple(strengths)
    except TypeError:
        raise ValueError("%s: strengths must be a sequence of numbers, got %r" % (what, strengths))
    if not 1 <= len(gs) <= MAX_BIAS_STRENGTHS:
        raise ValueError("%s: strengths must hold 1 .. %d values (one launch scores them all), got %d" % (what, MAX_BIAS_STRENGTHS, len(gs)))
    for g in gs:
        if isinstance(g, bool) or not isinstance(g, (int, float)) or not math.isfinite(g):
            raise ValueError("%s: every one of strengths must be a finite number, got %r" % (what, g))
    return tuple(float(g) for g in gs)


def _check_bias(what, name, v, n, device=None):
    """a per-class vector in logit units (`class_bias`, a sweep's direction or origin), checked -> fp32 [n] on `device`: a
    tensor or a sequence of n finite numbers; anything else is a ValueError naming it"""
    try:
        if isinstance(v, (str, bytes)) or (torch.is_tensor(v) and (v.dtype == torch.bool or v.dtype.is_complex)):
            raise TypeError
        t = (v.detach() if torch.is_tensor(v) else torch.as_tensor(v)).to(device=device, dtype=torch.float32).contiguous()
    except (TypeError, ValueError, RuntimeError):
        raise ValueError("%s: %s must be a tensor or sequence of %d finite numbers, got %r" % (what, name, n, v))
    if tuple(t.shape) != (n,) or not bool(torch.isfinite(t).all()):
        raise ValueError("%s: %s must be a tensor or sequence of %d finite numbers, got %s"
                         % (what, name, n, "shape %s" % (tuple(t.shape),) if tuple(t.shape) != (n,) else "a value that is not finite"))
    return t.clone() if torch.is_tensor(v) and t.data_ptr() == v.data_ptr() else t


def scaled_bias(direction, strength, origin=None):
    """The one place a strength becomes a bias: direction.float() * fp32(strength), plus origin.float() where given -- one
    rounded product and one rounded sum, fp32 [n] on the direction's device.  `Segmenter.bias_sweep_raw` uses it for row k
    and `BiasSweep.bias` to hand out the winner, so the two agree bit for bit."""
    b = torch.as_tensor(direction).float() * torch.tensor(strength, dtype=torch.float32)
    return b if origin is None else b + torch.as_tensor(origin).float().to(b.device)


def first_maximum(values):
    """the label rule of the resizing kernels on values [B, n, h, w] -> int64 [B, h, w]: the smallest class of maximal value,
    `v > best` from -inf on -- a NaN never wins (torch.argmax would rank it first), and a pixel whose values are all NaN is
    class 0"""
    return torch.where(values.isnan(), torch.full_like(values, float("-inf")), values).argmax(dim=1)


def bias_sweep_reference(grids, hp, wp, gt, raw_labels=True, dtype=torch.float64):
    """Specification of hip.seg_score_grids: grids [K, B, hp*wp, n] (or a sequence of K [B, hp*wp, n]), class fastest -- K score
    grids of the same images holding ANY fp32 values (one forward's logits under K biases, softmaxed or not); gt uint8 / int16
    [B, h, w] -> (areas int64 [K, 3, n], tally int64 [2]).  Per k the grid is resized to gt's (h, w) by
    `upsample_argmax_reference` (bilinear, align_corners=False, evaluated in `dtype`), the label is `first_maximum` of the
    resized values (torch.argmax's, except that a NaN never wins), and `areas_reference` scores the labels: row k is by
    definition what `hip.seg_score(grids[k], hp, wp, gt, raw_labels)` counts.  tally does not depend on k.  The kernel
    interpolates in fp32 (`hip.seg_predict`'s values, bit for bit); this is the fp64 statement it is held against.  Runs on
    any device."""
    gt = torch.as_tensor(gt)
    if gt.dim() != 3:
        raise ValueError("bias_sweep_reference: the ground truth must be [B, h, w], got %s" % (tuple(gt.shape),))
    h, w = int(gt.shape[1]), int(gt.shape[2])
    grids = list(grids)
    if not grids:
        raise ValueError("bias_sweep_reference: no strengths")
    n = int(grids[0].shape[-1])
    areas, tally = [], None
    for g in grids:
        a, tally = areas_reference(first_maximum(upsample_argmax_reference(g, hp, wp, h, w, dtype)[2]), gt, n, raw_labels)
        areas.append(a)
    return torch.stack(areas), tally


class BiasSweep:
    """`bias_sweep_reference`'s counters on the device, summed over everything swept into them: for the K strengths
    `strengths` (a tuple of floats) of the bias direction `direction` from `origin` (fp32 [n] each, zeros for origin=None),
    `areas` int64 [K, 3, n] -- row k is `SegmentationScore.areas` of a Segmenter whose `class_bias` is
    `scaled_bias(direction, strengths[k], origin)` -- and `tally` int64 [2].  `hip.seg_score_grids` adds to these tensors in
    place, so one sweep can span a validation set (`Segmenter.bias_sweep_raw(..., into=sweep)`)."""

    def __init__(self, strengths, direction, origin=None, device=None):
        self.strengths = _check_strengths("BiasSweep", strengths)
        try:
            n = len(direction)
        except TypeError:
            n = 0
        if n < 1:
            raise ValueError("BiasSweep: direction must be a tensor or sequence of n >= 1 finite numbers, got %r" % (direction,))
        self.direction = _check_bias("BiasSweep", "direction", direction, n, device)
        self.n = n
        dev = self.direction.device
        self.origin = torch.zeros(self.n, dtype=torch.float32, device=dev) if origin is None \
            else _check_bias("BiasSweep", "origin", origin, self.n, dev)
        self.areas = torch.zeros(len(self.strengths), 3, self.n, dtype=torch.int64, device=dev)
        self.tally = torch.zeros(2, dtype=torch.int64, device=dev)

    def _same(self, strengths, direction, origin):
        """whether a sweep of these strengths, direction and origin (fp32 [n] on this sweep's device) counts what this one counts:
        equal strengths, bit-equal vectors"""
        bits = lambda t: t.view(torch.int32)
        return tuple(strengths) == self.strengths and direction.shape == self.direction.shape \
            and direction.device == self.direction.device and origin.device == self.direction.device \
            and torch.equal(bits(direction), bits(self.direction)) and torch.equal(bits(origin), bits(self.origin))

    def add_(self, other):
        if not isinstance(other, BiasSweep):
            raise ValueError("BiasSweep.add_: a BiasSweep is needed, got %s" % type(other))
        if other.n != self.n:
            raise ValueError("BiasSweep.add_: %d classes against %d" % (other.n, self.n))
        if other.areas.device != self.areas.device:
            raise ValueError("BiasSweep.add_: a sweep on %s against one on %s" % (other.areas.device, self.areas.device))
        if tuple(other.strengths) != self.strengths:
            raise ValueError("BiasSweep.add_: strengths %r against %r: sweeps of different lists do not add"
                             % (other.strengths, self.strengths))
        if not self._same(other.strengths, other.direction, other.origin):
            raise ValueError("BiasSweep.add_: the two sweeps' direction or origin differ: rows of different biases do not add")
        self.areas += other.areas
        self.tally += other.tally
        return self

    def _row(self, what, k):
        if not isinstance(k, int) or isinstance(k, bool) or not 0 <= k < len(self.strengths):
            raise ValueError("BiasSweep.%s: k must be an int in 0 .. %d, got %r" % (what, len(self.strengths) - 1, k))
        return k

    def score(self, k):
        """row k as a `SegmentationScore` ON the sweep's counters (shared memory, nothing copied): every summary that reads
        `areas` works on it -- `summary`, `group_summary`, `overprediction`, `logging_output`.  The sweep counts no confusion
        matrix, so `merged` and `confusions` answer with their ValueError, as on any score without one."""
        return SegmentationScore(self.n, areas=self.areas[self._row("score", k)], tally=self.tally)

    def bias(self, k_or_strength):
        """the fp32 [n] bias of a row, `scaled_bias(direction, strength, origin)`: an int names the row, a float one of
        `strengths`.  Then: `seg.class_bias = sweep.bias(sweep.best())`."""
        if isinstance(k_or_strength, int) and not isinstance(k_or_strength, bool):
            g = self.strengths[self._row("bias", k_or_strength)]
        elif isinstance(k_or_strength, float) and k_or_strength in self.strengths:
            g = k_or_strength
        else:
            raise ValueError("BiasSweep.bias: a row 0 .. %d (int) or one of the strengths %r (float) is needed, got %r"
                             % (len(self.strengths) - 1, self.strengths, k_or_strength))
        return scaled_bias(self.direction, g, self.origin)

    def summary(self, groups=None):
        """-> {"strengths": [K], "mIoU": [K], "mAcc": [K], "aAcc": [K], "IoU": [K][n], "pixels"} by `SegmentationScore.summary`'s
        formulas and rounding, row by row; with groups = {name: class ids} also name: {"mIoU": [K], "mAcc": [K]} and "hIoU":
        [K], `SegmentationScore.group_summary`'s.  The one place that synchronises with the host: one round trip.  Ground
        truth out of range is an IndexError, as in `SegmentationScore.summary`."""
        K, n = len(self.strengths), self.n
        names, ids = [], []
        for name in ([] if groups is None else list(groups)):
            c = torch.as_tensor(list(groups[name]), dtype=torch.long).reshape(-1)
            if name in ("hIoU", "strengths", "mIoU", "mAcc", "aAcc", "IoU", "pixels") or c.numel() == 0 or int(c.min()) < 0 \
                    or int(c.max()) >= n:
                raise ValueError("BiasSweep.summary: group %r must hold class ids in [0, %d) (and not carry the name of a figure), "
                                 "got %s" % (name, n, c.tolist()))
            names.append(name)
            ids.append(c)
        flat = torch.cat([self.areas.reshape(-1), self.tally]).cpu()
        pixels, bad = int(flat[-2]), int(flat[-1])
        if bad != 0:
            raise IndexError("BiasSweep: tally[1] = %d ground-truth pixels hold a class outside [0, %d) that is not an "
                             "ignore value (wrong raw_labels, or a label map of another dataset?)" % (bad, n))
        a = flat[:-2].reshape(K, 3, n).double()
        ai, ap, al = a[:, 0], a[:, 1], a[:, 2]
        iou, acc = ai / (ap + al - ai), ai / al
        r4 = lambda v: round(float(v), 4)
        out = {"strengths": list(self.strengths), "mIoU": [r4(torch.nanmean(row)) for row in iou],
               "mAcc": [r4(torch.nanmean(row)) for row in acc], "aAcc": [r4(v) for v in ai.sum(1) / ap.sum(1)],
               "IoU": [[r4(v) for v in row] for row in iou.tolist()], "pixels": pixels}
        if names:
            mious = [[torch.nanmean(row[c]) for c in ids] for row in iou]
            for j, (name, c) in enumerate(zip(names, ids)):
                out[name] = {"mIoU": [r4(m[j]) for m in mious], "mAcc": [r4(torch.nanmean(row[c])) for row in acc]}
            out["hIoU"] = []
            for m in mious:
                mi = torch.stack(m)
                out["hIoU"].append(r4(0.0 if bool((mi == 0).any()) else len(names) / (1.0 / mi).sum()))
        return out

    def best(self, metric="mIoU", groups=None):
        """the strength whose row has the highest `metric` of `summary(groups)` (the rounded figures), the first one on a tie;
        rows whose figure is NaN do not compete.  metric: "mIoU", "mAcc", "aAcc", or with `groups` "hIoU" or a group's name
        (its mIoU).  One host round trip, and `summary`'s IndexError; a ValueError without scored pixels.  Then:
        `seg.class_bias = sweep.bias(sweep.best())`."""
        plain = ("mIoU", "mAcc", "aAcc")
        if metric not in plain and (groups is None or (metric != "hIoU" and metric not in groups)):
            raise ValueError("BiasSweep.best: metric must be one of %r, or with groups 'hIoU' or a group's name, got %r"
                             % (plain, metric))
        s = self.summary(groups)
        vals = s[metric] if metric in plain or metric == "hIoU" else s[metric]["mIoU"]
        live = [k for k, v in enumerate(vals) if not math.isnan(v)]
        if not s["pixels"] or not live:
            raise ValueError("BiasSweep.best: no scored pixels have been swept")
        return self.strengths[max(live, key=lambda k: vals[k])]              # max keeps the first of equal values


def pseudo_thresholds(hist, keep=1.0, floor=0.0):
    """The per-class confidence thresholds of self-training from a confidence histogram int64 [n, 256] -> int32 [n], values in
    0 .. 256 (bins: a pixel of class c passes iff conf_bin(conf) >= t_c), on hist's device with no host round trip.  In integers:

      N_c = sum_b hist[c, b],  K_c = (N_c round(keep * 65536)) >> 16,  S_c(t) = sum_{b >= t} hist[c, b]
      q_c = #{t in 0 .. 255 : S_c(t) > K_c}: the smallest t that keeps at most the `keep` share of class c (a bin that ties is
            rejected whole); t_c = max(q_c, ceil(floor * 256))

    keep=1, floor=tau is the fixed threshold (every kept pixel has conf >= tau); keep < 1 the class-balanced one (CBST: the
    most confident share of every class, so rare classes are not starved by a global threshold); a class without pixels
    gets the floor.  keep or floor outside [0, 1]: ValueError."""
    import math
    if not isinstance(keep, (int, float)) or isinstance(keep, bool) or not 0.0 <= keep <= 1.0:
        raise ValueError("pseudo_thresholds: keep must be a number in [0, 1], got %r" % (keep,))
    if not isinstance(floor, (int, float)) or isinstance(floor, bool) or not 0.0 <= floor <= 1.0:
        raise ValueError("pseudo_thresholds: floor must be a number in [0, 1], got %r" % (floor,))
    if not torch.is_tensor(hist) or hist.dtype != torch.int64 or hist.dim() != 2 or hist.shape[1] != CONF_BINS:
        raise ValueError("pseudo_thresholds: hist must be int64 [n, %d], got %s" % (
            CONF_BINS, (hist.dtype, tuple(hist.shape)) if torch.is_tensor(hist) else type(hist)))
    K = (hist.sum(1) * int(round(float(keep) * 65536.0))) >> 16
    S = hist.flip(1).cumsum(1).flip(1)
    q = (S > K[:, None]).sum(1)
    return q.clamp_min(int(math.ceil(float(floor) * 256.0))).to(torch.int32)


def pseudo_label_reference(labels, conf, thresholds, n, boundary=0, raw_labels=True, weight=False):
    """Specification of hip.seg_pseudo, in integers: labels integer [H, W] (or [B, H, W]), conf fp32 of that shape, thresholds
    integer [n] (bins) -> (out uint8 [.., H, W], kept int64 [2, n]).  A pixel of label l is kept iff

      0 <= l < n,  conf_bin(conf) >= thresholds[l],  and with boundary = r (0 .. 4) no pixel INSIDE the image with |dx| <= r and
      |dy| <= r carries a different label value: `render_reference`'s contour predicate, on the labels given (the predicted
      ones), not on the filtered ones.

    A kept pixel becomes l + 1 with raw_labels (the label-PNG convention `augment.remap_label` undoes) or l without; every
    other pixel 255, which both conventions ignore.  kept[1, c] = #(label = c), kept[0, c] = those that were kept.
    n <= 254 with raw_labels, n <= 255 without (ValueError).  Runs on any device.
    weight=True: -> (out, kept, weight uint8 of out's shape), the per-pixel loss weight of the weighted criterion: 0 where
    the pixel was dropped, max(conf_bin(conf), 1) where it was kept."""
    r = _boundary_arg("pseudo_label_reference", boundary)
    lab, conf = _labels_conf("pseudo_label_reference", labels, conf, n)
    if lab.dim() not in (2, 3):
        raise ValueError("pseudo_label_reference: labels must be [H, W] or [B, H, W], got %s" % (tuple(lab.shape),))
    if n > hip.seg_pseudo_max_classes(raw_labels):
        raise ValueError("pseudo_label_reference: n = %d classes, the uint8 output holds at most %d with raw_labels=%s"
                         % (n, hip.seg_pseudo_max_classes(raw_labels), bool(raw_labels)))
    thr = torch.as_tensor(thresholds)
    if thr.dtype.is_floating_point or thr.dtype == torch.bool or tuple(thr.shape) != (n,):
        raise ValueError("pseudo_label_reference: thresholds must be integer [%d], got %s %s" % (n, thr.dtype, tuple(thr.shape)))
    thr = thr.long().to(lab.device)
    inside = (lab >= 0) & (lab < n)
    cls = lab.clamp(0, n - 1)
    keep = inside & ~_label_edges(lab, r) & (conf_bin(conf) >= thr[cls])
    out = torch.where(keep, cls + (1 if raw_labels else 0), torch.full_like(cls, 255)).to(torch.uint8)
    kept = torch.stack([torch.bincount(cls[keep], minlength=n), torch.bincount(cls[inside], minlength=n)])
    if weight:
        b = conf_bin(conf)
        return out, kept, torch.where(keep, b.clamp_min(1), torch.zeros_like(b)).to(torch.uint8)
    return out, kept


def _connectivity_arg(what, connectivity):
    if not isinstance(connectivity, int) or isinstance(connectivity, bool) or connectivity not in (4, 8):
        raise ValueError("%s: connectivity must be the int 4 or 8, got %r" % (what, connectivity))
    return connectivity


def _min_region_arg(what, min_region):
    if not isinstance(min_region, int) or isinstance(min_region, bool) or not 1 <= min_region < 2 ** 31:
        raise ValueError("%s: min_region must be an int in 1 .. 2**31 - 1 (1 drops nothing), got %r" % (what, min_region))
    return min_region


def _region_labels(what, labels):
    labels = torch.as_tensor(labels)
    if labels.dtype.is_floating_point or labels.dtype.is_complex or labels.dtype == torch.bool:
        raise ValueError("%s: labels must be integer, got %s" % (what, labels.dtype))
    if labels.dim() not in (2, 3) or labels.numel() < 1:
        raise ValueError("%s: labels must be [H, W] or [B, H, W] with at least one pixel, got %s" % (what, tuple(labels.shape)))
    if labels.numel() >= 2 ** 31:
        raise ValueError("%s: labels %s hold 2**31 pixels or more" % (what, tuple(labels.shape)))
    return labels


def regions_reference(labels, connectivity=4):
    """Specification of hip.seg_regions: labels integer [H, W] (or [B, H, W]) -> (root, size), both int32 of labels' shape.

    Two pixels of one image are adjacent under connectivity=4 iff they differ by one step in x or in y; under connectivity=8 the
    diagonal steps count too (any other connectivity: ValueError).  A region is a maximal set of pixels that is connected
    through adjacency and carries the same label value: values are compared as they are (as `boundary_areas_reference` does),
    so 255, a negative int16 and anything outside [0, n) are values of their own and form regions like any other; regions
    never cross from one image of a batch into the next.
      root[p] = the smallest y W + x inside its image over the pixels of p's region: canonical, no numbering by discovery
      size[p] = the region's pixel count
    Computed by iterating "the minimum over the equal-valued neighbours, then a pointer jump" until nothing moves: root[p] <= p
    always names a pixel of p's region, so the fixed point is the region's smallest index.  Runs on any device."""
    what = "regions_reference"
    conn = _connectivity_arg(what, connectivity)
    labels = _region_labels(what, labels)
    lab = labels.reshape((-1,) + tuple(labels.shape[-2:]))
    B, H, W = lab.shape
    steps = [(0, 1), (1, 0)] + ([(1, 1), (1, -1)] if conn == 8 else [])
    pairs = []                                  # (here, there) slices with their equal-value masks, both directions
    for dy, dx in steps:
        if dy >= H or abs(dx) >= W:
            continue
        here = (slice(None), slice(0, H - dy), slice(max(-dx, 0), W - max(dx, 0)))
        there = (slice(None), slice(dy, H), slice(max(dx, 0), W - max(-dx, 0)))
        pairs.append((here, there, lab[here] == lab[there]))
    root = torch.arange(H * W, dtype=torch.int64, device=lab.device).reshape(1, H, W).expand(B, H, W).contiguous()
    while True:
        new = root.clone()
        for here, there, same in pairs:
            new[here] = torch.where(same, torch.minimum(new[here], root[there]), new[here])
            new[there] = torch.where(same, torch.minimum(new[there], root[here]), new[there])
        flat = new.reshape(B, H * W)
        new = flat.gather(1, flat).reshape(B, H, W)                # the pointer jump
        if torch.equal(new, root):
            break
        root = new
    offs = torch.arange(B, dtype=torch.int64, device=lab.device).reshape(B, 1, 1) * (H * W)
    size = torch.bincount((root + offs).reshape(-1), minlength=B * H * W)[(root + offs)]
    return root.to(torch.int32).reshape(labels.shape), size.to(torch.int32).reshape(labels.shape)


def region_drop_reference(labels, size, min_region, fill=255, n=None, raw_labels=True, weight=None):
    """Specification of hip.seg_region_drop's last step: labels integer [H, W] (or [B, H, W]), size = `regions_reference`'s of
    them -> (out, dropped) or, with a weight plane (labels' shape), (out, dropped, weight).

    A pixel whose value is not `fill` and whose size < min_region becomes `fill`, and its weight 0; every other pixel and
    weight is unchanged, so regions of the value `fill` are never touched.  dropped int64 [n]: the dropped pixels per class,
    the class being value - 1 with raw_labels, else the value; values outside the classes are dropped but not counted.
    n None: every class a uint8 map holds (254 with raw_labels, else 255).  min_region: an int >= 1, 1 drops nothing; fill:
    an int in 0 .. 255; anything else is a ValueError.  Runs on any device."""
    what = "region_drop_reference"
    min_region = _min_region_arg(what, min_region)
    labels = _region_labels(what, labels)
    size = torch.as_tensor(size)
    if size.dtype.is_floating_point or size.dtype == torch.bool or size.shape != labels.shape:
        raise ValueError("%s: size must be integer %s, got %s %s" % (what, tuple(labels.shape), size.dtype, tuple(size.shape)))
    if not isinstance(fill, int) or isinstance(fill, bool) or not 0 <= fill <= 255:
        raise ValueError("%s: fill must be an int in 0 .. 255, got %r" % (what, fill))
    if n is None:
        n = hip.seg_pseudo_max_classes(raw_labels)
    if not isinstance(n, int) or isinstance(n, bool) or not 1 <= n <= hip.SEG_REGION_MAX_CLASSES:
        raise ValueError("%s: n must be an int in 1 .. %d, got %r" % (what, hip.SEG_REGION_MAX_CLASSES, n))
    if weight is not None:
        weight = torch.as_tensor(weight)
        if weight.shape != labels.shape:
            raise ValueError("%s: weight must have the labels' shape %s, got %s" % (what, tuple(labels.shape), tuple(weight.shape)))
    drop = (labels != fill) & (size.to(labels.device) < min_region)
    out = torch.where(drop, torch.full_like(labels, fill), labels)
    cls = labels.long() - (1 if raw_labels else 0)
    dropped = torch.bincount(cls[drop & (cls >= 0) & (cls < n)], minlength=n)
    if weight is not None:
        return out, dropped, torch.where(drop.to(weight.device), torch.zeros_like(weight), weight)
    return out, dropped


def _passes_arg(what, passes):
    if not isinstance(passes, int) or isinstance(passes, bool) or passes < 1:
        raise ValueError("%s: passes must be an int >= 1, got %r" % (what, passes))
    return passes


def _sieve_pass(lab, K, conn, ignore):
    """one pass of `sieve_reference` on lab int64 [B, H, W] -> the new map"""
    B, H, W = lab.shape
    dev = lab.device
    root, size = regions_reference(lab, conn)
    root, size = root.reshape(B, H, W).long(), size.reshape(B, H, W).long()
    offs = torch.arange(B, dtype=torch.int64, device=dev).reshape(B, 1, 1) * (H * W)
    key = size * (1 << 32) + ((1 << 32) - 1 - root)                 # (size, -root), lexicographic; size < 2^31
    live = torch.ones_like(lab, dtype=torch.bool) if ignore is None else lab != ignore
    small = (size < K) & live
    best = torch.zeros(B * H * W, dtype=torch.int64, device=dev)    # per region, at its root: the largest key that may take it
    slot = root + offs
    for dy, dx in ((0, 1), (1, 0)):                                 # always 4-adjacency, both ways
        if dy >= H or dx >= W:
            continue
        a = (slice(None), slice(0, H - dy), slice(0, W - dx))
        b = (slice(None), slice(dy, H), slice(dx, W))
        for here, there in ((a, b), (b, a)):
            vote = small[here] & (slot[here] != slot[there]) & live[there] & (key[there] > key[here])
            best.scatter_reduce_(0, slot[here][vote], key[there][vote], "amax")
    won = best[slot]
    take = small & (won > 0)
    winner = (1 << 32) - 1 - (won & ((1 << 32) - 1)) + offs          # the winning neighbour's root pixel
    return torch.where(take, lab.reshape(-1)[torch.where(take, winner, slot)], lab)


def sieve_reference(labels, min_region, connectivity=4, passes=1, ignore=None, n=None, raw_labels=False, conf=None):
    """Specification of hip.seg_sieve: labels integer [H, W] (or [B, H, W]) -> (out, moved) or, with a conf plane (labels'
    shape), (out, moved, conf).  The sieve filter GIS users know from gdal_sieve, in a form whose result does not depend on any
    order of processing: small regions take the value of their largest neighbour.

    One pass, per image, everything decided from the pass's input map at once:
      1. root, size = `regions_reference(labels, connectivity)`.  Every region has the key (size, -root), compared
         lexicographically; keys are unique within an image.
      2. A region R is small iff size < min_region and its value is not `ignore` (None: no value is).
      3. The neighbours of R are the regions Q != R that hold a pixel one step in x or y from a pixel of R -- 4-adjacency
         whatever `connectivity` is, so a neighbour always differs in value -- inside the same image; regions of the value
         `ignore` are never neighbours.
      4. R takes the value of the neighbour with the largest key, and only if that key is larger than R's own; otherwise it
         stays.  So two small regions never swap (the smaller joins the larger), a region of min_region pixels or more is never
         relabelled and only grows, and no pixel ever becomes `ignore`.
    `passes` (an int >= 1) repeats this on the previous pass's output, the regions recomputed each time.
      out    the labels' dtype and shape
      moved  int64 [2, n], the final map against the input: moved[0, c] the pixels that were class c and are not any more,
             moved[1, c] those that are class c and were not; class = value - 1 with raw_labels, else the value; values
             outside [0, n) are not counted.  n None: hip.SEG_SIEVE_MAX_CLASSES
      conf   0 where out != labels, untouched elsewhere: the model never stated a confidence for the label such a pixel
             carries now
    min_region 1 is the identity.  A bad argument is a ValueError naming it.  Runs on any device."""
    what = "sieve_reference"
    K = _min_region_arg(what, min_region)
    conn = _connectivity_arg(what, connectivity)
    passes = _passes_arg(what, passes)
    labels = _region_labels(what, labels)
    if ignore is not None and (not isinstance(ignore, int) or isinstance(ignore, bool)):
        raise ValueError("%s: ignore must be None or an int, got %r" % (what, ignore))
    if n is None:
        n = hip.SEG_SIEVE_MAX_CLASSES
    if not isinstance(n, int) or isinstance(n, bool) or not 1 <= n <= hip.SEG_SIEVE_MAX_CLASSES:
        raise ValueError("%s: n must be an int in 1 .. %d, got %r" % (what, hip.SEG_SIEVE_MAX_CLASSES, n))
    if conf is not None:
        conf = torch.as_tensor(conf)
        if conf.shape != labels.shape:
            raise ValueError("%s: conf must have the labels' shape %s, got %s" % (what, tuple(labels.shape), tuple(conf.shape)))
    first = labels.reshape((-1,) + tuple(labels.shape[-2:])).long()
    lab = first
    for _ in range(passes):
        new = _sieve_pass(lab, K, conn, ignore)
        if torch.equal(new, lab):               # a fixed point: every further pass decides the same from the same map
            break
        lab = new
    changed = lab != first
    raw = 1 if raw_labels else 0
    was, now = first[changed] - raw, lab[changed] - raw
    moved = torch.stack([torch.bincount(was[(was >= 0) & (was < n)], minlength=n),
                         torch.bincount(now[(now >= 0) & (now < n)], minlength=n)])
    out = lab.to(labels.dtype).reshape(labels.shape)
    if conf is not None:
        return out, moved, torch.where(changed.reshape(labels.shape).to(conf.device), torch.zeros_like(conf), conf)
    return out, moved


def conf_q16(conf):
    """fp32 confidences -> 16-bit fixed point, int64 of the same shape: clamp(floor(conf * 65536), 0, 65535) evaluated in fp32
    (the product is exact), NaN -> 0, +inf -> 65535: what the region table sums.  `conf_q16(c) >> 8 == conf_bin(c)` for every
    fp32 c.  Runs on any device."""
    conf = torch.as_tensor(conf)
    if conf.dtype != torch.float32:
        raise ValueError("conf_q16: conf must be float32, got %s" % conf.dtype)
    q = torch.floor(conf * 65536.0)
    return torch.where(torch.isnan(q), torch.zeros_like(q), q).clamp(0.0, 65535.0).long()


def _max_regions_arg(what, max_regions):
    if not isinstance(max_regions, int) or isinstance(max_regions, bool) or not 1 <= max_regions <= hip.SEG_REGION_TABLE_MAX:
        raise ValueError("%s: max_regions must be an int in 1 .. %d, got %r" % (what, hip.SEG_REGION_TABLE_MAX, max_regions))
    return max_regions


def _ignore_arg(what, ignore):
    if ignore is not None and (not isinstance(ignore, int) or isinstance(ignore, bool)):
        raise ValueError("%s: ignore must be None or an int, got %r" % (what, ignore))
    return ignore


def region_table_reference(labels, conf=None, connectivity=4, min_region=1, ignore=None, max_regions=1024, regions=None):
    """Specification of hip.seg_region_table: labels integer [H, W] (or [B, H, W]), conf fp32 of the same shape or None ->
    (rows int32 [B, R, 8], sums int64 [B, R, 3], count int32 [B], slot int32 of the labels' shape), R = max_regions, the
    leading B absent for an [H, W] map.

    Regions, root and size are `regions_reference(labels, connectivity)`'s.  A region is listed iff size >= min_region and its
    value is not `ignore` (None: no value is).  The listed regions of an image are numbered 0, 1, ... in ascending order of
    root -- canonical, not an order of discovery; count[b] is their number, which may exceed R.  For a listed region with
    number s < R:
      rows[b, s] = (value, root, size, x0, y0, x1, y1, 0)      the box inclusive, in pixels of the image
      sums[b, s] = (sum x, sum y, sum q) over its pixels        q = `conf_q16(conf)`; 0 without conf
    Rows from min(count[b], R) on are zero here (the kernel does not write them).  slot[p] = the row of p's region, -1 where the
    region is not listed or its number is >= R.  Everything is an integer.  regions: `regions_reference(labels, connectivity)`'s
    (root, size) where the caller holds them already (they are not computed again).  A bad argument is a ValueError naming it.
    Runs on any device."""
    what = "region_table_reference"
    conn = _connectivity_arg(what, connectivity)
    K = _min_region_arg(what, min_region)
    _ignore_arg(what, ignore)
    R = _max_regions_arg(what, max_regions)
    labels = _region_labels(what, labels)
    if conf is not None:
        conf = torch.as_tensor(conf)
        if conf.dtype != torch.float32 or conf.shape != labels.shape:
            raise ValueError("%s: conf must be float32 %s, got %s %s" % (what, tuple(labels.shape), conf.dtype, tuple(conf.shape)))
    root, size = regions_reference(labels, conn) if regions is None else (torch.as_tensor(r).to(labels.device) for r in regions)
    if root.shape != labels.shape or size.shape != labels.shape:
        raise ValueError("%s: regions must be (root, size) of the labels' shape %s, got %s %s" % (
            what, tuple(labels.shape), tuple(root.shape), tuple(size.shape)))
    lead, (H, W) = tuple(labels.shape[:-2]), labels.shape[-2:]
    dev = labels.device
    lab = labels.reshape(-1, H * W).long()
    root, size = root.reshape(-1, H * W).long(), size.reshape(-1, H * W).long()
    B = lab.shape[0]
    pix = torch.arange(H * W, dtype=torch.int64, device=dev).reshape(1, H * W)
    listed = size >= K if ignore is None else (size >= K) & (lab != ignore)
    flag = listed & (root == pix)                                   # the listed regions' roots
    number = flag.long().cumsum(1) - 1                              # ascending root = ascending flat index
    count = flag.sum(1)
    at_root = torch.where(flag & (number < R), number, torch.full_like(number, -1))
    slot = at_root.gather(1, root)
    on = slot >= 0
    key = (slot + torch.arange(B, dtype=torch.int64, device=dev).reshape(B, 1) * R)[on]
    x, y = (pix % W).expand(B, H * W)[on], (pix // W).expand(B, H * W)[on]
    q = conf_q16(conf.to(dev)).reshape(B, H * W)[on] if conf is not None else torch.zeros_like(x)
    big = 2 ** 31 - 1
    lowest = torch.full((B * R,), big, dtype=torch.int64, device=dev)
    highest = torch.full((B * R,), -1, dtype=torch.int64, device=dev)
    box = torch.stack([lowest.scatter_reduce(0, key, x, "amin"), lowest.scatter_reduce(0, key, y, "amin"),
                       highest.scatter_reduce(0, key, x, "amax"), highest.scatter_reduce(0, key, y, "amax")], 1)
    nothing = torch.zeros(B * R, dtype=torch.int64, device=dev)
    sums = torch.stack([nothing.index_add(0, key, v) for v in (x, y, q)], 1)
    rows = torch.zeros(B * R, 8, dtype=torch.int64, device=dev)
    head = (at_root + torch.arange(B, dtype=torch.int64, device=dev).reshape(B, 1) * R)[at_root >= 0]
    written = torch.zeros(B * R, dtype=torch.bool, device=dev)
    written[head] = True
    rows[head, 0], rows[head, 1], rows[head, 2] = lab[at_root >= 0], root[at_root >= 0], size[at_root >= 0]
    rows[:, 3:7] = torch.where(written[:, None], box, torch.zeros_like(box))
    return (rows.to(torch.int32).reshape(lead + (R, 8)), sums.reshape(lead + (R, 3)), count.to(torch.int32).reshape(lead),
            slot.to(torch.int32).reshape(labels.shape))


class RegionTable:
    """The connected regions of ONE image's label map, on the device: what `hip.seg_region_table` wrote (rows int32 [R, 8],
    sums int64 [R, 3], count int32 scalar, slot int32 [H, W]) beside the labels [H, W] and the conf [H, W] (or None) it was
    made from.  count may exceed R = rows.shape[0]: `truncated()`.  The accessors return device tensors of the WRITTEN rows,
    the first min(count, R), in ascending order of the regions' roots; which rows those are is decided on the device (a
    boolean mask), so only `to_list` synchronises with the host."""

    def __init__(self, rows, sums, count, slot, labels, conf=None):
        self.rows, self.sums, self.count, self.slot, self.labels, self.conf = rows, sums, count, slot, labels, conf

    @property
    def max_regions(self):
        return int(self.rows.shape[0])

    def truncated(self):
        """device bool: more regions are listed than the table holds"""
        return self.count > self.max_regions

    def _written(self):
        return torch.arange(self.max_regions, device=self.rows.device) < self.count

    def values(self):
        return self.rows[self._written(), 0]

    def roots(self):
        return self.rows[self._written(), 1]

    def areas(self):
        return self.rows[self._written(), 2]

    def boxes(self):
        """int32 [k, 4]: (x0, y0, x1, y1), inclusive"""
        return self.rows[self._written(), 3:7]

    def centroids(self):
        """float64 [k, 2]: (mean x, mean y) = the coordinate sums / the area"""
        w = self._written()
        return self.sums[w, :2].double() / self.rows[w, 2:3].double()

    def mean_conf(self):
        """float64 [k]: sum q / (65536 area); 0 where the table was made without conf"""
        w = self._written()
        return self.sums[w, 2].double() / (65536.0 * self.rows[w, 2].double())

    def to_list(self, names=None):
        """the one host round trip -> a list of dicts(value, name, area, box (x0, y0, x1, y1), centroid (x, y), confidence), one
        per written row; names: a sequence indexed by value (a value outside it has the name None), or None.  confidence is
        None where the table was made without conf"""
        w = self._written()
        rows, sums = self.rows[w].cpu().tolist(), self.sums[w].cpu().tolist()
        out = []
        for r, s in zip(rows, sums):
            v, area = r[0], r[2]
            out.append({"value": v, "name": names[v] if names is not None and 0 <= v < len(names) else None, "area": area,
                        "box": tuple(r[3:7]), "centroid": (s[0] / area, s[1] / area),
                        "confidence": None if self.conf is None else s[2] / (65536.0 * area)})
        return out


def _max_runs_arg(what, max_runs):
    if not isinstance(max_runs, int) or isinstance(max_runs, bool) or not 1 <= max_runs <= hip.SEG_RLE_MAX_RUNS:
        raise ValueError("%s: max_runs must be an int in 1 .. %d, got %r" % (what, hip.SEG_RLE_MAX_RUNS, max_runs))
    return max_runs


def rle_encode_reference(labels, max_runs=65536):
    """Specification of hip.seg_rle_encode: labels uint8 / int16 [H, W] (or [B, H, W]) -> (runs int32 [B, R, 2], count int32
    [B]), R = max_runs, the leading B absent for an [H, W] map: the runs of each map in COCO's run order.

    Per image f[i] = labels[i % H, i // H] for 0 <= i < H W: column-major.  Position i starts a run iff i == 0 or
    f[i] != f[i - 1], the values compared as they are (255 and negative int16 values are values of their own).  A run goes on
    across a column boundary, as COCO's does, and never from one image into the next.  Runs are numbered 0, 1, ... in
    ascending order of start; count[b] is their number, which may exceed R.  For s < min(count[b], R),
    runs[b, s] = (start, value); the entries behind are zero here (the kernel does not write them).  A run's length is the
    next run's start (H W for the last) minus its own.  Everything is an integer.  A bad argument is a ValueError naming it.
    Runs on any device."""
    what = "rle_encode_reference"
    R = _max_runs_arg(what, max_runs)
    labels = torch.as_tensor(labels)
    if labels.dtype not in (torch.uint8, torch.int16):
        raise ValueError("%s: labels must be uint8 or int16, got %s" % (what, labels.dtype))
    labels = _region_labels(what, labels)
    lead, (H, W) = tuple(labels.shape[:-2]), labels.shape[-2:]
    dev = labels.device
    f = labels.reshape(-1, H, W).transpose(1, 2).reshape(-1, H * W).long()
    B = f.shape[0]
    first = torch.ones(B, 1, dtype=torch.bool, device=dev)
    flag = torch.cat([first, f[:, 1:] != f[:, :-1]], 1)
    number = flag.long().cumsum(1) - 1
    count = flag.sum(1)
    runs = torch.zeros(B * R, 2, dtype=torch.int64, device=dev)
    on = flag & (number < R)
    key = (number + torch.arange(B, dtype=torch.int64, device=dev).reshape(B, 1) * R)[on]
    pos = torch.arange(H * W, dtype=torch.int64, device=dev).reshape(1, H * W).expand(B, H * W)
    runs[key, 0], runs[key, 1] = pos[on], f[on]
    return runs.to(torch.int32).reshape(lead + (R, 2)), count.to(torch.int32).reshape(lead)


def rle_decode_reference(runs, count, H, W, dtype=torch.uint8, fill=255):
    """Specification of hip.seg_rle_decode: runs int32 [R, 2] (or [B, R, 2]), count int32 of the leading shape -> (out `dtype`
    [H, W] (or [B, H, W]), flag int32 [1]).  With m = min(count[b], R): out[b, y, x] = (dtype) value[s], s the largest index
    below m with start[s] <= x H + y (0 where there is none: flag bit 1 says so); with m <= 0 the image is `fill`.  flag: bit 0
    where count[b] > R -- a truncated table, whose tail carries the last written run's value -- and bit 1 where m <= 0 or
    start[0] != 0, over all images.  For a table whose starts do not ascend the pixels are whatever the search finds (the
    kernel's search differs); the flag bits hold for any table.  `rle_decode_reference(*rle_encode_reference(x, R), H, W,
    x.dtype)[0]` is x wherever count <= R.  Runs on any device."""
    what = "rle_decode_reference"
    runs, count = torch.as_tensor(runs), torch.as_tensor(count)
    if runs.dtype != torch.int32 or runs.dim() not in (2, 3) or runs.shape[-1] != 2 or runs.shape[-2] < 1:
        raise ValueError("%s: runs must be int32 [R, 2] or [B, R, 2], got %s %s" % (what, runs.dtype, tuple(runs.shape)))
    lead, R = tuple(runs.shape[:-2]), int(runs.shape[-2])
    if count.dtype != torch.int32 or tuple(count.shape) != lead:
        raise ValueError("%s: count must be int32 %s, got %s %s" % (what, lead, count.dtype, tuple(count.shape)))
    if dtype not in (torch.uint8, torch.int16):
        raise ValueError("%s: dtype must be torch.uint8 or torch.int16, got %r" % (what, dtype))
    dev = runs.device
    tab, cnt = runs.reshape(-1, R, 2).long(), count.reshape(-1).long().to(dev)
    B = tab.shape[0]
    out = torch.empty(B, H, W, dtype=dtype, device=dev)
    pos = (torch.arange(W, dtype=torch.int64, device=dev).reshape(1, W) * H
           + torch.arange(H, dtype=torch.int64, device=dev).reshape(H, 1))          # [H, W]: x H + y
    flag = 0
    for b in range(B):
        c = int(cnt[b])
        m = min(c, R)
        flag |= (1 if c > R else 0) | (2 if m <= 0 or int(tab[b, 0, 0]) != 0 else 0)
        if m <= 0:
            out[b] = fill
            continue
        s = (torch.searchsorted(tab[b, :m, 0].contiguous(), pos.reshape(-1), right=True) - 1).clamp(0, m - 1)
        out[b] = tab[b, :m, 1][s].reshape(H, W).to(dtype)
    return out.reshape(lead + (H, W)), torch.tensor([flag], dtype=torch.int32, device=dev)


# ---- COCO's RLE on the host: the counts of a class's binary mask and cocoapi's string form of them (maskApi.c: rleToString,
# rleFrString).  pycocotools is not needed; no string it produced has been compared.
def coco_counts(starts, values, c, HW):
    """the uncompressed COCO counts of the binary mask `labels == c`, from a label map's runs in COCO's order (starts and
    values of equal length, ascending starts from 0, HW pixels in all) -> a list of ints that alternates 0-runs and 1-runs and
    begins with a 0-run, which may be 0 long.  A class that is absent gives [HW]."""
    import numpy as np
    starts, values = np.asarray(starts, dtype=np.int64).reshape(-1), np.asarray(values, dtype=np.int64).reshape(-1)
    if starts.shape != values.shape or starts.size < 1 or starts[0] != 0 or HW < 1 or (np.diff(starts) <= 0).any() or starts[-1] >= HW:
        raise ValueError("coco_counts: starts must ascend from 0 below HW = %r and match values, got %d starts and %d values"
                         % (HW, starts.size, values.size))
    on = values == c
    change = np.flatnonzero(on[1:] != on[:-1]) + 1                  # the runs at which the mask changes
    bounds = np.concatenate([starts[:1], starts[change], [HW]])
    counts = np.diff(bounds).tolist()
    return [0] + counts if on[0] else counts


def coco_mask_reference(labels, c):
    """the same list as `coco_counts`, taken from the dense mask directly: labels [H, W] -> the run lengths of
    (labels == c) in column-major order, beginning with the 0-run"""
    import numpy as np
    f = (np.asarray(torch.as_tensor(labels).cpu()).astype(np.int64) == c).T.reshape(-1)
    change = np.flatnonzero(f[1:] != f[:-1]) + 1
    counts = np.diff(np.concatenate([[0], change, [f.size]])).tolist()
    return [0] + counts if f[0] else counts


def coco_rle_string(counts):
    """cocoapi's rleToString: the compressed string of uncompressed counts.  From the fourth count on the stored value is
    counts[i] - counts[i - 2]; each value leaves 5 bits at a time, low bits first, a chunk carrying bit 0x20 while more follow
    (more: x != -1 where bit 4 of the chunk is set, else x != 0, x shifted arithmetically), as the char chunk + 48"""
    out = []
    for i, x in enumerate(counts):
        x = int(x)
        if i > 2:
            x -= int(counts[i - 2])
        more = True
        while more:
            c = x & 0x1f
            x >>= 5                                                 # arithmetic, as C's on a signed long
            more = x != -1 if c & 0x10 else x != 0
            if more:
                c |= 0x20
            out.append(chr(c + 48))
    return "".join(out)


def coco_rle_counts(string):
    """cocoapi's rleFrString: the counts of a compressed string; the last chunk of a value sign-extends"""
    counts, p, n = [], 0, len(string)
    while p < n:
        x, k, more = 0, 0, True
        while more:
            if p >= n:
                raise ValueError("coco_rle_counts: the string ends inside a value")
            c = ord(string[p]) - 48
            if not 0 <= c < 64:
                raise ValueError("coco_rle_counts: %r at %d is no RLE character" % (string[p], p))
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and c & 0x10:
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


class RunLengthMap:
    """ONE image's label map as the table of its runs in COCO's run order, on the device: what `hip.seg_rle_encode` wrote
    (runs int32 [R, 2] of (start, value), count int32 scalar) with the map's shape (H, W) and dtype.  count may exceed
    R = runs.shape[0]: `truncated()`.  The accessors return device tensors of the WRITTEN runs, the first min(count, R); which
    those are is decided on the device (a boolean mask), so only `to_coco` synchronises with the host.  n: the number of
    classes where the maker knows it (a Segmenter does), else None."""

    def __init__(self, runs, count, shape, dtype, n=None):
        self.runs, self.count, self.shape, self.dtype, self.n = runs, count, (int(shape[0]), int(shape[1])), dtype, n

    @property
    def max_runs(self):
        return int(self.runs.shape[0])

    @property
    def nbytes(self):
        """the bytes of the table as it is held: 8 per entry of runs and the count word (a stored table needs the first
        `count` entries only)"""
        return self.runs.numel() * 4 + 4

    def truncated(self):
        """device bool: the map has more runs than the table holds"""
        return self.count > self.max_runs

    def _written(self):
        return torch.arange(self.max_runs, device=self.runs.device) < self.count

    def starts(self):
        return self.runs[self._written(), 0]

    def values(self):
        return self.runs[self._written(), 1]

    def lengths(self):
        """int32 [k]: the next run's start minus the run's own, the last run ending at H W (in a truncated table the last
        written run carries the rest of the map)"""
        s = self.starts()
        return torch.diff(s, append=s.new_full((1,), self.shape[0] * self.shape[1]))

    def areas(self, n):
        """int64 [n]: the pixels of every class 0 .. n - 1, from values and lengths"""
        v, l = self.values().long(), self.lengths().long()
        ok = (v >= 0) & (v < n)
        return torch.zeros(n, dtype=torch.int64, device=v.device).index_add_(0, torch.where(ok, v, torch.zeros_like(v)),
                                                                            torch.where(ok, l, torch.zeros_like(l)))

    def decode(self, out=None):
        """the label map [H, W] of `dtype` again: one `hip.seg_rle_decode`"""
        return hip.seg_rle_decode(self.runs, self.count, self.shape[0], self.shape[1], self.dtype, out=out)[0]

    def _classes(self, category_ids):
        if category_ids is not None:
            return len(category_ids)
        return self.n if self.n is not None else 255

    def to_coco(self, image_id, category_ids=None):
        """the one host round trip -> COCO stuff results: a list of dicts(image_id, category_id, segmentation=dict(size=[H, W],
        counts=<compressed str>)), one per value in [0, n) that the map holds, in ascending class order; n = len(category_ids)
        where given, else the maker's class count, else 255.  category_id = category_ids[c] if given, else c.  A value outside
        [0, n), such as 255, gets no entry.  A truncated table is a ValueError."""
        H, W = self.shape
        count = int(self.count)
        if count > self.max_runs:
            raise ValueError("RunLengthMap.to_coco: the table is truncated: the map has %d runs, max_runs is %d" % (count, self.max_runs))
        tab = self.runs[:count].cpu().numpy()
        starts, values = tab[:, 0], tab[:, 1]
        n = self._classes(category_ids)
        out = []
        for c in sorted(set(int(v) for v in values.tolist() if 0 <= v < n)):
            out.append({"image_id": image_id, "category_id": category_ids[c] if category_ids is not None else c,
                        "segmentation": {"size": [H, W], "counts": coco_rle_string(coco_counts(starts, values, c, H * W))}})
        return out

    @classmethod
    def from_coco(cls, entries, shape, class_of=None, fill=255, dtype=torch.uint8, device=None, n=None):
        """the other way, on the host: COCO results of ONE image (dicts with category_id and segmentation: size, counts as a
        compressed str or a list) -> the RunLengthMap of the label map that holds class_of[category_id] (category_id itself
        without class_of) under every mask and `fill` elsewhere, equal neighbours merged into one run.  The masks must be
        disjoint and of `shape`, else ValueError."""
        import numpy as np
        H, W = int(shape[0]), int(shape[1])
        flat = np.full(H * W, fill, dtype=np.int64)
        taken = np.zeros(H * W, dtype=bool)
        for e in entries:
            seg = e["segmentation"]
            if [int(v) for v in seg["size"]] != [H, W]:
                raise ValueError("RunLengthMap.from_coco: an entry of size %r in a map of shape %r" % (seg["size"], (H, W)))
            counts = coco_rle_counts(seg["counts"]) if isinstance(seg["counts"], str) else [int(v) for v in seg["counts"]]
            if sum(counts) != H * W or any(v < 0 for v in counts):
                raise ValueError("RunLengthMap.from_coco: the counts of category %r do not add up to H W = %d" % (e["category_id"], H * W))
            value = class_of[e["category_id"]] if class_of is not None else e["category_id"]
            ends = np.cumsum(counts)
            for a, b in zip(ends[0::2].tolist(), ends[1::2].tolist()):         # the 1-runs
                if taken[a:b].any():
                    raise ValueError("RunLengthMap.from_coco: the mask of category %r overlaps another" % (e["category_id"],))
                taken[a:b] = True
                flat[a:b] = value
        starts = np.concatenate([[0], np.flatnonzero(flat[1:] != flat[:-1]) + 1])
        runs = torch.from_numpy(np.stack([starts, flat[starts]], 1)).to(torch.int32)
        count = torch.tensor(len(starts), dtype=torch.int32)
        return cls(runs.to(device=device), count.to(device=device), (H, W), dtype, n)


def _check_sieve(sieve, sieve_connectivity, sieve_passes):
    """the three sieve keywords of the Segmenter, checked -> (sieve, sieve_connectivity, sieve_passes)"""
    if sieve is not None and (not isinstance(sieve, int) or isinstance(sieve, bool) or not 1 <= sieve < 2 ** 31):
        raise ValueError("Segmenter: sieve must be None or an int in 1 .. 2**31 - 1 (the smallest region kept; 1 moves nothing), "
                         "got %r" % (sieve,))
    if not isinstance(sieve_connectivity, int) or isinstance(sieve_connectivity, bool) or sieve_connectivity not in (4, 8):
        raise ValueError("Segmenter: sieve_connectivity must be the int 4 or 8, got %r" % (sieve_connectivity,))
    if not isinstance(sieve_passes, int) or isinstance(sieve_passes, bool) or not 1 <= sieve_passes <= hip.SEG_SIEVE_MAX_PASSES:
        raise ValueError("Segmenter: sieve_passes must be an int in 1 .. %d, got %r" % (hip.SEG_SIEVE_MAX_PASSES, sieve_passes))
    return sieve, sieve_connectivity, sieve_passes


class _PseudoLabelFields(NamedTuple):
    labels: torch.Tensor                       # [H, W] uint8: the pseudo-label map `train_sample` takes (255 = ignored)
    predicted: torch.Tensor                    # [H, W] uint8 / int16: what `segment_raw` gave
    conf: torch.Tensor                         # [H, W] fp32: the winning class's probability
    kept: torch.Tensor                         # [2, n] int64: per class the kept and the predicted pixels of this image
    weight: Optional[torch.Tensor] = None      # [H, W] uint8 (return_weight): 0 = dropped, else max(conf_bin(conf), 1)


class PseudoLabelResult(_PseudoLabelFields):
    """The five fields above, as a tuple (it unpacks and compares as it always did), and one attribute behind them:
    region_dropped, int64 [n] or None -- with `pseudo_label_raw(min_region=)` the pixels per class that the region filter took
    out of `labels` (and out of kept[0]).  Keyword-only; it is not an element of the tuple."""
    region_dropped: Optional[torch.Tensor] = None

    def __new__(cls, labels, predicted, conf, kept, weight=None, *, region_dropped=None):
        self = super().__new__(cls, labels, predicted, conf, kept, weight)
        self.region_dropped = region_dropped
        return self


class ConfidenceHistogram:
    """`confidence_histogram_reference`'s counters on the device, summed over everything counted into them: `hist` int64
    [n, 256] (class, confidence bin) and `tally` int64 [2].  `hip.seg_conf_hist` adds to these tensors in place, so one
    histogram can span a whole data set (`Segmenter.pseudo_label_raw(..., hist=h)`) and the thresholds be balanced over it."""

    def __init__(self, n, device=None, hist=None, tally=None):
        self.n = int(n)
        self.hist = torch.zeros(self.n, CONF_BINS, dtype=torch.int64, device=device) if hist is None else hist
        self.tally = torch.zeros(2, dtype=torch.int64, device=self.hist.device) if tally is None else tally
        if self.hist.dtype != torch.int64 or tuple(self.hist.shape) != (self.n, CONF_BINS) or self.tally.dtype != torch.int64 \
                or tuple(self.tally.shape) != (2,) or self.hist.device != self.tally.device:
            raise ValueError("ConfidenceHistogram: hist must be int64 [%d, %d] and tally int64 [2] on one device, got %s %s and %s %s"
                             % (self.n, CONF_BINS, self.hist.dtype, tuple(self.hist.shape), self.tally.dtype, tuple(self.tally.shape)))

    def add_(self, other):
        if other.n != self.n:
            raise ValueError("ConfidenceHistogram.add_: %d classes against %d" % (other.n, self.n))
        self.hist += other.hist.to(self.hist.device)
        self.tally += other.tally.to(self.tally.device)
        return self

    def thresholds(self, keep=1.0, floor=0.0):
        """`pseudo_thresholds(self.hist, keep, floor)`: int32 [n] on the device, no host round trip"""
        return pseudo_thresholds(self.hist, keep, floor)

    def summary(self):
        """-> {"pixels", "outside", "share": [n], "median_bin": [n]}: the labels inside / outside [0, n), per class its share of
        the inside pixels (rounded to 4 digits; NaN without pixels) and the bin of its median confidence -- the smallest b with
        2 sum_{b' <= b} hist[c, b'] >= N_c, None for a class without pixels.  One host round trip."""
        N = self.hist.sum(1)
        median = (2 * self.hist.cumsum(1) < N[:, None]).sum(1)
        flat = torch.cat([N, median, self.tally]).tolist()
        n, pixels = self.n, flat[-2]
        return {"pixels": int(pixels), "outside": int(flat[-1]),
                "share": [round(flat[c] / pixels, 4) if pixels else float("nan") for c in range(n)],
                "median_bin": [int(flat[n + c]) if flat[c] else None for c in range(n)]}


class SegmentationScore:
    """The counters of `areas_reference` on the device, summed over everything scored into them: `areas` int64 [3, n],
    `tally` int64 [2].  The scoring kernels add to these tensors in place.

    confusion: None (the default: no matrix, memory and behaviour as without the argument), True (a zeroed one) or a tensor:
    `confusion_reference`'s matrix int64 [n, n + 1] on the same device, which class is taken for which; `evaluate_raw(...,
    confusion=True)` fills it (`hip.seg_confusion`).  `confusions`, `confusion_summary` and `merged` read it.

    boundary: None (the default: no counters, memory and behaviour as without the argument), True (zeroed ones) or a tensor:
    `boundary_areas_reference`'s counters int64 [3, n] on the same device, the three rows of `areas` restricted to the pixels
    within d of a contour, d = `boundary_distance(h, w, boundary_ratio)` per image; `evaluate_raw(..., boundary_iou=True)` fills
    them (`hip.seg_boundary_areas`), and `summary` / `group_summary` then report Boundary IoU beside IoU.

    calibration: None (the default: no counters, memory and behaviour as without the argument), True (zeroed ones) or a tensor:
    `calibration_reference`'s counters int64 [n, 256, 2] on the same device, pixels per (predicted class, confidence bin, hit);
    `evaluate_raw(..., calibration=True)` fills them (`hip.seg_calibration`), with `calibration_tally` int64 [2] beside them
    (scored pixels with a label inside / outside [0, n)).  `reliability`, `precision_thresholds` and `summary` ("ECE", "MCE",
    "cECE") read them.

    trimap: None (the default: no counters, memory and behaviour as without the argument), True (zeroed ones) or a tensor:
    `trimap_areas_reference`'s counters int64 [K, 3, n] on the same device, the three rows of `areas` per ring of the
    ground truth's distance to a contour, for the K radii `trimap_radii` (None: `default_trimap_radii()`);
    `evaluate_raw(..., trimap=True)` fills them (`hip.seg_trimap_areas`), and `summary` / `trimap_summary` / `group_summary`
    then report mIoU and accuracy within r pixels of a ground-truth contour, for every r."""

    def __init__(self, n, device=None, areas=None, tally=None, confusion=None, boundary=None, boundary_ratio=0.02,
                 calibration=None, trimap=None, trimap_radii=None):
        self.n = int(n)
        self.areas = torch.zeros(3, self.n, dtype=torch.int64, device=device) if areas is None else areas
        self.tally = torch.zeros(2, dtype=torch.int64, device=device) if tally is None else tally
        if self.areas.dtype != torch.int64 or tuple(self.areas.shape) != (3, self.n) or self.tally.dtype != torch.int64 \
                or tuple(self.tally.shape) != (2,) or self.areas.device != self.tally.device:
            raise ValueError("SegmentationScore: areas must be int64 [3, %d] and tally int64 [2] on one device, got %s %s and %s %s"
                             % (self.n, self.areas.dtype, tuple(self.areas.shape), self.tally.dtype, tuple(self.tally.shape)))
        if confusion is None or confusion is False:
            self.confusion = None
        elif confusion is True:
            self.confusion = torch.zeros(self.n, self.n + 1, dtype=torch.int64, device=self.areas.device)
        else:
            self.confusion = confusion
            if not torch.is_tensor(confusion) or confusion.dtype != torch.int64 or tuple(confusion.shape) != (self.n, self.n + 1) \
                    or confusion.device != self.areas.device:
                raise ValueError("SegmentationScore: confusion must be None, True or int64 [%d, %d] on the device of areas, got %s"
                                 % (self.n, self.n + 1, (confusion.dtype, tuple(confusion.shape), confusion.device)
                                    if torch.is_tensor(confusion) else type(confusion)))
        self.boundary_ratio = _boundary_ratio("SegmentationScore", boundary_ratio)
        if boundary is None or boundary is False:
            self.boundary = None
        elif boundary is True:
            self.boundary = torch.zeros(3, self.n, dtype=torch.int64, device=self.areas.device)
        else:
            self.boundary = boundary
            if not torch.is_tensor(boundary) or boundary.dtype != torch.int64 or tuple(boundary.shape) != (3, self.n) \
                    or boundary.device != self.areas.device:
                raise ValueError("SegmentationScore: boundary must be None, True or int64 [3, %d] on the device of areas, got %s"
                                 % (self.n, (boundary.dtype, tuple(boundary.shape), boundary.device)
                                    if torch.is_tensor(boundary) else type(boundary)))
        if calibration is None or calibration is False:
            self.calibration = self.calibration_tally = None
        else:
            if calibration is True:
                calibration = torch.zeros(self.n, CONF_BINS, 2, dtype=torch.int64, device=self.areas.device)
            if not torch.is_tensor(calibration) or calibration.dtype != torch.int64 \
                    or tuple(calibration.shape) != (self.n, CONF_BINS, 2) or calibration.device != self.areas.device:
                raise ValueError("SegmentationScore: calibration must be None, True or int64 [%d, %d, 2] on the device of areas, got %s"
                                 % (self.n, CONF_BINS, (calibration.dtype, tuple(calibration.shape), calibration.device)
                                    if torch.is_tensor(calibration) else type(calibration)))
            self.calibration = calibration
            self.calibration_tally = torch.zeros(2, dtype=torch.int64, device=self.areas.device)
        if trimap is None or trimap is False:
            self.trimap = self.trimap_radii = None
        else:
            self.trimap_radii = _trimap_radii("SegmentationScore", default_trimap_radii() if trimap_radii is None else trimap_radii)
            K = len(self.trimap_radii)
            if trimap is True:
                trimap = torch.zeros(K, 3, self.n, dtype=torch.int64, device=self.areas.device)
            if not torch.is_tensor(trimap) or trimap.dtype != torch.int64 or tuple(trimap.shape) != (K, 3, self.n) \
                    or trimap.device != self.areas.device:
                raise ValueError("SegmentationScore: trimap must be None, True or int64 [%d, 3, %d] on the device of areas, got %s"
                                 % (K, self.n, (trimap.dtype, tuple(trimap.shape), trimap.device)
                                    if torch.is_tensor(trimap) else type(trimap)))
            self.trimap = trimap

    def add_(self, other):
        if other.n != self.n:
            raise ValueError("SegmentationScore.add_: %d classes against %d" % (other.n, self.n))
        if (self.confusion is None) != (other.confusion is None):
            raise ValueError("SegmentationScore.add_: one score has a confusion matrix and the other has none")
        if (self.boundary is None) != (other.boundary is None):
            raise ValueError("SegmentationScore.add_: one score has boundary counters and the other has none")
        if (self.calibration is None) != (other.calibration is None):
            raise ValueError("SegmentationScore.add_: one score has calibration counters and the other has none")
        if self.boundary is not None and self.boundary_ratio != other.boundary_ratio:
            raise ValueError("SegmentationScore.add_: boundary counters of ratio %r against ratio %r: bands of different widths "
                             "do not add" % (self.boundary_ratio, other.boundary_ratio))
        if (self.trimap is None) != (other.trimap is None):
            raise ValueError("SegmentationScore.add_: one score has trimap counters and the other has none")
        if self.trimap is not None and self.trimap_radii != other.trimap_radii:
            raise ValueError("SegmentationScore.add_: trimap counters of radii %r against radii %r: rings of different widths "
                             "do not add" % (self.trimap_radii, other.trimap_radii))
        self.areas += other.areas.to(self.areas.device)
        self.tally += other.tally.to(self.tally.device)
        if self.confusion is not None:
            self.confusion += other.confusion.to(self.confusion.device)
        if self.boundary is not None:
            self.boundary += other.boundary.to(self.boundary.device)
        if self.calibration is not None:
            self.calibration += other.calibration.to(self.calibration.device)
            self.calibration_tally += other.calibration_tally.to(self.calibration_tally.device)
        if self.trimap is not None:
            self.trimap += other.trimap.to(self.trimap.device)
        return self

    def _matrix(self, what):
        if self.confusion is None:
            raise ValueError("SegmentationScore.%s needs a confusion matrix: SegmentationScore(n, confusion=True), "
                             "evaluate_raw(..., confusion=True)" % what)
        return self.confusion

    def confusions(self, k=10):
        """the k largest off-diagonal entries of the matrix, largest first (ties: lower gt class, then lower predicted class)
        -> [(gt class, predicted class, pixels, share of the gt class's scored pixels)], entries of no pixels left out.
        Predicted class n is the outside column.  One host round trip."""
        C = self._matrix("confusions").cpu()
        n, rows = self.n, C.sum(1)
        off = C.clone()
        off[:, :n].fill_diagonal_(0)
        flat = off.reshape(-1)
        order = torch.argsort(flat, descending=True, stable=True)[:max(int(k), 0)].tolist()
        return [(i // (n + 1), i % (n + 1), int(flat[i]), int(flat[i]) / int(rows[i // (n + 1)])) for i in order if int(flat[i]) > 0]

    def confusion_summary(self):
        """-> the row-normalised matrix, float64 [n, n + 1] on the matrix's device: entry [c, p] is the share of class c's scored
        pixels labelled p (its diagonal is `summary()["Acc"]`, unrounded).  The row of a class without pixels is NaN, as
        `summary()` reports an absent class."""
        C = self._matrix("confusion_summary").double()
        return C / C.sum(1, keepdim=True)

    def merged(self, mapping, m=None):
        """The score under a coarser label set (171 classes to 27 super-categories, seen / unseen groups) -> a new
        `SegmentationScore(m, confusion=True)`.  mapping: a list / tensor of n new class ids in [0, m), or -1 to drop the class
        from the ground truth; m: None is max(mapping) + 1.  The new matrix is the old one with rows and columns summed per
        new id; the rows of dropped classes are removed, and predictions of a dropped class go to the outside column.  areas
        and tally[0] are rebuilt from it (the identities of `confusion_reference`), tally[1] is carried over.  By
        specification this is scoring the mapped label maps: `confusion_reference(mapping[labels], mapping[gt], m,
        raw_labels=False)` with -1 -> m in the ground truth.  Needs a confusion matrix (ValueError without one).
        The new score carries NO boundary counters, whether this one does or not: merging classes erases the contours between
        them, so the band areas of a coarser label set do not follow from the finer one's (they need a second pass over the
        mapped label maps).  For the same reason it carries NO trimap counters: the rings are measured from the contours of
        the finer ground truth.  It carries NO calibration counters either: a merged class's confidence is the SUM of its
        members' probabilities, not their maximum, so the (class, confidence bin) counts cannot be re-keyed."""
        C = self._matrix("merged")
        mp = torch.as_tensor(mapping).reshape(-1)
        if mp.dtype.is_floating_point or mp.dtype == torch.bool or mp.numel() != self.n:
            raise ValueError("SegmentationScore.merged: mapping must hold %d integer class ids, got %s %s" % (self.n, mp.dtype, tuple(mp.shape)))
        mp = mp.long().cpu()
        m = int(mp.max()) + 1 if m is None else int(m)
        if m < 1 or int(mp.min()) < -1 or int(mp.max()) >= m:
            raise ValueError("SegmentationScore.merged: new class ids must lie in [0, %d), or be -1, got %d .. %d" % (m, int(mp.min()), int(mp.max())))
        to = torch.where(mp < 0, torch.full_like(mp, m), mp).to(C.device)          # dropped: row m (removed), column m (outside)
        rows = torch.zeros(m + 1, self.n + 1, dtype=torch.int64, device=C.device).index_add_(0, to, C)
        cols = torch.cat([to, torch.full_like(to[:1], m)])                        # the outside column stays outside
        M = torch.zeros(m + 1, m + 1, dtype=torch.int64, device=C.device).index_add_(1, cols, rows)[:m].contiguous()
        areas = torch.stack([M[:, :m].diagonal(), M[:, :m].sum(0), M.sum(1)])
        return SegmentationScore(m, areas=areas, tally=torch.stack([M.sum(), self.tally[1].to(C.device)]), confusion=M)

    def _counters(self, what):
        if self.calibration is None:
            raise ValueError("SegmentationScore.%s needs calibration counters: SegmentationScore(n, calibration=True), "
                             "evaluate_raw(..., calibration=True)" % what)
        return self.calibration

    def reliability(self, bins=16, per_class=False):
        """The reliability diagram (Guo et al., ICML 2017) -> (pixels int64, accuracy float64, confidence float64), each [bins],
        or [n, bins] per predicted class with `per_class`: coarse bin m holds the pixels whose confidence lies in
        [m / bins, (m + 1) / bins), accuracy is the share of them whose label is the ground truth's class and confidence their
        mean confidence; both NaN where the bin is empty.  bins must divide 256 (ValueError).  The confidence of a fine bin b
        is taken as its midpoint (b + 0.5) / 256, so the confidence reported for a coarse bin differs from the true mean
        confidence of its pixels by at most 1 / 512.  On the score's device, float64 from the integers; not synchronising."""
        cal = self._counters("reliability")
        if not isinstance(bins, int) or isinstance(bins, bool) or bins < 1 or CONF_BINS % bins:
            raise ValueError("SegmentationScore.reliability: bins must be an int that divides %d, got %r" % (CONF_BINS, bins))
        N, H, C = _reliability_bins(cal, bins, per_class)
        out = (N.long(), H / N, C / N)
        return out if per_class else tuple(t[0] for t in out)

    def precision_thresholds(self, target, min_pixels=1):
        """Per-class pseudo-label thresholds by MEASURED precision -> int32 [n] bins on the score's device, what
        `Segmenter.pseudo_label_raw(thresholds=)` and `hip.seg_pseudo` take.  With N_cb / H_cb the pixels / hits of predicted
        class c in fine bin b: t_c is the smallest t with  sum_{b >= t} N_cb >= min_pixels  and
        sum_{b >= t} H_cb >= target * sum_{b >= t} N_cb  (integer suffix sums, compared in float64); 256 -- nothing kept --
        where no t does, as for a class never predicted.  target outside (0, 1] or min_pixels < 1: ValueError.  Not
        synchronising."""
        cal = self._counters("precision_thresholds")
        if isinstance(target, bool) or not isinstance(target, (int, float)) or not 0.0 < target <= 1.0:
            raise ValueError("SegmentationScore.precision_thresholds: target must be a number in (0, 1], got %r" % (target,))
        if not isinstance(min_pixels, int) or isinstance(min_pixels, bool) or min_pixels < 1:
            raise ValueError("SegmentationScore.precision_thresholds: min_pixels must be an int >= 1, got %r" % (min_pixels,))
        SN = cal.sum(-1).flip(1).cumsum(1).flip(1)
        SH = cal[..., 1].flip(1).cumsum(1).flip(1)
        ok = (SN >= min_pixels) & (SH.double() >= float(target) * SN.double())
        t = torch.arange(CONF_BINS, device=cal.device).expand_as(ok)
        return torch.where(ok, t, torch.full_like(t, CONF_BINS)).amin(1).to(torch.int32)

    def group_summary(self, groups):
        """groups: {name: class ids} (seen / unseen, things / stuff) -> {name: {"mIoU", "mAcc"}, ..., "hIoU"}: per group the nanmean
        of `summary()`'s per-class IoU / Acc over the group's classes, unrounded, then rounded to 4 digits as `summary()` does
        (and "mBIoU", the same of the per-class Boundary IoU, where the score carries boundary counters, and "trimap_mIoU":
        [K], the same of the per-class IoU within each radius, where it carries trimap counters);
        hIoU is the harmonic mean of the groups' mIoU, the seen / unseen figure of zero-shot segmentation tables (0 where a
        group's mIoU is 0, NaN where a group has no class with pixels).  Needs `areas` only; one host round trip; ground
        truth out of range is `summary()`'s IndexError."""
        names = list(groups)
        ids = []
        for name in names:
            c = torch.as_tensor(list(groups[name]), dtype=torch.long).reshape(-1)
            if name == "hIoU" or c.numel() == 0 or int(c.min()) < 0 or int(c.max()) >= self.n:
                raise ValueError("SegmentationScore.group_summary: group %r must hold class ids in [0, %d) (and not be named "
                                 "'hIoU'), got %s" % (name, self.n, c.tolist()))
            ids.append(c)
        counters = [self.areas.reshape(-1), self.tally] + ([] if self.boundary is None else [self.boundary.reshape(-1)])
        if self.trimap is not None:
            counters.append(self.trimap.cumsum(0).reshape(-1))
        flat = torch.cat(counters).cpu()
        self._refuse_out_of_range(int(flat[3 * self.n + 1]))
        a = flat[:3 * self.n].reshape(3, self.n).double()
        iou, acc = a[0] / (a[1] + a[2] - a[0]), a[0] / a[2]
        r4 = lambda v: round(float(v), 4)
        mious = [torch.nanmean(iou[c]) for c in ids]
        out = {name: {"mIoU": r4(mi), "mAcc": r4(torch.nanmean(acc[c]))} for name, c, mi in zip(names, ids, mious)}
        if self.boundary is not None:
            b = flat[3 * self.n + 2:6 * self.n + 2].reshape(3, self.n).double()
            biou = b[0] / (b[1] + b[2] - b[0])
            for name, c in zip(names, ids):
                out[name]["mBIoU"] = r4(torch.nanmean(biou[c]))
        if self.trimap is not None:
            t = flat[len(flat) - self.trimap.numel():].reshape(-1, 3, self.n).double()
            tiou = t[:, 0] / (t[:, 1] + t[:, 2] - t[:, 0])
            for name, c in zip(names, ids):
                out[name]["trimap_mIoU"] = [r4(torch.nanmean(row[c])) for row in tiou]
        mi = torch.stack(mious)
        out["hIoU"] = r4(0.0 if bool((mi == 0).any()) else len(names) / (1.0 / mi).sum())
        return out

    def logging_output(self):
        """the four histograms under the reference's keys, as `SegCriterion.reduce_metrics` takes them (float64, not the
        reference's float32: the counts of a validation set pass 2^24)"""
        a = self.areas.double()
        return {"area_intersect": a[0], "area_pred_label": a[1], "area_label": a[2], "area_union": a[1] + a[2] - a[0]}

    def overprediction(self):
        """-> float64 [n] on the device, log(areas[1] + 1) - log(areas[2] + 1): how much more often a class is predicted than
        labelled, 0 for a class neither predicted nor present.  The data-driven direction of `Segmenter.bias_sweep_raw`
        (subtracting it makes the over-predicted classes rarer).  Does not synchronise with the host."""
        a = self.areas.double()
        return torch.log(a[1] + 1.0) - torch.log(a[2] + 1.0)

    def _refuse_out_of_range(self, bad):
        """bad: tally[1] as the host read it"""
        if bad != 0:
            raise IndexError("SegmentationScore: tally[1] = %d ground-truth pixels hold a class outside [0, %d) that is not an "
                             "ignore value (wrong raw_labels, or a label map of another dataset?)" % (int(bad), self.n))

    def summary(self):
        """-> {"aAcc", "mIoU", "mAcc", "IoU": [n], "Acc": [n], "pixels"} by `SegCriterion.reduce_metrics`' formulas and rounding
        (nanmean over the classes, round(..., 4)).  The one place that synchronises with the host.  Ground truth out of range
        is an IndexError: the reference's F.cross_entropy fails on such a label, and a score that left pixels out is not
        reported as if it had not.  A score with boundary counters b also gives "mBIoU" and "BIoU": [n], Boundary IoU =
        b[0] / (b[1] + b[2] - b[0]) per class, with the same nanmean and rounding, in the same round trip.  A score with
        trimap counters also gives `trimap_summary()`'s "trimap_radii", "trimap_mIoU", "trimap_aAcc" and "trimap_pixels", [K]
        each, in the same round trip.  A score with calibration counters also gives "ECE" = sum_m (N_m / N) |acc_m - conf_m| over `reliability(16)`'s bins of all classes
        together, "MCE", the largest |acc_m - conf_m| of a non-empty bin, and "cECE": [n], the ECE of every predicted class
        alone (NaN for a class never predicted; ECE and MCE are NaN without pixels): float64 from the integers, NOT rounded, in
        the same round trip.  A fine bin's confidence is its midpoint, so each is within 1 / 512 of the figure the raw
        confidences would give for the same bins."""
        m, n = self.logging_output(), self.n
        ai, ap, al, au = m["area_intersect"], m["area_pred_label"], m["area_label"], m["area_union"]
        iou, acc = ai / au, ai / al
        parts = [torch.stack([ai.sum() / ap.sum(), torch.nanmean(iou), torch.nanmean(acc)]), iou, acc, self.tally.double()]
        if self.boundary is not None:
            b = self.boundary.double()
            biou = b[0] / (b[1] + b[2] - b[0])
            parts += [torch.nanmean(biou)[None], biou]
        if self.trimap is not None:
            parts.append(self._trimap_figures(False))
        if self.calibration is not None:
            ece, mce = _calibration_errors(*_reliability_bins(self.calibration, 16, False))
            parts += [ece, mce, _calibration_errors(*_reliability_bins(self.calibration, 16, True))[0]]
        flat = torch.cat(parts).tolist()
        self._refuse_out_of_range(flat[3 + 2 * n + 1])
        r4 = lambda v: round(float(v), 4)
        out = {"aAcc": r4(flat[0]), "mIoU": r4(flat[1]), "mAcc": r4(flat[2]), "IoU": [r4(v) for v in flat[3:3 + n]],
               "Acc": [r4(v) for v in flat[3 + n:3 + 2 * n]], "pixels": int(flat[3 + 2 * n])}
        if self.boundary is not None:
            out["mBIoU"] = r4(flat[5 + 2 * n])
            out["BIoU"] = [r4(v) for v in flat[6 + 2 * n:6 + 3 * n]]
        if self.trimap is not None:
            at = 5 + 2 * n + (0 if self.boundary is None else 1 + n)
            out.update(self._trimap_read(flat[at:at + 3 * len(self.trimap_radii)], False))
        if self.calibration is not None:
            at = len(flat) - n - 2
            out["ECE"], out["MCE"], out["cECE"] = flat[at], flat[at + 1], flat[at + 2:]
        return out

    def _trimap_figures(self, per_class):
        """the trimap's figures on the cumulative sums over the rings, `summary()`'s formulas: float64 [3 K] = aAcc, mIoU and
        the scored pixels within each radius, and with `per_class` the K n per-class IoUs behind them"""
        if self.trimap is None:
            raise ValueError("SegmentationScore.trimap_summary needs trimap counters: SegmentationScore(n, trimap=True), "
                             "evaluate_raw(..., trimap=True)")
        c = self.trimap.cumsum(0).double()
        ai, ap, al = c[:, 0], c[:, 1], c[:, 2]
        iou = ai / (ap + al - ai)
        parts = [ai.sum(1) / ap.sum(1), torch.stack([torch.nanmean(row) for row in iou]), al.sum(1)]
        return torch.cat(parts + ([iou.reshape(-1)] if per_class else []))

    def _trimap_read(self, flat, per_class):
        """`_trimap_figures` as the host read it -> the dictionary's entries"""
        K, n = len(self.trimap_radii), self.n
        r4 = lambda v: round(float(v), 4)
        out = {"trimap_radii": list(self.trimap_radii), "trimap_mIoU": [r4(v) for v in flat[K:2 * K]],
               "trimap_aAcc": [r4(v) for v in flat[:K]], "trimap_pixels": [int(v) for v in flat[2 * K:3 * K]]}
        if per_class:
            out["trimap_IoU"] = [[r4(v) for v in flat[3 * K + k * n:3 * K + (k + 1) * n]] for k in range(K)]
        return out

    def trimap_summary(self, per_class=False):
        """-> {"trimap_radii": [K], "trimap_mIoU": [K], "trimap_aAcc": [K], "trimap_pixels": [K]}, and with `per_class`
        "trimap_IoU": [K][n]: `summary()`'s mIoU / aAcc / IoU (its formulas and rounding) restricted to the scored pixels within
        r_k of a ground-truth contour -- the cumulative sums of the rings' counters -- and the number of those pixels.  Needs
        trimap counters (ValueError without them).  One host round trip."""
        return self._trimap_read(self._trimap_figures(per_class).tolist(), per_class)


def source_tokens(category_token_ids, prompt_ids=PROMPT_IDS, num_seg_tokens=None):
    """bos + prompt + the category names back to back + eos, int64 [L] (segmentation_dataset.py:143-160: the prompt the
    model was tuned with, then every class name)"""
    names = [torch.as_tensor(x, dtype=torch.long).reshape(-1) for x in category_token_ids]
    if num_seg_tokens is not None and len(names) != num_seg_tokens:
        raise ValueError("Segmenter: %d category names for a model with num_seg_tokens = %d" % (len(names), num_seg_tokens))
    return torch.cat([torch.tensor([BOS], dtype=torch.long), torch.as_tensor(list(prompt_ids), dtype=torch.long)] + names
                     + [torch.tensor([EOS], dtype=torch.long)])


def _check_classes(n, want_uint8=False):
    if n < 1 or n > MAX_CLASSES:
        raise ValueError("Segmenter: n = %d classes, hip.seg_predict takes 1 .. %d" % (n, MAX_CLASSES))
    if want_uint8 and n > 256:
        raise ValueError("Segmenter: uint8 labels hold at most 256 classes, the model has n = %d (int16 labels)" % n)


def _check_pamr(pamr_iters, pamr_dilations, crf_iters):
    """the two PAMR keywords of the Segmenter, checked -> (pamr_iters, the dilations as a tuple of ints)"""
    if isinstance(pamr_iters, bool) or not isinstance(pamr_iters, int) or pamr_iters < 0:
        raise ValueError("Segmenter: pamr_iters must be an int >= 0, got %r" % (pamr_iters,))
    if pamr_iters > 0 and crf_iters > 0:
        raise ValueError("Segmenter: pamr_iters = %d together with crf_iters = %d: the two refinements take the same slot, "
                         "choose one" % (pamr_iters, crf_iters))
    if not isinstance(pamr_dilations, (tuple, list)) or not 1 <= len(pamr_dilations) <= hip.SEG_PAMR_MAX_DILATIONS \
            or any(isinstance(d, bool) or not isinstance(d, int) or not 1 <= d <= hip.SEG_PAMR_MAX_DILATION for d in pamr_dilations):
        raise ValueError("Segmenter: pamr_dilations must be 1 .. %d ints in 1 .. %d, got %r"
                         % (hip.SEG_PAMR_MAX_DILATIONS, hip.SEG_PAMR_MAX_DILATION, pamr_dilations))
    return pamr_iters, tuple(pamr_dilations)


def _pamr_bytes(rgb):
    """the CRF's images (RGB in 0 .. 255, any dtype) as what `hip.seg_pamr` takes: rounded and clamped to bytes"""
    if torch.is_tensor(rgb):
        return rgb if rgb.dtype == torch.uint8 else rgb.round().clamp(0, 255).to(torch.uint8)
    return [_pamr_bytes(t) for t in rgb]


class Segmenter:
    sieve, sieve_connectivity, sieve_passes, sieve_moved = None, 4, 2, None      # off, unless the constructor says otherwise
    _class_bias = None

    def __init__(self, model, task=None, category_token_ids=None, prompt_ids=PROMPT_IDS, upsample="probs", smooth_iters=0,
                 smooth_topk=3, temperature=1.0, crf_iters=0, full_context_alignment=False, label_dtype=None, slide_views=False,
                 pamr_iters=0, pamr_dilations=PAMR_DILATIONS, sieve=None, sieve_connectivity=4, sieve_passes=2, class_bias=None):
        """model: a SegOFAModel on the device.  The class names come from `category_token_ids` (one id sequence per class),
        else the task's `category_token_ids`, else the task's `category_list` through `task.encode_category`.
        upsample: "probs" resizes the per-patch softmax (temperature), the reference demo's order; "logits" resizes the raw
        scores, the criterion's eval order.  smooth_iters > 0: both feed hip.neighbour_smoothing's probabilities.
        crf_iters > 0: mean-field iterations of crf.rgb_dense_crf on the resized values.
        pamr_iters > 0: iterations of pixel-adaptive mask refinement (`hip.seg_pamr`, csrc/pamr.hip; `pamr_reference` is the
        specification) on the resized values, guided by the ORIGINAL uint8 photo, in the slot of the CRF and not together with
        it: the predict launch hands over every class's value and `hip.seg_pamr` supplies the labels, conf and probs, in every
        setting (single view, ms+flip, slide, slide over views).  Its cost is linear in the pixels, and every value stays a
        convex combination of the values it was given, so conf keeps its meaning (a probability where it was one).
        pamr_dilations: 1 .. 8 ints in 1 .. 32, the rings of 8 neighbours; the defaults are the published ones, with
        pamr_iters=10.  Not built: a batch dimension (one `hip.seg_pamr` per image), PAMR inside `calibrate_raw` (a ValueError).
        label_dtype: None (uint8 up to 256 classes, else int16) or torch.uint8 to insist on bytes.
        slide_views: False: `slide` takes a single view, as ever.  True: `segment_raw` / `evaluate_raw(slide=...)` slide over
        EVERY view of `scales` and `flip` and finish each image with one launch of `hip.seg_predict_slide_views` (see
        `segment_raw`).
        sieve: None: off, the launches as ever.  K (an int >= 1): every label map this Segmenter decides on is finished by one
        `hip.seg_sieve(labels, K, sieve_connectivity, sieve_passes, n=n, conf=conf)` (csrc/sieve.hip; `sieve_reference` is the
        specification and states the rule): connected regions (sieve_connectivity 4 or 8) of fewer than K pixels take the
        value of their largest 4-adjacent neighbour region, sieve_passes (1 .. 8) times over -- islands vanish, holes close.
        It runs behind the CRF / PAMR where those are on and in every setting (single view, ms+flip, slide, slide over views;
        `__call__`, `segment_raw` and everything built on them: `render_raw`, `pseudo_label_raw`, `evaluate_raw`, `evaluate`).
        conf is set to 0 where the sieve changed the label (the model never stated a confidence for the label such a pixel
        carries now: under `pseudo_label_raw` it has bin 0, is dropped by any floor > 0 or keep < 1, and has weight 1 under
        return_weight where it is kept); probs, where asked for, are returned as they were, NOT re-ranked.  `sieve_moved`,
        int64 [2, n] on the device (None before the first sieved call), accumulates `hip.seg_sieve`'s moved over the calls:
        per class the pixels that left and that joined; nothing synchronises with the host.  Not built: the sieve inside
        `calibrate_raw` / `calibrate` and calibration counters behind a sieve (both a ValueError).
        class_bias: None: no per-class term, the launches as ever.  A tensor or sequence of n finite numbers, in logit units,
        kept as fp32 [n] on the model's device (`seg.class_bias`, assignable afterwards through the same check): it is
        SUBTRACTED from the logits in front of the temperature, a_c = (z_c - b_c) / T with z the bf16 logit widened to fp32
        and the difference one fp32 subtraction -- a positive entry makes a class rarer (prior-shift correction; logit
        adjustment, Menon et al., ICLR 2021; the calibration factor of the zero-shot segmentation tables).  "probs" and the
        smoothing take the softmax of a, so every value stays a probability and every consumer of one keeps its meaning;
        "logits" resizes z_c - b_c (no temperature, as without it).  `patch_scores` / `patch_scores_at` then call
        `hip.rows_to_f32_biased` / `hip.neighbour_smoothing(bias=)` (csrc/bsweep.hip), and because the bias is part of the
        grid it holds in every setting and method with no other change.  `bias_sweep_raw` finds its strength."""
        if upsample not in ("probs", "logits"):
            raise ValueError("Segmenter: upsample must be 'probs' or 'logits', got %r" % (upsample,))
        self.model, self.task = model, task
        self.n = int(model.cfg.num_seg_tokens)
        if label_dtype not in (None, torch.uint8, torch.int16):
            raise ValueError("Segmenter: label_dtype must be None, torch.uint8 or torch.int16, got %r" % (label_dtype,))
        _check_classes(self.n, want_uint8=label_dtype == torch.uint8)
        names = category_token_ids
        if names is None:
            names = getattr(task, "category_token_ids", None)
        if names is None:
            cats = getattr(task, "category_list", "") or ""
            cats = [x.strip() for x in cats.split(",")] if cats else []
            if task is None or not cats:
                raise ValueError("Segmenter: no class names -- pass category_token_ids, or a task with category_token_ids "
                                 "or category_list (+ BPE)")
            names = [task.encode_category(" %s" % x) for x in cats]
        self.src = source_tokens(names, prompt_ids, self.n)
        self.upsample, self.temperature = upsample, float(temperature)
        self.smooth_iters, self.smooth_topk, self.crf_iters = int(smooth_iters), int(smooth_topk), int(crf_iters)
        self.pamr_iters, self.pamr_dilations = _check_pamr(pamr_iters, pamr_dilations, self.crf_iters)
        self.sieve, self.sieve_connectivity, self.sieve_passes = _check_sieve(sieve, sieve_connectivity, sieve_passes)
        self.sieve_moved = None
        self.full_context_alignment = bool(full_context_alignment)
        self.label_dtype = label_dtype
        self.slide_views = bool(slide_views)
        self._src_dev = None
        self._palette_dev = None
        self.class_bias = class_bias

    @property
    def class_bias(self):
        """the per-class bias, fp32 [n] on the model's device, or None (see the constructor)"""
        return self._class_bias

    @class_bias.setter
    def class_bias(self, value):
        self._class_bias = None if value is None else _check_bias("Segmenter", "class_bias", value, self.n,
                                                                  next(self.model.parameters()).device)

    # -- inputs --------------------------------------------------------------------------
    @staticmethod
    def prepare_images(images):
        """-> (normalised float [B, 3, H, W], RGB in 0..255 as float [B, H, W, 3] or None when the input was already normalised)"""
        if images.dtype == torch.uint8:
            if images.dim() == 3:
                images = images[None]
            if images.dim() != 4 or images.shape[-1] != 3:
                raise ValueError("Segmenter: uint8 images must be RGB [B, H, W, 3] or [H, W, 3], got %s" % (tuple(images.shape),))
            rgb = images.float()
            return ((rgb / 255.0 - 0.5) / 0.5).permute(0, 3, 1, 2).contiguous(), rgb
        if not images.dtype.is_floating_point or images.dim() != 4 or images.shape[1] != 3:
            raise ValueError("Segmenter: images must be normalised float [B, 3, H, W] or uint8 RGB [B, H, W, 3] / [H, W, 3], "
                             "got %s %s" % (images.dtype, tuple(images.shape)))
        return images, None

    def net_input(self, patch_images):
        B, dev = patch_images.shape[0], patch_images.device
        if self._src_dev is None or self._src_dev.device != dev:
            self._src_dev = self.src.to(dev)
        L = self.src.numel()
        return {"src_tokens": self._src_dev[None].expand(B, L).contiguous(),
                "src_lengths": torch.full((B,), L, dtype=torch.long, device=dev),
                "patch_images": patch_images,
                "patch_masks": torch.ones(B, dtype=torch.bool, device=dev),
                "prev_output_tokens": torch.full((B, 1), BOS, dtype=torch.long, device=dev)}

    @staticmethod
    def _sizes(out_hw, B, HW, crf, has_crf_images):
        """-> (list of B (h, w) or None for one size, the one size)"""
        if out_hw is None:
            return None, tuple(HW)
        if len(out_hw) == 2 and all(isinstance(v, int) for v in out_hw):
            one = (int(out_hw[0]), int(out_hw[1]))
            if crf and one != tuple(HW) and not has_crf_images:
                raise ValueError("Segmenter: crf_images is required when out_hw %s differs from the input size %s (the CRF needs "
                                 "the image at the output resolution)" % (one, tuple(HW)))
            return None, one
        sizes = [(int(a), int(b)) for a, b in out_hw]
        if len(sizes) != B:
            raise ValueError("Segmenter: out_hw lists %d sizes for a batch of %d" % (len(sizes), B))
        if crf and not has_crf_images and any(s != tuple(HW) for s in sizes):
            raise ValueError("Segmenter: crf_images is required when out_hw %s differs from the input size %s (the CRF needs "
                             "the image at the output resolution)" % (sizes, tuple(HW)))
        return sizes, None

    # -- the call ------------------------------------------------------------------------
    def patch_scores(self, patch_images):
        """model forward -> (scores fp32 [B, hp*wp, n] in the chosen mode, hp, wp)"""
        pad, hp, wp, feat = self._padded_logits(patch_images)
        with torch.no_grad():
            if self._class_bias is not None:
                scores = self._biased_grid(pad, hp, wp, feat, self._class_bias)
            elif self.smooth_iters > 0:
                scores = hip.neighbour_smoothing(pad, self.n, feat, self.smooth_iters, self.smooth_topk, self.temperature)
            else:
                scores = hip.rows_to_f32(pad, self.n, hp * wp, softmax=self.upsample == "probs", temperature=self.temperature)
        return scores, hp, wp

    def _biased_grid(self, pad, hp, wp, feat, bias, temperature=None, softmax=None):
        """`patch_scores`' grid of one forward's padded logits under the per-class `bias` (fp32 [n] on the device), through the
        biased bindings; temperature / softmax: None for the Segmenter's own"""
        T = self.temperature if temperature is None else temperature
        if self.smooth_iters > 0:
            return hip.neighbour_smoothing(pad, self.n, feat, self.smooth_iters, self.smooth_topk, T, bias=bias)
        return hip.rows_to_f32_biased(pad, self.n, hp * wp, bias, softmax=self.upsample == "probs" if softmax is None else softmax,
                                      temperature=T)

    def patch_scores_biased(self, patch_images, biases):
        """ONE model forward -> (grids fp32 [K, B, hp*wp, n], hp, wp): that forward's padded logits under each of the K per-class
        biases (fp32 [n] on the device each), in the Segmenter's own mode, temperature and smoothing -- grid k is bit for bit
        what `patch_scores` of this Segmenter with `class_bias = biases[k]` gives.  The Segmenter's own `class_bias` is not
        consulted."""
        pad, hp, wp, feat = self._padded_logits(patch_images)
        with torch.no_grad():
            return torch.stack([self._biased_grid(pad, hp, wp, feat, b) for b in biases]), hp, wp

    def _padded_logits(self, patch_images):
        """model forward in eval mode -> (the padded logits bf16 [B, T, ld], hp, wp, the trunk features [B, hp*wp, D]): what
        `patch_scores` turns into scores, before the temperature enters"""
        model = self.model
        was_training = model.training
        if was_training:
            model.eval()
        try:
            with torch.no_grad():
                _, extra = model(**self.net_input(patch_images), full_context_alignment=self.full_context_alignment)
        finally:
            if was_training:
                model.train()
        hp, wp = extra["encoder_returns"]["image_embed_shape"][0]
        return extra["logits_padded"], hp, wp, extra["encoder_returns"]["image_embed_before_proj"][0]

    def patch_scores_at(self, patch_images, temperatures):
        """ONE model forward -> (grids fp32 [K, B, hp*wp, n], hp, wp): the class probabilities of that forward's padded logits at
        each of the K temperatures, `hip.rows_to_f32(softmax=True, temperature=T_k)` (with `smooth_iters > 0`:
        `hip.neighbour_smoothing(..., T_k)`) run K times -- grid k is bit for bit what `patch_scores` of a
        `Segmenter(temperature=T_k, upsample="probs")` gives.  The Segmenter's own `temperature` is not consulted; its
        `class_bias`, where set, is (the biased bindings, with the same bias at every temperature)."""
        pad, hp, wp, feat = self._padded_logits(patch_images)
        with torch.no_grad():
            if self._class_bias is not None:
                grids = [self._biased_grid(pad, hp, wp, feat, self._class_bias, T, True) for T in temperatures]
            elif self.smooth_iters > 0:
                grids = [hip.neighbour_smoothing(pad, self.n, feat, self.smooth_iters, self.smooth_topk, T) for T in temperatures]
            else:
                grids = [hip.rows_to_f32(pad, self.n, hp * wp, softmax=True, temperature=T) for T in temperatures]
            return torch.stack(grids), hp, wp

    def _views_merge(self, vs):
        """the merge of the K views (scores, hp, wp, flip) of one image or batch; one plain view is the single-view kernel"""
        if len(vs) == 1 and not vs[0][3]:
            return _Merge(lambda h, w, **kw: hip.seg_predict(*vs[0][:3], h, w, **kw),
                          lambda gt, **kw: hip.seg_score(*vs[0][:3], gt, **kw))
        return _Merge(lambda h, w, **kw: hip.seg_predict_views(vs, h, w, **kw), lambda gt, **kw: hip.seg_score_views(vs, gt, **kw))

    def _slide_merge(self, vs, sl):
        """the merge of one image's views (scores [1, Nw, hpw*wpw, n], hpw, wpw, oh, ow, flip) under `slide` = (crop, stride): the
        slide-views kernel on a Segmenter built with `slide_views` (for one view too), else the windows kernel on the one view"""
        if self.slide_views:
            # raw logits are normalised per view behind the merge (mmseg's order); the per-patch softmax and the neighbour
            # smoothing hand over probabilities, whose merge is linear
            softmax = self.upsample == "logits" and self.smooth_iters == 0
            return _Merge(lambda h, w, **kw: hip.seg_predict_slide_views(vs, *sl, h, w, softmax, **kw),
                          lambda gt, **kw: hip.seg_score_slide_views(vs, *sl, gt, softmax, **kw))
        (one,) = vs
        return _Merge(lambda h, w, **kw: hip.seg_predict_windows(*one[:5], *sl, h, w, **kw),
                      lambda gt, **kw: hip.seg_score_windows(*one[:5], *sl, gt, **kw))

    def _label(self, merge, h, w, rgb, return_conf, return_probs):
        """one image (or batch) from its merge to a SegmentationResult at h x w: the predict launch, which with the CRF on hands
        every class's value to `_crf`, as it does with PAMR on; rgb: the CRF's images (with PAMR: as uint8), else None.  With
        the sieve on, `_sieve` finishes the labels"""
        crf = self.crf_iters > 0 or self.pamr_iters > 0
        out = merge.predict(h, w, conf=return_conf and not crf, probs=return_probs or crf, label_dtype=self.label_dtype)
        res = self._crf(out, rgb, return_conf, return_probs)
        return res if self.sieve is None else self._sieve(res)

    def _sieve(self, res):
        """the labels [B, h, w] of a result through one `hip.seg_sieve`, its conf zeroed where they changed, its probs kept"""
        labels = res.labels.contiguous()
        conf = None if res.conf is None else res.conf.contiguous()
        if self.sieve_moved is None or self.sieve_moved.device != labels.device:
            self.sieve_moved = torch.zeros(2, self.n, dtype=torch.int64, device=labels.device)
        labels, _ = hip.seg_sieve(labels, self.sieve, self.sieve_connectivity, self.sieve_passes, n=self.n, conf=conf,
                                  moved=self.sieve_moved)
        return SegmentationResult(labels, conf, res.probs)

    def _crf(self, out, rgb, return_conf, return_probs):
        labels, conf, probs = out
        if self.crf_iters > 0:
            from .crf import rgb_dense_crf
            q = torch.stack([rgb_dense_crf(rgb[b], probs[b], self.crf_iters) for b in range(probs.shape[0])])
            labels = q.argmax(1).to(labels.dtype)
            conf = q.amax(1) if return_conf else None
            probs = q if return_probs else None
        elif self.pamr_iters > 0:
            res = [hip.seg_pamr(probs[b], rgb[b].contiguous(), self.pamr_iters, self.pamr_dilations, conf=return_conf,
                                probs_out=return_probs, label_dtype=labels.dtype) for b in range(probs.shape[0])]
            labels, conf, probs = (None if col[0] is None else col[0][None] if len(col) == 1 else torch.stack(col)
                                   for col in zip(*res))
        return SegmentationResult(labels, conf, probs)

    def __call__(self, images, out_hw=None, crf_images=None, return_conf=False, return_probs=False):
        patch_images, rgb = self.prepare_images(images)
        B, _, H, W = patch_images.shape
        crf = self.crf_iters > 0 or self.pamr_iters > 0
        sizes, one = self._sizes(out_hw, B, (H, W), crf, crf_images is not None)
        if crf:
            if crf_images is not None:
                rgb = [torch.as_tensor(c).to(patch_images.device).float() for c in crf_images]
            elif rgb is None:
                rgb = ((patch_images.float() * 0.5 + 0.5) * 255.0).permute(0, 2, 3, 1).contiguous()
            if self.pamr_iters > 0:
                rgb = _pamr_bytes(rgb)
        scores, hp, wp = self.patch_scores(patch_images)
        with torch.no_grad():
            if sizes is None:
                return self._label(self._views_merge([(scores, hp, wp, False)]), *one, rgb, return_conf, return_probs)
            return [self._label(self._views_merge([(scores[b:b + 1], hp, wp, False)]), *s, rgb[b:b + 1] if crf else None,
                                return_conf, return_probs) for b, s in enumerate(sizes)]

    # -- raw images of any size ----------------------------------------------------------
    def segment_raw(self, images, max_batch=8, mean=None, std=None, reverse_channels=False, return_conf=False,
                    return_probs=False, scales=(1.0,), flip=False, slide=None):
        """Raw images in, as they come off disk: one uint8 RGB [H, W, 3] tensor or a list of them, of differing shapes, on the
        host or the device -> a list of SegmentationResult in input order, image i with labels [H_i, W_i] (conf [H_i, W_i],
        probs [n, H_i, W_i]) on the device.

        Every image goes through the reference's evaluation transform (segmentation_dataset.py:169-172,218,256) in one kernel,
        `hip.image_load`: resized with its aspect kept so that the short side is at most P = model.cfg.patch_image_size and
        the long side at most 4 P (`imageio.eval_size`), the channel order KEPT (the reference reverses it twice, :218 `to BGR`
        for the mmseg transforms and :256 `to RGB` behind them, so the network was tuned on RGB, the order `__call__` feeds
        too; `reverse_channels=True` is for a model trained on BGR), normalised with `mean` / `std` -- 0.5 by
        default; `imageio.IMAGENET_DEFAULT_MEAN` / `IMAGENET_DEFAULT_STD` is the reference's other choice
        (`imagenet_default_mean_and_std`, :148-156).  The network runs at that variable aspect and the scores are resized to
        the image's own shape, as the reference scores at `ori_shape`.

        Images of equal source shape share one `image_load` launch, images of equal network size one forward of at most
        `max_batch` (`imageio.plan_views`).  With the CRF on, the ORIGINAL image is the CRF image, in RGB, not reversed.
        With device images nothing synchronises with the host, after the first call per (mean, std), which copies the
        normalisation table to the device.

        scales, flip: mmseg's `MultiScaleFlipAug(img_ratios=scales, flip=flip)`.  The views of an image are, per ratio in the
        order given, the image at `eval_size(H, W, P, ratio)` and then, with `flip`, that tensor mirrored along its width
        (mirrored after the resize, as mmseg does); each runs the forward above, views of equal network size sharing it
        (`imageio.plan_views`), and `hip.seg_predict_views` turns the views of an image into one label map at [H_i, W_i]: the
        mean of the resized, un-mirrored scores, which is also what the CRF takes.  At most 16 views; more than one view
        needs upsample="probs" (averaging raw logits is not mmseg's rule).  The default is the single view above: the same
        launches as without these arguments, `hip.seg_predict` at the end.

        slide: sliding-window inference, mmseg's `test_cfg=dict(mode='slide', crop_size, stride)`.  None: off, the launches
        above.  True: crop = P and stride = 2 P // 3 (341 at 512, 426 at 640, the usual configs); (crop, stride), each an int
        or an (h, w) pair: as given.  The image is resized to `eval_size(H, W, P, scales[0])` and cut into overlapping windows
        (`imageio.slide_windows`), written directly by `hip.image_load_windows`; every window runs the forward above (and
        the smoothing, per window) at the window's size -- with crop = P the trained grid, so no resized-bias entry is
        built and the windows of all images fill the same batches (`imageio.plan_slide_views`) -- and ONE launch of
        `hip.seg_predict_windows` per image resizes the windows' scores, averages them where windows overlap and resizes
        the result to [H_i, W_i]: no per-window [n, crop, crop] tensor, sum or count plane is written.  `slide_reference` is
        the specification; the reference never slides, so there is no golden for it.  Both `upsample` modes are allowed:
        "logits" is mmseg's single-scale order (the logits are merged, and the argmax is unchanged by the softmax mmseg
        applies afterwards), "probs" the demo's order (the per-patch softmax is merged).  A single view only: `slide` with
        several scales or `flip` is a ValueError, because mmseg applies the softmax between the window merge and the view
        average, which a kernel that is linear in the scores cannot express -- unless the Segmenter was built with
        `slide_views=True`: then every view of `scales` / `flip` is cut into windows (a mirrored view from the mirrored
        resized image), the windows of all views and images share the forwards (`imageio.plan_slide_views`), and ONE launch
        of `hip.seg_predict_slide_views` per image merges each view's windows, resizes to [H_i, W_i], un-mirrors and averages
        the views.  With upsample="logits" (and no smoothing) the launch applies the softmax per view between the merge and
        the average, mmseg's order, so several views are allowed with it here; with "probs" or the smoothing the scores are
        probabilities already and the launch is linear.  `slide_views_reference` is the specification.  At most 16 views
        and 64 windows per view."""
        sl = self._check_slide("segment_raw", slide, scales, flip)
        checked = self._check_raw("segment_raw", images, scales, flip, sl)
        plan = self._plan_slide(checked, sl, max_batch)
        if checked is None:
            return []
        imgs, shapes, merges = self._front(checked, sl, plan, max_batch, mean, std, reverse_channels)
        crf, out = self.crf_iters > 0, []
        with torch.no_grad():
            for i, merge in enumerate(merges):
                rgb = imgs[i][None].float() if crf else imgs[i][None] if self.pamr_iters > 0 else None
                r = self._label(merge, *shapes[i], rgb, return_conf, return_probs)
                out.append(SegmentationResult(*(None if t is None else t[0] for t in r)))
        return out

    def _check_raw(self, what, images, scales, flip, sl=None):
        """the arguments of `segment_raw` / `evaluate_raw`, checked on the host -> (the (ratio, flip) views, the images as a
        list, scales, flip), or None for an empty list.  sl: what `_check_slide` gave"""
        views = view_list(scales, flip)
        if len(views) > 1 and self.upsample != "probs" and not (self.slide_views and sl is not None):
            raise ValueError("Segmenter.%s: %d views need upsample='probs' (mmseg averages the resized probabilities; "
                             "averaging raw logits is not its rule), this Segmenter has upsample=%r" % (what, len(views), self.upsample))
        imgs = [images] if torch.is_tensor(images) else list(images)
        if not imgs:
            return None
        for im in imgs:
            if not torch.is_tensor(im) or im.dtype != torch.uint8 or im.dim() != 3 or im.shape[-1] != 3 or im.numel() == 0:
                raise ValueError("Segmenter.%s: every image must be a uint8 RGB [H, W, 3] tensor, got %s"
                                 % (what, (im.dtype, tuple(im.shape)) if torch.is_tensor(im) else type(im),))
        return views, imgs, scales, flip

    def _check_slide(self, what, slide, scales, flip):
        """the `slide` argument of `segment_raw` / `evaluate_raw`, checked on the host -> None (off) or (crop, stride)"""
        if slide is None or slide is False:
            return None
        if len(view_list(scales, flip)) > 1 and not self.slide_views:
            raise ValueError("Segmenter.%s: slide takes a single view, got scales=%r, flip=%r (mmseg applies the softmax between "
                             "the window merge and the view average)" % (what, tuple(scales), flip))
        P = int(self.model.cfg.patch_image_size)
        if slide is True:
            return P, 2 * P // 3
        if not isinstance(slide, (tuple, list)) or len(slide) != 2:
            raise ValueError("Segmenter.%s: slide must be None, True or (crop, stride), got %r" % (what, slide))
        crop, stride = slide
        slide_windows(1, 1, crop, stride)                     # crop and stride against the rule, on an image of one window
        return crop, stride

    def _plan_slide(self, checked, sl, max_batch):
        """the windows and launches of a `slide` call, on the host (more than 64 windows of an image is a ValueError here) ->
        (the images' (H, W), `imageio.plan_slide_views`' result: one unflipped view without `slide_views`), or None without `slide`
        or images"""
        if sl is None or checked is None:
            return None
        shapes = [(int(im.shape[0]), int(im.shape[1])) for im in checked[1]]
        return shapes, plan_slide_views(shapes, self.model.cfg.patch_image_size, sl[0], sl[1], checked[2], checked[3], max_batch)

    def _front(self, checked, sl, plan, max_batch, mean, std, reverse_channels):
        """everything of `segment_raw` and `evaluate_raw` in front of the last launch per image: the loads and the forwards of the
        setting -> (the images on the device, their (H, W), per image its `_Merge`)"""
        if sl is None:
            return self._raw_views(*checked, max_batch, mean, std, reverse_channels)
        return self._raw_window_views(checked[1], sl, plan, mean, std, reverse_channels)

    def _raw_window_views(self, imgs, sl, plan, mean, std, reverse_channels):
        """the front with `slide`: the windows of every view loaded in one launch per (source shape, size, flip), one forward per
        window size and `max_batch` windows of whatever view and image (`plan`: what `_plan_slide` gave; without `slide_views`
        it holds the one unflipped view) -> (the images on the device, their (H, W), per image the `_slide_merge` of its views
        (scores [1, Nw, hpw*wpw, n], hpw, wpw, oh, ow, flip) in view order)"""
        mean, std = HALF if mean is None else mean, HALF if std is None else std
        dev = next(self.model.parameters()).device
        shapes, (views, per_image, loads, forwards) = plan
        imgs = [im.to(dev, non_blocking=True) for im in imgs]
        x, grid = {}, {}
        got = [[[None] * (len(ys) * len(xs)) for _, ys, xs, _ in pv] for pv in per_image]
        with torch.no_grad():
            for _, size, flipped, idx in loads:
                t = hip.image_load_windows(torch.stack([imgs[i] for i in idx]), size[0], size[1], sl[0], sl[1], mean, std,
                                           reverse_channels, flip=flipped)
                for k, wins in enumerate(t.chunk(len(idx))):
                    x[idx[k], size, flipped] = wins
            for size, ivk in forwards:
                scores, hp, wp = self.patch_scores(torch.stack([x[i, per_image[i][v][0], views[v][1]][k] for i, v, k in ivk]))
                for j, (i, v, k) in enumerate(ivk):
                    got[i][v][k], grid[i, v] = scores[j], (hp, wp)
        return imgs, shapes, [self._slide_merge([(torch.stack(got[i][v])[None], *grid[i, v], *per_image[i][v][0], views[v][1])
                                                 for v in range(len(views))], sl) for i in range(len(imgs))]

    def _raw_views(self, views, imgs, scales, flip, max_batch, mean, std, reverse_channels, scores=None, merge=None):
        """the front without `slide`: every image loaded once per ratio, one forward per network size -> (the images on the
        device, their (H, W), per image the `_views_merge` of its views (scores [1, hp*wp, n], hp, wp, flip) in view order).
        scores: what a batch goes through in place of `patch_scores`, -> (a tensor whose first dimension is the batch's, hp,
        wp); merge: what an image's views go through in place of `_views_merge`"""
        scores, merge = scores or self.patch_scores, merge or self._views_merge
        mean, std = HALF if mean is None else mean, HALF if std is None else std
        dev = next(self.model.parameters()).device
        imgs = [im.to(dev, non_blocking=True) for im in imgs]
        shapes = [(int(im.shape[0]), int(im.shape[1])) for im in imgs]
        _, loads, forwards = plan_views(shapes, self.model.cfg.patch_image_size, scales, flip, max_batch)
        x, per_image = {}, [[None] * len(views) for _ in imgs]
        with torch.no_grad():
            for _, size, idx in loads:
                t = hip.image_load(torch.stack([imgs[i] for i in idx]), size[0], size[1], mean, std, reverse_channels)
                for k, i in enumerate(idx):
                    x[i, size] = t[k]
            for size, iv in forwards:
                got, hp, wp = scores(torch.stack([x[i, size].flip(-1) if views[v][1] else x[i, size] for i, v in iv]))
                for k, (i, v) in enumerate(iv):
                    per_image[i][v] = (got[k:k + 1], hp, wp, views[v][1])
        return imgs, shapes, [merge(vs) for vs in per_image]

    # -- the label map as a picture --------------------------------------------------------
    def render_raw(self, images, palette=None, opacity=0.5, boundary=0, boundary_color=(255, 255, 255), fade_by_conf=False,
                   **segment_raw_kwargs):
        """`segment_raw` and the two pictures a person looks at, the reference demo's last three lines
        (visualize_segmentation_web.ipynb cell 4: `cmap[labels]` and `image * (1 - opacity) + cmap[labels] * opacity`), on the
        device -> a list of `RenderResult(picture, labels, conf)` in input order, picture uint8 [H_i, W_i, 3].

        images, and the keywords scales, flip, slide, max_batch, mean, std, reverse_channels: as in `segment_raw`, which runs
        unchanged (the CRF and the smoothing follow the Segmenter's construction); then ONE launch of `hip.seg_render` per
        image colours its label map over the ORIGINAL uint8 photo (`render_reference` states the rule, in integers).
        palette: None (`default_palette(n)`) or uint8 [>= n, 3], on the host or the device.  opacity in [0, 1]: 0.5 is the
        demo's "overlap" picture bit for bit, 1.0 its "segmentation" picture.  boundary = r in 0 .. 4: pixels with another class
        within r pixels are drawn in `boundary_color` (0: no contours).  fade_by_conf: the opacity of a pixel is scaled by the
        winning class's value there, so uncertain regions show the photo (`segment_raw(return_conf=True)`; a ValueError with
        the CRF on).  Host images are uploaded once and the pictures stay on the device; with device images (and a device or
        default palette after the first call) nothing synchronises with the host.  A bad argument is a ValueError before
        anything is launched."""
        extra = sorted(set(segment_raw_kwargs) - {"scales", "flip", "slide", "max_batch", "mean", "std", "reverse_channels"})
        if extra:
            raise TypeError("Segmenter.render_raw: unexpected keyword(s) %s" % ", ".join(extra))
        _render_args("Segmenter.render_raw", opacity, boundary, boundary_color)
        if fade_by_conf and self.crf_iters > 0:
            raise ValueError("Segmenter.render_raw: fade_by_conf needs the winning class's value, which the CRF path does not "
                             "hand over (crf_iters = %d)" % self.crf_iters)
        if palette is not None and (not torch.is_tensor(palette) or palette.dtype != torch.uint8 or palette.dim() != 2
                                    or palette.shape[1] != 3 or palette.shape[0] < self.n):
            raise ValueError("Segmenter.render_raw: palette must be a uint8 [>= %d, 3] tensor, got %s" % (
                self.n, (palette.dtype, tuple(palette.shape)) if torch.is_tensor(palette) else type(palette)))
        dev = next(self.model.parameters()).device
        imgs = [images] if torch.is_tensor(images) else list(images)
        imgs = [im.to(dev, non_blocking=True) if torch.is_tensor(im) else im for im in imgs]       # the one upload
        res = self.segment_raw(imgs, return_conf=fade_by_conf, **segment_raw_kwargs)
        if palette is None:
            if self._palette_dev is None or self._palette_dev.device != dev:
                self._palette_dev = default_palette(self.n).to(dev)
            palette = self._palette_dev
        palette = palette[:MAX_CLASSES].to(dev).contiguous()        # the labels are below n <= MAX_CLASSES
        with torch.no_grad():
            return [RenderResult(hip.seg_render(r.labels, im.contiguous(), palette, opacity, boundary, tuple(boundary_color),
                                                conf=r.conf if fade_by_conf else None), r.labels, r.conf if fade_by_conf else None)
                    for im, r in zip(imgs, res)]

    # -- pseudo-labels for self-training ---------------------------------------------------
    def _conf_setting(self, sl):
        """-> None where `segment_raw(return_conf=True)`'s conf is a probability in this construction (sl: what `_check_slide`
        gave), else the name of the setting that makes it something else"""
        if self.crf_iters > 0 or self.smooth_iters > 0 or self.upsample == "probs":
            return None         # the CRF's marginal; the smoothing's probabilities; the per-patch softmax, merged linearly
        if self.slide_views and sl is not None:
            return None         # `_slide_merge` asks the launch for the softmax per view behind the merge
        return "upsample=%r (conf is the winning class's resized raw logit)" % (self.upsample,)

    def _need_probability(self, what, sl, need="the confidence must be a probability",
                          remedy="use upsample='probs', the smoothing, the CRF, or slide_views with slide"):
        """a ValueError naming the setting where `_conf_setting(sl)` names one"""
        bad = self._conf_setting(sl)
        if bad is not None:
            raise ValueError("%s: %s, this Segmenter has %s; %s" % (what, need, bad, remedy))

    def pseudo_label_raw(self, images, keep=1.0, floor=0.0, boundary=0, raw_labels=True, hist=None, thresholds=None,
                         scales=(1.0,), flip=False, slide=None, max_batch=8, mean=None, std=None, reverse_channels=False,
                         return_weight=False, min_region=None, region_connectivity=4):
        """Unlabeled photographs -> label maps `task.train_sample` accepts, holding only the pixels the model is confident
        of: the self-training step (CBST, MaskCLIP+) that adapts the image-free model to a target domain, on the device ->
        a list of `PseudoLabelResult(labels uint8 [H_i, W_i], predicted, conf, kept)` in input order.

        images, scales, flip, slide, max_batch, mean, std, reverse_channels: as in `segment_raw`.  In this order:
          1. `segment_raw(..., return_conf=True)`, unchanged: the label map and the winning class's probability per image
             (on a `Segmenter(sieve=K)` the sieved map, a relabelled pixel with conf 0: bin 0, dropped by any floor > 0 or
             keep < 1, weight 1 under return_weight where it is kept);
          2. one launch of `hip.seg_conf_hist` per image adds its (class, confidence bin) pairs to `hist` -- a
             `ConfidenceHistogram` to accumulate into, so that the thresholds are balanced over a whole data set across
             calls, or None for a fresh one that spans this call's images;
          3. `hist.thresholds(keep, floor)` (`pseudo_thresholds` states the rule; on the device): keep=1, floor=tau is the fixed
             threshold tau, keep < 1 keeps the most confident `keep` share of every class.  thresholds: int32 [n] bins given by
             the caller instead (a previous pass's): steps 2 and 3 are skipped, and keep, floor and hist are not read;
          4. one launch of `hip.seg_pseudo` per image: a pixel is kept where its class's threshold is met and, with
             boundary = r in 1 .. 4, no other class lies within r pixels (`pseudo_label_reference` states the rule); kept pixels
             become class + 1 with raw_labels (what a `TrainTransform(raw_labels=True)`, the default, takes), else the class id;
             every other pixel 255, ignored by both.  return_weight: the same launch also writes the result's `weight`, uint8
             [H_i, W_i]: 0 where the pixel was dropped, else max(conf_bin(conf), 1) -- the per-pixel loss weight that
             `task.train_sample(..., weights=)` carries to the weighted criterion;
          5. with min_region = K (an int >= 1; None: this step does not exist and the call is the one above, launch for
             launch): one `hip.seg_region_drop` per image on the FILTERED map -- every connected region (region_connectivity 4
             or 8; `regions_reference` states the rule) of fewer than K pixels becomes 255 and its weights 0, the speckles the
             model predicted and the crumbs the filters of step 4 cut off alike; 255 itself is never a region to drop.  The
             result's `region_dropped` int64 [n] holds the dropped pixels per class, and kept[0] has them subtracted, on the
             device (`region_drop_reference` states the rule).
        Nothing synchronises with the host.  Between the passes every image's labels and conf stay alive: 5 bytes per pixel
        (6 with int16 labels) for the whole call, which bounds the images of one call, not of a data set.

        The confidence must be a probability: upsample="probs", the smoothing, the CRF, or `slide_views` sliding (the softmax
        inside the launch).  Raw logits (upsample="logits" elsewhere) are a ValueError naming the setting, as are more than
        254 classes (255 without raw_labels) for the uint8 map, before anything is launched."""
        what = "Segmenter.pseudo_label_raw"
        _boundary_arg(what, boundary)
        if self.n > hip.seg_pseudo_max_classes(raw_labels):
            raise ValueError("%s: the uint8 pseudo-label map holds at most %d classes with raw_labels=%s, the model has n = %d"
                             % (what, hip.seg_pseudo_max_classes(raw_labels), bool(raw_labels), self.n))
        _connectivity_arg(what + ": region_connectivity", region_connectivity)
        if min_region is not None:
            _min_region_arg(what, min_region)
        sl = self._check_slide("pseudo_label_raw", slide, scales, flip)
        self._need_probability(what, sl)
        dev = next(self.model.parameters()).device
        if thresholds is not None:
            if not torch.is_tensor(thresholds) or thresholds.dtype != torch.int32 or tuple(thresholds.shape) != (self.n,):
                raise ValueError("%s: thresholds must be an int32 [%d] tensor of bins, got %s" % (
                    what, self.n, (thresholds.dtype, tuple(thresholds.shape)) if torch.is_tensor(thresholds) else type(thresholds)))
        else:
            pseudo_thresholds(torch.zeros(1, CONF_BINS, dtype=torch.int64), keep, floor)          # keep and floor, on the host
            if hist is None:
                hist = ConfidenceHistogram(self.n, dev)
            elif not isinstance(hist, ConfidenceHistogram) or hist.n != self.n or hist.hist.device != dev:
                raise ValueError("%s: hist must be a ConfidenceHistogram of %d classes on %s" % (what, self.n, dev))
        res = self.segment_raw(images, max_batch=max_batch, mean=mean, std=std, reverse_channels=reverse_channels, return_conf=True,
                               scales=scales, flip=flip, slide=slide)
        with torch.no_grad():
            pairs = [(r.labels.contiguous(), r.conf.contiguous()) for r in res]
            if thresholds is None:
                for labels, conf in pairs:
                    hip.seg_conf_hist(labels, conf, self.n, hist=hist.hist, tally=hist.tally)
                thresholds = hist.thresholds(keep, floor)
            else:
                thresholds = thresholds.to(dev).contiguous()
            out = []
            for labels, conf in pairs:
                wt = None
                if return_weight:
                    pseudo, kept, wt = hip.seg_pseudo(labels, conf, thresholds, self.n, boundary, bool(raw_labels), weight=True)
                else:
                    pseudo, kept = hip.seg_pseudo(labels, conf, thresholds, self.n, boundary, bool(raw_labels))
                if min_region is None:
                    out.append(PseudoLabelResult(pseudo, labels, conf, kept, wt))
                    continue
                pseudo, dropped, _ = hip.seg_region_drop(pseudo, region_connectivity, min_region, fill=255, n=self.n,
                                                         raw_labels=bool(raw_labels), weight=wt)
                kept[0] -= dropped
                out.append(PseudoLabelResult(pseudo, labels, conf, kept, wt, region_dropped=dropped))
        return out

    # -- the list of objects -----------------------------------------------------------------
    def _region_args(self, what, min_region, connectivity, max_regions, ignore):
        _min_region_arg(what, min_region)
        _connectivity_arg(what, connectivity)
        _max_regions_arg(what, max_regions)
        _ignore_arg(what, ignore)

    def _wants_conf(self, sl):
        """whether the region tables of this construction sum a confidence: where it is a probability (`_conf_setting`), and
        behind PAMR, which keeps what it was given"""
        return self._conf_setting(sl) is None or self.pamr_iters > 0

    @staticmethod
    def _region_table(labels, conf, min_region, connectivity, max_regions, ignore):
        """one image's labels [H, W] (and conf) -> its RegionTable through one `hip.seg_region_table`"""
        labels = labels.contiguous()
        conf = None if conf is None else conf.contiguous()
        rows, sums, count, slot = hip.seg_region_table(labels, conf, connectivity, min_region, ignore, max_regions)
        return RegionTable(rows, sums, count, slot, labels, conf)

    def regions_raw(self, images, min_region=1, connectivity=4, max_regions=1024, ignore=None, max_batch=8, scales=(1.0,),
                    flip=False, slide=None, mean=None, std=None, reverse_channels=False):
        """Raw images -> what is in them: a list of `RegionTable` in input order, one row per connected region of the image's
        label map with its class value, area, bounding box, centroid sums and summed confidence, on the device.

        images, scales, flip, slide, max_batch, mean, std, reverse_channels: as in `segment_raw`, which runs unchanged (with a
        `Segmenter(sieve=K)` the sieved map, so behind `hip.seg_sieve`); then ONE `hip.seg_region_table` per image
        (`region_table_reference` states the rule): regions of `connectivity` 4 or 8 with at least min_region pixels and a
        value other than `ignore`, numbered in ascending order of their roots, the first max_regions of them in the table
        (`RegionTable.truncated()` says whether more were listed).  The confidence is summed where this construction's conf is
        a probability -- upsample="probs", the smoothing, the CRF, PAMR, or `slide_views` sliding; with raw logits
        (upsample="logits" elsewhere) no conf is asked of `segment_raw`, the tables' third sum is 0 and `RegionTable.conf` is
        None: the boxes need no confidence.  Nothing synchronises with the host; `RegionTable.to_list` is the one round trip.
        A bad argument is a ValueError before anything is launched."""
        what = "Segmenter.regions_raw"
        self._region_args(what, min_region, connectivity, max_regions, ignore)
        sl = self._check_slide("regions_raw", slide, scales, flip)
        res = self.segment_raw(images, max_batch=max_batch, mean=mean, std=std, reverse_channels=reverse_channels,
                               return_conf=self._wants_conf(sl), scales=scales, flip=flip, slide=slide)
        with torch.no_grad():
            return [self._region_table(r.labels, r.conf, min_region, connectivity, max_regions, ignore) for r in res]

    def regions(self, images, out_hw=None, min_region=1, connectivity=4, max_regions=1024, ignore=None, crf_images=None):
        """`regions_raw` for what `__call__` takes: a ready batch (and out_hw, crf_images as there) -> a list of `RegionTable`,
        one per image of the batch, each through one `hip.seg_region_table` behind `__call__`'s launches"""
        self._region_args("Segmenter.regions", min_region, connectivity, max_regions, ignore)
        res = self(images, out_hw=out_hw, crf_images=crf_images, return_conf=self._wants_conf(None))
        per_image = [(r.labels[0], None if r.conf is None else r.conf[0]) for r in res] if isinstance(res, list) else \
            [(res.labels[b], None if res.conf is None else res.conf[b]) for b in range(res.labels.shape[0])]
        with torch.no_grad():
            return [self._region_table(l, c, min_region, connectivity, max_regions, ignore) for l, c in per_image]

    # -- run-length label maps ------------------------------------------------------------------
    def _run_length_map(self, labels, max_runs):
        """one image's labels [H, W] -> its RunLengthMap through one `hip.seg_rle_encode`"""
        labels = labels.contiguous()
        runs, count = hip.seg_rle_encode(labels, max_runs)
        return RunLengthMap(runs, count, tuple(labels.shape), labels.dtype, self.n)

    def export_raw(self, images, max_runs=65536, max_batch=8, scales=(1.0,), flip=False, slide=None, mean=None, std=None,
                   reverse_channels=False):
        """Raw images -> their label maps as run tables in COCO's run order: a list of `RunLengthMap` in input order, on the
        device; `RunLengthMap.to_coco` gives COCO stuff results.

        images, scales, flip, slide, max_batch, mean, std, reverse_channels: as in `segment_raw`, which runs unchanged, with no
        conf asked for (behind the CRF / PAMR / sieve where this Segmenter has them); then ONE `hip.seg_rle_encode` per image
        (`rle_encode_reference` states the rule): the first max_runs runs of the map (`RunLengthMap.truncated()` says whether
        it has more).  Nothing synchronises with the host; `RunLengthMap.to_coco` is the one round trip.  A bad argument is a
        ValueError before anything is launched."""
        _max_runs_arg("Segmenter.export_raw", max_runs)
        res = self.segment_raw(images, max_batch=max_batch, mean=mean, std=std, reverse_channels=reverse_channels, scales=scales,
                               flip=flip, slide=slide)
        with torch.no_grad():
            return [self._run_length_map(r.labels, max_runs) for r in res]

    def export(self, images, out_hw=None, crf_images=None, max_runs=65536):
        """`export_raw` for what `__call__` takes: a ready batch (and out_hw, crf_images as there) -> a list of `RunLengthMap`,
        one per image of the batch, each through one `hip.seg_rle_encode` behind `__call__`'s launches"""
        _max_runs_arg("Segmenter.export", max_runs)
        res = self(images, out_hw=out_hw, crf_images=crf_images)
        maps = [r.labels[0] for r in res] if isinstance(res, list) else [res.labels[b] for b in range(res.labels.shape[0])]
        with torch.no_grad():
            return [self._run_length_map(l, max_runs) for l in maps]

    # -- scoring against ground truth -----------------------------------------------------
    def _score_into(self, what, into, dev, confusion=False, boundary_iou=False, shapes=(), calibration=False, sl=None,
                    trimap=False):
        """the score a scoring call adds to, its arguments checked before anything is launched.  shapes: the (h, w) of the
        ground-truth maps, in order: with boundary counters, each one's band must fit the kernel"""
        if not isinstance(confusion, bool):
            raise ValueError("Segmenter.%s: confusion must be True or False (a matrix to add to goes in with `into`), got %s"
                             % (what, type(confusion)))
        if not isinstance(calibration, bool):
            raise ValueError("Segmenter.%s: calibration must be True or False (counters to add to go in with `into`), got %s"
                             % (what, type(calibration)))
        if self.sieve is not None and (calibration or (isinstance(into, SegmentationScore) and into.calibration is not None)):
            raise ValueError("Segmenter.%s: calibration counters behind sieve = %d are not built (a relabelled pixel has no "
                             "confidence to count); score with a Segmenter(sieve=None)" % (what, self.sieve))
        ratio = None
        if boundary_iou is not False:
            ratio = 0.02 if boundary_iou is True else _boundary_ratio("Segmenter.%s: boundary_iou is True, False or a ratio" % what,
                                                                      boundary_iou)
        radii = None
        if trimap is not False:
            radii = default_trimap_radii() if trimap is True else _trimap_radii(
                "Segmenter.%s" % what, trimap, "trimap is True, False or a tuple of radii, which")
        if into is None:
            score = SegmentationScore(self.n, dev, confusion=confusion, boundary=ratio is not None,
                                      boundary_ratio=0.02 if ratio is None else ratio, calibration=calibration,
                                      trimap=radii is not None, trimap_radii=radii)
        else:
            if not isinstance(into, SegmentationScore) or into.n != self.n or into.areas.device != dev:
                raise ValueError("Segmenter.%s: into must be a SegmentationScore of %d classes on %s" % (what, self.n, dev))
            if confusion and into.confusion is None:
                raise ValueError("Segmenter.%s: confusion=True, but `into` carries no confusion matrix (SegmentationScore(n, device, "
                                 "confusion=True))" % what)
            if ratio is not None and into.boundary is None:
                raise ValueError("Segmenter.%s: boundary_iou=%r, but `into` carries no boundary counters (SegmentationScore(n, "
                                 "device, boundary=True))" % (what, boundary_iou))
            if ratio is not None and into.boundary_ratio != ratio:
                raise ValueError("Segmenter.%s: boundary_iou asks for a band of ratio %r, `into` counts bands of ratio %r"
                                 % (what, ratio, into.boundary_ratio))
            if calibration and into.calibration is None:
                raise ValueError("Segmenter.%s: calibration=True, but `into` carries no calibration counters (SegmentationScore(n, "
                                 "device, calibration=True))" % what)
            if radii is not None and into.trimap is None:
                raise ValueError("Segmenter.%s: trimap=%r, but `into` carries no trimap counters (SegmentationScore(n, device, "
                                 "trimap=True))" % (what, trimap))
            if radii is not None and into.trimap_radii != radii:
                raise ValueError("Segmenter.%s: trimap asks for the radii %r, `into` counts the radii %r"
                                 % (what, radii, into.trimap_radii))
            score = into
        if score.calibration is not None:
            self._need_probability("Segmenter.%s" % what, sl)
        if score.boundary is not None:
            for i, (h, w) in enumerate(shapes):
                d = boundary_distance(h, w, score.boundary_ratio)
                if d > hip.SEG_BOUNDARY_MAX_D:
                    raise ValueError("Segmenter.%s: image %d (%d x %d) has a boundary band of d = %d pixels at ratio %r, "
                                     "hip.seg_boundary_areas takes 1 .. %d" % (what, i, h, w, d, score.boundary_ratio,
                                                                               hip.SEG_BOUNDARY_MAX_D))
        return score

    def _count(self, score, merge, gt, raw_labels, rgb, return_labels):
        """The scoring step of `evaluate_raw` / `evaluate`: one image's (or batch's) merge against gt [B, h, w] into `score` -> its
        labels [B, h, w] or None.  The epilogue of the merge's scoring launch adds to the counters.  With the CRF (or PAMR, or the sieve) on, the
        label map comes from `_label` (rgb: the CRF's images), not from the scoring kernel, and `hip.seg_areas` counts it.  Where
        the score carries a confusion matrix, the launch is asked for its label map and `hip.seg_confusion` counts the pairs
        of the same labels behind it on the same stream; where it carries boundary counters, likewise, and
        `hip.seg_boundary_areas` counts the band areas of the same labels with d = `boundary_distance` of gt's size.  Where
        it carries calibration counters, the launch (with the CRF, `_label`) is asked for its conf as well and
        `hip.seg_calibration` counts labels, conf and gt behind the other two.  Where it carries trimap counters, the launch
        is asked for its label map as well and `hip.seg_trimap_areas` (the ground truth's distance plane, then the rings'
        counters) follows behind all of them."""
        kw = dict(raw_labels=raw_labels, areas=score.areas, tally=score.tally)
        pairs, bands, cal = score.confusion is not None, score.boundary is not None, score.calibration is not None
        rings = score.trimap is not None
        if self.crf_iters > 0 or self.pamr_iters > 0 or self.sieve is not None:
            res = self._label(merge, int(gt.shape[1]), int(gt.shape[2]), rgb, cal, False)
            labels, conf = res.labels.contiguous(), res.conf
            hip.seg_areas(labels, gt, self.n, **kw)
        else:
            labels, conf = merge.score(gt, labels=return_labels or pairs or bands or cal or rings, conf=cal,
                                       label_dtype=self.label_dtype, **kw)[2:4]
        if pairs:
            hip.seg_confusion(labels, gt, self.n, raw_labels, confusion=score.confusion)
        if bands:
            hip.seg_boundary_areas(labels, gt, self.n, boundary_distance(int(gt.shape[1]), int(gt.shape[2]), score.boundary_ratio),
                                   raw_labels, bareas=score.boundary)
        if cal:
            hip.seg_calibration(labels, conf.contiguous(), gt, self.n, raw_labels, calibration=score.calibration,
                                tally=score.calibration_tally)
        if rings:
            hip.seg_trimap_areas(labels, gt, self.n, score.trimap_radii, raw_labels, trimap=score.trimap)
        return labels if return_labels else None

    def evaluate_raw(self, images, label_maps, raw_labels=True, scales=(1.0,), flip=False, max_batch=8, mean=None, std=None,
                     reverse_channels=False, into=None, return_labels=False, slide=None, confusion=False, boundary_iou=False,
                     calibration=False, trimap=False):
        """`segment_raw` scored against ground truth on the device -> a `SegmentationScore` (or (score, [labels [H_i, W_i], ...])
        with `return_labels`, the labels being `segment_raw`'s).

        images, scales, flip, max_batch, mean, std, reverse_channels: as in `segment_raw`, whose pipeline this runs unchanged
        up to the last launch per image; that launch (`hip.seg_score` / `hip.seg_score_views`) also counts the label map it
        decides on against the image's ground truth and, without `return_labels`, writes nothing else.  With the CRF on, the
        CRF's argmax is counted by `hip.seg_areas`; with the sieve on (`Segmenter(sieve=K)`), likewise the sieved labels --
        predict, `hip.seg_sieve`, `hip.seg_areas` -- and the matrix and the bands follow on the sieved labels; calibration
        counters behind a sieve are a ValueError naming the setting, before anything is launched.
        label_maps: one uint8 / int16 [H, W] tensor or a list, on the host or the device, entry i of image i's shape.
        raw_labels=True: the label PNGs' values, 0 and 255 ignored and x -> class x - 1 (`areas_reference` states the rule);
        False: class ids, n and 255 ignored.  into: a score to accumulate into (a whole validation set needs no host round
        trip; `summary()` is the only one).  A mismatch of count, shape or dtype is a ValueError before anything is launched.
        slide: as in `segment_raw`; the last launch per image is then `hip.seg_score_windows` (`hip.seg_score_slide_views` on a
        Segmenter built with `slide_views=True`).
        confusion: True, or an `into` that carries a matrix: the score also counts which class is taken for which
        (`SegmentationScore.confusion`, int64 [n, n + 1]; `confusion_reference` is the specification).  In every setting the
        scoring launch then writes its label map and one launch of `hip.seg_confusion` per image counts the pairs of the same
        labels on the same stream; areas / tally still come from the epilogue and are bit for bit what they are without it,
        and no host synchronisation is added.  confusion=True with an `into` that has no matrix is a ValueError before
        anything is launched.
        boundary_iou: True (a band of 2 % of the image diagonal), a ratio in (0, 1), or an `into` that carries boundary
        counters: the score also counts Boundary IoU's band areas (`SegmentationScore.boundary`, int64 [3, n];
        `boundary_areas_reference` is the specification), and `summary()` gains "mBIoU" and "BIoU".  As with the matrix, the
        scoring launch writes its label map and one launch of `hip.seg_boundary_areas` per image counts the same labels (the
        CRF's with the CRF on) on the same stream, with d = `boundary_distance(H_i, W_i, ratio)`: the band is measured at the
        ground truth's resolution, the image's own.  areas, tally, the matrix and the labels are bit for bit what they are
        without it, no host synchronisation is added, and a call without it makes the launches it always made.  A ValueError
        before anything is launched: a ratio other than `into`'s, `into` without the counters, an image whose d passes
        `hip.SEG_BOUNDARY_MAX_D` = 64 (a diagonal above 3200 pixels at 2 %).
        calibration: True, or an `into` that carries calibration counters: the score also counts how often a confidence is
        right (`SegmentationScore.calibration`, int64 [n, 256, 2]: pixels per predicted class, confidence bin and hit;
        `calibration_reference` is the specification), and `summary()` gains "ECE", "MCE" and "cECE";
        `score.reliability()` is the diagram and `score.precision_thresholds(target)` the per-class thresholds of a measured
        precision for `pseudo_label_raw(thresholds=)`.  The scoring launch then also writes its labels and conf
        (`segment_raw(return_conf=True)`'s; with the CRF on, the CRF's) and one launch of `hip.seg_calibration` per image
        counts them on the same stream, behind the matrix's and the bands' launches.  Everything else is bit for bit what it
        is without it, no host synchronisation is added, and a call without it makes the launches it always made.  The
        confidence must be a probability: raw logits (upsample="logits" outside `slide_views` sliding) are a ValueError naming
        the setting, as in `pseudo_label_raw`; so are anything but a bool and calibration=True with an `into` that lacks the
        counters, all before anything is launched.
        trimap: True (`default_trimap_radii()` = 1, 2, 4, 8, 16, 32 pixels), a tuple of 1 .. 8 strictly ascending radii in
        1 .. 128, or an `into` that carries trimap counters: the score also counts WHERE the errors sit relative to the
        ground truth's contours (`SegmentationScore.trimap`, int64 [K, 3, n]: the three rows of `areas` per ring of the exact
        Euclidean distance to the nearest ground-truth pixel of another value; `trimap_areas_reference` is the
        specification), and `summary()` gains "trimap_radii", "trimap_mIoU", "trimap_aAcc" and "trimap_pixels";
        `score.trimap_summary(per_class=True)` adds the per-class IoU within every radius.  The scoring launch then writes
        its label map and `hip.seg_trimap_areas` counts the same labels per image on the same stream (two launches of
        `hip.seg_distance` on the ground truth, one counting launch), behind the matrix's, the bands' and the calibration's
        launches.  Everything else is bit for bit what it is without it, no host synchronisation is added, and a call
        without it makes the launches it always made.  Radii other than `into`'s, `into` without the counters and anything
        but True, False or such a tuple are ValueErrors before anything is launched."""
        sl = self._check_slide("evaluate_raw", slide, scales, flip)
        checked = self._check_raw("evaluate_raw", images, scales, flip, sl)
        plan = self._plan_slide(checked, sl, max_batch)
        gts = _check_label_maps("Segmenter.evaluate_raw", [] if checked is None else checked[1], label_maps)
        dev = next(self.model.parameters()).device
        score = self._score_into("evaluate_raw", into, dev, confusion, boundary_iou, [tuple(g.shape) for g in gts], calibration, sl,
                                 trimap)
        if checked is None:
            return (score, []) if return_labels else score
        gts = [g.to(dev, non_blocking=True).contiguous() for g in gts]
        imgs, shapes, merges = self._front(checked, sl, plan, max_batch, mean, std, reverse_channels)
        crf, out = self.crf_iters > 0, []
        with torch.no_grad():
            for i, merge in enumerate(merges):
                rgb = imgs[i][None].float() if crf else imgs[i][None] if self.pamr_iters > 0 else None
                labels = self._count(score, merge, gts[i][None], raw_labels, rgb, return_labels)
                out.append(None if labels is None else labels[0])
        return (score, out) if return_labels else score

    def evaluate(self, images, label_maps, raw_labels=True, into=None, return_labels=False, confusion=False, boundary_iou=False,
                 calibration=False, trimap=False):
        """`__call__` scored against ground truth: images as `__call__` takes them (normalised float [B, 3, H, W] or uint8 RGB
        [B, H, W, 3] / [H, W, 3]), label_maps uint8 / int16 [B, h, w] (or [h, w] for one image): the label map is taken at the
        ground truth's own size, as `out_hw` would.  -> a `SegmentationScore`, or (score, labels [B, h, w]) with `return_labels`;
        raw_labels, into, confusion, boundary_iou, calibration, trimap: as in `evaluate_raw`; the band areas of the whole batch are
        one launch of `hip.seg_boundary_areas`, d from the label maps' size, its calibration counts one of `hip.seg_calibration`,
        and its trimap counters one call of `hip.seg_trimap_areas` (distances never cross from one image into the next)."""
        gt = _check_batch_gt("Segmenter.evaluate", images, label_maps)
        patch_images, rgb = self.prepare_images(images)
        B, _, H, W = patch_images.shape
        crf = self.crf_iters > 0 or self.pamr_iters > 0
        if crf and tuple(gt.shape[1:]) != (H, W):
            raise ValueError("Segmenter.evaluate: with the CRF (crf_iters) or PAMR (pamr_iters) on, the label maps must have the "
                             "images' size %s, got %s" % ((H, W), tuple(gt.shape[1:])))
        score = self._score_into("evaluate", into, patch_images.device, confusion, boundary_iou, [tuple(gt.shape[1:])], calibration,
                                 trimap=trimap)
        if crf and rgb is None:
            rgb = ((patch_images.float() * 0.5 + 0.5) * 255.0).permute(0, 2, 3, 1).contiguous()
        if self.pamr_iters > 0:
            rgb = _pamr_bytes(rgb)
        scores, hp, wp = self.patch_scores(patch_images)
        with torch.no_grad():
            labels = self._count(score, self._views_merge([(scores, hp, wp, False)]), gt.to(patch_images.device).contiguous(),
                                 raw_labels, rgb, return_labels)
        return (score, labels) if return_labels else score

    # -- choosing the temperature ---------------------------------------------------------
    def _sweep_into(self, what, temperatures, into, dev, scales=(1.0,), flip=False, slide=None):
        """the sweep a calibrating call adds to, every argument and setting checked before anything is launched"""
        if len(view_list(scales, flip)) != 1 or flip:
            raise ValueError("Segmenter.%s: a temperature sweep takes one plain view, got scales=%r, flip=%r (the mean of several "
                             "views' probabilities is not one softmax of one forward's logits)" % (what, tuple(scales), flip))
        if slide is not None and slide is not False:
            raise ValueError("Segmenter.%s: a temperature sweep does not slide, got slide=%r (windows are merged before the "
                             "temperature could be applied per pixel)" % (what, slide))
        if self.crf_iters > 0:
            raise ValueError("Segmenter.%s: a temperature sweep scores the network's probabilities, this Segmenter has "
                             "crf_iters = %d (the CRF's marginals are not a function of one temperature)" % (what, self.crf_iters))
        if self.pamr_iters > 0:
            raise ValueError("Segmenter.%s: a temperature sweep scores the network's probabilities, this Segmenter has "
                             "pamr_iters = %d (the sweep's launch resizes and scores in one pass: PAMR inside it is not built)"
                             % (what, self.pamr_iters))
        if self.sieve is not None:
            raise ValueError("Segmenter.%s: a temperature sweep scores the network's probabilities, this Segmenter has "
                             "sieve = %d (the sweep never forms a label map to sieve)" % (what, self.sieve))
        self._need_probability("Segmenter.%s" % what, None, "the values must be probabilities", "use upsample='probs' or the smoothing")
        temps = _check_temperatures("Segmenter.%s" % what, default_temperatures() if temperatures is None else temperatures)
        if into is None:
            return TemperatureSweep(temps, dev, self.n)
        if not isinstance(into, TemperatureSweep) or into.temperatures != temps or into.n not in (None, self.n) or into.hist.device != dev:
            raise ValueError("Segmenter.%s: into must be a TemperatureSweep of the temperatures %r and %d classes on %s, got %s"
                             % (what, temps, self.n, dev, (into.temperatures, into.n, into.hist.device)
                                if isinstance(into, TemperatureSweep) else type(into)))
        into.n = self.n
        return into

    def calibrate_raw(self, images, label_maps, temperatures=None, raw_labels=True, max_batch=8, mean=None, std=None,
                      reverse_channels=False, into=None, scales=(1.0,), flip=False, slide=None):
        """Temperature scaling (Guo et al., ICML 2017) from a labelled validation set -> a `TemperatureSweep`: which softmax
        temperature makes this model's confidences mean what they say.  `evaluate_raw`'s front for a single plain view
        (images, label_maps, raw_labels, max_batch, mean, std, reverse_channels and the checks of images and label maps: as
        there), but the forward runs ONCE per batch; `patch_scores_at` then turns its padded logits into K grids of
        probabilities, one `hip.rows_to_f32(softmax=True, temperature=T_k)` (with the smoothing: `hip.neighbour_smoothing`)
        per temperature, and ONE launch of `hip.seg_temperature_sweep` per image (csrc/tsweep.hip) scores all K against the
        image's ground truth: per temperature the reliability counts, the summed NLL and the summed Brier score.  No
        [n, H, W] tensor exists and nothing synchronises with the host; `sweep.summary()` is the one round trip.
        temperatures: 1 .. 16 finite numbers > 0, None: `default_temperatures()`.  The Segmenter's own `temperature` is not
        consulted; afterwards `seg.temperature = sweep.best()`.  into: a sweep of the same temperatures, class count and
        device to accumulate into (a whole validation set).  `temperature_sweep_reference` is the specification.
        A ValueError naming the setting, before anything is launched: `scales` / `flip` other than one plain view, `slide`,
        `crf_iters > 0`, `pamr_iters > 0`, `sieve`, upsample="logits" without the smoothing (the values must be probabilities), a bad temperature list,
        an `into` that does not match."""
        what = "calibrate_raw"
        dev = next(self.model.parameters()).device
        sweep = self._sweep_into(what, temperatures, into, dev, scales, flip, slide)
        checked = self._check_raw(what, images, scales, flip)
        gts = _check_label_maps("Segmenter.calibrate_raw", [] if checked is None else checked[1], label_maps)
        if checked is None:
            return sweep
        gts = [g.to(dev, non_blocking=True).contiguous() for g in gts]

        def grids_at(x):                # sample-major, as `_raw_views` cuts a batch into its images
            grids, hp, wp = self.patch_scores_at(x, sweep.temperatures)
            return grids.transpose(0, 1), hp, wp

        per_image = self._raw_views(*checked, max_batch, mean, std, reverse_channels, scores=grids_at, merge=lambda vs: vs[0])[2]
        with torch.no_grad():
            for (grids, hp, wp, _), g in zip(per_image, gts):        # in image order: the sums do not depend on the batches
                grids = grids.transpose(0, 1).contiguous()
                hip.seg_temperature_sweep(grids, hp, wp, g[None], raw_labels, hist=sweep.hist, sums=sweep.sums, tally=sweep.tally)
        return sweep

    def calibrate(self, images, label_maps, temperatures=None, raw_labels=True, into=None):
        """`calibrate_raw` for what `evaluate` takes: images normalised float [B, 3, H, W] or uint8 RGB [B, H, W, 3] / [H, W, 3],
        label_maps uint8 / int16 [B, h, w] (or [h, w] for one image) -> a `TemperatureSweep`: one forward, K
        `hip.rows_to_f32` and one launch of `hip.seg_temperature_sweep` for the whole batch, at the ground truth's own size."""
        gt = _check_batch_gt("Segmenter.calibrate", images, label_maps)
        patch_images, _ = self.prepare_images(images)
        sweep = self._sweep_into("calibrate", temperatures, into, patch_images.device)
        grids, hp, wp = self.patch_scores_at(patch_images, sweep.temperatures)
        with torch.no_grad():
            hip.seg_temperature_sweep(grids, hp, wp, gt.to(patch_images.device).contiguous(), raw_labels, hist=sweep.hist,
                                      sums=sweep.sums, tally=sweep.tally)
        return sweep

    # -- choosing the class bias ----------------------------------------------------------
    def _bias_sweep_into(self, what, direction, strengths, into, dev, scales=(1.0,), flip=False, slide=None):
        """the sweep a bias-sweeping call adds to, every argument and setting checked before anything is launched"""
        if len(view_list(scales, flip)) != 1 or flip:
            raise ValueError("Segmenter.%s: a bias sweep takes one plain view, got scales=%r, flip=%r (the launch scores K grids of "
                             "one forward; the mean over several views is not built into it)" % (what, tuple(scales), flip))
        if slide is not None and slide is not False:
            raise ValueError("Segmenter.%s: a bias sweep does not slide, got slide=%r (the launch scores K grids of one forward; "
                             "the window merge is not built into it)" % (what, slide))
        if self.crf_iters > 0:
            raise ValueError("Segmenter.%s: a bias sweep scores the network's grids, this Segmenter has crf_iters = %d (the "
                             "sweep's launch resizes and scores in one pass: the CRF inside it is not built)" % (what, self.crf_iters))
        if self.pamr_iters > 0:
            raise ValueError("Segmenter.%s: a bias sweep scores the network's grids, this Segmenter has pamr_iters = %d (the "
                             "sweep's launch resizes and scores in one pass: PAMR inside it is not built)" % (what, self.pamr_iters))
        if self.sieve is not None:
            raise ValueError("Segmenter.%s: a bias sweep scores the network's grids, this Segmenter has sieve = %d (the sweep "
                             "never forms a label map to sieve)" % (what, self.sieve))
        direction = _check_bias("Segmenter.%s" % what, "direction", direction, self.n, dev)
        gs = _check_strengths("Segmenter.%s" % what, default_bias_strengths() if strengths is None else strengths)
        origin = torch.zeros(self.n, dtype=torch.float32, device=dev) if self._class_bias is None else self._class_bias.to(dev)
        if into is None:
            return BiasSweep(gs, direction, origin, dev)
        if not isinstance(into, BiasSweep) or into.n != self.n or into.areas.device != dev or not into._same(gs, direction, origin):
            raise ValueError("Segmenter.%s: into must be a BiasSweep of the strengths %r, this direction, this Segmenter's class_bias "
                             "as origin and %d classes on %s, got %s"
                             % (what, gs, self.n, dev, (into.strengths, into.n, into.areas.device) if isinstance(into, BiasSweep)
                                else type(into)))
        return into

    def bias_sweep_raw(self, images, label_maps, direction, strengths=None, raw_labels=True, max_batch=8, mean=None, std=None,
                       reverse_channels=False, into=None, scales=(1.0,), flip=False, slide=None):
        """The strength of a per-class bias from a labelled validation set -> a `BiasSweep`: how far along `direction` the logits
        must be shifted for the label maps to score best.  `evaluate_raw`'s front for a single plain view (images, label_maps,
        raw_labels, max_batch, mean, std, reverse_channels and the checks of images and label maps: as there), but the
        forward runs ONCE per batch; `patch_scores_biased` then turns its padded logits into K grids, one
        `hip.rows_to_f32_biased` (with the smoothing: `hip.neighbour_smoothing(bias=)`) per strength, in the Segmenter's own
        mode and temperature, and ONE launch of `hip.seg_score_grids` per image (csrc/bsweep.hip) scores all K against the
        image's ground truth: per strength the three rows of `SegmentationScore.areas`, so mIoU, mAcc, aAcc, the groups' mIoU
        and hIoU exist per strength.  No [n, H, W] tensor exists and nothing synchronises with the host; `sweep.summary()` is
        the one round trip.
        direction: a tensor or sequence of n finite numbers -- `score.overprediction()` (the data-driven one), a 0 / 1 mask of
        the seen classes (the zero-shot calibration factor), log(prior_source) - log(prior_target) (prior shift).
        strengths: 1 .. 16 finite numbers, None: `default_bias_strengths()`.  The Segmenter's own `class_bias` is the ORIGIN:
        row k is this Segmenter with `class_bias = scaled_bias(direction, strengths[k], origin)` (zeros for None), so
        strength 0 reproduces it and a second sweep along another direction continues from the first; afterwards
        `seg.class_bias = sweep.bias(sweep.best())`.  "probs", "logits" and the smoothing are all allowed: the counters need
        no probabilities.  into: a sweep of the same strengths, direction, origin, class count and device to accumulate into.
        `bias_sweep_reference` is the specification.
        A ValueError naming the setting, before anything is launched: `scales` / `flip` other than one plain view, `slide`,
        `crf_iters > 0`, `pamr_iters > 0`, `sieve`, a direction that is not n finite numbers, a bad strength list, an `into`
        that does not match."""
        what = "bias_sweep_raw"
        dev = next(self.model.parameters()).device
        sweep = self._bias_sweep_into(what, direction, strengths, into, dev, scales, flip, slide)
        checked = self._check_raw(what, images, scales, flip)
        gts = _check_label_maps("Segmenter.bias_sweep_raw", [] if checked is None else checked[1], label_maps)
        if checked is None:
            return sweep
        gts = [g.to(dev, non_blocking=True).contiguous() for g in gts]
        biases = [sweep.bias(k) for k in range(len(sweep.strengths))]

        def grids_at(x):                # sample-major, as `_raw_views` cuts a batch into its images
            grids, hp, wp = self.patch_scores_biased(x, biases)
            return grids.transpose(0, 1), hp, wp

        per_image = self._raw_views(*checked, max_batch, mean, std, reverse_channels, scores=grids_at, merge=lambda vs: vs[0])[2]
        with torch.no_grad():
            for (grids, hp, wp, _), g in zip(per_image, gts):        # in image order
                grids = grids.transpose(0, 1).contiguous()
                hip.seg_score_grids(grids, hp, wp, g[None], raw_labels, areas=sweep.areas, tally=sweep.tally)
        return sweep

    def bias_sweep(self, images, label_maps, direction, strengths=None, raw_labels=True, into=None):
        """`bias_sweep_raw` for what `evaluate` takes: images normalised float [B, 3, H, W] or uint8 RGB [B, H, W, 3] / [H, W, 3],
        label_maps uint8 / int16 [B, h, w] (or [h, w] for one image) -> a `BiasSweep`: one forward, K biased row launches and
        one launch of `hip.seg_score_grids` for the whole batch, at the ground truth's own size."""
        gt = _check_batch_gt("Segmenter.bias_sweep", images, label_maps)
        patch_images, _ = self.prepare_images(images)
        sweep = self._bias_sweep_into("bias_sweep", direction, strengths, into, patch_images.device)
        grids, hp, wp = self.patch_scores_biased(patch_images, [sweep.bias(k) for k in range(len(sweep.strengths))])
        with torch.no_grad():
            hip.seg_score_grids(grids, hp, wp, gt.to(patch_images.device).contiguous(), raw_labels, areas=sweep.areas,
                                tally=sweep.tally)
        return sweep
