"""The reference's evaluation transform for raw images: sizes, the CPU specification of `hip.image_load`, and the grouping
of `Segmenter.segment_raw` (`plan_views`; `plan_groups` is its single-view form).  Needs no GPU to import.

The reference evaluates an image as it comes off disk (segmentation_dataset.py:169-172,218,256):
`MultiScaleFlipAug(img_scale=(4 P, P), flip=False, [Resize(keep_ratio=True), ...])` resizes it so that the short side is at
most P and the long side at most 4 P (`eval_size`), and the result is normalised with mean / std 0.5, or the ImageNet
values under `imagenet_default_mean_and_std` (:148-156).  The dataset reverses the channels TWICE -- :218 `to BGR` in front of
the mmseg transforms, which expect BGR, and :256 (:243 in training) `to RGB` behind them -- so the two cancel: the network
sees RGB, as PIL delivers it, and `reverse_channels` is off by default (the switch is for a model trained on BGR).  `image_load_reference` is that transform as a specification in plain torch
indexing; `hip.image_load` (csrc/imgload.hip) is the implementation.

Sliding-window inference (`Segmenter.segment_raw(slide=...)`, mmseg's `test_cfg mode='slide'`): `slide_windows` is the window
rule, `plan_slide` the grouping of a call, `image_load_windows_reference` the specification of `hip.image_load_windows`;
`plan_slide_views` groups a call that slides over every view of multi-scale + flip (`Segmenter(slide_views=True)`).
"""
import torch

IMAGENET_DEFAULT_MEAN = (0.485, 0.456, 0.406)
IMAGENET_DEFAULT_STD = (0.229, 0.224, 0.225)
HALF = (0.5, 0.5, 0.5)


def eval_size(h, w, patch_image_size, ratio=1.0):
    """-> (oh, ow): mmcv's `rescale_size((w, h), (int(4 P ratio), int(P ratio)))` in Python floats.  `ratio` is one entry of
    `MultiScaleFlipAug(img_ratios=...)`, which scales the pair before `Resize(keep_ratio=True)` sees it."""
    P = int(patch_image_size)
    if h < 1 or w < 1 or P < 1:
        raise ValueError("eval_size: h, w and patch_image_size must be >= 1, got %r %r %r" % (h, w, patch_image_size))
    if not ratio > 0:
        raise ValueError("eval_size: ratio must be > 0, got %r" % (ratio,))
    long_side, short_side = int(4 * P * ratio), int(P * ratio)
    if short_side < 1:
        raise ValueError("eval_size: int(patch_image_size * ratio) = int(%d * %r) is below 1" % (P, ratio))
    s = min(long_side / max(h, w), short_side / min(h, w))
    return int(h * s + 0.5), int(w * s + 0.5)


def _triple(v, what):
    v = tuple(float(x) for x in v)
    if len(v) != 3:
        raise ValueError("image_load: %s must have three entries, got %r" % (what, v))
    return v


def normalisation_table(mean=HALF, std=HALF):
    """fp32 [3, 256] on the host: (k / 255 - mean[c]) / std[c] in torch fp32 -- every value `image_load` can return"""
    mean, std = _triple(mean, "mean"), _triple(std, "std")
    k = torch.arange(256, dtype=torch.float32) / 255
    return torch.stack([(k - mean[c]) / std[c] for c in range(3)])


def source_coords(out, inn, dtype=torch.float64, device=None):
    """one axis of the resize, `out` samples over `inn`: (i0 int64 [out], i1 int64 [out], lambda `dtype` [out]) by the
    integer rule -- num = max((2d+1) in - out, 0), i0 = min(num // (2 out), in-1), i1 = min(i0+1, in-1),
    lambda = float(num - i0 2 out) / float(2 out), 0 where i0 == i1"""
    d = torch.arange(out, dtype=torch.int64, device=device)
    num = ((2 * d + 1) * inn - out).clamp_min(0)
    i0 = (num // (2 * out)).clamp_max(inn - 1)
    i1 = (i0 + 1).clamp_max(inn - 1)
    lam = (num - i0 * (2 * out)).to(dtype) / torch.tensor(2 * out, dtype=torch.int64, device=device).to(dtype)
    return i0, i1, torch.where(i0 == i1, torch.zeros_like(lam), lam)


def resize_to_grey(src, ycoords, xcoords):
    """the resize step of both specifications (`image_load_reference`, `augment.train_load_reference`): src `dtype` [..., H0, W0],
    ycoords / xcoords: (i0, i1, lambda) per destination row / column as `source_coords` returns them (or a window of them) ->
    (q uint8 [..., rows, columns], v `dtype` the same shape): weights and the four-term sum
    v = w00 a + w01 b + w10 c + w11 d in `dtype`, q = clamp(floor(v + 0.5), 0, 255) as the reference's uint8 resize"""
    (y0, y1, ly), (x0, x1, lx) = ycoords, xcoords
    ly, lx = ly[:, None], lx[None, :]
    top, bot = src[..., y0, :], src[..., y1, :]
    v = ((1 - ly) * (1 - lx)) * top[..., x0] + ((1 - ly) * lx) * top[..., x1] + (ly * (1 - lx)) * bot[..., x0] \
        + (ly * lx) * bot[..., x1]
    return (v + 0.5).floor().clamp(0, 255).to(torch.uint8), v


def image_load_reference(images_u8, oh, ow, mean=HALF, std=HALF, reverse_channels=False, dtype=torch.float64,
                         out_dtype=torch.float32):
    """CPU specification of hip.image_load: uint8 [B, H0, W0, 3] -> (normalised `out_dtype` [B, 3, oh, ow], q uint8
    [B, 3, oh, ow], v `dtype` [B, 3, oh, ow]).  Bilinear resize with align_corners=False and no antialiasing
    (`F.interpolate` / `cv2.INTER_LINEAR`), the source coordinate in integers (`source_coords`), v and q by
    `resize_to_grey` in `dtype`; the output is `normalisation_table(mean, std)[c][q]`, channel c reading source channel 2 - c when
    `reverse_channels`.  Runs on any device.

    NOT pinned: `cv2` (what mmcv's Resize calls) evaluates the same filter with 11-bit fixed-point weights, and `cv2` is
    not available where this project is tested.  The share of pixels at which that fixed-point rounding lands on the
    neighbouring grey level has not been measured."""
    if images_u8.dtype != torch.uint8 or images_u8.dim() != 4 or images_u8.shape[-1] != 3:
        raise ValueError("image_load: images must be uint8 [B, H0, W0, 3], got %s %s" % (images_u8.dtype, tuple(images_u8.shape)))
    B, H0, W0, _ = images_u8.shape
    if B < 1 or H0 < 1 or W0 < 1 or oh < 1 or ow < 1:
        raise ValueError("image_load: empty source %s or destination %s" % (tuple(images_u8.shape), (oh, ow)))
    dev = images_u8.device
    src = images_u8.permute(0, 3, 1, 2)
    if reverse_channels:
        src = src.flip(1)
    src = src.to(dtype)
    q, v = resize_to_grey(src, source_coords(oh, H0, dtype, dev), source_coords(ow, W0, dtype, dev))
    lut = normalisation_table(mean, std).to(dev)
    norm = torch.stack([lut[c][q[:, c].long()] for c in range(3)], 1).to(out_dtype)
    return norm, q, v


def plan_groups(shapes, patch_image_size, max_batch=8):
    """The launches of Segmenter.segment_raw for images of the given (H, W) shapes at one view per image (`plan_views` with its
    default arguments gives the same plan), as a pure function:
    -> (loads, forwards).  loads: [((H, W), (oh, ow), [indices])], one `image_load` launch per distinct source shape, in order
    of first appearance; forwards: [((oh, ow), [indices])], one model forward per entry: images of equal network size in
    input order, at most `max_batch` of them."""
    if max_batch < 1:
        raise ValueError("segment_raw: max_batch must be >= 1, got %r" % (max_batch,))
    loads, by_size = {}, {}
    for i, (h, w) in enumerate(shapes):
        h, w = int(h), int(w)
        size = eval_size(h, w, patch_image_size)
        loads.setdefault((h, w), (size, []))[1].append(i)
        by_size.setdefault(size, []).append(i)
    forwards = [(size, idx[k:k + max_batch]) for size, idx in by_size.items() for k in range(0, len(idx), max_batch)]
    return [(hw, size, idx) for hw, (size, idx) in loads.items()], forwards


MAX_VIEWS = 16


def view_list(scales=(1.0,), flip=False):
    """-> [(ratio, flipped)]: the views of one image in mmseg's MultiScaleFlipAug order -- per ratio, in the order given, the
    unflipped view and then, with `flip`, the mirrored one"""
    scales = [float(r) for r in scales]
    if not scales or any(not r > 0 for r in scales):
        raise ValueError("segment_raw: scales must be a non-empty sequence of ratios > 0, got %r" % (scales,))
    views = [(r, f) for r in scales for f in ((False, True) if flip else (False,))]
    if len(views) > MAX_VIEWS:
        raise ValueError("segment_raw: %d views (%d scales%s), hip.seg_predict_views takes at most %d"
                         % (len(views), len(scales), " x 2 flips" if flip else "", MAX_VIEWS))
    return views


def plan_views(shapes, patch_image_size, scales=(1.0,), flip=False, max_batch=8):
    """`plan_groups` for multi-scale + flip inference, as a pure function: -> (views, loads, forwards).
    views: `view_list(scales, flip)`; view v of image i is the pair (i, v).
    loads: [((H, W), (oh, ow), [image indices])], one `image_load` launch per distinct (source shape, network size), in order
    of first appearance -- a mirrored view is the loaded tensor flipped, and ratios that give one size share the load.
    forwards: [((oh, ow), [(i, v)])], one model forward per entry: the views of equal network size, mirrored or not, in
    (image, view) order, at most `max_batch` of them; the entries of one size follow each other, so the engine meets every
    size once."""
    if max_batch < 1:
        raise ValueError("segment_raw: max_batch must be >= 1, got %r" % (max_batch,))
    views = view_list(scales, flip)
    loads, by_size = {}, {}
    for i, (h, w) in enumerate(shapes):
        h, w = int(h), int(w)
        for v, (ratio, _) in enumerate(views):
            size = eval_size(h, w, patch_image_size, ratio)
            idx = loads.setdefault(((h, w), size), [])
            if i not in idx:
                idx.append(i)
            by_size.setdefault(size, []).append((i, v))
    forwards = [(size, iv[k:k + max_batch]) for size, iv in by_size.items() for k in range(0, len(iv), max_batch)]
    return views, [(hw, size, idx) for (hw, size), idx in loads.items()], forwards


# ---- sliding-window inference (mmseg's test_cfg mode='slide'; Segmenter.segment_raw(slide=...)) ----
MAX_WINDOWS = 64         # == IFSEG_SLIDE_MAX_WINDOWS of include/ifseg_hip.h


def _pair(v, what):
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError("slide_windows: %s must be an int or an (h, w) pair, got %r" % (what, v))
        return int(v[0]), int(v[1])
    return int(v), int(v)


def slide_windows(oh, ow, crop, stride):
    """The windows of an [oh, ow] image by mmseg's `slide_inference` rule -> (ys, xs, ch, cw).  `crop` and `stride` are each
    an int or an (h, w) pair.  Per axis of length o with crop c and stride s there are g = max(o - c + s - 1, 0) // s + 1
    windows, window i starting at max(min(i s + c, o) - c, 0), every one of extent min(c, o): the last window is pulled back
    inside the image, and an axis shorter than the crop has one shorter window.  The windows of the image are the cross
    product of the starts `ys` and `xs`, ys outer (window k = iy len(xs) + ix), each of size (ch, cw).
    ValueError: a crop or stride < 1, a stride above its crop (gaps), more than MAX_WINDOWS windows."""
    (c_h, c_w), (s_h, s_w) = _pair(crop, "crop"), _pair(stride, "stride")
    oh, ow = int(oh), int(ow)
    if oh < 1 or ow < 1:
        raise ValueError("slide_windows: the image must be at least 1 x 1, got %d x %d" % (oh, ow))
    if min(c_h, c_w) < 1 or min(s_h, s_w) < 1:
        raise ValueError("slide_windows: crop and stride must be >= 1, got crop %r, stride %r" % (crop, stride))
    if s_h > c_h or s_w > c_w:
        raise ValueError("slide_windows: a stride above the crop leaves pixels uncovered, got crop %r, stride %r" % (crop, stride))

    def axis(o, c, s):
        g = max(o - c + s - 1, 0) // s + 1
        return [max(min(i * s + c, o) - c, 0) for i in range(g)], min(c, o)

    (ys, ch), (xs, cw) = axis(oh, c_h, s_h), axis(ow, c_w, s_w)
    if len(ys) * len(xs) > MAX_WINDOWS:
        raise ValueError("slide_windows: %d x %d windows of an image of %d x %d (crop %r, stride %r), at most %d"
                         % (len(ys), len(xs), oh, ow, crop, stride, MAX_WINDOWS))
    return ys, xs, ch, cw


def plan_slide(shapes, patch_image_size, crop, stride, ratio=1.0, max_batch=8):
    """`plan_views` for sliding-window inference, as a pure function: `plan_slide_views`' plan for the one unflipped view at
    `ratio`, without the view index -> (per_image, loads, forwards).
    per_image: [((oh, ow), ys, xs, (ch, cw))], image i at `eval_size(H, W, P, ratio)` and its `slide_windows`; window k of
    image i is the pair (i, k).
    loads: [((H, W), (oh, ow), [image indices])], one `image_load_windows` launch per distinct (source shape, (oh, ow)), in
    order of first appearance.
    forwards: [((ch, cw), [(i, k)])], one model forward per entry: the windows of one size, of whatever image, in
    (image, window) order, at most `max_batch` of them; the entries of one size follow each other."""
    per_image, loads, forwards = _plan_windows(shapes, patch_image_size, crop, stride, [(ratio, False)], max_batch)
    return ([mine[0] for mine in per_image], [(hw, size, idx) for hw, size, _, idx in loads],
            [(size, [(i, k) for i, _, k in ivk]) for size, ivk in forwards])


def plan_slide_views(shapes, patch_image_size, crop, stride, scales=(1.0,), flip=False, max_batch=8):
    """`plan_slide` for multi-scale + flip over sliding windows, as a pure function: -> (views, per_image, loads, forwards).
    views: `view_list(scales, flip)`; view v of image i is the pair (i, v), window k of it the triple (i, v, k).
    per_image: [[((oh, ow), ys, xs, (ch, cw))] per view], image i at `eval_size(H, W, P, ratio_v)` and its `slide_windows`
    (a mirrored view has its unmirrored twin's geometry; its windows are cut from the mirrored image).
    loads: [((H, W), (oh, ow), flipped, [image indices])], one `image_load_windows` launch per distinct (source shape, size,
    flip), in order of first appearance; ratios that give one size share the load.
    forwards: [((ch, cw), [(i, v, k)])], one model forward per entry: the windows of one size, of whatever view and image, in
    (image, view, window) order, at most `max_batch` of them; the entries of one size follow each other.
    ValueError: more than MAX_VIEWS views, more than MAX_WINDOWS windows in any view, a crop or stride outside the rule."""
    if max_batch < 1:                                         # here as well: this refusal comes before view_list's
        raise ValueError("segment_raw: max_batch must be >= 1, got %r" % (max_batch,))
    views = view_list(scales, flip)
    return (views,) + _plan_windows(shapes, patch_image_size, crop, stride, views, max_batch)


def _plan_windows(shapes, patch_image_size, crop, stride, views, max_batch):
    """the plan of `plan_slide_views` for the given (ratio, flipped) views -> (per_image, loads, forwards)"""
    if max_batch < 1:
        raise ValueError("segment_raw: max_batch must be >= 1, got %r" % (max_batch,))
    per_image, loads, by_size = [], {}, {}
    for i, (h, w) in enumerate(shapes):
        h, w = int(h), int(w)
        mine = []
        for v, (ratio, flipped) in enumerate(views):
            size = eval_size(h, w, patch_image_size, ratio)
            ys, xs, ch, cw = slide_windows(size[0], size[1], crop, stride)
            mine.append((size, ys, xs, (ch, cw)))
            idx = loads.setdefault(((h, w), size, flipped), [])
            if i not in idx:
                idx.append(i)
            by_size.setdefault((ch, cw), []).extend((i, v, k) for k in range(len(ys) * len(xs)))
        per_image.append(mine)
    forwards = [(size, ivk[k:k + max_batch]) for size, ivk in by_size.items() for k in range(0, len(ivk), max_batch)]
    return per_image, [(hw, size, f, idx) for (hw, size, f), idx in loads.items()], forwards


def image_load_windows_reference(images_u8, oh, ow, crop, stride, mean=HALF, std=HALF, reverse_channels=False,
                                 dtype=torch.float64, out_dtype=torch.float32, flip=False):
    """CPU specification of hip.image_load_windows: uint8 [B, H0, W0, 3] -> normalised `out_dtype` [B Nw, 3, ch, cw]: element
    (b Nw + k, c, y, x) is `image_load_reference`'s element (b, c, ys[k] + y, xs[k] + x) at (oh, ow), the windows being
    `slide_windows(oh, ow, crop, stride)`.  A window is a slice of the loaded image, never a resize of its own.
    flip: the windows are slices of the loaded image mirrored along its width (after the resize, as mmseg mirrors)."""
    ys, xs, ch, cw = slide_windows(oh, ow, crop, stride)
    full = image_load_reference(images_u8, oh, ow, mean, std, reverse_channels, dtype, out_dtype)[0]
    if flip:
        full = full.flip(-1)
    wins = torch.stack([full[:, :, y:y + ch, x:x + cw] for y in ys for x in xs], 1)
    return wins.reshape(full.shape[0] * len(ys) * len(xs), 3, ch, cw)
