"""The reference's TRAINING transform for raw images and raw label maps: the CPU specification of `hip.train_draw` /
`hip.train_load` (csrc/trainload.hip) and `TrainTransform`, the caller of both.  Needs no GPU to import.

The reference trains on (data/mm_data/segmentation_dataset.py:157-163, 239-251, 268-269)

    Resize(img_scale=(4 P, P), ratio_range=(0.5, 2.0), min_size=P) -> RandomCrop((P, P), cat_max_ratio=0.75)
    -> RandomFlip(0.5) -> PhotoMetricDistortion() -> Normalize

on `cv2`.  Here the four stages are one pure function of (seed, sample ordinal): uint8 images [H0, W0, 3] (RGB) and uint8
label maps [H0, W0] of any size in, `patch_images` [B, 3, P, P] and `target` int64 [B, P*P + 1] (seg_id_offset + class,
EOS last: what `SegCriterion.compute_loss` takes) out.  With `raw_labels` the label is remapped as the dataset does at
:231-233 -- raw 0 and raw 255 become `nseg` ('unknown'), any other x becomes x - 1 -- else it is taken as class ids;
either way a class above `nseg` is clamped to `nseg`.

RANDOM STREAM.  The project's counter generator (`artificial.splitmix64`, csrc/common.h), for sample ordinal n:

    u(n, i) = splitmix64(seed + (n << 32) + i)  mod 2^64,     t(n, i) = u(n, i) >> 32

    slot i     parameter
    0          scale       new_short = max(P, (P (lo2 2^32 + span2 t)) >> 33),  lo2 = 2 lo, span2 = 2 (hi - lo) of
                           `ratio_range` (integers; (0.5, 2.0): (P (2^32 + 3 t)) >> 33 = int(P r), r = 0.5 + 1.5 t / 2^32)
    1 + 2k     off_h of crop candidate k = 0..10:  (t (new_h - P + 1)) >> 32
    2 + 2k     off_w of crop candidate k:          (t (new_w - P + 1)) >> 32
    23         bits of t: 0 flip, 1 brightness on, 2 mode, 3 contrast on, 4 saturation on, 5 hue on
    24         beta    = ((t >> 9) - 2^22) / 2^17          in [-32, 32) on a 2^-17 grid
    25         alpha_c = (2^22 + (t >> 9)) / 2^23          in [0.5, 1.5) on a 2^-23 grid
    26         alpha_s = (2^22 + (t >> 9)) / 2^23
    27         delta   = ((t 36) >> 32) - 18               in [-18, 17]   (numpy's randint(-18, 18))

Every parameter is an integer or a dyadic fraction with at most 24 significant bits: exact in fp32, so the host and the
device agree bit for bit.

GEOMETRY, in integers.  With s = min(H0, W0) the short side becomes new_short and the long side
(2 new_short long + s) // (2 s).  The image is resized from (H0, W0) to (new_h, new_w) by `imageio.image_load_reference`'s
rule (`source_coords`, the four-weight sum, q = clamp(floor(v + 0.5), 0, 255)), the label by nearest
src = min(dst in // out, in - 1); then the P x P window at (off_h, off_w) is cut and flipped horizontally.  Only the window
is ever evaluated.  2 in out >= 2^31 on an axis is refused, as by `ifseg_image_load`.

CROP CHOICE (mmseg RandomCrop.__call__).  On the remapped, resized label map: the first candidate k in 0..9 whose window
holds more than one class and 4 max(count) < 3 sum(count); else candidate 10, unchecked.  'unknown' counts as a class.

PHOTOMETRIC STAGE (mmseg PhotoMetricDistortion), per pixel on the grey levels q: brightness; contrast if mode = 1;
saturation; hue; contrast if mode = 0.  convert(x, alpha, beta) = uint8(trunc(clip(fp32(x) alpha + beta, 0, 255))) with
alpha = 1 or beta = 0: one IEEE fp32 operation.  Saturation and hue each make an 8-bit HSV round trip, in exact integers
(`rgb_to_hsv8`, `hsv8_to_rgb`): H in [0, 180), S and V in [0, 255], every quotient rounded half up.

The record of a sample, int32 [16] (`draw_params`):

    0 new_h  1 new_w  2 off_h  3 off_w  4 k  5 flip  6 brightness on  7 contrast on  8 saturation on  9 hue on  10 mode
    11 beta  12 alpha_c  13 alpha_s (fp32 bit patterns)  14 delta  15 zero (reserved)

NOT pinned against the reference: `cv2`'s resize evaluates the bilinear filter with 11-bit fixed-point weights; its 8-bit
HSV conversions are table-driven (fixed-point reciprocals), here they are the exactly rounded quotients; mmcv evaluates
the long side as int(long * float(scale) + 0.5) in Python floats, here it is the integer rule above.  `cv2` and `mmcv` are
not available where this project is tested.  The reference reverses the channels in front of mmseg and back behind it
(:218, :243), so its HSV reads true colours; here the input is RGB and stays RGB, and `reverse_channels` applies to the
order of the output planes only, as in `image_load`.  The reference's `downsampled_target` is not produced.
"""
import numpy as np
import torch

from .artificial import _M64, splitmix64
from .imageio import HALF, normalisation_table, resize_to_grey, source_coords

RECORD = 16
(R_NEW_H, R_NEW_W, R_OFF_H, R_OFF_W, R_K, R_FLIP, R_BRIGHT, R_CONTRAST, R_SAT, R_HUE, R_MODE, R_BETA, R_ALPHA_C, R_ALPHA_S,
 R_DELTA, R_ZERO) = range(RECORD)
CANDIDATES = 11
HSV_D = 7650
EOS = 2


# ------------------------------------------------------------------------------------------------- parameters
def ratio_halves(ratio_range):
    """(lo, hi) -> (lo2, span2) = (2 lo, 2 (hi - lo)), which must be integers"""
    lo, hi = (float(x) for x in ratio_range)
    lo2, span2 = 2 * lo, 2 * (hi - lo)
    if lo2 != int(lo2) or span2 != int(span2) or lo2 < 0 or span2 < 0 or lo2 + span2 > 64:
        raise ValueError("train transform: ratio_range %r must hold multiples of 0.5 with 0 <= lo <= hi <= 32" % (ratio_range,))
    return int(lo2), int(span2)


def new_short_of(t, P, lo2=1, span2=3):
    """the drawn short side, from the 32-bit draw t"""
    return max(int(P), (int(P) * ((lo2 << 32) + span2 * int(t))) >> 33)


def resized_size(H0, W0, new_short):
    """-> (new_h, new_w): the short side becomes new_short, the long one (2 new_short long + s) // (2 s)"""
    s = min(H0, W0)
    long_side = lambda n: (2 * new_short * n + s) // (2 * s)
    return (new_short, long_side(W0)) if H0 <= W0 else (long_side(H0), new_short)


def check_axis(inn, out, what="train transform"):
    if inn < 1 or out < 1 or 2 * inn * out >= 2 ** 31:
        raise ValueError("%s: 2 * in * out must stay below 2**31 per axis, got %d -> %d" % (what, inn, out))


def f32_bits(x):
    return int(np.float32(x).view(np.int32))


def bits_f32(i):
    return np.int32(i).view(np.float32)


def draws(seed, ordinal, n=28):
    """t(n, 0 .. n-1) as python ints"""
    base = ((int(seed) & _M64) + (int(ordinal) << 32)) & _M64
    with np.errstate(over="ignore"):
        u = splitmix64(np.uint64(base) + np.arange(n, dtype=np.uint64))
    return [int(v) for v in (u >> np.uint64(32))]


def remap_label(label_u8, nseg, raw_labels=True):
    """uint8 [...] -> int64 class ids in [0, nseg]"""
    x = torch.as_tensor(label_u8)
    if x.dtype != torch.uint8:
        raise ValueError("train transform: label maps must be uint8, got %s" % x.dtype)
    x = x.long()
    if raw_labels:
        x = torch.where((x == 0) | (x == 255), torch.full_like(x, nseg), x - 1)
    return x.clamp_max(nseg)


def nearest_axis(out, inn):
    """int64 [out]: src = min(dst in // out, in - 1)"""
    return ((torch.arange(out, dtype=torch.int64) * inn) // out).clamp_max(inn - 1)


def crop_ok(window, P):
    """mmseg's test on a cropped class map: more than one class and max(count) / sum(count) < 0.75, in integers"""
    cnt = torch.bincount(window.reshape(-1))
    return int((cnt > 0).sum()) > 1 and 4 * int(cnt.max()) < 3 * P * P


def draw_params(shapes, labels, P, nseg, seed, first_ordinal, ratio_range=(0.5, 2.0), photometric=True, flip=True,
                raw_labels=True):
    """int32 [B, 16]: the records of the samples at ordinals first_ordinal + b.  shapes: [(H0, W0)], labels: uint8 [H0, W0]
    label maps (the crop choice reads them)."""
    P, nseg, first = int(P), int(nseg), int(first_ordinal)
    B = len(shapes)
    if P < 16 or P % 16 or not 1 <= nseg <= 255:
        raise ValueError("train transform: P must be a multiple of 16 and 1 <= nseg <= 255, got P = %d, nseg = %d" % (P, nseg))
    if first < 0 or first + B > 1 << 32:
        raise ValueError("train transform: ordinals must lie in [0, 2^32)")
    if len(labels) != B:
        raise ValueError("train transform: %d shapes for %d label maps" % (B, len(labels)))
    lo2, span2 = ratio_halves(ratio_range)
    out = np.zeros((B, RECORD), dtype=np.int32)
    for b, ((H0, W0), lab) in enumerate(zip(shapes, labels)):
        H0, W0 = int(H0), int(W0)
        if tuple(lab.shape) != (H0, W0):
            raise ValueError("train transform: label map %s for an image of %d x %d" % (tuple(lab.shape), H0, W0))
        t = draws(seed, first + b)
        new_h, new_w = resized_size(H0, W0, new_short_of(t[0], P, lo2, span2))
        check_axis(H0, new_h)
        check_axis(W0, new_w)
        cls = remap_label(torch.as_tensor(lab).cpu(), nseg, raw_labels)
        iy, ix = nearest_axis(new_h, H0), nearest_axis(new_w, W0)
        for k in range(CANDIDATES):
            off_h, off_w = (t[1 + 2 * k] * (new_h - P + 1)) >> 32, (t[2 + 2 * k] * (new_w - P + 1)) >> 32
            if k == CANDIDATES - 1 or crop_ok(cls[iy[off_h:off_h + P]][:, ix[off_w:off_w + P]], P):
                break
        bits = t[23]
        m = t[24] >> 9
        ph = 1 if photometric else 0
        out[b] = (new_h, new_w, off_h, off_w, k, (bits & 1) if flip else 0, ph & (bits >> 1), ph & (bits >> 3), ph & (bits >> 4),
                  ph & (bits >> 5), (bits >> 2) & 1, f32_bits((m - 2 ** 22) / 2.0 ** 17), f32_bits((2 ** 22 + (t[25] >> 9)) / 2.0 ** 23),
                  f32_bits((2 ** 22 + (t[26] >> 9)) / 2.0 ** 23), ((t[27] * 36) >> 32) - 18, 0)
    return torch.from_numpy(out)


# ------------------------------------------------------------------------------------------------- photometric stage
def convert(x, alpha=1.0, beta=0.0):
    """mmseg's convert on integer grey levels: uint8(trunc(clip(fp32(x) alpha + beta, 0, 255))); one of alpha = 1,
    beta = 0 must hold (a single fp32 operation)"""
    alpha, beta = np.float32(alpha), np.float32(beta)
    assert alpha == 1 or beta == 0
    v = np.asarray(x).astype(np.float32)
    v = v * alpha if beta == 0 else v + beta
    return np.trunc(np.clip(v, np.float32(0), np.float32(255))).astype(np.int64)


def rgb_to_hsv8(rgb):
    """integer [..., 3] grey levels -> int64 [..., 3] (H in [0, 180), S, V in [0, 255]):
    V = max, d = max - min, S = (510 d + V) // (2 V) (0 when V = 0), H = round_half_up((30 x + off d) / d) mod 180 with
    (x, off) = (g - b, 0), (b - r, 60), (r - g, 120) for the maximum at r, g, b (ties in that order), 0 when d = 0"""
    a = np.asarray(rgb).astype(np.int64)
    r, g, b = a[..., 0], a[..., 1], a[..., 2]
    V = np.maximum(np.maximum(r, g), b)
    d = V - np.minimum(np.minimum(r, g), b)
    S = np.where(V > 0, (510 * d + V) // np.maximum(2 * V, 1), 0)
    x = np.where(V == r, g - b, np.where(V == g, b - r, r - g))
    off = np.where(V == r, 0, np.where(V == g, 60, 120))
    dd = np.maximum(d, 1)
    H = np.where(d > 0, ((2 * (30 * x + off * d) + d) // (2 * dd)) % 180, 0)
    return np.stack([H, S, V], -1)


def hsv8_to_rgb(hsv):
    """int64 [..., 3] (H, S, V) -> int64 [..., 3] grey levels: sec = H // 30, f = H mod 30, D = 7650,
    p = rd(30 V (255 - S)), q = rd(V (D - S f)), t = rd(V (D - S (30 - f))), rd(n) = (2 n + D) // (2 D);
    (r, g, b) = (V,t,p), (q,V,p), (p,V,t), (p,q,V), (t,p,V), (V,p,q) for sec = 0..5"""
    a = np.asarray(hsv).astype(np.int64)
    H, S, V = a[..., 0], a[..., 1], a[..., 2]
    sec, f, D = H // 30, H % 30, HSV_D
    rd = lambda n: (2 * n + D) // (2 * D)
    p, q, t = rd(30 * V * (255 - S)), rd(V * (D - S * f)), rd(V * (D - S * (30 - f)))
    pick = lambda c: np.choose(sec, c)
    return np.stack([pick([V, q, p, p, t, V]), pick([t, V, V, q, p, p]), pick([p, p, t, V, V, q])], -1)


def photometric(q_rgb, record):
    """the photometric stage on grey levels [..., 3] (RGB) under one record -> uint8 [..., 3]"""
    rec = [int(v) for v in record]
    img = np.asarray(q_rgb).astype(np.int64)
    contrast = lambda x: convert(x, alpha=bits_f32(rec[R_ALPHA_C])) if rec[R_CONTRAST] else x
    if rec[R_BRIGHT]:
        img = convert(img, beta=bits_f32(rec[R_BETA]))
    if rec[R_MODE] == 1:
        img = contrast(img)
    if rec[R_SAT]:
        hsv = rgb_to_hsv8(img)
        hsv[..., 1] = convert(hsv[..., 1], alpha=bits_f32(rec[R_ALPHA_S]))
        img = hsv8_to_rgb(hsv)
    if rec[R_HUE]:
        hsv = rgb_to_hsv8(img)
        hsv[..., 0] = (hsv[..., 0] + rec[R_DELTA]) % 180
        img = hsv8_to_rgb(hsv)
    if rec[R_MODE] == 0:
        img = contrast(img)
    return img.astype(np.uint8)


# ------------------------------------------------------------------------------------------------- the transform
def check_record(rec, H0, W0, P):
    new_h, new_w, off_h, off_w = (int(v) for v in rec[:4])
    if new_h < P or new_w < P or not 0 <= off_h <= new_h - P or not 0 <= off_w <= new_w - P:
        raise ValueError("train transform: record (new %d x %d, offset %d, %d) does not hold a %d x %d window"
                         % (new_h, new_w, off_h, off_w, P, P))
    check_axis(H0, new_h)
    check_axis(W0, new_w)
    return new_h, new_w, off_h, off_w


def train_load_reference(images, labels, params, P, nseg, seg_id_offset, mean=HALF, std=HALF, reverse_channels=False,
                         raw_labels=True, eos=EOS, dtype=torch.float64, out_dtype=torch.float32):
    """CPU specification of hip.train_load.  images: uint8 [H0, W0, 3] each, labels: uint8 [H0, W0] each, params int32
    [B, 16] -> (patch_images `out_dtype` [B, 3, P, P], target int64 [B, P*P + 1], q uint8 [B, P, P, 3]: the grey levels
    behind the photometric stage (RGB), q0 uint8 [B, P, P, 3]: those in front of it).  Weights and the four-term sum of
    the resize are evaluated in `dtype`, on the window only."""
    P = int(P)
    B = len(images)
    params = torch.as_tensor(params).cpu()
    if tuple(params.shape) != (B, RECORD) or len(labels) != B:
        raise ValueError("train transform: %d images, %d label maps, records %s" % (B, len(labels), tuple(params.shape)))
    lut = normalisation_table(mean, std)
    norm = torch.empty(B, 3, P, P, dtype=out_dtype)
    target = torch.empty(B, P * P + 1, dtype=torch.int64)
    qs, q0s = [], []
    for b in range(B):
        img, lab, rec = torch.as_tensor(images[b]).cpu(), torch.as_tensor(labels[b]).cpu(), params[b].tolist()
        if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[-1] != 3 or tuple(lab.shape) != tuple(img.shape[:2]):
            raise ValueError("train transform: image %s %s with label map %s" % (img.dtype, tuple(img.shape), tuple(lab.shape)))
        H0, W0 = img.shape[:2]
        new_h, new_w, off_h, off_w = check_record(rec, H0, W0, P)
        ys = off_h + torch.arange(P)
        xs = off_w + (torch.arange(P - 1, -1, -1) if rec[R_FLIP] else torch.arange(P))
        q0 = resize_to_grey(img.permute(2, 0, 1).to(dtype), [v[ys] for v in source_coords(new_h, H0, dtype)],
                            [v[xs] for v in source_coords(new_w, W0, dtype)])[0].permute(1, 2, 0).contiguous()
        q = torch.from_numpy(photometric(q0.numpy(), rec))
        q0s.append(q0)
        qs.append(q)
        planes = q.permute(2, 0, 1).long()
        if reverse_channels:
            planes = planes.flip(0)
        norm[b] = torch.stack([lut[c][planes[c]] for c in range(3)]).to(out_dtype)
        cls = remap_label(lab, nseg, raw_labels)[nearest_axis(new_h, H0)[ys]][:, nearest_axis(new_w, W0)[xs]]
        target[b, :-1] = seg_id_offset + cls.reshape(-1)
        target[b, -1] = eos
    return norm, target, torch.stack(qs), torch.stack(q0s)


def train_plane_reference(planes, params, P):
    """CPU specification of hip.train_load_plane.  planes: uint8 [H0, W0] each (per-pixel loss weights, or anything else that
    must follow the label map), params int32 [B, 16] -> uint8 [B, P*P]: the label tap of `train_load_reference`
    (src = min(dst in // out, in - 1) on the resized grid, the window at the record's offset, mirrored under flip) on the
    plane's own bytes, nothing remapped."""
    P = int(P)
    B = len(planes)
    params = torch.as_tensor(params).cpu()
    if tuple(params.shape) != (B, RECORD):
        raise ValueError("train transform: %d planes, records %s" % (B, tuple(params.shape)))
    out = torch.empty(B, P * P, dtype=torch.uint8)
    for b in range(B):
        pl, rec = torch.as_tensor(planes[b]).cpu(), params[b].tolist()
        if pl.dtype != torch.uint8 or pl.dim() != 2:
            raise ValueError("train transform: planes must be uint8 [H0, W0], got %s %s" % (pl.dtype, tuple(pl.shape)))
        H0, W0 = pl.shape
        new_h, new_w, off_h, off_w = check_record(rec, H0, W0, P)
        ys = off_h + torch.arange(P)
        xs = off_w + (torch.arange(P - 1, -1, -1) if rec[R_FLIP] else torch.arange(P))
        out[b] = pl[nearest_axis(new_h, H0)[ys]][:, nearest_axis(new_w, W0)[xs]].reshape(-1)
    return out


class TrainTransform:
    def __init__(self, P, nseg, seg_id_offset, mean=HALF, std=HALF, seed=1, device="cpu", photometric=True, flip=True,
                 ratio_range=(0.5, 2.0), raw_labels=True, dtype=torch.float32, reverse_channels=False, eos=EOS):
        """device "cpu" runs the specification of this module, any other device the kernels of csrc/trainload.hip"""
        self.P, self.nseg, self.seg_id_offset = int(P), int(nseg), int(seg_id_offset)
        if self.P < 16 or self.P % 16 or not 1 <= self.nseg <= 255:
            raise ValueError("TrainTransform: P must be a multiple of 16 and 1 <= nseg <= 255, got P = %d, nseg = %d"
                             % (self.P, self.nseg))
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError("TrainTransform: dtype must be torch.float32 or torch.bfloat16, got %s" % dtype)
        self.mean, self.std = tuple(float(x) for x in mean), tuple(float(x) for x in std)
        self.seed, self.device = int(seed) & _M64, torch.device(device)
        self.photometric, self.flip, self.raw_labels = bool(photometric), bool(flip), bool(raw_labels)
        self.ratio_range, self.dtype, self.reverse_channels, self.eos = tuple(ratio_range), dtype, bool(reverse_channels), int(eos)
        ratio_halves(self.ratio_range)

    def _sources(self, images, labels):
        if len(images) != len(labels) or not len(images):
            raise ValueError("TrainTransform: %d images and %d label maps" % (len(images), len(labels)))
        for img, lab in zip(images, labels):
            if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[-1] != 3:
                raise ValueError("TrainTransform: images must be uint8 [H0, W0, 3], got %s %s" % (img.dtype, tuple(img.shape)))
            if lab.dtype != torch.uint8 or tuple(lab.shape) != tuple(img.shape[:2]):
                raise ValueError("TrainTransform: label maps must be uint8 [H0, W0] of the image's size, got %s %s for %s"
                                 % (lab.dtype, tuple(lab.shape), tuple(img.shape)))
        if self.device.type == "cpu":
            return list(images), list(labels)
        put = lambda t: t.to(self.device, non_blocking=True).contiguous()
        return [put(t) for t in images], [put(t) for t in labels]

    def draw(self, images, labels, first_ordinal):
        """-> int32 [B, 16] on the transform's device"""
        images, labels = self._sources(images, labels)
        return self._draw(labels, first_ordinal)

    def _draw(self, labels, first_ordinal, table=None):
        if self.device.type == "cpu":
            return draw_params([tuple(l.shape) for l in labels], labels, self.P, self.nseg, self.seed, first_ordinal,
                               self.ratio_range, self.photometric, self.flip, self.raw_labels)
        from . import hip
        return hip.train_draw(labels, self.P, self.nseg, self.seed, first_ordinal, self.ratio_range, self.photometric, self.flip,
                              self.raw_labels, table=table)

    def _planes(self, weights, labels):
        """per-pixel weight planes: uint8 [H0, W0] of their label map's size, moved to the transform's device"""
        if len(weights) != len(labels):
            raise ValueError("TrainTransform: %d weight planes for %d label maps" % (len(weights), len(labels)))
        for w, lab in zip(weights, labels):
            if not torch.is_tensor(w) or w.dtype != torch.uint8 or tuple(w.shape) != tuple(lab.shape):
                raise ValueError("TrainTransform: weight planes must be uint8 [H0, W0] of the label map's size, got %s for %s"
                                 % ((w.dtype, tuple(w.shape)) if torch.is_tensor(w) else type(w), tuple(lab.shape)))
        if self.device.type == "cpu":
            return list(weights)
        return [w.to(self.device, non_blocking=True).contiguous() for w in weights]

    def _apply_planes(self, planes, params):
        if self.device.type == "cpu":
            return train_plane_reference(planes, params, self.P)
        from . import hip
        return hip.train_load_plane(planes, params, self.P)

    def apply(self, images, labels, params, weights=None):
        """the caller's records -> (patch_images [B, 3, P, P], target int64 [B, P*P + 1]); with `weights` (uint8 [H0, W0]
        per sample) a third tensor, uint8 [B, P*P]: the planes sampled where the labels were (`train_plane_reference`)"""
        images, labels = self._sources(images, labels)
        if weights is None:
            return self._apply(images, labels, params)
        planes = self._planes(weights, labels)
        return tuple(self._apply(images, labels, params)) + (self._apply_planes(planes, params),)

    def _apply(self, images, labels, params, table=None):
        if self.device.type == "cpu":
            return train_load_reference(images, labels, params, self.P, self.nseg, self.seg_id_offset, self.mean, self.std,
                                        self.reverse_channels, self.raw_labels, self.eos, out_dtype=self.dtype)[:2]
        from . import hip
        return hip.train_load(images, labels, params, self.P, self.nseg, self.seg_id_offset, self.mean, self.std,
                              self.reverse_channels, self.raw_labels, self.dtype, self.eos, table=table)

    def __call__(self, images, labels, first_ordinal, weights=None):
        images, labels = self._sources(images, labels)
        if weights is None:
            return self._apply(images, labels, self._draw(labels, first_ordinal))
        planes = self._planes(weights, labels)
        params = self._draw(labels, first_ordinal)
        return tuple(self._apply(images, labels, params)) + (self._apply_planes(planes, params),)
