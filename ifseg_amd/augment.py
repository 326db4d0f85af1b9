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

The second half of the module mixes two such batches (ClassMix / CutMix: `mix_draw_reference`, `mix_apply_reference`,
`BatchMix`; csrc/mix.hip) on the slots of the same stream behind the transform's 28; its rule stands above `check_mix`.
The third section is the strong augmentation of a mixed batch (colour jitter, then Gaussian blur: `strong_draw_reference`,
`strong_apply_reference`, `StrongAugment`; csrc/strong.hip) on slots 192..199; its rule stands above `BLUR_WEIGHTS`.
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


def check_patch(P, what, max_p=None):
    if P < 16 or P % 16 or (max_p is not None and P > max_p):
        raise ValueError("%s: P must be a multiple of 16%s, got %d" % (what, "" if max_p is None else " in 16 .. %d" % max_p, P))


def check_nseg(nseg, what):
    if not 1 <= nseg <= 255:
        raise ValueError("%s: 1 <= nseg <= 255 (uint8 label maps), got %d" % (what, nseg))


def check_ordinals(first, B, what):
    """the ordinals first .. first + B - 1 of a call: the stream's n has 32 bits"""
    if B < 1 or first < 0 or first + B > 1 << 32:
        raise ValueError("%s: B >= 1 and ordinals in [0, 2**32), got B = %d at %d" % (what, B, first))


def check_records(records, B, what, name="records"):
    if records.dtype != torch.int32 or tuple(records.shape) != (B, RECORD):
        raise ValueError("%s: %s must be int32 [%d, 16], got %s %s" % (what, name, B, records.dtype, tuple(records.shape)))


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


def photo_words(t, gate):
    """the nine photometric words of a record -- brightness on, contrast on, saturation on, hue on, mode, beta, alpha_c,
    alpha_s, delta -- from five consecutive draws t (slots 23..27 of the transform, 193..197 of the strong augmentation);
    the four "on" bits are ANDed with `gate`"""
    bits, g = t[0], 1 if gate else 0
    return (g & (bits >> 1), g & (bits >> 3), g & (bits >> 4), g & (bits >> 5), (bits >> 2) & 1,
            f32_bits(((t[1] >> 9) - 2 ** 22) / 2.0 ** 17), f32_bits((2 ** 22 + (t[2] >> 9)) / 2.0 ** 23),
            f32_bits((2 ** 22 + (t[3] >> 9)) / 2.0 ** 23), ((t[4] * 36) >> 32) - 18)


def draw_params(shapes, labels, P, nseg, seed, first_ordinal, ratio_range=(0.5, 2.0), photometric=True, flip=True,
                raw_labels=True):
    """int32 [B, 16]: the records of the samples at ordinals first_ordinal + b.  shapes: [(H0, W0)], labels: uint8 [H0, W0]
    label maps (the crop choice reads them)."""
    P, nseg, first = int(P), int(nseg), int(first_ordinal)
    B = len(shapes)
    check_patch(P, "train transform")
    check_nseg(nseg, "train transform")
    check_ordinals(first, B, "train transform")
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
        out[b] = (new_h, new_w, off_h, off_w, k, (t[23] & 1) if flip else 0) + photo_words(t[23:28], photometric) + (0,)
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


def photometric(q_rgb, record, base=R_BRIGHT):
    """the photometric stage on grey levels [..., 3] (RGB) under the nine words of one record that start at `base`
    (`photo_words`' order; R_BRIGHT in a transform's record, S_BRIGHT in a strong one) -> uint8 [..., 3]"""
    bright, contrast_on, sat, hue, mode, beta, alpha_c, alpha_s, delta = [int(v) for v in record][base:base + 9]
    img = np.asarray(q_rgb).astype(np.int64)
    contrast = lambda x: convert(x, alpha=bits_f32(alpha_c)) if contrast_on else x
    if bright:
        img = convert(img, beta=bits_f32(beta))
    if mode == 1:
        img = contrast(img)
    if sat:
        hsv = rgb_to_hsv8(img)
        hsv[..., 1] = convert(hsv[..., 1], alpha=bits_f32(alpha_s))
        img = hsv8_to_rgb(hsv)
    if hue:
        hsv = rgb_to_hsv8(img)
        hsv[..., 0] = (hsv[..., 0] + delta) % 180                                  # any delta: reduced mod 180 here
        img = hsv8_to_rgb(hsv)
    if mode == 0:
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
        check_patch(self.P, "TrainTransform")
        check_nseg(self.nseg, "TrainTransform")
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


# ------------------------------------------------------------------------------------------------- the batch mix
# ClassMix / CutMix of a labelled (source) batch into a pseudo-labelled (destination) batch: the CPU specification of
# `hip.mix_draw` / `hip.mix_apply` (csrc/mix.hip) and `BatchMix`, the caller of both.  Two batches in `train_sample`'s layout
# and of the same B and P: patch_images [B, 3, P, P] (fp32 or bf16, the same in both), target int64 [B, P*P + 1] and
# optionally target_weight uint8 [B, P*P].
#
# CLASS OF A SOURCE PIXEL.  c = target - seg_id_offset in 64 bits (wrapping); the pixel has a class only if 0 <= c < nseg.
# `nseg` ('unknown'), -1 (a poisoned sample of `train_load`) and any other value have none: never present, never pasted.
#
# RANDOM STREAM.  The transform's t(n, i) for the sample ordinal n = first_ordinal + b, on the slots behind the transform's
# 28: a mix with the transform's seed and ordinal is independent of the transform's draws.
#
#     slot i     parameter
#     28, 29     bh, bw = P // 4 + ((t (P // 2 + 1)) >> 32)                     mask "box" (CutMix)
#     30, 31     y0 = (t (P - bh + 1)) >> 32,  x0 = (t (P - bw + 1)) >> 32      the box is rows y0 .. y0 + bh, columns x0 .. x0 + bw
#     32 + i     j = i + ((t (n - i)) >> 32), swap c_i and c_j, i = 0 .. m - 1  mask "class" (ClassMix)
#
# "class": c_0 < ... < c_{n-1} the classes present in the source sample, m = (n + 1) // 2; after the partial Fisher-Yates
# above the chosen set is c_0 .. c_{m-1} (nothing when n = 0).  The box rule is this project's own: neither the reference nor
# mmseg has one to pin against.
#
# The record of a sample, int32 [16]:
#
#     0..7 chosen-class bits (class c is bit c & 31 of word c >> 5)   8 y0  9 x0  10 y1  11 x1 (exclusive ends)
#     12 n present   13 m chosen   14, 15 zero
#
# "class" leaves 8..11 zero, "box" leaves 0..7, 12 and 13 zero.
#
# APPLY.  Pixel (y, x) of sample b is selected if its source class's bit is set or y0 <= y < y1 and x0 <= x < x1 (the union:
# a caller's own record may carry both).  Selected pixels take the source's three image values, target value and weight,
# all others keep the destination's; a missing weight plane reads as 255, and no plane comes out if neither batch has one.
# out_target[b, P*P] (EOS) is the destination's.  Everything is a copy: parity is exact, NaN payloads included.  No address
# depends on a record: a box outside the image selects less, bits at or above nseg are never consulted.
MIX_SLOT_BOX, MIX_SLOT_CLASS = 28, 32
(M_BITS, M_Y0, M_X0, M_Y1, M_X1, M_PRESENT, M_CHOSEN) = (0, 8, 9, 10, 11, 12, 13)
MIX_MASKS = ("class", "box")
MIX_MAX_P = 4096


def check_mix(P, nseg, mask="class", what="batch mix"):
    check_patch(P, what, MIX_MAX_P)
    check_nseg(nseg, what)
    if mask not in MIX_MASKS:
        raise ValueError("%s: mask must be one of %r, got %r" % (what, MIX_MASKS, mask))


def mix_patch_size(target, what="batch mix"):
    """P of a target int64 [B, P*P + 1]"""
    if not torch.is_tensor(target) or target.dtype != torch.int64 or target.dim() != 2 or target.shape[0] < 1 or target.shape[1] < 2:
        raise ValueError("%s: a target must be int64 [B, P*P + 1] with B >= 1, got %s"
                         % (what, (target.dtype, tuple(target.shape)) if torch.is_tensor(target) else type(target)))
    P = int(round((target.shape[1] - 1) ** 0.5))
    if P * P + 1 != target.shape[1]:
        raise ValueError("%s: a target row holds P*P + 1 entries, got %d" % (what, target.shape[1]))
    return P


def check_mix_batches(src_images, src_target, src_weight, dst_images, dst_target, dst_weight, what="batch mix"):
    """the shapes and dtypes of two batches that can be mixed -> (B, P); reads no values"""
    P = mix_patch_size(src_target, what)
    B = src_target.shape[0]
    if tuple(dst_target.shape) != tuple(src_target.shape) or dst_target.dtype != torch.int64:
        raise ValueError("%s: the two targets must be int64 of one shape (equal B and P), got %s and %s %s"
                         % (what, tuple(src_target.shape), dst_target.dtype, tuple(dst_target.shape)))
    for name, img in (("source", src_images), ("destination", dst_images)):
        if img.dtype not in (torch.float32, torch.bfloat16) or tuple(img.shape) != (B, 3, P, P):
            raise ValueError("%s: the %s images must be fp32 or bf16 [%d, 3, %d, %d], got %s %s"
                             % (what, name, B, P, P, img.dtype, tuple(img.shape)))
    if src_images.dtype != dst_images.dtype:
        raise ValueError("%s: the two image batches must share a dtype, got %s and %s" % (what, src_images.dtype, dst_images.dtype))
    for name, w in (("source", src_weight), ("destination", dst_weight)):
        if w is not None and (w.dtype != torch.uint8 or tuple(w.shape) != (B, P * P)):
            raise ValueError("%s: the %s weight plane must be uint8 [%d, %d], got %s %s" % (what, name, B, P * P, w.dtype, tuple(w.shape)))
    return B, P


def mix_batch(x):
    """a sample in `train_sample`'s layout, or (images, target[, weight]) -> (images, target, weight | None)"""
    if isinstance(x, dict):
        return x["net_input"]["patch_images"], x["target"], x.get("target_weight")
    x = tuple(x)
    if len(x) not in (2, 3):
        raise ValueError("batch mix: a batch is a sample or (images, target[, weight]), got %d entries" % len(x))
    return x[0], x[1], (x[2] if len(x) == 3 else None)


def mix_classes(target_row, nseg, seg_id_offset):
    """the classes present in one source target row (int64 [P*P], EOS not included), ascending"""
    c = torch.as_tensor(target_row).reshape(-1) - int(seg_id_offset)               # wraps in 64 bits, as on the device
    return torch.unique(c[(c >= 0) & (c < nseg)]).tolist()


def mix_choice(present, seed, ordinal):
    """the chosen half of the ascending class list `present`: the partial Fisher-Yates on slots 32 .. 32 + m - 1"""
    c, n = list(present), len(present)
    m = (n + 1) // 2
    t = draws(seed, ordinal, MIX_SLOT_CLASS + m)
    for i in range(m):
        j = i + ((t[MIX_SLOT_CLASS + i] * (n - i)) >> 32)
        c[i], c[j] = c[j], c[i]
    return c[:m]


def mix_box(P, seed, ordinal):
    """-> (y0, x0, y1, x1) of the CutMix box, exclusive ends"""
    t = draws(seed, ordinal, MIX_SLOT_BOX + 4)[MIX_SLOT_BOX:]
    bh, bw = P // 4 + ((t[0] * (P // 2 + 1)) >> 32), P // 4 + ((t[1] * (P // 2 + 1)) >> 32)
    y0, x0 = (t[2] * (P - bh + 1)) >> 32, (t[3] * (P - bw + 1)) >> 32
    return y0, x0, y0 + bh, x0 + bw


def mix_draw_reference(src_target, nseg, seg_id_offset, seed, first_ordinal, mask="class"):
    """CPU specification of hip.mix_draw.  src_target int64 [B, P*P + 1] -> the records int32 [B, 16] of the samples at
    ordinals first_ordinal + b."""
    src_target = torch.as_tensor(src_target).cpu()
    P, nseg, first = mix_patch_size(src_target), int(nseg), int(first_ordinal)
    check_mix(P, nseg, mask)
    B = src_target.shape[0]
    check_ordinals(first, B, "batch mix")
    out = np.zeros((B, RECORD), dtype=np.uint32)
    for b in range(B):
        if mask == "box":
            out[b, M_Y0:M_X1 + 1] = mix_box(P, seed, first + b)
            continue
        present = mix_classes(src_target[b, :-1], nseg, seg_id_offset)
        chosen = mix_choice(present, seed, first + b)
        for c in chosen:
            out[b, M_BITS + (c >> 5)] |= np.uint32(1 << (c & 31))
        out[b, M_PRESENT], out[b, M_CHOSEN] = len(present), len(chosen)
    return torch.from_numpy(out.view(np.int32))


def mix_selection(records, src_target, nseg, seg_id_offset):
    """bool [B, P*P]: the pixels the records select"""
    records = torch.as_tensor(records).cpu()
    src_target = torch.as_tensor(src_target).cpu()
    P = mix_patch_size(src_target)
    B = src_target.shape[0]
    check_records(records, B, "batch mix")
    rec = records.long()
    c = src_target[:, :-1] - int(seg_id_offset)
    has = (c >= 0) & (c < nseg)
    cc = torch.where(has, c, torch.zeros_like(c))
    word = rec[:, M_BITS:M_BITS + 8].gather(1, cc >> 5)
    sel = has & (((word >> (cc & 31)) & 1) == 1)
    y, x = torch.arange(P)[None, :, None], torch.arange(P)[None, None, :]
    r = lambda k: rec[:, k, None, None]
    box = (y >= r(M_Y0)) & (y < r(M_Y1)) & (x >= r(M_X0)) & (x < r(M_X1))
    return sel | box.reshape(B, P * P)


def mix_apply_reference(records, src, dst, nseg, seg_id_offset):
    """CPU specification of hip.mix_apply.  records int32 [B, 16], src / dst: samples in `train_sample`'s layout or
    (images, target[, weight]) -> (images [B, 3, P, P], target int64 [B, P*P + 1], weight uint8 [B, P*P] | None)"""
    (si, st, sw), (di, dt, dw) = ([None if t is None else torch.as_tensor(t).cpu() for t in mix_batch(x)] for x in (src, dst))
    B, P = check_mix_batches(si, st, sw, di, dt, dw)
    check_mix(P, int(nseg))
    sel = mix_selection(records, st, int(nseg), seg_id_offset)
    # images through an integer view: a copy, whatever the bits say
    iv = torch.int32 if si.dtype == torch.float32 else torch.int16
    images = torch.where(sel.reshape(B, 1, P, P), si.contiguous().view(iv), di.contiguous().view(iv)).view(si.dtype)
    target = dt.clone()
    target[:, :-1] = torch.where(sel, st[:, :-1], dt[:, :-1])
    if sw is None and dw is None:
        return images, target, None
    full = torch.full((B, P * P), 255, dtype=torch.uint8)
    return images, target, torch.where(sel, full if sw is None else sw, full if dw is None else dw)


class BatchMix:
    def __init__(self, P, nseg, seg_id_offset, seed=1, device="cpu", mask="class"):
        """device "cpu" runs the specification of this module, any other device the kernels of csrc/mix.hip"""
        self.P, self.nseg, self.seg_id_offset = int(P), int(nseg), int(seg_id_offset)
        check_mix(self.P, self.nseg, mask, "BatchMix")
        self.seed, self.device, self.mask = int(seed) & _M64, torch.device(device), mask

    def _batch(self, x):
        img, tgt, wgt = mix_batch(x)
        if mix_patch_size(tgt, "BatchMix") != self.P:
            raise ValueError("BatchMix: built for P = %d, got a target of %s" % (self.P, tuple(tgt.shape)))
        return tuple(None if t is None else t.to(self.device) for t in (img, tgt, wgt))

    def draw(self, src, first_ordinal):
        """src: a sample, (images, target[, weight]) or the source target itself -> int32 [B, 16] on the mix's device"""
        tgt = src if torch.is_tensor(src) else mix_batch(src)[1]
        if mix_patch_size(tgt, "BatchMix") != self.P:
            raise ValueError("BatchMix: built for P = %d, got a target of %s" % (self.P, tuple(tgt.shape)))
        tgt = tgt.to(self.device)
        if self.device.type == "cpu":
            return mix_draw_reference(tgt, self.nseg, self.seg_id_offset, self.seed, first_ordinal, self.mask)
        from . import hip
        return hip.mix_draw(tgt.contiguous(), self.nseg, self.seg_id_offset, self.seed, first_ordinal, self.mask)

    def apply(self, records, src, dst, out=None):
        """the caller's records -> (images, target, weight | None); out: (images, target, weight | None) to write into on a
        GPU device, which may be the destination's own tensors"""
        (si, st, sw), (di, dt, dw) = self._batch(src), self._batch(dst)
        check_mix_batches(si, st, sw, di, dt, dw, "BatchMix")
        if self.device.type == "cpu":
            return mix_apply_reference(records, (si, st, sw), (di, dt, dw), self.nseg, self.seg_id_offset)
        from . import hip
        c = lambda t: None if t is None else t.contiguous()
        return hip.mix_apply(records.to(self.device).contiguous(), c(si), c(st), c(di), c(dt), self.nseg, self.seg_id_offset,
                             src_weight=c(sw), dst_weight=c(dw), out=out)

    def __call__(self, src, dst, first_ordinal):
        return self.apply(self.draw(src, first_ordinal), src, dst)


# ------------------------------------------------------------------------------------------------- the strong augmentation
# DACS' `strong_transform` behind the mix: colour jitter (p = 0.8), then Gaussian blur (p = 0.5), on the images of a mixed
# sample -- the CPU specification of `hip.strong_draw` / `hip.strong_apply` (csrc/strong.hip) and `StrongAugment`, the caller
# of both.  Images [B, 3, P, P], fp32 or bf16, in `train_sample`'s layout -> the same shape and dtype; labels and weight
# planes are not touched.  Everything between the input and the output is integer.
#
# GREY LEVELS.  lut = imageio.normalisation_table(mean, std) (fp32 [3, 256], increasing per row: std <= 0 is refused) and
# mid[c][k] = fp32((float64(lut[c][k-1]) + float64(lut[c][k])) / 2), k = 1..255.  The grey level of a value x in plane c is
# q = #{k : fp32(x) >= mid[c][k]}: comparisons only.  Every table value gives its own index back, a NaN gives 0, +inf 255,
# anything else the nearest level.  Plane c holds colour 2 - c under `reverse_channels`, else c, and uses lut[c].
#
# JITTER.  `photometric(q_rgb, record)` above, unchanged, on true colours (planes un-reversed first).
#
# BLUR.  Separable, 9 taps, integer weights w0..w4 with w0 + 2 (w1 + w2 + w3 + w4) = 4096, the border reflected without
# repeating the edge, r(i) = -i for i < 0, 2 (P - 1) - i for i >= P:
#     h[y][x] = sum_{d=-4..4} w|d| q'[y][r(x + d)]      v[y][x] = sum_d w|d| h[r(y + d)][x]      q'' = (v + 2^23) >> 24
# inside unsigned 32 bits (<= 255 2^24 + 2^23); weights (4096, 0, 0, 0, 0) are the identity.  `BLUR_WEIGHTS` int [64, 5]: for
# sigma index s, sigma = 0.15 + s / 64 in [0.15, 1.135), g_i = exp(-i^2 / (2 sigma^2)), Z = g_0 + 2 sum_{i>=1} g_i in float64,
# w_i = floor(4096 g_i / Z + 0.5) for i = 1..4, w_0 = 4096 - 2 sum w_i.  No tap beyond 4 rounds to a non-zero weight, and no
# product 4096 g_i / Z lies closer than 1.3e-3 to a rounding boundary: a libm off by an ulp cannot change the table.
#
# OUTPUT.  lut[c][q''], cast to the image dtype.
#
# RANDOM STREAM.  The transform's t(n, i) at the sample ordinal n = first_ordinal + b, slots 192..199 (the transform ends at
# slot 27, the box uses 28..31, ClassMix at most 32..159):
#
#     192        jitter gate: on iff (t >> 24) < jitter_p8 (205: 0.80)
#     193        bits of t, in slot 23's positions: 1 brightness on, 2 mode, 3 contrast on, 4 saturation on, 5 hue on; the four
#                "on" bits ANDed with the gate
#     194..197   beta, alpha_c, alpha_s, delta by the formulas of slots 24..27
#     198        blur gate: on iff (t >> 24) < blur_p8 (128: 0.50)
#     199        sigma index t >> 26
#
# The record of a sample, int32 [16]:
#
#     0 bright  1 contrast  2 sat  3 hue  4 mode  5 beta  6 alpha_c  7 alpha_s (fp32 bit patterns)  8 delta
#     9 sigma index (-1: blur off)  10..14 w0..w4  15 zero
#
# With blur off words 10..14 are (4096, 0, 0, 0, 0).  A caller may pass its own records (a box filter, say).  A record is
# valid iff words 0..4 are in {0, 1}, the three floats are finite, every w_i >= 0 and w0 + 2 sum w = 4096; delta is reduced
# mod 180.  An invalid record poisons its sample with NaN images; nothing is indexed through a record.
#
# NOT pinned: kornia's float `ColorJitter` and its kernel-size rule (neither kornia nor DACS is available where this project
# is tested).  The jitter is this project's integer PhotoMetricDistortion chain at its existing strengths; the blur truncates
# at radius 4 because 12-bit weights are zero beyond it.
STRONG_SLOT = 192
(S_BRIGHT, S_CONTRAST, S_SAT, S_HUE, S_MODE, S_BETA, S_ALPHA_C, S_ALPHA_S, S_DELTA, S_SIGMA, S_W0) = range(11)
BLUR_RADIUS, BLUR_ONE, BLUR_SIGMAS = 4, 4096, 64
STRONG_MAX_P = 4096


def blur_weights(sigma, taps=BLUR_RADIUS, tail=16):
    """(w0, .., w_taps) of one sigma by the rule above; Z sums every tap up to `tail`, behind which g_i vanishes beside g_0 in
    float64 for any sigma of the table.  Every tap beyond `taps` must round to a zero weight."""
    g = [float(np.exp(np.float64(-i * i) / (2 * np.float64(sigma) ** 2))) for i in range(tail + 1)]
    Z = g[0] + 2 * sum(g[1:])
    w = [int(np.floor(BLUR_ONE * g[i] / Z + 0.5)) for i in range(1, tail + 1)]
    if any(w[taps:]):
        raise ValueError("blur_weights: sigma %r needs more than %d taps" % (sigma, taps))
    return [BLUR_ONE - 2 * sum(w[:taps])] + w[:taps]


BLUR_WEIGHTS = np.array([blur_weights(0.15 + s / 64.0) for s in range(BLUR_SIGMAS)], dtype=np.int64)
BLUR_IDENTITY = (BLUR_ONE, 0, 0, 0, 0)


def check_strong(P, mean=HALF, std=HALF, jitter_p8=205, blur_p8=128, what="strong augmentation"):
    check_patch(P, what, STRONG_MAX_P)
    if len(tuple(mean)) != 3 or len(tuple(std)) != 3 or not all(float(s) > 0 for s in std):
        raise ValueError("%s: mean and std hold three entries and std > 0 (the table must increase), got %r %r" % (what, mean, std))
    for name, p8 in (("jitter_p8", jitter_p8), ("blur_p8", blur_p8)):
        if not 0 <= int(p8) <= 256:
            raise ValueError("%s: %s must lie in 0 .. 256, got %r" % (what, name, p8))


def check_strong_images(images, what="strong augmentation"):
    """-> (B, P) of images fp32 or bf16 [B, 3, P, P]; reads no values"""
    if not torch.is_tensor(images) or images.dtype not in (torch.float32, torch.bfloat16) or images.dim() != 4 \
            or images.shape[0] < 1 or images.shape[1] != 3 or images.shape[2] != images.shape[3]:
        raise ValueError("%s: images must be fp32 or bf16 [B, 3, P, P] with B >= 1, got %s"
                         % (what, (images.dtype, tuple(images.shape)) if torch.is_tensor(images) else type(images)))
    B, P = int(images.shape[0]), int(images.shape[2])
    check_patch(P, what, STRONG_MAX_P)
    if B * 3 * P * P >= 2 ** 31:
        raise ValueError("%s: B * 3 * P * P must stay below 2**31, got B = %d, P = %d" % (what, B, P))
    return B, P


def strong_draw_reference(B, seed, first_ordinal, jitter_p8=205, blur_p8=128):
    """CPU specification of hip.strong_draw -> the records int32 [B, 16] of the samples at ordinals first_ordinal + b"""
    B, first, jitter_p8, blur_p8 = int(B), int(first_ordinal), int(jitter_p8), int(blur_p8)
    check_strong(16, jitter_p8=jitter_p8, blur_p8=blur_p8)
    check_ordinals(first, B, "strong augmentation")
    out = np.zeros((B, RECORD), dtype=np.int32)
    for b in range(B):
        t = draws(seed, first + b, STRONG_SLOT + 8)[STRONG_SLOT:]
        blur = (t[6] >> 24) < blur_p8
        s = t[7] >> 26
        out[b, :S_W0] = photo_words(t[1:6], (t[0] >> 24) < jitter_p8) + (s if blur else -1,)
        out[b, S_W0:S_W0 + 5] = BLUR_WEIGHTS[s] if blur else BLUR_IDENTITY
    return torch.from_numpy(out)


def strong_midpoints(lut):
    """fp32 [3, 255]: mid[c][k - 1] = fp32((float64(lut[c][k-1]) + float64(lut[c][k])) / 2), k = 1..255"""
    t = np.asarray(lut, dtype=np.float32).astype(np.float64)
    return ((t[:, :-1] + t[:, 1:]) / 2).astype(np.float32)


def grey_levels(images, mean=HALF, std=HALF):
    """images fp32 or bf16 [..., 3, H, W] -> int64 of the same shape: per plane c the number of midpoints of lut[c] at or
    below the value (0 for a NaN).  The midpoints do not decrease, so the count is a search."""
    check_strong(16, mean, std)
    mid = strong_midpoints(normalisation_table(mean, std).numpy())
    x = torch.as_tensor(images).cpu().float().numpy()
    q = np.empty(x.shape, dtype=np.int64)
    for c in range(3):
        assert bool((np.diff(mid[c]) >= 0).all())
        plane = x[..., c, :, :]
        q[..., c, :, :] = np.where(np.isnan(plane), 0, np.searchsorted(mid[c], plane, side="right"))
    return q


def strong_record_valid(rec):
    rec = [int(v) for v in rec]
    w = rec[S_W0:S_W0 + 5]
    return (all(v in (0, 1) for v in rec[S_BRIGHT:S_MODE + 1]) and all(bool(np.isfinite(bits_f32(v))) for v in rec[S_BETA:S_ALPHA_S + 1])
            and all(v >= 0 for v in w) and w[0] + 2 * sum(w[1:]) == BLUR_ONE)


def blur_levels(q, w):
    """integer grey levels [P, P, C] under weights (w0..w4) -> int64 [P, P, C] by the rule above"""
    q = np.asarray(q).astype(np.int64)
    P, R = q.shape[0], BLUR_RADIUS
    w = [int(v) for v in w]
    pad = np.pad(q, ((R, R), (R, R), (0, 0)), mode="reflect")                      # numpy's "reflect" does not repeat the edge
    h = sum(w[abs(d)] * pad[:, R + d:R + d + P] for d in range(-R, R + 1))         # [P + 8, P, C]: h at the reflected rows
    v = sum(w[abs(d)] * h[R + d:R + d + P] for d in range(-R, R + 1))
    assert int(v.max()) <= 255 << 24
    return (v + (1 << 23)) >> 24


def strong_apply_reference(records, images, mean=HALF, std=HALF, reverse_channels=False):
    """CPU specification of hip.strong_apply.  records int32 [B, 16], images fp32 or bf16 [B, 3, P, P] -> images of the same
    shape and dtype: grey levels, jitter, blur, table, per sample under its record; NaN for an invalid record."""
    images = torch.as_tensor(images).cpu()
    B, P = check_strong_images(images)
    check_strong(P, mean, std)
    records = torch.as_tensor(records).cpu()
    check_records(records, B, "strong augmentation")
    lut = normalisation_table(mean, std)
    q = grey_levels(images, mean, std)                                             # [B, 3, P, P], planes
    out = torch.empty(B, 3, P, P, dtype=images.dtype)
    for b in range(B):
        rec = records[b].tolist()
        if not strong_record_valid(rec):
            out[b] = float("nan")
            continue
        rgb = np.moveaxis(q[b][::-1] if reverse_channels else q[b], 0, -1)         # [P, P, 3], true colours
        qq = blur_levels(photometric(rgb, rec, base=S_BRIGHT), rec[S_W0:S_W0 + 5])
        planes = torch.from_numpy(np.ascontiguousarray(np.moveaxis(qq, -1, 0)))
        if reverse_channels:
            planes = planes.flip(0)
        out[b] = torch.stack([lut[c][planes[c]] for c in range(3)]).to(images.dtype)
    return out


class StrongAugment:
    def __init__(self, P, mean=HALF, std=HALF, seed=1, device="cpu", jitter_p8=205, blur_p8=128, reverse_channels=False):
        """device "cpu" runs the specification of this module, any other device the kernels of csrc/strong.hip"""
        self.P = int(P)
        check_strong(self.P, mean, std, jitter_p8, blur_p8, "StrongAugment")
        self.mean, self.std = tuple(float(x) for x in mean), tuple(float(x) for x in std)
        self.seed, self.device = int(seed) & _M64, torch.device(device)
        self.jitter_p8, self.blur_p8, self.reverse_channels = int(jitter_p8), int(blur_p8), bool(reverse_channels)

    def draw(self, B, first_ordinal):
        """-> int32 [B, 16] on the augmentation's device"""
        if self.device.type == "cpu":
            return strong_draw_reference(B, self.seed, first_ordinal, self.jitter_p8, self.blur_p8)
        from . import hip
        return hip.strong_draw(B, self.seed, first_ordinal, self.jitter_p8, self.blur_p8, device=self.device)

    def apply(self, records, images, out=None):
        """the caller's records -> images; out: a tensor to write into on a GPU device, which shares no byte with `images`"""
        B, P = check_strong_images(images, "StrongAugment")
        if P != self.P:
            raise ValueError("StrongAugment: built for P = %d, got images of %s" % (self.P, tuple(images.shape)))
        images = images.to(self.device)
        if self.device.type == "cpu":
            return strong_apply_reference(records, images, self.mean, self.std, self.reverse_channels)
        from . import hip
        return hip.strong_apply(records.to(self.device).contiguous(), images.contiguous(), self.mean, self.std,
                                self.reverse_channels, out=out)

    def __call__(self, images, first_ordinal):
        return self.apply(self.draw(images.shape[0], first_ordinal), images)
