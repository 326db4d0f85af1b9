"""CPU: the specification of the training transform (ifseg_amd/augment.py) -- the integer HSV rule against its float64
definition, the photometric stage against a restatement of mmseg's PhotoMetricDistortion, the drawn parameters, the crop choice
against brute force, the link to `imageio.image_load_reference`, the sample layout of `SegmentationTask.train_sample` and the
C header."""
import os
import re

import numpy as np
import pytest
import torch

import _image_load_cases as IC
import _train_load_cases as C
from ifseg_amd import augment as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------- HSV
def _colours():
    """a lattice of the cube, all greys, and every colour with a channel at 0 or 255 on a finer lattice"""
    ax = np.arange(0, 256, 5)
    lat = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    grey = np.repeat(np.arange(256)[:, None], 3, 1)
    fine = np.arange(256)
    faces = []
    for ch in range(3):
        for end in (0, 255):
            a, b = np.meshgrid(fine, fine, indexing="ij")
            f = np.stack([a.reshape(-1), b.reshape(-1)], -1)
            faces.append(np.insert(f, ch, end, axis=1))
    return np.concatenate([lat, grey] + faces)


def _hsv_float64(rgb):
    r, g, b = (rgb[:, i].astype(np.float64) for i in range(3))
    V = np.maximum(np.maximum(r, g), b)
    d = V - np.minimum(np.minimum(r, g), b)
    S = np.where(V > 0, 255 * d / np.maximum(V, 1), 0)
    dd = np.maximum(d, 1)
    H = np.where(V == r, 30 * (g - b) / dd, np.where(V == g, 60 + 30 * (b - r) / dd, 120 + 30 * (r - g) / dd))
    H = np.where(d > 0, H, 0)
    return np.stack([np.floor(H + 0.5) % 180, np.floor(S + 0.5), V], -1).astype(np.int64)


def test_hsv_rule():
    rgb = _colours()
    hsv = A.rgb_to_hsv8(rgb)
    assert np.array_equal(hsv, _hsv_float64(rgb))
    assert hsv[:, 0].min() == 0 and hsv[:, 0].max() == 179 and hsv[:, 1].max() == 255
    back = A.hsv8_to_rgb(hsv)
    assert np.array_equal(back.max(-1), hsv[:, 2])
    err = np.abs(back - rgb).max()
    print("HSV round trip: max error %d grey levels over %d colours" % (err, len(rgb)))
    assert err <= 4
    assert back.min() >= 0 and back.max() <= 255


# ------------------------------------------------------------------------------------------------- photometric
def _mmseg_photometric(img, draws):
    """mmseg's PhotoMetricDistortion.__call__ restated: `draws` replays its random calls in order (randint(2), uniform, ...);
    mmcv's bgr2hsv / hsv2bgr are the 8-bit conversions of the specification (the image here is RGB)"""
    it = iter(draws)

    def convert(x, alpha=1, beta=0):
        x = x.astype(np.float32) * np.float32(alpha) + np.float32(beta)
        return np.clip(x, 0, 255).astype(np.uint8)

    def brightness(img):
        if next(it):
            return convert(img, beta=next(it))
        return img

    def contrast(img):
        if next(it):
            return convert(img, alpha=next(it))
        return img

    def saturation(img):
        if next(it):
            hsv = A.rgb_to_hsv8(img)
            hsv[:, :, 1] = convert(hsv[:, :, 1], alpha=next(it))
            img = A.hsv8_to_rgb(hsv).astype(np.uint8)
        return img

    def hue(img):
        if next(it):
            hsv = A.rgb_to_hsv8(img)
            hsv[:, :, 0] = (hsv[:, :, 0].astype(int) + next(it)) % 180
            img = A.hsv8_to_rgb(hsv).astype(np.uint8)
        return img

    img = brightness(img)
    mode = next(it)
    if mode == 1:
        img = contrast(img)
    img = saturation(img)
    img = hue(img)
    if mode == 0:
        img = contrast(img)
    return img


def _photo_image():
    """random colours, plus pixels that clip: near black, near white, saturated primaries (S = 255) and greys (S = 0), and hues
    within 18 of both ends of [0, 180)"""
    g = np.random.default_rng(5)
    rnd = g.integers(0, 256, (24, 16, 3))
    edge = np.array([[0, 0, 0], [255, 255, 255], [3, 1, 2], [250, 254, 253], [255, 0, 0], [0, 255, 0], [0, 0, 255], [128, 128, 128],
                     [255, 0, 20], [255, 20, 0], [200, 10, 40], [200, 40, 10], [255, 255, 0], [1, 255, 254], [90, 30, 30], [30, 30, 90]])
    return np.concatenate([rnd, np.tile(edge[None], (2, 1, 1))], 0).astype(np.uint8)


@pytest.mark.parametrize("combo", range(32))
def test_photometric_against_mmseg_control_flow(combo):
    b_on, mode, c_on, s_on, h_on = ((combo >> i) & 1 for i in range(5))
    img = _photo_image()
    seen_wrap_lo = seen_wrap_hi = seen_s_clip = seen_lo = seen_hi = False
    for beta, alpha_c, alpha_s, delta in ((C.BLO, C.LO, C.LO, -18), (C.BHI, C.HI, C.HI, 17), (-7.25, 1.25, 0.75, 5)):
        rec = C.record(64, 64, 0, 0, 0, b_on, c_on, s_on, h_on, mode, beta, alpha_c, alpha_s, delta)
        draws = [b_on] + ([np.float32(beta)] if b_on else []) + [mode]
        con = [c_on] + ([np.float32(alpha_c)] if c_on else [])
        mid = [s_on] + ([np.float32(alpha_s)] if s_on else []) + [h_on] + ([delta] if h_on else [])
        draws += (con + mid) if mode == 1 else (mid + con)
        got = A.photometric(img, rec)
        assert got.dtype == np.uint8 and np.array_equal(got, _mmseg_photometric(img, draws))
        # what the inputs have to exercise (checked on the stage's own input, brightness being the first stage)
        hsv = A.rgb_to_hsv8(img)
        seen_wrap_lo |= bool((hsv[..., 0] + delta < 0).any())
        seen_wrap_hi |= bool((hsv[..., 0] + delta >= 180).any())
        seen_s_clip |= bool((hsv[..., 1].astype(np.float32) * np.float32(alpha_s) > 255).any()) and bool((hsv[..., 1] == 0).any())
        seen_lo |= bool((img.astype(np.float32) + np.float32(beta) < 0).any())
        seen_hi |= bool((img.astype(np.float32) + np.float32(beta) > 255).any())
    assert seen_wrap_lo and seen_wrap_hi and seen_s_clip and seen_lo and seen_hi


def test_photometric_clipping_and_wrap_values():
    """hand-checked values: brightness clips at both ends, S clips at 255 and stays 0 on a grey, hue wraps at both ends"""
    px = np.array([[[10, 200, 250]]], dtype=np.uint8)
    assert A.photometric(px, C.record(64, 64, 0, 0, bright=1, beta=-32.0)).tolist() == [[[0, 168, 218]]]
    assert A.photometric(px, C.record(64, 64, 0, 0, bright=1, beta=31.5)).tolist() == [[[41, 231, 255]]]
    assert A.convert(np.array([200, 255]), alpha=1.4).tolist() == [255, 255] and A.convert(np.array([3]), alpha=0.5).tolist() == [1]
    grey = np.array([[[77, 77, 77]]], dtype=np.uint8)
    assert np.array_equal(A.photometric(grey, C.record(64, 64, 0, 0, sat=1, alpha_s=C.HI, hue=1, delta=17)), grey)
    red = np.array([[[255, 0, 10]]])                                    # H = round(30 * -10 / 255) mod 180 = 179
    assert A.rgb_to_hsv8(red)[0, 0].tolist() == [179, 255, 255]
    h_of = lambda rec: int(A.rgb_to_hsv8(A.photometric(red.astype(np.uint8), rec))[0, 0, 0])
    assert h_of(C.record(64, 64, 0, 0, hue=1, delta=17)) == 16                                       # 179 + 17 wraps to 16
    orange = np.array([[[255, 20, 0]]], dtype=np.uint8)                 # H = round(30 * 20 / 255) = 2
    assert A.rgb_to_hsv8(orange)[0, 0, 0] == 2
    assert int(A.rgb_to_hsv8(A.photometric(orange, C.record(64, 64, 0, 0, hue=1, delta=-18)))[0, 0, 0]) == 164   # 2 - 18 wraps


# ------------------------------------------------------------------------------------------------- drawn parameters
def test_scale_rule():
    for P in (64, 96, 512):
        assert A.new_short_of(0, P) == P and A.new_short_of(2 ** 32 - 1, P) == 2 * P - 1
        for t in (1, 2 ** 30, (2 ** 32) // 3, (2 ** 32) // 3 + 1):
            r = 0.5 + 1.5 * t / 2 ** 32
            assert A.new_short_of(t, P) == max(int(P * r), P)
            if r < 1:
                assert A.new_short_of(t, P) == P
        assert A.new_short_of(12345, P, 2, 0) == P                      # ratio_range (1, 1)
    P, seed = 64, 9
    t0 = np.array([A.draws(seed, n, 1)[0] for n in range(4096)])
    ns = np.array([A.new_short_of(int(t), P) for t in t0])
    assert ns.min() == P and ns.max() < 2 * P
    # P(r < 1) = 1/3, plus P(int(P r) = P) = 1 / (1.5 P): 0.344 at P = 64; the binomial sd over 4096 draws is 0.7 %
    share = float((ns == P).mean())
    print("share of new_short == P over 4096 ordinals: %.4f" % share)
    assert 0.28 <= share <= 0.40
    # the long side, and the refusal of 2 in out >= 2^31
    assert A.resized_size(480, 640, 512) == (512, (2 * 512 * 640 + 480) // 960) == (512, 683)
    assert A.resized_size(375, 500, 64) == (64, 85) and A.resized_size(500, 375, 64) == (85, 64)
    with pytest.raises(ValueError, match="2 \\*\\* 31|2\\*\\*31"):
        A.draw_params([(2 ** 16, 8)], [torch.zeros(2 ** 16, 8, dtype=torch.uint8)], 1024, 5, 1, 0)


def test_record_fields_and_grids():
    lab = C.label("checker", 40, 50)
    recs = A.draw_params([(40, 50)] * 64, [lab] * 64, 64, C.NSEG, 5, 100)
    assert recs.dtype == torch.int32 and recs.shape == (64, 16)
    for n, rec in enumerate(recs.tolist()):
        t = A.draws(5, 100 + n)
        new_h, new_w, off_h, off_w, k = rec[:5]
        assert (new_h, new_w) == A.resized_size(40, 50, A.new_short_of(t[0], 64)) and k == 0
        assert 0 <= off_h <= new_h - 64 and 0 <= off_w <= new_w - 64
        assert rec[5:11] == [t[23] & 1, (t[23] >> 1) & 1, (t[23] >> 3) & 1, (t[23] >> 4) & 1, (t[23] >> 5) & 1, (t[23] >> 2) & 1]
        beta, ac, as_ = (float(A.bits_f32(rec[i])) for i in (11, 12, 13))
        assert -32 <= beta < 32 and beta * 2 ** 17 == int(beta * 2 ** 17)
        assert 0.5 <= ac < 1.5 and ac * 2 ** 23 == int(ac * 2 ** 23) and 0.5 <= as_ < 1.5 and as_ * 2 ** 23 == int(as_ * 2 ** 23)
        assert -18 <= rec[14] <= 17 and rec[15] == 0
    assert set(recs[:, 5].tolist()) == {0, 1} and len(set(recs[:, 14].tolist())) > 10
    off = A.draw_params([(40, 50)] * 64, [lab] * 64, 64, C.NSEG, 5, 100, photometric=False, flip=False)
    assert not off[:, 5:10].any() and torch.equal(off[:, :5], recs[:, :5]) and torch.equal(off[:, 10:], recs[:, 10:])


def test_batching_is_by_ordinal():
    imgs, labs = C.ragged_batch()
    shapes = [tuple(l.shape) for l in labs]
    for first in C.DRAW_ORDINALS:
        recs = A.draw_params(shapes, labs, 64, C.NSEG, 3, first)
        for b in range(len(labs)):
            assert torch.equal(recs[b], A.draw_params(shapes[b:b + 1], labs[b:b + 1], 64, C.NSEG, 3, first + b)[0])
    tf = A.TrainTransform(64, C.NSEG, C.SEG0, seed=3)
    img_b, tgt_b = tf(imgs, labs, 7)
    for b in (0, 3):
        i1, t1 = tf(imgs[b:b + 1], labs[b:b + 1], 7 + b)
        assert torch.equal(i1[0], img_b[b]) and torch.equal(t1[0], tgt_b[b])
    with pytest.raises(ValueError, match="ordinals"):
        A.draw_params(shapes, labs, 64, C.NSEG, 3, 2 ** 32 - 2)


# ------------------------------------------------------------------------------------------------- crop choice
def _brute_force_k(lab, rec_size, P, t):
    """mmseg's RandomCrop.__call__ on the resized class map, with np.unique as it writes it"""
    new_h, new_w = rec_size
    H0, W0 = lab.shape
    cls = A.remap_label(lab, C.NSEG).numpy()
    full = cls[np.minimum(np.arange(new_h) * H0 // new_h, H0 - 1)][:, np.minimum(np.arange(new_w) * W0 // new_w, W0 - 1)]
    for k in range(10):
        oh, ow = (t[1 + 2 * k] * (new_h - P + 1)) >> 32, (t[2 + 2 * k] * (new_w - P + 1)) >> 32
        labels, cnt = np.unique(full[oh:oh + P, ow:ow + P], return_counts=True)
        cnt = cnt[labels != 255]
        if len(cnt) > 1 and np.max(cnt) / np.sum(cnt) < 0.75:
            return k, oh, ow
    return 10, (t[21] * (new_h - P + 1)) >> 32, (t[22] * (new_w - P + 1)) >> 32


@pytest.mark.parametrize("ratio", [(1.0, 1.0), (0.5, 2.0)])
def test_crop_choice_against_brute_force(ratio):
    P, H0, W0 = 64, 32, 80                                              # resized: 64 x 160 at ratio 1
    ks = {}
    for kind in ("checker", "flat", "mixed"):
        lab = C.label(kind, H0, W0)
        recs = A.draw_params([(H0, W0)] * 32, [lab] * 32, P, C.NSEG, C.CROP_SEED, 0, ratio_range=ratio)
        for n, rec in enumerate(recs.tolist()):
            if ratio == (1.0, 1.0):
                assert rec[:2] == [64, 160]
            assert (rec[4], rec[2], rec[3]) == _brute_force_k(lab, rec[:2], P, A.draws(C.CROP_SEED, n)), (kind, n)
        ks[kind] = recs[:, 4].tolist()
    assert set(ks["checker"]) == {0} and set(ks["flat"]) == {10}
    print("mixed map, k over 32 ordinals:", ks["mixed"])
    assert 0 in ks["mixed"] and any(1 <= k <= 9 for k in ks["mixed"])


# ------------------------------------------------------------------------------------------------- link to image_load
@pytest.mark.parametrize("shape", [(37, 29), (16, 24), (50, 120)])
def test_plain_transform_is_image_load_cropped(shape):
    from ifseg_amd.imageio import image_load_reference
    H0, W0 = shape
    P = 32
    img, lab = C.image(H0, W0, 1), C.label("random", H0, W0)
    tf = A.TrainTransform(P, C.NSEG, C.SEG0, seed=4, photometric=False, flip=False, ratio_range=(1, 1))
    rec = tf.draw([img], [lab], 17)
    new_h, new_w, off_h, off_w = rec[0, :4].tolist()
    assert min(new_h, new_w) == P and not rec[0, 5:10].any()
    out, tgt = tf.apply([img], [lab], rec)
    full = image_load_reference(img[None], new_h, new_w)[0]
    assert out.dtype == torch.float32 and torch.equal(out, full[:, :, off_h:off_h + P, off_w:off_w + P])
    cls = A.remap_label(lab, C.NSEG)[A.nearest_axis(new_h, H0)][:, A.nearest_axis(new_w, W0)]
    want = torch.cat([C.SEG0 + cls[off_h:off_h + P, off_w:off_w + P].reshape(-1), torch.tensor([2])])
    assert tgt.dtype == torch.int64 and torch.equal(tgt[0], want) and torch.equal(tgt[0], C.target_of(lab, rec[0], P))
    # flip mirrors both, class ids are taken as they are with raw_labels=False, reversed planes are reversed planes
    rec[0, A.R_FLIP] = 1
    o2, t2 = tf.apply([img], [lab], rec)
    assert torch.equal(o2, out.flip(-1)) and torch.equal(t2[0, :-1].view(P, P), tgt[0, :-1].view(P, P).flip(-1))
    ids = A.TrainTransform(P, C.NSEG, C.SEG0, raw_labels=False, reverse_channels=True, dtype=torch.bfloat16)
    o3, t3 = ids.apply([img], [lab], rec)
    assert o3.dtype == torch.bfloat16 and torch.equal(o3, o2.flip(1).to(torch.bfloat16))
    assert torch.equal(t3[0, :-1] - C.SEG0, lab.long().clamp_max(C.NSEG)[A.nearest_axis(new_h, H0)][:, A.nearest_axis(new_w, W0)]
                       [off_h:off_h + P, off_w:off_w + P].flip(-1).reshape(-1))
    # a record that holds no window, and a label map of another size
    bad = rec.clone()
    bad[0, 0] = P - 1
    with pytest.raises(ValueError, match="window"):
        tf.apply([img], [lab], bad)
    with pytest.raises(ValueError, match="label map"):
        tf([img], [lab[:-1]], 0)


def test_general_cases_margin_cap_and_exact_family_is_exact():
    """what the GPU file relies on: the undecided share of every general case is below the cap, and on the exact family the
    fp32 and the fp64 specification are the same tensors"""
    for i in range(len(C.GENERAL_SOURCES)):
        img, lab, rec, ref, ys, xs = C.general_case(i)
        print(C.GENERAL_SOURCES[i], "->", rec[:4].tolist(), "e = %.2e, left out %.3f %%" % (ref.e, 100 * ref.undecided_share))
        assert ref.undecided_share <= IC.MARGIN_CAP
    for which in (0, 1):
        P, imgs, labs, params = C.exact_family(which)
        n32, t32, q32, q032 = C.exact_reference(which)
        n64, t64, q64, q064 = A.train_load_reference(imgs, labs, params, P, C.NSEG, C.SEG0)
        assert torch.equal(n32, n64) and torch.equal(t32, t64) and torch.equal(q32, q64) and torch.equal(q032, q064)
        for b in range(len(imgs)):
            assert torch.equal(t32[b], C.target_of(labs[b], params[b], P))
        changed = [(q32[b] != q032[b]).any().item() for b in range(len(imgs))]
        assert changed == [False] + [True] * 7


# ------------------------------------------------------------------------------------------------- task surface
def test_train_sample_layout():
    from ifseg_amd.artificial import trainer_first_ordinal
    from ifseg_amd.predict import source_tokens
    from ifseg_amd.tasks.mm_tasks import SegmentationTask
    from ifseg_amd.tasks.mm_tasks.segmentation import PROMPT_IDS
    names = [[31], [32, 33], [34], [35, 36, 37], [38]]
    task = SegmentationTask(num_seg_tokens=5, patch_image_size=64, n_base_vocab=C.SEG0, category_token_ids=names)
    tf = task.build_train_transform("cpu", seed=2)
    assert (tf.P, tf.nseg, tf.seg_id_offset, tf.seed, tf.mean) == (64, 5, C.SEG0, 2, (0.5, 0.5, 0.5))
    imgs, labs = C.ragged_batch()
    first = trainer_first_ordinal(3, 0, 0, 1, 1, len(imgs))
    s = task.train_sample(imgs, labs, first)
    task.src_len = source_tokens(names, PROMPT_IDS).numel()
    syn = task.synthetic_sample(len(imgs), "cpu")

    def walk(a, b, path=""):
        assert type(a) is type(b), (path, type(a), type(b))
        if isinstance(a, dict):
            assert list(a) == list(b), (path, list(a), list(b))
            for k in a:
                walk(a[k], b[k], path + "/" + k)
        elif isinstance(a, torch.Tensor):
            assert a.dtype == b.dtype and a.shape == b.shape, (path, a.dtype, b.dtype, a.shape, b.shape)
        else:
            assert a == b, (path, a, b)
    walk(s, syn)
    assert s["ntokens"] == len(imgs) * (64 * 64 + 1)
    assert torch.equal(s["net_input"]["src_tokens"][1], source_tokens(names, PROMPT_IDS))
    tgt = s["target"]
    assert (tgt[:, -1] == 2).all() and tgt[:, :-1].min() >= C.SEG0 and tgt[:, :-1].max() <= C.SEG0 + 5
    again = task.train_sample(imgs, labs, first)
    assert torch.equal(again["net_input"]["patch_images"], s["net_input"]["patch_images"]) and torch.equal(again["target"], tgt)
    other = task.train_sample(imgs, labs, first + len(imgs))
    assert not torch.equal(other["net_input"]["patch_images"], s["net_input"]["patch_images"])
    imagenet = SegmentationTask(num_seg_tokens=5, patch_image_size=64, n_base_vocab=C.SEG0, category_token_ids=names)
    imagenet.cfg.imagenet_default_mean_and_std = True
    assert imagenet.build_train_transform().mean == (0.485, 0.456, 0.406)


def test_header_declares_the_entry_points_and_keeps_the_abi():
    h = open(os.path.join(ROOT, "include", "ifseg_hip.h")).read()
    assert re.search(r"#define IFSEG_ABI_VERSION 21\b", h)
    for sym in ("ifseg_train_draw", "ifseg_train_load", "ifseg_train_load_staging"):
        assert re.search(r"\bint %s\(" % sym, h), sym
    assert "ifseg_train_src" in h
    from ifseg_amd import hip
    assert hip.ABI_VERSION == 21 and callable(hip.train_draw) and callable(hip.train_load)
