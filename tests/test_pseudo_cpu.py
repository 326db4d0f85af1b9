"""CPU: the specification of the pseudo-label path (`ifseg_amd.predict`: conf_bin, confidence_histogram_reference,
pseudo_thresholds, pseudo_label_reference, ConfidenceHistogram) by its properties and against an independent per-pixel loop,
the header, the refusals of the bindings, the ops and `Segmenter.pseudo_label_raw` before anything reaches the library, and
the launch sequence of `pseudo_label_raw` with recording fakes."""
import os
import re

import pytest
import torch

from ifseg_amd import augment, hip
from ifseg_amd.predict import (ConfidenceHistogram, PseudoLabelResult, Segmenter, conf_bin, confidence_histogram_reference,
                               default_palette, pseudo_label_reference, pseudo_thresholds, render_reference)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 11, 13
SPECIAL = [0.0, 1.0, float("nan"), float("inf"), float("-inf"), 1.7, -0.3, 255 / 256]


def _case(dtype, n, seed=0):
    """an 11 x 13 label map of blocks, single pixels and values outside [0, n), and a confidence plane with every special value"""
    g = torch.Generator().manual_seed(seed)
    labels = torch.randint(0, n, (4, 5), generator=g).repeat_interleave(3, 0).repeat_interleave(3, 1)[:H, :W].clone()
    labels[2, 3], labels[10, 12], labels[0, 0] = (labels[2, 3] + 1) % n, (labels[10, 12] + 1) % n, (labels[0, 0] + 1) % n
    labels[5, 6:9] = 255
    if dtype == torch.int16:
        labels[7:9, 1] = -1
        labels[9, 9] = 300
    conf = torch.rand(H, W, generator=g)
    conf[0, :8] = torch.tensor(SPECIAL)
    return labels.to(dtype), conf


def test_conf_bin():
    below, above = torch.nextafter(torch.tensor(0.5), torch.tensor(0.0)), torch.nextafter(torch.tensor(0.5), torch.tensor(1.0))
    conf = torch.tensor(SPECIAL + [float(below), 0.5, float(above), 1 / 256, float(torch.nextafter(torch.tensor(1 / 256), torch.tensor(0.0)))])
    assert conf_bin(conf).tolist() == [0, 255, 0, 255, 0, 255, 0, 255, 127, 128, 128, 1, 0]
    assert conf_bin(conf).dtype == torch.int64
    with pytest.raises(ValueError):
        conf_bin(conf.double())


@pytest.mark.parametrize("dtype,n", [(torch.uint8, 15), (torch.int16, 7)])
def test_histogram_reference_against_a_loop(dtype, n):
    labels, conf = _case(dtype, n)
    hist, tally = confidence_histogram_reference(labels, conf, n)
    want, inside = torch.zeros(n, 256, dtype=torch.int64), 0
    bins = conf_bin(conf).tolist()
    for y in range(H):
        for x in range(W):
            l = int(labels[y, x])
            if 0 <= l < n:
                want[l, bins[y][x]] += 1
                inside += 1
    assert hist.dtype == torch.int64 and torch.equal(hist, want)
    assert tally.tolist() == [inside, H * W - inside] and int(hist.sum()) == inside and inside < H * W
    with pytest.raises(ValueError):
        confidence_histogram_reference(labels.float(), conf, n)
    with pytest.raises(ValueError):
        confidence_histogram_reference(labels, conf[:, :12], n)


def _random_hist(n, seed):
    g = torch.Generator().manual_seed(seed)
    hist = torch.randint(0, 50, (n, 256), generator=g) * (torch.rand(n, 256, generator=g) < 0.3)
    hist[1] = 0                                                   # a class without pixels
    hist[2] = 0
    hist[2, 200] = 40                                             # a class in one bin: every threshold ties
    return hist.long()


def test_threshold_rule():
    n = 9
    hist = _random_hist(n, 1)
    N = hist.sum(1)
    S = lambda t: hist[:, t:].sum(1) if t < 256 else torch.zeros_like(N)
    t = pseudo_thresholds(hist)                                   # keep = 1, floor = 0: everything
    assert t.dtype == torch.int32 and t.tolist() == [0] * n
    t = pseudo_thresholds(hist, keep=0.0)                         # nothing: above the class's highest occupied bin
    for c in range(n):
        top = hist[c].nonzero()
        assert int(t[c]) == (int(top.max()) + 1 if top.numel() else 0)
    for keep in (0.1, 0.5, 0.75, 0.999):
        t = pseudo_thresholds(hist, keep=keep)
        K = (N * int(round(keep * 65536))) >> 16
        for c in range(n):
            tc = int(t[c])
            assert 0 <= tc <= 256 and int(S(tc)[c]) <= int(K[c])
            if tc > 0:
                assert int(S(tc - 1)[c]) > int(K[c])
        assert int(t[1]) == 0 and int(t[2]) == 201               # no pixels: the floor; one bin that ties: rejected whole
    for floor in (0.3, 0.5, 1.0, 1 / 512):
        want = {0.3: 77, 0.5: 128, 1.0: 256, 1 / 512: 1}[floor]
        assert pseudo_thresholds(hist, floor=floor).tolist() == [want] * n
        assert (pseudo_thresholds(hist, keep=0.5, floor=floor) >= want).all()
        assert int(pseudo_thresholds(hist, keep=0.5, floor=floor)[1]) == want
    for kw in (dict(keep=1.01), dict(keep=-0.1), dict(floor=1.5), dict(floor=-1e-9), dict(keep=float("nan")), dict(keep="0.5")):
        with pytest.raises(ValueError):
            pseudo_thresholds(hist, **kw)
    for bad in (hist.int(), hist[:, :255], hist[0]):
        with pytest.raises(ValueError):
            pseudo_thresholds(bad)


def _loop(labels, conf, thr, n, r, raw):
    """the rule of pseudo_label_reference, pixel by pixel in Python integers"""
    lab, bins = labels.tolist(), conf_bin(conf).tolist()
    out = torch.full((H, W), 255, dtype=torch.uint8)
    kept = torch.zeros(2, n, dtype=torch.int64)
    for y in range(H):
        for x in range(W):
            l = lab[y][x]
            if not 0 <= l < n:
                continue
            kept[1, l] += 1
            edge = any(lab[yy][xx] != l for yy in range(max(y - r, 0), min(y + r, H - 1) + 1)
                       for xx in range(max(x - r, 0), min(x + r, W - 1) + 1))
            if not edge and bins[y][x] >= thr[l]:
                out[y, x] = l + (1 if raw else 0)
                kept[0, l] += 1
    return out, kept


@pytest.mark.parametrize("dtype,n", [(torch.uint8, 15), (torch.int16, 7)])
def test_filter_reference_against_a_loop(dtype, n):
    labels, conf = _case(dtype, n)
    thr = torch.randint(0, 257, (n,), generator=torch.Generator().manual_seed(3), dtype=torch.int32)
    thr[0], thr[1] = 0, 256
    for r in (0, 1, 2, 4):
        for raw in (True, False):
            out, kept = pseudo_label_reference(labels, conf, thr, n, r, raw)
            want, wkept = _loop(labels, conf, thr.tolist(), n, r, raw)
            assert out.dtype == torch.uint8 and torch.equal(out, want) and torch.equal(kept, wkept), (r, raw)
    both = pseudo_label_reference(torch.stack([labels, labels.flip(0)]), torch.stack([conf, conf.flip(0)]), thr, n, 1)
    one = pseudo_label_reference(labels, conf, thr, n, 1)
    assert torch.equal(both[0][0], one[0]) and torch.equal(both[0][1], one[0].flip(0)) and torch.equal(both[1], 2 * one[1])


def test_filter_properties():
    n = 15
    labels, conf = _case(torch.uint8, n)
    inside = labels < n
    hist, tally = confidence_histogram_reference(labels, conf, n)
    # keep = 1, floor = 0 keeps every in-range pixel; keep = 0 none
    out, kept = pseudo_label_reference(labels, conf, pseudo_thresholds(hist), n)
    assert torch.equal(out != 255, inside) and torch.equal(kept[0], kept[1]) and int(kept[1].sum()) == int(tally[0])
    assert torch.equal(kept[1], hist.sum(1))
    out, kept = pseudo_label_reference(labels, conf, pseudo_thresholds(hist, keep=0.0), n)
    assert (out == 255).all() and not kept[0].any() and torch.equal(kept[1], hist.sum(1))
    # the class-balanced share: at most keep N_c of every class, and the most confident ones
    out, kept = pseudo_label_reference(labels, conf, pseudo_thresholds(hist, keep=0.5), n)
    assert (kept[0] <= (kept[1] * 32768 >> 16)).all() and 0 < int(kept[0].sum()) < int(kept[1].sum())
    # floor = tau is honoured
    for tau in (0.25, 0.5, 0.9):
        out, _ = pseudo_label_reference(labels, conf, pseudo_thresholds(hist, floor=tau), n)
        assert (conf[out != 255] >= tau).all() and (out != 255).any()
        if tau * 256 == int(tau * 256):                           # a threshold on a bin's edge is the comparison itself
            assert torch.equal(out != 255, inside & (torch.nan_to_num(conf, nan=0.0) >= tau))
    # the boundary band is render_reference's contour mask: opacity 0 leaves a black image black except for the marker colour
    for r in (1, 2, 4):
        marker = torch.tensor([255, 0, 255], dtype=torch.uint8)
        pic = render_reference(labels, torch.zeros(H, W, 3, dtype=torch.uint8), default_palette(n), 0.0, r, (255, 0, 255))
        edge = (pic == marker).all(-1)
        out, _ = pseudo_label_reference(labels, conf, torch.zeros(n, dtype=torch.int32), n, r)
        assert torch.equal(out != 255, inside & ~edge) and edge.any() and (r > 1 or (inside & ~edge).any())
    # augment.remap_label undoes the raw encoding: the kept classes, n elsewhere
    thr = pseudo_thresholds(hist, keep=0.5)
    raw, _ = pseudo_label_reference(labels, conf, thr, n, 1, raw_labels=True)
    ids, _ = pseudo_label_reference(labels, conf, thr, n, 1, raw_labels=False)
    keep = raw != 255
    want = torch.where(keep, labels.long(), torch.full((H, W), n))
    assert torch.equal(augment.remap_label(raw, n), want) and torch.equal(augment.remap_label(ids, n, raw_labels=False), want)
    # the limits of the uint8 output
    big = torch.zeros(H, W, dtype=torch.int16)
    pseudo_label_reference(big, conf, torch.zeros(254, dtype=torch.int32), 254)
    pseudo_label_reference(big, conf, torch.zeros(255, dtype=torch.int32), 255, raw_labels=False)
    for bad_n, raw_labels in ((255, True), (256, False)):
        with pytest.raises(ValueError):
            pseudo_label_reference(big, conf, torch.zeros(bad_n, dtype=torch.int32), bad_n, raw_labels=raw_labels)
    for kw in (dict(boundary=5), dict(boundary=-1), dict(boundary=1.0), dict(thresholds=torch.zeros(n - 1, dtype=torch.int32)),
               dict(thresholds=torch.zeros(n)), dict(conf=conf.double()), dict(labels=labels.float())):
        args = dict(labels=labels, conf=conf, thresholds=thr, n=n)
        args.update(kw)
        with pytest.raises(ValueError):
            pseudo_label_reference(**args)


def test_confidence_histogram_class():
    n = 7
    labels, conf = _case(torch.int16, n)
    hist, tally = confidence_histogram_reference(labels, conf, n)
    h = ConfidenceHistogram(n, hist=hist.clone(), tally=tally.clone())
    h.add_(ConfidenceHistogram(n, hist=hist, tally=tally))
    assert torch.equal(h.hist, 2 * hist) and torch.equal(h.tally, 2 * tally)
    assert torch.equal(h.thresholds(0.5, 0.25), pseudo_thresholds(2 * hist, 0.5, 0.25))
    s = h.summary()
    assert s["pixels"] == 2 * int(tally[0]) and s["outside"] == 2 * int(tally[1]) and len(s["share"]) == n
    assert abs(sum(s["share"]) - 1.0) < 1e-3
    for c in range(n):
        bins = sorted(conf_bin(conf[labels == c]).tolist())
        assert s["median_bin"][c] == (bins[(len(bins) - 1) // 2] if bins else None)
    empty = ConfidenceHistogram(3).summary()
    assert empty["pixels"] == 0 and empty["median_bin"] == [None] * 3
    with pytest.raises(ValueError):
        h.add_(ConfidenceHistogram(n + 1))
    with pytest.raises(ValueError):
        ConfidenceHistogram(n, hist=hist.int())


# ------------------------------------------------------------------------------------------------- surface and refusals
def test_header_declares_the_entry_points():
    with open(os.path.join(ROOT, "include", "ifseg_hip.h")) as f:
        header = f.read()
    assert re.search(r"^int ifseg_seg_conf_hist\(", header, re.M) and re.search(r"^int ifseg_seg_pseudo\(", header, re.M)
    assert re.search(r"#define\s+IFSEG_ABI_VERSION\s+21\b", header) and hip.ABI_VERSION == 21
    assert os.path.exists(os.path.join(ROOT, "ifseg_amd", "csrc", "pseudo.hip"))


def _no_library(monkeypatch):
    def fail():
        raise RuntimeError("the library was reached")
    monkeypatch.setattr(hip, "lib", fail)


def test_bindings_refuse_before_they_launch(monkeypatch):
    _no_library(monkeypatch)
    n = 15
    labels, conf = _case(torch.uint8, n)
    thr = torch.zeros(n, dtype=torch.int32)
    common = [dict(labels=labels.long()), dict(labels=labels.t().contiguous().t()), dict(conf=conf.double()), dict(conf=conf[:, :12]),
              dict(conf=conf[None]), dict(n=0), dict(n=n + 0.0)]
    for kw in common + [dict(n=513), dict(hist=torch.zeros(n, 256, dtype=torch.int32)), dict(hist=torch.zeros(n + 1, 256, dtype=torch.int64)),
                        dict(tally=torch.zeros(3, dtype=torch.int64))]:
        args = dict(labels=labels, conf=conf, n=n)
        args.update(kw)
        with pytest.raises(AssertionError):
            hip.seg_conf_hist(**args)
    for kw in common + [dict(boundary=5), dict(boundary=-1), dict(boundary=1.0), dict(thresholds=thr[:-1]), dict(thresholds=thr.long()),
                        dict(thresholds=thr.float()), dict(kept=torch.zeros(2, n, dtype=torch.int32)), dict(kept=torch.zeros(3, n, dtype=torch.int64)),
                        dict(labels=labels.reshape(-1), conf=conf.reshape(-1)), dict(out=labels), dict(out=torch.zeros(H, W))]:
        args = dict(labels=labels, conf=conf, thresholds=thr, n=n)
        args.update(kw)
        with pytest.raises(AssertionError):
            hip.seg_pseudo(**args)
    wide = torch.zeros(H, W, dtype=torch.int16)
    for bad_n, raw in ((255, True), (256, False)):
        with pytest.raises(AssertionError):
            hip.seg_pseudo(wide, conf, torch.zeros(bad_n, dtype=torch.int32), bad_n, raw_labels=raw)
    # good arguments get as far as the library
    with pytest.raises(RuntimeError, match="the library was reached"):
        hip.seg_conf_hist(labels, conf, n)
    with pytest.raises(RuntimeError, match="the library was reached"):
        hip.seg_pseudo(wide, conf, torch.zeros(255, dtype=torch.int32), 255, 4, False)
    assert hip.seg_pseudo_max_classes(True) == 254 and hip.seg_pseudo_max_classes(False) == 255


def test_ops_are_registered_with_fake_kernels():
    import ifseg_amd.ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    hist_op, pseudo_op = torch.ops.ifseg.seg_conf_hist, torch.ops.ifseg.seg_pseudo
    with FakeTensorMode():
        lab = torch.empty(2, 9, 7, dtype=torch.int16, device="cuda")
        conf = torch.empty(2, 9, 7, device="cuda")
        thr = torch.empty(150, dtype=torch.int32, device="cuda")
        hist, tally = hist_op(lab, conf, 300)
        assert hist.shape == (300, 256) and hist.dtype == torch.int64 and tally.shape == (2,) and tally.dtype == torch.int64 and hist.is_cuda
        out, kept = pseudo_op(lab, conf, thr, 150, 1, True)
        assert out.shape == (2, 9, 7) and out.dtype == torch.uint8 and kept.shape == (2, 150) and kept.dtype == torch.int64 and out.is_cuda
        out, kept = pseudo_op(lab[0].to(torch.uint8), conf[0], thr, 150, 0, False)
        assert out.shape == (9, 7) and out.dtype == torch.uint8
        for bad in (lambda: hist_op(lab.long(), conf, 15), lambda: hist_op(lab, conf[:1], 15), lambda: hist_op(lab, conf, 513),
                    lambda: hist_op(lab, conf.double(), 15), lambda: pseudo_op(lab, conf, thr, 150, 5, True),
                    lambda: pseudo_op(lab, conf, thr, 149, 1, True), lambda: pseudo_op(lab, conf, thr.long(), 150, 1, True),
                    lambda: pseudo_op(lab, conf, torch.empty(255, dtype=torch.int32, device="cuda"), 255, 1, True),
                    lambda: pseudo_op(lab.reshape(-1), conf.reshape(-1), thr, 150, 1, True)):
            with pytest.raises(ValueError):
                bad()
        pseudo_op(lab, conf, torch.empty(255, dtype=torch.int32, device="cuda"), 255, 1, False)


# ------------------------------------------------------------------------------------------------- the Segmenter
N, P, GRID = 5, 64, 16
A, B = (64, 96), (128, 128)
SLIDE = (64, 32)
MS = dict(scales=(0.5, 1.0), flip=True)


class _Model(torch.nn.Linear):
    """as much of a model as the Segmenter looks at outside `patch_scores`"""

    def __init__(self, n=N):
        super().__init__(1, 1)
        self.cfg = type("Cfg", (), {"num_seg_tokens": n, "patch_image_size": P})()


class Recorder:
    """Recording fakes of every binding `pseudo_label_raw` and `segment_raw` may reach.  The front's tensors are not followed
    (tests/test_segmenter_launches_cpu.py does that for `segment_raw`): what is compared is the sequence of launches with
    their shapes and flags, and that the tensors of the two new launches are the ones the merge handed out."""

    def __init__(self, monkeypatch):
        self.log, self.handed = [], []
        for name in ("image_load", "image_load_windows", "seg_predict", "seg_predict_views", "seg_predict_windows",
                     "seg_predict_slide_views", "seg_conf_hist", "seg_pseudo"):
            monkeypatch.setattr(hip, name, getattr(self, name))
        for name in ("lib", "seg_render", "rows_to_f32", "neighbour_smoothing", "seg_score", "seg_score_views", "seg_score_windows",
                     "seg_score_slide_views", "seg_areas", "seg_confusion"):
            monkeypatch.setattr(hip, name, lambda *a, **k: pytest.fail("an unrecorded binding was reached"))
        monkeypatch.setattr(Segmenter, "patch_scores", lambda seg, x: self.forward(x))

    def image_load(self, images, oh, ow, mean, std, reverse_channels):
        self.log.append(("image_load", len(images), tuple(images.shape[1:3]), (oh, ow)))
        return torch.zeros(len(images), 3, oh, ow)

    def image_load_windows(self, images, oh, ow, crop, stride, mean, std, reverse_channels, flip=False):
        from ifseg_amd.imageio import slide_windows
        ys, xs, ch, cw = slide_windows(oh, ow, crop, stride)
        self.log.append(("image_load_windows", len(images), tuple(images.shape[1:3]), (oh, ow), (crop, stride), flip))
        return torch.zeros(len(images) * len(ys) * len(xs), 3, ch, cw)

    def forward(self, x):
        self.log.append(("forward", tuple(x.shape)))
        hp, wp = -(-x.shape[2] // GRID), -(-x.shape[3] // GRID)
        return torch.zeros(x.shape[0], hp * wp, N), hp, wp

    def _out(self, name, h, w, conf, probs, label_dtype, **flags):
        assert label_dtype is None
        self.log.append((name, (1, h, w), dict(conf=conf, probs=probs, **flags)))
        labels = torch.full((1, h, w), len(self.handed) % N, dtype=torch.uint8)
        self.handed.append((labels, torch.full((1, h, w), 0.5) if conf else None))
        return labels, self.handed[-1][1], torch.zeros(1, N, h, w) if probs else None

    def seg_predict(self, scores, hp, wp, h, w, conf=False, probs=False, label_dtype=None):
        return self._out("seg_predict", h, w, conf, probs, label_dtype)

    def seg_predict_views(self, views, h, w, conf=False, probs=False, label_dtype=None):
        return self._out("seg_predict_views", h, w, conf, probs, label_dtype)

    def seg_predict_windows(self, scores, hpw, wpw, oh, ow, crop, stride, h, w, conf=False, probs=False, label_dtype=None):
        return self._out("seg_predict_windows", h, w, conf, probs, label_dtype)

    def seg_predict_slide_views(self, views, crop, stride, h, w, softmax, conf=False, probs=False, label_dtype=None):
        return self._out("seg_predict_slide_views", h, w, conf, probs, label_dtype, softmax=softmax)

    def _image_of(self, labels, conf):
        """which image's merge handed out these two tensors (by storage)"""
        for i, (l, c) in enumerate(self.handed):
            if l.data_ptr() == labels.data_ptr() and c is not None and c.data_ptr() == conf.data_ptr():
                return i
        pytest.fail("a launch was given tensors that no merge handed out")

    def seg_conf_hist(self, labels, conf, n, hist=None, tally=None):
        assert n == N and labels.is_contiguous() and conf.is_contiguous() and hist is not None and tally is not None
        assert tuple(hist.shape) == (N, 256) and tuple(tally.shape) == (2,)
        self.log.append(("seg_conf_hist", self._image_of(labels, conf), tuple(labels.shape)))
        hist[int(labels.reshape(-1)[0]), 128] += labels.numel()
        tally[0] += labels.numel()
        return hist, tally

    def seg_pseudo(self, labels, conf, thresholds, n, boundary=0, raw_labels=True, kept=None, out=None):
        assert n == N and labels.is_contiguous() and conf.is_contiguous() and kept is None and out is None
        assert thresholds.dtype == torch.int32 and tuple(thresholds.shape) == (N,)
        self.log.append(("seg_pseudo", self._image_of(labels, conf), tuple(labels.shape), thresholds.tolist(), boundary, raw_labels))
        return torch.full(labels.shape, 255, dtype=torch.uint8), torch.zeros(2, N, dtype=torch.int64)


def _images():
    return [torch.full(hw + (3,), i, dtype=torch.uint8) for i, hw in enumerate((A, B))]


SETTINGS = {  # name: (Segmenter arguments, call arguments, the predict kernel, its extra flags)
    "single": ({}, {}, "seg_predict", {}),
    "msflip": ({}, MS, "seg_predict_views", {}),
    "slide": ({}, dict(slide=SLIDE), "seg_predict_windows", {}),
    "slide_views_logits": (dict(slide_views=True, upsample="logits"), dict(slide=SLIDE, **MS), "seg_predict_slide_views", dict(softmax=True)),
}


@pytest.mark.parametrize("given", [False, True], ids=["hist", "thresholds"])
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_launch_sequence(monkeypatch, setting, given):
    ctor, call, kernel, flags = SETTINGS[setting]
    # what segment_raw(return_conf=True) launches in this setting, recorded from segment_raw itself
    rec0 = Recorder(monkeypatch)
    Segmenter(_Model(), category_token_ids=[[1]] * N, **ctor).segment_raw(_images(), max_batch=3, return_conf=True, **call)
    front = rec0.log
    assert [e[0] for e in front[-2:]] == [kernel, kernel] and front[-1][2] == dict(conf=True, probs=False, **flags)
    assert front[-2][1] == (1,) + A and front[-1][1] == (1,) + B

    rec = Recorder(monkeypatch)
    seg = Segmenter(_Model(), category_token_ids=[[1]] * N, **ctor)
    hist = ConfidenceHistogram(N)
    thr = torch.tensor([0, 256, 3, 77, 128], dtype=torch.int32)
    kw = dict(thresholds=thr) if given else dict(hist=hist, keep=0.5, floor=0.25)
    out = seg.pseudo_label_raw(_images(), boundary=2, max_batch=3, **kw, **call)
    assert len(out) == 2 and all(isinstance(r, PseudoLabelResult) for r in out)
    assert [tuple(r.labels.shape) for r in out] == [A, B] and all(r.labels.dtype == torch.uint8 for r in out)
    assert [tuple(r.predicted.shape) for r in out] == [A, B] and [tuple(r.conf.shape) for r in out] == [A, B]
    assert all(tuple(r.kept.shape) == (2, N) for r in out)
    # the front and the merges are segment_raw's, then one histogram launch per image, then one filter launch per image
    assert rec.log[:len(front)] == front
    rest = rec.log[len(front):]
    if given:
        want_thr = thr.tolist()
        assert not hist.hist.any()
        want = []
    else:
        # the fake histogram put image 0 (label 0) and image 1 (label 1) into bin 128: keep = 0.5 rejects the tied bin
        want_thr = [129, 129, 64, 64, 64]
        assert int(hist.tally[0]) == A[0] * A[1] + B[0] * B[1]
        want = [("seg_conf_hist", 0, A), ("seg_conf_hist", 1, B)]
    want += [("seg_pseudo", 0, A, want_thr, 2, True), ("seg_pseudo", 1, B, want_thr, 2, True)]
    assert rest == want


def test_segmenter_refuses_before_anything_is_launched(monkeypatch):
    rec = Recorder(monkeypatch)
    names = [[1]] * N
    imgs = _images()
    # raw logits are no probability: the setting is named
    for ctor, call in ((dict(upsample="logits"), {}), (dict(upsample="logits"), dict(slide=SLIDE)),
                       (dict(upsample="logits", slide_views=True), {})):
        with pytest.raises(ValueError, match="upsample='logits'"):
            Segmenter(_Model(), category_token_ids=names, **ctor).pseudo_label_raw(imgs, **call)
    # ... and these hand over probabilities (every fake returns, so the call runs through)
    monkeypatch.setattr(hip, "neighbour_smoothing", lambda *a, **k: None)
    for ctor, call in ((dict(upsample="probs"), {}), (dict(upsample="logits", smooth_iters=2), {}),
                       (dict(upsample="logits", slide_views=True), dict(slide=SLIDE))):
        del rec.log[:]
        assert len(Segmenter(_Model(), category_token_ids=names, **ctor).pseudo_label_raw(imgs, **call)) == 2
    del rec.log[:]
    # too many classes for the uint8 map
    for n, raw in ((255, True), (256, False), (300, True)):
        with pytest.raises(ValueError, match="at most"):
            Segmenter(_Model(n), category_token_ids=[[1]] * n).pseudo_label_raw(imgs, raw_labels=raw)
    seg = Segmenter(_Model(), category_token_ids=names)
    for kw in (dict(keep=1.5), dict(keep=-0.1), dict(floor=2.0), dict(boundary=5), dict(boundary=0.5), dict(hist=ConfidenceHistogram(N + 1)),
               dict(hist=torch.zeros(N, 256, dtype=torch.int64)), dict(thresholds=torch.zeros(N, dtype=torch.int64)),
               dict(thresholds=torch.zeros(N + 1, dtype=torch.int32)), dict(thresholds=[0] * N), dict(scales=(0.5, 1.0), slide=SLIDE)):
        with pytest.raises(ValueError):
            seg.pseudo_label_raw(imgs, **kw)
    assert rec.log == []
    assert seg.pseudo_label_raw([]) == []


def test_task_methods(monkeypatch):
    """`SegmentationTask.pseudo_label_raw` splits constructor keywords as `evaluate_raw` does; `self_train_sample` is
    `pseudo_label_raw` followed by `train_sample` on the pseudo-labels and checks raw_labels against the transform's"""
    from ifseg_amd.tasks.mm_tasks import SegmentationTask
    rec = Recorder(monkeypatch)
    task = SegmentationTask(num_seg_tokens=N, patch_image_size=P, n_base_vocab=100, category_token_ids=[[5]] * N)
    imgs = _images()
    out = task.pseudo_label_raw(_Model(), imgs, upsample="logits", smooth_iters=0, slide_views=True, slide=SLIDE, keep=0.5, max_batch=3)
    assert len(out) == 2 and rec.log[-1][:3] == ("seg_pseudo", 1, B)
    with pytest.raises(ValueError, match="upsample='logits'"):
        task.pseudo_label_raw(_Model(), imgs, upsample="logits")

    task.build_train_transform("cpu", seed=3)
    seen = {}

    def train_sample(images, labels, first_ordinal):
        seen.update(images=images, labels=labels, first_ordinal=first_ordinal)
        return "batch"
    monkeypatch.setattr(task, "train_sample", train_sample)
    assert task.self_train_sample(_Model(), imgs, 7, keep=0.5, boundary=1) == "batch"
    assert seen["first_ordinal"] == 7 and [tuple(l.shape) for l in seen["labels"]] == [A, B] and len(seen["images"]) == 2
    assert all(l.dtype == torch.uint8 and (l == 255).all() for l in seen["labels"])
    assert rec.log[-1][5] is True                                 # raw_labels followed the transform's
    with pytest.raises(ValueError, match="raw_labels"):
        task.self_train_sample(_Model(), imgs, 7, raw_labels=False)
    task.build_train_transform("cpu", seed=3, raw_labels=False)
    task.self_train_sample(_Model(), imgs, 7)
    assert rec.log[-1][5] is False
