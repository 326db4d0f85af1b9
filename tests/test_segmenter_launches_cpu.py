"""CPU: which launches a Segmenter makes, in which order and with which flags, in every setting of `segment_raw`,
`evaluate_raw`, `__call__` and `evaluate` (ifseg_amd/predict.py).  The model forward and every `hip` binding the Segmenter
calls are replaced by recording fakes that return tensors of the right shape and dtype; the expected sequences below are
written out from the docstrings of predict.py and imageio.py, not produced by the code under test.

The two images: A is 64 x 96 and B is 128 x 128.  With P = 64, `eval_size` puts A at (64, 96) and B at (64, 64) at ratio 1,
and A at (32, 48) and B at (32, 32) at ratio 0.5.  slide=(64, 32) cuts (64, 96) into two 64 x 64 windows and (64, 64) into
one; an image smaller than the crop is one window of its own size.  max_batch is 3."""
import pytest
import torch

from ifseg_amd import hip
from ifseg_amd.predict import Segmenter, SegmentationScore

N, P, GRID = 5, 64, 16
A, B = (64, 96), (128, 128)
SLIDE = (64, 32)
MS = dict(scales=(0.5, 1.0), flip=True)


class _Model(torch.nn.Linear):
    """as much of a model as the Segmenter looks at outside `patch_scores`"""

    def __init__(self):
        super().__init__(1, 1)
        self.cfg = type("Cfg", (), {"num_seg_tokens": N, "patch_image_size": P})()


class Recorder:
    """Every tensor the fakes hand out carries a serial number (value = serial * 1024 + column), so the next fake can say
    what it was given, and whether it was mirrored on the way."""

    def __init__(self, monkeypatch):
        self.log, self.tags = [], []
        for name in ("image_load", "image_load_windows", "seg_predict", "seg_predict_views", "seg_predict_windows",
                     "seg_predict_slide_views", "seg_score", "seg_score_views", "seg_score_windows", "seg_score_slide_views",
                     "seg_areas", "seg_confusion"):
            monkeypatch.setattr(hip, name, getattr(self, name))
        for name in ("lib", "seg_render", "rows_to_f32", "neighbour_smoothing"):
            monkeypatch.setattr(hip, name, lambda *a, **k: pytest.fail("an unrecorded binding was reached"))
        import ifseg_amd.crf
        monkeypatch.setattr(ifseg_amd.crf, "rgb_dense_crf", self.crf)
        monkeypatch.setattr(Segmenter, "patch_scores", lambda seg, x: self.forward(x))

    def coded(self, tag, *shape):
        self.tags.append(tag)
        return ((len(self.tags) - 1) * 1024 + torch.arange(shape[-1], dtype=torch.float32)).expand(*shape).contiguous()

    def tag(self, t):
        """-> (the tag of a coded tensor of any shape, whether its columns were reversed)"""
        row = t.reshape(-1, t.shape[-1])[0]
        return self.tags[int(row.min()) // 1024], bool(row[0] > row[-1])

    # ---- the front
    def image_load(self, images, oh, ow, mean, std, reverse_channels):
        ids = [int(im[0, 0, 0]) for im in images]
        self.log.append(("image_load", ids, tuple(images.shape[1:3]), (oh, ow)))
        return torch.stack([self.coded((i, (oh, ow)), 3, oh, ow) for i in ids])

    def image_load_windows(self, images, oh, ow, crop, stride, mean, std, reverse_channels, flip=False):
        from ifseg_amd.imageio import slide_windows
        ys, xs, ch, cw = slide_windows(oh, ow, crop, stride)
        ids = [int(im[0, 0, 0]) for im in images]
        self.log.append(("image_load_windows", ids, tuple(images.shape[1:3]), (oh, ow), (crop, stride), flip))
        return torch.stack([self.coded((i, (oh, ow), flip, k), 3, ch, cw) for i in ids for k in range(len(ys) * len(xs))])

    def forward(self, x):
        items = []
        for one in x:
            tag, mirrored = self.tag(one)
            assert len(tag) == 2 or not mirrored
            items.append(tag + (mirrored,) if len(tag) == 2 else tag)
        self.log.append(("forward", items))
        hp, wp = -(-x.shape[2] // GRID), -(-x.shape[3] // GRID)
        return torch.stack([self.coded(item, hp * wp, N) for item in items]), hp, wp

    # ---- the last launches
    def _out(self, name, what, B, h, w, conf, probs, label_dtype, gt=None, labels=True, areas=None, tally=None, raw_labels=None,
             softmax=None):
        assert label_dtype is None
        flags = dict(conf=conf, probs=probs)
        if gt is not None:
            assert tuple(gt.shape) == (B, h, w) and gt.dtype == torch.uint8
            flags.update(labels=labels, counters=areas is not None and tally is not None, raw_labels=raw_labels)
        if softmax is not None:
            flags["softmax"] = softmax
        self.log.append((name, what, (B, h, w), flags))
        out = (torch.zeros(B, h, w, dtype=torch.uint8) if labels else None, torch.zeros(B, h, w) if conf else None,
               torch.zeros(B, N, h, w) if probs else None)
        return out if gt is None else (areas, tally) + out

    def _views(self, views):
        """-> per view (what the forward saw, hp, wp, flip)"""
        return [(self.tag(s)[0],) + tuple(rest) for s, *rest in views]

    def _windows(self, scores, *rest):
        """-> (what the forward saw per window, hpw, wpw, ...)"""
        assert scores.dim() == 4 and scores.shape[0] == 1
        return ([self.tag(s)[0] for s in scores[0]],) + tuple(rest)

    def seg_predict(self, scores, hp, wp, h, w, conf=False, probs=False, label_dtype=None):
        return self._out("seg_predict", ([self.tag(s)[0] for s in scores], hp, wp), len(scores), h, w, conf, probs, label_dtype)

    def seg_score(self, scores, hp, wp, gt, label_dtype=None, **kw):
        kw = {"conf": False, "probs": False, **kw}
        return self._out("seg_score", ([self.tag(s)[0] for s in scores], hp, wp), *gt.shape, label_dtype=label_dtype, gt=gt, **kw)

    def seg_predict_views(self, views, h, w, conf=False, probs=False, label_dtype=None):
        return self._out("seg_predict_views", self._views(views), 1, h, w, conf, probs, label_dtype)

    def seg_score_views(self, views, gt, label_dtype=None, **kw):
        kw = {"conf": False, "probs": False, **kw}
        return self._out("seg_score_views", self._views(views), *gt.shape, label_dtype=label_dtype, gt=gt, **kw)

    def seg_predict_windows(self, scores, hpw, wpw, oh, ow, crop, stride, h, w, conf=False, probs=False, label_dtype=None):
        return self._out("seg_predict_windows", self._windows(scores, hpw, wpw, oh, ow, crop, stride), 1, h, w, conf, probs, label_dtype)

    def seg_score_windows(self, scores, hpw, wpw, oh, ow, crop, stride, gt, label_dtype=None, **kw):
        kw = {"conf": False, "probs": False, **kw}
        return self._out("seg_score_windows", self._windows(scores, hpw, wpw, oh, ow, crop, stride), *gt.shape,
                         label_dtype=label_dtype, gt=gt, **kw)

    def seg_predict_slide_views(self, views, crop, stride, h, w, softmax, conf=False, probs=False, label_dtype=None):
        return self._out("seg_predict_slide_views", ([self._windows(*v) for v in views], crop, stride), 1, h, w, conf, probs,
                         label_dtype, softmax=softmax)

    def seg_score_slide_views(self, views, crop, stride, gt, softmax, label_dtype=None, **kw):
        kw = {"conf": False, "probs": False, **kw}
        return self._out("seg_score_slide_views", ([self._windows(*v) for v in views], crop, stride), *gt.shape,
                         label_dtype=label_dtype, gt=gt, softmax=softmax, **kw)

    def seg_areas(self, labels, gt, n, raw_labels=True, areas=None, tally=None):
        assert labels.is_contiguous() and labels.shape == gt.shape and n == N
        self.log.append(("seg_areas", tuple(labels.shape), dict(counters=areas is not None and tally is not None, raw_labels=raw_labels)))
        return areas, tally

    def seg_confusion(self, labels, gt, n, raw_labels=True, confusion=None):
        assert labels.is_contiguous() and labels.shape == gt.shape and n == N
        self.log.append(("seg_confusion", tuple(labels.shape), dict(matrix=confusion is not None, raw_labels=raw_labels)))
        return confusion

    def crf(self, rgb, probs, iters):
        self.log.append(("crf", float(rgb[0, 0, 0]), tuple(rgb.shape), tuple(probs.shape), iters))
        return probs


# ------------------------------------------------------------------------------------------------- the expected sequences
def _images():
    """image i is filled with the value i, which the fake loads and the fake CRF read back"""
    imgs = [torch.full(hw + (3,), i, dtype=torch.uint8) for i, hw in enumerate((A, B))]
    return imgs, [torch.ones(hw, dtype=torch.uint8) for hw in (A, B)]


def _g(size):
    """the patch grid of a network input"""
    return -(-size[0] // GRID), -(-size[1] // GRID)


def _front(setting):
    """-> (the loads and forwards of a setting, per image the `what` of its last launch).  Views of a setting are, per ratio,
    the unflipped and then the flipped one; forwards take the views (windows) of one size in (image, view, window) order, three
    at a time, the sizes in order of first appearance."""
    if setting == "single":
        return ([("image_load", [0], A, (64, 96)), ("image_load", [1], B, (64, 64)),
                 ("forward", [(0, (64, 96), False)]), ("forward", [(1, (64, 64), False)])],
                [([(0, (64, 96), False)], 4, 6), ([(1, (64, 64), False)], 4, 4)])
    if setting == "msflip":
        return ([("image_load", [0], A, (32, 48)), ("image_load", [0], A, (64, 96)),
                 ("image_load", [1], B, (32, 32)), ("image_load", [1], B, (64, 64)),
                 ("forward", [(0, (32, 48), False), (0, (32, 48), True)]), ("forward", [(0, (64, 96), False), (0, (64, 96), True)]),
                 ("forward", [(1, (32, 32), False), (1, (32, 32), True)]), ("forward", [(1, (64, 64), False), (1, (64, 64), True)])],
                [[((0, (32, 48), False), 2, 3, False), ((0, (32, 48), True), 2, 3, True),
                  ((0, (64, 96), False), 4, 6, False), ((0, (64, 96), True), 4, 6, True)],
                 [((1, (32, 32), False), 2, 2, False), ((1, (32, 32), True), 2, 2, True),
                  ((1, (64, 64), False), 4, 4, False), ((1, (64, 64), True), 4, 4, True)]])
    if setting == "slide":
        a0, a1, b0 = (0, (64, 96), False, 0), (0, (64, 96), False, 1), (1, (64, 64), False, 0)
        return ([("image_load_windows", [0], A, (64, 96), SLIDE, False), ("image_load_windows", [1], B, (64, 64), SLIDE, False),
                 ("forward", [a0, a1, b0])],
                [([a0, a1], 4, 4, 64, 96) + SLIDE, ([b0], 4, 4, 64, 64) + SLIDE])
    assert setting == "slide_views"
    w = lambda i, size, flip, count: [(i, size, flip, k) for k in range(count)]
    loads = [("image_load_windows", [i], hw, size, SLIDE, flip)
             for i, hw, sizes in ((0, A, ((32, 48), (64, 96))), (1, B, ((32, 32), (64, 64)))) for size in sizes for flip in (False, True)]
    a_small, a_full = w(0, (32, 48), False, 1) + w(0, (32, 48), True, 1), w(0, (64, 96), False, 2) + w(0, (64, 96), True, 2)
    b_small, b_full = w(1, (32, 32), False, 1) + w(1, (32, 32), True, 1), w(1, (64, 64), False, 1) + w(1, (64, 64), True, 1)
    big = a_full + b_full                                     # the 64 x 64 windows of both images share their forwards
    forwards = [("forward", a_small), ("forward", big[:3]), ("forward", big[3:]), ("forward", b_small)]
    per_image = [([(a_small[:1], 2, 3, 32, 48, False), (a_small[1:], 2, 3, 32, 48, True),
                   (a_full[:2], 4, 4, 64, 96, False), (a_full[2:], 4, 4, 64, 96, True)],) + SLIDE,
                 ([(b_small[:1], 2, 2, 32, 32, False), (b_small[1:], 2, 2, 32, 32, True),
                   (b_full[:1], 4, 4, 64, 64, False), (b_full[1:], 4, 4, 64, 64, True)],) + SLIDE]
    return loads + forwards, per_image


SETTINGS = {  # name: (front, Segmenter arguments, call arguments, the kernel's name after seg_predict / seg_score, softmax flag)
    "single": ("single", {}, {}, "", None),
    "msflip": ("msflip", {}, MS, "_views", None),
    "slide": ("slide", {}, dict(slide=SLIDE), "_windows", None),
    "slide_views_probs": ("slide_views", dict(slide_views=True), dict(slide=SLIDE, **MS), "_slide_views", False),
    "slide_views_logits": ("slide_views", dict(slide_views=True, upsample="logits"), dict(slide=SLIDE, **MS), "_slide_views", True),
}


def _expected(setting, crf, method):
    front, _, _, kernel, softmax = SETTINGS[setting]
    log, whats = _front(front)
    sm = {} if softmax is None else {"softmax": softmax}
    for i, (what, hw) in enumerate(zip(whats, (A, B))):
        shape = (1,) + hw
        if method == "segment_raw":                           # called with return_conf=True
            if crf:     # the CRF takes every class's value and gives the labels and the winning value itself
                log += [("seg_predict" + kernel, what, shape, dict(conf=False, probs=True, **sm)), ("crf", float(i), hw + (3,), (N,) + hw, 2)]
            else:
                log += [("seg_predict" + kernel, what, shape, dict(conf=True, probs=False, **sm))]
            continue
        pairs = method == "evaluate_raw_confusion"
        if crf:         # the CRF's argmax is counted by seg_areas
            log += [("seg_predict" + kernel, what, shape, dict(conf=False, probs=True, **sm)), ("crf", float(i), hw + (3,), (N,) + hw, 2),
                    ("seg_areas", shape, dict(counters=True, raw_labels=True))]
        else:           # the scoring launch writes nothing but counters, unless the matrix needs its label map
            log += [("seg_score" + kernel, what, shape, dict(conf=False, probs=False, labels=pairs, counters=True, raw_labels=True, **sm))]
        if pairs:
            log += [("seg_confusion", shape, dict(matrix=True, raw_labels=True))]
    return log


@pytest.mark.parametrize("method", ["segment_raw", "evaluate_raw", "evaluate_raw_confusion"])
@pytest.mark.parametrize("crf", [False, True], ids=["plain", "crf"])
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_raw_launch_sequence(monkeypatch, setting, crf, method):
    rec = Recorder(monkeypatch)
    seg = Segmenter(_Model(), category_token_ids=[[1]] * N, crf_iters=2 if crf else 0, **SETTINGS[setting][1])
    imgs, gts = _images()
    if method == "segment_raw":
        out = seg.segment_raw(imgs, max_batch=3, return_conf=True, **SETTINGS[setting][2])
        assert [tuple(r.labels.shape) for r in out] == [A, B] and all(r.conf is not None and r.probs is None for r in out)
    else:
        score = seg.evaluate_raw(imgs, gts, max_batch=3, confusion=method.endswith("confusion"), **SETTINGS[setting][2])
        assert isinstance(score, SegmentationScore) and (score.confusion is not None) == method.endswith("confusion")
    want = _expected(setting, crf, method)
    assert len(rec.log) == len(want), [e[0] for e in rec.log]
    for k, (got, exp) in enumerate(zip(rec.log, want)):
        assert got == exp, (k, got, exp)


@pytest.mark.parametrize("crf", [False, True], ids=["plain", "crf"])
def test_call_and_evaluate_launch_sequence(monkeypatch, crf):
    """`__call__` and `evaluate` take a ready batch: one forward, then seg_predict / seg_score for the whole batch (per image
    with a list of output sizes)"""
    rec = Recorder(monkeypatch)
    seg = Segmenter(_Model(), category_token_ids=[[1]] * N, crf_iters=2 if crf else 0)
    x = torch.stack([rec.coded(("x", b), 3, 32, 48) for b in range(2)])
    items = [("x", 0, False), ("x", 1, False)]
    grey = [float((x[b, 0, 0, 0] * 0.5 + 0.5) * 255.0) for b in range(2)]       # the CRF image of a normalised input
    crf_events = [("crf", grey[b], (32, 48, 3), (N, 32, 48), 2) for b in range(2)]
    gt = torch.ones(2, 32, 48, dtype=torch.uint8)

    res = seg(x, return_probs=True)
    assert tuple(res.labels.shape) == (2, 32, 48) and res.conf is None and res.probs is not None
    want = [("forward", items), ("seg_predict", (items, 2, 3), (2, 32, 48), dict(conf=False, probs=True))] + (crf_events if crf else [])
    assert rec.log == want

    del rec.log[:]
    sizes = [(32, 48), (32, 48)] if crf else [(40, 50), (7, 9)]
    res = seg(x, out_hw=sizes, return_conf=True)
    assert [tuple(r.labels.shape) for r in res] == [(1,) + s for s in sizes]
    want = [("forward", items)]
    for b, s in enumerate(sizes):
        want += [("seg_predict", (items[b:b + 1], 2, 3), (1,) + s, dict(conf=not crf, probs=crf))] + crf_events[b:b + 1] * crf
    assert rec.log == want

    for pairs in (False, True):
        del rec.log[:]
        seg.evaluate(x, gt, confusion=pairs)
        if crf:
            want = [("forward", items), ("seg_predict", (items, 2, 3), (2, 32, 48), dict(conf=False, probs=True))] + crf_events \
                + [("seg_areas", (2, 32, 48), dict(counters=True, raw_labels=True))]
        else:
            want = [("forward", items), ("seg_score", (items, 2, 3), (2, 32, 48),
                                         dict(conf=False, probs=False, labels=pairs, counters=True, raw_labels=True))]
        assert rec.log == want + [("seg_confusion", (2, 32, 48), dict(matrix=True, raw_labels=True))] * pairs
