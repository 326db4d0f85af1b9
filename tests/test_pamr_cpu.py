"""CPU: pixel-adaptive mask refinement (ifseg_amd/predict.py pamr_reference, Segmenter(pamr_iters=), csrc/pamr.hip).  The
closed form against a literal transcription of the published module, the properties of the rule, the 1 % cap of the margin
rule for every case of tests/_pamr_cases.py, the ValueErrors of the Segmenter, the task's keyword tuples, the header, and the
launches a Segmenter with PAMR makes -- written out by hand from the docstrings of predict.py, with recording fakes in the
manner of test_segmenter_launches_cpu.py."""
import inspect
import os
import re

import pytest
import torch

import _pamr_cases as C
from ifseg_amd import hip
from ifseg_amd.predict import (PAMR_DILATIONS, Segmenter, SegmentationScore, pamr_affinity_reference, pamr_iterate_reference,
                               pamr_reference)

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


# ------------------------------------------------------------------------------------------------- the specification
@pytest.mark.parametrize("name", ["tiny", "one_tile", "ten_iters", "one_wide_ring", "odd"])
def test_closed_form_is_the_published_module(name):
    """`pamr_reference` in fp64 equals the transcription of the upstream module fed the same grey levels (upstream feeds the
    normalised image: the ratio is scale-free per channel, only the 1e-8 differs)"""
    c = C.case(name)
    x = c.image.permute(2, 0, 1)[None].double()
    mask, a = C.upstream_pamr(x, c.values[None].double(), c.dilations, c.iters)
    assert (a[0, 0] - c.w64).abs().max().item() <= 1e-13
    assert (mask[0] - c.probs).abs().max().item() <= 1e-13


def test_values_stay_probabilities_and_weights_are_convex():
    for name in ("tiny", "ten_iters", "blocks"):
        c = C.case(name)
        assert (c.w64 >= 0).all() and (c.w64.sum(0) - 1).abs().max().item() <= 1e-14
        assert (c.probs.sum(0) - 1).abs().max().item() <= 1e-6         # the fp32 inputs sum to 1 within their own rounding
        assert c.probs.min().item() >= c.values.min().item() - 1e-12 and c.probs.max().item() <= c.values.max().item() + 1e-12
        assert torch.equal(c.labels, c.probs.argmax(0)) and torch.equal(c.conf, c.probs.amax(0))


def test_flat_image_gives_equal_weights():
    img = torch.full((9, 11, 3), 77, dtype=torch.uint8)
    for dt in (torch.float64, torch.float32):
        w = pamr_affinity_reference(img, (1, 3), dt)
        assert w.shape == (16, 9, 11) and torch.equal(w, torch.full_like(w, 1.0 / 16))
    m = torch.rand(3, 9, 11, dtype=torch.float64)
    # equal weights: the mean of the 16 clamped neighbours; a constant plane is a fixed point
    assert torch.allclose(pamr_iterate_reference(w.double(), torch.ones(3, 9, 11), (1, 3)), torch.ones(3, 9, 11, dtype=torch.float64))
    labels, conf, out = pamr_reference(img, m, (1, 3), 1)
    assert out.shape == m.shape and torch.equal(labels, out.argmax(0))


def test_all_classes_equal_gives_label_zero():
    c = C.case("tiny")
    labels, conf, out = pamr_reference(c.image, torch.full((4, c.H, c.W), 0.25), c.dilations, 2)
    assert int(labels.abs().max()) == 0


@pytest.mark.parametrize("name", list(C.CASES))
def test_margin_cap_holds(name):
    """the GPU test leaves out the pixels whose top-2 margin is below 32 e: at most 1 % of every case"""
    c = C.case(name)
    print("%s: e_w = %.3g, e_iter = %.3g, e = %.3g, undecided = %.4f" % (name, c.e_w, c.e_iter, c.e, c.undecided_share))
    assert c.undecided_share <= C.MARGIN_CAP, (name, c.undecided_share)
    assert c.e_w < 1e-5 and c.e_iter < 1e-5 and c.e < 1e-5            # the fp32 specification is a usable yardstick


# ------------------------------------------------------------------------------------------------- the surface
N, P, GRID = 5, 64, 16
A, B = (64, 96), (128, 128)


class _Model(torch.nn.Linear):
    def __init__(self):
        super().__init__(1, 1)
        self.cfg = type("Cfg", (), {"num_seg_tokens": N, "patch_image_size": P})()


def _seg(**kw):
    return Segmenter(_Model(), category_token_ids=[[1]] * N, **kw)


@pytest.mark.parametrize("kw, word", [
    (dict(pamr_iters=2, crf_iters=1), "crf_iters"),
    (dict(pamr_iters=-1), "pamr_iters"), (dict(pamr_iters=1.5), "pamr_iters"), (dict(pamr_iters=True), "pamr_iters"),
    (dict(pamr_iters=2, pamr_dilations=()), "pamr_dilations"), (dict(pamr_iters=2, pamr_dilations=(1,) * 9), "pamr_dilations"),
    (dict(pamr_iters=2, pamr_dilations=(0,)), "pamr_dilations"), (dict(pamr_iters=2, pamr_dilations=(33,)), "pamr_dilations"),
    (dict(pamr_iters=2, pamr_dilations=(1, 2.0)), "pamr_dilations"), (dict(pamr_iters=2, pamr_dilations=3), "pamr_dilations"),
    (dict(pamr_dilations=(64,)), "pamr_dilations"),
])
def test_constructor_refusals(kw, word):
    with pytest.raises(ValueError, match=word):
        _seg(**kw)


def test_defaults_and_limits():
    seg = _seg()
    assert seg.pamr_iters == 0 and seg.pamr_dilations == (1, 2, 4, 8, 12, 24) == PAMR_DILATIONS == hip.SEG_PAMR_DILATIONS
    assert hip.SEG_PAMR_MAX_DILATION == 32 and hip.SEG_PAMR_MAX_DILATIONS == 8
    assert _seg(pamr_iters=3, pamr_dilations=[1, 32]).pamr_dilations == (1, 32)
    sig = inspect.signature(hip.seg_pamr).parameters
    assert list(sig) == ["probs", "image", "iters", "dilations", "conf", "probs_out", "label_dtype"]
    assert sig["iters"].default == 10 and sig["dilations"].default == (1, 2, 4, 8, 12, 24)
    assert list(inspect.signature(hip.pamr_iterate).parameters) == ["w", "src", "dst", "dilations", "labels", "conf"]
    assert list(inspect.signature(hip.pamr_affinity).parameters) == ["image", "dilations"]


def test_calibrate_raw_refuses_pamr(monkeypatch):
    monkeypatch.setattr(hip, "lib", lambda *a, **k: pytest.fail("a launch was reached"))
    seg = _seg(pamr_iters=2)
    with pytest.raises(ValueError, match="pamr_iters"):
        seg.calibrate_raw([torch.zeros(A + (3,), dtype=torch.uint8)], [torch.ones(A, dtype=torch.uint8)])
    with pytest.raises(ValueError, match="pamr_iters"):
        seg.calibrate(torch.zeros(1, 3, 64, 64), torch.ones(1, 64, 64, dtype=torch.uint8))


def test_out_hw_needs_crf_images_with_pamr():
    seg = _seg(pamr_iters=2)
    with pytest.raises(ValueError, match="crf_images"):
        seg(torch.zeros(1, 3, 64, 64), out_hw=(32, 32))


def test_task_tuples_carry_the_keywords():
    from ifseg_amd.tasks.mm_tasks import segmentation
    src = inspect.getsource(segmentation)
    tuples = re.findall(r"ctor = \(([^)]*)\)", src)
    assert len(tuples) == 4
    for t in tuples:
        assert '"pamr_iters"' in t and '"pamr_dilations"' in t and '"crf_iters"' in t, t


def test_header_declares_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "ifseg_hip.h")).read()
    for name in ("ifseg_pamr_affinity", "ifseg_pamr_iterate", "ifseg_pamr_limit"):
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
    assert int(re.search(r"#define IFSEG_ABI_VERSION (\d+)", hdr).group(1)) == 21 == hip.ABI_VERSION


def test_op_is_registered_with_a_fake_kernel():
    import ifseg_amd.ops  # noqa: F401
    probs, image = torch.empty(260, 9, 11, device="meta"), torch.empty(9, 11, 3, device="meta", dtype=torch.uint8)
    labels, conf, out = torch.ops.ifseg.seg_pamr(probs, image, 3, [1, 2], True, False)
    assert labels.shape == (9, 11) and labels.dtype == torch.int16 and conf.shape == (9, 11) and out.numel() == 0
    labels, conf, out = torch.ops.ifseg.seg_pamr(probs[:5], image, 1, [1], False, True)
    assert labels.dtype == torch.uint8 and conf.numel() == 0 and out.shape == (5, 9, 11)
    for bad in ((probs, image, 0, [1]), (probs, image, 1, []), (probs, image, 1, [33]), (probs, image[:8], 1, [1])):
        with pytest.raises(ValueError):
            torch.ops.ifseg.seg_pamr(*bad, False, False)


# ------------------------------------------------------------------------------------------------- the launches
class Recorder:
    """recording fakes of the forward and of every binding a Segmenter with PAMR may reach; anything else fails the test"""

    def __init__(self, monkeypatch):
        self.log = []
        for name in ("image_load", "seg_predict", "seg_score", "seg_pamr", "seg_areas", "seg_confusion", "seg_calibration", "seg_render"):
            monkeypatch.setattr(hip, name, getattr(self, name))
        for name in ("lib", "rows_to_f32", "neighbour_smoothing", "pamr_affinity", "pamr_iterate", "seg_predict_views",
                     "seg_score_views", "seg_boundary_areas"):
            monkeypatch.setattr(hip, name, lambda *a, **k: pytest.fail("an unrecorded binding was reached"))
        monkeypatch.setattr(Segmenter, "patch_scores", lambda seg, x: self.forward(x))

    def image_load(self, images, oh, ow, mean, std, reverse_channels):
        self.log.append(("image_load", [int(im[0, 0, 0]) for im in images], (oh, ow)))
        return torch.zeros(len(images), 3, oh, ow)

    def forward(self, x):
        self.log.append(("forward", tuple(x.shape)))
        hp, wp = -(-x.shape[2] // GRID), -(-x.shape[3] // GRID)
        return torch.zeros(x.shape[0], hp * wp, N), hp, wp

    def seg_predict(self, scores, hp, wp, h, w, conf=False, probs=False, label_dtype=None):
        self.log.append(("seg_predict", (hp, wp), (h, w), dict(conf=conf, probs=probs)))
        B = len(scores)
        return (torch.zeros(B, h, w, dtype=torch.uint8), torch.zeros(B, h, w) if conf else None,
                torch.full((B, N, h, w), 0.2) if probs else None)

    def seg_score(self, scores, hp, wp, gt, label_dtype=None, raw_labels=True, labels=False, conf=False, probs=False, areas=None,
                  tally=None):
        self.log.append(("seg_score", (hp, wp), tuple(gt.shape), dict(labels=labels, conf=conf, probs=probs, raw_labels=raw_labels)))
        return (areas, tally, torch.zeros(gt.shape, dtype=torch.uint8) if labels else None,
                torch.zeros(gt.shape) if conf else None, None)

    def seg_pamr(self, probs, image, iters=10, dilations=PAMR_DILATIONS, conf=False, probs_out=False, label_dtype=None):
        assert probs.dtype == torch.float32 and probs.dim() == 3 and probs.is_contiguous()
        assert image.dtype == torch.uint8 and tuple(image.shape) == tuple(probs.shape[1:]) + (3,) and image.is_contiguous()
        self.log.append(("seg_pamr", int(image[0, 0, 0]), tuple(probs.shape), iters, tuple(dilations),
                         dict(conf=conf, probs_out=probs_out, label_dtype=label_dtype)))
        H, W = probs.shape[1:]
        return torch.zeros(H, W, dtype=torch.uint8), torch.zeros(H, W) if conf else None, probs.clone() if probs_out else None

    def seg_areas(self, labels, gt, n, raw_labels=True, areas=None, tally=None):
        assert labels.is_contiguous() and labels.shape == gt.shape and n == N
        self.log.append(("seg_areas", tuple(labels.shape), dict(counters=areas is not None and tally is not None, raw_labels=raw_labels)))
        return areas, tally

    def seg_confusion(self, labels, gt, n, raw_labels=True, confusion=None):
        assert labels.is_contiguous() and labels.shape == gt.shape and n == N
        self.log.append(("seg_confusion", tuple(labels.shape), dict(matrix=confusion is not None, raw_labels=raw_labels)))
        return confusion

    def seg_calibration(self, labels, conf, gt, n, raw_labels=True, calibration=None, tally=None):
        assert labels.shape == gt.shape == conf.shape and conf.dtype == torch.float32 and n == N
        self.log.append(("seg_calibration", tuple(labels.shape), dict(counters=calibration is not None and tally is not None)))
        return calibration, tally

    def seg_render(self, labels, image, palette, opacity, boundary, boundary_color, conf=None):
        self.log.append(("seg_render", tuple(labels.shape), dict(conf=conf is not None)))
        return torch.zeros_like(image)


def _images():
    """image i is filled with the value i, which the fakes read back"""
    return [torch.full(hw + (3,), i, dtype=torch.uint8) for i, hw in enumerate((A, B))], [torch.ones(hw, dtype=torch.uint8) for hw in (A, B)]


FRONT = [("image_load", [0], (64, 96)), ("image_load", [1], (64, 64)), ("forward", (1, 3, 64, 96)), ("forward", (1, 3, 64, 64))]
GRIDS = ((4, 6), (4, 4))
U8 = torch.uint8


def test_segment_raw_launches(monkeypatch):
    """`segment_raw` with pamr_iters=3: per image the predict launch, asked for every class's value and nothing else, then
    `seg_pamr` on the ORIGINAL uint8 photo, which supplies labels, conf and probs"""
    rec = Recorder(monkeypatch)
    seg = _seg(pamr_iters=3, pamr_dilations=(1, 2))
    imgs, _ = _images()
    out = seg.segment_raw(imgs, max_batch=3, return_conf=True)
    assert [tuple(r.labels.shape) for r in out] == [A, B] and all(r.conf is not None and r.probs is None for r in out)
    want = list(FRONT)
    for i, hw in enumerate((A, B)):
        want += [("seg_predict", GRIDS[i], hw, dict(conf=False, probs=True)),
                 ("seg_pamr", i, (N,) + hw, 3, (1, 2), dict(conf=True, probs_out=False, label_dtype=U8))]
    assert rec.log == want
    del rec.log[:]
    out = seg.segment_raw(imgs[:1], return_probs=True)
    assert out[0].conf is None and tuple(out[0].probs.shape) == (N,) + A
    assert rec.log[-1] == ("seg_pamr", 0, (N,) + A, 3, (1, 2), dict(conf=False, probs_out=True, label_dtype=U8))


@pytest.mark.parametrize("extra", ["plain", "confusion", "calibration"])
def test_evaluate_raw_launches(monkeypatch, extra):
    """`evaluate_raw`: `seg_pamr`'s labels are counted by `seg_areas`, then the optional counters, as on the CRF branch"""
    rec = Recorder(monkeypatch)
    seg = _seg(pamr_iters=3)
    imgs, gts = _images()
    score = seg.evaluate_raw(imgs, gts, max_batch=3, confusion=extra == "confusion", calibration=extra == "calibration")
    assert isinstance(score, SegmentationScore)
    want = list(FRONT)
    for i, hw in enumerate((A, B)):
        want += [("seg_predict", GRIDS[i], hw, dict(conf=False, probs=True)),
                 ("seg_pamr", i, (N,) + hw, 3, PAMR_DILATIONS, dict(conf=extra == "calibration", probs_out=False, label_dtype=U8)),
                 ("seg_areas", (1,) + hw, dict(counters=True, raw_labels=True))]
        if extra == "confusion":
            want += [("seg_confusion", (1,) + hw, dict(matrix=True, raw_labels=True))]
        if extra == "calibration":
            want += [("seg_calibration", (1,) + hw, dict(counters=True))]
    assert rec.log == want


def test_without_pamr_the_launches_of_today(monkeypatch):
    """pamr_iters=0 (the default, and given explicitly with other dilations): `seg_predict` with conf, `seg_score` alone"""
    for kw in ({}, dict(pamr_iters=0, pamr_dilations=(3,))):
        rec = Recorder(monkeypatch)
        seg = _seg(**kw)
        imgs, gts = _images()
        seg.segment_raw(imgs, max_batch=3, return_conf=True)
        assert rec.log == FRONT + [("seg_predict", GRIDS[i], hw, dict(conf=True, probs=False)) for i, hw in enumerate((A, B))]
        del rec.log[:]
        seg.evaluate_raw(imgs, gts, max_batch=3, confusion=True)
        want = list(FRONT)
        for i, hw in enumerate((A, B)):
            want += [("seg_score", GRIDS[i], (1,) + hw, dict(labels=True, conf=False, probs=False, raw_labels=True)),
                     ("seg_confusion", (1,) + hw, dict(matrix=True, raw_labels=True))]
        assert rec.log == want


def test_call_evaluate_and_render_launches(monkeypatch):
    """`__call__` and `evaluate` take a batch: one predict launch, then one `seg_pamr` per image on the CRF's image rule rounded
    to bytes; `render_raw(fade_by_conf=True)` is allowed, the conf being handed over"""
    rec = Recorder(monkeypatch)
    seg = _seg(pamr_iters=2)
    x = torch.stack([torch.full((3, 32, 48), v) for v in (-1.0, 0.2)])          # grey levels 0 and 153
    res = seg(x, return_conf=True)
    assert tuple(res.labels.shape) == (2, 32, 48) and tuple(res.conf.shape) == (2, 32, 48) and res.probs is None
    pam = [("seg_pamr", g, (N, 32, 48), 2, PAMR_DILATIONS, dict(conf=True, probs_out=False, label_dtype=U8)) for g in (0, 153)]
    assert rec.log == [("forward", (2, 3, 32, 48)), ("seg_predict", (2, 3), (32, 48), dict(conf=False, probs=True))] + pam
    del rec.log[:]
    photos = torch.stack([torch.full((40, 50, 3), v, dtype=torch.uint8) for v in (7, 9)])
    res = seg(x, out_hw=(40, 50), crf_images=photos)
    assert tuple(res.labels.shape) == (2, 40, 50)
    assert [e[:3] for e in rec.log[2:]] == [("seg_pamr", 7, (N, 40, 50)), ("seg_pamr", 9, (N, 40, 50))]
    del rec.log[:]
    seg.evaluate(x, torch.ones(2, 32, 48, dtype=torch.uint8))
    assert [e[0] for e in rec.log] == ["forward", "seg_predict", "seg_pamr", "seg_pamr", "seg_areas"]
    assert rec.log[-1] == ("seg_areas", (2, 32, 48), dict(counters=True, raw_labels=True))
    del rec.log[:]
    imgs, _ = _images()
    pics = seg.render_raw(imgs[:1], fade_by_conf=True)
    assert tuple(pics[0].picture.shape) == A + (3,) and pics[0].conf is not None
    assert [e[0] for e in rec.log] == ["image_load", "forward", "seg_predict", "seg_pamr", "seg_render"]
    assert rec.log[3][5]["conf"] is True and rec.log[4] == ("seg_render", A, dict(conf=True))
