"""CPU: the specification of Boundary IoU's counters (`ifseg_amd.predict.boundary_areas_reference`) against a literal
transcription of upstream's `mask_to_boundary` class by class, its identities with `areas_reference`, `boundary_distance`, what
`SegmentationScore` does with the counters (`add_`, `summary`, `group_summary`, `merged`), the header and the library's limits,
the refusals of the binding, the op and `evaluate_raw` before anything reaches the library, and the Segmenter's launch sequence
in every setting with recording fakes.  The counters are integers: every comparison is exact, and no pixel is left out."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import _boundary_cases as BC
import _score_cases as SC
import test_segmenter_launches_cpu as L
from ifseg_amd import hip
from ifseg_amd.predict import (SegmentationScore, Segmenter, areas_reference, boundary_areas_reference, boundary_distance)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------- the rule
def _mask_to_boundary(mask, d):
    """upstream's mask_to_boundary, literally: one ring of zeros around the mask, d times a 3 x 3 minimum that ignores positions
    outside the array, the ring cropped, mask - eroded"""
    h, w = mask.shape
    x = F.pad(mask.double()[None, None], (1, 1, 1, 1), value=0.0)
    for _ in range(d):
        x = -F.max_pool2d(-x, 3, 1, 1)                         # the pooling pads with -inf: outside positions take no part
    return mask.double() - x[0, 0, 1:h + 1, 1:w + 1]


def _band_by_erosion(m, d):
    """a pixel is in the band of its map iff it is on the boundary of its own value's mask"""
    band = torch.zeros(m.shape, dtype=torch.bool)
    for v in torch.unique(m).tolist():
        b = _mask_to_boundary(m == v, d)
        assert ((b == 0) | (b == 1)).all() and not b[m != v].any()
        band |= b.bool()
    return band


def _check_against_erosion(labels, gt, n, d, raw):
    bareas, band = boundary_areas_reference(labels, gt, n, d, raw)
    assert bareas.dtype == torch.int64 and bareas.shape == (3, n) and band.dtype == torch.uint8 and band.shape == gt.shape
    assert torch.equal((band & 1).bool(), _band_by_erosion(gt.long(), d))
    assert torch.equal((band & 2).bool(), _band_by_erosion(labels.long(), d)) and int(band.max()) <= 3
    # the counters from the bands, value by value
    scored, cls, _ = SC.by_hand(labels, gt, n, raw)
    want = torch.zeros(3, n, dtype=torch.int64)
    for p, c, s, b in zip(labels.reshape(-1).tolist(), cls.reshape(-1).tolist(), scored.reshape(-1).tolist(), band.reshape(-1).tolist()):
        if s:
            want[2, c] += b & 1
            if 0 <= p < n:
                want[1, p] += b >> 1
                want[0, p] += (p == c) and b == 3
    assert torch.equal(bareas, want)


@pytest.mark.parametrize("raw", [True, False], ids=["raw", "ids"])
@pytest.mark.parametrize("k", range(4), ids=BC.IDS[:4])
def test_reference_is_the_erosion_on_block_maps(k, raw):
    assert BC.nonempty(k, "i16", raw, True)
    labels, gt, n = BC.maps(BC.TABLE[k], torch.int16, torch.uint8, raw, outside=True)
    assert ((labels < 0) | (labels >= n)).any() and (gt == 255).any()
    _check_against_erosion(labels, gt, n, BC.TABLE[k][2], raw)


@pytest.mark.parametrize("d", [1, 2, 3, 7])
@pytest.mark.parametrize("n,dtype", [(1, torch.uint8), (5, torch.uint8), (40, torch.int16)])
def test_reference_is_the_erosion_on_random_maps(n, dtype, d):
    labels, gt = SC.labels_and_gt(n, True, dtype, seed=d, size=(23, 19))
    labels[3:9, 2:11] = 2 % n                                   # some room for an interior at d = 1, 2
    gt[2:10, 4:12] = 1
    labels[0, 0], labels[22, 18] = -1, n
    _check_against_erosion(labels, gt, n, d, True)
    # any leading shape: two maps at once are the two maps one after the other
    both, bands = boundary_areas_reference(torch.stack([labels, labels.flip(0)]), torch.stack([gt, gt.flip(1)]), n, d)
    one, b1 = boundary_areas_reference(labels, gt, n, d)
    two, b2 = boundary_areas_reference(labels.flip(0), gt.flip(1), n, d)
    assert torch.equal(both, one + two) and torch.equal(bands, torch.stack([b1, b2]))


def test_reference_refusals():
    labels, gt = SC.labels_and_gt(5, True, torch.uint8)
    with pytest.raises(ValueError, match="boundary_areas_reference: ground truth must be uint8 or int16"):
        boundary_areas_reference(labels, gt.long(), 5, 2)
    with pytest.raises(ValueError, match="boundary_areas_reference: labels must be integer"):
        boundary_areas_reference(labels.float(), gt, 5, 2)
    for bad in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError, match="d must be an int >= 1"):
            boundary_areas_reference(labels, gt, 5, bad)
    with pytest.raises(ValueError, match=r"\[\.\.\., h, w\]"):
        boundary_areas_reference(labels.reshape(-1), gt.reshape(-1), 5, 2)


def test_boundary_distance():
    assert [boundary_distance(h, w) for h, w in ((512, 683), (1024, 2048), (300, 400), (37, 91))] == [17, 46, 10, 2]
    assert boundary_distance(1, 1) == 1 and boundary_distance(20, 20) == 1 and boundary_distance(3, 4, 0.0001) == 1
    assert boundary_distance(300, 400, 0.05) == 25 and boundary_distance(2263, 2263) == 64 and boundary_distance(2300, 2300) == 65
    assert isinstance(boundary_distance(512, 683), int)


@pytest.mark.parametrize("outside", [False, True], ids=["inside", "outside"])
@pytest.mark.parametrize("k", range(len(BC.TABLE)), ids=BC.IDS)
def test_band_areas_never_pass_areas(k, outside):
    assert BC.nonempty(k, "i16", True, outside)
    bareas, band, areas = BC.reference(k, "i16", True, outside)
    assert (bareas <= areas).all() and (bareas[0] <= torch.minimum(bareas[1], bareas[2])).all()


@pytest.mark.parametrize("raw", [True, False], ids=["raw", "ids"])
def test_a_band_wider_than_the_image_is_areas(raw):
    for k in (0, 3):
        labels, gt, n = BC.maps(BC.TABLE[k], torch.int16, torch.uint8, raw, outside=True)
        h, w = gt.shape
        areas = areas_reference(labels, gt, n, raw)[0]
        for d in (max(h, w), max(h, w) + 5):
            bareas, band = boundary_areas_reference(labels, gt, n, d, raw)
            assert torch.equal(bareas, areas) and band.eq(3).all()
    labels, gt = SC.labels_and_gt(7, raw, torch.int16)
    assert torch.equal(boundary_areas_reference(labels, gt, 7, 40, raw)[0], areas_reference(labels, gt, 7, raw)[0])


def test_the_band_of_a_constant_map_is_the_frame():
    h, w, n = 31, 47, 5
    for d in (1, 3, 16):
        gt = torch.full((h, w), 3, dtype=torch.uint8)
        bareas, band = boundary_areas_reference(torch.full((h, w), 1, dtype=torch.int16), gt, n, d)      # raw 3 is class 2
        frame = torch.ones(h, w, dtype=torch.bool)
        frame[d:h - d, d:w - d] = False
        assert torch.equal(band, frame.to(torch.uint8) * 3)
        size = int(frame.sum())
        assert bareas.tolist() == [[0] * n, [0, size, 0, 0, 0], [0, 0, size, 0, 0]] and (size == h * w) == (d == 16)
        same = boundary_areas_reference(torch.full((h, w), 2, dtype=torch.int16), gt, n, d)[0]
        assert same.tolist() == [[0, 0, size, 0, 0]] * 3


# ------------------------------------------------------------------------------------------------- the score
def _score(k, boundary=True, ratio=0.02):
    bareas, _, areas = BC.reference(k, "i16", True, False)
    n = areas.shape[1]
    return SegmentationScore(n, areas=areas.clone(), tally=torch.tensor([int(areas[2].sum()), 0]),
                             boundary=bareas.clone() if boundary else None, boundary_ratio=ratio)


def test_score_constructor_and_add():
    assert SegmentationScore(7).boundary is None and SegmentationScore(7, boundary=False).boundary is None
    t = SegmentationScore(7, torch.device("cpu"), boundary=True)
    assert t.boundary.dtype == torch.int64 and t.boundary.shape == (3, 7) and not t.boundary.any() and t.boundary_ratio == 0.02
    given = torch.zeros(3, 7, dtype=torch.int64)
    assert SegmentationScore(7, boundary=given, boundary_ratio=0.05).boundary is given
    for bad in (torch.zeros(3, 6, dtype=torch.int64), torch.zeros(3, 7, dtype=torch.int32), torch.zeros(3, 7), [[0] * 7] * 3, 1):
        with pytest.raises(ValueError, match=r"boundary must be None, True or int64 \[3, 7\]"):
            SegmentationScore(7, boundary=bad)
    for bad in (0, 1, -0.1, 1.5, "0.02", True, None):
        with pytest.raises(ValueError, match="boundary ratio must be a number in"):
            SegmentationScore(7, boundary=True, boundary_ratio=bad)
    a, b = _score(0), _score(0)
    b.boundary += 1
    tot = SegmentationScore(a.n, boundary=True).add_(a).add_(b)
    assert torch.equal(tot.boundary, a.boundary + b.boundary) and torch.equal(tot.areas, 2 * a.areas)
    # one with and one without, or two ratios, are refused either way round, and nothing is added
    keep = tot.areas.clone()
    plain = _score(0, boundary=False)
    with pytest.raises(ValueError, match="boundary counters and the other has none"):
        tot.add_(plain)
    with pytest.raises(ValueError, match="boundary counters and the other has none"):
        plain.add_(a)
    with pytest.raises(ValueError, match="ratio 0.02 against ratio 0.05"):
        tot.add_(_score(0, ratio=0.05))
    assert torch.equal(tot.areas, keep) and torch.equal(plain.areas, a.areas)
    # two scores without counters add whatever their ratios say
    assert torch.equal(plain.add_(_score(0, boundary=False, ratio=0.05)).areas, 2 * a.areas)


def test_summary_gains_boundary_iou_and_is_unchanged_without():
    s, plain = _score(3), _score(3, boundary=False)
    got, base = s.summary(), plain.summary()
    assert list(base) == ["aAcc", "mIoU", "mAcc", "IoU", "Acc", "pixels"]
    assert list(got) == list(base) + ["mBIoU", "BIoU"] and repr({k: got[k] for k in base}) == repr(base)
    b = s.boundary.double()
    biou = b[0] / (b[1] + b[2] - b[0])
    assert got["BIoU"] == [round(float(v), 4) for v in biou] and got["mBIoU"] == round(float(torch.nanmean(biou)), 4)
    assert 0 < got["mBIoU"] < got["mIoU"]                     # shifted blocks: the bands overlap less than the regions
    # an absent class is NaN and stays out of the mean
    s.boundary[:, 0] = 0
    again = s.summary()
    assert again["BIoU"][0] != again["BIoU"][0] and again["mBIoU"] == round(float(torch.nanmean(biou[1:])), 4)
    # ground truth out of range is refused as ever
    s.tally[1] = 2
    with pytest.raises(IndexError, match=r"tally\[1\] = 2"):
        s.summary()


def test_group_summary_and_merged():
    s, plain = _score(3), _score(3, boundary=False)
    n = s.n
    groups = {"low": range(0, n // 2), "high": range(n // 2, n)}
    got, base = s.group_summary(groups), plain.group_summary(groups)
    b = s.boundary.double()
    biou = b[0] / (b[1] + b[2] - b[0])
    for name, ids in groups.items():
        assert got[name] == dict(base[name], mBIoU=round(float(torch.nanmean(biou[list(ids)])), 4))
        assert list(base[name]) == ["mIoU", "mAcc"]
    assert got["hIoU"] == base["hIoU"]
    s.tally[1] = 1
    with pytest.raises(IndexError, match=r"tally\[1\] = 1"):
        s.group_summary(groups)
    # merged: the coarser score has no boundary counters
    labels, gt, n = BC.maps(BC.TABLE[0], torch.int16, torch.uint8)
    from ifseg_amd.predict import confusion_reference
    areas, tally = areas_reference(labels, gt, n)
    full = SegmentationScore(n, areas=areas, tally=tally, confusion=confusion_reference(labels, gt, n),
                             boundary=boundary_areas_reference(labels, gt, n, 1)[0])
    two = full.merged([c % 2 for c in range(n)])
    assert two.boundary is None and two.confusion is not None and "mBIoU" not in two.summary() and "mBIoU" in full.summary()
    assert "contours" in SegmentationScore.merged.__doc__


# ------------------------------------------------------------------------------------------------- header, library, refusals
def test_header_declares_the_entries_and_keeps_the_abi_version():
    with open(os.path.join(ROOT, "include", "ifseg_hip.h")) as f:
        header = f.read()
    assert re.search(r"^int ifseg_seg_boundary_areas\(const void\* labels, int label_bytes, const void\* gt, int gt_bytes, int B, "
                     r"int h, int w, int n, int d,\s+int raw_labels, void\* bareas, void\* band, void\* stream\);", header, re.M)
    assert re.search(r"^int ifseg_seg_boundary_limit\(int which\);", header, re.M)
    assert re.search(r"#define\s+IFSEG_ABI_VERSION\s+21\b", header) and hip.ABI_VERSION == 21
    with open(os.path.join(ROOT, "ifseg_amd", "csrc", "boundary.hip")) as f:
        src = f.read()
    assert int(re.search(r"constexpr int SEG_BOUNDARY_MAX_D = (\d+);", src).group(1)) == hip.SEG_BOUNDARY_MAX_D == 64
    assert int(re.search(r"constexpr int SB_MAX_CLASSES = (\d+);", src).group(1)) == hip.SEG_PREDICT_MAX_CLASSES
    assert hip.seg_boundary_limits() == (hip.SEG_BOUNDARY_MAX_D, hip.SEG_PREDICT_MAX_CLASSES)
    assert hip.lib().ifseg_seg_boundary_limit(2) == -3 and hip.lib().ifseg_seg_boundary_limit(-1) == -3
    assert boundary_distance(1024, 2048) <= hip.SEG_BOUNDARY_MAX_D


def _no_library(monkeypatch):
    def fail():
        raise RuntimeError("the library was reached")
    monkeypatch.setattr(hip, "lib", fail)


def test_binding_refuses_before_it_launches(monkeypatch):
    _no_library(monkeypatch)
    lab, gt = torch.zeros(2, 4, 6, dtype=torch.uint8), torch.zeros(2, 4, 6, dtype=torch.int16)
    for bad in ((lab.long(), gt), (lab, gt.long()), (lab[:, :, :5], gt), (lab, gt.transpose(1, 2)), (lab.reshape(-1), gt.reshape(-1)),
                (lab[None], gt[None]), (lab[:0], gt[:0])):
        with pytest.raises(AssertionError):
            hip.seg_boundary_areas(*bad, 5, 2)
    for n in (0, 513):
        with pytest.raises(AssertionError):
            hip.seg_boundary_areas(lab, gt, n, 2)
    for d in (0, -1, 65, 2.0, True, None):
        with pytest.raises(AssertionError):
            hip.seg_boundary_areas(lab, gt, 5, d)
    for bad in (torch.zeros(3, 4, dtype=torch.int64), torch.zeros(3, 5, dtype=torch.int32), torch.zeros(5, 3, dtype=torch.int64).t()):
        with pytest.raises(AssertionError):
            hip.seg_boundary_areas(lab, gt, 5, 2, bareas=bad)


def test_op_is_registered_with_a_fake_kernel():
    import ifseg_amd.ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    op = torch.ops.ifseg.seg_boundary_areas
    with FakeTensorMode():
        lab = torch.empty(2, 9, 7, dtype=torch.uint8, device="cuda")
        gt = torch.empty(2, 9, 7, dtype=torch.int16, device="cuda")
        for n, d in ((1, 1), (150, 17), (512, 64)):
            bareas, band = op(lab, gt, n, d, True)
            assert bareas.shape == (3, n) and bareas.dtype == torch.int64 and bareas.is_cuda
            assert band.shape == (2, 9, 7) and band.dtype == torch.uint8 and band.is_cuda
        assert op(lab[0], gt[0], 5, 2, False)[1].shape == (9, 7)
        with pytest.raises(Exception, match="seg_boundary_areas: labels must be uint8 or int16"):
            op(lab.long(), gt, 150, 2, True)
        with pytest.raises(Exception, match="seg_boundary_areas: ground truth must be uint8 or int16"):
            op(lab, gt.long(), 150, 2, True)
        with pytest.raises(Exception, match="must have one shape"):
            op(lab[:1], gt, 150, 2, True)
        with pytest.raises(Exception, match="n = 513 classes"):
            op(lab, gt, 513, 2, False)
        for d in (0, 65, -3):
            with pytest.raises(Exception, match="d = %d, the band's half width must be in 1 .. SEG_BOUNDARY_MAX_D = 64" % d):
                op(lab, gt, 5, d, True)
        with pytest.raises(Exception, match=r"must be \[B, h, w\] or \[h, w\]"):
            op(lab[None], gt[None], 5, 2, True)


class _Model(torch.nn.Linear):
    """as much of a model as the checks of evaluate_raw look at"""

    def __init__(self):
        super().__init__(1, 1)
        self.cfg = type("Cfg", (), {"num_seg_tokens": 5, "patch_image_size": 128})()


def test_evaluate_raw_refuses_before_it_launches(monkeypatch):
    _no_library(monkeypatch)
    monkeypatch.setattr(hip, "image_load", lambda *a, **k: (_ for _ in ()).throw(RuntimeError("image_load was reached")))
    seg = Segmenter(_Model(), category_token_ids=[[31], [32], [33], [34], [35]])
    im, gt = [torch.zeros(60, 90, 3, dtype=torch.uint8)], [torch.zeros(60, 90, dtype=torch.uint8)]
    with pytest.raises(ValueError, match="evaluate_raw: boundary_iou=True, but `into` carries no boundary counters"):
        seg.evaluate_raw(im, gt, into=SegmentationScore(5), boundary_iou=True)
    with pytest.raises(ValueError, match="evaluate_raw: boundary_iou asks for a band of ratio 0.02, `into` counts bands of ratio 0.05"):
        seg.evaluate_raw(im, gt, into=SegmentationScore(5, boundary=True, boundary_ratio=0.05), boundary_iou=True)
    with pytest.raises(ValueError, match="ratio 0.01, `into` counts bands of ratio 0.02"):
        seg.evaluate_raw(im, gt, into=SegmentationScore(5, boundary=True), boundary_iou=0.01)
    for bad in (0, 1, 1.0, -0.02, "yes", None, torch.zeros(3, 5, dtype=torch.int64)):
        with pytest.raises(ValueError, match="evaluate_raw: boundary_iou is True, False or a ratio"):
            seg.evaluate_raw(im, gt, boundary_iou=bad)
    # d above the kernel's limit names the image and its d: 0.02 of a 3300-pixel diagonal is 66, the first image's is 2
    big = [im[0], torch.zeros(1980, 2640, 3, dtype=torch.uint8)]
    big_gt = [gt[0], torch.zeros(1980, 2640, dtype=torch.uint8)]
    with pytest.raises(ValueError, match=r"evaluate_raw: image 1 \(1980 x 2640\) has a boundary band of d = 66 pixels"):
        seg.evaluate_raw(big, big_gt, boundary_iou=True)
    with pytest.raises(ValueError, match=r"image 0 \(60 x 90\) has a boundary band of d = 65"):
        seg.evaluate_raw(im, gt, boundary_iou=0.6)
    with pytest.raises(ValueError, match=r"image 1 .* d = 66"):
        seg.evaluate_raw(big, big_gt, into=SegmentationScore(5, boundary=True))
    with pytest.raises(ValueError, match="evaluate: boundary_iou=True, but `into` carries no boundary counters"):
        seg.evaluate(torch.zeros(1, 3, 128, 128), torch.zeros(1, 128, 128, dtype=torch.uint8), into=SegmentationScore(5), boundary_iou=True)
    # nothing to score: the empty score has counters when asked for them, and `into` comes back as it was
    empty = seg.evaluate_raw([], [], boundary_iou=0.05)
    assert empty.boundary.shape == (3, 5) and not empty.boundary.any() and empty.boundary_ratio == 0.05
    assert seg.evaluate_raw([], []).boundary is None and seg.evaluate_raw([], [], boundary_iou=False).boundary is None
    into = SegmentationScore(5, boundary=True)
    assert seg.evaluate_raw([], [], into=into) is into and seg.evaluate_raw([], [], into=into, boundary_iou=True) is into
    assert seg.evaluate_raw([], [], into=into, boundary_iou=0.02) is into


# ------------------------------------------------------------------------------------------------- the launches
class Recorder(L.Recorder):
    def __init__(self, monkeypatch):
        super().__init__(monkeypatch)
        monkeypatch.setattr(hip, "seg_boundary_areas", self.seg_boundary_areas)

    def seg_boundary_areas(self, labels, gt, n, d, raw_labels=True, bareas=None, band=False):
        assert labels.is_contiguous() and labels.shape == gt.shape and labels.dim() == 3 and n == L.N and not band
        self.log.append(("seg_boundary_areas", tuple(labels.shape), d, dict(counters=bareas is not None, raw_labels=raw_labels)))
        return bareas, None


def _with_boundary(want, ratio, pairs, crf):
    """the expected log of a run without boundary counters -> with them: every scoring launch is asked for its label map, and one
    seg_boundary_areas follows each image's last counting launch (seg_confusion where the matrix is counted, else seg_areas
    behind the CRF, else the scoring launch), with d of the image's own shape"""
    last = "seg_confusion" if pairs else "seg_areas" if crf else "seg_score"
    out = []
    for e in want:
        if e[0].startswith("seg_score"):
            e = e[:3] + (dict(e[3], labels=True),)
        out.append(e)
        if e[0].startswith(last):
            shape = e[2] if e[0].startswith("seg_score") else e[1]
            out.append(("seg_boundary_areas", shape, boundary_distance(shape[1], shape[2], ratio), dict(counters=True, raw_labels=True)))
    return out


@pytest.mark.parametrize("pairs", [False, True], ids=["alone", "with_confusion"])
@pytest.mark.parametrize("crf", [False, True], ids=["plain", "crf"])
@pytest.mark.parametrize("setting", list(L.SETTINGS))
def test_raw_launch_sequence_with_boundary(monkeypatch, setting, crf, pairs):
    imgs, gts = L._images()
    kw = dict(max_batch=3, confusion=pairs, **L.SETTINGS[setting][2])
    base = L._expected(setting, crf, "evaluate_raw_confusion" if pairs else "evaluate_raw")
    for boundary_iou, ratio in ((False, None), (True, 0.02), (0.05, 0.05)):
        rec = Recorder(monkeypatch)
        seg = Segmenter(L._Model(), category_token_ids=[[1]] * L.N, crf_iters=2 if crf else 0, **L.SETTINGS[setting][1])
        score = seg.evaluate_raw(imgs, gts, boundary_iou=boundary_iou, **kw)
        assert (score.boundary is not None) == (ratio is not None) and (score.confusion is not None) == pairs
        want = base if ratio is None else _with_boundary(base, ratio, pairs, crf)
        assert rec.log == want, (boundary_iou, rec.log, want)
        if ratio is not None:
            calls = [e for e in rec.log if e[0] == "seg_boundary_areas"]
            assert [(e[1], e[2]) for e in calls] == [((1,) + hw, boundary_distance(*hw, ratio)) for hw in (L.A, L.B)]
            # an `into` that carries the counters decides without the keyword
            del rec.log[:]
            assert seg.evaluate_raw(imgs, gts, into=score, **kw) is score and rec.log == want
    assert [boundary_distance(*hw) for hw in (L.A, L.B)] == [2, 4] and [boundary_distance(*hw, 0.05) for hw in (L.A, L.B)] == [6, 9]


@pytest.mark.parametrize("crf", [False, True], ids=["plain", "crf"])
def test_evaluate_launch_sequence_with_boundary(monkeypatch, crf):
    """`evaluate` takes a ready batch: one seg_boundary_areas for the whole batch behind its counting launch"""
    rec = Recorder(monkeypatch)
    seg = Segmenter(L._Model(), category_token_ids=[[1]] * L.N, crf_iters=2 if crf else 0)
    x = torch.stack([rec.coded(("x", b), 3, 32, 48) for b in range(2)])
    gt = torch.ones(2, 32, 48, dtype=torch.uint8)
    logs = {}
    for pairs in (False, True):
        for boundary_iou in (False, True):
            del rec.log[:]
            score = seg.evaluate(x, gt, confusion=pairs, boundary_iou=boundary_iou)
            assert (score.boundary is not None) == boundary_iou
            logs[pairs, boundary_iou] = list(rec.log)
    for pairs in (False, True):
        want = [e[:3] + (dict(e[3], labels=True),) if e[0] == "seg_score" else e for e in logs[pairs, False]]
        want.append(("seg_boundary_areas", (2, 32, 48), boundary_distance(32, 48), dict(counters=True, raw_labels=True)))
        assert logs[pairs, True] == want
    assert logs[False, False][-1][0] == ("seg_areas" if crf else "seg_score") and logs[True, False][-1][0] == "seg_confusion"
