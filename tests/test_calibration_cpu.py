"""Confidence calibration, the parts that need no GPU: `calibration_reference` against a per-pixel loop and against the other
counters' specifications, the score's readers (ECE, the reliability diagram, thresholds by measured precision), `add_` /
`merged` / refusals, and the header."""
import math
import os
import re

import pytest
import torch

import _calib_cases as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _loop(labels, conf, gt, n, raw_labels):
    """calibration_reference, one pixel at a time in plain Python"""
    cal, tally = torch.zeros(n, 256, 2, dtype=torch.int64), [0, 0]
    for l, c, g in zip(labels.reshape(-1).tolist(), conf.reshape(-1).tolist(), gt.reshape(-1).tolist()):
        if (g in (0, 255)) if raw_labels else (g in (n, 255)):
            continue
        cls = g - 1 if raw_labels else g
        if not 0 <= cls < n:
            continue
        if not 0 <= l < n:
            tally[1] += 1
            continue
        tally[0] += 1
        q = c * 256.0                                            # exact: a power of two
        b = 0 if math.isnan(q) else int(min(max(math.floor(q), 0.0), 255.0)) if not math.isinf(q) else (255 if q > 0 else 0)
        cal[l, b, int(l == cls)] += 1
    return cal, torch.tensor(tally)


@pytest.mark.parametrize("n,ldt,gdt,raw", [(5, torch.uint8, torch.uint8, True), (5, torch.int16, torch.int16, True),
                                           (5, torch.int16, torch.uint8, False), (300, torch.int16, torch.int16, True)],
                         ids=["u8_u8_raw", "i16_i16_raw", "i16_u8_ids", "n300_i16"])
def test_reference_is_the_per_pixel_loop(n, ldt, gdt, raw):
    from ifseg_amd.predict import calibration_reference
    labels, conf, gt = CC.maps(7 * 13, n, ldt, gdt, n, random=True, raw_labels=raw)
    labels[-4:] = torch.tensor([255, 255, 255, 255] if ldt == torch.uint8 else [-1, n, 511, -32768]).to(ldt)
    gt[-4:] = 1                                                  # scored pixels with a label outside the classes
    labels, conf, gt = labels.reshape(7, 13), conf.reshape(7, 13), gt.reshape(7, 13)
    got = calibration_reference(labels, conf, gt, n, raw)
    want = _loop(labels, conf, gt, n, raw)
    assert got[0].dtype == torch.int64 and got[0].shape == (n, 256, 2) and got[1].shape == (2,)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert int(want[1][1]) >= 4 and 0 < int(want[0][..., 1].sum()) < int(want[1][0])
    if n == 5:
        assert CC.telling(*want)


@pytest.mark.parametrize("n,ldt,gdt,raw", [(15, torch.uint8, torch.uint8, True), (150, torch.uint8, torch.int16, True),
                                           (33, torch.int16, torch.uint8, False)], ids=["n15", "n150", "n33_ids"])
def test_reference_agrees_with_the_other_counters(n, ldt, gdt, raw):
    """summed over bins and hit it is the per-class count of the scored, in-range labels; its hits are the intersections;
    its total the scored pixels with a label inside; with every pixel scored, summed over hit it is the confidence histogram"""
    from ifseg_amd.predict import areas_reference, calibration_reference, confidence_histogram_reference
    labels, conf, gt = CC.maps(5000, n, ldt, gdt, n + 1, random=True, raw_labels=raw)
    cal, tally = calibration_reference(labels, conf, gt, n, raw)
    assert CC.telling(cal, tally)
    areas, atally = areas_reference(labels, gt, n, raw)
    assert torch.equal(cal.sum((1, 2)), areas[1]) and torch.equal(cal[..., 1].sum(1), areas[0])
    assert int(cal.sum()) == int(tally[0]) and int(tally.sum()) == int(atally[0]) < 5000
    every = torch.full_like(gt, 1 if raw else 0)                 # class 0 everywhere: every pixel scored
    hist, htally = confidence_histogram_reference(labels, conf, n)
    cal1, tally1 = calibration_reference(labels, conf, every, n, raw)
    assert torch.equal(cal1.sum(2), hist) and torch.equal(tally1, htally)
    with pytest.raises(ValueError, match="calibration_reference"):
        calibration_reference(labels, conf.double(), gt, n, raw)
    with pytest.raises(ValueError, match="calibration_reference"):
        calibration_reference(labels, conf[:-1], gt, n, raw)
    with pytest.raises(ValueError, match="calibration_reference"):
        calibration_reference(labels, conf, gt.long(), n, raw)


def _score(n=6, npix=20000, seed=3, sharp=False):
    """a score filled by the reference from confidences in [0, 1) that mean something: a pixel is right with probability
    conf ** 2 (an over-confident model) -> (score, labels, conf, gt)"""
    from ifseg_amd.predict import SegmentationScore, calibration_reference
    g = torch.Generator().manual_seed(seed)
    labels = torch.randint(0, n - 1, (npix,), generator=g).to(torch.uint8)         # class n - 1 is never predicted
    conf = torch.rand(npix, generator=g)
    right = torch.rand(npix, generator=g) < (conf if sharp else conf * conf)
    wrong = (labels.long() + 1 + torch.randint(0, n - 1, (npix,), generator=g)) % n
    gt = (torch.where(right, labels.long(), wrong) + 1).to(torch.uint8)
    gt[::97] = 255
    cal, tally = calibration_reference(labels, conf, gt, n)
    score = SegmentationScore(n, calibration=cal)
    score.calibration_tally += tally
    return score, labels, conf, gt


def test_ece_is_within_half_a_fine_bin_of_the_raw_confidences():
    """`summary()`'s ECE / MCE / cECE at 16 bins against the same sums over the raw confidences' true bin means, float64: a
    fine bin's midpoint is within 1 / 512 of every confidence in it, so each figure is within 1 / 512"""
    n = 6
    score, labels, conf, gt = _score(n)
    s = score.summary()
    scored = gt != 255
    lab, c, hit = labels[scored].long(), conf[scored].double(), (labels[scored].long() == gt[scored].long() - 1).double()
    m = (c * 16).floor().long().clamp(0, 15)

    def ece_of(sel):
        N = int(sel.sum())
        gaps = []
        for k in range(16):
            here = sel & (m == k)
            if int(here.sum()):
                gaps.append((int(here.sum()) / N, abs(float(hit[here].mean()) - float(c[here].mean()))))
        return sum(w * gap for w, gap in gaps), max(gap for _, gap in gaps)

    ece, mce = ece_of(torch.ones_like(lab, dtype=torch.bool))
    assert ece > 0.05                                            # an over-confident model: there is something to measure
    assert abs(s["ECE"] - ece) <= 1 / 512 and abs(s["MCE"] - mce) <= 1 / 512
    assert len(s["cECE"]) == n and math.isnan(s["cECE"][n - 1])
    for cl in range(n - 1):
        assert abs(s["cECE"][cl] - ece_of(lab == cl)[0]) <= 1 / 512
    assert s["pixels"] == int(score.tally[0]) == 0               # areas were not filled here; the other keys are still there
    # the diagram behind it
    N, acc, cf = score.reliability()
    assert N.dtype == torch.int64 and N.shape == acc.shape == cf.shape == (16,) and int(N.sum()) == int(scored.sum())
    assert abs(float((N.double() / N.sum() * (acc - cf).abs()).sum()) - s["ECE"]) < 1e-12
    for k in range(16):
        assert abs(float(cf[k]) - float(c[m == k].mean())) <= 1 / 512 and float(acc[k]) == float(hit[m == k].mean())
    Nc, accc, cfc = score.reliability(bins=4, per_class=True)
    assert Nc.shape == (n, 4) and torch.equal(Nc.sum(0), N.reshape(4, 4).sum(1)) and bool(accc[n - 1].isnan().all())
    assert torch.equal(score.reliability(bins=256)[0], score.calibration.sum((0, 2)))
    for bad in (0, 3, 512, 16.0, True):
        with pytest.raises(ValueError, match="bins"):
            score.reliability(bins=bad)
    # a calibrated model has a small ECE by the same code
    assert _score(n, sharp=True)[0].summary()["ECE"] < 0.02


def _brute_thresholds(cal, target, min_pixels):
    out = []
    for c in range(cal.shape[0]):
        t_c = 256
        for t in range(256):
            N, H = int(cal[c, t:].sum()), int(cal[c, t:, 1].sum())
            if N >= min_pixels and float(H) >= float(target) * float(N):
                t_c = t
                break
        out.append(t_c)
    return torch.tensor(out, dtype=torch.int32)


def test_precision_thresholds_and_what_they_keep():
    from ifseg_amd.predict import pseudo_label_reference
    n = 6
    score, labels, conf, gt = _score(n)
    cal = score.calibration
    cal[2, 255] = torch.tensor([0, 3])                           # class 2: its last bin is all hits, so target = 1.0 is met there
    cal[2, 254, 0] += 1
    for target, min_pixels in ((0.5, 1), (0.8, 1), (0.8, 500), (1.0, 1), (0.999, 10 ** 9)):
        got = score.precision_thresholds(target, min_pixels)
        assert got.dtype == torch.int32 and got.shape == (n,)
        assert torch.equal(got, _brute_thresholds(cal, target, min_pixels)), (target, min_pixels)
        assert int(got[n - 1]) == 256                            # the class never predicted keeps nothing
    assert int(score.precision_thresholds(1.0)[2]) == 255 and score.precision_thresholds(0.999, 10 ** 9).tolist() == [256] * n
    assert 0 < int(score.precision_thresholds(0.8)[0]) < 256
    for bad in (0.0, -0.1, 1.5, True, "0.5"):
        with pytest.raises(ValueError, match="target"):
            score.precision_thresholds(bad)
    for bad in (0, 1.0, True):
        with pytest.raises(ValueError, match="min_pixels"):
            score.precision_thresholds(0.5, bad)
    # what the filter keeps under those thresholds is, per class, at least `target` right -- on the maps they were measured on
    score, labels, conf, gt = _score(n)
    for target in (0.5, 0.8):
        thr = score.precision_thresholds(target)
        out, kept = pseudo_label_reference(labels.reshape(100, 200), conf.reshape(100, 200), thr, n, boundary=0)
        out, g = out.reshape(-1), gt
        some = 0
        for c in range(n):
            if int(thr[c]) == 256:
                assert int(kept[0, c]) == 0
                continue
            here = (out == c + 1) & (g != 255)                   # kept pixels of class c that are scored
            some += int(here.sum())
            assert int(here.sum()) > 0 and float((g[here] == c + 1).double().mean()) >= target
        assert some > 0


def test_score_carries_the_counters():
    from ifseg_amd.predict import SegmentationScore
    n = 4
    plain = SegmentationScore(n)
    assert plain.calibration is None and plain.calibration_tally is None and "ECE" not in plain.summary()
    a, b = SegmentationScore(n, calibration=True), SegmentationScore(n, calibration=True, confusion=True)
    assert a.calibration.dtype == torch.int64 and a.calibration.shape == (n, 256, 2) and a.calibration_tally.tolist() == [0, 0]
    s = a.summary()
    assert math.isnan(s["ECE"]) and math.isnan(s["MCE"]) and len(s["cECE"]) == n and all(math.isnan(v) for v in s["cECE"])
    a.calibration[1, 200, 1], a.calibration[1, 10, 0], a.calibration_tally[0] = 5, 2, 7
    two = SegmentationScore(n, calibration=a.calibration.clone())
    two.calibration_tally += a.calibration_tally
    assert two.add_(a) is two and torch.equal(two.calibration, 2 * a.calibration) and two.calibration_tally.tolist() == [14, 0]
    with pytest.raises(ValueError, match="calibration"):
        plain.add_(a)
    with pytest.raises(ValueError, match="calibration"):
        a.add_(plain)
    for bad in (torch.zeros(n, 256, 2), torch.zeros(n, 256, dtype=torch.int64), "yes"):
        with pytest.raises(ValueError, match="calibration"):
            SegmentationScore(n, calibration=bad)
    for reader in (plain.reliability, lambda: plain.precision_thresholds(0.5)):
        with pytest.raises(ValueError, match="needs calibration counters"):
            reader()
    # merged() drops the counters, as it drops the boundary ones, and says why
    b.confusion[0, 0] = 3
    merged = b.merged([0, 0, 1, 1])
    assert merged.calibration is None and merged.calibration_tally is None and merged.confusion is not None
    assert "sum" in SegmentationScore.merged.__doc__.lower() and "calibration" in SegmentationScore.merged.__doc__


def test_evaluate_refuses_before_anything_runs():
    """the keyword's checks need no model beyond its configuration: a stand-in with no parameters cannot have launched anything"""
    from ifseg_amd.predict import SegmentationScore, Segmenter
    seg = Segmenter.__new__(Segmenter)
    seg.n, seg.crf_iters, seg.smooth_iters, seg.upsample, seg.slide_views = 4, 0, 0, "probs", False
    dev = torch.device("cpu")
    for bad in (1, None, torch.zeros(4, 256, 2, dtype=torch.int64), "yes"):
        with pytest.raises(ValueError, match="calibration must be True or False"):
            seg._score_into("evaluate_raw", None, dev, calibration=bad)
    with pytest.raises(ValueError, match="carries no calibration counters"):
        seg._score_into("evaluate_raw", SegmentationScore(4), dev, calibration=True)
    carried = SegmentationScore(4, calibration=True)
    assert seg._score_into("evaluate_raw", carried, dev) is carried
    assert seg._score_into("evaluate_raw", None, dev, calibration=True).calibration is not None
    assert seg._score_into("evaluate_raw", None, dev).calibration is None
    seg.upsample = "logits"
    for kw in (dict(calibration=True), dict(into=carried)):
        with pytest.raises(ValueError, match=r"confidence must be a probability.*upsample='logits'"):
            seg._score_into("evaluate_raw", kw.get("into"), dev, calibration=kw.get("calibration", False))
    seg.slide_views = True                                       # the softmax inside the slide-views launch
    assert seg._score_into("evaluate_raw", None, dev, calibration=True, sl=(128, 85)).calibration is not None
    assert seg._score_into("evaluate_raw", None, dev).calibration is None        # without the keyword raw logits are scored as ever


def test_header_and_bindings_declare_the_entries():
    from ifseg_amd import hip
    with open(os.path.join(ROOT, "include", "ifseg_hip.h")) as fh:
        text = fh.read()
    assert int(re.search(r"#define\s+IFSEG_ABI_VERSION\s+(\d+)", text).group(1)) == 21 == hip.ABI_VERSION
    decl = re.search(r"int ifseg_seg_calibration\(([^;]*)\);", text).group(1)
    names = [a.split()[-1].lstrip("*") for a in decl.replace("\n", " ").split(",")]
    assert names == ["labels", "label_bytes", "conf", "gt", "gt_bytes", "npix", "n", "raw_labels", "calibration", "tally", "stream"]
    assert "int ifseg_seg_calibration_limit(int which);" in text
    assert hip.SEG_CALIBRATION_DIRECT_CLASSES == 32 and hip.SEG_CALIBRATION_DIRECT_CLASSES * 512 * 4 == 64 * 1024
    assert callable(hip.seg_calibration) and callable(hip.seg_calibration_limits)
