"""CPU: the specification of the scoring counters (`ifseg_amd.predict.areas_reference`) against the criterion's own
`compute_metric`, `SegmentationScore` against `SegCriterion.reduce_metrics`, the header, and the refusals of the bindings, of
`Segmenter.evaluate_raw` and of the ops before anything reaches the library."""
import os
import re

import pytest
import torch

import _score_cases as SC
from ifseg_amd import hip
from ifseg_amd.criterions import SegCriterion
from ifseg_amd.predict import SegmentationScore, Segmenter, areas_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(1, torch.uint8), (5, torch.uint8), (5, torch.int16), (150, torch.uint8), (150, torch.int16), (257, torch.int16)]


@pytest.mark.parametrize("raw_labels", [True, False], ids=["raw", "ids"])
@pytest.mark.parametrize("n,dtype", CASES)
def test_areas_reference_is_compute_metric_on_the_masked_inputs(n, dtype, raw_labels):
    labels, gt = SC.labels_and_gt(n, raw_labels, dtype)
    present = {SC.kind(int(v), n, raw_labels) for v in gt.reshape(-1)}
    assert -1 in present and -2 in present and (n - 1 in present or n == 1) and 0 in present      # every kind is there
    areas, tally = areas_reference(labels, gt, n, raw_labels)
    assert areas.dtype == torch.int64 and areas.shape == (3, n) and tally.dtype == torch.int64 and tally.shape == (2,)
    scored, cls, bad = SC.by_hand(labels, gt, n, raw_labels)
    # the criterion's valid_step: masked pixels leave the scores and the target, then compute_metric (three histc)
    lprobs = torch.nn.functional.one_hot(labels[scored], n).float()
    a_i, a_p, a_l, a_u = SegCriterion.compute_metric(lprobs, cls[scored])
    assert torch.equal(areas[0].float(), a_i) and torch.equal(areas[1].float(), a_p) and torch.equal(areas[2].float(), a_l)
    assert tally.tolist() == [int(scored.sum()), bad] and bad > 0
    assert int(tally[0]) == int(areas[1].sum()) == int(areas[2].sum())
    assert int(areas[0].sum()) == int((labels[scored] == cls[scored]).sum()) > 0


def test_areas_reference_shapes_dtypes_and_refusals():
    labels, gt = SC.labels_and_gt(5, True, torch.uint8, size=(2, 3, 11, 7))
    a, t = areas_reference(labels, gt, 5)
    b, u = areas_reference(labels.to(torch.uint8).reshape(6, 77), gt.reshape(6, 77), 5, raw_labels=True)
    assert torch.equal(a, b) and torch.equal(t, u)
    # a predicted label outside [0, n) on a scored pixel: in tally[0] and areas[2] alone
    a, t = areas_reference(torch.tensor([[7, 1, -1]]), torch.tensor([[2, 2, 3]], dtype=torch.int16), 5)
    assert a.tolist() == [[0, 1, 0, 0, 0], [0, 1, 0, 0, 0], [0, 2, 1, 0, 0]] and t.tolist() == [3, 0]
    with pytest.raises(ValueError, match="uint8 or int16"):
        areas_reference(labels, gt.long(), 5)
    with pytest.raises(ValueError, match="labels must be integer"):
        areas_reference(labels.float(), gt, 5)
    with pytest.raises(ValueError, match="shape"):
        areas_reference(labels[0], gt, 5)


def _two_scores(n=7):
    out = []
    for seed in (1, 2):
        labels, gt = SC.labels_and_gt(n, True, torch.uint8, seed=seed)
        gt = torch.where(torch.tensor([SC.kind(int(v), n, True) for v in gt.reshape(-1)]).reshape(gt.shape) == -2,
                         torch.zeros_like(gt), gt)                                    # nothing out of range
        gt = torch.where(gt == 3, torch.zeros_like(gt), gt)                          # class 2 never occurs in the ground truth
        labels = torch.where(labels == 4, torch.zeros_like(labels), labels)          # class 4 is never predicted
        out.append(SegmentationScore(n, areas=areas_reference(labels, gt, n)[0], tally=areas_reference(labels, gt, n)[1]))
    return out


def test_summary_is_reduce_metrics_on_two_scores():
    a, b = _two_scores()
    for k in ("area_intersect", "area_pred_label", "area_label", "area_union"):
        assert a.logging_output()[k].dtype.is_floating_point and a.logging_output()[k].shape == (7,)
    want = SegCriterion.reduce_metrics([a.logging_output(), b.logging_output()])
    tot = SegmentationScore(7).add_(a).add_(b)
    assert torch.equal(tot.areas, a.areas + b.areas) and torch.equal(tot.tally, a.tally + b.tally)
    got = tot.summary()
    assert sorted(got) == ["Acc", "IoU", "aAcc", "mAcc", "mIoU", "pixels"]
    assert (got["aAcc"], got["mIoU"], got["mAcc"]) == (want["aAcc"], want["mIoU"], want["mAcc"])
    assert 0 < got["mIoU"] < 1 and got["pixels"] == int(tot.tally[0])
    ar = tot.areas.double()
    iou, acc = ar[0] / (ar[1] + ar[2] - ar[0]), ar[0] / ar[2]
    assert len(got["IoU"]) == 7 and len(got["Acc"]) == 7
    for c in range(7):
        for mine, ref in ((got["IoU"][c], iou[c]), (got["Acc"][c], acc[c])):
            assert (mine != mine) == bool(torch.isnan(ref)) and (mine != mine or mine == round(float(ref), 4))
    assert got["Acc"][2] != got["Acc"][2]                                             # 0 / 0: left out by nanmean
    assert got["mAcc"] == round(float(torch.nanmean(acc)), 4) and got["mIoU"] == round(float(torch.nanmean(iou)), 4)
    # add_ refuses another class count
    with pytest.raises(ValueError, match="classes"):
        tot.add_(SegmentationScore(5))
    with pytest.raises(ValueError, match="int64"):
        SegmentationScore(5, areas=torch.zeros(3, 4, dtype=torch.int64))


def test_summary_raises_on_ground_truth_out_of_range():
    labels, gt = SC.labels_and_gt(5, True, torch.uint8)
    areas, tally = areas_reference(labels, gt, 5)
    assert int(tally[1]) > 0
    with pytest.raises(IndexError, match=r"tally\[1\] = %d" % int(tally[1])):
        SegmentationScore(5, areas=areas, tally=tally).summary()


def test_header_declares_the_entry_points_and_keeps_the_abi_version():
    with open(os.path.join(ROOT, "include", "ifseg_hip.h")) as f:
        header = f.read()
    for name in ("ifseg_seg_areas", "ifseg_seg_score", "ifseg_seg_score_views"):
        assert re.search(r"^int %s\(" % name, header, re.M), name
    assert re.search(r"#define\s+IFSEG_ABI_VERSION\s+21\b", header) and hip.ABI_VERSION == 21


def _no_library(monkeypatch):
    def fail():
        raise RuntimeError("the library was reached")
    monkeypatch.setattr(hip, "lib", fail)


def test_bindings_refuse_before_they_launch(monkeypatch):
    _no_library(monkeypatch)
    lab, gt = torch.zeros(4, 6, dtype=torch.uint8), torch.zeros(4, 6, dtype=torch.uint8)
    for bad in ((lab.long(), gt), (lab, gt.long()), (lab[:, :5], gt), (lab, gt.t()), (lab.t(), gt.t())):
        with pytest.raises(AssertionError):
            hip.seg_areas(*bad, 5)
    for n in (0, 513):
        with pytest.raises(AssertionError):
            hip.seg_areas(lab, gt, n)
    with pytest.raises(AssertionError):
        hip.seg_areas(lab, gt, 5, areas=torch.zeros(3, 4, dtype=torch.int64))
    with pytest.raises(AssertionError):
        hip.seg_areas(lab, gt, 5, tally=torch.zeros(2, dtype=torch.int32))
    ok, g3 = torch.zeros(2, 6, 5), torch.zeros(2, 32, 48, dtype=torch.uint8)
    for bad in (ok.double(), ok.transpose(1, 2), ok[0]):
        with pytest.raises(AssertionError):
            hip.seg_score(bad, 2, 3, g3)
        with pytest.raises(AssertionError):
            hip.seg_score_views([(bad, 2, 3, False)], g3)
    for bad_gt in (g3.long(), g3[0], g3[:1], g3.transpose(1, 2)):
        with pytest.raises(AssertionError):
            hip.seg_score(ok, 2, 3, bad_gt)
        with pytest.raises(AssertionError):
            hip.seg_score_views([(ok, 2, 3, False)], bad_gt)
    with pytest.raises(AssertionError):
        hip.seg_score(ok, 2, 2, g3)                                                  # hp * wp != rows
    with pytest.raises(AssertionError):
        hip.seg_score(torch.zeros(1, 1, 513), 1, 1, g3[:1])                          # n > 512
    with pytest.raises(AssertionError):
        hip.seg_score(torch.zeros(1, 1, 257), 1, 1, g3[:1], labels=True, label_dtype=torch.uint8)
    with pytest.raises(AssertionError):
        hip.seg_score(ok, 2, 3, g3, areas=torch.zeros(3, 5))                         # float counters
    with pytest.raises(AssertionError):
        hip.seg_score_views([(ok, 2, 3, False)] * 17, g3)
    with pytest.raises(AssertionError):
        hip.seg_score_views([(ok, 2, 3, False), (torch.zeros(2, 6, 4), 2, 3, True)], g3)


class _Model(torch.nn.Linear):
    """as much of a model as the checks of evaluate_raw look at"""

    def __init__(self):
        super().__init__(1, 1)
        self.cfg = type("Cfg", (), {"num_seg_tokens": 5, "patch_image_size": 128})()


def test_evaluate_raw_refuses_before_it_launches(monkeypatch):
    _no_library(monkeypatch)
    monkeypatch.setattr(hip, "image_load", lambda *a, **k: (_ for _ in ()).throw(RuntimeError("image_load was reached")))
    seg = Segmenter(_Model(), category_token_ids=[[31], [32], [33], [34], [35]])
    im = [torch.zeros(60, 90, 3, dtype=torch.uint8), torch.zeros(64, 64, 3, dtype=torch.uint8)]
    gt = [torch.zeros(60, 90, dtype=torch.uint8), torch.zeros(64, 64, dtype=torch.int16)]
    with pytest.raises(ValueError, match="1 label maps for 2 images"):
        seg.evaluate_raw(im, gt[:1])
    with pytest.raises(ValueError, match="2 label maps for 1 images"):
        seg.evaluate_raw(im[0], gt)
    with pytest.raises(ValueError, match=r"label map 1 must be a uint8 or int16 tensor of its image's shape \(64, 64\)"):
        seg.evaluate_raw(im, [gt[0], gt[0]])
    with pytest.raises(ValueError, match="label map 0 must be a uint8 or int16 tensor"):
        seg.evaluate_raw(im, [gt[0].long(), gt[1]])
    with pytest.raises(ValueError, match="label map 1"):
        seg.evaluate_raw(im, [gt[0], gt[1].numpy()])
    with pytest.raises(ValueError, match="evaluate_raw: every image must be a uint8 RGB"):
        seg.evaluate_raw([im[0].float()], gt[:1])
    with pytest.raises(ValueError, match="into must be a SegmentationScore of 5 classes"):
        seg.evaluate_raw(im, gt, into=SegmentationScore(6))
    with pytest.raises(ValueError, match="evaluate_raw: 2 views need upsample='probs'"):
        Segmenter(_Model(), category_token_ids=[[31]] * 5, upsample="logits").evaluate_raw(im, gt, flip=True)
    with pytest.raises(ValueError, match="evaluate: label_maps must be a uint8 or int16 tensor"):
        seg.evaluate(torch.zeros(2, 3, 128, 128), torch.zeros(2, 128, 128))
    with pytest.raises(ValueError, match="evaluate: 3 label maps for images"):
        seg.evaluate(torch.zeros(2, 3, 128, 128), torch.zeros(3, 128, 128, dtype=torch.uint8))
    # nothing to score: an empty score, or `into` as it was
    empty = seg.evaluate_raw([], [])
    assert isinstance(empty, SegmentationScore) and not empty.areas.any() and empty.areas.shape == (3, 5)
    # segment_raw still names itself
    with pytest.raises(ValueError, match="segment_raw: every image must be a uint8 RGB"):
        seg.segment_raw([im[0].float()])


def test_ops_are_registered_with_fake_kernels():
    import ifseg_amd.ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    areas_op, score_op = torch.ops.ifseg.seg_areas, torch.ops.ifseg.seg_score_views
    with FakeTensorMode():
        lab = torch.empty(2, 9, 7, dtype=torch.uint8, device="cuda")
        gt = torch.empty(2, 9, 7, dtype=torch.int16, device="cuda")
        a, t = areas_op(lab, gt, 150, True)
        assert a.shape == (3, 150) and a.dtype == torch.int64 and t.shape == (2,) and t.dtype == torch.int64 and a.is_cuda
        with pytest.raises(Exception, match="labels must be uint8 or int16"):
            areas_op(lab.long(), gt, 150, True)
        with pytest.raises(Exception, match="ground truth must be uint8 or int16"):
            areas_op(lab, gt.long(), 150, True)
        with pytest.raises(Exception, match="must have one shape"):
            areas_op(lab[:1], gt, 150, True)
        with pytest.raises(Exception, match="n = 513 classes"):
            areas_op(lab, gt, 513, True)
        s = [torch.empty(2, 6, 300, device="cuda"), torch.empty(2, 24, 300, device="cuda")]
        args = (s, [2, 4], [3, 6], [False, True])
        a, t, l, c, p = score_op(*args, gt, False, True, False, True)
        assert a.shape == (3, 300) and t.shape == (2,) and l.shape == (2, 9, 7) and l.dtype == torch.int16
        assert c.numel() == 0 and p.shape == (2, 300, 9, 7)
        a, t, l, c, p = score_op(*args, gt, True, False, False, False)
        assert a.shape == (3, 300) and l.numel() == 0 and c.numel() == 0 and p.numel() == 0
        with pytest.raises(Exception, match="ground truth must be uint8 or int16"):
            score_op(*args, gt.float(), True, False, False, False)
        with pytest.raises(Exception, match=r"ground truth must be \[B, h, w\]"):
            score_op(*args, gt[0], True, False, False, False)
        with pytest.raises(Exception, match="for a batch of 2"):
            score_op(*args, gt[:1], True, False, False, False)
        with pytest.raises(Exception, match="scores must be fp32"):
            score_op([x.double() for x in s], *args[1:], gt, True, False, False, False)
