"""CPU: the specification of the class confusion matrix (`ifseg_amd.predict.confusion_reference`) against a plain double
loop, its four identities with `areas_reference`, and what `SegmentationScore` does with the matrix (`add_`, `confusions`,
`confusion_summary`, `merged`, `group_summary`), the header, the binding's and `evaluate_raw`'s refusals before anything
reaches the library, and the op's fake kernel.  The counters are integers: every comparison of counters is exact."""
import os
import re

import pytest
import torch

import _score_cases as SC
from ifseg_amd import hip
from ifseg_amd.predict import SegmentationScore, Segmenter, areas_reference, confusion_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(1, torch.uint8), (5, torch.uint8), (5, torch.int16), (150, torch.uint8), (150, torch.int16), (257, torch.int16)]


def _with_outside(labels, n, seed=0):
    """some predictions outside [0, n): negative, n itself, far beyond"""
    g = torch.Generator().manual_seed(6000 + seed)
    out = labels.clone().reshape(-1)
    where = torch.randperm(out.numel(), generator=g)[:out.numel() // 7]
    out[where] = torch.tensor([-1, n, n + 3, 255, -300, 32767])[torch.randint(0, 6, (where.numel(),), generator=g)]
    return out.reshape(labels.shape)


def _double_loop(labels, gt, n, raw_labels):
    C = [[0] * (n + 1) for _ in range(n)]
    for p, v in zip(labels.reshape(-1).tolist(), gt.reshape(-1).tolist()):
        c = SC.kind(v, n, raw_labels)
        if c >= 0:
            C[c][p if 0 <= p < n else n] += 1
    return torch.tensor(C, dtype=torch.int64).reshape(n, n + 1)


@pytest.mark.parametrize("raw_labels", [True, False], ids=["raw", "ids"])
@pytest.mark.parametrize("n,dtype", [(1, torch.uint8), (5, torch.uint8), (5, torch.int16), (40, torch.int16), (150, torch.uint8)])
def test_confusion_reference_is_the_double_loop(n, dtype, raw_labels):
    labels, gt = SC.labels_and_gt(n, raw_labels, dtype, size=(23, 19))
    present = {SC.kind(int(v), n, raw_labels) for v in gt.reshape(-1)}
    assert -1 in present and -2 in present and 0 in present                          # every kind of ground truth is there
    labels = _with_outside(labels, n)
    assert ((labels < 0) | (labels >= n)).any()
    C = confusion_reference(labels, gt, n, raw_labels)
    assert C.dtype == torch.int64 and C.shape == (n, n + 1)
    assert torch.equal(C, _double_loop(labels, gt, n, raw_labels))
    assert int(C[:, n].sum()) > 0 and int(C[:, :n].sum()) > 0
    # any shape and any integer dtype of labels, as areas_reference
    D = confusion_reference(labels.to(torch.int16).reshape(19, 23), gt.reshape(19, 23), n, raw_labels)
    assert torch.equal(C, D)


@pytest.mark.parametrize("outside", [False, True], ids=["inside", "outside"])
@pytest.mark.parametrize("raw_labels", [True, False], ids=["raw", "ids"])
@pytest.mark.parametrize("n,dtype", CASES)
def test_four_identities_with_areas_reference(n, dtype, raw_labels, outside):
    labels, gt = SC.labels_and_gt(n, raw_labels, dtype)
    if outside:
        labels = _with_outside(labels, n, 1)
    areas, tally = areas_reference(labels, gt, n, raw_labels)
    C = confusion_reference(labels, gt, n, raw_labels)
    assert int(C.sum()) == int(tally[0]) > 0
    assert torch.equal(C[:, :n].diagonal(), areas[0])
    assert torch.equal(C[:, :n].sum(0), areas[1])
    assert torch.equal(C.sum(1), areas[2])
    assert bool(C[:, n].any()) == (outside and n > 0)


def test_confusion_reference_refusals_are_areas_reference_s():
    labels, gt = SC.labels_and_gt(5, True, torch.uint8)
    with pytest.raises(ValueError, match="confusion_reference: ground truth must be uint8 or int16"):
        confusion_reference(labels, gt.long(), 5)
    with pytest.raises(ValueError, match="confusion_reference: labels must be integer"):
        confusion_reference(labels.float(), gt, 5)
    with pytest.raises(ValueError, match="shape"):
        confusion_reference(labels[0], gt, 5)


def _score(n, seed, raw=True, dtype=torch.uint8, confusion=True, outside=True):
    """a score of one random map without ground truth out of range -> (score, labels, gt)"""
    labels, gt = SC.labels_and_gt(n, raw, dtype, seed=seed)
    cls = torch.tensor([SC.kind(int(v), n, raw) for v in gt.reshape(-1)]).reshape(gt.shape)
    gt = torch.where(cls == -2, torch.full_like(gt, 255), gt)
    if outside:
        labels = _with_outside(labels, n, seed)
    areas, tally = areas_reference(labels, gt, n, raw)
    assert int(tally[1]) == 0
    return SegmentationScore(n, areas=areas, tally=tally,
                             confusion=confusion_reference(labels, gt, n, raw) if confusion else None), labels, gt


def test_score_constructor_and_add():
    s = SegmentationScore(7)
    assert s.confusion is None and SegmentationScore(7, confusion=False).confusion is None
    t = SegmentationScore(7, torch.device("cpu"), confusion=True)
    assert t.confusion.dtype == torch.int64 and t.confusion.shape == (7, 8) and not t.confusion.any()
    given = torch.zeros(7, 8, dtype=torch.int64)
    assert SegmentationScore(7, confusion=given).confusion is given
    for bad in (torch.zeros(7, 7, dtype=torch.int64), torch.zeros(7, 8, dtype=torch.int32), torch.zeros(8, 8, dtype=torch.int64),
                torch.zeros(7, 8), [[0] * 8] * 7, 1):
        with pytest.raises(ValueError, match=r"confusion must be None, True or int64 \[7, 8\]"):
            SegmentationScore(7, confusion=bad)
    a, b = _score(7, 1)[0], _score(7, 2)[0]
    tot = SegmentationScore(7, confusion=True).add_(a).add_(b)
    assert torch.equal(tot.confusion, a.confusion + b.confusion) and torch.equal(tot.areas, a.areas + b.areas)
    assert torch.equal(tot.tally, a.tally + b.tally)
    # without matrices: as ever
    c, d = _score(7, 1, confusion=False)[0], _score(7, 2, confusion=False)[0]
    plain = SegmentationScore(7).add_(c).add_(d)
    assert plain.confusion is None and torch.equal(plain.areas, tot.areas) and repr(plain.summary()) == repr(tot.summary())
    # one with and one without is refused, either way round, and nothing is added
    keep = tot.areas.clone()
    with pytest.raises(ValueError, match="confusion matrix"):
        tot.add_(c)
    with pytest.raises(ValueError, match="confusion matrix"):
        plain.add_(a)
    assert torch.equal(tot.areas, keep)
    for call in (lambda: plain.confusions(), lambda: plain.confusion_summary(), lambda: plain.merged([0] * 7)):
        with pytest.raises(ValueError, match="needs a confusion matrix"):
            call()


def test_confusions_lists_the_largest_off_diagonal_entries():
    C = torch.tensor([[50, 3, 0, 7],
                      [9, 10, 0, 1],
                      [0, 0, 0, 0]])
    s = SegmentationScore(3, confusion=C.clone())
    got = s.confusions()
    assert got == [(1, 0, 9, 9 / 20), (0, 3, 7, 7 / 60), (0, 1, 3, 3 / 60), (1, 3, 1, 1 / 20)]
    assert s.confusions(2) == got[:2] and s.confusions(0) == []
    # the default is ten, and the diagonal is never listed
    score, labels, gt = _score(40, 3, dtype=torch.int16)
    top = score.confusions()
    assert len(top) == 10 and all(c != p for c, p, _, _ in top)
    off = score.confusion.clone()
    off[:, :40].fill_diagonal_(0)
    assert [v for _, _, v, _ in top] == sorted(off.reshape(-1).tolist(), reverse=True)[:10]
    assert all(v == int(off[c, p]) and share == v / int(score.areas[2][c]) for c, p, v, share in top)


def test_confusion_summary_normalises_rows_and_leaves_absent_classes_nan():
    C = torch.tensor([[50, 3, 0, 7],
                      [9, 10, 0, 1],
                      [0, 0, 0, 0]])
    R = SegmentationScore(3, confusion=C).confusion_summary()
    assert R.dtype == torch.float64 and R.shape == (3, 4)
    assert torch.equal(R[:2], C[:2].double() / torch.tensor([[60.0], [20.0]]))
    assert torch.isnan(R[2]).all() and not torch.isnan(R[:2]).any()
    score = _score(7, 4)[0]
    acc = score.summary()["Acc"]
    assert [round(float(v), 4) for v in score.confusion_summary()[:, :7].diagonal()] == acc


def _mapped(labels, gt, mapping, n, m, raw):
    """the label maps under `mapping`: predictions outside [0, n) stay outside (-1), dropped classes become -1 in the labels
    and m ('unknown' under raw_labels=False) in the ground truth, as do the ignore values; nothing here is out of range"""
    mp = torch.tensor(mapping)
    inside = (labels >= 0) & (labels < n)
    new_labels = torch.where(inside, mp[labels.clamp(0, n - 1)], torch.full_like(labels, -1))
    cls = torch.tensor([SC.kind(int(v), n, raw) for v in gt.reshape(-1)]).reshape(gt.shape)
    assert (cls != -2).all()
    to = mp[cls.clamp(0, n - 1)]
    new_gt = torch.where((cls < 0) | (to < 0), torch.full_like(to, m), to).to(torch.int16)
    return new_labels, new_gt


MAPPINGS = {"many_to_one": ([0, 0, 1, 2, 1, 0, 2], 3), "with_drop": ([1, -1, 0, 1, -1, 2, 0], 3), "identity": (list(range(7)), 7),
            "gap": ([0, 3, 3, 0, 3, 0, 0], 4)}


@pytest.mark.parametrize("raw", [True, False], ids=["raw", "ids"])
@pytest.mark.parametrize("name", list(MAPPINGS))
def test_merged_is_scoring_the_mapped_maps(name, raw):
    mapping, m = MAPPINGS[name]
    n = 7
    score, labels, gt = _score(n, 5, raw, torch.int16)
    got = score.merged(mapping)
    assert isinstance(got, SegmentationScore) and got.n == m and got is not score
    new_labels, new_gt = _mapped(labels, gt, mapping, n, m, raw)
    want = confusion_reference(new_labels, new_gt, m, raw_labels=False)
    assert got.confusion.dtype == torch.int64 and torch.equal(got.confusion, want)
    areas, tally = areas_reference(new_labels, new_gt, m, raw_labels=False)
    assert torch.equal(got.areas, areas) and torch.equal(got.tally, tally)
    assert repr(got.summary()) == repr(SegmentationScore(m, areas=areas, tally=tally).summary())     # repr: NaN equals NaN
    if name == "identity":
        assert torch.equal(got.confusion, score.confusion) and torch.equal(got.areas, score.areas) and repr(got.summary()) == repr(score.summary())
    if name == "with_drop":
        assert int(got.tally[0]) < int(score.tally[0]) and int(got.confusion[:, m].sum()) > int(score.confusion[:, n].sum())
    # a tensor is a mapping too, and m may be given: empty classes behind the last id
    wide = score.merged(torch.tensor(mapping), m=m + 2)
    assert wide.n == m + 2 and torch.equal(wide.confusion[:m, :m], got.confusion[:, :m]) and not wide.confusion[m:].any()
    assert torch.equal(wide.confusion[:m, m + 2], got.confusion[:, m])


def test_merged_carries_tally_1_and_refuses_bad_mappings():
    score = _score(7, 6)[0]
    score.tally[1] = 4
    assert score.merged([0] * 7).tally.tolist() == [int(score.tally[0]), 4]
    for bad in ([0] * 6, [0.0] * 7, [0, 0, 0, 0, 0, 0, -2]):
        with pytest.raises(ValueError, match="merged"):
            score.merged(bad)
    with pytest.raises(ValueError, match=r"in \[0, 2\)"):
        score.merged([0, 1, 2, 0, 0, 0, 0], m=2)


def test_group_summary_is_the_formula_on_summary_s_per_class_values():
    n = 9
    # per-class IoU and Acc that four digits hold exactly, so that the formula on summary()'s rounded lists is exact: the
    # classes' (intersect, predicted, label) pixels; class 8 is absent (NaN), class 7 is never found (IoU 0)
    per_class = [(1, 3, 2), (2, 6, 4), (1, 1, 4), (3, 6, 5), (5, 5, 5), (1, 7, 4), (2, 2, 2), (0, 3, 5), (0, 0, 0)]
    areas = torch.tensor(per_class).t().contiguous()
    score = SegmentationScore(n, areas=areas, tally=torch.tensor([int(areas[2].sum()), 0]))
    s = score.summary()
    assert all(v != v or abs(v * 10000 - round(v * 10000)) < 1e-9 for v in s["IoU"] + s["Acc"])
    assert s["IoU"][:4] == [0.25, 0.25, 0.25, 0.375] and s["Acc"][:4] == [0.5, 0.5, 0.25, 0.6]
    groups = {"seen": [0, 1, 2, 3, 8], "unseen": [4, 5, 6], "tail": (7, 2)}
    got = score.group_summary(groups)
    assert list(got) == ["seen", "unseen", "tail", "hIoU"]
    iou, acc = torch.tensor(s["IoU"], dtype=torch.float64), torch.tensor(s["Acc"], dtype=torch.float64)
    mious = []
    for name, ids in groups.items():
        mious.append(float(torch.nanmean(iou[list(ids)])))
        assert got[name] == {"mIoU": round(mious[-1], 4), "mAcc": round(float(torch.nanmean(acc[list(ids)])), 4)}, name
    assert got["hIoU"] == round(3 / sum(1 / v for v in mious), 4) and min(mious) - 1e-4 <= got["hIoU"] <= max(mious) + 1e-4
    # all classes in one group: summary()'s own means
    whole = score.group_summary({"all": range(n)})
    assert whole["all"] == {"mIoU": s["mIoU"], "mAcc": s["mAcc"]} and whole["hIoU"] == s["mIoU"]
    # a group whose mIoU is 0 takes the harmonic mean to 0; a group of absent classes is NaN, and so is hIoU
    assert score.group_summary({"a": [0], "none": [7]})["hIoU"] == 0.0
    absent = score.group_summary({"a": [0], "absent": [8]})
    assert absent["absent"]["mIoU"] != absent["absent"]["mIoU"] and absent["hIoU"] != absent["hIoU"]
    # a random score: the group means are taken over unrounded values as summary()'s are, so the formula on the rounded
    # lists is within one step of the fourth digit (5e-5 from the inputs' rounding, and the rounding of the result)
    rnd = _score(40, 7, dtype=torch.int16, confusion=False)[0]
    rs, halves = rnd.summary(), {"low": range(0, 20), "high": range(20, 40)}
    rg = rnd.group_summary(halves)
    for name, ids in halves.items():
        by_hand = float(torch.nanmean(torch.tensor(rs["IoU"], dtype=torch.float64)[list(ids)]))
        assert abs(rg[name]["mIoU"] - by_hand) <= 1e-4 + 1e-12, (name, rg[name], by_hand)
    a = rnd.areas.double()
    exact = [float(torch.nanmean((a[0] / (a[1] + a[2] - a[0]))[list(ids)])) for ids in halves.values()]
    assert [rg["low"]["mIoU"], rg["high"]["mIoU"]] == [round(v, 4) for v in exact]
    assert rg["hIoU"] == round(2 / (1 / exact[0] + 1 / exact[1]), 4)
    # refusals: class ids out of range, an empty group, the reserved name; ground truth out of range as summary()
    for bad in ({"a": [0, 9]}, {"a": [-1]}, {"a": []}, {"hIoU": [0]}):
        with pytest.raises(ValueError, match="group_summary"):
            score.group_summary(bad)
    score.tally[1] = 3
    with pytest.raises(IndexError, match=r"tally\[1\] = 3"):
        score.group_summary({"a": [0]})


def test_header_declares_the_entry_point_and_keeps_the_abi_version():
    with open(os.path.join(ROOT, "include", "ifseg_hip.h")) as f:
        header = f.read()
    assert re.search(r"^int ifseg_seg_confusion\(", header, re.M)
    assert re.search(r"#define\s+IFSEG_ABI_VERSION\s+21\b", header) and hip.ABI_VERSION == 21
    assert callable(hip.seg_confusion)
    with open(os.path.join(ROOT, "ifseg_amd", "csrc", "predict.hip")) as f:
        src = f.read()
    with open(os.path.join(ROOT, "ifseg_amd", "csrc", "count.h")) as f:      # the walk and the hashed table, namespace count
        shared = f.read()
    # the exported constants are the kernel's
    assert int(re.search(r"constexpr int SC_DIRECT_MAX = (\d+);", src).group(1)) == hip.SEG_CONFUSION_DIRECT_MAX
    assert 1 << int(re.search(r"constexpr int SLOT_BITS = (\d+);", shared).group(1)) == hip.SEG_CONFUSION_SLOTS
    assert re.search(r"^int ifseg_seg_confusion_limit\(int which\);", header, re.M) and callable(hip.seg_confusion_limits)
    assert int(re.search(r"constexpr int MAX_BLOCKS = (\d+);", shared).group(1)) == hip.SEG_CONFUSION_MAX_BLOCKS
    assert hip.SEG_CONFUSION_STEP_PIXELS == 256 * 16
    # and the loaded library states the same four
    assert hip.seg_confusion_limits() == (hip.SEG_CONFUSION_DIRECT_MAX, hip.SEG_CONFUSION_SLOTS, hip.SEG_CONFUSION_STEP_PIXELS,
                                          hip.SEG_CONFUSION_MAX_BLOCKS)
    assert hip.lib().ifseg_seg_confusion_limit(4) == -3 and hip.lib().ifseg_seg_confusion_limit(-1) == -3
    assert 127 * 128 <= hip.SEG_CONFUSION_DIRECT_MAX < 128 * 129 and hip.SEG_CONFUSION_DIRECT_MAX * 4 <= 65536
    assert 2 * hip.SEG_CONFUSION_SLOTS * 4 <= 65536


def _no_library(monkeypatch):
    def fail():
        raise RuntimeError("the library was reached")
    monkeypatch.setattr(hip, "lib", fail)


def test_binding_refuses_before_it_launches(monkeypatch):
    _no_library(monkeypatch)
    lab, gt = torch.zeros(4, 6, dtype=torch.uint8), torch.zeros(4, 6, dtype=torch.uint8)
    for bad in ((lab.long(), gt), (lab, gt.long()), (lab[:, :5], gt), (lab, gt.t()), (lab.t(), gt.t())):
        with pytest.raises(AssertionError):
            hip.seg_confusion(*bad, 5)
    for n in (0, 513):
        with pytest.raises(AssertionError):
            hip.seg_confusion(lab, gt, n)
    with pytest.raises(AssertionError):
        hip.seg_confusion(lab[:0], gt[:0], 5)
    for bad in (torch.zeros(5, 5, dtype=torch.int64), torch.zeros(5, 6, dtype=torch.int32), torch.zeros(6, 5, dtype=torch.int64).t()):
        with pytest.raises(AssertionError):
            hip.seg_confusion(lab, gt, 5, confusion=bad)


class _Model(torch.nn.Linear):
    """as much of a model as the checks of evaluate_raw look at"""

    def __init__(self):
        super().__init__(1, 1)
        self.cfg = type("Cfg", (), {"num_seg_tokens": 5, "patch_image_size": 128})()


def test_evaluate_raw_refuses_a_matrixless_into_before_it_launches(monkeypatch):
    _no_library(monkeypatch)
    monkeypatch.setattr(hip, "image_load", lambda *a, **k: (_ for _ in ()).throw(RuntimeError("image_load was reached")))
    seg = Segmenter(_Model(), category_token_ids=[[31], [32], [33], [34], [35]])
    im, gt = [torch.zeros(60, 90, 3, dtype=torch.uint8)], [torch.zeros(60, 90, dtype=torch.uint8)]
    with pytest.raises(ValueError, match="evaluate_raw: confusion=True, but `into` carries no confusion matrix"):
        seg.evaluate_raw(im, gt, into=SegmentationScore(5), confusion=True)
    for bad in (torch.zeros(5, 6, dtype=torch.int64), 1, None):
        with pytest.raises(ValueError, match="evaluate_raw: confusion must be True or False"):
            seg.evaluate_raw(im, gt, confusion=bad)
    with pytest.raises(ValueError, match="evaluate: confusion=True, but `into` carries no confusion matrix"):
        seg.evaluate(torch.zeros(1, 3, 128, 128), torch.zeros(1, 128, 128, dtype=torch.uint8), into=SegmentationScore(5), confusion=True)
    # nothing to score: the empty score has a matrix when asked for one, and `into` comes back as it was
    empty = seg.evaluate_raw([], [], confusion=True)
    assert empty.confusion.shape == (5, 6) and not empty.confusion.any() and seg.evaluate_raw([], []).confusion is None
    into = SegmentationScore(5, confusion=True)
    assert seg.evaluate_raw([], [], into=into) is into and seg.evaluate_raw([], [], into=into, confusion=True) is into


def test_op_is_registered_with_a_fake_kernel():
    import ifseg_amd.ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    op = torch.ops.ifseg.seg_confusion
    with FakeTensorMode():
        lab = torch.empty(2, 9, 7, dtype=torch.uint8, device="cuda")
        gt = torch.empty(2, 9, 7, dtype=torch.int16, device="cuda")
        for n in (1, 150, 512):
            C = op(lab, gt, n, True)
            assert C.shape == (n, n + 1) and C.dtype == torch.int64 and C.is_cuda
        with pytest.raises(Exception, match="seg_confusion: labels must be uint8 or int16"):
            op(lab.long(), gt, 150, True)
        with pytest.raises(Exception, match="seg_confusion: ground truth must be uint8 or int16"):
            op(lab, gt.long(), 150, True)
        with pytest.raises(Exception, match="must have one shape"):
            op(lab[:1], gt, 150, True)
        with pytest.raises(Exception, match="n = 513 classes"):
            op(lab, gt, 513, False)
        with pytest.raises(Exception, match="n = 0 classes"):
            op(lab, gt, 0, False)
        with pytest.raises(Exception, match="pixels"):
            op(lab[:0], gt[:0], 5, True)
