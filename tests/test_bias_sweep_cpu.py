"""CPU: the per-class bias and its sweep -- `predict.bias_sweep_reference` against a literal transcription, `scaled_bias`'s two
roundings, `SegmentationScore.overprediction`, `BiasSweep`, a known answer, which launches a Segmenter makes with and without
`class_bias` and in `bias_sweep_raw` / `bias_sweep` (recording fakes, as tests/test_temperature_sweep_cpu.py), every refusal,
and the surface: the C entries on host memory, the header, the limits, the task."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import _bias_sweep_cases as BC
from ifseg_amd import hip
from ifseg_amd.predict import (BiasSweep, Segmenter, SegmentationScore, areas_reference, bias_sweep_reference,
                               default_bias_strengths, first_maximum, scaled_bias, upsample_argmax_reference)
from test_segmenter_launches_cpu import A, B, N, _Model, _images
from test_temperature_sweep_cpu import SweepRecorder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_SHAPE, BAD_ARG = -2, -3
LITERAL = ("small_ids_i16_oor", "small_raw_u8_oor", "small_down_ids_u8", "n1", "ragged_k1", "identity")


# ------------------------------------------------------------------------------------------------- the rule
def test_default_bias_strengths():
    g = default_bias_strengths()
    assert len(g) == 16 == hip.SEG_SCORE_GRIDS_MAX and g[0] == 0.0 and g[1] == 0.25 and g[-1] == 3.75
    assert all(a < b for a, b in zip(g, g[1:]))


@pytest.mark.parametrize("name", LITERAL)
def test_reference_is_the_literal_rule(name):
    """both raw_labels settings, uint8 and int16 ground truth, ignore values, an out-of-range value, n = 1, up- and
    downscaling, logit-like grids with negative values, the tie and the two NaN pixels: every counter exactly"""
    grids, gt, (hp, wp, n, raw), where = BC.make(name)
    areas, tally = bias_sweep_reference(grids, hp, wp, gt, raw)
    want_a, want_t = BC.literal(grids, hp, wp, gt, raw)
    K = grids.shape[0]
    assert areas.dtype == torch.int64 and areas.shape == (K, 3, n) and tally.dtype == torch.int64 and tally.shape == (2,)
    assert torch.equal(tally, want_t) and int(tally[0]) > 0 and (int(tally[1]) > 0) == {**BC.KINDS, **BC.SMALL_KINDS}[name][2]
    assert torch.equal(areas, want_a)
    assert areas[:, 1].sum(1).tolist() == areas[:, 2].sum(1).tolist() == [int(tally[0])] * K
    # a sequence of K grids is the stacked tensor; row k is areas_reference of grid k's labels
    seq = bias_sweep_reference([g for g in grids], hp, wp, gt, raw)
    assert torch.equal(seq[0], areas) and torch.equal(seq[1], tally)
    h, w = gt.shape[1:]
    for k in range(K):
        labels = first_maximum(upsample_argmax_reference(grids[k], hp, wp, h, w)[2])
        assert torch.equal(areas_reference(labels, gt, n, raw)[0], areas[k])
        for kind, (y, x, t) in where.items():
            assert int(labels[0, y, x]) == {"tie": t - 1, "nan": 0, "allnan": 0}[kind], (kind, k)
    with pytest.raises(ValueError, match="no strengths"):
        bias_sweep_reference([], hp, wp, gt, raw)
    with pytest.raises(ValueError, match=r"must be \[B, h, w\]"):
        bias_sweep_reference(grids, hp, wp, gt[0], raw)


def test_first_maximum_is_argmax_but_for_nan():
    v = torch.randn(2, 7, 5, 6)
    assert torch.equal(first_maximum(v), v.argmax(1))
    v[0, 3, 1, 1] = float("nan")
    v[1, :, 2, 2] = float("nan")
    v[0, 2:4, 4, 4] = 9.0
    lab = first_maximum(v)
    assert int(lab[0, 1, 1]) != 3 and int(lab[1, 2, 2]) == 0 and int(lab[0, 4, 4]) == 2


def test_scaled_bias_is_one_product_and_one_sum():
    g = torch.Generator().manual_seed(3)
    d, o = torch.randn(64, generator=g) * 3, torch.randn(64, generator=g)
    for s in (0.3, -1.7, 1e-3, 2.25, 0.0, 1 / 3):
        prod = d.numpy() * np.float32(s)
        assert prod.dtype == np.float32
        assert np.array_equal(scaled_bias(d, s).numpy().view(np.int32), prod.view(np.int32))
        want = prod + o.numpy()
        assert np.array_equal(scaled_bias(d, s, o).numpy().view(np.int32), want.view(np.int32))
        # a wider direction is rounded to fp32 first, a sequence is taken as it is
        assert torch.equal(scaled_bias(d.double(), s, o.double()), scaled_bias(d, s, o))
        assert torch.equal(scaled_bias(d.tolist(), s), scaled_bias(d, s))
    z = scaled_bias(d.abs(), 0)
    assert z.dtype == torch.float32 and torch.equal(z.view(torch.int32), torch.zeros(64, dtype=torch.int32))     # +0.0 exactly


def test_overprediction_hand_values():
    areas = torch.tensor([[1, 0, 0, 0], [3, 0, 7, 0], [1, 5, 0, 0]])
    score = SegmentationScore(4, areas=areas)
    o = score.overprediction()
    assert o.dtype == torch.float64 and o.shape == (4,) and o.device == areas.device
    want = [math.log(4) - math.log(2), -math.log(6), math.log(8), 0.0]
    assert torch.allclose(o, torch.tensor(want, dtype=torch.float64), rtol=1e-15, atol=0.0) and float(o[3]) == 0.0


# ------------------------------------------------------------------------------------------------- the sweep object
def _filled(strengths, n, seed, groups_have_pixels=True):
    g = torch.Generator().manual_seed(seed)
    sweep = BiasSweep(strengths, torch.randn(n, generator=g), torch.randn(n, generator=g))
    K = len(strengths)
    label = torch.randint(1, 200, (n,), generator=g)
    inter = torch.stack([(label * torch.rand(n, generator=g)).long() for _ in range(K)])
    extra = torch.randint(0, 50, (K, n), generator=g)
    # predicted = intersection + false positives, padded so that every row predicts as many pixels as are labelled
    pred = inter + extra
    pred[:, 0] += int(label.sum()) + 50 * n - pred.sum(1)
    sweep.areas += torch.stack([inter, pred, label.expand(K, n)], 1)
    sweep.tally[0] = int(label.sum())
    return sweep


def test_summary_and_best_are_the_rows_scores():
    gs = (0.0, 0.5, 1.0, -0.25)
    sweep = _filled(gs, 6, 11)
    groups = {"seen": [0, 1, 2, 3], "unseen": [4, 5]}
    s, sg = sweep.summary(), sweep.summary(groups)
    assert s["strengths"] == list(gs) and s["pixels"] == int(sweep.tally[0]) and set(s) == {"strengths", "mIoU", "mAcc", "aAcc", "IoU", "pixels"}
    for k in range(len(gs)):
        sc = sweep.score(k)
        assert isinstance(sc, SegmentationScore) and sc.areas.data_ptr() == sweep.areas[k].data_ptr() and sc.tally is sweep.tally
        one, grp = sc.summary(), sc.group_summary(groups)
        assert (s["mIoU"][k], s["mAcc"][k], s["aAcc"][k], s["IoU"][k]) == (one["mIoU"], one["mAcc"], one["aAcc"], one["IoU"])
        assert sg["seen"]["mIoU"][k] == grp["seen"]["mIoU"] and sg["unseen"]["mIoU"][k] == grp["unseen"]["mIoU"]
        assert sg["seen"]["mAcc"][k] == grp["seen"]["mAcc"] and sg["hIoU"][k] == grp["hIoU"]
        ak = sweep.areas[k].double()
        assert torch.equal(sc.overprediction(), torch.log(ak[1] + 1.0) - torch.log(ak[2] + 1.0))
    with pytest.raises(ValueError, match="needs a confusion matrix"):             # the sweep counts none
        sweep.score(0).merged([0, 0, 1, 1, 2, 2])
    for metric, vals in (("mIoU", s["mIoU"]), ("mAcc", s["mAcc"]), ("aAcc", s["aAcc"])):
        assert sweep.best(metric) == gs[max(range(4), key=lambda k: vals[k])]
    assert sweep.best("hIoU", groups) == gs[max(range(4), key=lambda k: sg["hIoU"][k])]
    assert sweep.best("unseen", groups) == gs[max(range(4), key=lambda k: sg["unseen"]["mIoU"][k])]
    # sharing memory: what is scored into a row's score shows in the sweep
    sweep.score(2).areas[0, 0] += 1
    assert sweep.summary()["IoU"][2][0] != s["IoU"][2][0]
    for metric, grp in (("hIoU", None), ("seen", None), ("IoU", None), ("other", groups), (3, None)):
        with pytest.raises(ValueError, match="metric must be one of"):
            sweep.best(metric, grp)
    for bad in ({"hIoU": [0]}, {"mIoU": [0]}, {"a": []}, {"a": [6]}, {"a": [-1]}):
        with pytest.raises(ValueError, match="group .* must hold class ids"):
            sweep.summary(bad)


def test_best_takes_the_first_of_equal_rows_and_refuses_without_pixels():
    sweep = BiasSweep((2.0, 0.5, 1.0, 1.5), [1.0, 0.0, 0.0])
    assert sweep.n == 3 and torch.equal(sweep.origin, torch.zeros(3)) and sweep.direction.dtype == torch.float32
    with pytest.raises(ValueError, match="no scored pixels"):
        sweep.best()
    assert sweep.summary()["pixels"] == 0 and math.isnan(sweep.summary()["mIoU"][0])
    low, high = torch.tensor([[1, 1, 1], [4, 3, 3], [3, 3, 4]]), torch.tensor([[3, 2, 3], [3, 3, 4], [3, 3, 4]])
    sweep.areas += torch.stack([low, high, high, low])
    sweep.tally[0] = 10
    assert sweep.best() == 0.5 and sweep.best("aAcc") == 0.5 and sweep.best("mAcc") == 0.5
    # ground truth out of range raises, as SegmentationScore.summary does
    sweep.tally[1] = 2
    for call in (sweep.summary, sweep.best, sweep.score(0).summary):
        with pytest.raises(IndexError, match=r"tally\[1\] = 2"):
            call()


def test_bias_rows_add_and_refusals():
    d, o = torch.tensor([1.0, -2.0, 0.5]), torch.tensor([0.25, 0.0, -1.0])
    gs = (0.0, 0.3, -1.0)
    a, b = BiasSweep(gs, d, o), BiasSweep(gs, d.double(), o.tolist())
    assert a.strengths == gs and a.n == 3 and a.areas.shape == (3, 3, 3) and a.tally.shape == (2,)
    for k, g in enumerate(gs):
        assert torch.equal(a.bias(k), scaled_bias(d, g, o)) and torch.equal(a.bias(g), a.bias(k))
    assert torch.equal(a.bias(0), o)                              # strength 0 is the origin
    for bad in (3, -1, 0.7, True, "0", None):
        with pytest.raises(ValueError, match="BiasSweep.bias"):
            a.bias(bad)
    for bad in (3, -1, 1.0, True):
        with pytest.raises(ValueError, match="k must be an int"):
            a.score(bad)
    a.areas[1, 1, 2], b.areas[1, 1, 2], b.tally[0] = 5, 7, 4
    assert a.add_(b) is a and int(a.areas[1, 1, 2]) == 12 and a.tally.tolist() == [4, 0]
    nudged = d.clone()
    nudged[1] = torch.nextafter(nudged[1], torch.tensor(0.0))
    for other, match in ((BiasSweep((0.0, 0.3), d, o), "different lists do not add"), (BiasSweep(gs, nudged, o), "direction or origin differ"),
                         (BiasSweep(gs, d), "direction or origin differ"), (BiasSweep(gs, d[:2], o[:2]), "2 classes against 3"),
                         ("sweep", "a BiasSweep is needed")):
        with pytest.raises(ValueError, match=match):
            a.add_(other)
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="a sweep on"):
            a.add_(BiasSweep(gs, d, o, "cuda:0"))
    for bad in ((), tuple(range(17)), (1.0, float("inf")), (float("nan"),), (True,), ("1",), 3.0):
        with pytest.raises(ValueError, match="strengths"):
            BiasSweep(bad, d)
    for bad in ([], 3.0, [1.0, float("nan")], [1.0, float("inf")], "abc", [[1.0, 2.0]], torch.zeros(2, 2), torch.tensor([True, False])):
        with pytest.raises(ValueError, match="direction"):
            BiasSweep(gs, bad)
    with pytest.raises(ValueError, match="origin"):
        BiasSweep(gs, d, [0.0, 1.0])


def test_known_answer():
    """n = 5 on a 6 x 7 grid at identity size; z = 2 onehot(t) with 3 added to class 0: class 0 is over-predicted by 3, wins
    everywhere up to and including the exact tie at strength 1.0, every pixel is right from 1.5 to 5.0, and at 5.5 class 0
    has sunk below the others' zeros on its own pixels"""
    n, hp, wp = 5, 6, 7
    t = torch.randint(0, 5, (hp, wp), generator=torch.Generator().manual_seed(0))
    t[0, :5] = torch.arange(5)
    z = 2.0 * torch.nn.functional.one_hot(t.reshape(-1), n).float()[None]
    z[..., 0] += 3
    d = torch.tensor([1.0, 0, 0, 0, 0])
    gs = tuple(j / 2 for j in range(12))
    grids = torch.stack([torch.softmax(z - scaled_bias(d, g), -1) for g in gs])
    gt = t[None].to(torch.uint8)
    for dtype in (torch.float32, torch.float64):
        sweep = BiasSweep(gs, d)
        areas, tally = bias_sweep_reference(grids, hp, wp, gt, raw_labels=False, dtype=dtype)
        sweep.areas += areas
        sweep.tally += tally
        s = sweep.summary()
        assert s["pixels"] == 42
        assert s["mIoU"] == [0.0238] * 3 + [1.0] * 8 + [0.7375]
        assert sweep.best("mIoU") == 1.5 and sweep.best("aAcc") == 1.5
        assert torch.equal(sweep.bias(sweep.best()), torch.tensor([1.5, 0, 0, 0, 0]))
    # the data-driven direction points at the same class
    over = SegmentationScore(n, areas=sweep.areas[0], tally=sweep.tally).overprediction()
    assert int(over.argmax()) == 0 and bool((over[1:] < 0).all())


# ------------------------------------------------------------------------------------------------- which launches
class BiasRecorder(SweepRecorder):
    """the SweepRecorder with the biased names recorded too; the plain names keep their fixed signatures, so a call that hands
    them a bias fails"""

    def __init__(self, monkeypatch):
        super().__init__(monkeypatch)
        monkeypatch.setattr(hip, "rows_to_f32_biased", self.rows_to_f32_biased)
        monkeypatch.setattr(hip, "neighbour_smoothing", self.smoothing)
        monkeypatch.setattr(hip, "seg_score_grids", self.score_grids)
        monkeypatch.setattr(Segmenter, "patch_scores", _PATCH_SCORES)

    def rows_to_f32_biased(self, pad, nseg, rows, bias, softmax=False, temperature=1.0):
        items = [self.tag(p)[0][1:] for p in pad]
        assert nseg == N and all(self.tag(p)[0][0] == "pad" for p in pad) and bias.dtype == torch.float32 and bias.shape == (N,)
        self.log.append(("rows_to_f32_biased", items, bias.tolist(), softmax, temperature))
        return torch.stack([self.coded((it, tuple(bias.tolist())), rows, N) for it in items])

    def smoothing(self, pad, nseg, feat, iters, topk, temperature=1.0, **kw):
        if not kw:
            return self.neighbour_smoothing(pad, nseg, feat, iters, topk, temperature)            # today's signature
        assert list(kw) == ["bias"] and kw["bias"].dtype == torch.float32 and kw["bias"].shape == (N,)
        items = [self.tag(p)[0][1:] for p in pad]
        self.log.append(("neighbour_smoothing_biased", items, kw["bias"].tolist(), iters, topk, temperature))
        return torch.stack([self.coded((it, tuple(kw["bias"].tolist())), feat.shape[1], N) for it in items])

    def score_grids(self, grids, hp, wp, gt, raw_labels=True, areas=None, tally=None, staging_bytes=None):
        assert grids.is_contiguous() and grids.dim() == 4 and grids.shape[1] == gt.shape[0] and staging_bytes is None
        what = [[self.tag(g)[0] for g in gk] for gk in grids]
        self.log.append(("seg_score_grids", what, hp, wp, tuple(gt.shape), raw_labels,
                         areas is not None and tuple(areas.shape) == (grids.shape[0], 3, N) and tally is not None))
        return areas, tally


_PATCH_SCORES = Segmenter.patch_scores       # the real one: the Recorder replaces it, the sweep recorders split it further
BIAS = [0.5, -1.0, 0.0, 2.0, 0.25]
a_, b_ = (0, (64, 96), False), (1, (64, 64), False)


@pytest.mark.parametrize("smooth", [False, True], ids=["rows", "smoothing"])
@pytest.mark.parametrize("upsample", ["probs", "logits"])
def test_without_class_bias_the_launches_are_today_s(monkeypatch, smooth, upsample):
    """`__call__`, `segment_raw`, `evaluate_raw` and `calibrate_raw` of a Segmenter that never names the bias: the plain
    bindings with today's arguments (the fakes have the fixed signatures and fail on anything more)"""
    rec = BiasRecorder(monkeypatch)
    seg = Segmenter(_Model(), category_token_ids=[[1]] * N, temperature=2.0, upsample=upsample, smooth_iters=2 if smooth else 0)
    assert seg.class_bias is None
    imgs, gts = _images()
    row = (lambda it, T=2.0: ("neighbour_smoothing", [it], 2, 3, T)) if smooth else \
        (lambda it, T=2.0: ("rows_to_f32", [it], upsample == "probs" or T != 2.0, T))
    seg.segment_raw(imgs, max_batch=3)
    seg.evaluate_raw(imgs, gts, max_batch=3)
    x = torch.stack([rec.coded(("x", 0), 3, 32, 48)])
    seg(x)
    rows = [e for e in rec.log if e[0] in ("rows_to_f32", "neighbour_smoothing")]
    assert rows == [row(a_), row(b_)] * 2 + [row(("x", 0, False))]
    assert not any("biased" in e[0] or e[0] == "seg_score_grids" for e in rec.log)
    if upsample == "probs" or smooth:
        del rec.log[:]
        seg.calibrate_raw(imgs[:1], gts[:1], temperatures=(0.5, 4.0), max_batch=3)
        assert [e for e in rec.log if e[0] in ("rows_to_f32", "neighbour_smoothing")] == [row(a_, 0.5), row(a_, 4.0)]


@pytest.mark.parametrize("smooth", [False, True], ids=["rows", "smoothing"])
@pytest.mark.parametrize("upsample", ["probs", "logits"])
def test_with_class_bias_the_biased_names_are_called(monkeypatch, smooth, upsample):
    rec = BiasRecorder(monkeypatch)
    seg = Segmenter(_Model(), category_token_ids=[[1]] * N, temperature=2.0, upsample=upsample, smooth_iters=2 if smooth else 0,
                    class_bias=BIAS)
    assert seg.class_bias.dtype == torch.float32 and seg.class_bias.tolist() == BIAS
    imgs, gts = _images()
    row = (lambda it, T=2.0, sm=None: ("neighbour_smoothing_biased", [it], BIAS, 2, 3, T)) if smooth else \
        (lambda it, T=2.0, sm=upsample == "probs": ("rows_to_f32_biased", [it], BIAS, sm, T))
    seg.segment_raw(imgs, max_batch=3)
    seg.evaluate_raw(imgs, gts, max_batch=3)
    seg(torch.stack([rec.coded(("x", 0), 3, 32, 48)]))
    assert [e for e in rec.log if "rows" in e[0] or "smoothing" in e[0]] == [row(a_), row(b_)] * 2 + [row(("x", 0, False))]
    # the scoring launch sees the biased grid
    assert [e[1][0] for e in rec.log if e[0] == "seg_score"] == [[(a_, tuple(BIAS))], [(b_, tuple(BIAS))]]
    if upsample == "probs" or smooth:
        del rec.log[:]
        seg.calibrate_raw(imgs[:1], gts[:1], temperatures=(0.5, 4.0), max_batch=3)
        assert [e for e in rec.log if "rows" in e[0] or "smoothing" in e[0]] == [row(a_, 0.5, True), row(a_, 4.0, True)]
    # assignable afterwards, through the same check; None switches it off
    seg.class_bias = torch.arange(N, dtype=torch.float64)
    assert seg.class_bias.dtype == torch.float32 and seg.class_bias.tolist() == [0.0, 1.0, 2.0, 3.0, 4.0]
    seg.class_bias = None
    del rec.log[:]
    seg.segment_raw(imgs[:1], max_batch=3)
    assert not any("biased" in e[0] for e in rec.log)


GS = (0.0, 0.5, -1.0)
DIR = [1.0, 0.0, -2.0, 0.0, 0.5]


@pytest.mark.parametrize("origin", [None, BIAS], ids=["no_origin", "origin"])
@pytest.mark.parametrize("smooth", [False, True], ids=["rows", "smoothing"])
def test_bias_sweep_raw_launches(monkeypatch, smooth, origin):
    """one forward per batch, K biased row launches per batch on that forward's logits with `scaled_bias(direction, g_k, origin)`
    in the Segmenter's own mode and temperature, one scoring launch per image in image order, and no other scoring launch"""
    rec = BiasRecorder(monkeypatch)
    seg = Segmenter(_Model(), category_token_ids=[[1]] * N, temperature=2.0, upsample="logits", smooth_iters=2 if smooth else 0,
                    class_bias=origin)
    imgs, gts = _images()
    sweep = seg.bias_sweep_raw(imgs, gts, DIR, strengths=GS, max_batch=3)
    assert isinstance(sweep, BiasSweep) and sweep.strengths == GS and sweep.n == N and sweep.direction.tolist() == DIR
    assert sweep.origin.tolist() == (origin or [0.0] * N)
    bs = [scaled_bias(torch.tensor(DIR), g, None if origin is None else torch.tensor(origin)).tolist() for g in GS]
    assert [sweep.bias(k).tolist() for k in range(3)] == bs and bs[0] == (origin or [0.0] * N)
    row = (lambda it, b: ("neighbour_smoothing_biased", [it], b, 2, 3, 2.0)) if smooth else \
        (lambda it, b: ("rows_to_f32_biased", [it], b, False, 2.0))
    assert rec.log == ([("image_load", [0], A, (64, 96)), ("image_load", [1], B, (64, 64)), ("forward", [a_])]
                       + [row(a_, b) for b in bs] + [("forward", [b_])] + [row(b_, b) for b in bs]
                       + [("seg_score_grids", [[(a_, tuple(b))] for b in bs], 4, 6, (1,) + A, True, True),
                          ("seg_score_grids", [[(b_, tuple(b))] for b in bs], 4, 4, (1,) + B, True, True)])
    # into: the same sweep comes back; images of one size share a forward
    del rec.log[:]
    again = seg.bias_sweep_raw([imgs[1], imgs[1]], [gts[1], gts[1]], torch.tensor(DIR), strengths=GS, raw_labels=False, into=sweep)
    assert again is sweep
    assert [e[0] for e in rec.log] == ["image_load", "forward"] + [row(b_, bs[0])[0]] * 3 + ["seg_score_grids"] * 2
    assert rec.log[1] == ("forward", [b_, b_]) and rec.log[-1][4:] == ((1,) + B, False, True)
    # the default list; an empty call
    del rec.log[:]
    full = seg.bias_sweep_raw(imgs[:1], gts[:1], DIR)
    assert full.strengths == default_bias_strengths() and len([e for e in rec.log if e[0] == row(a_, bs[0])[0]]) == 16
    assert seg.bias_sweep_raw([], [], DIR).tally.tolist() == [0, 0]
    # the Segmenter itself is as it was
    assert (seg.class_bias is None) if origin is None else seg.class_bias.tolist() == origin


def test_bias_sweep_launches(monkeypatch):
    rec = BiasRecorder(monkeypatch)
    seg = Segmenter(_Model(), category_token_ids=[[1]] * N)
    x = torch.stack([rec.coded(("x", b), 3, 32, 48) for b in range(2)])
    items = [("x", 0, False), ("x", 1, False)]
    gt = torch.ones(2, 40, 50, dtype=torch.uint8)
    sweep = seg.bias_sweep(x, gt, DIR, strengths=GS)
    bs = [scaled_bias(torch.tensor(DIR), g, torch.zeros(N)).tolist() for g in GS]
    assert rec.log == ([("forward", items)] + [("rows_to_f32_biased", items, b, True, 1.0) for b in bs]
                       + [("seg_score_grids", [[(it, tuple(b)) for it in items] for b in bs], 2, 3, (2, 40, 50), True, True)])
    assert sweep.strengths == GS and seg.bias_sweep(x, gt, DIR, strengths=GS, into=sweep) is sweep
    with pytest.raises(ValueError, match="2 label maps for images"):
        seg.bias_sweep(x[:1], gt, DIR)


def test_refusals_launch_nothing(monkeypatch):
    rec = BiasRecorder(monkeypatch)
    monkeypatch.setattr(hip, "lib", lambda: pytest.fail("the library was reached"))
    mk = lambda **kw: Segmenter(_Model(), category_token_ids=[[1]] * N, **kw)
    imgs, gts = _images()
    seg = mk()
    cases = [
        (seg, dict(scales=(0.5, 1.0)), "scales="), (seg, dict(flip=True), "flip=True"), (seg, dict(slide=True), "slide=True"),
        (mk(slide_views=True), dict(slide=(64, 32)), "slide="), (mk(crf_iters=2), {}, "crf_iters = 2"),
        (mk(pamr_iters=3), {}, "pamr_iters = 3"), (mk(sieve=8), {}, "sieve = 8"),
        (seg, dict(direction=[1.0] * (N - 1)), "direction must be a tensor or sequence of 5 finite numbers"),
        (seg, dict(direction=[1.0] * (N - 1) + [float("nan")]), "direction must be .* 5 finite numbers"),
        (seg, dict(direction=torch.full((N,), float("inf"))), "direction must be"), (seg, dict(direction="hello"), "direction must be"),
        (seg, dict(direction=None), "direction must be"), (seg, dict(direction=3.0), "direction must be"),
        (seg, dict(strengths=()), "strengths must hold 1 .. 16"), (seg, dict(strengths=tuple(range(17))), "1 .. 16"),
        (seg, dict(strengths=(1.0, float("inf"))), "finite number"), (seg, dict(strengths=(float("nan"),)), "finite number"),
        (seg, dict(strengths=2.0), "must be a sequence"),
        (seg, dict(strengths=GS, into=BiasSweep((0.0, 0.5), DIR)), "into must be a BiasSweep"),
        (seg, dict(strengths=GS, into=BiasSweep(GS, [2.0] + DIR[1:])), "into must be a BiasSweep"),
        (seg, dict(strengths=GS, into=BiasSweep(GS, DIR, BIAS)), "into must be a BiasSweep"),
        (mk(class_bias=BIAS), dict(strengths=GS, into=BiasSweep(GS, DIR)), "into must be a BiasSweep"),
        (seg, dict(into="sweep"), "into must be a BiasSweep"),
    ]
    for s, kw, match in cases:
        kw = dict(kw)
        with pytest.raises(ValueError, match=match):
            s.bias_sweep_raw(imgs, gts, kw.pop("direction", DIR), **kw)
    # both orders and the smoothing are allowed
    for kw in (dict(upsample="logits"), dict(upsample="probs"), dict(upsample="logits", smooth_iters=1)):
        assert mk(**kw)._bias_sweep_into("bias_sweep_raw", DIR, GS, None, torch.device("cpu")).n == N
    with pytest.raises(ValueError, match="1 label maps for 2 images"):
        seg.bias_sweep_raw(imgs, gts[:1], DIR)
    with pytest.raises(ValueError, match="label map 1 must be a uint8 or int16 tensor of its image's shape"):
        seg.bias_sweep_raw(imgs, [gts[0], gts[1][:5]], DIR)
    with pytest.raises(ValueError, match="every image must be a uint8 RGB"):
        seg.bias_sweep_raw([imgs[0].float()], gts[:1], DIR)
    for s, kw, match in cases[4:]:
        kw = dict(kw)
        with pytest.raises(ValueError, match=match):
            s.bias_sweep(torch.zeros(1, 3, 32, 32), torch.ones(1, 32, 32, dtype=torch.uint8), kw.pop("direction", DIR), **kw)
    if torch.cuda.is_available():                      # an `into` on another device
        with pytest.raises(ValueError, match="into must be a BiasSweep"):
            seg.bias_sweep_raw(imgs, gts, DIR, strengths=GS, into=BiasSweep(GS, DIR, device="cuda:0"))
    # the constructor and the assignment
    for bad in ([1.0] * (N + 1), [1.0] * (N - 1) + [float("nan")], "bias", 1.0, torch.zeros(N, 1), torch.zeros(N, dtype=torch.bool)):
        with pytest.raises(ValueError, match="Segmenter: class_bias must be a tensor or sequence of 5 finite numbers"):
            mk(class_bias=bad)
        with pytest.raises(ValueError, match="class_bias must be"):
            seg.class_bias = bad
    assert seg.class_bias is None and rec.log == []


def test_class_bias_is_the_last_keyword_and_a_copy():
    import inspect
    assert list(inspect.signature(Segmenter.__init__).parameters)[-1] == "class_bias"
    mine = torch.ones(N)
    seg = Segmenter(_Model(), category_token_ids=[[1]] * N, class_bias=mine)
    mine[0] = 9.0
    assert seg.class_bias.tolist() == [1.0] * N


# ------------------------------------------------------------------------------------------------- the surface
def test_task_method_goes_to_the_segmenter(monkeypatch):
    from ifseg_amd.tasks.mm_tasks.segmentation import SegmentationTask
    rec = BiasRecorder(monkeypatch)
    imgs, gts = _images()
    task = SegmentationTask(num_seg_tokens=N, patch_image_size=64, category_token_ids=[[1]] * N)
    sweep = task.bias_sweep_raw(_Model(), imgs, gts, DIR, strengths=GS, max_batch=3, smooth_iters=1, class_bias=BIAS, upsample="logits")
    assert isinstance(sweep, BiasSweep) and sweep.strengths == GS and sweep.origin.tolist() == BIAS
    names = [e[0] for e in rec.log]
    assert names.count("neighbour_smoothing_biased") == 6 and names.count("seg_score_grids") == 2 and names.count("forward") == 2
    # the four written-out tuples carry the keyword; the new method reads the constructor's signature
    src = open(os.path.join(ROOT, "ifseg_amd", "tasks", "mm_tasks", "segmentation.py")).read()
    tuples = re.findall(r"ctor = \(([^)]*)\)", src)
    assert len(tuples) == 4 and all('"class_bias"' in t and '"sieve_passes"' in t for t in tuples)
    body = src.split("def bias_sweep_raw(")[1].split("\n    def ")[0]
    assert "inspect.signature(Segmenter.__init__)" in body and "ctor = (" not in body
    del rec.log[:]
    task.evaluate_raw(_Model(), imgs, gts, class_bias=BIAS, max_batch=3)
    assert [e[0] for e in rec.log].count("rows_to_f32_biased") == 2


def test_header_constants_and_no_new_op():
    header = open(os.path.join(ROOT, "include", "ifseg_hip.h")).read()
    for name in ("ifseg_softmax_rows_bias(", "ifseg_seg_score_grids(", "ifseg_seg_score_grids_staging(", "ifseg_seg_score_grids_limit("):
        assert "int " + name in header, name
    assert int(re.search(r"#define IFSEG_ABI_VERSION (\d+)", header).group(1)) == 21 == hip.ABI_VERSION
    assert hip.SEG_SCORE_GRIDS_MAX == 16 and hip.SEG_SCORE_GRIDS_STAGING_BYTES == 65536 - (3 * 512 + 4) * 4 == 59376
    src = open(os.path.join(ROOT, "ifseg_amd", "csrc", "bsweep.hip")).read()
    assert "BS_MAX_K = 16" in src and "BS_MAX_CLASSES = 512" in src and "hipMalloc" not in src and "Synchronize" not in src
    assert "double" not in src.split("seg_score_grids_kernel(")[1].split("// whether")[0]          # no fp64 in the kernel
    assert "hipFuncSetAttribute" not in src                                                        # no LDS attribute is raised
    import ifseg_amd.ops  # noqa: F401
    assert not any("score_grids" in name or "rows_bias" in name or "bias_sweep" in name or "biased" in name for name in dir(torch.ops.ifseg))


def _library():
    if not os.path.exists(hip.LIB_PATH):
        from ifseg_amd.build import build
        build(verbose=False)
    return hip.lib()


def test_library_exports_and_limits():
    lib = _library()
    assert all(hasattr(lib, name) for name in ("ifseg_softmax_rows_bias", "ifseg_seg_score_grids", "ifseg_seg_score_grids_staging",
                                               "ifseg_seg_score_grids_limit"))
    assert hip.seg_score_grids_limits() == (hip.SEG_SCORE_GRIDS_MAX, hip.SEG_PREDICT_MAX_CLASSES, 16, 64,
                                            hip.SEG_SCORE_GRIDS_STAGING_BYTES) == (16, 512, 16, 64, 59376)
    assert lib.ifseg_seg_score_grids_limit(ctypes.c_int(5)) == BAD_ARG and lib.ifseg_seg_score_grids_limit(ctypes.c_int(-1)) == BAD_ARG
    # the staging setter hands back the previous ceiling and restores it
    assert lib.ifseg_seg_score_grids_staging(ctypes.c_int(0)) == 65536 and lib.ifseg_seg_score_grids_staging(ctypes.c_int(-1)) == 0
    assert lib.ifseg_seg_score_grids_staging(ctypes.c_int(-1)) == 65536


def test_c_entry_refusals_need_no_device():
    """every refusal returns before anything is launched or dereferenced: the buffers are host memory here"""
    lib = _library()
    K, Bn, hp, wp, n, h, w = 3, 2, 2, 3, 5, 17, 65
    keep = []

    def buf(nbytes):
        raw = ctypes.create_string_buffer(nbytes + 64)
        keep.append(raw)
        return (ctypes.addressof(raw) + 63) & ~63                 # 64-byte aligned

    gbytes, tbytes, abytes = 4 * K * Bn * hp * wp * n, 2 * Bn * h * w, 8 * K * 3 * n
    a = dict(grids=buf(gbytes), gt=buf(tbytes), areas=buf(abytes), tally=buf(16))
    r = dict(logits=buf(2 * 4 * 8), bias=buf(4 * n), prob=buf(4 * 4 * n))
    before = [bytes(raw) for raw in keep]
    ci, vp, ll, cf = ctypes.c_int, ctypes.c_void_p, ctypes.c_longlong, ctypes.c_float

    def score(K=K, B=Bn, hp=hp, wp=wp, n=n, h=h, w=w, gb=2, **ptr):
        p = dict(a, **ptr)
        return lib.ifseg_seg_score_grids(vp(p["grids"]), ci(K), ci(B), ci(hp), ci(wp), ci(n), ci(h), ci(w), vp(p["gt"]), ci(gb), ci(1),
                                         vp(p["areas"]), vp(p["tally"]), None)

    for name in a:
        assert score(**{name: None}) == BAD_ARG, name
    assert score(grids=a["grids"] + 2) == BAD_ARG and score(gt=a["gt"] + 1) == BAD_ARG
    assert score(areas=a["areas"] + 4) == BAD_ARG and score(tally=a["tally"] + 4) == BAD_ARG
    for kw in (dict(K=0), dict(K=17), dict(K=-1), dict(n=0), dict(n=513), dict(n=-1), dict(gb=0), dict(gb=3), dict(gb=4)):
        assert score(**kw) == BAD_ARG, kw
    for kw in (dict(B=0), dict(hp=0), dict(wp=0), dict(h=0), dict(w=-1), dict(hp=2 ** 15, h=2 ** 15), dict(wp=2 ** 15, w=2 ** 15),
               dict(B=2 ** 11, h=2 ** 10, w=2 ** 10), dict(hp=2 ** 11, wp=2 ** 11)):
        assert score(**kw) == BAD_SHAPE, kw
    # a counter sharing a byte with an input or with the other counter
    assert score(areas=a["grids"]) == BAD_ARG and score(areas=a["grids"] + ((gbytes - 8) & ~7)) == BAD_ARG
    assert score(areas=a["gt"]) == BAD_ARG and score(tally=a["gt"] + ((tbytes - 8) & ~7)) == BAD_ARG
    assert score(tally=a["grids"] + 8) == BAD_ARG and score(tally=a["areas"]) == BAD_ARG and score(tally=a["areas"] + abytes - 8) == BAD_ARG
    assert score(areas=a["tally"] - abytes + 8) == BAD_ARG

    def rows(rows=4, n=n, rpb=2, **ptr):
        p = dict(r, **ptr)
        return lib.ifseg_softmax_rows_bias(vp(p["logits"]), ll(16), ci(rpb), ci(8), vp(p["bias"]), vp(p["prob"]), ci(rows), ci(n),
                                           cf(1.0), ci(1), None)

    for name in r:
        assert rows(**{name: None}) == BAD_ARG, name
    assert rows(logits=r["logits"] + 1) == BAD_ARG and rows(bias=r["bias"] + 2) == BAD_ARG and rows(prob=r["prob"] + 2) == BAD_ARG
    assert rows(n=0) == BAD_ARG and rows(rpb=0) == BAD_ARG
    assert rows(bias=r["prob"]) == BAD_ARG and rows(bias=r["prob"] + 4 * 4 * n - 4) == BAD_ARG and rows(prob=r["bias"] + 4 * (n - 1)) == BAD_ARG
    assert rows(rows=0) == 0 and rows(rows=-3) == 0               # nothing to do, as ifseg_softmax_rows
    assert [bytes(raw) for raw in keep] == before                 # nothing was written
