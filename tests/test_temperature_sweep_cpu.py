"""CPU: the rule of the temperature sweep (`predict.temperature_sweep_reference`, `temperature_sweep_from_probs`) against literal
formulas, the recovery of a known temperature, `TemperatureSweep`, and which launches `Segmenter.calibrate_raw` / `calibrate`
make (recording fakes, as tests/test_segmenter_launches_cpu.py)."""
import math

import pytest
import torch
import torch.nn.functional as F

import _tsweep_cases as TC
from ifseg_amd import hip
from ifseg_amd.predict import (FLT_MIN, Segmenter, TemperatureSweep, _scored_mask, areas_reference, calibration_reference,
                               default_temperatures, temperature_sweep_from_probs, temperature_sweep_reference,
                               upsample_argmax_reference)
from test_segmenter_launches_cpu import A, B, N, Recorder, _Model, _images

LITERAL = ("small_ids_i16_oor", "small_raw_u8_oor", "small_down_ids_u8", "n1", "ragged_k1", "identity")


def test_default_temperatures():
    t = default_temperatures()
    assert len(t) == 16 == hip.SEG_SWEEP_MAX_TEMPERATURES and t[7] == 1.0 and t[11] == 2.0 and t[-1] == 4.0
    assert abs(t[0] - 0.2973) < 1e-4 and all(a < b for a, b in zip(t, t[1:]))
    assert FLT_MIN == 2.0 ** -126


@pytest.mark.parametrize("name", LITERAL)
def test_reference_is_the_literal_rule(name):
    """both raw_labels settings, uint8 and int16 ground truth, ignore values, an out-of-range value, n = 1, up- and
    downscaling: the counters exactly, the sums to the rounding of a float64 sum of a few thousand terms"""
    grids, gt, (hp, wp, n, raw), where = TC.make(name)
    hist, sums, tally = temperature_sweep_reference(grids, hp, wp, gt, raw)
    want_h, want_s, want_t = TC.literal(grids, hp, wp, gt, raw)
    K = grids.shape[0]
    assert hist.dtype == torch.int64 and hist.shape == (K, 256, 2) and sums.dtype == torch.float64 and sums.shape == (K, 2)
    assert torch.equal(tally, want_t) and int(tally[0]) > 0 and (int(tally[1]) > 0) == {**TC.KINDS, **TC.SMALL_KINDS}[name][2]
    assert torch.equal(hist, want_h) and hist.sum((1, 2)).tolist() == [int(tally[0])] * K
    # the two evaluations order the four products differently: a value moves by a few of ITS ulps, so a term -log p by a few
    # 2^-52 in absolute terms whatever p is (d log p = dp / p), a Brier term by less
    assert torch.allclose(sums, want_s, rtol=1e-12, atol=int(tally[0]) * 2.0 ** -48)
    # an unscored pixel contributes nowhere: every ignored value swapped for the other ignore value, same counters
    ign = (0, 255) if raw else (n, 255)
    if gt.dtype == torch.int16 or max(ign) <= 255:
        g2 = torch.where(gt == ign[0], torch.full_like(gt, ign[1]), torch.where(gt == ign[1], torch.full_like(gt, ign[0]), gt))
        again = temperature_sweep_reference(grids, hp, wp, g2, raw)
        assert all(torch.equal(a, b) for a, b in zip(again, (hist, sums, tally)))
    if where:
        y, x, t = where["zero"]
        assert float(upsample_argmax_reference(grids[0], hp, wp, *gt.shape[1:])[2][0, t, y, x]) == 0.0
        assert float(sums[0, 0]) >= -math.log(FLT_MIN) > 87.3 and hist[0, 255].sum() >= 1


@pytest.mark.parametrize("name", LITERAL + ("x16_two_images",))
def test_rows_are_the_calibration_counters_and_the_torch_losses(name):
    grids, gt, (hp, wp, n, raw), _ = TC.make(name)
    h, w = gt.shape[1:]
    hist, sums, tally = temperature_sweep_reference(grids, hp, wp, gt, raw)
    for k in range(grids.shape[0]):
        labels, conf, probs = upsample_argmax_reference(grids[k], hp, wp, h, w)
        cal = calibration_reference(labels, conf.float(), gt, n, raw)[0]
        assert torch.equal(hist[k], cal.sum(0))
        assert torch.equal(tally, areas_reference(labels, gt, n, raw)[1])
        _, cls, scored, _ = _scored_mask("test", labels, gt, n, raw)
        p = probs.permute(0, 2, 3, 1).reshape(-1, n)[scored]
        assert p.dtype == torch.float64
        nll = F.nll_loss(p.clamp_min(FLT_MIN).log(), cls[scored], reduction="sum")
        brier = ((p - F.one_hot(cls[scored], n).double()) ** 2).sum()
        # the expanded square cancels: a pixel's term is within a few ulps of sum p^2 + 2 p_t + 1 <= 4 of the binomial's
        assert torch.allclose(sums[k, 0], nll, rtol=1e-12, atol=0.0)
        assert torch.allclose(sums[k, 1], brier, rtol=0.0, atol=int(tally[0]) * 2.0 ** -48)
    # from values at image resolution: the same arithmetic, and fp32 values are taken as they are
    p32 = [upsample_argmax_reference(g, hp, wp, h, w, torch.float32)[2] for g in grids]
    a = temperature_sweep_from_probs(p32, gt, n, raw)
    b = temperature_sweep_from_probs([p.double() for p in p32], gt, n, raw)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    with pytest.raises(ValueError, match="no temperatures"):
        temperature_sweep_from_probs([], gt, n, raw)
    with pytest.raises(ValueError, match="values 0 must be floating"):
        temperature_sweep_from_probs([p32[0][:, :, :-1]], gt, n, raw)


def _sweep_of(factor, n, seed):
    """identity geometry 32 x 32; y ~ Categorical(softmax(z)), the grids softmax(factor z / T_k): the model is over-confident by
    `factor`, and T = factor undoes it"""
    g = torch.Generator().manual_seed(seed)
    z = 3.0 * torch.randn(1, 32 * 32, n, generator=g, dtype=torch.float64)
    y = torch.multinomial(torch.softmax(z[0], -1), 1, generator=g).reshape(1, 32, 32).to(torch.uint8)
    temps = default_temperatures()
    grids = torch.stack([torch.softmax(factor * z / T, -1).float() for T in temps])
    sweep = TemperatureSweep(temps, n=n)
    hist, sums, tally = temperature_sweep_reference(grids, 32, 32, y, raw_labels=False)
    sweep.hist += hist
    sweep.sums += sums
    sweep.tally += tally
    return sweep


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("factor", [2.0, 0.5, 1.0])
def test_a_known_temperature_is_recovered(factor, seed):
    sweep = _sweep_of(factor, 15, seed)
    assert sweep.best() == factor
    s = sweep.summary()
    assert s["pixels"] == 1024 and s["best"] == factor and s["temperatures"] == list(default_temperatures())
    k = s["temperatures"].index(factor)
    assert s["NLL"][k] == min(s["NLL"]) and len(s["Brier"]) == len(s["ECE"]) == len(s["MCE"]) == len(s["aAcc"]) == 16
    # the argmax does not depend on the temperature
    assert max(s["aAcc"]) - min(s["aAcc"]) < 1e-12 and 0.0 < s["aAcc"][0] < 1.0


def test_temperature_sweep_object():
    a, b = _sweep_of(2.0, 15, 5), _sweep_of(2.0, 15, 6)
    both = TemperatureSweep(default_temperatures(), n=15).add_(a).add_(b)
    assert torch.equal(both.hist, a.hist + b.hist) and torch.equal(both.sums, a.sums + b.sums) and both.tally.tolist() == [2048, 0]
    s = both.summary()
    assert s["pixels"] == 2048 and s["NLL"] == (both.sums[:, 0] / 2048).tolist() and s["Brier"] == (both.sums[:, 1] / 2048).tolist()
    # ECE / MCE / aAcc are the 16-bin figures of the row's counters; reliability is the row's diagram
    for k in (0, 7, 15):
        N_, acc, conf = both.reliability(k)
        assert N_.dtype == torch.int64 and N_.shape == acc.shape == conf.shape == (16,) and int(N_.sum()) == 2048
        fine = both.hist[k].double()
        want_n = fine.sum(-1).reshape(16, 16).sum(-1)
        assert torch.equal(N_.double(), want_n)
        live = want_n > 0
        gap = (acc - conf).abs()[live]
        assert math.isclose(s["ECE"][k], float((want_n[live] * gap).sum() / 2048), rel_tol=1e-12)
        assert math.isclose(s["MCE"][k], float(gap.max()), rel_tol=1e-12)
        assert math.isclose(s["aAcc"][k], float(fine[:, 1].sum() / 2048), rel_tol=1e-12)
        assert torch.isnan(acc[~live]).all()
    assert both.reliability(3, bins=4)[0].shape == (4,)
    # the tie rule: the first of equal mean NLLs wins
    tie = TemperatureSweep((0.5, 1.0, 2.0))
    tie.sums[:, 0] = torch.tensor([3.0, 2.0, 2.0], dtype=torch.float64)
    tie.tally[0] = 4
    tie.hist[:, 200, 1] = 4
    assert tie.best() == 1.0 and tie.summary()["NLL"] == [0.75, 0.5, 0.5]
    # ground truth out of range raises, as SegmentationScore.summary does
    tie.tally[1] = 1
    with pytest.raises(IndexError, match="tally\\[1\\] = 1"):
        tie.summary()
    with pytest.raises(IndexError):
        tie.best()
    empty = TemperatureSweep((1.0, 2.0))
    assert empty.summary()["best"] is None and empty.summary()["pixels"] == 0 and math.isnan(empty.summary()["NLL"][0])
    with pytest.raises(ValueError, match="no scored pixels"):
        empty.best()
    with pytest.raises(ValueError, match="different lists do not add"):
        both.add_(tie)
    with pytest.raises(ValueError, match="15 classes|classes against"):
        both.add_(TemperatureSweep(default_temperatures(), n=3))
    for bad in ((), tuple(range(1, 18)), (1.0, 0.0), (1.0, -2.0), (float("inf"),), (float("nan"),), (True,), ("1",), 3.0):
        with pytest.raises(ValueError, match="temperatures"):
            TemperatureSweep(bad)
    with pytest.raises(ValueError, match="bins must be an int that divides 256"):
        both.reliability(0, bins=10)
    with pytest.raises(ValueError, match="k must be an int"):
        both.reliability(16)


# ------------------------------------------------------------------------------------------------- which launches
class SweepRecorder(Recorder):
    """the Recorder with the forward split where `patch_scores_at` splits it: the padded logits of a batch, the softmax per
    temperature, and the sweep launch"""

    def __init__(self, monkeypatch):
        super().__init__(monkeypatch)
        monkeypatch.setattr(Segmenter, "_padded_logits", lambda seg, x: self.logits(x))
        monkeypatch.setattr(hip, "rows_to_f32", self.rows_to_f32)
        monkeypatch.setattr(hip, "neighbour_smoothing", self.neighbour_smoothing)
        monkeypatch.setattr(hip, "seg_temperature_sweep", self.sweep)

    def logits(self, x):
        _, hp, wp = self.forward(x)                               # records ("forward", items)
        items = self.log[-1][1]
        return (torch.stack([self.coded(("pad",) + it, hp * wp + 1, 8) for it in items]), hp, wp,
                torch.stack([self.coded(("feat",) + it, hp * wp, 4) for it in items]))

    def rows_to_f32(self, pad, nseg, rows, softmax=False, temperature=1.0):
        items = [self.tag(p)[0][1:] for p in pad]
        assert nseg == N and all(self.tag(p)[0][0] == "pad" for p in pad)
        self.log.append(("rows_to_f32", items, softmax, temperature))
        return torch.stack([self.coded((it, temperature), rows, N) for it in items])

    def neighbour_smoothing(self, pad, nseg, feat, iters, topk, temperature=1.0):
        items = [self.tag(p)[0][1:] for p in pad]
        assert [self.tag(f)[0] for f in feat] == [("feat",) + it for it in items]
        self.log.append(("neighbour_smoothing", items, iters, topk, temperature))
        return torch.stack([self.coded((it, temperature), feat.shape[1], N) for it in items])

    def sweep(self, grids, hp, wp, gt, raw_labels=True, hist=None, sums=None, tally=None, staging_bytes=None):
        assert grids.is_contiguous() and grids.dim() == 4 and grids.shape[1] == gt.shape[0] and staging_bytes is None
        what = [[self.tag(g)[0] for g in gk] for gk in grids]
        self.log.append(("seg_temperature_sweep", what, hp, wp, tuple(gt.shape), raw_labels,
                         hist is not None and sums is not None and tally is not None))
        return hist, sums, tally


TEMPS = (0.5, 1.0, 2.0)


@pytest.mark.parametrize("smooth", [False, True], ids=["softmax", "smoothing"])
def test_calibrate_raw_launches(monkeypatch, smooth):
    """one forward per batch, K softmaxes per batch on that forward's logits, one sweep launch per image in image order, and no
    scoring launch; the Segmenter's own temperature is not consulted"""
    rec = SweepRecorder(monkeypatch)
    seg = Segmenter(_Model(), category_token_ids=[[1]] * N, temperature=7.0, smooth_iters=2 if smooth else 0, smooth_topk=3)
    imgs, gts = _images()
    sweep = seg.calibrate_raw(imgs, gts, temperatures=TEMPS, max_batch=3)
    assert isinstance(sweep, TemperatureSweep) and sweep.temperatures == TEMPS and sweep.n == N
    a, b = (0, (64, 96), False), (1, (64, 64), False)
    soft = (lambda it, T: ("neighbour_smoothing", [it], 2, 3, T)) if smooth else (lambda it, T: ("rows_to_f32", [it], True, T))
    assert rec.log == ([("image_load", [0], A, (64, 96)), ("image_load", [1], B, (64, 64)), ("forward", [a])]
                       + [soft(a, T) for T in TEMPS] + [("forward", [b])] + [soft(b, T) for T in TEMPS]
                       + [("seg_temperature_sweep", [[(a, T)] for T in TEMPS], 4, 6, (1,) + A, True, True),
                          ("seg_temperature_sweep", [[(b, T)] for T in TEMPS], 4, 4, (1,) + B, True, True)])
    # into: the same sweep comes back; images of one size share a forward
    del rec.log[:]
    again = seg.calibrate_raw([imgs[1], imgs[1]], [gts[1], gts[1]], temperatures=TEMPS, raw_labels=False, into=sweep)
    assert again is sweep
    assert [e[0] for e in rec.log] == ["image_load", "forward"] + [soft(b, 1.0)[0]] * 3 + ["seg_temperature_sweep"] * 2
    assert rec.log[1] == ("forward", [b, b]) and rec.log[-1][4:] == ((1,) + B, False, True)
    # the default list
    del rec.log[:]
    full = seg.calibrate_raw(imgs[:1], gts[:1])
    assert full.temperatures == default_temperatures() and len([e for e in rec.log if e[0] == soft(a, 1.0)[0]]) == 16
    assert [e[-1] for e in rec.log if e[0] == soft(a, 1.0)[0]] == list(default_temperatures())
    assert seg.calibrate_raw([], []).tally.tolist() == [0, 0]


def test_calibrate_launches(monkeypatch):
    rec = SweepRecorder(monkeypatch)
    seg = Segmenter(_Model(), category_token_ids=[[1]] * N)
    x = torch.stack([rec.coded(("x", b), 3, 32, 48) for b in range(2)])
    items = [("x", 0, False), ("x", 1, False)]
    gt = torch.ones(2, 40, 50, dtype=torch.uint8)
    sweep = seg.calibrate(x, gt, temperatures=TEMPS)
    assert rec.log == ([("forward", items)] + [("rows_to_f32", items, True, T) for T in TEMPS]
                       + [("seg_temperature_sweep", [[(it, T) for it in items] for T in TEMPS], 2, 3, (2, 40, 50), True, True)])
    assert sweep.temperatures == TEMPS
    with pytest.raises(ValueError, match="2 label maps for images"):
        seg.calibrate(x[:1], gt)


def test_calibrate_refusals_launch_nothing(monkeypatch):
    rec = SweepRecorder(monkeypatch)
    mk = lambda **kw: Segmenter(_Model(), category_token_ids=[[1]] * N, **kw)
    imgs, gts = _images()
    seg = mk()
    other = TemperatureSweep(TEMPS, n=N + 1)
    cases = [
        (seg, dict(scales=(0.5, 1.0)), "scales="), (seg, dict(flip=True), "flip=True"), (seg, dict(slide=True), "slide=True"),
        (mk(slide_views=True), dict(slide=(64, 32)), "slide="), (mk(crf_iters=2), {}, "crf_iters = 2"),
        (mk(upsample="logits"), {}, r"must be probabilities.*upsample='logits'"),
        (seg, dict(temperatures=()), "temperatures must hold 1 .. 16"), (seg, dict(temperatures=tuple(range(1, 18))), "1 .. 16"),
        (seg, dict(temperatures=(1.0, 0.0)), "finite number > 0"), (seg, dict(temperatures=(float("nan"),)), "finite number > 0"),
        (seg, dict(temperatures=(float("inf"),)), "finite number > 0"),
        (seg, dict(temperatures=TEMPS, into=TemperatureSweep((0.5, 1.0))), "into must be a TemperatureSweep"),
        (seg, dict(temperatures=TEMPS, into=other), "into must be a TemperatureSweep"),
        (seg, dict(into="sweep"), "into must be a TemperatureSweep"),
    ]
    for s, kw, match in cases:
        with pytest.raises(ValueError, match=match):
            s.calibrate_raw(imgs, gts, **kw)
    # the smoothing makes probabilities of either order
    assert mk(upsample="logits", smooth_iters=1)._sweep_into("calibrate_raw", TEMPS, None, torch.device("cpu")).n == N
    with pytest.raises(ValueError, match="1 label maps for 2 images"):
        seg.calibrate_raw(imgs, gts[:1])
    with pytest.raises(ValueError, match="label map 1 must be a uint8 or int16 tensor of its image's shape"):
        seg.calibrate_raw(imgs, [gts[0], gts[1][:5]])
    with pytest.raises(ValueError, match="every image must be a uint8 RGB"):
        seg.calibrate_raw([imgs[0].float()], gts[:1])
    for s, kw, match in cases[4:]:
        with pytest.raises(ValueError, match=match):
            s.calibrate(torch.zeros(1, 3, 32, 32), torch.ones(1, 32, 32, dtype=torch.uint8), **kw)
    if torch.cuda.is_available():                      # an `into` on another device
        with pytest.raises(ValueError, match="into must be a TemperatureSweep"):
            seg.calibrate_raw(imgs, gts, temperatures=TEMPS, into=TemperatureSweep(TEMPS, "cuda:0", N))
    assert rec.log == []


def test_task_method_goes_to_the_segmenter(monkeypatch):
    from ifseg_amd.tasks.mm_tasks.segmentation import SegmentationTask
    rec = SweepRecorder(monkeypatch)
    imgs, gts = _images()
    task = SegmentationTask(num_seg_tokens=N, patch_image_size=64, category_token_ids=[[1]] * N)
    sweep = task.calibrate_raw(_Model(), imgs, gts, temperatures=TEMPS, max_batch=3, smooth_iters=1)
    assert isinstance(sweep, TemperatureSweep) and sweep.temperatures == TEMPS
    assert [e[0] for e in rec.log].count("neighbour_smoothing") == 6 and [e[0] for e in rec.log].count("seg_temperature_sweep") == 2
