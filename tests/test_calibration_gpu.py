"""hip.seg_calibration (csrc/calib.hip) and Segmenter.evaluate_raw(calibration=True) on the GPU: exact parity to
`predict.calibration_reference` in both table regimes, at every kind of size and alignment, through the op, and end to end."""
import ctypes

import pytest
import torch

import _calib_cases as CC
import _predict_cases as PC
import _score_cases as SC
from test_confusion_gpu import SETTINGS
from test_predict_views_gpu import e2e  # noqa: F401  (the segofa_tiny fixture with its three raw shapes)

pytestmark = pytest.mark.gpu

BAD_SHAPE, BAD_ARG = -2, -3
SIZES = (1, 15, 255, 4096, 4097, 70001)
OFFSETS = ((0, 0, 0), (3, 1, 5), (5, 2, 1), (15, 3, 7))         # elements: labels, conf, ground truth


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ifseg_amd.ops  # noqa: F401
    return torch.device("cuda:0")


# (n, labels' dtype, ground truth's dtype, raw_labels): both table regimes on both sides of the switch, the dtypes mixed
SPEC_CASES = [(15, torch.uint8, torch.uint8, True), (32, torch.uint8, torch.int16, True), (33, torch.int16, torch.uint8, False),
              (150, torch.uint8, torch.uint8, False), (300, torch.int16, torch.int16, True)]


@pytest.mark.parametrize("n,ldt,gdt,raw", SPEC_CASES,
                         ids=["n15_direct", "n32_direct_gt16", "n33_hashed_lab16_ids", "n150_hashed_ids", "n300_i16_hashed"])
def test_counters_are_the_specification(n, ldt, gdt, raw):
    """piecewise-constant labels with random conf and ground truth at every pixel count (one pixel, below and at one group, one
    workgroup step and one pixel more, several workgroups), at element offsets that put a head in front of the labels' first
    16-byte boundary and the confidences and the ground truth off theirs; a second launch into the same counters doubles
    them.  Every reference table from 255 pixels on has hits and misses in more than one bin and scored pixels with a label
    outside the classes; the two below it (1 and 15 pixels, all scored, all inside) hold every pixel"""
    from ifseg_amd import hip
    from ifseg_amd.predict import calibration_reference
    dev = _dev()
    assert (n <= hip.SEG_CALIBRATION_DIRECT_CLASSES) == (n <= 32)
    keys, same = [], []
    for npix in SIZES:
        labels, conf, gt = CC.maps(npix, n, ldt, gdt, npix + n, False, raw)
        want_c, want_t = calibration_reference(labels, conf, gt, n, raw)
        assert int(want_c.sum()) == int(want_t[0]) and int(want_t.sum()) <= npix
        assert CC.telling(want_c, want_t) if npix >= 255 else int(want_c.sum()) == npix
        want_c, want_t = want_c.to(dev), want_t.to(dev)
        labbuf, confbuf = torch.zeros(npix + 16, dtype=ldt, device=dev), torch.zeros(npix + 16, device=dev)
        gtbuf = torch.zeros(npix + 16, dtype=gdt, device=dev)
        for lo, co, go in OFFSETS:
            ld, cd, gd = labbuf[lo:lo + npix].copy_(labels), confbuf[co:co + npix].copy_(conf), gtbuf[go:go + npix].copy_(gt)
            cal, tally = hip.seg_calibration(ld, cd, gd, n, raw)
            assert cal.dtype == torch.int64 and cal.shape == (n, 256, 2) and tally.dtype == torch.int64 and tally.shape == (2,)
            first = (cal == want_c).all() & (tally == want_t).all()
            again = hip.seg_calibration(ld, cd, gd, n, raw, calibration=cal, tally=tally)
            assert again[0] is cal and again[1] is tally
            keys.append((npix, lo, co, go))
            same.append(torch.stack([first, (cal == 2 * want_c).all() & (tally == 2 * want_t).all(), cal.sum() == tally[0]]))
    same = torch.stack(same).cpu().tolist()                       # the one synchronisation
    wrong = [(k, ok) for k, ok in zip(keys, same) if not all(ok)]  # (first launch, accumulated, sum == tally[0])
    assert len(keys) == 24 and not wrong, wrong[:10]


def test_limits_are_the_library_s():
    from ifseg_amd import hip
    _dev()
    assert hip.seg_calibration_limits() == (hip.SEG_CALIBRATION_DIRECT_CLASSES, hip.SEG_CALIBRATION_SLOTS,
                                            hip.SEG_CALIBRATION_STEP_PIXELS, hip.SEG_CALIBRATION_MAX_BLOCKS) == (32, 4096, 4096, 512)
    assert hip.lib().ifseg_seg_calibration_limit(ctypes.c_int(4)) == BAD_ARG


@pytest.mark.parametrize("n,ldt,gdt", [(150, torch.uint8, torch.uint8), (300, torch.int16, torch.int16)], ids=["n150", "n300_i16"])
def test_counters_of_a_large_map(n, ldt, gdt):
    """1100 x 2000 pixels with a class per pixel: more than 512 workgroups' worth of steps, so the grid-stride loop runs, and
    far more distinct keys than a workgroup's table has slots (76 800 possible at n = 150 against 4096): the global-memory path"""
    from ifseg_amd import hip
    from ifseg_amd.predict import calibration_reference
    dev = _dev()
    H, W = 1100, 2000
    assert H * W > hip.SEG_CALIBRATION_MAX_BLOCKS * hip.SEG_CALIBRATION_STEP_PIXELS
    labels, conf, gt = (t.reshape(H, W) for t in CC.maps(H * W, n, ldt, gdt, 7, True))
    want_c, want_t = calibration_reference(labels, conf, gt, n)
    assert CC.telling(want_c, want_t) and int((want_c > 0).sum()) > 8 * hip.SEG_CALIBRATION_SLOTS
    cal, tally = hip.seg_calibration(labels.to(dev), conf.to(dev), gt.to(dev), n)
    assert torch.equal(cal.cpu(), want_c) and torch.equal(tally.cpu(), want_t) and int(cal.sum()) == int(tally[0])


def test_entry_point_refusals():
    """each refusal returns its code and launches nothing: the counters stay zero; the limits themselves pass"""
    from ifseg_amd import hip
    dev = _dev()
    lib = hip.lib()
    i, ll, vp = ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p
    p = lambda t, off=0: vp(t.data_ptr() + off)
    lab, gt = torch.zeros(64, dtype=torch.int16, device=dev), torch.ones(64, dtype=torch.int16, device=dev)
    conf = torch.zeros(64, device=dev)
    cal, tally = torch.zeros(512 * 512 + 1, dtype=torch.int64, device=dev), torch.zeros(3, dtype=torch.int64, device=dev)

    def call(labels=p(lab), lb=2, cf=p(conf), g=p(gt), gb=2, npix=16, n=5, raw=1, c=p(cal), t=p(tally)):
        return lib.ifseg_seg_calibration(labels, i(lb), cf, g, i(gb), ll(npix), i(n), i(raw), c, t, None)

    for bad in (dict(labels=vp(None)), dict(cf=vp(None)), dict(g=vp(None)), dict(c=vp(None)), dict(t=vp(None)), dict(lb=0),
                dict(lb=4), dict(gb=0), dict(gb=3), dict(labels=p(lab, 1)), dict(g=p(gt, 1)), dict(cf=p(conf, 2)),
                dict(c=p(cal, 4)), dict(t=p(tally, 4)), dict(n=0), dict(n=513)):
        assert call(**bad) == BAD_ARG, bad
    for bad in (dict(npix=0), dict(npix=-1), dict(npix=2 ** 31)):
        assert call(**bad) == BAD_SHAPE, bad
    torch.cuda.synchronize()
    assert not cal.any() and not tally.any()                      # no launch so far
    # n = 512 and byte maps at odd addresses: 16 pixels of label 0, conf 0, raw ground truth 1 of an int16 seen as bytes
    # from its second byte on (0, 1, 0, 1, ...): ignored on the even pixels, class 0 on the odd ones
    assert call(n=512, lb=1, gb=1, labels=p(lab, 1), g=p(gt, 3), cf=p(conf, 4), c=p(cal, 8), t=p(tally, 8)) == 0
    torch.cuda.synchronize()
    assert int(cal[1 + 1]) == 8 and int(cal.sum()) == 8 and tally.tolist() == [0, 8, 0]


@pytest.mark.parametrize("n,dtype", [(15, torch.uint8), (150, torch.int16)], ids=["n15_direct", "n150_i16_hashed"])
def test_agrees_with_seg_areas_on_one_input(n, dtype):
    """summed over bins and hit the counters are seg_areas' predicted row, their hits its intersect row"""
    from ifseg_amd import hip
    dev = _dev()
    labels, conf, gt = CC.maps(10101, n, dtype, dtype, n, False)
    ld, cd, gd = labels.to(dev), conf.to(dev), gt.to(dev)
    cal, tally = hip.seg_calibration(ld, cd, gd, n)
    areas, atally = hip.seg_areas(ld, gd, n)
    same = torch.stack([(cal.sum((1, 2)) == areas[1]).all(), (cal[..., 1].sum(1) == areas[0]).all(), tally.sum() == atally[0],
                        areas[0].sum() > 0, tally[1] > 0])
    assert same.cpu().tolist() == [True] * 5


def test_op_matches_the_binding():
    from ifseg_amd import hip
    from ifseg_amd.predict import calibration_reference
    dev = _dev()
    H, W, n = 17, 66, 150
    labels, conf, gt = (t.reshape(2, H, W) for t in CC.maps(2 * H * W, n, torch.int16, torch.uint8, 3, True))
    assert CC.telling(*calibration_reference(labels, conf, gt, n))
    labels, conf, gt = labels.to(dev), conf.to(dev), gt.to(dev)
    op = torch.ops.ifseg.seg_calibration
    want_c, want_t = hip.seg_calibration(labels, conf, gt, n)
    got_c, got_t = op(labels, conf, gt, n, True)
    assert torch.equal(got_c, want_c) and torch.equal(got_t, want_t) and int(got_c.sum()) > 0
    ids_c, ids_t = op(labels, conf, gt, n, False)
    ref_c, ref_t = hip.seg_calibration(labels, conf, gt, n, False)
    assert torch.equal(ids_c, ref_c) and torch.equal(ids_t, ref_t) and not torch.equal(ids_c, want_c)
    # non-contiguous inputs are copied
    t = op(labels.transpose(1, 2), conf.transpose(1, 2), gt.transpose(1, 2), n, True)
    assert torch.equal(t[0], want_c) and torch.equal(t[1], want_t)
    torch.library.opcheck(op, (labels, conf, gt, n, True), test_utils=("test_schema", "test_autograd_registration", "test_faketensor"))
    # on a side stream the op follows PyTorch's current stream
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        side = op(labels, conf, gt, n, True)
    st.synchronize()
    assert torch.equal(side[0], want_c) and torch.equal(side[1], want_t)
    for bad in (lambda: op(labels.long(), conf, gt, n, True), lambda: op(labels, conf.double(), gt, n, True),
                lambda: op(labels, conf, gt.long(), n, True), lambda: op(labels, conf, gt[:1], n, True),
                lambda: op(labels, conf[:1], gt, n, True), lambda: op(labels, conf, gt, 0, True), lambda: op(labels, conf, gt, 513, True)):
        with pytest.raises(ValueError, match="ifseg::seg_calibration"):
            bad()


# ------------------------------------------------------------------------------------------------- end to end
def _gts(raw, n):
    return [SC.ground_truth(tuple(r.shape[:2]), n, True, k, torch.int16 if k == 1 else torch.uint8) for k, r in enumerate(raw)]


def _reference(labels, confs, gts, n):
    from ifseg_amd.predict import calibration_reference
    pairs = [calibration_reference(l.cpu(), c.cpu(), g, n) for l, c, g in zip(labels, confs, gts)]
    return sum(p[0] for p in pairs), sum(p[1] for p in pairs)


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_evaluate_raw_with_calibration(e2e, setting):  # noqa: F811
    from ifseg_amd.predict import SegmentationScore, boundary_areas_reference, boundary_distance, confusion_reference
    m, raw, ocfg, mk = e2e
    n = ocfg.num_seg_tokens
    kw, call = SETTINGS[setting]
    seg = mk(**kw)
    gts = _gts(raw, n)
    score, labels = seg.evaluate_raw(raw, gts, calibration=True, return_labels=True, **call)
    cal = score.calibration
    assert cal.is_cuda and cal.dtype == torch.int64 and cal.shape == (n, 256, 2) and score.confusion is None and score.boundary is None
    # the counters are the specification's of the labels the same call returned and segment_raw's conf
    outs = seg.segment_raw(raw, return_conf=True, **call)
    assert all(torch.equal(l, o.labels) for l, o in zip(labels, outs))
    want_c, want_t = _reference(labels, [o.conf for o in outs], gts, n)
    hits, misses = want_c[..., 1].sum(0), want_c[..., 0].sum(0)
    assert int((hits > 0).sum()) > 1 and int((misses > 0).sum()) > 1          # the model's labels are all inside: no second tally
    assert torch.equal(cal.cpu(), want_c) and torch.equal(score.calibration_tally.cpu(), want_t)
    assert torch.equal(cal.sum((1, 2)), score.areas[1]) and torch.equal(cal[..., 1].sum(1), score.areas[0])
    s = score.summary()
    assert 0.0 <= s["ECE"] <= s["MCE"] <= 1.0 and len(s["cECE"]) == n
    # areas, tally and the labels are what they are without it
    plain, plain_labels = seg.evaluate_raw(raw, gts, return_labels=True, **call)
    assert plain.calibration is None and torch.equal(plain.areas, score.areas) and torch.equal(plain.tally, score.tally)
    assert all(torch.equal(a, c) and a.dtype == c.dtype for a, c in zip(labels, plain_labels))
    assert repr({k: v for k, v in s.items() if k not in ("ECE", "MCE", "cECE")}) == repr(plain.summary())   # repr: NaN equals NaN
    # without return_labels the counters are the same; `into` accumulates without the keyword
    alone = seg.evaluate_raw(raw, gts, calibration=True, **call)
    assert isinstance(alone, SegmentationScore) and torch.equal(alone.calibration, cal) and torch.equal(alone.areas, score.areas)
    twice = seg.evaluate_raw(raw, gts, into=alone, **call)
    assert twice is alone and torch.equal(alone.calibration, 2 * cal) and torch.equal(alone.areas, 2 * score.areas)
    assert torch.equal(alone.calibration_tally, 2 * score.calibration_tally)
    # together with the matrix and the bands: each equal to its own reference, and to a call without the keyword
    every = seg.evaluate_raw(raw, gts, calibration=True, confusion=True, boundary_iou=True, **call)
    two = seg.evaluate_raw(raw, gts, confusion=True, boundary_iou=True, **call)
    assert torch.equal(every.calibration, cal) and torch.equal(every.areas, score.areas) and torch.equal(every.tally, score.tally)
    assert torch.equal(every.confusion, two.confusion) and torch.equal(every.boundary, two.boundary)
    assert torch.equal(every.confusion.cpu(), sum(confusion_reference(l.cpu(), g, n) for l, g in zip(labels, gts)))
    assert torch.equal(every.boundary.cpu(), sum(boundary_areas_reference(l.cpu(), g, n, boundary_distance(*g.shape))[0]
                                                 for l, g in zip(labels, gts)))


def test_thresholds_by_measured_precision_feed_the_filter(e2e):  # noqa: F811
    """`precision_thresholds` of an evaluation go into `pseudo_label_raw(thresholds=)` as they are, and on the evaluated images
    every class that keeps pixels is at least `target` right on its kept, scored pixels"""
    m, raw, ocfg, mk = e2e
    n = ocfg.num_seg_tokens
    seg, gts = mk(), _gts(raw, n)
    score = seg.evaluate_raw(raw, gts, calibration=True)
    target = 0.5
    thr = score.precision_thresholds(target)
    assert thr.is_cuda and thr.dtype == torch.int32 and thr.shape == (n,)
    res = seg.pseudo_label_raw(raw, thresholds=thr)
    thr = thr.cpu()
    kept_any = 0
    for c in range(n):
        right = total = 0
        for r, g in zip(res, gts):
            out, g = r.labels.cpu(), g.long()
            here = (out == c + 1) & (g != 0) & (g != 255)
            right, total = right + int((g[here] == c + 1).sum()), total + int(here.sum())
        if int(thr[c]) == 256:
            assert sum(int(r.kept[0, c]) for r in res) == 0
            continue
        kept_any += total
        assert total > 0 and right >= target * total, (c, right, total)
    assert (thr < 256).any() and kept_any > 0


def test_refusals_evaluate_and_task(e2e):  # noqa: F811
    from ifseg_amd.predict import SegmentationScore
    from ifseg_amd.tasks.mm_tasks.segmentation import SegmentationTask
    m, raw, ocfg, mk = e2e
    n = ocfg.num_seg_tokens
    seg, gts = mk(), _gts(raw, n)
    with pytest.raises(ValueError, match=r"confidence must be a probability.*upsample='logits'"):
        mk(upsample="logits").evaluate_raw(raw, gts, calibration=True)
    with pytest.raises(ValueError, match="calibration must be True or False"):
        seg.evaluate_raw(raw, gts, calibration=torch.zeros(n, 256, 2, dtype=torch.int64, device="cuda:0"))
    with pytest.raises(ValueError, match="carries no calibration counters"):
        seg.evaluate_raw(raw, gts, calibration=True, into=SegmentationScore(n, "cuda:0"))
    whole = seg.evaluate_raw(raw, gts, calibration=True)
    task = SegmentationTask(num_seg_tokens=n, patch_image_size=ocfg.patch_image_size, category_token_ids=PC.E2E_NAMES)
    ts = task.evaluate_raw(m, raw, gts, prompt_ids=PC.E2E_PROMPT, calibration=True)
    assert torch.equal(ts.calibration, whole.calibration) and torch.equal(ts.areas, whole.areas)
    assert repr(ts.summary()) == repr(whole.summary()) and "ECE" in ts.summary()
    # the batch call: one launch for the batch
    tiled, gtile = raw[2].repeat(2, 2, 1), gts[2].repeat(2, 2)                        # 128 x 128, the network's own size
    img, g = torch.stack([tiled, tiled.flip(0)]).to("cuda:0"), torch.stack([gtile, gtile.flip(1)])
    a, la = seg.evaluate(img, g, return_labels=True, calibration=True)
    conf = seg(img, return_conf=True).conf
    want = _reference([la], [conf], [g], n)
    assert torch.equal(a.calibration.cpu(), want[0]) and torch.equal(a.calibration_tally.cpu(), want[1]) and int(want[0].sum()) > 0
    c = seg.evaluate(img, g)
    assert c.calibration is None and torch.equal(a.areas, c.areas) and torch.equal(a.tally, c.tally)
