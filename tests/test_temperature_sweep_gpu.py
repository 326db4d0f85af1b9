"""hip.seg_temperature_sweep (csrc/tsweep.hip) and Segmenter.calibrate_raw on the GPU: the integers exactly against the existing
scoring and calibration launches, the floats against the same arithmetic on the existing kernel's probs within the rounding of
an fp64 log and sum, both against the fp64 `predict.temperature_sweep_reference` under the project's 4 e rule; the op, the
refusals, the limits; end to end on the segofa_tiny fixture."""
import ctypes

import pytest
import torch

import _predict_cases as PC
import _score_cases as SC
import _tsweep_cases as TC
from test_predict_views_gpu import e2e  # noqa: F401  (the segofa_tiny fixture with its three raw shapes)

pytestmark = pytest.mark.gpu

BAD_SHAPE, BAD_ARG = -2, -3
_made = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ifseg_amd.ops  # noqa: F401
    return torch.device("cuda:0")


def _case(name):
    """a case on the device with everything the tests of one shape share, computed once and left unchanged: the existing
    kernel's (labels, conf, probs, tally) per grid and the sweep at the default staging"""
    from ifseg_amd import hip
    dev = _dev()
    if name not in _made:
        grids, gt, (hp, wp, n, raw), where = TC.make(name)
        gd, gtd = grids.to(dev), gt.to(dev)
        per_k = []
        for k in range(gd.shape[0]):
            _, tally, labels, conf, probs = hip.seg_score(gd[k], hp, wp, gtd, raw_labels=raw, labels=True, conf=True, probs=True)
            per_k.append((labels, conf, probs, tally))
        _made[name] = (grids, gt, gd, gtd, hp, wp, n, raw, where, per_k, hip.seg_temperature_sweep(gd, hp, wp, gtd, raw))
    return _made[name]


@pytest.mark.parametrize("name", list(TC.SHAPES))
def test_integers_are_the_scoring_and_calibration_launches(name):
    """hist[k] is hip.seg_calibration of seg_score's (labels_k, conf_k) summed over the classes, tally is seg_score's, at the
    default staging and with every tile reading global memory; a second launch into the same counters doubles them; the three
    doctored pixels are where they should be"""
    from ifseg_amd import hip
    grids, gt, gd, gtd, hp, wp, n, raw, where, per_k, (hist, sums, tally) = _case(name)
    K = gd.shape[0]
    assert hist.dtype == torch.int64 and hist.shape == (K, 256, 2) and sums.dtype == torch.float64 and sums.shape == (K, 2)
    assert tally.dtype == torch.int64 and tally.shape == (2,)
    unstaged = hip.seg_temperature_sweep(gd, hp, wp, gtd, raw, staging_bytes=0)
    h2, s2, t2 = hip.seg_temperature_sweep(gd, hp, wp, gtd, raw)
    again = hip.seg_temperature_sweep(gd, hp, wp, gtd, raw, hist=h2, sums=s2, tally=t2)
    assert again[0] is h2 and again[1] is s2 and again[2] is t2
    checks = [(tally == per_k[0][3]).all(), (hist.sum((1, 2)) == tally[0]).all(), tally[0] > 0,
              (tally[1] > 0) == torch.tensor(TC.KINDS[name][2], device=gd.device),
              # staging_bytes=0 gives the same bits in every output; two runs too; the second launch doubles
              (unstaged[0] == hist).all() & (unstaged[1] == sums).all() & (unstaged[2] == tally).all(),
              (h2 == 2 * hist).all() & (t2 == 2 * tally).all() & (s2 == 2 * sums).all()]
    for k, (labels, conf, _, tk) in enumerate(per_k):
        cal, _ = hip.seg_calibration(labels, conf, gtd, n, raw)
        checks += [(hist[k] == cal.sum(0)).all(), (tk == tally).all()]
    y, x, t = where["tie"]
    lab0, conf0, probs0, _ = per_k[0]
    checks += [probs0[0, t, y, x] == probs0[0, t - 1, y, x], lab0[0, y, x] == t - 1, conf0[0, y, x] == probs0[0, t, y, x]]
    y, x, t = where["zero"]
    checks += [probs0[0, t, y, x] == 0.0]
    y, x, t = where["one"]
    checks += [lab0[0, y, x] == t, conf0[0, y, x] >= 255.0 / 256.0, hist[0, 255, 1] >= 1]
    if name not in ("downscale",):
        checks += [conf0[0, y, x] == 1.0]
    got = torch.stack([c.reshape(()) for c in checks]).cpu().tolist()      # the one synchronisation
    assert all(got), got


@pytest.mark.parametrize("name", list(TC.SHAPES))
def test_floats_within_the_rounding_of_fp64(name):
    """the kernel's p_kt and p_kc are seg_score's probs, bit for bit, so against `temperature_sweep_from_probs` of those probs
    on the device only the fp64 log (2 ulp) and the order of an fp64 sum of N <= 2^17 non-negative terms differ:
    |nll - want| <= 2^-35 want, |brier - want| <= 2^-35 sum_i (sum_c p^2 + 2 p_t + 1)"""
    from ifseg_amd.predict import FLT_MIN, temperature_sweep_from_probs
    grids, gt, gd, gtd, hp, wp, n, raw, where, per_k, (hist, sums, tally) = _case(name)
    assert gtd.numel() <= 2 ** 17
    want_h, want_s, want_t = temperature_sweep_from_probs([p for _, _, p, _ in per_k], gtd, n, raw)
    scale = torch.stack([TC.terms(p, gtd, n, raw)[2].sum() for _, _, p, _ in per_k])
    got, want, scale = sums.cpu(), want_s.cpu(), scale.cpu()
    print(name, "nll rel", ((got[:, 0] - want[:, 0]).abs() / want[:, 0]).max().item(), "brier / scale",
          ((got[:, 1] - want[:, 1]).abs() / scale).max().item(), "bound", 2.0 ** -35)
    assert torch.equal(hist.cpu(), want_h.cpu()) and torch.equal(tally.cpu(), want_t.cpu())
    assert ((got[:, 0] - want[:, 0]).abs() <= 2.0 ** -35 * want[:, 0]).all()
    assert ((got[:, 1] - want[:, 1]).abs() <= 2.0 ** -35 * scale).all()
    # the doctored zero costs -log(FLT_MIN), not infinity
    assert torch.isfinite(got).all() and float(got[0, 0]) >= -torch.log(torch.tensor(FLT_MIN, dtype=torch.float64)).item()


@pytest.mark.parametrize("name", list(TC.SHAPES))
def test_against_the_fp64_reference(name):
    """the specification interpolates in fp64, so values move by the coordinate rule's rounding.  The project's rule: with
    e = sum_i |term_i(reference in fp32) - term_i(reference in fp64)| the kernel's per-k sums are within 4 e of the fp64
    reference's -- plus the rounding of the fp64 log and sum order of the test above, 2^-35 of the sum's scale, which is all
    that is left where the two references agree exactly (the identity geometry: e = 0).  Labels are compared only on pixels
    whose fp64 margin exceeds 4 e_value, e_value the largest |value in fp32 - value in fp64| (tests/_predict_cases.py).
    Measured, the largest |kernel - reference| / e over k and both sums: 0.04, 0.18, 0.11, 0.40, 0.19 and (e = 0) 0 on the six
    shapes in SHAPES' order"""
    from ifseg_amd.predict import temperature_sweep_reference, upsample_argmax_reference
    grids, gt, gd, gtd, hp, wp, n, raw, where, per_k, (hist, sums, tally) = _case(name)
    h, w = gt.shape[1:]
    ref_h, ref_s, ref_t = temperature_sweep_reference(grids, hp, wp, gt, raw)
    assert torch.equal(tally.cpu(), ref_t)
    got = sums.cpu()
    worst = 0.0
    for k in range(grids.shape[0]):
        l64, _, p64 = upsample_argmax_reference(grids[k], hp, wp, h, w, torch.float64)
        p32 = upsample_argmax_reference(grids[k], hp, wp, h, w, torch.float32)[2]
        n64, b64, s64, scored = TC.terms(p64, gt, n, raw)
        n32, b32, _, _ = TC.terms(p32, gt, n, raw)
        e_n, e_b = float((n32 - n64).abs().sum()), float((b32 - b64).abs().sum())
        d_n, d_b = abs(float(got[k, 0] - ref_s[k, 0])), abs(float(got[k, 1] - ref_s[k, 1]))
        for d, e in ((d_n, e_n), (d_b, e_b)):
            if e > 0:
                worst = max(worst, d / e)
        print(name, k, "nll", d_n, "e", e_n, "brier", d_b, "e", e_b)
        assert d_n <= 4 * e_n + 2.0 ** -35 * float(n64.sum()) and d_b <= 4 * e_b + 2.0 ** -35 * float(s64.sum()), (k, d_n, e_n, d_b, e_b)
        # labels on the decided pixels
        e_value = float((p32.double() - p64).abs().max())
        lab = per_k[k][0].cpu().long()
        if n > 1:
            top2 = p64.topk(2, dim=1).values
            decided = (top2[:, 0] - top2[:, 1]) >= 4 * e_value
        else:
            decided = torch.ones_like(l64, dtype=torch.bool)
        assert decided.float().mean() > 0.9 and not ((lab != l64) & decided).any()
    print(name, "largest |kernel - fp64 reference| / e over k and both sums:", worst)


def test_two_runs_give_equal_bits():
    from ifseg_amd import hip
    grids, gt, gd, gtd, hp, wp, n, raw, where, per_k, first = _case("k16_odd_ratios")
    second = hip.seg_temperature_sweep(gd, hp, wp, gtd, raw)
    same = torch.stack([(a == b).all() for a, b in zip(first, second)] + [(first[1].view(torch.int64) == second[1].view(torch.int64)).all()])
    assert same.cpu().tolist() == [True] * 4


def test_nothing_but_the_counters_is_written_and_nothing_synchronises():
    """the grids and the ground truth sit between guard bands that keep their pattern, and the call returns while a long
    kernel queued in front of it is still running"""
    from ifseg_amd import hip
    grids, gt, gd, gtd, hp, wp, n, raw, where, per_k, first = _case("x16_two_images")
    dev = gd.device
    buf = torch.full((gd.numel() + 512,), 7.25, device=dev)
    buf[256:256 + gd.numel()] = gd.reshape(-1)
    g = buf[256:256 + gd.numel()].view(gd.shape)
    gbuf = torch.full((gtd.numel() + 256,), 77, dtype=gtd.dtype, device=dev)
    gbuf[128:128 + gtd.numel()] = gtd.reshape(-1)
    gg = gbuf[128:128 + gtd.numel()].view(gtd.shape)
    big = torch.randn(4096, 4096, device=dev)
    torch.cuda.synchronize()
    done = torch.cuda.Event()
    for _ in range(20):
        big = big @ big * 1e-3
    out = hip.seg_temperature_sweep(g, hp, wp, gg, raw)
    done.record()
    still_running = not done.query()                  # the call came back with the queue not drained
    torch.cuda.synchronize()
    assert still_running
    assert all(torch.equal(a, b) for a, b in zip(out, first))
    assert (buf[:256] == 7.25).all() and (buf[256 + gd.numel():] == 7.25).all() and torch.equal(g, gd)
    assert (gbuf[:128] == 77).all() and (gbuf[128 + gtd.numel():] == 77).all() and torch.equal(gg, gtd)


def test_op_matches_the_binding():
    from ifseg_amd import hip
    grids, gt, gd, gtd, hp, wp, n, raw, where, per_k, want = _case("x16_two_images")
    op = torch.ops.ifseg.seg_temperature_sweep
    got = op(gd, hp, wp, gtd, raw)
    assert all(torch.equal(a, b) and a.dtype == b.dtype for a, b in zip(got, want))
    flipped = op(gd, hp, wp, gtd, not raw)
    ref = hip.seg_temperature_sweep(gd, hp, wp, gtd, not raw)
    assert all(torch.equal(a, b) for a, b in zip(flipped, ref)) and not torch.equal(flipped[0], want[0])
    # non-contiguous inputs are copied
    t = op(gd.transpose(0, 1).contiguous().transpose(0, 1), hp, wp, gtd.transpose(1, 2).contiguous().transpose(1, 2), raw)
    assert all(torch.equal(a, b) for a, b in zip(t, want))
    # the fake kernel: shapes and dtypes
    torch.library.opcheck(op, (gd, hp, wp, gtd, raw), test_utils=("test_schema", "test_autograd_registration", "test_faketensor"))
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        side = op(gd, hp, wp, gtd, raw)
    st.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(side, want))
    for bad in (lambda: op(gd.double(), hp, wp, gtd, raw), lambda: op(gd[0], hp, wp, gtd, raw), lambda: op(gd, hp + 1, wp, gtd, raw),
                lambda: op(gd, hp, wp, gtd.long(), raw), lambda: op(gd, hp, wp, gtd[:1], raw), lambda: op(gd, hp, wp, gtd[0], raw),
                lambda: op(gd.repeat(5, 1, 1, 1), hp, wp, gtd, raw), lambda: op(gd[..., :0], hp, wp, gtd, raw)):
        with pytest.raises(ValueError, match="ifseg::seg_temperature_sweep"):
            bad()


def test_limits_are_the_library_s():
    from ifseg_amd import hip
    _dev()
    assert hip.seg_temperature_sweep_limits() == (hip.SEG_SWEEP_MAX_TEMPERATURES, hip.SEG_PREDICT_MAX_CLASSES, 16, 64,
                                                  hip.SEG_SWEEP_STAGING_BYTES) == (16, 512, 16, 64, 31728)
    assert hip.lib().ifseg_seg_temperature_sweep_limit(ctypes.c_int(5)) == BAD_ARG


def test_entry_point_refusals():
    """each refusal returns its code and launches nothing: the counters stay zero; the limits themselves pass"""
    from ifseg_amd import hip
    dev = _dev()
    lib = hip.lib()
    i, vp = ctypes.c_int, ctypes.c_void_p
    p = lambda t, off=0: vp(t.data_ptr() + off)
    grids = torch.full((16 * 4 * 512 + 4,), 1.0 / 512, device=dev)
    gt = torch.ones(64, dtype=torch.int16, device=dev)
    hist, tally = torch.zeros(16 * 512 + 1, dtype=torch.int64, device=dev), torch.zeros(3, dtype=torch.int64, device=dev)
    sums, part = torch.zeros(33, dtype=torch.float64, device=dev), torch.zeros(64, dtype=torch.float64, device=dev)

    def call(g=p(grids), K=2, B=1, hp=2, wp=2, n=5, h=4, w=4, t=p(gt), gb=2, raw=1, hi=p(hist), ta=p(tally), s=p(sums), pa=p(part)):
        return lib.ifseg_seg_temperature_sweep(g, i(K), i(B), i(hp), i(wp), i(n), i(h), i(w), t, i(gb), i(raw), hi, ta, s, pa, None)

    for bad in (dict(g=vp(None)), dict(t=vp(None)), dict(hi=vp(None)), dict(ta=vp(None)), dict(s=vp(None)), dict(pa=vp(None)),
                dict(g=p(grids, 2)), dict(t=p(gt, 1)), dict(hi=p(hist, 4)), dict(ta=p(tally, 4)), dict(s=p(sums, 4)), dict(pa=p(part, 4)),
                dict(K=0), dict(K=17), dict(n=0), dict(n=513), dict(gb=0), dict(gb=3), dict(gb=4)):
        assert call(**bad) == BAD_ARG, bad
    for bad in (dict(B=0), dict(hp=0), dict(wp=0), dict(h=0), dict(w=0), dict(hp=2 ** 15, h=2 ** 15), dict(wp=2 ** 15, w=2 ** 15),
                dict(B=2 ** 11, h=2 ** 10, w=2 ** 10), dict(hp=2 ** 11, wp=2 ** 11)):
        assert call(**bad) == BAD_SHAPE, bad
    torch.cuda.synchronize()
    assert not hist.any() and not tally.any() and not sums.any() and not part.any()                 # no launch so far
    # K = 16 and n = 512 pass, a byte ground truth at an odd address: 4 pixels (0, 1, 0, 1 as bytes from the int16's second
    # byte on): raw 0 ignored, raw 1 = class 0, whose value is 1 / 512 on every grid
    assert call(K=16, n=512, hp=1, wp=1, h=1, w=4, gb=1, t=p(gt, 1), g=p(grids, 16), hi=p(hist, 8), ta=p(tally, 8), s=p(sums, 8),
                pa=p(part, 8)) == 0
    torch.cuda.synchronize()
    assert tally.tolist() == [0, 2, 0] and int(hist.sum()) == 32 and int(hist[1 + 2 * 0 + 1]) == 2      # bin 0, a hit
    want = 2 * torch.log(torch.tensor(512.0, dtype=torch.float64))
    assert torch.allclose(sums[1:33].reshape(16, 2)[:, 0].cpu(), want.expand(16), rtol=2.0 ** -35, atol=0.0)
    assert torch.equal(part[1:33], sums[1:33])


# ------------------------------------------------------------------------------------------------- end to end
TEMPS = (0.5, 1.0, 2.0)


def _gts(raw, n):
    return [SC.ground_truth(tuple(r.shape[:2]), n, True, k, torch.int16 if k == 1 else torch.uint8) for k, r in enumerate(raw)]


@pytest.mark.parametrize("smooth", [0, 1], ids=["softmax", "smoothing"])
def test_calibrate_raw_rows_are_evaluate_raw_at_each_temperature(e2e, smooth):  # noqa: F811
    from ifseg_amd.predict import TemperatureSweep
    m, raw, ocfg, mk = e2e
    n = ocfg.num_seg_tokens
    gts = _gts(raw, n)
    seg = mk(smooth_iters=smooth, temperature=3.0)                # its own temperature is not consulted
    sweep = seg.calibrate_raw(raw, gts, temperatures=TEMPS)
    assert isinstance(sweep, TemperatureSweep) and sweep.hist.is_cuda and sweep.n == n and sweep.temperatures == TEMPS
    for k, T in enumerate(TEMPS):
        score = mk(smooth_iters=smooth, temperature=T).evaluate_raw(raw, gts, calibration=True)
        assert torch.equal(sweep.hist[k], score.calibration.sum(0)) and torch.equal(sweep.tally, score.tally)
        assert torch.equal(sweep.tally[:1], score.calibration_tally[:1]) and int(score.calibration_tally[1]) == 0
    s = sweep.summary()
    assert s["pixels"] == int(sweep.tally[0]) > 0 and s["best"] in TEMPS and len(s["NLL"]) == 3 and all(v > 0 for v in s["NLL"])
    assert all(0 < v < 2 for v in s["Brier"]) and all(0 <= e <= c <= 1 for e, c in zip(s["ECE"], s["MCE"]))
    # into= over two calls equals one call, bit for bit
    two = seg.calibrate_raw(raw[:2], gts[:2], temperatures=TEMPS)
    assert seg.calibrate_raw(raw[2:], gts[2:], temperatures=TEMPS, into=two) is two
    assert torch.equal(two.hist, sweep.hist) and torch.equal(two.tally, sweep.tally) and torch.equal(two.sums, sweep.sums)


def test_task_and_batch_call(e2e):  # noqa: F811
    from ifseg_amd.tasks.mm_tasks.segmentation import SegmentationTask
    m, raw, ocfg, mk = e2e
    n = ocfg.num_seg_tokens
    seg, gts = mk(), _gts(raw, n)
    whole = seg.calibrate_raw(raw, gts, temperatures=TEMPS)
    task = SegmentationTask(num_seg_tokens=n, patch_image_size=ocfg.patch_image_size, category_token_ids=PC.E2E_NAMES)
    ts = task.calibrate_raw(m, raw, gts, prompt_ids=PC.E2E_PROMPT, temperatures=TEMPS)
    assert torch.equal(ts.hist, whole.hist) and torch.equal(ts.sums, whole.sums) and torch.equal(ts.tally, whole.tally)
    assert repr(ts.summary()) == repr(whole.summary())
    seg.temperature = whole.best()
    assert seg.temperature in TEMPS
    # `calibrate` equals `calibrate_raw` on images already at network size: 128 x 128 photos, loaded by the same kernel
    from ifseg_amd import hip
    tiled, gtile = raw[2].repeat(2, 2, 1), gts[2].repeat(2, 2)
    photos, g = [tiled, tiled.flip(0).contiguous()], [gtile, gtile.flip(0).contiguous()]
    a = seg.calibrate_raw(photos, g, temperatures=TEMPS)
    x = hip.image_load(torch.stack(photos).to("cuda:0"), 128, 128)
    b = seg.calibrate(x, torch.stack(g), temperatures=TEMPS)
    assert torch.equal(a.hist, b.hist) and torch.equal(a.tally, b.tally) and int(a.tally[0]) > 0
    # one launch for the batch adds the tiles of both images in one order, two launches image by image: the last bits may differ
    assert torch.allclose(a.sums, b.sums, rtol=2.0 ** -40, atol=0.0)
