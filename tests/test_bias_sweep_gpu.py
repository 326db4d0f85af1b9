"""hip.rows_to_f32_biased, hip.seg_score_grids (csrc/bsweep.hip) and the Segmenter's class_bias / bias_sweep_raw on the GPU: the
biased rows exactly (copy mode, bias 0) and within `_post_cases.softmax_ref`'s bound (softmax mode); the sweep's counters
exactly against the existing scoring and predict launches on every case of tests/_bias_sweep_cases.py; the limits, the
refusals; end to end on the segofa_tiny fixture."""
import ctypes

import numpy as np
import pytest
import torch

import _bias_sweep_cases as BC
import _post_cases as pc
import _predict_cases as PC
import _score_cases as SC
from test_predict_views_gpu import e2e  # noqa: F401  (the segofa_tiny fixture with its three raw shapes)

pytestmark = pytest.mark.gpu

BAD_SHAPE, BAD_ARG = -2, -3
_made = {}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ifseg_amd.ops  # noqa: F401
    return torch.device("cuda:0")


def _bits(t):
    return t.view(torch.int32)


# ------------------------------------------------------------------------------------------------- the biased rows
def _pad(n, dev):
    x = pc.softmax_logits(n)                                   # bf16-exact, [2, 70, n + 5], |x| <= 1.25
    return x, torch.from_numpy(np.array(x, dtype=np.float32)).to(torch.bfloat16).to(dev)


def _bias_of(n, dev, seed=0):
    b = torch.rand(n, generator=torch.Generator().manual_seed(660 + n + seed)) * 2.5 - 1.25
    return b, b.to(dev)


@pytest.mark.parametrize("n", pc.SOFTMAX_NS)
def test_biased_rows_copy_mode_is_one_fp32_subtraction(n):
    from ifseg_amd import hip
    dev = _dev()
    x, pad = _pad(n, dev)
    b, bd = _bias_of(n, dev)
    got = hip.rows_to_f32_biased(pad, n, pc.SOFTMAX_RPB, bd)
    want = x[:, :pc.SOFTMAX_RPB, :n].astype(np.float32) - b.numpy()[None, None]
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, pc.SOFTMAX_RPB, n)
    assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))
    # the temperature is not applied in copy mode
    assert torch.equal(_bits(hip.rows_to_f32_biased(pad, n, pc.SOFTMAX_RPB, bd, temperature=0.5)), _bits(got))


@pytest.mark.parametrize("temp", [1.0, 0.5, 2.0])
@pytest.mark.parametrize("n", pc.SOFTMAX_NS)
def test_biased_rows_softmax_within_the_bound(n, temp):
    from ifseg_amd import hip
    dev = _dev()
    x, pad = _pad(n, dev)
    b, bd = _bias_of(n, dev, 1)
    got = hip.rows_to_f32_biased(pad, n, pc.SOFTMAX_RPB, bd, softmax=True, temperature=temp).double().cpu().numpy()
    a = (x[:, :pc.SOFTMAX_RPB, :n].astype(np.float64) - b.double().numpy()[None, None]) / temp
    e = np.exp(a - a.max(-1, keepdims=True))
    ref = e / e.sum(-1, keepdims=True)
    r, at = pc.worst_ratio(got, ref, (16 + 2 * n) * pc.U * ref)
    print("rows_to_f32_biased n=%d T=%g: %.3f of the bound at %s" % (n, temp, r, at))
    assert r <= 1.0, (r, at)


@pytest.mark.parametrize("n", pc.SOFTMAX_NS)
def test_zero_bias_gives_the_plain_kernel_s_bits(n):
    from ifseg_amd import hip
    dev = _dev()
    _, pad = _pad(n, dev)
    zero = torch.zeros(n, device=dev)
    checks = [(_bits(hip.rows_to_f32_biased(pad, n, pc.SOFTMAX_RPB, zero)) == _bits(hip.rows_to_f32(pad, n, pc.SOFTMAX_RPB))).all()]
    for temp in (1.0, 0.5, 2.0, 0.7):
        a = hip.rows_to_f32_biased(pad, n, pc.SOFTMAX_RPB, zero, softmax=True, temperature=temp)
        b = hip.rows_to_f32(pad, n, pc.SOFTMAX_RPB, softmax=True, temperature=temp)
        checks.append((_bits(a) == _bits(b)).all())
    assert torch.stack(checks).cpu().tolist() == [True] * 5


def test_biased_rows_sit_between_canaries():
    """the C entry on an output inside a guarded allocation, both modes; the logits and the bias keep their bits"""
    from ifseg_amd import hip
    dev = _dev()
    n, rows = 5, 127
    _, pad = _pad(n, dev)
    _, bd = _bias_of(n, dev)
    pad0, b0 = pad.clone(), bd.clone()
    i, ll, f, vp = ctypes.c_int, ctypes.c_longlong, ctypes.c_float, ctypes.c_void_p
    for softmax in (0, 1):
        full = torch.full((rows * n + 64,), -77.5, device=dev)
        out = full[32:32 + rows * n]
        assert hip.lib().ifseg_softmax_rows_bias(vp(pad.data_ptr()), ll(pad.stride(0)), i(pc.SOFTMAX_RPB), i(pad.stride(1)),
                                                 vp(bd.data_ptr()), vp(out.data_ptr()), i(rows), i(n), f(2.0), i(softmax),
                                                 hip._stream()) == 0
        want = hip.rows_to_f32_biased(pad, n, pc.SOFTMAX_RPB, bd, softmax=bool(softmax), temperature=0.5).reshape(-1, n)[:rows]
        assert torch.equal(_bits(out.view(rows, n)), _bits(want))
        assert bool((full[:32] == -77.5).all()) and bool((full[32 + rows * n:] == -77.5).all())
    assert torch.equal(pad.view(torch.int16), pad0.view(torch.int16)) and torch.equal(_bits(bd), _bits(b0))


def test_smoothing_with_zero_bias_is_the_plain_smoothing():
    from ifseg_amd import hip
    dev = _dev()
    n, P, D = 5, 64, 64
    _, pad = _pad(n, dev)                                      # [2, 70, 10]: 64 patch rows and more
    feat = torch.randn(2, P, D, generator=torch.Generator().manual_seed(5)).to(torch.bfloat16).to(dev)
    plain = hip.neighbour_smoothing(pad, n, feat, 2, 3, 0.5)
    zero = hip.neighbour_smoothing(pad, n, feat, 2, 3, 0.5, bias=torch.zeros(n, device=dev))
    _, bd = _bias_of(n, dev)
    moved = hip.neighbour_smoothing(pad, n, feat, 2, 3, 0.5, bias=bd)
    assert torch.equal(_bits(plain), _bits(zero)) and not torch.equal(moved, plain)
    assert torch.allclose(moved.sum(-1), torch.ones(2, P, device=dev), rtol=0, atol=1e-5)          # still probabilities


# ------------------------------------------------------------------------------------------------- the scoring launch
def _case(name):
    """a case on the device with what the tests of one shape share, computed once and left unchanged: the existing kernels'
    (areas, tally, labels, probs) per grid and the sweep's counters at the default staging"""
    from ifseg_amd import hip
    dev = _dev()
    if name not in _made:
        grids, gt, (hp, wp, n, raw), where = BC.make(name)
        gd, gtd = grids.to(dev), gt.to(dev)
        h, w = gt.shape[1:]
        per_k = []
        for k in range(gd.shape[0]):
            areas, tally = hip.seg_score(gd[k], hp, wp, gtd, raw_labels=raw)[:2]
            labels, _, probs = hip.seg_predict(gd[k], hp, wp, h, w, probs=True)
            per_k.append((areas, tally, labels, probs))
        _made[name] = (gd, gtd, hp, wp, n, raw, where, per_k, hip.seg_score_grids(gd, hp, wp, gtd, raw))
    return _made[name]


@pytest.mark.parametrize("name", list(BC.SHAPES))
def test_rows_are_the_scoring_launch_s_counters(name):
    """row k is hip.seg_score's areas of grid k and tally is its tally, at the default staging and with every tile reading
    global memory; row k is areas_reference of hip.seg_predict's values under the first-maximum rule; the ground truth may
    sit at any element offset; a second launch into the same counters doubles them; two launches give equal bits; the three
    doctored pixels are labelled as the rule says"""
    from ifseg_amd import hip
    from ifseg_amd.predict import areas_reference, first_maximum
    gd, gtd, hp, wp, n, raw, where, per_k, (areas, tally) = _case(name)
    K = gd.shape[0]
    assert areas.dtype == torch.int64 and tuple(areas.shape) == (K, 3, n) and tally.dtype == torch.int64 and tuple(tally.shape) == (2,)
    unstaged = hip.seg_score_grids(gd, hp, wp, gtd, raw, staging_bytes=0)
    a2, t2 = hip.seg_score_grids(gd, hp, wp, gtd, raw)
    again = hip.seg_score_grids(gd, hp, wp, gtd, raw, areas=a2, tally=t2)
    assert again[0] is a2 and again[1] is t2
    checks = [tally[0] > 0, (tally[1] > 0) == torch.tensor(BC.KINDS[name][2], device=gd.device),
              (areas[:, 1].sum(1) == tally[0]).all() & (areas[:, 2].sum(1) == tally[0]).all(),
              (unstaged[0] == areas).all() & (unstaged[1] == tally).all(), (a2 == 2 * areas).all() & (t2 == 2 * tally).all()]
    second = hip.seg_score_grids(gd, hp, wp, gtd, raw)
    checks += [(second[0] == areas).all() & (second[1] == tally).all()]
    for k, (ak, tk, labels, probs) in enumerate(per_k):
        checks += [(areas[k] == ak).all(), (tk == tally).all()]
        lab = first_maximum(probs)
        ref_a, ref_t = areas_reference(lab, gtd, n, raw)
        checks += [(lab == labels.long()).all(), (areas[k] == ref_a).all(), (tally == ref_t).all()]
        for kind, (y, x, t) in where.items():
            checks.append(labels[0, y, x] == {"tie": t - 1, "nan": 0, "allnan": 0}[kind])
    # the ground truth in views at element offsets 0, 1 and 3 of a larger allocation, the counters between canaries
    for off in (0, 1, 3):
        gbuf = torch.full((gtd.numel() + 8,), 77, dtype=gtd.dtype, device=gd.device)
        gbuf[off:off + gtd.numel()] = gtd.reshape(-1)
        gv = gbuf[off:off + gtd.numel()].view(gtd.shape)
        abuf = torch.full((areas.numel() + 16,), -5, dtype=torch.int64, device=gd.device)
        tbuf = torch.full((2 + 16,), -5, dtype=torch.int64, device=gd.device)
        av, tv = abuf[8:8 + areas.numel()].view(areas.shape), tbuf[8:10]
        av.zero_()
        tv.zero_()
        got = hip.seg_score_grids(gd, hp, wp, gv, raw, areas=av, tally=tv, staging_bytes=None if off != 1 else 0)
        checks += [(got[0] == areas).all() & (got[1] == tally).all(), (abuf[:8] == -5).all() & (abuf[8 + areas.numel():] == -5).all(),
                   (tbuf[:8] == -5).all() & (tbuf[10:] == -5).all(), (gbuf[:off] == 77).all() & (gbuf[off + gtd.numel():] == 77).all()]
    got = torch.stack([c.reshape(()) for c in checks]).cpu().tolist()      # the one synchronisation
    assert all(got), got


def test_limits_are_the_library_s():
    from ifseg_amd import hip
    _dev()
    assert hip.seg_score_grids_limits() == (hip.SEG_SCORE_GRIDS_MAX, hip.SEG_PREDICT_MAX_CLASSES, 16, 64,
                                            hip.SEG_SCORE_GRIDS_STAGING_BYTES) == (16, 512, 16, 64, 59376)
    assert hip.lib().ifseg_seg_score_grids_limit(ctypes.c_int(5)) == BAD_ARG


def test_entry_point_refusals():
    """each refusal returns its code and launches nothing: the counters stay zero; the limits themselves pass"""
    from ifseg_amd import hip
    dev = _dev()
    lib = hip.lib()
    i, vp = ctypes.c_int, ctypes.c_void_p
    p = lambda t, off=0: vp(t.data_ptr() + off)
    grids = torch.full((16 * 4 * 512 + 4,), 0.25, device=dev)
    gt = torch.ones(64, dtype=torch.int16, device=dev)
    areas, tally = torch.zeros(16 * 3 * 512 + 1, dtype=torch.int64, device=dev), torch.zeros(3, dtype=torch.int64, device=dev)

    def call(g=p(grids), K=2, B=1, hp=2, wp=2, n=5, h=4, w=4, t=p(gt), gb=2, raw=1, ar=p(areas), ta=p(tally)):
        return lib.ifseg_seg_score_grids(g, i(K), i(B), i(hp), i(wp), i(n), i(h), i(w), t, i(gb), i(raw), ar, ta, None)

    for bad in (dict(g=vp(None)), dict(t=vp(None)), dict(ar=vp(None)), dict(ta=vp(None)), dict(g=p(grids, 2)), dict(t=p(gt, 1)),
                dict(ar=p(areas, 4)), dict(ta=p(tally, 4)), dict(K=0), dict(K=17), dict(n=0), dict(n=513), dict(gb=0), dict(gb=3),
                dict(ta=p(areas, 8)), dict(ar=p(tally)), dict(ar=p(grids)), dict(ta=p(gt))):
        assert call(**bad) == BAD_ARG, bad
    for bad in (dict(B=0), dict(hp=0), dict(wp=0), dict(h=0), dict(w=0), dict(hp=2 ** 15, h=2 ** 15), dict(wp=2 ** 15, w=2 ** 15),
                dict(B=2 ** 11, h=2 ** 10, w=2 ** 10), dict(hp=2 ** 11, wp=2 ** 11)):
        assert call(**bad) == BAD_SHAPE, bad
    torch.cuda.synchronize()
    assert not areas.any() and not tally.any()                    # no launch so far
    # K = 16 and n = 512 pass, a byte ground truth at an odd address: 4 pixels (0, 1, 0, 1 as bytes from the int16's second
    # byte on): raw 0 ignored, raw 1 = class 0; every value of a grid is 0.25, so the first maximum is class 0: two hits per k
    assert call(K=16, n=512, hp=1, wp=1, h=1, w=4, gb=1, t=p(gt, 1), g=p(grids, 16), ar=p(areas, 8), ta=p(tally, 8)) == 0
    torch.cuda.synchronize()
    a = areas[1:].reshape(16, 3, 512)
    assert tally.tolist() == [0, 2, 0] and a[:, :, 0].tolist() == [[2, 2, 2]] * 16 and int(a.sum()) == 96 and int(areas[0]) == 0


# ------------------------------------------------------------------------------------------------- end to end
GS = (0.0, 0.75, -0.5, 2.0)


def _gts(raw, n):
    return [SC.ground_truth(tuple(r.shape[:2]), n, True, k, torch.int16 if k == 1 else torch.uint8) for k, r in enumerate(raw)]


def _vectors(n, dev):
    g = torch.Generator().manual_seed(77)
    return torch.randn(n, generator=g).to(dev), (0.5 * torch.randn(n, generator=g)).to(dev)


def test_zero_class_bias_is_the_plain_segmenter_and_a_bias_is_the_biased_rows(e2e):  # noqa: F811
    from ifseg_amd import hip
    m, raw, ocfg, mk = e2e
    n, dev = ocfg.num_seg_tokens, torch.device("cuda:0")
    for kw in (dict(), dict(upsample="logits"), dict(smooth_iters=2, temperature=0.5)):
        plain, zero = mk(**kw), mk(class_bias=torch.zeros(n), **kw)
        assert zero.class_bias.is_cuda and zero.class_bias.dtype == torch.float32
        for a, b in zip(plain.segment_raw(raw, return_conf=True), zero.segment_raw(raw, return_conf=True)):
            assert torch.equal(a.labels, b.labels) and torch.equal(_bits(a.conf), _bits(b.conf))
    d, _ = _vectors(n, dev)
    P = ocfg.patch_image_size
    x = hip.image_load(torch.stack([raw[2], raw[2].flip(0).contiguous()]).to(dev), P, P)
    for kw in (dict(temperature=2.0), dict(upsample="logits", temperature=2.0)):
        seg = mk(class_bias=d, **kw)
        pad, hp, wp, _ = seg._padded_logits(x)
        want = hip.rows_to_f32_biased(pad, n, hp * wp, d, softmax=seg.upsample == "probs", temperature=2.0)
        got, hp2, wp2 = seg.patch_scores(x)
        assert (hp2, wp2) == (hp, wp) and torch.equal(_bits(got), _bits(want)) and not torch.equal(got, mk(**kw).patch_scores(x)[0])
        if seg.upsample == "logits":                              # by hand: one fp32 subtraction
            assert torch.equal(_bits(got), _bits(pad[:, :hp * wp, :n].float() - d))
        grids = seg.patch_scores_biased(x, [d, torch.zeros(n, device=dev)])[0]
        assert torch.equal(_bits(grids[0]), _bits(got)) and torch.equal(_bits(grids[1]), _bits(mk(**kw).patch_scores(x)[0]))


@pytest.mark.parametrize("with_origin", [False, True], ids=["no_origin", "origin"])
@pytest.mark.parametrize("mode", ["probs", "logits", "smoothing"])
def test_bias_sweep_raw_rows_are_evaluate_raw_at_each_strength(e2e, mode, with_origin):  # noqa: F811
    from ifseg_amd.predict import BiasSweep, scaled_bias
    m, raw, ocfg, mk = e2e
    n, dev = ocfg.num_seg_tokens, torch.device("cuda:0")
    kw = dict(probs=dict(temperature=0.5), logits=dict(upsample="logits"), smoothing=dict(smooth_iters=2))[mode]
    d, o = _vectors(n, dev)
    origin = o if with_origin else None
    gts = _gts(raw, n)
    seg = mk(class_bias=origin, **kw)
    sweep = seg.bias_sweep_raw(raw, gts, d, strengths=GS)
    assert isinstance(sweep, BiasSweep) and sweep.areas.is_cuda and sweep.n == n and sweep.strengths == GS
    assert torch.equal(sweep.origin, o if with_origin else torch.zeros(n, device=dev)) and torch.equal(sweep.direction, d)
    rows = []
    for k, g in enumerate(GS):
        b = scaled_bias(d, g, origin)
        assert torch.equal(b, sweep.bias(k))
        score = mk(class_bias=b, **kw).evaluate_raw(raw, gts)
        rows.append(score.areas)
        assert torch.equal(sweep.areas[k], score.areas) and torch.equal(sweep.tally, score.tally)
    # strength 0 reproduces the Segmenter; the strengths are not all the same label map
    assert torch.equal(sweep.areas[0], seg.evaluate_raw(raw, gts).areas) and not torch.equal(rows[0], rows[3])
    s = sweep.summary({"low": list(range(n // 2)), "high": list(range(n // 2, n))})
    assert s["pixels"] == int(sweep.tally[0]) > 0 and len(s["mIoU"]) == len(s["hIoU"]) == 4 and sweep.best() in GS
    # into= over two calls equals one call
    two = seg.bias_sweep_raw(raw[:2], gts[:2], d, strengths=GS)
    assert seg.bias_sweep_raw(raw[2:], gts[2:], d, strengths=GS, into=two) is two
    assert torch.equal(two.areas, sweep.areas) and torch.equal(two.tally, sweep.tally)


def test_task_and_batch_call(e2e):  # noqa: F811
    from ifseg_amd import hip
    from ifseg_amd.tasks.mm_tasks.segmentation import SegmentationTask
    m, raw, ocfg, mk = e2e
    n, dev = ocfg.num_seg_tokens, torch.device("cuda:0")
    d, o = _vectors(n, dev)
    seg, gts = mk(class_bias=o), _gts(raw, n)
    whole = seg.bias_sweep_raw(raw, gts, d, strengths=GS)
    task = SegmentationTask(num_seg_tokens=n, patch_image_size=ocfg.patch_image_size, category_token_ids=PC.E2E_NAMES)
    ts = task.bias_sweep_raw(m, raw, gts, d, prompt_ids=PC.E2E_PROMPT, strengths=GS, class_bias=o)
    assert torch.equal(ts.areas, whole.areas) and torch.equal(ts.tally, whole.tally) and repr(ts.summary()) == repr(whole.summary())
    seg.class_bias = whole.bias(whole.best())
    assert torch.equal(seg.evaluate_raw(raw, gts).areas, whole.areas[GS.index(whole.best())])
    # `bias_sweep` equals `bias_sweep_raw` on images already at network size
    seg = mk(class_bias=o)
    tiled, gtile = raw[2].repeat(2, 2, 1), gts[2].repeat(2, 2)
    photos, g = [tiled, tiled.flip(0).contiguous()], [gtile, gtile.flip(0).contiguous()]
    a = seg.bias_sweep_raw(photos, g, d, strengths=GS)
    b = seg.bias_sweep(hip.image_load(torch.stack(photos).to(dev), 128, 128), torch.stack(g), d, strengths=GS)
    assert torch.equal(a.areas, b.areas) and torch.equal(a.tally, b.tally) and int(a.tally[0]) > 0


@pytest.mark.parametrize("setting", ["slide", "msflip", "sieve"])
def test_class_bias_holds_in_every_setting(e2e, setting):  # noqa: F811
    """the labels of `segment_raw` with `class_bias` are those of a plain Segmenter whose grids are biased by hand: every
    forward of the setting (windows, views) passes through the bias"""
    from ifseg_amd import hip
    m, raw, ocfg, mk = e2e
    n, dev = ocfg.num_seg_tokens, torch.device("cuda:0")
    d, _ = _vectors(n, dev)
    ctor, call = dict(slide=({}, dict(slide=True)), msflip=({}, dict(scales=(0.5, 1.0), flip=True)),
                      sieve=(dict(sieve=8, upsample="logits"), {}))[setting]
    plain = mk(**ctor)

    def by_hand(x):
        pad, hp, wp, _ = plain._padded_logits(x)
        if plain.upsample == "logits":                            # one fp32 subtraction, in torch
            return (pad[:, :hp * wp, :n].float() - d).contiguous(), hp, wp
        return hip.rows_to_f32_biased(pad, n, hp * wp, d, softmax=True, temperature=plain.temperature), hp, wp

    plain.patch_scores = by_hand
    want = plain.segment_raw(raw, **call)
    got = mk(class_bias=d, **ctor).segment_raw(raw, **call)
    unbiased = mk(**ctor).segment_raw(raw, **call)
    assert all(torch.equal(a.labels, b.labels) for a, b in zip(got, want))
    assert not all(torch.equal(a.labels, b.labels) for a, b in zip(got, unbiased))
