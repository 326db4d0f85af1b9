"""GPU: pixel-adaptive mask refinement, csrc/pamr.hip -- hip.pamr_affinity, hip.pamr_iterate and hip.seg_pamr against the fp64
specification `predict.pamr_reference` under the rule of tests/_pamr_cases.py (values within 4 e, labels wherever the top-2
margin is >= 32 e), the properties the binding promises (the right ping-pong buffer, probs untouched, equal bits of two runs,
label 0 on ties), the raw C entries' refusals, the op through the dispatcher, and Segmenter(pamr_iters=) end to end on the
segofa_tiny fixture.  Every test prints the figures it asserts on."""
import ctypes

import pytest
import torch

import _pamr_cases as C
import _score_cases as SC
from test_predict_views_gpu import e2e  # noqa: F401  (the segofa_tiny fixture with its three raw shapes)

pytestmark = pytest.mark.gpu

BAD_SHAPE, BAD_ARG = -2, -3


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ifseg_amd.ops  # noqa: F401
    return torch.device("cuda:0")


@pytest.mark.parametrize("name", list(C.CASES))
def test_affinity_is_the_specification(name):
    from ifseg_amd import hip
    dev, c = _dev(), C.case(name)
    w = hip.pamr_affinity(c.image.to(dev), c.dilations)
    assert w.shape == c.w64.shape and w.dtype == torch.float32
    d = (w.cpu().double() - c.w64).abs().max().item()
    print("%s: weights |kernel - specification| = %.3g = %.2f e (e = %.3g)" % (name, d, d / c.e_w, c.e_w))
    assert d <= C.VALUE_FACTOR * c.e_w, (name, d, c.e_w)
    assert (w.sum(0).cpu() - 1).abs().max().item() <= 1e-5 and w.min().item() >= 0


@pytest.mark.parametrize("name", list(C.CASES))
def test_iterate_on_the_specifications_weights(name):
    """the gather and the dot product alone: the fp32 weights of the specification in, the fp64 iteration of those weights as
    the reference"""
    from ifseg_amd import hip
    dev, c = _dev(), C.case(name)
    w, src = c.w32.to(dev).contiguous(), c.values.to(dev)
    for _ in range(c.iters):
        dst = torch.full_like(src, float("nan"))
        hip.pamr_iterate(w, src, dst, c.dilations)
        src = dst
    d = (src.cpu().double() - c.iter64).abs().max().item()
    print("%s: iterate |kernel - fp64| = %.3g = %.2f e (e = %.3g)" % (name, d, d / c.e_iter, c.e_iter))
    assert d <= C.VALUE_FACTOR * c.e_iter, (name, d, c.e_iter)


@pytest.mark.parametrize("name", list(C.CASES))
def test_seg_pamr_is_the_specification(name):
    from ifseg_amd import hip
    dev, c = _dev(), C.case(name)
    probs = c.values.to(dev)
    keep = probs.clone()
    labels, conf, out = hip.seg_pamr(probs, c.image.to(dev), c.iters, c.dilations, conf=True, probs_out=True)
    assert labels.dtype == (torch.uint8 if c.n <= 256 else torch.int16) and tuple(labels.shape) == (c.H, c.W)
    c.check(labels, conf, out)
    # conf is the value at the returned label, the label its first maximum; the input is untouched
    assert torch.equal(conf, out.gather(0, labels.long()[None])[0]) and torch.equal(labels.long(), out.argmax(0))
    assert torch.equal(probs, keep)
    # two runs give equal bits; the outputs that were not asked for are None
    l2, c2, o2 = hip.seg_pamr(probs, c.image.to(dev), c.iters, c.dilations, conf=True, probs_out=True)
    assert torch.equal(l2, labels) and torch.equal(c2, conf) and torch.equal(o2, out)
    l3, c3, o3 = hip.seg_pamr(probs, c.image.to(dev), c.iters, c.dilations)
    assert torch.equal(l3, labels) and c3 is None and o3 is None


@pytest.mark.parametrize("iters", [1, 2, 3])
def test_odd_and_even_iteration_counts_return_the_right_buffer(iters):
    from ifseg_amd import hip
    dev, c = _dev(), C.case("ten_iters")
    img, probs = c.image.to(dev), c.values.to(dev)
    keep = probs.clone()
    labels, conf, out = hip.seg_pamr(probs, img, iters, c.dilations, conf=True, probs_out=True)
    w, src = hip.pamr_affinity(img, c.dilations), probs
    for _ in range(iters):
        src = hip.pamr_iterate(w, src, torch.empty_like(probs), c.dilations)
    assert torch.equal(out, src) and torch.equal(probs, keep) and out.data_ptr() != probs.data_ptr()
    assert torch.equal(labels.long(), src.argmax(0)) and torch.equal(conf, src.amax(0))
    ref = C.pamr_reference(c.image, c.values, c.dilations, iters, torch.float64)[2]
    assert (out.cpu().double() - ref).abs().max().item() <= C.VALUE_FACTOR * c.e


def test_ties_give_label_zero_and_int16_labels():
    from ifseg_amd import hip
    dev, c = _dev(), C.case("int16")
    flat = torch.full((c.n, c.H, c.W), 1.0 / 256, device=dev)           # exact in fp32: every convex combination is the value
    labels, conf, out = hip.seg_pamr(flat, c.image.to(dev), 2, c.dilations, conf=True, probs_out=True)
    assert labels.dtype == torch.int16 and int(labels.abs().max()) == 0
    for n in (3, 256):
        labels, _, _ = hip.seg_pamr(flat[:n].contiguous(), c.image.to(dev), 1, c.dilations)
        assert labels.dtype == torch.uint8 and int(labels.max()) == 0
    labels, _, _ = hip.seg_pamr(flat[:3].contiguous(), c.image.to(dev), 1, c.dilations, label_dtype=torch.int16)
    assert labels.dtype == torch.int16


def test_limits_and_entry_point_refusals():
    from ifseg_amd import hip
    dev = _dev()
    assert hip.seg_pamr_limits() == (hip.SEG_PAMR_MAX_DILATIONS, hip.SEG_PAMR_MAX_DILATION, hip.SEG_PREDICT_MAX_CLASSES) == (8, 32, 512)
    lib, i, p = hip.lib(), ctypes.c_int, ctypes.c_void_p
    H, W, n = 6, 9, 3
    img = torch.zeros(H, W, 3, dtype=torch.uint8, device=dev)
    w = torch.zeros(8 * 8, H, W, device=dev)
    src, dst = torch.zeros(n, H, W, device=dev), torch.full((n, H, W), 5.0, device=dev)
    lab = torch.full((H, W), 9, dtype=torch.uint8, device=dev)
    arr = lambda *d: (i * max(len(d), 1))(*d)

    def aff(image=img, h=H, ww=W, d=(1, 2), D=None, out=w):
        return lib.ifseg_pamr_affinity(p(image.data_ptr()) if image is not None else None, i(h), i(ww), arr(*d) if d is not None else None,
                                       i(len(d) if D is None else D), p(out.data_ptr()) if out is not None else None, None)

    def it(ww=w, s=src, d_=dst, nn=n, h=H, wd=W, d=(1, 2), D=None, labels=None, lb=0):
        return lib.ifseg_pamr_iterate(p(ww.data_ptr()) if ww is not None else None, p(s.data_ptr()) if s is not None else None,
                                      p(d_.data_ptr()) if d_ is not None else None, i(nn), i(h), i(wd), arr(*d), i(len(d) if D is None else D),
                                      p(labels.data_ptr()) if labels is not None else None, i(lb), None, None)

    for rc, want in ((aff(image=None), BAD_ARG), (aff(out=None), BAD_ARG), (aff(d=None, D=1), BAD_ARG), (aff(D=0), BAD_ARG), (aff(d=(1,) * 9), BAD_ARG),
                     (aff(d=(0,)), BAD_ARG), (aff(d=(1, 33)), BAD_ARG), (aff(h=0), BAD_SHAPE), (aff(ww=-1), BAD_SHAPE),
                     (aff(h=1 << 15, ww=1 << 14, d=(1,)), BAD_SHAPE),
                     (it(ww=None), BAD_ARG), (it(s=None), BAD_ARG), (it(d_=None), BAD_ARG), (it(nn=0), BAD_ARG), (it(nn=513), BAD_ARG),
                     (it(d=(1, 40)), BAD_ARG), (it(D=9, d=(1,) * 9), BAD_ARG), (it(d_=src), BAD_ARG), (it(d_=w), BAD_ARG),
                     (it(labels=lab, lb=3), BAD_ARG), (it(labels=lab, lb=1, nn=257), BAD_ARG), (it(h=0), BAD_SHAPE),
                     (it(nn=512, h=1 << 12, wd=1 << 10), BAD_SHAPE)):
        assert rc == want, (rc, want)
    torch.cuda.synchronize()
    # nothing was launched on a refusal
    assert float(dst.min()) == 5.0 and int(lab.min()) == 9 and float(w.abs().max()) == 0.0
    assert lib.ifseg_pamr_limit(i(3)) == BAD_ARG


def test_op_matches_binding():
    from ifseg_amd import hip
    dev, c = _dev(), C.case("thin_last_tile")
    probs, img = c.values.to(dev), c.image.to(dev)
    want = hip.seg_pamr(probs, img, 2, (1, 4), conf=True, probs_out=True)
    got = torch.ops.ifseg.seg_pamr(probs, img, 2, [1, 4], True, True)
    assert all(torch.equal(a, b) and a.dtype == b.dtype for a, b in zip(got, want))
    labels, conf, out = torch.ops.ifseg.seg_pamr(probs, img, 2, [1, 4], False, False)
    assert torch.equal(labels, want[0]) and conf.numel() == 0 and out.numel() == 0
    # on a side stream the op follows PyTorch's current stream
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        again = torch.ops.ifseg.seg_pamr(probs, img, 2, [1, 4], True, True)
    st.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(again, want))


# ------------------------------------------------------------------------------------------------- end to end
SETTINGS = {"single": ({}, {}), "ms_flip": ({}, {"scales": (0.75, 1.0), "flip": True}), "slide": ({}, {"slide": True}),
            "slide_views": ({"slide_views": True}, {"slide": True, "scales": (0.75, 1.0), "flip": True})}


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_segmenter_with_pamr(e2e, setting):  # noqa: F811
    """`segment_raw` with pamr_iters=2 is, bit for bit, `hip.seg_pamr` of the values a Segmenter without it returns and the
    original photo; `evaluate_raw` counts exactly those labels"""
    from ifseg_amd import hip
    from ifseg_amd.predict import areas_reference, confusion_reference
    m, raw, ocfg, mk = e2e
    n = ocfg.num_seg_tokens
    kw, call = SETTINGS[setting]
    dil = (1, 2, 4)
    plain, seg = mk(**kw), mk(pamr_iters=2, pamr_dilations=dil, **kw)
    base = plain.segment_raw(raw, return_probs=True, **call)
    got = seg.segment_raw(raw, return_conf=True, return_probs=True, **call)
    changed = 0
    for b, g, r in zip(base, got, raw):
        labels, conf, probs = hip.seg_pamr(b.probs.contiguous(), r.to("cuda:0"), 2, dil, conf=True, probs_out=True)
        assert torch.equal(g.labels, labels) and torch.equal(g.conf, conf) and torch.equal(g.probs, probs)
        assert g.labels.dtype == b.labels.dtype and tuple(g.labels.shape) == tuple(r.shape[:2])
        changed += int((probs != b.probs).sum())
    assert changed > 0                                                  # the refinement did something
    only = seg.segment_raw(raw, **call)
    assert all(torch.equal(a.labels, b.labels) and a.conf is None and a.probs is None for a, b in zip(only, got))
    # scored: areas, tally and the matrix are the specification's of those labels
    gts = [SC.ground_truth(tuple(r.shape[:2]), n, True, k, torch.int16 if k == 1 else torch.uint8) for k, r in enumerate(raw)]
    score, labels = seg.evaluate_raw(raw, gts, confusion=True, return_labels=True, **call)
    assert all(torch.equal(a, b.labels) for a, b in zip(labels, got))
    want = [areas_reference(l.cpu(), g, n) for l, g in zip(labels, gts)]
    assert torch.equal(score.areas.cpu(), sum(a for a, _ in want)) and torch.equal(score.tally.cpu(), sum(t for _, t in want))
    assert torch.equal(score.confusion.cpu(), sum(confusion_reference(l.cpu(), g, n) for l, g in zip(labels, gts)))
    assert int(score.tally[0]) > 0


def test_segmenter_calibration_render_and_pseudo_labels_with_pamr(e2e):  # noqa: F811
    """what sits behind the conf: the calibration counters, `render_raw(fade_by_conf=True)` and `pseudo_label_raw` take
    `seg_pamr`'s labels and conf"""
    from ifseg_amd import hip
    from ifseg_amd.predict import calibration_reference
    m, raw, ocfg, mk = e2e
    n = ocfg.num_seg_tokens
    seg = mk(pamr_iters=1, pamr_dilations=(1, 3))
    got = seg.segment_raw(raw, return_conf=True)
    gts = [SC.ground_truth(tuple(r.shape[:2]), n, True, k) for k, r in enumerate(raw)]
    score = seg.evaluate_raw(raw, gts, calibration=True)
    want = sum(calibration_reference(g.labels.cpu(), g.conf.cpu(), t, n)[0] for g, t in zip(got, gts))
    assert torch.equal(score.calibration.cpu(), want)
    pics = seg.render_raw(raw, fade_by_conf=True)
    for pic, g, r in zip(pics, got, raw):
        assert torch.equal(pic.labels, g.labels) and torch.equal(pic.conf, g.conf)
        assert torch.equal(pic.picture, hip.seg_render(g.labels, r.to("cuda:0"), seg._palette_dev, 0.5, 0, (255, 255, 255), conf=g.conf))
    out = seg.pseudo_label_raw(raw, keep=0.5)
    assert all(torch.equal(o.predicted, g.labels) and torch.equal(o.conf, g.conf) for o, g in zip(out, got))
    # the batch call: the CRF's image rule, rounded to bytes
    tiled = raw[2].repeat(2, 2, 1).to("cuda:0")                         # 128 x 128, the network's own size
    res = seg(tiled[None], return_conf=True, return_probs=True)
    base = mk()(tiled[None], return_probs=True)
    labels, conf, probs = hip.seg_pamr(base.probs[0].contiguous(), tiled, 1, (1, 3), conf=True, probs_out=True)
    assert torch.equal(res.labels[0], labels) and torch.equal(res.conf[0], conf) and torch.equal(res.probs[0], probs)
