"""GPU: the scoring counters of csrc/predict.hip -- hip.seg_areas, hip.seg_score, hip.seg_score_views -- against the CPU
specification `areas_reference`, the ops through the dispatcher, and Segmenter.evaluate_raw end to end on the segofa_tiny
fixture.  The counters are integers: every comparison of counters is exact.

A scoring launch is compared with ITSELF first (its counters are `areas_reference` of the labels the same launch wrote, whatever
a near-tie decided), then its labels with the predict kernels' (bit for bit), then its counters with the fp64 specification: a
pixel whose label the case's `Reference` leaves undecided may sit in other bins than the reference's label, which moves at
most two units of L1 distance per histogram (one bin down, one up), so the distance is at most 2 u for u undecided scored
pixels; the ground-truth histogram and the tallies do not depend on the prediction and are exact."""
import ctypes

import pytest
import torch

import _predict_cases as PC
import _predict_views_cases as VC
import _score_cases as SC
from test_predict_views_gpu import e2e  # noqa: F401  (the segofa_tiny fixture with its three raw shapes)

pytestmark = pytest.mark.gpu

PATHS = {"staged": None, "direct": 0}
BAD_SHAPE, BAD_ARG = -2, -3


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ifseg_amd.ops  # noqa: F401
    return torch.device("cuda:0")


def _ref(labels, gt, n, raw=True):
    from ifseg_amd.predict import areas_reference
    return areas_reference(labels.cpu(), gt.cpu(), n, raw)


def _same(areas, tally, ref):
    return torch.equal(areas.cpu(), ref[0]) and torch.equal(tally.cpu(), ref[1])


# ------------------------------------------------------------------------------------------------- seg_areas
NPIX = (1, 3, 63, 1024, 37 * 91 * 3)
AREA_NS = ((1, torch.uint8), (15, torch.uint8), (150, torch.uint8), (257, torch.int16), (512, torch.int16))


@pytest.mark.parametrize("raw", [True, False], ids=["raw", "ids"])
@pytest.mark.parametrize("gt_dtype", [torch.uint8, torch.int16], ids=["gt8", "gt16"])
@pytest.mark.parametrize("n,ldt", AREA_NS)
def test_seg_areas_is_the_specification(n, ldt, gt_dtype, raw):
    from ifseg_amd import hip
    dev = _dev()
    for npix in NPIX:
        g = torch.Generator().manual_seed(npix + n)
        labels = torch.randint(0, n, (npix,), generator=g).to(ldt)
        gt = SC.ground_truth((npix,), n, raw, npix, gt_dtype)
        if npix >= 63:                                       # every kind of value, where there is room
            special = torch.tensor(SC.every_kind(n, raw, gt_dtype)).to(gt_dtype)
            gt[:special.numel()] = special
        areas, tally = hip.seg_areas(labels.to(dev), gt.to(dev), n, raw)
        assert areas.dtype == torch.int64 and areas.shape == (3, n) and tally.shape == (2,)
        assert _same(areas, tally, _ref(labels, gt, n, raw)), (npix, n)


@pytest.mark.parametrize("ldt,gt_dtype", [(torch.uint8, torch.uint8), (torch.uint8, torch.int16), (torch.int16, torch.uint8),
                                          (torch.int16, torch.int16)], ids=["l8g8", "l8g16", "l16g8", "l16g16"])
def test_seg_areas_at_every_alignment_with_canaries(ldt, gt_dtype):
    """label and ground-truth pointers at every element offset inside 16 bytes, independently; the counters sit between
    canaries and are accumulated into: the second call doubles them"""
    from ifseg_amd import hip
    dev = _dev()
    n, npix = 150, 1000
    g = torch.Generator().manual_seed(9)
    lbuf = torch.randint(0, n, (npix + 16,), generator=g).to(ldt).to(dev)
    gbuf = SC.ground_truth((npix + 16,), n, True, 3, gt_dtype).to(dev)
    assert lbuf.data_ptr() % 16 == 0 and gbuf.data_ptr() % 16 == 0
    cbuf = torch.full((8 + 3 * n + 8 + 2 + 8,), -12345, dtype=torch.int64, device=dev)
    areas, tally = cbuf[8:8 + 3 * n].view(3, n), cbuf[16 + 3 * n:18 + 3 * n]
    refs = {}
    for lo in range(0, 16 // lbuf.element_size()):
        for go in range(0, 16 // gbuf.element_size()):
            # another length per offset pair, so that the tail takes every length too
            m = npix - 16 + (lo * 5 + go) % 17
            lab, gt = lbuf[lo:lo + m], gbuf[go:go + m]
            areas.zero_(), tally.zero_()
            hip.seg_areas(lab, gt, n, True, areas=areas, tally=tally)
            refs[lo, go] = (areas.clone(), tally.clone(), lab.cpu(), gt.cpu())
    hip.seg_areas(lab, gt, n, True, areas=areas, tally=tally)
    assert torch.equal(areas, 2 * refs[lo, go][0]) and torch.equal(tally, 2 * refs[lo, go][1])
    assert cbuf[:8].eq(-12345).all() and cbuf[8 + 3 * n:16 + 3 * n].eq(-12345).all() and cbuf[18 + 3 * n:].eq(-12345).all()
    for key, (a, t, lab, gt) in refs.items():
        assert _same(a, t, _ref(lab, gt, n)), key


def test_seg_areas_one_class_everywhere_and_nothing_scored():
    from ifseg_amd import hip
    dev = _dev()
    n, shape = 15, (3, 37, 91)
    labels = torch.full(shape, 4, dtype=torch.uint8, device=dev)
    areas, tally = hip.seg_areas(labels, torch.full(shape, 5, dtype=torch.uint8, device=dev), n)      # raw 5 is class 4
    want = torch.zeros(3, n, dtype=torch.int64)
    want[:, 4] = labels.numel()
    assert torch.equal(areas.cpu(), want) and tally.tolist() == [labels.numel(), 0]
    for value, raw in ((0, True), (255, True), (n, False), (255, False)):
        areas, tally = hip.seg_areas(labels, torch.full(shape, value, dtype=torch.uint8, device=dev), n, raw)
        assert not areas.any() and tally.tolist() == [0, 0], (value, raw)
    # everything out of range: nothing scored, everything tallied
    areas, tally = hip.seg_areas(labels, torch.full(shape, n + 1, dtype=torch.int16, device=dev), n)
    assert not areas.any() and tally.tolist() == [0, labels.numel()]
    # a predicted label outside [0, n): the pixel is scored, and in the ground truth's histogram only
    bad = torch.tensor([3, 200, -5, 3], dtype=torch.int16, device=dev)
    areas, tally = hip.seg_areas(bad, torch.tensor([4, 4, 4, 9], dtype=torch.uint8, device=dev), n)
    assert _same(areas, tally, _ref(bad, torch.tensor([4, 4, 4, 9], dtype=torch.uint8), n)) and tally.tolist() == [4, 0]
    assert areas[:, 3].tolist() == [2 - 1, 2, 3] and int(areas[1].sum()) == 2


# ------------------------------------------------------------------------------------------------- seg_score
def _check_score_call(call, gt, n, raw, what):
    """the launch against itself: its counters are the specification's of the labels it wrote; without labels (and with every
    output) the same counters; -> (areas, tally, labels)"""
    areas, tally, labels, conf, probs = call(labels=True)
    assert conf is None and probs is None and labels.shape == gt.shape
    assert _same(areas, tally, _ref(labels, gt, n, raw)), what
    a2, t2, l2, c2, p2 = call(labels=False)
    assert l2 is None and c2 is None and p2 is None and torch.equal(a2, areas) and torch.equal(t2, tally), what
    a3, t3, l3, c3, p3 = call(labels=True, conf=True, probs=True)
    assert torch.equal(a3, areas) and torch.equal(t3, tally) and torch.equal(l3, labels) and c3 is not None and p3 is not None
    return areas, tally, labels


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("shape", PC.EXACT_SHAPES)
def test_seg_score_exact_family_labels_unchanged(shape, path):
    from ifseg_amd import hip
    dev = _dev()
    B, hp, wp, n = shape
    h, w = 16 * hp, 16 * wp
    s = PC.exact_scores(shape).to(dev)
    for raw, gdt in ((True, torch.uint8), (False, torch.int16)):
        gt = SC.ground_truth((B, h, w), n, raw, n, gdt).to(dev)
        call = lambda **kw: hip.seg_score(s, hp, wp, gt, raw, staging_bytes=PATHS[path], **kw)
        areas, tally, labels = _check_score_call(call, gt, n, raw, (shape, path, raw))
        pl, pc, pp = hip.seg_predict(s, hp, wp, h, w, conf=True, probs=True, staging_bytes=PATHS[path])
        _, _, l3, c3, p3 = call(labels=True, conf=True, probs=True)
        assert labels.dtype == pl.dtype and torch.equal(labels, pl) and torch.equal(l3, pl)
        assert torch.equal(c3.view(torch.int32), pc.view(torch.int32)) and torch.equal(p3.view(torch.int32), pp.view(torch.int32))


@pytest.mark.parametrize("softmaxed", [False, True], ids=["raw", "softmax"])
@pytest.mark.parametrize("shape", PC.GENERAL_SHAPES[:6])
def test_seg_score_general_family_and_fp64_specification(shape, softmaxed):
    from ifseg_amd import hip
    dev = _dev()
    hp, wp, n, h, w = shape
    seed = PC.SEEDS[0]
    s = PC.general_scores(shape, seed, softmaxed)
    ref = PC.Reference(s, hp, wp, h, w)
    assert ref.undecided_share <= PC.MARGIN_CAP
    gt = SC.ground_truth((1, h, w), n, True, seed)
    sd, gd = s.to(dev), gt.to(dev)
    for path, sb in PATHS.items():
        call = lambda **kw: hip.seg_score(sd, hp, wp, gd, True, staging_bytes=sb, **kw)
        areas, tally, labels = _check_score_call(call, gd, n, True, (shape, path))
        assert torch.equal(labels, hip.seg_predict(sd, hp, wp, h, w, staging_bytes=sb)[0])
        _against_fp64(areas, tally, ref, gt, n, (shape, path))


def _against_fp64(areas, tally, ref, gt, n, what):
    want, wt = _ref(ref.labels, gt, n)
    scored = torch.tensor([SC.kind(int(v), n, True) >= 0 for v in gt.reshape(-1)]).reshape(gt.shape)
    u = int((scored & ~ref.decided).sum())
    dist = (areas.cpu() - want).abs().sum(1).tolist()
    print(what, "undecided scored pixels u = %d, L1 distances %s (bound %d)" % (u, dist, 2 * u))
    assert all(d <= 2 * u for d in dist), (what, dist, u)
    assert torch.equal(areas[2].cpu(), want[2]) and torch.equal(tally.cpu(), wt), what


# ------------------------------------------------------------------------------------------------- seg_score_views
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("K", VC.EXACT_KS)
@pytest.mark.parametrize("shape", VC.EXACT_SHAPES)
def test_seg_score_views_exact_family_labels_unchanged(shape, K, path):
    from ifseg_amd import hip
    dev = _dev()
    B, gh, gw, n = shape
    h, w = 16 * gh, 16 * gw
    vd = VC.to_device(VC.exact_views(shape, K), dev)
    raw = K != 2
    gt = SC.ground_truth((B, h, w), n, raw, n + K, torch.int16 if K == 4 else torch.uint8).to(dev)
    call = lambda **kw: hip.seg_score_views(vd, gt, raw, staging_bytes=PATHS[path], **kw)
    areas, tally, labels = _check_score_call(call, gt, n, raw, (shape, K, path))
    pl, pc, pp = hip.seg_predict_views(vd, h, w, conf=True, probs=True, staging_bytes=PATHS[path])
    _, _, l3, c3, p3 = call(labels=True, conf=True, probs=True)
    assert labels.dtype == pl.dtype and torch.equal(labels, pl) and torch.equal(l3, pl)
    assert torch.equal(c3.view(torch.int32), pc.view(torch.int32)) and torch.equal(p3.view(torch.int32), pp.view(torch.int32))


def _views_case(vd, views, key, gt, n, h, w, what):
    from ifseg_amd import hip
    ref = VC.reference(key, views, h, w)
    assert ref.undecided_share <= PC.MARGIN_CAP
    gd = gt.to(vd[0][0].device)
    for path, sb in PATHS.items():
        call = lambda **kw: hip.seg_score_views(vd, gd, True, staging_bytes=sb, **kw)
        areas, tally, labels = _check_score_call(call, gd, n, True, (what, path))
        assert torch.equal(labels, hip.seg_predict_views(vd, h, w, staging_bytes=sb)[0])
        _against_fp64(areas, tally, ref, gt, n, (what, path))


@pytest.mark.parametrize("softmaxed", [False, True], ids=["raw", "softmax"])
@pytest.mark.parametrize("case", VC.GENERAL_CASES)
def test_seg_score_views_general_family_and_fp64_specification(case, softmaxed):
    dev = _dev()
    K, n, h, w = case
    seed = VC.SEEDS[0]
    views = VC.general_views(K, n, seed, softmaxed)
    gt = SC.ground_truth((1, h, w), n, True, seed + K)
    _views_case(VC.to_device(views, dev), views, ("general", K, n, h, w, softmaxed, seed), gt, n, h, w, case)


def test_seg_score_views_batch_and_footprints_beyond_the_staging_buffer():
    dev = _dev()
    B, K, n, h, w = VC.BATCH_CASE
    views = VC.general_views(K, n, 11, True, batch=B)
    _views_case(VC.to_device(views, dev), views, ("batch",), SC.ground_truth((B, h, w), n, True, 11), n, h, w, "batch 3")
    K, n, h, w, grids = VC.DIRECT_CASE
    views = VC.general_views(K, n, 1, False, batch=2, grids=grids)
    _views_case(VC.to_device(views, dev), views, ("direct",), SC.ground_truth((2, h, w), n, True, 12, torch.int16), n, h, w, "direct")


def test_score_accumulates_between_canaries():
    """counters handed in are added to, and nothing lands beside them"""
    from ifseg_amd import hip
    dev = _dev()
    hp, wp, n, h, w = PC.GENERAL_SHAPES[1]
    s = PC.general_scores(PC.GENERAL_SHAPES[1], 2, True, batch=2).to(dev)
    gt = SC.ground_truth((2, h, w), n, True, 5).to(dev)
    cbuf = torch.full((8 + 3 * n + 8 + 2 + 8,), -777, dtype=torch.int64, device=dev)
    areas, tally = cbuf[8:8 + 3 * n].view(3, n), cbuf[16 + 3 * n:18 + 3 * n]
    areas.zero_(), tally.zero_()
    a1, t1 = hip.seg_score(s, hp, wp, gt)[:2]
    hip.seg_score(s, hp, wp, gt, areas=areas, tally=tally)
    assert torch.equal(areas, a1) and torch.equal(tally, t1)
    r = hip.seg_score_views([(s, hp, wp, False)], gt, areas=areas, tally=tally)
    assert r[0] is areas and r[1] is tally and torch.equal(areas, 2 * a1) and torch.equal(tally, 2 * t1)
    hip.seg_areas(hip.seg_predict(s, hp, wp, h, w)[0], gt, n, areas=areas, tally=tally)
    assert torch.equal(areas, 3 * a1) and torch.equal(tally, 3 * t1)
    assert cbuf[:8].eq(-777).all() and cbuf[8 + 3 * n:16 + 3 * n].eq(-777).all() and cbuf[18 + 3 * n:].eq(-777).all()


# ------------------------------------------------------------------------------------------------- the C entry points
def test_entry_point_refusals():
    """each new refusal returns its code and launches nothing: poisoned counters and labels stay poisoned"""
    from ifseg_amd import hip
    dev = _dev()
    lib = hip.lib()
    i, ll, vp = ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p
    p = lambda t, off=0: vp(t.data_ptr() + off) if t is not None else vp(None)
    s = torch.zeros(1, 4, 512, device=dev)
    out = torch.full((64,), 77, dtype=torch.int16, device=dev)
    cnt = torch.full((3 * 512 + 2 + 1,), -5, dtype=torch.int64, device=dev)
    gt = torch.zeros(64, dtype=torch.int16, device=dev)
    areas, tally = cnt[:3 * 512], cnt[3 * 512:3 * 512 + 2]
    table = (hip._PredictView * 17)(*[hip._PredictView(s.data_ptr(), 2, 2, 0)] * 17)

    def score(n=5, gtp=p(gt), gb=2, ar=p(areas), ta=p(tally), labels=p(out), lb=2, h=4, w=4, B=1, sc=p(s)):
        return lib.ifseg_seg_score(sc, i(B), i(2), i(2), i(n), i(h), i(w), labels, i(lb), None, None, gtp, i(gb), i(1), ar, ta, None)

    def views(K=1, n=5, gtp=p(gt), gb=2, ar=p(areas), ta=p(tally), labels=p(out), lb=2, h=4, w=4, B=1, tb=table):
        return lib.ifseg_seg_score_views(tb, i(K), i(B), i(n), i(h), i(w), labels, i(lb), None, None, gtp, i(gb), i(1), ar, ta, None)

    def only(n=5, lab=p(out), lb=2, gtp=p(gt), gb=2, npix=16, ar=p(areas), ta=p(tally)):
        return lib.ifseg_seg_areas(lab, i(lb), gtp, i(gb), ll(npix), i(n), i(1), ar, ta, None)

    for call in (score, views, only):
        assert call(gb=0) == BAD_ARG and call(gb=3) == BAD_ARG and call(gb=4) == BAD_ARG
        assert call(gtp=vp(None)) == BAD_ARG and call(ar=vp(None)) == BAD_ARG and call(ta=vp(None)) == BAD_ARG
        assert call(ar=p(areas, 4)) == BAD_ARG and call(ta=p(tally, 4)) == BAD_ARG
        assert call(gtp=p(gt, 1)) == BAD_ARG                                          # int16 ground truth at an odd address
        assert call(n=0) == BAD_ARG and call(n=513) == BAD_ARG
    # the predict entry points' own refusals carry over
    for call in (score, views):
        assert call(lb=4) == BAD_ARG and call(n=300, lb=1) == BAD_ARG and call(labels=p(out, 2)) == BAD_ARG
        assert call(h=0) == BAD_SHAPE and call(w=-1) == BAD_SHAPE and call(B=0) == BAD_SHAPE
        assert call(h=2 ** 16, w=2 ** 15) == BAD_SHAPE
    assert score(sc=vp(None)) == BAD_ARG
    assert views(K=0) == BAD_ARG and views(K=17) == BAD_ARG and views(tb=ctypes.POINTER(hip._PredictView)()) == BAD_ARG
    assert only(lab=vp(None)) == BAD_ARG and only(lb=3) == BAD_ARG and only(lab=p(out, 1)) == BAD_ARG
    assert only(npix=0) == BAD_SHAPE and only(npix=2 ** 31) == BAD_SHAPE
    torch.cuda.synchronize()
    assert out.eq(77).all() and cnt.eq(-5).all()                                     # no launch so far
    # the limits themselves pass: K = 16, n = 512, int16 ground truth, no outputs at all
    areas.zero_(), tally.zero_()
    assert views(K=16, n=512, labels=vp(None), lb=0) == 0 and score(n=512, labels=vp(None), lb=0) == 0
    assert only(n=512, lab=p(gt)) == 0
    torch.cuda.synchronize()
    # ground truth 0 everywhere is ignored under raw labels: nothing scored, nothing written
    assert out.eq(77).all() and not areas.any() and not tally.any() and cnt[-1] == -5


# ------------------------------------------------------------------------------------------------- the ops
def test_ops_match_bindings_and_opcheck():
    from ifseg_amd import hip
    dev = _dev()
    n, h, w = 257, 40, 23
    views = VC.to_device(VC.general_views(3, n, 3, False, batch=2, grids=[(2, 3), (4, 6), (3, 2)]), dev)
    gt = SC.ground_truth((2, h, w), n, True, 1, torch.int16).to(dev)
    args = ([v[0] for v in views], [v[1] for v in views], [v[2] for v in views], [v[3] for v in views], gt, True)
    ra, rt, rl, rc, rp = hip.seg_score_views(views, gt, True, labels=True, conf=True, probs=True)
    a, t, l, c, p = torch.ops.ifseg.seg_score_views(*args, True, True, True)
    assert l.dtype == torch.int16 and all(torch.equal(x, y) for x, y in zip((a, t, l, c, p), (ra, rt, rl, rc, rp)))
    a, t, l, c, p = torch.ops.ifseg.seg_score_views(*args, False, False, False)
    assert torch.equal(a, ra) and torch.equal(t, rt) and l.numel() == 0 and l.dtype == torch.int16 and c.numel() == 0 and p.numel() == 0
    # a single view is K = 1, and equals seg_score
    one = torch.ops.ifseg.seg_score_views(args[0][:1], [2], [3], [False], gt, True, True, False, False)
    two = hip.seg_score(views[0][0], 2, 3, gt, labels=True)
    assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1]) and torch.equal(one[2], two[2])
    # seg_areas: fresh counters, equal to the binding's; non-contiguous inputs are copied
    a, t = torch.ops.ifseg.seg_areas(rl, gt, n, True)
    assert torch.equal(a, ra) and torch.equal(t, rt)
    a2, t2 = torch.ops.ifseg.seg_areas(rl.transpose(1, 2), gt.transpose(1, 2), n, True)
    assert torch.equal(a2, ra) and torch.equal(t2, rt) and a2.data_ptr() != a.data_ptr()
    utils = ("test_schema", "test_autograd_registration", "test_faketensor")
    torch.library.opcheck(torch.ops.ifseg.seg_areas, (rl, gt, n, True), test_utils=utils)
    torch.library.opcheck(torch.ops.ifseg.seg_areas, (rl[0, :5].contiguous().to(torch.uint8), gt[0, :5].contiguous(), n, False),
                          test_utils=utils)
    torch.library.opcheck(torch.ops.ifseg.seg_score_views, (*args, True, True, True), test_utils=utils)
    small = ([s[:1, :, :5].contiguous() for s in args[0]], *args[1:4], gt[:1, :7, :9].contiguous().to(torch.uint8), False)
    torch.library.opcheck(torch.ops.ifseg.seg_score_views, (*small, False, False, False), test_utils=utils)
    # on a side stream the ops follow PyTorch's current stream
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        a3 = torch.ops.ifseg.seg_score_views(*args, False, False, False)[0]
        a4 = torch.ops.ifseg.seg_areas(rl, gt, n, True)[0]
    st.synchronize()
    assert torch.equal(a3, ra) and torch.equal(a4, ra)


# ------------------------------------------------------------------------------------------------- end to end
def _gts(raw, n, dtype=torch.uint8):
    return [SC.ground_truth(tuple(r.shape[:2]), n, True, k, dtype) for k, r in enumerate(raw)]


def _sum_of(outs, gts, n):
    from ifseg_amd.predict import areas_reference
    areas, tally = torch.zeros(3, n, dtype=torch.int64), torch.zeros(2, dtype=torch.int64)
    for o, g in zip(outs, gts):
        a, t = areas_reference(o.labels.cpu(), g, n)
        areas, tally = areas + a, tally + t
    return areas, tally


@pytest.mark.parametrize("kw,call", [({}, {}), ({}, {"scales": (0.5, 1.0, 1.5), "flip": True}), ({"smooth_iters": 2}, {}),
                                     ({"crf_iters": 1}, {}), ({"crf_iters": 1}, {"scales": (0.5, 1.0), "flip": True})],
                         ids=["single", "ms_flip", "smoothing", "crf", "crf_ms_flip"])
def test_evaluate_raw_is_segment_raw_scored(e2e, kw, call):  # noqa: F811
    from ifseg_amd.predict import SegmentationScore
    m, raw, ocfg, mk = e2e
    n = ocfg.num_seg_tokens
    seg, gts = mk(**kw), _gts(raw, n)
    outs = seg.segment_raw(raw, **call)
    score = seg.evaluate_raw(raw, gts, **call)
    assert isinstance(score, SegmentationScore) and score.areas.is_cuda and score.areas.dtype == torch.int64
    assert _same(score.areas, score.tally, _sum_of(outs, gts, n))
    assert int(score.tally[0]) > 0 and int(score.tally[1]) == 0
    # return_labels: segment_raw's labels, the same score
    again, labels = seg.evaluate_raw(raw, [g.to("cuda:0") for g in gts], return_labels=True, **call)
    assert torch.equal(again.areas, score.areas) and torch.equal(again.tally, score.tally)
    assert len(labels) == 3 and all(torch.equal(l, o.labels) and l.dtype == o.labels.dtype for l, o in zip(labels, outs))


def test_evaluate_raw_into_order_summary_and_task(e2e):  # noqa: F811
    from ifseg_amd.criterions import SegCriterion
    from ifseg_amd.tasks.mm_tasks.segmentation import SegmentationTask
    m, raw, ocfg, mk = e2e
    n = ocfg.num_seg_tokens
    seg, gts = mk(), _gts(raw, n)
    first = seg.evaluate_raw(raw[:2], gts[:2])
    keep = first.areas.clone()
    total = seg.evaluate_raw(raw[2], gts[2], into=first)
    assert total is first and not torch.equal(first.areas, keep)
    whole = seg.evaluate_raw(raw, gts)
    assert torch.equal(total.areas, whole.areas) and torch.equal(total.tally, whole.tally)
    # a list with repeated shapes batches and keeps the order: int16 ground truth, two scales and flip
    order = [2, 0, 2, 0]
    imgs, g16 = [raw[k] for k in order], [_gts(raw, n, torch.int16)[k] for k in order]
    g16[2] = SC.ground_truth(tuple(raw[2].shape[:2]), n, True, 99, torch.int16)       # another map for the repeated image
    call = dict(max_batch=3, scales=(0.5, 1.0), flip=True)
    score, labels = seg.evaluate_raw(imgs, g16, return_labels=True, **call)
    outs = seg.segment_raw(imgs, **call)
    assert [tuple(l.shape) for l in labels] == [(64, 64), (60, 90), (64, 64), (60, 90)]
    assert all(torch.equal(l, o.labels) for l, o in zip(labels, outs))
    assert _same(score.areas, score.tally, _sum_of(outs, g16, n))
    # summary: reduce_metrics' numbers
    got, want = whole.summary(), SegCriterion.reduce_metrics([whole.logging_output()])
    assert (got["aAcc"], got["mIoU"], got["mAcc"]) == (want["aAcc"], want["mIoU"], want["mAcc"])
    assert got["pixels"] == int(whole.tally[0]) and len(got["IoU"]) == n
    # class ids instead of raw values, through the batch call: the same score as the raw maps of the same classes
    tiled, gtile = raw[2].repeat(2, 2, 1), gts[2].repeat(2, 2)                        # 128 x 128, the network's own size
    img, graw = torch.stack([tiled, tiled.flip(0)]).to("cuda:0"), torch.stack([gtile, gtile.flip(1)])
    ids = torch.where((graw == 0) | (graw == 255), torch.full_like(graw, n), graw - 1)
    a, la = seg.evaluate(img, graw.to("cuda:0"), return_labels=True)
    b = seg.evaluate(img, ids, raw_labels=False)
    assert torch.equal(a.areas, b.areas) and torch.equal(a.tally, b.tally) and torch.equal(la, seg(img).labels)
    assert _same(a.areas, a.tally, _ref(la, graw, n))
    # label maps of another size than the images: the label map is taken at the ground truth's size, as out_hw does
    small = SC.ground_truth((2, 60, 90), n, True, 21)
    c, lc = seg.evaluate(img, small, return_labels=True)
    assert torch.equal(lc, seg(img, out_hw=(60, 90)).labels) and _same(c.areas, c.tally, _ref(lc, small, n))
    # ground truth out of range is refused by summary, not ignored
    wrong = seg.evaluate_raw(raw[0], torch.full(tuple(raw[0].shape[:2]), n + 1, dtype=torch.uint8))
    with pytest.raises(IndexError, match=r"tally\[1\] = %d" % (60 * 90)):
        wrong.summary()
    # the task's convenience
    task = SegmentationTask(num_seg_tokens=n, patch_image_size=ocfg.patch_image_size, category_token_ids=PC.E2E_NAMES)
    ts = task.evaluate_raw(m, raw, gts, prompt_ids=PC.E2E_PROMPT)
    assert torch.equal(ts.areas, whole.areas) and torch.equal(ts.tally, whole.tally)
