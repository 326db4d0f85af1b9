"""GPU: hip.seg_distance / hip.seg_trimap_areas (csrc/distance.hip) against their specifications (`distance_reference`,
`trimap_areas_reference`) -- every shape, pattern, max_distance, border setting and dtype of tests/_distance_cases.py, in views
at element offsets 0, 1 and 3 between canaries, called twice into the same output; the disc cut by the clamp, a map with pixels
farther than R, a batch whose images must not see each other; the trimap counters on tests/_boundary_cases.py's block maps in
every dtype pair; the raw C entries' refusals; and `Segmenter.evaluate_raw(trimap=)` / `evaluate` end to end on the
segofa_tiny fixture.  Everything is an integer: every comparison is `torch.equal`, and no pixel is left out."""
import ctypes

import pytest
import torch

import _boundary_cases as BC
import _distance_cases as T
from test_boundary_gpu import _gts
from test_confusion_gpu import SETTINGS
from test_predict_views_gpu import e2e  # noqa: F401  (the segofa_tiny fixture with its three raw shapes)
from test_regions_gpu import _untouched, _view

pytestmark = pytest.mark.gpu

OFFSETS = (0, 1, 3)
BAD_SHAPE, BAD_ARG = -2, -3
U16 = torch.uint16


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ifseg_amd.ops  # noqa: F401
    return torch.device("cuda:0")


def _distance_case(hip, key, short, R, border, off, dev):
    """labels in a view at element offset `off`, the output in another between canaries; a second call gives equal bits"""
    lab = T.labels_as(key, short)
    what = (key, short, R, border, off)
    want = T.reference(key, R, border)
    d, buf_l = _view(lab.shape, lab.dtype, off, 99, dev, lab)
    fresh = hip.seg_distance(d, R, border)
    assert fresh.dtype == U16 and fresh.shape == lab.shape and fresh.is_contiguous(), what
    assert torch.equal(fresh.cpu(), want), what
    o16, buf_o = _view(lab.shape, torch.int16, OFFSETS[(OFFSETS.index(off) + 1) % 3], 77, dev)    # the canaries as int16
    out = o16.view(U16)
    got = hip.seg_distance(d, R, border, out=out)
    assert got is out and torch.equal(out.cpu(), want), what
    assert _untouched(buf_o, o16.storage_offset(), lab.numel(), 77), what
    assert torch.equal(d.cpu(), lab) and _untouched(buf_l, off, lab.numel(), 99), what            # the input is only read
    first = buf_o.clone()
    hip.seg_distance(d, R, border, out=out)
    assert torch.equal(first, buf_o), what                                                       # equal bits
    return want


@pytest.mark.parametrize("pattern", T.PATTERNS)
def test_seg_distance_equals_the_specification(pattern):
    from ifseg_amd import hip
    dev = _dev()
    far = near = 0
    for i, key in enumerate(T.case_keys((pattern,))):
        for j, R in enumerate(T.RADII):
            for border in (False, True):
                for short in (False, True):
                    want = _distance_case(hip, key, short, R, border, OFFSETS[(i + j + short) % 3], dev)
                    far += int((want == T.FAR).sum())
                    near += int((want != T.FAR).sum())
                if pattern == "constant" and not border:
                    assert bool((want == T.FAR).all())
    assert far > 0 and near > 0                                       # both sides of the clamp, in every pattern


def test_the_disc_cut_by_the_clamp():
    """one pixel of another value in a constant 300 x 400 map at R = 128: a disc across many tile seams, R and R + 1 at the rim"""
    from ifseg_amd import hip
    dev = _dev()
    for short in (False, True):
        got = hip.seg_distance(T.labels_as("disc", short).to(dev), 128).cpu()
        assert torch.equal(got, T.reference("disc", 128, False))
        d = got.long()
        assert int(d[150, 72]) == 128 * 128 and int(d[150, 71]) == T.FAR and int(d[22, 200]) == 128 * 128 and int(d[21, 200]) == T.FAR
        assert int(d[150 - 77, 200 + 102]) == 77 * 77 + 102 * 102 and int(d[150 - 78, 200 + 102]) == T.FAR
    for R in (1, 17, 127):
        assert torch.equal(hip.seg_distance(T.labels_of("disc").to(dev), R, True).cpu(), T.reference("disc", R, True)), R


def test_pixels_farther_than_the_largest_distance():
    from ifseg_amd import hip
    dev = _dev()
    want = T.reference("table7", 64, False)
    assert bool((want == T.FAR).any()) and bool((want != T.FAR).any())
    for short in (False, True):
        _distance_case(hip, "table7", short, 64, False, 1, dev)
    _distance_case(hip, "table7", False, 64, True, 3, dev)


def test_distances_do_not_cross_from_one_image_into_the_next():
    from ifseg_amd import hip
    dev = _dev()
    batch = T.labels_of("batch")
    assert int(batch[0, -1, 0]) == int(batch[1, 0, 0]) == int(batch[1, -1, 0]) == int(batch[2, 0, 0])
    for R in (4, 17, 128):
        for border in (False, True):
            for short in (False, True):
                want = _distance_case(hip, "batch", short, R, border, OFFSETS[R % 3], dev)
                assert border or bool((want[1] == T.FAR).all())       # the constant image sees neither neighbour
                for b in range(3):                                    # and each image alone gives its own plane
                    one = hip.seg_distance(T.labels_as("batch", short)[b].contiguous().to(dev), R, border)
                    assert torch.equal(one.cpu(), want[b]), (R, border, short, b)


def test_distance_entry_point_refusals_and_limits():
    """each refusal returns its code and launches nothing: the poisoned buffers stay poisoned; the limits themselves pass"""
    from ifseg_amd import hip
    dev = _dev()
    lib = hip.lib()
    i, vp = ctypes.c_int, ctypes.c_void_p
    p = lambda t, off=0: vp(t.data_ptr() + off) if t is not None else vp(None)
    h, w = 6, 40
    lab = torch.zeros(h * w + 8, dtype=torch.int16, device=dev)
    work = torch.full((h * w + 8,), 99, dtype=torch.uint8, device=dev)
    out = torch.full((h * w + 8,), 7, dtype=torch.int16, device=dev)

    def call(R=2, labp=p(lab), lb=2, B=1, h=h, w=w, border=0, wp=p(work), op=p(out)):
        return lib.ifseg_seg_distance(labp, i(lb), i(B), i(h), i(w), i(R), i(border), wp, op, None)

    assert call(R=0) == BAD_ARG and call(R=129) == BAD_ARG and call(R=-2) == BAD_ARG
    assert call(B=0) == BAD_SHAPE and call(h=0) == BAD_SHAPE and call(w=-1) == BAD_SHAPE
    assert call(B=2, h=32768, w=32768) == BAD_SHAPE and call(B=1, h=65536, w=32768) == BAD_SHAPE
    assert call(B=2 ** 30, h=2, w=1) == BAD_SHAPE and call(B=65536, h=65536, w=65536) == BAD_SHAPE
    assert call(labp=vp(None)) == BAD_ARG and call(wp=vp(None)) == BAD_ARG and call(op=vp(None)) == BAD_ARG
    assert call(labp=p(lab, 1)) == BAD_ARG and call(op=p(out, 1)) == BAD_ARG          # 2-byte elements at an odd address
    for bad in (0, 3, 4, -1):
        assert call(lb=bad) == BAD_ARG
    assert call(wp=p(lab)) == BAD_ARG and call(op=p(lab)) == BAD_ARG and call(wp=p(out)) == BAD_ARG      # shared bytes
    assert call(op=p(lab, 2 * h * w - 2)) == BAD_ARG and call(wp=p(out, 2 * h * w - 1)) == BAD_ARG
    torch.cuda.synchronize()
    assert work.eq(99).all() and out.eq(7).all()                                       # no launch so far
    assert hip.seg_distance_limits() == (128, 65535, 8, 512)
    # the limits themselves pass: R = 128 on a constant map (no border: all far), maps and planes at odd element offsets
    assert call(R=128) == 0
    torch.cuda.synchronize()
    assert out[:h * w].eq(-1).all() and out[h * w:].eq(7).all() and work[:h * w].eq(255).all() and work[h * w:].eq(99).all()
    assert call(R=128, border=1, labp=p(lab, 2), wp=p(work, 3), op=p(out, 6)) == 0
    torch.cuda.synchronize()
    y, x = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    edge = torch.minimum(torch.minimum(x + 1, w - x), torch.minimum(y + 1, h - y))
    assert torch.equal(out[3:3 + h * w].view(h, w).cpu().long(), edge * edge) and out[3 + h * w:].eq(7).all()
    assert work[3 + h * w:].eq(99).all()


# ------------------------------------------------------------------------------------------------- the trimap counters
@pytest.mark.parametrize("raw", [True, False], ids=["raw", "ids"])
@pytest.mark.parametrize("gdt", list(BC.DTYPES), ids=["gt8", "gt16"])
@pytest.mark.parametrize("ldt", list(BC.DTYPES), ids=["l8", "l16"])
@pytest.mark.parametrize("k", range(len(BC.TABLE)), ids=BC.IDS)
def test_seg_trimap_areas_is_the_specification(k, ldt, gdt, raw):
    from ifseg_amd import hip
    dev = _dev()
    radii = T.TRIMAP_RADII[k]
    for outside in (False, True):
        assert T.trimap_nonempty(k, ldt, raw, outside)                                # a condition on the inputs
        labels, gt, n = BC.maps(BC.TABLE[k], BC.DTYPES[ldt], BC.DTYPES[gdt], raw, outside)
        want = T.trimap_reference(k, ldt, raw, outside)[0]
        ld, gd = labels.to(dev), gt.to(dev)
        trimap, dist = hip.seg_trimap_areas(ld, gd, n, radii, raw)
        assert trimap.dtype == torch.int64 and trimap.is_contiguous() and torch.equal(trimap.cpu(), want), outside
        assert dist.dtype == U16 and torch.equal(dist.cpu(), T.gt_distance(k, raw)), outside
        # adding into a given table: a second call doubles it; a plane passed in is read, not computed again
        again, same = hip.seg_trimap_areas(ld, gd, n, radii, raw, trimap=trimap, dist=dist)
        assert again is trimap and same is dist and torch.equal(trimap.cpu(), 2 * want), outside
        # a plane of a larger max_distance puts the same pixels into the same rings; [1, h, w] is [h, w]
        wide = hip.seg_distance(gd, min(radii[-1] + 9, 128))
        one, _ = hip.seg_trimap_areas(ld[None], gd[None], n, list(radii), raw, dist=wide[None])
        assert torch.equal(one.cpu(), want), outside


def test_trimap_border_batches_and_canaries():
    """border=True against the specification; a batch is the sum of its images; the counters sit between canaries"""
    from ifseg_amd import hip
    from ifseg_amd.predict import trimap_areas_reference
    dev = _dev()
    k, radii = 2, (1, 2, 5, 9)
    pairs = [BC.maps(BC.TABLE[k], torch.int16, torch.uint8, True, o)[:2] for o in (False, True)]
    n = BC.classes(BC.TABLE[k])
    labels = torch.stack([pairs[0][0], pairs[1][0].flip(0)])
    gt = torch.stack([pairs[0][1], pairs[1][1].flip(1)])
    for border in (False, True):
        want = trimap_areas_reference(labels, gt, n, radii, border=border)
        each = sum(trimap_areas_reference(l, g, n, radii, border=border) for l, g in zip(labels, gt))
        assert torch.equal(want, each) and bool((want.sum(2) > 0).all())
        cbuf = torch.full((8 + want.numel() + 8,), -12345, dtype=torch.int64, device=dev)
        trimap = cbuf[8:8 + want.numel()].view(want.shape)
        trimap.zero_()
        got, dist = hip.seg_trimap_areas(labels.to(dev), gt.to(dev), n, radii, border=border, trimap=trimap)
        assert got is trimap and torch.equal(trimap.cpu(), want), border
        assert cbuf[:8].eq(-12345).all() and cbuf[8 + want.numel():].eq(-12345).all()
    assert not torch.equal(trimap_areas_reference(labels, gt, n, radii), want)        # the border moves pixels between rings


@pytest.mark.parametrize("n,K", [(1, 1), (150, 6), (512, 8)])
def test_trimap_class_counts_and_ring_counts_at_the_limits(n, K):
    from ifseg_amd import hip
    from ifseg_amd.predict import trimap_areas_reference
    from test_boundary_gpu import _random_blocks
    dev = _dev()
    radii = (1, 2, 3, 4, 6, 9, 14, 20)[:K]
    labels, gt = _random_blocks(70, 131, n, n, torch.int16, torch.int16, 40, 60)
    want = trimap_areas_reference(labels, gt, n, radii)
    assert int(want[:, 0].sum()) > 0 and bool((want.sum((1, 2)) > 0).all())
    got, _ = hip.seg_trimap_areas(labels.to(dev), gt.to(dev), n, radii)
    assert torch.equal(got.cpu(), want)


def test_trimap_entry_point_refusals():
    from ifseg_amd import hip
    dev = _dev()
    lib = hip.lib()
    i, vp = ctypes.c_int, ctypes.c_void_p
    p = lambda t, off=0: vp(t.data_ptr() + off) if t is not None else vp(None)
    h, w = 6, 40
    lab = torch.zeros(h * w + 8, dtype=torch.int16, device=dev)
    gt = torch.zeros(h * w + 8, dtype=torch.int16, device=dev)
    dist = torch.ones(h * w + 8, dtype=torch.int16, device=dev)
    cnt = torch.full((8 * 3 * 512 + 1,), -5, dtype=torch.int64, device=dev)

    def call(n=5, radii=(1, 2, 4), K=None, labp=p(lab), lb=2, gtp=p(gt), gb=2, dp=p(dist), B=1, h=h, w=w, cp=p(cnt)):
        table = (i * len(radii))(*radii)
        return lib.ifseg_seg_trimap_areas(labp, i(lb), gtp, i(gb), dp, i(B), i(h), i(w), i(n), table, i(len(radii) if K is None else K),
                                          i(1), cp, None)

    assert call(n=0) == BAD_ARG and call(n=513) == BAD_ARG and call(n=-1) == BAD_ARG
    assert call(K=0) == BAD_ARG and call(K=9) == BAD_ARG and call(K=-1) == BAD_ARG
    for bad in ((0, 1), (1, 1), (2, 1), (1, 129), (-3,)):
        assert call(radii=bad) == BAD_ARG, bad
    assert call(B=0) == BAD_SHAPE and call(h=0) == BAD_SHAPE and call(w=-1) == BAD_SHAPE and call(B=2, h=32768, w=32768) == BAD_SHAPE
    assert call(labp=vp(None)) == BAD_ARG and call(gtp=vp(None)) == BAD_ARG and call(dp=vp(None)) == BAD_ARG and call(cp=vp(None)) == BAD_ARG
    assert call(labp=p(lab, 1)) == BAD_ARG and call(gtp=p(gt, 1)) == BAD_ARG and call(dp=p(dist, 1)) == BAD_ARG
    assert call(cp=p(cnt, 4)) == BAD_ARG                                               # the counters not 8-byte aligned
    assert call(cp=p(lab)) == BAD_ARG and call(cp=p(gt)) == BAD_ARG and call(cp=p(dist)) == BAD_ARG
    for bad in (0, 3, 4, -1):
        assert call(lb=bad) == BAD_ARG and call(gb=bad) == BAD_ARG
    torch.cuda.synchronize()
    assert cnt.eq(-5).all()                                                            # no launch so far
    # the limits themselves pass: K = 8 with n = 512 (48 KiB of LDS), maps at odd element offsets.  Ground truth 0 everywhere
    # is ignored under raw labels, so no counter is written
    assert call(n=512, radii=(1, 2, 3, 4, 5, 6, 7, 128)) == 0 and call(n=1, radii=(128,), lb=1, gb=1) == 0
    assert call(labp=p(lab, 2), gtp=p(gt, 6), dp=p(dist, 10)) == 0
    torch.cuda.synchronize()
    assert cnt.eq(-5).all()


# ------------------------------------------------------------------------------------------------- end to end
RADII = (1, 2, 4)


def _want(labels, gts, n, radii=RADII):
    from ifseg_amd.predict import trimap_areas_reference
    return sum(trimap_areas_reference(l.cpu(), g, n, radii) for l, g in zip(labels, gts))


@pytest.mark.parametrize("setting", list(SETTINGS) + ["pamr", "sieve"])
def test_evaluate_raw_with_trimap(e2e, setting):  # noqa: F811
    from ifseg_amd.predict import SegmentationScore, boundary_areas_reference, boundary_distance, confusion_reference
    m, raw, ocfg, mk = e2e
    n = ocfg.num_seg_tokens
    kw, call = {"pamr": ({"pamr_iters": 1, "pamr_dilations": (1, 3)}, {}), "sieve": ({"sieve": 8}, {})}.get(setting) or SETTINGS[setting]
    seg = mk(**kw)
    gts = _gts(raw, n)
    score, labels = seg.evaluate_raw(raw, gts, trimap=RADII, return_labels=True, **call)
    t = score.trimap
    assert t.is_cuda and t.dtype == torch.int64 and t.shape == (3, 3, n) and score.trimap_radii == RADII
    assert score.confusion is None and score.boundary is None and score.calibration is None
    # the counters are the specification's of the labels the same call returned, summed over the images
    want = _want(labels, gts, n)
    assert torch.equal(t.cpu(), want) and bool((want[:, 2].sum(1) > 0).all()) and (t.sum(0) <= score.areas).all()
    s = score.summary()
    assert s["trimap_radii"] == [1, 2, 4] and len(s["trimap_mIoU"]) == 3 and s["trimap_pixels"] == want[:, 2].sum(1).cumsum(0).tolist()
    assert len(score.trimap_summary(per_class=True)["trimap_IoU"][0]) == n
    # areas, tally and the labels are what they are without it
    plain, plain_labels = seg.evaluate_raw(raw, gts, return_labels=True, **call)
    assert plain.trimap is None and torch.equal(plain.areas, score.areas) and torch.equal(plain.tally, score.tally)
    assert all(torch.equal(a, c) and a.dtype == c.dtype for a, c in zip(labels, plain_labels))
    assert repr({k: v for k, v in s.items() if not k.startswith("trimap")}) == repr(plain.summary())      # repr: NaN equals NaN
    # without return_labels the counters are the same; `into` accumulates across two calls without the keyword
    alone = seg.evaluate_raw(raw, gts, trimap=RADII, **call)
    assert isinstance(alone, SegmentationScore) and torch.equal(alone.trimap, t) and torch.equal(alone.areas, score.areas)
    twice = seg.evaluate_raw(raw, gts, into=alone, **call)
    assert twice is alone and torch.equal(alone.trimap, 2 * t) and torch.equal(alone.areas, 2 * score.areas)
    # the default radii; together with the matrix and the bands: each bit-equal to what it is alone
    default = seg.evaluate_raw(raw, gts, trimap=True, **call)
    assert default.trimap_radii == (1, 2, 4, 8, 16, 32) and torch.equal(default.trimap.cpu(), _want(labels, gts, n, default.trimap_radii))
    both = seg.evaluate_raw(raw, gts, trimap=RADII, confusion=True, boundary_iou=True, **call)
    assert torch.equal(both.trimap, t) and torch.equal(both.areas, score.areas) and torch.equal(both.tally, score.tally)
    others = seg.evaluate_raw(raw, gts, confusion=True, boundary_iou=True, **call)
    assert torch.equal(both.confusion, others.confusion) and torch.equal(both.boundary, others.boundary)
    assert torch.equal(both.confusion.cpu(), sum(confusion_reference(l.cpu(), g, n) for l, g in zip(labels, gts)))
    assert torch.equal(both.boundary.cpu(), sum(boundary_areas_reference(l.cpu(), g, n, boundary_distance(*g.shape))[0]
                                                for l, g in zip(labels, gts)))


def test_evaluate_and_task_pass_trimap_on(e2e):  # noqa: F811
    import _predict_cases as PC
    from ifseg_amd.predict import trimap_areas_reference
    from ifseg_amd.tasks.mm_tasks.segmentation import SegmentationTask
    m, raw, ocfg, mk = e2e
    n = ocfg.num_seg_tokens
    seg = mk()
    gts = _gts(raw, n)
    whole = seg.evaluate_raw(raw, gts, trimap=RADII)
    task = SegmentationTask(num_seg_tokens=n, patch_image_size=ocfg.patch_image_size, category_token_ids=PC.E2E_NAMES)
    ts = task.evaluate_raw(m, raw, gts, prompt_ids=PC.E2E_PROMPT, trimap=RADII)
    assert torch.equal(ts.trimap, whole.trimap) and torch.equal(ts.areas, whole.areas)
    assert repr(ts.summary()) == repr(whole.summary()) and "trimap_mIoU" in ts.summary()
    # the batch call: one counting launch for the batch, and no distance crosses from one image into the next
    tiled, gtile = raw[2].repeat(2, 2, 1), gts[2].repeat(2, 2)                        # 128 x 128, the network's own size
    img, g = torch.stack([tiled, tiled.flip(0)]).to("cuda:0"), torch.stack([gtile, gtile.flip(1)])
    a, la = seg.evaluate(img, g, return_labels=True, trimap=RADII)
    assert torch.equal(a.trimap.cpu(), trimap_areas_reference(la.cpu(), g, n, RADII)) and int(a.trimap[:, 2].sum()) > 0
    assert torch.equal(a.trimap.cpu(), sum(trimap_areas_reference(la[b].cpu(), g[b], n, RADII) for b in range(2)))
    c = seg.evaluate(img, g)
    assert c.trimap is None and torch.equal(a.areas, c.areas) and torch.equal(a.tally, c.tally)
    seg.evaluate(img, g, into=a)
    assert torch.equal(a.trimap.cpu(), 2 * trimap_areas_reference(la.cpu(), g, n, RADII)) and torch.equal(a.areas, 2 * c.areas)
