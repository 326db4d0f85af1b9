"""GPU: Boundary IoU's band areas of csrc/boundary.hip -- hip.seg_boundary_areas at every band width class (below and above the
small label halo's limit, 16 / 17, the maximum 64), ragged tiles, every dtype pair and element alignment -- against the CPU
specification `boundary_areas_reference`, the raw C entry's refusals, the op through the dispatcher, and
Segmenter.evaluate_raw(boundary_iou=True) end to end on the segofa_tiny fixture.  The counters and the bands are integers:
every comparison is exact, and no pixel is left out."""
import ctypes

import pytest
import torch

import _boundary_cases as BC
import _score_cases as SC
from test_confusion_gpu import SETTINGS
from test_predict_views_gpu import e2e  # noqa: F401  (the segofa_tiny fixture with its three raw shapes)

pytestmark = pytest.mark.gpu

BAD_SHAPE, BAD_ARG = -2, -3


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ifseg_amd.ops  # noqa: F401
    return torch.device("cuda:0")


def _ref(labels, gt, n, d, raw=True):
    from ifseg_amd.predict import boundary_areas_reference
    return boundary_areas_reference(labels.cpu(), gt.cpu(), n, d, raw)


def _same(got, want, what=None):
    bareas, band = got
    assert bareas.dtype == torch.int64 and bareas.is_contiguous() and band.dtype == torch.uint8 and band.shape == want[1].shape
    assert torch.equal(band.cpu(), want[1]), what
    assert torch.equal(bareas.cpu(), want[0]), what


def _random_blocks(h, w, n, seed, ldt, gdt, bh=9, bw=21):
    """blocks of random classes, a tenth of the ground truth's blocks ignored; the labels are other blocks, shifted, with
    some labels outside [0, n)"""
    g = torch.Generator().manual_seed(9000 + seed)
    up = lambda t: t.repeat_interleave(bh, 0).repeat_interleave(bw, 1)
    cells = (-(-h // bh) + 1, -(-w // bw) + 1)
    gt = torch.randint(1, n + 1, cells, generator=g)
    gt = torch.where(gt == 255, torch.ones_like(gt), gt)
    drop = torch.rand(cells, generator=g)
    gt = torch.where(drop < 0.05, torch.zeros_like(gt), torch.where(drop < 0.1, torch.full_like(gt, 255), gt))
    labels = torch.where(torch.rand(cells, generator=g) < 0.6, gt - 1, torch.randint(0, n, cells, generator=g))
    labels = torch.where(torch.rand(cells, generator=g) < 0.05, torch.full_like(labels, n if ldt == torch.uint8 else -2), labels)
    return up(labels)[2:h + 2, 3:w + 3].contiguous().to(ldt), up(gt)[:h, :w].contiguous().to(gdt)


# ------------------------------------------------------------------------------------------------- the specification
@pytest.mark.parametrize("raw", [True, False], ids=["raw", "ids"])
@pytest.mark.parametrize("gdt", list(BC.DTYPES), ids=["gt8", "gt16"])
@pytest.mark.parametrize("ldt", list(BC.DTYPES), ids=["l8", "l16"])
@pytest.mark.parametrize("k", range(len(BC.TABLE)), ids=BC.IDS)
def test_seg_boundary_areas_is_the_specification(k, ldt, gdt, raw):
    from ifseg_amd import hip
    dev = _dev()
    d = BC.TABLE[k][2]
    for outside in (False, True):
        assert BC.nonempty(k, ldt, raw, outside)                                      # a condition on the inputs
        labels, gt, n = BC.maps(BC.TABLE[k], BC.DTYPES[ldt], BC.DTYPES[gdt], raw, outside)
        want = BC.reference(k, ldt, raw, outside)
        _same(hip.seg_boundary_areas(labels.to(dev), gt.to(dev), n, d, raw, band=True), want, outside)
        # without the band the counters are the same, and [1, h, w] is [h, w]
        bareas, none = hip.seg_boundary_areas(labels[None].to(dev), gt[None].to(dev), n, d, raw)
        assert none is None and torch.equal(bareas.cpu(), want[0])


def test_a_batch_of_different_maps():
    from ifseg_amd import hip
    dev = _dev()
    h, w, n = 45, 150, 15
    pairs = [_random_blocks(h, w, n, s, torch.uint8, torch.uint8) for s in range(3)]
    labels, gt = torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])
    for d in (1, 3, 6, 20):
        got = hip.seg_boundary_areas(labels.to(dev), gt.to(dev), n, d, band=True)
        _same(got, _ref(labels, gt, n, d), d)
        each = [_ref(l, g, n, d) for l, g in pairs]
        assert torch.equal(got[0].cpu(), sum(e[0] for e in each)) and torch.equal(got[1].cpu(), torch.stack([e[1] for e in each]))
        assert (d == 20 or each[0][1].ne(each[1][1]).any()) and int(each[0][0][0].sum()) > 0      # conditions on the inputs


@pytest.mark.parametrize("shape", [(1, 1), (1, 200), (200, 1), (40, 5), (5, 40), (17, 65)])
def test_degenerate_sizes(shape):
    from ifseg_amd import hip
    dev = _dev()
    n = 7
    labels, gt = _random_blocks(*shape, n, shape[0], torch.int16, torch.uint8, 3, 4)
    for d in (1, 2, 6, 7, 64):                                                        # w < d, h < d among them
        _same(hip.seg_boundary_areas(labels.to(dev), gt.to(dev), n, d, band=True), _ref(labels, gt, n, d), d)


@pytest.mark.parametrize("ldt,gdt", [("u8", "u8"), ("i16", "i16")])
def test_a_band_wider_than_the_image_gives_seg_areas(ldt, gdt):
    from ifseg_amd import hip
    dev = _dev()
    h, w, n = 50, 61, 40
    labels, gt = _random_blocks(h, w, n, 4, BC.DTYPES[ldt], BC.DTYPES[gdt])
    ld, gd = labels.to(dev), gt.to(dev)
    areas, tally = hip.seg_areas(ld, gd, n)
    assert int(tally[0]) > 0 and (ld.long().lt(0) | ld.long().ge(n)).any()
    for d in (61, 64):
        bareas, band = hip.seg_boundary_areas(ld, gd, n, d, band=True)
        assert torch.equal(bareas, areas) and band.eq(3).all()
    assert not torch.equal(hip.seg_boundary_areas(ld, gd, n, 3)[0], areas)


@pytest.mark.parametrize("ldt,gdt", [("u8", "u8"), ("u8", "i16"), ("i16", "u8"), ("i16", "i16")], ids=["l8g8", "l8g16", "l16g8", "l16g16"])
def test_every_element_alignment(ldt, gdt):
    """both maps at every element offset inside 16 bytes, independently: slices of flat buffers viewed as [h, w]"""
    from ifseg_amd import hip
    dev = _dev()
    k = 1
    h, w, d = BC.TABLE[k][:3]
    labels, gt, n = BC.maps(BC.TABLE[k], BC.DTYPES[ldt], BC.DTYPES[gdt], True, True)
    want = BC.reference(k, ldt, True, True)
    lbuf = torch.zeros(h * w + 16, dtype=labels.dtype, device=dev)
    gbuf = torch.zeros(h * w + 16, dtype=gt.dtype, device=dev)
    assert lbuf.data_ptr() % 16 == 0 and gbuf.data_ptr() % 16 == 0
    got = {}
    for lo in range(16 // lbuf.element_size()):
        lab = lbuf[lo:lo + h * w].view(h, w)
        lab.copy_(labels)
        for go in range(16 // gbuf.element_size()):
            g = gbuf[go:go + h * w].view(h, w)
            g.copy_(gt)
            got[lo, go] = hip.seg_boundary_areas(lab, g, n, d, band=True)
    for key, res in got.items():
        _same(res, want, key)


@pytest.mark.parametrize("n,ldt,gdt", [(1, "u8", "u8"), (15, "u8", "u8"), (150, "u8", "i16"), (512, "i16", "i16")])
def test_class_counts_and_canaries(n, ldt, gdt):
    """n at both limits; bareas sits between canaries and is accumulated into: a second call doubles it; the band sits between
    canaries too (the C entry, which takes the caller's buffer)"""
    from ifseg_amd import hip
    dev = _dev()
    h, w, d = 70, 131, 5
    labels, gt = _random_blocks(h, w, n, n, BC.DTYPES[ldt], BC.DTYPES[gdt])
    want = _ref(labels, gt, n, d)
    assert int(want[0][0].sum()) > 0
    ld, gd = labels.to(dev), gt.to(dev)
    cbuf = torch.full((8 + 3 * n + 8,), -12345, dtype=torch.int64, device=dev)
    bareas = cbuf[8:8 + 3 * n].view(3, n)
    bareas.zero_()
    got = hip.seg_boundary_areas(ld, gd, n, d, bareas=bareas, band=True)
    assert got[0] is bareas
    _same(got, want)
    hip.seg_boundary_areas(ld, gd, n, d, bareas=bareas)
    assert torch.equal(bareas.cpu(), 2 * want[0])
    assert cbuf[:8].eq(-12345).all() and cbuf[8 + 3 * n:].eq(-12345).all()
    bbuf = torch.full((64 + h * w + 64,), 77, dtype=torch.uint8, device=dev)
    vp, i = ctypes.c_void_p, ctypes.c_int
    for off in (64, 61):                                                              # the band itself at any alignment
        bbuf.fill_(77)
        rc = hip.lib().ifseg_seg_boundary_areas(vp(ld.data_ptr()), i(ld.element_size()), vp(gd.data_ptr()), i(gd.element_size()), i(1),
                                                i(h), i(w), i(n), i(d), i(1), vp(bareas.data_ptr()), vp(bbuf.data_ptr() + off),
                                                vp(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
        assert torch.equal(bbuf[off:off + h * w].view(h, w).cpu(), want[1])
        assert bbuf[:off].eq(77).all() and bbuf[off + h * w:].eq(77).all()
    assert torch.equal(bareas.cpu(), 4 * want[0])


# ------------------------------------------------------------------------------------------------- the C entry point
def test_entry_point_refusals_and_limits():
    """each refusal returns its code and launches nothing: the poisoned buffers stay poisoned; the limits themselves pass"""
    from ifseg_amd import hip
    dev = _dev()
    lib = hip.lib()
    i, vp = ctypes.c_int, ctypes.c_void_p
    p = lambda t, off=0: vp(t.data_ptr() + off) if t is not None else vp(None)
    h, w = 6, 40
    lab = torch.zeros(h * w + 8, dtype=torch.int16, device=dev)
    gt = torch.zeros(h * w + 8, dtype=torch.int16, device=dev)
    cnt = torch.full((3 * 512 + 1,), -5, dtype=torch.int64, device=dev)
    band = torch.full((h * w + 8,), 99, dtype=torch.uint8, device=dev)

    def call(n=5, d=2, labp=p(lab), lb=2, gtp=p(gt), gb=2, B=1, h=h, w=w, cp=p(cnt), bp=p(band)):
        return lib.ifseg_seg_boundary_areas(labp, i(lb), gtp, i(gb), i(B), i(h), i(w), i(n), i(d), i(1), cp, bp, None)

    assert call(n=0) == BAD_ARG and call(n=513) == BAD_ARG and call(n=-1) == BAD_ARG
    assert call(d=0) == BAD_ARG and call(d=65) == BAD_ARG and call(d=-2) == BAD_ARG
    assert call(B=0) == BAD_SHAPE and call(h=0) == BAD_SHAPE and call(w=-1) == BAD_SHAPE
    assert call(B=2, h=32768, w=32768) == BAD_SHAPE and call(B=1, h=65536, w=32768) == BAD_SHAPE
    assert call(B=2 ** 30, h=2, w=1) == BAD_SHAPE and call(B=65536, h=65536, w=65536) == BAD_SHAPE
    assert call(labp=vp(None)) == BAD_ARG and call(gtp=vp(None)) == BAD_ARG and call(cp=vp(None)) == BAD_ARG
    assert call(labp=p(lab, 1)) == BAD_ARG and call(gtp=p(gt, 1)) == BAD_ARG        # int16 at an odd address
    assert call(cp=p(cnt, 4)) == BAD_ARG                                             # the counters not 8-byte aligned
    for bad in (0, 3, 4, -1):
        assert call(lb=bad) == BAD_ARG and call(gb=bad) == BAD_ARG
    torch.cuda.synchronize()
    assert cnt.eq(-5).all() and band.eq(99).all()                                     # no launch so far
    assert hip.seg_boundary_limits() == (64, 512) == (hip.SEG_BOUNDARY_MAX_D, hip.SEG_PREDICT_MAX_CLASSES)
    # the limits themselves pass: d = 64 with n = 512 (more than 64 KiB of LDS), maps at odd element offsets, no band.  Ground
    # truth 0 everywhere is ignored under raw labels, so no counter is written
    assert call(n=512, d=64, bp=vp(None)) == 0 and call(n=1, d=1, lb=1, gb=1, bp=vp(None)) == 0
    assert call(labp=p(lab, 2), gtp=p(gt, 6), bp=vp(None)) == 0
    torch.cuda.synchronize()
    assert cnt.eq(-5).all() and band.eq(99).all()
    assert call(n=512, d=64) == 0                                                     # and the band of a constant map at d = 64
    torch.cuda.synchronize()
    assert cnt.eq(-5).all() and band[:h * w].eq(3).all() and band[h * w:].eq(99).all()


# ------------------------------------------------------------------------------------------------- the op
def test_op_matches_binding_and_opcheck():
    from ifseg_amd import hip
    dev = _dev()
    n, d, shape = 257, 4, (2, 40, 83)
    pairs = [_random_blocks(40, 83, n, s, torch.int16, torch.int16) for s in (1, 2)]
    labels, gt = torch.stack([p[0] for p in pairs]).to(dev), torch.stack([p[1] for p in pairs]).to(dev)
    want = hip.seg_boundary_areas(labels, gt, n, d, band=True)
    _same(want, _ref(labels, gt, n, d))
    got = torch.ops.ifseg.seg_boundary_areas(labels, gt, n, d, True)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and got[1].shape == shape
    # fresh counters on every call; non-contiguous inputs are copied
    lt, gtt = labels.transpose(1, 2).contiguous().transpose(1, 2), gt.transpose(1, 2).contiguous().transpose(1, 2)
    assert not lt.is_contiguous()
    again = torch.ops.ifseg.seg_boundary_areas(lt, gtt, n, d, True)
    assert torch.equal(again[0], want[0]) and torch.equal(again[1], want[1]) and again[0].data_ptr() != got[0].data_ptr()
    ids = torch.where((gt == 0) | (gt == 255), torch.full_like(gt, n), gt - 1)
    _same(torch.ops.ifseg.seg_boundary_areas(labels[0], ids[0], n, d, False), _ref(labels[0], ids[0], n, d, False))
    utils = ("test_schema", "test_autograd_registration", "test_faketensor")
    torch.library.opcheck(torch.ops.ifseg.seg_boundary_areas, (labels, gt, n, d, True), test_utils=utils)
    torch.library.opcheck(torch.ops.ifseg.seg_boundary_areas, (labels[0, :5].contiguous().to(torch.uint8), gt[0, :5].contiguous(), 15, 1, False),
                          test_utils=utils)
    # on a side stream the op follows PyTorch's current stream
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        side = torch.ops.ifseg.seg_boundary_areas(labels, gt, n, d, True)
    st.synchronize()
    assert torch.equal(side[0], want[0]) and torch.equal(side[1], want[1])


# ------------------------------------------------------------------------------------------------- end to end
def _gts(raw, n):
    """ground truth in blocks of 8 x 8 pixels, so that both bands have an interior"""
    out = []
    for k, r in enumerate(raw):
        h, w = r.shape[:2]
        small = SC.ground_truth((-(-h // 8), -(-w // 8)), n, True, k, torch.int16 if k == 1 else torch.uint8)
        out.append(small.repeat_interleave(8, 0).repeat_interleave(8, 1)[:h, :w].contiguous())
    return out


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_evaluate_raw_with_boundary_iou(e2e, setting):  # noqa: F811
    from ifseg_amd.predict import SegmentationScore, boundary_areas_reference, boundary_distance, confusion_reference
    m, raw, ocfg, mk = e2e
    n = ocfg.num_seg_tokens
    kw, call = SETTINGS[setting]
    seg = mk(**kw)
    gts = _gts(raw, n)
    score, labels = seg.evaluate_raw(raw, gts, boundary_iou=True, return_labels=True, **call)
    b = score.boundary
    assert b.is_cuda and b.dtype == torch.int64 and b.shape == (3, n) and score.confusion is None and score.boundary_ratio == 0.02
    # the counters are the specification's of the labels the same call returned, summed over the images, d per image
    ds = [boundary_distance(*g.shape) for g in gts]
    assert ds == [2, 2, 2]
    want = sum(boundary_areas_reference(l.cpu(), g, n, d)[0] for l, g, d in zip(labels, gts, ds))
    assert torch.equal(b.cpu(), want) and int(want[2].sum()) > 0 and (b <= score.areas).all() and not torch.equal(b, score.areas)
    s = score.summary()
    assert "mBIoU" in s and len(s["BIoU"]) == n
    # areas, tally and the labels are what they are without it
    plain, plain_labels = seg.evaluate_raw(raw, gts, return_labels=True, **call)
    assert plain.boundary is None and torch.equal(plain.areas, score.areas) and torch.equal(plain.tally, score.tally)
    assert all(torch.equal(a, c) and a.dtype == c.dtype for a, c in zip(labels, plain_labels))
    assert repr({k: v for k, v in s.items() if k not in ("mBIoU", "BIoU")}) == repr(plain.summary())      # repr: NaN equals NaN
    # without return_labels the counters are the same; `into` accumulates without the keyword; another ratio, another band
    alone = seg.evaluate_raw(raw, gts, boundary_iou=True, **call)
    assert isinstance(alone, SegmentationScore) and torch.equal(alone.boundary, b) and torch.equal(alone.areas, score.areas)
    twice = seg.evaluate_raw(raw, gts, into=alone, **call)
    assert twice is alone and torch.equal(alone.boundary, 2 * b) and torch.equal(alone.areas, 2 * score.areas)
    wide = seg.evaluate_raw(raw, gts, boundary_iou=0.05, **call)
    want5 = sum(boundary_areas_reference(l.cpu(), g, n, boundary_distance(*g.shape, 0.05))[0] for l, g in zip(labels, gts))
    assert torch.equal(wide.boundary.cpu(), want5) and (wide.boundary >= b).all() and torch.equal(wide.areas, score.areas)
    # together with the matrix: each equal to its own reference
    both = seg.evaluate_raw(raw, gts, boundary_iou=True, confusion=True, **call)
    assert torch.equal(both.boundary, b) and torch.equal(both.areas, score.areas)
    assert torch.equal(both.confusion.cpu(), sum(confusion_reference(l.cpu(), g, n) for l, g in zip(labels, gts)))


def test_evaluate_and_task_pass_boundary_iou_on(e2e):  # noqa: F811
    import _predict_cases as PC
    from ifseg_amd.predict import boundary_areas_reference, boundary_distance
    from ifseg_amd.tasks.mm_tasks.segmentation import SegmentationTask
    m, raw, ocfg, mk = e2e
    n = ocfg.num_seg_tokens
    seg = mk()
    gts = _gts(raw, n)
    whole = seg.evaluate_raw(raw, gts, boundary_iou=True)
    task = SegmentationTask(num_seg_tokens=n, patch_image_size=ocfg.patch_image_size, category_token_ids=PC.E2E_NAMES)
    ts = task.evaluate_raw(m, raw, gts, prompt_ids=PC.E2E_PROMPT, boundary_iou=True)
    assert torch.equal(ts.boundary, whole.boundary) and torch.equal(ts.areas, whole.areas)
    assert repr(ts.summary()) == repr(whole.summary()) and "mBIoU" in ts.summary()
    # the batch call: one launch for the batch, d from the label maps' size
    tiled, gtile = raw[2].repeat(2, 2, 1), gts[2].repeat(2, 2)                        # 128 x 128, the network's own size
    img, g = torch.stack([tiled, tiled.flip(0)]).to("cuda:0"), torch.stack([gtile, gtile.flip(1)])
    a, la = seg.evaluate(img, g, return_labels=True, boundary_iou=True)
    assert boundary_distance(128, 128) == 4
    assert torch.equal(a.boundary.cpu(), boundary_areas_reference(la.cpu(), g, n, 4)[0]) and int(a.boundary[2].sum()) > 0
    c = seg.evaluate(img, g)
    assert c.boundary is None and torch.equal(a.areas, c.areas) and torch.equal(a.tally, c.tally)
