"""GPU: the class confusion matrix of csrc/predict.hip -- hip.seg_confusion, both of its counting regimes (the direct LDS table
up to n = 127, the hashed table above, and the route past a crowded hashed table) -- against the CPU specification
`confusion_reference`, the raw C entry's refusals, the op through the dispatcher, and Segmenter.evaluate_raw(confusion=True)
end to end on the segofa_tiny fixture.  The counters are integers: every comparison is exact, and no pixel is left out."""
import ctypes

import pytest
import torch

import _score_cases as SC
from test_predict_views_gpu import e2e  # noqa: F401  (the segofa_tiny fixture with its three raw shapes)

pytestmark = pytest.mark.gpu

BAD_SHAPE, BAD_ARG = -2, -3


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ifseg_amd.ops  # noqa: F401
    return torch.device("cuda:0")


def _ref(labels, gt, n, raw=True):
    from ifseg_amd.predict import confusion_reference
    return confusion_reference(labels.cpu(), gt.cpu(), n, raw)


def _runs(values, npix, g):
    """piecewise constant: runs of 50 .. 200 pixels, each of one of `values`"""
    lengths = torch.randint(50, 201, (npix // 50 + 1,), generator=g)
    return values[torch.randint(0, len(values), lengths.shape, generator=g)].repeat_interleave(lengths)[:npix]


def _labels(npix, n, ldt, seed, runs):
    """predictions in [0, n), about one in eight outside it: n itself, beyond, 255, negative (what the dtype holds)"""
    g = torch.Generator().manual_seed(7000 + seed)
    lo, hi = (0, 255) if ldt == torch.uint8 else (-32768, 32767)
    outside = [v for v in (n, n + 3, 255, -1, -300, 32767) if lo <= v <= hi and not 0 <= v < n]
    values = torch.cat([torch.arange(n).repeat(7 * len(outside)), torch.tensor(outside, dtype=torch.long).repeat(n)])
    out = _runs(values, npix, g) if runs else values[torch.randint(0, len(values), (npix,), generator=g)]
    return out.to(ldt)


def _ground_truth(npix, n, raw, seed, dtype, runs):
    """valid classes and ignore values, every kind of value in front where there is room"""
    gt = SC.ground_truth((npix,), n, raw, seed, dtype)
    if runs:
        gt = _runs(gt[:max(npix // 4, 1)].long(), npix, torch.Generator().manual_seed(8000 + seed)).to(dtype)
    if npix >= 63:
        special = torch.tensor(SC.every_kind(n, raw, dtype)).to(dtype)
        gt[:special.numel()] = special
    return gt


# ------------------------------------------------------------------------------------------------- the specification
NPIX = (1, 3, 63, 1024, 37 * 91 * 3)
NS = ((1, torch.uint8), (15, torch.uint8), (127, torch.uint8), (128, torch.uint8), (150, torch.uint8), (257, torch.int16),
      (512, torch.int16))


@pytest.mark.parametrize("raw", [True, False], ids=["raw", "ids"])
@pytest.mark.parametrize("gt_dtype", [torch.uint8, torch.int16], ids=["gt8", "gt16"])
@pytest.mark.parametrize("n,ldt", NS)
def test_seg_confusion_is_the_specification(n, ldt, gt_dtype, raw):
    from ifseg_amd import hip
    dev = _dev()
    assert (n * (n + 1) <= hip.SEG_CONFUSION_DIRECT_MAX) == (n <= 127)              # both sides of the switch are in NS
    for npix in NPIX:
        for runs in (True, False):
            labels = _labels(npix, n, ldt, npix + n, runs)
            gt = _ground_truth(npix, n, raw, npix + n, gt_dtype, runs)
            C = hip.seg_confusion(labels.to(dev), gt.to(dev), n, raw)
            assert C.dtype == torch.int64 and C.shape == (n, n + 1) and C.is_contiguous()
            want = _ref(labels, gt, n, raw)
            assert torch.equal(C.cpu(), want), (npix, n, runs)
            if npix >= 1024 and not runs:
                assert int(want[:, n].sum()) > 0 and int(want[:, :n].sum()) > 0         # outside predictions were among them
        # the identities with seg_areas' counters of the same inputs (the last of the loop)
        areas, tally = hip.seg_areas(labels.to(dev), gt.to(dev), n, raw)
        assert int(C.sum()) == int(tally[0]) and torch.equal(C[:, :n].diagonal(), areas[0])
        assert torch.equal(C[:, :n].sum(0), areas[1]) and torch.equal(C.sum(1), areas[2])


@pytest.mark.parametrize("ldt,gt_dtype", [(torch.uint8, torch.uint8), (torch.uint8, torch.int16), (torch.int16, torch.uint8),
                                          (torch.int16, torch.int16)], ids=["l8g8", "l8g16", "l16g8", "l16g16"])
@pytest.mark.parametrize("n", [150, 15], ids=["hashed", "direct"])
def test_seg_confusion_at_every_alignment_with_canaries(n, ldt, gt_dtype):
    """label and ground-truth pointers at every element offset inside 16 bytes, independently; the matrix sits between
    canaries and is accumulated into: the second call doubles it.  n = 150 counts in the hashed table, 15 in the direct one"""
    from ifseg_amd import hip
    dev = _dev()
    npix = 1000
    assert (n * (n + 1) > hip.SEG_CONFUSION_DIRECT_MAX) == (n == 150)
    assert hip.seg_confusion_limits() == (hip.SEG_CONFUSION_DIRECT_MAX, hip.SEG_CONFUSION_SLOTS, hip.SEG_CONFUSION_STEP_PIXELS,
                                          hip.SEG_CONFUSION_MAX_BLOCKS)
    lbuf = _labels(npix + 16, n, ldt, 9, True).to(dev)
    gbuf = SC.ground_truth((npix + 16,), n, True, 3, gt_dtype).to(dev)
    assert lbuf.data_ptr() % 16 == 0 and gbuf.data_ptr() % 16 == 0
    cbuf = torch.full((8 + n * (n + 1) + 8,), -12345, dtype=torch.int64, device=dev)
    C = cbuf[8:8 + n * (n + 1)].view(n, n + 1)
    refs = {}
    for lo in range(0, 16 // lbuf.element_size()):
        for go in range(0, 16 // gbuf.element_size()):
            # another length per offset pair, so that the tail takes every length too
            m = npix - 16 + (lo * 5 + go) % 17
            lab, gt = lbuf[lo:lo + m], gbuf[go:go + m]
            C.zero_()
            assert hip.seg_confusion(lab, gt, n, True, confusion=C) is C
            refs[lo, go] = (C.clone(), lab.cpu(), gt.cpu())
    hip.seg_confusion(lab, gt, n, True, confusion=C)
    assert torch.equal(C, 2 * refs[lo, go][0])
    assert cbuf[:8].eq(-12345).all() and cbuf[8 + n * (n + 1):].eq(-12345).all()
    for key, (c, lab, gt) in refs.items():
        assert torch.equal(c.cpu(), _ref(lab, gt, n)), key


# ------------------------------------------------------------------------------------------------- past the hashed table
def _first_workgroup_pairs(labels, gt, n, hip):
    """the distinct (class, label) pairs among the scored pixels that the launch's first workgroup takes: labels at a
    16-byte boundary, so the pixels are groups of 16, a workgroup takes 256 groups per step and the grid strides"""
    npix = labels.numel()
    groups = npix // 16
    blocks = min(max((groups + 255) // 256, 1), hip.SEG_CONFUSION_MAX_BLOCKS)
    step = torch.arange(groups * 16) // hip.SEG_CONFUSION_STEP_PIXELS
    mine = (step % blocks) == 0
    g = gt[:groups * 16][mine].long()
    scored = (g != 0) & (g != 255) & (g >= 1) & (g <= n)
    return torch.unique((g[scored] - 1) * (n + 1) + labels[:groups * 16][mine][scored].long()).numel()


@pytest.mark.parametrize("half_constant", [False, True], ids=["random", "half_one_pair"])
def test_seg_confusion_beyond_the_hashed_table(half_constant):
    """n = 512 with independent random labels and ground truth per pixel: every workgroup meets more distinct pairs than its
    table has slots, so pairs leave by the direct route too; with the second half of the pixels one constant pair, that pair's
    aggregated adds arrive at a crowded table and reach its bin through the table in some workgroups and past it in others"""
    from ifseg_amd import hip
    dev = _dev()
    n = 512
    assert n * (n + 1) > hip.SEG_CONFUSION_DIRECT_MAX
    # every workgroup of a full grid takes `steps` steps; twice as many random pixels as the table has slots, and twice
    # that where half of them are constant
    steps = -(-2 * hip.SEG_CONFUSION_SLOTS // hip.SEG_CONFUSION_STEP_PIXELS) * (2 if half_constant else 1)
    npix = hip.SEG_CONFUSION_MAX_BLOCKS * hip.SEG_CONFUSION_STEP_PIXELS * steps
    g = torch.Generator().manual_seed(77)
    labels = torch.randint(0, n, (npix,), generator=g).to(torch.int16)
    gt = torch.randint(0, n + 2, (npix,), generator=g).to(torch.int16)               # raw values: 0 ignored, n + 1 out of range
    if half_constant:
        # the second half, so a workgroup has crowded its table before it meets the pair (299, 7) by the wave: in some
        # workgroups the pair still finds a slot, in others it goes past the table
        labels[npix // 2:], gt[npix // 2:] = 7, 300
    assert _first_workgroup_pairs(labels, gt, n, hip) > hip.SEG_CONFUSION_SLOTS
    ld, gd = labels.to(dev), gt.to(dev)
    assert ld.data_ptr() % 16 == 0
    C = hip.seg_confusion(ld, gd, n, True)
    want = _ref(labels, gt, n)
    assert torch.equal(C.cpu(), want)
    if half_constant:
        assert int(want[299, 7]) >= npix // 2
    areas, tally = hip.seg_areas(ld, gd, n, True)
    assert int(C.sum()) == int(tally[0]) and torch.equal(C.sum(1), areas[2]) and torch.equal(C[:, :n].sum(0), areas[1])


# ------------------------------------------------------------------------------------------------- degenerate maps
@pytest.mark.parametrize("n,ldt", [(15, torch.uint8), (150, torch.uint8), (300, torch.int16)])
def test_seg_confusion_degenerate_maps(n, ldt):
    from ifseg_amd import hip
    dev = _dev()
    shape = (3, 37, 91)
    npix = 3 * 37 * 91
    labels = torch.full(shape, 4, dtype=ldt, device=dev)
    C = hip.seg_confusion(labels, torch.full(shape, 6, dtype=torch.uint8, device=dev), n)          # raw 6 is class 5
    want = torch.zeros(n, n + 1, dtype=torch.int64)
    want[5, 4] = npix
    assert torch.equal(C.cpu(), want)
    # nothing scored: ignore values in both modes, and everything out of range
    for value, raw, gdt in ((0, True, torch.uint8), (255, True, torch.uint8), (n, False, torch.int16), (255, False, torch.uint8),
                            (n + 1, True, torch.int16), (-3, False, torch.int16)):
        C = hip.seg_confusion(labels, torch.full(shape, value, dtype=gdt, device=dev), n, raw)
        assert not C.any(), (value, raw)
    # all predictions outside: only column n is filled
    gt = SC.ground_truth(shape, n, True, 5, torch.int16)
    for value in (n, -1, 32767) if ldt == torch.int16 else (n, 255):
        C = hip.seg_confusion(torch.full(shape, value, dtype=ldt, device=dev), gt.to(dev), n)
        assert not C[:, :n].any() and int(C[:, n].sum()) > 0
        assert torch.equal(C.cpu(), _ref(torch.full(shape, value, dtype=ldt), gt, n))


# ------------------------------------------------------------------------------------------------- the C entry point
def test_entry_point_refusals():
    """each refusal returns its code and launches nothing: the poisoned matrix stays poisoned"""
    from ifseg_amd import hip
    dev = _dev()
    lib = hip.lib()
    i, ll, vp = ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p
    p = lambda t, off=0: vp(t.data_ptr() + off) if t is not None else vp(None)
    lab = torch.zeros(64, dtype=torch.int16, device=dev)
    gt = torch.zeros(64, dtype=torch.int16, device=dev)
    cnt = torch.full((512 * 513 + 1,), -5, dtype=torch.int64, device=dev)

    def call(n=5, labp=p(lab), lb=2, gtp=p(gt), gb=2, npix=16, cp=p(cnt)):
        return lib.ifseg_seg_confusion(labp, i(lb), gtp, i(gb), ll(npix), i(n), i(1), cp, None)

    assert call(n=0) == BAD_ARG and call(n=513) == BAD_ARG and call(n=-1) == BAD_ARG
    assert call(npix=0) == BAD_SHAPE and call(npix=-4) == BAD_SHAPE and call(npix=2 ** 31) == BAD_SHAPE
    assert call(labp=vp(None)) == BAD_ARG and call(gtp=vp(None)) == BAD_ARG and call(cp=vp(None)) == BAD_ARG
    assert call(labp=p(lab, 1)) == BAD_ARG and call(gtp=p(gt, 1)) == BAD_ARG        # int16 at an odd address
    assert call(cp=p(cnt, 4)) == BAD_ARG                                             # the matrix not 8-byte aligned
    for bad in (0, 3, 4, -1):
        assert call(lb=bad) == BAD_ARG and call(gb=bad) == BAD_ARG
    torch.cuda.synchronize()
    assert cnt.eq(-5).all()                                                           # no launch so far
    # the limits themselves pass: n = 512, ground truth 0 everywhere is ignored under raw labels, so nothing is written
    assert call(n=512) == 0 and call(n=1, lb=1, gb=1, npix=1) == 0 and call(labp=p(lab, 2), gtp=p(gt, 6), npix=40) == 0
    torch.cuda.synchronize()
    assert cnt.eq(-5).all()


# ------------------------------------------------------------------------------------------------- the op
def test_op_matches_binding_and_opcheck():
    from ifseg_amd import hip
    dev = _dev()
    n, shape = 257, (2, 40, 23)
    labels = _labels(2 * 40 * 23, n, torch.int16, 1, True).reshape(shape).to(dev)
    gt = SC.ground_truth(shape, n, True, 1, torch.int16).to(dev)
    want = hip.seg_confusion(labels, gt, n, True)
    assert torch.equal(want.cpu(), _ref(labels, gt, n))
    C = torch.ops.ifseg.seg_confusion(labels, gt, n, True)
    assert torch.equal(C, want) and C.dtype == torch.int64 and C.shape == (n, n + 1)
    # fresh counters on every call; non-contiguous inputs are copied
    C2 = torch.ops.ifseg.seg_confusion(labels.transpose(1, 2), gt.transpose(1, 2), n, True)
    assert torch.equal(C2, want) and C2.data_ptr() != C.data_ptr()
    ids = torch.where((gt == 0) | (gt == 255), torch.full_like(gt, n), gt - 1)
    assert torch.equal(torch.ops.ifseg.seg_confusion(labels, ids, n, False).cpu(), _ref(labels, ids, n, False))
    utils = ("test_schema", "test_autograd_registration", "test_faketensor")
    torch.library.opcheck(torch.ops.ifseg.seg_confusion, (labels, gt, n, True), test_utils=utils)
    torch.library.opcheck(torch.ops.ifseg.seg_confusion, (labels[0, :5].contiguous().to(torch.uint8), gt[0, :5].contiguous(), 15, False),
                          test_utils=utils)
    # on a side stream the op follows PyTorch's current stream
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        C3 = torch.ops.ifseg.seg_confusion(labels, gt, n, True)
    st.synchronize()
    assert torch.equal(C3, want)


# ------------------------------------------------------------------------------------------------- end to end
SETTINGS = {"single": ({}, {}), "ms_flip": ({}, {"scales": (0.75, 1.0), "flip": True}), "slide": ({}, {"slide": True}),
            "slide_views": ({"slide_views": True}, {"slide": True, "scales": (0.75, 1.0), "flip": True}),
            "crf": ({"crf_iters": 1}, {})}


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_evaluate_raw_with_confusion(e2e, setting):  # noqa: F811
    from ifseg_amd.predict import SegmentationScore, confusion_reference
    m, raw, ocfg, mk = e2e
    n = ocfg.num_seg_tokens
    kw, call = SETTINGS[setting]
    seg = mk(**kw)
    gts = [SC.ground_truth(tuple(r.shape[:2]), n, True, k, torch.int16 if k == 1 else torch.uint8) for k, r in enumerate(raw)]
    score, labels = seg.evaluate_raw(raw, gts, confusion=True, return_labels=True, **call)
    C = score.confusion
    assert C.is_cuda and C.dtype == torch.int64 and C.shape == (n, n + 1)
    # the matrix is the specification's of the labels the same call returned, summed over the images
    want = sum(confusion_reference(l.cpu(), g, n) for l, g in zip(labels, gts))
    assert torch.equal(C.cpu(), want) and int(want.sum()) > 0
    # the four identities within the one score
    assert int(C.sum()) == int(score.tally[0]) and torch.equal(C[:, :n].diagonal(), score.areas[0])
    assert torch.equal(C[:, :n].sum(0), score.areas[1]) and torch.equal(C.sum(1), score.areas[2])
    # areas, tally and the labels are what they are without the matrix
    plain, plain_labels = seg.evaluate_raw(raw, gts, confusion=False, return_labels=True, **call)
    assert plain.confusion is None and torch.equal(plain.areas, score.areas) and torch.equal(plain.tally, score.tally)
    assert all(torch.equal(a, b) and a.dtype == b.dtype for a, b in zip(labels, plain_labels))
    # without return_labels the matrix is the same and no labels come back
    alone = seg.evaluate_raw(raw, gts, confusion=True, **call)
    assert isinstance(alone, SegmentationScore) and torch.equal(alone.confusion, C) and torch.equal(alone.areas, score.areas)
    # `into` decides: a matrix-less score stays matrix-less, one with a matrix is accumulated into without the keyword
    into = seg.evaluate_raw(raw, gts, into=SegmentationScore(n, torch.device("cuda:0")), confusion=False, **call)
    assert into.confusion is None and torch.equal(into.areas, score.areas)
    twice = seg.evaluate_raw(raw, gts, into=alone, **call)
    assert twice is alone and torch.equal(alone.confusion, 2 * C) and torch.equal(alone.areas, 2 * score.areas)


def test_evaluate_and_task_pass_confusion_on(e2e):  # noqa: F811
    import _predict_cases as PC
    from ifseg_amd.predict import confusion_reference
    from ifseg_amd.tasks.mm_tasks.segmentation import SegmentationTask
    m, raw, ocfg, mk = e2e
    n = ocfg.num_seg_tokens
    seg = mk()
    gts = [SC.ground_truth(tuple(r.shape[:2]), n, True, k) for k, r in enumerate(raw)]
    whole = seg.evaluate_raw(raw, gts, confusion=True)
    task = SegmentationTask(num_seg_tokens=n, patch_image_size=ocfg.patch_image_size, category_token_ids=PC.E2E_NAMES)
    ts = task.evaluate_raw(m, raw, gts, prompt_ids=PC.E2E_PROMPT, confusion=True)
    assert torch.equal(ts.confusion, whole.confusion) and torch.equal(ts.areas, whole.areas)
    # the batch call
    tiled, gtile = raw[2].repeat(2, 2, 1), gts[2].repeat(2, 2)                        # 128 x 128, the network's own size
    img, g = torch.stack([tiled, tiled.flip(0)]).to("cuda:0"), torch.stack([gtile, gtile.flip(1)])
    a, la = seg.evaluate(img, g, return_labels=True, confusion=True)
    assert torch.equal(a.confusion.cpu(), confusion_reference(la.cpu(), g, n))
    b = seg.evaluate(img, g)
    assert b.confusion is None and torch.equal(a.areas, b.areas) and torch.equal(a.tally, b.tally)
    # what a user does with it: the largest confusions name pairs of the matrix, and merging to two groups keeps the pixels
    top = whole.confusions(3)
    assert all(int(whole.confusion[c, p]) == v and c != p for c, p, v, _ in top)
    two = whole.merged([k % 2 for k in range(n)])
    assert two.n == 2 and int(two.tally[0]) == int(whole.tally[0]) and int(two.confusion.sum()) == int(whole.confusion.sum())
