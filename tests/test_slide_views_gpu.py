"""GPU: multi-scale + flip over sliding windows -- hip.seg_predict_slide_views / hip.seg_score_slide_views (csrc/predict.hip)
against the CPU specification `slide_views_reference`, hip.image_load_windows(flip=True) (csrc/imgload.hip) against slices of the
mirrored hip.image_load, the two ops through the dispatcher, and Segmenter(slide_views=True).segment_raw / evaluate_raw end to
end on the segofa_tiny fixture.  The comparison rule is in tests/_slide_views_cases.py.

Data paths: the merge kernel stages the patches of every view's windows under a tile in LDS, view after view while the buffer
lasts, and reads global memory for the rest; `staging_bytes=0` sends every view down the second path."""
import pytest
import torch

import _predict_cases as PC
import _score_cases as SCO
import _slide_cases as SC
import _slide_views_cases as C

pytestmark = pytest.mark.gpu

PATHS = {"staged": None, "direct": 0}          # staging_bytes=...


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ifseg_amd.ops  # noqa: F401
    return torch.device("cuda:0")


def _bits(t):
    return t.view(torch.int32)


# ------------------------------------------------------------------------------------------------- exact family
@pytest.mark.parametrize("K", C.EXACT_VIEWS)
@pytest.mark.parametrize("name", list(SC.EXACT_CASES))
def test_exact_family_bit_for_bit(name, K):
    from ifseg_amd import hip
    from ifseg_amd.predict import slide_views_reference
    dev = _dev()
    views, crop, stride, h, w = C.exact_views(name, K)
    B, n = views[0][0].shape[0], views[0][0].shape[3]
    rl, rc, rp = slide_views_reference(views, crop, stride, h, w, False, torch.float64)
    vd = C.to_device(views, dev)
    for path, sb in PATHS.items():
        lab, conf, probs = hip.seg_predict_slide_views(vd, crop, stride, h, w, False, conf=True, probs=True, staging_bytes=sb)
        assert lab.dtype == (torch.int16 if n > 256 else torch.uint8) and lab.shape == (B, h, w)
        assert torch.equal(lab.cpu().long(), rl), path
        assert torch.equal(conf.cpu().double(), rc), path
        assert torch.equal(probs.cpu().double(), rp), path
        l2, c2, p2 = hip.seg_predict_slide_views(vd, crop, stride, h, w, False, staging_bytes=sb)
        assert torch.equal(l2, lab) and c2 is None and p2 is None


# ------------------------------------------------------------------------------------------------- general family
@pytest.mark.parametrize("softmax", [False, True], ids=["linear", "softmax"])
@pytest.mark.parametrize("case", C.GENERAL_CASES, ids=[str(i) for i in range(len(C.GENERAL_CASES))])
def test_general_family_both_paths(case, softmax):
    from ifseg_amd import hip
    dev = _dev()
    for seed in C.SEEDS:
        views, crop, stride, h, w = C.general_views(case, seed, softmax)
        ref = C.reference(("general", str(case), softmax, seed), views, crop, stride, h, w, softmax)
        print(case[:7], seed, "e = %.2e, undecided %.3f %%" % (ref.e, 100 * ref.undecided_share))
        vd = C.to_device(views, dev)
        got = {}
        for path, sb in PATHS.items():
            lab, conf, probs = got[path] = hip.seg_predict_slide_views(vd, crop, stride, h, w, softmax, conf=True, probs=True,
                                                                       staging_bytes=sb)
            print(path, "max |d| / e = %.3f" % ((probs.cpu().double() - ref.probs).abs().max().item() / ref.e))
            ref.check(lab, conf, probs, what=(case[:7], softmax, seed, path))
            assert torch.equal(hip.seg_predict_slide_views(vd, crop, stride, h, w, softmax, staging_bytes=sb)[0], lab)
        # staging_bytes=0 gives the same bits
        assert all(torch.equal(a, b) for a, b in zip(got["staged"], got["direct"]))


def test_batch_and_unaligned_rows():
    """B = 3 with an odd width: the rows of images 1 and 2 start at every alignment of the wide label / conf stores"""
    from ifseg_amd import hip
    dev = _dev()
    B, case = C.BATCH_CASE
    for softmax in (True, False):
        views, crop, stride, h, w = C.general_views(case, 11, softmax, batch=B)
        ref = C.reference(("batch",) if softmax else ("batch", "linear"), views, crop, stride, h, w, softmax)
        lab, conf, probs = hip.seg_predict_slide_views(C.to_device(views, dev), crop, stride, h, w, softmax, conf=True, probs=True)
        assert lab.shape == (B, h, w) and w % 4 != 0
        print("batch", softmax, "max |d| / e = %.3f" % ((probs.cpu().double() - ref.probs).abs().max().item() / ref.e))
        ref.check(lab, conf, probs, what=("batch 3", softmax))


def test_one_unflipped_linear_view_is_seg_predict_windows_bit_for_bit():
    from ifseg_amd import hip
    dev = _dev()
    for case in (SC.GENERAL_CASES[1], SC.GENERAL_CASES[3], SC.GENERAL_CASES[4]):
        hpw, wpw, n, oh, ow, crop, stride, h, w = case
        for softmaxed in (False, True):
            s = SC.general_scores(case, 3, softmaxed, batch=2).to(dev)
            for path, sb in PATHS.items():
                a = hip.seg_predict_slide_views([(s, hpw, wpw, oh, ow, False)], crop, stride, h, w, False, conf=True, probs=True,
                                                staging_bytes=sb)
                b = hip.seg_predict_windows(s, hpw, wpw, oh, ow, crop, stride, h, w, conf=True, probs=True, staging_bytes=sb)
                assert torch.equal(a[0], b[0]) and torch.equal(_bits(a[1]), _bits(b[1])) and torch.equal(_bits(a[2]), _bits(b[2]))


def test_entry_point_refusals():
    """the C entry refuses what the contract excludes, whatever the binding let through; nothing is launched"""
    import ctypes
    from ifseg_amd import hip
    dev = _dev()
    lib = hip.lib()
    s = torch.zeros(1, 64, 1, 513, device=dev)
    out = torch.full((64,), 77, dtype=torch.int16, device=dev)
    i, p = ctypes.c_int, lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else None)
    BAD_SHAPE, BAD_ARG = -2, -3

    def call(K=1, B=1, hpw=1, wpw=1, n=5, oh=8, ow=8, ch=4, cw=4, sh=4, sw=4, h=4, w=4, lb=2, scores=s, softmax=0, table=True):
        t = (hip._SlideView * max(K, 1))()
        for k in range(max(K, 1)):
            t[k] = hip._SlideView(p(scores), hpw, wpw, oh, ow, k % 2)
        return lib.ifseg_seg_predict_slide_views(t if table else None, i(K), i(B), i(n), i(ch), i(cw), i(sh), i(sw), i(h), i(w),
                                                 i(softmax), p(out), i(lb), None, None, None)

    assert call(table=False) == BAD_ARG and call(K=0) == BAD_ARG and call(K=17) == BAD_ARG and call(scores=None) == BAD_ARG
    assert call(n=513) == BAD_ARG and call(n=0) == BAD_ARG and call(n=300, lb=1) == BAD_ARG and call(lb=4) == BAD_ARG
    assert call(h=0) == BAD_SHAPE and call(B=0) == BAD_SHAPE and call(hpw=0) == BAD_SHAPE and call(oh=0) == BAD_SHAPE
    assert call(h=2 ** 16, w=2 ** 15) == BAD_SHAPE and call(sh=5) == BAD_SHAPE and call(cw=0) == BAD_SHAPE
    assert call(oh=9, ch=1, cw=1, sh=1, sw=1) == BAD_SHAPE                                   # 9 x 8 = 72 windows
    assert call(oh=64, ow=64, ch=8, cw=8, sh=8, sw=8, hpw=256, wpw=256) == BAD_SHAPE         # Nw hpw wpw >= 2^22
    gt = torch.zeros(16, dtype=torch.uint8, device=dev)
    cnt = torch.full((3 * 5 + 2,), 5, dtype=torch.int64, device=dev)
    t = (hip._SlideView * 1)(hip._SlideView(p(s), 1, 1, 8, 8, 0))

    def score(n=5, gtp=gt, gb=1, areas=cnt):
        return lib.ifseg_seg_score_slide_views(t, i(1), i(1), i(n), i(4), i(4), i(4), i(4), i(4), i(4), i(1), p(out), i(2), None, None,
                                               p(gtp), i(gb), i(1), p(areas), p(cnt[15:]), None)

    assert score(n=513) == BAD_ARG and score(gtp=None) == BAD_ARG and score(gb=3) == BAD_ARG and score(areas=None) == BAD_ARG
    torch.cuda.synchronize()
    assert out.eq(77).all() and cnt.eq(5).all()                                              # no launch so far
    # the limits themselves are fine: 16 views of 64 windows, 300 classes, int16 labels, both orders
    for softmax in (0, 1):
        out.fill_(77)
        assert call(K=16, n=300, ch=1, cw=1, sh=1, sw=1, softmax=softmax) == 0
        torch.cuda.synchronize()
        assert out[:16].eq(0).all() and out[16:].eq(77).all()
    assert score() == 0                                                                       # raw 0 everywhere: nothing scored
    torch.cuda.synchronize()
    assert cnt.eq(5).all()


# ------------------------------------------------------------------------------------------------- scoring
@pytest.mark.parametrize("raw", [True, False], ids=["raw", "ids"])
@pytest.mark.parametrize("gt_dtype", [torch.uint8, torch.int16], ids=["gt8", "gt16"])
def test_seg_score_slide_views_counts_its_own_labels(gt_dtype, raw):
    from ifseg_amd import hip
    from ifseg_amd.predict import areas_reference
    dev = _dev()
    for case, softmax in ((C.GENERAL_CASES[2], True), (C.GENERAL_CASES[3], False)):     # 16 views of 5 classes; 257 classes
        hpw, wpw, n, crop, stride, h, w, planes = case
        views, crop, stride, h, w = C.general_views(case, 1, softmax, batch=2)
        vd = C.to_device(views, dev)
        gt = SCO.ground_truth((2, h, w), n, raw, n, gt_dtype)
        special = torch.tensor(SCO.every_kind(n, raw, gt_dtype)).to(gt_dtype)
        gt.view(-1)[:special.numel()] = special
        gd = gt.to(dev)
        for path, sb in PATHS.items():
            plain = hip.seg_predict_slide_views(vd, crop, stride, h, w, softmax, conf=True, probs=True, staging_bytes=sb)
            areas, tally, lab, conf, probs = hip.seg_score_slide_views(vd, crop, stride, gd, softmax, raw, labels=True, conf=True,
                                                                       probs=True, staging_bytes=sb)
            assert all(torch.equal(a, b) for a, b in zip((lab, conf, probs), plain)), (case[:7], path)
            ra, rt = areas_reference(lab.cpu(), gt, n, raw)
            assert torch.equal(areas.cpu(), ra) and torch.equal(tally.cpu(), rt), (case[:7], path)
            # counters only: the same counters, nothing else written; accumulated into existing ones
            a2, t2, l2, c2, p2 = hip.seg_score_slide_views(vd, crop, stride, gd, softmax, raw, staging_bytes=sb)
            assert l2 is None and c2 is None and p2 is None and torch.equal(a2, areas) and torch.equal(t2, tally)
            a3, t3 = hip.seg_score_slide_views(vd, crop, stride, gd, softmax, raw, areas=a2, tally=t2, staging_bytes=sb)[:2]
            assert a3 is a2 and t3 is t2 and torch.equal(a3, 2 * areas) and torch.equal(t3, 2 * tally)


# ------------------------------------------------------------------------------------------------- mirrored windows
MIRROR_CASES = [((2, 48, 100), (64, 133), 64, 42),             # windows at x = 0, 42, 69: not symmetric
                ((1, 91, 37), (157, 64), 64, 42)]              # windows down the image, one column of them


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("case", MIRROR_CASES, ids=[str(i) for i in range(len(MIRROR_CASES))])
def test_image_load_windows_flip_is_slices_of_the_mirrored_image_load(case, path):
    from ifseg_amd import hip
    from ifseg_amd.imageio import IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD, slide_windows
    dev = _dev()
    (B, H0, W0), (oh, ow), crop, stride = case
    img = torch.randint(0, 256, (B, H0, W0, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(H0)).to(dev)
    ys, xs, ch, cw = slide_windows(oh, ow, crop, stride)
    nw = len(ys) * len(xs)
    for dtype in (torch.float32, torch.bfloat16):
        bits = torch.int32 if dtype == torch.float32 else torch.int16
        for kw in ({}, {"mean": IMAGENET_DEFAULT_MEAN, "std": IMAGENET_DEFAULT_STD, "reverse_channels": True}):
            full = hip.image_load(img, oh, ow, dtype=dtype, staging_bytes=PATHS[path], **kw).flip(-1)
            wins = hip.image_load_windows(img, oh, ow, crop, stride, dtype=dtype, staging_bytes=PATHS[path], flip=True, **kw)
            assert wins.shape == (B * nw, 3, ch, cw) and wins.dtype == dtype and wins.is_contiguous()
            want = torch.stack([full[:, :, y:y + ch, x:x + cw] for y in ys for x in xs], 1).reshape(B * nw, 3, ch, cw)
            assert torch.equal(wins.view(bits), want.contiguous().view(bits)), (dtype, kw)
            # flip=False is the entry point as it was
            plain = hip.image_load_windows(img, oh, ow, crop, stride, dtype=dtype, staging_bytes=PATHS[path], flip=False, **kw)
            assert torch.equal(plain.view(bits), hip.image_load_windows(img, oh, ow, crop, stride, dtype=dtype,
                                                                        staging_bytes=PATHS[path], **kw).view(bits))


# ------------------------------------------------------------------------------------------------- the ops
def test_ops_match_bindings_and_opcheck():
    from ifseg_amd import hip
    dev = _dev()
    case = C.GENERAL_CASES[3]                                  # 257 classes: int16 labels; a non-square crop
    hpw, wpw, n, crop, stride, h, w, planes = case
    views, crop, stride, h, w = C.general_views(case, 3, True, batch=2)
    vd = C.to_device(views, dev)
    scores = [v[0] for v in vd]
    args = (scores, [hpw] * 2, [wpw] * 2, [p[0] for p in planes], [p[1] for p in planes], [bool(p[2]) for p in planes], list(crop),
            list(stride))
    for softmax in (True, False):
        rl, rc, rp = hip.seg_predict_slide_views(vd, crop, stride, h, w, softmax, conf=True, probs=True)
        lab, conf, probs = torch.ops.ifseg.seg_predict_slide_views(*args, h, w, softmax, True, True)
        assert lab.dtype == torch.int16 and torch.equal(lab, rl) and torch.equal(conf, rc) and torch.equal(probs, rp)
        lab, conf, probs = torch.ops.ifseg.seg_predict_slide_views(*args, h, w, softmax, False, False)
        assert torch.equal(lab, rl) and conf.numel() == 0 and probs.numel() == 0
    # non-contiguous scores are copied, not refused
    st = scores[0].transpose(0, 1).contiguous().transpose(0, 1)
    assert not st.is_contiguous()
    assert torch.equal(torch.ops.ifseg.seg_predict_slide_views([st, scores[1]], *args[1:], h, w, False, False, False)[0], rl)
    gt = SCO.ground_truth((2, h, w), n, True, 1, torch.uint8).to(dev)
    ra, rt, _, _, _ = hip.seg_score_slide_views(vd, crop, stride, gt, False)
    areas, tally, lab, conf, probs = torch.ops.ifseg.seg_score_slide_views(*args, gt, False, True, True, False, False)
    assert torch.equal(areas, ra) and torch.equal(tally, rt) and torch.equal(lab, rl) and conf.numel() == 0 and probs.numel() == 0
    utils = ("test_schema", "test_autograd_registration", "test_faketensor")
    small = ([s[:1, :, :, :5].contiguous() for s in scores], *args[1:])
    torch.library.opcheck(torch.ops.ifseg.seg_predict_slide_views, (*small, 7, 9, True, True, True), test_utils=utils)
    torch.library.opcheck(torch.ops.ifseg.seg_predict_slide_views, (*small, 7, 9, False, False, False), test_utils=utils)
    torch.library.opcheck(torch.ops.ifseg.seg_score_slide_views, (*small, gt[:1, :7, :9].contiguous(), True, True, True, True, False),
                          test_utils=utils)
    # on a side stream the ops follow PyTorch's current stream
    st2 = torch.cuda.Stream()
    st2.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st2):
        l3 = torch.ops.ifseg.seg_predict_slide_views(*args, h, w, False, False, False)[0]
        a3 = torch.ops.ifseg.seg_score_slide_views(*args, gt, False, True, False, False, False)[0]
    st2.synchronize()
    assert torch.equal(l3, rl) and torch.equal(a3, ra)


# ------------------------------------------------------------------------------------------------- end to end
RAW_SHAPES = [(64, 160), (160, 64), (64, 64)]                  # the three raw shapes of test_slide_gpu.py, at P = 128
SCALES = (0.5, 1.0, 1.5)


@pytest.fixture(scope="module")
def e2e():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ifseg_amd.models.segofa import SegOFAModel, make_config
    from ifseg_amd.predict import Segmenter
    dev = torch.device("cuda:0")
    ocfg, sd, img, src = PC.e2e_fixture()
    m = SegOFAModel(make_config("segofa_tiny", embed_dim=ocfg.embed_dim, ffn_dim=ocfg.ffn_dim, heads=ocfg.heads,
                                enc_layers=ocfg.enc_layers, dec_layers=ocfg.dec_layers, resnet_layers=ocfg.resnet_layers,
                                num_seg_tokens=ocfg.num_seg_tokens, vocab_size=ocfg.vocab_size,
                                patch_image_size=ocfg.patch_image_size, orig_patch_image_size=ocfg.orig_patch_image_size))
    torch.nn.Module.load_state_dict(m, sd, strict=False)
    m.to(dev).eval()
    base = ((img * 0.5 + 0.5) * 255).round().clamp(0, 255)
    raw = [torch.nn.functional.interpolate(base[k % 2:k % 2 + 1], size=s, mode="bilinear", align_corners=False)[0]
           .round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous() for k, s in enumerate(RAW_SHAPES)]
    mk = lambda **kw: Segmenter(m, category_token_ids=PC.E2E_NAMES, prompt_ids=PC.E2E_PROMPT, slide_views=True, **kw)
    return m, raw, ocfg, mk


@pytest.mark.parametrize("upsample", ["logits", "probs"])
def test_segment_raw_slide_views_end_to_end(e2e, upsample):
    from ifseg_amd import hip
    from ifseg_amd.imageio import eval_size, view_list
    m, raw, ocfg, mk = e2e
    dev = torch.device("cuda:0")
    n, P = ocfg.num_seg_tokens, ocfg.patch_image_size
    crop, stride = P, 2 * P // 3
    seg = mk(upsample=upsample)
    softmax = upsample == "logits"
    outs = seg.segment_raw(raw, slide=True, scales=SCALES, flip=True, return_conf=True, return_probs=True)
    assert isinstance(outs, list) and len(outs) == 3
    for r, o in zip(raw, outs):
        H, W = r.shape[:2]
        assert o.labels.shape == (H, W) and o.labels.dtype == torch.uint8 and o.labels.is_cuda
        assert o.conf.shape == (H, W) and o.probs.shape == (n, H, W)
        # the specification, fed with the Segmenter's own patch scores of the loaded windows
        views = []
        for ratio, flipped in view_list(SCALES, True):
            oh, ow = eval_size(H, W, P, ratio)
            x = hip.image_load_windows(r[None].to(dev), oh, ow, crop, stride, flip=flipped)
            scores, hp, wp = seg.patch_scores(x)
            views.append((scores[None].contiguous(), hp, wp, oh, ow, flipped))
        ref = C.Reference(views, crop, stride, H, W, softmax)
        d = (o.probs[None].cpu().double() - ref.probs).abs().max().item()
        print(upsample, (H, W), "e = %.2e, undecided %.3f %%, max |d| / e = %.3f" % (ref.e, 100 * ref.undecided_share, d / ref.e))
        ref.check(o.labels[None], o.conf[None], o.probs[None], what=(upsample, H, W))
        if softmax:
            assert (o.probs.sum(0) - 1).abs().max().item() < 1e-5
    # labels only; a list with repeated shapes batches and keeps the order
    again = seg.segment_raw([raw[2], raw[0], raw[2], raw[1]], max_batch=3, slide=True, scales=SCALES, flip=True)
    assert all(a.conf is None and a.probs is None for a in again)
    for a, k in zip(again, (2, 0, 2, 1)):
        assert torch.equal(a.labels, outs[k].labels)
    # the default Segmenter still refuses
    from ifseg_amd.predict import Segmenter
    plain = Segmenter(m, category_token_ids=PC.E2E_NAMES, prompt_ids=PC.E2E_PROMPT)
    with pytest.raises(ValueError, match="slide takes a single view"):
        plain.segment_raw(raw, slide=True, scales=SCALES, flip=True)


def test_evaluate_raw_slide_views_end_to_end(e2e):
    from ifseg_amd.predict import SegmentationScore, areas_reference
    m, raw, ocfg, mk = e2e
    n = ocfg.num_seg_tokens
    gts = [SCO.ground_truth(tuple(r.shape[:2]), n, True, k, (torch.uint8, torch.int16)[k % 2]) for k, r in enumerate(raw)]
    kw = dict(slide=True, scales=SCALES, flip=True)
    for upsample in ("logits", "probs"):
        seg = mk(upsample=upsample)
        outs = seg.segment_raw(raw, **kw)
        score, labels = seg.evaluate_raw(raw, gts, return_labels=True, **kw)
        want_a, want_t = torch.zeros(3, n, dtype=torch.int64), torch.zeros(2, dtype=torch.int64)
        for o, lab, gt in zip(outs, labels, gts):
            assert torch.equal(lab, o.labels)
            a, t = areas_reference(lab.cpu(), gt, n, True)
            want_a += a
            want_t += t
        assert torch.equal(score.areas.cpu(), want_a) and torch.equal(score.tally.cpu(), want_t)
        ref = SegmentationScore(n, torch.device("cpu"), want_a.clone(), want_t.clone())
        assert score.summary() == ref.summary()
    # counters only, accumulated into an existing score; the task passes the keyword through
    into = SegmentationScore(n, score.areas.device)
    assert seg.evaluate_raw(raw, gts, into=into, **kw) is into
    seg.evaluate_raw(raw, gts, into=into, **kw)
    assert torch.equal(into.areas, 2 * score.areas) and torch.equal(into.tally, 2 * score.tally)
    from ifseg_amd.tasks.mm_tasks.segmentation import SegmentationTask
    task = SegmentationTask.__new__(SegmentationTask)
    seen = {}
    task.build_segmenter = lambda model, **k: (seen.update(k), mk(**{a: b for a, b in k.items() if a != "slide_views"}))[1]
    via = task.evaluate_raw(m, raw, gts, slide_views=True, upsample="probs", **kw)
    assert seen == {"slide_views": True, "upsample": "probs"}
    assert torch.equal(via.areas, score.areas) and torch.equal(via.tally, score.tally)
    # with the CRF on, the CRF's argmax is what is scored
    crf = mk(crf_iters=1)
    score, labels = crf.evaluate_raw(raw[:2], gts[:2], return_labels=True, **kw)
    want_a.zero_(), want_t.zero_()
    for lab, gt in zip(labels, gts):
        a, t = areas_reference(lab.cpu(), gt, n, True)
        want_a += a
        want_t += t
    assert torch.equal(score.areas.cpu(), want_a) and torch.equal(score.tally.cpu(), want_t)


def test_no_resized_bias_entry_when_every_window_runs_at_the_trained_grid(e2e):
    """crop = P and every scaled short side >= P: one network size for the whole call"""
    m, raw, ocfg, mk = e2e
    seg = mk(upsample="logits")
    seg.segment_raw(raw[2], slide=True)                        # the engine exists and has met the trained grid
    m.engine._rb_cache.clear()                                 # (the model is the module's: drop what earlier tests left)
    seg.segment_raw(raw[2], slide=True)
    before = dict(m.engine._rb_cache)
    outs = seg.segment_raw(raw, slide=True, scales=(1.0, 1.5), flip=True)
    assert len(outs) == 3 and dict(m.engine._rb_cache).keys() == before.keys()
    # a ratio below 1 has a short side below the crop: another window size, and an entry
    seg.segment_raw(raw[0], slide=True, scales=(0.5,), flip=False)
    assert len(m.engine._rb_cache) > len(before)
