"""GPU: sliding-window inference -- hip.seg_predict_windows / hip.seg_score_windows (csrc/predict.hip) against the CPU
specification `slide_reference`, hip.image_load_windows (csrc/imgload.hip) against slices of hip.image_load, the three ops
through the dispatcher, and Segmenter.segment_raw / evaluate_raw(slide=...) end to end on the segofa_tiny fixture.  The
comparison rule is in tests/_slide_cases.py.

Data paths: the merge kernel stages the patches of every window under a tile in LDS, or reads global memory where they do not
fit; `staging_bytes=0` sends every tile down the second path.  image_load_windows has image_load's two paths and switch."""
import ctypes

import pytest
import torch

import _predict_cases as PC
import _score_cases as SC
import _slide_cases as C

pytestmark = pytest.mark.gpu

PATHS = {"staged": None, "direct": 0}          # staging_bytes=...
BAD_SHAPE, BAD_ARG = -2, -3


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ifseg_amd.ops  # noqa: F401
    return torch.device("cuda:0")


def _bits(t):
    return t.view(torch.int32)


# ------------------------------------------------------------------------------------------------- exact family
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", list(C.EXACT_CASES))
def test_exact_family_bit_for_bit(name, path):
    from ifseg_amd import hip
    from ifseg_amd.predict import slide_reference
    dev = _dev()
    B, hpw, wpw, n, oh, ow, crop, stride, h, w = C.EXACT_CASES[name]
    geo = (hpw, wpw, oh, ow, crop, stride, h, w)
    s = C.exact_scores(name)
    rl, rc, rp = slide_reference(s, *geo, torch.float32)
    sd = s.to(dev)
    lab, conf, probs = hip.seg_predict_windows(sd, *geo, conf=True, probs=True, staging_bytes=PATHS[path])
    assert lab.dtype == (torch.int16 if n > 256 else torch.uint8) and lab.shape == (B, h, w)
    assert torch.equal(lab.cpu().long(), rl)
    assert torch.equal(conf.cpu(), rc)
    assert torch.equal(probs.cpu(), rp)
    # every combination of outputs gives the same labels
    for kw in ({}, {"conf": True}, {"probs": True}):
        l2, c2, p2 = hip.seg_predict_windows(sd, *geo, staging_bytes=PATHS[path], **kw)
        assert torch.equal(l2, lab) and (c2 is None) == ("conf" not in kw) and (p2 is None) == ("probs" not in kw)
        assert c2 is None or torch.equal(c2, conf)
        assert p2 is None or torch.equal(p2, probs)


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("shape", C.ONE_WINDOW_CASES)
def test_one_covering_window_is_seg_predict_bit_for_bit(shape, path):
    from ifseg_amd import hip
    dev = _dev()
    hp, wp, n, h, w = shape
    for softmaxed in (False, True):
        s = PC.general_scores(shape, 3, softmaxed, batch=2).to(dev)
        for crop, stride in (((h, w), (h, w)), ((h + 3, 2 * w), (h, 1))):     # the crop is the image, or larger than it
            a = hip.seg_predict_windows(s[:, None].contiguous(), hp, wp, h, w, crop, stride, h, w, conf=True, probs=True,
                                        staging_bytes=PATHS[path])
            b = hip.seg_predict(s, hp, wp, h, w, conf=True, probs=True, staging_bytes=PATHS[path])
            assert torch.equal(a[0], b[0]) and torch.equal(_bits(a[1]), _bits(b[1])) and torch.equal(_bits(a[2]), _bits(b[2]))


# ------------------------------------------------------------------------------------------------- general family
@pytest.mark.parametrize("softmaxed", [False, True], ids=["raw", "softmax"])
@pytest.mark.parametrize("case", C.GENERAL_CASES, ids=[str(i) for i in range(len(C.GENERAL_CASES))])
def test_general_family_both_paths(case, softmaxed):
    from ifseg_amd import hip
    dev = _dev()
    geo = case[:2] + case[3:]
    for seed in C.SEEDS:
        s = C.general_scores(case, seed, softmaxed)
        ref = C.reference(("general", case, softmaxed, seed), s, *geo)
        print(case, seed, "e = %.2e, undecided %.3f %%" % (ref.e, 100 * ref.undecided_share))
        sd = s.to(dev)
        for path, sb in PATHS.items():
            lab, conf, probs = hip.seg_predict_windows(sd, *geo, conf=True, probs=True, staging_bytes=sb)
            ref.check(lab, conf, probs, what=(case, seed, path))
            assert torch.equal(hip.seg_predict_windows(sd, *geo, staging_bytes=sb)[0], lab)


def test_batch_and_unaligned_rows():
    """B = 3 with an odd width: the rows of images 1 and 2 start at every alignment of the wide label / conf stores"""
    from ifseg_amd import hip
    dev = _dev()
    B, hpw, wpw, n, oh, ow, crop, stride, h, w = C.BATCH_CASE
    case = C.BATCH_CASE[1:]
    s = C.general_scores(case, 11, True, batch=B)
    ref = C.reference(("batch",), s, hpw, wpw, oh, ow, crop, stride, h, w)
    sd = s.to(dev)
    lab, conf, probs = hip.seg_predict_windows(sd, hpw, wpw, oh, ow, crop, stride, h, w, conf=True, probs=True)
    ref.check(lab, conf, probs, what="batch 3")
    # canaries around labels and conf, written at an offset of 32 bytes: nothing lands outside [B, h, w]
    N = B * h * w
    lbuf = torch.full((N + 64,), 201, dtype=torch.uint8, device=dev)
    cbuf = torch.full((N + 64,), 7.0, device=dev)
    assert lbuf[32:].data_ptr() % 16 == 0 and cbuf[32:].data_ptr() % 16 == 0
    i, p = ctypes.c_int, lambda t: ctypes.c_void_p(t.data_ptr())
    rc = hip.lib().ifseg_seg_predict_windows(p(sd), i(B), i(hpw), i(wpw), i(n), i(oh), i(ow), i(crop), i(crop), i(stride), i(stride),
                                             i(h), i(w), p(lbuf[32:]), i(1), p(cbuf[32:]), None,
                                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    assert lbuf[:32].eq(201).all() and lbuf[32 + N:].eq(201).all() and cbuf[:32].eq(7).all() and cbuf[32 + N:].eq(7).all()
    assert torch.equal(lbuf[32:32 + N].view(B, h, w), lab) and torch.equal(cbuf[32:32 + N].view(B, h, w), conf)


def test_entry_point_refusals():
    """the C entry refuses what the contract excludes, whatever the binding let through; nothing is launched"""
    from ifseg_amd import hip
    dev = _dev()
    lib = hip.lib()
    s = torch.zeros(1, 64, 1, 513, device=dev)
    out = torch.full((64,), 77, dtype=torch.int16, device=dev)
    i, p = ctypes.c_int, lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else None)

    def call(B=1, hpw=1, wpw=1, n=5, oh=8, ow=8, ch=4, cw=4, sh=4, sw=4, h=4, w=4, lb=2, labels=None, scores=s):
        return lib.ifseg_seg_predict_windows(p(scores), i(B), i(hpw), i(wpw), i(n), i(oh), i(ow), i(ch), i(cw), i(sh), i(sw), i(h), i(w),
                                             p(out) if labels is None else labels, i(lb), None, None, None)

    assert call(scores=None) == BAD_ARG
    assert call(n=513) == BAD_ARG and call(n=0) == BAD_ARG
    assert call(n=300, lb=1) == BAD_ARG and call(lb=4) == BAD_ARG                            # uint8 labels with n > 256
    assert call(labels=ctypes.c_void_p(out.data_ptr() + 2)) == BAD_ARG                       # misaligned labels
    assert call(labels=ctypes.c_void_p(None)) == BAD_ARG
    assert call(h=0) == BAD_SHAPE and call(w=-1) == BAD_SHAPE and call(B=0) == BAD_SHAPE
    assert call(hpw=0) == BAD_SHAPE and call(oh=0) == BAD_SHAPE and call(ow=-3) == BAD_SHAPE
    assert call(h=2 ** 16, w=2 ** 15) == BAD_SHAPE                                           # B h w >= 2^31
    assert call(sh=5) == BAD_SHAPE and call(sw=5) == BAD_SHAPE                               # stride > crop
    assert call(sh=0) == BAD_SHAPE and call(cw=0) == BAD_SHAPE and call(ch=-1) == BAD_SHAPE
    assert call(oh=9, ch=1, cw=1, sh=1, sw=1) == BAD_SHAPE                                   # 9 x 8 = 72 windows
    assert call(oh=64, ow=64, ch=8, cw=8, sh=8, sw=8, hpw=256, wpw=256) == BAD_SHAPE         # Nw hpw wpw >= 2^22
    # the scoring entry: the same, and its own
    gt = torch.zeros(16, dtype=torch.uint8, device=dev)
    cnt = torch.full((3 * 5 + 2,), 5, dtype=torch.int64, device=dev)

    def score(n=5, sh=4, gtp=gt, gb=1, areas=cnt, tally=cnt[15:]):
        return lib.ifseg_seg_score_windows(p(s), i(1), i(1), i(1), i(n), i(8), i(8), i(4), i(4), i(sh), i(4), i(4), i(4), p(out), i(2),
                                           None, None, p(gtp), i(gb), i(1), p(areas), p(tally), None)

    assert score(n=513) == BAD_ARG and score(sh=5) == BAD_SHAPE
    assert score(gtp=None) == BAD_ARG and score(gb=3) == BAD_ARG and score(areas=None) == BAD_ARG
    torch.cuda.synchronize()
    assert out.eq(77).all() and cnt.eq(5).all()                                              # no launch so far
    # the limits themselves are fine: 64 windows, 300 classes, int16 labels
    assert call(n=300, ch=1, cw=1, sh=1, sw=1) == 0
    torch.cuda.synchronize()
    assert out[:16].eq(0).all() and out[16:].eq(77).all()
    assert score() == 0                                                                       # raw 0 everywhere: nothing scored
    torch.cuda.synchronize()
    assert cnt.eq(5).all()


# ------------------------------------------------------------------------------------------------- the window batch
IMAGE_CASES = [((2, 50, 131), (64, 168), 64, 43),              # upscaling; windows at x = 0, 43, 86, 104
               ((1, 200, 517), (64, 168), 64, 43),             # a downscaling source
               ((1, 90, 70), (100, 75), (48, 64), (26, 11)),   # windows on both axes, a non-square crop, odd width
               ((1, 33, 40), (40, 90), 64, 30)]                # a short axis: windows of 40 x 64


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("case", IMAGE_CASES, ids=[str(i) for i in range(len(IMAGE_CASES))])
def test_image_load_windows_is_slices_of_image_load(case, path):
    from ifseg_amd import hip
    from ifseg_amd.imageio import IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD, slide_windows
    dev = _dev()
    (B, H0, W0), (oh, ow), crop, stride = case
    img = torch.randint(0, 256, (B, H0, W0, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(H0)).to(dev)
    ys, xs, ch, cw = slide_windows(oh, ow, crop, stride)
    nw = len(ys) * len(xs)
    for dtype in (torch.float32, torch.bfloat16):
        for kw in ({}, {"mean": IMAGENET_DEFAULT_MEAN, "std": IMAGENET_DEFAULT_STD, "reverse_channels": True}):
            full = hip.image_load(img, oh, ow, dtype=dtype, staging_bytes=PATHS[path], **kw)
            wins = hip.image_load_windows(img, oh, ow, crop, stride, dtype=dtype, staging_bytes=PATHS[path], **kw)
            assert wins.shape == (B * nw, 3, ch, cw) and wins.dtype == dtype and wins.is_contiguous()
            want = torch.stack([full[:, :, y:y + ch, x:x + cw] for y in ys for x in xs], 1).reshape(B * nw, 3, ch, cw)
            assert torch.equal(wins.view(torch.int32 if dtype == torch.float32 else torch.int16),
                               want.contiguous().view(torch.int32 if dtype == torch.float32 else torch.int16)), (dtype, kw)


def test_image_load_windows_entry_point_refusals():
    """nothing is launched on a refusal; the call the refusals were derived from succeeds"""
    from ifseg_amd import hip
    dev = _dev()
    out = torch.full((3 * 16,), 9.0, device=dev)
    lut = torch.zeros(3, 256, device=dev)
    small = torch.zeros(1, 4, 4, 3, dtype=torch.uint8, device=dev)
    i, p = ctypes.c_int, lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else None)

    def call(oh=4, ow=4, ch=4, cw=4, sh=4, sw=4, images=small, ob=4):
        return hip.lib().ifseg_image_load_windows(p(images), i(1), i(4), i(4), i(oh), i(ow), i(ch), i(cw), i(sh), i(sw), p(lut), i(0),
                                                  p(out), i(ob), None)

    assert call(images=None) == BAD_ARG and call(ob=3) == BAD_ARG
    assert call(sh=5) == BAD_SHAPE and call(sw=0) == BAD_SHAPE and call(ch=0) == BAD_SHAPE and call(oh=0) == BAD_SHAPE
    assert call(oh=9, ow=8, ch=1, cw=1, sh=1, sw=1) == BAD_SHAPE                              # 72 windows
    torch.cuda.synchronize()
    assert out.eq(9).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert out.eq(0).all()


# ------------------------------------------------------------------------------------------------- scoring
@pytest.mark.parametrize("raw", [True, False], ids=["raw", "ids"])
@pytest.mark.parametrize("gt_dtype", [torch.uint8, torch.int16], ids=["gt8", "gt16"])
def test_seg_score_windows_counts_its_own_labels(gt_dtype, raw):
    from ifseg_amd import hip
    from ifseg_amd.predict import areas_reference
    dev = _dev()
    for case in (C.GENERAL_CASES[2], C.GENERAL_CASES[4]):      # 5 classes / 9 windows, and 257 classes (int16 labels)
        hpw, wpw, n, oh, ow, crop, stride, h, w = case
        geo = (hpw, wpw, oh, ow, crop, stride)
        s = C.general_scores(case, 1, True, batch=2).to(dev)
        gt = SC.ground_truth((2, h, w), n, raw, n, gt_dtype)
        special = torch.tensor(SC.every_kind(n, raw, gt_dtype)).to(gt_dtype)
        gt.view(-1)[:special.numel()] = special
        gd = gt.to(dev)
        for path, sb in PATHS.items():
            plain = hip.seg_predict_windows(s, *geo, h, w, conf=True, probs=True, staging_bytes=sb)
            areas, tally, lab, conf, probs = hip.seg_score_windows(s, *geo, gd, raw, labels=True, conf=True, probs=True,
                                                                   staging_bytes=sb)
            assert all(torch.equal(a, b) for a, b in zip((lab, conf, probs), plain)), (case, path)
            ra, rt = areas_reference(lab.cpu(), gt, n, raw)
            assert torch.equal(areas.cpu(), ra) and torch.equal(tally.cpu(), rt), (case, path)
            # counters only: the same counters, nothing else written; accumulated into existing ones
            a2, t2, l2, c2, p2 = hip.seg_score_windows(s, *geo, gd, raw, staging_bytes=sb)
            assert l2 is None and c2 is None and p2 is None and torch.equal(a2, areas) and torch.equal(t2, tally)
            a3, t3 = hip.seg_score_windows(s, *geo, gd, raw, areas=a2, tally=t2, staging_bytes=sb)[:2]
            assert a3 is a2 and t3 is t2 and torch.equal(a3, 2 * areas) and torch.equal(t3, 2 * tally)


# ------------------------------------------------------------------------------------------------- the ops
def test_ops_match_bindings_and_opcheck():
    from ifseg_amd import hip
    dev = _dev()
    case = C.GENERAL_CASES[4]                                  # 257 classes: int16 labels
    hpw, wpw, n, oh, ow, crop, stride, h, w = case
    s = C.general_scores(case, 3, False, batch=2).to(dev)
    args = (s, hpw, wpw, oh, ow, list(crop), list(stride))
    rl, rc, rp = hip.seg_predict_windows(s, hpw, wpw, oh, ow, crop, stride, h, w, conf=True, probs=True)
    lab, conf, probs = torch.ops.ifseg.seg_predict_windows(*args, h, w, True, True)
    assert lab.dtype == torch.int16 and torch.equal(lab, rl) and torch.equal(conf, rc) and torch.equal(probs, rp)
    lab, conf, probs = torch.ops.ifseg.seg_predict_windows(*args, h, w, False, False)
    assert torch.equal(lab, rl) and conf.numel() == 0 and probs.numel() == 0
    # non-contiguous scores are copied, not refused
    st = s.transpose(0, 1).contiguous().transpose(0, 1)
    assert not st.is_contiguous()
    assert torch.equal(torch.ops.ifseg.seg_predict_windows(st, *args[1:], h, w, False, False)[0], rl)
    gt = SC.ground_truth((2, h, w), n, True, 1, torch.uint8).to(dev)
    ra, rt, _, _, _ = hip.seg_score_windows(s, hpw, wpw, oh, ow, crop, stride, gt)
    areas, tally, lab, conf, probs = torch.ops.ifseg.seg_score_windows(*args, gt, True, True, False, False)
    assert torch.equal(areas, ra) and torch.equal(tally, rt) and torch.equal(lab, rl) and conf.numel() == 0 and probs.numel() == 0
    img = torch.randint(0, 256, (2, 50, 131, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(4)).to(dev)
    largs = (img, 64, 168, [64, 64], [43, 43], [0.5] * 3, [0.5] * 3, False)
    for dtype in (torch.float32, torch.bfloat16):
        assert torch.equal(torch.ops.ifseg.image_load_windows(*largs, dtype), hip.image_load_windows(img, 64, 168, 64, 43, dtype=dtype))
    utils = ("test_schema", "test_autograd_registration", "test_faketensor")
    small = (s[:1, :, :, :5].contiguous(), *args[1:])
    torch.library.opcheck(torch.ops.ifseg.seg_predict_windows, (*small, 7, 9, True, True), test_utils=utils)
    torch.library.opcheck(torch.ops.ifseg.seg_predict_windows, (*small, 7, 9, False, False), test_utils=utils)
    torch.library.opcheck(torch.ops.ifseg.seg_score_windows, (*small, gt[:1, :7, :9].contiguous(), True, True, True, False), test_utils=utils)
    torch.library.opcheck(torch.ops.ifseg.image_load_windows, (*largs, torch.bfloat16), test_utils=utils)
    # on a side stream the ops follow PyTorch's current stream
    st2 = torch.cuda.Stream()
    st2.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st2):
        l3 = torch.ops.ifseg.seg_predict_windows(*args, h, w, False, False)[0]
        a3 = torch.ops.ifseg.seg_score_windows(*args, gt, True, False, False, False)[0]
        w3 = torch.ops.ifseg.image_load_windows(*largs, torch.float32)
    st2.synchronize()
    assert torch.equal(l3, rl) and torch.equal(a3, ra) and torch.equal(w3, hip.image_load_windows(img, 64, 168, 64, 43))


# ------------------------------------------------------------------------------------------------- end to end
RAW_SHAPES = [(64, 160), (160, 64), (64, 64)]                  # at P = 128: (128, 320), (320, 128), (128, 128) -> 4, 4, 1 windows


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
    mk = lambda **kw: Segmenter(m, category_token_ids=PC.E2E_NAMES, prompt_ids=PC.E2E_PROMPT, **kw)
    return m, raw, ocfg, mk


class _Grids:
    """records (hp, wp) of every `patch_scores` call of a Segmenter"""

    def __init__(self, seg):
        self.seg, self.seen, self.inner = seg, [], seg.patch_scores
        seg.patch_scores = self

    def __call__(self, x):
        scores, hp, wp = self.inner(x)
        self.seen.append((x.shape[0], hp, wp))
        return scores, hp, wp


def test_segment_raw_slide_end_to_end(e2e):
    from ifseg_amd import hip
    from ifseg_amd.imageio import eval_size, slide_windows
    m, raw, ocfg, mk = e2e
    dev = torch.device("cuda:0")
    n, P = ocfg.num_seg_tokens, ocfg.patch_image_size
    g = P // 16
    crop, stride = P, 2 * P // 3
    for upsample in ("probs", "logits"):
        seg = mk(upsample=upsample)
        plain = seg.segment_raw(raw, return_conf=True, return_probs=True)
        rec = _Grids(seg)
        outs = seg.segment_raw(raw, slide=True, return_conf=True, return_probs=True)
        # every forward ran at the fixture's own grid; nine windows in batches of at most eight
        assert rec.seen == [(8, g, g), (1, g, g)], rec.seen
        assert isinstance(outs, list) and len(outs) == 3
        for r, o, nw in zip(raw, outs, (4, 4, 1)):
            H, W = r.shape[:2]
            oh, ow = eval_size(H, W, P)
            ys, xs, ch, cw = slide_windows(oh, ow, crop, stride)
            assert len(ys) * len(xs) == nw and (ch, cw) == (P, P)
            assert o.labels.shape == (H, W) and o.labels.dtype == torch.uint8 and o.labels.is_cuda
            assert o.conf.shape == (H, W) and o.probs.shape == (n, H, W)
            # the hand composition: the window batch, the forward per window batch, the merge
            x = hip.image_load_windows(r[None].to(dev), oh, ow, crop, stride)
            assert x.shape == (nw, 3, P, P)
            scores, hp, wp = rec.inner(x)
            assert (hp, wp) == (g, g)
            lab, conf, probs = hip.seg_predict_windows(scores[None].contiguous(), hp, wp, oh, ow, crop, stride, H, W, conf=True,
                                                       probs=True)
            assert torch.equal(o.labels, lab[0]) and torch.equal(o.conf, conf[0]) and torch.equal(o.probs, probs[0])
            ref = C.Reference(scores[None], hp, wp, oh, ow, crop, stride, H, W)
            print(upsample, (H, W), "e = %.2e, undecided %.3f %%" % (ref.e, 100 * ref.undecided_share))
            ref.check(o.labels[None], o.conf[None], o.probs[None], what=(upsample, H, W))
        seg.patch_scores = rec.inner
        # slide=None is today's path, bit for bit; an explicit (crop, stride) equal to the default is the default
        same = seg.segment_raw(raw, slide=None, return_conf=True, return_probs=True)
        for a, b in zip(plain, same):
            assert torch.equal(a.labels, b.labels) and torch.equal(a.conf, b.conf) and torch.equal(a.probs, b.probs)
        again = seg.segment_raw(raw, slide=(crop, (stride, stride)), return_probs=True)
        assert all(torch.equal(a.probs, b.probs) and a.conf is None for a, b in zip(again, outs))
        # sliding is another result than the whole image where there is more than one window
        assert not torch.equal(outs[0].probs, plain[0].probs)
    # a list with repeated shapes batches and keeps the order; labels only
    seg = mk()
    outs = seg.segment_raw(raw, slide=True)
    again = seg.segment_raw([raw[2], raw[0], raw[2], raw[1], raw[0]], max_batch=3, slide=True)
    assert [tuple(a.labels.shape) for a in again] == [(64, 64), (64, 160), (64, 64), (160, 64), (64, 160)]
    assert all(a.conf is None and a.probs is None for a in again)
    for a, k in zip(again, (2, 0, 2, 1, 0)):
        assert torch.equal(a.labels, outs[k].labels)
    one = seg.segment_raw(raw[0].to(dev), slide=True)
    assert len(one) == 1 and torch.equal(one[0].labels, outs[0].labels)


def test_evaluate_raw_slide_end_to_end(e2e):
    from ifseg_amd.predict import SegmentationScore, areas_reference
    m, raw, ocfg, mk = e2e
    n = ocfg.num_seg_tokens
    gts = [SC.ground_truth(tuple(r.shape[:2]), n, True, k, (torch.uint8, torch.int16)[k % 2]) for k, r in enumerate(raw)]
    seg = mk()
    outs = seg.segment_raw(raw, slide=True)
    score, labels = seg.evaluate_raw(raw, gts, slide=True, return_labels=True)
    want_a, want_t = torch.zeros(3, n, dtype=torch.int64), torch.zeros(2, dtype=torch.int64)
    for o, lab, gt in zip(outs, labels, gts):
        assert torch.equal(lab, o.labels)
        a, t = areas_reference(lab.cpu(), gt, n, True)
        want_a += a
        want_t += t
    assert torch.equal(score.areas.cpu(), want_a) and torch.equal(score.tally.cpu(), want_t)
    # counters only, accumulated into an existing score; the task forwards the argument
    into = SegmentationScore(n, score.areas.device)
    assert seg.evaluate_raw(raw, gts, slide=True, into=into) is into
    seg.evaluate_raw(raw, gts, slide=True, into=into)
    assert torch.equal(into.areas, 2 * score.areas) and torch.equal(into.tally, 2 * score.tally)
    from ifseg_amd.tasks.mm_tasks.segmentation import SegmentationTask
    task = SegmentationTask.__new__(SegmentationTask)
    task.build_segmenter = lambda model, **kw: mk(**kw)
    via = task.evaluate_raw(m, raw, gts, slide=True)
    assert torch.equal(via.areas, score.areas) and torch.equal(via.tally, score.tally)
    # with the CRF on, the CRF's argmax is what is scored
    crf = mk(crf_iters=1)
    score, labels = crf.evaluate_raw(raw[:2], gts[:2], slide=True, return_labels=True)
    want_a.zero_(), want_t.zero_()
    for lab, gt in zip(labels, gts):
        a, t = areas_reference(lab.cpu(), gt, n, True)
        want_a += a
        want_t += t
    assert torch.equal(score.areas.cpu(), want_a) and torch.equal(score.tally.cpu(), want_t)


def test_segment_raw_slide_with_smoothing_and_crf(e2e):
    m, raw, ocfg, mk = e2e
    n = ocfg.num_seg_tokens
    for kw in ({"smooth_iters": 2}, {"crf_iters": 1}):
        outs = mk(**kw).segment_raw(raw, slide=True, return_conf=True, return_probs=True)
        for r, o in zip(raw, outs):
            H, W = r.shape[:2]
            assert o.labels.shape == (H, W) and o.conf.shape == (H, W) and o.probs.shape == (n, H, W)
            assert torch.isfinite(o.probs).all() and torch.isfinite(o.conf).all()
            assert torch.equal(o.labels.long(), o.probs.argmax(0))
