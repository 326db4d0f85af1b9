"""GPU: hip.seg_predict_views (csrc/predict.hip) against the CPU specification `upsample_views_reference`,
torch.ops.ifseg.seg_predict_views through the dispatcher, and Segmenter.segment_raw(scales, flip) end to end on the segofa_tiny
fixture.  The comparison rule is in tests/_predict_views_cases.py.

Which path of the kernel a case takes: views get LDS in view order while the staging buffer lasts, per 16-class chunk.  The
exact family and the K = 3 / K = 5 general cases fit it whole; the K = 12 cases at 33 x 31 (one tile under twelve whole grids,
about 90 KiB) stage their first views and read the rest from global memory in the same launch; `staging_bytes=0` sends every
view down the direct-global path; DIRECT_CASE (a 40 x 40 grid under one tile) takes it on its own."""
import ctypes

import pytest
import torch

import _predict_cases as PC
import _predict_views_cases as C

pytestmark = pytest.mark.gpu

PATHS = {"staged": None, "direct": 0}          # hip.seg_predict_views(staging_bytes=...)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ifseg_amd.ops  # noqa: F401
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------- exact family
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("K", C.EXACT_KS)
@pytest.mark.parametrize("shape", C.EXACT_SHAPES)
def test_exact_family_bit_for_bit(shape, K, path):
    from ifseg_amd import hip
    from ifseg_amd.predict import upsample_views_reference
    dev = _dev()
    B, gh, gw, n = shape
    h, w = 16 * gh, 16 * gw
    views = C.exact_views(shape, K)
    rl, rc, rp = upsample_views_reference(views, h, w, torch.float32)
    vd = C.to_device(views, dev)
    lab, conf, probs = hip.seg_predict_views(vd, h, w, conf=True, probs=True, staging_bytes=PATHS[path])
    assert lab.dtype == (torch.int16 if n > 256 else torch.uint8) and lab.shape == (B, h, w)
    assert torch.equal(lab.cpu().long(), rl)
    assert torch.equal(conf.cpu(), rc)
    assert torch.equal(probs.cpu(), rp)
    # every combination of outputs gives the same labels
    for kw in ({}, {"conf": True}, {"probs": True}):
        l2, c2, p2 = hip.seg_predict_views(vd, h, w, staging_bytes=PATHS[path], **kw)
        assert torch.equal(l2, lab) and (c2 is None) == ("conf" not in kw) and (p2 is None) == ("probs" not in kw)
        assert c2 is None or torch.equal(c2, conf)
        assert p2 is None or torch.equal(p2, probs)


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("shape", [PC.GENERAL_SHAPES[1], PC.GENERAL_SHAPES[2]])
def test_one_unflipped_view_is_seg_predict_bit_for_bit(shape, path):
    from ifseg_amd import hip
    dev = _dev()
    hp, wp, n, h, w = shape
    for softmaxed in (False, True):
        s = PC.general_scores(shape, 3, softmaxed, batch=2).to(dev)
        a = hip.seg_predict_views([(s, hp, wp, False)], h, w, conf=True, probs=True, staging_bytes=PATHS[path])
        b = hip.seg_predict(s, hp, wp, h, w, conf=True, probs=True, staging_bytes=PATHS[path])
        assert torch.equal(a[0], b[0]) and torch.equal(_bits(a[1]), _bits(b[1])) and torch.equal(_bits(a[2]), _bits(b[2]))


@pytest.mark.parametrize("path", list(PATHS))
def test_one_flipped_view_is_seg_predict_on_the_reversed_grid(path):
    from ifseg_amd import hip
    dev = _dev()
    hp, wp, n, h, w = 4, 6, 150, 37, 91
    s = PC.general_scores((hp, wp, n, h, w), 5, True, batch=2).to(dev)
    rev = s.view(2, hp, wp, n).flip(2).reshape(2, hp * wp, n).contiguous()
    a = hip.seg_predict_views([(s, hp, wp, True)], h, w, conf=True, probs=True, staging_bytes=PATHS[path])
    b = hip.seg_predict(rev, hp, wp, h, w, conf=True, probs=True, staging_bytes=PATHS[path])
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert not torch.equal(a[2], hip.seg_predict(s, hp, wp, h, w, probs=True)[2])


# ------------------------------------------------------------------------------------------------- general family
@pytest.mark.parametrize("softmaxed", [False, True], ids=["raw", "softmax"])
@pytest.mark.parametrize("case", C.GENERAL_CASES)
def test_general_family_both_paths(case, softmaxed):
    from ifseg_amd import hip
    dev = _dev()
    K, n, h, w = case
    for seed in C.SEEDS:
        views = C.general_views(K, n, seed, softmaxed)
        ref = C.reference(("general", K, n, h, w, softmaxed, seed), views, h, w)
        print(case, seed, "e = %.2e, undecided %.3f %%" % (ref.e, 100 * ref.undecided_share))
        vd = C.to_device(views, dev)
        for path, sb in PATHS.items():
            lab, conf, probs = hip.seg_predict_views(vd, h, w, conf=True, probs=True, staging_bytes=sb)
            ref.check(lab, conf, probs, what=(case, seed, path))
            assert torch.equal(hip.seg_predict_views(vd, h, w, staging_bytes=sb)[0], lab)


def test_footprints_beyond_the_staging_buffer():
    """strong downscaling with many classes: the 40 x 40 view fits no staging buffer and reads global memory, the 20 x 20 view
    beside it is staged; a batch of 2"""
    from ifseg_amd import hip
    dev = _dev()
    K, n, h, w, grids = C.DIRECT_CASE
    views = C.general_views(K, n, 1, False, batch=2, grids=grids)
    ref = C.reference(("direct",), views, h, w)
    lab, conf, probs = hip.seg_predict_views(C.to_device(views, dev), h, w, conf=True, probs=True)
    assert lab.dtype == torch.int16
    ref.check(lab, conf, probs, what="direct")


def test_batch_and_unaligned_rows():
    """B = 3 with an odd width: the rows of images 1 and 2 start at every alignment of the wide label / conf stores"""
    from ifseg_amd import hip
    dev = _dev()
    B, K, n, h, w = C.BATCH_CASE
    views = C.general_views(K, n, 11, True, batch=B)
    ref = C.reference(("batch",), views, h, w)
    vd = C.to_device(views, dev)
    lab, conf, probs = hip.seg_predict_views(vd, h, w, conf=True, probs=True)
    ref.check(lab, conf, probs, what="batch 3")
    # canaries around labels and conf, written at an offset of 32 bytes: nothing lands outside [B, h, w]
    N = B * h * w
    lbuf = torch.full((N + 64,), 201, dtype=torch.uint8, device=dev)
    cbuf = torch.full((N + 64,), 7.0, device=dev)
    assert lbuf[32:].data_ptr() % 16 == 0 and cbuf[32:].data_ptr() % 16 == 0
    table = (hip._PredictView * K)(*[hip._PredictView(s.data_ptr(), hp, wp, int(f)) for s, hp, wp, f in vd])
    i, p = ctypes.c_int, lambda t: ctypes.c_void_p(t.data_ptr())
    rc = hip.lib().ifseg_seg_predict_views(table, i(K), i(B), i(n), i(h), i(w), p(lbuf[32:]), i(1), p(cbuf[32:]), None,
                                           ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    assert lbuf[:32].eq(201).all() and lbuf[32 + N:].eq(201).all() and cbuf[:32].eq(7).all() and cbuf[32 + N:].eq(7).all()
    assert torch.equal(lbuf[32:32 + N].view(B, h, w), lab) and torch.equal(cbuf[32:32 + N].view(B, h, w), conf)


def test_entry_point_refusals():
    """the C entry refuses what the contract excludes, whatever the binding let through; nothing is launched"""
    from ifseg_amd import hip
    dev = _dev()
    lib = hip.lib()
    s = torch.zeros(1, 4, 513, device=dev)
    out = torch.full((64,), 77, dtype=torch.int16, device=dev)
    i, p = ctypes.c_int, lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else None)
    one = lambda ptr: hip._PredictView(ptr, 2, 2, 0)

    def call(K=1, n=5, h=4, w=4, lb=2, table=None, labels=None, B=1):
        table = (hip._PredictView * 17)(*[one(s.data_ptr())] * 17) if table is None else table
        return lib.ifseg_seg_predict_views(table, i(K), i(B), i(n), i(h), i(w), p(out) if labels is None else labels, i(lb), None,
                                           None, None)

    BAD_SHAPE, BAD_ARG = -2, -3
    assert call(K=0) == BAD_ARG and call(K=17) == BAD_ARG and call(K=-1) == BAD_ARG
    assert call(table=ctypes.POINTER(hip._PredictView)()) == BAD_ARG                         # a null table
    assert call(K=2, table=(hip._PredictView * 2)(one(s.data_ptr()), one(None))) == BAD_ARG   # a view without scores
    assert call(n=513) == BAD_ARG and call(n=0) == BAD_ARG
    assert call(n=300, lb=1) == BAD_ARG and call(lb=4) == BAD_ARG                            # uint8 labels with n > 256
    assert call(labels=ctypes.c_void_p(out.data_ptr() + 2)) == BAD_ARG                       # misaligned labels
    assert call(h=0) == BAD_SHAPE and call(w=-1) == BAD_SHAPE and call(B=0) == BAD_SHAPE
    assert call(h=2 ** 16, w=2 ** 15) == BAD_SHAPE                                           # B h w >= 2^31
    assert call(table=(hip._PredictView * 1)(hip._PredictView(s.data_ptr(), 0, 2, 0))) == BAD_SHAPE
    torch.cuda.synchronize()
    assert out.eq(77).all()                                                                  # no launch so far
    assert call(K=16, n=300) == 0                                                            # the limits themselves are fine
    torch.cuda.synchronize()
    assert out[:16].eq(0).all() and out[16:].eq(77).all()


# ------------------------------------------------------------------------------------------------- the op
def test_op_matches_binding_and_opcheck():
    from ifseg_amd import hip
    dev = _dev()
    n, h, w = 257, 40, 23
    views = C.to_device(C.general_views(3, n, 3, False, batch=2, grids=[(2, 3), (4, 6), (3, 2)]), dev)
    args = ([v[0] for v in views], [v[1] for v in views], [v[2] for v in views], [v[3] for v in views], h, w)
    lab, conf, probs = torch.ops.ifseg.seg_predict_views(*args, True, True)
    rl, rc, rp = hip.seg_predict_views(views, h, w, conf=True, probs=True)
    assert lab.dtype == torch.int16 and torch.equal(lab, rl) and torch.equal(conf, rc) and torch.equal(probs, rp)
    lab, conf, probs = torch.ops.ifseg.seg_predict_views(*args, False, False)
    assert torch.equal(lab, rl) and conf.numel() == 0 and probs.numel() == 0
    # a non-contiguous view is copied, not refused
    st = [s.transpose(0, 1).contiguous().transpose(0, 1) for s in args[0]]
    assert not st[0].is_contiguous()
    assert torch.equal(torch.ops.ifseg.seg_predict_views(st, *args[1:], False, False)[0], rl)
    utils = ("test_schema", "test_autograd_registration", "test_faketensor")
    torch.library.opcheck(torch.ops.ifseg.seg_predict_views, (*args, True, True), test_utils=utils)
    small = ([s[:1, :, :5].contiguous() for s in args[0]], *args[1:4], 7, 9)
    torch.library.opcheck(torch.ops.ifseg.seg_predict_views, (*small, False, False), test_utils=utils)
    # on a side stream the op follows PyTorch's current stream
    st2 = torch.cuda.Stream()
    st2.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st2):
        l3 = torch.ops.ifseg.seg_predict_views(*args, False, False)[0]
    st2.synchronize()
    assert torch.equal(l3, rl)


# ------------------------------------------------------------------------------------------------- end to end
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
    # raw photographs: the fixture's own images, resized on the host to the three source shapes and quantised
    base = ((img * 0.5 + 0.5) * 255).round().clamp(0, 255)
    raw = [torch.nn.functional.interpolate(base[k % 2:k % 2 + 1], size=s, mode="bilinear", align_corners=False)[0]
           .round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous() for k, s in enumerate([(60, 90), (90, 60), (64, 64)])]
    mk = lambda **kw: Segmenter(m, category_token_ids=PC.E2E_NAMES, prompt_ids=PC.E2E_PROMPT, **kw)
    return m, raw, ocfg, mk


SCALES = (0.5, 1.0, 1.5)


def _views_of(seg, r, P, dev):
    """the per-view scores of one raw image, one forward per view"""
    from ifseg_amd import hip
    from ifseg_amd.imageio import eval_size
    out = []
    for ratio in SCALES:
        oh, ow = eval_size(r.shape[0], r.shape[1], P, ratio)
        x = hip.image_load(r[None].to(dev), oh, ow)
        for flip in (False, True):
            scores, hp, wp = seg.patch_scores(x.flip(-1) if flip else x)
            out.append((scores, hp, wp, flip))
    return out


def test_segment_raw_multi_scale_flip_end_to_end(e2e):
    from ifseg_amd import hip
    m, raw, ocfg, mk = e2e
    dev = torch.device("cuda:0")
    n = ocfg.num_seg_tokens
    seg = mk()
    outs = seg.segment_raw(raw, scales=SCALES, flip=True, return_conf=True, return_probs=True)
    assert isinstance(outs, list) and len(outs) == 3
    for r, o in zip(raw, outs):
        H, W = r.shape[:2]
        assert o.labels.shape == (H, W) and o.labels.dtype == torch.uint8 and o.labels.is_cuda
        assert o.conf.shape == (H, W) and o.probs.shape == (n, H, W)
        views = _views_of(seg, r, ocfg.patch_image_size, dev)
        assert len(views) == 6 and len({(hp, wp) for _, hp, wp, _ in views}) == 3
        lab, conf, probs = hip.seg_predict_views(views, H, W, conf=True, probs=True)
        assert torch.equal(o.labels, lab[0]) and torch.equal(o.conf, conf[0]) and torch.equal(o.probs, probs[0])
        ref = C.Reference(views, H, W)
        print((H, W), "e = %.2e, undecided %.3f %%" % (ref.e, 100 * ref.undecided_share))
        ref.check(o.labels[None], o.conf[None], o.probs[None], what=(H, W))
    # the default arguments are today's single-view path
    plain = seg.segment_raw(raw, return_conf=True, return_probs=True)
    same = seg.segment_raw(raw, scales=(1.0,), flip=False, return_conf=True, return_probs=True)
    for a, b in zip(plain, same):
        assert torch.equal(a.labels, b.labels) and torch.equal(a.conf, b.conf) and torch.equal(a.probs, b.probs)
    # a flip-only ensemble is another result than the single view
    both = seg.segment_raw(raw, flip=True, return_probs=True)
    assert any(not torch.equal(a.probs, b.probs) for a, b in zip(plain, both))
    # a list with repeated shapes batches and keeps the order; labels only
    again = seg.segment_raw([raw[2], raw[0], raw[2], raw[0]], max_batch=3, scales=(0.5, 1.0), flip=True)
    assert [tuple(a.labels.shape) for a in again] == [(64, 64), (60, 90), (64, 64), (60, 90)]
    assert all(a.conf is None and a.probs is None for a in again)
    assert torch.equal(again[0].labels, again[2].labels) and torch.equal(again[1].labels, again[3].labels)
    one = seg.segment_raw(raw[0].to(dev), scales=SCALES, flip=True)
    assert len(one) == 1 and torch.equal(one[0].labels, outs[0].labels)


def test_segment_raw_multi_scale_with_smoothing_and_crf(e2e):
    m, raw, ocfg, mk = e2e
    n = ocfg.num_seg_tokens
    for kw in ({"smooth_iters": 2}, {"crf_iters": 1}):
        outs = mk(**kw).segment_raw(raw, scales=(0.5, 1.0), flip=True, return_conf=True, return_probs=True)
        for r, o in zip(raw, outs):
            H, W = r.shape[:2]
            assert o.labels.shape == (H, W) and o.conf.shape == (H, W) and o.probs.shape == (n, H, W)
            assert torch.isfinite(o.probs).all() and torch.isfinite(o.conf).all()
            assert torch.equal(o.labels.long(), o.probs.argmax(0))
