"""GPU: hip.seg_predict (csrc/predict.hip) against the CPU specification, torch.ops.ifseg.seg_predict through the dispatcher,
and ifseg_amd.predict.Segmenter end to end on the segofa_tiny fixture.  The comparison rule is in tests/_predict_cases.py.

Which path of the kernel a case takes: with the default staging buffer every tile of EXACT_SHAPES and GENERAL_SHAPES stages its
patch rows in LDS (the largest footprint, 8 x 8 patches of 15 classes under the one tile of the 5 x 3 downscale, is 5 KiB);
`staging_bytes=0` sends the same case down the direct-global path; DIRECT_SHAPES take the direct path on their own (their
footprints, 3.3 MB and 75 KiB+, exceed any staging buffer)."""
import pytest
import torch

import _predict_cases as C

pytestmark = pytest.mark.gpu

PATHS = {"staged": None, "direct": 0}          # hip.seg_predict(staging_bytes=...)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ifseg_amd.ops  # noqa: F401
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------- exact family
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("shape", C.EXACT_SHAPES)
def test_exact_family_bit_for_bit(shape, path):
    from ifseg_amd import hip
    from ifseg_amd.predict import upsample_argmax_reference
    dev = _dev()
    B, hp, wp, n = shape
    h, w = 16 * hp, 16 * wp
    s = C.exact_scores(shape)
    rl, rc, rp = upsample_argmax_reference(s, hp, wp, h, w, torch.float32)
    sd = s.to(dev)
    lab, conf, probs = hip.seg_predict(sd, hp, wp, h, w, conf=True, probs=True, staging_bytes=PATHS[path])
    assert lab.dtype == (torch.int16 if n > 256 else torch.uint8) and lab.shape == (B, h, w)
    assert torch.equal(lab.cpu().long(), rl)
    assert torch.equal(conf.cpu(), rc)
    assert torch.equal(probs.cpu(), rp)
    # every combination of outputs gives the same labels
    for kw in ({}, {"conf": True}, {"probs": True}):
        l2, c2, p2 = hip.seg_predict(sd, hp, wp, h, w, staging_bytes=PATHS[path], **kw)
        assert torch.equal(l2, lab) and (c2 is None) == ("conf" not in kw) and (p2 is None) == ("probs" not in kw)
        assert c2 is None or torch.equal(c2, conf)
        assert p2 is None or torch.equal(p2, probs)
    # the metric kernel sees the same label map: a seeded all-valid target per image
    seg0 = 1000
    g = torch.Generator().manual_seed(5)
    for b in range(B):
        t = torch.randint(0, n, (h * w,), generator=g)
        _, hist = hip.seg_eval(sd[b], hp, wp, (t + seg0).to(dev), h, w, seg0)
        lb = rl[b].reshape(-1)
        assert torch.equal(hist[1].cpu(), torch.bincount(lb, minlength=n))
        assert torch.equal(hist[0].cpu(), torch.bincount(lb[lb == t], minlength=n))


# ------------------------------------------------------------------------------------------------- general sizes
@pytest.mark.parametrize("softmaxed", [False, True], ids=["raw", "softmax"])
@pytest.mark.parametrize("shape", C.GENERAL_SHAPES)
def test_general_sizes_both_paths(shape, softmaxed):
    """seeds 1..7, each on the LDS-staged path (the default: every tile of these shapes fits) and, with the binding's switch,
    on the direct-global path"""
    from ifseg_amd import hip
    dev = _dev()
    hp, wp, n, h, w = shape
    for seed in C.SEEDS:
        s = C.general_scores(shape, seed, softmaxed)
        ref = C.Reference(s, hp, wp, h, w)
        print(shape, seed, "e = %.2e, undecided %.3f %%" % (ref.e, 100 * ref.undecided_share))
        for path, sb in PATHS.items():
            lab, conf, probs = hip.seg_predict(s.to(dev), hp, wp, h, w, conf=True, probs=True, staging_bytes=sb)
            ref.check(lab, conf, probs, what=(shape, seed, path))
            lab2, _, _ = hip.seg_predict(s.to(dev), hp, wp, h, w, staging_bytes=sb)
            assert torch.equal(lab2, lab)


@pytest.mark.parametrize("shape", C.DIRECT_SHAPES)
def test_footprints_beyond_the_staging_buffer(shape):
    """strong downscaling with many classes: no tile fits the staging buffer, the kernel reads global memory on its own;
    a batch of 2 with the second image checked as well"""
    from ifseg_amd import hip
    dev = _dev()
    hp, wp, n, h, w = shape
    for seed in (1, 2):
        s = C.general_scores(shape, seed, False, batch=2)
        ref = C.Reference(s, hp, wp, h, w)
        lab, conf, probs = hip.seg_predict(s.to(dev), hp, wp, h, w, conf=True, probs=True)
        assert lab.dtype == torch.int16
        ref.check(lab, conf, probs, what=(shape, seed))


def test_batch_and_unaligned_rows():
    """B = 3 with an odd width: the rows of images 1 and 2 start at every alignment of the wide label / conf stores"""
    from ifseg_amd import hip
    dev = _dev()
    hp, wp, n, h, w = 4, 6, 150, 37, 91
    s = C.general_scores((hp, wp, n, h, w), 11, True, batch=3)
    ref = C.Reference(s, hp, wp, h, w)
    lab, conf, probs = hip.seg_predict(s.to(dev), hp, wp, h, w, conf=True, probs=True)
    ref.check(lab, conf, probs, what="batch 3")
    # canaries around labels and conf: nothing is written outside [B, h, w], whatever the alignment of the last row's end
    import ctypes
    N = 3 * h * w
    lbuf = torch.full((N + 64,), 201, dtype=torch.uint8, device=dev)
    cbuf = torch.full((N + 64,), 7.0, device=dev)
    sd = s.to(dev)
    i, p = ctypes.c_int, lambda t: ctypes.c_void_p(t.data_ptr())
    assert lbuf[32:].data_ptr() % 16 == 0 and cbuf[32:].data_ptr() % 16 == 0
    rc = hip.lib().ifseg_seg_predict(p(sd), i(3), i(hp), i(wp), i(n), i(h), i(w), p(lbuf[32:]), i(1), p(cbuf[32:]), None,
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    assert lbuf[:32].eq(201).all() and lbuf[32 + N:].eq(201).all() and cbuf[:32].eq(7).all() and cbuf[32 + N:].eq(7).all()
    assert torch.equal(lbuf[32:32 + N].view(3, h, w), lab) and torch.equal(cbuf[32:32 + N].view(3, h, w), conf)


def test_entry_point_refusals():
    """the C entry refuses what the contract excludes, whatever the binding let through"""
    import ctypes
    from ifseg_amd import hip
    dev = _dev()
    lib = hip.lib()
    s = torch.zeros(1, 4, 300, device=dev)
    out = torch.zeros(64, dtype=torch.int16, device=dev)
    i, p = ctypes.c_int, lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else None)
    call = lambda n, h, w, lb, B=1: lib.ifseg_seg_predict(p(s), i(B), i(2), i(2), i(n), i(h), i(w), p(out), i(lb), None, None, None)
    assert call(300, 4, 4, 2) == 0
    assert call(300, 4, 4, 1) == -3          # uint8 labels with n > 256
    assert call(300, 4, 4, 4) == -3
    assert call(513, 4, 4, 2) == -3 and call(0, 4, 4, 2) == -3
    assert call(5, 0, 4, 2) == -2 and call(5, 4, -1, 2) == -2 and call(5, 4, 4, 2, B=0) == -2
    assert call(5, 2 ** 16, 2 ** 15, 2) == -2                     # B h w >= 2^31
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- the op
def test_op_matches_binding_and_opcheck():
    from ifseg_amd import hip
    dev = _dev()
    hp, wp, n, h, w = 2, 3, 257, 40, 23
    s = C.general_scores((hp, wp, n, h, w), 3, False, batch=2).to(dev)
    lab, conf, probs = torch.ops.ifseg.seg_predict(s, hp, wp, h, w, True, True)
    rl, rc, rp = hip.seg_predict(s, hp, wp, h, w, conf=True, probs=True)
    assert lab.dtype == torch.int16 and torch.equal(lab, rl) and torch.equal(conf, rc) and torch.equal(probs, rp)
    lab, conf, probs = torch.ops.ifseg.seg_predict(s, hp, wp, h, w, False, False)
    assert torch.equal(lab, rl) and conf.numel() == 0 and probs.numel() == 0
    # a non-contiguous view is copied, not refused
    st = s.transpose(0, 1).contiguous().transpose(0, 1)
    assert torch.equal(torch.ops.ifseg.seg_predict(st, hp, wp, h, w, False, False)[0], rl)
    utils = ("test_schema", "test_autograd_registration", "test_faketensor")
    torch.library.opcheck(torch.ops.ifseg.seg_predict, (s, hp, wp, h, w, True, True), test_utils=utils)
    torch.library.opcheck(torch.ops.ifseg.seg_predict, (s[:1, :, :5].contiguous(), hp, wp, 7, 9, False, False), test_utils=utils)
    # on a side stream the op follows PyTorch's current stream
    st2 = torch.cuda.Stream()
    st2.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st2):
        l3 = torch.ops.ifseg.seg_predict(s, hp, wp, h, w, False, False)[0]
    st2.synchronize()
    assert torch.equal(l3, rl)


# ------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def e2e():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from ifseg_amd.models.segofa import SegOFAModel, make_config
    dev = torch.device("cuda:0")
    ocfg, sd, img, src = C.e2e_fixture()
    m = SegOFAModel(make_config("segofa_tiny", embed_dim=ocfg.embed_dim, ffn_dim=ocfg.ffn_dim, heads=ocfg.heads,
                                enc_layers=ocfg.enc_layers, dec_layers=ocfg.dec_layers, resnet_layers=ocfg.resnet_layers,
                                num_seg_tokens=ocfg.num_seg_tokens, vocab_size=ocfg.vocab_size,
                                patch_image_size=ocfg.patch_image_size, orig_patch_image_size=ocfg.orig_patch_image_size))
    torch.nn.Module.load_state_dict(m, sd, strict=False)
    return m.to(dev), img.to(dev), ocfg


def _segmenter(m, **kw):
    from ifseg_amd.predict import Segmenter
    return Segmenter(m, category_token_ids=C.E2E_NAMES, prompt_ids=C.E2E_PROMPT, **kw)


@pytest.mark.parametrize("mode", ["probs", "logits"])
def test_segmenter_vs_specification_on_its_own_logits(e2e, mode):
    from ifseg_amd import hip
    m, img, ocfg = e2e
    n = ocfg.num_seg_tokens
    m.train()
    seg = _segmenter(m, upsample=mode)
    res = seg(img, return_conf=True, return_probs=True)
    assert m.training                                     # the training flag is restored
    assert res.labels.shape == (2, 128, 128) and res.labels.dtype == torch.uint8 and res.labels.is_cuda
    assert res.conf.shape == (2, 128, 128) and res.probs.shape == (2, n, 128, 128)
    pad = m.engine.ws["logits_pad"]
    lo = pad[:, :64, :n].float().cpu()
    ref = C.Reference(lo.softmax(-1) if mode == "probs" else lo, 8, 8, 128, 128)
    print(mode, "e = %.2e, undecided %.3f %%" % (ref.e, 100 * ref.undecided_share), "classes", ref.labels.unique().tolist())
    assert ref.labels.unique().numel() >= 3
    if mode == "logits":
        ref.check(res.labels, res.conf, res.probs, what=mode)
    else:
        # the device softmax (fast exponential) is not the specification's: labels under the margin rule, values on the
        # device's own softmax
        ref.check(res.labels, what=mode)
        own = C.Reference(hip.rows_to_f32(pad, n, 64, softmax=True), 8, 8, 128, 128)
        own.check(res.labels, res.conf, res.probs, what="probs on the device softmax")
    m.eval()
    res2 = seg(img)
    assert not m.training and res2.conf is None and res2.probs is None and torch.equal(res2.labels, res.labels)
    # uint8 RGB input: normalised on the device, same path
    rgb = ((img * 0.5 + 0.5) * 255).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    r8 = seg(rgb)
    assert r8.labels.shape == (2, 128, 128)
    x8 = ((rgb.float() / 255 - 0.5) / 0.5).permute(0, 3, 1, 2).contiguous()
    assert torch.equal(r8.labels, seg(x8).labels)


def test_segmenter_smoothing(e2e):
    from ifseg_amd import hip
    m, img, ocfg = e2e
    n = ocfg.num_seg_tokens
    m.eval()
    seg = _segmenter(m, smooth_iters=2, smooth_topk=3, temperature=0.5)
    res = seg(img, return_conf=True, return_probs=True)
    with torch.no_grad():
        _, extra = m(**seg.net_input(img))
    prob = hip.neighbour_smoothing(extra["logits_padded"], n, extra["encoder_returns"]["image_embed_before_proj"][0], 2, 3, 0.5)
    ref = C.Reference(prob, 8, 8, 128, 128)
    ref.check(res.labels, res.conf, res.probs, what="smoothing")
    # and exactly the kernel on that input
    assert torch.equal(res.labels, hip.seg_predict(prob, 8, 8, 128, 128)[0])


def test_segmenter_crf_and_size_lists(e2e):
    from ifseg_amd import hip
    from ifseg_amd.crf import rgb_dense_crf
    m, img, ocfg = e2e
    n = ocfg.num_seg_tokens
    m.eval()
    seg = _segmenter(m, crf_iters=2)
    res = seg(img, return_probs=True)
    base = _segmenter(m)(img, return_probs=True)
    rgb = ((img.float() * 0.5 + 0.5) * 255.0).permute(0, 2, 3, 1).contiguous()
    for b in range(2):
        q = rgb_dense_crf(rgb[b], base.probs[b], 2)
        assert torch.equal(res.labels[b].long(), q.argmax(0))
        assert torch.equal(res.probs[b], q)
    assert res.labels.dtype == torch.uint8
    # crf_images at another output size
    ci = torch.randint(0, 256, (2, 40, 56, 3), generator=torch.Generator().manual_seed(2)).to(img.device)
    r2 = seg(img, out_hw=(40, 56), crf_images=ci)
    p2 = hip.seg_predict(hip.rows_to_f32(m.engine.ws["logits_pad"], n, 64, softmax=True), 8, 8, 40, 56, probs=True)[2]
    for b in range(2):
        assert torch.equal(r2.labels[b].long(), rgb_dense_crf(ci[b].float(), p2[b], 2).argmax(0))
    # a list of sizes: one map per image
    outs = _segmenter(m)(img, out_hw=[(100, 75), (37, 91)], return_conf=True)
    assert isinstance(outs, list) and len(outs) == 2
    assert outs[0].labels.shape == (1, 100, 75) and outs[1].labels.shape == (1, 37, 91) and outs[1].conf.shape == (1, 37, 91)
    sc = hip.rows_to_f32(m.engine.ws["logits_pad"], n, 64, softmax=True)
    assert torch.equal(outs[1].labels, hip.seg_predict(sc[1:2], 8, 8, 37, 91)[0])
    assert torch.equal(outs[0].labels, hip.seg_predict(sc[0:1], 8, 8, 100, 75)[0])
