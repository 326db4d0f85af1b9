"""GPU: hip.image_load (csrc/imgload.hip) against the CPU specification of ifseg_amd/imageio.py, torch.ops.ifseg.image_load
through the dispatcher, and Segmenter.segment_raw end to end on the segofa_tiny fixture.  The comparison rule is in
tests/_image_load_cases.py.

Which path of the kernel a case takes: with the default staging buffer every tile of the exact and the general family stages
its source bytes in LDS (the largest footprint, 40 rows x 152 pixels under a tile of the 700 x 300 downscale, is 18 KiB);
`staging_bytes=0` sends the same case down the direct-global path; the 2000 x 1500 -> 16 x 12 case takes the direct path on
its own (its footprint, the whole 9 MB image under one tile, exceeds any staging buffer)."""
import pytest
import torch

import _image_load_cases as C
import _predict_cases as PC

pytestmark = pytest.mark.gpu

PATHS = {"staged": None, "direct": 0}          # hip.image_load(staging_bytes=...)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ifseg_amd.ops  # noqa: F401
    return torch.device("cuda:0")


def _q(img_dev, oh, ow, staging_bytes=None, reverse_channels=False):
    """the device's grey levels, through the table that carries q itself"""
    from ifseg_amd import hip
    return C.q_of(hip.image_load(img_dev, oh, ow, C.Q_MEAN, C.Q_STD, reverse_channels, staging_bytes=staging_bytes))


# ------------------------------------------------------------------------------------------------- exact family
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("shape", C.exact_shapes())
def test_exact_family_bit_for_bit(shape, path):
    from ifseg_amd import hip
    from ifseg_amd.imageio import image_load_reference
    dev = _dev()
    B, H0, W0, oh, ow = shape
    img = C.exact_images(shape)
    d = img.to(dev)
    sb = PATHS[path]
    for rev in (True, False):
        n32, q32, _ = image_load_reference(img, oh, ow, reverse_channels=rev, dtype=torch.float32)
        assert torch.equal(_q(d, oh, ow, sb, rev).cpu(), q32)
        o32 = hip.image_load(d, oh, ow, reverse_channels=rev, staging_bytes=sb)
        assert o32.dtype == torch.float32 and o32.shape == (B, 3, oh, ow) and o32.is_contiguous()
        assert torch.equal(o32.cpu(), n32)
        o16 = hip.image_load(d, oh, ow, reverse_channels=rev, dtype=torch.bfloat16, staging_bytes=sb)
        assert o16.dtype == torch.bfloat16 and torch.equal(o16.cpu(), n32.to(torch.bfloat16))
    # per-channel statistics, into a caller's tensor
    from ifseg_amd.imageio import IMAGENET_DEFAULT_MEAN as M, IMAGENET_DEFAULT_STD as S
    out = torch.empty(B, 3, oh, ow, device=dev)
    assert hip.image_load(d, oh, ow, M, S, staging_bytes=sb, out=out) is out
    assert torch.equal(out.cpu(), image_load_reference(img, oh, ow, M, S, dtype=torch.float32)[0])


# ------------------------------------------------------------------------------------------------- general sizes
@pytest.mark.parametrize("case", C.GENERAL_CASES)
def test_general_sizes_both_paths(case):
    """seeds 1..3, each on the LDS-staged path (the default: every tile of these cases fits) and, with the binding's switch,
    on the direct-global path; fp32 and bf16 output"""
    from ifseg_amd import hip
    dev = _dev()
    for seed in C.SEEDS:
        img, oh, ow, ref = C.general_reference(case, seed)
        print(case, seed, "-> %d x %d  e = %.2e, left out %.3f %%" % (oh, ow, ref.e, 100 * ref.undecided_share))
        d = img.to(dev)
        for path, sb in PATHS.items():
            q = _q(d, oh, ow, sb)
            print("   ", path, "grey levels off the reference: %d of %d" % (int((q.cpu() != ref.q).sum()), q.numel()))
            ref.check(q, hip.image_load(d, oh, ow, staging_bytes=sb), what=(case, seed, path, "fp32"))
            ref.check(q, hip.image_load(d, oh, ow, dtype=torch.bfloat16, staging_bytes=sb), what=(case, seed, path, "bf16"))


def test_footprint_beyond_the_staging_buffer():
    """strong downscaling: the one tile's footprint is the whole image, the kernel reads global memory on its own; a batch of
    2 with the second image checked as well"""
    from ifseg_amd import hip
    dev = _dev()
    H0, W0, oh, ow = 2000, 1500, 16, 12
    img = C.images(2, H0, W0, 21)
    ref = C.Reference(img, oh, ow)
    d = img.to(dev)
    q = _q(d, oh, ow)
    ref.check(q, hip.image_load(d, oh, ow), what="direct, fp32")
    ref.check(q, hip.image_load(d, oh, ow, dtype=torch.bfloat16), what="direct, bf16")


@pytest.mark.parametrize("ow", [63, 65, 129])
def test_batch_and_unaligned_rows(ow):
    """B = 3, 111-byte source rows (every shift of the aligned staging loads) and odd output widths in bf16: the rows of the
    planes start on even and odd elements, so pairs, leading and trailing halves and the cut last tile are all taken"""
    from ifseg_amd import hip
    dev = _dev()
    B, H0, W0, oh = 3, 29, 37, 35
    img = C.images(B, H0, W0, 40 + ow)
    ref = C.Reference(img, oh, ow)
    # the source at every byte alignment: a view into a larger buffer
    big = torch.zeros(B * H0 * W0 * 3 + 8, dtype=torch.uint8, device=dev)
    N = B * 3 * oh * ow
    for shift in range(4):
        view = big[shift:shift + B * H0 * W0 * 3].view(B, H0, W0, 3)
        view.copy_(img.to(dev))
        assert view.data_ptr() % 4 == (big.data_ptr() + shift) % 4
        for path, sb in PATHS.items():
            q = _q(view, oh, ow, sb)
            # canaries around the output: nothing is written outside [B, 3, oh, ow]
            buf = torch.full((N + 64,), 7.0, dtype=torch.bfloat16, device=dev)
            out = buf[32:32 + N].view(B, 3, oh, ow)
            assert out.data_ptr() % 16 == 0
            hip.image_load(view, oh, ow, dtype=torch.bfloat16, staging_bytes=sb, out=out)
            assert buf[:32].eq(7).all() and buf[32 + N:].eq(7).all()
            ref.check(q, out, what=(ow, shift, path, "bf16"))
            ref.check(q, hip.image_load(view, oh, ow, staging_bytes=sb), what=(ow, shift, path, "fp32"))


def test_entry_point_refusals():
    """the C entry refuses what the contract excludes: error codes only, nothing launched"""
    import ctypes
    from ifseg_amd import hip
    dev = _dev()
    lib = hip.lib()
    img = torch.zeros(1, 4, 4, 3, dtype=torch.uint8, device=dev)
    out = torch.full((1024,), 3.0, device=dev)
    lut = torch.zeros(3, 256, device=dev)
    i, p = ctypes.c_int, lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None

    def call(B=1, H0=4, W0=4, oh=8, ow=8, im=img, lu=lut, o=out, ob=4):
        return lib.ifseg_image_load(p(im), i(B), i(H0), i(W0), i(oh), i(ow), p(lu), i(1), p(o), i(ob), None)

    assert call() == 0 and call(ob=2) == 0
    assert call(im=None) == -3 and call(lu=None) == -3 and call(o=None) == -3
    assert call(ob=1) == -3 and call(ob=8) == -3                              # fp32 and bf16 only
    assert call(o=out[1:]) == -3 and call(o=out[2:], ob=2) == -3              # 16-byte aligned output
    assert call(B=0) == -2 and call(H0=0) == -2 and call(W0=-1) == -2 and call(oh=0) == -2 and call(ow=0) == -2
    assert call(H0=2 ** 15, W0=2 ** 15) == -2                                 # B H0 W0 3 >= 2^31
    assert call(oh=2 ** 15, ow=2 ** 15) == -2                                 # B 3 oh ow >= 2^31
    assert call(H0=2 ** 16, W0=1, oh=2 ** 15, ow=1) == -2                     # the integer coordinate: 2 H0 oh >= 2^31
    torch.cuda.synchronize()
    # through the binding: RuntimeError with the code
    with pytest.raises(RuntimeError, match="image_load failed with code -3"):
        hip.image_load(img, 8, 8, out=out[1:1 + 192].view(1, 3, 8, 8))
    tall = torch.zeros(1, 2 ** 16, 1, 3, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="image_load failed with code -2"):
        hip.image_load(tall, 2 ** 15, 1)
    # the staging switch returns the previous limit, and the binding restores it
    prev = lib.ifseg_image_load_staging(i(1000))
    assert prev > 60000 and lib.ifseg_image_load_staging(i(-1)) == 1000 and lib.ifseg_image_load_staging(i(prev)) == prev
    hip.image_load(img, 8, 8, staging_bytes=0)
    assert lib.ifseg_image_load_staging(i(prev)) == prev
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- the op
def test_op_matches_binding_and_opcheck():
    from ifseg_amd import hip
    from ifseg_amd.imageio import IMAGENET_DEFAULT_MEAN as M, IMAGENET_DEFAULT_STD as S
    dev = _dev()
    img = C.images(2, 23, 40, 9).to(dev)
    op = torch.ops.ifseg.image_load
    for dt in (torch.float32, torch.bfloat16):
        o = op(img, 47, 81, list(M), list(S), True, dt)
        assert o.dtype == dt and torch.equal(o, hip.image_load(img, 47, 81, M, S, True, dt))
    assert torch.equal(op(img, 47, 81, [0.5] * 3, [0.5] * 3, True, torch.float32), hip.image_load(img, 47, 81, reverse_channels=True))
    # a non-contiguous view is copied, not refused
    nc = img.transpose(1, 2).contiguous().transpose(1, 2)
    assert not nc.is_contiguous()
    assert torch.equal(op(nc, 47, 81, [0.5] * 3, [0.5] * 3, False, torch.float32), hip.image_load(img, 47, 81))
    utils = ("test_schema", "test_autograd_registration", "test_faketensor")
    torch.library.opcheck(op, (img, 47, 81, [0.5] * 3, [0.5] * 3, True, torch.float32), test_utils=utils)
    torch.library.opcheck(op, (img[:1], 5, 3, list(M), list(S), False, torch.bfloat16), test_utils=utils)
    # on a side stream the op follows PyTorch's current stream
    ref = hip.image_load(img, 47, 81)
    st2 = torch.cuda.Stream()
    st2.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st2):
        o3 = op(img, 47, 81, [0.5] * 3, [0.5] * 3, False, torch.float32)
    st2.synchronize()
    assert torch.equal(o3, ref)


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


def test_segment_raw_end_to_end(e2e):
    from ifseg_amd.imageio import eval_size, image_load_reference
    m, raw, ocfg, mk = e2e
    dev = torch.device("cuda:0")
    seg = mk()
    outs = seg.segment_raw(raw, return_conf=True, return_probs=True)          # host tensors, one list
    assert isinstance(outs, list) and len(outs) == 3
    n = ocfg.num_seg_tokens
    sizes = [eval_size(r.shape[0], r.shape[1], ocfg.patch_image_size) for r in raw]
    assert sizes == [(128, 192), (192, 128), (128, 128)]
    classes = set()
    for r, o, (oh, ow) in zip(raw, outs, sizes):
        H, W = r.shape[:2]
        assert o.labels.shape == (H, W) and o.labels.dtype == torch.uint8 and o.labels.is_cuda
        assert o.conf.shape == (H, W) and o.probs.shape == (n, H, W)
        # the existing path on the specification's tensor: same engine, same kernels, and q agrees (exact-family ratios)
        norm, q, _ = image_load_reference(r[None], oh, ow, dtype=torch.float32)
        assert torch.equal(norm, image_load_reference(r[None], oh, ow, dtype=torch.float64)[0])
        want = seg(norm.to(dev), out_hw=(H, W), return_conf=True, return_probs=True)
        assert torch.equal(o.labels, want.labels[0]) and torch.equal(o.conf, want.conf[0]) and torch.equal(o.probs, want.probs[0])
        classes |= set(o.labels.unique().tolist())
    assert len(classes) >= 2                                                  # not one flat class
    # device tensors, one image, labels only; a list with a repeated shape batches and keeps the order
    one = seg.segment_raw(raw[0].to(dev))
    assert len(one) == 1 and one[0].conf is None and one[0].probs is None and torch.equal(one[0].labels, outs[0].labels)
    again = seg.segment_raw([raw[2], raw[0], raw[2], raw[0]], max_batch=2)
    assert [tuple(a.labels.shape) for a in again] == [(64, 64), (60, 90), (64, 64), (60, 90)]
    assert torch.equal(again[0].labels, again[2].labels) and torch.equal(again[1].labels, again[3].labels)
    # the default keeps RGB, the order __call__ feeds: at the model's own size (the identity resize) the network input of both
    # entry points is the same tensor up to the device's division.  prepare_images divides on the device (a reciprocal
    # multiply: <= 1 ulp of a value below 1, 6e-8, doubled by / 0.5), the kernel reads the host-built table: 2^-22 covers
    # it, a swapped channel order would be off by O(1) on a random image
    from ifseg_amd import hip
    sq = C.images(1, 128, 128, 5).to(dev)
    d = (hip.image_load(sq, 128, 128) - seg.prepare_images(sq)[0]).abs().max().item()
    print("max |image_load - prepare_images| at the identity size = %.2e" % d)
    assert d <= 2.0 ** -22
    # reversed is another input to the network
    bgr = seg.segment_raw(raw[0], reverse_channels=True, return_probs=True)[0]
    assert not torch.equal(bgr.probs, outs[0].probs)
    assert torch.equal(bgr.probs, seg.segment_raw(raw[0].flip(-1).contiguous(), return_probs=True)[0].probs)


def test_segment_raw_with_crf(e2e):
    m, raw, ocfg, mk = e2e
    outs = mk(crf_iters=1).segment_raw(raw, return_conf=True, return_probs=True)
    for r, o in zip(raw, outs):
        H, W = r.shape[:2]
        assert o.labels.shape == (H, W) and o.probs.shape == (ocfg.num_seg_tokens, H, W)
        assert torch.isfinite(o.probs).all() and torch.isfinite(o.conf).all()
        assert torch.equal(o.labels.long(), o.probs.argmax(0))
