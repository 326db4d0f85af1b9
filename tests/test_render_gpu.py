"""GPU: hip.seg_render (csrc/render.hip) against the CPU specification `render_reference`, at every byte alignment between
canaries, batched, through the dispatcher, and Segmenter.render_raw end to end on the segofa_tiny fixture.  The rule is integer:
every comparison is `torch.equal`."""
import ctypes

import pytest
import torch

from test_predict_views_gpu import e2e  # noqa: F401  (the segofa_tiny fixture with its three raw shapes)

pytestmark = pytest.mark.gpu

HS, WS = (1, 3, 15, 16, 17, 33), (1, 2, 3, 4, 63, 64, 65, 66, 129)      # every residue of 3 W mod 4, both tile seams
RS, OPACITIES = (0, 1, 4), (0.0, 0.3, 0.5, 1.0)
CASES = [(1, torch.uint8), (15, torch.uint8), (150, torch.uint8), (300, torch.int16)]
BAD_SHAPE, BAD_ARG = -2, -3


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ifseg_amd.ops  # noqa: F401
    return torch.device("cuda:0")


def make_labels(H, W, n, dtype, seed, B=None):
    """blocks of 8 x 32 pixels, so that class edges fall exactly on the tile seams x = 64 and y = 16; single-pixel regions, also
    on both sides of the seams; values outside the palette (255 for bytes unless it is a class, negative and large int16)"""
    g = torch.Generator().manual_seed(seed)
    lead = () if B is None else (B,)
    blocks = torch.randint(0, n, lead + ((H + 7) // 8, (W + 31) // 32), generator=g)
    lab = blocks.repeat_interleave(8, -2).repeat_interleave(32, -1)[..., :H, :W].clone()
    outside = [255] if dtype == torch.uint8 else [-1, n, 511, -32768, 32767, 255 if n <= 255 else -2]
    other = lambda v: (v + 1) % n if n > 1 else outside[0]        # one class: a single pixel of it would be no region
    spots = [(15, 63), (16, 64), (0, 0), (H - 1, W - 1), (H // 2, W // 3), (16, 63), (2, 64)]
    for k, (y, x) in enumerate(spots):
        if y < H and x < W:
            lab[..., y, x] = other(int(lab.reshape(-1, H, W)[0, y, x])) if k % 3 else outside[k % len(outside)]
    for v in outside:                                             # a few more, anywhere
        lab[..., int(torch.randint(0, H, (1,), generator=g)), int(torch.randint(0, W, (1,), generator=g))] = v
    return lab.to(dtype)


def make_conf(shape, seed):
    g = torch.Generator().manual_seed(seed)
    conf = torch.rand(shape, generator=g)
    flat = conf.reshape(-1)
    special = torch.tensor([0.0, 1.0, float("nan"), 1.7, -0.3, float("inf"), float("-inf"), 0.5 / 255, 254.5 / 255])
    flat[:min(special.numel(), flat.numel())] = special[:flat.numel()]
    return conf


def make_image(shape, seed):
    return torch.randint(0, 256, tuple(shape) + (3,), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


def _palette(n):
    from ifseg_amd.predict import default_palette
    return default_palette(n)


@pytest.mark.parametrize("n,dtype", CASES, ids=["n1", "n15", "n150", "n300_i16"])
def test_kernel_is_the_specification(n, dtype):
    from ifseg_amd import hip
    from ifseg_amd.predict import render_reference
    dev = _dev()
    pal = _palette(n)
    pal_d = pal.to(dev)
    keys, same = [], []
    for H in HS:
        for W in WS:
            labels, image, conf = make_labels(H, W, n, dtype, H * 131 + W), make_image((H, W), W), make_conf((H, W), H)
            ld, im_d, cf_d = labels.to(dev), image.to(dev), conf.to(dev)
            for r in RS:
                color = (255, 255, 255) if r != 1 else (7, 130, 251)
                for opacity in OPACITIES:
                    for c, c_d in ((None, None), (conf, cf_d)):
                        want = render_reference(labels, image, pal, opacity, r, color, c)
                        got = hip.seg_render(ld, im_d, pal_d, opacity, r, color, conf=c_d)
                        assert got.dtype == torch.uint8 and got.shape == (H, W, 3)
                        keys.append((H, W, r, opacity, c is not None))
                        same.append((got == want.to(dev)).all())
    same = torch.stack(same).cpu().tolist()                       # the one synchronisation
    wrong = [k for k, ok in zip(keys, same) if not ok]
    assert len(keys) == len(HS) * len(WS) * len(RS) * len(OPACITIES) * 2 and not wrong, wrong[:10]


def test_contours_cross_the_tile_seams_and_fit_an_image_smaller_than_r():
    """what the label maps above are built to do, checked on the reference so that the comparison is not vacuous"""
    from ifseg_amd import hip
    from ifseg_amd.predict import render_reference
    dev = _dev()
    white = torch.tensor([255, 255, 255], dtype=torch.uint8)
    labels, image = make_labels(33, 129, 15, torch.uint8, 5), torch.zeros(33, 129, 3, dtype=torch.uint8)
    for r in (1, 4):
        edge = (render_reference(labels, image, _palette(15), 0.0, r) == white).all(-1)
        for y, x in ((15, 63), (16, 64), (15, 64), (16, 63)):     # contour pixels on each side of both seams
            assert edge[y, x], (r, y, x)
        got = hip.seg_render(labels.to(dev), image.to(dev), _palette(15).to(dev), 0.0, r)
        assert torch.equal((got.cpu() == white).all(-1), edge) and 0 < int(edge.sum()) < edge.numel()
    # a 3 x 2 image under r = 4: every window is the whole image
    small = torch.tensor([[0, 0], [0, 1], [0, 0]], dtype=torch.uint8)
    got = hip.seg_render(small.to(dev), make_image((3, 2), 1).to(dev), _palette(2).to(dev), 1.0, 4)
    assert (got.cpu() == white).all() and torch.equal(got.cpu(), render_reference(small, make_image((3, 2), 1), _palette(2), 1.0, 4))
    got = hip.seg_render(torch.zeros(3, 2, dtype=torch.uint8, device=dev), make_image((3, 2), 1).to(dev), _palette(2).to(dev), 1.0, 4)
    assert not got.any()                                          # one class everywhere: no contour, colour 0 at opacity 1


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16], ids=["u8", "i16"])
def test_every_alignment_between_canaries(dtype):
    """image, output and labels as views into larger flat buffers at every byte offset 0 .. 3 independently (int16 labels: even and
    odd element offsets); 64 canary bytes in front of and behind the output; a second launch writes the same bytes"""
    from ifseg_amd import hip
    from ifseg_amd.predict import render_reference
    dev = _dev()
    n = 15 if dtype == torch.uint8 else 300
    pal = _palette(n)
    palbuf = torch.zeros(3 * n + 4, dtype=torch.uint8, device=dev)
    keys, same = [], []
    for H, W in ((5, 65), (17, 130)):
        labels, image, conf = make_labels(H, W, n, dtype, 3), make_image((H, W), 4), make_conf((H, W), 5)
        want = {c: render_reference(labels, image, pal, 0.3, 1, (9, 8, 7), conf if c else None).to(dev) for c in (False, True)}
        cf_d = conf.to(dev)
        imbuf = torch.zeros(H * W * 3 + 4, dtype=torch.uint8, device=dev)
        labbuf = torch.zeros(H * W + 4, dtype=dtype, device=dev)
        outbuf = torch.empty(64 + 4 + H * W * 3 + 64, dtype=torch.uint8, device=dev)
        assert imbuf.data_ptr() % 4 == 0 and labbuf.data_ptr() % 4 == 0 and outbuf.data_ptr() % 4 == 0 and palbuf.data_ptr() % 4 == 0
        for io in range(4):
            im_d = imbuf[io:io + H * W * 3].view(H, W, 3).copy_(image)
            for lo in range(4 if dtype == torch.uint8 else 2):
                ld = labbuf[lo:lo + H * W].view(H, W).copy_(labels)
                for oo in range(4):
                    outbuf.fill_(0xA5)
                    out = outbuf[64 + oo:64 + oo + H * W * 3].view(H, W, 3)
                    pal_d = palbuf[(io + lo) % 4:(io + lo) % 4 + 3 * n].view(n, 3).copy_(pal)
                    assert im_d.data_ptr() % 4 == io and out.data_ptr() % 4 == oo and ld.data_ptr() % 4 == lo * ld.element_size()
                    with_conf = (io + lo + oo) % 2 == 1
                    got = hip.seg_render(ld, im_d, pal_d, 0.3, 1, (9, 8, 7), conf=cf_d if with_conf else None, out=out)
                    assert got is out
                    first = outbuf.clone()
                    hip.seg_render(ld, im_d, pal_d, 0.3, 1, (9, 8, 7), conf=cf_d if with_conf else None, out=out)
                    keys.append((H, W, io, lo, oo))
                    same.append(torch.stack([(out == want[with_conf]).all(), (outbuf[:64 + oo] == 0xA5).all(),
                                             (outbuf[64 + oo + H * W * 3:] == 0xA5).all(), (outbuf == first).all()]))
    same = torch.stack(same).cpu().tolist()
    wrong = [(k, ok) for k, ok in zip(keys, same) if not all(ok)]             # (picture, canary in front, canary behind, relaunch)
    assert len(keys) == 2 * 4 * 4 * (4 if dtype == torch.uint8 else 2) and not wrong, wrong[:10]


def test_batch_is_three_single_launches():
    from ifseg_amd import hip
    from ifseg_amd.predict import render_reference
    dev = _dev()
    B, H, W, n = 3, 17, 65, 150
    labels, image, conf = make_labels(H, W, n, torch.uint8, 8, B=B), make_image((B, H, W), 9), make_conf((B, H, W), 10)
    ld, im_d, cf_d, pal_d = labels.to(dev), image.to(dev), conf.to(dev), _palette(n).to(dev)
    for c, c_d in ((None, None), (conf, cf_d)):
        got = hip.seg_render(ld, im_d, pal_d, 0.3, 1, conf=c_d)
        assert got.shape == (B, H, W, 3)
        for b in range(B):
            assert torch.equal(got[b], hip.seg_render(ld[b], im_d[b], pal_d, 0.3, 1, conf=None if c is None else c_d[b])), b
        assert torch.equal(got.cpu(), render_reference(labels, image, _palette(n), 0.3, 1, conf=c))
    assert not torch.equal(got[0], got[1])


def test_entry_point_refusals():
    """each refusal returns its code and launches nothing: the poisoned output stays poisoned"""
    from ifseg_amd import hip
    dev = _dev()
    lib = hip.lib()
    i, vp = ctypes.c_int, ctypes.c_void_p
    p = lambda t, off=0: vp(t.data_ptr() + off) if t is not None else vp(None)
    lab = torch.zeros(64, dtype=torch.int16, device=dev)
    img, pal = torch.zeros(16 * 3, dtype=torch.uint8, device=dev), torch.zeros(512 * 3, dtype=torch.uint8, device=dev)
    conf = torch.zeros(17, device=dev)
    out = torch.full((16 * 3 + 8,), 77, dtype=torch.uint8, device=dev)

    def call(labels=p(lab), lb=2, image=p(img), palette=p(pal), n=5, cf=vp(None), B=1, H=4, W=4, alpha=128, r=1, rgb=0xffffff, o=p(out, 4)):
        return lib.ifseg_seg_render(labels, i(lb), image, palette, i(n), cf, i(B), i(H), i(W), i(alpha), i(r), i(rgb), o, None)

    for bad in (dict(labels=vp(None)), dict(image=vp(None)), dict(palette=vp(None)), dict(o=vp(None)), dict(lb=0), dict(lb=3), dict(lb=4),
                dict(labels=p(lab, 1)), dict(cf=p(conf, 2)), dict(n=0), dict(n=513), dict(r=-1), dict(r=5), dict(alpha=-1),
                dict(alpha=257), dict(rgb=-1), dict(rgb=0x1000000)):
        assert call(**bad) == BAD_ARG, bad
    for bad in (dict(B=0), dict(H=0), dict(W=-1), dict(H=2 ** 16, W=2 ** 15), dict(B=2 ** 11, H=2 ** 10, W=2 ** 10)):
        assert call(**bad) == BAD_SHAPE, bad
    torch.cuda.synchronize()
    assert out.eq(77).all()                                       # no launch so far
    # the limits themselves pass: n = 512, r = 4, alpha = 256, labels at an odd byte when they are bytes, conf given
    assert call(n=512, r=4, alpha=256, lb=1, labels=p(lab, 1), cf=p(conf, 4)) == 0
    torch.cuda.synchronize()
    assert out[:4].eq(77).all() and out[4 + 48:].eq(77).all() and not out[4:4 + 48].any()      # class 0 of a zero palette


def test_op_matches_the_binding_and_refuses(monkeypatch):
    from ifseg_amd import hip
    dev = _dev()
    H, W, n = 17, 66, 300
    labels, image, conf = make_labels(H, W, n, torch.int16, 1, B=2).to(dev), make_image((2, H, W), 2).to(dev), make_conf((2, H, W), 3).to(dev)
    pal = _palette(n).to(dev)
    op = torch.ops.ifseg.seg_render
    want = hip.seg_render(labels, image, pal, 0.3, 1, (1, 2, 3), conf=conf)
    got = op(labels, image, pal, 0.3, 1, [1, 2, 3], conf)
    assert torch.equal(got, want) and got.data_ptr() != want.data_ptr()
    assert torch.equal(op(labels[0], image[0], pal, 1.0, 0, [0, 0, 0], None), hip.seg_render(labels[0], image[0], pal, 1.0, 0, (0, 0, 0)))
    # non-contiguous inputs are copied
    assert torch.equal(op(labels.transpose(1, 2), image.transpose(1, 2), pal, 0.3, 1, [1, 2, 3], conf.transpose(1, 2)),
                       want.transpose(1, 2))
    utils = ("test_schema", "test_autograd_registration", "test_faketensor")
    torch.library.opcheck(op, (labels, image, pal, 0.3, 1, [1, 2, 3], conf), test_utils=utils)
    torch.library.opcheck(op, (labels[0].to(torch.uint8), image[0], pal, 0.5, 0, [255, 255, 255], None), test_utils=utils)
    # on a side stream the op follows PyTorch's current stream
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        side = op(labels, image, pal, 0.3, 1, [1, 2, 3], conf)
    st.synchronize()
    assert torch.equal(side, want)
    # bad arguments: a ValueError, and no launch
    monkeypatch.setattr(hip, "seg_render", lambda *a, **k: (_ for _ in ()).throw(RuntimeError("seg_render was reached")))
    for bad in ((labels.long(), image, pal, 0.5, 0, [0, 0, 0], None), (labels, image.float(), pal, 0.5, 0, [0, 0, 0], None),
                (labels, image[:1], pal, 0.5, 0, [0, 0, 0], None), (labels, image, pal[:0], 0.5, 0, [0, 0, 0], None),
                (labels, image, pal, 1.5, 0, [0, 0, 0], None), (labels, image, pal, 0.5, 5, [0, 0, 0], None),
                (labels, image, pal, 0.5, 1, [0, 0, 256], None), (labels, image, pal, 0.5, 1, [0, 0, 0], conf[0])):
        with pytest.raises(ValueError, match="ifseg::seg_render"):
            op(*bad)
    with pytest.raises(RuntimeError, match="seg_render was reached"):
        op(labels, image, pal, 0.5, 0, [0, 0, 0], None)


# ------------------------------------------------------------------------------------------------- end to end
@pytest.mark.parametrize("call,fade", [({}, False), ({"scales": (0.5, 1.0), "flip": True}, False), ({"slide": True}, False), ({}, True)],
                         ids=["single", "ms_flip", "slide", "fade_by_conf"])
def test_render_raw_is_segment_raw_rendered(e2e, call, fade):  # noqa: F811
    from ifseg_amd.predict import RenderResult, default_palette, render_reference
    m, raw, ocfg, mk = e2e
    n = ocfg.num_seg_tokens
    seg = mk()
    before = seg.segment_raw(raw, return_conf=fade, **call)
    res = seg.render_raw(raw, boundary=1, fade_by_conf=fade, **call)
    after = seg.segment_raw(raw, return_conf=fade, **call)
    assert len(res) == 3 and all(isinstance(r, RenderResult) for r in res)
    for r, b, a, photo in zip(res, before, after, raw):
        assert torch.equal(r.labels, b.labels) and r.labels.dtype == b.labels.dtype and torch.equal(a.labels, b.labels)
        assert r.picture.is_cuda and r.picture.dtype == torch.uint8 and r.picture.shape == photo.shape
        if fade:
            assert torch.equal(r.conf, b.conf) and torch.equal(a.conf, b.conf)
        else:
            assert r.conf is None
        want = render_reference(r.labels.cpu(), photo, default_palette(n), 0.5, 1, conf=r.conf.cpu() if fade else None)
        assert torch.equal(r.picture.cpu(), want)
        assert not torch.equal(r.picture.cpu(), photo)             # something was drawn


def test_render_raw_palette_opacity_device_images_and_task(e2e):  # noqa: F811
    from ifseg_amd.predict import render_reference
    from ifseg_amd.tasks.mm_tasks.segmentation import SegmentationTask
    import _predict_cases as PC
    m, raw, ocfg, mk = e2e
    n = ocfg.num_seg_tokens
    seg = mk()
    pal = torch.randint(0, 256, (n + 3, 3), generator=torch.Generator().manual_seed(4), dtype=torch.uint8)
    dev_raw = [r.to("cuda:0") for r in raw]
    res = seg.render_raw(dev_raw, palette=pal.to("cuda:0"), opacity=1.0, boundary=2, boundary_color=(0, 255, 0))
    for r, photo in zip(res, raw):
        assert torch.equal(r.picture.cpu(), render_reference(r.labels.cpu(), photo, pal, 1.0, 2, (0, 255, 0)))
    one = seg.render_raw(raw[1], palette=pal)                      # one image, a host palette, no contours
    assert len(one) == 1 and torch.equal(one[0].picture.cpu(), render_reference(one[0].labels.cpu(), raw[1], pal))
    with pytest.raises(ValueError, match="fade_by_conf"):
        mk(crf_iters=1).render_raw(raw, fade_by_conf=True)
    task = SegmentationTask(num_seg_tokens=n, patch_image_size=ocfg.patch_image_size, category_token_ids=PC.E2E_NAMES)
    ts = task.render_raw(m, raw, prompt_ids=PC.E2E_PROMPT, boundary=1)
    mine = seg.render_raw(raw, boundary=1)
    assert all(torch.equal(a.picture, b.picture) and torch.equal(a.labels, b.labels) for a, b in zip(ts, mine))
