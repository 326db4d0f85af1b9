"""CPU: the specification of the rendering kernel (`ifseg_amd.predict.render_reference`, `default_palette`) against an
independent per-pixel loop and against the reference demo's numpy formula, the header, and the refusals of the binding, the op
and `Segmenter.render_raw` before anything reaches the library."""
import math
import os
import re

import numpy as np
import pytest
import torch

from ifseg_amd import hip
from ifseg_amd.predict import RenderResult, Segmenter, default_palette, render_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 11, 13


def _case(dtype, n, seed=0):
    """an 11 x 13 label map of blocks, single pixels and values outside the palette, its image and a confidence plane with
    every special value"""
    g = torch.Generator().manual_seed(seed)
    labels = torch.randint(0, n, (4, 5), generator=g).repeat_interleave(3, 0).repeat_interleave(3, 1)[:H, :W].clone()
    labels[2, 3], labels[10, 12], labels[0, 0] = (labels[2, 3] + 1) % n, (labels[10, 12] + 1) % n, (labels[0, 0] + 1) % n
    labels[5, 6:9] = 255                                          # "ignore": outside the palette for n <= 255
    if dtype == torch.int16:
        labels[7:9, 1] = -1
        labels[9, 9] = 300
    labels = labels.to(dtype)
    image = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)
    conf = torch.rand(H, W, generator=g)
    conf[0, :6] = torch.tensor([0.0, 1.0, float("nan"), 1.7, -0.3, float("inf")])
    conf[1, 0], conf[1, 1] = 0.5 / 255, 254.5 / 255               # the rounding of q at both ends
    return labels, image, conf


def _loop(labels, image, palette, opacity, r, color, conf):
    """the rule of render_reference, pixel by pixel in Python integers"""
    alpha = int(math.floor(opacity * 256 + 0.5))
    n, out = len(palette), np.zeros((H, W, 3), dtype=np.uint8)
    lab, img, pal = labels.tolist(), image.tolist(), palette.tolist()
    for y in range(H):
        for x in range(W):
            edge = any(lab[yy][xx] != lab[y][x] for yy in range(max(y - r, 0), min(y + r, H - 1) + 1)
                       for xx in range(max(x - r, 0), min(x + r, W - 1) + 1))
            a = alpha
            if conf is not None:
                v = np.float32(np.float32(conf[y, x].item()) * np.float32(255)) + np.float32(0.5)
                q = 0 if np.isnan(v) else int(min(max(np.floor(v), 0), 255))
                a = (alpha * q + 127) // 255
            if edge:
                out[y, x] = color
            elif 0 <= lab[y][x] < n:
                out[y, x] = [(img[y][x][c] * (256 - a) + pal[lab[y][x]][c] * a) >> 8 for c in range(3)]
            else:
                out[y, x] = img[y][x]
    return torch.from_numpy(out)


@pytest.mark.parametrize("with_conf", [False, True], ids=["plain", "conf"])
@pytest.mark.parametrize("dtype,n", [(torch.uint8, 15), (torch.int16, 15), (torch.uint8, 256)], ids=["u8", "i16", "u8_n256"])
def test_render_reference_is_the_per_pixel_loop(dtype, n, with_conf):
    labels, image, conf = _case(dtype, n)
    conf = conf if with_conf else None
    palette = default_palette(n)
    for r in (0, 1, 2, 4):
        for opacity in (0.0, 0.3, 0.5, 1.0):
            color = (255, 255, 255) if r != 2 else (1, 200, 30)
            got = render_reference(labels, image, palette, opacity, r, color, conf)
            assert got.dtype == torch.uint8 and got.shape == (H, W, 3)
            assert torch.equal(got, _loop(labels, image, palette, opacity, r, color, conf)), (r, opacity)
    # out-of-palette pixels away from a contour keep the image; at r = 0 every one of them does
    got = render_reference(labels, image, palette, 1.0, 0)
    outside = (labels.long() < 0) | (labels.long() >= n)
    assert torch.equal(got[outside], image[outside]) and (outside.any() or n == 256)
    # batched input is the images one by one
    both = render_reference(torch.stack([labels, labels.flip(0)]), torch.stack([image, image.flip(1)]), palette, 0.3, 1)
    assert both.shape == (2, H, W, 3) and torch.equal(both[0], render_reference(labels, image, palette, 0.3, 1))
    assert torch.equal(both[1], render_reference(labels.flip(0), image.flip(1), palette, 0.3, 1))


def test_render_reference_is_the_demo_formula_on_every_value_pair():
    """image value v x colour value c, all 256 x 256 pairs: opacity 0.5 is the notebook's float64 blend truncated to uint8,
    opacity 1.0 its cmap[labels]; any other opacity stays within one grey level of the float64 formula"""
    v = torch.arange(256, dtype=torch.uint8)
    image = v[:, None, None].expand(256, 256, 3).contiguous()
    labels = v[None, :].expand(256, 256).contiguous()
    cmap = v[:, None].expand(256, 3).contiguous()
    im64, c64 = image.numpy().astype(np.float64), cmap.numpy()[labels.numpy()].astype(np.float64)
    half = (im64 * 0.5 + c64 * 0.5).astype(np.uint8)
    assert torch.equal(render_reference(labels, image, cmap, 0.5), torch.from_numpy(half))
    assert torch.equal(render_reference(labels, image, cmap, 1.0), torch.from_numpy(cmap.numpy()[labels.numpy()]))
    assert torch.equal(render_reference(labels, image, cmap, 0.0), image)
    rng = np.random.RandomState(0)
    for opacity in rng.rand(20).tolist():
        want = (im64 * (1 - opacity) + c64 * opacity).astype(np.uint8).astype(np.int64)
        got = render_reference(labels, image, cmap, opacity).numpy().astype(np.int64)
        assert np.abs(got - want).max() <= 1, opacity


def test_render_reference_refusals():
    labels, image, conf = _case(torch.uint8, 15)
    pal = default_palette(15)
    for bad in (1.5, -0.1, float("nan"), "0.5"):
        with pytest.raises(ValueError, match="opacity"):
            render_reference(labels, image, pal, bad)
    for bad in (5, -1, 1.0, True):
        with pytest.raises(ValueError, match="boundary must be"):
            render_reference(labels, image, pal, 0.5, bad)
    for bad in ((255, 255), (0, 0, 256), (0.5, 0, 0)):
        with pytest.raises(ValueError, match="boundary_color"):
            render_reference(labels, image, pal, 0.5, 1, bad)
    with pytest.raises(ValueError, match="labels must be integer"):
        render_reference(labels.float(), image, pal)
    with pytest.raises(ValueError, match="image must be uint8"):
        render_reference(labels, image[:, :12], pal)
    with pytest.raises(ValueError, match="palette must be uint8"):
        render_reference(labels, image, pal[:0])
    with pytest.raises(ValueError, match="conf must be float32"):
        render_reference(labels, image, pal, conf=conf.double())


def test_default_palette():
    p = default_palette(512)
    assert p.dtype == torch.uint8 and p.shape == (512, 3)
    assert len({tuple(c) for c in p.tolist()}) == 512
    assert p[0].tolist() == [0, 0, 0] and p[1].tolist() == [128, 0, 0]
    assert p[255].tolist() == [224, 224, 192] and p[256].tolist() == [0, 0, 32]
    assert torch.equal(default_palette(21), p[:21]) and p[15].tolist() == [192, 128, 128]      # VOC's own 21 colours


def test_header_declares_the_entry_point_and_keeps_the_abi_version():
    with open(os.path.join(ROOT, "include", "ifseg_hip.h")) as f:
        header = f.read()
    assert re.search(r"^int ifseg_seg_render\(", header, re.M)
    assert re.search(r"#define\s+IFSEG_ABI_VERSION\s+21\b", header) and hip.ABI_VERSION == 21


def _no_library(monkeypatch):
    def fail():
        raise RuntimeError("the library was reached")
    monkeypatch.setattr(hip, "lib", fail)


def test_binding_refuses_before_it_launches(monkeypatch):
    _no_library(monkeypatch)
    labels, image, conf = _case(torch.uint8, 15)
    pal = default_palette(15)
    wide = torch.zeros(H, W, 4, dtype=torch.uint8)
    bad_calls = [
        dict(labels=labels.long()),                                                   # int64 labels
        dict(image=image.float()),                                                    # float image
        dict(image=wide[:, :, :3]),                                                   # a non-contiguous image
        dict(labels=labels.t().contiguous().t()),                                     # non-contiguous labels
        dict(image=image[:, :12].contiguous()),                                       # mismatched shapes
        dict(labels=labels[None], image=image),
        dict(boundary=5), dict(boundary=-1), dict(boundary=1.0),
        dict(opacity=1.5), dict(opacity=-0.01),
        dict(palette=pal[:0]),                                                        # an empty palette
        dict(palette=default_palette(512).repeat(2, 1)),                              # 1024 classes
        dict(palette=pal.int()),
        dict(boundary_color=(0, 0, 256)), dict(boundary_color=(1, 2)),
        dict(conf=conf.double()), dict(conf=conf[:, :12]),
        dict(out=image),                                                              # out aliasing the image
        dict(out=torch.zeros(H, W, 3)),
    ]
    for kw in bad_calls:
        args = dict(labels=labels, image=image, palette=pal)
        args.update(kw)
        with pytest.raises(AssertionError):
            hip.seg_render(**args)
    # out overlapping the labels, and overlapping the image by one byte
    buf = torch.zeros(H * W * 3 + H * W, dtype=torch.uint8)
    with pytest.raises(AssertionError, match="overlaps"):
        hip.seg_render(buf[H * W * 3 - 1:H * W * 3 - 1 + H * W].view(H, W), image, pal, out=buf[:H * W * 3].view(H, W, 3))
    two = torch.zeros(2 * H * W * 3 - 1, dtype=torch.uint8)
    with pytest.raises(AssertionError, match="overlaps"):
        hip.seg_render(labels, two[:H * W * 3].view(H, W, 3), pal, out=two[H * W * 3 - 1:].view(H, W, 3))
    # good arguments get as far as the library
    with pytest.raises(RuntimeError, match="the library was reached"):
        hip.seg_render(labels, image, pal, 0.3, 4, (1, 2, 3), conf=conf, out=torch.empty_like(image))
    assert [hip.render_alpha(o) for o in (0.0, 0.3, 0.5, 1.0)] == [0, 77, 128, 256]


def test_op_is_registered_with_a_fake_kernel():
    import ifseg_amd.ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    op = torch.ops.ifseg.seg_render
    with FakeTensorMode():
        lab = torch.empty(2, 9, 7, dtype=torch.int16, device="cuda")
        img = torch.empty(2, 9, 7, 3, dtype=torch.uint8, device="cuda")
        pal = torch.empty(300, 3, dtype=torch.uint8, device="cuda")
        conf = torch.empty(2, 9, 7, device="cuda")
        out = op(lab, img, pal, 0.5, 1, [255, 255, 255], None)
        assert out.shape == (2, 9, 7, 3) and out.dtype == torch.uint8 and out.is_cuda
        out = op(lab[0], img[0], pal, 1.0, 0, [0, 0, 0], conf[0])
        assert out.shape == (9, 7, 3) and out.dtype == torch.uint8
        for bad, what in (((lab.long(), img, pal, 0.5, 0, [0, 0, 0], None), "labels must be uint8 or int16"),
                          ((lab, img.float(), pal, 0.5, 0, [0, 0, 0], None), "image must be uint8"),
                          ((lab, img[:1], pal, 0.5, 0, [0, 0, 0], None), "image must be uint8"),
                          ((lab, img, pal[:0], 0.5, 0, [0, 0, 0], None), "palette must be uint8"),
                          ((lab, img, pal, 1.5, 0, [0, 0, 0], None), "opacity must be in"),
                          ((lab, img, pal, 0.5, 5, [0, 0, 0], None), "boundary must be in"),
                          ((lab, img, pal, 0.5, 1, [0, 0, 300], None), "boundary_color"),
                          ((lab, img, pal, 0.5, 1, [0, 0, 0], conf[0]), "conf must be float32")):
            with pytest.raises(Exception, match=what):
                op(*bad)
    meta = op(torch.empty(9, 7, dtype=torch.uint8, device="meta"), torch.empty(9, 7, 3, dtype=torch.uint8, device="meta"),
              torch.empty(15, 3, dtype=torch.uint8, device="meta"), 0.5, 0, [0, 0, 0], None)
    assert meta.shape == (9, 7, 3) and meta.dtype == torch.uint8 and meta.device.type == "meta"


class _Model(torch.nn.Linear):
    """as much of a model as the checks of render_raw look at"""

    def __init__(self):
        super().__init__(1, 1)
        self.cfg = type("Cfg", (), {"num_seg_tokens": 5, "patch_image_size": 128})()


def test_render_raw_refuses_before_it_launches(monkeypatch):
    _no_library(monkeypatch)
    monkeypatch.setattr(hip, "image_load", lambda *a, **k: (_ for _ in ()).throw(RuntimeError("image_load was reached")))
    names = [[31], [32], [33], [34], [35]]
    seg = Segmenter(_Model(), category_token_ids=names)
    im = [torch.zeros(60, 90, 3, dtype=torch.uint8)]
    with pytest.raises(ValueError, match="fade_by_conf"):
        Segmenter(_Model(), category_token_ids=names, crf_iters=2).render_raw(im, fade_by_conf=True)
    with pytest.raises(ValueError, match=r"palette must be a uint8 \[>= 5, 3\]"):
        seg.render_raw(im, palette=default_palette(4))
    with pytest.raises(ValueError, match="palette must be"):
        seg.render_raw(im, palette=default_palette(5).float())
    with pytest.raises(ValueError, match="opacity"):
        seg.render_raw(im, opacity=1.5)
    with pytest.raises(ValueError, match="boundary must be"):
        seg.render_raw(im, boundary=5)
    with pytest.raises(TypeError, match="return_probs"):
        seg.render_raw(im, return_probs=True)
    with pytest.raises(ValueError, match="segment_raw: every image must be a uint8 RGB"):
        seg.render_raw([im[0].float()])
    assert seg.render_raw([]) == [] and RenderResult._fields == ("picture", "labels", "conf")
