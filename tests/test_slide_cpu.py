"""CPU: the surface of sliding-window inference (imageio.slide_windows / plan_slide / image_load_windows_reference,
predict.slide_reference, Segmenter.segment_raw(slide=...), the bindings and torch.ops.ifseg.*_windows) and the premises of the
GPU tests in test_slide_gpu.py (exactness of the exact family; the 1 % cap of the general family)."""
import os
import re
import types

import pytest
import torch

import _slide_cases as C
from ifseg_amd import hip
from ifseg_amd import ops  # noqa: F401  (registers torch.ops.ifseg.*)
from ifseg_amd import imageio
from ifseg_amd.imageio import eval_size, image_load_reference, image_load_windows_reference, plan_slide, slide_windows
from ifseg_amd.predict import Segmenter, slide_reference, upsample_argmax_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------- the window rule
def _mmseg_windows(h_img, w_img, h_crop, w_crop, h_stride, w_stride):
    """mmseg's slide_inference loop, restated literally -> [(y1, y2, x1, x2)]"""
    h_grids = max(h_img - h_crop + h_stride - 1, 0) // h_stride + 1
    w_grids = max(w_img - w_crop + w_stride - 1, 0) // w_stride + 1
    out = []
    for h_idx in range(h_grids):
        for w_idx in range(w_grids):
            y1 = h_idx * h_stride
            x1 = w_idx * w_stride
            y2 = min(y1 + h_crop, h_img)
            x2 = min(x1 + w_crop, w_img)
            y1 = max(y2 - h_crop, 0)
            x1 = max(x2 - w_crop, 0)
            out.append((y1, y2, x1, x2))
    return out


RULE_CASES = [(512, 683, 512, 341), (64, 160, 64, 42), (100, 90, 64, 21), (40, 200, (48, 80), (30, 50)), (60, 90, (64, 96), 43),
              (1, 1, 1, 1), (7, 300, 16, 16), (131, 128, 128, 1), (640, 2560, 640, 426)]


@pytest.mark.parametrize("case", RULE_CASES)
def test_slide_windows_is_mmsegs_loop(case):
    oh, ow, crop, stride = case
    (c_h, c_w), (s_h, s_w) = imageio._pair(crop, "crop"), imageio._pair(stride, "stride")
    ys, xs, ch, cw = slide_windows(oh, ow, crop, stride)
    want = _mmseg_windows(oh, ow, c_h, c_w, s_h, s_w)
    assert [(y, y + ch, x, x + cw) for y in ys for x in xs] == want
    assert (ch, cw) == (min(c_h, oh), min(c_w, ow))
    # no pixel uncovered, the last window ends at the edge, the starts increase
    count = torch.zeros(oh, ow)
    for y1, y2, x1, x2 in want:
        count[y1:y2, x1:x2] += 1
    assert count.min() >= 1
    assert ys[-1] + ch == oh and xs[-1] + cw == ow and ys[0] == 0 and xs[0] == 0
    assert all(a < b for a, b in zip(ys, ys[1:])) and all(a < b for a, b in zip(xs, xs[1:]))


def test_slide_windows_by_hand():
    assert slide_windows(512, 683, 512, 341) == ([0], [0, 171], 512, 512)
    assert slide_windows(100, 90, 64, 21) == ([0, 21, 36], [0, 21, 26], 64, 64)
    assert slide_windows(40, 200, (48, 80), (30, 50)) == ([0], [0, 50, 100, 120], 40, 80)        # the short axis: one short window
    assert slide_windows(60, 90, (64, 96), 43) == ([0], [0], 60, 90)
    assert slide_windows(64, 64, 8, 8)[:2] == (list(range(0, 64, 8)),) * 2                       # 64 windows: the limit itself
    assert imageio.MAX_WINDOWS == hip.SLIDE_MAX_WINDOWS == 64


def test_slide_windows_refusals():
    with pytest.raises(ValueError, match="crop and stride must be >= 1"):
        slide_windows(64, 64, 32, 0)
    with pytest.raises(ValueError, match="crop and stride must be >= 1"):
        slide_windows(64, 64, (32, 0), 1)
    with pytest.raises(ValueError, match="a stride above the crop leaves pixels uncovered"):
        slide_windows(64, 64, 16, (16, 17))
    with pytest.raises(ValueError, match=r"9 x 8 windows .* at most 64"):
        slide_windows(72, 64, 8, 8)
    with pytest.raises(ValueError, match="an int or an \\(h, w\\) pair"):
        slide_windows(64, 64, (8, 8, 8), 8)


# ------------------------------------------------------------------------------------------------- the specifications
@pytest.mark.parametrize("shape", C.ONE_WINDOW_CASES)
def test_reference_with_one_covering_window_is_the_single_view_reference(shape):
    hp, wp, n, h, w = shape
    s = torch.randn(2, hp * wp, n, generator=torch.Generator().manual_seed(5))
    for dtype in (torch.float32, torch.float64):
        a = slide_reference(s[:, None], hp, wp, h, w, (h + 3, w), (h, 1), h, w, dtype)
        b = upsample_argmax_reference(s, hp, wp, h, w, dtype)
        assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_reference_by_hand():
    """two 1 x 1-patch windows of 4 pixels at stride 2 over 6 pixels: constant windows, the overlap is their mean"""
    s = torch.tensor([[[[1.0, 0.0]], [[3.0, 8.0]]]])                                             # [1, 2, 1, 2]
    lab, conf, probs = slide_reference(s, 1, 1, 1, 6, (1, 4), (1, 2), 1, 6)
    assert probs[0, 0, 0].tolist() == [1, 1, 2, 2, 3, 3] and probs[0, 1, 0].tolist() == [0, 0, 4, 4, 8, 8]
    assert lab[0, 0].tolist() == [0, 0, 1, 1, 1, 1] and conf[0, 0].tolist() == [1, 1, 4, 4, 8, 8]
    # the second stage: to 3 pixels, each the mean of a pair
    lab, conf, probs = slide_reference(s, 1, 1, 1, 6, (1, 4), (1, 2), 1, 3)
    assert probs[0, :, 0].tolist() == [[1, 2, 3], [0, 4, 8]]


@pytest.mark.parametrize("name", list(C.EXACT_CASES))
def test_exact_family_is_exact_in_fp32(name):
    B, hpw, wpw, n, oh, ow, crop, stride, h, w = C.EXACT_CASES[name]
    ys, xs, ch, cw = slide_windows(oh, ow, crop, stride)
    c_h, c_w = imageio._pair(crop, "crop")
    s_h, s_w = imageio._pair(stride, "stride")
    assert (ch, cw) == (16 * hpw, 16 * wpw) and (oh - ch) % s_h == 0 and (ow - cw) % s_w == 0
    assert 2 * s_h >= c_h and 2 * s_w >= c_w and (h, w) in ((oh, ow), (2 * oh, 2 * ow))
    s = C.exact_scores(name)
    a = slide_reference(s, hpw, wpw, oh, ow, crop, stride, h, w, torch.float32)
    b = slide_reference(s, hpw, wpw, oh, ow, crop, stride, h, w, torch.float64)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].double(), b[1]) and torch.equal(a[2].double(), b[2])


def test_general_family_margin_cap_holds():
    for case in C.GENERAL_CASES:
        hpw, wpw, n, oh, ow, crop, stride, h, w = case
        for softmaxed in (False, True):
            ref = C.reference(("general", case, softmaxed, 1), C.general_scores(case, 1, softmaxed), hpw, wpw, oh, ow, crop, stride, h, w)
            assert ref.e > 0 and ref.undecided_share <= C.MARGIN_CAP, (case, softmaxed, ref.e, ref.undecided_share)


def test_image_load_windows_reference_is_slices_of_image_load_reference():
    img = torch.randint(0, 256, (2, 50, 131, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(3))
    oh, ow, crop, stride = 64, 168, 64, 43
    ys, xs, ch, cw = slide_windows(oh, ow, crop, stride)
    assert (ys, xs, ch, cw) == ([0], [0, 43, 86, 104], 64, 64)
    for out_dtype in (torch.float32, torch.bfloat16):
        full = image_load_reference(img, oh, ow, out_dtype=out_dtype)[0]
        wins = image_load_windows_reference(img, oh, ow, crop, stride, out_dtype=out_dtype)
        assert wins.shape == (2 * 4, 3, 64, 64) and wins.dtype == out_dtype
        for b in range(2):
            for k, x in enumerate(xs):
                assert torch.equal(wins[b * 4 + k], full[b, :, :, x:x + 64])


# ------------------------------------------------------------------------------------------------- the plan
def test_plan_slide_is_pure_and_batches_windows_of_different_images():
    P = 64
    shapes = [(64, 160), (160, 64), (64, 64), (64, 160), (32, 48)]
    per_image, loads, forwards = plan_slide(shapes, P, P, 2 * P // 3, max_batch=3)
    assert [p[0] for p in per_image] == [eval_size(h, w, P) for h, w in shapes] == [(64, 160), (160, 64), (64, 64), (64, 160), (64, 96)]
    assert per_image[0][1:] == ([0], [0, 42, 84, 96], (64, 64)) and per_image[1][1:] == ([0, 42, 84, 96], [0], (64, 64))
    assert per_image[2][1:] == ([0], [0], (64, 64)) and per_image[4][1:] == ([0], [0, 32], (64, 64))
    # one load per distinct (source shape, size), in order of first appearance
    assert loads == [((64, 160), (64, 160), [0, 3]), ((160, 64), (160, 64), [1]), ((64, 64), (64, 64), [2]), ((32, 48), (64, 96), [4])]
    # every window runs at (64, 64): one size, windows of different images mixed freely, in (image, window) order
    order = [(i, k) for i, nw in enumerate((4, 4, 1, 4, 2)) for k in range(nw)]
    assert all(size == (64, 64) and 1 <= len(ik) <= 3 for size, ik in forwards)
    assert [ik for _, chunk in forwards for ik in chunk] == order
    assert [len(ik) for _, ik in forwards] == [3, 3, 3, 3, 3]
    # another ratio, another crop: two window sizes, each in chunks of its own
    per_image, loads, forwards = plan_slide([(64, 160), (20, 64)], P, (64, 96), 48, ratio=1.0, max_batch=8)
    assert [p[3] for p in per_image] == [(64, 96), (64, 96)]
    per_image, loads, forwards = plan_slide([(64, 160), (64, 64)], P, (64, 96), 48, max_batch=2)
    assert [p[3] for p in per_image] == [(64, 96), (64, 64)]
    assert forwards == [((64, 96), [(0, 0), (0, 1)]), ((64, 96), [(0, 2)]), ((64, 64), [(1, 0)])]
    with pytest.raises(ValueError, match="max_batch"):
        plan_slide(shapes, P, P, P, max_batch=0)
    with pytest.raises(ValueError, match="at most 64"):
        plan_slide([(64, 256)], P, 8, 4)


# ------------------------------------------------------------------------------------------------- refusals, by name
def _stub(upsample="probs"):
    model = types.SimpleNamespace(cfg=types.SimpleNamespace(num_seg_tokens=2, patch_image_size=64), training=False)
    return Segmenter(model, category_token_ids=[[1], [2]], upsample=upsample)


def test_segment_raw_and_evaluate_raw_refuse_before_any_launch():
    """the stub model has no parameters and no forward: a refusal that came later would fail in another way"""
    img, gt = torch.zeros(8, 8, 3, dtype=torch.uint8), torch.zeros(8, 8, dtype=torch.uint8)
    for call in (lambda **kw: _stub().segment_raw(img, **kw), lambda **kw: _stub().evaluate_raw(img, gt, **kw)):
        with pytest.raises(ValueError, match="slide takes a single view"):
            call(slide=True, flip=True)
        with pytest.raises(ValueError, match="slide takes a single view"):
            call(slide=(64, 42), scales=(0.5, 1.0))
        with pytest.raises(ValueError, match="a stride above the crop"):
            call(slide=(32, 33))
        with pytest.raises(ValueError, match="crop and stride must be >= 1"):
            call(slide=((32, 0), 8))
        with pytest.raises(ValueError, match=r"slide must be None, True or \(crop, stride\)"):
            call(slide=64)
        with pytest.raises(ValueError, match="at most 64"):
            call(slide=(4, 2))                                 # the 64 x 64 network image under 31 x 31 windows
    assert _stub().segment_raw([], slide=True) == []
    # logits are allowed with slide (one view)
    with pytest.raises(ValueError, match="slide takes a single view"):
        _stub("logits").segment_raw(img, slide=True, flip=True)


def test_bindings_refuse_before_they_launch():
    ok = torch.zeros(2, 2, 16, 5)                              # 64 x 96 under crop 64, stride 32: two windows
    geo = (4, 4, 64, 96, 64, 32)
    for bad in (ok.double(), ok.transpose(2, 3), ok[0], ok[:, :1]):
        with pytest.raises(AssertionError):
            hip.seg_predict_windows(bad, *geo, 64, 96)
    with pytest.raises(AssertionError):
        hip.seg_predict_windows(ok, 4, 3, 64, 96, 64, 32, 64, 96)                          # hpw * wpw != rows
    with pytest.raises(AssertionError, match="stride above the crop"):
        hip.seg_predict_windows(ok, 4, 4, 64, 96, 64, 65, 64, 96)
    with pytest.raises(AssertionError):
        hip.seg_predict_windows(ok, *geo, 0, 96)
    with pytest.raises(AssertionError):
        hip.seg_predict_windows(torch.zeros(1, 2, 16, 257), *geo, 64, 96, label_dtype=torch.uint8)
    with pytest.raises(AssertionError):
        hip.seg_score_windows(ok, *geo, torch.zeros(1, 64, 96, dtype=torch.uint8))         # another B
    with pytest.raises(AssertionError):
        hip.seg_score_windows(ok, *geo, torch.zeros(2, 64, 96, dtype=torch.int32))
    img = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(AssertionError, match="at most 64"):
        hip.image_load_windows(img, 72, 64, 8, 8)
    with pytest.raises(AssertionError):
        hip.image_load_windows(img.float(), 64, 64, 64, 42)
    with pytest.raises(AssertionError, match="device tensor required"):
        hip.image_load_windows(img, 64, 64, 64, 42)


# ------------------------------------------------------------------------------------------------- the ops
def test_ops_exist_and_refuse_on_fake_tensors():
    from torch._subclasses.fake_tensor import FakeTensorMode
    pw, sw, lw = torch.ops.ifseg.seg_predict_windows, torch.ops.ifseg.seg_score_windows, torch.ops.ifseg.image_load_windows
    with FakeTensorMode():
        s = torch.empty(2, 2, 16, 5, device="cuda")
        with pytest.raises(Exception, match="scores must be fp32"):
            pw(s.to(torch.bfloat16), 4, 4, 64, 96, [64, 64], [32, 32], 64, 96, False, False)
        with pytest.raises(Exception, match=r"scores.shape\[1\] = 2, the window rule gives 3 windows"):
            pw(s, 4, 4, 64, 128, [64, 64], [32, 32], 64, 96, False, False)
        with pytest.raises(Exception, match=r"scores.shape\[2\] = 16, expected hpw \* wpw = 12"):
            pw(s, 4, 3, 64, 96, [64, 64], [32, 32], 64, 96, False, False)
        with pytest.raises(Exception, match="a stride above the crop"):
            pw(s, 4, 4, 64, 96, [64, 64], [32, 65], 64, 96, False, False)
        with pytest.raises(Exception, match=r"crop and stride must be \(h, w\) pairs"):
            pw(s, 4, 4, 64, 96, [64], [32, 32], 64, 96, False, False)
        with pytest.raises(Exception, match="n = 513 classes"):
            pw(torch.empty(1, 2, 16, 513, device="cuda"), 4, 4, 64, 96, [64, 64], [32, 32], 64, 96, False, False)
        with pytest.raises(Exception, match="B \\* h \\* w < 2\\*\\*31"):
            pw(s, 4, 4, 64, 96, [64, 64], [32, 32], 2 ** 15, 2 ** 15, False, False)
        with pytest.raises(Exception, match="ground truth must be uint8 or int16"):
            sw(s, 4, 4, 64, 96, [64, 64], [32, 32], torch.empty(2, 64, 96, dtype=torch.int64, device="cuda"), True, False, False, False)
        with pytest.raises(Exception, match="for a batch of 2"):
            sw(s, 4, 4, 64, 96, [64, 64], [32, 32], torch.empty(1, 64, 96, dtype=torch.uint8, device="cuda"), True, False, False, False)
        img = torch.empty(2, 50, 131, 3, dtype=torch.uint8, device="cuda")
        with pytest.raises(Exception, match="images must be uint8"):
            lw(img.float(), 64, 168, [64, 64], [43, 43], [0.5] * 3, [0.5] * 3, False, torch.float32)
        with pytest.raises(Exception, match="at most 64"):
            lw(img, 64, 168, [8, 8], [4, 4], [0.5] * 3, [0.5] * 3, False, torch.float32)


def test_op_fake_kernel_shapes_and_dtypes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    pw, sw, lw = torch.ops.ifseg.seg_predict_windows, torch.ops.ifseg.seg_score_windows, torch.ops.ifseg.image_load_windows
    geo = (4, 4, 100, 90, [64, 64], [21, 21])                  # 9 windows
    with FakeTensorMode():
        for n, ldt in ((1, torch.uint8), (256, torch.uint8), (257, torch.int16), (512, torch.int16)):
            s = torch.empty(3, 9, 16, n, device="cuda")
            lab, conf, probs = pw(s, *geo, 133, 77, True, True)
            assert lab.shape == (3, 133, 77) and lab.dtype == ldt and lab.device.type == "cuda"
            assert conf.shape == (3, 133, 77) and conf.dtype == torch.float32
            assert probs.shape == (3, n, 133, 77) and probs.dtype == torch.float32
            lab, conf, probs = pw(s, *geo, 5, 1, False, False)
            assert lab.shape == (3, 5, 1) and conf.shape == (0,) and probs.shape == (0,)
            for gdt in (torch.uint8, torch.int16):
                gt = torch.empty(3, 37, 91, dtype=gdt, device="cuda")
                areas, tally, lab, conf, probs = sw(s, *geo, gt, True, False, True, False)
                assert areas.shape == (3, n) and areas.dtype == torch.int64 and tally.shape == (2,) and tally.dtype == torch.int64
                assert lab.shape == (0,) and lab.dtype == ldt and conf.shape == (3, 37, 91) and probs.shape == (0,)
                lab = sw(s, *geo, gt, False, True, False, True)[2]
                assert lab.shape == (3, 37, 91) and lab.dtype == ldt
        img = torch.empty(2, 50, 131, 3, dtype=torch.uint8, device="cuda")
        for dt in (torch.float32, torch.bfloat16):
            out = lw(img, 64, 168, [64, 64], [43, 43], [0.5] * 3, [0.5] * 3, False, dt)
            assert out.shape == (8, 3, 64, 64) and out.dtype == dt and out.device.type == "cuda"
        assert lw(img, 40, 200, [48, 80], [30, 50], [0.5] * 3, [0.5] * 3, True, torch.float32).shape == (8, 3, 40, 80)


def test_header_declares_the_entry_points_and_abi_is_still_21():
    hdr = open(os.path.join(ROOT, "include", "ifseg_hip.h")).read()
    assert int(re.search(r"#define\s+IFSEG_ABI_VERSION\s+(\d+)", hdr).group(1)) == hip.ABI_VERSION == 21
    assert "#define IFSEG_SLIDE_MAX_WINDOWS 64" in hdr
    assert "int ifseg_image_load_windows(const void* images, int B, int H0, int W0, int oh, int ow, int crop_h, int crop_w" in hdr
    assert "int ifseg_seg_predict_windows(const float* scores, int B, int hpw, int wpw, int n, int oh, int ow, int crop_h" in hdr
    assert "int ifseg_seg_score_windows(const float* scores, int B, int hpw, int wpw, int n, int oh, int ow, int crop_h" in hdr
    assert "int ifseg_seg_predict_windows_staging(int max_bytes);" in hdr
