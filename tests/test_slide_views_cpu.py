"""CPU: the surface of multi-scale + flip over sliding windows (predict.slide_views_reference, imageio.plan_slide_views, the
`flip` keyword of image_load_windows_reference, Segmenter(slide_views=True), the bindings and torch.ops.ifseg.*_slide_views) and
the premises of the GPU tests in test_slide_views_gpu.py (exactness of the exact family; the 1 % cap of the general family)."""
import os
import re
import types

import pytest
import torch
import torch.nn.functional as F

import _slide_cases as SC
import _slide_views_cases as C
from ifseg_amd import hip
from ifseg_amd import ops  # noqa: F401  (registers torch.ops.ifseg.*)
from ifseg_amd.imageio import (eval_size, image_load_reference, image_load_windows_reference, plan_slide_views, slide_windows,
                               view_list)
from ifseg_amd.predict import Segmenter, slide_reference, slide_views_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------- the specification
def _mmseg_aug_test(views, h_crop, w_crop, h_stride, w_stride, ori_shape, dtype):
    """mmseg's EncoderDecoder.aug_test over inference(mode='slide'), restated in plain torch: `views` is a list of
    (crop_logits(y1, y2, x1, x2) -> [B, n, y2 - y1, x2 - x1], (h_img, w_img), flip) -> (seg_pred, mean of the softmaxes)"""
    total = None
    for crop_logits, (h_img, w_img), flip in views:
        h_grids = max(h_img - h_crop + h_stride - 1, 0) // h_stride + 1
        w_grids = max(w_img - w_crop + w_stride - 1, 0) // w_stride + 1
        preds = count_mat = None
        for h_idx in range(h_grids):
            for w_idx in range(w_grids):
                y1 = h_idx * h_stride
                x1 = w_idx * w_stride
                y2 = min(y1 + h_crop, h_img)
                x2 = min(x1 + w_crop, w_img)
                y1 = max(y2 - h_crop, 0)
                x1 = max(x2 - w_crop, 0)
                crop_seg_logit = crop_logits(h_idx * w_grids + w_idx, y2 - y1, x2 - x1)
                if preds is None:
                    preds = crop_seg_logit.new_zeros(crop_seg_logit.shape[0], crop_seg_logit.shape[1], h_img, w_img)
                    count_mat = crop_seg_logit.new_zeros(1, 1, h_img, w_img)
                preds += F.pad(crop_seg_logit, (int(x1), int(preds.shape[3] - x2), int(y1), int(preds.shape[2] - y2)))
                count_mat[:, :, y1:y2, x1:x2] += 1
        assert (count_mat == 0).sum() == 0
        seg_logit = preds / count_mat
        seg_logit = F.interpolate(seg_logit, size=ori_shape, mode="bilinear", align_corners=False)     # rescale=True
        output = F.softmax(seg_logit, dim=1)
        if flip:
            output = output.flip(dims=(3,))
        total = output if total is None else total + output
    total = total / len(views)
    return total.argmax(dim=1), total


@pytest.mark.parametrize("case", [C.GENERAL_CASES[0], C.GENERAL_CASES[3], C.GENERAL_CASES[5]], ids=["ade", "nonsquare", "one"])
def test_reference_is_mmsegs_aug_test_over_slide_inference(case):
    hpw, wpw, n, crop, stride, h, w, planes = case
    views, crop, stride, h, w = C.general_views(case, 4, True, batch=2)
    (c_h, c_w), (s_h, s_w) = (crop, crop) if isinstance(crop, int) else crop, (stride, stride) if isinstance(stride, int) else stride

    def head(scores):
        # the decode head's logits of one crop, resized to the crop as encode_decode does
        return lambda k, ch, cw: F.interpolate(scores[:, k].double().transpose(1, 2).reshape(scores.shape[0], n, hpw, wpw),
                                               size=(ch, cw), mode="bilinear", align_corners=False)

    want_lab, want = _mmseg_aug_test([(head(s), (oh, ow), flip) for s, _, _, oh, ow, flip in views], c_h, c_w, s_h, s_w, (h, w),
                                     torch.float64)
    lab, conf, probs = slide_views_reference(views, crop, stride, h, w, True)
    # the same operations up to the place of the division by K and of the flip (a permutation in front of a pixel-wise softmax)
    assert (probs - want).abs().max().item() < 1e-15
    assert torch.equal(lab, want_lab) and torch.equal(conf, probs.amax(1))


def test_one_unflipped_linear_view_is_slide_reference():
    for case in SC.GENERAL_CASES[1:3]:
        hpw, wpw, n, oh, ow, crop, stride, h, w = case
        s = SC.general_scores(case, 2, True, batch=2)
        for dtype in (torch.float32, torch.float64):
            a = slide_views_reference([(s, hpw, wpw, oh, ow, False)], crop, stride, h, w, False, dtype)
            b = slide_reference(s, hpw, wpw, oh, ow, crop, stride, h, w, dtype)
            assert all(torch.equal(x, y) for x, y in zip(a, b))
        # a flipped view is the unflipped result mirrored; softmax is per pixel over the classes
        a = slide_views_reference([(s, hpw, wpw, oh, ow, True)], crop, stride, h, w, True)[2]
        assert torch.equal(a, b[2].flip(-1).softmax(1))


@pytest.mark.parametrize("K", C.EXACT_VIEWS)
@pytest.mark.parametrize("name", list(SC.EXACT_CASES))
def test_exact_family_is_exact_in_fp32_and_independent_of_view_order(name, K):
    views, crop, stride, h, w = C.exact_views(name, K)
    assert [v[5] for v in views] == [bool(k % 2) for k in range(K)]
    a = slide_views_reference(views, crop, stride, h, w, False, torch.float32)
    b = slide_views_reference(views, crop, stride, h, w, False, torch.float64)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].double(), b[1]) and torch.equal(a[2].double(), b[2])
    c = slide_views_reference(views[::-1], crop, stride, h, w, False, torch.float32)
    assert all(torch.equal(x, y) for x, y in zip(a, c))
    # fresh scores per view: the views differ
    assert not torch.equal(views[0][0], views[1][0])


@pytest.mark.parametrize("softmax", [False, True], ids=["linear", "softmax"])
@pytest.mark.parametrize("case", C.GENERAL_CASES, ids=[str(i) for i in range(len(C.GENERAL_CASES))])
def test_general_family_margin_cap_holds(case, softmax):
    for seed in C.SEEDS:
        ref = C.reference(("general", str(case), softmax, seed), *C.general_views(case, seed, softmax), softmax)
        print(case[:7], softmax, seed, "e = %.2e, undecided %.4f %%" % (ref.e, 100 * ref.undecided_share))
        assert ref.e > 0 and ref.undecided_share <= C.MARGIN_CAP, (case, softmax, seed, ref.e, ref.undecided_share)
        assert not ((ref.labels32 != ref.labels) & ref.decided).any()
    ref = C.reference(("batch",), *C.general_views(C.BATCH_CASE[1], 11, True, batch=C.BATCH_CASE[0]), True)
    assert ref.e > 0 and ref.undecided_share <= C.MARGIN_CAP


def test_general_cases_are_what_the_limits_allow():
    for hpw, wpw, n, crop, stride, h, w, planes in C.GENERAL_CASES:
        assert 1 <= len(planes) <= 16 and n <= 512
        assert all(SC.n_windows(oh, ow, crop, stride) <= 64 for oh, ow, _ in planes)
    assert len(C.GENERAL_CASES[2][7]) == 16 and max(SC.n_windows(oh, ow, 32, 21) for oh, ow, _ in C.GENERAL_CASES[2][7]) == 40


def test_image_load_windows_reference_flip_is_slices_of_the_mirrored_image():
    img = torch.randint(0, 256, (2, 48, 100, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(3))
    oh, ow, crop, stride = 64, 133, 64, 42
    ys, xs, ch, cw = slide_windows(oh, ow, crop, stride)
    assert (ys, xs) == ([0], [0, 42, 69])                      # not symmetric: mirrored windows are not flipped windows
    full = image_load_reference(img, oh, ow)[0]
    wins = image_load_windows_reference(img, oh, ow, crop, stride, flip=True)
    plain = image_load_windows_reference(img, oh, ow, crop, stride)
    assert torch.equal(plain, image_load_windows_reference(img, oh, ow, crop, stride, flip=False))
    for b in range(2):
        for k, x in enumerate(xs):
            assert torch.equal(wins[b * 3 + k], full[b].flip(-1)[:, :, x:x + 64])
    assert not torch.equal(wins[1], plain[1].flip(-1))


# ------------------------------------------------------------------------------------------------- the plan
def test_plan_slide_views_is_pure_and_batches_across_views():
    P = 64
    shapes = [(64, 160), (160, 64), (64, 160)]
    args = (shapes, P, P, 2 * P // 3, (1.0, 1.5), True, 5)
    views, per_image, loads, forwards = plan_slide_views(*args)
    assert plan_slide_views(*args) == (views, per_image, loads, forwards)
    assert views == view_list((1.0, 1.5), True) == [(1.0, False), (1.0, True), (1.5, False), (1.5, True)]
    assert [[p[0] for p in pv] for pv in per_image] == [[eval_size(h, w, P, r) for r, _ in views] for h, w in shapes]
    assert per_image[0][0] == ((64, 160), [0], [0, 42, 84, 96], (64, 64)) and per_image[0][1] == per_image[0][0]
    assert per_image[0][2] == ((96, 240), [0, 32], [0, 42, 84, 126, 168, 176], (64, 64))
    # one load per distinct (source shape, size, flip), in order of first appearance
    assert loads == [((64, 160), (64, 160), False, [0, 2]), ((64, 160), (64, 160), True, [0, 2]),
                     ((64, 160), (96, 240), False, [0, 2]), ((64, 160), (96, 240), True, [0, 2]),
                     ((160, 64), (160, 64), False, [1]), ((160, 64), (160, 64), True, [1]),
                     ((160, 64), (240, 96), False, [1]), ((160, 64), (240, 96), True, [1])]
    # every window of every view and image runs at (64, 64): one size, full batches across views and images
    order = [(i, v, k) for i in range(3) for v, nw in enumerate((4, 4, 12, 12)) for k in range(nw)]
    assert all(size == (64, 64) for size, _ in forwards)
    assert [ivk for _, chunk in forwards for ivk in chunk] == order
    assert [len(c) for _, c in forwards] == [5] * 19 + [1]
    assert any(len({v for _, v, _ in c}) > 1 for _, c in forwards) and any(len({i for i, _, _ in c}) > 1 for _, c in forwards)
    # ratios that give one size share a load; a short axis gives a second window size with chunks of its own
    views, per_image, loads, forwards = plan_slide_views([(64, 160)], P, P, 42, (0.5, 1.0), False, 8)
    assert [p[3] for p in per_image[0]] == [(32, 64), (64, 64)]
    assert forwards == [((32, 64), [(0, 0, 0), (0, 0, 1)]), ((64, 64), [(0, 1, 0), (0, 1, 1), (0, 1, 2), (0, 1, 3)])]
    with pytest.raises(ValueError, match="max_batch"):
        plan_slide_views(shapes, P, P, P, max_batch=0)
    with pytest.raises(ValueError, match="at most 64"):
        plan_slide_views([(64, 64)], P, 16, 8, (1.0, 2.0))     # the second view: 15 x 15 windows
    with pytest.raises(ValueError, match="at most 16"):
        plan_slide_views(shapes, P, P, P, [1.0 + 0.1 * i for i in range(9)], True)


# ------------------------------------------------------------------------------------------------- refusals, by name
def _stub(**kw):
    model = types.SimpleNamespace(cfg=types.SimpleNamespace(num_seg_tokens=2, patch_image_size=64), training=False)
    return Segmenter(model, category_token_ids=[[1], [2]], **kw)


def test_slide_views_segmenter_refuses_before_any_launch():
    """the stub model has no parameters and no forward: a refusal that came later would fail in another way"""
    img, gt = torch.zeros(8, 8, 3, dtype=torch.uint8), torch.zeros(8, 8, dtype=torch.uint8)
    for upsample in ("probs", "logits"):
        seg = _stub(upsample=upsample, slide_views=True)
        for call in (lambda **kw: seg.segment_raw(img, **kw), lambda **kw: seg.evaluate_raw(img, gt, **kw)):
            with pytest.raises(ValueError, match="18 views .* at most 16"):
                call(slide=True, scales=[1.0 + 0.1 * i for i in range(9)], flip=True)
            with pytest.raises(ValueError, match="at most 64"):
                call(slide=(8, 4), scales=(0.5, 1.0), flip=True)       # the 64 x 64 view under 15 x 15 windows
            with pytest.raises(ValueError, match="a stride above the crop"):
                call(slide=(32, 33), flip=True)
            with pytest.raises(ValueError, match="crop and stride must be >= 1"):
                call(slide=((32, 0), 8), scales=(1.0, 1.5))
            with pytest.raises(ValueError, match=r"slide must be None, True or \(crop, stride\)"):
                call(slide=64, flip=True)
        assert seg.segment_raw([], slide=True, flip=True) == []
    # without slide the opt-in changes nothing: several views still need upsample="probs"
    with pytest.raises(ValueError, match="views need upsample='probs'"):
        _stub(upsample="logits", slide_views=True).segment_raw(img, flip=True)
    # and without the opt-in the refusal is today's
    with pytest.raises(ValueError, match="slide takes a single view"):
        _stub().segment_raw(img, slide=True, flip=True)


def test_bindings_refuse_before_they_launch():
    ok = torch.zeros(2, 2, 16, 5)                              # 64 x 96 under crop 64, stride 32: two windows
    view = (ok, 4, 4, 64, 96, False)
    for bad in (ok.double(), ok.transpose(2, 3), ok[0], ok[:, :1]):
        with pytest.raises(AssertionError):
            hip.seg_predict_slide_views([(bad,) + view[1:]], 64, 32, 64, 96, False)
    with pytest.raises(AssertionError):
        hip.seg_predict_slide_views([], 64, 32, 64, 96, False)
    with pytest.raises(AssertionError):
        hip.seg_predict_slide_views([view] * 17, 64, 32, 64, 96, False)
    with pytest.raises(AssertionError):
        hip.seg_predict_slide_views([view, (ok[:1], 4, 4, 64, 96, True)], 64, 32, 64, 96, True)       # another B
    with pytest.raises(AssertionError, match="stride above the crop"):
        hip.seg_predict_slide_views([view], 64, 65, 64, 96, False)
    with pytest.raises(AssertionError):
        hip.seg_predict_slide_views([view], 64, 32, 0, 96, False)
    with pytest.raises(AssertionError):
        hip.seg_score_slide_views([view], 64, 32, torch.zeros(1, 64, 96, dtype=torch.uint8), False)   # another B
    with pytest.raises(AssertionError):
        hip.seg_score_slide_views([view], 64, 32, torch.zeros(2, 64, 96, dtype=torch.int32), True)
    with pytest.raises(AssertionError, match="device tensor required"):
        hip.image_load_windows(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), 64, 64, 64, 42, flip=True)


# ------------------------------------------------------------------------------------------------- the ops
def test_ops_exist_refuse_and_shape_their_fake_outputs():
    from torch._subclasses.fake_tensor import FakeTensorMode
    pv, sv = torch.ops.ifseg.seg_predict_slide_views, torch.ops.ifseg.seg_score_slide_views
    with FakeTensorMode():
        s = torch.empty(2, 2, 16, 5, device="cuda")
        t = torch.empty(2, 3, 16, 5, device="cuda")            # 64 x 128: three windows
        geo = ([4, 4], [4, 4], [64, 64], [96, 128], [False, True], [64, 64], [32, 32])
        with pytest.raises(Exception, match="scores must be fp32"):
            pv([s.to(torch.bfloat16), t], *geo, 64, 96, True, False, False)
        with pytest.raises(Exception, match=r"view 1: scores.shape\[1\] = 2, the window rule gives 3 windows"):
            pv([s, s], *geo, 64, 96, True, False, False)
        with pytest.raises(Exception, match="all views share B and n"):
            pv([s, t[:1]], *geo, 64, 96, True, False, False)
        with pytest.raises(Exception, match="one of each per view"):
            pv([s, t], [4], *geo[1:], 64, 96, True, False, False)
        with pytest.raises(Exception, match="17 views"):
            pv([s] * 17, *([x[0]] * 17 for x in geo[:5]), *geo[5:], 64, 96, True, False, False)
        with pytest.raises(Exception, match="a stride above the crop"):
            pv([s, t], *geo[:6], [32, 65], 64, 96, True, False, False)
        with pytest.raises(Exception, match="ground truth must be uint8 or int16"):
            sv([s, t], *geo, torch.empty(2, 64, 96, dtype=torch.int64, device="cuda"), True, True, False, False, False)
        with pytest.raises(Exception, match="for a batch of 2"):
            sv([s, t], *geo, torch.empty(1, 64, 96, dtype=torch.uint8, device="cuda"), True, True, False, False, False)
        for n, ldt in ((1, torch.uint8), (256, torch.uint8), (257, torch.int16)):
            a, b = torch.empty(3, 2, 16, n, device="cuda"), torch.empty(3, 3, 16, n, device="cuda")
            lab, conf, probs = pv([a, b], *geo, 37, 91, True, True, True)
            assert lab.shape == (3, 37, 91) and lab.dtype == ldt and lab.device.type == "cuda"
            assert conf.shape == (3, 37, 91) and probs.shape == (3, n, 37, 91) and probs.dtype == torch.float32
            lab, conf, probs = pv([a, b], *geo, 5, 1, False, False, False)
            assert lab.shape == (3, 5, 1) and conf.shape == (0,) and probs.shape == (0,)
            gt = torch.empty(3, 37, 91, dtype=torch.int16, device="cuda")
            areas, tally, lab, conf, probs = sv([a, b], *geo, gt, True, True, False, True, False)
            assert areas.shape == (3, n) and areas.dtype == torch.int64 and tally.shape == (2,)
            assert lab.shape == (0,) and lab.dtype == ldt and conf.shape == (3, 37, 91) and probs.shape == (0,)


def test_header_declares_the_entry_points_and_abi_is_still_21():
    hdr = open(os.path.join(ROOT, "include", "ifseg_hip.h")).read()
    assert int(re.search(r"#define\s+IFSEG_ABI_VERSION\s+(\d+)", hdr).group(1)) == hip.ABI_VERSION == 21
    assert "int ifseg_seg_predict_slide_views(const ifseg_slide_view* views, int K, int B, int n, int crop_h, int crop_w" in hdr
    assert "int ifseg_seg_score_slide_views(const ifseg_slide_view* views, int K, int B, int n, int crop_h, int crop_w" in hdr
    assert "int ifseg_seg_predict_slide_views_staging(int max_bytes);" in hdr
    assert "int ifseg_image_load_windows_mirrored(const void* images, int B, int H0, int W0, int oh, int ow, int crop_h" in hdr
    assert "} ifseg_slide_view;" in hdr
