"""CPU: the surface of multi-scale + flip inference (imageio.eval_size / plan_views, predict.upsample_views_reference,
Segmenter.segment_raw(scales, flip), hip.seg_predict_views, torch.ops.ifseg.seg_predict_views) and the premises of the GPU
tests in test_predict_views_gpu.py (exactness of the exact family; the 1 % cap of the general family)."""
import os
import re
import types

import pytest
import torch

import _predict_cases as PC
import _predict_views_cases as C
from ifseg_amd import hip
from ifseg_amd import ops  # noqa: F401  (registers torch.ops.ifseg.*)
from ifseg_amd.imageio import eval_size, plan_groups, plan_views, view_list
from ifseg_amd.predict import Segmenter, upsample_argmax_reference, upsample_views_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------- sizes
def test_eval_size_ratio_one_is_the_old_rule():
    for P in (16, 128, 384, 512):
        for h, w in [(60, 90), (90, 60), (64, 64), (1, 1), (1, 5000), (5000, 3), (512, 683), (683, 512), (375, 500), (33, 31),
                     (2048, 2049), (100, 1000), (7, 3000)]:
            s = min(4 * P / max(h, w), P / min(h, w))
            old = (int(h * s + 0.5), int(w * s + 0.5))
            assert eval_size(h, w, P) == old == eval_size(h, w, P, 1.0) == eval_size(h, w, P, ratio=1)


def test_eval_size_ratios_by_hand():
    """mmseg: the pair is (int(4 P r), int(P r)), then rescale_size: s = min(long / max(h, w), short / min(h, w)), int(x s + 0.5)"""
    assert eval_size(512, 683, 512, 0.5) == (256, 342)             # (1024, 256): s = 0.5, 341.5 + 0.5
    assert eval_size(512, 683, 512, 1.5) == (768, 1025)            # (3072, 768): s = 1.5, 1024.5 + 0.5
    assert eval_size(512, 683, 512, 1.75) == (896, 1195)           # (3584, 896): s = 1.75, 1195.25 + 0.5
    assert eval_size(100, 1000, 128, 0.5) == (26, 256)             # (256, 64): the LONG side binds, s = 0.256, 25.6 + 0.5
    assert eval_size(50, 80, 100, 1.75) == (175, 280)              # (700, 175): s = 3.5
    assert eval_size(44, 44, 30, 0.75) == (22, 22)                 # int(22.5) = 22 comes first: s = 0.5, not 23
    for bad in (0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="ratio must be > 0"):
            eval_size(10, 10, 16, bad)
    with pytest.raises(ValueError, match="is below 1"):
        eval_size(10, 10, 16, 0.05)


# ------------------------------------------------------------------------------------------------- the specification
def test_reference_with_one_unflipped_view_is_the_single_view_reference():
    s = PC.general_scores((4, 6, 15, 37, 91), 3, False, batch=2)
    for dt in (torch.float32, torch.float64):
        a, b = upsample_views_reference([(s, 4, 6, False)], 37, 91, dt), upsample_argmax_reference(s, 4, 6, 37, 91, dt)
        assert all(torch.equal(x, y) for x, y in zip(a, b)) and a[2].dtype == dt


def test_reference_flip_order_and_mean_by_hand():
    # one class on a 1 x 2 grid to 1 x 2: the identity resize, so a flipped view is its grid reversed
    s = torch.tensor([[[1.0], [3.0]]])
    lab, conf, probs = upsample_views_reference([(s, 1, 2, True)], 1, 2)
    assert probs.tolist() == [[[[3.0, 1.0]]]] and lab.tolist() == [[[0, 0]]] and conf.tolist() == [[[3.0, 1.0]]]
    # the flip comes BEFORE the resize: 1 x 2 -> 1 x 4 of the reversed grid
    up = upsample_views_reference([(s, 1, 2, True)], 1, 4)[2]
    assert up.flatten().tolist() == [3.0, 2.5, 1.5, 1.0]
    # the mean of four views, two classes; ties name the first class
    t = torch.tensor([[[0.0, 6.0], [6.0, 0.0]]])
    lab, conf, probs = upsample_views_reference([(t, 1, 2, False), (t, 1, 2, True), (t, 1, 2, False), (t, 1, 2, False)], 1, 2)
    assert torch.equal(probs, torch.tensor([[[[1.5, 4.5]], [[4.5, 1.5]]]], dtype=torch.float64))
    assert lab.tolist() == [[[1, 0]]] and conf.tolist() == [[[4.5, 4.5]]]
    assert upsample_views_reference([(t, 1, 2, False), (t, 1, 2, True)], 1, 2)[0].tolist() == [[[0, 0]]]


# ------------------------------------------------------------------------------------------------- premises of the GPU tests
@pytest.mark.parametrize("K", C.EXACT_KS)
@pytest.mark.parametrize("shape", C.EXACT_SHAPES)
def test_exact_family_is_exact_in_fp32(shape, K):
    B, gh, gw, n = shape
    views = C.exact_views(shape, K)
    assert len(views) == K
    if K == 4:
        assert {(hp, wp) for _, hp, wp, _ in views} >= {(gh // 2, gw // 2), (gh, gw), (2 * gh, 2 * gw)}
        assert {f for *_, f in views} == {False, True}
    l32, c32, p32 = upsample_views_reference(views, 16 * gh, 16 * gw, torch.float32)
    l64, c64, p64 = upsample_views_reference(views, 16 * gh, 16 * gw, torch.float64)
    assert torch.equal(p32.double(), p64) and torch.equal(l32, l64) and torch.equal(c32.double(), c64)
    top2 = p64.topk(2, dim=1).values
    ties = (top2[:, 0] == top2[:, 1]).float().mean().item()
    print(shape, K, "exact ties: %.2f %% of the pixels" % (100 * ties))
    assert ties > 0 or K > 1          # the first-maximum rule is exercised (ties get rare as the views multiply)


def _general_cases():
    for K, n, h, w in C.GENERAL_CASES:
        for softmaxed in (False, True):
            for seed in C.SEEDS:
                yield ("general", K, n, h, w, softmaxed, seed), C.general_views(K, n, seed, softmaxed), h, w
    K, n, h, w, grids = C.DIRECT_CASE
    yield ("direct",), C.general_views(K, n, 1, False, batch=2, grids=grids), h, w
    B, K, n, h, w = C.BATCH_CASE
    yield ("batch",), C.general_views(K, n, 11, True, batch=B), h, w


def test_general_family_margin_cap_holds():
    """the GPU tests leave out the pixels whose top-2 margin is below 32 e: they must be at most 1 % of every case"""
    for key, views, h, w in _general_cases():
        ref = C.reference(key, views, h, w)
        print(key, "e = %.2e, undecided %.3f %%" % (ref.e, 100 * ref.undecided_share))
        assert 0 < ref.e < 1e-4
        assert ref.undecided_share <= PC.MARGIN_CAP


# ------------------------------------------------------------------------------------------------- the view plan
def test_view_list_order_and_refusals():
    assert view_list() == [(1.0, False)]
    assert view_list((0.5, 1.0), flip=True) == [(0.5, False), (0.5, True), (1.0, False), (1.0, True)]
    assert view_list((1.5, 0.5)) == [(1.5, False), (0.5, False)]                     # the order given, not sorted
    assert len(view_list([1.0] * 16)) == 16 and len(view_list([1.0] * 8, flip=True)) == 16
    for bad in ((), (1.0, 0.0), (-0.5,)):
        with pytest.raises(ValueError, match="non-empty sequence of ratios > 0"):
            view_list(bad)
    with pytest.raises(ValueError, match="17 views"):
        view_list([1.0] * 17)
    with pytest.raises(ValueError, match=r"18 views \(9 scales x 2 flips\)"):
        view_list([1.0] * 9, flip=True)


def test_plan_views_is_pure_and_batches_by_size():
    shapes = [(60, 90), (64, 64), (60, 90), (30, 45)]
    views, loads, forwards = plan_views(shapes, 128, scales=(0.5, 1.0), flip=True, max_batch=8)
    assert views == [(0.5, False), (0.5, True), (1.0, False), (1.0, True)]
    # one load per (source shape, network size), in order of first appearance; the mirrored view loads nothing
    assert loads == [((60, 90), (64, 96), [0, 2]), ((60, 90), (128, 192), [0, 2]), ((64, 64), (64, 64), [1]),
                     ((64, 64), (128, 128), [1]), ((30, 45), (64, 96), [3]), ((30, 45), (128, 192), [3])]
    # one size after the other; mirrored and plain views of a size share the forward, in (image, view) order
    assert forwards == [((64, 96), [(0, 0), (0, 1), (2, 0), (2, 1), (3, 0), (3, 1)]),
                        ((128, 192), [(0, 2), (0, 3), (2, 2), (2, 3), (3, 2), (3, 3)]),
                        ((64, 64), [(1, 0), (1, 1)]), ((128, 128), [(1, 2), (1, 3)])]
    _, _, f2 = plan_views(shapes, 128, scales=(0.5, 1.0), flip=True, max_batch=4)
    assert f2[:2] == [((64, 96), [(0, 0), (0, 1), (2, 0), (2, 1)]), ((64, 96), [(3, 0), (3, 1)])]
    assert [s for s, _ in f2] == [(64, 96)] * 2 + [(128, 192)] * 2 + [(64, 64), (128, 128)]       # every size once, in a row
    # every view of every image runs once
    assert sorted(iv for _, ivs in f2 for iv in ivs) == [(i, v) for i in range(4) for v in range(4)]
    # two ratios of one size share the load; the single view is plan_groups
    _, l3, f3 = plan_views([(64, 64)], 128, scales=(1.0, 1.0))
    assert l3 == [((64, 64), (128, 128), [0])] and f3 == [((128, 128), [(0, 0), (0, 1)])]
    shapes7 = [(60, 90), (90, 60), (64, 64), (60, 90), (30, 45), (120, 180), (60, 90)]
    _, l1, f1 = plan_views(shapes7, 128, max_batch=2)
    g_loads, g_forwards = plan_groups(shapes7, 128, max_batch=2)
    assert l1 == g_loads and [(s, [i for i, _ in iv]) for s, iv in f1] == g_forwards
    assert plan_views([], 128, (0.5,), True) == ([(0.5, False), (0.5, True)], [], [])
    with pytest.raises(ValueError, match="max_batch"):
        plan_views(shapes, 128, max_batch=0)
    with pytest.raises(ValueError, match="17 views"):
        plan_views(shapes, 128, scales=[1.0] * 17)


# ------------------------------------------------------------------------------------------------- refusals, by name
def _stub(upsample="probs"):
    model = types.SimpleNamespace(cfg=types.SimpleNamespace(num_seg_tokens=2, patch_image_size=64), training=False)
    return Segmenter(model, category_token_ids=[[1], [2]], upsample=upsample)


def test_segment_raw_refuses_before_any_launch():
    """the stub model has no parameters and no forward: a refusal that came later would fail in another way"""
    img = torch.zeros(8, 8, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="2 views need upsample='probs'"):
        _stub("logits").segment_raw(img, flip=True)
    with pytest.raises(ValueError, match="3 views need upsample='probs'"):
        _stub("logits").segment_raw(img, scales=(0.5, 1.0, 1.5))
    for bad in ((), (0.0,), (1.0, -1.0)):
        with pytest.raises(ValueError, match="non-empty sequence of ratios > 0"):
            _stub().segment_raw(img, scales=bad)
    with pytest.raises(ValueError, match=r"18 views \(9 scales x 2 flips\).*at most 16"):
        _stub().segment_raw(img, scales=[1.0] * 9, flip=True)
    assert _stub().segment_raw([], scales=(0.5, 1.0), flip=True) == []
    with pytest.raises(ValueError, match=r"uint8 RGB \[H, W, 3\]"):
        _stub().segment_raw([torch.zeros(8, 8, 3)], flip=True)


def test_binding_refuses_before_it_launches():
    ok = torch.zeros(2, 6, 5)
    for bad in (ok.double(), ok.transpose(1, 2), ok[0]):
        with pytest.raises(AssertionError):
            hip.seg_predict_views([(bad, 2, 3, False)], 32, 48)
    with pytest.raises(AssertionError):
        hip.seg_predict_views([(ok, 2, 2, False)], 32, 48)                                   # hp * wp != rows
    with pytest.raises(AssertionError):
        hip.seg_predict_views([(ok, 2, 3, False), (torch.zeros(1, 6, 5), 2, 3, True)], 32, 48)   # another B
    with pytest.raises(AssertionError):
        hip.seg_predict_views([(ok, 2, 3, False), (torch.zeros(2, 6, 4), 2, 3, True)], 32, 48)   # another n
    with pytest.raises(AssertionError):
        hip.seg_predict_views([], 32, 48)
    with pytest.raises(AssertionError):
        hip.seg_predict_views([(ok, 2, 3, False)] * 17, 32, 48)
    with pytest.raises(AssertionError):
        hip.seg_predict_views([(torch.zeros(1, 1, 513), 1, 1, False)], 4, 4)
    with pytest.raises(AssertionError):
        hip.seg_predict_views([(torch.zeros(1, 1, 257), 1, 1, False)], 4, 4, label_dtype=torch.uint8)
    with pytest.raises(AssertionError):
        hip.seg_predict_views([(ok, 2, 3, False)], 0, 48)


def test_op_refusals_on_fake_tensors():
    from torch._subclasses.fake_tensor import FakeTensorMode
    op = torch.ops.ifseg.seg_predict_views
    with FakeTensorMode():
        s = torch.empty(2, 6, 5, device="cuda")
        t = torch.empty(2, 24, 5, device="cuda")
        with pytest.raises(Exception, match="scores must be fp32.*view 1"):
            op([s, t.to(torch.bfloat16)], [2, 4], [3, 6], [False, True], 32, 48, False, False)
        with pytest.raises(Exception, match=r"n = 513 classes, the kernel takes 1 .. FUSED_MAX_CLASSES = 512"):
            op([torch.empty(1, 6, 513, device="cuda")], [2], [3], [False], 32, 48, False, False)
        with pytest.raises(Exception, match=r"view 1: scores.shape\[1\] = 24, expected hp \* wp = 18"):
            op([s, t], [2, 3], [3, 6], [False, True], 32, 48, False, False)
        with pytest.raises(Exception, match="all views share B and n"):
            op([s, torch.empty(1, 24, 5, device="cuda")], [2, 4], [3, 6], [False, True], 32, 48, False, False)
        with pytest.raises(Exception, match="17 views, the kernel takes 1 .. 16"):
            op([s] * 17, [2] * 17, [3] * 17, [False] * 17, 32, 48, False, False)
        with pytest.raises(Exception, match="one of each per view"):
            op([s, t], [2, 4], [3, 6], [False], 32, 48, False, False)
        with pytest.raises(Exception, match="empty batch"):
            op([torch.empty(0, 6, 5, device="cuda")], [2], [3], [False], 32, 48, False, False)
        with pytest.raises(Exception, match="B \\* h \\* w < 2\\*\\*31"):
            op([s], [2], [3], [False], 2 ** 15, 2 ** 15, False, False)


def test_op_fake_kernel_shapes_and_dtypes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    op = torch.ops.ifseg.seg_predict_views
    with FakeTensorMode():
        for n, ldt in ((1, torch.uint8), (256, torch.uint8), (257, torch.int16), (512, torch.int16)):
            s, t = torch.empty(3, 6, n, device="cuda"), torch.empty(3, 20, n, device="cuda")
            lab, conf, probs = op([s, t], [2, 5], [3, 4], [False, True], 37, 91, True, True)
            assert lab.shape == (3, 37, 91) and lab.dtype == ldt and lab.device.type == "cuda"
            assert conf.shape == (3, 37, 91) and conf.dtype == torch.float32
            assert probs.shape == (3, n, 37, 91) and probs.dtype == torch.float32
            lab, conf, probs = op([s], [2], [3], [True], 5, 1, False, False)
            assert lab.shape == (3, 5, 1) and conf.shape == (0,) and probs.shape == (0,)
            assert conf.dtype == torch.float32 and probs.dtype == torch.float32
            lab, conf, probs = op([t, s], [4, 3], [5, 2], [False, False], 5, 1, True, False)
            assert conf.shape == (3, 5, 1) and probs.shape == (0,)


def test_header_declares_the_entry_points_and_abi_is_still_21():
    hdr = open(os.path.join(ROOT, "include", "ifseg_hip.h")).read()
    assert int(re.search(r"#define\s+IFSEG_ABI_VERSION\s+(\d+)", hdr).group(1)) == hip.ABI_VERSION == 21
    assert "typedef struct {\n  const float* scores;" in hdr and "} ifseg_predict_view;" in hdr
    assert "int ifseg_seg_predict_views(const ifseg_predict_view* views, int K, int B, int n, int h, int w, void* labels" in hdr
    assert "int ifseg_seg_predict_views_staging(int max_bytes);" in hdr
    assert hip.SEG_PREDICT_MAX_VIEWS == 16
