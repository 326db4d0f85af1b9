"""CPU: the specification of hip.image_load (ifseg_amd/imageio.py), the surface of torch.ops.ifseg.image_load and
Segmenter.segment_raw's grouping, and the premises of the GPU tests in test_image_load_gpu.py (exactness of the exact family;
the 1 % cap of the general family)."""
import os

import pytest
import torch
import torch.nn.functional as F

import _image_load_cases as C
from ifseg_amd import hip
from ifseg_amd import ops  # noqa: F401  (registers torch.ops.ifseg.*)
from ifseg_amd.imageio import (IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD, eval_size, image_load_reference,
                               normalisation_table, plan_groups, source_coords)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------- sizes
@pytest.mark.parametrize("h, w, P, want", [(480, 640, 512, (512, 683)), (375, 500, 512, (512, 683)), (60, 90, 128, (128, 192)),
                                           (700, 300, 128, (299, 128)), (33, 250, 128, (68, 512)), (1, 1, 128, (128, 128))])
def test_eval_size_table(h, w, P, want):
    assert eval_size(h, w, P) == want
    assert eval_size(w, h, P) == want[::-1]


# ------------------------------------------------------------------------------------------------- the filter
def _interp64(img, oh, ow):
    return F.interpolate(img.permute(0, 3, 1, 2).double(), size=(oh, ow), mode="bilinear", align_corners=False)


@pytest.mark.parametrize("shape", C.exact_shapes())
def test_exact_family_spec_is_interpolate_and_exact_in_fp32(shape):
    B, H0, W0, oh, ow = shape
    img = C.exact_images(shape)
    n64, q64, v64 = image_load_reference(img, oh, ow, dtype=torch.float64)
    n32, q32, v32 = image_load_reference(img, oh, ow, dtype=torch.float32)
    assert v32.dtype == torch.float32 and n64.shape == (B, 3, oh, ow) and q64.dtype == torch.uint8
    d = (v64 - _interp64(img, oh, ow)).abs().max().item()
    print(shape, "max |spec - F.interpolate| = %.2e" % d)
    assert d <= 1e-9
    assert torch.equal(v32.double(), v64) and torch.equal(q32, q64) and torch.equal(n32, n64)
    assert torch.equal(v64 * 4096, (v64 * 4096).round())
    if shape == C.EXACT_RATIO:
        ties = ((v64 - v64.floor()) == 0.5).float().mean().item()
        print(shape, "exact .5 ties: %.3f %% of the pixels" % (100 * ties))
        assert ties > 0                                   # round-half-up is exercised
        assert torch.equal(q64[(v64 - v64.floor()) == 0.5].double(), v64[(v64 - v64.floor()) == 0.5] + 0.5)


@pytest.mark.parametrize("case", C.GENERAL_CASES)
def test_general_family_spec_is_interpolate_and_margin_cap_holds(case):
    """the GPU test leaves out the pixels whose value lies within 32 e of a rounding boundary: at most 1 % of every case"""
    for seed in C.SEEDS:
        img, oh, ow, ref = C.general_reference(case, seed)
        assert (oh, ow) == eval_size(case[0], case[1], case[2])
        d = (ref.v - _interp64(img, oh, ow)).abs().max().item()
        print(case, seed, "-> %d x %d  e = %.2e, left out %.3f %%, max |spec - F.interpolate| = %.2e"
              % (oh, ow, ref.e, 100 * ref.undecided_share, d))
        assert d <= 1e-9
        assert 0 < ref.e < 1e-4
        assert ref.undecided_share <= C.MARGIN_CAP
        # the rule passes on the fp32 specification itself
        n32, q32, _ = image_load_reference(img, oh, ow, dtype=torch.float32)
        ref.check(q32, n32, what=(case, seed, "fp32 specification"))
        ref.check(q32, n32.to(torch.bfloat16), what=(case, seed, "fp32 specification, bf16 out"))


def test_source_coords_by_hand():
    # 2 -> 4: centres at -0.25, 0.25, 0.75, 1.25 -> clamped at 0, and at the last sample
    i0, i1, lam = source_coords(4, 2, torch.float32)
    assert i0.tolist() == [0, 0, 0, 1] and i1.tolist() == [1, 1, 1, 1]
    assert lam.tolist() == [0.0, 0.25, 0.75, 0.0] and lam.dtype == torch.float32
    # 4 -> 2 (downscale, no antialiasing): centres at 0.5 and 2.5
    i0, i1, lam = source_coords(2, 4)
    assert i0.tolist() == [0, 2] and i1.tolist() == [1, 3] and lam.tolist() == [0.5, 0.5] and lam.dtype == torch.float64
    i0, i1, lam = source_coords(5, 1)
    assert i0.tolist() == [0] * 5 and i1.tolist() == [0] * 5 and lam.tolist() == [0.0] * 5


def test_channel_reversal_and_per_channel_normalisation_by_hand():
    img = torch.tensor([[[[0, 10, 20], [100, 110, 120]], [[200, 210, 220], [255, 1, 2]]]], dtype=torch.uint8)   # [1, 2, 2, 3]
    mean, std = (0.1, 0.2, 0.3), (0.5, 0.25, 2.0)
    norm, q, v = image_load_reference(img, 2, 2, mean, std, reverse_channels=True)
    assert torch.equal(q[0, 0], img[0, :, :, 2]) and torch.equal(q[0, 1], img[0, :, :, 1]) and torch.equal(q[0, 2], img[0, :, :, 0])
    f = lambda x, c: (torch.tensor(float(x)) / 255 - mean[c]) / std[c]
    assert norm.dtype == torch.float32
    assert norm[0, 0, 0, 1] == f(120, 0) and norm[0, 1, 1, 0] == f(210, 1) and norm[0, 2, 1, 1] == f(255, 2) and norm[0, 2, 0, 0] == f(0, 2)
    norm2, q2, _ = image_load_reference(img, 2, 2, mean, std, reverse_channels=False, out_dtype=torch.bfloat16)
    assert torch.equal(q2[0], img[0].permute(2, 0, 1)) and norm2.dtype == torch.bfloat16
    assert norm2[0, 0, 0, 1] == f(100, 0).to(torch.bfloat16) and norm2[0, 2, 1, 0] == f(220, 2).to(torch.bfloat16)
    # a 2 x 2 -> 1 x 1 resize averages the four pixels, and .5 rounds up: (0 + 100 + 200 + 255) / 4 = 138.75, (20 + 120 + 220 + 2) / 4 = 90.5
    _, q3, v3 = image_load_reference(img, 1, 1, reverse_channels=False)
    assert v3[0, :, 0, 0].tolist() == [138.75, 82.75, 90.5] and q3[0, :, 0, 0].tolist() == [139, 83, 91]
    # the table: default = the pipeline's (x / 255 - 0.5) / 0.5; the q-carrying table of the GPU tests rounds to k
    k = torch.arange(256, dtype=torch.float32)
    assert torch.equal(normalisation_table()[1], (k / 255 - 0.5) / 0.5)
    assert torch.equal(normalisation_table(C.Q_MEAN, C.Q_STD).round(), k[None].expand(3, 256))
    t = normalisation_table(IMAGENET_DEFAULT_MEAN, IMAGENET_DEFAULT_STD)
    assert t.shape == (3, 256) and abs(t[0, 0].item() + 0.485 / 0.229) < 1e-6
    with pytest.raises(ValueError, match="three entries"):
        normalisation_table((0.5,), (0.5,))
    with pytest.raises(ValueError, match=r"uint8 \[B, H0, W0, 3\]"):
        image_load_reference(img.float(), 2, 2)


# ------------------------------------------------------------------------------------------------- grouping
def test_segment_raw_grouping():
    shapes = [(60, 90), (90, 60), (64, 64), (60, 90), (30, 45), (120, 180), (60, 90)]
    loads, forwards = plan_groups(shapes, 128, max_batch=8)
    # one launch per source shape, in order of first appearance
    assert loads == [((60, 90), (128, 192), [0, 3, 6]), ((90, 60), (192, 128), [1]), ((64, 64), (128, 128), [2]),
                     ((30, 45), (128, 192), [4]), ((120, 180), (128, 192), [5])]
    # one forward per network size: 60 x 90, 30 x 45 and 120 x 180 all run at 128 x 192, in input order
    assert forwards == [((128, 192), [0, 3, 4, 5, 6]), ((192, 128), [1]), ((128, 128), [2])]
    _, f2 = plan_groups(shapes, 128, max_batch=2)
    assert f2 == [((128, 192), [0, 3]), ((128, 192), [4, 5]), ((128, 192), [6]), ((192, 128), [1]), ((128, 128), [2])]
    # every image is loaded once and run once
    assert sorted(i for _, _, idx in loads for i in idx) == list(range(7)) == sorted(i for _, idx in f2 for i in idx)
    assert plan_groups([], 128) == ([], [])
    with pytest.raises(ValueError, match="max_batch"):
        plan_groups(shapes, 128, max_batch=0)


def test_segment_raw_refuses_what_is_not_a_raw_image():
    import types
    from ifseg_amd.predict import Segmenter
    seg = Segmenter(types.SimpleNamespace(cfg=types.SimpleNamespace(num_seg_tokens=2, patch_image_size=64), training=False),
                    category_token_ids=[[1], [2]])
    assert seg.segment_raw([]) == []
    for bad in (torch.zeros(8, 8, 3), torch.zeros(3, 8, 8, dtype=torch.uint8), torch.zeros(1, 8, 8, 3, dtype=torch.uint8)):
        with pytest.raises(ValueError, match=r"uint8 RGB \[H, W, 3\]"):
            seg.segment_raw([bad])


# ------------------------------------------------------------------------------------------------- binding and op
def test_binding_refuses_before_it_launches():
    ok = torch.zeros(2, 6, 5, 3, dtype=torch.uint8)
    for bad in (ok.float(), ok.transpose(1, 2), ok[0], torch.zeros(2, 6, 5, 4, dtype=torch.uint8)):
        with pytest.raises(AssertionError):
            hip.image_load(bad, 12, 10)
    with pytest.raises(AssertionError):
        hip.image_load(ok, 0, 10)
    with pytest.raises(AssertionError):
        hip.image_load(ok, 12, 10, dtype=torch.float16)


def test_op_fake_kernel_and_refusals():
    from torch._subclasses.fake_tensor import FakeTensorMode
    op = torch.ops.ifseg.image_load
    half = [0.5, 0.5, 0.5]
    with FakeTensorMode():
        x = torch.empty(3, 37, 61, 3, dtype=torch.uint8, device="cuda")
        for dt in (torch.float32, torch.bfloat16):
            o = op(x, 128, 211, half, half, True, dt)
            assert o.shape == (3, 3, 128, 211) and o.dtype == dt and o.device.type == "cuda"
        with pytest.raises(Exception, match="images must be uint8"):
            op(x.float(), 128, 211, half, half, True, torch.float32)
        with pytest.raises(Exception, match=r"images must be \[B, H0, W0, 3\]"):
            op(x[0], 128, 211, half, half, True, torch.float32)
        with pytest.raises(Exception, match="destination size"):
            op(x, 0, 211, half, half, True, torch.float32)
        with pytest.raises(Exception, match="three entries"):
            op(x, 8, 8, [0.5], half, True, torch.float32)
        with pytest.raises(Exception, match="torch.float32 or torch.bfloat16"):
            op(x, 8, 8, half, half, True, torch.float16)
        with pytest.raises(Exception, match=r"below 2\*\*31"):
            op(x, 2 ** 15, 2 ** 15, half, half, True, torch.float32)


def test_header_declares_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "ifseg_hip.h")).read()
    assert "int ifseg_image_load(const void* images, int B, int H0, int W0, int oh, int ow, const float* lut" in hdr
    assert "int ifseg_image_load_staging(int max_bytes);" in hdr
