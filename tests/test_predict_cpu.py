"""CPU: the surface of the inference entry point (ifseg_amd/predict.py, torch.ops.ifseg.seg_predict, hip.seg_predict) and
the premises of the GPU tests in test_predict_gpu.py (exactness of the exact family; the 1 % cap of the general family)."""
import os
import re
import types

import pytest
import torch

import _predict_cases as C
from ifseg_amd import hip
from ifseg_amd import ops  # noqa: F401  (registers torch.ops.ifseg.*)
from ifseg_amd.predict import Segmenter, SegmentationResult, source_tokens, upsample_argmax_reference
from ifseg_amd.tasks.mm_tasks.segmentation import BOS, EOS, PROMPT_IDS, SegmentationTask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(n, training=False):
    return types.SimpleNamespace(cfg=types.SimpleNamespace(num_seg_tokens=n), training=training)


# ------------------------------------------------------------------------------------------------- premises of the GPU tests
@pytest.mark.parametrize("shape", C.EXACT_SHAPES)
def test_exact_family_is_exact_in_fp32(shape):
    B, hp, wp, n = shape
    s = C.exact_scores(shape)
    l32, c32, p32 = upsample_argmax_reference(s, hp, wp, 16 * hp, 16 * wp, torch.float32)
    l64, c64, p64 = upsample_argmax_reference(s, hp, wp, 16 * hp, 16 * wp, torch.float64)
    assert torch.equal(p32.double(), p64) and torch.equal(l32, l64) and torch.equal(c32.double(), c64)
    assert torch.equal(p64 * 1024, (p64 * 1024).round())
    if n > 1:
        top2 = p64.topk(2, dim=1).values
        ties = (top2[:, 0] == top2[:, 1]).float().mean().item()
        print(shape, "exact ties: %.1f %% of the pixels" % (100 * ties))
        assert ties > 0.01          # the first-maximum rule is exercised


@pytest.mark.parametrize("softmaxed", [False, True], ids=["raw", "softmax"])
@pytest.mark.parametrize("shape", C.GENERAL_SHAPES + C.DIRECT_SHAPES)
def test_general_family_margin_cap_holds(shape, softmaxed):
    """the GPU test leaves out the pixels whose top-2 margin is below 32 e: they must be at most 1 % of every case"""
    hp, wp, n, h, w = shape
    for seed in C.SEEDS:
        ref = C.Reference(C.general_scores(shape, seed, softmaxed), hp, wp, h, w)
        print(shape, seed, "e = %.2e, undecided %.3f %%" % (ref.e, 100 * ref.undecided_share))
        assert 0 < ref.e < 1e-4
        assert ref.undecided_share <= C.MARGIN_CAP


def test_e2e_fixture_margin_cap_holds_on_the_oracle_logits():
    """the end-to-end GPU test compares labels under the same rule: on the oracle's (bf16-rounded) logits of that fixture the
    cap holds in both modes, so the seeded model is not too flat for the test to mean something"""
    import segofa_ref as O
    ocfg, sd, img, src = C.e2e_fixture()
    with torch.no_grad():
        logits, extra = O.segofa_forward(sd, ocfg, src[None].repeat(2, 1), img)
    hp, wp = extra["encoder_returns"]["image_embed_shape"]
    lo = logits[:, : hp * wp].to(torch.bfloat16).float()
    for name, s in (("logits", lo), ("probs", lo.softmax(-1))):
        ref = C.Reference(s, hp, wp, 128, 128)
        print(name, "e = %.2e, undecided %.3f %%" % (ref.e, 100 * ref.undecided_share), "classes", ref.labels.unique().tolist())
        assert ref.undecided_share <= C.MARGIN_CAP
        assert ref.labels.unique().numel() >= 3         # not one flat class


# ------------------------------------------------------------------------------------------------- Segmenter: net input
def test_source_token_layout_and_padding():
    names = [[5, 6], [7], [8, 9, 10]]
    src = source_tokens(names, PROMPT_IDS, 3)
    assert src.dtype == torch.int64
    assert src.tolist() == [BOS] + list(PROMPT_IDS) + [5, 6, 7, 8, 9, 10] + [EOS]
    seg = Segmenter(_model(3), category_token_ids=names)
    ni = seg.net_input(torch.zeros(4, 3, 32, 48))
    L = 1 + len(PROMPT_IDS) + 6 + 1
    assert ni["src_tokens"].shape == (4, L) and ni["src_tokens"].is_contiguous()
    assert all(torch.equal(ni["src_tokens"][b], src) for b in range(4))       # one prompt for the batch: no padding
    assert ni["src_lengths"].tolist() == [L] * 4
    assert ni["prev_output_tokens"].tolist() == [[BOS]] * 4 and ni["prev_output_tokens"].dtype == torch.int64
    assert ni["patch_masks"].dtype == torch.bool and ni["patch_masks"].all() and ni["patch_masks"].shape == (4,)
    assert ni["patch_images"].shape == (4, 3, 32, 48)


def test_names_come_from_the_task_and_build_segmenter():
    names = [[11], [12, 13]]
    task = SegmentationTask(num_seg_tokens=2, patch_image_size=64, category_token_ids=names)
    seg = task.build_segmenter(_model(2), prompt_ids=(40, 41), upsample="logits")
    assert isinstance(seg, Segmenter) and seg.upsample == "logits"
    assert seg.src.tolist() == [BOS, 40, 41, 11, 12, 13, EOS]
    # explicit names win over the task's
    assert Segmenter(_model(2), task=task, category_token_ids=[[1], [2]], prompt_ids=()).src.tolist() == [BOS, 1, 2, EOS]
    # category_list without a BPE encoder: the task says what is missing
    t2 = SegmentationTask(num_seg_tokens=2, patch_image_size=64)
    t2.category_list = "cat,dog"
    with pytest.raises(RuntimeError, match="BPE"):
        Segmenter(_model(2), task=t2)
    with pytest.raises(ValueError, match="no class names"):
        Segmenter(_model(2))


def test_uint8_images_are_normalised_like_the_pipeline():
    g = torch.Generator().manual_seed(0)
    im = torch.randint(0, 256, (2, 6, 5, 3), generator=g, dtype=torch.uint8)
    x, rgb = Segmenter.prepare_images(im)
    assert x.shape == (2, 3, 6, 5) and x.dtype == torch.float32 and x.is_contiguous()
    assert torch.equal(x, ((im.float() / 255 - 0.5) / 0.5).permute(0, 3, 1, 2))
    assert torch.equal(rgb, im.float())
    x1, _ = Segmenter.prepare_images(im[0])
    assert torch.equal(x1, x[:1])
    f = torch.zeros(2, 3, 8, 8)
    assert Segmenter.prepare_images(f)[0] is f and Segmenter.prepare_images(f)[1] is None
    with pytest.raises(ValueError, match="images must be"):
        Segmenter.prepare_images(torch.zeros(2, 8, 8, 3))
    with pytest.raises(ValueError, match="uint8 images must be RGB"):
        Segmenter.prepare_images(torch.zeros(2, 3, 8, 8, dtype=torch.uint8))


# ------------------------------------------------------------------------------------------------- refusals, by name
def test_segmenter_refusals():
    with pytest.raises(ValueError, match="3 category names for a model with num_seg_tokens = 5"):
        Segmenter(_model(5), category_token_ids=[[1], [2], [3]])
    with pytest.raises(ValueError, match="n = 513 classes"):
        Segmenter(_model(513), category_token_ids=[[1]] * 513)
    with pytest.raises(ValueError, match="uint8 labels hold at most 256 classes"):
        Segmenter(_model(257), category_token_ids=[[1]] * 257, label_dtype=torch.uint8)
    Segmenter(_model(257), category_token_ids=[[1]] * 257)                      # int16 labels: fine
    with pytest.raises(ValueError, match="upsample must be"):
        Segmenter(_model(1), category_token_ids=[[1]], upsample="nearest")
    seg = Segmenter(_model(2), category_token_ids=[[1], [2]], crf_iters=2)
    with pytest.raises(ValueError, match="crf_images is required"):
        seg(torch.zeros(1, 3, 32, 32), out_hw=(40, 32))
    with pytest.raises(ValueError, match="crf_images is required"):
        seg(torch.zeros(2, 3, 32, 32), out_hw=[(32, 32), (20, 32)])
    with pytest.raises(ValueError, match="lists 1 sizes for a batch of 2"):
        Segmenter(_model(2), category_token_ids=[[1], [2]])(torch.zeros(2, 3, 32, 32), out_hw=[(32, 32)])


def test_binding_refuses_before_it_launches():
    """hip.seg_predict asserts dtype, contiguity and shape before the library is touched"""
    ok = torch.zeros(2, 6, 5)
    for bad in (ok.double(), ok.transpose(1, 2), ok[0]):
        with pytest.raises(AssertionError):
            hip.seg_predict(bad, 2, 3, 32, 48)
    with pytest.raises(AssertionError):
        hip.seg_predict(ok, 2, 2, 32, 48)                           # hp * wp != rows
    with pytest.raises(AssertionError):
        hip.seg_predict(torch.zeros(1, 1, 513), 1, 1, 4, 4)         # n > 512
    with pytest.raises(AssertionError):
        hip.seg_predict(torch.zeros(1, 1, 257), 1, 1, 4, 4, label_dtype=torch.uint8)
    with pytest.raises(AssertionError):
        hip.seg_predict(ok, 2, 3, 0, 48)


def test_op_refusals_on_fake_tensors():
    from torch._subclasses.fake_tensor import FakeTensorMode
    op = torch.ops.ifseg.seg_predict
    with FakeTensorMode():
        s = torch.empty(2, 6, 5, device="cuda")
        with pytest.raises(Exception, match="scores must be fp32"):
            op(s.to(torch.bfloat16), 2, 3, 32, 48, False, False)
        with pytest.raises(Exception, match=r"n = 513 classes, the kernel takes 1 .. FUSED_MAX_CLASSES = 512"):
            op(torch.empty(1, 6, 513, device="cuda"), 2, 3, 32, 48, False, False)
        with pytest.raises(Exception, match=r"scores.shape\[1\] = 6, expected hp \* wp = 4"):
            op(s, 2, 2, 32, 48, False, False)
        with pytest.raises(Exception, match="empty batch"):
            op(torch.empty(0, 6, 5, device="cuda"), 2, 3, 32, 48, False, False)
        with pytest.raises(Exception, match="B \\* h \\* w < 2\\*\\*31"):
            op(s, 2, 3, 2 ** 15, 2 ** 15, False, False)


def test_op_fake_kernel_shapes_and_dtypes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    op = torch.ops.ifseg.seg_predict
    with FakeTensorMode():
        for n, ldt in ((1, torch.uint8), (256, torch.uint8), (257, torch.int16), (512, torch.int16)):
            s = torch.empty(3, 6, n, device="cuda")
            lab, conf, probs = op(s, 2, 3, 37, 91, True, True)
            assert lab.shape == (3, 37, 91) and lab.dtype == ldt and lab.device.type == "cuda"
            assert conf.shape == (3, 37, 91) and conf.dtype == torch.float32
            assert probs.shape == (3, n, 37, 91) and probs.dtype == torch.float32
            lab, conf, probs = op(s, 2, 3, 5, 1, False, False)
            assert lab.shape == (3, 5, 1) and conf.shape == (0,) and probs.shape == (0,)
            assert conf.dtype == torch.float32 and probs.dtype == torch.float32
            lab, conf, probs = op(s, 2, 3, 5, 1, True, False)
            assert conf.shape == (3, 5, 1) and probs.shape == (0,)


def test_abi_version_is_21_in_header_and_binding():
    hdr = open(os.path.join(ROOT, "include", "ifseg_hip.h")).read()
    assert int(re.search(r"#define\s+IFSEG_ABI_VERSION\s+(\d+)", hdr).group(1)) == hip.ABI_VERSION == 21
    assert "int ifseg_seg_predict(const float* scores, int B, int hp, int wp, int n, int h, int w" in hdr


def test_reference_matches_the_criterions_upsample():
    """upsample_argmax_reference is F.interpolate in the asked dtype + argmax, i.e. SegCriterion.upsample_logits + argmax"""
    from ifseg_amd.criterions import SegCriterion
    s = C.general_scores((4, 6, 15, 37, 91), 3, False, batch=2)
    lab, conf, probs = upsample_argmax_reference(s, 4, 6, 37, 91, torch.float32)
    up = SegCriterion.upsample_logits(torch.cat([s, s[:, :1]], 1), 4, 6, 37, 91)[:, :-1]          # [B, h*w, n]
    assert torch.equal(probs, up.transpose(1, 2).reshape(2, 15, 37, 91))
    assert torch.equal(lab, up.argmax(-1).reshape(2, 37, 91)) and torch.equal(conf, up.max(-1).values.reshape(2, 37, 91))
    assert isinstance(SegmentationResult(lab, None, None), tuple)
