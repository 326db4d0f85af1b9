"""CPU: the two specifications of the OHEM pixel sampler (`hardness_reference`, `ohem_reference`) against a literal
transcription of the upstream sampler and against `upsample_logits` + softmax, the criterion's reference path with
`ohem_thresh`, the refusals, and the C ABI surface."""
import ctypes
import os
import re
import types

import pytest
import torch

import _ohem_cases as OC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG0 = OC.SEG0
TRAINING = types.SimpleNamespace(training=True)
EVAL = types.SimpleNamespace(training=False)


def _bits(h):
    return h.to(torch.float32).contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF


@pytest.mark.parametrize("kind", OC.KINDS)
@pytest.mark.parametrize("B,N", [(1, 1), (2, 255), (3, 1031)])
def test_reference_is_the_upstream_sampler(kind, B, N):
    """every regime of (thresh, min_kept) on every kind of plane: the plane is 255 exactly on upstream's kept pixels, and info
    counts them"""
    from ifseg_amd.criterions.seg_criterion import ohem_reference
    h = OC.plane(kind, B, N)
    cand = _bits(h) <= OC.ONE_BITS
    kept_any = dropped_any = False
    for thresh, min_kept in OC.regimes(B, N):
        plane, info = ohem_reference(h, thresh, min_kept)
        want = OC.upstream_sample(h, cand, thresh, min_kept)
        assert plane.dtype == torch.uint8 and tuple(plane.shape) == (B, N)
        assert torch.equal(plane, want.to(torch.uint8) * 255), (kind, thresh, min_kept)
        assert info.dtype == torch.int64 and info.tolist()[:2] == [int(cand.sum()), int(want.sum())]
        kept_any |= bool(want.any())
        dropped_any |= bool((cand & ~want).any())
    if kind == "none":
        assert not kept_any
    elif N > 1:
        assert kept_any and dropped_any


def test_regimes_by_hand():
    from ifseg_amd.criterions.seg_criterion import ohem_reference
    f32 = lambda v: int(torch.tensor(v, dtype=torch.float32).view(torch.int32))
    h = torch.tensor([[0.1, 0.2, 0.3, -1.0], [0.4, 0.8, 0.9, 0.2]])
    # thresh decides: k = 0, the minimum 0.1 < 0.7
    p, i = ohem_reference(h, 0.7, 0)
    assert p.tolist() == [[255, 255, 255, 0], [255, 0, 0, 255]] and i.tolist() == [7, 5, f32(0.7), f32(0.1)]
    # min_kept decides: k = 2 * 3 = 6 = |V| - 1, the maximum; everything below it
    p, i = ohem_reference(h, 0.0, 3)
    assert p.tolist() == [[255, 255, 255, 0], [255, 255, 0, 255]] and i.tolist() == [7, 6, f32(0.9), f32(0.9)]
    # min_kept * B >= |V|
    assert torch.equal(ohem_reference(h, 0.0, 10 ** 6)[0], p)
    # exact ties at the k-th value: k = 2 -> sorted[2] = 0.2 (twice): both dropped, only 0.1 is below
    p, i = ohem_reference(h, 0.0, 1)
    assert p.tolist() == [[255, 0, 0, 0], [0, 0, 0, 0]] and i.tolist() == [7, 1, f32(0.2), f32(0.2)]
    # min_kept = 0, thresh = 0: nothing is below the minimum
    p, i = ohem_reference(h, 0.0, 0)
    assert int(p.sum()) == 0 and i.tolist() == [7, 0, f32(0.1), f32(0.1)]
    # no valid pixel
    p, i = ohem_reference(torch.full((2, 3), -1.0), 0.7, 5)
    assert int(p.sum()) == 0 and i.tolist() == [0, 0, f32(0.7), 0]
    # all values equal: nothing is strictly below the k-th
    p, i = ohem_reference(torch.full((2, 3), 0.9), 0.7, 2)
    assert int(p.sum()) == 0 and i.tolist() == [6, 0, f32(0.9), f32(0.9)]
    # thresh is rounded to fp32 once: fp32(0.7) is not below itself
    p, _ = ohem_reference(torch.tensor([[0.7, 0.69999]]), 0.7, 0)
    assert p.tolist() == [[0, 255]]


def test_candidate_rule():
    """-1, -0.0, NaN, 1.0, the float above 1.0, 0 and a denormal; fp64 input is rounded to fp32 first"""
    from ifseg_amd.criterions.seg_criterion import ohem_reference
    above = torch.tensor([OC.ONE_BITS + 1], dtype=torch.int32).view(torch.float32)[0]
    h = torch.tensor([[-1.0, -0.0, float("nan"), 1.0, 0.0, 0.0, 1e-40, 0.5, float("inf")]])
    h[0, 4] = above
    # k = 8 -> min(8, 4 - 1) = 3: the maximum of the candidates {1.0, 0, 1e-40, 0.5} = 1.0
    plane, info = ohem_reference(h, 0.0, 8)
    assert plane.tolist() == [[0, 0, 0, 0, 0, 255, 255, 255, 0]]
    assert info.tolist() == [4, 3, OC.ONE_BITS, OC.ONE_BITS]
    plane64, info64 = ohem_reference(h.double(), 0.0, 8)
    assert torch.equal(plane64, plane) and torch.equal(info64, info)
    # thresh = 1.0: every candidate below 1.0, 1.0 itself is not
    plane, info = ohem_reference(h, 1.0, 0)
    assert plane.tolist() == [[0, 0, 0, 0, 0, 255, 255, 255, 0]] and info.tolist() == [4, 3, OC.ONE_BITS, 0]


def test_weight_plane_composes():
    from ifseg_amd.criterions.seg_criterion import ohem_reference
    B, N = 3, 1031
    h, w = OC.plane("half", B, N), OC.weight_plane(B, N)
    for thresh, min_kept in OC.regimes(B, N):
        p0, i0 = ohem_reference(h, thresh, min_kept)
        p1, i1 = ohem_reference(h, thresh, min_kept, w)
        assert torch.equal(p1, torch.where(p0 == 255, w, torch.zeros_like(w))) and torch.equal(i0, i1)
    with pytest.raises(ValueError, match="weight"):
        ohem_reference(h, 0.7, 1, w[:, :-1])
    with pytest.raises(ValueError, match="weight"):
        ohem_reference(h, 0.7, 1, w.float())


@pytest.mark.parametrize("nseg,B,hp,wp", [(5, 2, 3, 4), (17, 2, 3, 4)])
def test_hardness_reference_is_softmax_at_the_label(nseg, B, hp, wp):
    from ifseg_amd.criterions import SegCriterion
    from ifseg_amd.criterions.seg_criterion import hardness_reference
    lp, tgt = OC.hard_inputs(nseg, B, hp, wp)
    tgt = tgt.clone()
    tgt[(tgt < SEG0) & (tgt > 2)] = SEG0 + nseg                              # what compute_loss_torch's mask does not know
    tgt[tgt > SEG0 + nseg] = SEG0 + nseg
    H, W = 16 * hp, 16 * wp
    scores = SegCriterion.upsample_logits(lp[:, :, :nseg].float(), hp, wp, H, W)
    hard = hardness_reference(scores, tgt, SEG0, nseg)
    assert hard.dtype == torch.float32 and tuple(hard.shape) == (B, H * W)
    assert hardness_reference(scores.double(), tgt, SEG0, nseg).dtype == torch.float64
    assert torch.equal(hardness_reference(scores[:, :-1], tgt, SEG0, nseg), hard)
    assert torch.equal(hardness_reference(scores, tgt[:, :-1], SEG0, nseg), hard)
    mask = (tgt == 1) | (tgt == SEG0 + nseg) | (tgt == 2)                    # compute_loss_torch's
    drop = mask[:, :-1]
    assert torch.equal(hard == -1.0, drop) and bool(drop.any()) and bool((~drop).any())
    p = torch.softmax(scores[:, :-1], -1)
    want = p[~drop].gather(1, (tgt[:, :-1][~drop] - SEG0)[:, None])[:, 0]
    assert torch.equal(hard[~drop], want.clamp(max=1.0))
    assert float(hard.max()) <= 1.0
    # labels that are no class and not pad / eos / ignore either: -1, as the kernels drop them
    lp, tgt = OC.hard_inputs(nseg, B, hp, wp)
    hard = hardness_reference(scores, tgt, SEG0, nseg)
    assert float(hard[0, 5]) == -1.0 and float(hard[0, 40]) == -1.0 and float(hard[B - 1, H * W - 7]) == -1.0


def _net_output(nseg, B, hp, wp, ignore_only=True):
    lp, tgt = OC.hard_inputs(nseg, B, hp, wp)
    tgt = tgt.clone()
    tgt[(tgt < SEG0) & (tgt > 2)] = SEG0 + nseg
    tgt[tgt > SEG0 + nseg] = SEG0 + nseg
    H, W = 16 * hp, 16 * wp
    logits = lp[:, :, :nseg].float()
    extra = {"encoder_returns": {"image_embed_shape": [(hp, wp)]}}
    sample = {"target": tgt, "net_input": {"patch_images": torch.zeros(B, 3, H, W)}}
    return (logits, extra), sample


@pytest.mark.parametrize("norm", ["weights", "pixels"])
def test_criterion_reference_path(norm):
    from ifseg_amd.criterions import SegCriterion
    from ifseg_amd.criterions.seg_criterion import hardness_reference, ohem_reference, weighted_loss_reference
    nseg, B, hp, wp = 17, 2, 3, 4
    H, W = 16 * hp, 16 * wp
    net_output, sample = _net_output(nseg, B, hp, wp)
    kw = dict(unsupervised_segmentation=False, init_seg_with_text=False, num_seg_tokens=nseg, seg_id_offset=SEG0)
    min_kept = H * W // 4
    crit = SegCriterion(ohem_thresh=0.7, ohem_min_kept=min_kept, weight_norm=norm, **kw)
    assert crit.ohem_info is None
    loss, metrics, _ = crit.compute_loss_torch(TRAINING, net_output, sample, 0)
    scores = SegCriterion.upsample_logits(net_output[0], hp, wp, H, W)
    plane, info = ohem_reference(hardness_reference(scores, sample["target"], SEG0, nseg), 0.7, min_kept)
    want = weighted_loss_reference(scores[:, :H * W], sample["target"], SEG0, nseg, None, plane, 0.0, norm)
    assert torch.equal(loss, want) and torch.equal(crit.ohem_info, info)
    assert 0 < int(info[1]) < int(info[0])
    # a sample's own plane composes
    tw = OC.weight_plane(B, H * W)
    loss_w, _, _ = crit.compute_loss_torch(TRAINING, net_output, dict(sample, target_weight=tw), 0)
    plane_w, _ = ohem_reference(hardness_reference(scores, sample["target"], SEG0, nseg), 0.7, min_kept, tw)
    assert torch.equal(loss_w, weighted_loss_reference(scores[:, :H * W], sample["target"], SEG0, nseg, None, plane_w, 0.0, norm))
    # without the keyword, and in evaluation, the loss is what it was: plain cross entropy over the valid pixels
    tgt = sample["target"]
    mask = (tgt == 1) | (tgt == SEG0 + nseg) | (tgt == 2)
    plain = torch.nn.functional.cross_entropy(scores[~mask], tgt[~mask] - SEG0)
    base = SegCriterion(weight_norm=norm, **kw)
    assert base.ohem_thresh is None
    assert torch.equal(base.compute_loss_torch(TRAINING, net_output, sample, 0)[0], plain)
    assert torch.equal(crit.compute_loss_torch(EVAL, net_output, sample, 0)[0], plain)
    assert base.ohem_info is None and float(plain) != float(loss)


def test_refusals():
    from ifseg_amd.criterions import SegCriterion
    from ifseg_amd.criterions.seg_criterion import ohem_reference
    kw = dict(unsupervised_segmentation=False, init_seg_with_text=False, num_seg_tokens=5, seg_id_offset=SEG0)
    for bad in (-0.1, 1.5, float("nan"), "0.7"):
        with pytest.raises(ValueError, match="thresh"):
            SegCriterion(ohem_thresh=bad, **kw)
        with pytest.raises(ValueError, match="thresh"):
            ohem_reference(torch.zeros(1, 4), bad, 1)
    for bad in (-1, 1.5):
        with pytest.raises(ValueError, match="min_kept"):
            SegCriterion(ohem_thresh=0.7, ohem_min_kept=bad, **kw)
        with pytest.raises(ValueError, match="min_kept"):
            ohem_reference(torch.zeros(1, 4), 0.7, bad)
    with pytest.raises(ValueError, match="loss-ranked"):
        SegCriterion(ohem_thresh=None, ohem_min_kept=5000, **kw)
    with pytest.raises(ValueError, match="thresh"):
        ohem_reference(torch.zeros(1, 4), None, 1)
    c = SegCriterion(ohem_thresh=0, ohem_min_kept=0, **kw)
    assert c.ohem_thresh == 0.0 and c.ohem_min_kept == 0
    assert SegCriterion(**kw).ohem_thresh is None


def test_abi_declares_and_exports_the_entry_points():
    from ifseg_amd import hip
    hdr = open(os.path.join(ROOT, "include", "ifseg_hip.h")).read()
    names = set(re.findall(r"\bint\s+(ifseg_\w+)\s*\(", hdr))
    assert {"ifseg_seg_hardness", "ifseg_ohem_select"} <= names
    assert int(re.search(r"#define IFSEG_ABI_VERSION (\d+)", hdr).group(1)) == 21 == hip.ABI_VERSION
    if not os.path.exists(hip.LIB_PATH):
        from ifseg_amd.build import build
        build(verbose=False)
    lib = hip.lib()
    assert hasattr(lib, "ifseg_seg_hardness") and hasattr(lib, "ifseg_ohem_select")
    lib.ifseg_abi_version.restype = ctypes.c_int
    assert lib.ifseg_abi_version() == 21
    src = open(os.path.join(ROOT, "ifseg_amd", "csrc", "ohem.hip")).read()
    assert int(re.search(r"OHEM_WORK_WORDS = STATE \+ (\d+)", src).group(1)) + 3 * 1024 == hip.OHEM_WORK_WORDS
