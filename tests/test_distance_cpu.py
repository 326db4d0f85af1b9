"""CPU: the exact distance transform and the trimap counters (ifseg_amd/predict.py: distance_reference,
trimap_areas_reference; hip.seg_distance / seg_trimap_areas; csrc/distance.hip) without a device.  The specification against a
brute-force minimum, against scipy's EDT value by value, and against a Python transcription of the two kernel passes -- the
separable claim the kernels rest on; the trimap counters' identities with `areas_reference` and hand-written answers; what
`SegmentationScore` does with the counters; every refusal of the specification, the bindings, the Segmenter and the C
entries; the header; the launches a Segmenter makes, recorded by fakes.  Integers throughout: every comparison is exact."""
import ctypes
import os
import re

import pytest
import torch

import _boundary_cases as BC
import _distance_cases as T
import test_segmenter_launches_cpu as L
from test_boundary_cpu import Recorder as BoundaryRecorder, _with_boundary
from ifseg_amd import hip
from ifseg_amd.predict import (SegmentationScore, Segmenter, areas_reference, confusion_reference, default_trimap_radii,
                               distance_reference, trimap_areas_reference)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_SHAPE, BAD_ARG = -2, -3
U16 = torch.uint16
SMALL = T.SHAPES[:7]                             # up to 33 x 129: what the literal loops take in seconds


# ------------------------------------------------------------------------------------------------- the distance
@pytest.mark.parametrize("pattern", T.PATTERNS)
def test_reference_equals_the_brute_force_minimum(pattern):
    far = 0
    for key in T.case_keys((pattern,), SMALL):
        for border in (False, True):
            exact = T.brute(key, border)
            for R in T.RADII:
                got = T.reference(key, R, border)
                assert got.dtype == U16 and got.shape == T.labels_of(key).shape
                assert torch.equal(got.long(), T.clamp(exact, R)), (key, R, border)
                far += int((got == T.FAR).sum())
            if border:
                y, x = torch.meshgrid(torch.arange(key[1]), torch.arange(key[2]), indexing="ij")
                edge = torch.minimum(torch.minimum(x + 1, key[2] - x), torch.minimum(y + 1, key[1] - y))
                assert (exact <= edge * edge).all(), key
    assert far > 0                                                    # the clamp cuts something in every pattern
    if pattern == "constant":
        for key in T.case_keys((pattern,)):
            for R in T.RADII:
                assert (T.reference(key, R, False) == T.FAR).all()    # no other value anywhere


@pytest.mark.parametrize("key", T.case_keys() + ["disc", "table7"], ids=str)
def test_reference_equals_scipy_value_by_value(key):
    ndimage = pytest.importorskip("scipy.ndimage")
    import numpy as np
    lab = T.labels_of(key)
    values = torch.unique(lab).tolist()
    if len(values) == 1:                        # scipy's transform of an all-ones mask has no background to measure from
        assert all(bool((T.reference(key, R, False) == T.FAR).all()) for R in T.RADII)
        return
    want = torch.zeros(lab.shape, dtype=torch.int64)
    for c in values:
        e = ndimage.distance_transform_edt((lab == c).numpy())
        want = torch.where(lab == c, torch.from_numpy(np.rint(e * e).astype(np.int64)), want)
    for R in (T.RADII if isinstance(key, tuple) else (64, 128)):
        assert torch.equal(T.reference(key, R, False).long(), T.clamp(want, R)), (key, R)


@pytest.mark.parametrize("pattern", T.PATTERNS)
def test_the_two_passes_equal_the_reference(pattern):
    """(a) columns, (b) rows bounded by the pixel's own best: what csrc/distance.hip computes"""
    for key in T.case_keys((pattern,), T.SHAPES[:6]) + ([(pattern, 33, 129)] if pattern in ("blocks", "random5") else []):
        lab = T.labels_of(key)
        for border in (False, True):
            for R in (T.RADII if key[1] * key[2] <= 1200 else T.RADII[:3]):
                v, out = T.two_passes(lab, R, border)
                assert out == T.reference(key, R, border).tolist(), (key, R, border)
                assert all(1 <= e <= R or e == 255 for row in v for e in row), (key, R, border)


def test_reference_values_dtypes_and_batches():
    for key in (("random5", 17, 65), ("blocks", 33, 129), ("checkerboard", 3, 2)):
        for border in (False, True):
            assert torch.equal(distance_reference(T.labels_as(key, True), 17, border), T.reference(key, 17, border)), key
    assert bool((T.labels_as(("random5", 17, 65), True) < 0).any())
    # 255 and a negative value are values of their own
    lab = torch.tensor([[255, 255, 0, 0]], dtype=torch.uint8)
    assert distance_reference(lab, 2).tolist() == [[4, 1, 1, 4]] and distance_reference(lab, 1).tolist() == [[T.FAR, 1, 1, T.FAR]]
    assert distance_reference(torch.tensor([[-1, -1, 7]], dtype=torch.int16), 3, True).tolist() == [[1, 1, 1]]
    assert distance_reference(torch.tensor([[5, 5, 5, 5, 5]], dtype=torch.uint8), 3, True).tolist() == [[1, 1, 1, 1, 1]]
    assert distance_reference(torch.tensor([[5, 5, 5, 5, 5]], dtype=torch.uint8).t(), 2, True).t().tolist() == [[1, 1, 1, 1, 1]]
    wide = distance_reference(torch.full((7, 9), 5, dtype=torch.uint8), 3, True)
    F = T.FAR
    assert wide[3].tolist() == [1, 4, 9, F, F, F, 9, 4, 1] and wide[:, 4].tolist() == [1, 4, 9, F, 9, 4, 1]
    assert int(distance_reference(torch.full((9, 11), 5, dtype=torch.uint8), 3, True)[4, 5]) == T.FAR
    # a batch is its images one by one: distances never cross from one image into the next
    batch = T.labels_of("batch")
    for R in (4, 17, 128):
        for border in (False, True):
            whole = distance_reference(batch, R, border)
            assert torch.equal(whole, torch.stack([distance_reference(b, R, border) for b in batch])), (R, border)
        assert (distance_reference(batch, R)[1] == T.FAR).all()       # the constant image between the two others
    assert int(batch[0, -1, 0]) == int(batch[1, 0, 0]) == int(batch[1, -1, 0]) == int(batch[2, 0, 0])


def test_the_disc_is_cut_at_the_rim():
    d = T.reference("disc", 128, False).long()
    assert int(d[150, 200]) == 1 and int(d[150, 72]) == 128 * 128 and int(d[150, 71]) == T.FAR and int(d[22, 200]) == 128 * 128
    assert int(d[21, 200]) == T.FAR and int(d[150 - 77, 200 + 102]) == 77 * 77 + 102 * 102 <= 128 * 128
    assert int(d[150 - 78, 200 + 102]) == T.FAR and 78 * 78 + 102 * 102 > 128 * 128
    inside = d != T.FAR
    assert int(inside.sum()) == sum(1 for y in range(-128, 129) for x in range(-128, 129) if 0 < y * y + x * x <= 128 * 128) + 1
    far64 = T.reference("table7", 64, False)
    assert bool((far64 == T.FAR).any()) and bool((far64 != T.FAR).any())


def test_reference_refusals():
    lab = torch.zeros(3, 4, dtype=torch.uint8)
    for bad in (0, 129, -1, 2.0, True, None):
        with pytest.raises(ValueError, match="distance_reference: max_distance"):
            distance_reference(lab, bad)
    for bad in (lab.long(), lab.float(), lab.reshape(-1), lab[None, None], lab[:0]):
        with pytest.raises(ValueError, match="distance_reference: labels"):
            distance_reference(bad, 3)
    gt = torch.ones(3, 4, dtype=torch.uint8)
    for bad in ((), (0,), (1, 1), (2, 1), (1, 129), (1.0, 2), (True, 2), tuple(range(1, 10)), 3, None):
        with pytest.raises(ValueError, match="trimap_areas_reference: radii"):
            trimap_areas_reference(lab, gt, 5, bad)
    with pytest.raises(ValueError, match="trimap_areas_reference: ground truth must be uint8 or int16"):
        trimap_areas_reference(lab, gt.long(), 5, (1, 2))
    with pytest.raises(ValueError, match="trimap_areas_reference: labels must be integer"):
        trimap_areas_reference(lab.float(), gt, 5, (1, 2))
    with pytest.raises(ValueError, match="trimap_areas_reference: dist"):
        trimap_areas_reference(lab, gt, 5, (1, 2), dist=torch.zeros(3, 4, dtype=torch.int32))
    assert default_trimap_radii() == (1, 2, 4, 8, 16, 32)


# ------------------------------------------------------------------------------------------------- the trimap counters
@pytest.mark.parametrize("outside", [False, True], ids=["inside", "outside"])
@pytest.mark.parametrize("raw", [True, False], ids=["raw", "ids"])
@pytest.mark.parametrize("k", range(len(BC.TABLE)), ids=BC.IDS)
def test_rings_and_the_pixels_beyond_add_up_to_areas(k, raw, outside):
    assert T.trimap_nonempty(k, "i16", raw, outside)
    trimap, areas = T.trimap_reference(k, "i16", raw, outside)
    radii = T.TRIMAP_RADII[k]
    assert trimap.dtype == torch.int64 and trimap.shape == (len(radii), 3, BC.classes(BC.TABLE[k]))
    labels, gt, n = BC.maps(BC.TABLE[k], torch.int16, torch.uint8, raw, outside)
    assert torch.equal(trimap, trimap_areas_reference(labels, gt, n, radii, raw))        # with its own distance plane
    # a ring from the last radius to one that reaches every pixel holds what is left: with it the rings sum to areas
    last, rest = trimap_areas_reference(labels, gt, n, (radii[-1], 128), raw)
    assert torch.equal(last, trimap.sum(0)) and torch.equal(last + rest, areas) and int(rest.sum()) > 0
    assert (trimap.sum(0) <= areas).all() and (trimap[:, 0] <= torch.minimum(trimap[:, 1], trimap[:, 2])).all()


def test_a_last_radius_that_reaches_every_pixel_gives_areas():
    labels, gt, n = BC.maps(BC.TABLE[0], torch.int16, torch.uint8, True, True)
    d2 = distance_reference(gt, 128).long()
    assert int(d2.max()) == 49                                        # no pixel is farther than 7 from another value
    trimap = trimap_areas_reference(labels, gt, n, (1, 4, 11))
    areas = areas_reference(labels, gt, n)[0]
    assert torch.equal(trimap.cumsum(0)[-1], areas) and not torch.equal(trimap.cumsum(0)[1], areas) and int(trimap[2].sum()) > 0
    # two maps at once are the two maps one after the other
    both = trimap_areas_reference(torch.stack([labels, labels.flip(0)]), torch.stack([gt, gt.flip(1)]), n, (1, 4, 11))
    assert torch.equal(both, trimap + trimap_areas_reference(labels.flip(0), gt.flip(1), n, (1, 4, 11)))


def test_trimap_by_hand():
    gt = torch.tensor([[1, 1],
                       [1, 1],
                       [2, 1]], dtype=torch.uint8)
    assert distance_reference(gt, 3).tolist() == [[4, 5], [1, 2], [1, 1]]
    pred = torch.tensor([[0, 1],
                         [0, 0],
                         [1, 5]], dtype=torch.uint8)                  # 5: outside [0, 2)
    assert trimap_areas_reference(pred, gt, 2, (1, 2)).tolist() == [[[1, 1], [1, 1], [2, 1]], [[2, 0], [2, 0], [2, 0]]]
    assert trimap_areas_reference(pred, gt, 2, (1, 2), border=True).tolist() == [[[3, 1], [3, 2], [5, 1]], [[0, 0]] * 3]
    assert trimap_areas_reference(pred, gt, 2, (2,)).tolist() == [[[3, 1], [3, 1], [4, 1]]]
    # two blocks, 2 x 8: the rings are the columns at 1, at 2 .. 3 and beyond 3 from the seam
    gt = torch.tensor([[1, 1, 1, 1, 2, 2, 2, 2]] * 2, dtype=torch.int16)
    pred = torch.zeros(2, 8, dtype=torch.int16)
    assert trimap_areas_reference(pred, gt, 2, (1, 3)).tolist() == [[[2, 0], [4, 0], [2, 2]], [[4, 0], [8, 0], [4, 4]]]
    # an ignore value is a value of its own for the distance, and is never scored
    gt[0, 0] = 0
    assert distance_reference(gt, 8)[:, :4].tolist() == [[1, 1, 4, 1], [1, 2, 4, 1]]
    assert trimap_areas_reference(pred, gt, 2, (1, 3)).tolist() == [[[4, 0], [6, 0], [4, 2]], [[3, 0], [7, 0], [3, 4]]]
    ids = torch.where(gt == 0, torch.full_like(gt, 2), gt - 1)
    assert trimap_areas_reference(pred, ids, 2, (1, 3), raw_labels=False).tolist() == [[[4, 0], [6, 0], [4, 2]], [[3, 0], [7, 0], [3, 4]]]


# ------------------------------------------------------------------------------------------------- the score
def _score(k=3, trimap=True):
    t, areas = T.trimap_reference(k, "i16", True, False)
    n = areas.shape[1]
    return SegmentationScore(n, areas=areas.clone(), tally=torch.tensor([int(areas[2].sum()), 0]),
                             trimap=t.clone() if trimap else None, trimap_radii=T.TRIMAP_RADII[k] if trimap else None)


def test_score_constructor_and_add():
    assert SegmentationScore(7).trimap is None and SegmentationScore(7, trimap=False).trimap is None
    assert SegmentationScore(7).trimap_radii is None
    t = SegmentationScore(7, torch.device("cpu"), trimap=True)
    assert t.trimap.dtype == torch.int64 and t.trimap.shape == (6, 3, 7) and not t.trimap.any() and t.trimap_radii == (1, 2, 4, 8, 16, 32)
    given = torch.zeros(2, 3, 7, dtype=torch.int64)
    s = SegmentationScore(7, trimap=given, trimap_radii=[3, 9])
    assert s.trimap is given and s.trimap_radii == (3, 9)
    for bad in (torch.zeros(3, 3, 7, dtype=torch.int64), torch.zeros(2, 3, 7, dtype=torch.int32), torch.zeros(2, 3, 7), [[0]], 1):
        with pytest.raises(ValueError, match=r"trimap must be None, True or int64 \[2, 3, 7\]"):
            SegmentationScore(7, trimap=bad, trimap_radii=(3, 9))
    for bad in ((), (2, 2), (3, 1), (0, 1), (1, 129), (1.5,), 4, tuple(range(1, 10))):
        with pytest.raises(ValueError, match="SegmentationScore: radii must be"):
            SegmentationScore(7, trimap=True, trimap_radii=bad)
    a, b = _score(), _score()
    b.trimap += 1
    tot = SegmentationScore(a.n, trimap=True, trimap_radii=a.trimap_radii).add_(a).add_(b)
    assert torch.equal(tot.trimap, a.trimap + b.trimap) and torch.equal(tot.areas, 2 * a.areas)
    keep = tot.areas.clone()
    plain = _score(trimap=False)
    with pytest.raises(ValueError, match="trimap counters and the other has none"):
        tot.add_(plain)
    with pytest.raises(ValueError, match="trimap counters and the other has none"):
        plain.add_(a)
    other = SegmentationScore(a.n, trimap=True, trimap_radii=(1, 2, 3, 4))
    with pytest.raises(ValueError, match=r"radii \(2, 5, 12\) against radii \(1, 2, 3, 4\)"):
        tot.add_(other)
    assert torch.equal(tot.areas, keep) and torch.equal(plain.areas, a.areas)
    assert torch.equal(plain.add_(_score(trimap=False)).areas, 2 * a.areas)


def _figures(s):
    c = s.trimap.cumsum(0).double()
    iou = c[:, 0] / (c[:, 1] + c[:, 2] - c[:, 0])
    r4 = lambda v: round(float(v), 4)
    return ([r4(torch.nanmean(row)) for row in iou], [r4(c[k, 0].sum() / c[k, 1].sum()) for k in range(len(c))],
            [int(c[k, 2].sum()) for k in range(len(c))], [[r4(v) for v in row] for row in iou])


def test_summary_gains_the_trimap_curve_and_is_unchanged_without():
    s, plain = _score(), _score(trimap=False)
    got, base = s.summary(), plain.summary()
    assert list(base) == ["aAcc", "mIoU", "mAcc", "IoU", "Acc", "pixels"]
    assert list(got) == list(base) + ["trimap_radii", "trimap_mIoU", "trimap_aAcc", "trimap_pixels"]
    assert repr({k: got[k] for k in base}) == repr(base)
    miou, aacc, pixels, iou = _figures(s)
    assert got["trimap_radii"] == [2, 5, 12] and got["trimap_mIoU"] == miou and got["trimap_aAcc"] == aacc and got["trimap_pixels"] == pixels
    assert pixels == sorted(pixels) and 0 < pixels[0] < pixels[-1] < got["pixels"]
    assert 0 < miou[0] < miou[-1] < got["mIoU"]                       # shifted blocks: the errors sit at the contours
    assert s.trimap_summary() == {k: got[k] for k in got if k.startswith("trimap")}
    per = s.trimap_summary(per_class=True)
    assert list(per) == ["trimap_radii", "trimap_mIoU", "trimap_aAcc", "trimap_pixels", "trimap_IoU"] and per["trimap_IoU"] == iou
    assert len(per["trimap_IoU"]) == 3 and all(len(row) == s.n for row in per["trimap_IoU"])
    with pytest.raises(ValueError, match="needs trimap counters"):
        plain.trimap_summary()
    # beside the boundary and the calibration counters every entry keeps its place
    full = SegmentationScore(s.n, areas=s.areas, tally=s.tally, boundary=BC.reference(3, "i16")[0].clone(), calibration=True,
                             trimap=s.trimap, trimap_radii=s.trimap_radii)
    both = full.summary()
    assert repr({k: both[k] for k in got}) == repr(got) and "mBIoU" in both and "ECE" in both and len(both["cECE"]) == s.n
    only_b = SegmentationScore(s.n, areas=s.areas, tally=s.tally, boundary=full.boundary).summary()
    assert both["mBIoU"] == only_b["mBIoU"] and both["BIoU"] == only_b["BIoU"]
    # an absent class is NaN and stays out of the mean; ground truth out of range is refused as ever
    s.trimap[:, :, 0] = 0
    again = s.trimap_summary(per_class=True)
    assert all(row[0] != row[0] for row in again["trimap_IoU"]) and again["trimap_mIoU"] == _figures(s)[0]
    s.tally[1] = 2
    with pytest.raises(IndexError, match=r"tally\[1\] = 2"):
        s.summary()


def test_group_summary_and_merged():
    s, plain = _score(), _score(trimap=False)
    n = s.n
    groups = {"low": range(0, n // 2), "high": range(n // 2, n)}
    got, base = s.group_summary(groups), plain.group_summary(groups)
    iou = _figures(s)[3]
    c = s.trimap.cumsum(0).double()
    exact = c[:, 0] / (c[:, 1] + c[:, 2] - c[:, 0])
    for name, ids in groups.items():
        want = [round(float(torch.nanmean(row[list(ids)])), 4) for row in exact]
        assert got[name] == dict(base[name], trimap_mIoU=want) and list(base[name]) == ["mIoU", "mAcc"]
    assert got["hIoU"] == base["hIoU"] and len(iou) == 3
    withb = SegmentationScore(n, areas=s.areas, tally=s.tally, boundary=BC.reference(3, "i16")[0].clone(), trimap=s.trimap,
                              trimap_radii=s.trimap_radii).group_summary(groups)
    onlyb = SegmentationScore(n, areas=s.areas, tally=s.tally, boundary=BC.reference(3, "i16")[0].clone()).group_summary(groups)
    for name in groups:
        assert withb[name] == dict(onlyb[name], trimap_mIoU=got[name]["trimap_mIoU"])
    # merged: the coarser score has no trimap counters
    labels, gt, n0 = BC.maps(BC.TABLE[0], torch.int16, torch.uint8)
    areas, tally = areas_reference(labels, gt, n0)
    full = SegmentationScore(n0, areas=areas, tally=tally, confusion=confusion_reference(labels, gt, n0),
                             trimap=trimap_areas_reference(labels, gt, n0, (1, 2, 3)), trimap_radii=(1, 2, 3))
    two = full.merged([c % 2 for c in range(n0)])
    assert two.trimap is None and two.trimap_radii is None and "trimap_mIoU" not in two.summary() and "trimap_mIoU" in full.summary()
    assert "trimap" in SegmentationScore.merged.__doc__


# ------------------------------------------------------------------------------------------------- header, library, refusals
def test_header_declares_the_entries_and_keeps_the_abi_version():
    with open(os.path.join(ROOT, "include", "ifseg_hip.h")) as f:
        header = f.read()
    with open(os.path.join(ROOT, "ifseg_amd", "csrc", "distance.hip")) as f:
        src = f.read()
    for name in ("ifseg_seg_distance", "ifseg_seg_trimap_areas", "ifseg_seg_distance_limit"):
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert 'extern "C" int %s(' % name in src, name
    assert re.search(r"#define\s+IFSEG_ABI_VERSION\s+21\b", header) and hip.ABI_VERSION == 21
    assert int(re.search(r"constexpr int SEG_DISTANCE_MAX = (\d+);", src).group(1)) == hip.SEG_DISTANCE_MAX == 128
    assert int(re.search(r"constexpr int SEG_DISTANCE_FAR = (\d+);", src).group(1)) == hip.SEG_DISTANCE_FAR == 65535 == T.FAR
    assert int(re.search(r"constexpr int SEG_TRIMAP_MAX_RADII = (\d+);", src).group(1)) == hip.SEG_TRIMAP_MAX_RADII == 8
    assert int(re.search(r"constexpr int SD_MAX_CLASSES = (\d+);", src).group(1)) == hip.SEG_PREDICT_MAX_CLASSES
    assert hip.SEG_DISTANCE_MAX ** 2 < hip.SEG_DISTANCE_FAR < 2 ** 16 and len(default_trimap_radii()) <= hip.SEG_TRIMAP_MAX_RADII
    kernels = src.split("seg_trimap_kernel(")[0].split("namespace {")[1]
    assert "atomic" not in kernels and "bin_add" not in kernels       # the two distance launches have no atomics


def test_no_torch_op_was_added():
    import ifseg_amd.ops  # noqa: F401
    assert not any("distance" in name or "trimap" in name for name in dir(torch.ops.ifseg))


def _library():
    if not os.path.exists(hip.LIB_PATH):
        from ifseg_amd.build import build
        build(verbose=False)
    return hip.lib()


def test_library_exports_and_limits():
    lib = _library()
    assert all(hasattr(lib, name) for name in ("ifseg_seg_distance", "ifseg_seg_trimap_areas", "ifseg_seg_distance_limit"))
    assert hip.seg_distance_limits() == (hip.SEG_DISTANCE_MAX, hip.SEG_DISTANCE_FAR, hip.SEG_TRIMAP_MAX_RADII,
                                         hip.SEG_PREDICT_MAX_CLASSES) == (128, 65535, 8, 512)
    assert lib.ifseg_seg_distance_limit(ctypes.c_int(4)) == BAD_ARG and lib.ifseg_seg_distance_limit(ctypes.c_int(-1)) == BAD_ARG


def test_c_entry_refusals_need_no_device():
    """every refusal returns before anything is launched or dereferenced: the buffers are host memory here"""
    lib = _library()
    B, H, W, n, K = 2, 17, 65, 5, 3
    npix = B * H * W
    keep = []

    def buf(nbytes):
        raw = ctypes.create_string_buffer(nbytes + 64)
        keep.append(raw)
        return (ctypes.addressof(raw) + 63) & ~63                 # 64-byte aligned

    a = dict(labels=buf(2 * npix), gt=buf(2 * npix), work=buf(npix), out=buf(2 * npix), dist=buf(2 * npix), trimap=buf(8 * 8 * 3 * 512))
    before = [bytes(raw) for raw in keep]
    ci, vp = ctypes.c_int, ctypes.c_void_p

    def dist(lb=2, b=B, h=H, w=W, r=17, border=0, **ptr):
        p = dict(a, **ptr)
        return lib.ifseg_seg_distance(vp(p["labels"]), ci(lb), ci(b), ci(h), ci(w), ci(r), ci(border), vp(p["work"]), vp(p["out"]), None)

    def tri(lb=2, gb=2, b=B, h=H, w=W, n=n, radii=(1, 4, 9), k=None, **ptr):
        p = dict(a, **ptr)
        table = (ci * max(len(radii), 1))(*radii) if radii is not None else None
        return lib.ifseg_seg_trimap_areas(vp(p["labels"]), ci(lb), vp(p["gt"]), ci(gb), vp(p["dist"]), ci(b), ci(h), ci(w), ci(n),
                                          table, ci(len(radii) if k is None else k), ci(1), vp(p["trimap"]), None)

    for name in ("labels", "work", "out"):
        assert dist(**{name: None}) == BAD_ARG, name
    assert dist(labels=a["labels"] + 1) == BAD_ARG and dist(out=a["out"] + 1) == BAD_ARG      # 2-byte elements at an odd address
    for kw in (dict(lb=0), dict(lb=3), dict(lb=4), dict(lb=-1), dict(r=0), dict(r=129), dict(r=-1)):
        assert dist(**kw) == BAD_ARG, kw
    for kw in (dict(b=0), dict(h=0), dict(w=-1), dict(b=1 << 15, h=1 << 8, w=1 << 8), dict(b=1, h=1 << 16, w=1 << 15)):
        assert dist(**kw) == BAD_SHAPE, kw
    for x, y in (("labels", "work"), ("labels", "out"), ("work", "out")):                    # any two sharing a byte
        assert dist(**{y: a[x]}) == BAD_ARG and dist(**{x: a[y]}) == BAD_ARG, (x, y)
    assert dist(work=a["out"] + 2 * npix - 1) == BAD_ARG and dist(out=a["labels"] + 2 * npix - 2) == BAD_ARG

    for name in ("labels", "gt", "dist", "trimap"):
        assert tri(**{name: None}) == BAD_ARG, name
    assert tri(radii=None, k=3) == BAD_ARG
    assert tri(labels=a["labels"] + 1) == BAD_ARG and tri(gt=a["gt"] + 1) == BAD_ARG and tri(dist=a["dist"] + 1) == BAD_ARG
    assert tri(trimap=a["trimap"] + 4) == BAD_ARG                     # the counters not 8-byte aligned
    for kw in (dict(lb=0), dict(lb=3), dict(gb=0), dict(gb=4), dict(n=0), dict(n=513), dict(n=-1), dict(k=0), dict(k=9), dict(k=-1),
               dict(radii=(0, 1, 2)), dict(radii=(1, 1, 2)), dict(radii=(3, 2, 5)), dict(radii=(1, 2, 129)), dict(radii=(-4,))):
        assert tri(**kw) == BAD_ARG, kw
    for kw in (dict(b=0), dict(h=0), dict(w=-1), dict(b=1 << 15, h=1 << 8, w=1 << 8)):
        assert tri(**kw) == BAD_SHAPE, kw
    for name in ("labels", "gt", "dist"):                             # the counters sharing a byte with a map
        assert tri(trimap=a[name]) == BAD_ARG and tri(trimap=a[name] + ((2 * npix - 8) & ~7)) == BAD_ARG, name
    assert [bytes(raw) for raw in keep] == before                     # nothing was written


def test_binding_refusals_come_before_any_launch(monkeypatch):
    """every one is a ValueError that names its argument, raised on CPU tensors: the library was not reached"""
    monkeypatch.setattr(hip, "lib", lambda: pytest.fail("the library was reached"))
    lab, gt = torch.zeros(2, 4, 6, dtype=torch.uint8), torch.zeros(2, 4, 6, dtype=torch.int16)
    dist, tri = hip.seg_distance, hip.seg_trimap_areas
    plane = torch.zeros(2, 4, 6, dtype=U16)
    shared = torch.zeros(256, dtype=torch.int64)
    for call, what in ((lambda: dist(lab.long(), 3), "labels"), (lambda: dist(lab.float(), 3), "labels"), (lambda: dist([[0]], 3), "labels"),
                       (lambda: dist(lab.transpose(1, 2), 3), "labels"), (lambda: dist(lab.reshape(-1), 3), "labels"),
                       (lambda: dist(lab[None], 3), "labels"), (lambda: dist(lab[:0], 3), "labels"),
                       (lambda: dist(lab, 0), "max_distance"), (lambda: dist(lab, 129), "max_distance"),
                       (lambda: dist(lab, 3.0), "max_distance"), (lambda: dist(lab, True), "max_distance"),
                       (lambda: dist(lab, 3, border=1), "border"), (lambda: dist(lab, 3, border=None), "border"),
                       (lambda: dist(lab, 3, out=plane[0]), "out"), (lambda: dist(lab, 3, out=plane.view(torch.int16)), "out"),
                       (lambda: dist(lab, 3, out=plane.transpose(1, 2)), "out"), (lambda: dist(lab, 3, out=[0]), "out"),
                       (lambda: dist(shared.view(torch.uint8)[:48].view(2, 4, 6), 3, out=shared.view(U16)[:48].view(2, 4, 6)),
                        "out overlaps labels"),
                       (lambda: tri(lab.long(), gt, 5, (1, 2)), "labels"), (lambda: tri(lab[None], gt[None], 5, (1, 2)), "labels"),
                       (lambda: tri(lab, gt.long(), 5, (1, 2)), "gt"), (lambda: tri(lab, gt[:1], 5, (1, 2)), "gt"),
                       (lambda: tri(lab, gt.transpose(1, 2), 5, (1, 2)), "gt"),
                       (lambda: tri(lab, gt, 0, (1, 2)), "n must"), (lambda: tri(lab, gt, 513, (1, 2)), "n must"),
                       (lambda: tri(lab, gt, 5.0, (1, 2)), "n must"),
                       (lambda: tri(lab, gt, 5, ()), "radii"), (lambda: tri(lab, gt, 5, (2, 2)), "radii"), (lambda: tri(lab, gt, 5, (3, 1)), "radii"),
                       (lambda: tri(lab, gt, 5, (0, 1)), "radii"), (lambda: tri(lab, gt, 5, (1, 129)), "radii"), (lambda: tri(lab, gt, 5, 4), "radii"),
                       (lambda: tri(lab, gt, 5, (1.0, 2)), "radii"), (lambda: tri(lab, gt, 5, tuple(range(1, 10))), "radii"),
                       (lambda: tri(lab, gt, 5, (1, 2), border="yes"), "border"),
                       (lambda: tri(lab, gt, 5, (1, 2), trimap=torch.zeros(3, 3, 5, dtype=torch.int64)), "trimap"),
                       (lambda: tri(lab, gt, 5, (1, 2), trimap=torch.zeros(2, 3, 5, dtype=torch.int32)), "trimap"),
                       (lambda: tri(lab, gt, 5, (1, 2), trimap=torch.zeros(2, 5, 3, dtype=torch.int64).transpose(1, 2)), "trimap"),
                       (lambda: tri(lab, gt, 5, (1, 2), dist=plane[0]), "dist"), (lambda: tri(lab, gt, 5, (1, 2), dist=plane.long()), "dist"),
                       (lambda: tri(lab, gt, 5, (1, 2), trimap=shared[:30].view(2, 3, 5), dist=shared.view(U16)[:48].view(2, 4, 6)),
                        "dist overlaps trimap")):
        with pytest.raises(ValueError, match=what):
            call()


def test_evaluate_raw_refuses_before_it_launches(monkeypatch):
    from test_boundary_cpu import _Model, _no_library
    _no_library(monkeypatch)
    monkeypatch.setattr(hip, "image_load", lambda *a, **k: (_ for _ in ()).throw(RuntimeError("image_load was reached")))
    seg = Segmenter(_Model(), category_token_ids=[[31], [32], [33], [34], [35]])
    im, gt = [torch.zeros(60, 90, 3, dtype=torch.uint8)], [torch.zeros(60, 90, dtype=torch.uint8)]
    with pytest.raises(ValueError, match="evaluate_raw: trimap=True, but `into` carries no trimap counters"):
        seg.evaluate_raw(im, gt, into=SegmentationScore(5), trimap=True)
    with pytest.raises(ValueError, match=r"evaluate_raw: trimap asks for the radii \(1, 2, 4, 8, 16, 32\), `into` counts the radii \(1, 2\)"):
        seg.evaluate_raw(im, gt, into=SegmentationScore(5, trimap=True, trimap_radii=(1, 2)), trimap=True)
    with pytest.raises(ValueError, match=r"radii \(1, 3\), `into` counts the radii \(1, 2, 4, 8, 16, 32\)"):
        seg.evaluate_raw(im, gt, into=SegmentationScore(5, trimap=True), trimap=(1, 3))
    for bad in (0, 1, 2.0, "yes", None, (), (2, 1), (1, 200), torch.zeros(6, 3, 5, dtype=torch.int64)):
        with pytest.raises(ValueError, match="evaluate_raw: trimap is True, False or a tuple of radii"):
            seg.evaluate_raw(im, gt, trimap=bad)
    with pytest.raises(ValueError, match="evaluate: trimap=True, but `into` carries no trimap counters"):
        seg.evaluate(torch.zeros(1, 3, 128, 128), torch.zeros(1, 128, 128, dtype=torch.uint8), into=SegmentationScore(5), trimap=True)
    # nothing to score: the empty score has counters when asked for them, and `into` comes back as it was
    empty = seg.evaluate_raw([], [], trimap=(2, 9))
    assert empty.trimap.shape == (2, 3, 5) and not empty.trimap.any() and empty.trimap_radii == (2, 9)
    assert seg.evaluate_raw([], [], trimap=True).trimap_radii == default_trimap_radii()
    assert seg.evaluate_raw([], []).trimap is None and seg.evaluate_raw([], [], trimap=False).trimap is None
    into = SegmentationScore(5, trimap=True)
    assert seg.evaluate_raw([], [], into=into) is into and seg.evaluate_raw([], [], into=into, trimap=True) is into
    assert seg.evaluate_raw([], [], into=into, trimap=[1, 2, 4, 8, 16, 32]) is into


# ------------------------------------------------------------------------------------------------- the launches
RADII = (1, 3, 9)


class Recorder(BoundaryRecorder):
    def __init__(self, monkeypatch):
        super().__init__(monkeypatch)
        monkeypatch.setattr(hip, "seg_trimap_areas", self.seg_trimap_areas)
        monkeypatch.setattr(hip, "seg_distance", lambda *a, **k: pytest.fail("seg_distance was reached past seg_trimap_areas"))

    def seg_trimap_areas(self, labels, gt, n, radii, raw_labels=True, border=False, trimap=None, dist=None):
        assert labels.is_contiguous() and labels.shape == gt.shape and labels.dim() == 3 and n == L.N and dist is None and not border
        self.log.append(("seg_trimap_areas", tuple(labels.shape), tuple(radii), dict(counters=trimap is not None, raw_labels=raw_labels)))
        return trimap, None


def _with_trimap(want, radii, last):
    """the expected log of a run without trimap counters -> with them: every scoring launch is asked for its label map, and one
    seg_trimap_areas follows each image's last counting launch"""
    out = []
    for e in want:
        if e[0].startswith("seg_score"):
            e = e[:3] + (dict(e[3], labels=True),)
        out.append(e)
        if e[0].startswith(last):
            shape = e[2] if e[0].startswith("seg_score") else e[1]
            out.append(("seg_trimap_areas", shape, radii, dict(counters=True, raw_labels=True)))
    return out


@pytest.mark.parametrize("others", [False, True], ids=["alone", "with_confusion_and_boundary"])
@pytest.mark.parametrize("crf", [False, True], ids=["plain", "crf"])
@pytest.mark.parametrize("setting", list(L.SETTINGS))
def test_raw_launch_sequence_with_and_without_trimap(monkeypatch, setting, crf, others):
    imgs, gts = L._images()
    kw = dict(max_batch=3, confusion=others, boundary_iou=others, **L.SETTINGS[setting][2])
    base = L._expected(setting, crf, "evaluate_raw_confusion" if others else "evaluate_raw")
    if others:
        base = _with_boundary(base, 0.02, True, crf)
    last = "seg_boundary_areas" if others else "seg_areas" if crf else "seg_score"
    for trimap, radii in ((False, None), (True, default_trimap_radii()), (RADII, RADII), (list(RADII), RADII)):
        rec = Recorder(monkeypatch)
        seg = Segmenter(L._Model(), category_token_ids=[[1]] * L.N, crf_iters=2 if crf else 0, **L.SETTINGS[setting][1])
        score = seg.evaluate_raw(imgs, gts, trimap=trimap, **kw)
        assert (score.trimap is not None) == (radii is not None) and score.trimap_radii == radii
        assert (score.confusion is not None) == others == (score.boundary is not None)
        want = base if radii is None else _with_trimap(base, radii, last)
        assert rec.log == want, (trimap, rec.log, want)
        if radii is not None:
            calls = [e for e in rec.log if e[0] == "seg_trimap_areas"]
            assert [(e[1], e[2]) for e in calls] == [((1,) + hw, radii) for hw in (L.A, L.B)]
            # an `into` that carries the counters decides without the keyword
            del rec.log[:]
            assert seg.evaluate_raw(imgs, gts, into=score, **kw) is score and rec.log == want


@pytest.mark.parametrize("setting", list(L.SETTINGS))
def test_a_segmenter_that_counts_no_trimap_launches_what_it_did(monkeypatch, setting):
    rec = L.Recorder(monkeypatch)
    for name in ("seg_distance", "seg_trimap_areas"):
        monkeypatch.setattr(hip, name, lambda *a, **k: pytest.fail("a distance binding was reached"))
    for crf in (False, True):
        seg = Segmenter(L._Model(), category_token_ids=[[1]] * L.N, crf_iters=2 if crf else 0, **L.SETTINGS[setting][1])
        imgs, gts = L._images()
        for kw in ({}, dict(trimap=False)):
            del rec.log[:]
            seg.evaluate_raw(imgs, gts, max_batch=3, **kw, **L.SETTINGS[setting][2])
            assert rec.log == L._expected(setting, crf, "evaluate_raw")
        del rec.log[:]
        seg.segment_raw(imgs, max_batch=3, return_conf=True, **L.SETTINGS[setting][2])
        assert rec.log == L._expected(setting, crf, "segment_raw")


@pytest.mark.parametrize("crf", [False, True], ids=["plain", "crf"])
def test_evaluate_launch_sequence_with_trimap(monkeypatch, crf):
    """`evaluate` takes a ready batch: one seg_trimap_areas for the whole batch behind its other counting launches"""
    rec = Recorder(monkeypatch)
    seg = Segmenter(L._Model(), category_token_ids=[[1]] * L.N, crf_iters=2 if crf else 0)
    x = torch.stack([rec.coded(("x", b), 3, 32, 48) for b in range(2)])
    gt = torch.ones(2, 32, 48, dtype=torch.uint8)
    logs = {}
    for others in (False, True):
        for trimap in (False, RADII):
            del rec.log[:]
            score = seg.evaluate(x, gt, confusion=others, boundary_iou=others, trimap=trimap)
            assert (score.trimap is not None) == (trimap is not False)
            logs[others, trimap is not False] = list(rec.log)
    for others in (False, True):
        want = [e[:3] + (dict(e[3], labels=True),) if e[0] == "seg_score" else e for e in logs[others, False]]
        want.append(("seg_trimap_areas", (2, 32, 48), RADII, dict(counters=True, raw_labels=True)))
        assert logs[others, True] == want
    assert logs[False, False][-1][0] == ("seg_areas" if crf else "seg_score") and logs[True, False][-1][0] == "seg_boundary_areas"


def test_task_hands_the_keyword_on(monkeypatch):
    from ifseg_amd.tasks.mm_tasks import SegmentationTask
    task = SegmentationTask(num_seg_tokens=5, patch_image_size=64, n_base_vocab=100, category_token_ids=[[5]] * 5)
    seen = []

    class Seg:
        def __getattr__(self, name):
            return lambda *a, **kw: seen.append((name, kw))

    monkeypatch.setattr(task, "build_segmenter", lambda model, **kw: seen.append(("ctor", kw)) or Seg())
    task.evaluate_raw(None, [], [], sieve=16, trimap=(1, 2, 4), max_batch=2)
    assert seen == [("ctor", dict(sieve=16)), ("evaluate_raw", dict(slide=None, trimap=(1, 2, 4), max_batch=2))]
    assert "trimap" in SegmentationTask.evaluate_raw.__doc__
