"""CPU: the specifications of the connected-region kernels (ifseg_amd/predict.py: regions_reference, region_drop_reference)
against hand-written answers and scipy.ndimage.label, a Python transcription of csrc/regions.hip's decomposition against the
specification, every refusal that comes before a launch, the header, and which `hip` calls `Segmenter.pseudo_label_raw` makes
without and with min_region."""
import os
import re

import pytest
import torch

import _regions_cases as C
from ifseg_amd import hip, ops
from ifseg_amd.predict import PseudoLabelResult, Segmenter, region_drop_reference, regions_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32 = torch.int32


def t32(rows):
    return torch.tensor(rows, dtype=I32)


# ------------------------------------------------------------------------------------------------- hand-written answers
def test_reference_by_hand():
    # 1: a diagonal pair joins at connectivity 8 only; the value 255 and a value of its own are regions like any other
    lab = torch.tensor([[1, 0, 255],
                        [0, 1, 255]], dtype=torch.uint8)
    root, size = regions_reference(lab, 4)
    assert root.dtype == I32 and size.dtype == I32
    assert torch.equal(root, t32([[0, 1, 2], [3, 4, 2]])) and torch.equal(size, t32([[1, 1, 2], [1, 1, 2]]))
    root, size = regions_reference(lab, 8)
    assert torch.equal(root, t32([[0, 1, 2], [1, 0, 2]])) and torch.equal(size, t32([[2, 2, 2], [2, 2, 2]]))
    # 2: a ring around a pixel of its own value that it does not touch; negative int16 values
    lab = torch.tensor([[-2, -2, -2, -2, -2],
                        [-2, 7, 7, 7, -2],
                        [-2, 7, -2, 7, -2],
                        [-2, 7, 7, 7, -2],
                        [-2, -2, -2, -2, -2]], dtype=torch.int16)
    for conn in (4, 8):
        root, size = regions_reference(lab, conn)
        want_root = torch.zeros(5, 5, dtype=I32)
        want_root[1:4, 1:4] = 6
        want_root[2, 2] = 12
        want_size = torch.full((5, 5), 16, dtype=I32)
        want_size[1:4, 1:4] = 8
        want_size[2, 2] = 1
        assert torch.equal(root, want_root) and torch.equal(size, want_size)
    # 3: a batch whose images would join through their touching rows; a U whose smallest index is not where a scan starts it
    lab = torch.tensor([[[3, 0, 3],
                         [3, 3, 3]],
                        [[3, 3, 3],
                         [0, 0, 0]]], dtype=torch.int64)
    root, size = regions_reference(lab, 4)
    assert torch.equal(root, t32([[[0, 1, 0], [0, 0, 0]], [[0, 0, 0], [3, 3, 3]]]))
    assert torch.equal(size, t32([[[5, 1, 5], [5, 5, 5]], [[3, 3, 3], [3, 3, 3]]]))


# ------------------------------------------------------------------------------------------------- scipy
def _scipy_answer(lab, conn):
    """scipy.ndimage.label per distinct value, the component's smallest flat index and its bincount"""
    import numpy as np
    from scipy import ndimage
    a = lab.numpy()
    H, W = a.shape
    structure = np.ones((3, 3), dtype=int) if conn == 8 else None
    root = np.zeros((H, W), dtype=np.int64)
    size = np.zeros((H, W), dtype=np.int64)
    flat = np.arange(H * W).reshape(H, W)
    for v in np.unique(a):
        comp, k = ndimage.label(a == v, structure=structure)
        if k == 0:
            continue
        idx = np.arange(1, k + 1)
        mins = ndimage.minimum(flat, comp, idx)
        counts = np.bincount(comp.reshape(-1), minlength=k + 1)
        mask = comp > 0
        root[mask] = np.asarray(mins)[comp[mask] - 1]
        size[mask] = counts[comp[mask]]
    return torch.from_numpy(root).to(I32), torch.from_numpy(size).to(I32)


@pytest.mark.parametrize("conn", C.CONNECTIVITIES)
@pytest.mark.parametrize("name", C.PATTERNS)
def test_reference_against_scipy(name, conn):
    pytest.importorskip("scipy")
    for key in C.case_keys((name,)):
        root, size = C.reference(key, conn)
        want_root, want_size = _scipy_answer(C.labels_of(key), conn)
        assert torch.equal(root, want_root) and torch.equal(size, want_size), key


@pytest.mark.parametrize("conn", C.CONNECTIVITIES)
def test_reference_batches_do_not_join(conn):
    for key in ("batch", "batch_constant", "batch_short"):
        lab = C.labels_of(key)
        root, size = C.reference(key, conn)
        assert root.shape == lab.shape
        for b in range(lab.shape[0]):
            r, s = regions_reference(lab[b], conn)
            assert torch.equal(root[b], r) and torch.equal(size[b], s), (key, b)
    lab = C.labels_of("batch_constant")
    assert int(C.reference("batch_constant", conn)[1].max()) == lab.shape[1] * lab.shape[2]


def test_checkerboard_and_serpentine_are_what_they_claim():
    lab = C.case("checkerboard", 33, 129)
    assert int(C.reference(("checkerboard", 33, 129, False), 4)[1].max()) == 1
    root8 = C.reference(("checkerboard", 33, 129, False), 8)[0]
    assert sorted(root8.unique().tolist()) == [0, 1]
    size = C.reference(("serpentine", 33, 129, False), 4)[1]
    assert int(size.max()) == 17 * 129 + 16 and int(size[0, 0]) == int(size.max())         # one chain of about 2 200 pixels
    assert lab.shape == (33, 129)


# ------------------------------------------------------------------------------------------------- the decomposition
DECOMPOSED = ((16, 64), (17, 65), (33, 129), (48, 200), (1, 200), (33, 1), (3, 2))


@pytest.mark.parametrize("conn", C.CONNECTIVITIES)
@pytest.mark.parametrize("name", C.PATTERNS)
def test_decomposition_equals_the_specification(name, conn):
    """tile-local roots, the seam unions in shuffled orders with many in flight, the flatten, the summed local counts"""
    for H, W in DECOMPOSED:
        short = name in C.INT16_PATTERNS and (H + W) % 2 == 1
        key = (name, H, W, short)
        want_root, want_size = C.reference(key, conn)
        for seed in range(3):
            root, size, atomics = C.decomposition(C.labels_of(key), conn, seed)
            assert torch.equal(root, want_root) and torch.equal(size, want_size), (key, seed)
        if name == "checkerboard" and conn == 4:
            assert atomics == 0                                   # pairs whose values differ issue nothing
        if name == "constant":
            tiles_y, tiles_x = -(-H // 16), -(-W // 64)
            # one atomic per tile that joins an earlier one: roots that already agree issue none
            assert atomics >= tiles_y * tiles_x - 1


# ------------------------------------------------------------------------------------------------- the drop rule
@pytest.mark.parametrize("conn", C.CONNECTIVITIES)
def test_region_drop_reference(conn):
    g = torch.Generator().manual_seed(5)
    for name, H, W, n in (("random2", 33, 130, 4), ("random5", 33, 130, 4), ("blocks", 48, 200, 5)):
        lab = C.pattern(name, H, W) if name == "blocks" else torch.randint(0, int(name[-1]), (H, W), generator=g).to(torch.uint8)
        root, size = regions_reference(lab, conn)
        weight = torch.randint(1, 256, (H, W), generator=g).to(torch.uint8)
        out, dropped = region_drop_reference(lab, size, 1, n=n)
        assert torch.equal(out, lab) and not dropped.any()        # min_region = 1 is the identity
        out, dropped, wt = region_drop_reference(lab, size, H * W + 1, fill=255, n=n, weight=weight)
        assert bool((out == 255).all()) and not wt[lab != 255].any() and torch.equal(wt[lab == 255], weight[lab == 255])
        for K in (2, 8):
            for raw in (True, False):
                for fill in (255, 0):
                    out, dropped, wt = region_drop_reference(lab, size, K, fill=fill, n=n, raw_labels=raw, weight=weight)
                    changed = out != lab
                    want = (lab != fill) & (size < K)
                    assert torch.equal(changed, want)
                    if name != "blocks":
                        assert bool(changed.any()) and bool((~changed & (lab != fill)).any())   # both sets are non-empty
                    assert bool((out[changed] == fill).all()) and torch.equal(out[~changed], lab[~changed])
                    assert not wt[changed].any() and torch.equal(wt[~changed], weight[~changed])
                    cls = lab.long() - (1 if raw else 0)
                    inr = (cls >= 0) & (cls < n)
                    assert dropped.dtype == torch.int64 and tuple(dropped.shape) == (n,)
                    assert int(dropped.sum()) == int((changed & inr).sum())
                    for c in range(n):
                        assert int(dropped[c]) == int((changed & (cls == c)).sum())
                    # regions of the value `fill` are never touched, and a second pass over the result drops nothing new
                    assert torch.equal(out == fill, (lab == fill) | changed)
    # n None: every class a uint8 map holds
    assert tuple(region_drop_reference(lab, size, 2)[1].shape) == (254,)
    assert tuple(region_drop_reference(lab, size, 2, raw_labels=False)[1].shape) == (255,)


# ------------------------------------------------------------------------------------------------- refusals
def test_reference_refusals():
    lab = torch.zeros(3, 4, dtype=torch.uint8)
    size = torch.ones(3, 4, dtype=I32)
    for conn in (0, 6, 4.0, "8", True, None):
        with pytest.raises(ValueError, match="connectivity"):
            regions_reference(lab, conn)
    for bad in (lab.float(), lab.bool(), lab.reshape(-1), lab.reshape(1, 1, 3, 4), torch.zeros(0, 4, dtype=torch.uint8)):
        with pytest.raises(ValueError, match="labels"):
            regions_reference(bad)
    for K in (0, -1, 2.0, True, None, 2 ** 31):
        with pytest.raises(ValueError, match="min_region"):
            region_drop_reference(lab, size, K)
    for kw, what in ((dict(fill=256), "fill"), (dict(fill=-1), "fill"), (dict(fill=1.0), "fill"), (dict(n=0), "n must"),
                     (dict(n=256), "n must"), (dict(weight=torch.zeros(3, 5)), "weight")):
        with pytest.raises(ValueError, match=what):
            region_drop_reference(lab, size, 2, **kw)
    with pytest.raises(ValueError, match="size"):
        region_drop_reference(lab, size[:2], 2)
    with pytest.raises(ValueError, match="size"):
        region_drop_reference(lab, size.float(), 2)


def test_binding_refusals_come_before_any_launch(monkeypatch):
    """every one is a ValueError that names its argument, raised on CPU tensors: the library was not reached"""
    monkeypatch.setattr(hip, "lib", lambda: pytest.fail("the library was reached"))
    lab = torch.zeros(3, 4, dtype=torch.uint8)
    for call, what in ((lambda: hip.seg_regions(lab, 6), "connectivity"), (lambda: hip.seg_regions(lab, True), "connectivity"),
                       (lambda: hip.seg_regions(lab.long()), "labels"), (lambda: hip.seg_regions(lab.reshape(-1)), "labels"),
                       (lambda: hip.seg_regions(lab.t()), "labels"), (lambda: hip.seg_regions([[0]]), "labels"),
                       (lambda: hip.seg_regions(lab, root=torch.zeros(3, 4)), "root"),
                       (lambda: hip.seg_regions(lab, size=torch.zeros(4, 3, dtype=I32)), "size"),
                       (lambda: hip.seg_regions(lab, flag=torch.zeros(2, dtype=I32)), "flag"),
                       (lambda: hip.seg_regions(lab, flag=torch.zeros(1)), "flag"),
                       (lambda: hip.seg_region_drop(lab.to(torch.int16), 4, 2), "labels"),
                       (lambda: hip.seg_region_drop(lab, 5, 2), "connectivity"),
                       (lambda: hip.seg_region_drop(lab, 4, 0), "min_region"), (lambda: hip.seg_region_drop(lab, 4, 2.0), "min_region"),
                       (lambda: hip.seg_region_drop(lab, 4, 2 ** 31), "min_region"),
                       (lambda: hip.seg_region_drop(lab, 4, 2, fill=256), "fill"), (lambda: hip.seg_region_drop(lab, 4, 2, n=0), "n must"),
                       (lambda: hip.seg_region_drop(lab, 4, 2, n=256), "n must"),
                       (lambda: hip.seg_region_drop(lab, 4, 2, weight=torch.zeros(3, 4)), "weight"),
                       (lambda: hip.seg_region_drop(lab, 4, 2, out=lab), "out"),
                       (lambda: hip.seg_region_drop(lab, 4, 2, out=torch.zeros(3, 4, dtype=I32)), "out"),
                       (lambda: hip.seg_region_drop(lab, 4, 2, n=3, dropped=torch.zeros(4, dtype=torch.int64)), "dropped"),
                       (lambda: hip.seg_region_drop(lab, 4, 2, n=3, dropped=torch.zeros(3, dtype=I32)), "dropped")):
        with pytest.raises(ValueError, match=what):
            call()
    same = torch.zeros(3, 4, dtype=I32)
    with pytest.raises(ValueError, match="root and size"):
        hip.seg_regions(lab, root=same, size=same)
    assert hip.SEG_REGION_MAX_CLASSES == 255


def test_ops_are_registered_with_fake_kernels():
    """the fake kernels run the real ones' check helper first, and give the real ones' shapes and dtypes"""
    from torch._subclasses.fake_tensor import FakeTensorMode
    assert ops.seg_regions is not None and ops.seg_region_drop is not None
    regions_op, drop_op = torch.ops.ifseg.seg_regions, torch.ops.ifseg.seg_region_drop
    with FakeTensorMode():
        lab = torch.empty(2, 17, 65, dtype=torch.uint8, device="cuda")
        root, size = regions_op(lab, 8)
        assert root.shape == lab.shape and size.shape == lab.shape and root.dtype == I32 and size.dtype == I32 and root.is_cuda
        root, size = regions_op(lab[0].to(torch.int16), 4)
        assert root.shape == (17, 65) and size.dtype == I32
        out, dropped, size = drop_op(lab, 4, 8, 255, 150, True)
        assert out.shape == lab.shape and out.dtype == torch.uint8 and tuple(dropped.shape) == (150,) and dropped.dtype == torch.int64
        assert size.shape == lab.shape and size.dtype == I32 and out.is_cuda
        for bad in (lambda: regions_op(lab, 6), lambda: regions_op(lab.float(), 4), lambda: regions_op(lab.reshape(-1), 4),
                    lambda: drop_op(lab.to(torch.int16), 4, 8, 255, 150, True), lambda: drop_op(lab, 4, 0, 255, 150, True),
                    lambda: drop_op(lab, 4, 8, 256, 150, True), lambda: drop_op(lab, 4, 8, 255, 256, True),
                    lambda: drop_op(lab, 5, 8, 255, 150, True)):
            with pytest.raises(ValueError, match="ifseg::seg_region"):
                bad()


# ------------------------------------------------------------------------------------------------- the header
def test_header_declares_the_entry_points_and_keeps_the_abi():
    with open(os.path.join(ROOT, "include", "ifseg_hip.h")) as f:
        text = f.read()
    assert int(re.search(r"#define\s+IFSEG_ABI_VERSION\s+(\d+)", text).group(1)) == 21 == hip.ABI_VERSION
    for name in ("ifseg_seg_regions", "ifseg_seg_region_drop", "ifseg_seg_regions_limit"):
        assert re.search(r"^int %s\(" % name, text, re.M), name
    with open(os.path.join(ROOT, "ifseg_amd", "csrc", "regions.hip")) as f:
        src = f.read()
    for name in ("ifseg_seg_regions", "ifseg_seg_region_drop", "ifseg_seg_regions_limit"):
        assert 'extern "C" int %s(' % name in src, name


# ------------------------------------------------------------------------------------------------- the Segmenter's calls
def _recorder(monkeypatch):
    from test_pseudo_cpu import Recorder

    class Rec(Recorder):
        def __init__(self, monkeypatch):
            super().__init__(monkeypatch)
            monkeypatch.setattr(hip, "seg_region_drop", self.seg_region_drop)
            monkeypatch.setattr(hip, "seg_regions", lambda *a, **k: pytest.fail("an unrecorded binding was reached"))
            self.pseudo_out = []

        def seg_pseudo(self, labels, conf, thresholds, n, boundary=0, raw_labels=True, kept=None, out=None, weight=False):
            if weight:
                res = super().seg_pseudo(labels, conf, thresholds, n, boundary, raw_labels, kept, out)
                res = res + (torch.full(labels.shape, 9, dtype=torch.uint8),)
            else:
                res = super().seg_pseudo(labels, conf, thresholds, n, boundary, raw_labels, kept, out)
            res[1][0] += 10                                       # ten kept pixels per class
            self.pseudo_out.append(res)
            return res

        def seg_region_drop(self, labels, connectivity=4, min_region=1, fill=255, n=None, raw_labels=True, weight=None, out=None,
                            dropped=None, flag=None):
            image = [i for i, res in enumerate(self.pseudo_out) if res[0] is labels]
            assert len(image) == 1 and out is None and dropped is None and flag is None       # the FILTERED map of one image
            assert (weight is None) == (len(self.pseudo_out[image[0]]) == 2)
            assert weight is None or weight is self.pseudo_out[image[0]][2]
            self.log.append(("seg_region_drop", image[0], tuple(labels.shape), connectivity, min_region, fill, n, raw_labels,
                             weight is not None))
            return torch.full(labels.shape, 254, dtype=torch.uint8), torch.arange(n, dtype=torch.int64), None

    return Rec(monkeypatch)


@pytest.mark.parametrize("weight", [False, True], ids=["plain", "weight"])
def test_pseudo_label_raw_makes_one_more_call_per_image(monkeypatch, weight):
    from test_pseudo_cpu import A, B, N, _Model, _images
    thr = torch.tensor([0, 256, 3, 77, 128], dtype=torch.int32)
    kw = dict(thresholds=thr, boundary=1, max_batch=3, return_weight=weight)

    rec0 = _recorder(monkeypatch)
    out0 = Segmenter(_Model(), category_token_ids=[[1]] * N).pseudo_label_raw(_images(), **kw)
    before = rec0.log
    assert [e[0] for e in before].count("seg_pseudo") == 2 and not any(e[0] == "seg_region_drop" for e in before)
    assert all(r.region_dropped is None and len(r) == 5 for r in out0)
    assert all(int(r.kept[0, c]) == 10 for r in out0 for c in range(N))

    rec = _recorder(monkeypatch)
    out = Segmenter(_Model(), category_token_ids=[[1]] * N).pseudo_label_raw(_images(), min_region=8, region_connectivity=8, **kw)
    # exactly the previous calls, and behind each image's filter launch one drop on that image's filtered map
    drops = [e for e in rec.log if e[0] == "seg_region_drop"]
    assert [e for e in rec.log if e[0] != "seg_region_drop"] == before
    assert drops == [("seg_region_drop", 0, A, 8, 8, 255, N, True, weight), ("seg_region_drop", 1, B, 8, 8, 255, N, True, weight)]
    assert [e[0] for e in rec.log[-4:]] == ["seg_pseudo", "seg_region_drop", "seg_pseudo", "seg_region_drop"]
    for r in out:
        assert isinstance(r, PseudoLabelResult) and len(r) == 5 and bool((r.labels == 254).all())
        assert r.region_dropped.tolist() == list(range(N)) and r.kept[0].tolist() == [10 - c for c in range(N)]
        assert (r.weight is not None) == weight

    seg = Segmenter(_Model(), category_token_ids=[[1]] * N)
    del rec.log[:]
    for bad, what in ((dict(min_region=0), "min_region"), (dict(min_region=2.5), "min_region"), (dict(min_region=True), "min_region"),
                      (dict(min_region=8, region_connectivity=6), "region_connectivity"), (dict(region_connectivity=5), "region_connectivity")):
        with pytest.raises(ValueError, match=what):
            seg.pseudo_label_raw(_images(), **bad)
    assert rec.log == []


def test_pseudo_label_result_keeps_its_tuple():
    a, b, c, d, e, f = (torch.zeros(1) for _ in range(6))
    r = PseudoLabelResult(a, b, c, d, e, region_dropped=f)
    assert tuple(r) == (a, b, c, d, e) and r.region_dropped is f and r.weight is e
    assert PseudoLabelResult(a, b, c, d).region_dropped is None
    labels, predicted, conf, kept, weight = r


def test_dacs_sample_passes_the_keywords_through(monkeypatch):
    from ifseg_amd.tasks.mm_tasks import SegmentationTask
    task = SegmentationTask(num_seg_tokens=5, patch_image_size=64, n_base_vocab=100, category_token_ids=[[5]] * 5)
    seen = {}
    monkeypatch.setattr(task, "train_sample", lambda *a, **k: "source")
    monkeypatch.setattr(task, "mix_samples", lambda *a, **k: "mixed")

    def self_train_sample(model, unlabeled, first, trainer=None, confidence_weight=False, **kw):
        seen.update(kw, confidence_weight=confidence_weight)
        return "target"

    monkeypatch.setattr(task, "self_train_sample", self_train_sample)
    assert task.dacs_sample(None, [torch.zeros(4, 4, 3, dtype=torch.uint8)], [None], [None], 0, min_region=8, region_connectivity=8) == "mixed"
    assert seen == dict(min_region=8, region_connectivity=8, confidence_weight=True)
    for name in ("pseudo_label_raw", "self_train_sample", "dacs_sample"):
        assert "min_region" in getattr(SegmentationTask, name).__doc__ and "region_connectivity" in getattr(SegmentationTask, name).__doc__
