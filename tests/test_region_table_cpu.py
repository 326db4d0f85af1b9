"""CPU: the region table (ifseg_amd/predict.py: region_table_reference, RegionTable, Segmenter.regions_raw / regions;
hip.seg_region_table; csrc/regiontab.hip) without a device.  The specification against a brute-force flood fill on every case and
setting of tests/_region_table_cases.py and against scipy.ndimage where it imports; the fixed-point identity; a Python
transcription of the kernels' decomposition against the specification; every refusal, of the specification, the binding, the
Segmenter and the C entry; the header; the launches a Segmenter makes, recorded by fakes; `RegionTable.to_list` by hand."""
import ctypes
import os
import re

import pytest
import torch

import _region_table_cases as T
import _regions_cases as C
import test_segmenter_launches_cpu as L
from test_sieve_cpu import Recorder as SieveRecorder, _sieved, K as SIEVE_K, CONN as SIEVE_CONN, PASSES as SIEVE_PASSES
from ifseg_amd import hip
from ifseg_amd.predict import RegionTable, Segmenter, conf_bin, conf_q16, region_table_reference, regions_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_SHAPE, BAD_ARG = -2, -3


# ------------------------------------------------------------------------------------------------- the specification
def _assert_equals_flood(key, conn, setting):
    rows, sums, count, slot = T.reference(key, conn, setting)
    R = setting[2]
    lab = T.labels_of(key)
    H, W = lab.shape[-2:]
    assert rows.dtype == torch.int32 and sums.dtype == torch.int64 and count.dtype == torch.int32 and slot.dtype == torch.int32
    assert tuple(rows.shape) == tuple(lab.shape[:-2]) + (R, 8) and tuple(sums.shape) == tuple(lab.shape[:-2]) + (R, 3)
    assert tuple(count.shape) == tuple(lab.shape[:-2]) and slot.shape == lab.shape
    want = T.flood_table(key, conn, setting)
    got = T.written(rows, sums, count, R)
    for b, ((w_rows, w_sums, w_count, w_slot), (g_rows, g_sums)) in enumerate(zip(want, got)):
        what = (key, conn, setting, b)
        assert int(count.reshape(-1)[b]) == w_count, what
        assert g_rows.tolist() == w_rows and g_sums.tolist() == w_sums, what
        assert slot.reshape(-1, H, W)[b].tolist() == w_slot, what
        k = min(w_count, R)
        assert not rows.reshape(-1, R, 8)[b, k:].any() and not sums.reshape(-1, R, 3)[b, k:].any(), what   # zero behind
    return count


@pytest.mark.parametrize("conn", T.CONNECTIVITIES)
@pytest.mark.parametrize("name", T.PATTERNS + ("batches",))
def test_reference_equals_the_flood_fill(name, conn):
    keys = T.BATCHES if name == "batches" else T.case_keys((name,))
    truncated = 0
    for key in keys:
        for setting in T.SETTINGS:
            count = _assert_equals_flood(key, conn, setting)
            truncated += int((count > setting[2]).sum())
    assert truncated > 0 or name == "constant"                    # max_regions 1 and 7 cut tables short (one region: never)


def test_reference_is_regions_reference_and_takes_its_planes():
    lab = T.labels_of(("blocks", 33, 129, False))
    a = region_table_reference(lab, None, 8, 2, None, 50)
    b = region_table_reference(lab, None, 8, 2, None, 50, regions=regions_reference(lab, 8))
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    rows, _, count, slot = a
    root, size = regions_reference(lab, 8)
    k = min(int(count), 50)
    on = slot >= 0
    assert torch.equal(rows[:k, 1].long()[slot[on].long()], root[on].long())
    assert torch.equal(rows[:k, 2].long()[slot[on].long()], size[on].long())
    assert bool((rows[1:k, 1] > rows[:k - 1, 1]).all())           # ascending roots


@pytest.mark.parametrize("conn", T.CONNECTIVITIES)
def test_reference_equals_scipy(conn):
    """the boxes from find_objects and the sums from sum_labels on the specification's own slot plane, and the number of
    components from scipy's labelling of every value"""
    ndimage = pytest.importorskip("scipy.ndimage")
    import numpy as np
    structure = np.ones((3, 3), dtype=int) if conn == 8 else None
    for key in T.case_keys():
        lab = T.labels_of(key)
        H, W = lab.shape
        rows, sums, count, slot = T.reference(key, conn, (1, False, 4096, True))
        a = lab.numpy().astype(np.int64)
        assert sum(ndimage.label(a == v, structure)[1] for v in np.unique(a)) == int(count), (key, conn)
        k = min(int(count), 4096)
        comp = slot.numpy().astype(np.int64) + 1                  # 0: no row
        boxes = ndimage.find_objects(comp, max_label=k)
        assert [(s[1].start, s[0].start, s[1].stop - 1, s[0].stop - 1) for s in boxes] == [tuple(r) for r in rows[:k, 3:7].tolist()]
        idx = np.arange(1, k + 1)
        ys, xs = np.mgrid[0:H, 0:W]
        q = T.q16(T.conf_of(key).numpy())
        for col, plane in enumerate((xs, ys, q)):
            got = ndimage.sum_labels(plane.astype(np.float64), comp, idx)       # exact: the sums are far below 2^53
            assert got.astype(np.int64).tolist() == sums[:k, col].tolist(), (key, conn, col)
        assert ndimage.sum_labels(np.ones((H, W)), comp, idx).astype(np.int64).tolist() == rows[:k, 2].tolist()


def test_q16_and_the_confidence_bin():
    """conf_q16(c) >> 8 == conf_bin(c): on every fp32 whose low 8 mantissa bits are zero (2^24 patterns: every exponent, both
    signs, NaNs and infinities), on the floats around every k / 65536, and on 2^22 random bit patterns"""
    g = torch.Generator().manual_seed(5)
    every = (torch.arange(1 << 24, dtype=torch.int64) << 8).to(torch.int32).view(torch.float32)
    k = torch.arange(0, 65537, dtype=torch.float32) / 65536.0
    around = torch.cat([(k.view(torch.int32) + d).view(torch.float32) for d in (-2, -1, 0, 1, 2)])
    rnd = torch.randint(-2 ** 31, 2 ** 31, (1 << 22,), generator=g, dtype=torch.int64).to(torch.int32).view(torch.float32)
    special = torch.tensor([float("nan"), float("inf"), -float("inf"), 0.0, -0.0, 1.0, 0.99999994, 3.0e38, -1.0, 1e-45, 2.0 ** -16])
    for c in (every, around, rnd, special):
        q = conf_q16(c)
        assert q.dtype == torch.int64 and int(q.min()) >= 0 and int(q.max()) <= 65535
        assert torch.equal(q >> 8, conf_bin(c))
    assert conf_q16(special).tolist() == [0, 65535, 0, 0, 0, 65535, 65535, 65535, 0, 0, 1]
    import numpy as np
    assert T.q16(special.numpy()).tolist() == conf_q16(special).tolist()
    assert np.array_equal(T.q16(rnd.numpy()), conf_q16(rnd).numpy())


def test_reference_by_hand():
    lab = torch.tensor([[1, 1, 2, 2, 2, 0],
                        [1, 0, 2, 0, 2, 0],
                        [1, 0, 2, 2, 2, 0],
                        [0, 0, 3, 3, 0, 1]], dtype=torch.uint8)
    conf = torch.full((4, 6), 0.5)
    rows, sums, count, slot = region_table_reference(lab, conf, 4, 1, None, 8)
    # roots: 1 at 0; 2 at 2; 0 at 5 (the right column, 3 px); 0 at 7 (the left blob: (1,1) (2,1) (3,0) (3,1), 4 px); 0 at 9 (the hole);
    # 3 at 20; 0 at 22; 1 at 23
    assert int(count) == 8
    assert rows.tolist() == [[1, 0, 4, 0, 0, 1, 2, 0], [2, 2, 8, 2, 0, 4, 2, 0], [0, 5, 3, 5, 0, 5, 2, 0], [0, 7, 4, 0, 1, 1, 3, 0],
                             [0, 9, 1, 3, 1, 3, 1, 0], [3, 20, 2, 2, 3, 3, 3, 0], [0, 22, 1, 4, 3, 4, 3, 0], [1, 23, 1, 5, 3, 5, 3, 0]]
    assert sums[:, :2].tolist() == [[1, 3], [24, 8], [15, 3], [3, 9], [3, 1], [5, 6], [4, 3], [5, 3]]
    assert sums[:, 2].tolist() == [32768 * a for a in (4, 8, 3, 4, 1, 2, 1, 1)]
    assert slot.tolist() == [[0, 0, 1, 1, 1, 2], [0, 3, 1, 4, 1, 2], [0, 3, 1, 1, 1, 2], [3, 3, 5, 5, 6, 7]]
    # connectivity 8 joins (3, 4) to the right column through a corner; min_region 2 and ignore 2 leave 1 @ 0, 0 @ 5, 0 @ 7 and
    # 3 @ 20, of which R = 2 rows hold the first two
    rows8, sums8, count8, slot8 = region_table_reference(lab, None, 8, 2, 2, 2)
    assert int(count8) == 4 and rows8.tolist() == [[1, 0, 4, 0, 0, 1, 2, 0], [0, 5, 4, 4, 0, 5, 3, 0]]
    assert sums8.tolist() == [[1, 3, 0], [19, 6, 0]]
    assert slot8.tolist() == [[0, 0, -1, -1, -1, 1], [0, -1, -1, -1, -1, 1], [0, -1, -1, -1, -1, 1], [-1, -1, -1, -1, 1, -1]]


# ------------------------------------------------------------------------------------------------- the kernels' decomposition
@pytest.mark.parametrize("conn", T.CONNECTIVITIES)
@pytest.mark.parametrize("name", T.PATTERNS)
def test_decomposition_equals_the_reference(name, conn):
    """every map under six of the 24 settings, rotating from map to map so that every pattern meets every setting many times
    (each map's six hold both min_regions, all three max_regions, with and without ignore and conf); the full tiles and
    random5 at 48 x 200, which send runs past the table, under all 24.  (All 24 on every map is a minute of Python.)"""
    direct_at = {}
    full = (("checkerboard", 16, 64, False), ("checkerboard", 17, 65, True), ("random5", 48, 200, False))
    for i, key in enumerate(T.case_keys((name,))):
        lab = T.labels_of(key)
        root, size = C.reference(key, conn)
        chosen = T.SETTINGS if key in full else [((1, 9)[(i + j) % 2], bool((j // 2 + i // 6) % 2), (1, 7, 4096)[(j + i // 2) % 3], bool((j // 3 + i // 12) % 2))
                                                  for j in range(6)]
        for j, setting in enumerate(chosen):
            conf, K, ignore, R = T.arguments(key, setting)
            rows, sums, count, slot, direct = T.decomposition(lab, root, size, conf, K, ignore, R, seed=i * 24 + j)
            w_rows, w_sums, w_count, w_slot = T.reference(key, conn, setting)
            what = (key, conn, setting)
            k = min(int(w_count), R)
            assert count == int(w_count) and rows[:k] == w_rows[:k].tolist() and sums[:k] == w_sums[:k].tolist(), what
            assert all(r is None for r in rows[k:]) and all(s is None for s in sums[k:]), what       # never touched
            assert slot == w_slot.reshape(-1).tolist(), what
            if setting == (1, False, 4096, True):
                direct_at[key] = direct
        assert {s[0] for s in chosen} == {1, 9} and {s[2] for s in chosen} == {1, 7, 4096}
        assert {s[1] for s in chosen} == {False, True} == {s[3] for s in chosen}
    if name == "checkerboard" and conn == 4:                      # 1024 regions in a tile
        assert direct_at[("checkerboard", 16, 64, False)] > 0 and direct_at[("checkerboard", 17, 65, True)] > 0
    if name == "random5":
        assert direct_at[("random5", 48, 200, False)] > 0         # the table was filled past its probes


# ------------------------------------------------------------------------------------------------- refusals
def test_reference_refusals():
    lab = torch.zeros(3, 4, dtype=torch.uint8)
    for call, what in ((lambda: region_table_reference(lab, connectivity=6), "connectivity"),
                       (lambda: region_table_reference(lab, min_region=0), "min_region"),
                       (lambda: region_table_reference(lab, min_region=1.0), "min_region"),
                       (lambda: region_table_reference(lab, ignore=0.5), "ignore"),
                       (lambda: region_table_reference(lab, ignore=True), "ignore"),
                       (lambda: region_table_reference(lab, max_regions=0), "max_regions"),
                       (lambda: region_table_reference(lab, max_regions=2 ** 20 + 1), "max_regions"),
                       (lambda: region_table_reference(lab, max_regions=True), "max_regions"),
                       (lambda: region_table_reference(lab.float()), "labels"),
                       (lambda: region_table_reference(lab.reshape(-1)), "labels"),
                       (lambda: region_table_reference(lab, torch.zeros(3, 4, dtype=torch.float64)), "conf"),
                       (lambda: region_table_reference(lab, torch.zeros(4, 3)), "conf"),
                       (lambda: region_table_reference(lab, regions=(torch.zeros(4, 3), torch.zeros(4, 3))), "regions"),
                       (lambda: conf_q16(torch.zeros(3, dtype=torch.float64)), "conf")):
        with pytest.raises(ValueError, match=what):
            call()


def test_binding_refusals_come_before_any_launch(monkeypatch):
    """every one is a ValueError that names its argument, raised on CPU tensors: the library was not reached"""
    monkeypatch.setattr(hip, "lib", lambda: pytest.fail("the library was reached"))
    lab = torch.zeros(3, 4, dtype=torch.uint8)
    f = hip.seg_region_table
    i32, i64 = torch.int32, torch.int64
    shared = torch.zeros(64, dtype=i32)
    for call, what in ((lambda: f(lab.long()), "labels"), (lambda: f(lab.t()), "labels"), (lambda: f(lab.reshape(-1)), "labels"),
                       (lambda: f([[0]]), "labels"), (lambda: f(lab, connectivity=6), "connectivity"),
                       (lambda: f(lab, connectivity=True), "connectivity"), (lambda: f(lab, min_region=0), "min_region"),
                       (lambda: f(lab, min_region=2.0), "min_region"), (lambda: f(lab, min_region=2 ** 31), "min_region"),
                       (lambda: f(lab, ignore=0.5), "ignore"), (lambda: f(lab, ignore=False), "ignore"),
                       (lambda: f(lab, max_regions=0), "max_regions"), (lambda: f(lab, max_regions=2 ** 20 + 1), "max_regions"),
                       (lambda: f(lab, max_regions=8.0), "max_regions"), (lambda: f(lab, max_regions=True), "max_regions"),
                       (lambda: f(lab, torch.zeros(3, 4, dtype=torch.float64)), "conf"), (lambda: f(lab, torch.zeros(4, 3)), "conf"),
                       (lambda: f(lab, torch.zeros(3, 4, dtype=torch.float16)), "conf"),
                       (lambda: f(lab, max_regions=8, rows=torch.zeros(8, 7, dtype=i32)), "rows"),
                       (lambda: f(lab, max_regions=8, rows=torch.zeros(8, 8, dtype=i64)), "rows"),
                       (lambda: f(lab, max_regions=8, rows=torch.zeros(1, 8, 8, dtype=i32)), "rows"),
                       (lambda: f(lab, max_regions=8, rows=torch.zeros(8, 16, dtype=i32)[:, ::2]), "rows"),
                       (lambda: f(lab, max_regions=8, sums=torch.zeros(8, 3, dtype=i32)), "sums"),
                       (lambda: f(lab, max_regions=8, sums=torch.zeros(9, 3, dtype=i64)), "sums"),
                       (lambda: f(lab, count=torch.zeros(1, dtype=i32)), "count"),
                       (lambda: f(lab, count=torch.zeros((), dtype=i64)), "count"),
                       (lambda: f(lab[None], count=torch.zeros((), dtype=i32)), "count"),
                       (lambda: f(lab, slot=torch.zeros(4, 3, dtype=i32)), "slot"),
                       (lambda: f(lab, slot=torch.zeros(3, 4, dtype=i64)), "slot"),
                       (lambda: f(lab, slot=[0]), "slot"),
                       (lambda: f(lab, max_regions=1, rows=shared[:8].view(1, 8), slot=shared[4:16].view(3, 4)), "slot overlaps rows"),
                       (lambda: f(lab, count=shared[3].view(()), slot=shared[:12].view(3, 4)), "slot overlaps count"),
                       (lambda: f(lab, slot=shared[:12].view(3, 4), flag=shared[11:12]), "slot overlaps flag"),
                       (lambda: f(lab, torch.zeros(3, 4), slot=lab.view(torch.int8)), "slot"),
                       (lambda: f(lab, flag=torch.zeros(2, dtype=i32)), "flag")):
        with pytest.raises(ValueError, match=what):
            call()
    conf = shared[:12].view(torch.float32).view(3, 4)
    with pytest.raises(ValueError, match="slot overlaps conf"):
        f(lab, conf, slot=shared[:12].view(3, 4))


def test_segmenter_refusals_come_before_any_launch(monkeypatch):
    rec = L.Recorder(monkeypatch)                                 # hip.lib and every binding fail or record
    monkeypatch.setattr(hip, "seg_region_table", lambda *a, **k: pytest.fail("the binding was reached"))
    seg = Segmenter(L._Model(), category_token_ids=[[1]] * L.N)
    imgs, _ = L._images()
    x = torch.zeros(2, 3, 32, 48)
    for kw, what in ((dict(min_region=0), "min_region"), (dict(min_region=1.5), "min_region"), (dict(connectivity=5), "connectivity"),
                     (dict(max_regions=0), "max_regions"), (dict(max_regions=2 ** 20 + 1), "max_regions"), (dict(ignore=1.0), "ignore")):
        with pytest.raises(ValueError, match=what):
            seg.regions_raw(imgs, **kw)
        with pytest.raises(ValueError, match=what):
            seg.regions(x, **kw)
    with pytest.raises(TypeError):
        seg.regions_raw(imgs, return_probs=True)
    assert rec.log == []


# ------------------------------------------------------------------------------------------------- the header, the library
def test_header_declares_the_entry_points_and_keeps_the_abi():
    with open(os.path.join(ROOT, "include", "ifseg_hip.h")) as f:
        text = f.read()
    assert int(re.search(r"#define\s+IFSEG_ABI_VERSION\s+(\d+)", text).group(1)) == 21 == hip.ABI_VERSION
    with open(os.path.join(ROOT, "ifseg_amd", "csrc", "regiontab.hip")) as f:
        src = f.read()
    for name in ("ifseg_seg_region_table", "ifseg_seg_region_table_limit"):
        assert re.search(r"^int %s\(" % name, text, re.M), name
        assert 'extern "C" int %s(' % name in src, name
    assert hip.SEG_REGION_TABLE_MAX == 2 ** 20 == 1 << int(re.search(r"RT_MAX_REGIONS = 1 << (\d+);", src).group(1))
    assert hip.SEG_REGION_TABLE_BLOCK == 1024 == int(re.search(r"RT_BLOCK = (\d+);", src).group(1)) == T.BLOCK
    assert T.SLOTS == 1 << int(re.search(r"RT_SLOT_BITS = (\d+);", src).group(1))
    assert T.PROBES == int(re.search(r"RT_PROBES = (\d+);", src).group(1))
    assert 9 * T.SLOTS * 4 <= 65536                               # the table's LDS
    assert "ifseg_seg_regions(" in src                            # regions.hip is called through its C entry


def _library():
    if not os.path.exists(hip.LIB_PATH):
        from ifseg_amd.build import build
        build(verbose=False)
    return hip.lib()


def test_library_exports_and_limits():
    lib = _library()
    assert hasattr(lib, "ifseg_seg_region_table") and hasattr(lib, "ifseg_seg_region_table_limit")
    assert hip.seg_region_table_limits() == (16, 64, hip.SEG_REGION_TABLE_BLOCK, hip.SEG_REGION_TABLE_MAX)
    assert lib.ifseg_seg_region_table_limit(ctypes.c_int(4)) == BAD_ARG and lib.ifseg_seg_region_table_limit(ctypes.c_int(-1)) == BAD_ARG


def test_c_entry_refusals_need_no_device():
    """every refusal returns before anything is launched or dereferenced: the buffers are host memory here"""
    lib = _library()
    B, H, W, R = 2, 17, 65, 8
    npix = B * H * W
    nblk = -(-(H * W) // 1024)
    keep = []

    def buf(nbytes):
        raw = ctypes.create_string_buffer(nbytes + 64)
        keep.append(raw)
        return (ctypes.addressof(raw) + 63) & ~63                 # 64-byte aligned

    a = dict(labels=buf(2 * npix), conf=buf(4 * npix), work=buf(4 * npix), count=buf(4 * npix), root=buf(4 * npix), size=buf(4 * npix),
             blk=buf(4 * B * nblk), rows=buf(32 * B * R), sums=buf(24 * B * R), nreg=buf(4 * B), slot=buf(4 * npix), flag=buf(4))
    before = [bytes(raw) for raw in keep]
    ci, vp = ctypes.c_int, ctypes.c_void_p

    def table(lb=2, b=B, h=H, w=W, conn=4, K=1, r=R, **ptr):
        p = dict(a, **ptr)
        return lib.ifseg_seg_region_table(vp(p["labels"]), ci(lb), vp(p["conf"]), ci(b), ci(h), ci(w), ci(conn), ci(K), ci(0), ci(0),
                                          ci(r), vp(p["work"]), vp(p["count"]), vp(p["root"]), vp(p["size"]), vp(p["blk"]),
                                          vp(p["rows"]), vp(p["sums"]), vp(p["nreg"]), vp(p["slot"]), vp(p["flag"]), None)

    names = ("labels", "work", "count", "root", "size", "blk", "rows", "sums", "nreg", "slot", "flag")
    for name in names:
        assert table(**{name: None}) == BAD_ARG, name             # null (conf alone may be)
    for name in names[1:] + ("conf",):
        assert table(**{name: a[name] + 2}) == BAD_ARG, name      # misaligned
    assert table(labels=a["labels"] + 1) == BAD_ARG and table(sums=a["sums"] + 4) == BAD_ARG
    for kw in (dict(lb=0), dict(lb=3), dict(conn=0), dict(conn=6), dict(K=0), dict(K=-2), dict(r=0), dict(r=-1), dict(r=2 ** 20 + 1)):
        assert table(**kw) == BAD_ARG, kw
    order = ("labels", "conf") + names[1:]
    for i, x in enumerate(order):                                 # any two buffers sharing a byte
        for y in order[i + 1:]:
            assert table(**{y: a[x]}) == BAD_ARG, (x, y)
    assert table(slot=a["root"] + 4 * (npix - 1)) == BAD_ARG and table(rows=a["sums"] + 24 * B * R - 4) == BAD_ARG
    for kw in (dict(b=0), dict(h=0), dict(w=-1), dict(b=1 << 15, h=1 << 8, w=1 << 8)):
        assert table(**kw) == BAD_SHAPE, kw
    assert [bytes(raw) for raw in keep] == before                 # nothing was written


# ------------------------------------------------------------------------------------------------- the Segmenter's calls
REGION = dict(min_region=5, connectivity=8, max_regions=32, ignore=0)


class Recorder(SieveRecorder):
    def __init__(self, monkeypatch):
        super().__init__(monkeypatch)
        monkeypatch.setattr(hip, "seg_region_table", self.seg_region_table)

    def seg_region_table(self, labels, conf=None, connectivity=4, min_region=1, ignore=None, max_regions=1024, rows=None, sums=None,
                         count=None, slot=None, flag=None):
        assert labels.is_contiguous() and labels.dim() == 2 and rows is None and sums is None and count is None and slot is None
        assert flag is None and (conf is None or (conf.shape == labels.shape and conf.dtype == torch.float32 and conf.is_contiguous()))
        self.log.append(("seg_region_table", tuple(labels.shape), (min_region, connectivity, max_regions, ignore),
                         dict(conf=conf is not None)))
        R = max_regions
        return (torch.zeros(R, 8, dtype=torch.int32), torch.zeros(R, 3, dtype=torch.int64), torch.zeros((), dtype=torch.int32),
                torch.zeros(labels.shape, dtype=torch.int32))


def _tables(conf, shapes=(L.A, L.B)):
    return [("seg_region_table", hw, (5, 8, 32, 0), dict(conf=conf)) for hw in shapes]


def _without_conf(log):
    return [e[:3] + (dict(e[3], conf=False),) if e[0].startswith("seg_predict") else e for e in log]


@pytest.mark.parametrize("sieve", [False, True], ids=["plain", "sieve"])
@pytest.mark.parametrize("crf", [False, True], ids=["plain", "crf"])
@pytest.mark.parametrize("setting", list(L.SETTINGS))
def test_regions_raw_launch_sequence(monkeypatch, setting, crf, sieve):
    """segment_raw(return_conf=True)'s launches, a seg_sieve behind each image's where sieve= is set, then one seg_region_table
    per image"""
    rec = Recorder(monkeypatch)
    extra = dict(sieve=SIEVE_K, sieve_connectivity=SIEVE_CONN, sieve_passes=SIEVE_PASSES) if sieve else {}
    seg = Segmenter(L._Model(), category_token_ids=[[1]] * L.N, crf_iters=2 if crf else 0, **extra, **L.SETTINGS[setting][1])
    imgs, _ = L._images()
    out = seg.regions_raw(imgs, max_batch=3, **REGION, **L.SETTINGS[setting][2])
    assert len(out) == 2 and all(isinstance(t, RegionTable) for t in out)
    assert [tuple(t.labels.shape) for t in out] == [L.A, L.B] and all(t.conf is not None and t.max_regions == 32 for t in out)
    want = L._expected(setting, crf, "segment_raw")
    want = (_sieved(want, True) if sieve else want) + _tables(True)
    assert len(rec.log) == len(want), [e[0] for e in rec.log]
    for k, (got, exp) in enumerate(zip(rec.log, want)):
        assert got == exp, (k, got, exp)


@pytest.mark.parametrize("sieve", [False, True], ids=["plain", "sieve"])
def test_regions_raw_with_raw_logits_asks_for_no_conf(monkeypatch, sieve):
    """upsample="logits" outside the settings that make a probability: no conf plane is asked for, and it is no ValueError"""
    rec = Recorder(monkeypatch)
    extra = dict(sieve=SIEVE_K, sieve_connectivity=SIEVE_CONN, sieve_passes=SIEVE_PASSES) if sieve else {}
    seg = Segmenter(L._Model(), category_token_ids=[[1]] * L.N, upsample="logits", **extra)
    imgs, _ = L._images()
    out = seg.regions_raw(imgs, max_batch=3, **REGION)
    assert all(t.conf is None for t in out)
    want = _without_conf(L._expected("single", False, "segment_raw"))
    assert rec.log == (_sieved(want, False) if sieve else want) + _tables(False)
    # the CRF's marginal is a probability whatever went in
    del rec.log[:]
    out = Segmenter(L._Model(), category_token_ids=[[1]] * L.N, upsample="logits", crf_iters=2).regions_raw(imgs, max_batch=3, **REGION)
    assert all(t.conf is not None for t in out) and rec.log == L._expected("single", True, "segment_raw") + _tables(True)


def test_regions_launch_sequence(monkeypatch):
    """`regions` takes what `__call__` takes: its launches, then one seg_region_table per image of the batch"""
    rec = Recorder(monkeypatch)
    seg = Segmenter(L._Model(), category_token_ids=[[1]] * L.N)
    x = torch.stack([rec.coded(("x", b), 3, 32, 48) for b in range(2)])
    items = [("x", 0, False), ("x", 1, False)]
    out = seg.regions(x, **REGION)
    assert len(out) == 2 and all(tuple(t.labels.shape) == (32, 48) and t.conf is not None for t in out)
    assert rec.log == [("forward", items), ("seg_predict", (items, 2, 3), (2, 32, 48), dict(conf=True, probs=False))] \
        + _tables(True, [(32, 48)] * 2)
    del rec.log[:]
    sizes = [(40, 50), (7, 9)]
    out = seg.regions(x, out_hw=sizes, **REGION)
    assert [tuple(t.labels.shape) for t in out] == sizes
    want = [("forward", items)] + [("seg_predict", (items[b:b + 1], 2, 3), (1,) + s, dict(conf=True, probs=False)) for b, s in enumerate(sizes)]
    assert rec.log == want + _tables(True, sizes)


@pytest.mark.parametrize("method", ["segment_raw", "evaluate_raw", "evaluate_raw_confusion"])
@pytest.mark.parametrize("setting", list(L.SETTINGS))
def test_a_segmenter_that_asks_for_no_table_launches_what_it_did(monkeypatch, setting, method):
    rec = L.Recorder(monkeypatch)
    monkeypatch.setattr(hip, "seg_region_table", lambda *a, **k: pytest.fail("seg_region_table was reached"))
    seg = Segmenter(L._Model(), category_token_ids=[[1]] * L.N, **L.SETTINGS[setting][1])
    imgs, gts = L._images()
    if method == "segment_raw":
        seg.segment_raw(imgs, max_batch=3, return_conf=True, **L.SETTINGS[setting][2])
    else:
        seg.evaluate_raw(imgs, gts, max_batch=3, confusion=method.endswith("confusion"), **L.SETTINGS[setting][2])
    assert rec.log == L._expected(setting, False, method)


def test_task_hands_the_keywords_on(monkeypatch):
    from ifseg_amd.tasks.mm_tasks import SegmentationTask
    task = SegmentationTask(num_seg_tokens=5, patch_image_size=64, n_base_vocab=100, category_token_ids=[[5]] * 5)
    seen = []

    class Seg:
        def __getattr__(self, name):
            return lambda *a, **kw: seen.append((name, kw))

    monkeypatch.setattr(task, "build_segmenter", lambda model, **kw: seen.append(("ctor", kw)) or Seg())
    task.regions_raw(None, [], sieve=16, sieve_connectivity=8, upsample="logits", pamr_iters=2, min_region=4, connectivity=8,
                     max_regions=64, ignore=3, max_batch=2, slide=True)
    assert seen[0] == ("ctor", dict(sieve=16, sieve_connectivity=8, upsample="logits", pamr_iters=2))
    assert seen[1] == ("regions_raw", dict(min_region=4, connectivity=8, max_regions=64, ignore=3, max_batch=2, slide=True))


# ------------------------------------------------------------------------------------------------- RegionTable
def test_region_table_by_hand():
    lab = torch.tensor([[1, 1, 2, 2, 2, 0],
                        [1, 0, 2, 0, 2, 0],
                        [1, 0, 2, 2, 2, 0],
                        [0, 0, 3, 3, 0, 1]], dtype=torch.uint8)
    conf = torch.full((4, 6), 0.5)
    conf[0, 0] = 1.0                                              # q = 65535
    table = RegionTable(*region_table_reference(lab, conf, 4, 2, None, 5), lab, conf)
    assert not bool(table.truncated()) and int(table.count) == 5 and table.max_regions == 5
    got = table.to_list(names=["floor", "chair", "sofa"])
    assert got == [
        dict(value=1, name="chair", area=4, box=(0, 0, 1, 2), centroid=(0.25, 0.75), confidence=(65535 + 3 * 32768) / (65536.0 * 4)),
        dict(value=2, name="sofa", area=8, box=(2, 0, 4, 2), centroid=(3.0, 1.0), confidence=0.5),
        dict(value=0, name="floor", area=3, box=(5, 0, 5, 2), centroid=(5.0, 1.0), confidence=0.5),
        dict(value=0, name="floor", area=4, box=(0, 1, 1, 3), centroid=(0.75, 2.25), confidence=0.5),
        dict(value=3, name=None, area=2, box=(2, 3, 3, 3), centroid=(2.5, 3.0), confidence=0.5)]
    assert table.values().tolist() == [1, 2, 0, 0, 3] and table.areas().tolist() == [4, 8, 3, 4, 2]
    assert table.roots().tolist() == [0, 2, 5, 7, 20]
    assert table.boxes().tolist() == [[0, 0, 1, 2], [2, 0, 4, 2], [5, 0, 5, 2], [0, 1, 1, 3], [2, 3, 3, 3]]
    assert table.centroids().dtype == torch.float64
    assert table.centroids().tolist() == [[0.25, 0.75], [3.0, 1.0], [5.0, 1.0], [0.75, 2.25], [2.5, 3.0]]
    assert table.mean_conf().dtype == torch.float64 and table.mean_conf().tolist() == [g["confidence"] for g in got]
    # a truncated table lists its first rows; a value outside the names has none; without conf there is no confidence
    short = RegionTable(*region_table_reference(lab, None, 4, 1, None, 6), lab, None)
    assert bool(short.truncated()) and int(short.count) == 8
    got = short.to_list(names=["floor", "chair", "sofa"])
    assert len(got) == 6 and got[5] == dict(value=3, name=None, area=2, box=(2, 3, 3, 3), centroid=(2.5, 3.0), confidence=None)
    assert short.to_list()[0]["name"] is None and short.mean_conf().tolist() == [0.0] * 6
    few = RegionTable(*region_table_reference(lab, None, 4, 100, None, 6), lab, None)
    assert few.to_list() == [] and tuple(few.boxes().shape) == (0, 4) and not bool(few.truncated())
