"""GPU: hip.seg_region_table (csrc/regiontab.hip) against its specification (`region_table_reference`) on every case and setting
of tests/_region_table_cases.py -- both connectivities, min_region 1 and 9, with and without an ignored value, max_regions 1, 7
and 4096, with and without conf, uint8 and int16, batched -- in views at element offsets 0, 1 and 3 between canaries, with
caller-given outputs between canaries, called twice into the same outputs, and `Segmenter.regions_raw` end to end on the
segofa_tiny fixture.  Everything is an integer: every comparison is `torch.equal`."""
import pytest
import torch

import _region_table_cases as T
from test_predict_views_gpu import e2e  # noqa: F401  (the segofa_tiny fixture with its three raw shapes)
from test_regions_gpu import _untouched, _view

pytestmark = pytest.mark.gpu

OFFSETS = (0, 1, 3)
I32, I64 = torch.int32, torch.int64


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ifseg_amd.ops  # noqa: F401
    return torch.device("cuda:0")


def _assert_table(got, want, R, what):
    """rows and sums in their written part, count and slot in full"""
    rows, sums, count, slot = (t.cpu() for t in got)
    w_rows, w_sums, w_count, w_slot = want
    assert rows.dtype == I32 and sums.dtype == I64 and count.dtype == I32 and slot.dtype == I32, what
    assert rows.shape == w_rows.shape and sums.shape == w_sums.shape and count.shape == w_count.shape, what
    assert torch.equal(count, w_count) and torch.equal(slot, w_slot), what
    for (g_r, g_s), (w_r, w_s) in zip(T.written(rows, sums, count, R), T.written(w_rows, w_sums, w_count, R)):
        assert torch.equal(g_r, w_r) and torch.equal(g_s, w_s), what
    return rows, sums, count


def _run_case(hip, key, conn, setting, dev, flag):
    conf, K, ignore, R = T.arguments(key, setting)
    got = hip.seg_region_table(T.labels_of(key).to(dev), None if conf is None else conf.to(dev), conn, K, ignore, R, flag=flag)
    want = T.reference(key, conn, setting)
    rows, sums, count = _assert_table(got, want, R, (key, conn, setting))
    assert torch.equal(rows, want[0]) and torch.equal(sums, want[1])       # a table allocated by the binding is zero behind
    return int((count > R).sum())


@pytest.mark.parametrize("conn", T.CONNECTIVITIES)
@pytest.mark.parametrize("name", T.PATTERNS)
def test_seg_region_table_equals_the_specification(name, conn):
    from ifseg_amd import hip
    dev = _dev()
    flag = torch.zeros(1, dtype=I32, device=dev)
    truncated = 0
    for key in T.case_keys((name,)):
        for setting in T.SETTINGS:
            truncated += _run_case(hip, key, conn, setting, dev, flag)
    assert truncated > 0 or name == "constant"                    # max_regions 1 and 7 cut the tables short
    assert int(flag) == 0                                         # no loop of the region kernels ran out of its budget


@pytest.mark.parametrize("conn", T.CONNECTIVITIES)
def test_seg_region_table_batched(conn):
    """B = 3 where the last row of one image equals the first row of the next: no region, rank or row crosses into the next"""
    from ifseg_amd import hip
    dev = _dev()
    flag = torch.zeros(1, dtype=I32, device=dev)
    for key in T.BATCHES:
        for setting in T.SETTINGS:
            _run_case(hip, key, conn, setting, dev, flag)
    assert int(flag) == 0


@pytest.mark.parametrize("conn", T.CONNECTIVITIES)
def test_seg_region_table_layouts_and_repeats(conn):
    """every tensor a view at an element offset between canaries; the caller's outputs keep their canaries behind the written
    rows; a second call into the same outputs gives the same bits"""
    from ifseg_amd import hip
    dev = _dev()
    flag = torch.zeros(1, dtype=I32, device=dev)
    keys = [("random5", 48, 200, False), ("checkerboard", 17, 65, True), ("checkerboard", 16, 64, False), ("blocks", 33, 129, False),
            ("rings", 33, 129, True), ("constant", 1, 1, False), ("serpentine", 48, 200, False), ("random2", 3, 2, False), "batch",
            "batch_short"]
    for i, key in enumerate(keys):
        lab = T.labels_of(key)
        lead = tuple(lab.shape[:-2])
        for n, setting in enumerate(((1, False, 4096, True), (9, True, 7, True), (1, True, 1, False), (9, False, 4096, False))):
            conf, K, ignore, R = T.arguments(key, setting)
            off = OFFSETS[(i + n) % 3]
            nxt = lambda k: OFFSETS[(OFFSETS.index(off) + k) % 3]
            what = (key, conn, setting, off)
            d, buf_l = _view(lab.shape, lab.dtype, off, 99, dev, lab)
            cf, buf_c = (None, None) if conf is None else _view(lab.shape, torch.float32, nxt(1), -5.0, dev, conf)
            rows, buf_r = _view(lead + (R, 8), I32, nxt(2), -7, dev)
            sums, buf_s = _view(lead + (R, 3), I64, off, -7, dev)
            count, buf_n = _view(lead, I32, nxt(1), -7, dev)
            slot, buf_p = _view(lab.shape, I32, nxt(2), -7, dev)
            got = hip.seg_region_table(d, cf, conn, K, ignore, R, rows=rows, sums=sums, count=count, slot=slot, flag=flag)
            assert got[0] is rows and got[1] is sums and got[2] is count and got[3] is slot, what
            want = T.reference(key, conn, setting)
            _assert_table(got, want, R, what)
            for b, k in enumerate(want[2].reshape(-1).tolist()):  # behind the written rows: the caller's bytes
                assert bool((rows.reshape(-1, R, 8)[b, min(k, R):] == -7).all()), what
                assert bool((sums.reshape(-1, R, 3)[b, min(k, R):] == -7).all()), what
            assert _untouched(buf_r, rows.storage_offset(), rows.numel(), -7) and _untouched(buf_s, off, sums.numel(), -7), what
            assert _untouched(buf_n, count.storage_offset(), count.numel(), -7), what
            assert _untouched(buf_p, slot.storage_offset(), slot.numel(), -7), what
            assert torch.equal(d.cpu(), lab) and _untouched(buf_l, off, lab.numel(), 99), what       # the inputs are only read
            if cf is not None:
                assert torch.equal(cf.cpu().view(I32), conf.view(I32)) and _untouched(buf_c, cf.storage_offset(), lab.numel(), -5.0)
            first = [buf.clone() for buf in (buf_r, buf_s, buf_n, buf_p)]
            hip.seg_region_table(d, cf, conn, K, ignore, R, rows=rows, sums=sums, count=count, slot=slot, flag=flag)
            assert all(torch.equal(a, b) for a, b in zip(first, (buf_r, buf_s, buf_n, buf_p))), what   # equal bits
    assert int(flag) == 0
    # an ignored value the map's dtype cannot hold ignores nothing
    key, setting = ("blocks", 33, 129, False), (9, False, 4096, True)
    got = hip.seg_region_table(T.labels_of(key).to(dev), T.conf_of(key).to(dev), conn, 9, ignore=-1, max_regions=4096)
    _assert_table(got, T.reference(key, conn, setting), 4096, key)


def test_limits_match_the_constants():
    from ifseg_amd import hip
    _dev()
    assert hip.seg_region_table_limits() == (16, 64, hip.SEG_REGION_TABLE_BLOCK, hip.SEG_REGION_TABLE_MAX) == (16, 64, 1024, 2 ** 20)
    assert hip.seg_regions_limits()[:2] == hip.seg_region_table_limits()[:2]


# ------------------------------------------------------------------------------------------------- end to end
def _assert_tables(tables, results, kw, with_conf=True):
    from ifseg_amd.predict import RegionTable, region_table_reference
    assert len(tables) == len(results)
    some = 0
    for t, r in zip(tables, results):
        assert isinstance(t, RegionTable)
        conf = r.conf.cpu() if with_conf else None
        R = kw.get("max_regions", 1024)
        want = region_table_reference(r.labels.cpu(), conf, kw.get("connectivity", 4), kw.get("min_region", 1), kw.get("ignore"), R)
        _assert_table((t.rows, t.sums, t.count, t.slot), want, R, kw)
        assert torch.equal(t.labels, r.labels) and (t.conf is None if not with_conf else torch.equal(t.conf.view(I32), r.conf.view(I32)))
        some += int(t.count)
        listed = t.to_list()
        assert len(listed) == min(int(t.count), R) == len(t.areas()) and [d["area"] for d in listed] == t.areas().tolist()
    assert some > 0


def test_segmenter_regions_end_to_end(e2e):  # noqa: F811
    m, raw, ocfg, mk = e2e
    n = ocfg.num_seg_tokens
    seg = mk()
    base = seg.segment_raw(raw, return_conf=True)
    _assert_tables(seg.regions_raw(raw), base, {})
    kw = dict(min_region=6, connectivity=8, max_regions=5, ignore=int(base[0].labels[0, 0]))
    tables = seg.regions_raw(raw, **kw)
    _assert_tables(tables, base, kw)
    assert any(bool(t.truncated()) for t in tables)
    # behind the sieve: the table of the sieved map and its conf
    sieved = mk(sieve=8)
    _assert_tables(sieved.regions_raw(raw, min_region=2), sieved.segment_raw(raw, return_conf=True), dict(min_region=2))
    # raw logits: no conf, the third sum 0
    logits = mk(upsample="logits")
    tables = logits.regions_raw(raw, max_regions=64)
    _assert_tables(tables, logits.segment_raw(raw), dict(max_regions=64), with_conf=False)
    assert all(not t.sums[:, 2].any() for t in tables)
    # what __call__ takes
    from ifseg_amd import hip
    P = ocfg.patch_image_size
    x = hip.image_load(torch.stack([raw[2], raw[2].flip(0)]).to(next(m.parameters()).device), P, P)
    res = seg(x, return_conf=True)
    from ifseg_amd.predict import SegmentationResult
    per_image = [SegmentationResult(res.labels[b], res.conf[b], None) for b in range(2)]
    _assert_tables(seg.regions(x, min_region=3), per_image, dict(min_region=3))
    # the task forwards its keywords: the constructor's to the Segmenter, the others to regions_raw
    from ifseg_amd.tasks.mm_tasks import SegmentationTask
    from test_predict_views_gpu import PC
    task = SegmentationTask(num_seg_tokens=n, patch_image_size=P, category_token_ids=PC.E2E_NAMES)
    got = task.regions_raw(m, raw, prompt_ids=PC.E2E_PROMPT, sieve=8, min_region=2)
    mine = sieved.regions_raw(raw, min_region=2)
    assert all(torch.equal(a.rows, b.rows) and torch.equal(a.sums, b.sums) and torch.equal(a.count, b.count)
               and torch.equal(a.slot, b.slot) for a, b in zip(got, mine))
