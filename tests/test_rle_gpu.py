"""GPU: hip.seg_rle_encode / hip.seg_rle_decode (csrc/rle.hip) against their specifications (`rle_encode_reference`,
`rle_decode_reference`) on every case of tests/_rle_cases.py -- uint8 and int16, batched, max_runs 1, 7 and 16384 -- in views at
element offsets 0, 1 and 3 between canaries, with caller-given outputs between canaries, called twice into the same outputs, and
`Segmenter.export_raw` / `export` / `task.export_raw` end to end on the segofa_tiny fixture.  Everything is an integer: every
comparison is `torch.equal`."""
import pytest
import torch

import _rle_cases as T
from test_predict_views_gpu import e2e  # noqa: F401  (the segofa_tiny fixture with its three raw shapes)
from test_regions_gpu import _untouched, _view

pytestmark = pytest.mark.gpu

OFFSETS = (0, 1, 3)
I32 = torch.int32


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ifseg_amd.ops  # noqa: F401
    return torch.device("cuda:0")


def _assert_runs(got, want, R, what):
    """count in full, runs in their written part"""
    runs, count = (t.cpu() for t in got)
    w_runs, w_count = want
    assert runs.dtype == I32 and count.dtype == I32 and runs.shape == w_runs.shape and count.shape == w_count.shape, what
    assert torch.equal(count, w_count), what
    for g, w in zip(T.written(runs, count, R), T.written(w_runs, w_count, R)):
        assert torch.equal(g, w), what
    return runs, count


def _runs_view(lead, R, off, dev):
    """a run table that starts `off` RUNS (8-byte words) into a buffer of -7s -> (view [.., R, 2], buffer int32)"""
    view, buf = _view(lead + (R, 2), I32, 2 * off, -7, dev)
    assert view.data_ptr() % 8 == 0
    return view, buf


def _encode_case(hip, key, R, off, dev):
    """labels in a view at element offset `off`; caller-given outputs between canaries; a second call gives equal bits"""
    lab = T.labels_of(key)
    lead = tuple(lab.shape[:-2])
    what = (key, R, off)
    d, buf_l = _view(lab.shape, lab.dtype, off, 99, dev, lab)
    want = T.reference(key, R)
    fresh = hip.seg_rle_encode(d, R)
    runs_f, _ = _assert_runs(fresh, want, R, what)
    assert torch.equal(runs_f, want[0]), what                     # a table allocated by the binding is zero behind
    nxt = lambda k: OFFSETS[(OFFSETS.index(off) + k) % 3]
    runs, buf_r = _runs_view(lead, R, nxt(1), dev)
    count, buf_c = _view(lead, I32, nxt(2), -7, dev)
    got = hip.seg_rle_encode(d, R, runs=runs, count=count)
    assert got[0] is runs and got[1] is count, what
    _assert_runs(got, want, R, what)
    for b, k in enumerate(want[1].reshape(-1).tolist()):          # behind the written runs: the caller's bytes
        assert bool((runs.reshape(-1, R, 2)[b, min(k, R):] == -7).all()), what
    assert _untouched(buf_r, runs.storage_offset(), runs.numel(), -7) and _untouched(buf_c, count.storage_offset(), count.numel(), -7), what
    assert torch.equal(d.cpu(), lab) and _untouched(buf_l, off, lab.numel(), 99), what        # the input is only read
    first = (buf_r.clone(), buf_c.clone())
    hip.seg_rle_encode(d, R, runs=runs, count=count)
    assert torch.equal(first[0], buf_r) and torch.equal(first[1], buf_c), what               # equal bits
    return fresh, int((want[1] > R).sum())


def _decode_case(hip, key, R, off, dev, table):
    """the table of the encoder back into a map between canaries; the flag bits; equal to the input where nothing is cut"""
    from ifseg_amd.predict import rle_decode_reference
    lab = T.labels_of(key)
    H, W = lab.shape[-2:]
    lead = tuple(lab.shape[:-2])
    what = (key, R, off)
    want, w_flag = rle_decode_reference(*T.reference(key, R), H, W, lab.dtype)
    out, buf_o = _view(lab.shape, lab.dtype, off, 99, dev)
    flag = torch.zeros(1, dtype=I32, device=dev)
    got = hip.seg_rle_decode(table[0], table[1], H, W, lab.dtype, out=out, flag=flag)
    assert got[0] is out and got[1] is flag, what
    assert torch.equal(out.cpu(), want) and flag.tolist() == w_flag.tolist(), what
    assert _untouched(buf_o, off, lab.numel(), 99), what
    truncated = bool((T.reference(key, R)[1] > R).any())
    assert flag.tolist() == [1 if truncated else 0], what
    if not truncated:
        assert torch.equal(out.cpu(), lab), what                  # decode(encode(x)) == x
    fresh, fresh_flag = hip.seg_rle_decode(table[0], table[1], H, W, lab.dtype)
    assert torch.equal(fresh, out) and fresh.shape == lead + (H, W) and fresh_flag.tolist() == flag.tolist(), what


@pytest.mark.parametrize("name", T.PATTERNS)
def test_seg_rle_equals_the_specification(name):
    from ifseg_amd import hip
    dev = _dev()
    truncated = 0
    for i, key in enumerate(T.case_keys((name,))):
        for j, R in enumerate(T.MAX_RUNS):
            off = OFFSETS[(i + j) % 3]
            table, cut = _encode_case(hip, key, R, off, dev)
            truncated += cut
            _decode_case(hip, key, R, OFFSETS[(i + j + 1) % 3], dev, table)
    assert truncated > 0 or name == "constant"                    # max_runs 1 and 7 cut the tables short


def test_seg_rle_batched():
    """B = 3 where an image ends with the value the next one begins with: a run breaks there, and no rank crosses over"""
    from ifseg_amd import hip
    dev = _dev()
    for i, key in enumerate(T.BATCHES):
        for j, R in enumerate(T.MAX_RUNS):
            table, _ = _encode_case(hip, key, R, OFFSETS[(i + j) % 3], dev)
            _decode_case(hip, key, R, OFFSETS[(i + j + 2) % 3], dev, table)
    runs, count = hip.seg_rle_encode(T.labels_of("batch_constant").to(dev), 4)
    assert count.tolist() == [1, 1, 1] and runs[:, 0, 0].tolist() == [0, 0, 0]


def test_seg_rle_decode_flags_empty_and_malformed_tables():
    """count <= 0: the image is fill and bit 1 is set; start[0] != 0: bit 1; count > R: bit 0; a given flag is never cleared; a
    table whose starts do not ascend is read inside [0, m) only (the canaries and the device stay whole)"""
    from ifseg_amd import hip
    from ifseg_amd.predict import rle_decode_reference
    dev = _dev()
    key = ("random5", 33, 129, False)
    lab = T.labels_of(key)
    H, W = lab.shape
    runs, count = T.reference(key, 16384)
    k = int(count)
    d_runs = runs.to(dev)
    for c in (0, -3):
        out, buf = _view((H, W), torch.uint8, 1, 99, dev)
        _, flag = hip.seg_rle_decode(d_runs, torch.tensor(c, dtype=I32, device=dev), H, W, fill=9, out=out)
        assert bool((out == 9).all()) and flag.tolist() == [2] and _untouched(buf, 1, H * W, 99)
    shifted = runs.clone()
    shifted[0, 0] = 5
    want, w_flag = rle_decode_reference(shifted, count, H, W)
    out, flag = hip.seg_rle_decode(shifted.to(dev), count.to(dev), H, W)
    assert torch.equal(out.cpu(), want) and flag.tolist() == w_flag.tolist() == [2]
    # one flag word watches many calls; in a batch each image adds its bits
    tab = torch.stack([runs[:64], shifted[:64], runs[:64]]).to(dev)
    cnt = torch.tensor([k, 64, 0], dtype=I32, device=dev)
    want, w_flag = rle_decode_reference(tab.cpu(), cnt.cpu(), H, W)
    out, flag = hip.seg_rle_decode(tab, cnt, H, W)
    assert torch.equal(out.cpu(), want) and flag.tolist() == w_flag.tolist() == [3]
    hip.seg_rle_decode(d_runs, count.to(dev), H, W, flag=flag)
    assert flag.tolist() == [3]
    g = torch.Generator().manual_seed(2)
    for trial, bad in enumerate((runs[:k][torch.randperm(k, generator=g)], torch.zeros(k, 2, dtype=I32),
                                 torch.randint(-2 ** 31, 2 ** 31, (k, 2), generator=g, dtype=torch.int64).to(I32))):
        view, buf_r = _runs_view((), k, 1, dev)
        view.copy_(bad)
        out, buf = _view((H, W), torch.uint8, 3, 99, dev)
        _, flag = hip.seg_rle_decode(view, torch.tensor(k + trial, dtype=I32, device=dev), H, W, out=out)
        assert flag.tolist() == [(1 if trial else 0) | (2 if int(bad[0, 0]) != 0 else 0)], trial
        assert _untouched(buf, 3, H * W, 99) and _untouched(buf_r, 2, 2 * k, -7), trial
        values = set(bad[:, 1].tolist())
        assert set(out.cpu().reshape(-1).tolist()) <= {v & 255 for v in values}, trial       # every pixel is a value of the table


def test_limits_match_the_constants():
    from ifseg_amd import hip
    _dev()
    assert hip.seg_rle_limits() == (hip.SEG_RLE_CHUNK, hip.SEG_RLE_COLS, hip.SEG_RLE_MAX_RUNS) == (T.CHUNK, T.COLS, 2 ** 24)


# ------------------------------------------------------------------------------------------------- end to end
def _assert_maps(maps, results, R, n):
    from ifseg_amd.predict import RunLengthMap, coco_mask_reference, coco_rle_string, rle_encode_reference
    assert len(maps) == len(results)
    for i, (m, r) in enumerate(zip(maps, results)):
        assert isinstance(m, RunLengthMap) and m.shape == tuple(r.labels.shape) and m.dtype == r.labels.dtype and m.n == n
        lab = r.labels.cpu()
        want = rle_encode_reference(lab, R)
        _assert_runs((m.runs, m.count), want, R, i)
        assert not bool(m.truncated()) and torch.equal(m.decode(), r.labels)
        assert torch.equal(m.areas(n).cpu(), torch.bincount(lab.reshape(-1).long(), minlength=n)[:n])
        entries = m.to_coco(i)
        present = sorted(set(v for v in lab.reshape(-1).tolist() if 0 <= v < n))
        assert [e["category_id"] for e in entries] == present and len(present) > 0
        for e, c in zip(entries, present):
            assert e["image_id"] == i and e["segmentation"]["size"] == list(lab.shape)
            assert e["segmentation"]["counts"] == coco_rle_string(coco_mask_reference(lab, c))
        back = RunLengthMap.from_coco(entries, m.shape, dtype=m.dtype, device=m.runs.device)
        assert torch.equal(back.decode(), r.labels)


def test_segmenter_export_end_to_end(e2e):  # noqa: F811
    m, raw, ocfg, mk = e2e
    n = ocfg.num_seg_tokens
    seg = mk()
    base = seg.segment_raw(raw)
    _assert_maps(seg.export_raw(raw), base, 65536, n)
    _assert_maps(seg.export_raw(raw, max_runs=8192), base, 8192, n)
    short = seg.export_raw(raw, max_runs=1)
    assert all(int(t.count) == int(f.count) for t, f in zip(short, seg.export_raw(raw)))
    assert any(bool(t.truncated()) for t in short)
    # behind the sieve: the runs of the sieved map
    sieved = mk(sieve=8)
    _assert_maps(sieved.export_raw(raw), sieved.segment_raw(raw), 65536, n)
    # what __call__ takes
    from ifseg_amd import hip
    from ifseg_amd.predict import SegmentationResult
    P = ocfg.patch_image_size
    x = hip.image_load(torch.stack([raw[2], raw[2].flip(0)]).to(next(m.parameters()).device), P, P)
    res = seg(x)
    _assert_maps(seg.export(x), [SegmentationResult(res.labels[b], None, None) for b in range(2)], 65536, n)
    res = sieved(x)
    _assert_maps(sieved.export(x, max_runs=8192), [SegmentationResult(res.labels[b], None, None) for b in range(2)], 8192, n)
    # the task forwards its keywords: the constructor's to the Segmenter, the others to export_raw
    from ifseg_amd.tasks.mm_tasks import SegmentationTask
    from test_predict_views_gpu import PC
    task = SegmentationTask(num_seg_tokens=n, patch_image_size=P, category_token_ids=PC.E2E_NAMES)
    got = task.export_raw(m, raw, prompt_ids=PC.E2E_PROMPT, sieve=8, max_runs=8192)
    mine = sieved.export_raw(raw, max_runs=8192)
    assert all(torch.equal(a.runs, b.runs) and torch.equal(a.count, b.count) for a, b in zip(got, mine))
    _assert_maps(got, sieved.segment_raw(raw), 8192, n)
