"""CPU: run-length label maps (ifseg_amd/predict.py: rle_encode_reference, rle_decode_reference, the COCO codec, RunLengthMap,
Segmenter.export_raw / export; hip.seg_rle_encode / seg_rle_decode; csrc/rle.hip) without a device.  The specification against
a literal loop over f on every case of tests/_rle_cases.py; the COCO counts against the dense mask; cocoapi's string both ways;
Python transcriptions of the three encode launches and of the decoder's search-and-walk against the specifications; every
refusal, of the specification, the binding, the Segmenter and the C entries; the header; the launches a Segmenter makes,
recorded by fakes."""
import ctypes
import os
import random
import re

import pytest
import torch

import _rle_cases as T
import test_pamr_cpu as PM
import test_segmenter_launches_cpu as L
from test_sieve_cpu import Recorder as SieveRecorder, _sieved, K as SIEVE_K, CONN as SIEVE_CONN, PASSES as SIEVE_PASSES
from ifseg_amd import hip
from ifseg_amd.predict import (RunLengthMap, Segmenter, coco_counts, coco_mask_reference, coco_rle_counts, coco_rle_string,
                               rle_decode_reference, rle_encode_reference)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_SHAPE, BAD_ARG = -2, -3
I32 = torch.int32


# ------------------------------------------------------------------------------------------------- the specification
def _assert_equals_literal(key, R):
    lab = T.labels_of(key)
    H, W = lab.shape[-2:]
    runs, count = T.reference(key, R)
    assert runs.dtype == I32 and count.dtype == I32
    assert tuple(runs.shape) == tuple(lab.shape[:-2]) + (R, 2) and tuple(count.shape) == tuple(lab.shape[:-2])
    for b, (got, img) in enumerate(zip(T.written(runs, count, R), lab.reshape(-1, H, W))):
        want = T.literal(img)
        assert int(count.reshape(-1)[b]) == len(want), (key, R, b)
        assert got.tolist() == want[:R], (key, R, b)
        assert not runs.reshape(-1, R, 2)[b, min(len(want), R):].any(), (key, R, b)      # zero behind
    return count


@pytest.mark.parametrize("name", T.PATTERNS + ("batches",))
def test_reference_equals_the_literal_loop(name):
    keys = T.BATCHES if name == "batches" else T.case_keys((name,))
    truncated = 0
    for key in keys:
        for R in T.MAX_RUNS:
            count = _assert_equals_literal(key, R)
            truncated += int((count > R).sum())
            assert R < 16384 or not bool((count > R).any())           # the largest table holds every map
    assert truncated > 0 or name == "constant"


def test_reference_known_counts():
    n = lambda key: int(T.reference(key, 16384)[1])
    assert n(("checkerboard", 16, 64, False)) == 961                  # H even: the run goes on across each of the 63 seams
    assert n(("checkerboard", 17, 65, False)) == 1105 == 17 * 65      # H odd: one per pixel
    assert n(("checkerboard", 1, 65, True)) == 65 and n(("checkerboard", 65, 1, False)) == 65
    assert all(n(("constant", H, W, False)) == 1 for H, W in T.SHAPES)
    assert n(("vstripes", 48, 200, False)) == 200 and n(("hstripes", 48, 200, False)) == 48 * 200
    assert n(("hstripes", 33, 129, False)) == 33 * 129 - 128          # H odd: the stripe goes on across each of the 128 seams
    # a run breaks between the images of a batch although the values are equal there
    lab = T.labels_of("batch_constant")
    assert bool((lab == lab[0, 0, 0]).all()) and T.reference("batch_constant", 7)[1].tolist() == [1, 1, 1]
    for key in T.BATCHES:
        lab = T.labels_of(key)
        assert all(int(lab[b, 0, 0]) == int(lab[b - 1, -1, -1]) for b in (1, 2))
        runs, count = T.reference(key, 16384)
        for b in range(3):
            one = rle_encode_reference(lab[b], 16384)
            assert int(one[1]) == int(count[b]) and torch.equal(one[0], runs[b])
            assert runs[b, 0].tolist() == [0, int(lab[b, 0, 0])]


def test_reference_by_hand():
    lab = torch.tensor([[1, 1, 2],
                        [1, 0, 2],
                        [0, 0, 255]], dtype=torch.uint8)
    # f = 1 1 0 | 1 0 0 | 2 2 255
    runs, count = rle_encode_reference(lab, 8)
    assert int(count) == 6 and runs.tolist() == [[0, 1], [2, 0], [3, 1], [4, 0], [6, 2], [8, 255], [0, 0], [0, 0]]
    runs, count = rle_encode_reference(lab, 2)
    assert int(count) == 6 and runs.tolist() == [[0, 1], [2, 0]]
    out, flag = rle_decode_reference(runs, count, 3, 3)
    assert out.tolist() == [[1, 0, 0], [1, 0, 0], [0, 0, 0]] and flag.tolist() == [1]   # the tail carries the last written value
    short = torch.tensor([[-3, -3], [7, -3]], dtype=torch.int16)
    runs, count = rle_encode_reference(short, 4)
    assert int(count) == 3 and runs[:3].tolist() == [[0, -3], [1, 7], [2, -3]]
    out, flag = rle_decode_reference(runs, count, 2, 2, torch.int16)
    assert torch.equal(out, short) and flag.tolist() == [0]


def test_reference_refusals():
    lab = torch.zeros(3, 4, dtype=torch.uint8)
    runs, count = rle_encode_reference(lab, 4)
    for call, what in ((lambda: rle_encode_reference(lab, 0), "max_runs"), (lambda: rle_encode_reference(lab, 2 ** 24 + 1), "max_runs"),
                       (lambda: rle_encode_reference(lab, True), "max_runs"), (lambda: rle_encode_reference(lab, 4.0), "max_runs"),
                       (lambda: rle_encode_reference(lab.long()), "labels"), (lambda: rle_encode_reference(lab.float()), "labels"),
                       (lambda: rle_encode_reference(lab.reshape(-1)), "labels"),
                       (lambda: rle_decode_reference(runs.long(), count, 3, 4), "runs"),
                       (lambda: rle_decode_reference(runs[:, :1], count, 3, 4), "runs"),
                       (lambda: rle_decode_reference(runs, count.long(), 3, 4), "count"),
                       (lambda: rle_decode_reference(runs, count[None], 3, 4), "count"),
                       (lambda: rle_decode_reference(runs, count, 3, 4, torch.int32), "dtype"),
                       (lambda: coco_counts([1, 2], [0, 0], 0, 4), "starts"), (lambda: coco_counts([0, 2], [0], 0, 4), "starts"),
                       (lambda: coco_counts([0, 4], [0, 1], 0, 4), "starts"), (lambda: coco_rle_counts("0~"), "RLE character"),
                       (lambda: coco_rle_counts("P"), "ends inside")):
        with pytest.raises(ValueError, match=what):
            call()


# ------------------------------------------------------------------------------------------------- COCO's counts and string
HAND = (([0, 4], "04"), ([2, 3, 1, 1], "231N"), ([100000, 5, 3, 70000], "PeQ353[[T2"))


def test_hand_strings():
    for counts, string in HAND:
        assert coco_rle_string(counts) == string and coco_rle_counts(string) == counts


def test_string_round_trip_on_large_and_small_counts():
    rng = random.Random(3)
    top = 2 ** 31 - 1
    lists = [[top], [0, top], [top, 0, top, 0, top], [1, top, 1, top, 1], [0, 1, top, 1, 0, top], [top, 1, 1, top], [15, 16, 31, 32, 1023, 1024]]
    for _ in range(300):
        k = rng.randrange(1, 12)
        lists.append([rng.choice((0, 1, 15, 16, 31, 32, 1023, 1024, 32767, 32768, rng.randrange(top), top)) for _ in range(k)])
    for counts in lists:
        s = coco_rle_string(counts)
        assert all(48 <= ord(ch) < 112 for ch in s) and coco_rle_counts(s) == counts, counts


@pytest.mark.parametrize("name", T.PATTERNS)
def test_coco_counts_equal_the_dense_mask_and_round_trip(name):
    for key in T.case_keys((name,)):
        lab = T.labels_of(key)
        H, W = lab.shape
        runs, count = T.reference(key, 16384)
        tab = runs[:int(count)]
        starts, values = tab[:, 0].numpy(), tab[:, 1].numpy()
        classes = sorted(set(lab.reshape(-1).tolist())) + [77]        # 77: absent everywhere
        for c in classes:
            got = coco_counts(starts, values, c, H * W)
            assert got == coco_mask_reference(lab, c), (key, c)
            assert sum(got) == H * W and all(v > 0 for v in got[1:]) and got[0] >= 0, (key, c)
            assert sum(got[1::2]) == int((lab == c).sum()), (key, c)
            assert coco_rle_counts(coco_rle_string(got)) == got, (key, c)
        assert coco_counts(starts, values, 77, H * W) == [H * W]


# ------------------------------------------------------------------------------------------------- the kernels' decomposition
@pytest.mark.parametrize("name", T.PATTERNS + ("batches",))
def test_encode_decomposition_equals_the_reference(name):
    keys = T.BATCHES if name == "batches" else T.case_keys((name,))
    for key in keys:
        lab = T.labels_of(key)
        H, W = lab.shape[-2:]
        for R in T.MAX_RUNS:
            w_runs, w_count = T.reference(key, R)
            for b, img in enumerate(lab.reshape(-1, H, W)):
                runs, count = T.encode_decomposition(img, R)
                k = min(count, R)
                assert count == int(w_count.reshape(-1)[b]), (key, R, b)
                assert runs[:k] == w_runs.reshape(-1, R, 2)[b, :k].tolist(), (key, R, b)
                assert all(r is None for r in runs[k:]), (key, R, b)                  # never touched


@pytest.mark.parametrize("name", T.PATTERNS)
def test_decode_decomposition_equals_the_reference(name):
    for key in T.case_keys((name,)):
        lab = T.labels_of(key)
        H, W = lab.shape
        for R in T.MAX_RUNS:
            runs, count = T.reference(key, R)
            want, w_flag = rle_decode_reference(runs, count, H, W, lab.dtype)
            got, flag, reads = T.decode_decomposition(runs.tolist(), int(count), H, W)
            m = min(int(count), R)
            assert got == want.tolist() and [flag] == w_flag.tolist() and reads <= set(range(m)), (key, R)
            assert flag == (1 if int(count) > R else 0)
            if int(count) <= R:
                assert torch.equal(want, lab), (key, R)                               # decode(encode(x)) == x


def test_decode_of_empty_shifted_and_scrambled_tables():
    """a malformed table gives wrong pixels, the specified flag bits, and no read outside [0, m)"""
    key = ("random5", 17, 65, False)
    H, W = 17, 65
    runs, count = T.reference(key, 16384)
    k = int(count)
    tab = runs[:k].clone()
    rng = random.Random(5)
    for c in (0, -4):                                                                 # empty: the image is fill
        want, w_flag = rle_decode_reference(tab, torch.tensor(c, dtype=I32), H, W, fill=9)
        got, flag, reads = T.decode_decomposition(tab.tolist(), c, H, W, fill=9)
        assert got == want.tolist() == [[9] * W] * H and flag == 2 and w_flag.tolist() == [2] and reads == set()
    shifted = tab.clone()
    shifted[0, 0] = 5                                                                 # start[0] != 0: bit 1; s = 0 below it
    want, w_flag = rle_decode_reference(shifted, count, H, W)
    got, flag, reads = T.decode_decomposition(shifted.tolist(), k, H, W)
    assert got == want.tolist() and flag == 2 and w_flag.tolist() == [2] and reads <= set(range(k))
    for trial in range(6):
        bad = tab.clone()
        if trial % 3 == 0:
            bad = bad[torch.randperm(k, generator=torch.Generator().manual_seed(trial))]
        elif trial % 3 == 1:
            bad[:, 0] = torch.tensor([rng.choice((-2 ** 31, -1, 0, 7, H * W, 2 ** 31 - 1)) for _ in range(k)], dtype=I32)
        else:
            bad[:, 0] = 0
        c = (k, k + 3, 40)[trial % 3]
        table = bad[:min(c, k)] if trial % 2 else bad
        R = table.shape[0]
        got, flag, reads = T.decode_decomposition(table.tolist(), c, H, W)
        _, w_flag = rle_decode_reference(table, torch.tensor(c, dtype=I32), H, W)
        m = min(c, R)
        assert [flag] == w_flag.tolist() == [(1 if c > R else 0) | (2 if int(table[0, 0]) != 0 else 0)], trial
        assert reads <= set(range(m)) and all(v is not None for row in got for v in row), trial


# ------------------------------------------------------------------------------------------------- RunLengthMap
def test_run_length_map_by_hand():
    lab = torch.tensor([[1, 1, 2],
                        [1, 0, 2],
                        [0, 0, 255]], dtype=torch.uint8)
    m = RunLengthMap(*rle_encode_reference(lab, 8), lab.shape, lab.dtype)
    assert m.max_runs == 8 and not bool(m.truncated()) and m.nbytes == 8 * 8 + 4 and m.shape == (3, 3)
    assert m.starts().tolist() == [0, 2, 3, 4, 6, 8] and m.values().tolist() == [1, 0, 1, 0, 2, 255]
    assert m.lengths().tolist() == [2, 1, 1, 2, 2, 1]
    assert m.areas(3).dtype == torch.int64 and m.areas(3).tolist() == [3, 3, 2] and m.areas(2).tolist() == [3, 3]
    got = m.to_coco(17, category_ids=[92, 93, 94])
    assert [e["category_id"] for e in got] == [92, 93, 94] and all(e["image_id"] == 17 for e in got)
    assert all(e["segmentation"]["size"] == [3, 3] and isinstance(e["segmentation"]["counts"], str) for e in got)
    assert [coco_rle_counts(e["segmentation"]["counts"]) for e in got] == [[2, 1, 1, 2, 3], [0, 2, 1, 1, 5], [6, 2, 1]]
    assert [e["category_id"] for e in m.to_coco(0)] == [0, 1, 2]                      # 255 is no class without a count either
    assert [e["category_id"] for e in RunLengthMap(m.runs, m.count, m.shape, m.dtype, n=2).to_coco(0)] == [0, 1]
    short = RunLengthMap(*rle_encode_reference(lab, 4), lab.shape, lab.dtype)
    assert bool(short.truncated()) and short.lengths().tolist() == [2, 1, 1, 5]
    with pytest.raises(ValueError, match="truncated"):
        short.to_coco(0)


@pytest.mark.parametrize("short", [False, True])
def test_from_coco_of_to_coco_decodes_to_the_map(short):
    for H, W in T.SHAPES:
        lab = T.labels_of(("random5", H, W, short))
        lab = (lab + 2 if short else lab).contiguous()                # values 0 .. 4: all of them classes
        m = RunLengthMap(*rle_encode_reference(lab, 16384), lab.shape, lab.dtype, n=5)
        ids = [11, 12, 13, 14, 15]
        entries = m.to_coco(3, ids)
        assert [e["category_id"] for e in entries] == [ids[c] for c in sorted(set(lab.reshape(-1).tolist()))]
        back = RunLengthMap.from_coco(entries, (H, W), class_of={v: c for c, v in enumerate(ids)}, dtype=lab.dtype)
        assert back.shape == (H, W) and torch.equal(back.runs, m.runs[:int(m.count)]) and int(back.count) == int(m.count)
        out, flag = rle_decode_reference(back.runs, back.count, H, W, lab.dtype)
        assert torch.equal(out, lab) and flag.tolist() == [0]
    # uncovered pixels are fill and join into one run; masks that share a pixel are refused
    lab = torch.tensor([[0, 1], [1, 1]], dtype=torch.uint8)
    entries = RunLengthMap(*rle_encode_reference(lab, 8), (2, 2), torch.uint8, n=2).to_coco(0)
    only = RunLengthMap.from_coco(entries[1:], (2, 2), fill=200)
    assert only.runs.tolist() == [[0, 200], [1, 1]] and int(only.count) == 2
    with pytest.raises(ValueError, match="overlaps"):
        RunLengthMap.from_coco(entries + entries[:1], (2, 2))
    with pytest.raises(ValueError, match="size"):
        RunLengthMap.from_coco(entries, (2, 3))
    with pytest.raises(ValueError, match="add up"):
        RunLengthMap.from_coco([dict(category_id=1, segmentation=dict(size=[2, 2], counts=[1, 2]))], (2, 2))
    plain = RunLengthMap.from_coco([dict(category_id=1, segmentation=dict(size=[2, 2], counts=[1, 3]))], (2, 2), fill=0)
    assert plain.runs.tolist() == [[0, 0], [1, 1]]


# ------------------------------------------------------------------------------------------------- refusals
def test_binding_refusals_come_before_any_launch(monkeypatch):
    """every one is a ValueError that names its argument, raised on CPU tensors: the library was not reached"""
    monkeypatch.setattr(hip, "lib", lambda: pytest.fail("the library was reached"))
    lab = torch.zeros(3, 4, dtype=torch.uint8)
    enc, dec = hip.seg_rle_encode, hip.seg_rle_decode
    shared = torch.zeros(64, dtype=I32)
    assert shared.data_ptr() % 8 == 0
    runs, count = torch.zeros(8, 2, dtype=I32), torch.zeros((), dtype=I32)
    for call, what in ((lambda: enc(lab.long()), "labels"), (lambda: enc(lab.t()), "labels"), (lambda: enc(lab.reshape(-1)), "labels"),
                       (lambda: enc([[0]]), "labels"), (lambda: enc(lab.to(torch.int8)), "labels"),
                       (lambda: enc(lab, 0), "max_runs"), (lambda: enc(lab, 2 ** 24 + 1), "max_runs"), (lambda: enc(lab, 8.0), "max_runs"),
                       (lambda: enc(lab, True), "max_runs"),
                       (lambda: enc(lab, 8, runs=torch.zeros(8, 3, dtype=I32)), "runs"),
                       (lambda: enc(lab, 8, runs=torch.zeros(8, 2, dtype=torch.int64)), "runs"),
                       (lambda: enc(lab, 8, runs=torch.zeros(1, 8, 2, dtype=I32)), "runs"),
                       (lambda: enc(lab, 8, runs=torch.zeros(8, 4, dtype=I32)[:, ::2]), "runs"),
                       (lambda: enc(lab, 8, runs=shared[1:17].view(8, 2)), "runs must be a contiguous, 8-byte aligned"),
                       (lambda: enc(lab, 8, runs=[0]), "runs"),
                       (lambda: enc(lab, count=torch.zeros(1, dtype=I32)), "count"),
                       (lambda: enc(lab, count=torch.zeros((), dtype=torch.int64)), "count"),
                       (lambda: enc(lab[None], count=torch.zeros((), dtype=I32)), "count"),
                       (lambda: enc(shared.view(torch.uint8)[:12].view(3, 4), 8, runs=shared[:16].view(8, 2)), "runs overlaps labels"),
                       (lambda: enc(lab, 8, runs=shared[:16].view(8, 2), count=shared[3].view(())), "count overlaps runs"),
                       (lambda: enc(shared.view(torch.uint8)[:12].view(3, 4), count=shared[2].view(())), "count overlaps labels"),
                       (lambda: dec(runs.long(), count, 3, 4), "runs"), (lambda: dec(runs[:, :1], count, 3, 4), "runs"),
                       (lambda: dec(runs.reshape(-1), count, 3, 4), "runs"), (lambda: dec(shared[1:17].view(8, 2), count, 3, 4), "runs"),
                       (lambda: dec(None, count, 3, 4), "runs"),
                       (lambda: dec(runs, None, 3, 4), "count"), (lambda: dec(runs, count.long(), 3, 4), "count"),
                       (lambda: dec(runs, count[None], 3, 4), "count"), (lambda: dec(runs[None], count, 3, 4), "count"),
                       (lambda: dec(runs, count, 0, 4), "H must"), (lambda: dec(runs, count, 3, True), "W must"),
                       (lambda: dec(runs, count, 3.0, 4), "H must"), (lambda: dec(runs, count, 2 ** 16, 2 ** 15), "pixels"),
                       (lambda: dec(runs, count, 3, 4, torch.int32), "dtype"), (lambda: dec(runs, count, 3, 4, fill=256), "fill"),
                       (lambda: dec(runs, count, 3, 4, fill=-1), "fill"), (lambda: dec(runs, count, 3, 4, torch.int16, fill=2 ** 15), "fill"),
                       (lambda: dec(runs, count, 3, 4, fill=1.0), "fill"),
                       (lambda: dec(runs, count, 3, 4, out=torch.zeros(4, 3, dtype=torch.uint8)), "out"),
                       (lambda: dec(runs, count, 3, 4, out=torch.zeros(3, 4, dtype=torch.int16)), "out"),
                       (lambda: dec(shared[:16].view(8, 2), count, 3, 4, out=shared.view(torch.uint8)[60:72].view(3, 4)), "out overlaps runs"),
                       (lambda: dec(runs, shared[0].view(()), 3, 4, out=shared.view(torch.uint8)[:12].view(3, 4)), "out overlaps count"),
                       (lambda: dec(shared[:16].view(8, 2), shared[15].view(()), 3, 4), "count overlaps runs"),
                       (lambda: dec(runs, count, 3, 4, flag=torch.zeros(2, dtype=I32)), "flag"),
                       (lambda: dec(shared[:16].view(8, 2), count, 3, 4, flag=shared[15:16]), "runs overlaps flag"),
                       (lambda: dec(runs, shared[0].view(()), 3, 4, flag=shared[:1]), "count overlaps flag")):
        with pytest.raises(ValueError, match=what):
            call()


def test_segmenter_refusals_come_before_any_launch(monkeypatch):
    rec = L.Recorder(monkeypatch)                                 # hip.lib and every binding fail or record
    monkeypatch.setattr(hip, "seg_rle_encode", lambda *a, **k: pytest.fail("the binding was reached"))
    seg = Segmenter(L._Model(), category_token_ids=[[1]] * L.N)
    imgs, _ = L._images()
    x = torch.zeros(2, 3, 32, 48)
    for bad in (0, 2 ** 24 + 1, 8.0, True):
        with pytest.raises(ValueError, match="max_runs"):
            seg.export_raw(imgs, max_runs=bad)
        with pytest.raises(ValueError, match="max_runs"):
            seg.export(x, max_runs=bad)
    with pytest.raises(TypeError):
        seg.export_raw(imgs, return_conf=True)
    with pytest.raises(ValueError, match="slide"):
        seg.export_raw(imgs, slide=L.SLIDE, flip=True)
    assert rec.log == []


# ------------------------------------------------------------------------------------------------- the header, the library
def test_header_declares_the_entry_points_and_keeps_the_abi():
    with open(os.path.join(ROOT, "include", "ifseg_hip.h")) as f:
        text = f.read()
    assert int(re.search(r"#define\s+IFSEG_ABI_VERSION\s+(\d+)", text).group(1)) == 21 == hip.ABI_VERSION
    with open(os.path.join(ROOT, "ifseg_amd", "csrc", "rle.hip")) as f:
        src = f.read()
    for name in ("ifseg_seg_rle_encode", "ifseg_seg_rle_decode", "ifseg_seg_rle_limit"):
        assert re.search(r"^int %s\(" % name, text, re.M), name
        assert 'extern "C" int %s(' % name in src, name
    assert hip.SEG_RLE_MAX_RUNS == 2 ** 24 == 1 << int(re.search(r"RL_MAX_RUNS = 1 << (\d+);", src).group(1))
    assert hip.SEG_RLE_CHUNK == 32 == int(re.search(r"RL_CHUNK = (\d+);", src).group(1)) == T.CHUNK
    assert hip.SEG_RLE_COLS == 64 == int(re.search(r"RL_COLS = (\d+);", src).group(1)) == T.COLS
    assert T.ROWS * 4 == T.CHUNK and "RL_ROWS = RL_CHUNK / 4;" in src
    assert "atomic" not in src.split("rle_decode_kernel(")[0].split("namespace {")[1]     # the encoder has none


def test_no_torch_op_was_added():
    import ifseg_amd.ops  # noqa: F401
    assert not any("rle" in name for name in dir(torch.ops.ifseg))


def _library():
    if not os.path.exists(hip.LIB_PATH):
        from ifseg_amd.build import build
        build(verbose=False)
    return hip.lib()


def test_library_exports_and_limits():
    lib = _library()
    assert all(hasattr(lib, name) for name in ("ifseg_seg_rle_encode", "ifseg_seg_rle_decode", "ifseg_seg_rle_limit"))
    assert hip.seg_rle_limits() == (hip.SEG_RLE_CHUNK, hip.SEG_RLE_COLS, hip.SEG_RLE_MAX_RUNS) == (32, 64, 2 ** 24)
    assert lib.ifseg_seg_rle_limit(ctypes.c_int(3)) == BAD_ARG and lib.ifseg_seg_rle_limit(ctypes.c_int(-1)) == BAD_ARG


def test_c_entry_refusals_need_no_device():
    """every refusal returns before anything is launched or dereferenced: the buffers are host memory here"""
    lib = _library()
    B, H, W, R = 2, 17, 65, 8
    npix = B * H * W
    nseg = W * -(-H // 32)
    keep = []

    def buf(nbytes):
        raw = ctypes.create_string_buffer(nbytes + 64)
        keep.append(raw)
        return (ctypes.addressof(raw) + 63) & ~63                 # 64-byte aligned

    a = dict(labels=buf(2 * npix), seg=buf(4 * B * nseg), runs=buf(8 * B * R), count=buf(4 * B), out=buf(2 * npix), flag=buf(4))
    before = [bytes(raw) for raw in keep]
    ci, vp = ctypes.c_int, ctypes.c_void_p

    def enc(lb=2, b=B, h=H, w=W, r=R, **ptr):
        p = dict(a, **ptr)
        return lib.ifseg_seg_rle_encode(vp(p["labels"]), ci(lb), ci(b), ci(h), ci(w), ci(r), vp(p["seg"]), vp(p["runs"]),
                                        vp(p["count"]), None)

    def dec(lb=2, b=B, h=H, w=W, r=R, fill=255, **ptr):
        p = dict(a, **ptr)
        return lib.ifseg_seg_rle_decode(vp(p["runs"]), vp(p["count"]), ci(b), ci(h), ci(w), ci(r), ci(lb), ci(fill), vp(p["out"]),
                                        vp(p["flag"]), None)

    for call, names in ((enc, ("labels", "seg", "runs", "count")), (dec, ("runs", "count", "out", "flag"))):
        for name in names:
            assert call(**{name: None}) == BAD_ARG, name          # null
        for name in names:
            if name not in ("labels", "out"):
                assert call(**{name: a[name] + 2}) == BAD_ARG, name       # misaligned
        assert call(runs=a["runs"] + 4) == BAD_ARG                # a run is one 8-byte word
        for i, x in enumerate(names):                             # any two buffers sharing a byte
            for y in names[i + 1:]:
                assert call(**{y: a[x]}) == BAD_ARG, (x, y)
        for kw in (dict(lb=0), dict(lb=3), dict(lb=4), dict(r=0), dict(r=-1), dict(r=2 ** 24 + 1)):
            assert call(**kw) == BAD_ARG, kw
        for kw in (dict(b=0), dict(h=0), dict(w=-1), dict(b=1 << 15, h=1 << 8, w=1 << 8)):
            assert call(**kw) == BAD_SHAPE, kw
    assert enc(labels=a["labels"] + 1) == BAD_ARG and dec(out=a["out"] + 1) == BAD_ARG      # int16 at an odd address
    assert enc(count=a["runs"] + 8 * B * R - 4) == BAD_ARG and dec(flag=a["out"] + 2 * npix - 4) == BAD_ARG
    for kw in (dict(lb=1, fill=256), dict(lb=1, fill=-1), dict(lb=2, fill=32768), dict(lb=2, fill=-32769)):
        assert dec(**kw) == BAD_ARG, kw
    assert [bytes(raw) for raw in keep] == before                 # nothing was written


# ------------------------------------------------------------------------------------------------- the Segmenter's calls
MAX_RUNS = 77


def _fake_encode(log):
    def seg_rle_encode(labels, max_runs=65536, runs=None, count=None):
        assert labels.is_contiguous() and labels.dim() == 2 and labels.dtype == torch.uint8 and runs is None and count is None
        log.append(("seg_rle_encode", tuple(labels.shape), max_runs))
        return torch.zeros(max_runs, 2, dtype=I32), torch.zeros((), dtype=I32)
    return seg_rle_encode


class Recorder(SieveRecorder):
    def __init__(self, monkeypatch):
        super().__init__(monkeypatch)
        monkeypatch.setattr(hip, "seg_rle_encode", _fake_encode(self.log))
        monkeypatch.setattr(hip, "seg_rle_decode", lambda *a, **k: pytest.fail("seg_rle_decode was reached"))


def _encodes(shapes=(L.A, L.B)):
    return [("seg_rle_encode", hw, MAX_RUNS) for hw in shapes]


def _without_conf(log):
    return [e[:3] + (dict(e[3], conf=False),) if e[0].startswith("seg_predict") else e for e in log]


@pytest.mark.parametrize("sieve", [False, True], ids=["plain", "sieve"])
@pytest.mark.parametrize("crf", [False, True], ids=["plain", "crf"])
@pytest.mark.parametrize("setting", list(L.SETTINGS))
def test_export_raw_launch_sequence(monkeypatch, setting, crf, sieve):
    """segment_raw's launches with no conf asked for, a seg_sieve behind each image's where sieve= is set, then one
    seg_rle_encode per image"""
    rec = Recorder(monkeypatch)
    extra = dict(sieve=SIEVE_K, sieve_connectivity=SIEVE_CONN, sieve_passes=SIEVE_PASSES) if sieve else {}
    seg = Segmenter(L._Model(), category_token_ids=[[1]] * L.N, crf_iters=2 if crf else 0, **extra, **L.SETTINGS[setting][1])
    imgs, _ = L._images()
    out = seg.export_raw(imgs, max_runs=MAX_RUNS, max_batch=3, **L.SETTINGS[setting][2])
    assert len(out) == 2 and all(isinstance(m, RunLengthMap) for m in out)
    assert [m.shape for m in out] == [L.A, L.B] and all(m.max_runs == MAX_RUNS and m.dtype == torch.uint8 and m.n == L.N for m in out)
    want = _without_conf(L._expected(setting, crf, "segment_raw"))
    want = (_sieved(want, False) if sieve else want) + _encodes()
    assert len(rec.log) == len(want), [e[0] for e in rec.log]
    for k, (got, exp) in enumerate(zip(rec.log, want)):
        assert got == exp, (k, got, exp)


def test_export_launch_sequence(monkeypatch):
    """`export` takes what `__call__` takes: its launches, then one seg_rle_encode per image of the batch"""
    rec = Recorder(monkeypatch)
    seg = Segmenter(L._Model(), category_token_ids=[[1]] * L.N)
    x = torch.stack([rec.coded(("x", b), 3, 32, 48) for b in range(2)])
    items = [("x", 0, False), ("x", 1, False)]
    out = seg.export(x, max_runs=MAX_RUNS)
    assert len(out) == 2 and all(m.shape == (32, 48) for m in out)
    assert rec.log == [("forward", items), ("seg_predict", (items, 2, 3), (2, 32, 48), dict(conf=False, probs=False))] \
        + _encodes([(32, 48)] * 2)
    del rec.log[:]
    sizes = [(40, 50), (7, 9)]
    out = seg.export(x, out_hw=sizes, max_runs=MAX_RUNS)
    assert [m.shape for m in out] == sizes
    want = [("forward", items)] + [("seg_predict", (items[b:b + 1], 2, 3), (1,) + s, dict(conf=False, probs=False)) for b, s in enumerate(sizes)]
    assert rec.log == want + _encodes(sizes)
    # with the CRF and the sieve: behind both
    del rec.log[:]
    seg = Segmenter(L._Model(), category_token_ids=[[1]] * L.N, crf_iters=2, sieve=SIEVE_K, sieve_connectivity=SIEVE_CONN,
                    sieve_passes=SIEVE_PASSES)
    seg.export(x, max_runs=MAX_RUNS)
    assert [e[0] for e in rec.log] == ["forward", "seg_predict", "crf", "crf", "seg_sieve", "seg_rle_encode", "seg_rle_encode"]


def test_export_raw_behind_pamr(monkeypatch):
    """pamr_iters=3: per image the predict launch with every class's value, `seg_pamr` with neither conf nor probs asked for,
    and then the encodes"""
    rec = PM.Recorder(monkeypatch)
    monkeypatch.setattr(hip, "seg_rle_encode", _fake_encode(rec.log))
    seg = PM._seg(pamr_iters=3, pamr_dilations=(1, 2))
    imgs, _ = PM._images()
    out = seg.export_raw(imgs, max_runs=MAX_RUNS, max_batch=3)
    assert [m.shape for m in out] == [PM.A, PM.B]
    want = list(PM.FRONT)
    for i, hw in enumerate((PM.A, PM.B)):
        want += [("seg_predict", PM.GRIDS[i], hw, dict(conf=False, probs=True)),
                 ("seg_pamr", i, (PM.N,) + hw, 3, (1, 2), dict(conf=False, probs_out=False, label_dtype=PM.U8))]
    assert rec.log == want + _encodes((PM.A, PM.B))


@pytest.mark.parametrize("setting", list(L.SETTINGS))
def test_a_segmenter_that_exports_nothing_launches_what_it_did(monkeypatch, setting):
    rec = L.Recorder(monkeypatch)
    for name in ("seg_rle_encode", "seg_rle_decode"):
        monkeypatch.setattr(hip, name, lambda *a, **k: pytest.fail("a run-length binding was reached"))
    seg = Segmenter(L._Model(), category_token_ids=[[1]] * L.N, **L.SETTINGS[setting][1])
    imgs, gts = L._images()
    seg.segment_raw(imgs, max_batch=3, return_conf=True, **L.SETTINGS[setting][2])
    assert rec.log == L._expected(setting, False, "segment_raw")
    del rec.log[:]
    seg.evaluate_raw(imgs, gts, max_batch=3, **L.SETTINGS[setting][2])
    assert rec.log == L._expected(setting, False, "evaluate_raw")


def test_task_hands_the_keywords_on(monkeypatch):
    from ifseg_amd.tasks.mm_tasks import SegmentationTask
    task = SegmentationTask(num_seg_tokens=5, patch_image_size=64, n_base_vocab=100, category_token_ids=[[5]] * 5)
    seen = []

    class Seg:
        def __getattr__(self, name):
            return lambda *a, **kw: seen.append((name, kw))

    monkeypatch.setattr(task, "build_segmenter", lambda model, **kw: seen.append(("ctor", kw)) or Seg())
    task.export_raw(None, [], sieve=16, sieve_connectivity=8, upsample="logits", pamr_iters=2, max_runs=64, max_batch=2, slide=True)
    assert seen[0] == ("ctor", dict(sieve=16, sieve_connectivity=8, upsample="logits", pamr_iters=2))
    assert seen[1] == ("export_raw", dict(max_runs=64, max_batch=2, slide=True))
