"""CPU: the specification of the sieve (ifseg_amd/predict.py: sieve_reference) against a literal flood-fill transcription of its
four statements and against hand-written answers, its invariants, the header and the constants, every refusal that comes before
a launch, and which `hip` calls a `Segmenter(sieve=K)` makes."""
import os
import re

import pytest
import torch

import _sieve_cases as S
import test_segmenter_launches_cpu as L
from ifseg_amd import hip
from ifseg_amd.predict import Segmenter, SegmentationScore, regions_reference, sieve_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS4 = ((-1, 0), (0, -1), (0, 1), (1, 0))
STEPS8 = STEPS4 + ((-1, -1), (-1, 1), (1, -1), (1, 1))


# ------------------------------------------------------------------------------------------------- the literal rule
def literal_pass(lab, K, conn, ignore):
    """one pass on one image, lab a list of rows -> the new rows: flood fills, then the four statements word for word"""
    H, W = len(lab), len(lab[0])
    region = [[-1] * W for _ in range(H)]
    regions = []                                                  # (value, root, pixels); raster order finds the root first
    for y0 in range(H):
        for x0 in range(W):
            if region[y0][x0] >= 0:
                continue
            k, v = len(regions), lab[y0][x0]
            region[y0][x0] = k
            stack, pixels = [(y0, x0)], []
            while stack:
                y, x = stack.pop()
                pixels.append((y, x))
                for dy, dx in (STEPS8 if conn == 8 else STEPS4):
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < H and 0 <= xx < W and region[yy][xx] < 0 and lab[yy][xx] == v:
                        region[yy][xx] = k
                        stack.append((yy, xx))
            regions.append((v, y0 * W + x0, pixels))
    key = [(len(px), -root) for _, root, px in regions]           # 1: (size, -root), lexicographic
    out = [row[:] for row in lab]
    for k, (v, _, pixels) in enumerate(regions):
        if not (len(pixels) < K and v != ignore):                 # 2: small
            continue
        nb = set()                                                # 3: always 4-adjacency; never a region of the ignored value
        for y, x in pixels:
            for dy, dx in STEPS4:
                yy, xx = y + dy, x + dx
                if 0 <= yy < H and 0 <= xx < W and region[yy][xx] != k and lab[yy][xx] != ignore:
                    nb.add(region[yy][xx])
        if not nb:
            continue
        q = max(nb, key=lambda r: key[r])                         # 4: the largest key, and only if larger than its own
        if key[q] > key[k]:
            for y, x in pixels:
                out[y][x] = regions[q][0]
    return out


def literal(labels, K, conn, ignore):
    """one pass on [H, W] or [B, H, W], image by image"""
    if labels.dim() == 3:
        return torch.stack([literal(one, K, conn, ignore) for one in labels])
    return torch.tensor(literal_pass(labels.tolist(), K, conn, ignore), dtype=labels.dtype)


@pytest.mark.parametrize("conn", S.CONNECTIVITIES)
@pytest.mark.parametrize("name", S.PATTERNS + ("batches",))
def test_reference_equals_the_literal_rule(name, conn):
    keys = S.BATCHES if name == "batches" else [(name, H, W, False) for H, W in S.SHAPES]
    for key in keys:
        lab = S.labels_of(key)
        for K in S.MIN_REGIONS:
            for ignore in (None, S.present_value(key)):
                cur = lab
                for k in range(3):                                # pass by pass
                    want = literal(cur, K, conn, ignore)
                    got = sieve_reference(cur, K, conn, 1, ignore)[0]
                    assert got.dtype == lab.dtype and torch.equal(got, want), (key, K, ignore, k)
                    cur = want
                assert torch.equal(S.reference(key, conn, K, 3, ignore)[0], cur), (key, K, ignore)


def test_reference_by_hand():
    lab = torch.tensor([[1, 1, 1, 1, 1, 2],
                        [1, 3, 1, 4, 4, 2],
                        [1, 1, 1, 1, 1, 2],
                        [0, 0, 5, 6, 6, 2]], dtype=torch.uint8)
    # K = 2: the 3 is an island of the 1s; the 5 (key (1, -20)) takes the larger of its neighbours 1 (13), 0 and 6 (2 each)
    out, moved = sieve_reference(lab, 2, n=7)
    want = lab.clone()
    want[1, 1] = 1
    want[3, 2] = 1
    assert torch.equal(out, want)
    assert moved.tolist() == [[0, 0, 0, 1, 0, 1, 0], [0, 2, 0, 0, 0, 0, 0]]
    # K = 3: the pairs join their largest neighbour as well: 4 4 -> 1; 0 0 -> 1; 6 6 -> 1 (13 pixels against the 2s' 4)
    out, moved = sieve_reference(lab, 3, n=7)
    want = torch.ones_like(lab)
    want[:, 5] = 2
    assert torch.equal(out, want)
    # with the 1s ignored, no region may take their value; the 3 has no other neighbour and stays, the 5 joins the 0s (the
    # smaller root wins the tie with the 6s), and the 4s and the 6s join the 2s
    out, _ = sieve_reference(lab, 3, ignore=1, n=7)
    want = lab.clone()
    want[3, 2] = 0
    want[1, 3:5] = 2
    want[3, 3:5] = 2
    assert torch.equal(out, want)
    # a second pass: 0 0 0 has three pixels now and stays
    assert torch.equal(sieve_reference(lab, 3, passes=2, ignore=1, n=7)[0], want)
    # two single pixels never swap: the one with the larger root joins the other
    pair = torch.tensor([[7, 9]], dtype=torch.int16)
    assert sieve_reference(pair, 5)[0].tolist() == [[7, 7]]
    # raw_labels: class = value - 1; a value of 0 is not counted
    out, moved = sieve_reference(torch.tensor([[0, 2, 2]], dtype=torch.uint8), 2, n=3, raw_labels=True)
    assert out.tolist() == [[2, 2, 2]] and moved.tolist() == [[0, 0, 0], [0, 1, 0]]


def _fixed_point(lab, K, conn, ignore, cap=64):
    for _ in range(cap):
        new = sieve_reference(lab, K, conn, 1, ignore)[0]
        if torch.equal(new, lab):
            return lab
        lab = new
    raise AssertionError("no fixed point within %d passes" % cap)


@pytest.mark.parametrize("conn", S.CONNECTIVITIES)
def test_invariants(conn):
    keys = [(p, H, W, s) for p, s in (("speckled", False), ("random5", True), ("blocks", False), ("rings", False),
                                      ("checkerboard", False)) for H, W in ((17, 65), (33, 129))] + ["batch"]
    for key in keys:
        lab = S.labels_of(key)
        conf = S.conf_of(key)
        ign = S.present_value(key)
        _, size = regions_reference(lab, conn)
        assert torch.equal(sieve_reference(lab, 1, conn, 3)[0], lab)                  # K = 1 is the identity
        for K in (2, 9, 10 ** 6):
            for passes in (1, 3):
                out, moved, cf = S.reference(key, conn, K, passes, None)
                assert out.dtype == lab.dtype and out.shape == lab.shape and moved.dtype == torch.int64
                assert torch.equal(out[size >= K], lab[size >= K])                    # a region of K pixels or more only grows
                changed = out != lab
                assert torch.equal(cf == 0, changed) and torch.equal(cf[~changed], conf[~changed])
                inside = (lab.long() >= 0) & (lab.long() < S.N) & (out.long() >= 0) & (out.long() < S.N)
                if bool(inside.all()):
                    assert int(moved[0].sum()) == int(moved[1].sum()) == int(changed.sum())
                was = lab[changed].long()
                assert torch.equal(moved[0], torch.bincount(was[(was >= 0) & (was < S.N)], minlength=S.N))
                out_i = S.reference(key, conn, K, passes, ign)[0]
                assert torch.equal(out_i == ign, lab == ign)                          # nothing becomes `ignore`, no `ignore` changes
                if lab.dim() == 3:                                                    # a batch is its images one by one
                    for b in range(lab.shape[0]):
                        one = sieve_reference(lab[b], K, conn, passes, None, n=S.N)
                        assert torch.equal(one[0], out[b])
                    assert torch.equal(sum(sieve_reference(lab[b], K, conn, passes, None, n=S.N)[1] for b in range(lab.shape[0])), moved)
        if key == "batch" or key[1] > 17 or key[0] == "checkerboard":
            continue                            # (the checkerboard is the worst case: all keys tie on size, a pixel per pass)
        for K in (2, 9):                                          # at the fixed point nothing is small and below a neighbour
            for ignore in (None, ign):
                fixed = _fixed_point(lab, K, conn, ignore)
                assert torch.equal(literal(fixed, K, conn, ignore), fixed), (key, K, ignore)


def test_speckles_vanish():
    """What the filter is for: 16 x 50 blocks with 5 % of the pixels flipped.  A flipped pixel comes back unless it sits in a
    cluster of K or more flipped pixels of one value (at 5 % and K >= 4: a few in 10 000) or beside a block edge, where the
    other block may be its largest neighbour (16 % of the pixels lie beside an edge, 5 % of them are flipped, at most all of
    those go wrong: 0.8 %), so at least 99 % of the map is the clean one, where 95 % were.  One pass can leave a pixel whose
    only neighbours were small themselves (it takes a value that moves on in the same pass); the next pass takes it."""
    key = ("speckled", 48, 200, False)
    lab, clean = S.labels_of(key), S.clean_blocks(48, 200)
    assert 0.94 < float((lab == clean).float().mean()) < 0.96
    for conn in (4, 8):
        for K in (4, 16):
            out = S.reference(key, conn, K, 3, None)[0]
            assert float((out == clean).float().mean()) >= 0.99, (conn, K)
            assert int(regions_reference(out, conn)[1].min()) >= K, (conn, K)
            assert torch.equal(sieve_reference(out, K, conn)[0], out)                 # a fixed point


# ------------------------------------------------------------------------------------------------- refusals
def test_reference_refusals():
    lab = torch.zeros(3, 4, dtype=torch.uint8)
    for kw, what in ((dict(min_region=0), "min_region"), (dict(min_region=2.0), "min_region"), (dict(min_region=True), "min_region"),
                     (dict(min_region=2 ** 31), "min_region"), (dict(connectivity=6), "connectivity"), (dict(passes=0), "passes"),
                     (dict(passes=1.0), "passes"), (dict(ignore=1.5), "ignore"), (dict(ignore=True), "ignore"), (dict(n=0), "n must"),
                     (dict(n=513), "n must"), (dict(conf=torch.zeros(4, 3)), "conf")):
        with pytest.raises(ValueError, match=what):
            sieve_reference(lab, **{"min_region": 2, **kw})
    for bad in (lab.float(), lab.bool(), lab.reshape(-1)):
        with pytest.raises(ValueError, match="labels"):
            sieve_reference(bad, 2)


def test_binding_refusals_come_before_any_launch(monkeypatch):
    """every one is a ValueError that names its argument, raised on CPU tensors: the library was not reached"""
    monkeypatch.setattr(hip, "lib", lambda: pytest.fail("the library was reached"))
    lab = torch.zeros(3, 4, dtype=torch.uint8)
    i64 = torch.int64
    for call, what in ((lambda: hip.seg_sieve(lab, 0), "min_region"), (lambda: hip.seg_sieve(lab, 2.0), "min_region"),
                       (lambda: hip.seg_sieve(lab, True), "min_region"), (lambda: hip.seg_sieve(lab, 2 ** 31), "min_region"),
                       (lambda: hip.seg_sieve(lab, 2, 6), "connectivity"), (lambda: hip.seg_sieve(lab, 2, True), "connectivity"),
                       (lambda: hip.seg_sieve(lab, 2, passes=0), "passes"), (lambda: hip.seg_sieve(lab, 2, passes=9), "passes"),
                       (lambda: hip.seg_sieve(lab, 2, passes=2.0), "passes"), (lambda: hip.seg_sieve(lab, 2, ignore=0.5), "ignore"),
                       (lambda: hip.seg_sieve(lab, 2, ignore=False), "ignore"), (lambda: hip.seg_sieve(lab, 2, n=0), "n must"),
                       (lambda: hip.seg_sieve(lab, 2, n=513), "n must"), (lambda: hip.seg_sieve(lab.long(), 2), "labels"),
                       (lambda: hip.seg_sieve(lab.t(), 2), "labels"), (lambda: hip.seg_sieve(lab.reshape(-1), 2), "labels"),
                       (lambda: hip.seg_sieve([[0]], 2), "labels"), (lambda: hip.seg_sieve(lab, 2, out=lab), "out"),
                       (lambda: hip.seg_sieve(lab, 2, out=torch.zeros(3, 4, dtype=torch.int16)), "out"),
                       (lambda: hip.seg_sieve(lab, 2, conf=torch.zeros(3, 4, dtype=torch.float64)), "conf"),
                       (lambda: hip.seg_sieve(lab, 2, conf=torch.zeros(4, 3)), "conf"),
                       (lambda: hip.seg_sieve(lab, 2, n=3, moved=torch.zeros(2, 4, dtype=i64)), "moved"),
                       (lambda: hip.seg_sieve(lab, 2, n=3, moved=torch.zeros(2, 3, dtype=torch.int32)), "moved"),
                       (lambda: hip.seg_sieve(lab, 2, n=3, moved=torch.zeros(3, dtype=i64)), "moved"),
                       (lambda: hip.seg_sieve(lab, 2, flag=torch.zeros(2, dtype=torch.int32)), "flag")):
        with pytest.raises(ValueError, match=what):
            call()


def test_segmenter_refusals_come_before_any_launch(monkeypatch):
    rec = L.Recorder(monkeypatch)                                 # hip.lib and every binding fail or record
    mk = lambda **kw: Segmenter(L._Model(), category_token_ids=[[1]] * L.N, **kw)
    for kw, what in ((dict(sieve=0), "sieve must"), (dict(sieve=2.5), "sieve must"), (dict(sieve=True), "sieve must"),
                     (dict(sieve=2 ** 31), "sieve must"), (dict(sieve=4, sieve_connectivity=6), "sieve_connectivity"),
                     (dict(sieve_connectivity=True), "sieve_connectivity"), (dict(sieve=4, sieve_passes=0), "sieve_passes"),
                     (dict(sieve_passes=9), "sieve_passes"), (dict(sieve=4, sieve_passes=2.0), "sieve_passes")):
        with pytest.raises(ValueError, match=what):
            mk(**kw)
    seg = mk(sieve=4)
    assert (seg.sieve, seg.sieve_connectivity, seg.sieve_passes, seg.sieve_moved) == (4, 4, 2, None)
    assert mk().sieve is None
    imgs, gts = L._images()
    x, gt = torch.zeros(2, 3, 32, 48), torch.ones(2, 32, 48, dtype=torch.uint8)
    carrying = SegmentationScore(L.N, torch.device("cpu"), calibration=True)
    for call in (lambda: seg.evaluate_raw(imgs, gts, calibration=True), lambda: seg.evaluate_raw(imgs, gts, into=carrying),
                 lambda: seg.evaluate(x, gt, calibration=True), lambda: seg.evaluate(x, gt, into=carrying),
                 lambda: seg.calibrate_raw(imgs, gts), lambda: seg.calibrate(x, gt)):
        with pytest.raises(ValueError, match="sieve = 4"):
            call()
    assert rec.log == []


# ------------------------------------------------------------------------------------------------- the header, the constants
def test_header_declares_the_entry_points_and_keeps_the_abi():
    with open(os.path.join(ROOT, "include", "ifseg_hip.h")) as f:
        text = f.read()
    assert int(re.search(r"#define\s+IFSEG_ABI_VERSION\s+(\d+)", text).group(1)) == 21 == hip.ABI_VERSION
    with open(os.path.join(ROOT, "ifseg_amd", "csrc", "sieve.hip")) as f:
        src = f.read()
    for name in ("ifseg_seg_sieve", "ifseg_seg_sieve_limit"):
        assert re.search(r"^int %s\(" % name, text, re.M), name
        assert 'extern "C" int %s(' % name in src, name
    assert hip.SEG_SIEVE_MAX_PASSES == 8 == int(re.search(r"SV_MAX_PASSES = (\d+);", src).group(1))
    assert hip.SEG_SIEVE_MAX_CLASSES == 512 == int(re.search(r"SV_MAX_CLASSES = (\d+);", src).group(1))
    assert callable(hip.seg_sieve_limits)


def test_task_hands_the_keywords_to_the_constructor(monkeypatch):
    from ifseg_amd.tasks.mm_tasks import SegmentationTask
    task = SegmentationTask(num_seg_tokens=5, patch_image_size=64, n_base_vocab=100, category_token_ids=[[5]] * 5)
    seen = []

    class Seg:
        def __getattr__(self, name):
            return lambda *a, **kw: seen.append((name, kw))

    monkeypatch.setattr(task, "build_segmenter", lambda model, **kw: seen.append(("ctor", kw)) or Seg())
    for name in ("evaluate_raw", "calibrate_raw", "render_raw", "pseudo_label_raw"):
        del seen[:]
        args = (None, [], []) if name in ("evaluate_raw", "calibrate_raw") else (None, [])
        getattr(task, name)(*args, sieve=16, sieve_connectivity=8, sieve_passes=3, max_batch=2)
        assert seen[0] == ("ctor", dict(sieve=16, sieve_connectivity=8, sieve_passes=3))
        assert seen[1][0] == name and seen[1][1].get("max_batch") == 2 and "sieve" not in seen[1][1]


# ------------------------------------------------------------------------------------------------- the Segmenter's calls
K, CONN, PASSES = 16, 8, 3


class Recorder(L.Recorder):
    def __init__(self, monkeypatch):
        super().__init__(monkeypatch)
        monkeypatch.setattr(hip, "seg_sieve", self.seg_sieve)
        self.moved = []

    def seg_sieve(self, labels, min_region, connectivity=4, passes=1, ignore=None, n=None, raw_labels=False, conf=None, out=None,
                  moved=None, flag=None):
        assert labels.is_contiguous() and labels.dim() == 3 and ignore is None and not raw_labels and out is None and flag is None
        assert conf is None or (conf.shape == labels.shape and conf.dtype == torch.float32 and conf.is_contiguous())
        assert moved.dtype == torch.int64 and tuple(moved.shape) == (2, L.N)
        self.moved.append(moved)
        self.log.append(("seg_sieve", tuple(labels.shape), (min_region, connectivity, passes, n), dict(conf=conf is not None)))
        return torch.full_like(labels, 3), moved


def _sieved(log, conf_at):
    """the expected log of the existing suite with one seg_sieve behind every image's predict launch (and its CRF)"""
    out = []
    for k, e in enumerate(log):
        nxt = log[k + 1][0] if k + 1 < len(log) else ""
        out.append(e)
        if (e[0].startswith("seg_predict") and nxt != "crf") or e[0] == "crf":
            shape = e[2] if e[0] != "crf" else (1,) + e[2][:2]
            out.append(("seg_sieve", shape, (K, CONN, PASSES, L.N), dict(conf=conf_at)))
    return out


@pytest.mark.parametrize("method", ["segment_raw", "evaluate_raw", "evaluate_raw_confusion"])
@pytest.mark.parametrize("crf", [False, True], ids=["plain", "crf"])
@pytest.mark.parametrize("setting", list(L.SETTINGS))
def test_raw_launch_sequence_with_the_sieve(monkeypatch, setting, crf, method):
    rec = Recorder(monkeypatch)
    seg = Segmenter(L._Model(), category_token_ids=[[1]] * L.N, crf_iters=2 if crf else 0, sieve=K, sieve_connectivity=CONN,
                    sieve_passes=PASSES, **L.SETTINGS[setting][1])
    imgs, gts = L._images()
    if method == "segment_raw":
        out = seg.segment_raw(imgs, max_batch=3, return_conf=True, **L.SETTINGS[setting][2])
        assert [tuple(r.labels.shape) for r in out] == [L.A, L.B] and all(r.conf is not None and r.probs is None for r in out)
        assert all(bool((r.labels == 3).all()) for r in out)      # the sieved map is what comes back
        want = _sieved(L._expected(setting, crf, method), True)
    else:
        pairs = method.endswith("confusion")
        score = seg.evaluate_raw(imgs, gts, max_batch=3, confusion=pairs, **L.SETTINGS[setting][2])
        assert isinstance(score, SegmentationScore) and (score.confusion is not None) == pairs
        # predict -> (CRF) -> sieve -> seg_areas -> seg_confusion: the branch the CRF takes, whether it is on or not
        front, whats = L._front(L.SETTINGS[setting][0])
        kernel, softmax = L.SETTINGS[setting][3:5]
        sm = {} if softmax is None else {"softmax": softmax}
        want = list(front)
        for i, (what, hw) in enumerate(zip(whats, (L.A, L.B))):
            shape = (1,) + hw
            want += [("seg_predict" + kernel, what, shape, dict(conf=False, probs=crf, **sm))]
            want += [("crf", float(i), hw + (3,), (L.N,) + hw, 2)] * crf
            want += [("seg_sieve", shape, (K, CONN, PASSES, L.N), dict(conf=False)),
                     ("seg_areas", shape, dict(counters=True, raw_labels=True))]
            want += [("seg_confusion", shape, dict(matrix=True, raw_labels=True))] * pairs
    assert len(rec.log) == len(want), [e[0] for e in rec.log]
    for k, (got, exp) in enumerate(zip(rec.log, want)):
        assert got == exp, (k, got, exp)
    assert len(rec.moved) == 2 and all(m is seg.sieve_moved for m in rec.moved)     # one counter, accumulated over the calls


@pytest.mark.parametrize("crf", [False, True], ids=["plain", "crf"])
def test_call_and_evaluate_launch_sequence_with_the_sieve(monkeypatch, crf):
    rec = Recorder(monkeypatch)
    seg = Segmenter(L._Model(), category_token_ids=[[1]] * L.N, crf_iters=2 if crf else 0, sieve=K, sieve_connectivity=CONN,
                    sieve_passes=PASSES)
    x = torch.stack([rec.coded(("x", b), 3, 32, 48) for b in range(2)])
    items = [("x", 0, False), ("x", 1, False)]
    grey = [float((x[b, 0, 0, 0] * 0.5 + 0.5) * 255.0) for b in range(2)]
    crf_events = [("crf", grey[b], (32, 48, 3), (L.N, 32, 48), 2) for b in range(2)]
    sieve = lambda shape, conf: ("seg_sieve", shape, (K, CONN, PASSES, L.N), dict(conf=conf))

    res = seg(x, return_probs=True)
    assert bool((res.labels == 3).all()) and res.conf is None and res.probs is not None       # probs as they were
    want = [("forward", items), ("seg_predict", (items, 2, 3), (2, 32, 48), dict(conf=False, probs=True))] + (crf_events if crf else [])
    assert rec.log == want + [sieve((2, 32, 48), False)]

    del rec.log[:]
    sizes = [(32, 48), (32, 48)] if crf else [(40, 50), (7, 9)]
    res = seg(x, out_hw=sizes, return_conf=True)
    want = [("forward", items)]
    for b, s in enumerate(sizes):
        want += [("seg_predict", (items[b:b + 1], 2, 3), (1,) + s, dict(conf=not crf, probs=crf))] + crf_events[b:b + 1] * crf
        want += [sieve((1,) + s, True)]
    assert rec.log == want

    gt = torch.ones(2, 32, 48, dtype=torch.uint8)
    for pairs in (False, True):
        del rec.log[:]
        seg.evaluate(x, gt, confusion=pairs)
        want = [("forward", items), ("seg_predict", (items, 2, 3), (2, 32, 48), dict(conf=False, probs=crf))] + crf_events * crf \
            + [sieve((2, 32, 48), False), ("seg_areas", (2, 32, 48), dict(counters=True, raw_labels=True))]
        assert rec.log == want + [("seg_confusion", (2, 32, 48), dict(matrix=True, raw_labels=True))] * pairs


def test_sieve_none_is_the_code_as_it_was(monkeypatch):
    """without the keyword no sieve is launched, in any method"""
    rec = Recorder(monkeypatch)
    seg = Segmenter(L._Model(), category_token_ids=[[1]] * L.N)
    imgs, gts = L._images()
    seg.segment_raw(imgs, max_batch=3, return_conf=True)
    seg.evaluate_raw(imgs, gts, max_batch=3, confusion=True)
    assert not any(e[0] == "seg_sieve" for e in rec.log) and seg.sieve_moved is None
    assert [e for e in rec.log] == L._expected("single", False, "segment_raw") + L._expected("single", False, "evaluate_raw_confusion")
