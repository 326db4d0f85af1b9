"""GPU: hip.seg_sieve (csrc/sieve.hip) against its specification (`sieve_reference`) on every case of tests/_sieve_cases.py --
both connectivities, three region sizes, one and three passes, uint8 and int16, with and without an ignored value, batched --
in views at element offsets 0, 1 and 3 between canaries, called twice into the same outputs, the C entry's refusals, and a
`Segmenter(sieve=)` end to end on the segofa_tiny fixture.  Everything is integer: every comparison is `torch.equal`."""
import ctypes

import pytest
import torch

import _sieve_cases as S
from test_predict_views_gpu import e2e  # noqa: F401  (the segofa_tiny fixture with its three raw shapes)
from test_regions_gpu import _untouched, _view

pytestmark = pytest.mark.gpu

BAD_SHAPE, BAD_ARG = -2, -3
OFFSETS = (0, 1, 3)
I32 = torch.int32


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ifseg_amd.ops  # noqa: F401
    return torch.device("cuda:0")


def _run_case(hip, key, conn, K, passes, ignore, off, dev, flag, raw=False, layout=False):
    lab = S.labels_of(key)
    w_out, w_moved, w_conf = S.reference(key, conn, K, passes, ignore, raw)
    what = (key, conn, K, passes, ignore, off)
    if not layout:
        conf = S.conf_of(key).to(dev)
        out, moved = hip.seg_sieve(lab.to(dev), K, conn, passes, ignore, n=S.N, raw_labels=raw, conf=conf, flag=flag)
        assert out.dtype == lab.dtype and torch.equal(out.cpu(), w_out), what
        assert moved.dtype == torch.int64 and torch.equal(moved.cpu(), w_moved), what
        assert torch.equal(conf.cpu(), w_conf), what
        return
    # every tensor a view at an element offset between canaries; then a second call into the same out / moved
    d, buf_l = _view(lab.shape, lab.dtype, off, 99, dev, lab)
    out, buf_o = _view(lab.shape, lab.dtype, OFFSETS[(OFFSETS.index(off) + 1) % 3], 77, dev)
    conf, buf_c = _view(lab.shape, torch.float32, OFFSETS[(OFFSETS.index(off) + 2) % 3], -5.0, dev, S.conf_of(key))
    got = hip.seg_sieve(d, K, conn, passes, ignore, n=S.N, raw_labels=raw, conf=conf, out=out, flag=flag)
    assert got[0] is out and torch.equal(out.cpu(), w_out) and torch.equal(got[1].cpu(), w_moved), what
    assert torch.equal(conf.cpu(), w_conf), what
    assert _untouched(buf_o, out.storage_offset(), lab.numel(), 77) and _untouched(buf_c, conf.storage_offset(), lab.numel(), -5.0)
    assert torch.equal(d.cpu(), lab) and _untouched(buf_l, off, lab.numel(), 99), what         # the input is only read
    again = hip.seg_sieve(d, K, conn, passes, ignore, n=S.N, raw_labels=raw, conf=conf, out=out, moved=got[1], flag=flag)
    assert again[0] is out and again[1] is got[1] and torch.equal(out.cpu(), w_out), what
    assert torch.equal(again[1].cpu(), 2 * w_moved) and torch.equal(conf.cpu(), w_conf), what  # accumulated: doubled


@pytest.mark.parametrize("conn", S.CONNECTIVITIES)
@pytest.mark.parametrize("name", S.PATTERNS)
def test_seg_sieve_equals_the_specification(name, conn):
    from ifseg_amd import hip
    dev = _dev()
    flag = torch.zeros(1, dtype=I32, device=dev)
    for key in S.case_keys((name,)):
        for K in S.MIN_REGIONS:
            for passes in (1, 3):
                for ignore in (None, S.present_value(key)):
                    _run_case(hip, key, conn, K, passes, ignore, 0, dev, flag)
    assert int(flag) == 0                                         # no loop of the region kernels ran out of its budget


@pytest.mark.parametrize("conn", S.CONNECTIVITIES)
def test_seg_sieve_batched(conn):
    """B = 3 where the last row of one image equals the first row of the next: no vote crosses from one image into the next"""
    from ifseg_amd import hip
    dev = _dev()
    flag = torch.zeros(1, dtype=I32, device=dev)
    for key in S.BATCHES:
        for K in S.MIN_REGIONS:
            for passes in (1, 3):
                for ignore in (None, S.present_value(key)):
                    _run_case(hip, key, conn, K, passes, ignore, 0, dev, flag)
    assert int(flag) == 0


@pytest.mark.parametrize("conn", S.CONNECTIVITIES)
def test_seg_sieve_layouts_and_repeats(conn):
    from ifseg_amd import hip
    dev = _dev()
    flag = torch.zeros(1, dtype=I32, device=dev)
    keys = [("speckled", 48, 200, False), ("speckled", 33, 129, True), ("random5", 17, 65, True), ("blocks", 33, 129, False),
            ("checkerboard", 3, 2, False), ("constant", 1, 1, False), ("rings", 1, 65, True), "batch", "batch_short"]
    for i, key in enumerate(keys):
        for K, passes, ignore, raw in ((2, 1, None, False), (9, 3, S.present_value(key), True), (9, 2, None, True),
                                       (10 ** 6, 8, None, False)):
            _run_case(hip, key, conn, K, passes, ignore, OFFSETS[i % 3], dev, flag, raw, layout=True)
    assert int(flag) == 0
    # an ignored value the map's dtype cannot hold ignores nothing; fresh outputs when none are given
    lab = S.labels_of(("speckled", 33, 129, False)).to(dev)
    out, moved = hip.seg_sieve(lab, 9, conn, 2, ignore=-1, n=S.N)
    want = S.reference(("speckled", 33, 129, False), conn, 9, 2, None)
    assert torch.equal(out.cpu(), want[0]) and torch.equal(moved.cpu(), want[1])
    assert torch.equal(hip.seg_sieve(lab, 1, conn)[0], lab)       # K = 1 is the identity


def test_c_entry_refusals_and_limits():
    from ifseg_amd import hip
    dev = _dev()
    L = hip.lib()
    assert hip.seg_sieve_limits() == (16, 64, hip.SEG_SIEVE_MAX_PASSES, hip.SEG_SIEVE_MAX_CLASSES)
    assert L.ifseg_seg_sieve_limit(ctypes.c_int(4)) == BAD_ARG and L.ifseg_seg_sieve_limit(ctypes.c_int(-1)) == BAD_ARG
    B, H, W = 2, 17, 65
    npix = B * H * W
    lab = torch.zeros(npix + 2, dtype=torch.int16, device=dev)
    planes = torch.full((4, npix + 4), -7, dtype=I32, device=dev)
    best = torch.full((npix + 2,), -7, dtype=torch.int64, device=dev)
    maps = torch.full((2, npix + 2), 77, dtype=torch.int16, device=dev)
    conf = torch.full((npix + 2,), 0.5, device=dev)
    moved = torch.zeros(2 * 8 + 2, dtype=torch.int64, device=dev)
    flag = torch.zeros(4, dtype=I32, device=dev)
    p = lambda t, byte=0: ctypes.c_void_p(t.data_ptr() + byte)
    ci = ctypes.c_int

    def sieve(labels=p(lab), lb=2, b=B, h=H, w=W, conn=4, K=2, passes=2, n=8, work=p(planes[0]), count=p(planes[1]),
              root=p(planes[2]), size=p(planes[3]), bst=p(best), tmp=p(maps[0]), out=p(maps[1]), cf=p(conf), mv=p(moved), fl=p(flag)):
        return L.ifseg_seg_sieve(labels, ci(lb), ci(b), ci(h), ci(w), ci(conn), ci(K), ci(passes), ci(0), ci(0), ci(n), ci(0), work,
                                 count, root, size, bst, tmp, out, cf, mv, fl, None)

    for kw in (dict(labels=None), dict(work=None), dict(count=None), dict(root=None), dict(size=None), dict(bst=None), dict(out=None),
               dict(mv=None), dict(fl=None), dict(tmp=None), dict(lb=3), dict(lb=0), dict(labels=p(lab, 1)), dict(out=p(maps[1], 1)),
               dict(tmp=p(maps[0], 1)), dict(work=p(planes[0], 2)), dict(size=p(planes[3], 1)), dict(fl=p(flag, 2)), dict(cf=p(conf, 2)),
               dict(bst=p(best, 4)), dict(mv=p(moved, 4)), dict(conn=0), dict(conn=6), dict(K=0), dict(K=-3), dict(passes=0),
               dict(passes=9), dict(n=0), dict(n=513), dict(root=p(planes[1])), dict(size=p(planes[0], 4)), dict(work=p(lab)),
               dict(out=p(lab)), dict(out=p(lab, 2)), dict(tmp=p(maps[1])), dict(tmp=p(lab)), dict(bst=p(planes[0])),
               dict(cf=p(planes[2])), dict(mv=p(best)), dict(out=p(best)), dict(fl=p(planes[3], 8))):
        assert sieve(**kw) == BAD_ARG, kw
    for kw in (dict(b=0), dict(h=0), dict(w=-1), dict(b=1 << 15, h=1 << 8, w=1 << 8)):
        assert sieve(**kw) == BAD_SHAPE, kw
    torch.cuda.synchronize()
    # nothing was launched on a refusal
    assert bool((planes == -7).all()) and bool((best == -7).all()) and bool((maps == 77).all()) and bool((conf == 0.5).all())
    assert not flag.any() and not moved.any()
    # one pass takes no tmp, and conf is optional
    assert sieve(passes=1, tmp=None, cf=None) == 0
    torch.cuda.synchronize()
    assert bool((maps[1, :npix] == 0).all()) and bool((maps[1, npix:] == 77).all()) and bool((maps[0] == 77).all())
    assert not flag.any() and not moved.any()


# ------------------------------------------------------------------------------------------------- end to end
def test_segmenter_sieve_end_to_end(e2e):  # noqa: F811
    from ifseg_amd.predict import areas_reference, confusion_reference, sieve_reference
    m, raw, ocfg, mk = e2e
    n = ocfg.num_seg_tokens
    plain, seg = mk(), mk(sieve=8)
    assert seg.sieve_moved is None
    base = plain.segment_raw(raw, return_conf=True, return_probs=True)
    res = seg.segment_raw(raw, return_conf=True, return_probs=True)
    some = 0
    total = torch.zeros(2, n, dtype=torch.int64)
    wants = []
    for r, b in zip(res, base):
        want, moved, conf = sieve_reference(b.labels.cpu(), 8, 4, 2, n=n, conf=b.conf.cpu())
        assert r.labels.dtype == b.labels.dtype and torch.equal(r.labels.cpu(), want)
        assert torch.equal(r.conf.cpu(), conf) and torch.equal(r.probs, b.probs)      # conf zeroed where moved, probs as they were
        some += int(moved[0].sum())
        total += moved
        wants.append(want)
    assert some > 0                                               # the sieve found something to move
    assert torch.equal(seg.sieve_moved.cpu(), total)
    # other settings of the constructor reach the launch
    for r, b in zip(mk(sieve=20, sieve_connectivity=8, sieve_passes=1).segment_raw(raw), base):
        assert torch.equal(r.labels.cpu(), sieve_reference(b.labels.cpu(), 20, 8, 1, n=n)[0])

    # evaluate_raw counts the sieved labels
    g = torch.Generator().manual_seed(3)
    gts = [torch.randint(0, n + 1, tuple(w.shape), generator=g).to(torch.uint8) for w in wants]
    score, labels = seg.evaluate_raw(raw, gts, confusion=True, return_labels=True)
    areas = sum(areas_reference(w, gt, n)[0] for w, gt in zip(wants, gts))
    matrix = sum(confusion_reference(w, gt, n) for w, gt in zip(wants, gts))
    assert all(torch.equal(l.cpu(), w) for l, w in zip(labels, wants))
    assert torch.equal(score.areas.cpu(), areas) and torch.equal(score.confusion.cpu(), matrix)
    assert torch.equal(seg.sieve_moved.cpu(), 2 * total)

    # pseudo-labels: a relabelled pixel has conf 0 and is kept by no floor > 0
    for r, w, b in zip(seg.pseudo_label_raw(raw, floor=0.5), wants, base):
        assert torch.equal(r.predicted.cpu(), w)
        changed = w != b.labels.cpu()
        assert bool((r.labels.cpu()[changed] == 255).all()) and bool((r.conf.cpu()[changed] == 0).all())
