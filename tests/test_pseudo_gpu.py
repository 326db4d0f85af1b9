"""GPU: hip.seg_conf_hist and hip.seg_pseudo (csrc/pseudo.hip) against their CPU specifications
(`confidence_histogram_reference`, `pseudo_label_reference`), at every byte alignment between canaries, batched, through the
dispatcher, `Segmenter.pseudo_label_raw` end to end on the segofa_tiny fixture and `task.self_train_sample` through one
training step.  Everything is integer: every comparison is `torch.equal`."""
import ctypes

import pytest
import torch

import _predict_cases as PC
from test_predict_views_gpu import e2e  # noqa: F401  (the segofa_tiny fixture with its three raw shapes)
from test_render_gpu import make_labels  # class edges on both tile seams, single-pixel regions, labels outside [0, n)

pytestmark = pytest.mark.gpu

HS, WS, RS = (1, 3, 15, 16, 17, 33), (1, 2, 3, 4, 63, 64, 65, 66, 129), (0, 1, 4)
BAD_SHAPE, BAD_ARG = -2, -3
SPECIAL = [0.0, 1.0, float("nan"), float("inf"), float("-inf"), 1.7, -0.3, 255 / 256, 0.49999997, 0.5, 0.50000006]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ifseg_amd.ops  # noqa: F401
    return torch.device("cuda:0")


def make_conf(shape, seed):
    """uniform in [0, 1) with the special values up front (as many as fit)"""
    conf = torch.rand(shape, generator=torch.Generator().manual_seed(seed))
    flat = conf.reshape(-1)
    flat[:min(len(SPECIAL), flat.numel())] = torch.tensor(SPECIAL)[:flat.numel()]
    return conf


def make_thresholds(n, seed):
    thr = torch.randint(0, 257, (n,), generator=torch.Generator().manual_seed(seed), dtype=torch.int32)
    if n == 1:
        thr[0] = (0, 256, 100)[seed % 3]
    if n > 2:
        thr[seed % n], thr[(seed + 1) % n], thr[(seed + 2) % n] = 0, 256, 128
    return thr


# ------------------------------------------------------------------------------------------------- the histogram
def flat_labels(npix, n, dtype, seed, random):
    """a flat label map: runs of 512 pixels of one class (a scan of a piecewise-constant map) or a class per pixel, with labels
    outside [0, n) sprinkled in"""
    g = torch.Generator().manual_seed(seed)
    if random:
        lab = torch.randint(0, n, (npix,), generator=g)
    else:
        lab = torch.randint(0, n, (npix // 512 + 1,), generator=g).repeat_interleave(512)[:npix].clone()
    outside = [255] if dtype == torch.uint8 else [-1, n, 511, -32768, 32767]
    if npix > 16:
        where = torch.randint(0, npix, (9,), generator=g)
        lab[where] = torch.tensor(outside)[torch.arange(9) % len(outside)]
    return lab.to(dtype)


HIST_CASES = [(15, torch.uint8), (64, torch.uint8), (65, torch.uint8), (150, torch.uint8), (300, torch.int16)]


@pytest.mark.parametrize("n,dtype", HIST_CASES, ids=["n15_direct", "n64_direct", "n65_hashed", "n150_hashed", "n300_i16_hashed"])
def test_histogram_is_the_specification(n, dtype):
    """piecewise-constant labels with random conf at every pixel count (one pixel, below and at one group, one workgroup step
    and one pixel more, several workgroups), at element offsets that put a head in front of the labels' first 16-byte boundary
    and the confidences off theirs; a second launch into the same counters doubles them"""
    from ifseg_amd import hip
    from ifseg_amd.predict import confidence_histogram_reference
    dev = _dev()
    assert (n <= hip.SEG_CONF_HIST_DIRECT_CLASSES) == (n <= 64)
    keys, same = [], []
    for npix in (1, 15, 255, 4096, 4097, 70001):
        labels, conf = flat_labels(npix, n, dtype, npix, False), make_conf((npix,), npix + 1)
        want_h, want_t = confidence_histogram_reference(labels, conf, n)
        assert int(want_h.sum()) == int(want_t[0]) and int(want_t.sum()) == npix
        want_h, want_t = want_h.to(dev), want_t.to(dev)
        labbuf, confbuf = torch.zeros(npix + 16, dtype=dtype, device=dev), torch.zeros(npix + 16, device=dev)
        for lo, co in ((0, 0), (3, 1), (5, 2), (15, 3)):
            ld, cd = labbuf[lo:lo + npix].copy_(labels), confbuf[co:co + npix].copy_(conf)
            hist, tally = hip.seg_conf_hist(ld, cd, n)
            assert hist.dtype == torch.int64 and hist.shape == (n, 256) and tally.shape == (2,)
            first = (hist == want_h).all() & (tally == want_t).all()
            again = hip.seg_conf_hist(ld, cd, n, hist=hist, tally=tally)
            assert again[0] is hist and again[1] is tally
            keys.append((npix, lo, co))
            same.append(torch.stack([first, (hist == 2 * want_h).all() & (tally == 2 * want_t).all(), hist.sum() == tally[0]]))
    same = torch.stack(same).cpu().tolist()                       # the one synchronisation
    wrong = [(k, ok) for k, ok in zip(keys, same) if not all(ok)]  # (first launch, accumulated, sum == tally[0])
    assert len(keys) == 24 and not wrong, wrong[:10]


@pytest.mark.parametrize("n,dtype,random", [(15, torch.uint8, False), (150, torch.uint8, False), (150, torch.uint8, True),
                                            (300, torch.int16, True)], ids=["n15", "n150", "n150_random", "n300_i16_random"])
def test_histogram_of_a_large_map(n, dtype, random):
    """1100 x 2000 pixels: more than 512 workgroups' worth of steps, so the grid-stride loop runs; with a class per pixel a
    workgroup meets some 7000 of the 38 400 (n = 150) possible pairs against 4096 slots: the global-memory path"""
    from ifseg_amd import hip
    from ifseg_amd.predict import confidence_histogram_reference
    dev = _dev()
    H, W = 1100, 2000
    assert H * W > 512 * 4096
    labels, conf = flat_labels(H * W, n, dtype, 7, random).reshape(H, W), make_conf((H, W), 8)
    want_h, want_t = confidence_histogram_reference(labels, conf, n)
    if random and n == 150:
        assert int((want_h > 0).sum()) > 8 * hip.SEG_CONF_HIST_SLOTS
    hist, tally = hip.seg_conf_hist(labels.to(dev), conf.to(dev), n)
    assert torch.equal(hist.cpu(), want_h) and torch.equal(tally.cpu(), want_t) and int(hist.sum()) == int(tally[0])


def test_histogram_entry_point_refusals():
    from ifseg_amd import hip
    dev = _dev()
    lib = hip.lib()
    i, ll, vp = ctypes.c_int, ctypes.c_longlong, ctypes.c_void_p
    p = lambda t, off=0: vp(t.data_ptr() + off)
    lab, conf = torch.zeros(64, dtype=torch.int16, device=dev), torch.zeros(64, device=dev)
    hist, tally = torch.zeros(512 * 256 + 1, dtype=torch.int64, device=dev), torch.zeros(3, dtype=torch.int64, device=dev)

    def call(labels=p(lab), lb=2, cf=p(conf), npix=16, n=5, h=p(hist), t=p(tally)):
        return lib.ifseg_seg_conf_hist(labels, i(lb), cf, ll(npix), i(n), h, t, None)

    for bad in (dict(labels=vp(None)), dict(cf=vp(None)), dict(h=vp(None)), dict(t=vp(None)), dict(lb=0), dict(lb=4),
                dict(labels=p(lab, 1)), dict(cf=p(conf, 2)), dict(h=p(hist, 4)), dict(t=p(tally, 4)), dict(n=0), dict(n=513)):
        assert call(**bad) == BAD_ARG, bad
    for bad in (dict(npix=0), dict(npix=-1), dict(npix=2 ** 31)):
        assert call(**bad) == BAD_SHAPE, bad
    torch.cuda.synchronize()
    assert not hist.any() and not tally.any()                     # no launch so far
    assert call(n=512, lb=1, labels=p(lab, 1), cf=p(conf, 4), h=p(hist, 8), t=p(tally, 8)) == 0
    torch.cuda.synchronize()
    assert int(hist[1]) == 16 and int(hist.sum()) == 16 and tally.tolist() == [0, 16, 0]      # 16 pixels of class 0, conf 0


# ------------------------------------------------------------------------------------------------- the filter
FILTER_CASES = [(1, torch.uint8), (15, torch.uint8), (150, torch.uint8), (254, torch.uint8), (15, torch.int16), (254, torch.int16)]


@pytest.mark.parametrize("n,dtype", FILTER_CASES, ids=["n1", "n15", "n150", "n254", "n15_i16", "n254_i16"])
def test_filter_is_the_specification(n, dtype):
    from ifseg_amd import hip
    from ifseg_amd.predict import pseudo_label_reference
    dev = _dev()
    keys, same = [], []
    for H in HS:
        for W in WS:
            labels, conf = make_labels(H, W, n, dtype, H * 131 + W), make_conf((H, W), H)
            thr = make_thresholds(n, H + W)
            ld, cd, td = labels.to(dev), conf.to(dev), thr.to(dev)
            for r in RS:
                for raw in (True, False):
                    want, wkept = pseudo_label_reference(labels, conf, thr, n, r, raw)
                    got, kept = hip.seg_pseudo(ld, cd, td, n, r, raw)
                    assert got.dtype == torch.uint8 and got.shape == (H, W) and kept.dtype == torch.int64 and kept.shape == (2, n)
                    keys.append((H, W, r, raw))
                    same.append((got == want.to(dev)).all() & (kept == wkept.to(dev)).all())
    same = torch.stack(same).cpu().tolist()                       # the one synchronisation
    wrong = [k for k, ok in zip(keys, same) if not ok]
    assert len(keys) == len(HS) * len(WS) * len(RS) * 2 and not wrong, wrong[:10]


def test_filter_band_crosses_the_tile_seams_and_thresholds_bite():
    """what the inputs above are built to do, checked on the reference so that the comparison is not vacuous"""
    from ifseg_amd import hip
    from ifseg_amd.predict import pseudo_label_reference
    dev = _dev()
    n = 15
    labels, conf = make_labels(33, 129, n, torch.uint8, 5), make_conf((33, 129), 6)
    zero = torch.zeros(n, dtype=torch.int32)
    for r in (1, 4):
        out, _ = pseudo_label_reference(labels, conf, zero, n, r)
        for y, x in ((15, 63), (16, 64), (15, 64), (16, 63)):     # band pixels on each side of both seams
            assert int(out[y, x]) == 255, (r, y, x)
        got, _ = hip.seg_pseudo(labels.to(dev), conf.to(dev), zero.to(dev), n, r)
        assert torch.equal(got.cpu(), out) and 0 < int((out == 255).sum()) < out.numel()
    # thresholds 0 and 256: all of a class, none of it
    c = int(labels[4, 16])                                        # the class of a block's interior
    assert c < n
    thr = zero.clone()
    thr[c] = 256
    got, kept = hip.seg_pseudo(labels.to(dev), conf.to(dev), thr.to(dev), n, 0, False)
    inside = labels < n
    assert torch.equal(got.cpu() != 255, inside & (labels != c)) and int(kept[0, c]) == 0 and int(kept[1, c]) == int((labels == c).sum()) > 0
    assert torch.equal(got.cpu()[inside & (labels != c)], labels[inside & (labels != c)])
    # a 3 x 2 image under r = 4: every window is the whole image
    small = torch.tensor([[0, 0], [0, 1], [0, 0]], dtype=torch.uint8)
    got, kept = hip.seg_pseudo(small.to(dev), torch.ones(3, 2, device=dev), torch.zeros(2, dtype=torch.int32, device=dev), 2, 4)
    assert got.eq(255).all() and kept.tolist() == [[0, 0], [5, 1]]


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16], ids=["u8", "i16"])
def test_filter_at_every_alignment_between_canaries(dtype):
    """output, labels and conf as views into larger flat buffers: the output at every byte offset 0 .. 3 (rows of W bytes, odd W),
    labels and conf at element offsets; 64 canary bytes in front of and behind the output; `kept` accumulates over a second
    launch, which writes the same bytes"""
    from ifseg_amd import hip
    from ifseg_amd.predict import pseudo_label_reference
    dev = _dev()
    n = 15
    keys, same = [], []
    for H, W in ((5, 65), (17, 130), (3, 3)):
        labels, conf, thr = make_labels(H, W, n, dtype, 3), make_conf((H, W), 5), make_thresholds(n, 4)
        want, wkept = (t.to(dev) for t in pseudo_label_reference(labels, conf, thr, n, 1, True))
        td = thr.to(dev)
        labbuf, confbuf = torch.zeros(H * W + 4, dtype=dtype, device=dev), torch.zeros(H * W + 4, device=dev)
        outbuf = torch.empty(64 + 4 + H * W + 64, dtype=torch.uint8, device=dev)
        assert outbuf.data_ptr() % 4 == 0 and labbuf.data_ptr() % 4 == 0
        for lo in range(4 if dtype == torch.uint8 else 2):
            ld = labbuf[lo:lo + H * W].view(H, W).copy_(labels)
            cd = confbuf[lo % 2:lo % 2 + H * W].view(H, W).copy_(conf)
            for oo in range(4):
                outbuf.fill_(0xA5)
                out = outbuf[64 + oo:64 + oo + H * W].view(H, W)
                assert out.data_ptr() % 4 == oo
                got, kept = hip.seg_pseudo(ld, cd, td, n, 1, True, out=out)
                assert got is out
                first = outbuf.clone()
                hip.seg_pseudo(ld, cd, td, n, 1, True, kept=kept, out=out)
                keys.append((H, W, lo, oo))
                same.append(torch.stack([(out == want).all(), (outbuf[:64 + oo] == 0xA5).all(), (outbuf[64 + oo + H * W:] == 0xA5).all(),
                                         (outbuf == first).all(), (kept == 2 * wkept).all()]))
    same = torch.stack(same).cpu().tolist()
    wrong = [(k, ok) for k, ok in zip(keys, same) if not all(ok)]  # (map, canary in front, canary behind, relaunch, kept twice)
    assert len(keys) == 3 * 4 * (4 if dtype == torch.uint8 else 2) and not wrong, wrong[:10]


def test_filter_batch_is_three_single_launches():
    from ifseg_amd import hip
    from ifseg_amd.predict import pseudo_label_reference
    dev = _dev()
    B, H, W, n = 3, 17, 65, 150
    labels, conf, thr = make_labels(H, W, n, torch.uint8, 8, B=B), make_conf((B, H, W), 10), make_thresholds(n, 2)
    ld, cd, td = labels.to(dev), conf.to(dev), thr.to(dev)
    got, kept = hip.seg_pseudo(ld, cd, td, n, 1)
    total = torch.zeros(2, n, dtype=torch.int64, device=dev)
    for b in range(B):
        one, _ = hip.seg_pseudo(ld[b], cd[b], td, n, 1, kept=total)
        assert torch.equal(got[b], one), b
    want, wkept = pseudo_label_reference(labels, conf, thr, n, 1)
    assert torch.equal(got.cpu(), want) and torch.equal(kept.cpu(), wkept) and torch.equal(total, kept)


def test_filter_entry_point_refusals():
    from ifseg_amd import hip
    dev = _dev()
    lib = hip.lib()
    i, vp = ctypes.c_int, ctypes.c_void_p
    p = lambda t, off=0: vp(t.data_ptr() + off)
    lab, conf = torch.zeros(64, dtype=torch.int16, device=dev), torch.ones(64, device=dev)
    thr, kept = torch.zeros(256, dtype=torch.int32, device=dev), torch.zeros(2 * 255 + 1, dtype=torch.int64, device=dev)
    out = torch.full((16 + 8,), 77, dtype=torch.uint8, device=dev)

    def call(labels=p(lab), lb=2, cf=p(conf), t=p(thr), n=5, B=1, H=4, W=4, r=1, raw=1, o=p(out, 3), k=p(kept)):
        return lib.ifseg_seg_pseudo(labels, i(lb), cf, t, i(n), i(B), i(H), i(W), i(r), i(raw), o, k, None)

    for bad in (dict(labels=vp(None)), dict(cf=vp(None)), dict(t=vp(None)), dict(o=vp(None)), dict(k=vp(None)), dict(lb=0), dict(lb=3),
                dict(labels=p(lab, 1)), dict(cf=p(conf, 2)), dict(t=p(thr, 2)), dict(k=p(kept, 4)), dict(n=0), dict(n=255),
                dict(n=256, raw=0), dict(r=-1), dict(r=5)):
        assert call(**bad) == BAD_ARG, bad
    for bad in (dict(B=0), dict(H=0), dict(W=-1), dict(H=2 ** 16, W=2 ** 15), dict(B=2 ** 11, H=2 ** 10, W=2 ** 10)):
        assert call(**bad) == BAD_SHAPE, bad
    torch.cuda.synchronize()
    assert out.eq(77).all() and not kept.any()                    # no launch so far
    # the limits themselves pass: n = 255 without raw labels, r = 4, byte labels at an odd address, every pointer offset
    assert call(n=255, raw=0, r=4, lb=1, labels=p(lab, 1), cf=p(conf, 4), t=p(thr, 4), k=p(kept, 8)) == 0
    torch.cuda.synchronize()
    assert out[:3].eq(77).all() and out[3 + 16:].eq(77).all() and not out[3:3 + 16].any()      # class 0 everywhere, kept as 0
    assert int(kept[1]) == 16 and int(kept[1 + 255]) == 16 and int(kept.sum()) == 32


# ------------------------------------------------------------------------------------------------- the shared parts
@pytest.mark.parametrize("n,dtype", [(15, torch.uint8), (150, torch.uint8), (150, torch.int16)], ids=["n15_direct", "n150_hashed", "n150_i16_hashed"])
def test_four_counters_agree_on_one_input(n, dtype):
    """one label map through everything csrc/count.h and tile.h's halo section hold: the walk with an integer second stream
    (seg_areas, seg_confusion), with a float one (seg_conf_hist), both table regimes (n = 15 direct, n = 150 hashed for the
    histogram and the matrix alike) and the halo kernel's counters (seg_pseudo).  With every pixel scored and every threshold
    0, each of the four counts the pixels per predicted label: torch.bincount of the labels in [0, n).  The labels start 5
    elements behind a 16-byte boundary and 3 x 37 x 91 = 10 101 pixels leave a tail"""
    from ifseg_amd import hip
    from ifseg_amd.predict import areas_reference, confidence_histogram_reference, confusion_reference, pseudo_label_reference
    dev = _dev()
    B, H, W = 3, 37, 91
    g = torch.Generator().manual_seed(n)
    labels = torch.randint(0, n, (B, (H + 7) // 8, (W + 31) // 32), generator=g).repeat_interleave(8, 1).repeat_interleave(32, 2)
    labels = labels[:, :H, :W].clone()
    outside = [255] if dtype == torch.uint8 else [-1, n, 32767]
    for k, (b, y, x) in enumerate(((0, 0, 0), (0, 0, 7), (1, 16, 63), (1, 16, 64), (2, 36, 90), (2, 20, 45))):
        labels[b, y, x] = outside[k % len(outside)]
    labels = labels.to(dtype)
    conf, thr = make_conf((B, H, W), n + 1), torch.zeros(n, dtype=torch.int32)
    gt = torch.randint(1, n + 1, (B, H, W), generator=g).to(dtype)           # raw values: class + 1, none ignored
    inside = (labels.long() >= 0) & (labels.long() < n)
    want, n_out = torch.bincount(labels.long()[inside], minlength=n), int((~inside).sum())
    assert n_out == 6 and int(want.sum()) == B * H * W - 6 and int((want > 0).sum()) > 1
    # the specifications agree by construction
    ref_h, ref_t = confidence_histogram_reference(labels, conf, n)
    ref_c = confusion_reference(labels, gt, n)
    assert torch.equal(ref_h.sum(1), want) and int(ref_t[1]) == n_out
    assert torch.equal(pseudo_label_reference(labels, conf, thr, n, 1)[1][1], want)
    assert torch.equal(areas_reference(labels, gt, n)[0][1], want)
    assert torch.equal(ref_c[:, :n].sum(0), want) and int(ref_c[:, n].sum()) == n_out

    buf = torch.zeros(5 + B * H * W + 16, dtype=dtype, device=dev)
    ld = buf[5:5 + B * H * W].view(B, H, W).copy_(labels)
    assert buf.data_ptr() % 16 == 0 and ld.data_ptr() % 16 == 5 * ld.element_size()      # a head, and with it a tail
    cd, gd, td, want = conf.to(dev), gt.to(dev), thr.to(dev), want.to(dev)
    hist, tally = hip.seg_conf_hist(ld, cd, n)
    kept = hip.seg_pseudo(ld, cd, td, n, boundary=1)[1]
    areas = hip.seg_areas(ld, gd, n)[0]
    confusion = hip.seg_confusion(ld, gd, n)
    same = torch.stack([(hist.sum(1) == want).all(), (kept[1] == want).all(), (areas[1] == want).all(),
                        (confusion[:, :n].sum(0) == want).all(), tally[1] == n_out, confusion[:, n].sum() == n_out])
    assert same.cpu().tolist() == [True] * 6       # (histogram, filter, areas, confusion, outside: histogram, confusion)


# ------------------------------------------------------------------------------------------------- the dispatcher
def test_ops_match_the_bindings():
    from ifseg_amd import hip
    dev = _dev()
    H, W, n = 17, 66, 150
    labels, conf = make_labels(H, W, n, torch.int16, 1, B=2).to(dev), make_conf((2, H, W), 3).to(dev)
    thr = make_thresholds(n, 5).to(dev)
    hist_op, pseudo_op = torch.ops.ifseg.seg_conf_hist, torch.ops.ifseg.seg_pseudo
    want_h, want_t = hip.seg_conf_hist(labels, conf, n)
    got_h, got_t = hist_op(labels, conf, n)
    assert torch.equal(got_h, want_h) and torch.equal(got_t, want_t) and int(got_h.sum()) > 0
    want, wkept = hip.seg_pseudo(labels, conf, thr, n, 1, True)
    got, kept = pseudo_op(labels, conf, thr, n, 1, True)
    assert torch.equal(got, want) and torch.equal(kept, wkept) and got.data_ptr() != want.data_ptr()
    one = pseudo_op(labels[0].to(torch.uint8), conf[0], thr, n, 0, False)
    ref = hip.seg_pseudo(labels[0].to(torch.uint8), conf[0], thr, n, 0, False)
    assert torch.equal(one[0], ref[0]) and torch.equal(one[1], ref[1])
    # non-contiguous inputs are copied
    t = pseudo_op(labels.transpose(1, 2), conf.transpose(1, 2), thr, n, 1, True)
    assert torch.equal(t[0], want.transpose(1, 2)) and torch.equal(t[1], wkept)
    assert torch.equal(hist_op(labels.transpose(1, 2), conf.transpose(1, 2), n)[0], want_h)
    utils = ("test_schema", "test_autograd_registration", "test_faketensor")
    torch.library.opcheck(hist_op, (labels, conf, n), test_utils=utils)
    torch.library.opcheck(pseudo_op, (labels, conf, thr, n, 1, True), test_utils=utils)
    torch.library.opcheck(pseudo_op, (labels[0].to(torch.uint8), conf[0], thr, n, 0, False), test_utils=utils)
    # on a side stream the ops follow PyTorch's current stream
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        side_h, side = hist_op(labels, conf, n)[0], pseudo_op(labels, conf, thr, n, 1, True)[0]
    st.synchronize()
    assert torch.equal(side_h, want_h) and torch.equal(side, want)
    for bad in (lambda: hist_op(labels.long(), conf, n), lambda: hist_op(labels, conf, 513), lambda: pseudo_op(labels, conf, thr, n, 5, True),
                lambda: pseudo_op(labels, conf, thr[:-1], n, 1, True), lambda: pseudo_op(labels, conf, thr.long(), n, 1, True)):
        with pytest.raises(ValueError, match="ifseg::seg_"):
            bad()


# ------------------------------------------------------------------------------------------------- end to end
def _check_results(res, raw, n, hist, thr, boundary, raw_labels=True):
    """one call's results against the specification on its own predicted labels and conf -> the histogram of its images"""
    from ifseg_amd.predict import PseudoLabelResult, confidence_histogram_reference, pseudo_label_reference
    assert len(res) == len(raw) and all(isinstance(r, PseudoLabelResult) for r in res)
    total_h, total_t = torch.zeros(n, 256, dtype=torch.int64), torch.zeros(2, dtype=torch.int64)
    for r, photo in zip(res, raw):
        assert r.labels.is_cuda and r.labels.dtype == torch.uint8 and r.labels.shape == photo.shape[:2] == r.predicted.shape == r.conf.shape
        h, t = confidence_histogram_reference(r.predicted.cpu(), r.conf.cpu(), n)
        total_h += h
        total_t += t
        want, wkept = pseudo_label_reference(r.predicted.cpu(), r.conf.cpu(), thr.cpu(), n, boundary, raw_labels)
        assert torch.equal(r.labels.cpu(), want) and torch.equal(r.kept.cpu(), wkept)
    return total_h, total_t


@pytest.mark.parametrize("call", [{}, {"scales": (0.5, 1.0), "flip": True}], ids=["single", "ms_flip"])
def test_pseudo_label_raw_end_to_end(e2e, call):  # noqa: F811
    from ifseg_amd.predict import ConfidenceHistogram, pseudo_thresholds
    m, raw, ocfg, mk = e2e
    n = ocfg.num_seg_tokens
    seg = mk()
    before = seg.segment_raw(raw, return_conf=True, **call)
    for kw in (dict(keep=0.5, boundary=1), dict(keep=1.0, floor=0.5)):
        hist = ConfidenceHistogram(n, "cuda:0")
        res = seg.pseudo_label_raw(raw, hist=hist, **kw, **call)
        for r, b in zip(res, before):
            assert torch.equal(r.predicted, b.labels) and torch.equal(r.conf, b.conf)
            assert float(r.conf.min()) >= 0.0 and float(r.conf.max()) <= 1.0 + 1e-6   # a probability
        thr = hist.thresholds(kw["keep"], kw.get("floor", 0.0))
        assert torch.equal(thr.cpu(), pseudo_thresholds(hist.hist.cpu(), kw["keep"], kw.get("floor", 0.0)))
        total_h, total_t = _check_results(res, raw, n, hist, thr, kw.get("boundary", 0))
        assert torch.equal(hist.hist.cpu(), total_h) and torch.equal(hist.tally.cpu(), total_t)
        assert int(total_t[0]) == sum(p.shape[0] * p.shape[1] for p in raw) and int(total_t[1]) == 0
        kept = sum(int(r.kept[0].sum()) for r in res)
        if "floor" in kw:                                                             # the fixed threshold is the comparison itself
            assert all(torch.equal(r.labels != 255, r.conf >= 0.5) for r in res)
        else:                                                                         # the filter filtered, and not everything
            assert 0 < kept < int(total_t[0])
        assert hist.summary()["pixels"] == int(total_t[0])
    # a second call into the same histogram: the thresholds are those of both sets
    more = seg.pseudo_label_raw(raw[:2], hist=hist, keep=0.5, **call)
    two_h, _ = _check_results(more, raw[:2], n, hist, hist.thresholds(0.5), 0)
    assert torch.equal(hist.hist.cpu(), total_h + two_h)
    # given thresholds: no histogram is touched, and the class ids come out unshifted without raw_labels
    snapshot = hist.hist.clone()
    thr = hist.thresholds(0.25)
    given = seg.pseudo_label_raw(raw, thresholds=thr, hist=hist, boundary=2, raw_labels=False, **call)
    _check_results(given, raw, n, hist, thr, 2, raw_labels=False)
    assert torch.equal(hist.hist, snapshot)


def test_pseudo_label_raw_refusals_and_task(e2e):  # noqa: F811
    from ifseg_amd.tasks.mm_tasks.segmentation import SegmentationTask
    m, raw, ocfg, mk = e2e
    n = ocfg.num_seg_tokens
    with pytest.raises(ValueError, match="upsample='logits'"):
        mk(upsample="logits").pseudo_label_raw(raw)
    task = SegmentationTask(num_seg_tokens=n, patch_image_size=ocfg.patch_image_size, category_token_ids=PC.E2E_NAMES)
    ts = task.pseudo_label_raw(m, raw, prompt_ids=PC.E2E_PROMPT, keep=0.5, boundary=1)
    mine = mk().pseudo_label_raw(raw, keep=0.5, boundary=1)
    assert all(torch.equal(a.labels, b.labels) and torch.equal(a.kept, b.kept) for a, b in zip(ts, mine))


def test_self_train_sample_through_one_training_step(e2e):  # noqa: F811
    """segofa_tiny at P = 128: `task.self_train_sample` on the three raw photographs is `train_sample` on the pseudo-labels of the
    same weights, one `Trainer.train_step` on it gives a finite loss, and with keep = 0 every target pixel is the ignore class"""
    from ifseg_amd.criterions import SegCriterion
    from ifseg_amd.models.segofa import SegOFAModel, make_config
    from ifseg_amd.tasks.mm_tasks import SegmentationTask
    from ifseg_amd.trainer import Trainer
    dev = _dev()
    _, raw, ocfg, _ = e2e
    _, sd, _, src = PC.e2e_fixture()
    P, n = ocfg.patch_image_size, ocfg.num_seg_tokens
    task = SegmentationTask(num_seg_tokens=n, patch_image_size=P, n_base_vocab=ocfg.vocab_size - 1, category_token_ids=PC.E2E_NAMES)
    task.prompt_ids = PC.E2E_PROMPT
    tf = task.build_train_transform(dev, seed=6, ratio_range=(1, 1))
    m = SegOFAModel(make_config("segofa_tiny", embed_dim=ocfg.embed_dim, ffn_dim=ocfg.ffn_dim, heads=ocfg.heads,
                                enc_layers=ocfg.enc_layers, dec_layers=ocfg.dec_layers, resnet_layers=ocfg.resnet_layers,
                                num_seg_tokens=n, vocab_size=ocfg.vocab_size, patch_image_size=P,
                                orig_patch_image_size=ocfg.orig_patch_image_size))
    torch.nn.Module.load_state_dict(m, sd, strict=False)
    m.cfg.dropout = m.cfg.encoder_drop_path_rate = m.cfg.decoder_drop_path_rate = 0.0
    m.to(dev)
    kw = dict(prompt_ids=PC.E2E_PROMPT, keep=0.5, boundary=1)
    s = task.self_train_sample(m, raw, 4, **kw)
    pseudo = task.pseudo_label_raw(m, raw, **kw)
    ref = task.train_sample(raw, [r.labels for r in pseudo], 4)
    assert s["target"].is_cuda and tuple(s["target"].shape) == (3, P * P + 1)
    assert torch.equal(s["target"], ref["target"]) and torch.equal(s["net_input"]["patch_images"], ref["net_input"]["patch_images"])
    assert torch.equal(s["net_input"]["src_tokens"][0].cpu(), src)
    body = s["target"][:, :-1] - task.seg_id_offset
    assert int(body.min()) >= 0 and int(body.max()) == n and bool((body < n).any())      # kept classes and the ignore class
    none = task.self_train_sample(m, raw, 4, prompt_ids=PC.E2E_PROMPT, keep=0.0)
    assert bool((none["target"][:, :-1] == task.seg_id_offset + n).all())
    with pytest.raises(ValueError, match="raw_labels"):
        task.self_train_sample(m, raw, 4, prompt_ids=PC.E2E_PROMPT, raw_labels=not tf.raw_labels)
    tr = Trainer(m, SegCriterion(task, unsupervised_segmentation=False, init_seg_with_text=False), task, device=dev)
    loss = float(tr.train_step([s])[0]["loss"])
    tr.check_overflow(wait=True)
    torch.cuda.synchronize()
    assert loss == loss and abs(loss) != float("inf") and loss > 0.0
