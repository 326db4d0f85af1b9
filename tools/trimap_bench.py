"""The exact distance transform and the trimap counters on the device (csrc/distance.hip: hip.seg_distance,
hip.seg_trimap_areas; Segmenter.evaluate_raw(trimap=True)) against what a user does without them: `gt.cpu()`,
`scipy.ndimage.distance_transform_edt` once per present value, then masks and `numpy.bincount` per radius -- the device wait
and the copies included -- per call as enqueued from Python.
  512 x 683 at 15 and 150 classes, 1024 x 2048 at 19 classes, two inputs each:
  piecewise   ground truth in blocks of 64 x 64 pixels, a tenth of the BLOCKS ignored, the labels the same blocks shifted by
              (5, 7): distances up to 32 and beyond, so the row scans run long
  random      independent random labels and ground truth per pixel: every pixel's distance is 1 or so
`hip.seg_distance` at R = 8, 32 and 128 and `hip.seg_trimap_areas` with the default radii (1 .. 32), with `hip.seg_areas` and
`hip.seg_boundary_areas` at d = 32 on the same maps for scale; and `Segmenter.evaluate_raw` on SegOFA-Base with and without
`trimap=True` (--no-model leaves it out).

THE EXPECTATION, written down before the first run: the launches are bound by the halo they stage, so a call should cost
`seg_boundary_areas` at d = 32 times the ratio of the elements staged per 16 x 64 tile.  seg_boundary_areas stages
2 (16 + 2 d) (64 + 2 d) = 20 480 at d = 32; seg_distance stages (16 + 2 R) 64 for its columns and 2 * 16 (64 + 2 R) for its
rows (labels and v): 4 608 at R = 8 (x 0.23), 9 216 at R = 32 (x 0.45), 27 648 at R = 128 (x 1.35).  seg_trimap_areas with the
default radii is that at R = 32 plus one counting walk: x 0.45 of seg_boundary_areas plus one seg_areas.  A figure more than
a quarter above its expectation is marked MISSED; one slower than the host path is marked LOSES.

The device variants of a row alternate window by window in one process; a window is at least 0.5 s of enqueued calls between
two device events after a warm-up; the figure is the median over the windows, [min, max] its run-to-run spread.  The host path
takes seconds per call: it is called once in each of the first three windows, timed by the host's clock behind a device synchronise.  Both sides are
checked to give the same integers before they are timed.

    python tools/trimap_bench.py [--windows 5] [--window-s 0.5] [--no-model] [--out profiles/trimap_bench.txt]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from boundary_bench import MODEL_CLASSES, SIZES, random_maps
from predict_bench import window
from predict_tta_bench import H, P, W

DISTANCES = (8, 32, 128)
EXPECTED = {8: 4608 / 20480, 32: 9216 / 20480, 128: 27648 / 20480}     # of seg_boundary_areas at d = 32
SLACK = 1.25


def piecewise(h, w, n, dev):
    g = torch.Generator().manual_seed(1)
    cells = ((h + 63) // 64 + 1, (w + 63) // 64 + 1)
    blocks = torch.randint(1, n + 1, cells, generator=g)
    drop = torch.rand(cells, generator=g)
    holes = torch.where(drop < 0.05, torch.zeros_like(blocks), torch.where(drop < 0.10, torch.full_like(blocks, 255), blocks))
    up = lambda t: t.repeat_interleave(64, 0).repeat_interleave(64, 1)
    return (up(blocks)[5:h + 5, 7:w + 7] - 1).to(torch.uint8)[None].contiguous().to(dev), up(holes)[:h, :w].to(torch.uint8)[None].contiguous().to(dev)


def host_distance(gt):
    """what a user does today -> float64 [h, w], the Euclidean distance to the nearest pixel of another value"""
    from scipy import ndimage
    g = gt.cpu().numpy()[0]
    out = np.full(g.shape, np.inf)
    for c in np.unique(g):
        m = g == c
        out[m] = ndimage.distance_transform_edt(m)[m]
    return g, out


def host_trimap(labels, gt, n, radii):
    """-> int64 [K, 3, n], raw labels"""
    g, d = host_distance(gt)
    p = labels.cpu().numpy()[0].astype(np.int64)
    g = g.astype(np.int64)
    scored = (g != 0) & (g != 255) & (g <= n)
    cls, known = g - 1, scored & (p < n)
    out, lo = [], 0.0
    for r in radii:
        ring = (d > lo) & (d <= r)
        out.append(np.stack([np.bincount(p[known & (p == cls) & ring], minlength=n), np.bincount(p[known & ring], minlength=n),
                             np.bincount(cls[scored & ring], minlength=n)]))
        lo = float(r)
    return torch.from_numpy(np.stack(out))


def host_us(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e6


def measure(device_fns, host_fn, a):
    """-> [(median, min, max)] microseconds, the device functions first, the host function last"""
    for f in device_fns:
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    us = [[] for _ in range(len(device_fns) + 1)]
    for _ in range(a.windows):
        for i, f in enumerate(device_fns):
            us[i].append(window(f, a.window_s))
        if len(us[-1]) < 3:
            us[-1].append(host_us(host_fn))
    return [(statistics.median(u), min(u), max(u)) for u in us]


def fmt(name, r):
    return "%s %10.1f [%10.1f, %10.1f]" % ((name,) + tuple(r))


def verdict(measured, expected, host):
    return ("expected <= %8.1f: %s" % (expected, "met" if measured <= SLACK * expected else "MISSED")
            + ("" if measured < host else "   LOSES to the host path"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.5)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ifseg_amd import hip
    from ifseg_amd.predict import default_trimap_radii
    dev = torch.device("cuda:0")
    radii = default_trimap_radii()
    lines = ["the distance transform and the trimap counters on the device vs gt.cpu() + scipy's EDT per present value + masks + "
             "numpy.bincount: median [min, max] microseconds over %d alternating windows of >= %.1f s (host: one call in each of the first three windows)"
             % (a.windows, a.window_s),
             "one label map per call; expectation = seg_boundary_areas(d = 32) x the ratio of the halo elements staged (x %.2f, "
             "x %.2f, x %.2f at R = 8, 32, 128), + seg_areas for the counters; MISSED: more than x %.2f above it"
             % (EXPECTED[8], EXPECTED[32], EXPECTED[128], SLACK), ""]

    def emit(text):
        lines.append(text)
        print(text, flush=True)

    for h, w, n in SIZES:
        for name, make in (("piecewise", piecewise), ("random", random_maps)):
            labels, gt = make(h, w, n, dev)
            # the same integers on both sides, before anything is timed
            got, plane = hip.seg_trimap_areas(labels, gt, n, radii)
            assert torch.equal(got.cpu(), host_trimap(labels, gt, n, radii)) and int(got[:, 0].sum()) > 0
            d = host_distance(gt)[1]
            for R in DISTANCES:
                mine = hip.seg_distance(gt, R).cpu().numpy()[0].astype(np.int64)
                want = np.where(d <= R, np.rint(d * d), 65535).astype(np.int64)
                assert np.array_equal(mine, want), (h, w, n, name, R)
            res = measure([lambda: hip.seg_distance(gt, 8), lambda: hip.seg_distance(gt, 32), lambda: hip.seg_distance(gt, 128),
                           lambda: hip.seg_trimap_areas(labels, gt, n, radii), lambda: hip.seg_trimap_areas(labels, gt, n, radii, dist=plane),
                           lambda: hip.seg_areas(labels, gt, n), lambda: hip.seg_boundary_areas(labels, gt, n, 32)],
                          lambda: host_trimap(labels, gt, n, radii), a)
            host_d = measure([], lambda: host_distance(gt), a)[0]
            areas, bands = res[5][0], res[6][0]
            emit("%4d x %4d n %3d %-9s" % (h, w, n, name))
            emit("    " + fmt("(seg_areas)", res[5]) + "   " + fmt("(seg_boundary_areas d 32)", res[6]))
            emit("    " + fmt("host EDT per value", host_d) + "   " + fmt("host EDT + masks + bincount", res[7]))
            for i, R in enumerate(DISTANCES):
                emit("    " + fmt("seg_distance R %3d" % R, res[i]) + "   x%8.1f vs host   " % (host_d[0] / res[i][0])
                     + verdict(res[i][0], EXPECTED[R] * bands, host_d[0]))
            emit("    " + fmt("seg_trimap_areas  ", res[3]) + "   x%8.1f vs host   " % (res[7][0] / res[3][0])
                 + verdict(res[3][0], EXPECTED[32] * bands + areas, res[7][0]))
            emit("    " + fmt("  (dist= given)   ", res[4]))
    if not a.no_model:
        from ifseg_amd.tasks.mm_tasks.segmentation import SegmentationTask
        emit("")
        emit("end to end, SegOFA-Base, one raw uint8 %d x %d image, default radii; x = with / without" % (H, W))
        for n in MODEL_CLASSES:
            torch.manual_seed(0)
            g = torch.Generator().manual_seed(7)
            names = [torch.randint(4, 50000, (int(k),), generator=g) for k in torch.randint(1, 4, (n,), generator=g)]
            task = SegmentationTask(num_seg_tokens=n, patch_image_size=P, arch="segofa_base", category_token_ids=names)
            model = task.build_model().to(dev).eval()
            seg = task.build_segmenter(model)
            img = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).to(dev)
            gt = piecewise(H, W, n, dev)[1][0]
            for name, kw in (("single view", {}), ("ms+flip", dict(scales=(0.5, 0.75, 1.0, 1.25, 1.5, 1.75), flip=True))):
                plain = lambda: seg.evaluate_raw(img, gt, **kw)
                with_rings = lambda: seg.evaluate_raw(img, gt, trimap=True, **kw)
                score, labels = seg.evaluate_raw(img, gt, trimap=True, return_labels=True, **kw)
                assert torch.equal(score.trimap.cpu(), host_trimap(labels[0][None], gt[None], n, radii))
                assert torch.equal(score.areas, plain().areas)
                for f in (plain, with_rings):
                    for _ in range(3):
                        f()
                us = [[], []]
                for _ in range(a.windows):
                    for i, f in enumerate((plain, with_rings)):
                        us[i].append(window(f, a.window_s))
                res = [(statistics.median(u), min(u), max(u)) for u in us]
                emit("  n %3d %-12s " % (n, name) + fmt("evaluate_raw", res[0]) + "   " + fmt("trimap=True", res[1])
                     + "   x%5.3f" % (res[1][0] / res[0][0]))
            del model, seg
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
