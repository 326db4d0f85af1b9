"""The region table on the device (csrc/regiontab.hip: hip.seg_region_table; Segmenter.regions_raw) against what a user does
without it, per call as enqueued from Python.  One 512 x 683 uint8 map with a conf plane at connectivity 4 and 8:
  piecewise      classes in blocks of 32 x 32 pixels with 2 % of the pixels flipped to another class: what a segmenter gives
  random         an independent class per pixel, over 5 values: as many tile-local regions as a map can hold
  checkerboard   H W single-pixel regions at connectivity 4, two regions at 8
and per map
  table        hip.seg_region_table(labels, conf, max_regions=R), R = 2^14 (the piecewise map's regions fit) or 2^19 (every
               region of the other two fits)
  seg_regions  hip.seg_regions alone: the floor, the table's first launches
  torch        the device-only composition the table replaces: seg_regions, torch.unique(return_inverse=True) on the roots
               and seven scatter_reduce (four box corners, three sums) over the pixels; its unique synchronises with the host
  cpu+scipy    labels.cpu(), scipy.ndimage.label per present class, find_objects and three sum_labels, the boxes copied back
               (left out when scipy is not installed)
and `Segmenter.regions_raw` against `segment_raw(return_conf=True)` on SegOFA-Base, per image (--no-model leaves it out).
The variants of a row alternate window by window in one process; a window is at least 0.5 s of enqueued calls between two
device events after a warm-up; the figure is the median over the windows, [min, max] its run-to-run spread: a difference inside
the spread is no difference.  The table is checked against the specification, and the torch composition against the table,
before anything is timed.

    python tools/region_table_bench.py [--windows 5] [--window-s 0.5] [--no-model] [--out profiles/region_table_bench.txt]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from evaluate_bench import row
from predict_tta_bench import H, P, W
from regions_bench import maps as region_maps


def maps():
    piece, rnd, _ = region_maps()
    y = torch.arange(H).reshape(H, 1).expand(H, W)
    x = torch.arange(W).reshape(1, W).expand(H, W)
    return piece, rnd, ("checkerboard", ((y + x) % 2).to(torch.uint8))


def torch_table(hip, labels, conf, conn):
    """the composition: -> (roots, boxes int64 [k, 4], sums int64 [k, 3]) in ascending order of root"""
    from ifseg_amd.predict import conf_q16
    root, _ = hip.seg_regions(labels, conn)
    roots, inv = torch.unique(root.reshape(-1), return_inverse=True)
    k = roots.numel()
    pix = torch.arange(H * W, device=labels.device)
    x, y, q = pix % W, pix // W, conf_q16(conf).reshape(-1)
    big = torch.full((k,), 2 ** 31 - 1, dtype=torch.int64, device=labels.device)
    low = torch.full((k,), -1, dtype=torch.int64, device=labels.device)
    zero = torch.zeros(k, dtype=torch.int64, device=labels.device)
    boxes = torch.stack([big.scatter_reduce(0, inv, x, "amin"), big.scatter_reduce(0, inv, y, "amin"),
                         low.scatter_reduce(0, inv, x, "amax"), low.scatter_reduce(0, inv, y, "amax")], 1)
    sums = torch.stack([zero.scatter_reduce(0, inv, v, "sum") for v in (x, y, q)], 1)
    return roots, boxes, sums


def scipy_table(labels, conf, conn):
    """what a user does today -> the boxes, back on the device"""
    import numpy as np
    from scipy import ndimage
    a, c = labels.cpu().numpy(), conf.cpu().numpy()
    structure = np.ones((3, 3), dtype=int) if conn == 8 else None
    ys, xs = np.mgrid[0:H, 0:W]
    boxes = []
    for v in np.unique(a):
        comp, k = ndimage.label(a == v, structure=structure)
        idx = np.arange(1, k + 1)
        sx, sy, sc = (ndimage.sum_labels(p, comp, idx) for p in (xs, ys, c))
        boxes += [(s[1].start, s[0].start, s[1].stop - 1, s[0].stop - 1) for s in ndimage.find_objects(comp)]
    return torch.tensor(boxes).to(labels.device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.5)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ifseg_amd import hip
    from ifseg_amd.predict import region_table_reference
    try:
        import scipy  # noqa: F401
        have_scipy = True
    except ImportError:
        have_scipy = False
    dev = torch.device("cuda:0")
    lines = ["the region table on the device vs seg_regions alone (the floor), vs seg_regions + torch.unique + seven scatter_reduce, "
             "and vs labels.cpu() + scipy.ndimage: median [min, max] microseconds over %d alternating windows of >= %.1f s"
             % (a.windows, a.window_s),
             "one %d x %d uint8 map with conf; x = seg_regions / table (below 1: what the table costs over its floor)%s"
             % (H, W, "" if have_scipy else "  (scipy is not installed: NOT MEASURED)"), ""]
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    g = torch.Generator().manual_seed(11)
    conf = torch.rand(H, W, generator=g).to(dev)
    for conn in (4, 8):
        for name, lab in maps():
            d = lab.to(dev)
            R = 1 << 14 if name == "piecewise" else 1 << 19
            want = region_table_reference(d, conf, conn, 1, None, R)
            got = hip.seg_region_table(d, conf, conn, max_regions=R, flag=flag)
            k = int(want[2])
            assert k <= R, (name, conn, k, R)
            assert int(flag) == 0 and all(torch.equal(x, y) for x, y in zip(got, want)), (name, conn)
            roots, boxes, sums = torch_table(hip, d, conf, conn)
            assert torch.equal(roots, got[0][:k, 1].long()) and torch.equal(boxes, got[0][:k, 3:7].long()) and torch.equal(sums, got[1][:k])
            fns = [lambda: hip.seg_region_table(d, conf, conn, max_regions=R), lambda: hip.seg_regions(d, conn),
                   lambda: torch_table(hip, d, conf, conn)]
            labels = ["table", "seg_regions", "torch"]
            if have_scipy and name != "checkerboard":
                assert scipy_table(d, conf, conn).shape[0] == k
                fns.append(lambda: scipy_table(d, conf, conn))
                labels.append("cpu+scipy")
            row(lines, "conn %d %-12s %6d regions" % (conn, name, k), fns, labels, a)
    if not a.no_model:
        from ifseg_amd.tasks.mm_tasks.segmentation import SegmentationTask
        lines += ["", "end to end, SegOFA-Base, one raw uint8 %d x %d image; x = segment_raw / regions_raw" % (H, W)]
        n = 150
        torch.manual_seed(0)
        g = torch.Generator().manual_seed(7)
        names = [torch.randint(4, 50000, (int(k),), generator=g) for k in torch.randint(1, 4, (n,), generator=g)]
        task = SegmentationTask(num_seg_tokens=n, patch_image_size=P, arch="segofa_base", category_token_ids=names)
        model = task.build_model().to(dev).eval()
        seg = task.build_segmenter(model)
        img = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).to(dev)
        for conn in (4, 8):
            table = lambda: seg.regions_raw(img, connectivity=conn)
            plain = lambda: seg.segment_raw(img, return_conf=True)
            t, r = table()[0], plain()[0]
            want = region_table_reference(r.labels, r.conf, conn, 1, None, 1024)
            k = min(int(want[2]), 1024)
            assert torch.equal(t.count, want[2]) and torch.equal(t.rows[:k], want[0][:k]) and torch.equal(t.sums[:k], want[1][:k])
            row(lines, "n %3d conn %d, %6d regions" % (n, conn, int(want[2])), [table, plain], ("regions_raw", "segment_raw"), a)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
