"""Connected regions on the device (csrc/regions.hip: hip.seg_regions, hip.seg_region_drop; Segmenter.pseudo_label_raw(min_region=))
against what a user does without them, per call as enqueued from Python.  One 512 x 683 uint8 map at connectivity 4 and 8:
  piecewise    classes in blocks of 32 x 32 pixels with 2 % of the pixels flipped to another class: what a segmenter gives
  random       an independent class per pixel, over 5 values: as many tile-local regions as a map can hold
  serpentine   full even rows joined alternately at the right and the left end: one chain through every tile, the long chase
and per map
  seg_regions, seg_region_drop(min_region=8)
  cpu+scipy    labels.cpu(), scipy.ndimage.label per present class with the components below 8 pixels set to 255, the result
               copied back: its device wait is part of it (left out when scipy is not installed)
  torch        the specification's iteration on the device (predict.regions_reference on device tensors: the data stays there,
               the convergence test reads one flag per iteration).  On the serpentine it needs thousands of iterations: timed
               once, not in windows
and `Segmenter.pseudo_label_raw` on SegOFA-Base with and without min_region=8, per image (--no-model leaves it out).
The variants of a row alternate window by window in one process; a window is at least 0.5 s of enqueued calls between two
device events after a warm-up; the figure is the median over the windows, [min, max] its run-to-run spread: a difference inside
the spread is no difference.  Every variant's result is checked against the specification before it is timed.

    python tools/regions_bench.py [--windows 5] [--window-s 0.5] [--no-model] [--out profiles/regions_bench.txt]
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from evaluate_bench import row
from predict_tta_bench import H, P, W

MIN_REGION = 8


def maps():
    g = torch.Generator().manual_seed(3)
    blocks = torch.randint(0, 15, ((H + 31) // 32, (W + 31) // 32), generator=g)
    piece = blocks.repeat_interleave(32, 0).repeat_interleave(32, 1)[:H, :W].clone()
    flip = torch.rand(H, W, generator=g) < 0.02
    piece[flip] = (piece[flip] + 1 + torch.randint(0, 14, (int(flip.sum()),), generator=g)) % 15
    y = torch.arange(H).reshape(H, 1).expand(H, W)
    x = torch.arange(W).reshape(1, W).expand(H, W)
    joint = torch.where(y % 4 == 1, x == W - 1, x == 0)
    serp = torch.where((y % 2 == 0) | joint, 1, 0)
    return (("piecewise", piece.to(torch.uint8)), ("random", torch.randint(0, 5, (H, W), generator=g).to(torch.uint8)),
            ("serpentine", serp.to(torch.uint8)))


def scipy_drop(labels, conn):
    """what a user does today -> the filtered map, back on the device"""
    import numpy as np
    from scipy import ndimage
    a = labels.cpu().numpy()
    out = a.copy()
    structure = np.ones((3, 3), dtype=int) if conn == 8 else None
    for v in np.unique(a):
        if v == 255:
            continue
        comp, k = ndimage.label(a == v, structure=structure)
        small = np.bincount(comp.reshape(-1), minlength=k + 1) < MIN_REGION
        small[0] = False
        out[small[comp]] = 255
    return torch.from_numpy(out).to(labels.device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.5)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ifseg_amd import hip
    from ifseg_amd.predict import region_drop_reference, regions_reference
    try:
        import scipy  # noqa: F401
        have_scipy = True
    except ImportError:
        have_scipy = False
    dev = torch.device("cuda:0")
    lines = ["connected regions on the device vs labels.cpu() + scipy.ndimage.label and vs the specification's iteration in torch: "
             "median [min, max] microseconds over %d alternating windows of >= %.1f s" % (a.windows, a.window_s),
             "one %d x %d uint8 map, min_region %d; x = cpu+scipy / seg_regions%s"
             % (H, W, MIN_REGION, "" if have_scipy else "  (scipy is not installed: NOT MEASURED, x = torch / seg_regions)"), ""]
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    for conn in (4, 8):
        for name, lab in maps():
            d = lab.to(dev)
            regions_reference(d, conn)                                # the specification on the device: once to warm up, then timed
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            w_root, w_size = regions_reference(d, conn)
            torch.cuda.synchronize()
            spec_us = (time.perf_counter() - t0) * 1e6
            w_out, w_dropped = region_drop_reference(d, w_size, MIN_REGION, n=15, raw_labels=False)
            root, size = hip.seg_regions(d, conn, flag=flag)
            out, dropped, _ = hip.seg_region_drop(d, conn, MIN_REGION, n=15, raw_labels=False, flag=flag)
            assert torch.equal(root, w_root) and torch.equal(size, w_size)
            assert torch.equal(out, w_out) and torch.equal(dropped, w_dropped) and int(flag) == 0
            w_root, w_out = w_root.cpu(), w_out.cpu()
            fns = [lambda: hip.seg_regions(d, conn), lambda: hip.seg_region_drop(d, conn, MIN_REGION, n=15, raw_labels=False)]
            labels = ["seg_regions", "seg_region_drop"]
            if have_scipy:
                assert torch.equal(scipy_drop(d, conn).cpu(), w_out)
                fns.insert(1, lambda: scipy_drop(d, conn))
                labels.insert(1, "cpu+scipy")
            once = ""
            if name == "serpentine":
                once = "   torch (one run, host clock) %9.1f" % spec_us
            else:
                fns.insert(len(fns) - 1 if have_scipy else 1, lambda: regions_reference(d, conn))
                labels.insert(len(labels) - 1 if have_scipy else 1, "torch")
            row(lines, "conn %d %-10s %6d regions" % (conn, name, int((w_root == torch.arange(H * W).reshape(H, W)).sum())),
                fns, labels, a)
            if once:
                lines[-1] += once
                print(once, flush=True)
    if not a.no_model:
        from ifseg_amd.tasks.mm_tasks.segmentation import SegmentationTask
        lines += ["", "end to end, SegOFA-Base, one raw uint8 %d x %d image, keep 0.5, boundary 1; x = with / without" % (H, W)]
        n = 150
        torch.manual_seed(0)
        g = torch.Generator().manual_seed(7)
        names = [torch.randint(4, 50000, (int(k),), generator=g) for k in torch.randint(1, 4, (n,), generator=g)]
        task = SegmentationTask(num_seg_tokens=n, patch_image_size=P, arch="segofa_base", category_token_ids=names)
        model = task.build_model().to(dev).eval()
        seg = task.build_segmenter(model)
        img = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).to(dev)
        for conn in (4, 8):
            kw = dict(keep=0.5, boundary=1, region_connectivity=conn)
            plain = lambda: seg.pseudo_label_raw(img, **kw)
            with_drop = lambda: seg.pseudo_label_raw(img, min_region=MIN_REGION, **kw)
            p, r = plain()[0], with_drop()[0]
            want = region_drop_reference(p.labels.cpu(), regions_reference(p.labels.cpu(), conn)[1], MIN_REGION, n=n)
            assert torch.equal(r.labels.cpu(), want[0]) and torch.equal(r.region_dropped.cpu(), want[1])
            row(lines, "n %3d conn %d, %6d pixels dropped" % (n, conn, int(want[1].sum())), [plain, with_drop],
                ("pseudo_label_raw", "min_region=8"), a)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
