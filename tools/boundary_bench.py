"""Boundary IoU's band areas on the device (csrc/boundary.hip: hip.seg_boundary_areas; Segmenter.evaluate_raw(boundary_iou=True))
against the composition it replaces, on the same device and of the same rule (`predict.boundary_areas_reference`): per map a
separable `max_pool2d` of the values and of their negatives (row pass, column pass), window maximum != window minimum or
the frame of width d, then the scored mask and three `torch.bincount` -- written without boolean indexing, so it does not
synchronise with the host either -- per call as enqueued from Python.
  512 x 683 (d = 17) at 15 and 150 classes, 1024 x 2048 (d = 46) at 19 classes, two inputs each:
  piecewise   ground truth in blocks of 32 x 32 pixels with a tenth ignored, the labels the same blocks shifted by (5, 7)
  random      independent random labels and ground truth per pixel: every window holds two values, the band is everything
and `Segmenter.evaluate_raw` on SegOFA-Base with and without `boundary_iou=True` (--no-model leaves it out).
The variants of a row alternate window by window in one process; a window is at least 0.5 s of enqueued calls between two
device events after a warm-up; the figure is the median over the windows, [min, max] its run-to-run spread: a difference inside
the spread is no difference.  The two sides of a row are checked to give the same integers before they are timed.

    python tools/boundary_bench.py [--windows 5] [--window-s 0.5] [--no-model] [--out profiles/boundary_bench.txt]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from evaluate_bench import row
from predict_tta_bench import H, P, W

SIZES = ((H, W, 15), (H, W, 150), (1024, 2048, 19))
MODEL_CLASSES = (15, 150)


def piecewise(h, w, n, dev):
    g = torch.Generator().manual_seed(1)
    blocks = torch.randint(1, n + 1, ((h + 31) // 32 + 1, (w + 31) // 32 + 1), generator=g)
    full = blocks.repeat_interleave(32, 0).repeat_interleave(32, 1)
    drop = torch.rand(h, w, generator=g)
    gt = torch.where(drop < 0.05, torch.zeros(h, w, dtype=torch.long), torch.where(drop < 0.10, torch.full((h, w), 255), full[:h, :w]))
    return (full[5:h + 5, 7:w + 7] - 1).to(torch.uint8)[None].contiguous().to(dev), gt.to(torch.uint8)[None].to(dev)


def random_maps(h, w, n, dev):
    g = torch.Generator().manual_seed(2)
    return (torch.randint(0, n, (1, h, w), generator=g).to(torch.uint8).to(dev),
            torch.randint(0, n + 1, (1, h, w), generator=g).to(torch.uint8).to(dev))


def _band(v, d):
    h, w = v.shape[-2:]
    f = v.float()[:, None]
    pool = lambda t: F.max_pool2d(F.max_pool2d(t, (1, 2 * d + 1), 1, (0, d)), (2 * d + 1, 1), 1, (d, 0))
    frame = torch.ones(h, w, dtype=torch.bool, device=v.device)
    frame[d:h - d, d:w - d] = False
    return (pool(f) != -pool(-f))[:, 0] | frame


def torch_boundary_areas(labels, gt, n, d):
    """the rule on the device with torch alone, raw labels -> bareas int64 [3, n]"""
    g, p = gt.long(), labels.long()
    gb, pb = _band(g, d), _band(p, d)
    scored = (g != 0) & (g != 255) & (g <= n)
    cls, known = g - 1, scored & (p < n)
    none = torch.full_like(p, n)
    count = lambda key, on: torch.bincount(torch.where(on, key, none).reshape(-1), minlength=n + 1)[:n]
    return torch.stack([count(p, known & (p == cls) & gb & pb), count(p, known & pb), count(cls, scored & gb)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.5)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ifseg_amd import hip
    from ifseg_amd.predict import boundary_distance
    dev = torch.device("cuda:0")
    lines = ["Boundary IoU band areas on the device vs separable max_pool2d + masks + three torch.bincount: median [min, max] "
             "microseconds over %d alternating windows of >= %.1f s" % (a.windows, a.window_s),
             "one label map per call; x = composition / new", "", "hip.seg_boundary_areas (a given label map)"]
    for h, w, n in SIZES:
        d = boundary_distance(h, w)
        for name, make in (("piecewise", piecewise), ("random", random_maps)):
            labels, gt = make(h, w, n, dev)
            got = hip.seg_boundary_areas(labels, gt, n, d)[0]
            assert torch.equal(got, torch_boundary_areas(labels, gt, n, d)) and int(got[0].sum()) > 0
            row(lines, "%4d x %4d d %2d n %3d %-9s" % (h, w, d, n, name),
                [lambda: hip.seg_boundary_areas(labels, gt, n, d), lambda: torch_boundary_areas(labels, gt, n, d),
                 lambda: hip.seg_boundary_areas(labels, gt, n, d, band=True), lambda: hip.seg_areas(labels, gt, n)],
                ("seg_boundary_areas", "pool+bincount", "(with band)", "(seg_areas)"), a)
    if not a.no_model:
        from ifseg_amd.tasks.mm_tasks.segmentation import SegmentationTask
        lines += ["", "end to end, SegOFA-Base, one raw uint8 %d x %d image (d = %d); x = with / without" % (H, W, boundary_distance(H, W))]
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
                with_bands = lambda: seg.evaluate_raw(img, gt, boundary_iou=True, **kw)
                score, labels = seg.evaluate_raw(img, gt, boundary_iou=True, return_labels=True, **kw)
                assert torch.equal(score.boundary, torch_boundary_areas(labels[0][None], gt[None], n, boundary_distance(H, W)))
                assert torch.equal(score.areas, plain().areas)
                row(lines, "n %3d %-12s" % (n, name), [plain, with_bands], ("evaluate_raw", "boundary_iou=True"), a)
            del model, seg
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
