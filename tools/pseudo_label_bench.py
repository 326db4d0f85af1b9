"""Confidence-filtered pseudo-labels on the device (csrc/pseudo.hip: hip.seg_conf_hist, hip.seg_pseudo;
Segmenter.pseudo_label_raw) against the torch composition they replace, on the same device, per call as enqueued from Python:

  histogram   one bincount over label * 256 + bin of the in-range pixels (the sorted-histogram way to a per-class threshold; a
              per-class `torch.quantile` needs a host round trip per class for its mask and sorts every class)
  filter      the threshold gathered per pixel, r > 0: the (2 r + 1)^2 - 1 shifted comparisons of the ignore band, torch.where,
              and two bincounts for `kept`

One 512 x 683 map, n = 15 (direct LDS table) and 150 (hashed), r = 0 and 1, two inputs each:
  piecewise   the argmax and winning probability of `hip.seg_predict` on random per-patch scores: what a segmenter gives
  random      an independent random label and confidence per pixel: the worst case for the histogram's table
and `Segmenter.pseudo_label_raw` against `Segmenter.segment_raw(return_conf=True)` on SegOFA-Base (--no-model leaves it out).
The variants of a row alternate window by window in one process; a window is at least 0.5 s of enqueued calls between two
device events after a warm-up; the figure is the median over the windows, [min, max] its run-to-run spread: a difference inside
the spread is no difference.  The two sides of a row are checked to give the same result before they are timed.

    python tools/pseudo_label_bench.py [--windows 5] [--window-s 0.5] [--no-model] [--out profiles/pseudo_label_bench.txt]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from evaluate_bench import row
from predict_tta_bench import H, P, W

CLASSES = (15, 150)
RADII = (0, 1)


def piecewise(n, dev):
    """-> (labels uint8, conf fp32) [H, W]: seg_predict's argmax and winning probability of random per-patch scores"""
    from ifseg_amd import hip
    g = torch.Generator().manual_seed(1)
    hp, wp = (H + 15) // 16, (W + 15) // 16
    labels, conf, _ = hip.seg_predict((3.0 * torch.randn(1, hp * wp, n, generator=g)).softmax(-1).to(dev), hp, wp, H, W, conf=True)
    return labels[0].contiguous(), conf[0].contiguous()


def random_maps(n, dev):
    g = torch.Generator().manual_seed(2)
    return torch.randint(0, n, (H, W), generator=g).to(torch.uint8).to(dev), torch.rand(H, W, generator=g).to(dev)


def torch_bins(conf):
    return torch.nan_to_num(torch.floor(conf * 256.0), nan=0.0).clamp_(0.0, 255.0).long()


def torch_hist(labels, conf, n):
    lab = labels.reshape(-1).long()
    inside = lab < n
    return torch.bincount(lab[inside] * 256 + torch_bins(conf).reshape(-1)[inside], minlength=n * 256).reshape(n, 256)


def torch_filter(labels, conf, thr, n, r):
    lab = labels.long()
    inside = lab < n
    cls = lab.clamp_max(n - 1)
    keep = inside & (torch_bins(conf) >= thr.long()[cls])
    if r:
        edge = torch.zeros_like(inside)
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                if dy or dx:
                    here = (slice(max(-dy, 0), H - max(dy, 0)), slice(max(-dx, 0), W - max(dx, 0)))
                    there = (slice(max(dy, 0), H - max(-dy, 0)), slice(max(dx, 0), W - max(-dx, 0)))
                    edge[here] |= lab[here] != lab[there]
        keep &= ~edge
    out = torch.where(keep, cls + 1, torch.full_like(cls, 255)).to(torch.uint8)
    return out, torch.stack([torch.bincount(cls[keep], minlength=n), torch.bincount(cls[inside], minlength=n)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.5)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ifseg_amd import hip
    from ifseg_amd.predict import pseudo_thresholds
    dev = torch.device("cuda:0")
    lines = ["pseudo-labels on the device vs the torch composition: median [min, max] microseconds over %d alternating windows of "
             ">= %.1f s" % (a.windows, a.window_s),
             "one %d x %d label map with its confidences; x = composition / new; histogram: direct LDS table up to n = %d, above it "
             "%d hashed slots" % (H, W, hip.SEG_CONF_HIST_DIRECT_CLASSES, hip.SEG_CONF_HIST_SLOTS), ""]
    for n in CLASSES:
        for name, make in (("piecewise", piecewise), ("random", random_maps)):
            labels, conf = make(n, dev)
            hist = hip.seg_conf_hist(labels, conf, n)[0]
            assert torch.equal(hist, torch_hist(labels, conf, n))
            row(lines, "hist   n %3d %-9s %6d pairs" % (n, name, int((hist != 0).sum())),
                [lambda: hip.seg_conf_hist(labels, conf, n), lambda: torch_hist(labels, conf, n)], ("seg_conf_hist", "bincount"), a)
            thr = pseudo_thresholds(hist, keep=0.5)
            for r in RADII:
                got, want = hip.seg_pseudo(labels, conf, thr, n, r), torch_filter(labels, conf, thr, n, r)
                assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
                row(lines, "filter n %3d %-9s r %d" % (n, name, r),
                    [lambda: hip.seg_pseudo(labels, conf, thr, n, r), lambda: torch_filter(labels, conf, thr, n, r)],
                    ("seg_pseudo", "torch"), a)
    if not a.no_model:
        from ifseg_amd.tasks.mm_tasks.segmentation import SegmentationTask
        lines += ["", "end to end, SegOFA-Base, one raw uint8 %d x %d image; x = segment_raw / pseudo_label_raw" % (H, W)]
        for n in CLASSES:
            torch.manual_seed(0)
            g = torch.Generator().manual_seed(7)
            names = [torch.randint(4, 50000, (int(k),), generator=g) for k in torch.randint(1, 4, (n,), generator=g)]
            task = SegmentationTask(num_seg_tokens=n, patch_image_size=P, arch="segofa_base", category_token_ids=names)
            model = task.build_model().to(dev).eval()
            seg = task.build_segmenter(model)
            img = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).to(dev)
            for name, kw in (("single view", {}), ("ms+flip", dict(scales=(0.5, 0.75, 1.0, 1.25, 1.5, 1.75), flip=True))):
                row(lines, "n %3d %-12s" % (n, name), [lambda: seg.pseudo_label_raw(img, keep=0.5, boundary=1, **kw),
                                                       lambda: seg.segment_raw(img, return_conf=True, **kw)],
                    ("pseudo_label_raw", "segment_raw(conf)"), a)
            del model, seg
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
