"""Confidence calibration counted on the device (csrc/calib.hip: hip.seg_calibration; Segmenter.evaluate_raw(calibration=True))
against the composition it replaces, on the same device: the scored mask with boolean indexing, then one bincount over the
(label, bin, hit) index --

    g = gt.long();  keep = (g != 0) & (g != 255) & (g <= n);  lab = labels.long()[keep]
    b = nan_to_num(floor(conf * 256)).clamp(0, 255).long()[keep]
    torch.bincount((lab * 256 + b) * 2 + (lab == g[keep] - 1), minlength=n * 512).reshape(n, 256, 2)

-- per call as enqueued from Python.  One 512 x 683 map, n = 15 (direct LDS table), 150 and 512 (hashed LDS table), two inputs
each:
  piecewise   the argmax and winning probability of `hip.seg_predict` on random per-patch scores against ground truth in blocks
              of 32 x 32 pixels: what a segmenter gives, and what the wave pre-aggregation in front of the table is for (the
              confidence still varies from pixel to pixel, so fewer lanes share a key than in the confusion matrix)
  random      an independent random label, confidence and ground truth per pixel: the worst case for the table (every lane
              another key; above n = 32 a workgroup's keys crowd its table and part of them goes to global memory directly)
and `Segmenter.evaluate_raw` on SegOFA-Base with and without `calibration=True` (--no-model leaves it out).
The variants of a row alternate window by window in one process; a window is at least 0.5 s of enqueued calls between two
device events after a warm-up; the figure is the median over the windows, [min, max] its run-to-run spread: a difference inside
the spread is no difference.  The two sides of a row are checked to give the same counters before they are timed.

    python tools/calibration_bench.py [--windows 5] [--window-s 0.5] [--no-model] [--out profiles/calibration_bench.txt]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from confusion_bench import gt_dtype
from evaluate_bench import row
from predict_tta_bench import H, P, W
from pseudo_label_bench import torch_bins

CLASSES = (15, 150, 512)
MODEL_CLASSES = (15, 150)


def block_gt(n, g, dev):
    """ground truth [H, W] in blocks of 32 x 32 pixels with about 10 % of the pixels ignored (0 and 255)"""
    blocks = torch.randint(1, n + 1, ((H + 31) // 32, (W + 31) // 32), generator=g)
    blocks = torch.where(blocks == 255, torch.ones_like(blocks), blocks)             # 255 is an ignore value, not class 254
    gt = blocks.repeat_interleave(32, 0).repeat_interleave(32, 1)[:H, :W]
    drop = torch.rand(H, W, generator=g)
    gt = torch.where(drop < 0.05, torch.zeros_like(gt), torch.where(drop < 0.10, torch.full_like(gt, 255), gt))
    return gt.to(gt_dtype(n)).to(dev)


def piecewise(n, dev):
    """-> (labels, conf, gt) [H, W]: seg_predict's argmax and winning probability of random per-patch scores"""
    from ifseg_amd import hip
    g = torch.Generator().manual_seed(1)
    hp, wp = (H + 15) // 16, (W + 15) // 16
    labels, conf, _ = hip.seg_predict((3.0 * torch.randn(1, hp * wp, n, generator=g)).softmax(-1).to(dev), hp, wp, H, W, conf=True)
    return labels[0].contiguous(), conf[0].contiguous(), block_gt(n, g, dev)


def random_maps(n, dev):
    g = torch.Generator().manual_seed(2)
    labels = torch.randint(0, n, (H, W), generator=g).to(torch.uint8 if n <= 256 else torch.int16)
    gt = torch.randint(0, n + 1, (H, W), generator=g)
    gt = torch.where(gt == 255, torch.zeros_like(gt), gt)
    return labels.to(dev), torch.rand(H, W, generator=g).to(dev), gt.to(gt_dtype(n)).to(dev)


def bincount_calibration(labels, conf, gt, n):
    g = gt.reshape(-1).long()
    keep = (g != 0) & (g != 255) & (g <= n)
    lab, b = labels.reshape(-1).long()[keep], torch_bins(conf).reshape(-1)[keep]
    return torch.bincount((lab * 256 + b) * 2 + (lab == g[keep] - 1), minlength=n * 512).reshape(n, 256, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.5)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ifseg_amd import hip
    dev = torch.device("cuda:0")
    lines = ["calibration counters on the device vs scored mask + torch.bincount: median [min, max] microseconds over %d alternating "
             "windows of >= %.1f s" % (a.windows, a.window_s),
             "one %d x %d map; x = composition / new; direct LDS table up to n = %d, above it %d hashed slots"
             % (H, W, hip.SEG_CALIBRATION_DIRECT_CLASSES, hip.SEG_CALIBRATION_SLOTS), "", "hip.seg_calibration (a given label map)"]
    for n in CLASSES:
        for name, make in (("piecewise", piecewise), ("random", random_maps)):
            labels, conf, gt = make(n, dev)
            got = hip.seg_calibration(labels, conf, gt, n)[0]
            assert torch.equal(got, bincount_calibration(labels, conf, gt, n)) and int(got[..., 1].sum()) > 0
            row(lines, "n %3d %-9s %6d keys" % (n, name, int((got != 0).sum())),
                [lambda: hip.seg_calibration(labels, conf, gt, n), lambda: bincount_calibration(labels, conf, gt, n),
                 lambda: hip.seg_conf_hist(labels, conf, n), lambda: hip.seg_confusion(labels, gt, n)],
                ("seg_calibration", "mask+bincount", "(seg_conf_hist)", "(seg_confusion)"), a)
    if not a.no_model:
        from ifseg_amd.tasks.mm_tasks.segmentation import SegmentationTask
        lines += ["", "end to end, SegOFA-Base, one raw uint8 %d x %d image; x = with / without" % (H, W)]
        for n in MODEL_CLASSES:
            torch.manual_seed(0)
            g = torch.Generator().manual_seed(7)
            names = [torch.randint(4, 50000, (int(k),), generator=g) for k in torch.randint(1, 4, (n,), generator=g)]
            task = SegmentationTask(num_seg_tokens=n, patch_image_size=P, arch="segofa_base", category_token_ids=names)
            model = task.build_model().to(dev).eval()
            seg = task.build_segmenter(model)
            img = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).to(dev)
            gt = block_gt(n, torch.Generator().manual_seed(1), dev)
            for name, kw in (("single view", {}), ("ms+flip", dict(scales=(0.5, 0.75, 1.0, 1.25, 1.5, 1.75), flip=True))):
                plain = lambda: seg.evaluate_raw(img, gt, **kw)
                with_counters = lambda: seg.evaluate_raw(img, gt, calibration=True, **kw)
                score, labels = seg.evaluate_raw(img, gt, calibration=True, return_labels=True, **kw)
                conf = seg.segment_raw(img, return_conf=True, **kw)[0].conf
                assert torch.equal(score.calibration, bincount_calibration(labels[0], conf, gt, n))
                assert torch.equal(score.areas, plain().areas)
                row(lines, "n %3d %-12s" % (n, name), [plain, with_counters], ("evaluate_raw", "calibration=True"), a)
            del model, seg
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
