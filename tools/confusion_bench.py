"""The class confusion matrix on the device (csrc/predict.hip: hip.seg_confusion; Segmenter.evaluate_raw(confusion=True)) against
the composition it replaces, on the same device: the scored mask, then one bincount over the pair index --

    g = gt.long();  keep = (g != 0) & (g != 255) & (g <= n)
    torch.bincount((g[keep] - 1) * (n + 1) + labels.long()[keep], minlength=n * (n + 1)).reshape(n, n + 1)

-- per call as enqueued from Python.  One 512 x 683 label map, n = 15 (direct LDS table), 150 and 512 (hashed LDS table),
two inputs each:
  piecewise   the argmax of `hip.seg_predict` on smooth random scores against ground truth in blocks of 32 x 32 pixels: what a
              segmenter gives, and what the wave pre-aggregation in front of the table is for
  random      independent random labels and ground truth per pixel: the worst case for the table (every lane another pair;
              at n = 512 a workgroup's pairs crowd its table and part of them goes to global memory directly)
and `Segmenter.evaluate_raw` on SegOFA-Base with and without `confusion=True` (--no-model leaves it out).
The variants of a row alternate window by window in one process; a window is at least 0.5 s of enqueued calls between two
device events after a warm-up; the figure is the median over the windows, [min, max] its run-to-run spread: a difference inside
the spread is no difference.  The two sides of a row are checked to give the same matrix before they are timed.

    python tools/confusion_bench.py [--windows 5] [--window-s 0.5] [--no-model] [--out profiles/confusion_bench.txt]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from evaluate_bench import row
from predict_tta_bench import H, P, W

CLASSES = (15, 150, 512)
MODEL_CLASSES = (15, 150)


def gt_dtype(n):
    return torch.uint8 if n < 255 else torch.int16


def piecewise(n, dev):
    """-> (labels, gt) [1, H, W]: seg_predict's argmax of random per-patch scores, ground truth in blocks of 32 x 32 pixels with
    about 10 % of the pixels ignored (0 and 255)"""
    from ifseg_amd import hip
    g = torch.Generator().manual_seed(1)
    hp, wp = (H + 15) // 16, (W + 15) // 16
    labels = hip.seg_predict(torch.randn(1, hp * wp, n, generator=g).softmax(-1).to(dev), hp, wp, H, W)[0]
    blocks = torch.randint(1, n + 1, ((H + 31) // 32, (W + 31) // 32), generator=g)
    blocks = torch.where(blocks == 255, torch.ones_like(blocks), blocks)             # 255 is an ignore value, not class 254
    gt = blocks.repeat_interleave(32, 0).repeat_interleave(32, 1)[:H, :W]
    drop = torch.rand(H, W, generator=g)
    gt = torch.where(drop < 0.05, torch.zeros_like(gt), torch.where(drop < 0.10, torch.full_like(gt, 255), gt))
    return labels, gt.to(gt_dtype(n))[None].to(dev)


def random_maps(n, dev):
    g = torch.Generator().manual_seed(2)
    labels = torch.randint(0, n, (1, H, W), generator=g).to(torch.uint8 if n <= 256 else torch.int16)
    gt = torch.randint(0, n + 1, (1, H, W), generator=g)
    gt = torch.where(gt == 255, torch.zeros_like(gt), gt)
    return labels.to(dev), gt.to(gt_dtype(n)).to(dev)


def bincount_confusion(labels, gt, n):
    g = gt.reshape(-1).long()
    keep = (g != 0) & (g != 255) & (g <= n)
    return torch.bincount((g[keep] - 1) * (n + 1) + labels.reshape(-1).long()[keep], minlength=n * (n + 1)).reshape(n, n + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.5)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ifseg_amd import hip
    dev = torch.device("cuda:0")
    lines = ["confusion matrix on the device vs scored mask + torch.bincount: median [min, max] microseconds over %d alternating "
             "windows of >= %.1f s" % (a.windows, a.window_s),
             "one %d x %d label map; x = composition / new; direct LDS table up to n (n + 1) = %d, above it %d hashed slots"
             % (H, W, hip.SEG_CONFUSION_DIRECT_MAX, hip.SEG_CONFUSION_SLOTS), "", "hip.seg_confusion (a given label map)"]
    for n in CLASSES:
        for name, make in (("piecewise", piecewise), ("random", random_maps)):
            labels, gt = make(n, dev)
            assert torch.equal(hip.seg_confusion(labels, gt, n), bincount_confusion(labels, gt, n))
            pairs = int((hip.seg_confusion(labels, gt, n) != 0).sum())
            row(lines, "n %3d %-9s %6d pairs" % (n, name, pairs), [lambda: hip.seg_confusion(labels, gt, n),
                                                                  lambda: bincount_confusion(labels, gt, n),
                                                                  lambda: hip.seg_areas(labels, gt, n)],
                ("seg_confusion", "mask+bincount", "(seg_areas)"), a)
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
            gt = piecewise(n, dev)[1][0]
            for name, kw in (("single view", {}), ("ms+flip", dict(scales=(0.5, 0.75, 1.0, 1.25, 1.5, 1.75), flip=True))):
                plain = lambda: seg.evaluate_raw(img, gt, **kw)
                with_matrix = lambda: seg.evaluate_raw(img, gt, confusion=True, **kw)
                score, labels = seg.evaluate_raw(img, gt, confusion=True, return_labels=True, **kw)
                assert torch.equal(score.confusion, bincount_confusion(labels[0], gt, n)) and torch.equal(score.areas, plain().areas)
                row(lines, "n %3d %-12s" % (n, name), [plain, with_matrix], ("evaluate_raw", "confusion=True"), a)
            del model, seg
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
