"""Scoring on the device (csrc/predict.hip: hip.seg_score, hip.seg_score_views, hip.seg_areas; Segmenter.evaluate_raw) against the
composition it replaces, on the same device: the label map from `hip.seg_predict` / `hip.seg_predict_views` (end to end:
`Segmenter.segment_raw`), then the reference's `compute_metric` (seg_criterion.py:349-362) on the pixels its mask keeps --

    keep = (gt != 0) & (gt != 255);  pred, target = labels[keep].float(), gt[keep].float() - 1
    histc(pred[pred == target]), histc(pred), histc(target)            # bins = n, min = 0, max = n - 1

-- the label map written, read again, and five more passes over the image.

Cases: 15 and 150 classes, one 512 x 683 image, P = 512; a single view, and the six ratios 0.5 .. 1.75 with flip (K = 12,
"ms+flip").  Three blocks:
  kernels      the last launch alone, on given score grids: the scoring launch (counters only) against predict + histc
  seg_areas    `hip.seg_areas` on a given label map against the three histc, and `hip.seg_predict` + `hip.seg_areas` against
               `hip.seg_eval` (the criterion's kernel: resize, argmax, histogram and the display loss of one view in one launch,
               three global atomics per pixel) on the same scores
  end to end   `Segmenter.evaluate_raw` against `segment_raw` + histc, SegOFA-Base (--no-model leaves it out): the forward
               dominates, so this block shows what the difference amounts to in a call
The variants of a row alternate window by window in one process; a window is at least 0.5 s of enqueued calls between two
device events after a warm-up; the figure is the median over the windows, [min, max] its run-to-run spread: a difference inside
the spread is no difference.  The two sides of a row are checked to give the same counters before they are timed.

    python tools/evaluate_bench.py [--windows 5] [--window-s 0.5] [--no-model] [--out profiles/evaluate_bench.txt]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from predict_bench import alternate
from predict_tta_bench import H, P, W

CLASSES = (15, 150)
CASES = [("single view", (1.0,), False), ("ms+flip", (0.5, 0.75, 1.0, 1.25, 1.5, 1.75), True)]


def make_views(n, scales, flip, dev):
    from ifseg_amd.imageio import eval_size, view_list
    g = torch.Generator().manual_seed(1)
    views = []
    for ratio, flipped in view_list(scales, flip):
        oh, ow = eval_size(H, W, P, ratio)
        hp, wp = (oh + 15) // 16, (ow + 15) // 16
        views.append((torch.randn(1, hp * wp, n, generator=g).softmax(-1).to(dev), hp, wp, flipped))
    return views


def make_gt(n, dev):
    """a label PNG's values: classes 1 .. n in blocks of 32 x 32 pixels, about 10 % of the pixels ignored (0 and 255)"""
    g = torch.Generator().manual_seed(2)
    blocks = torch.randint(1, n + 1, ((H + 31) // 32, (W + 31) // 32), generator=g)
    gt = blocks.repeat_interleave(32, 0).repeat_interleave(32, 1)[:H, :W]
    drop = torch.rand(H, W, generator=g)
    gt = torch.where(drop < 0.05, torch.zeros_like(gt), torch.where(drop < 0.10, torch.full_like(gt, 255), gt))
    return gt.to(torch.uint8)[None].to(dev)


def histc_metric(labels, gt, n):
    """the reference's compute_metric on the device, behind the reference's mask -> float [3, n]"""
    keep = (gt != 0) & (gt != 255)
    pred, target = labels[keep].float(), gt[keep].float() - 1
    h = lambda t: torch.histc(t, bins=n, min=0, max=n - 1)
    return torch.stack([h(pred[pred == target]), h(pred), h(target)])


def row(lines, name, fns, labels, a):
    res = alternate(fns, a.windows, a.window_s)
    base = res[1][0]
    lines.append("  %-34s " % name + "   ".join("%s %9.1f [%9.1f, %9.1f]" % (lab, m, lo, hi) for lab, (m, lo, hi) in zip(labels, res))
                 + "   x%5.2f" % (base / res[0][0]))
    print(lines[-1], flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.5)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ifseg_amd import hip
    dev = torch.device("cuda:0")
    lines = ["scoring on the device vs label map + compute_metric (three torch.histc): median [min, max] microseconds over %d "
             "alternating windows of >= %.1f s" % (a.windows, a.window_s),
             "one %d x %d image, P %d; x = composition / new" % (H, W, P), "", "kernels (the last launch of a call, on given scores)"]
    for n in CLASSES:
        gt = make_gt(n, dev)
        for name, scales, flip in CASES:
            views = make_views(n, scales, flip, dev)
            if len(views) == 1:
                s, hp, wp, _ = views[0]
                new = lambda: hip.seg_score(s, hp, wp, gt)
                both = lambda: hip.seg_score(s, hp, wp, gt, labels=True)
                old = lambda: histc_metric(hip.seg_predict(s, hp, wp, H, W)[0], gt, n)
            else:
                new = lambda: hip.seg_score_views(views, gt)
                both = lambda: hip.seg_score_views(views, gt, labels=True)
                old = lambda: histc_metric(hip.seg_predict_views(views, H, W)[0], gt, n)
            assert torch.equal(new()[0].float(), old()) and torch.equal(both()[0], new()[0])
            row(lines, "n %3d %-12s K %2d" % (n, name, len(views)), [new, old, both], ("counters", "predict+histc", "counters+labels"), a)
    lines += ["", "seg_areas (a given label map; and the criterion's seg_eval on one view's scores, target = every pixel a class)"]
    for n in CLASSES:
        gt = make_gt(n, dev)
        s, hp, wp, _ = make_views(n, (1.0,), False, dev)[0]
        labels = hip.seg_predict(s, hp, wp, H, W)[0]
        assert torch.equal(hip.seg_areas(labels, gt, n)[0].float(), histc_metric(labels, gt, n))
        row(lines, "n %3d seg_areas" % n, [lambda: hip.seg_areas(labels, gt, n), lambda: histc_metric(labels, gt, n)],
            ("seg_areas", "3 x histc"), a)
        full = gt.clamp(1, n)                                  # seg_eval's target has no ignore value here: every pixel scored
        target = full.reshape(-1).long() - 1
        mine = hip.seg_areas(hip.seg_predict(s, hp, wp, H, W)[0], full, n)[0]
        far = (mine - hip.seg_eval(s[0], hp, wp, target, H, W, 0)[1]).abs().sum().item()     # near-ties may fall differently
        row(lines, "n %3d predict + seg_areas (L1 %d)" % (n, far), [lambda: hip.seg_areas(hip.seg_predict(s, hp, wp, H, W)[0], full, n),
                                                      lambda: hip.seg_eval(s[0], hp, wp, target, H, W, 0),
                                                      lambda: hip.seg_score(s, hp, wp, full)],
            ("predict+seg_areas", "seg_eval (+ loss)", "seg_score"), a)
    if not a.no_model:
        from ifseg_amd.tasks.mm_tasks.segmentation import SegmentationTask
        lines += ["", "end to end, SegOFA-Base, one raw uint8 %d x %d image" % (H, W)]
        for n in CLASSES:
            torch.manual_seed(0)
            g = torch.Generator().manual_seed(7)
            names = [torch.randint(4, 50000, (int(k),), generator=g) for k in torch.randint(1, 4, (n,), generator=g)]
            task = SegmentationTask(num_seg_tokens=n, patch_image_size=P, arch="segofa_base", category_token_ids=names)
            model = task.build_model().to(dev).eval()
            seg = task.build_segmenter(model)
            img = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).to(dev)
            gt = make_gt(n, dev)[0]
            for name, scales, flip in CASES:
                new = lambda: seg.evaluate_raw(img, gt, scales=scales, flip=flip)
                old = lambda: histc_metric(seg.segment_raw(img, scales=scales, flip=flip)[0].labels, gt, n)
                assert torch.equal(new().areas.float(), old())
                row(lines, "n %3d %-12s" % (n, name), [new, old], ("evaluate_raw", "segment_raw+histc"), a)
            del model, seg
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
