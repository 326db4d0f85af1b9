"""Multi-scale + flip over sliding windows (Segmenter(slide_views=True); csrc/predict.hip: hip.seg_predict_slide_views) measured on
the device.

Block 1, the last launch against the composition it replaces: per view

    p = hip.seg_predict_windows(scores_k, ..., probs=True)[2];  p.flip(-1) if mirrored;  p.softmax(1) in softmax mode

added up, multiplied by 1 / K, and `argmax(1)` -- K tensors [n, h, w] written and read again.  Cases: 15 and 150 classes, a
512 x 683 image at P = 512 with the default slide (crop 512, stride 341), six ratios x flip (12 views), both modes.

Block 2, end to end on SegOFA-Base (--no-model leaves it out): `Segmenter(slide_views=True, upsample="logits").segment_raw(img,
slide=True, scales, flip=True)` against today's `Segmenter().segment_raw(img, scales, flip=True)` for one 512 x 683 image, time
per image; then `torch.cuda.max_memory_allocated()` after a set of four images of distinct aspects, first with the windows (with
a ratio >= 1 every forward at 512 x 512) and then without (one resized-bias entry of the engine per aspect and ratio).
--model-scales chooses the ratios of this block.

The variants of a row alternate window by window in one process; a window is at least 0.5 s of enqueued calls between two
device events after a warm-up; the figure is the median over the windows, [min, max] its run-to-run spread.

    python tools/predict_slide_views_bench.py [--windows 5] [--window-s 0.5] [--no-model] [--model-scales 0.5,0.75,...] [--out profiles/predict_slide_views_bench.txt]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from predict_bench import alternate

P = 512
CROP, STRIDE = P, 2 * P // 3
CLASSES = (15, 150)
IMAGE = (512, 683)
SCALES = (0.5, 0.75, 1.0, 1.25, 1.5, 1.75)
ASPECTS = ((512, 683), (683, 512), (512, 768), (600, 512))


def composition(views, h, w, softmax, want_probs):
    from ifseg_amd import hip
    total = None
    for s, hpw, wpw, oh, ow, flip in views:
        p = hip.seg_predict_windows(s, hpw, wpw, oh, ow, CROP, STRIDE, h, w, probs=True)[2]
        if flip:
            p = p.flip(-1)
        if softmax:
            p = p.softmax(1)
        total = p if total is None else total + p
    total = total * (1.0 / len(views))
    labels = total.argmax(1)
    return (labels, total) if want_probs else labels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.5)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--model-scales", default=",".join(str(r) for r in SCALES))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ifseg_amd import hip
    from ifseg_amd.imageio import eval_size, slide_windows, view_list
    dev = torch.device("cuda:0")
    h, w = IMAGE
    lines = ["hip.seg_predict_slide_views vs K x (hip.seg_predict_windows(probs=True) [+ flip] [+ softmax] + add) + scale + argmax: "
             "median [min, max] microseconds over %d alternating windows of >= %.1f s" % (a.windows, a.window_s),
             "P %d, crop %d, stride %d, image %d x %d, ratios %s x flip; MB = what the composition writes between its launches; "
             "x = composition / kernel" % (P, CROP, STRIDE, h, w, SCALES)]
    for n in CLASSES:
        for softmax in (False, True):
            views, nwin = [], 0
            for k, (ratio, flip) in enumerate(view_list(SCALES, True)):
                oh, ow = eval_size(h, w, P, ratio)
                ys, xs, ch, cw = slide_windows(oh, ow, CROP, STRIDE)
                nw, hpw, wpw = len(ys) * len(xs), ch // 16, cw // 16
                s = torch.randn(1, nw, hpw * wpw, n, generator=torch.Generator().manual_seed(k))
                views.append(((s if softmax else s.softmax(-1)).to(dev), hpw, wpw, oh, ow, flip))
                nwin += nw
            pk = hip.seg_predict_slide_views(views, CROP, STRIDE, h, w, softmax, probs=True)[2]
            pc = composition(views, h, w, softmax, True)[1]
            lines.append("")
            lines.append("n %d, %s mode, %d views, %d windows in all; %.1f MB; max |kernel - composition| = %.2e"
                         % (n, "softmax" if softmax else "linear", len(views), nwin, len(views) * n * h * w * 4 / 1e6,
                            (pk - pc).abs().max().item()))
            for variant, want in (("labels", False), ("labels+probs", True)):
                fns = [lambda: hip.seg_predict_slide_views(views, CROP, STRIDE, h, w, softmax, probs=want),
                       lambda: composition(views, h, w, softmax, want),
                       lambda: hip.seg_predict_slide_views(views, CROP, STRIDE, h, w, softmax, probs=want, staging_bytes=0)]
                (k, kmin, kmax), (c, cmin, cmax), (d, dmin, dmax) = alternate(fns, a.windows, a.window_s)
                lines.append("  %-13s kernel %9.1f [%9.1f, %9.1f]   composition %9.1f [%9.1f, %9.1f]   x%6.2f   direct-global path %9.1f"
                             % (variant, k, kmin, kmax, c, cmin, cmax, c / k, d))
                print(lines[-1], flush=True)
    if not a.no_model:
        from ifseg_amd.tasks.mm_tasks.segmentation import SegmentationTask
        n = 150
        scales = tuple(float(r) for r in a.model_scales.split(","))
        torch.manual_seed(0)
        g = torch.Generator().manual_seed(7)
        names = [torch.randint(4, 50000, (int(k),), generator=g) for k in torch.randint(1, 4, (n,), generator=g)]
        task = SegmentationTask(num_seg_tokens=n, patch_image_size=P, arch="segofa_base", category_token_ids=names)
        model = task.build_model().to(dev).eval()
        sv = task.build_segmenter(model, upsample="logits", slide_views=True)
        ms = task.build_segmenter(model)
        imgs = [torch.randint(0, 256, (hh, ww, 3), generator=g, dtype=torch.uint8).to(dev) for hh, ww in ASPECTS]
        lines += ["", "end to end, SegOFA-Base, n %d, raw uint8 images, ratios %s x flip" % (n, scales)]
        mem = []
        for seg, kw in ((sv, {"slide": True}), (ms, {})):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            for im in imgs:
                seg.segment_raw(im, scales=scales, flip=True, **kw)
            torch.cuda.synchronize()
            mem.append(torch.cuda.max_memory_allocated() / 2 ** 20)
        lines.append("  max_memory_allocated after the four aspects %s: windows %.0f MiB, then whole views %.0f MiB"
                     % (" ".join("%dx%d" % s for s in ASPECTS), mem[0], mem[1]))
        print(lines[-1], flush=True)
        fns = [lambda: sv.segment_raw(imgs[0], slide=True, scales=scales, flip=True),
               lambda: ms.segment_raw(imgs[0], scales=scales, flip=True)]
        (k, kmin, kmax), (c, cmin, cmax) = alternate(fns, a.windows, a.window_s)
        lines.append("  one %d x %d image: windows %9.1f [%9.1f, %9.1f]   whole views %9.1f [%9.1f, %9.1f]   x%6.2f (whole / windows)"
                     % (*ASPECTS[0], k, kmin, kmax, c, cmin, cmax, c / k))
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
