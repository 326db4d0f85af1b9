"""Sliding-window inference (Segmenter.segment_raw(slide=...); csrc/predict.hip: hip.seg_predict_windows) measured on the device.

Block 1, the last launch against the composition it replaces: per window

    hip.seg_predict(scores_k, hpw, wpw, ch, cw, probs=True)[2]

added into a zero [n, oh, ow] plane at the window's place, a count plane, one division, `F.interpolate` to the image's shape
where it differs from (oh, ow), and `argmax(1)` -- Nw tensors [n, ch, cw], the sum and the count written and read again.
Cases: 15 and 150 classes, P = 512 with the default slide (crop 512, stride 341): a 512 x 683 image (network size 512 x 683, two
windows, the second stage is the identity) and a 480 x 640 image (the same network size, resized back to 480 x 640).

Block 2, end to end on SegOFA-Base (--no-model leaves it out): `segment_raw(img, slide=True)` against `segment_raw(img)` for one
512 x 683 image, time per image; then `torch.cuda.max_memory_allocated()` after a set of four images of distinct aspects, first
with slide (every forward at 512 x 512) and then without (one resized-bias entry of the engine per aspect).

The variants of a row alternate window by window in one process; a window is at least 0.5 s of enqueued calls between two
device events after a warm-up; the figure is the median over the windows, [min, max] its run-to-run spread.

    python tools/predict_slide_bench.py [--windows 5] [--window-s 0.5] [--no-model] [--out profiles/predict_slide_bench.txt]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from predict_bench import alternate

P = 512
CROP, STRIDE = P, 2 * P // 3
CLASSES = (15, 150)
IMAGES = ((512, 683), (480, 640))
ASPECTS = ((512, 683), (683, 512), (512, 768), (600, 512))     # four network sizes without slide, one with


def composition(scores, hpw, wpw, oh, ow, h, w, windows, want_probs):
    from ifseg_amd import hip
    ys, xs, ch, cw = windows
    n = scores.shape[-1]
    total = torch.zeros(1, n, oh, ow, device=scores.device)
    count = torch.zeros(1, 1, oh, ow, device=scores.device)
    for k, (y, x) in enumerate((y, x) for y in ys for x in xs):
        total[:, :, y:y + ch, x:x + cw] += hip.seg_predict(scores[:, k], hpw, wpw, ch, cw, probs=True)[2]
        count[:, :, y:y + ch, x:x + cw] += 1
    total /= count
    if (h, w) != (oh, ow):
        total = F.interpolate(total, size=(h, w), mode="bilinear", align_corners=False)
    labels = total.argmax(1)
    return (labels, total) if want_probs else labels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.5)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ifseg_amd import hip
    from ifseg_amd.imageio import eval_size, slide_windows
    dev = torch.device("cuda:0")
    lines = ["hip.seg_predict_windows vs Nw x hip.seg_predict(probs=True) + padded adds + count + divide (+ F.interpolate) + argmax: "
             "median [min, max] microseconds over %d alternating windows of >= %.1f s" % (a.windows, a.window_s),
             "P %d, crop %d, stride %d; MB = what the composition writes between its launches; x = composition / kernel" % (P, CROP, STRIDE)]
    for n in CLASSES:
        for h, w in IMAGES:
            oh, ow = eval_size(h, w, P)
            windows = slide_windows(oh, ow, CROP, STRIDE)
            ys, xs, ch, cw = windows
            nw, hpw, wpw = len(ys) * len(xs), ch // 16, cw // 16
            s = torch.randn(1, nw, hpw * wpw, n, generator=torch.Generator().manual_seed(1)).softmax(-1).to(dev)
            geo = (hpw, wpw, oh, ow, CROP, STRIDE, h, w)
            pk = hip.seg_predict_windows(s, *geo, probs=True)[2]
            pc = composition(s, hpw, wpw, oh, ow, h, w, windows, True)[1]
            between = (nw * n * ch * cw + n * oh * ow + oh * ow + (n * h * w if (h, w) != (oh, ow) else 0)) * 4
            lines.append("")
            lines.append("n %d, image %d x %d, network %d x %d, %d windows of %d x %d (%d x %d patches); %.1f MB; max |kernel - "
                         "composition| = %.2e" % (n, h, w, oh, ow, nw, ch, cw, hpw, wpw, between / 1e6, (pk - pc).abs().max().item()))
            for variant, want in (("labels", False), ("labels+probs", True)):
                fns = [lambda: hip.seg_predict_windows(s, *geo, probs=want),
                       lambda: composition(s, hpw, wpw, oh, ow, h, w, windows, want),
                       lambda: hip.seg_predict_windows(s, *geo, probs=want, staging_bytes=0)]
                (k, kmin, kmax), (c, cmin, cmax), (d, dmin, dmax) = alternate(fns, a.windows, a.window_s)
                lines.append("  %-13s kernel %9.1f [%9.1f, %9.1f]   composition %9.1f [%9.1f, %9.1f]   x%6.2f   direct-global path %9.1f"
                             % (variant, k, kmin, kmax, c, cmin, cmax, c / k, d))
                print(lines[-1], flush=True)
    if not a.no_model:
        from ifseg_amd.tasks.mm_tasks.segmentation import SegmentationTask
        n = 150
        torch.manual_seed(0)
        g = torch.Generator().manual_seed(7)
        names = [torch.randint(4, 50000, (int(k),), generator=g) for k in torch.randint(1, 4, (n,), generator=g)]
        task = SegmentationTask(num_seg_tokens=n, patch_image_size=P, arch="segofa_base", category_token_ids=names)
        model = task.build_model().to(dev).eval()
        seg = task.build_segmenter(model)
        imgs = [torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).to(dev) for h, w in ASPECTS]
        lines += ["", "end to end, SegOFA-Base, n %d, raw uint8 images" % n]
        # memory first, on a fresh engine: the slide set, then the same set without slide
        mem = []
        for slide in (True, None):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            for im in imgs:
                seg.segment_raw(im, slide=slide)
            torch.cuda.synchronize()
            mem.append(torch.cuda.max_memory_allocated() / 2 ** 20)
        lines.append("  max_memory_allocated after the four aspects %s: slide=True %.0f MiB, then slide=None %.0f MiB"
                     % (" ".join("%dx%d" % s for s in ASPECTS), mem[0], mem[1]))
        print(lines[-1], flush=True)
        fns = [lambda: seg.segment_raw(imgs[0], slide=True), lambda: seg.segment_raw(imgs[0])]
        (k, kmin, kmax), (c, cmin, cmax) = alternate(fns, a.windows, a.window_s)
        lines.append("  one %d x %d image: slide=True %9.1f [%9.1f, %9.1f]   whole image %9.1f [%9.1f, %9.1f]   x%6.2f (whole / slide)"
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
