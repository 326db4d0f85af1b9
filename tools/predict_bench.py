"""hip.seg_predict (csrc/predict.hip) against the composition a user had before it, on the same device:

    F.interpolate(scores.transpose(1, 2).reshape(B, n, hp, wp), (h, w), mode="bilinear", align_corners=False).argmax(1)

in three variants -- labels only, labels + conf (torch: .max(1)), labels + probs (torch: the interpolated tensor is kept).
Both sides alternate window by window in one process; a window is at least 0.5 s of enqueued calls between two device events
after a warm-up; the figure is the median over the windows.  Every kernel row carries its byte floor
(B P n 4 read + B h w label_bytes written, + B h w 4 for conf, + B n h w 4 for probs) and the share of the HBM rate
(6.3 TB/s achievable on MI355X, 8 TB/s nominal) that floor over the measured time amounts to.

The last block times one Segmenter call (SegOFA-Base, batch 8, 512 x 512, 15 classes) against the model forward alone.

    python tools/predict_bench.py [--windows 5] [--window-s 0.5] [--out profiles/predict_ab.txt] [--no-model]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

HBM_ACHIEVABLE, HBM_NOMINAL = 6.3e12, 8.0e12
SHAPES = [(8, 32, 32, 15, 512, 512), (8, 32, 32, 150, 512, 512), (2, 40, 40, 171, 640, 640), (1, 32, 32, 150, 500, 375)]


def window(fn, seconds):
    """-> microseconds per call over one window of at least `seconds`"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    iters = max(3, int(seconds * 1e3 / max(e0.elapsed_time(e1), 1e-3)) + 1)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def alternate(fns, windows, seconds):
    for f in fns:
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    us = [[] for _ in fns]
    for _ in range(windows):
        for i, f in enumerate(fns):
            us[i].append(window(f, seconds))
    return [(statistics.median(u), min(u), max(u)) for u in us]


def torch_side(scores, hp, wp, h, w, variant):
    B, P, n = scores.shape
    up = F.interpolate(scores.transpose(1, 2).reshape(B, n, hp, wp), size=(h, w), mode="bilinear", align_corners=False)
    if variant == "labels":
        return up.argmax(1)
    if variant == "labels+conf":
        return up.max(1)
    return up.argmax(1), up


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-model", action="store_true")
    a = ap.parse_args()
    from ifseg_amd import hip
    dev = torch.device("cuda:0")
    lines = ["hip.seg_predict vs F.interpolate(...).argmax(1): median [min, max] microseconds over %d alternating windows of >= %.1f s"
             % (a.windows, a.window_s),
             "floor = algorithmic bytes; share = floor / time over %.1f TB/s achievable (%.1f TB/s nominal)" % (HBM_ACHIEVABLE / 1e12, HBM_NOMINAL / 1e12)]
    for (B, hp, wp, n, h, w) in SHAPES:
        s = torch.randn(B, hp * wp, n, generator=torch.Generator().manual_seed(1)).softmax(-1).to(dev)
        lb = 1 if n <= 256 else 2
        lines.append("")
        lines.append("B %d  %d x %d -> %d x %d  n %d" % (B, hp, wp, h, w, n))
        for variant, kw in (("labels", {}), ("labels+conf", {"conf": True}), ("labels+probs", {"probs": True})):
            floor = B * hp * wp * n * 4 + B * h * w * lb + (B * h * w * 4 if "conf" in kw else 0) + (B * n * h * w * 4 if "probs" in kw else 0)
            fns = [lambda: hip.seg_predict(s, hp, wp, h, w, **kw), lambda: torch_side(s, hp, wp, h, w, variant),
                   lambda: hip.seg_predict(s, hp, wp, h, w, staging_bytes=0, **kw)]
            (k, kmin, kmax), (t, tmin, tmax), (d, dmin, dmax) = alternate(fns, a.windows, a.window_s)
            lines.append("  %-13s kernel %9.1f [%9.1f, %9.1f]   torch %9.1f [%9.1f, %9.1f]   x%5.2f   floor %8.2f MB  share %5.1f %% (%4.1f %% nominal)"
                         "   direct-global path %9.1f" % (variant, k, kmin, kmax, t, tmin, tmax, t / k, floor / 1e6,
                                                          100 * floor / (k * 1e-6) / HBM_ACHIEVABLE, 100 * floor / (k * 1e-6) / HBM_NOMINAL, d))
            print(lines[-1], flush=True)
    if not a.no_model:
        from ifseg_amd.predict import Segmenter
        from ifseg_amd.tasks.mm_tasks.segmentation import SegmentationTask
        torch.manual_seed(0)
        g = torch.Generator().manual_seed(7)
        names = [torch.randint(4, 50000, (int(k),), generator=g) for k in torch.randint(1, 4, (15,), generator=g)]
        task = SegmentationTask(num_seg_tokens=15, patch_image_size=512, arch="segofa_base", category_token_ids=names)
        model = task.build_model().to(dev).eval()
        img = torch.randn(8, 3, 512, 512, generator=g).to(dev).to(torch.bfloat16)
        seg = task.build_segmenter(model)
        ni = seg.net_input(img)

        def fwd():
            with torch.no_grad():
                model(**ni)

        (c, cmin, cmax), (f, fmin, fmax) = alternate([lambda: seg(img), fwd], a.windows, a.window_s)
        lines.append("")
        lines.append("Segmenter call, SegOFA-Base, B 8, 512 x 512, 15 classes (upsample='probs', labels only): %9.1f [%9.1f, %9.1f] us;"
                     "  model forward alone %9.1f [%9.1f, %9.1f] us;  post-processing %6.1f us = %4.2f %% of the call"
                     % (c, cmin, cmax, f, fmin, fmax, c - f, 100 * (c - f) / c))
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
