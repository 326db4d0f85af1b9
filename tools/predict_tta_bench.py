"""hip.seg_predict_views (csrc/predict.hip) against the composition a user had before it, on the same device: per view

    hip.seg_predict(scores_k [flipped back on the grid], hp_k, wp_k, h, w, probs=True)[2]

then K - 1 torch adds, one multiply by 1 / K and `argmax(1)` -- K tensors [n, h, w] written and read again.  The un-mirroring of
the composition is not timed (the grids are flipped beforehand), so the comparison favours it.

Cases: 150 classes, one 512 x 683 image, P = 512: the six ratios 0.5 .. 1.75 with flip (K = 12, "ms+flip"), and the flip-only
ensemble (K = 2).  Variants: labels only, and labels + probs (what the CRF takes).  Both sides alternate window by window in
one process; a window is at least 0.5 s of enqueued calls between two device events after a warm-up; the figure is the
median over the windows.  Every row carries the bytes each side moves through device memory by its algorithm: the kernel reads
the K grids and writes the label map (+ probs); the composition writes K [n, h, w] tensors, reads and writes them again in the
adds and the multiply, and reads the mean in the argmax.

    python tools/predict_tta_bench.py [--windows 5] [--window-s 0.5] [--out profiles/predict_tta_bench.txt]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from predict_bench import alternate

N, H, W, P = 150, 512, 683, 512
CASES = [("ms+flip", (0.5, 0.75, 1.0, 1.25, 1.5, 1.75), True), ("flip only", (1.0,), True)]


def make_views(scales, flip, dev):
    from ifseg_amd.imageio import eval_size, view_list
    g = torch.Generator().manual_seed(1)
    views = []
    for ratio, flipped in view_list(scales, flip):
        oh, ow = eval_size(H, W, P, ratio)
        hp, wp = (oh + 15) // 16, (ow + 15) // 16
        views.append((torch.randn(1, hp * wp, N, generator=g).softmax(-1).to(dev), hp, wp, flipped))
    return views


def composition(plain, want_probs):
    """the parent commit's way: `plain` holds the grids already un-mirrored"""
    from ifseg_amd import hip
    total = None
    for s, hp, wp in plain:
        p = hip.seg_predict(s, hp, wp, H, W, probs=True)[2]
        total = p if total is None else total.add_(p)
    total.mul_(1.0 / len(plain))
    labels = total.argmax(1)
    return (labels, total) if want_probs else labels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ifseg_amd import hip
    dev = torch.device("cuda:0")
    lines = ["hip.seg_predict_views vs K x hip.seg_predict(probs=True) + adds + argmax: median [min, max] microseconds over %d "
             "alternating windows of >= %.1f s" % (a.windows, a.window_s),
             "n %d, one %d x %d image, P %d; MB = bytes the algorithm moves through device memory" % (N, H, W, P)]
    plane = N * H * W * 4
    for name, scales, flip in CASES:
        views = make_views(scales, flip, dev)
        K = len(views)
        plain = [(s.view(1, hp, wp, N).flip(2).reshape(1, hp * wp, N).contiguous() if f else s, hp, wp) for s, hp, wp, f in views]
        grids = sum(s.numel() * 4 for s, *_ in views)
        # the two sides compute the same labels (up to the order of the additions: compare the values)
        pk = hip.seg_predict_views(views, H, W, probs=True)[2]
        pc = composition(plain, True)[1]
        lines.append("")
        lines.append("%s: K %d, grids %s, %.2f MB of scores; max |kernel - composition| = %.2e"
                     % (name, K, " ".join("%dx%d" % (hp, wp) for _, hp, wp, _ in views), grids / 1e6, (pk - pc).abs().max().item()))
        for variant, want in (("labels", False), ("labels+probs", True)):
            kernel_bytes = grids + H * W + (plane if want else 0)
            # K seg_predict: grids read, K planes written; K - 1 adds: 2 reads + 1 write each; multiply: read + write;
            # argmax: one read + the label map (int64)
            comp_bytes = grids + K * plane + (K - 1) * 3 * plane + 2 * plane + plane + H * W * 8
            fns = [lambda: hip.seg_predict_views(views, H, W, probs=want), lambda: composition(plain, want),
                   lambda: hip.seg_predict_views(views, H, W, probs=want, staging_bytes=0)]
            (k, kmin, kmax), (c, cmin, cmax), (d, dmin, dmax) = alternate(fns, a.windows, a.window_s)
            lines.append("  %-13s kernel %9.1f [%9.1f, %9.1f] %8.2f MB   composition %9.1f [%9.1f, %9.1f] %8.2f MB   x%6.2f"
                         "   direct-global path %9.1f" % (variant, k, kmin, kmax, kernel_bytes / 1e6, c, cmin, cmax, comp_bytes / 1e6,
                                                          c / k, d))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
