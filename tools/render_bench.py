"""The label map as a picture on the device (csrc/render.hip: hip.seg_render; Segmenter.render_raw) against the torch composition it
replaces, on the same device -- the demo's last lines written with tensor operations:

    colour = palette[labels.long()]                                                   # an int64 gather
    picture = (image.float() * (1 - opacity) + colour.float() * opacity).to(torch.uint8)
    r = 1:  edge = any of the eight shifted comparisons of the label map;  picture = torch.where(edge[..., None], white, picture)

-- the label map widened to int64, a [H, W, 3] gather, two float images, a cast, and for the contour eight comparisons over
the image and one more pass.  (The composition blends in fp32; at opacity 0.5 both sides give the same bytes, which is checked
before anything is timed.)

Cases: one 512 x 683 image, 15 and 150 classes, r = 0 and r = 1, opacity 0.5; the label map in blocks of 32 x 32 pixels.  The two
sides of a row alternate window by window in one process; a window is at least 0.5 s of enqueued calls between two device
events after a warm-up; the figure is the median over the windows, [min, max] its run-to-run spread: a difference inside the
spread is no difference.  floor = the bytes the launch has to move (labels, image in, picture out) over 6.3 TB/s.

    python tools/render_bench.py [--windows 5] [--window-s 0.5] [--out profiles/render_bench.txt]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from predict_bench import HBM_ACHIEVABLE, alternate

H, W = 512, 683
CLASSES = (15, 150)
OPACITY = 0.5


def make_labels(n, dev):
    g = torch.Generator().manual_seed(2)
    blocks = torch.randint(0, n, ((H + 31) // 32, (W + 31) // 32), generator=g)
    return blocks.repeat_interleave(32, 0).repeat_interleave(32, 1)[:H, :W].to(torch.uint8).contiguous().to(dev)


def torch_side(labels, image, palette, opacity, r, white):
    colour = palette[labels.long()]
    picture = (image.float() * (1 - opacity) + colour.float() * opacity).to(torch.uint8)
    if r == 0:
        return picture
    edge = torch.zeros_like(labels, dtype=torch.bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dy or dx:
                here = (slice(max(-dy, 0), H - max(dy, 0)), slice(max(-dx, 0), W - max(dx, 0)))
                there = (slice(max(dy, 0), H - max(-dy, 0)), slice(max(dx, 0), W - max(-dx, 0)))
                edge[here] |= labels[here] != labels[there]
    return torch.where(edge[..., None], white, picture)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ifseg_amd import hip
    from ifseg_amd.predict import default_palette
    dev = torch.device("cuda:0")
    floor = H * W * 7 / HBM_ACHIEVABLE * 1e6
    lines = ["hip.seg_render vs the torch composition (gather, float blend, cast, shifted comparisons): median [min, max] microseconds "
             "over %d alternating windows of >= %.1f s" % (a.windows, a.window_s),
             "one %d x %d image, opacity %.1f; x = composition / new; floor = 7 B per pixel over %.1f TB/s = %.2f us"
             % (H, W, OPACITY, HBM_ACHIEVABLE / 1e12, floor), ""]
    image = torch.randint(0, 256, (H, W, 3), generator=torch.Generator().manual_seed(1), dtype=torch.uint8).to(dev)
    white = torch.tensor([255, 255, 255], dtype=torch.uint8, device=dev)
    for n in CLASSES:
        labels, palette = make_labels(n, dev), default_palette(n).to(dev)
        out = torch.empty_like(image)
        for r in (0, 1):
            new = lambda: hip.seg_render(labels, image, palette, OPACITY, r, out=out)
            old = lambda: torch_side(labels, image, palette, OPACITY, r, white)
            assert torch.equal(new(), old())
            res = alternate([new, old], a.windows, a.window_s)
            lines.append("  n %3d r %d   " % (n, r) + "   ".join("%s %8.1f [%8.1f, %8.1f]" % (lab, m, lo, hi) for lab, (m, lo, hi)
                                                              in zip(("seg_render", "torch"), res)) + "   x%6.2f" % (res[1][0] / res[0][0]))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
