"""Pixel-adaptive mask refinement on the device (csrc/pamr.hip: hip.pamr_affinity, hip.pamr_iterate, hip.seg_pamr;
Segmenter(pamr_iters=)) against the composition it replaces, on the same device: the published module as torch operations in
fp32 -- per dilation F.pad(mode="replicate") and a dilated 3 x 3 conv2d with the fixed kernel banks (centre minus neighbour,
the nine taps, the neighbour), .std, .mean, softmax, and per iteration the [n, 8 D, H, W] gather times the weights, summed.

Cases: one 512 x 683 image at 15 and 150 classes, with the default dilations (1, 2, 4, 8, 12, 24) and with (1,); ten
iterations.  Four blocks:
  launches     the affinity launch and one iterate launch alone, with the algorithmic bytes of each
  seg_pamr     the whole call (1 + 10 launches) against the torch composition of the same rule, whose values it matches
  dense CRF    `crf.rgb_dense_crf`, the project's other image-guided refinement, at a size both run (256 x 341, 15 classes)
  end to end   `Segmenter.segment_raw` with and without pamr_iters=10, SegOFA-Base (--no-model leaves it out)
The variants of a row alternate window by window in one process; a window is at least 0.5 s of enqueued calls between two
device events after a warm-up; the figure is the median over the windows, [min, max] its run-to-run spread: a difference inside
the spread is no difference.  A row says so where the launches lose.

    python tools/pamr_bench.py [--windows 5] [--window-s 0.5] [--no-model] [--out profiles/pamr_bench.txt]

The iterate kernel has two layouts: four rows per thread on a 16 x 64 tile (the smaller share of halo) and two rows on an
8 x 64 tile (half the registers, twice the waves); the library picks by D.  Forcing one is a laboratory switch of the library,
read once per process, so each is timed by a run of its own whose output is appended:

    IFSEG_LAB=1 IFSEG_PAMR_RPT=4 python tools/pamr_bench.py --launches-only >> profiles/pamr_bench.txt
    IFSEG_LAB=1 IFSEG_PAMR_RPT=2 python tools/pamr_bench.py --launches-only >> profiles/pamr_bench.txt
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from predict_bench import alternate
from predict_tta_bench import H, P, W

CLASSES = (15, 150)
DEFAULTS = (1, 2, 4, 8, 12, 24)
ITERS = 10
RING = [(0, 0), (0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1), (2, 2)]


def make_image(h, w, dev):
    """16-pixel blocks of random colours plus noise of +-6 grey levels"""
    g = torch.Generator().manual_seed(3)
    blocks = torch.randint(0, 256, ((h + 15) // 16, (w + 15) // 16, 3), generator=g)
    img = blocks.repeat_interleave(16, 0).repeat_interleave(16, 1)[:h, :w]
    return (img + torch.randint(-6, 7, (h, w, 3), generator=g)).clamp(0, 255).to(torch.uint8).contiguous().to(dev)


def make_values(n, h, w, dev):
    g = torch.Generator().manual_seed(4)
    grid = (3.0 * torch.randn(1, n, h // 16 + 1, w // 16 + 1, generator=g)).softmax(1)
    return F.interpolate(grid, size=(h, w), mode="bilinear", align_corners=False)[0].contiguous().to(dev)


class TorchPamr:
    """the published module on the device, fp32"""

    def __init__(self, dilations, dev):
        self.dilations = dilations
        self.k_abs, self.k_copy, self.k_std = torch.zeros(8, 1, 3, 3), torch.zeros(8, 1, 3, 3), torch.zeros(9, 1, 3, 3)
        for i, (r, c) in enumerate(RING):
            self.k_abs[i, 0, 1, 1], self.k_abs[i, 0, r, c], self.k_copy[i, 0, r, c] = 1, -1, 1
        for i in range(9):
            self.k_std[i, 0, i // 3, i % 3] = 1
        self.k_abs, self.k_copy, self.k_std = self.k_abs.to(dev), self.k_copy.to(dev), self.k_std.to(dev)

    def local(self, x, kernel):
        B, K, h, w = x.size()
        x = x.view(B * K, 1, h, w)
        affs = [F.conv2d(F.pad(x, [d] * 4, mode="replicate"), kernel, dilation=d) for d in self.dilations]
        return torch.cat(affs, 1).view(B, K, -1, h, w)

    def affinity(self, image):
        x = image.permute(2, 0, 1)[None].float()
        a = -self.local(x, self.k_abs).abs() / (1e-8 + 0.1 * self.local(x, self.k_std).std(2, keepdim=True))
        return F.softmax(a.mean(1, keepdim=True), 2)

    def iterate(self, a, mask):
        return (self.local(mask, self.k_copy) * a).sum(2)

    def __call__(self, image, values, iters):
        a, mask = self.affinity(image), values[None]
        for _ in range(iters):
            mask = self.iterate(a, mask)
        return mask.argmax(1)[0], mask[0]


def row(lines, name, fns, labels, a, note="", versus=True):
    """one row; versus: the second variant is the composition the first replaces (a ratio, and a flag where the launches lose)"""
    res = alternate(fns, a.windows, a.window_s)
    text = "  %-30s " % name + "   ".join("%s %10.1f [%10.1f, %10.1f]" % (lab, m, lo, hi) for lab, (m, lo, hi) in zip(labels, res))
    if versus and len(res) > 1:
        text += "   x%6.2f%s" % (res[1][0] / res[0][0], "   THE LAUNCHES LOSE" if res[1][0] < res[0][0] else "")
    if callable(note):
        note = note(res)
    lines.append(text + note)
    print(lines[-1], file=sys.stderr, flush=True)                     # progress; the text goes to --out / stdout at the end


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.5)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--launches-only", action="store_true", help="the first block alone (the layout comparison below)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ifseg_amd import hip
    from ifseg_amd.crf import rgb_dense_crf
    dev = torch.device("cuda:0")
    img = make_image(H, W, dev)
    lines = ["pixel-adaptive mask refinement, hip.seg_pamr vs the published module as torch operations (fp32, same device): median "
             "[min, max] microseconds per call as enqueued over %d alternating windows of >= %.1f s" % (a.windows, a.window_s),
             "one %d x %d image, %d iterations; x = composition / new" % (H, W, ITERS), "",
             "launches (alone; bytes = the algorithmic traffic: every input read once, every output written once)"]
    for dil in (DEFAULTS, (1,)):
        K = 8 * len(dil)
        w = hip.pamr_affinity(img, dil)
        row(lines, "affinity  D %d" % len(dil), [lambda: hip.pamr_affinity(img, dil)], ("affinity",), a,
            "   %6.1f MB" % ((H * W * 3 + K * H * W * 4) / 1e6))
        for n in CLASSES:
            src = make_values(n, H, W, dev)
            dst = torch.empty_like(src)
            row(lines, "iterate   D %d  n %3d" % (len(dil), n), [lambda: hip.pamr_iterate(w, src, dst, dil)], ("iterate ",), a,
                "   %6.1f MB" % ((K * H * W * 4 + 2 * n * H * W * 4) / 1e6))
    if a.launches_only:
        lines = ["", "the same launches with IFSEG_LAB=%s IFSEG_PAMR_RPT=%s (rows per thread forced: 4 = 16 x 64 tiles, 2 = 8 x 64 tiles)"
                 % (os.environ.get("IFSEG_LAB"), os.environ.get("IFSEG_PAMR_RPT"))] + lines[4:]
        sys.stdout.write("\n".join(lines) + "\n")
        return
    lines += ["", "seg_pamr (1 affinity + %d iterate launches) vs the torch composition; |diff| = the largest difference of the values" % ITERS]
    for dil in (DEFAULTS, (1,)):
        ref = TorchPamr(dil, dev)
        for n in CLASSES:
            values = make_values(n, H, W, dev)
            labels, _, out = hip.seg_pamr(values, img, ITERS, dil, probs_out=True)
            tl, tv = ref(img, values, ITERS)
            diff = (out - tv).abs().max().item()
            same = (labels.long() == tl).float().mean().item()
            row(lines, "D %d  n %3d" % (len(dil), n), [lambda: hip.seg_pamr(values, img, ITERS, dil), lambda: ref(img, values, ITERS)],
                ("seg_pamr", "torch"), a, "   |diff| %.1e  labels equal %.4f" % (diff, same))
            del tl, tv
    h2, w2, n2 = H // 2, W // 2, 15
    img2, values2 = make_image(h2, w2, dev), make_values(n2, h2, w2, dev)
    lines += ["", "against the dense CRF (crf.rgb_dense_crf, %d mean-field iterations: exact dense kernels, quadratic in the pixels), "
              "%d x %d, n %d" % (ITERS, h2, w2, n2)]
    rgb = img2.float()
    row(lines, "defaults", [lambda: hip.seg_pamr(values2, img2, ITERS, DEFAULTS), lambda: rgb_dense_crf(rgb, values2, ITERS)],
        ("seg_pamr", "dense CRF"), a)
    if not a.no_model:
        from ifseg_amd.tasks.mm_tasks.segmentation import SegmentationTask
        lines += ["", "end to end, SegOFA-Base, one raw uint8 %d x %d image: segment_raw without and with pamr_iters=%d" % (H, W, ITERS)]
        for n in CLASSES:
            torch.manual_seed(0)
            g = torch.Generator().manual_seed(7)
            names = [torch.randint(4, 50000, (int(k),), generator=g) for k in torch.randint(1, 4, (n,), generator=g)]
            task = SegmentationTask(num_seg_tokens=n, patch_image_size=P, arch="segofa_base", category_token_ids=names)
            model = task.build_model().to(dev).eval()
            plain, seg = task.build_segmenter(model), task.build_segmenter(model, pamr_iters=ITERS)
            row(lines, "n %3d" % n, [lambda: seg.segment_raw(img), lambda: plain.segment_raw(img)], ("with PAMR", "without"), a,
                lambda res: "   PAMR adds %.1f us" % (res[0][0] - res[1][0]), versus=False)
            del model, plain, seg
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
