"""The bias sweep on the device (csrc/bsweep.hip: hip.seg_score_grids; Segmenter.bias_sweep_raw) against what it replaces, on
the same device, per call as enqueued from Python.  One 512 x 683 image, K = 16 strengths
(`predict.default_bias_strengths()`), n = 15 and 150 classes.

(a) the launch on given grids (z - g_k d of one z = 3 randn: logit-like), against
      K x seg_score     K x hip.seg_score, counters only: the floor it must be compared with, what K label maps cost today
      (tsweep)          hip.seg_temperature_sweep on the same grids, whose walk it shares minus the fp64 work
      (unstaged)        the launch with every tile reading global memory (staging_bytes=0)
(b) end to end on SegOFA-Base (--no-model leaves it out): `bias_sweep_raw` against K x `evaluate_raw` on K Segmenters with
    `class_bias` set to the K rows, which is how a caller searches without it -- one forward against K.
The variants of a row alternate window by window in one process; a window is at least 0.5 s of enqueued calls between two
device events after a warm-up; the figure is the median over the windows, [min, max] its run-to-run spread: a difference inside
the spread is no difference.  The two sides of a row are checked to agree before they are timed.

    python tools/bias_sweep_bench.py [--windows 5] [--window-s 0.5] [--no-model] [--out profiles/bias_sweep_bench.txt]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from calibration_bench import block_gt
from evaluate_bench import row
from predict_tta_bench import H, P, W

CLASSES = (15, 150)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.5)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ifseg_amd import hip
    from ifseg_amd.predict import default_bias_strengths, scaled_bias
    dev = torch.device("cuda:0")
    gs = default_bias_strengths()
    K = len(gs)
    hp, wp = (H + 15) // 16, (W + 15) // 16
    lines = ["bias sweep on the device vs what it replaces: median [min, max] microseconds over %d alternating windows of "
             ">= %.1f s" % (a.windows, a.window_s),
             "one %d x %d image, %d x %d patches, K = %d strengths; x = K x seg_score / new" % (H, W, hp, wp, K), "",
             "hip.seg_score_grids (given grids, one launch)"]
    for n in CLASSES:
        g = torch.Generator().manual_seed(1)
        z = 3.0 * torch.randn(1, hp * wp, n, generator=g)
        d = torch.randn(n, generator=g)
        grids = torch.stack([z - scaled_bias(d, s) for s in gs]).to(dev).contiguous()
        gt = block_gt(n, g, dev)[None].contiguous()
        areas, tally = hip.seg_score_grids(grids, hp, wp, gt)
        want = [hip.seg_score(grids[k], hp, wp, gt)[:2] for k in range(K)]
        assert all(torch.equal(areas[k], want[k][0]) and torch.equal(tally, want[k][1]) for k in range(K)) and int(tally[0]) > 0
        row(lines, "n %3d" % n,
            [lambda: hip.seg_score_grids(grids, hp, wp, gt), lambda: [hip.seg_score(grids[k], hp, wp, gt) for k in range(K)],
             lambda: hip.seg_temperature_sweep(grids, hp, wp, gt), lambda: hip.seg_score_grids(grids, hp, wp, gt, staging_bytes=0)],
            ("seg_score_grids", "K x seg_score", "(tsweep)", "(unstaged)"), a)
    if not a.no_model:
        from ifseg_amd.tasks.mm_tasks.segmentation import SegmentationTask
        lines += ["", "end to end, SegOFA-Base, one raw uint8 %d x %d image, K = %d; x = K x evaluate_raw / bias_sweep_raw" % (H, W, K)]
        for n in CLASSES:
            torch.manual_seed(0)
            g = torch.Generator().manual_seed(7)
            names = [torch.randint(4, 50000, (int(k),), generator=g) for k in torch.randint(1, 4, (n,), generator=g)]
            task = SegmentationTask(num_seg_tokens=n, patch_image_size=P, arch="segofa_base", category_token_ids=names)
            model = task.build_model().to(dev).eval()
            d = torch.randn(n, generator=g).to(dev)
            seg = task.build_segmenter(model)
            segs = [task.build_segmenter(model, class_bias=scaled_bias(d, s, torch.zeros(n, device=dev))) for s in gs]
            img = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).to(dev)
            gt = block_gt(n, torch.Generator().manual_seed(1), dev)
            new = lambda: seg.bias_sweep_raw(img, gt, d, strengths=gs)
            old = lambda: [s.evaluate_raw(img, gt) for s in segs]
            sweep, scores = new(), old()
            assert all(torch.equal(sweep.areas[k], scores[k].areas) for k in range(K))
            row(lines, "n %3d single view" % n, [new, old], ("bias_sweep_raw", "K x evaluate_raw(class_bias)"), a)
            del model, seg, segs
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
