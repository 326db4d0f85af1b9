"""The temperature sweep on the device (csrc/tsweep.hip: hip.seg_temperature_sweep; Segmenter.calibrate_raw) against what it
replaces, on the same device, per call as enqueued from Python.  One 512 x 683 image, K = 16 temperatures
(`predict.default_temperatures()`), n = 15 and 150 classes.

(a) the launch pair (the sweep and the small launch that adds the tiles' sums) on given grids, against
      composition   K x (hip.seg_score(labels, conf, probs=True) + hip.seg_calibration + the two proper scores in torch: the
                    true class's value gathered from the [n, H, W] probs, its log, the sum of squares, masked by the scored
                    pixels and summed in float64), written without boolean indexing so that it does not wait for the device
      (K x score)   K x hip.seg_score alone, counters only: the floor, what K label maps cost without any of the new outputs
      (unstaged)    the sweep with every tile reading global memory (staging_bytes=0)
(b) end to end on SegOFA-Base (--no-model leaves it out): `calibrate_raw` against K x `evaluate_raw(calibration=True)` on K
    Segmenters of the K temperatures, which is how a caller searched before -- one forward against K.
The variants of a row alternate window by window in one process; a window is at least 0.5 s of enqueued calls between two
device events after a warm-up; the figure is the median over the windows, [min, max] its run-to-run spread: a difference inside
the spread is no difference.  The two sides of a row are checked to agree before they are timed.

    python tools/temperature_sweep_bench.py [--windows 5] [--window-s 0.5] [--no-model] [--out profiles/temperature_sweep_bench.txt]
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


def composition(grids, hp, wp, gt, n):
    """what a caller had: per temperature the scoring launch with its [n, H, W] probs, the calibration launch, and NLL / Brier
    in torch -> (hist [K, 256, 2], sums [K, 2])"""
    from ifseg_amd import hip
    from ifseg_amd.predict import FLT_MIN
    g = gt.long()
    scored = ((g != 0) & (g != 255) & (g <= n)).double()
    t = (g - 1).clamp(0, n - 1)
    hist, sums = [], []
    for k in range(grids.shape[0]):
        _, _, labels, conf, probs = hip.seg_score(grids[k], hp, wp, gt, labels=True, conf=True, probs=True)
        hist.append(hip.seg_calibration(labels, conf, gt, n)[0].sum(0))
        pt = probs.gather(1, t[:, None])[:, 0].double()
        nll = -(pt.clamp_min(FLT_MIN).log() * scored).sum()
        brier = (((probs.double() ** 2).sum(1) - 2.0 * pt + 1.0) * scored).sum()
        sums.append(torch.stack([nll, brier]))
    return torch.stack(hist), torch.stack(sums)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.5)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ifseg_amd import hip
    from ifseg_amd.predict import default_temperatures
    dev = torch.device("cuda:0")
    temps = default_temperatures()
    K = len(temps)
    hp, wp = (H + 15) // 16, (W + 15) // 16
    lines = ["temperature sweep on the device vs what it replaces: median [min, max] microseconds over %d alternating windows of "
             ">= %.1f s" % (a.windows, a.window_s),
             "one %d x %d image, %d x %d patches, K = %d temperatures; x = composition / new" % (H, W, hp, wp, K), "",
             "hip.seg_temperature_sweep (given grids; the sweep and the launch that adds the tiles' sums)"]
    for n in CLASSES:
        g = torch.Generator().manual_seed(1)
        z = 3.0 * torch.randn(1, hp * wp, n, generator=g)
        grids = torch.stack([(z / T).softmax(-1) for T in temps]).to(dev).contiguous()
        gt = block_gt(n, g, dev)[None].contiguous()
        hist, sums, tally = hip.seg_temperature_sweep(grids, hp, wp, gt)
        want_h, want_s = composition(grids, hp, wp, gt, n)
        assert torch.equal(hist, want_h) and torch.allclose(sums, want_s, rtol=1e-9, atol=0.0) and int(tally[0]) > 0
        row(lines, "n %3d" % n,
            [lambda: hip.seg_temperature_sweep(grids, hp, wp, gt), lambda: composition(grids, hp, wp, gt, n),
             lambda: [hip.seg_score(grids[k], hp, wp, gt) for k in range(K)],
             lambda: hip.seg_temperature_sweep(grids, hp, wp, gt, staging_bytes=0)],
            ("seg_temperature_sweep", "composition", "(K x seg_score)", "(unstaged)"), a)
    if not a.no_model:
        from ifseg_amd.tasks.mm_tasks.segmentation import SegmentationTask
        lines += ["", "end to end, SegOFA-Base, one raw uint8 %d x %d image, K = %d; x = K x evaluate_raw / calibrate_raw" % (H, W, K)]
        for n in CLASSES:
            torch.manual_seed(0)
            g = torch.Generator().manual_seed(7)
            names = [torch.randint(4, 50000, (int(k),), generator=g) for k in torch.randint(1, 4, (n,), generator=g)]
            task = SegmentationTask(num_seg_tokens=n, patch_image_size=P, arch="segofa_base", category_token_ids=names)
            model = task.build_model().to(dev).eval()
            seg = task.build_segmenter(model)
            segs = [task.build_segmenter(model, temperature=T) for T in temps]
            img = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).to(dev)
            gt = block_gt(n, torch.Generator().manual_seed(1), dev)
            new = lambda: seg.calibrate_raw(img, gt, temperatures=temps)
            old = lambda: [s.evaluate_raw(img, gt, calibration=True) for s in segs]
            sweep, scores = new(), old()
            assert all(torch.equal(sweep.hist[k], scores[k].calibration.sum(0)) for k in range(K))
            row(lines, "n %3d single view" % n, [new, old], ("calibrate_raw", "K x evaluate_raw(calibration=True)"), a)
            del model, seg, segs
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
