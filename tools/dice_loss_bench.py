"""The Dice auxiliary loss (csrc/dice.hip: pass A, pass B and the two-source gather), per call as enqueued from Python:

  launch  B = 8, 32 x 32 cells (512 x 512 pixels), n = 15 and 150: each new launch alone -- `hip.seg_dice_sums` (pass A + the
          reduction over a sample's tiles), pass B on given sums, the two-source gather
  loss    `hip.seg_loss_dice` (CE tiles + reduce, pass A + reduce, pass B, gather) against `hip.seg_loss` on the same logits, and
          against the torch composition on the device (`upsample_logits` + `dice_loss_reference` + cross entropy, forward and
          backward: the launches give both)
  step    `Trainer.train_step` on SegOFA-Base, B = 8, with and without `dice_weight=3.0`, one trainer per process: each variant
          runs in a child process of its own and reports its own windows (--no-model leaves it out)

The variants of a row alternate window by window in one process (the step row: one process each); a window is at least 0.5 s of
enqueued calls between two device events after a warm-up; the figure is the median over the windows, [min, max] its run-to-run
spread: a difference inside the spread is no difference.  The launches are checked against the composition before they are timed.

    python tools/dice_loss_bench.py [--windows 5] [--window-s 0.5] [--no-model] [--out profiles/dice_loss_bench.txt]
"""
import argparse
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from evaluate_bench import row
from predict_bench import alternate
from weighted_loss_bench import B, CLASSES, HP, SEG0, WP, loss_inputs

DICE_WEIGHT = 3.0


def step_child(n, dice, a):
    """one trainer in this process: the windows of `Trainer.train_step` -> "STEP median min max" on stdout"""
    from ifseg_amd.criterions import SegCriterion
    from ifseg_amd.tasks.mm_tasks import SegmentationTask
    from ifseg_amd.trainer import Trainer
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    task = SegmentationTask(num_seg_tokens=n, patch_image_size=512, arch="segofa_base")
    model = task.build_model()
    crit = SegCriterion(task, unsupervised_segmentation=False, init_seg_with_text=False, dice_weight=DICE_WEIGHT if dice else None)
    tr = Trainer(model, crit, task, device=dev)
    sm = task.synthetic_sample(B, dev, seed=200)
    sm["net_input"]["patch_images"] = sm["net_input"]["patch_images"].to(torch.bfloat16)
    (m, lo, hi), = alternate([lambda: tr.train_step([sm])], a.windows, a.window_s)
    print("STEP %.1f %.1f %.1f" % (m, lo, hi), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.5)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step-child", nargs=2, metavar=("N", "DICE"), default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step_child:
        return step_child(int(a.step_child[0]), a.step_child[1] == "1", a)
    from ifseg_amd import hip
    from ifseg_amd.criterions import SegCriterion
    from ifseg_amd.criterions.seg_criterion import dice_loss_reference, weighted_loss_reference
    dev = torch.device("cuda:0")
    lines = ["the Dice auxiliary loss: median [min, max] microseconds over %d alternating windows of >= %.1f s" % (a.windows, a.window_s),
             "B %d, %d x %d cells, dice_weight %.1f, smooth 1; x = second / first (the rows of two variants)" % (B, HP, WP, DICE_WEIGHT), ""]
    Hl, Wl = 16 * HP, 16 * WP
    for n in CLASSES:
        lp, tgt, _, _ = loss_inputs(n, dev)
        tile = torch.empty(B * HP * WP * 9 * n, device=dev)
        sp = torch.empty(B * HP * WP * (2 + 3 * n), device=dev)
        stats, dl, loss = torch.empty(2 + 3 * n, device=dev), torch.empty_like(lp), torch.empty(1, device=dev)
        bufs = {}
        both = lambda: hip.seg_loss_dice(lp, tgt, HP, WP, Hl, Wl, n, SEG0, DICE_WEIGHT, 1.0, bufs=bufs)
        plain = lambda: hip.seg_loss(lp, tgt, HP, WP, Hl, Wl, n, SEG0, tile, sp, stats, dl, loss)
        sums = lambda: hip.seg_dice_sums(lp, tgt, HP, WP, Hl, Wl, n, SEG0, bufs=bufs)
        head = hip._seg_tile_args(lp, tgt, B, HP, WP, Hl, Wl, n, SEG0, 1, 2)
        lib, p = hip.lib(), hip._ptr

        def pass_b():
            hip._check(lib.ifseg_seg_dice_tiles(*head, p(bufs["dice_sums"]), None, hip.c_float(DICE_WEIGHT), hip.c_float(1.0),
                                                p(bufs["dice_tile"]), p(bufs["dice_val"]), hip._stream()), "seg_dice_tiles")

        def gather():
            d = bufs["dl"]
            hip._check(lib.ifseg_seg_loss_gather_sum(p(bufs["tile"]), p(bufs["stats"]), p(bufs["dice_tile"]), p(bufs["dice_val"]), p(d),
                                                     hip.c_int(d.stride(1)), hip.c_ll(d.stride(0)), hip.c_int(B), hip.c_int(HP),
                                                     hip.c_int(WP), hip.c_int(n), p(bufs["loss3"]), hip._stream()), "seg_loss_gather_sum")

        lf = lp[:, :, :n].float().requires_grad_(True)

        def composition():
            lf.grad = None
            scores = SegCriterion.upsample_logits(lf, HP, WP, Hl, Wl)
            ref = weighted_loss_reference(scores, tgt, SEG0, n) + DICE_WEIGHT * dice_loss_reference(scores, tgt, SEG0, n)
            ref.backward()
            return ref

        ref = float(composition().detach())
        got = float(both()[0][0])
        assert abs(got - ref) < 2e-4 * max(1.0, abs(ref)), (got, ref)
        rel = float((bufs["dl"][:, :, :n].float() - lf.grad).norm() / lf.grad.norm())
        assert rel < 6e-3, rel
        lines.append("n %3d: loss %.6f (composition %.6f), gradient rel-L2 %.2e" % (n, got, ref, rel))
        res = alternate([sums, pass_b, gather], a.windows, a.window_s)       # three different launches: no ratio between them
        lines.append("  %-34s " % ("n %3d the new launches" % n) + "   ".join(
            "%s %9.1f [%9.1f, %9.1f]" % (lab, md, lo, hi) for lab, (md, lo, hi) in zip(("pass A + reduce", "pass B", "gather"), res)))
        print(lines[-1], flush=True)
        row(lines, "n %3d vs hip.seg_loss" % n, [both, plain], ("seg_loss_dice", "seg_loss"), a)
        row(lines, "n %3d vs torch" % n, [both, composition], ("seg_loss_dice", "upsample+references"), a)
        del lf, tile, sp, bufs, both, sums, pass_b, gather
        torch.cuda.empty_cache()

    if not a.no_model:
        lines += ["", "step: SegOFA-Base, B %d at 512 x 512, Trainer.train_step as enqueued (eager), one trainer per process" % B]
        for n in CLASSES:
            res = []
            for dice in (1, 0):
                cmd = [sys.executable, os.path.abspath(__file__), "--windows", str(a.windows), "--window-s", str(a.window_s),
                       "--step-child", str(n), str(dice)]
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
                got = [l for l in r.stdout.splitlines() if l.startswith("STEP ")]
                if r.returncode != 0 or not got:
                    raise RuntimeError("step child failed (%d):\n%s" % (r.returncode, r.stderr[-2000:]))
                res.append(tuple(float(x) for x in got[-1].split()[1:]))
            lines.append("  %-34s " % ("n %3d train_step" % n)
                         + "   ".join("%s %9.1f [%9.1f, %9.1f]" % (lab, m, lo, hi) for lab, (m, lo, hi) in zip(("dice 3.0", "plain"), res))
                         + "   x%5.2f   +%.1f us" % (res[1][0] / res[0][0], res[0][0] - res[1][0]))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
