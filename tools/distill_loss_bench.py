"""The distillation term (csrc/distill.hip: the KD tile pass, its reduction and the three-source gather), per call as enqueued
from Python:

  launch  B = 8, 32 x 32 cells (512 x 512 pixels), n = 15 and 150, T = 2: each KD launch alone -- the tile pass, the reduction
          of the per-tile pairs, the three-source gather (CE + KD) -- and `hip.seg_loss`'s tile launch for scale
  loss    `hip.seg_loss_distill` (CE tiles + reduce, KD tiles + reduce, gather) against `hip.seg_loss` on the same logits, and
          against the torch composition on the device (two `upsample_logits`, `distill_loss_reference` + cross entropy, forward
          and backward: the launches give both)
  step    `Trainer.train_step` on SegOFA-Base, B = 8, with and without `distill_weight`, teacher logits resident in the sample,
          one trainer per process: each variant runs in a child process of its own and reports its own windows
  teacher `task.distill_sample` with a second SegOFA-Base in the process (a second engine: its four streams share the hardware
          queues with the student's), alone and followed by the `train_step` it feeds, in a child of its own
          (--no-model leaves step and teacher out)

The variants of a row alternate window by window in one process (the step rows: one process each); a window is at least 0.5 s of
enqueued calls between two device events after a warm-up; the figure is the median over the windows, [min, max] its run-to-run
spread: a difference inside the spread is no difference.  The launches are checked against the composition before they are timed.

    python tools/distill_loss_bench.py [--windows 5] [--window-s 0.5] [--no-model] [--out profiles/distill_loss_bench.txt]
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

WEIGHT, T = 1.0, 2.0


def teacher_inputs(n, lp):
    """bf16(student + 0.5 randn) in the student's layout, NaN in the padding columns and the eos row"""
    g = torch.Generator().manual_seed(23 + n)
    te = torch.full(tuple(lp.shape), float("nan"), dtype=torch.bfloat16, device=lp.device)
    noise = (0.5 * torch.randn(B, HP * WP, n, generator=g)).to(lp.device)
    te[:, :HP * WP, :n] = (lp[:, :HP * WP, :n].float() + noise).to(torch.bfloat16)
    return te


def step_child(n, mode, a):
    """one trainer in this process: the windows of `Trainer.train_step` -> "STEP median min max" lines on stdout.
    mode: plain | kd (teacher logits resident in the sample) | teacher (a second model labels the sample before every step)"""
    from ifseg_amd.criterions import SegCriterion
    from ifseg_amd.tasks.mm_tasks import SegmentationTask
    from ifseg_amd.trainer import Trainer
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    task = SegmentationTask(num_seg_tokens=n, patch_image_size=512, arch="segofa_base")
    model = task.build_model()
    crit = SegCriterion(task, unsupervised_segmentation=False, init_seg_with_text=False,
                        distill_weight=None if mode == "plain" else WEIGHT, distill_temperature=T)
    tr = Trainer(model, crit, task, device=dev)
    sm = task.synthetic_sample(B, dev, seed=200)
    sm["net_input"]["patch_images"] = sm["net_input"]["patch_images"].to(torch.bfloat16)
    if mode == "teacher":
        torch.manual_seed(1)
        teacher = task.build_model().to(dev)
        label = lambda: task.distill_sample(sm, model, teacher=teacher)
        both = lambda: tr.train_step([label()])
        both()
        for fn in (label, both):
            (m, lo, hi), = alternate([fn], a.windows, a.window_s)
            print("STEP %.1f %.1f %.1f" % (m, lo, hi), flush=True)
        return
    if mode == "kd":
        g = torch.Generator().manual_seed(5)
        te = torch.full((B, HP * WP + 1, (n + 7) // 8 * 8), float("nan"), dtype=torch.bfloat16)
        te[:, :HP * WP, :n] = (2.0 * torch.randn(B, HP * WP, n, generator=g)).to(torch.bfloat16)
        sm["teacher_logits"] = te.to(dev)
    (m, lo, hi), = alternate([lambda: tr.train_step([sm])], a.windows, a.window_s)
    print("STEP %.1f %.1f %.1f" % (m, lo, hi), flush=True)


def run_child(n, mode, a):
    cmd = [sys.executable, os.path.abspath(__file__), "--windows", str(a.windows), "--window-s", str(a.window_s),
           "--step-child", str(n), mode]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    got = [l for l in r.stdout.splitlines() if l.startswith("STEP ")]
    if r.returncode != 0 or not got:
        raise RuntimeError("step child failed (%d):\n%s" % (r.returncode, r.stderr[-2000:]))
    return [tuple(float(x) for x in l.split()[1:]) for l in got]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.5)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step-child", nargs=2, metavar=("N", "MODE"), default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step_child:
        return step_child(int(a.step_child[0]), a.step_child[1], a)
    from ifseg_amd import hip
    from ifseg_amd.criterions import SegCriterion
    from ifseg_amd.criterions.seg_criterion import distill_loss_reference, weighted_loss_reference
    dev = torch.device("cuda:0")
    lines = ["the distillation term: median [min, max] microseconds over %d alternating windows of >= %.1f s" % (a.windows, a.window_s),
             "B %d, %d x %d cells, distill_weight %.1f, T %.1f, mask \"valid\"; x = second / first (the rows of two variants)"
             % (B, HP, WP, WEIGHT, T), ""]
    Hl, Wl = 16 * HP, 16 * WP
    for n in CLASSES:
        lp, tgt, _, _ = loss_inputs(n, dev)
        te = teacher_inputs(n, lp)
        tile = torch.empty(B * HP * WP * 9 * n, device=dev)
        sp = torch.empty(B * HP * WP * (2 + 3 * n), device=dev)
        stats, dl, loss = torch.empty(2 + 3 * n, device=dev), torch.empty_like(lp), torch.empty(1, device=dev)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        bufs = {}
        both = lambda: hip.seg_loss_distill(lp, te, tgt, HP, WP, Hl, Wl, n, SEG0, WEIGHT, T, bufs=bufs)
        plain = lambda: hip.seg_loss(lp, tgt, HP, WP, Hl, Wl, n, SEG0, tile, sp, stats, dl, loss)
        lib, p = hip.lib(), hip._ptr

        def kd_tiles():
            hip._check(lib.ifseg_seg_distill_tiles(
                p(lp), hip.c_int(lp.stride(1)), hip.c_ll(lp.stride(0)), p(te), hip.c_int(te.stride(1)), hip.c_ll(te.stride(0)), p(tgt),
                hip.c_ll(tgt.stride(0)), hip.c_int(B), hip.c_int(HP), hip.c_int(WP), hip.c_int(Hl), hip.c_int(Wl), hip.c_int(n),
                hip.c_ll(SEG0), hip.c_ll(1), hip.c_ll(2), hip.c_float(T), hip.c_int(0), p(bufs["kd_tile"]), p(bufs["kd_part"]),
                hip._stream()), "seg_distill_tiles")

        def kd_reduce():
            hip.reduce_parts(bufs["kd_part"], bufs["kd_stats"], 1, B * HP * WP, 2)

        def gather():
            hip._seg_gather(bufs, True, False, (WEIGHT, T), B, HP, WP, n)

        def ce_tiles():
            hip._check(lib.ifseg_seg_loss_tiles(
                p(lp), hip.c_int(lp.stride(1)), hip.c_ll(lp.stride(0)), p(tgt), hip.c_ll(tgt.stride(0)), hip.c_int(B), hip.c_int(HP),
                hip.c_int(WP), hip.c_int(Hl), hip.c_int(Wl), hip.c_int(n), hip.c_ll(SEG0), hip.c_ll(1), hip.c_ll(2), p(tile), p(sp),
                p(bad), hip.c_float(0.0), hip._stream()), "seg_loss_tiles")

        lf = lp[:, :, :n].float().requires_grad_(True)

        def composition():
            lf.grad = None
            scores = SegCriterion.upsample_logits(lf, HP, WP, Hl, Wl)
            t_up = SegCriterion.upsample_logits(te[:, :, :n].float(), HP, WP, Hl, Wl)
            ref = weighted_loss_reference(scores, tgt, SEG0, n) \
                + WEIGHT * distill_loss_reference(scores[:, :Hl * Wl], t_up[:, :Hl * Wl], tgt, SEG0, n, T)
            ref.backward()
            return ref

        ref = float(composition().detach())
        got = float(both()[0][0])
        assert abs(got - ref) < 2e-4 * max(1.0, abs(ref)), (got, ref)
        rel = float((bufs["dl"][:, :, :n].float() - lf.grad).norm() / lf.grad.norm())
        assert rel < 6e-3, rel
        lines.append("n %3d: loss %.6f (composition %.6f; KD term %.6f), gradient rel-L2 %.2e" % (n, got, ref, float(bufs["loss4"][3]), rel))
        res = alternate([kd_tiles, kd_reduce, gather, ce_tiles], a.windows, a.window_s)     # different launches: no ratio between them
        lines.append("  %-34s " % ("n %3d the launches" % n) + "   ".join(
            "%s %9.1f [%9.1f, %9.1f]" % (lab, md, lo, hi)
            for lab, (md, lo, hi) in zip(("KD tiles", "KD reduce", "gather3", "(seg_loss tiles)"), res))
            + "   KD tiles / seg_loss tiles x%5.2f" % (res[0][0] / res[3][0]))
        print(lines[-1], flush=True)
        row(lines, "n %3d vs hip.seg_loss" % n, [both, plain], ("seg_loss_distill", "seg_loss"), a)
        row(lines, "n %3d vs torch" % n, [both, composition], ("seg_loss_distill", "2 x upsample+references"), a)
        del lf, tile, sp, bufs, both, kd_tiles, kd_reduce, gather, ce_tiles
        torch.cuda.empty_cache()

    if not a.no_model:
        lines += ["", "step: SegOFA-Base, B %d at 512 x 512, Trainer.train_step as enqueued (eager), one trainer per process; "
                      "teacher logits resident in the sample" % B]
        plain_ms = {}
        for n in CLASSES:
            res = [run_child(n, mode, a)[0] for mode in ("kd", "plain")]
            plain_ms[n] = res[1][0]
            lines.append("  %-34s " % ("n %3d train_step" % n)
                         + "   ".join("%s %9.1f [%9.1f, %9.1f]" % (lab, m, lo, hi) for lab, (m, lo, hi) in zip(("distill 1.0", "plain"), res))
                         + "   x%5.2f   +%.1f us" % (res[1][0] / res[0][0], res[0][0] - res[1][0]))
            print(lines[-1], flush=True)
        lines += ["", "teacher: a second SegOFA-Base in the process labels the sample (task.distill_sample: one eval forward + a clone)"]
        for n in CLASSES:
            label, both = run_child(n, "teacher", a)
            lines.append("  %-34s " % ("n %3d second model" % n)
                         + "   ".join("%s %9.1f [%9.1f, %9.1f]" % (lab, m, lo, hi)
                                      for lab, (m, lo, hi) in zip(("distill_sample", "distill_sample + train_step"), (label, both)))
                         + "   +%.1f us on the plain step" % (both[0] - plain_ms[n]))
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
