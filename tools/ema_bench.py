"""The teacher averaged inside the optimizer launch (csrc/optim.hip: hip.adam_ema_step, hip.ema_swap; Trainer(store_ema=True))
against what it replaces, on the same device, per call as enqueued from Python:

  arena       random arenas of SegOFA-Base's trainable size: `hip.adam_step` alone (30 bytes per parameter), `hip.adam_ema_step`
              (40), and `hip.adam_step` followed by the torch composition of fairseq's two lines on the arena --
                  e32.mul_(d).add_(p16.float(), alpha=r); e16.copy_(e32)
              -- three more kernels and a bf16 -> fp32 temporary
  swap        `hip.ema_swap` (24 bytes per parameter) against three `copy_` through a temporary, for both precisions
  train_step  SegOFA-Base, B = 8, 512 x 512 (bench.py's headline shape, --no-model leaves it out): `Trainer.train_step` with
              the plain launch (off-updates of ema_update_freq) and with the teacher stepped on every update, on ONE trainer
The variants of a row alternate window by window in one process; a window is at least 0.5 s of enqueued calls between two
device events after a warm-up; the figure is the median over the windows, [min, max] its run-to-run spread: a difference inside
the spread is no difference.

    python tools/ema_bench.py [--windows 5] [--window-s 0.5] [--no-model] [--out profiles/ema_bench.txt]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from evaluate_bench import row

N_TRAIN = 109_327_656       # SegOFA-Base's trainable parameters (tests/test_surface_cpu.py)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.5)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ifseg_amd import hip
    from ifseg_amd.ema import ema_scalars
    dev = torch.device("cuda:0")
    n = (N_TRAIN + 7) // 8 * 8
    lines = ["the EMA teacher in the optimizer launch vs the torch composition: median [min, max] microseconds over %d alternating "
             "windows of >= %.1f s" % (a.windows, a.window_s),
             "arenas of %d elements (SegOFA-Base's trainable parameters); x = second / first" % n, ""]
    p32, m, v = torch.randn(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    g = (torch.randn(n, device=dev) * 1e-3).to(torch.bfloat16)
    p16 = p32.to(torch.bfloat16)
    e32, e16 = p32.clone(), p16.clone()
    ss = torch.ones(1, device=dev)
    d, r = ema_scalars(0.9999)
    step = [0]

    def adam():
        step[0] += 1
        hip.adam_step(p32, g, m, v, p16, 1e-4, 0.9, 0.999, 1e-8, 0.01, step[0], 1.0, 1.0, ss)

    def fused():
        step[0] += 1
        hip.adam_ema_step(p32, g, m, v, p16, e32, e16, 1e-4, 0.9, 0.999, 1e-8, 0.01, step[0], d, r, 1.0, 1.0, ss)

    def composed():
        adam()
        e32.mul_(d).add_(p16.float(), alpha=r)
        e16.copy_(e32)

    row(lines, "adam_ema_step / adam_step", [fused, adam], ("adam_ema_step", "adam_step"), a)
    row(lines, "adam_ema_step / adam_step + torch", [fused, composed], ("adam_ema_step", "adam_step + torch"), a)

    def swap_torch():
        for x, y in ((p32, e32), (p16, e16)):
            t = x.clone()
            x.copy_(y)
            y.copy_(t)

    row(lines, "ema_swap / three copies", [lambda: hip.ema_swap(p32, p16, e32, e16), swap_torch], ("ema_swap", "3 x copy_"), a)
    del p32, m, v, g, p16, e32, e16
    torch.cuda.empty_cache()
    if not a.no_model:
        from ifseg_amd.criterions import SegCriterion
        from ifseg_amd.tasks.mm_tasks import SegmentationTask
        from ifseg_amd.trainer import Trainer
        # ONE trainer for both sides: a second engine in the process brings four more streams onto the same hardware queues and
        # its steps serialise against them (28.3 against 16.2 ms per step when the two sides were two trainers) -- a cost of
        # the measurement, not of the teacher.  "plain" is this trainer on off-updates of ema_update_freq, which launch
        # hip.adam_step exactly as a trainer without store_ema does.
        lines += ["", "Trainer.train_step, SegOFA-Base, B = 8, 512 x 512, 15 classes (eager, trunk prefetch on), one trainer: every "
                  "update an off-update of", "ema_update_freq (the plain hip.adam_step launch) against every update stepping the "
                  "teacher; x = store_ema / plain"]
        torch.manual_seed(0)
        task = SegmentationTask(num_seg_tokens=15, patch_image_size=512, arch="segofa_base")
        tr = Trainer(task.build_model(), SegCriterion(task, unsupervised_segmentation=False, init_seg_with_text=False), task,
                     device=dev, lazy_logs=True, store_ema=True)
        ring = [task.synthetic_sample(8, dev, seed=1234 + 7919 * j) for j in range(2)]
        for s in ring:
            s["net_input"]["patch_images"] = s["net_input"]["patch_images"].to(torch.bfloat16)
        k = [0]

        def one(freq):
            k[0] += 1
            tr.ema.update_freq, tr.ema.counter = freq, 0
            tr.train_step([ring[k[0] % 2]], prefetch=[ring[(k[0] + 1) % 2]])
        row(lines, "train_step", [lambda: one(1 << 30), lambda: one(1)], ("plain", "store_ema"), a)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
