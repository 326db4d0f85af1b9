"""The OHEM pixel sampler (csrc/ohem.hip: hip.seg_hardness, hip.ohem_select), per call as enqueued from Python:

  hardness  B = 8, 32 x 32 cells (512 x 512 pixels), n = 15 and 150: `hip.seg_hardness` against `hip.seg_loss` (tiles + reduce +
            gather: the kernel whose front half it is) on the same logits
  select    `hip.ohem_select` alone on that plane (four launches), thresh 0.7, min_kept 100000
  pair      the two stages against the torch composition they replace: `upsample_logits`, softmax, gather, `sort` of the valid
            values, compare -- on the device, and with the one read-back (the k-th index) the composition needs
  step      `Trainer.train_step` on SegOFA-Base, B = 8, with and without `ohem_thresh=0.7` (--no-model leaves it out)

The variants of a row alternate window by window in one process; a window is at least 0.5 s of enqueued calls between two
device events after a warm-up; the figure is the median over the windows, [min, max] its run-to-run spread: a difference inside
the spread is no difference.  The pair is checked against the specifications' info before it is timed.

    python tools/ohem_bench.py [--windows 5] [--window-s 0.5] [--no-model] [--out profiles/ohem_bench.txt]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from evaluate_bench import row

CLASSES = (15, 150)
B, HP, WP, SEG0 = 8, 32, 32, 1000
THRESH, MIN_KEPT = 0.7, 100000


def inputs(n, dev):
    """weighted_loss_bench's logits and targets, with a bonus at the label of each cell's centre pixel so that p spreads over
    (0, 1) and both sides of thresh are populated"""
    g = torch.Generator().manual_seed(7)
    npad = (n + 7) // 8 * 8
    P = HP * WP
    logits = torch.randn(B, P + 1, n, generator=g) * 2
    tgt = torch.randint(0, n + 1, (B, 256 * P), generator=g)
    t2 = tgt.reshape(B, HP, 16, WP, 16)[:, :, 8, :, 8].reshape(B, P)
    ok = t2 < n
    b, c = torch.nonzero(ok, as_tuple=True)
    logits[b, c, t2[ok]] += 6.0
    lp = torch.zeros(B, P + 1, npad, dtype=torch.bfloat16)
    lp[:, :, :n] = logits
    tgt = torch.cat([tgt + SEG0, torch.full((B, 1), 2)], 1)
    return lp.to(dev), tgt.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.5)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ifseg_amd import hip
    from ifseg_amd.criterions import SegCriterion
    from ifseg_amd.criterions.seg_criterion import hardness_reference, ohem_reference
    dev = torch.device("cuda:0")
    Hl, Wl = 16 * HP, 16 * WP
    lines = ["the OHEM pixel sampler: median [min, max] microseconds over %d alternating windows of >= %.1f s" % (a.windows, a.window_s),
             "B %d, %d x %d cells, thresh %.1f, min_kept %d; x = other / first" % (B, HP, WP, THRESH, MIN_KEPT), ""]
    for n in CLASSES:
        lp, tgt = inputs(n, dev)
        tile = torch.empty(B * HP * WP * 9 * n, device=dev)
        sp = torch.empty(B * HP * WP * (2 + 3 * n), device=dev)
        stats, dl, loss = torch.empty(2 + 3 * n, device=dev), torch.empty_like(lp), torch.empty(1, device=dev)
        hard = torch.empty(B, Hl * Wl, device=dev)
        plane = torch.empty(B, Hl * Wl, dtype=torch.uint8, device=dev)
        info, work = torch.empty(4, dtype=torch.int64, device=dev), hip.ohem_workspace(dev)
        hardness = lambda: hip.seg_hardness(lp, tgt, HP, WP, Hl, Wl, n, SEG0, out=hard)
        select = lambda: hip.ohem_select(hard, THRESH, MIN_KEPT, out=plane, info=info, work=work)
        seg_loss = lambda: hip.seg_loss(lp, tgt, HP, WP, Hl, Wl, n, SEG0, tile, sp, stats, dl, loss)
        lf = lp[:, :, :n].float()
        body = tgt[:, :-1]

        def pair():
            hardness()
            return select()

        def composition(read_back=True):
            scores = SegCriterion.upsample_logits(lf, HP, WP, Hl, Wl)[:, :-1]
            valid = (body >= SEG0) & (body < SEG0 + n)
            p = torch.softmax(scores, -1).gather(2, (body - SEG0).clamp(0, n - 1).unsqueeze(-1)).squeeze(-1)
            srt = torch.where(valid, p, torch.full_like(p, 2.0)).reshape(-1).sort().values
            nv = valid.sum()
            k = torch.minimum(torch.full_like(nv, MIN_KEPT * B), nv - 1).clamp_min(0)
            kth = srt[int(k)] if read_back else srt.gather(0, k.reshape(1))[0]
            tau = torch.maximum(kth, kth.new_tensor(THRESH))
            return (valid & (p < tau)).to(torch.uint8) * 255

        with torch.no_grad():
            pair()
            want = ohem_reference(hardness_reference(SegCriterion.upsample_logits(lf, HP, WP, Hl, Wl), tgt, SEG0, n), THRESH, MIN_KEPT)[1]
            assert int(info[0]) == int(want[0]) and abs(int(info[1]) - int(want[1])) <= 0.01 * int(want[0]), (info.tolist(), want.tolist())
            lines.append("n %3d: valid %d, kept %d, tau %.6f" % (n, int(info[0]), int(info[1]),
                                                               float(info[2:3].to(torch.int32).view(torch.float32))))
            row(lines, "n %3d hardness vs hip.seg_loss" % n, [hardness, seg_loss], ("seg_hardness", "seg_loss"), a)
            row(lines, "n %3d select alone" % n, [select, hardness], ("ohem_select", "seg_hardness"), a)
            row(lines, "n %3d pair vs torch" % n, [pair, composition, lambda: composition(False)],
                ("pair", "torch + read-back", "torch on device"), a)
        del lf, tile, sp, hard, plane
        torch.cuda.empty_cache()

    if not a.no_model:
        from ifseg_amd.tasks.mm_tasks import SegmentationTask
        from ifseg_amd.trainer import Trainer
        lines += ["", "step: SegOFA-Base, B %d at 512 x 512, Trainer.train_step as enqueued (eager); x = plain / ohem" % B]
        for n in CLASSES:
            steps = []
            for thresh in (THRESH, None):
                torch.manual_seed(0)
                task = SegmentationTask(num_seg_tokens=n, patch_image_size=512, arch="segofa_base")
                model = task.build_model()
                crit = SegCriterion(task, unsupervised_segmentation=False, init_seg_with_text=False, ohem_thresh=thresh)
                tr = Trainer(model, crit, task, device=dev)
                sm = task.synthetic_sample(B, dev, seed=200)
                sm["net_input"]["patch_images"] = sm["net_input"]["patch_images"].to(torch.bfloat16)
                steps.append(lambda tr=tr, sm=sm: tr.train_step([sm]))
            row(lines, "n %3d train_step" % n, steps, ("ohem 0.7", "plain"), a)
            del steps, tr, model
            torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
