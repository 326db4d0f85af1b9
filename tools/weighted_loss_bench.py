"""The weighted criterion path (csrc/loss.hip: the weighted instantiation of the tile kernel; csrc/trainload.hip:
hip.train_load_plane; csrc/pseudo.hip: the weight plane of hip.seg_pseudo), per call as enqueued from Python:

  loss    B = 8, 32 x 32 cells (512 x 512 pixels), n = 15 and 150: `hip.seg_loss_weighted` (tiles + reduce + gather) with a
          weight plane and class weights, against `hip.seg_loss` on the same logits and against the torch composition with the
          same weights (`upsample_logits` + `weighted_loss_reference`, forward and backward: the kernel gives both)
  plane   `hip.train_load_plane` alone, B = 8 planes of 512 x 683 to P = 512, against `hip.train_load` on the same sources
  sample  `task.self_train_sample` on SegOFA-Base with and without `confidence_weight` (--no-model leaves it out)

The variants of a row alternate window by window in one process; a window is at least 0.5 s of enqueued calls between two
device events after a warm-up; the figure is the median over the windows, [min, max] its run-to-run spread: a difference inside
the spread is no difference.  The fused loss is checked against the composition before it is timed.

    python tools/weighted_loss_bench.py [--windows 5] [--window-s 0.5] [--no-model] [--out profiles/weighted_loss_bench.txt]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from evaluate_bench import row
from predict_tta_bench import H, P, W

CLASSES = (15, 150)
B, HP, WP, SEG0 = 8, 32, 32, 1000


def loss_inputs(n, dev):
    g = torch.Generator().manual_seed(7)
    npad = (n + 7) // 8 * 8
    lp = torch.zeros(B, HP * WP + 1, npad, dtype=torch.bfloat16)
    lp[:, :, :n] = torch.randn(B, HP * WP + 1, n, generator=g) * 2
    tgt = torch.randint(0, n + 1, (B, 256 * HP * WP), generator=g) + SEG0
    tgt = torch.cat([tgt, torch.full((B, 1), 2)], 1)
    cw = torch.rand(n, generator=g) * 1.5 + 0.5
    pw = torch.randint(0, 256, (B, 256 * HP * WP), generator=g, dtype=torch.uint8)
    return lp.to(dev), tgt.to(dev), cw.to(dev), pw.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.5)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ifseg_amd import hip
    from ifseg_amd.criterions import SegCriterion
    from ifseg_amd.criterions.seg_criterion import weighted_loss_reference
    dev = torch.device("cuda:0")
    lines = ["the weighted criterion path: median [min, max] microseconds over %d alternating windows of >= %.1f s"
             % (a.windows, a.window_s),
             "loss: B %d, %d x %d cells, plane + class weights, norm \"weights\"; x = other / weighted" % (B, HP, WP), ""]
    Hl, Wl = 16 * HP, 16 * WP
    for n in CLASSES:
        lp, tgt, cw, pw = loss_inputs(n, dev)
        tile = torch.empty(B * HP * WP * 9 * n, device=dev)
        sp = torch.empty(B * HP * WP * (2 + 3 * n), device=dev)
        stats, dl, loss = torch.empty(2 + 3 * n, device=dev), torch.empty_like(lp), torch.empty(1, device=dev)
        weighted = lambda: hip.seg_loss_weighted(lp, tgt, HP, WP, Hl, Wl, n, SEG0, tile, sp, stats, dl, loss, pixel_weight=pw,
                                                 class_weight=cw, label_smoothing=0.1)
        plain = lambda: hip.seg_loss(lp, tgt, HP, WP, Hl, Wl, n, SEG0, tile, sp, stats, dl, loss, label_smoothing=0.1)
        lf = lp[:, :, :n].float().requires_grad_(True)

        def composition():
            lf.grad = None
            ref = weighted_loss_reference(SegCriterion.upsample_logits(lf, HP, WP, Hl, Wl), tgt, SEG0, n, cw, pw, 0.1)
            ref.backward()
            return ref

        ref = composition()
        weighted()
        ref = float(ref.detach())
        assert abs(float(loss) - ref) < 2e-4 * max(1.0, abs(ref)), (float(loss), ref)
        row(lines, "loss n %3d vs hip.seg_loss" % n, [weighted, plain], ("weighted", "seg_loss"), a)
        row(lines, "loss n %3d vs torch" % n, [weighted, composition], ("weighted", "upsample+reference"), a)
        del lf, tile, sp
        torch.cuda.empty_cache()

    lines += ["", "plane: B %d sources of %d x %d to P %d, records drawn; x = train_load / train_load_plane" % (B, H, W, P)]
    g = torch.Generator().manual_seed(3)
    imgs = [torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).to(dev) for _ in range(B)]
    blocks = [torch.randint(1, 16, ((H + 31) // 32, (W + 31) // 32), generator=g) for _ in range(B)]
    labs = [b.repeat_interleave(32, 0).repeat_interleave(32, 1)[:H, :W].to(torch.uint8).contiguous().to(dev) for b in blocks]
    planes = [torch.randint(0, 256, (H, W), generator=g, dtype=torch.uint8).to(dev) for _ in range(B)]
    params = hip.train_draw(labs, P, 15, 1, 0)
    ptab, ltab = hip._train_table(None, planes), hip._train_table(imgs, labs)
    out_p = torch.empty(B, P * P, dtype=torch.uint8, device=dev)
    row(lines, "plane, table given", [lambda: hip.train_load_plane(planes, params, P, out=out_p, table=ptab),
                                     lambda: hip.train_load(imgs, labs, params, P, 15, SEG0, table=ltab)],
        ("train_load_plane", "train_load"), a)
    row(lines, "plane, table built per call", [lambda: hip.train_load_plane(planes, params, P, out=out_p),
                                              lambda: hip.train_load(imgs, labs, params, P, 15, SEG0)],
        ("train_load_plane", "train_load"), a)

    if not a.no_model:
        from ifseg_amd.tasks.mm_tasks.segmentation import SegmentationTask
        lines += ["", "sample: SegOFA-Base, B %d raw uint8 %d x %d photographs, keep 0.5, boundary 1; x = plain / confidence_weight"
                  % (B, H, W)]
        for n in CLASSES:
            torch.manual_seed(0)
            names = [torch.randint(4, 50000, (int(k),), generator=g) for k in torch.randint(1, 4, (n,), generator=g)]
            task = SegmentationTask(num_seg_tokens=n, patch_image_size=P, arch="segofa_base", category_token_ids=names)
            model = task.build_model().to(dev).eval()
            task.build_train_transform(dev, seed=1)
            kw = dict(keep=0.5, boundary=1)
            row(lines, "n %3d self_train_sample" % n, [lambda: task.self_train_sample(model, imgs, 0, confidence_weight=True, **kw),
                                                       lambda: task.self_train_sample(model, imgs, 0, **kw)],
                ("confidence_weight", "plain"), a)
            del model
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
