"""ClassMix / CutMix of two batches on the device (csrc/mix.hip: hip.mix_draw, hip.mix_apply; task.dacs_sample) against what
they replace, on the same device, per call as enqueued from Python:

  apply   the device-only torch composition: the chosen classes as a bool table per sample, gathered by the source's class,
          then three torch.where (images, target, weight).  The table is given to it ready-made.
  draw    the upstream host round trip (ClassMix / DACS): per sample `torch.unique` of the label map, the classes copied to the
          host, `numpy.random.choice` of half of them, the choice copied back.

B = 8, P = 512, fp32 and bf16 images, n = 15 and 150 classes, two source label maps each:
  piecewise   32 x 32 blocks of one class
  random      an independent class per pixel: every wave of the draw meets many classes
and `task.dacs_sample` against `train_sample` + `self_train_sample` (the two batches it mixes, unmixed) on SegOFA-Base
(--no-model leaves it out).  The variants of a row alternate window by window in one process; a window is at least 0.5 s of
enqueued calls between two device events after a warm-up; the figure is the median over the windows, [min, max] its
run-to-run spread: a difference inside the spread is no difference.  The two sides of an apply row are checked to give the
same result before they are timed.

    python tools/mix_bench.py [--windows 5] [--window-s 0.5] [--no-model] [--out profiles/mix_bench.txt]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from evaluate_bench import row

B, P = 8, 512
CLASSES = (15, 150)
SEG0 = 59457
EOS = 2


def targets(n, kind, seed, dev):
    """int64 [B, P*P + 1]: classes 0 .. n ('unknown' included), in 32 x 32 blocks or per pixel"""
    g = torch.Generator().manual_seed(seed)
    if kind == "piecewise":
        cls = torch.randint(0, n + 1, (B, P // 32, P // 32), generator=g).repeat_interleave(32, 1).repeat_interleave(32, 2)
    else:
        cls = torch.randint(0, n + 1, (B, P, P), generator=g)
    return torch.cat([cls.reshape(B, P * P) + SEG0, torch.full((B, 1), EOS)], 1).to(dev)


def torch_apply(table, si, st, sw, di, dt, dw, n):
    """table bool [B, n + 1]: the chosen classes ('unknown' never); EOS is below the offset and lands on class 0, where source
    and destination agree"""
    sel = table.gather(1, (st - SEG0).clamp_(0, n))
    return (torch.where(sel[:, :-1].reshape(B, 1, P, P), si, di), torch.where(sel, st, dt), torch.where(sel[:, :-1], sw, dw))


def host_draw(st, n, rng):
    """the upstream choice: one device round trip per sample"""
    out = []
    for b in range(st.shape[0]):
        classes = torch.unique(st[b, :-1])
        classes = classes[(classes >= SEG0) & (classes < SEG0 + n)]
        k = classes.shape[0]                                  # (a device tensor's shape is known only after the kernel ran)
        pick = rng.choice(k, (k + 1) // 2, replace=False)
        out.append(classes[torch.from_numpy(pick).to(st.device)])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.5)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ifseg_amd import hip
    dev = torch.device("cuda:0")
    mb = lambda eb, w: (B * P * P * (3 * 3 * eb + 3 * 8 + (3 if w else 0))) / 1e6
    lines = ["batch mix on the device vs what it replaces: median [min, max] microseconds over %d alternating windows of >= %.1f s"
             % (a.windows, a.window_s),
             "B = %d, P = %d, both weight planes; x = replaced / new.  Bytes an out-of-place apply moves (two batches read, one "
             "written): fp32 %.0f MB, bf16 %.0f MB" % (B, P, mb(4, True), mb(2, True)), ""]
    rng = np.random.default_rng(0)
    g = torch.Generator().manual_seed(3)
    sw, dw = (torch.randint(0, 256, (B, P * P), generator=g, dtype=torch.uint8).to(dev) for _ in range(2))
    for n in CLASSES:
        for kind in ("piecewise", "random"):
            st, dt = targets(n, kind, 1, dev), targets(n, kind, 2, dev)
            rec = hip.mix_draw(st, n, SEG0, 5, 0)
            row(lines, "draw  n %3d %-9s" % (n, kind), [lambda: hip.mix_draw(st, n, SEG0, 5, 0), lambda: host_draw(st, n, rng)],
                ("mix_draw", "unique+choice"), a)
            bits = rec[:, :8].cpu().numpy().view(np.uint32)
            table = torch.tensor([[bool((int(bits[b, c >> 5]) >> (c & 31)) & 1) and c < n for c in range(n + 1)] for b in range(B)]).to(dev)
            for dtype in (torch.float32, torch.bfloat16):
                si, di = (torch.randn(B, 3, P, P, generator=g).to(dtype).to(dev) for _ in range(2))
                got, want = hip.mix_apply(rec, si, st, di, dt, n, SEG0, src_weight=sw, dst_weight=dw), torch_apply(table, si, st, sw, di, dt, dw, n)
                assert all(torch.equal(x, y) for x, y in zip(got, want))
                row(lines, "apply n %3d %-9s %-8s" % (n, kind, str(dtype)[6:]),
                    [lambda: hip.mix_apply(rec, si, st, di, dt, n, SEG0, src_weight=sw, dst_weight=dw),
                     lambda: torch_apply(table, si, st, sw, di, dt, dw, n)], ("mix_apply", "gather+3 where"), a)
                if kind == "piecewise":
                    out = (di.clone(), dt.clone(), dw.clone())
                    row(lines, "  in place (out = destination)",
                        [lambda: hip.mix_apply(rec, si, st, out[0], out[1], n, SEG0, src_weight=sw, dst_weight=out[2], out=out),
                         lambda: hip.mix_apply(rec, si, st, di, dt, n, SEG0, src_weight=sw, dst_weight=dw)], ("in place", "out of place"), a)
    if not a.no_model:
        from ifseg_amd.tasks.mm_tasks.segmentation import SegmentationTask
        H, W, Bm, n = 512, 683, 2, 150
        lines += ["", "end to end, SegOFA-Base, n = %d, %d labelled + %d unlabelled raw uint8 %d x %d images; x = the two samples "
                  "unmixed / dacs_sample" % (n, Bm, Bm, H, W)]
        torch.manual_seed(0)
        g = torch.Generator().manual_seed(7)
        names = [torch.randint(4, 50000, (int(k),), generator=g) for k in torch.randint(1, 4, (n,), generator=g)]
        task = SegmentationTask(num_seg_tokens=n, patch_image_size=P, arch="segofa_base", category_token_ids=names)
        model = task.build_model().to(dev).eval()
        task.build_train_transform(dev, seed=1)
        imgs = [torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).to(dev) for _ in range(2 * Bm)]
        labs = [torch.randint(0, n + 1, ((H + 31) // 32, (W + 31) // 32), generator=g).repeat_interleave(32, 0).repeat_interleave(32, 1)[:H, :W]
                .to(torch.uint8).contiguous().to(dev) for _ in range(Bm)]
        kw = dict(keep=0.5, boundary=1)

        def unmixed():
            return task.train_sample(imgs[:Bm], labs, 0), task.self_train_sample(model, imgs[Bm:], 2 ** 31, confidence_weight=True, **kw)
        for mask in ("class", "box"):
            row(lines, "mask %-5s" % mask, [lambda: task.dacs_sample(model, imgs[:Bm], labs, imgs[Bm:], 0, mask=mask, **kw), unmixed],
                ("dacs_sample", "two samples"), a)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
