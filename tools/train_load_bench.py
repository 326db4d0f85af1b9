"""What feeding the supervised step from raw data costs: the training transform (ifseg_amd/augment.py, csrc/trainload.hip) alone,
and `Trainer.train_step` of the headline model (SegOFA-Base, batch 8, 512 x 512, 15 classes) with a FRESH `task.train_sample`
every step against a ring of PRE-BUILT samples, all in one process on one GPU, the variants alternating round by round.

  ring    the batch of every step comes from a ring of samples built once by `task.train_sample` (what bench.py times, with
          random tensors in their place)
  fresh   every step builds a batch from the raw sources: two table copies, `ifseg_train_draw`, `ifseg_train_load`
Both hand the trainer the next step's batch for its trunk prefetch; `fresh` builds that batch one step ahead, as a loader would.

The sources are synthetic uint8 images and label maps of COCO-like shapes, resident on the device (decoding and the copy of
the raw bytes are the loader's business, not this tool's).  The kernels alone are timed with device events over `iters` eager
calls; bytes = what the launch writes (patch_images + target), the figure the kernels of this layout are compared by -- the
source taps (12 bytes per pixel from LDS or L2, one label byte) are not counted.  Step times are host clocks around `steps`
enqueued updates ending in a device synchronise.

    python tools/train_load_bench.py [--steps 40] [--rounds 3] [--out profiles/train_load_bench.txt]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

SHAPES = [(480, 640), (375, 500), (640, 427), (426, 640), (500, 375), (640, 480), (333, 500), (480, 640)]     # (H0, W0)


def sources(B, nseg, dev, seed=1):
    """uint8 images (noise) and raw label maps (a coarse random class map, nearest-upscaled: blobs of some
    tens of pixels, raw values 0 .. nseg, 0 = 'unknown')"""
    g = torch.Generator().manual_seed(seed)
    imgs, labs = [], []
    for b in range(B):
        H0, W0 = SHAPES[b % len(SHAPES)]
        imgs.append(torch.randint(0, 256, (H0, W0, 3), generator=g, dtype=torch.uint8).to(dev))
        coarse = torch.randint(0, nseg + 1, (1, 1, 6, 8), generator=g).float()
        labs.append(torch.nn.functional.interpolate(coarse, size=(H0, W0), mode="nearest")[0, 0].to(torch.uint8).to(dev))
    return imgs, labs


def event_time(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def kernels_alone(lines, tf, imgs, labs, iters=200):
    from ifseg_amd import hip
    B, P = len(imgs), tf.P
    params = tf._draw(labs, 0)
    ks = params[:, 4].tolist()
    out = torch.empty(B, 3, P, P, dtype=tf.dtype, device=tf.device)
    tgt = torch.empty(B, P * P + 1, dtype=torch.long, device=tf.device)
    us_draw = event_time(lambda: tf._draw(labs, 0), iters)
    us_load = event_time(lambda: hip.train_load(imgs, labs, params, P, tf.nseg, tf.seg_id_offset, tf.mean, tf.std, False, True,
                                                tf.dtype, out=out, target=tgt), iters)
    us_direct = event_time(lambda: hip.train_load(imgs, labs, params, P, tf.nseg, tf.seg_id_offset, tf.mean, tf.std, False, True,
                                                  tf.dtype, staging_bytes=0, out=out, target=tgt), iters)
    us_both = event_time(lambda: tf(imgs, labs, 0), iters)
    nbytes = B * (3 * P * P * out.element_size() + (P * P + 1) * 8)
    taps = 10 * B * P * P
    name = {torch.float32: "fp32", torch.bfloat16: "bf16"}[tf.dtype]
    lines.append("B %d  P %d  %s  crop candidates taken: %s" % (B, P, name, ks))
    lines.append("  train_draw  (table copy + memset + 1 launch, %d workgroups): %8.1f us / batch   %5.1f M label taps  %6.1f G taps/s"
                 % (10 * B, us_draw, taps / 1e6, taps / us_draw / 1e3))
    lines.append("  train_load  (table copy + 1 launch), staged:                %8.1f us / batch   %5.1f MB written   %7.1f GB/s"
                 % (us_load, nbytes / 1e6, nbytes / us_load / 1e3))
    lines.append("  train_load, direct-global (staging limit 0):                %8.1f us / batch   %5.1f MB written   %7.1f GB/s"
                 % (us_direct, nbytes / 1e6, nbytes / us_direct / 1e3))
    lines.append("  draw + load as TrainTransform calls them (2 table copies, 2 allocations):  %8.1f us / batch" % us_both)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "train_load_bench.txt"))
    a = ap.parse_args()
    from ifseg_amd.artificial import trainer_first_ordinal
    from ifseg_amd.criterions import SegCriterion
    from ifseg_amd.tasks.mm_tasks import SegmentationTask
    from ifseg_amd.trainer import Trainer
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(0)
    nseg, size, B = 15, 512, a.batch
    g = torch.Generator().manual_seed(4321)
    names = [torch.randint(4, 50000, (1,), generator=g) for _ in range(nseg)]       # 36 source tokens, bench.py's length
    task = SegmentationTask(num_seg_tokens=nseg, patch_image_size=size, arch="segofa_base", category_token_ids=names)
    model = task.build_model()
    crit = SegCriterion(task, unsupervised_segmentation=False, init_seg_with_text=False)
    trainer = Trainer(model, crit, task, device=dev, lazy_logs=True)
    imgs, labs = sources(B, nseg, dev)

    lines = ["%s" % torch.cuda.get_device_name(dev),
             "training transform of raw images (csrc/trainload.hip), sources %s ..., resident on the device"
             % ", ".join("%dx%d" % (w, h) for h, w in SHAPES[:3]),
             "kernels alone: microseconds per batch over 200 eager calls (device events); GB/s over the bytes WRITTEN", ""]
    for dt in (torch.bfloat16, torch.float32):
        kernels_alone(lines, task.build_train_transform(dev, seed=1, dtype=dt), imgs, labs)
    lines.append("")

    task.build_train_transform(dev, seed=1, dtype=torch.bfloat16)
    RING = 4
    ring = [task.train_sample(imgs, labs, trainer_first_ordinal(j, 0, 0, 1, 1, B)) for j in range(RING)]
    count, ahead = [0], {}

    def batch(mode, i):
        if mode == "ring":
            return ring[i % RING]
        if i not in ahead:
            ahead.clear()
            ahead[i] = task.train_sample(imgs, labs, trainer_first_ordinal(RING + i, 0, 0, 1, 1, B))
        return ahead[i]

    def step(mode):
        # both variants hand the trainer the batch of the NEXT step as well (the trunk prefetch of bench.py's ring); `fresh`
        # builds that batch here, one step ahead, as a loader would
        i = count[0]
        count[0] += 1
        cur = batch(mode, i)
        nxt = ring[(i + 1) % RING] if mode == "ring" else task.train_sample(imgs, labs, trainer_first_ordinal(RING + i + 1, 0, 0, 1, 1, B))
        if mode != "ring":
            ahead.clear()
            ahead[i + 1] = nxt
        return trainer.train_step([cur], prefetch=[nxt])

    def timed(mode):
        torch.cuda.synchronize()
        t0 = time.time()
        for _ in range(a.steps):
            logs = step(mode)
        torch.cuda.synchronize()
        dt = (time.time() - t0) / a.steps * 1e3
        assert float(logs[0]["loss"]) == float(logs[0]["loss"])
        return dt

    modes = ("ring", "fresh")
    for m in modes:
        for _ in range(5):
            step(m)
    res = {m: [] for m in modes}
    for _ in range(a.rounds):
        for m in modes:
            res[m].append(timed(m))
    label = {"ring": "ring   pre-built samples", "fresh": "fresh  task.train_sample every step"}
    lines += ["supervised Trainer.train_step, segofa_base, batch %d, %dx%d, %d classes, bf16 patch_images" % (B, size, size, nseg),
              "%d rounds x %d steps per variant, variants alternating; ms per step (host clock, device synchronise at the end)"
              % (a.rounds, a.steps)]
    for m in modes:
        r = res[m]
        lines.append("%-54s median %7.2f ms   min %7.2f   max %7.2f   (%s)" % (label[m], statistics.median(r), min(r), max(r),
                                                                             " ".join("%.2f" % x for x in r)))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
