"""What feeding the image-free step costs: `Trainer.train_step` of the headline model (SegOFA-Base, batch 8, 512 x 512, 15 classes)
in its image-free form, all in one process on one GPU, the variants alternating round by round:

  pre   the artificial image of every step comes from a ring of PRE-BUILT samples (what `bench.py --image-free` times)
  (a)   a FRESH sample every step, built the only way the tree had before the device sampler: `task.synthetic_aux_sample`
        on the CPU (one torch.cat per patch) + the host-to-device copies
  (b)   a fresh sample every step from the device sampler (ifseg_amd/artificial.py, csrc/imfree.hip): the batch carries
        no aux_input
  (c)   the sampler alone: microseconds per batch and achieved GB/s over its algorithmic bytes
        (text2seg_target B (S^2 + 1) 8 + ids B P Lmax 8 + ends B P 8 + prev B (P + 1) 8 written, shapes / coarse
        B (2 + 32^2) 4 written once and the coarse map read by two launches)

Times are host clocks around `steps` enqueued updates ending in a device synchronise; (c) is timed with device events, once
enqueued eagerly (two ctypes calls and six allocations per batch on the host) and once as a replayed HIP graph.

    python tools/imfree_sampler_bench.py [--steps 40] [--rounds 3] [--out profiles/imfree_sampler_ab.txt]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch


def names_like_the_synthetic_sample(task, nseg, seed=4321):
    """1-3 random BPE ids per class, as `synthetic_aux_sample` names its classes"""
    g = torch.Generator().manual_seed(seed)
    n = torch.randint(1, 4, (nseg,), generator=g)
    return [torch.randint(4, min(50000, task.seg_id_offset - 1), (int(k),), generator=g) for k in n]


def sampler_alone(lines, smp, B, iters=200):
    dev = smp.device
    src = torch.zeros(B, 36, dtype=torch.long, device=dev)
    lens = torch.full((B,), 36, device=dev)
    for i in range(5):
        smp.sample(B, i * B, src, lens)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(iters):
        smp.sample(B, i * B, src, lens)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / iters
    P, S2, cs = smp.hp * smp.wp, 256 * smp.hp * smp.wp, smp.max_side ** 2
    nbytes = B * ((S2 + 1) * 8 + P * smp.Lmax * 8 + P * 8 + (P + 1) * 8 + (2 + cs) * 4 + 2 * cs * 4)
    lines.append("(c) sampler alone  B %d  grid %dx%d  image %dx%d  nseg %d  Lmax %d: %8.1f us / batch (draw + expand, 3 launches, "
                 "eager enqueue)  %6.1f MB  %7.1f GB/s" % (B, smp.hp, smp.wp, 16 * smp.hp, 16 * smp.wp, smp.nseg, smp.Lmax, us,
                                                          nbytes / 1e6, nbytes / us / 1e3))
    # the same three launches replayed from a HIP graph, the ordinal in a device word: no host work between the kernels
    word = torch.zeros(1, dtype=torch.long, device=dev)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        smp.sample(B, word, src, lens)
    for _ in range(5):
        graph.replay()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        graph.replay()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) * 1e3 / iters
    lines.append("    the same as a replayed HIP graph (ordinal in a device word):%s %8.1f us / batch  %7.1f GB/s"
                 % (" " * 12, us, nbytes / us / 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "imfree_sampler_ab.txt"))
    a = ap.parse_args()
    from ifseg_amd.artificial import ArtificialImageSampler
    from ifseg_amd.criterions import SegCriterion
    from ifseg_amd.tasks.mm_tasks import SegmentationTask
    from ifseg_amd.trainer import Trainer
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(0)
    nseg, size, B = 15, 512, a.batch
    task = SegmentationTask(num_seg_tokens=nseg, patch_image_size=size, arch="segofa_base")
    task.category_token_ids = names_like_the_synthetic_sample(task, nseg)
    task.cfg.artificial_image_type = "rand_k-1-33"
    model = task.build_model()
    crit = SegCriterion(task, unsupervised_segmentation=True, init_seg_with_text=False)
    trainer = Trainer(model, crit, task, device=dev, lazy_logs=True)
    RING = 4
    ring, ring_pre = [], []
    for j in range(RING):
        sm = task.synthetic_sample(B, dev, seed=1234 + 7919 * j)
        sm["net_input"]["patch_images"] = sm["net_input"]["patch_images"].to(torch.bfloat16)
        ring.append(sm)
        ring_pre.append(dict(sm, **task.synthetic_aux_sample(B, dev, seed=4321 + 7919 * j)))
    count = [0]

    def step(mode):
        i = count[0]
        count[0] += 1
        if mode == "pre":
            cur, src = ring_pre[i % RING], ring_pre
        elif mode == "a":
            cur, src = dict(ring[i % RING], **task.synthetic_aux_sample(B, dev, seed=100000 + i)), ring
        else:
            cur, src = ring[i % RING], ring
        return trainer.train_step([cur], prefetch=[src[(i + k) % RING] for k in range(1, RING + 1)])

    def timed(mode):
        torch.cuda.synchronize()
        t0 = time.time()
        for _ in range(a.steps):
            logs = step(mode)
        torch.cuda.synchronize()
        dt = (time.time() - t0) / a.steps * 1e3
        assert float(logs[0]["loss"]) == float(logs[0]["loss"])
        return dt

    modes = ("pre", "a", "b")
    for m in modes:
        for _ in range(5):
            step(m)
    res = {m: [] for m in modes}
    for _ in range(a.rounds):
        for m in modes:
            res[m].append(timed(m))
    label = {"pre": "pre  pre-built ring (bench.py --image-free)", "a": "(a)  fresh CPU sample + copy every step",
             "b": "(b)  fresh device sample every step"}
    lines = ["image-free Trainer.train_step, segofa_base, batch %d, %dx%d, %d classes, %s" % (B, size, size, nseg, torch.cuda.get_device_name(dev)),
             "%d rounds x %d steps per variant, variants alternating; ms per step (host clock, device synchronise at the end)" % (a.rounds, a.steps)]
    for m in modes:
        r = res[m]
        lines.append("%-46s median %7.2f ms   min %7.2f   max %7.2f   (%s)" % (label[m], statistics.median(r), min(r), max(r),
                                                                             " ".join("%.2f" % x for x in r)))
    assert crit._imfree_sampler is not None
    sampler_alone(lines, crit._imfree_sampler, B)
    g = torch.Generator().manual_seed(1)
    big = ArtificialImageSampler([torch.randint(4, 50000, (int(k),), generator=g) for k in torch.randint(1, 4, (172,), generator=g)],
                                 task.seg_id_offset, 40, 40, 1, 33, seed=1, device=dev)
    sampler_alone(lines, big, B)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
