"""The sieve on the device (csrc/sieve.hip: hip.seg_sieve; Segmenter(sieve=)) against its floor and against what a user does
without it, per call as enqueued from Python.  One 512 x 683 uint8 map, min_region 16, connectivity 4, passes 1 and 2:
  piecewise     classes in blocks of 32 x 32 pixels with 2 % of the pixels flipped to another class: what a segmenter gives
  random        an independent class per pixel, over 5 values: every region is small and every pixel votes
  checkerboard  the worst case for the rule (all keys tie on size), single-pixel regions throughout
and per map
  seg_regions   hip.seg_regions alone, once per pass: the floor (a pass is its launches plus three short ones)
  seg_sieve     the call
  torch         the specification as torch operations on the device (predict.sieve_reference on device tensors)
  cpu+scipy     labels.cpu(), scipy.ndimage.label per present class, a host loop over the components below 16 pixels that
                gives each the value of its largest 4-adjacent neighbour component, the result copied back: its device wait is
                part of it (one pass; left out when scipy is not installed).  It is what a user would write, not the rule bit
                for bit: ties go to whichever the loop meets first
and `Segmenter.segment_raw` on SegOFA-Base with sieve=16 against without, per image (--no-model leaves it out).
The variants of a row alternate window by window in one process; a window is at least 0.5 s of enqueued calls between two
device events after a warm-up; the figure is the median over the windows, [min, max] its run-to-run spread: a difference inside
the spread is no difference.  seg_sieve's result is checked against the specification before it is timed.

    python tools/sieve_bench.py [--windows 5] [--window-s 0.5] [--no-model] [--out profiles/sieve_bench.txt]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from evaluate_bench import row
from predict_tta_bench import H, P, W

MIN_REGION = 16


def maps():
    g = torch.Generator().manual_seed(3)
    blocks = torch.randint(0, 15, ((H + 31) // 32, (W + 31) // 32), generator=g)
    piece = blocks.repeat_interleave(32, 0).repeat_interleave(32, 1)[:H, :W].clone()
    flip = torch.rand(H, W, generator=g) < 0.02
    piece[flip] = (piece[flip] + 1 + torch.randint(0, 14, (int(flip.sum()),), generator=g)) % 15
    y = torch.arange(H).reshape(H, 1).expand(H, W)
    x = torch.arange(W).reshape(1, W).expand(H, W)
    return (("piecewise", piece.to(torch.uint8)), ("random", torch.randint(0, 5, (H, W), generator=g).to(torch.uint8)),
            ("checkerboard", ((y + x) % 2).to(torch.uint8)))


def scipy_sieve(labels):
    """what a user does today, one pass at connectivity 4 -> the sieved map, back on the device"""
    import numpy as np
    from scipy import ndimage
    a = labels.cpu().numpy()
    comp = np.zeros(a.shape, dtype=np.int64)
    k = 0
    for v in np.unique(a):
        c, kv = ndimage.label(a == v)
        comp[c > 0] = c[c > 0] + k
        k += kv
    size = np.bincount(comp.reshape(-1), minlength=k + 1)
    value = np.zeros(k + 1, dtype=a.dtype)
    value[comp.reshape(-1)] = a.reshape(-1)
    # the pairs of 4-adjacent components, once each way, sorted by the small one
    pairs = np.concatenate([np.stack([comp[:, :-1].reshape(-1), comp[:, 1:].reshape(-1)], 1),
                            np.stack([comp[:-1].reshape(-1), comp[1:].reshape(-1)], 1)])
    pairs = pairs[pairs[:, 0] != pairs[:, 1]]
    pairs = np.unique(np.concatenate([pairs, pairs[:, ::-1]]), axis=0)
    pairs = pairs[size[pairs[:, 0]] < MIN_REGION]
    new = value.copy()
    starts = np.flatnonzero(np.r_[True, pairs[1:, 0] != pairs[:-1, 0]]) if len(pairs) else np.zeros(0, dtype=np.int64)
    for s, e in zip(starts, np.r_[starts[1:], len(pairs)]):    # the host loop over the small components
        r, nb = pairs[s, 0], pairs[s:e, 1]
        q = nb[np.argmax(size[nb])]
        if size[q] > size[r] or (size[q] == size[r] and q < r):
            new[r] = value[q]
    return torch.from_numpy(new[comp]).to(labels.device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.5)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ifseg_amd import hip
    from ifseg_amd.predict import sieve_reference
    try:
        import scipy  # noqa: F401
        have_scipy = True
    except ImportError:
        have_scipy = False
    dev = torch.device("cuda:0")
    lines = ["the sieve on the device vs seg_regions alone (its floor), the specification in torch and labels.cpu() + scipy: "
             "median [min, max] microseconds over %d alternating windows of >= %.1f s" % (a.windows, a.window_s),
             "one %d x %d uint8 map, min_region %d, connectivity 4, n 15; x = seg_sieve / seg_regions%s"
             % (H, W, MIN_REGION, "" if have_scipy else "  (scipy is not installed: cpu+scipy NOT MEASURED)"), ""]
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    for name, lab in maps():
        d = lab.to(dev)
        for passes in (1, 2):
            want, w_moved = sieve_reference(d, MIN_REGION, 4, passes, n=15)
            out, moved = hip.seg_sieve(d, MIN_REGION, 4, passes, n=15, flag=flag)
            assert torch.equal(out, want) and torch.equal(moved, w_moved) and int(flag) == 0

            def floor():
                for _ in range(passes):
                    hip.seg_regions(d, 4)

            fns = [floor, lambda: hip.seg_sieve(d, MIN_REGION, 4, passes, n=15),
                   lambda: sieve_reference(d, MIN_REGION, 4, passes, n=15)]
            labels = ["seg_regions x%d" % passes, "seg_sieve", "torch"]
            if have_scipy and passes == 1:
                scipy_sieve(d)
                fns.append(lambda: scipy_sieve(d))
                labels.append("cpu+scipy")
            row(lines, "%-12s passes %d, %6d pixels moved" % (name, passes, int(w_moved[0].sum())), fns, labels, a)
    if not a.no_model:
        from ifseg_amd.tasks.mm_tasks.segmentation import SegmentationTask
        lines += ["", "end to end, SegOFA-Base, one raw uint8 %d x %d image, sieve %d, 2 passes; x = with / without" % (H, W, MIN_REGION)]
        n = 150
        torch.manual_seed(0)
        g = torch.Generator().manual_seed(7)
        names = [torch.randint(4, 50000, (int(k),), generator=g) for k in torch.randint(1, 4, (n,), generator=g)]
        task = SegmentationTask(num_seg_tokens=n, patch_image_size=P, arch="segofa_base", category_token_ids=names)
        model = task.build_model().to(dev).eval()
        plain_seg, sieve_seg = task.build_segmenter(model), task.build_segmenter(model, sieve=MIN_REGION)
        img = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8).to(dev)
        plain = lambda: plain_seg.segment_raw(img, return_conf=True)
        sieved = lambda: sieve_seg.segment_raw(img, return_conf=True)
        p, r = plain()[0], sieved()[0]
        want = sieve_reference(p.labels, MIN_REGION, 4, 2, n=n, conf=p.conf)
        assert torch.equal(r.labels, want[0]) and torch.equal(r.conf, want[2])
        row(lines, "n %3d, %6d pixels moved" % (n, int(want[1][0].sum())), [plain, sieved], ("segment_raw", "sieve=16"), a)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
