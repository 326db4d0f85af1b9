"""The strong augmentation of a mixed batch on the device (csrc/strong.hip: hip.strong_draw, hip.strong_apply;
task.dacs_sample(strong=True)) against what it replaces, on the same device, per call as enqueued from Python:

  apply   the device-only torch composition of the same rule: denormalise and round to grey levels, the photometric chain
          with its two 8-bit HSV round trips in integer tensors (the record's switches and parameters are given to it
          ready-made, as [B, 1, 1] tensors), reflect-pad, two depthwise conv2d in fp64 (the vertical sums pass 2^24), the
          rounding and a table gather.  Both sides are checked to give the same bits before they are timed.
  draw    timed alone, into a fresh records tensor and into `out=`: it replaces a handful of host random numbers, there is
          nothing on the device to compare it with.

B = 8, P = 512, fp32 and bf16 images of table values, records with both stages on.  And `task.dacs_sample(strong=True)`
against `strong=False` on SegOFA-Base (--no-model leaves it out).  The variants of a row alternate window by window in one
process; a window is at least 0.5 s of enqueued calls between two device events after a warm-up; the figure is the median
over the windows, [min, max] its run-to-run spread: a difference inside the spread is no difference.

    python tools/strong_aug_bench.py [--windows 5] [--window-s 0.5] [--no-model] [--out profiles/strong_aug_bench.txt]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

from evaluate_bench import row

B, P = 8, 512
D = 7650


def _convert(x, alpha=None, beta=None):
    v = x.float()
    v = v * alpha if beta is None else v + beta
    return v.clamp(0, 255).trunc().long()


def _to_hsv(r, g, b):
    V = torch.maximum(torch.maximum(r, g), b)
    d = V - torch.minimum(torch.minimum(r, g), b)
    S = torch.where(V > 0, (510 * d + V) // (2 * V).clamp_min(1), torch.zeros_like(V))
    x = torch.where(V == r, g - b, torch.where(V == g, b - r, r - g))
    off = torch.where(V == r, 0, torch.where(V == g, 60, 120))
    H = torch.where(d > 0, ((2 * (30 * x + off * d) + d) // (2 * d.clamp_min(1))) % 180, torch.zeros_like(V))
    return H, S, V


def _to_rgb(H, S, V):
    sec, f = H // 30, H % 30
    rd = lambda n: (2 * n + D) // (2 * D)
    p, q, t = rd(30 * V * (255 - S)), rd(V * (D - S * f)), rd(V * (D - S * (30 - f)))
    pick = lambda c: torch.stack(c).gather(0, sec[None])[0]
    return pick([V, q, p, p, t, V]), pick([t, V, V, q, p, p]), pick([p, p, t, V, V, q])


def torch_params(rec, dev):
    """the records, digested on the host into what the composition takes: switches bool [B, 1, 1], parameters fp32 / int64
    [B, 1, 1], the blur weights as two depthwise fp64 kernels per sample"""
    r = rec.cpu()
    sw = lambda k: (r[:, k] != 0).reshape(-1, 1, 1).to(dev)
    fl = lambda k: r[:, k].contiguous().view(torch.float32).reshape(-1, 1, 1).to(dev)
    w = r[:, 10:15].double()
    taps = torch.cat([w[:, 1:].flip(1), w], 1).to(dev)                             # [B, 9]
    return dict(bright=sw(0), contrast=sw(1), sat=sw(2), hue=sw(3), mode=sw(4), beta=fl(5), alpha_c=fl(6), alpha_s=fl(7),
                delta=(r[:, 8].long() % 180).reshape(-1, 1, 1).to(dev), taps=taps)


def torch_apply(p, img, lut, mean, std, conv_dtype=torch.float64):
    """-> images like `img`; the same rule as hip.strong_apply on table-valued images"""
    q = ((img.float() * std + mean) * 255).round().clamp(0, 255).long()
    r, g, b = q[:, 0], q[:, 1], q[:, 2]
    on3 = lambda m, new, old: tuple(torch.where(m, n, o) for n, o in zip(new, old))
    contrast = lambda c: tuple(_convert(x, alpha=p["alpha_c"]) for x in c)
    c = on3(p["bright"], tuple(_convert(x, beta=p["beta"]) for x in (r, g, b)), (r, g, b))
    c = on3(p["contrast"] & p["mode"], contrast(c), c)
    H, S, V = _to_hsv(*c)
    c = on3(p["sat"], _to_rgb(H, _convert(S, alpha=p["alpha_s"]), V), c)
    H, S, V = _to_hsv(*c)
    c = on3(p["hue"], _to_rgb((H + p["delta"]) % 180, S, V), c)
    c = on3(p["contrast"] & ~p["mode"], contrast(c), c)
    x = torch.stack(c, 1).to(conv_dtype)                                           # [B, 3, P, P]
    n = x.shape[0]
    x = F.pad(x.reshape(1, n * 3, P, P), (4, 4, 4, 4), mode="reflect")
    k = p["taps"].to(conv_dtype).repeat_interleave(3, 0)                           # one kernel per (sample, plane)
    x = F.conv2d(x, k.reshape(n * 3, 1, 1, 9), groups=n * 3)
    x = F.conv2d(x, k.reshape(n * 3, 1, 9, 1), groups=n * 3).reshape(n, 3, P, P)
    qq = (x.long() + (1 << 23)) >> 24
    return torch.stack([lut[ch][qq[:, ch]] for ch in range(3)], 1).to(img.dtype)


def both_on(seed=5):
    """the first ordinal from which B consecutive records have an operation of the jitter and the blur on"""
    from ifseg_amd import augment as A
    first = 0
    while True:
        rec = A.strong_draw_reference(B, seed, first)
        if bool((rec[:, :4].sum(1) > 0).all()) and bool((rec[:, 9] >= 0).all()):
            return first
        first += 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--window-s", type=float, default=0.5)
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ifseg_amd import hip
    from ifseg_amd.imageio import normalisation_table
    dev = torch.device("cuda:0")
    lines = ["strong augmentation on the device vs the torch composition of the same rule: median [min, max] microseconds over %d "
             "alternating windows of >= %.1f s" % (a.windows, a.window_s),
             "B = %d, P = %d, records with jitter and blur on; x = composition / new.  Bytes an apply moves (one batch read, one "
             "written): fp32 %.0f MB, bf16 %.0f MB" % (B, P, B * 3 * P * P * 8 / 1e6, B * 3 * P * P * 4 / 1e6), ""]
    first = both_on()
    rec = hip.strong_draw(B, 5, first, device=dev)
    row(lines, "draw", [lambda: hip.strong_draw(B, 5, first, device=dev), lambda: hip.strong_draw(B, 5, first, out=rec)],
        ("strong_draw", "into out="), a)
    lut = normalisation_table().to(dev)
    mean = torch.full((1, 3, 1, 1), 0.5, device=dev)
    std = torch.full((1, 3, 1, 1), 0.5, device=dev)
    params = torch_params(rec, dev)
    g = torch.Generator().manual_seed(3)
    q = torch.randint(0, 256, (B, 3, P, P), generator=g).to(dev)
    for dtype in (torch.float32, torch.bfloat16):
        img = torch.stack([lut[c][q[:, c]] for c in range(3)], 1).to(dtype)
        got, want = hip.strong_apply(rec, img), torch_apply(params, img, lut, mean, std)
        iv = torch.int32 if dtype == torch.float32 else torch.int16
        assert torch.equal(got.view(iv), want.view(iv)), "the torch composition and strong_apply disagree"
        out = torch.empty_like(img)
        row(lines, "apply %-8s" % str(dtype)[6:], [lambda: hip.strong_apply(rec, img, out=out), lambda: torch_apply(params, img, lut, mean, std)],
            ("strong_apply", "torch composition"), a)
    if not a.no_model:
        from ifseg_amd.tasks.mm_tasks.segmentation import SegmentationTask
        H, W, Bm, n = 512, 683, 2, 150
        lines += ["", "end to end, SegOFA-Base, n = %d, %d labelled + %d unlabelled raw uint8 %d x %d images; x = strong=False / "
                  "strong=True" % (n, Bm, Bm, H, W)]
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
        row(lines, "dacs_sample", [lambda: task.dacs_sample(model, imgs[:Bm], labs, imgs[Bm:], 0, strong=True, **kw),
                                   lambda: task.dacs_sample(model, imgs[:Bm], labs, imgs[Bm:], 0, **kw)], ("strong=True", "strong=False"), a)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
