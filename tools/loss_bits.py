"""Bit-compare (and time) the fused segmentation criterion -- csrc/loss.hip, ohem.hip, dice.hip, distill.hip on csrc/seg_tile.h --
between two checkouts or two builds of the library.

    python tools/loss_bits.py save PATH     # every output of every path of every case -> PATH   (run it in checkout A)
    python tools/loss_bits.py cmp PATH      # one line per output: bit-equal | n differ           (run it in checkout B)
    IFSEG_LIB=<library> python tools/loss_bits.py time     # microseconds per launch at the workload shapes

Only the surface a refactor of the family keeps is used, so one copy of this file runs in both checkouts: `hip.seg_loss`,
`seg_loss_weighted`, `seg_hardness`, `ohem_select`, `seg_dice_sums`, `seg_dice`, `seg_loss_dice`, `seg_distill`,
`seg_loss_distill`, the three gather entry points of the C ABI, and `SegCriterion.compute_loss` on a stub network output.
Inputs are the seeded host-side cases of the tests (`_dice_cases.dice_inputs` and `pixel_plane`, `_distill_cases.teacher` "far",
also as a `widen`ed view) at `_dice_cases.SHAPES`: 2 .. 512 classes, a single cell with every tap clamped, interior cells with
all nine partials, 8 x 8 tiles.  Paths: CE with eps 0 / 0.1; weighted CE (plane, class weights, both, each with norm_pixels on
and off); hardness, the OHEM plane and info; the Dice sums, Dice alone, CE + Dice plain and weighted; KD alone (mask valid / all
x T 1 / 2, and without a target), CE + KD, CE + Dice + KD; the three gather entries on the partials of those calls; the
criterion in four configurations (loss, metrics, d loss / d logits).  Every tensor is compared as integers; `cmp` exits 1 unless
all are equal.
`time`: every kernel of the family alone, through its C entry point (the ABI is the same in both builds, so IFSEG_LIB selects
the build), at B = 8, 32 x 32 cells, 15 and 150 classes: median [min, max] microseconds over 5 windows of 100 launches after a
warm-up of 20."""
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _dice_cases as DC  # noqa: E402
import _distill_cases as KC  # noqa: E402
from ifseg_amd import hip  # noqa: E402
from ifseg_amd.criterions import SegCriterion  # noqa: E402

dev = torch.device("cuda:0")
SEG0 = DC.SEG0
F32 = torch.float32
outs = {}
c_int, c_ll, c_float, p = ctypes.c_int, ctypes.c_longlong, ctypes.c_float, hip._ptr


def keep(name, **tensors):
    torch.cuda.synchronize()
    for k, t in tensors.items():
        outs["%s %s" % (name, k)] = t.detach().cpu().contiguous().clone()


def ce_bufs(lp, B, hp, wp, n):
    tiles = B * hp * wp
    return (torch.zeros(tiles * 9 * n, device=dev), torch.zeros(tiles * (2 + 3 * n), device=dev), torch.zeros(2 + 3 * n, device=dev),
            torch.zeros_like(lp), torch.zeros(1, device=dev))


def gather_out(lp, words):
    return torch.zeros_like(lp), torch.zeros(words, device=dev)


def gathers(name, lp, B, hp, wp, n, ce, dice, kd):
    """the three entry points on saved partials; ce = (tile, stats), dice = (dice_tile, dice_val), kd = (kd_tile, kd_stats, w, T)"""
    lib = hip.lib()
    tail = lambda dl: (p(dl), c_int(dl.stride(1)), c_ll(dl.stride(0)), c_int(B), c_int(hp), c_int(wp), c_int(n))
    none = (None, None)
    dl, lo = gather_out(lp, 1)
    hip._check(lib.ifseg_seg_loss_gather(p(ce[0]), p(ce[1]), *tail(dl), p(lo), hip._stream()), "gather")
    keep(name + " gather(ce)", dl=dl, loss=lo)
    for tag, c in (("ce,dice", ce), ("-,dice", none)):
        dl, lo = gather_out(lp, 3)
        hip._check(lib.ifseg_seg_loss_gather_sum(p(c[0]), p(c[1]), p(dice[0]), p(dice[1]), *tail(dl), p(lo), hip._stream()), "gather_sum")
        keep(name + " gather_sum(%s)" % tag, dl=dl, loss=lo)
    for tag, c, d, k in (("ce,dice,kd", ce, dice, kd), ("ce,-,kd", ce, none, kd), ("-,-,kd", none, none, kd), ("-,dice,kd", none, dice, kd),
                         ("ce,dice,-", ce, dice, None), ("-,dice,-", none, dice, None)):
        dl, lo = gather_out(lp, 4)
        ks = (p(k[0]), p(k[1]), c_float(k[2]), c_float(k[3])) if k is not None else (None, None, c_float(1.0), c_float(1.0))
        hip._check(lib.ifseg_seg_loss_gather3(p(c[0]), p(c[1]), p(d[0]), p(d[1]), *ks, *tail(dl), p(lo), hip._stream()), "gather3")
        keep(name + " gather3(%s)" % tag, dl=dl, loss=lo)


class _Engine:
    def deferred_check(self, *a, **kw):
        pass


class _Model:
    training = True
    engine = _Engine()


def criterion(name, lp, tgt, te, pw, cw, hp, wp, n):
    B, H, W = lp.shape[0], 16 * hp, 16 * wp
    base = dict(num_seg_tokens=n, seg_id_offset=SEG0, unsupervised_segmentation=False, init_seg_with_text=False, label_smoothing=0.1)
    images = torch.empty(B, 3, H, W, device=dev)
    clean = DC.clean_target(tgt, n)
    for tag, kw, weighted, taught in (
            ("plain", {}, False, False),
            ("weighted+ohem", dict(class_weight=cw.tolist(), weight_norm="pixels", ohem_thresh=0.7, ohem_min_kept=100), True, False),
            ("dice", dict(dice_weight=3.0, dice_smooth=0.5, dice_class_weight=cw.tolist(), class_weight=cw.tolist()), True, False),
            ("dice+kd", dict(dice_weight=3.0, distill_weight=1.5, distill_temperature=2.0), False, True)):
        crit = SegCriterion(None, **base, **kw)
        for rep in range(2):                                  # the second call runs on the buffers of the first
            logits = lp[:, :, :n].detach().clone().requires_grad_(True)
            extra = {"encoder_returns": {"image_embed_shape": [(hp, wp)]}, "logits_padded": lp}
            sample = {"target": clean, "net_input": {"patch_images": images}}
            if weighted:
                sample["target_weight"] = pw
            if taught:
                sample["teacher_logits"] = te
            loss, metrics, _ = crit.compute_loss(_Model(), (logits, extra), sample, 0)
            loss.backward()
            res = {"loss": loss, "dlogits": logits.grad}
            res.update({"m_" + k: v for k, v in metrics.items()})
            if crit.dice_sums is not None:
                res["dice_sums"] = crit.dice_sums
            if crit.distill_stats is not None:
                res["distill_stats"] = crit.distill_stats
            if crit.ohem_info is not None:
                res["ohem_info"] = crit.ohem_info
            keep("%s criterion %s #%d" % (name, tag, rep), **res)


def run_case(n, B, hp, wp):
    name = "n%d B%d %dx%d" % (n, B, hp, wp)
    H, W = 16 * hp, 16 * wp
    lp, tgt, cw = (t.to(dev) for t in DC.dice_inputs(n, B, hp, wp))
    pw = DC.pixel_plane(B, H * W).to(dev)
    te_host = KC.teacher(n, B, hp, wp, "far")
    te, te_wide = te_host.to(dev), KC.widen(te_host, dev)
    # CE
    for eps in (0.0, 0.1):
        tile, sp, stats, dl, loss = ce_bufs(lp, B, hp, wp, n)
        bad = torch.zeros(1, dtype=torch.int32, device=dev)
        hip.seg_loss(lp, tgt, hp, wp, H, W, n, SEG0, tile, sp, stats, dl, loss, bad_label=bad, label_smoothing=eps)
        keep("%s ce eps%g" % (name, eps), tile=tile, sp=sp, stats=stats, dl=dl, loss=loss, bad=bad)
    for tag, q, w in (("plane", pw, None), ("cw", None, cw), ("plane+cw", pw, cw), ("none", None, None)):
        for norm in (False, True):
            tile, sp, stats, dl, loss = ce_bufs(lp, B, hp, wp, n)
            hip.seg_loss_weighted(lp, tgt, hp, wp, H, W, n, SEG0, tile, sp, stats, dl, loss, pixel_weight=q, class_weight=w,
                                  norm_pixels=norm, label_smoothing=0.1)
            keep("%s wce %s norm%d" % (name, tag, norm), tile=tile, sp=sp, stats=stats, dl=dl, loss=loss)
    # hardness and the OHEM plane
    hard = hip.seg_hardness(lp, tgt, hp, wp, H, W, n, SEG0)
    keep(name + " hardness", plane=hard)
    for tag, q in (("", None), (" weight", pw)):
        plane, info = hip.ohem_select(hard, 0.7, 100, weight=q)
        keep(name + " ohem" + tag, plane=plane, info=info)
    # Dice
    keep(name + " dice_sums", sums=hip.seg_dice_sums(lp, tgt, hp, wp, H, W, n, SEG0))
    for tag, w in (("", None), (" cw", cw)):
        bufs = {}
        loss, dl = hip.seg_dice(lp, tgt, hp, wp, H, W, n, SEG0, 3.0, 0.5, class_weight=w, bufs=bufs)
        keep(name + " dice" + tag, loss=loss, dl=dl, loss3=bufs["loss3"], sums=bufs["dice_sums"], tile=bufs["dice_tile"], val=bufs["dice_val"])
    ce_dice = {}
    loss3, dl = hip.seg_loss_dice(lp, tgt, hp, wp, H, W, n, SEG0, 3.0, 1.0, dice_class_weight=cw, bufs=ce_dice)
    keep(name + " ce+dice", loss3=loss3, dl=dl, stats=ce_dice["stats"], bad=ce_dice["bad"])
    wb = {}
    loss3, dl = hip.seg_loss_dice(lp, tgt, hp, wp, H, W, n, SEG0, 3.0, 1.0, dice_class_weight=cw, bufs=wb, pixel_weight=pw,
                                  class_weight=cw, norm_pixels=True, label_smoothing=0.1)
    keep(name + " wce+dice", loss3=loss3, dl=dl, stats=wb["stats"])
    # distillation
    for mask in ("valid", "all"):
        for T in (1.0, 2.0):
            for tag, t in (("", te), (" wide", te_wide)):
                bufs = {}
                loss, dl = hip.seg_distill(lp, t, tgt, hp, wp, H, W, n, SEG0, 1.5, T, mask, bufs=bufs)
                keep("%s kd %s T%g%s" % (name, mask, T, tag), loss=loss, dl=dl, loss4=bufs["loss4"], stats=bufs["kd_stats"], tile=bufs["kd_tile"])
    bufs = {}
    loss, dl = hip.seg_distill(lp, te, None, hp, wp, H, W, n, SEG0, 1.5, 2.0, "all", bufs=bufs)
    keep(name + " kd no target", loss=loss, dl=dl, loss4=bufs["loss4"], stats=bufs["kd_stats"])
    ck = {}
    loss4, dl = hip.seg_loss_distill(lp, te, tgt, hp, wp, H, W, n, SEG0, 1.5, 2.0, bufs=ck, label_smoothing=0.1)
    keep(name + " ce+kd", loss4=loss4, dl=dl, stats=ck["stats"], kd_stats=ck["kd_stats"])
    all3 = {}
    loss4, dl = hip.seg_loss_distill(lp, te_wide, tgt, hp, wp, H, W, n, SEG0, 1.5, 2.0, "all", dice_weight=3.0, dice_smooth=0.5,
                                     dice_class_weight=cw, bufs=all3, pixel_weight=pw, class_weight=cw)
    keep(name + " wce+dice+kd", loss4=loss4, dl=dl, stats=all3["stats"], kd_stats=all3["kd_stats"], sums=all3["dice_sums"])
    # the three doors of the gather, on the partials of the call above
    gathers(name, lp, B, hp, wp, n, (all3["tile"], all3["stats"]), (all3["dice_tile"], all3["dice_val"]),
            (all3["kd_tile"], all3["kd_stats"], 1.5, 2.0))
    criterion(name, lp, tgt, te, pw, cw, hp, wp, n)


def bits(t):
    return t.view({torch.bfloat16: torch.int16, torch.float32: torch.int32}.get(t.dtype, t.dtype))


def timeit(f, warm=20, n=100, windows=5):
    for _ in range(warm):
        f()
    torch.cuda.synchronize()
    us = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            f()
        b.record()
        torch.cuda.synchronize()
        us.append(a.elapsed_time(b) / n * 1e3)
    return statistics.median(us), min(us), max(us)


def run_time():
    B, hp, wp = 8, 32, 32
    H, W, tiles = 16 * hp, 16 * wp, B * hp * wp
    lib, s = hip.lib(), hip._stream
    print("library %s" % hip.LIB_PATH)
    for n in (15, 150):
        g = torch.Generator().manual_seed(7)
        npad = (n + 7) // 8 * 8
        lp = torch.zeros(B, hp * wp + 1, npad, dtype=torch.bfloat16)
        lp[:, :, :n] = torch.randn(B, hp * wp + 1, n, generator=g) * 2
        te = torch.zeros_like(lp)
        te[:, :, :n] = torch.randn(B, hp * wp + 1, n, generator=g) * 3
        tgt = torch.cat([torch.randint(0, n + 1, (B, H * W), generator=g) + SEG0, torch.full((B, 1), 2)], 1)
        cw = torch.rand(n, generator=g) * 1.5 + 0.5
        pw = torch.randint(0, 256, (B, H * W), generator=g, dtype=torch.uint8)
        lp, te, tgt, cw, pw = (t.to(dev) for t in (lp, te, tgt, cw, pw))
        head = (p(lp), c_int(npad), c_ll(lp.stride(0)), p(tgt), c_ll(tgt.stride(0)), c_int(B), c_int(hp), c_int(wp), c_int(H), c_int(W),
                c_int(n), c_ll(SEG0), c_ll(1), c_ll(2))
        f = lambda k: torch.zeros(k, device=dev)
        tile, sp, stats, bad = f(tiles * 9 * n), f(tiles * (2 + 3 * n)), f(2 + 3 * n), torch.zeros(1, dtype=torch.int32, device=dev)
        hard, part, sums = f(B * H * W).view(B, H * W), f(tiles * 3 * n), f(B * 3 * n)
        dtile, dval, ktile, kpart, kstats = f(tiles * 9 * n), f(1), f(tiles * 9 * n), f(tiles * 2), f(2)
        dl, lo = torch.zeros_like(lp), f(4)
        out = (p(dl), c_int(npad), c_ll(dl.stride(0)), c_int(B), c_int(hp), c_int(wp), c_int(n), p(lo))
        ck = hip._check
        rows = [
            ("seg_loss_tile_kernel<false>", lambda: ck(lib.ifseg_seg_loss_tiles(*head, p(tile), p(sp), p(bad), c_float(0.1), s()), "t")),
            ("seg_loss_tile_kernel<true>", lambda: ck(lib.ifseg_seg_loss_tiles_weighted(*head, p(pw), c_ll(H * W), p(cw), c_int(1), p(tile), p(sp),
                                                                                        p(bad), c_float(0.1), s()), "t")),
            ("seg_hardness_kernel", lambda: ck(lib.ifseg_seg_hardness(*head, p(hard), c_ll(H * W), s()), "t")),
            ("seg_dice_sums_kernel", lambda: ck(lib.ifseg_seg_dice_sums(*head, p(part), s()), "t")),
            ("seg_dice_tile_kernel", lambda: ck(lib.ifseg_seg_dice_tiles(*head, p(sums), p(cw), c_float(3.0), c_float(1.0), p(dtile), p(dval), s()), "t")),
            ("seg_distill_tile_kernel", lambda: ck(lib.ifseg_seg_distill_tiles(*head[:3], p(te), c_int(npad), c_ll(te.stride(0)), *head[3:],
                                                                               c_float(2.0), c_int(0), p(ktile), p(kpart), s()), "t")),
            ("gather (ce)", lambda: ck(lib.ifseg_seg_loss_gather(p(tile), p(stats), *out, s()), "t")),
            ("gather_sum (ce, dice)", lambda: ck(lib.ifseg_seg_loss_gather_sum(p(tile), p(stats), p(dtile), p(dval), *out, s()), "t")),
            ("gather3 (ce, dice, kd)", lambda: ck(lib.ifseg_seg_loss_gather3(p(tile), p(stats), p(dtile), p(dval), p(ktile), p(kstats), c_float(1.5),
                                                                             c_float(2.0), *out, s()), "t")),
        ]
        # the statistics the later rows read, once: the CE and KD reductions, the Dice sums
        rows[0][1](); hip.reduce_parts(sp, stats, 1, tiles, 2 + 3 * n)
        rows[3][1](); hip.reduce_parts(part, sums, B, hp * wp, 3 * n)
        rows[5][1](); hip.reduce_parts(kpart, kstats, 1, tiles, 2)
        for label, fn in rows:
            print("n %3d  %-30s %8.1f [%8.1f, %8.1f] us" % ((n, label) + timeit(fn)), flush=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "time":
        run_time()
    elif mode in ("save", "cmp") and len(sys.argv) == 3:
        for shape in DC.SHAPES:
            run_case(*shape)
        if mode == "save":
            torch.save(outs, sys.argv[2])
            print("saved %d outputs of %s (%s) to %s" % (len(outs), ROOT, hip.LIB_PATH, sys.argv[2]))
        else:
            ref = torch.load(sys.argv[2])
            assert ref.keys() == outs.keys(), sorted(set(ref) ^ set(outs))
            ndiff = 0
            for k, t in outs.items():
                r = ref[k]
                assert r.dtype == t.dtype and r.shape == t.shape, (k, r.dtype, t.dtype, tuple(r.shape), tuple(t.shape))
                n = int((bits(t) != bits(r)).sum())
                ndiff += n > 0
                print("%-60s %-14s %9d  %s" % (k, str(t.dtype).replace("torch.", ""), t.numel(),
                                               "bit-equal" if n == 0 else "%d differ" % n))
            nzero = sum(1 for t in outs.values() if not bool(t.double().abs().sum() > 0))
            print("LOSS_BITS %d outputs (%d of them all zero), %s" % (len(outs), nzero, "all bit-equal" if ndiff == 0 else "%d differ" % ndiff))
            sys.exit(1 if ndiff else 0)
    else:
        sys.exit(__doc__)
