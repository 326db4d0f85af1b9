"""Conformance of the training-loss and optimizer kernels of csrc/loss.hip, csrc/dice.hip, csrc/distill.hip, csrc/ohem.hip and
csrc/optim.hip through the C ABI (ifseg_amd.hip.lib()), in the style of test_post_conformance_gpu.py: operands and outputs are views
inside larger allocations, 7s around the inputs (the row padding ldl > nseg, the eos row, the batch padding of the logits, the
target, the weight plane and the teacher included), a sentinel around the outputs that must be bit-identical after the call.
Data, fp64 references, the derived bounds and the case tables are in _loss_cases.py (its docstring holds the derivations);
test_loss_conformance_cpu.py checks them without a GPU.  Every test prints `worst |err| / bound` and where it occurred.

Part A: ifseg_seg_loss_tiles / _weighted: tile_partial and stats_part per element, histograms and bad_label exact.
Part B: ifseg_seg_dice_sums (+ ifseg_reduce_parts) and ifseg_seg_dice_tiles.      Part C: ifseg_seg_distill_tiles.
Part D: the gather's three doors: the exact integer stencil, the end-to-end gradient from real partials, the stated edge cases.
Part E: ifseg_seg_hardness per pixel, ifseg_ohem_select exact.                    Part F: ifseg_grad_sumsq_bf16, ifseg_adam_step.
Part G: argument rejection (return codes only).
profiles/loss_conformance.txt: the kernels seen in a trace of this file, the worst ratios, the wrong variants it catches.
"""
import ctypes

import numpy as np
import pytest
import torch

import _loss_cases as lc
from test_gemm_conformance_gpu import BAD_ARG, BAD_SHAPE, BF16, F32, GUARD, SENTINEL, _assert_surroundings, _bits, _dev, _flat_guarded

pytestmark = pytest.mark.gpu
I32, I64, U8 = torch.int32, torch.int64, torch.uint8
ci, cll, cf = ctypes.c_int, ctypes.c_longlong, ctypes.c_float


def P(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + off) if t is not None else None


def _ids(cases):
    return [c["id"] for c in cases]


def _lib():
    from ifseg_amd import hip
    _dev()
    return hip.lib(), hip._stream()


# ------------------------------------------------------------------------------------------------ plumbing
class _Buf:
    """a [B, rows, cols] view with strides (bs, ld, 1) inside one allocation filled with `fill`, 16 guard elements on both sides;
    `check` compares everything outside the view bit for bit with the state at construction (after `set`)"""

    def __init__(self, dev, dtype, B, rows, cols, ld=None, bs=None, fill=SENTINEL, values=None, zero=False):
        ld = cols if ld is None else ld
        bs = rows * ld if bs is None else bs
        self.shape, self.ld, self.bs = (B, rows, cols), ld, bs
        fill = (int(fill) & 0xFF if dtype == U8 else int(fill)) if dtype in (I32, I64, U8) else fill      # (uint8: 0xC0)
        self.full = torch.full((16 + B * bs + 16,), fill, dtype=dtype, device=dev)
        self.inner = lambda fl: fl.as_strided((B, rows, cols), (bs, ld, 1), 16)
        self.view = self.inner(self.full)
        if values is not None:
            self.view.copy_(torch.from_numpy(np.array(values)).to(dtype).reshape(B, rows, cols).to(dev))
        if zero:
            self.view.zero_()
        self.before = self.full.clone()

    def np(self):
        v = self.view
        return (v.double() if v.dtype in (F32, BF16) else v).cpu().numpy()

    def check(self, what):
        if self.full.dtype in (F32, BF16):
            return _assert_surroundings(self.full, self.before, self.inner, what)
        chk = self.full.clone()                                   # (integer outputs: compared as they are)
        self.inner(chk).copy_(self.inner(self.before))
        assert torch.equal(chk, self.before), "%s: wrote outside its output (guard band changed)" % what

    def unchanged(self):
        return torch.equal(_bits(self.full) if self.full.dtype in (F32, BF16) else self.full,
                           _bits(self.before) if self.full.dtype in (F32, BF16) else self.before)


def _flat(dev, n, dtype=F32, fill=SENTINEL, values=None, zero=False):
    return _Buf(dev, dtype, 1, 1, n, fill=fill, values=values, zero=zero)


def _within(what, got, ref, bound):
    r, at = lc.worst_ratio(got, ref, bound)
    print("[loss] %s: worst |err|/bound %.3f at %s" % (what, r, at))
    assert r <= 1.0, "%s: |err| is %.3f of the bound at %s (got %r, ref %r, bound %r)" % (
        what, r, at, np.asarray(got)[at], np.asarray(ref)[at], np.asarray(bound)[at])


def _exact(what, got, ref):
    bad = np.asarray(got) != np.asarray(ref)
    print("[loss] %s: exact, %d of %d differ" % (what, int(bad.sum()), bad.size))
    assert not bad.any(), "%s: %d of %d elements differ; first at %s: got %r, expected %r" % (
        what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), np.asarray(got)[bad][0], np.asarray(ref)[bad][0])


class _Tile:
    """the operands every tile entry shares, on the device inside guarded allocations"""

    def __init__(self, c, dev, teacher=False):
        d = lc.tile_data(c["id"])
        self.c, self.dev = c, dev
        B, hp, wp, n = c["B"], c["hp"], c["wp"], c["nseg"]
        self.B, self.hp, self.wp, self.n, self.H, self.W, self.P = B, hp, wp, n, 16 * hp, 16 * wp, hp * wp
        self.ldl = lc.ldl_of(c)
        pad = 24 if c["ldx"] else 0
        self.lg = _Buf(dev, BF16, B, self.P, n, ld=self.ldl, bs=(self.P + 1) * self.ldl + pad, fill=GUARD, values=d["logits"])
        self.tg = _Buf(dev, I64, B, 1, self.H * self.W, bs=self.H * self.W + 1 + (3 if c["ldx"] else 0), fill=GUARD, values=d["target"])
        self.te = None
        if teacher:
            strided = c["teacher"] == "strided"
            ldt = n + (5 if strided else 0)
            self.te = _Buf(dev, BF16, B, self.P, n, ld=ldt, bs=self.P * ldt + (9 if strided else 0), fill=GUARD, values=d["teacher"])
        self.tiles = B * hp * wp

    def head(self):
        return (P(self.lg.view), ci(self.ldl), cll(self.lg.bs), P(self.tg.view), cll(self.tg.bs), ci(self.B), ci(self.hp), ci(self.wp),
                ci(self.H), ci(self.W), ci(self.n), cll(lc.SEG0), cll(lc.PAD_ID), cll(lc.EOS_ID))

    def dlogits(self):
        return _Buf(self.dev, BF16, self.B, self.P + 1, self.ldl, bs=(self.P + 1) * self.ldl + (8 if self.c["ldx"] else 0))

    def inputs_untouched(self):
        assert self.lg.unchanged() and self.tg.unchanged() and (self.te is None or self.te.unchanged()), "an input was written"


def _reduce(inp, out, outer, parts, n):
    lib, s = _lib()
    assert lib.ifseg_reduce_parts(P(inp), P(out), ci(outer), ci(parts), cll(n), ci(0), ci(0), cf(1.0), s) == 0


def _ce_launch(t, weighted, cw=None, plane=None, norm_pixels=0, eps=None):
    """one CE tile launch -> (tile_partial, stats_part, bad) buffers"""
    lib, s = _lib()
    dev, n = t.dev, t.n
    tp = _flat(dev, t.tiles * 9 * n)
    sp = _flat(dev, t.tiles * (2 + 3 * n))
    bad = _flat(dev, 1, I32, zero=True)
    eps = t.c["eps"] if eps is None else eps
    if weighted:
        rc = lib.ifseg_seg_loss_tiles_weighted(*t.head(), P(plane.view) if plane is not None else None,
                                               cll(plane.bs if plane is not None else 0), P(cw.view) if cw is not None else None,
                                               ci(norm_pixels), P(tp.view), P(sp.view), P(bad.view), cf(eps), s)
    else:
        rc = lib.ifseg_seg_loss_tiles(*t.head(), P(tp.view), P(sp.view), P(bad.view), cf(eps), s)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return tp, sp, bad


def _ce_operands(t, weighted):
    c = t.c
    cw = lc.class_weights(c) if weighted else None
    plane = lc.pixel_plane(c) if weighted else None
    cwb = _flat(t.dev, t.n, fill=GUARD, values=cw) if cw is not None else None
    pb = _Buf(t.dev, U8, t.B, 1, t.H * t.W, bs=t.H * t.W + 5, fill=GUARD, values=plane) if plane is not None else None
    return cwb, pb


def _check_ce(what, t, tp, sp, bad, r):
    n = t.n
    for b in (tp, sp, bad):
        b.check(what)
    got_tp = tp.np().reshape(r["tp"].shape)
    spn = sp.np().reshape(t.B, t.hp, t.wp, 2 + 3 * n)
    assert np.isfinite(got_tp).all() and np.isfinite(spn).all(), "%s: a NaN or Inf" % what
    _within(what + " tile_partial", got_tp, r["tp"], r["tp_bound"])
    _within(what + " stats_part[0]", spn[..., 0], r["sp0"], r["sp0_bound"])
    if r["exact1"]:
        _exact(what + " stats_part[1]", spn[..., 1], r["sp1"])
    else:
        _within(what + " stats_part[1]", spn[..., 1], r["sp1"], r["sp1_bound"])
    _exact(what + " histograms", spn[..., 2:].reshape(r["hist"].shape), r["hist"])
    assert int(bad.np().reshape(-1)[0]) == lc.bad_label(t.c), "%s: bad_label" % what
    t.inputs_untouched()


# =========================================================================================================== part A
@pytest.mark.parametrize("case", lc.TILE_CASES, ids=_ids(lc.TILE_CASES))
def test_ce_tiles(case):
    """seg_loss_tile_kernel<false> against fp64; with neutral weights seg_loss_tile_kernel<true> gives the same bits"""
    t = _Tile(case, _dev())
    tp, sp, bad = _ce_launch(t, False)
    r = lc.ce_ref(case["id"], False)
    _check_ce("A %s plain" % case["id"], t, tp, sp, bad, r)
    if not r["valid"].any():
        assert not tp.np().any() and not sp.np().reshape(t.tiles, -1)[:, :2].any(), "no valid pixel: loss and gradient are exactly 0"
    # neutral weights (no plane, no class weights): the counts and histograms are the unweighted kernel's; at eps == 0 so is every
    # other bit (soft = hot = 1, unif = 0: each extra operation of the weighted kernel multiplies by 1 or adds a zero)
    tp2, sp2, bad2 = _ce_launch(t, True)
    s1, s2 = (x.np().reshape(t.tiles, -1) for x in (sp, sp2))
    assert np.array_equal(s1[:, 1:], s2[:, 1:]) and torch.equal(bad.full, bad2.full), "neutral weights: counts or histograms differ"
    _check_ce("A %s neutral weights" % case["id"], t, tp2, sp2, bad2, r)
    if case["eps"] == 0.0:
        assert torch.equal(_bits(tp.full), _bits(tp2.full)) and torch.equal(_bits(sp.full), _bits(sp2.full)), \
            "neutral weights, eps == 0: the weighted kernel differs from the unweighted one"


WEIGHTED = [c for c in lc.TILE_CASES if c["weighted"]]


@pytest.mark.parametrize("case", WEIGHTED, ids=_ids(WEIGHTED))
def test_ce_tiles_weighted(case):
    t = _Tile(case, _dev())
    cwb, pb = _ce_operands(t, True)
    tp, sp, bad = _ce_launch(t, True, cwb, pb, case["norm_pixels"])
    r = lc.ce_ref(case["id"])
    _check_ce("A %s weighted" % case["id"], t, tp, sp, bad, r)
    assert (cwb is None or cwb.unchanged()) and (pb is None or pb.unchanged())
    if case["cw"] == "zero":
        assert not tp.np().any() and not sp.np().reshape(t.tiles, -1)[:, :2].any(), "all-zero class weights: exactly 0"


def _gather(t, ce=None, stats=None, dice=None, dval=None, kd=None, kstats=None, kd_w=0.0, kd_t=0.0, door=3):
    """one gather launch through door 1 (CE alone), 2 (gather_sum) or 3 (gather3) -> (dlogits buffer, loss_out buffer)"""
    lib, s = _lib()
    dl = t.dlogits()
    nout = {1: 1, 2: 3, 3: 4}[door]
    lo = _flat(t.dev, nout)
    out = (P(dl.view), ci(t.ldl), cll(dl.bs), ci(t.B), ci(t.hp), ci(t.wp), ci(t.n), P(lo.view), s)
    p = lambda b: P(b.view) if b is not None else None
    if door == 1:
        rc = lib.ifseg_seg_loss_gather(p(ce), p(stats), *out)
    elif door == 2:
        rc = lib.ifseg_seg_loss_gather_sum(p(ce), p(stats), p(dice), p(dval), *out)
    else:
        rc = lib.ifseg_seg_loss_gather3(p(ce), p(stats), p(dice), p(dval), p(kd), p(kstats), cf(kd_w), cf(kd_t), *out)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return dl, lo


def _check_zeros(what, t, dl):
    """the contracted zeros: the class columns [nseg, ldl) and the eos row, exactly (+0.0 bits)"""
    dl.check(what)
    b = _bits(dl.view)
    assert not b[:, :, t.n:].any(), "%s: a class column in [nseg, ldl) is not +0.0" % what
    assert not b[:, t.P].any(), "%s: the eos row is not +0.0" % what


def test_doubling_the_plane_gives_the_same_dlogits_bits():
    case = lc.CASE["g2x2-n17-bad"]
    t = _Tile(case, _dev())
    cwb, _ = _ce_operands(t, True)
    half = lc.pixel_plane(case) // 2
    outs = []
    for plane in (half, half * 2):
        pb = _Buf(t.dev, U8, t.B, 1, t.H * t.W, bs=t.H * t.W + 5, fill=GUARD, values=plane)
        tp, sp, _ = _ce_launch(t, True, cwb, pb, 0)
        stats = _flat(t.dev, 2 + 3 * t.n)
        _reduce(sp.view, stats.view, 1, t.tiles, 2 + 3 * t.n)
        dl, lo = _gather(t, tp, stats, door=1)
        outs.append((dl, lo))
    assert torch.equal(_bits(outs[0][0].full), _bits(outs[1][0].full)) and bool(outs[0][0].view.float().abs().sum() > 0)
    assert torch.equal(_bits(outs[0][1].full), _bits(outs[1][1].full))


# =========================================================================================================== part B
def _dice_launch(t):
    lib, s = _lib()
    c, n = t.c, t.n
    part = _flat(t.dev, t.tiles * 3 * n)
    assert lib.ifseg_seg_dice_sums(*t.head(), P(part.view), s) == 0
    sums = _flat(t.dev, t.B * 3 * n)
    _reduce(part.view, sums.view, t.B, t.P, 3 * n)
    w = lc.class_weights(c, dice=True)
    cwb = _flat(t.dev, n, fill=GUARD, values=w) if w is not None else None
    tp, val = _flat(t.dev, t.tiles * 9 * n), _flat(t.dev, 1)
    assert lib.ifseg_seg_dice_tiles(*t.head(), P(sums.view), P(cwb.view) if cwb is not None else None, cf(lc.DICE_WEIGHT),
                                    cf(c["smooth"]), P(tp.view), P(val.view), s) == 0
    torch.cuda.synchronize()
    return part, sums, tp, val


@pytest.mark.parametrize("case", lc.DICE_CASES, ids=_ids(lc.DICE_CASES))
def test_dice(case):
    t = _Tile(case, _dev())
    part, sums, tp, val = _dice_launch(t)
    what = "B %s" % case["id"]
    r = lc.dice_ref(case["id"])
    for b in (part, sums, tp, val):
        b.check(what)
    got = sums.np().reshape(r["sums"].shape)
    _within(what + " sums", got, r["sums"], r["sums_bound"])
    _exact(what + " Y", got[:, 2], r["sums"][:, 2])
    gtp = tp.np().reshape(r["tp"].shape)
    assert np.isfinite(gtp).all()
    _within(what + " tile_partial", gtp, r["tp"], r["tp_bound"])
    _within(what + " dice_out", val.np().reshape(1), np.array([r["value"]]), np.array([r["value_bound"]]))
    inv = ~r["valid"].reshape(t.B, -1).any(1)
    if inv.any():
        assert not gtp[inv].any(), "%s: a sample without a valid pixel has a gradient" % what
        assert (got[inv] == 0).all()
    t.inputs_untouched()


# =========================================================================================================== part C
def _kd_launch(t):
    lib, s = _lib()
    c, n = t.c, t.n
    tp, part = _flat(t.dev, t.tiles * 9 * n), _flat(t.dev, t.tiles * 2)
    h = t.head()
    assert lib.ifseg_seg_distill_tiles(*h[:3], P(t.te.view), ci(t.te.ld), cll(t.te.bs), *h[3:], cf(c["T"]), ci(1 if c["mask_all"] else 0),
                                       P(tp.view), P(part.view), s) == 0
    torch.cuda.synchronize()
    return tp, part


@pytest.mark.parametrize("case", lc.KD_CASES, ids=_ids(lc.KD_CASES))
def test_distill(case):
    t = _Tile(case, _dev(), teacher=True)
    tp, part = _kd_launch(t)
    what = "C %s" % case["id"]
    r = lc.kd_ref(case["id"])
    tp.check(what)
    part.check(what)
    gtp, gp = tp.np().reshape(r["tp"].shape), part.np().reshape(t.B, t.hp, t.wp, 2)
    assert np.isfinite(gtp).all() and np.isfinite(gp).all()
    _within(what + " tile_partial", gtp, r["tp"], r["tp_bound"])
    _within(what + " kd_part[0]", gp[..., 0], r["kl"], r["kl_bound"])
    _exact(what + " kd_part[1]", gp[..., 1], r["count"])
    if case["teacher"] == "same":
        assert not gp[..., 0].any(), "%s: the KL of equal logits is not exactly 0" % what
    t.inputs_untouched()


# =========================================================================================================== part D
@pytest.mark.parametrize("hp,wp,B", lc.STENCIL_GRIDS, ids=["%dx%d-B%d" % g for g in lc.STENCIL_GRIDS])
def test_gather_stencil_is_exact(hp, wp, B):
    """small-integer partials, powers of two for Z, N, w and T: every fp32 operation is exact, dlogits equals the numpy stencil bit
    for bit -- which nine partials a cell sums, the clipping at the edges, the ky * 3 + kx layout; all three doors"""
    n = 5
    c = dict(id="stencil", B=B, hp=hp, wp=wp, nseg=n, ldx=8)
    dev = _dev()
    t = _Tile.__new__(_Tile)
    t.c, t.dev, t.B, t.hp, t.wp, t.n, t.P, t.ldl = c, dev, B, hp, wp, n, hp * wp, 16
    ce, di, kd = (lc.stencil_partials(B, hp, wp, n, s) for s in (1, 2, 3))
    bce, bdi, bkd = (_flat(dev, x.size, fill=GUARD, values=x.reshape(-1)) for x in (ce, di, kd))
    stats = _flat(dev, 2 + 3 * n, fill=GUARD, values=np.float32([3.0, 4.0] + [0.0] * (3 * n)))
    dval = _flat(dev, 1, fill=GUARD, values=np.float32([0.5]))
    kst = _flat(dev, 2, fill=GUARD, values=np.float32([1.0, 8.0]))
    g = lambda x: lc.stencil_gather(x.astype(np.float64))
    runs = {
        "door1 ce": (dict(ce=bce, stats=stats, door=1), g(ce) / 4, [0.75]),
        "door2 ce+dice": (dict(ce=bce, stats=stats, dice=bdi, dval=dval, door=2), g(ce) / 4 + g(di), [1.25, 0.75, 0.5]),
        "door2 dice": (dict(dice=bdi, dval=dval, door=2), g(di), [0.5, 0.0, 0.5]),
        "door3 all": (dict(ce=bce, stats=stats, dice=bdi, dval=dval, kd=bkd, kstats=kst, kd_w=2.0, kd_t=2.0),
                      g(ce) / 4 + g(di) + g(kd) * 0.5, [2.25, 0.75, 0.5, 1.0]),
        "door3 kd": (dict(kd=bkd, kstats=kst, kd_w=2.0, kd_t=2.0), g(kd) * 0.5, [1.0, 0.0, 0.0, 1.0]),
        "door3 ce+kd": (dict(ce=bce, stats=stats, kd=bkd, kstats=kst, kd_w=2.0, kd_t=2.0), g(ce) / 4 + g(kd) * 0.5, [1.75, 0.75, 0.0, 1.0]),
    }
    for name, (kw, want, loss) in runs.items():
        dl, lo = _gather(t, **kw)
        what = "D stencil %dx%d B%d %s" % (hp, wp, B, name)
        _check_zeros(what, t, dl)
        lo.check(what)
        got = dl.np()[:, :t.P, :n].reshape(want.shape)
        _exact(what, got, lc.bf16_round(want).astype(np.float64))
        _exact(what + " loss_out", lo.np().reshape(-1), np.array(loss))
    for b in (bce, bdi, bkd, stats, dval, kst):
        assert b.unchanged()


_real = {}


def _real_partials(case):
    """the tile kernels of parts A, B and C run once per case; their outputs feed the seven source subsets"""
    cid = case["id"]
    if cid not in _real:
        t = _Tile(case, _dev(), teacher=True)
        cwb, pb = _ce_operands(t, case["weighted"])
        tp, sp, _ = _ce_launch(t, case["weighted"], cwb, pb, case["norm_pixels"])
        stats = _flat(t.dev, 2 + 3 * t.n)
        _reduce(sp.view, stats.view, 1, t.tiles, 2 + 3 * t.n)
        _, _, dtp, dval = _dice_launch(t)
        ktp, kpart = _kd_launch(t)
        kst = _flat(t.dev, 2)
        _reduce(kpart.view, kst.view, 1, t.tiles, 2)
        torch.cuda.synchronize()
        _real[cid] = (t, tp, stats, dtp, dval, ktp, kst)
    return _real[cid]


@pytest.mark.parametrize("sub", range(1, 8), ids=lambda s: "sources%d" % s)
@pytest.mark.parametrize("case", lc.GATHER_CASES, ids=_ids(lc.GATHER_CASES))
def test_gather_from_real_partials(case, sub):
    """dlogits per element against the fp64 end-to-end gradient of CE + Dice + w KD, every non-empty subset of the sources (bit 0:
    CE, 1: Dice, 2: KD), through the narrowest door that takes the subset and through ifseg_seg_loss_gather3"""
    t, tp, stats, dtp, dval, ktp, kst = _real_partials(case)
    use = (bool(sub & 1), bool(sub & 2), bool(sub & 4))
    ref, bound, loss, lb = lc.gather_ref(case["id"], *use)
    kw = {}
    if use[0]:
        kw.update(ce=tp, stats=stats)
    if use[1]:
        kw.update(dice=dtp, dval=dval)
    if use[2]:
        kw.update(kd=ktp, kstats=kst, kd_w=lc.KD_W, kd_t=case["T"])
    doors = [3] + ([1] if sub == 1 else []) + ([2] if use[1] and not use[2] else [])
    for door in doors:
        dl, lo = _gather(t, door=door, **kw)
        what = "D %s sources %d door %d" % (case["id"], sub, door)
        _check_zeros(what, t, dl)
        lo.check(what)
        _within(what + " dlogits", dl.np()[:, :t.P, :t.n].reshape(ref.shape), ref, bound)
        nout = {1: 1, 2: 3, 3: 4}[door]
        _within(what + " loss_out", lo.np().reshape(-1), loss[:nout], lb[:nout])


def test_gather_edge_cases():
    """stats[1] == 0 and kd N == 0: the term and its gradient are exactly 0; a lone source keeps the sign of a zero"""
    dev = _dev()
    hp, wp, B, n = 2, 2, 1, 5
    t = _Tile.__new__(_Tile)
    t.c, t.dev, t.B, t.hp, t.wp, t.n, t.P, t.ldl = dict(ldx=8), dev, B, hp, wp, n, hp * wp, 16
    ce = lc.stencil_partials(B, hp, wp, n, 1)
    bce = _flat(dev, ce.size, fill=GUARD, values=ce.reshape(-1))
    zstats = _flat(dev, 2 + 3 * n, fill=GUARD, values=np.float32([3.0, 0.0] + [0.0] * (3 * n)))
    kst0 = _flat(dev, 2, fill=GUARD, values=np.float32([5.0, 0.0]))
    for door, kw in ((1, dict(ce=bce, stats=zstats)), (3, dict(ce=bce, stats=zstats, kd=bce, kstats=kst0, kd_w=2.0, kd_t=2.0))):
        dl, lo = _gather(t, door=door, **kw)
        _check_zeros("D edge Z=0 door %d" % door, t, dl)
        assert not dl.np().any() and not lo.np().any(), "Z == 0 (and N == 0): loss and gradient must be exactly 0"
    # CE alone, one partial of -2^-126 with Z = 2^30: the product underflows to -0.0 and nothing is added to it afterwards
    tiny = np.zeros((B, hp, wp, 9, n), dtype=np.float32)
    tiny[0, 0, 0, 4, 2] = np.float32(-2.0 ** -126)
    bt = _flat(dev, tiny.size, fill=GUARD)
    bt.view.copy_(torch.from_numpy(tiny.reshape(1, 1, -1)).to(dev))
    st4 = _flat(dev, 2 + 3 * n, fill=GUARD, values=np.float32([3.0, 2.0 ** 30] + [0.0] * (3 * n)))
    zero = _flat(dev, tiny.size, fill=GUARD, zero=True)
    dv = _flat(dev, 1, fill=GUARD, values=np.float32([0.0]))
    for door in (1, 3):
        dl, _ = _gather(t, ce=bt, stats=st4, door=door)
        assert int(_bits(dl.view)[0, 0, 2]) == -32768, "a lone source lost the sign of its zero (door %d)" % door
    dl, _ = _gather(t, ce=bt, stats=st4, dice=zero, dval=dv, door=3)
    assert int(_bits(dl.view)[0, 0, 2]) == 0                      # a second source adds its +0.0


# =========================================================================================================== part E
@pytest.mark.parametrize("case", lc.TILE_CASES, ids=_ids(lc.TILE_CASES))
def test_hardness(case):
    lib, s = _lib()
    t = _Tile(case, _dev())
    hw = t.H * t.W
    out = _Buf(t.dev, F32, t.B, 1, hw, bs=hw + 3)
    assert lib.ifseg_seg_hardness(*t.head(), P(out.view), cll(out.bs), s) == 0
    torch.cuda.synchronize()
    what = "E %s hardness" % case["id"]
    out.check(what)
    ref, bound = lc.hardness_ref(case["id"])
    got = out.np().reshape(ref.shape)
    assert (got[ref < 0] == -1.0).all() and (got[ref >= 0] >= 0).all(), "%s: -1.0f exactly on the invalid pixels, and only there" % what
    assert got.max() <= 1.0
    _within(what, got, ref, bound)
    t.inputs_untouched()


@pytest.mark.parametrize("case", lc.OHEM_CASES, ids=_ids(lc.OHEM_CASES))
def test_ohem_select(case):
    from ifseg_amd import hip
    lib, s = _lib()
    dev = _dev()
    h, w = lc.ohem_plane(case["id"])
    B, N = case["B"], case["N"]
    hb = _flat(dev, B * N, fill=GUARD)
    hb.view.copy_(torch.from_numpy(h.reshape(1, 1, -1).copy()).to(dev))          # bit for bit (NaN, -0.0)
    hb.before = hb.full.clone()
    wb = _flat(dev, B * N, U8, fill=GUARD, values=w.reshape(-1)) if w is not None else None
    work = torch.zeros(hip.OHEM_WORK_WORDS + 4, dtype=I64, device=dev)
    work[-4:] = int(SENTINEL)
    work0 = work.clone()
    want_plane, want_info = lc.ohem_expected(h, B, case["thresh"], case["min_kept"], w)
    for rep in range(2):
        out, info = _flat(dev, B * N, U8), _flat(dev, 4, I64)
        rc = lib.ifseg_ohem_select(P(hb.view), ci(B), cll(N), cf(case["thresh"]), cll(case["min_kept"]),
                                   P(wb.view) if wb is not None else None, P(out.view), P(info.view), P(work), s)
        assert rc == 0, rc
        torch.cuda.synchronize()
        what = "E ohem %s call %d" % (case["id"], rep)
        out.check(what)
        info.check(what)
        _exact(what + " info", info.np().reshape(-1), want_info)
        _exact(what + " plane", out.np().reshape(want_plane.shape), want_plane)
        assert torch.equal(work, work0), "%s: the workspace is not as the call found it" % what
    assert hb.unchanged() and (wb is None or wb.unchanged())


# =========================================================================================================== part F
@pytest.mark.parametrize("case", lc.SUMSQ_CASES, ids=_ids(lc.SUMSQ_CASES))
def test_grad_sumsq(case):
    lib, s = _lib()
    dev = _dev()
    n = case["n"]
    g = _flat(dev, max(n, 8), BF16, fill=GUARD)
    if n:
        g.view[0, 0, :n].copy_(torch.from_numpy(lc.sumsq_data(n, case["data"]).copy()).to(BF16).to(dev))
    g.before = g.full.clone()
    ws, out = _flat(dev, 1024), _flat(dev, 1)
    assert lib.ifseg_grad_sumsq_bf16(P(g.view), cll(n), P(ws.view), P(out.view), s) == 0
    torch.cuda.synchronize()
    what = "F sumsq %s" % case["id"]
    ws.check(what)
    out.check(what)
    assert g.unchanged()
    if n == 0:
        assert _bits(out.view).item() == 0, "n == 0 writes 0"
        return
    ref, bound = lc.sumsq_ref(n, case["data"])
    _within(what, out.np().reshape(1), np.array([ref]), np.array([bound]))


def _adam_buffers(dev, d, n, ema):
    bufs = {k: _flat(dev, n, F32, values=d[k]) for k in "pmv"}
    bufs["g"] = _flat(dev, n, BF16, fill=GUARD, values=d["g"])
    bufs["p16"] = _flat(dev, n, BF16)
    bufs["p16"].view.copy_(bufs["p"].view.to(BF16))
    bufs["p16"].before = bufs["p16"].full.clone()
    if ema:
        bufs["e32"] = _flat(dev, n, F32, values=d["p"] * np.float32(0.5))
        bufs["e16"] = _flat(dev, n, BF16)
        bufs["e16"].view.copy_(bufs["e32"].view.to(BF16))
        bufs["e16"].before = bufs["e16"].full.clone()
    return bufs


def _adam_call(c, b, n, sumsq, overflow, hyper, step=None, max_norm=None, decoy=False):
    lib, s = _lib()
    lr, gs = (0.123, 77.0) if decoy else (c["lr"], lc.GSCALE)
    tail = (cll(n), cf(lr), cf(lc.B1), cf(lc.B2), cf(lc.ADAM_EPS), cf(c["wd"]), ci(c["step"] if step is None else step), cf(gs),
            cf(max_norm), P(sumsq), P(overflow), P(hyper))
    head = (P(b["p"].view), P(b["g"].view), P(b["m"].view), P(b["v"].view), P(b["p16"].view))
    if "e32" in b:
        return lib.ifseg_adam_ema_step(*head, P(b["e32"].view), P(b["e16"].view), *tail, cf(0.75), cf(0.25), s)
    return lib.ifseg_adam_step(*head, *tail, s)


@pytest.mark.parametrize("case", lc.ADAM_CASES, ids=_ids(lc.ADAM_CASES))
def test_adam_step(case):
    """p32, m, v per element against fp64 Adam with double scalars; p16 is the bf16 rounding of the kernel's own p32"""
    dev = _dev()
    d = lc.adam_data(case["id"])
    n = case["n"]
    b = _adam_buffers(dev, d, n, case["ema"])
    sumsq = torch.tensor([float(d["sumsq"])], dtype=F32, device=dev) if d["use_sumsq"] else None
    overflow = torch.zeros(1, dtype=I32, device=dev)
    hyper = None
    if case["hyper"]:
        h = list(lc.adam_scalars(case)[2]) + ([0.75, 0.25] if case["ema"] else [])
        hyper = torch.tensor(np.float32(h), device=dev)
    assert _adam_call(case, b, n, sumsq, overflow, hyper, max_norm=d["max_norm"], decoy=case["hyper"]) == 0
    torch.cuda.synchronize()
    what = "F adam %s" % case["id"]
    r = lc.adam_ref(case["id"])
    for k in b:
        b[k].check(what)
    assert b["g"].unchanged() and int(overflow) == 0
    for k in "pmv":
        got = b[k].np().reshape(-1)
        assert np.isfinite(got).all()
        _within("%s %s (step %d)" % (what, k, case["step"]), got, r[k], r["d" + k])
    assert torch.equal(_bits(b["p16"].view), _bits(b["p"].view.to(BF16))), "%s: p16 is not the bf16 rounding of p32" % what
    _within(what + " p16", b["p16"].np().reshape(-1), r["p"], lc.U_BF16 * np.abs(r["p"]) + (1 + lc.U_BF16) * r["dp"])
    if case["ema"]:
        q = b["p16"].view.float()
        e0 = torch.from_numpy(d["p"] * np.float32(0.5)).to(dev).view_as(q)
        e64 = (e0.double() * 0.75 + 0.25 * q.double()).cpu().numpy().reshape(-1)
        _within(what + " e32", b["e32"].np().reshape(-1), e64, 3 * lc.U * (np.abs(e64) + np.abs(0.25 * q.double().cpu().numpy().reshape(-1))))
        assert torch.equal(_bits(b["e16"].view), _bits(b["e32"].view.to(BF16)))


@pytest.mark.parametrize("poison", [float("inf"), float("nan")], ids=["inf", "nan"])
@pytest.mark.parametrize("ema", [False, True], ids=["plain", "ema"])
def test_overflow_skips_the_update(poison, ema):
    """the sum of squares of a gradient with an Inf / a NaN is not finite; the step it feeds leaves every buffer bit-identical and
    raises the flag"""
    lib, s = _lib()
    dev = _dev()
    case = next(c for c in lc.ADAM_CASES if c["id"] == "n1027-step10-value")
    d = lc.adam_data(case["id"])
    n = case["n"]
    b = _adam_buffers(dev, d, n, ema)
    b["g"].view[0, 0, 517] = poison
    for k in b:
        b[k].before = b[k].full.clone()
    ws, ss = _flat(dev, 1024), _flat(dev, 1)
    assert lib.ifseg_grad_sumsq_bf16(P(b["g"].view), cll(n), P(ws.view), P(ss.view), s) == 0
    overflow = torch.zeros(1, dtype=I32, device=dev)
    assert _adam_call(case, b, n, ss.view, overflow, None, max_norm=1.0) == 0
    torch.cuda.synchronize()
    assert not np.isfinite(ss.np()).any() and int(overflow) == 1
    for k in b:
        assert b[k].unchanged(), k


# =========================================================================================================== part G
def test_optimizer_entry_point_refusals():
    """ifseg_adam_step / ifseg_adam_ema_step / ifseg_grad_sumsq_bf16: null and misaligned pointers are IFSEG_ERR_BAD_ARG before any
    launch; every pointer lies inside a live allocation large enough for the call as given; the buffers keep their bits"""
    lib, s = _lib()
    dev = _dev()
    n = 64
    f = lambda: torch.full((n + 16,), 7.0, dtype=F32, device=dev)
    h = lambda: torch.full((n + 16,), 7.0, dtype=BF16, device=dev)
    t = dict(p32=f(), g=h(), m=f(), v=f(), p16=h(), e32=f(), e16=h())
    names = ("p32", "g", "m", "v", "p16", "e32", "e16")

    def call(ema, nn=n, **ptr):
        a = {k: ptr.get(k, P(t[k])) for k in names}
        tail = (cll(nn), cf(1e-3), cf(0.9), cf(0.999), cf(1e-8), cf(0.1), ci(3), cf(1.0), cf(0.0), None, None, None)
        if ema:
            return lib.ifseg_adam_ema_step(a["p32"], a["g"], a["m"], a["v"], a["p16"], a["e32"], a["e16"], *tail, cf(0.5), cf(0.5), s)
        return lib.ifseg_adam_step(a["p32"], a["g"], a["m"], a["v"], a["p16"], *tail, s)

    for ema in (False, True):
        mine = names if ema else names[:5]
        for k in mine:
            assert call(ema, **{k: None}) == BAD_ARG, (ema, k, "null")
            step = 4 if t[k].dtype == F32 else 2                      # one element: 4 / 2 bytes off a 16 / 8 byte boundary
            assert call(ema, **{k: P(t[k], step)}) == BAD_ARG, (ema, k, "misaligned")
            if t[k].dtype == F32:
                assert call(ema, **{k: P(t[k], 8)}) == BAD_ARG, (ema, k, "8 of 16")
        assert call(ema, nn=0, p32=None) == 0 and call(ema, nn=-5, g=None) == 0           # n <= 0: nothing to do, nothing read
    ws, out = torch.full((1024 + 8,), 7.0, device=dev), torch.full((8,), 7.0, device=dev)
    sumsq = lambda g=P(t["g"]), nn=n, w=P(ws), o=P(out): lib.ifseg_grad_sumsq_bf16(g, cll(nn), w, o, s)
    assert sumsq(g=None) == BAD_ARG and sumsq(w=None) == BAD_ARG and sumsq(o=None) == BAD_ARG
    assert sumsq(g=P(t["g"], 2)) == BAD_ARG and sumsq(g=P(t["g"], 8)) == BAD_ARG and sumsq(nn=-1) == BAD_ARG
    assert sumsq(w=P(ws, 2)) == BAD_ARG and sumsq(o=P(out, 1)) == BAD_ARG
    torch.cuda.synchronize()
    for k in names:
        assert bool((t[k] == 7.0).all()), k
    assert bool((ws == 7.0).all()) and bool((out == 7.0).all())
    assert sumsq(nn=0) == 0
    torch.cuda.synchronize()
    assert float(out[0]) == 0.0 and bool((out[1:] == 7.0).all())


def test_seg_loss_refusals_no_other_test_names():
    """the refusals of csrc/seg_tile.h::check_tile_args, loss.hip, dice.hip, distill.hip and ohem.hip that the four
    test_entry_point_refusals do not reach: misaligned logits / target, hp / wp < 1, ldl < nseg, batch strides below a sample,
    label_smoothing outside [0, 1], the weighted entry's plane stride and class-weight alignment, the hardness plane, the select"""
    from ifseg_amd import hip
    lib, s = _lib()
    dev = _dev()
    B, hp, wp, n = 2, 2, 2, 17
    H, W, ldl = 16 * hp, 16 * wp, 24
    lg = torch.full((B * (hp * wp + 1) * ldl + 8,), 7.0, dtype=BF16, device=dev)
    tg = torch.full((B * (H * W + 1) + 8,), lc.SEG0, dtype=I64, device=dev)
    tiles = B * hp * wp
    tp = torch.full((tiles * 9 * n + 8,), 7.0, device=dev)
    sp = torch.full((tiles * (2 + 3 * n) + 8,), 7.0, device=dev)
    bad = torch.zeros(1, dtype=I32, device=dev)
    plane = torch.full((B * H * W + 8,), 7, dtype=U8, device=dev)
    cw = torch.full((n + 8,), 7.0, device=dev)
    hard = torch.full((B * H * W + 8,), 7.0, device=dev)

    def head(lgp=P(lg), tgp=P(tg), ldl_=ldl, lbs=(hp * wp + 1) * ldl, tbs=H * W + 1, B_=B, hp_=hp, wp_=wp, H_=H, W_=W, n_=n):
        return (lgp, ci(ldl_), cll(lbs), tgp, cll(tbs), ci(B_), ci(hp_), ci(wp_), ci(H_), ci(W_), ci(n_), cll(lc.SEG0), cll(1), cll(2))

    plain = lambda eps=0.0, **kw: lib.ifseg_seg_loss_tiles(*head(**kw), P(tp), P(sp), P(bad), cf(eps), s)
    wtd = lambda eps=0.0, pl=P(plane), pbs=H * W, cwp=P(cw), **kw: lib.ifseg_seg_loss_tiles_weighted(
        *head(**kw), pl, cll(pbs), cwp, ci(0), P(tp), P(sp), P(bad), cf(eps), s)
    hd = lambda out=P(hard), hbs=H * W, **kw: lib.ifseg_seg_hardness(*head(**kw), out, cll(hbs), s)
    dsum = lambda out=P(tp), **kw: lib.ifseg_seg_dice_sums(*head(**kw), out, s)
    for fn in (plain, wtd, hd, dsum):
        for kw in (dict(lgp=P(lg, 1)), dict(tgp=P(tg, 4)), dict(lgp=None), dict(tgp=None), dict(tbs=H * W - 1),
                   dict(lbs=hp * wp * ldl - 1)):
            assert fn(**kw) == BAD_ARG, (fn, kw)
        for kw in (dict(hp_=0, H_=0), dict(wp_=0, W_=0), dict(ldl_=n - 1), dict(hp_=-1, H_=-16)):
            assert fn(**kw) == BAD_SHAPE, (fn, kw)
    for eps in (-0.01, 1.01, float("nan"), float("inf")):
        assert plain(eps=eps) == BAD_ARG and wtd(eps=eps) == BAD_ARG, eps
    assert wtd(pbs=H * W - 1) == BAD_ARG and wtd(cwp=P(cw, 2)) == BAD_ARG
    assert hd(out=None) == BAD_ARG and hd(out=P(hard, 2)) == BAD_ARG and hd(hbs=H * W - 1) == BAD_ARG
    assert dsum(out=P(tp, 2)) == BAD_ARG
    # dice pass B and the distillation tiles: outputs missing or misaligned, the teacher's batch stride
    sums, val = torch.ones(B * 3 * n + 8, device=dev), torch.full((8,), 7.0, device=dev)
    dt = lambda sm=P(sums), out=P(tp), vo=P(val): lib.ifseg_seg_dice_tiles(*head(), sm, None, cf(0.5), cf(1.0), out, vo, s)
    assert dt(sm=None) == BAD_ARG and dt(out=None) == BAD_ARG and dt(vo=None) == BAD_ARG
    assert dt(sm=P(sums, 2)) == BAD_ARG and dt(out=P(tp, 2)) == BAD_ARG and dt(vo=P(val, 2)) == BAD_ARG
    h = head()
    kd = lambda tebs=hp * wp * ldl, out=P(tp), pt=P(sp): lib.ifseg_seg_distill_tiles(*h[:3], P(lg), ci(ldl), cll(tebs), *h[3:], cf(1.0), ci(0),
                                                                                      out, pt, s)
    assert kd(tebs=hp * wp * ldl - 1) == BAD_ARG and kd(out=P(tp, 2)) == BAD_ARG and kd(pt=P(sp, 2)) == BAD_ARG
    # the gather's two checked doors: a batch stride below a sample, misaligned pointers
    dl = torch.full((B * (hp * wp + 1) * ldl + 8,), 7.0, dtype=BF16, device=dev)
    lo = torch.full((8,), 7.0, device=dev)
    gs = lambda dlp=P(dl), dbs=(hp * wp + 1) * ldl, lop=P(lo), dv=P(val): lib.ifseg_seg_loss_gather_sum(
        None, None, P(tp), dv, dlp, ci(ldl), cll(dbs), ci(B), ci(hp), ci(wp), ci(n), lop, s)
    g3 = lambda dlp=P(dl), dbs=(hp * wp + 1) * ldl, lop=P(lo), dv=P(val): lib.ifseg_seg_loss_gather3(
        None, None, P(tp), dv, None, None, cf(0.0), cf(0.0), dlp, ci(ldl), cll(dbs), ci(B), ci(hp), ci(wp), ci(n), lop, s)
    for fn in (gs, g3):
        assert fn(dbs=(hp * wp + 1) * ldl - 1) == BAD_ARG and fn(dlp=P(dl, 1)) == BAD_ARG and fn(lop=P(lo, 2)) == BAD_ARG
        assert fn(dv=None) == BAD_ARG and fn(dlp=None) == BAD_ARG and fn(lop=None) == BAD_ARG
    # the select
    N = 130
    hv = torch.full((2 * N + 8,), 0.5, device=dev)
    out8 = torch.full((2 * N + 8,), 7, dtype=U8, device=dev)
    info = torch.full((8,), 7, dtype=I64, device=dev)
    work = torch.zeros(hip.OHEM_WORK_WORDS + 2, dtype=I64, device=dev)
    sel = lambda hp_=P(hv), B_=2, N_=N, th=0.7, mk=10, o=P(out8), i_=P(info), w=P(work): lib.ifseg_ohem_select(
        hp_, ci(B_), cll(N_), cf(th), cll(mk), None, o, i_, w, s)
    for kw in (dict(hp_=None), dict(o=None), dict(i_=None), dict(w=None), dict(hp_=P(hv, 2)), dict(i_=P(info, 4)), dict(w=P(work, 4)),
               dict(th=-0.1), dict(th=1.5), dict(th=float("nan")), dict(mk=-1), dict(mk=1 << 40)):
        assert sel(**kw) == BAD_ARG, kw
    for kw in (dict(B_=0), dict(N_=0), dict(B_=1 << 20), dict(B_=2, N_=1 << 30)):
        assert sel(**kw) == BAD_SHAPE, kw
    torch.cuda.synchronize()
    for x in (tp, sp, cw, hard, val, lo):
        assert bool((x == 7.0).all())
    assert bool((dl == 7.0).all()) and bool((out8 == 7).all()) and bool((info == 7).all()) and not work.any() and int(bad) == 0
