"""GPU: the distillation term (csrc/distill.hip) against its specification -- `hip.seg_distill` and `hip.seg_loss_distill` against
`distill_loss_reference` (+ the CE and Dice references) on `upsample_logits`, bit reproducibility, the entry points' refusals,
the dispatcher op, the criterion with `distill_weight` through `compute_loss` and `Trainer.train_step` (eager and
graph-captured) on the segofa_tiny fixture, and `task.distill_sample` with a second model and with the trainer's own teacher.

Tolerances (the issue's): loss |got - fp64 spec| <= 2e-4 |fp64 spec| (relative: the near losses are a few hundredths); gradient
bf16 against fp32 autograd of the specification, rel-L2 < 6e-3."""
import ctypes
import functools
import types

import pytest
import torch

import _dice_cases as DC
import _distill_cases as KC
import _predict_cases as PC
from test_dice_gpu import _ce_alone
from test_ema_gpu import same, taught  # noqa: F401  (segofa_tiny trained for three updates with a teacher, and that teacher as a model)
from test_ohem_gpu import _task
from test_predict_views_gpu import e2e  # noqa: F401  (the segofa_tiny fixture with its three raw shapes)
from test_weighted_loss_gpu import _rel, _student

pytestmark = pytest.mark.gpu

SEG0 = KC.SEG0
LAM = KC.LAMBDA
DW = 3.0
LOSS_RTOL, GRAD_RTOL = 2e-4, 6e-3


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ifseg_amd.ops  # noqa: F401
    return torch.device("cuda:0")


def _poisoned_bufs(lp):
    """the gradient buffer pre-filled, so that what the gather does not write shows"""
    return {"dl": torch.full(tuple(lp.shape), 3.0, dtype=torch.bfloat16, device=lp.device)}


# ------------------------------------------------------------------------------------------------- KD alone
@pytest.mark.parametrize("nseg,B,hp,wp", KC.SHAPES)
def test_distill_alone_is_the_specification(nseg, B, hp, wp):
    """every teacher (far, near) x T x mask: the loss within 2e-4 RELATIVE of the fp64 specification, the bf16 gradient within 6e-3
    rel-L2 of fp32 autograd, N exact, padding columns and the eos row zero in a pre-poisoned buffer, nothing non-finite although
    the teacher's padding and eos row are NaN; the all-ignore sample has a zero gradient under "valid" and one under "all".
    Measured on MI355X, worst loss error relative to the fp64 specification / worst gradient rel-L2 over the eight combinations,
    in the order of the cases: 1.2e-7 / 2.2e-3, 2.8e-7 / 1.8e-3, 1.2e-7 / 1.8e-3, 1.1e-7 / 1.8e-3, 1.3e-7 / 2.0e-3, 1.8e-7 / 2.0e-3,
    2.3e-7 / 2.0e-3, 1.2e-7 / 1.7e-3 (over all 64: loss 2e-9 .. 2.8e-7, gradient 0.7e-3 .. 2.2e-3; the bf16 rounding alone is
    0.9e-3 .. 2.6e-3 on these inputs)."""
    from ifseg_amd import hip
    dev = _dev()
    lp, tgt, _ = DC.dice_inputs(nseg, B, hp, wp)
    P, H, W = hp * wp, 16 * hp, 16 * wp
    lpd, tgd = lp.to(dev), tgt.to(dev)
    worst_l = worst_g = 0.0
    for kind in KC.TEACHERS:
        ted = KC.teacher(nseg, B, hp, wp, kind).to(dev)
        for T in KC.TEMPERATURES:
            for mask in KC.MASKS:
                l64, _, N, gref = KC.spec(nseg, B, hp, wp, kind, T, mask)
                bufs = _poisoned_bufs(lpd)
                loss, dl = hip.seg_distill(lpd, ted, tgd, hp, wp, H, W, nseg, SEG0, LAM, T, mask, bufs=bufs)
                assert dl is bufs["dl"] and tuple(loss.shape) == () and tuple(dl.shape) == tuple(lp.shape)
                l4, st, d = bufs["loss4"].cpu(), bufs["kd_stats"].cpu(), dl.cpu()
                want = LAM * l64
                lerr, rel = abs(float(l4[3]) - want) / abs(want), _rel(d[:, :, :nseg], gref)
                worst_l, worst_g = max(worst_l, lerr), max(worst_g, rel)
                print("kd nseg %d B %d %dx%d %s T %g %s: loss %.7f spec %.7f rel err %.2e, grad rel %.2e, N %d"
                      % (nseg, B, hp, wp, kind, T, mask, float(l4[3]), want, lerr, rel, N))
                assert want > 0.0 and float(gref.abs().max()) > 0.0 and N > 0
                assert bool(l4.isfinite().all()) and bool(d.float().isfinite().all())
                assert float(st[1]) == float(N)
                assert float(l4[0]) == float(l4[3]) == float(loss) and float(l4[1]) == 0.0 and float(l4[2]) == 0.0
                assert lerr <= LOSS_RTOL, (float(l4[3]), want)
                assert rel < GRAD_RTOL, rel
                assert float(d[:, :, nseg:].float().abs().sum()) == 0.0 and float(d[:, P].float().abs().sum()) == 0.0
                if B == 3:
                    if mask == "valid":
                        assert float(d[2].float().abs().max()) == 0.0 and float(gref[2].abs().max()) == 0.0
                    else:
                        assert float(d[2].float().abs().max()) > 0.0
    print("kd nseg %d B %d %dx%d: worst loss rel err %.2e, worst grad rel %.2e" % (nseg, B, hp, wp, worst_l, worst_g))


@pytest.mark.parametrize("nseg,B,hp,wp", KC.SHAPES)
def test_the_students_own_bits_as_teacher(nseg, B, hp, wp):
    """|loss| <= 1e-6 and the gradient's largest magnitude at most 1e-4 of the far case's: a cap, not a measurement (fp32 errors
    in p and q are ~1e-7 of differences of order one)"""
    from ifseg_amd import hip
    dev = _dev()
    lp, tgt, _ = DC.dice_inputs(nseg, B, hp, wp)
    H, W = 16 * hp, 16 * wp
    ted = KC.teacher(nseg, B, hp, wp, "same").to(dev)
    for T in KC.TEMPERATURES:
        for mask in KC.MASKS:
            far = float(KC.spec(nseg, B, hp, wp, "far", T, mask)[3].abs().max())
            loss, dl = hip.seg_distill(lp.to(dev), ted, tgt.to(dev), hp, wp, H, W, nseg, SEG0, LAM, T, mask, bufs={})
            gmax = float(dl.float().abs().max())
            print("kd same nseg %d T %g %s: loss %.3e, grad max %.3e (far %.3e)" % (nseg, T, mask, float(loss), gmax, far))
            assert abs(float(loss)) <= 1e-6 and gmax <= 1e-4 * far


@pytest.mark.parametrize("nseg,B,hp,wp", [(17, 2, 3, 4), (150, 1, 2, 3), (15, 3, 1, 1)])
def test_teacher_with_strides_of_its_own(nseg, B, hp, wp):
    """a teacher whose rows are 16 columns wider and whose samples lie 3 rows further apart than the student's, NaN in between:
    the bits of the contiguous teacher"""
    from ifseg_amd import hip
    dev = _dev()
    lp, tgt, _ = DC.dice_inputs(nseg, B, hp, wp)
    H, W = 16 * hp, 16 * wp
    te = KC.teacher(nseg, B, hp, wp, "near")
    a, b = {}, {}
    la, da = hip.seg_distill(lp.to(dev), te.to(dev), tgt.to(dev), hp, wp, H, W, nseg, SEG0, LAM, 2.0, "valid", bufs=a)
    lb, db = hip.seg_distill(lp.to(dev), KC.widen(te, dev), tgt.to(dev), hp, wp, H, W, nseg, SEG0, LAM, 2.0, "valid", bufs=b)
    assert torch.equal(la, lb) and torch.equal(da, db) and torch.equal(a["kd_tile"], b["kd_tile"]) and float(la) > 0.0


def test_a_batch_without_a_valid_pixel_gives_zeros():
    from ifseg_amd import hip
    dev = _dev()
    nseg, B, hp, wp = 15, 3, 1, 1
    lp, tgt, _ = DC.dice_inputs(nseg, B, hp, wp)
    te = KC.teacher(nseg, B, hp, wp, "far")
    lpd, tgd, ted = lp[2:].to(dev), tgt[2:].to(dev), te[2:].to(dev)
    bufs = _poisoned_bufs(lpd)
    loss, dl = hip.seg_distill(lpd, ted, tgd, hp, wp, 16, 16, nseg, SEG0, LAM, 2.0, "valid", bufs=bufs)
    assert float(loss) == 0.0 and bufs["loss4"].tolist() == [0.0] * 4 and float(bufs["kd_stats"][1]) == 0.0
    assert float(dl.float().abs().max()) == 0.0 and bool(bufs["kd_tile"].isfinite().all())
    loss, dl = hip.seg_distill(lpd, ted, None, hp, wp, 16, 16, nseg, SEG0, LAM, 2.0, "all", bufs={})     # no target needed
    assert float(loss) > 0.0 and float(dl.float().abs().max()) > 0.0


# ------------------------------------------------------------------------------------------------- CE (+ Dice) + KD
@functools.lru_cache(maxsize=None)
def _ce_reference(nseg, B, hp, wp, weighted):
    """`_dice_cases.combined_reference` without its Dice term -> (ce, d ce / d logits [B, P+1, n]) in fp32 with autograd"""
    from ifseg_amd.criterions import SegCriterion
    from ifseg_amd.criterions.seg_criterion import weighted_loss_reference
    lp, tgt, cw = DC.dice_inputs(nseg, B, hp, wp)
    H, W = 16 * hp, 16 * wp
    lf = lp[:, :, :nseg].float().clone().requires_grad_(True)
    scores = SegCriterion.upsample_logits(lf, hp, wp, H, W)
    clean = DC.clean_target(tgt, nseg)
    if weighted:
        ce = weighted_loss_reference(scores, clean, SEG0, nseg, cw, DC.pixel_plane(B, H * W), 0.0, "pixels")
    else:
        ce = weighted_loss_reference(scores, clean, SEG0, nseg)
    ce.backward()
    return ce.detach(), lf.grad.detach()


@pytest.mark.parametrize("nseg,B,hp,wp", KC.SHAPES)
def test_combined_is_the_sum_of_the_specifications(nseg, B, hp, wp):
    """with and without Dice, with and without the weighted CE (class weights + plane + "pixels"), near teacher at T = 2: the CE
    term and the statistics are the CE call's own bits, the Dice term `seg_loss_dice`'s, the KD term `seg_distill`'s; the total and
    its gradient match the sum of the references; `seg_loss` and `seg_loss_dice` give equal bits before and after.
    Measured on MI355X over the 32 combinations: total within 1.6e-7 relative, gradient rel-L2 1.3e-3 .. 2.1e-3."""
    from ifseg_amd import hip
    dev = _dev()
    lp, tgt, cw = DC.dice_inputs(nseg, B, hp, wp)
    P, H, W = hp * wp, 16 * hp, 16 * wp
    lpd, tgd, cwd, pwd = lp.to(dev), tgt.to(dev), cw.to(dev), DC.pixel_plane(B, H * W).to(dev)
    T, mask = 2.0, "valid"
    ted = KC.teacher(nseg, B, hp, wp, "near").to(dev)
    l64, _, _, gkd = KC.spec(nseg, B, hp, wp, "near", T, mask)
    kd_loss, _ = hip.seg_distill(lpd, ted, tgd, hp, wp, H, W, nseg, SEG0, LAM, T, mask, bufs={})
    for weighted in (False, True):
        kw = dict(pixel_weight=pwd, class_weight=cwd, norm_pixels=True) if weighted else {}
        ce_loss, ce_stats, ce_dl = _ce_alone(lpd, tgd, hp, wp, nseg, cwd, pwd, weighted)
        d3, d_dl = hip.seg_loss_dice(lpd, tgd, hp, wp, H, W, nseg, SEG0, DW, 1.0, dice_class_weight=cwd, bufs={}, **kw)
        d3, d_dl = d3.clone(), d_dl.clone()
        for dice in (False, True):
            if dice:
                total, ce, dv, gref = DC.combined_reference(nseg, B, hp, wp, weighted, DW)
            else:
                (ce, gref), dv = _ce_reference(nseg, B, hp, wp, weighted), torch.zeros(())
                total = ce
            want = float(total) + LAM * l64
            bufs = _poisoned_bufs(lpd)
            loss4, dl = hip.seg_loss_distill(lpd, ted, tgd, hp, wp, H, W, nseg, SEG0, LAM, T, mask,
                                             dice_weight=DW if dice else None, dice_class_weight=cwd if dice else None, bufs=bufs, **kw)
            assert torch.equal(loss4[1], ce_loss[0]) and torch.equal(bufs["stats"], ce_stats)
            assert torch.equal(loss4[2], d3[2]) if dice else float(loss4[2]) == 0.0
            assert torch.equal(loss4[3], kd_loss)
            assert torch.equal(loss4[0], (loss4[1] + loss4[2]) + loss4[3])
            l4, d = loss4.cpu(), dl.cpu()
            rel = _rel(d[:, :, :nseg], gref + gkd)
            lerr = abs(float(l4[0]) - want) / abs(want)
            print("ce+kd nseg %d B %d %dx%d weighted %d dice %d: total %.6f ref %.6f rel err %.2e (ce %.6f / %.6f, dice %.6f / %.6f, "
                  "kd %.6f / %.6f), grad rel %.2e" % (nseg, B, hp, wp, weighted, dice, float(l4[0]), want, lerr, float(l4[1]), float(ce),
                                                      float(l4[2]), float(dv), float(l4[3]), LAM * l64, rel))
            assert lerr <= LOSS_RTOL and abs(float(l4[3]) - LAM * l64) <= LOSS_RTOL * LAM * l64
            assert rel < GRAD_RTOL, rel
            assert float(d[:, :, nseg:].float().abs().sum()) == 0.0 and float(d[:, P].float().abs().sum()) == 0.0
            assert int(bufs["bad"]) == 1                                     # the poisoned out-of-range labels are flagged as ever
        # the older calls are untouched by the new ones
        ce_loss2, ce_stats2, ce_dl2 = _ce_alone(lpd, tgd, hp, wp, nseg, cwd, pwd, weighted)
        e3, e_dl = hip.seg_loss_dice(lpd, tgd, hp, wp, H, W, nseg, SEG0, DW, 1.0, dice_class_weight=cwd, bufs={}, **kw)
        assert torch.equal(ce_loss, ce_loss2) and torch.equal(ce_stats, ce_stats2) and torch.equal(ce_dl, ce_dl2)
        assert torch.equal(d3, e3) and torch.equal(d_dl, e_dl)


def test_the_same_launches_twice_give_equal_bits():
    """no atomics anywhere: every output and every intermediate of two runs into separate buffers is equal, and a second run
    into the same buffers allocates nothing"""
    from ifseg_amd import hip
    dev = _dev()
    nseg, B, hp, wp = 15, 2, 8, 8
    H, W = 16 * hp, 16 * wp
    lp, tgt, cw = DC.dice_inputs(nseg, B, hp, wp)
    lpd, tgd, cwd, pwd = lp.to(dev), tgt.to(dev), cw.to(dev), DC.pixel_plane(B, H * W).to(dev)
    ted = KC.teacher(nseg, B, hp, wp, "far").to(dev)
    run = lambda bufs: hip.seg_loss_distill(lpd, ted, tgd, hp, wp, H, W, nseg, SEG0, LAM, 2.0, "all", dice_weight=DW,
                                            dice_class_weight=cwd, bufs=bufs, pixel_weight=pwd, class_weight=cwd, norm_pixels=True)
    a, b = _poisoned_bufs(lpd), {}
    run(a)
    run(b)
    keys = ("loss4", "dl", "kd_tile", "kd_part", "kd_stats", "dice_sums", "dice_part", "dice_tile", "dice_val", "stats", "tile", "sp")
    assert sorted(a) == sorted(b) and set(keys) <= set(a)
    assert all(torch.equal(a[k], b[k]) for k in keys), [k for k in keys if not torch.equal(a[k], b[k])]
    first = {k: (v.data_ptr(), v.clone()) for k, v in a.items()}
    torch.cuda.synchronize()
    before, held = torch.cuda.memory_stats(dev)["allocation.all.allocated"], torch.cuda.memory_allocated(dev)
    run(a)
    assert torch.cuda.memory_stats(dev)["allocation.all.allocated"] == before and torch.cuda.memory_allocated(dev) == held
    assert all(a[k].data_ptr() == p and torch.equal(a[k], v) for k, (p, v) in first.items() if k != "bad")
    assert float(a["loss4"][3]) > 0.0 and float(a["dl"].float().abs().max()) > 0.0
    # KD alone as well
    c, d = {}, {}
    hip.seg_distill(lpd, ted, tgd, hp, wp, H, W, nseg, SEG0, LAM, 2.0, "all", bufs=c)
    hip.seg_distill(lpd, ted, tgd, hp, wp, H, W, nseg, SEG0, LAM, 2.0, "all", bufs=d)
    assert all(torch.equal(c[k], d[k]) for k in c) and torch.equal(c["loss4"][3], a["loss4"][3]) and torch.equal(c["kd_tile"], a["kd_tile"])
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated(dev)
    hip.seg_distill(lpd, ted, tgd, hp, wp, H, W, nseg, SEG0, LAM, 2.0, "all", bufs=c)
    assert torch.cuda.memory_allocated(dev) == held


# ------------------------------------------------------------------------------------------------- refusals
def test_entry_point_refusals():
    """return codes, nothing launched (the outputs keep their fill): bad geometry and a temperature <= 0 are -2, a missing pointer
    that is not optional -3; the binding's own assertions come before any of it"""
    from ifseg_amd import hip
    dev = _dev()
    nseg, B, hp, wp = 15, 2, 3, 4
    H, W = 16 * hp, 16 * wp
    lp, tgt, _ = (t.to(dev) for t in DC.dice_inputs(nseg, B, hp, wp))
    te = KC.teacher(nseg, B, hp, wp, "far").to(dev)
    tiles = B * hp * wp
    tile = torch.full((tiles * 9 * nseg,), 7.0, device=dev)
    part, stats = torch.full((tiles * 2,), 7.0, device=dev), torch.ones(2, device=dev)
    loss4, dl = torch.full((4,), 7.0, device=dev), torch.full_like(lp, 7.0)
    lib, p = hip.lib(), hip._ptr
    c_int, c_ll, c_float = ctypes.c_int, ctypes.c_longlong, ctypes.c_float

    def tiles_call(H_=H, W_=W, n_=nseg, B_=B, T_=2.0, lg=p(lp), tp=p(te), tg=p(tgt), all_=0, out=p(tile), pt=p(part), ldt=None):
        return lib.ifseg_seg_distill_tiles(lg, c_int(lp.stride(1)), c_ll(lp.stride(0)), tp, c_int(te.stride(1) if ldt is None else ldt),
                                           c_ll(te.stride(0)), tg, c_ll(tgt.stride(0)), c_int(B_), c_int(hp), c_int(wp), c_int(H_),
                                           c_int(W_), c_int(n_), c_ll(SEG0), c_ll(1), c_ll(2), c_float(T_), c_int(all_), out, pt,
                                           hip._stream())

    for kw in (dict(H_=H + 16), dict(W_=W - 16), dict(n_=0), dict(n_=513), dict(B_=0), dict(T_=0.0), dict(T_=-1.0),
               dict(T_=float("nan")), dict(T_=float("inf")), dict(ldt=nseg - 1)):
        assert tiles_call(**kw) == -2, kw
    for kw in (dict(lg=None), dict(tp=None), dict(tg=None), dict(out=None), dict(pt=None),
               dict(tp=ctypes.c_void_p(te.data_ptr() + 1))):
        assert tiles_call(**kw) == -3, kw

    def gather(ce=None, st=None, dt=None, dv=None, kt=p(tile), ks=p(stats), w=LAM, T_=2.0, n_=nseg, out=p(dl), lo=p(loss4)):
        return lib.ifseg_seg_loss_gather3(ce, st, dt, dv, kt, ks, c_float(w), c_float(T_), out, c_int(dl.stride(1)), c_ll(dl.stride(0)),
                                          c_int(B), c_int(hp), c_int(wp), c_int(n_), lo, hip._stream())

    for kw in (dict(kt=None), dict(ks=None), dict(ce=p(tile)), dict(dt=p(tile)), dict(out=None), dict(lo=None), dict(w=0.0),
               dict(w=float("nan"))):
        assert gather(**kw) == -3, kw
    for kw in (dict(n_=513), dict(n_=dl.stride(1) + 1), dict(n_=0), dict(T_=0.0), dict(T_=float("inf"))):
        assert gather(**kw) == -2, kw
    torch.cuda.synchronize()
    for t in (tile, part, loss4, dl):
        assert bool((t == 7.0).all())
    # the binding
    with pytest.raises(ValueError, match="distill_weight"):
        hip.seg_distill(lp, te, tgt, hp, wp, H, W, nseg, SEG0, 0.0)
    with pytest.raises(ValueError, match="distill_weight"):
        hip.seg_distill(lp, te, tgt, hp, wp, H, W, nseg, SEG0, None)
    with pytest.raises(ValueError, match="distill_temperature"):
        hip.seg_distill(lp, te, tgt, hp, wp, H, W, nseg, SEG0, LAM, float("nan"))
    with pytest.raises(ValueError, match="distill_mask"):
        hip.seg_loss_distill(lp, te, tgt, hp, wp, H, W, nseg, SEG0, LAM, 1.0, "some")
    with pytest.raises(ValueError, match="dice_weight"):
        hip.seg_loss_distill(lp, te, tgt, hp, wp, H, W, nseg, SEG0, LAM, dice_weight=0.0)
    with pytest.raises(AssertionError):
        hip.seg_distill(lp, te, tgt, hp, wp, H + 16, W, nseg, SEG0, LAM)
    with pytest.raises(AssertionError, match="target"):
        hip.seg_distill(lp, te, None, hp, wp, H, W, nseg, SEG0, LAM, 1.0, "valid")
    for bad in (te[:1], te[:, :hp * wp - 1], te[:, :, :nseg - 1], te.float(), te.cpu()):      # a teacher of another shape
        with pytest.raises(AssertionError, match="teacher"):
            hip.seg_distill(lp, bad, tgt, hp, wp, H, W, nseg, SEG0, LAM)
    with pytest.raises(AssertionError):
        hip.seg_distill(lp, te, tgt, hp, wp, H, W, nseg, SEG0, LAM, bufs={"dl": lp})            # overlapping buffers
    with pytest.raises(AssertionError, match="teacher"):
        hip.seg_distill(lp, te, tgt, hp, wp, H, W, nseg, SEG0, LAM, bufs={"dl": te})
    with pytest.raises(AssertionError, match="teacher"):
        hip.seg_distill(lp, te, tgt, hp, wp, H, W, nseg, SEG0, LAM, bufs={"kd_stats": te.view(torch.float32).reshape(-1)[4:6]})
    with pytest.raises(AssertionError):
        hip.seg_distill(lp, te, tgt, hp, wp, H, W, nseg, SEG0, LAM, bufs={"kd_stats": torch.empty(3, device=dev)})
    torch.cuda.synchronize()


def test_gather_entries_are_one_kernel():
    """one gather, three doors: on the same fp32 partials (seeded, made on the host) an entry with fewer sources writes the
    `dlogits` bits and the `loss_out[0]` of `ifseg_seg_loss_gather3` with the other sources null; the eos row and the padding
    columns are exactly zero in every call.  B = 2, 2 x 3 cells, 5 classes in rows of 8."""
    from ifseg_amd import hip
    dev = _dev()
    B, hp, wp, nseg, ld = 2, 2, 3, 5, 8
    g = torch.Generator().manual_seed(41)
    tiles = B * hp * wp
    ce, dice = (torch.randn(tiles * 9 * nseg, generator=g).to(dev) for _ in range(2))
    stats = torch.cat([torch.tensor([731.5, 1400.0]), torch.zeros(3 * nseg)]).to(dev)           # CE sum, Z, the histograms
    dval = (torch.rand(1, generator=g) + 0.5).to(dev)
    lib, p = hip.lib(), hip._ptr
    c_int, c_ll, c_float = ctypes.c_int, ctypes.c_longlong, ctypes.c_float

    def call(entry, *sources, words):
        dl = torch.full((B, hp * wp + 1, ld), 3.0, dtype=torch.bfloat16, device=dev)
        lo = torch.full((words,), 7.0, device=dev)
        rc = entry(*sources, p(dl), c_int(ld), c_ll(dl.stride(0)), c_int(B), c_int(hp), c_int(wp), c_int(nseg), p(lo), hip._stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert bool((dl[:, hp * wp] == 0).all()) and bool((dl[:, :, nseg:] == 0).all())        # the eos row, the padding columns
        assert float(dl[:, :hp * wp, :nseg].float().abs().min()) > 0.0                           # and everything else is written
        return dl.view(torch.int16), lo

    no_kd = (None, None, c_float(1.0), c_float(1.0))
    for name, few, three in (
            ("gather(ce)", call(lib.ifseg_seg_loss_gather, p(ce), p(stats), words=1),
             call(lib.ifseg_seg_loss_gather3, p(ce), p(stats), None, None, *no_kd, words=4)),
            ("gather_sum(ce, dice)", call(lib.ifseg_seg_loss_gather_sum, p(ce), p(stats), p(dice), p(dval), words=3),
             call(lib.ifseg_seg_loss_gather3, p(ce), p(stats), p(dice), p(dval), *no_kd, words=4)),
            ("gather_sum(-, dice)", call(lib.ifseg_seg_loss_gather_sum, None, None, p(dice), p(dval), words=3),
             call(lib.ifseg_seg_loss_gather3, None, None, p(dice), p(dval), *no_kd, words=4))):
        assert torch.equal(few[0], three[0]), name
        assert torch.equal(few[1][:1].view(torch.int32), three[1][:1].view(torch.int32)), (name, few[1], three[1])


# ------------------------------------------------------------------------------------------------- the dispatcher
def test_op_is_the_binding_and_differentiable():
    from ifseg_amd import hip
    dev = _dev()
    nseg, B, hp, wp = 15, 2, 3, 4
    H, W = 16 * hp, 16 * wp
    lp, tgt, _ = (t.to(dev) for t in DC.dice_inputs(nseg, B, hp, wp))
    te = KC.teacher(nseg, B, hp, wp, "far").to(dev)
    for target, mask in ((tgt, "valid"), (tgt, "all"), (None, "all")):
        bufs = {}
        want_loss, want_dl = hip.seg_distill(lp, te, target, hp, wp, H, W, nseg, SEG0, LAM, 2.0, mask, bufs=bufs)
        logits = lp[:, :, :nseg].clone().requires_grad_(True)                # 15 columns: the op pads them itself
        teacher = te.clone().requires_grad_(True)
        loss, stats, dl = torch.ops.ifseg.seg_distill(logits, teacher, target, hp, wp, H, W, SEG0, LAM, 2.0, mask == "all")
        assert torch.equal(loss, want_loss) and torch.equal(stats, bufs["kd_stats"]) and torch.equal(dl, want_dl)
        assert float(loss.detach()) > 0.0 and loss.requires_grad and not stats.requires_grad
        (loss * 3.0).backward()
        assert torch.equal(logits.grad, dl[:, :, :nseg] * torch.tensor(3.0, dtype=torch.bfloat16, device=dev))
        assert teacher.grad is None                                          # no gradient to the teacher


@pytest.mark.parametrize("nseg,B,hp,wp", [(15, 2, 8, 8), (150, 1, 2, 3), (171, 1, 4, 6)])
def test_op_takes_the_models_own_logits(nseg, B, hp, wp):
    """what the network hands out is a row-strided view [B, P+1, nseg] of its padded buffer (15, 150 and 171 classes are no
    multiple of 8): the op and the bindings take it as it is, for the student and for the teacher, and give the bits of the
    padded tensors"""
    from ifseg_amd import hip
    dev = _dev()
    H, W = 16 * hp, 16 * wp
    lp, tgt, cw = (t.to(dev) for t in DC.dice_inputs(nseg, B, hp, wp))
    te = KC.teacher(nseg, B, hp, wp, "near").to(dev)
    view, tview = lp[:, :, :nseg], te[:, :, :nseg]
    assert nseg % 8 and not view.is_contiguous() and view.stride(1) == lp.shape[2] and not tview.is_contiguous()
    bufs = {}
    want_loss, want_dl = hip.seg_distill(lp, te, tgt, hp, wp, H, W, nseg, SEG0, LAM, 2.0, bufs=bufs)
    vloss, vdl = hip.seg_distill(view, tview, tgt, hp, wp, H, W, nseg, SEG0, LAM, 2.0, bufs={})
    assert tuple(vdl.shape) == tuple(lp.shape) and torch.equal(vloss, want_loss) and torch.equal(vdl, want_dl)
    c4, cdl = hip.seg_loss_distill(lp, te, tgt, hp, wp, H, W, nseg, SEG0, LAM, 2.0, dice_weight=DW, bufs={})
    v4, vcdl = hip.seg_loss_distill(view, tview, tgt, hp, wp, H, W, nseg, SEG0, LAM, 2.0, dice_weight=DW, bufs={})
    assert torch.equal(v4, c4) and torch.equal(vcdl, cdl)
    logits = view.detach().requires_grad_(True)
    loss, stats, dl = torch.ops.ifseg.seg_distill(logits, tview, tgt, hp, wp, H, W, SEG0, LAM, 2.0, False)
    assert torch.equal(loss, want_loss) and torch.equal(stats, bufs["kd_stats"]) and torch.equal(dl, want_dl)
    assert float(loss.detach()) > 0.0 and float(dl.float().abs().max()) > 0.0
    loss.backward()
    assert tuple(logits.grad.shape) == (B, hp * wp + 1, nseg) and torch.equal(logits.grad, dl[:, :, :nseg])


# ------------------------------------------------------------------------------------------------- the criterion
def _noisy_teacher(pad, n, seed=3, scale=0.5):
    """the student's padded logits plus noise, NaN in the padding columns and the eos row"""
    g = torch.Generator().manual_seed(seed)
    t = torch.full(tuple(pad.shape), float("nan"), dtype=torch.bfloat16, device=pad.device)
    noise = (torch.randn(pad.shape[0], pad.shape[1] - 1, n, generator=g) * scale).to(pad.device)
    t[:, :-1, :n] = (pad[:, :-1, :n].float() + noise).to(torch.bfloat16)
    return t


def test_criterion_with_distill(e2e):  # noqa: F811
    """segofa_tiny at P = 128, modelled on test_criterion_with_dice: the fused `compute_loss` with `distill_weight` against
    `compute_loss_torch` (and its gradient against autograd of the references), alone, with the CE options, with Dice and with
    OHEM (the CE term is then the OHEM-only criterion's bits); a criterion without the term gives equal bits before and after.
    Measured on MI355X: kd_loss within 2e-5 relative of `compute_loss_torch`'s, gradient rel-L2 1.6e-3 .. 2.0e-3."""
    from ifseg_amd.criterions import SegCriterion
    from ifseg_amd.criterions.seg_criterion import distill_sums_reference
    dev = _dev()
    _, raw, ocfg, _ = e2e
    _, sd, _, _ = PC.e2e_fixture()
    P, n = ocfg.patch_image_size, ocfg.num_seg_tokens
    task = _task(ocfg)
    task.build_train_transform(dev, seed=6, ratio_range=(1, 1))
    m = _student(ocfg, sd, dev)
    s = task.self_train_sample(m, raw, 4, confidence_weight=True, prompt_ids=PC.E2E_PROMPT, keep=0.5, boundary=1)
    ckw = dict(unsupervised_segmentation=False, init_seg_with_text=False)
    cw = torch.linspace(0.5, 2.0, n).tolist()
    m.train()
    base = SegCriterion(task, **ckw)
    with torch.no_grad():
        out0 = m(**s["net_input"], full_context_alignment=base.full_context_alignment)
        s = dict(s, teacher_logits=_noisy_teacher(out0[1]["logits_padded"], n))
    plain = {k: v for k, v in s.items() if k != "target_weight"}
    tgt = s["target"]
    okw = dict(ohem_thresh=0.7, ohem_min_kept=P * P // 4)
    for sample, extra in ((plain, {}), (plain, dict(distill_temperature=2.0, distill_mask="all")),
                          (s, dict(class_weight=cw, weight_norm="pixels", distill_temperature=2.0)),
                          (plain, dict(dice_weight=3.0, dice_class_weight=cw, distill_temperature=2.0))):
        crit = SegCriterion(task, distill_weight=LAM, **extra, **ckw)
        with torch.no_grad():
            net_output = m(**sample["net_input"], full_context_alignment=crit.full_context_alignment)
            hp, wp = net_output[1]["encoder_returns"]["image_embed_shape"][0]
            before, mb, _ = base.compute_loss(m, net_output, plain, 0)
            fused, mf, _ = crit.compute_loss(m, net_output, sample, 0)
            dl = crit._bufs["dl"][:, :, :n].clone()
            stats = crit.distill_stats.clone()
            after, _, _ = base.compute_loss(m, net_output, plain, 0)
        ref, mr, _ = crit.compute_loss_torch(m, net_output, sample, 0)
        lf = net_output[1]["logits_padded"][:, :, :n].float().clone().requires_grad_(True)
        rl, _, _ = crit.compute_loss_torch(m, ((lf, net_output[1])), sample, 0)
        rl.backward()
        rel = _rel(dl, lf.grad)
        keys = ["loss", "nll_loss", "kd_loss"] + (["dice_loss"] if "dice_weight" in extra else [])
        got, want = dict(mf, loss=fused), dict(mr, loss=ref)
        print("criterion %s: " % sorted(extra) + ", ".join("%s %.6f / %.6f" % (k, float(got[k]), float(want[k])) for k in keys)
              + ", grad rel %.2e, stats %s / %s" % (rel, stats.tolist(), crit.distill_stats.tolist()))
        for k in keys:          # the KD term relatively; the CE and Dice terms (and the total that holds them) as their own tests do
            tol = LOSS_RTOL * (abs(float(want[k])) if k == "kd_loss" else max(1.0, abs(float(want[k]))))
            assert abs(float(got[k]) - float(want[k])) <= tol, (k, float(got[k]), float(want[k]))
        assert ("dice_loss" in mf) == ("dice_weight" in extra) and float(mf["kd_loss"]) > 0.0
        assert torch.equal(fused, (mf["nll_loss"] + mf.get("dice_loss", torch.zeros((), device=dev))) + mf["kd_loss"])
        assert rel < GRAD_RTOL, rel
        scores = SegCriterion.upsample_logits(lf.detach(), hp, wp, P, P)[:, :P * P]
        t_up = SegCriterion.upsample_logits(sample["teacher_logits"][:, :, :n].float(), hp, wp, P, P)[:, :P * P]
        want_stats = distill_sums_reference(scores, t_up, tgt, task.seg_id_offset, n, crit.distill_temperature, crit.distill_mask)
        assert float(stats[1]) == float(want_stats[1]) and abs(float(stats[0]) - float(want_stats[0])) <= LOSS_RTOL * float(want_stats[0])
        # the criterion without the term is untouched by calls with it on the same model
        assert torch.equal(before, after) and torch.equal(before, mb["nll_loss"]) and "kd_loss" not in mb
        assert float(fused) != float(before)
    # with OHEM: the CE term is the OHEM-only criterion's bits, the KD term the KD-only criterion's (the plane does not enter it)
    both, ohem, kd = SegCriterion(task, distill_weight=LAM, **okw, **ckw), SegCriterion(task, **okw, **ckw), SegCriterion(task, distill_weight=LAM, **ckw)
    with torch.no_grad():
        net_output = m(**plain["net_input"], full_context_alignment=both.full_context_alignment)
        fused, mf, _ = both.compute_loss(m, net_output, plain, 0)
        info = both.ohem_info.tolist()
        lo, _, _ = ohem.compute_loss(m, net_output, plain, 0)
        _, mk, _ = kd.compute_loss(m, net_output, plain, 0)
    assert 0 < info[1] < info[0] and torch.equal(both._bufs_ohem["plane"], ohem._bufs_ohem["plane"])
    assert torch.equal(mf["nll_loss"], lo) and torch.equal(mf["kd_loss"], mk["kd_loss"]) and torch.equal(fused, mf["nll_loss"] + mf["kd_loss"])
    # a training call without teacher logits is refused, a call that trains nothing skips the term
    with pytest.raises(ValueError, match="teacher_logits"):
        kd.compute_loss(m, net_output, {k: v for k, v in plain.items() if k != "teacher_logits"}, 0)
    with torch.no_grad():
        l0, m0, _ = kd.compute_loss(m, net_output, {k: v for k, v in plain.items() if k != "teacher_logits"}, 0)
        lb, _, _ = base.compute_loss(m, net_output, plain, 0)
    assert torch.equal(l0, lb) and "kd_loss" not in m0
    with pytest.raises(ValueError, match="shape"):
        kd.compute_loss(m, net_output, dict(plain, teacher_logits=plain["teacher_logits"][:, :-1]), 0)


# ------------------------------------------------------------------------------------------------- the teacher's logits
def test_distill_sample(taught):  # noqa: F811
    """with a second model as teacher the attached tensor is that model's own eval-mode logits, a clone that a later student
    forward leaves alone, and the teacher's training flag is restored; with `trainer=` it is what the student computes inside
    `tr.ema_weights()`, and the student's weights are back bit for bit; the refusals"""
    from ifseg_amd.criterions import SegCriterion
    tr, m, m2, raw, task, kw = taught
    s = task.self_train_sample(m, raw, 40, **kw)

    def logits_of(net):
        was = net.training
        net.eval()
        with torch.no_grad():
            _, extra = net(**s["net_input"], full_context_alignment=False)
            out = extra["logits_padded"].clone()
        net.train(was)
        return out

    m.train()
    m2.train()
    want = logits_of(m2)
    student = logits_of(m)
    ds = task.distill_sample(s, m, teacher=m2)
    got = ds["teacher_logits"]
    assert m2.training and m.training and set(ds) == set(s) | {"teacher_logits"} and ds["target"] is s["target"]
    assert got.dtype == torch.bfloat16 and same(got, want) and not same(got, student) and not got.requires_grad
    with torch.no_grad():
        _, extra = m2(**s["net_input"], full_context_alignment=False)
        m(**s["net_input"], full_context_alignment=False)
    assert got.data_ptr() != extra["logits_padded"].data_ptr() and same(got, want)
    # the trainer's own teacher
    p16, p32 = tr.eng.p16.clone(), tr.p32.clone()
    with tr.ema_weights():
        inside = logits_of(m)
    es = task.distill_sample(s, m, trainer=tr)
    torch.cuda.synchronize()
    assert same(es["teacher_logits"], inside) and not same(inside, student) and m.training
    assert same(tr.eng.p16, p16) and same(tr.p32, p32) and same(logits_of(m), student)
    # the criterion takes it
    # (every pixel: the usual choice on a pseudo-labelled batch, whose targets may be all ignore)
    crit = SegCriterion(task, unsupervised_segmentation=False, init_seg_with_text=False, distill_weight=LAM, distill_temperature=2.0,
                        distill_mask="all")
    with torch.no_grad():
        loss, metrics, _ = crit.compute_loss(m, m(**es["net_input"], full_context_alignment=False), es, 0)
    print("distill_sample: kd %.6f, stats %s, nll %.6f" % (float(metrics["kd_loss"]), crit.distill_stats.tolist(), float(metrics["nll_loss"])))
    assert float(crit.distill_stats[1]) == float(es["target"].shape[0] * (es["target"].shape[1] - 1))
    assert float(metrics["kd_loss"]) > 0.0 and float(loss) == float(metrics["nll_loss"] + metrics["kd_loss"])
    # refusals
    with pytest.raises(ValueError, match="teacher"):
        task.distill_sample(s, m)
    with pytest.raises(ValueError, match="another model"):
        task.distill_sample(s, m2, trainer=tr)
    with pytest.raises(ValueError, match="store_ema"):
        task.distill_sample(s, m2, trainer=types.SimpleNamespace(store_ema=False, model=m2))


# ------------------------------------------------------------------------------------------------- training
def _kd_steps(e2e, graphs, dice=False):  # noqa: F811
    """six `Trainer.train_step`s of segofa_tiny at P = 128 with a distilling criterion (test_dice_gpu._dice_steps' pattern), teacher
    logits resident in the two samples of the ring, once per entry of `graphs` (captured from the third step on, or eager) -> per
    run (losses, terms, distill stats, gradient arena, bf16 parameters, fp32 masters, graphs captured)"""
    from ifseg_amd.criterions import SegCriterion
    from ifseg_amd.trainer import Trainer
    dev = _dev()
    _, raw, ocfg, _ = e2e
    _, sd, _, _ = PC.e2e_fixture()
    task = _task(ocfg)
    import segofa_ref as O
    n, P = ocfg.num_seg_tokens, ocfg.patch_image_size
    cells = (P // 16) ** 2
    ring = []
    for j in range(2):
        batch = O.synthetic_batch(ocfg, 2, 12, seed=200 + j)
        sm = {"net_input": {k: batch[k].to(dev) for k in ("src_tokens", "patch_images", "patch_masks", "prev_output_tokens")},
              "target": batch["target"].to(dev), "ntokens": 1, "nsentences": 2}
        sm["net_input"]["patch_images"] = sm["net_input"]["patch_images"].to(torch.bfloat16)
        g = torch.Generator().manual_seed(300 + j)
        te = torch.full((2, cells + 1, (n + 7) // 8 * 8), float("nan"), dtype=torch.bfloat16)
        te[:, :cells, :n] = (2.0 * torch.randn(2, cells, n, generator=g)).to(torch.bfloat16)
        sm["teacher_logits"] = te.to(dev)
        ring.append(sm)

    def run(graph):
        torch.manual_seed(0)
        m = _student(ocfg, sd, dev)
        crit = SegCriterion(task, unsupervised_segmentation=False, init_seg_with_text=False, distill_weight=LAM, distill_temperature=2.0,
                            dice_weight=3.0 if dice else None)
        tr = Trainer(m, crit, task, device=dev)
        p0 = tr.p32.clone()
        losses, terms, stats = [], [], []
        for i in range(6):
            logs = tr.train_step([ring[i % 2]], prefetch=[ring[(i + 1) % 2]], graph=graph and i >= 2)
            losses.append(float(logs[-1]["loss"]))
            terms.append((float(logs[-1]["nll_loss"]), float(logs[-1]["kd_loss"]), float(logs[-1]["dice_loss"]) if dice else 0.0))
            stats.append(crit.distill_stats.clone())
        tr.check_overflow(wait=True)
        torch.cuda.synchronize()
        assert not torch.equal(tr.p32, p0)
        return losses, terms, torch.stack(stats), tr.eng.g16.clone(), tr.eng.p16.clone(), tr.p32.clone(), len(tr._graphs)

    return [run(g) for g in graphs]


@pytest.mark.parametrize("dice", [False, True])
def test_training_step_with_distill(e2e, dice):  # noqa: F811
    """`Trainer.train_step` with the term moves the weights (asserted in the run) without overflow; the logged loss is the finite
    positive sum of its logged terms"""
    (le, te, se, _, _, _, _), = _kd_steps(e2e, [False], dice)
    print("eager: losses", le, "nll / kd / dice", te)
    assert all(l == l and abs(l) != float("inf") and l > 0.0 for l in le)
    assert all(k > 0.0 and (d > 0.0) == dice and abs(l - (c + k + d)) <= 1e-6 * l for l, (c, k, d) in zip(le, te))
    assert bool((se[:, 1] > 0).all()) and bool((se[:, 0] > 0).all())


def test_captured_training_step_with_distill_is_bit_identical_to_eager(e2e):  # noqa: F811
    """test_captured_training_step_with_dice_is_bit_identical_to_eager's pattern: losses, terms, the distill statistics, gradients
    and parameters of the captured run (two graphs, each replayed on consecutive steps) are the eager run's bits"""
    (le, te, se, ge, pe, me, _), (lg, tg, sg, gg, pg, mg, ngraphs) = _kd_steps(e2e, [False, True])
    print("eager: losses", le, "nll / kd / dice", te)
    print("graph: losses", lg, "nll / kd / dice", tg)
    assert ngraphs == 2
    assert le == lg and te == tg, (le, lg, te, tg)
    for nm, x, y in (("distill stats", se, sg), ("gradient arena", ge, gg), ("bf16 parameters", pe, pg), ("fp32 masters", me, mg)):
        assert int((x != y).sum()) == 0, nm
