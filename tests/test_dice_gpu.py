"""GPU: the Dice auxiliary loss (csrc/dice.hip) against its specifications -- `hip.seg_dice_sums` against `dice_sums_reference`,
`hip.seg_dice` and `hip.seg_loss_dice` against `dice_loss_reference` (+ the CE reference) on `upsample_logits` with autograd, bit
reproducibility, the entry points' refusals, the dispatcher op, and the criterion with `dice_weight` through `compute_loss` and
`Trainer.train_step` (eager and graph-captured) on the segofa_tiny fixture."""
import ctypes

import pytest
import torch

import _dice_cases as DC
import _predict_cases as PC
from test_ohem_gpu import _task
from test_predict_views_gpu import e2e  # noqa: F401  (the segofa_tiny fixture with its three raw shapes)
from test_weighted_loss_gpu import _rel, _student

pytestmark = pytest.mark.gpu

SEG0 = DC.SEG0
DW = 3.0


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ifseg_amd.ops  # noqa: F401
    return torch.device("cuda:0")


def _poisoned_bufs(lp):
    """the gradient buffer pre-filled, so that what the gather does not write shows"""
    return {"dl": torch.full(tuple(lp.shape), 3.0, dtype=torch.bfloat16, device=lp.device)}


# ------------------------------------------------------------------------------------------------- pass A
@pytest.mark.parametrize("nseg,B,hp,wp", DC.SHAPES)
def test_sums_are_the_specification(nseg, B, hp, wp):
    """Y is exact (integers below 2^24).  I and P follow tests/_predict_cases.py's rule: e_pix = max |fp32 specification - fp64
    specification| over the valid pixels' softmax probabilities; a kernel probability may sit within 4 e_pix of the fp64 one, so a
    sum over the N_b valid pixels of a sample within 4 e_pix N_b of the fp64 specification's.  Derived, and loose on purpose: a
    wrong mask, batch-wide sums or a lost class chunk are errors of order one.
    Measured on MI355X, max over (sample, class) of |kernel - fp64| / (4 e_pix N_b), in the order of the cases:
    0.084, 0.011, 0.024, 0.008, 0.013, 0.002, 0.068, 0.003 (pass A keeps the softmax denominator and the tile's sums in fp64 and
    rounds each once: an fp32 emulation of the single cell, where all 256 pixels round alike, came to 1.6 on the host)."""
    from ifseg_amd import hip
    dev = _dev()
    lp, tgt, _ = DC.dice_inputs(nseg, B, hp, wp)
    s32, s64, nb, e_pix = DC.sums_specs(nseg, B, hp, wp)
    H, W = 16 * hp, 16 * wp
    bufs = {}
    got = hip.seg_dice_sums(lp.to(dev), tgt.to(dev), hp, wp, H, W, nseg, SEG0, bufs=bufs)
    assert got is bufs["dice_sums"] and got.dtype == torch.float32 and tuple(got.shape) == (B, 3, nseg)
    g = got.cpu().double()
    bound = 4.0 * e_pix * nb.double()                                        # [B]
    err = (g[:, :2] - s64[:, :2]).abs().amax(dim=(1, 2))
    mult = max(float(err[b] / bound[b]) for b in range(B) if nb[b] > 0)
    print("dice sums nseg %d B %d %dx%d: e_pix %.3e, N_b %s, max |I, P - fp64| %.3e = %.3f of the bound"
          % (nseg, B, hp, wp, e_pix, nb.tolist(), float(err.max()), mult))
    assert e_pix > 0.0 and int(nb.max()) > 0
    assert torch.equal(g[:, 2], s64[:, 2])
    assert bool((err <= bound).all()), (err.tolist(), bound.tolist())
    if B == 3:
        assert int(nb[2]) == 0 and float(g[2].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------- Dice alone
@pytest.mark.parametrize("nseg,B,hp,wp", DC.SHAPES)
def test_dice_alone_is_the_specification(nseg, B, hp, wp):
    """loss and gradient at test_fused_seg_loss's / test_weighted_kernel_is_the_specification's tolerances (the arithmetic class
    and the bf16 store are the same), with and without class weights"""
    from ifseg_amd import hip
    dev = _dev()
    lp, tgt, cw = DC.dice_inputs(nseg, B, hp, wp)
    P, H, W = hp * wp, 16 * hp, 16 * wp
    lpd, tgd = lp.to(dev), tgt.to(dev)
    for use_cw in (False, True):
        ref, gref = DC.dice_reference(nseg, B, hp, wp, use_cw, DW)
        bufs = _poisoned_bufs(lpd)
        loss, dl = hip.seg_dice(lpd, tgd, hp, wp, H, W, nseg, SEG0, DW, 1.0, class_weight=cw.to(dev) if use_cw else None, bufs=bufs)
        assert dl is bufs["dl"] and tuple(loss.shape) == ()
        l3, d = bufs["loss3"].cpu(), dl.cpu()
        rel = _rel(d[:, :, :nseg], gref)
        print("dice nseg %d B %d %dx%d cw %d: loss %.7f ref %.7f, grad rel %.2e" % (nseg, B, hp, wp, use_cw, float(l3[0]), float(ref), rel))
        assert float(ref) > 0.0 and float(gref.abs().max()) > 0.0
        assert abs(float(l3[0]) - float(ref)) < 2e-4 * max(1.0, abs(float(ref))), (float(l3[0]), float(ref))
        assert float(l3[1]) == 0.0 and float(l3[2]) == float(l3[0]) == float(loss)
        assert rel < 6e-3, rel
        assert float(d[:, :, nseg:].float().abs().sum()) == 0.0 and float(d[:, P].float().abs().sum()) == 0.0
        if B == 3:
            assert float(d[2].float().abs().max()) == 0.0 and float(gref[2].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------- CE + Dice
def _ce_alone(lpd, tgd, hp, wp, nseg, cw, pw, weighted):
    from ifseg_amd import hip
    dev = lpd.device
    B, P, H, W = lpd.shape[0], hp * wp, 16 * hp, 16 * wp
    tile = torch.empty(B * P * 9 * nseg, device=dev)
    sp = torch.empty(B * P * (2 + 3 * nseg), device=dev)
    stats = torch.empty(2 + 3 * nseg, device=dev)
    dl = torch.empty_like(lpd)
    loss = torch.empty(1, device=dev)
    if weighted:
        hip.seg_loss_weighted(lpd, tgd, hp, wp, H, W, nseg, SEG0, tile, sp, stats, dl, loss, pixel_weight=pw, class_weight=cw,
                              norm_pixels=True)
    else:
        hip.seg_loss(lpd, tgd, hp, wp, H, W, nseg, SEG0, tile, sp, stats, dl, loss)
    return loss, stats, dl


def _combined(lpd, tgd, hp, wp, nseg, cw, pw, weighted, bufs):
    from ifseg_amd import hip
    kw = dict(pixel_weight=pw, class_weight=cw, norm_pixels=True) if weighted else {}
    return hip.seg_loss_dice(lpd, tgd, hp, wp, 16 * hp, 16 * wp, nseg, SEG0, DW, 1.0, dice_class_weight=cw, bufs=bufs, **kw)


@pytest.mark.parametrize("nseg,B,hp,wp", DC.SHAPES)
def test_combined_is_the_sum_of_the_specifications(nseg, B, hp, wp):
    """unweighted CE, and CE with class_weight + plane + "pixels", each plus 3 x Dice: the same tolerances; the CE term and the
    statistics are the CE call's own bits, the total is the fp32 sum of the two terms"""
    dev = _dev()
    lp, tgt, cw = DC.dice_inputs(nseg, B, hp, wp)
    P, H, W = hp * wp, 16 * hp, 16 * wp
    lpd, tgd, cwd, pwd = lp.to(dev), tgt.to(dev), cw.to(dev), DC.pixel_plane(B, H * W).to(dev)
    for weighted in (False, True):
        total, ce, dice, gref = DC.combined_reference(nseg, B, hp, wp, weighted, DW)
        bufs = _poisoned_bufs(lpd)
        loss3, dl = _combined(lpd, tgd, hp, wp, nseg, cwd, pwd, weighted, bufs)
        ce_loss, ce_stats, _ = _ce_alone(lpd, tgd, hp, wp, nseg, cwd, pwd, weighted)
        assert torch.equal(loss3[1], ce_loss[0]) and torch.equal(bufs["stats"], ce_stats)
        assert torch.equal(loss3[0], loss3[1] + loss3[2])
        l3, d = loss3.cpu(), dl.cpu()
        rel = _rel(d[:, :, :nseg], gref)
        print("ce+dice nseg %d B %d %dx%d weighted %d: total %.6f ref %.6f, ce %.6f ref %.6f, dice %.6f ref %.6f, grad rel %.2e"
              % (nseg, B, hp, wp, weighted, float(l3[0]), float(total), float(l3[1]), float(ce), float(l3[2]), float(dice), rel))
        for got, want in zip(l3.tolist(), (float(total), float(ce), float(dice))):
            assert abs(got - want) < 2e-4 * max(1.0, abs(want)), (l3.tolist(), float(total), float(ce), float(dice))
        assert rel < 6e-3, rel
        assert float(d[:, :, nseg:].float().abs().sum()) == 0.0 and float(d[:, P].float().abs().sum()) == 0.0
        assert int(bufs["bad"]) == 1                                         # the poisoned out-of-range labels are flagged as ever


def test_the_same_launches_twice_give_equal_bits():
    """no atomics anywhere: every output and every intermediate of two runs into separate buffers is equal, and a second run
    into the same buffers allocates nothing"""
    dev = _dev()
    nseg, B, hp, wp = 15, 2, 8, 8
    lp, tgt, cw = DC.dice_inputs(nseg, B, hp, wp)
    lpd, tgd, cwd, pwd = lp.to(dev), tgt.to(dev), cw.to(dev), DC.pixel_plane(B, 256 * hp * wp).to(dev)
    a, b = _poisoned_bufs(lpd), {}
    _combined(lpd, tgd, hp, wp, nseg, cwd, pwd, True, a)
    _combined(lpd, tgd, hp, wp, nseg, cwd, pwd, True, b)
    keys = ("loss3", "dl", "dice_sums", "dice_part", "dice_tile", "dice_val", "stats", "tile", "sp")
    assert sorted(a) == sorted(b) and set(keys) <= set(a)
    assert all(torch.equal(a[k], b[k]) for k in keys), [k for k in keys if not torch.equal(a[k], b[k])]
    first = {k: (v.data_ptr(), v.clone()) for k, v in a.items()}
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats(dev)["allocation.all.allocated"]
    _combined(lpd, tgd, hp, wp, nseg, cwd, pwd, True, a)
    assert torch.cuda.memory_stats(dev)["allocation.all.allocated"] == before
    assert all(a[k].data_ptr() == p and torch.equal(a[k], v) for k, (p, v) in first.items() if k != "bad")
    assert float(a["loss3"][2]) > 0.0 and float(a["dl"].float().abs().max()) > 0.0


# ------------------------------------------------------------------------------------------------- refusals
def test_entry_point_refusals():
    """return codes, nothing launched (the outputs keep their fill): what ifseg_seg_loss_tiles refuses, smooth and dice_weight
    that are not finite numbers > 0, a misaligned class-weight pointer; the binding's own assertions come before any of it"""
    from ifseg_amd import hip
    dev = _dev()
    nseg, B, hp, wp = 15, 2, 3, 4
    H, W = 16 * hp, 16 * wp
    lp, tgt, cw = (t.to(dev) for t in DC.dice_inputs(nseg, B, hp, wp))
    tiles = B * hp * wp
    part = torch.full((tiles * 3 * nseg,), 7.0, device=dev)
    sums = torch.ones(B, 3, nseg, device=dev)
    tile = torch.full((tiles * 9 * nseg,), 7.0, device=dev)
    val, loss3, dl = torch.full((1,), 7.0, device=dev), torch.full((3,), 7.0, device=dev), torch.full_like(lp, 7.0)
    cwbuf = torch.ones(nseg + 1, device=dev)
    lib, p = hip.lib(), hip._ptr
    c_int, c_ll, c_float = ctypes.c_int, ctypes.c_longlong, ctypes.c_float

    def head(H_=H, W_=W, n_=nseg, B_=B):
        return (p(lp), c_int(lp.stride(1)), c_ll(lp.stride(0)), p(tgt), c_ll(tgt.stride(0)), c_int(B_), c_int(hp), c_int(wp),
                c_int(H_), c_int(W_), c_int(n_), c_ll(SEG0), c_ll(1), c_ll(2))

    def tiles_call(weight=DW, smooth=1.0, cwp=None, **kw):
        return lib.ifseg_seg_dice_tiles(*head(**kw), p(sums), cwp, c_float(weight), c_float(smooth), p(tile), p(val), hip._stream())

    for kw in (dict(H_=H + 16), dict(W_=W - 16), dict(n_=0), dict(n_=513), dict(B_=0)):
        assert lib.ifseg_seg_dice_sums(*head(**kw), p(part), hip._stream()) == -2, kw
        assert tiles_call(**kw) == -2, kw
    assert lib.ifseg_seg_dice_sums(*head(), None, hip._stream()) == -3
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert tiles_call(smooth=bad) == -3, bad
        assert tiles_call(weight=bad) == -3, bad
    assert tiles_call(cwp=ctypes.c_void_p(cwbuf.data_ptr() + 2)) == -3
    gather = lambda ce, st, dt, n_=nseg: lib.ifseg_seg_loss_gather_sum(
        ce, st, dt, p(val), p(dl), c_int(dl.stride(1)), c_ll(dl.stride(0)), c_int(B), c_int(hp), c_int(wp), c_int(n_), p(loss3), hip._stream())
    assert gather(None, None, None) == -3 and gather(p(tile), None, p(tile)) == -3
    assert gather(None, None, p(tile), 513) == -2 and gather(None, None, p(tile), dl.stride(1) + 1) == -2
    torch.cuda.synchronize()
    for t in (part, tile, val, loss3, dl):
        assert bool((t == 7.0).all())
    # the binding
    with pytest.raises(ValueError, match="dice_weight"):
        hip.seg_dice(lp, tgt, hp, wp, H, W, nseg, SEG0, 0.0)
    with pytest.raises(ValueError, match="dice_smooth"):
        hip.seg_dice(lp, tgt, hp, wp, H, W, nseg, SEG0, DW, float("nan"))
    with pytest.raises(AssertionError):
        hip.seg_dice(lp, tgt, hp, wp, H + 16, W, nseg, SEG0, DW)
    with pytest.raises(AssertionError):
        hip.seg_dice(lp, tgt, hp, wp, H, W, nseg, SEG0, DW, class_weight=cw.double())
    with pytest.raises(AssertionError):
        hip.seg_dice(lp, tgt, hp, wp, H, W, nseg, SEG0, DW, bufs={"dl": lp})
    with pytest.raises(AssertionError):
        hip.seg_dice_sums(lp, tgt, hp, wp, H, W, nseg, SEG0, bufs={"dice_sums": torch.empty(B, 3, nseg + 1, device=dev)})
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- the dispatcher
def test_op_is_the_binding_and_differentiable():
    from ifseg_amd import hip
    dev = _dev()
    nseg, B, hp, wp = 15, 2, 3, 4
    H, W = 16 * hp, 16 * wp
    lp, tgt, cw = (t.to(dev) for t in DC.dice_inputs(nseg, B, hp, wp))
    for w in (None, cw):
        bufs = {}
        want_loss, want_dl = hip.seg_dice(lp, tgt, hp, wp, H, W, nseg, SEG0, DW, 0.5, class_weight=w, bufs=bufs)
        logits = lp[:, :, :nseg].clone().requires_grad_(True)                # 15 columns: the op pads them itself
        loss, sums, dl = torch.ops.ifseg.seg_dice(logits, tgt, w, hp, wp, H, W, SEG0, DW, 0.5)
        assert torch.equal(loss, want_loss) and torch.equal(sums, bufs["dice_sums"]) and torch.equal(dl, want_dl)
        assert float(loss.detach()) > 0.0 and loss.requires_grad and not sums.requires_grad
        (loss * 3.0).backward()
        assert torch.equal(logits.grad, dl[:, :, :nseg] * torch.tensor(3.0, dtype=torch.bfloat16, device=dev))


@pytest.mark.parametrize("nseg,B,hp,wp", [(15, 2, 8, 8), (150, 1, 2, 3), (171, 1, 4, 6)])
def test_op_takes_the_models_own_logits(nseg, B, hp, wp):
    """what the network hands out is a row-strided view [B, P+1, nseg] of its padded buffer (15, 150 and 171 classes are no
    multiple of 8): the op and the binding take it as it is and give the bits of the padded tensor"""
    from ifseg_amd import hip
    dev = _dev()
    H, W = 16 * hp, 16 * wp
    lp, tgt, cw = (t.to(dev) for t in DC.dice_inputs(nseg, B, hp, wp))
    view = lp[:, :, :nseg]
    assert nseg % 8 and not view.is_contiguous() and view.stride(1) == lp.shape[2]
    bufs = {}
    want_loss, want_dl = hip.seg_dice(lp, tgt, hp, wp, H, W, nseg, SEG0, DW, 1.0, class_weight=cw, bufs=bufs)
    vbufs = {}
    vloss, vdl = hip.seg_dice(view, tgt, hp, wp, H, W, nseg, SEG0, DW, 1.0, class_weight=cw, bufs=vbufs)
    assert tuple(vdl.shape) == tuple(lp.shape) and torch.equal(vloss, want_loss) and torch.equal(vdl, want_dl)
    c3, cdl = hip.seg_loss_dice(lp, tgt, hp, wp, H, W, nseg, SEG0, DW, 1.0, dice_class_weight=cw, bufs={})
    v3, vcdl = hip.seg_loss_dice(view, tgt, hp, wp, H, W, nseg, SEG0, DW, 1.0, dice_class_weight=cw, bufs={})
    assert torch.equal(v3, c3) and torch.equal(vcdl, cdl)
    logits = view.detach().requires_grad_(True)
    loss, sums, dl = torch.ops.ifseg.seg_dice(logits, tgt, cw, hp, wp, H, W, SEG0, DW, 1.0)
    assert torch.equal(loss, want_loss) and torch.equal(sums, bufs["dice_sums"]) and torch.equal(dl, want_dl)
    assert float(loss.detach()) > 0.0 and float(dl.float().abs().max()) > 0.0
    loss.backward()
    assert tuple(logits.grad.shape) == (B, hp * wp + 1, nseg) and torch.equal(logits.grad, dl[:, :, :nseg])


# ------------------------------------------------------------------------------------------------- the criterion
def test_criterion_with_dice(e2e):  # noqa: F811
    """segofa_tiny at P = 128, modelled on test_criterion_with_ohem: the fused `compute_loss` with `dice_weight=3.0` against
    `compute_loss_torch` (and its gradient against autograd of the two references), with and without the CE options; a criterion
    without Dice gives equal bits before and after Dice calls on the same model"""
    from ifseg_amd.criterions import SegCriterion
    from ifseg_amd.criterions.seg_criterion import dice_loss_reference, dice_sums_reference
    dev = _dev()
    _, raw, ocfg, _ = e2e
    _, sd, _, _ = PC.e2e_fixture()
    P, n = ocfg.patch_image_size, ocfg.num_seg_tokens
    task = _task(ocfg)
    task.build_train_transform(dev, seed=6, ratio_range=(1, 1))
    m = _student(ocfg, sd, dev)
    s = task.self_train_sample(m, raw, 4, confidence_weight=True, prompt_ids=PC.E2E_PROMPT, keep=0.5, boundary=1)
    plain = {k: v for k, v in s.items() if k != "target_weight"}
    tgt = s["target"]
    ckw = dict(unsupervised_segmentation=False, init_seg_with_text=False)
    cw = torch.linspace(0.5, 2.0, n).tolist()
    m.train()
    base = SegCriterion(task, **ckw)
    for sample, extra in ((plain, {}), (s, dict(class_weight=cw, weight_norm="pixels", dice_class_weight=cw, dice_smooth=0.5))):
        crit = SegCriterion(task, dice_weight=3.0, **extra, **ckw)
        with torch.no_grad():
            net_output = m(**sample["net_input"], full_context_alignment=crit.full_context_alignment)
            hp, wp = net_output[1]["encoder_returns"]["image_embed_shape"][0]
            before, mb, _ = base.compute_loss(m, net_output, plain, 0)
            fused, mf, _ = crit.compute_loss(m, net_output, sample, 0)
            dl = crit._bufs["dl"][:, :, :n].clone()
            sums = crit.dice_sums.clone()
            after, _, _ = base.compute_loss(m, net_output, plain, 0)
        ref, mr, _ = crit.compute_loss_torch(m, net_output, sample, 0)
        lf = net_output[1]["logits_padded"][:, :, :n].float().clone().requires_grad_(True)
        rl, _, _ = crit.compute_loss_torch(m, ((lf, net_output[1])), sample, 0)
        rl.backward()
        rel = _rel(dl, lf.grad)
        print("criterion: fused %.6f ref %.6f (nll %.6f / %.6f, dice %.6f / %.6f), grad rel %.2e"
              % (float(fused), float(ref), float(mf["nll_loss"]), float(mr["nll_loss"]), float(mf["dice_loss"]), float(mr["dice_loss"]), rel))
        for k, got, want in (("loss", fused, ref), ("nll_loss", mf["nll_loss"], mr["nll_loss"]), ("dice_loss", mf["dice_loss"], mr["dice_loss"])):
            assert abs(float(got) - float(want)) < 2e-4 * max(1.0, abs(float(want))), (k, float(got), float(want))
        assert torch.equal(fused, mf["nll_loss"] + mf["dice_loss"]) and float(mf["dice_loss"]) > 0.0
        assert rel < 6e-3, rel
        scores = SegCriterion.upsample_logits(lf.detach(), hp, wp, P, P)
        want_sums = dice_sums_reference(scores, tgt, task.seg_id_offset, n)
        assert tuple(sums.shape) == (tgt.shape[0], 3, n) and torch.equal(sums[:, 2], want_sums[:, 2])
        assert float((sums - want_sums).abs().max()) <= 1e-4 * P * P
        want_dice = 3.0 * dice_loss_reference(scores, tgt, task.seg_id_offset, n, crit.dice_smooth, crit.dice_class_weight)
        assert abs(float(mr["dice_loss"]) - float(want_dice)) < 1e-6
        # the criterion without Dice is untouched by Dice calls on the same model
        assert torch.equal(before, after) and torch.equal(before, mb["nll_loss"]) and "dice_loss" not in mb
        assert float(fused) != float(before)


def test_criterion_with_dice_and_ohem(e2e):  # noqa: F811
    """`dice_weight` and `ohem_thresh` together: the CE term is the OHEM-only criterion's bits and the Dice term the Dice-only
    criterion's (the plane does not enter it); the sum and its gradient against `weighted_loss_reference` on the DEVICE's own
    plane (test_criterion_with_ohem's way: no threshold-margin pixel enters) plus `dice_loss_reference`, and the Dice term
    against `compute_loss_torch`'s, which selects a plane of its own"""
    from ifseg_amd.criterions import SegCriterion
    from ifseg_amd.criterions.seg_criterion import dice_loss_reference, weighted_loss_reference
    dev = _dev()
    _, raw, ocfg, _ = e2e
    _, sd, _, _ = PC.e2e_fixture()
    P, n = ocfg.patch_image_size, ocfg.num_seg_tokens
    task = _task(ocfg)
    task.build_train_transform(dev, seed=6, ratio_range=(1, 1))
    m = _student(ocfg, sd, dev)
    s = task.self_train_sample(m, raw, 4, prompt_ids=PC.E2E_PROMPT, keep=0.5, boundary=1)
    tgt = s["target"]
    ckw = dict(unsupervised_segmentation=False, init_seg_with_text=False)
    okw = dict(ohem_thresh=0.7, ohem_min_kept=P * P // 4)
    both, ohem, dice = SegCriterion(task, dice_weight=3.0, **okw, **ckw), SegCriterion(task, **okw, **ckw), SegCriterion(task, dice_weight=3.0, **ckw)
    m.train()
    with torch.no_grad():
        net_output = m(**s["net_input"], full_context_alignment=both.full_context_alignment)
        hp, wp = net_output[1]["encoder_returns"]["image_embed_shape"][0]
        fused, mf, _ = both.compute_loss(m, net_output, s, 0)
        plane, info = both._bufs_ohem["plane"].clone(), both.ohem_info.tolist()
        dl = both._bufs["dl"][:, :, :n].clone()
        lo, _, _ = ohem.compute_loss(m, net_output, s, 0)
        _, md, _ = dice.compute_loss(m, net_output, s, 0)
        _, mr, _ = both.compute_loss_torch(m, net_output, s, 0)
    assert 0 < info[1] < info[0] and torch.equal(plane, ohem._bufs_ohem["plane"])
    assert torch.equal(mf["nll_loss"], lo) and torch.equal(mf["dice_loss"], md["dice_loss"])
    assert torch.equal(fused, mf["nll_loss"] + mf["dice_loss"])
    lf = net_output[1]["logits_padded"][:, :, :n].float().clone().requires_grad_(True)
    scores = SegCriterion.upsample_logits(lf, hp, wp, P, P)
    ce = weighted_loss_reference(scores[:, :P * P], tgt, task.seg_id_offset, n, None, plane, 0.0, "weights")
    ref = ce + 3.0 * dice_loss_reference(scores[:, :P * P], tgt, task.seg_id_offset, n)
    ref.backward()
    ref, rel = float(ref.detach()), _rel(dl, lf.grad)
    print("dice + ohem: fused %.6f ref %.6f (nll %.6f / %.6f on the device's plane, %.6f on the reference's; dice %.6f / %.6f), "
          "grad rel %.2e, info %s" % (float(fused), ref, float(mf["nll_loss"]), float(ce.detach()), float(mr["nll_loss"]),
                                      float(mf["dice_loss"]), float(mr["dice_loss"]), rel, info))
    assert abs(float(fused) - ref) < 2e-4 * max(1.0, abs(ref)), (float(fused), ref)
    assert abs(float(mf["dice_loss"]) - float(mr["dice_loss"])) < 2e-4 * max(1.0, abs(float(mr["dice_loss"])))
    assert rel < 6e-3, rel


def _dice_steps(e2e, graphs):  # noqa: F811
    """six `Trainer.train_step`s of segofa_tiny at P = 128 with a Dice criterion (test_ohem_gpu._ohem_steps' pattern), once per
    entry of `graphs` (captured from the third step on, or eager) -> per run (losses, dice terms, dice sums, gradient arena, bf16
    parameters, fp32 masters, graphs captured)"""
    from ifseg_amd.criterions import SegCriterion
    from ifseg_amd.trainer import Trainer
    dev = _dev()
    _, raw, ocfg, _ = e2e
    _, sd, _, _ = PC.e2e_fixture()
    task = _task(ocfg)
    import segofa_ref as O
    ring = []
    for j in range(2):
        batch = O.synthetic_batch(ocfg, 2, 12, seed=200 + j)
        sm = {"net_input": {k: batch[k].to(dev) for k in ("src_tokens", "patch_images", "patch_masks", "prev_output_tokens")},
              "target": batch["target"].to(dev), "ntokens": 1, "nsentences": 2}
        sm["net_input"]["patch_images"] = sm["net_input"]["patch_images"].to(torch.bfloat16)
        ring.append(sm)

    def run(graph):
        torch.manual_seed(0)
        m = _student(ocfg, sd, dev)
        crit = SegCriterion(task, unsupervised_segmentation=False, init_seg_with_text=False, dice_weight=3.0)
        tr = Trainer(m, crit, task, device=dev)
        p0 = tr.p32.clone()
        losses, dices, sums = [], [], []
        for i in range(6):
            logs = tr.train_step([ring[i % 2]], prefetch=[ring[(i + 1) % 2]], graph=graph and i >= 2)
            losses.append(float(logs[-1]["loss"]))
            dices.append((float(logs[-1]["nll_loss"]), float(logs[-1]["dice_loss"])))
            sums.append(crit.dice_sums.clone())
        tr.check_overflow(wait=True)
        torch.cuda.synchronize()
        assert not torch.equal(tr.p32, p0)
        return losses, dices, torch.stack(sums), tr.eng.g16.clone(), tr.eng.p16.clone(), tr.p32.clone(), len(tr._graphs)

    return [run(g) for g in graphs]


def test_training_step_with_dice(e2e):  # noqa: F811
    """`Trainer.train_step` with a Dice criterion moves the weights (asserted in the run) without overflow; the logged loss is
    the finite positive sum of its two logged terms"""
    (le, de, se, _, _, _, _), = _dice_steps(e2e, [False])
    print("eager: losses", le, "nll / dice", de)
    assert all(l == l and abs(l) != float("inf") and l > 0.0 for l in le)
    assert all(d > 0.0 and abs(l - (c + d)) <= 1e-6 * l for l, (c, d) in zip(le, de))
    assert float(se[:, :, 2].sum()) > 0.0


def test_captured_training_step_with_dice_is_bit_identical_to_eager(e2e):  # noqa: F811
    """test_captured_training_step_with_ohem_is_bit_identical_to_eager's pattern: losses, both terms, the Dice sums, gradients
    and parameters of the captured run (two graphs, each replayed on consecutive steps) are the eager run's bits"""
    (le, de, se, ge, pe, me, _), (lg, dg, sg, gg, pg, mg, ngraphs) = _dice_steps(e2e, [False, True])
    print("eager: losses", le, "nll / dice", de)
    print("graph: losses", lg, "nll / dice", dg)
    assert ngraphs == 2
    assert le == lg and de == dg, (le, lg, de, dg)
    for nm, x, y in (("dice sums", se, sg), ("gradient arena", ge, gg), ("bf16 parameters", pe, pg), ("fp32 masters", me, mg)):
        assert int((x != y).sum()) == 0, nm
