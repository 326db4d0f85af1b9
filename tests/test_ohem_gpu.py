"""GPU: the OHEM pixel sampler (csrc/ohem.hip) against its specifications -- `hip.ohem_select` bit for bit against
`ohem_reference`, `hip.seg_hardness` within 4 e of `hardness_reference`, the pair end to end, the criterion's fused path with
`ohem_thresh`, one training step (eager and graph-captured) on the segofa_tiny fixture, and the dispatcher op."""
import pytest
import torch

import _ohem_cases as OC
import _predict_cases as PC
from test_predict_views_gpu import e2e  # noqa: F401  (the segofa_tiny fixture with its three raw shapes)
from test_weighted_loss_gpu import _rel, _student

pytestmark = pytest.mark.gpu

SEG0 = OC.SEG0


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ifseg_amd.ops  # noqa: F401
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------- the select
@pytest.mark.parametrize("B,N,weighted", [(1, 1, False), (2, 255, False), (2, 257, False), (3, 4099, False), (2, 257, True)])
def test_select_is_exact(B, N, weighted):
    """every kind of plane under every regime, each launched twice into the same workspace: plane and info are the
    specification's bits both times, so the workspace is left clean"""
    from ifseg_amd import hip
    from ifseg_amd.criterions.seg_criterion import ohem_reference
    dev = _dev()
    work = hip.ohem_workspace(dev)
    w = OC.weight_plane(B, N) if weighted else None
    wd = w.to(dev) if weighted else None
    keys, got, want = [], [], []
    for kind in OC.KINDS:
        h = OC.plane(kind, B, N)
        hd = h.to(dev)
        for thresh, min_kept in OC.regimes(B, N):
            rp, ri = ohem_reference(h, thresh, min_kept, w)
            for rep in range(2):
                p, i = hip.ohem_select(hd, thresh, min_kept, weight=wd, work=work)
                keys.append((kind, thresh, min_kept, rep))
                got.append((p, i))
                want.append((rp, ri))
    torch.cuda.synchronize()
    wrong = [(k, i.tolist(), ri.tolist()) for k, (p, i), (rp, ri) in zip(keys, got, want)
             if not (torch.equal(p.cpu(), rp) and torch.equal(i.cpu(), ri))]
    assert len(keys) == 2 * len(OC.KINDS) * 6 and not wrong, wrong[:8]
    # what the next call counts into without clearing it -- the first digit's histogram and the below-thresh counter -- is zero
    assert int(work[:1024].abs().sum()) == 0 and int(work[3 * 1024]) == 0


def test_select_writes_in_place_and_refuses():
    from ifseg_amd import hip
    from ifseg_amd.criterions.seg_criterion import ohem_reference
    dev = _dev()
    B, N = 2, 257
    h = OC.plane("uniform", B, N)
    hd = h.to(dev)
    buf = torch.full((64 + B * N + 64,), 0xA5, dtype=torch.uint8, device=dev)
    out, info = buf[64:64 + B * N].view(B, N), torch.empty(4, dtype=torch.int64, device=dev)
    p, i = hip.ohem_select(hd, 0.5, 10, out=out, info=info)
    rp, ri = ohem_reference(h, 0.5, 10)
    assert p is out and i is info and torch.equal(out.cpu(), rp) and torch.equal(info.cpu(), ri)
    assert bool((buf[:64] == 0xA5).all()) and bool((buf[64 + B * N:] == 0xA5).all())
    for bad in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError, match="thresh"):
            hip.ohem_select(hd, bad, 1)
    with pytest.raises(ValueError, match="min_kept"):
        hip.ohem_select(hd, 0.5, -1)
    with pytest.raises(AssertionError):
        hip.ohem_select(hd, 0.5, 1, out=hd.view(torch.uint8)[:, :N])
    with pytest.raises(AssertionError):
        hip.ohem_select(hd, 0.5, 1, work=torch.zeros(8, dtype=torch.int64, device=dev))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- the hardness plane
@pytest.mark.parametrize("nseg,B,hp,wp", OC.HARD_CASES)
def test_hardness_is_the_specification(nseg, B, hp, wp):
    """tests/_predict_cases.py's rule: e = max |fp32 specification - fp64 specification| of the case; the kernel's values sit
    within 4 e of the fp64 specification, and -1 at exactly the invalid pixels.
    Measured on MI355X, in multiples of e, in the order of the cases: 0.48, 0.44, 0.34, 0.77, 0.31, 0.24 (an fp32 running sum
    measured 4.29 at 150 classes: the kernel keeps the sum and the last exponential in fp64)."""
    from ifseg_amd import hip
    dev = _dev()
    lp, tgt = OC.hard_inputs(nseg, B, hp, wp)
    s32, s64, valid, e = OC.hard_specs(nseg, B, hp, wp)
    H, W = 16 * hp, 16 * wp
    out = torch.full((B, H * W), 7.0, device=dev)
    got = hip.seg_hardness(lp.to(dev), tgt.to(dev), hp, wp, H, W, nseg, SEG0, out=out)
    assert got is out
    g = got.cpu()
    err = float((g.double() - s64)[valid].abs().max())
    print("hardness nseg %d B %d %dx%d: e %.3e, kernel max err %.3e = %.2f e; p in [%.4f, %.4f], %.1f %% below 0.7"
          % (nseg, B, hp, wp, e, err, err / e, float(s64[valid].min()), float(s64[valid].max()),
             100.0 * float((s64[valid] < 0.7).double().mean())))
    assert e > 0.0 and bool(valid.any()) and bool((~valid).any())
    assert torch.equal(g == -1.0, ~valid)
    assert float(g[valid].min()) >= 0.0 and float(g[valid].max()) <= 1.0
    assert err <= 4 * e, (err, e)


# ------------------------------------------------------------------------------------------------- the pair
@pytest.mark.parametrize("nseg,B,hp,wp", [(17, 2, 3, 4), (150, 1, 2, 3), (15, 2, 8, 8)])
def test_pair_end_to_end(nseg, B, hp, wp):
    """Order statistics are 1-Lipschitz: 4 e on the values and 4 e on tau cannot flip a pixel with |p64 - tau64| > 8 e, so
    outside that band the kept plane is the references'; the band may hold at most 1 % of the valid pixels."""
    from ifseg_amd import hip
    from ifseg_amd.criterions.seg_criterion import ohem_reference
    dev = _dev()
    lp, tgt = OC.hard_inputs(nseg, B, hp, wp)
    s32, s64, valid, e = OC.hard_specs(nseg, B, hp, wp)
    H, W = 16 * hp, 16 * wp
    hard = hip.seg_hardness(lp.to(dev), tgt.to(dev), hp, wp, H, W, nseg, SEG0)
    nv = int(valid.sum())
    p64 = s64[valid].sort().values
    for thresh, min_kept in [(0.7, 0), (0.7, H * W // 2), (0.05, H * W // 4), (0.7, 10 ** 6), (0.0, 100)]:
        plane, info = hip.ohem_select(hard, thresh, min_kept)
        rp, ri = ohem_reference(s32, thresh, min_kept)
        tau64 = max(float(torch.tensor(thresh, dtype=torch.float32)), float(p64[min(min_kept * B, nv - 1)]))
        band = valid & ((s64 - tau64).abs() <= 8 * e)
        nband = int(band.sum())
        plane, info = plane.cpu(), info.cpu()
        print("pair nseg %d (%.2f, %d): valid %d, kept %d (reference %d), band %d = %.3f %%"
              % (nseg, thresh, min_kept, nv, int(info[1]), int(ri[1]), nband, 100.0 * nband / nv))
        assert nband <= 0.01 * nv, (nband, nv)
        assert torch.equal(plane[~band], rp[~band])
        assert bool(((plane == 0) | (plane == 255)).all()) and int((plane == 255).sum()) == int(info[1])
        assert int(info[0]) == int(ri[0]) == nv
        assert abs(int(info[1]) - int(ri[1])) <= nband


# ------------------------------------------------------------------------------------------------- the criterion
def _task(ocfg):
    from ifseg_amd.tasks.mm_tasks import SegmentationTask
    P, n = ocfg.patch_image_size, ocfg.num_seg_tokens
    task = SegmentationTask(num_seg_tokens=n, patch_image_size=P, n_base_vocab=ocfg.vocab_size - 1, category_token_ids=PC.E2E_NAMES)
    task.prompt_ids = PC.E2E_PROMPT
    return task


def test_criterion_with_ohem(e2e):  # noqa: F811
    """the fused `compute_loss` with `ohem_thresh` against `weighted_loss_reference` on `upsample_logits` and the DEVICE's own
    plane (so no threshold-margin pixel enters), at test_weighted_kernel_is_the_specification's tolerances"""
    from ifseg_amd.criterions import SegCriterion
    from ifseg_amd.criterions.seg_criterion import weighted_loss_reference
    dev = _dev()
    _, raw, ocfg, _ = e2e
    _, sd, _, _ = PC.e2e_fixture()
    P, n = ocfg.patch_image_size, ocfg.num_seg_tokens
    task = _task(ocfg)
    task.build_train_transform(dev, seed=6, ratio_range=(1, 1))
    m = _student(ocfg, sd, dev)
    kw = dict(prompt_ids=PC.E2E_PROMPT, keep=0.5, boundary=1)
    s = task.self_train_sample(m, raw, 4, confidence_weight=True, **kw)
    plain = {k: v for k, v in s.items() if k != "target_weight"}
    tw, tgt = s["target_weight"], s["target"]
    ckw = dict(unsupervised_segmentation=False, init_seg_with_text=False)
    m.train()
    for norm in ("weights", "pixels"):
        crit = SegCriterion(task, ohem_thresh=0.7, ohem_min_kept=P * P // 4, weight_norm=norm, **ckw)
        base = SegCriterion(task, **ckw)
        with torch.no_grad():
            net_output = m(**s["net_input"], full_context_alignment=crit.full_context_alignment)
            hp, wp = net_output[1]["encoder_returns"]["image_embed_shape"][0]
            before, _, _ = base.compute_loss(m, net_output, plain, 0)
            fused, _, _ = crit.compute_loss(m, net_output, plain, 0)
            plane, info = crit._bufs_ohem["plane"].clone(), crit.ohem_info.clone()
            dl = crit._bufs["dl"][:, :, :n].clone()
            fused_w, _, _ = crit.compute_loss(m, net_output, s, 0)
            plane_w = crit._bufs_ohem["plane"].clone()
            after, _, _ = base.compute_loss(m, net_output, plain, 0)
            m.eval()
            in_eval, _, _ = crit.compute_loss(m, net_output, plain, 0)
            m.train()
        lf = net_output[1]["logits_padded"][:, :, :n].float().clone().requires_grad_(True)
        scores = SegCriterion.upsample_logits(lf, hp, wp, P, P)
        ref = weighted_loss_reference(scores[:, :P * P], tgt, task.seg_id_offset, n, None, plane, 0.0, norm)
        ref.backward()
        ref = ref.detach()
        ref_w = weighted_loss_reference(scores.detach()[:, :P * P], tgt, task.seg_id_offset, n, None, plane_w, 0.0, norm)
        info = info.tolist()
        print("criterion (%s): fused %.6f ref %.6f, grad rel %.2e, info %s" % (norm, float(fused), float(ref.detach()), _rel(dl, lf.grad), info))
        body = tgt[:, :-1]
        nvalid = int(((body >= task.seg_id_offset) & (body < task.seg_id_offset + n)).sum())
        assert info[0] == nvalid and info[1] == int((plane == 255).sum()) and 0 < info[1] <= nvalid
        assert bool(((plane == 0) | (plane == 255)).all())
        assert abs(float(fused) - float(ref)) < 2e-4 * max(1.0, abs(float(ref))), (float(fused), float(ref))
        assert _rel(dl, lf.grad) < 6e-3, _rel(dl, lf.grad)
        # the sample's own plane composes: kept pixels hold target_weight, dropped pixels 0
        assert torch.equal(plane_w, torch.where(plane == 255, tw, torch.zeros_like(tw)))
        assert abs(float(fused_w) - float(ref_w)) < 2e-4 * max(1.0, abs(float(ref_w))), (float(fused_w), float(ref_w))
        # the unweighted criterion is untouched by OHEM calls on the same model, and evaluation by the keyword
        assert torch.equal(before, after) and torch.equal(in_eval, before)


def _ohem_steps(e2e, graphs):  # noqa: F811
    """six `Trainer.train_step`s of segofa_tiny at P = 128 with an OHEM criterion, once per entry of `graphs` (captured from the
    third step on, or eager) -> per run (losses, infos, gradient arena, bf16 parameters, fp32 masters, graphs captured)"""
    from ifseg_amd.criterions import SegCriterion
    from ifseg_amd.trainer import Trainer
    dev = _dev()
    _, raw, ocfg, _ = e2e
    _, sd, _, _ = PC.e2e_fixture()
    P = ocfg.patch_image_size
    task = _task(ocfg)
    import segofa_ref as O
    ring = []
    for j in range(2):                                                       # the graph test's ring: resident bf16 batches
        batch = O.synthetic_batch(ocfg, 2, 12, seed=200 + j)                 # (token ids inside the fixture's vocabulary)
        sm = {"net_input": {k: batch[k].to(dev) for k in ("src_tokens", "patch_images", "patch_masks", "prev_output_tokens")},
              "target": batch["target"].to(dev), "ntokens": 1, "nsentences": 2}
        sm["net_input"]["patch_images"] = sm["net_input"]["patch_images"].to(torch.bfloat16)
        ring.append(sm)

    def run(graph):
        torch.manual_seed(0)
        m = _student(ocfg, sd, dev)
        # thresh 0: tau is the k-th value itself, the hardest eighth of an image's pixels per image
        crit = SegCriterion(task, unsupervised_segmentation=False, init_seg_with_text=False, ohem_thresh=0.0, ohem_min_kept=P * P // 8)
        tr = Trainer(m, crit, task, device=dev)
        p0 = tr.p32.clone()
        losses, infos = [], []
        for i in range(6):
            logs = tr.train_step([ring[i % 2]], prefetch=[ring[(i + 1) % 2]], graph=graph and i >= 2)
            losses.append(float(logs[-1]["loss"]))
            infos.append(crit.ohem_info.tolist())
        tr.check_overflow(wait=True)
        torch.cuda.synchronize()
        assert not torch.equal(tr.p32, p0)
        return losses, infos, tr.eng.g16.clone(), tr.eng.p16.clone(), tr.p32.clone(), len(tr._graphs)

    return [run(g) for g in graphs]


def test_training_step_with_ohem(e2e):  # noqa: F811
    """`Trainer.train_step` with an OHEM criterion moves the weights (asserted in the run) without overflow and keeps some but
    not all valid pixels"""
    (le, ie, _, _, _, _), = _ohem_steps(e2e, [False])
    print("eager: losses", le, "info", ie)
    assert all(l == l and abs(l) != float("inf") and l > 0.0 for l in le)
    assert all(0 < i[1] < i[0] for i in ie), ie


def test_captured_training_step_with_ohem_is_bit_identical_to_eager(e2e):  # noqa: F811
    """test_graph_captured_training_step_is_bit_identical_to_eager's pattern on the segofa_tiny fixture: losses, the sampler's
    info, gradients and parameters of the captured run are the eager run's bits.  (In a process where a stream handle was left
    pinned with hip.set_stream the capture used to miss the criterion's and the optimizer's launches -- the first replay
    differed and later ones repeated one value, with or without OHEM; Trainer._graph_step now pins the capture stream.)"""
    (le, ie, ge, pe, me, _), (lg, ig, gg, pg, mg, ngraphs) = _ohem_steps(e2e, [False, True])
    print("eager: losses", le, "info", ie)
    print("graph: losses", lg, "info", ig)
    assert ngraphs == 2
    assert le == lg and ie == ig, (le, lg, ie, ig)
    for nm, x, y in (("gradient arena", ge, gg), ("bf16 parameters", pe, pg), ("fp32 masters", me, mg)):
        assert int((x != y).sum()) == 0, nm


# ------------------------------------------------------------------------------------------------- the dispatcher
def test_op_is_the_binding():
    from ifseg_amd import hip
    dev = _dev()
    nseg, B, hp, wp = 15, 2, 8, 8
    H, W = 16 * hp, 16 * wp
    lp, tgt = (t.to(dev) for t in OC.hard_inputs(nseg, B, hp, wp))
    w = OC.weight_plane(B, H * W).to(dev)
    for weight in (None, w):
        want = hip.ohem_select(hip.seg_hardness(lp, tgt, hp, wp, H, W, nseg, SEG0), 0.7, H * W // 4, weight=weight)
        got = torch.ops.ifseg.seg_ohem(lp[:, :, :nseg], tgt, weight, hp, wp, H, W, SEG0, 0.7, H * W // 4)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and 0 < int(got[1][1]) < int(got[1][0])
    meta = torch.ops.ifseg.seg_ohem(lp[:, :, :nseg].to("meta"), tgt.to("meta"), None, hp, wp, H, W, SEG0, 0.7, 5)
    assert meta[0].dtype == torch.uint8 and tuple(meta[0].shape) == (B, H * W) and meta[0].device.type == "meta"
    assert meta[1].dtype == torch.int64 and tuple(meta[1].shape) == (4,)
    with pytest.raises(ValueError, match="thresh"):
        torch.ops.ifseg.seg_ohem(lp[:, :, :nseg], tgt, None, hp, wp, H, W, SEG0, 1.5, 5)
    with pytest.raises(ValueError, match="pixel_weight"):
        torch.ops.ifseg.seg_ohem(lp[:, :, :nseg], tgt, w[:, :-1], hp, wp, H, W, SEG0, 0.7, 5)
