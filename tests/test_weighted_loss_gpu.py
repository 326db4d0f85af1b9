"""GPU: the weighted criterion path against its specifications -- the weighted instantiation of the fused loss kernel
(csrc/loss.hip) against `upsample_logits` + `weighted_loss_reference` with autograd, `hip.train_load_plane` against
`augment.train_plane_reference`, the weight plane of `hip.seg_pseudo` against `pseudo_label_reference`, the dispatcher op, and
`task.self_train_sample(confidence_weight=True)` through the criterion and one training step on the segofa_tiny fixture."""
import functools

import pytest
import torch

import _predict_cases as PC
import _train_load_cases as TC
from ifseg_amd import augment as A
from test_predict_views_gpu import e2e  # noqa: F401  (the segofa_tiny fixture with its three raw shapes)
from test_pseudo_gpu import SPECIAL, make_conf, make_thresholds
from test_render_gpu import make_labels

pytestmark = pytest.mark.gpu

SEG0 = 1000


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ifseg_amd.ops  # noqa: F401
    return torch.device("cuda:0")


def _rel(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


@functools.lru_cache(maxsize=None)
def _inputs(nseg, B, hp, wp):
    """test_fused_seg_loss's inputs plus the two weights, on the host, computed once per shape; nobody writes to them"""
    P, H, W = hp * wp, hp * 16, wp * 16
    npad = (nseg + 7) // 8 * 8
    g = torch.Generator().manual_seed(7)
    lp = torch.zeros(B, P + 1, npad, dtype=torch.bfloat16)
    lp[:, :, :nseg] = torch.randn(B, P + 1, nseg, generator=g) * 2
    tgt = torch.randint(0, nseg + 1, (B, H * W), generator=g) + SEG0        # includes the ignore label seg0 + nseg
    tgt = torch.cat([tgt, torch.full((B, 1), 2)], 1)
    cw = torch.rand(nseg, generator=g) * 1.5 + 0.5
    cw[nseg // 2] = 0.0
    pw = torch.randint(0, 256, (B, H, W), generator=g, dtype=torch.uint8)
    pw[0, :16, :16] = 0                                                      # one whole tile of zeros, one of 255
    pw[B - 1, H - 16:, W - 16:] = 255
    return lp, tgt, cw, pw.reshape(B, H * W)


def _launch(lp, tgt, hp, wp, nseg, eps, cw, pw, norm_pixels, weighted=True):
    from ifseg_amd import hip
    dev = lp.device
    B, P, H, W = lp.shape[0], hp * wp, hp * 16, wp * 16
    tile = torch.empty(B * P * 9 * nseg, device=dev)
    sp = torch.empty(B * P * (2 + 3 * nseg), device=dev)
    stats = torch.empty(2 + 3 * nseg, device=dev)
    dl = torch.full(tuple(lp.shape), 3.0, dtype=torch.bfloat16, device=dev)
    loss = torch.empty(1, device=dev)
    if weighted:
        hip.seg_loss_weighted(lp, tgt, hp, wp, H, W, nseg, SEG0, tile, sp, stats, dl, loss, pixel_weight=pw, class_weight=cw,
                              norm_pixels=norm_pixels, label_smoothing=eps)
    else:
        hip.seg_loss(lp, tgt, hp, wp, H, W, nseg, SEG0, tile, sp, stats, dl, loss, label_smoothing=eps)
    return loss, stats, dl


CASES = [(5, 2, 3, 4, 0.0, True, True, "weights"), (17, 2, 3, 4, 0.1, True, True, "weights"),
         (150, 1, 2, 3, 0.1, True, False, "weights"), (15, 2, 3, 4, 0.0, False, True, "pixels"),
         (15, 2, 3, 4, 0.1, True, True, "pixels"), (512, 1, 2, 3, 0.2, True, True, "pixels"),
         (171, 1, 4, 6, 0.0, False, True, "weights"), (15, 2, 8, 8, 0.1, True, True, "weights")]


@pytest.mark.parametrize("nseg,B,hp,wp,eps,use_cw,use_pw,norm", CASES)
def test_weighted_kernel_is_the_specification(nseg, B, hp, wp, eps, use_cw, use_pw, norm):
    """the tolerances are test_fused_seg_loss's: the arithmetic and the bf16 gradient store are the same"""
    from ifseg_amd.criterions import SegCriterion
    from ifseg_amd.criterions.seg_criterion import weighted_loss_reference
    dev = _dev()
    P, H, W = hp * wp, hp * 16, wp * 16
    lp, tgt, cw, pw = (t.to(dev) for t in _inputs(nseg, B, hp, wp))
    cw, pw = (cw if use_cw else None), (pw if use_pw else None)
    loss, stats, dl = _launch(lp, tgt, hp, wp, nseg, eps, cw, pw, norm == "pixels")
    lf = lp[:, :, :nseg].float().clone().requires_grad_(True)
    scores = SegCriterion.upsample_logits(lf, hp, wp, H, W)
    ref = weighted_loss_reference(scores, tgt, SEG0, nseg, cw, pw, eps, norm)
    ref.backward()
    mask = (tgt == 1) | (tgt == SEG0 + nseg) | (tgt == 2)
    t = tgt[~mask] - SEG0
    sc = scores.detach()[~mask]
    ai, ap, al, au = SegCriterion.compute_metric(sc, t)
    nvalid = int((~mask).sum())
    valid = ~mask[:, :-1]
    q64 = pw.double()[valid] if use_pw else torch.ones(nvalid, dtype=torch.float64, device=dev)
    c64 = cw.double()[t] if use_cw else torch.ones(nvalid, dtype=torch.float64, device=dev)
    Z = float((q64 * c64).sum()) if norm == "weights" else (255.0 if use_pw else 1.0) * nvalid
    torch.cuda.synchronize()
    print("loss", loss.item(), "ref", ref.item(), "grad rel", _rel(dl[:, :, :nseg], lf.grad), "Z", stats[1].item(), Z)
    assert abs(loss.item() - ref.item()) < 2e-4 * max(1.0, abs(ref.item())), (loss.item(), ref.item())
    assert _rel(dl[:, :, :nseg], lf.grad) < 6e-3, _rel(dl[:, :, :nseg], lf.grad)
    assert dl[:, :, nseg:].abs().sum() == 0 and dl[:, P].abs().sum() == 0
    assert abs(stats[1].item() - Z) <= 1e-6 * Z, (stats[1].item(), Z)
    if norm == "pixels" and not use_pw:
        assert stats[1].item() == nvalid
    n = nseg
    assert (stats[2 + n:2 + 2 * n] - ap).abs().sum().item() <= 1e-4 * H * W * B + 2
    assert torch.equal(stats[2 + 2 * n:2 + 3 * n], al)
    assert (stats[2:2 + n] - ai).abs().sum().item() <= 1e-4 * H * W * B + 2


def test_pixels_norm_without_a_plane_counts_the_valid_pixels():
    """norm "pixels" with class weights only: Z is exactly N_valid"""
    dev = _dev()
    nseg, B, hp, wp = 15, 2, 3, 4
    lp, tgt, cw, _ = (t.to(dev) for t in _inputs(nseg, B, hp, wp))
    _, stats, _ = _launch(lp, tgt, hp, wp, nseg, 0.1, cw, None, True)
    mask = (tgt == 1) | (tgt == SEG0 + nseg) | (tgt == 2)
    assert stats[1].item() == int((~mask).sum())


def test_neutral_weights_are_the_unweighted_kernel():
    dev = _dev()
    nseg, B, hp, wp = 15, 2, 3, 4
    lp, tgt, _, pw = (t.to(dev) for t in _inputs(nseg, B, hp, wp))
    mask = (tgt == 1) | (tgt == SEG0 + nseg) | (tgt == 2)
    for eps in (0.0, 0.1):
        l0, s0, d0 = _launch(lp, tgt, hp, wp, nseg, eps, None, None, False, weighted=False)
        for cw, plane in ((torch.ones(nseg, device=dev), torch.ones_like(pw)), (None, None)):
            l1, s1, d1 = _launch(lp, tgt, hp, wp, nseg, eps, cw, plane, False)
            assert torch.equal(s1[2:], s0[2:])
            assert s1[1].item() == int((~mask).sum()) == s0[1].item()
            assert abs(l1.item() - l0.item()) < 2e-4 * max(1.0, abs(l0.item())), (l1.item(), l0.item())
            assert _rel(d1[:, :, :nseg], d0[:, :, :nseg]) < 6e-3
            assert d1[:, :, nseg:].abs().sum() == 0 and d1[:, hp * wp].abs().sum() == 0


def test_scale_of_the_plane_does_not_change_a_bit():
    """norm "weights": every operation is linear in q and a factor two is exact in binary floating point"""
    dev = _dev()
    nseg, B, hp, wp = 15, 2, 3, 4
    lp, tgt, cw, pw = (t.to(dev) for t in _inputs(nseg, B, hp, wp))
    q = pw // 2                                                              # <= 127, zeros among them
    for eps in (0.0, 0.1):
        l1, s1, d1 = _launch(lp, tgt, hp, wp, nseg, eps, cw, q, False)
        l2, s2, d2 = _launch(lp, tgt, hp, wp, nseg, eps, cw, q * 2, False)
        assert torch.equal(l1, l2) and torch.equal(d1, d2) and torch.equal(s1[2:], s2[2:])
        assert torch.equal(s1[:2] * 2, s2[:2])
        assert float(l1) > 0.0 and float(d1.float().abs().max()) > 0.0


def test_all_zero_plane_and_the_same_launch_twice():
    dev = _dev()
    nseg, B, hp, wp = 15, 2, 3, 4
    lp, tgt, cw, pw = (t.to(dev) for t in _inputs(nseg, B, hp, wp))
    _, s0, _ = _launch(lp, tgt, hp, wp, nseg, 0.1, None, None, False, weighted=False)
    loss, stats, dl = _launch(lp, tgt, hp, wp, nseg, 0.1, cw, torch.zeros_like(pw), False)
    assert loss.item() == 0.0 and stats[0].item() == 0.0 and stats[1].item() == 0.0
    assert float(dl.float().abs().max()) == 0.0
    assert torch.equal(stats[2:], s0[2:]) and float(stats[2:].sum()) > 0.0   # the histograms are still counted
    a = _launch(lp, tgt, hp, wp, nseg, 0.1, cw, pw, False)
    b = _launch(lp, tgt, hp, wp, nseg, 0.1, cw, pw, False)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_entry_point_refusals():
    """return codes, nothing launched: the shapes the unweighted entry refuses, and a negative label_smoothing"""
    from ifseg_amd import hip
    dev = _dev()
    nseg, B, hp, wp = 15, 2, 3, 4
    lp, tgt, cw, pw = (t.to(dev) for t in _inputs(nseg, B, hp, wp))
    H, W = 16 * hp, 16 * wp
    buf = lambda k: torch.empty(k, device=dev)
    args = lambda **kw: dict(dict(pixel_weight=pw, class_weight=cw, label_smoothing=0.0), **kw)
    call = lambda H_, W_, n_, **kw: hip.seg_loss_weighted(lp, tgt, hp, wp, H_, W_, n_, SEG0, buf(B * hp * wp * 9 * nseg),
                                                          buf(B * hp * wp * (2 + 3 * nseg)), buf(2 + 3 * nseg),
                                                          torch.empty_like(lp), buf(1), **kw)
    with pytest.raises(RuntimeError, match="code -3"):
        call(H, W, nseg, **args(label_smoothing=-0.1))
    with pytest.raises(RuntimeError, match="code -2"):
        call(H + 16, W, nseg, **args(pixel_weight=None))
    with pytest.raises(RuntimeError, match="code -2"):
        call(H, W, 0, **args(class_weight=None))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- the plane
def _plane_records(H0, W0, P, flips):
    nh, nw = A.resized_size(H0, W0, max(P, 45))
    offs = [(0, 0), (nh - P, nw - P), ((nh - P) // 2, (nw - P) // 3)]
    return torch.tensor([TC.record(nh, nw, oh, ow, f) for (oh, ow), f in zip(offs, flips)], dtype=torch.int32)


@pytest.mark.parametrize("flip", [0, 1])
def test_train_load_plane_is_the_specification(flip):
    """B = 3 ragged sources at P = 32 under hand-written records (both offsets' ends), between canary bytes at output byte
    offsets 0 .. 3, with the records on the host and on the device"""
    from ifseg_amd import hip
    dev = _dev()
    P = 32
    shapes = [(37, 53), (80, 41), (37, 53)]
    planes = [TC.label("random", h, w) if i < 2 else TC.image(h, w, 5)[..., 0].contiguous() for i, (h, w) in enumerate(shapes)]
    recs = torch.cat([_plane_records(h, w, P, [flip] * 3)[i:i + 1] for i, (h, w) in enumerate(shapes)])
    want = A.train_plane_reference(planes, recs, P).to(dev)
    dplanes = [p.to(dev) for p in planes]
    same = []
    buf = torch.empty(64 + 4 + 3 * P * P + 64, dtype=torch.uint8, device=dev)
    for oo in range(4):
        for params in (recs, recs.to(dev)):
            buf.fill_(0xA5)
            out = buf[64 + oo:64 + oo + 3 * P * P].view(3, P * P)
            got = hip.train_load_plane(dplanes, params, P, out=out)
            assert got is out
            same.append(torch.stack([(out == want).all(), (buf[:64 + oo] == 0xA5).all(), (buf[64 + oo + 3 * P * P:] == 0xA5).all()]))
    fresh = hip.train_load_plane(dplanes, recs.to(dev), P, table=hip._train_table(None, dplanes))
    assert torch.equal(fresh, want)
    assert all(all(ok) for ok in torch.stack(same).cpu().tolist()), same


def test_train_load_plane_ragged_tiles_and_a_single_pixel_source():
    from ifseg_amd import hip
    dev = _dev()
    P = 33                                                                   # one tile column of 33, three tile rows: 16, 16, 1
    planes = [TC.label("random", 37, 53), torch.tensor([[77]], dtype=torch.uint8), TC.image(80, 41, 2)[..., 1].contiguous()]
    recs = torch.tensor([TC.record(40, 57, 7, 24, 1), TC.record(50, 50, 17, 0, 0), TC.record(120, 62, 87, 29, 1)], dtype=torch.int32)
    want = A.train_plane_reference(planes, recs, P)
    assert bool((want[1] == 77).all())
    buf = torch.full((3 * P * P + 128,), 0xA5, dtype=torch.uint8, device=dev)
    out = hip.train_load_plane([p.to(dev) for p in planes], recs.to(dev), P, out=buf[64:64 + 3 * P * P].view(3, P * P))
    assert torch.equal(out.cpu(), want)
    assert bool((buf[:64] == 0xA5).all()) and bool((buf[64 + 3 * P * P:] == 0xA5).all())
    # a record that holds no window: refused on the host, zeros for its sample from the device
    bad = recs.clone()
    bad[1, A.R_OFF_H] = 18
    with pytest.raises(RuntimeError, match="code -2"):
        hip.train_load_plane([p.to(dev) for p in planes], bad, P)
    got = hip.train_load_plane([p.to(dev) for p in planes], bad.to(dev), P).cpu()
    assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2]) and int(got[1].max()) == 0


def test_transform_carries_the_plane_like_the_cpu_transform():
    dev = _dev()
    P = 32
    imgs, labs = TC.ragged_batch()
    planes = [TC.image(*l.shape, 40 + i)[..., 0].contiguous() for i, l in enumerate(labs)]
    kw = dict(seed=9)
    cpu = A.TrainTransform(P, TC.NSEG, TC.SEG0, device="cpu", **kw)(imgs, labs, 11, weights=planes)
    gpu = A.TrainTransform(P, TC.NSEG, TC.SEG0, device=dev, **kw)(imgs, labs, 11, weights=planes)
    assert len(gpu) == 3 and gpu[2].is_cuda and gpu[2].dtype == torch.uint8
    assert torch.equal(gpu[1].cpu(), cpu[1]) and torch.equal(gpu[2].cpu(), cpu[2])


# ------------------------------------------------------------------------------------------------- the pseudo-label weight
@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16])
def test_pseudo_weight_is_the_specification(dtype):
    from ifseg_amd import hip
    from ifseg_amd.predict import pseudo_label_reference
    dev = _dev()
    n = 15
    assert len(SPECIAL) == 11
    keys, same = [], []
    for H, W in ((1, 1), (17, 65), (33, 129)):
        labels, conf, thr = make_labels(H, W, n, dtype, 3), make_conf((H, W), 5), make_thresholds(n, 4)
        if H * W == 1:
            labels[0, 0], thr[:] = 3, 0                                      # the one pixel is kept: conf 0.0, bin 0, weight 1
        ld, cd, td = labels.to(dev), conf.to(dev), thr.to(dev)
        for r in (0, 1, 4):
            want = [t.to(dev) for t in pseudo_label_reference(labels, conf, thr, n, r, True, weight=True)]
            out, kept, wt = hip.seg_pseudo(ld, cd, td, n, r, True, weight=True)
            out2, kept2 = hip.seg_pseudo(ld, cd, td, n, r, True)
            assert wt.dtype == torch.uint8 and wt.shape == out.shape
            keys.append((H, W, r))
            same.append(torch.stack([(out == want[0]).all(), (kept == want[1]).all(), (wt == want[2]).all(),
                                     (out == out2).all(), (kept == kept2).all(), ((wt == 0) == (out == 255)).all()]))
    same = torch.stack(same).cpu().tolist()
    wrong = [(k, ok) for k, ok in zip(keys, same) if not all(ok)]
    assert len(keys) == 9 and not wrong, wrong


# ------------------------------------------------------------------------------------------------- the dispatcher
def test_op_is_the_binding_and_differentiable():
    dev = _dev()
    nseg, B, hp, wp = 15, 2, 3, 4
    H, W = 16 * hp, 16 * wp
    lp, tgt, cw, pw = (t.to(dev) for t in _inputs(nseg, B, hp, wp))
    want = _launch(lp, tgt, hp, wp, nseg, 0.1, cw, pw, True)
    logits = lp[:, :, :nseg].clone().requires_grad_(True)                    # 15 columns: the op pads them itself
    loss, stats, dl, bad = torch.ops.ifseg.seg_loss_weighted(logits, tgt, pw, cw, hp, wp, H, W, SEG0, 0.1, True)
    assert torch.equal(loss, want[0][0]) and torch.equal(stats, want[1]) and torch.equal(dl, want[2]) and int(bad) == 0
    (loss * 3.0).backward()
    assert torch.equal(logits.grad, dl[:, :, :nseg] * torch.tensor(3.0, dtype=torch.bfloat16, device=dev))
    none = torch.ops.ifseg.seg_loss_weighted(lp[:, :, :nseg], tgt, None, None, hp, wp, H, W, SEG0, 0.0, False)
    plain = torch.ops.ifseg.seg_loss(lp[:, :, :nseg], tgt, hp, wp, H, W, SEG0, 0.0)
    assert torch.equal(none[1][1:], plain[1][1:]) and abs(float(none[0]) - float(plain[0])) < 2e-4 * max(1.0, float(plain[0]))


# ------------------------------------------------------------------------------------------------- end to end
def _student(ocfg, sd, dev):
    from ifseg_amd.models.segofa import SegOFAModel, make_config
    m = SegOFAModel(make_config("segofa_tiny", embed_dim=ocfg.embed_dim, ffn_dim=ocfg.ffn_dim, heads=ocfg.heads,
                                enc_layers=ocfg.enc_layers, dec_layers=ocfg.dec_layers, resnet_layers=ocfg.resnet_layers,
                                num_seg_tokens=ocfg.num_seg_tokens, vocab_size=ocfg.vocab_size,
                                patch_image_size=ocfg.patch_image_size, orig_patch_image_size=ocfg.orig_patch_image_size))
    torch.nn.Module.load_state_dict(m, sd, strict=False)
    m.cfg.dropout = m.cfg.encoder_drop_path_rate = m.cfg.decoder_drop_path_rate = 0.0
    return m.to(dev)


def test_confidence_weighted_self_training_step(e2e):  # noqa: F811
    """segofa_tiny at P = 128, modelled on test_self_train_sample_through_one_training_step: the sample's `target_weight` is
    the CPU transform of the results' weight planes, the fused weighted loss is `compute_loss_torch`'s, the unweighted loss
    is untouched by weighted calls, and one training step on the weighted sample moves the weights"""
    from ifseg_amd.criterions import SegCriterion
    from ifseg_amd.tasks.mm_tasks import SegmentationTask
    from ifseg_amd.trainer import Trainer
    dev = _dev()
    _, raw, ocfg, _ = e2e
    _, sd, _, src = PC.e2e_fixture()
    P, n = ocfg.patch_image_size, ocfg.num_seg_tokens
    task = SegmentationTask(num_seg_tokens=n, patch_image_size=P, n_base_vocab=ocfg.vocab_size - 1, category_token_ids=PC.E2E_NAMES)
    task.prompt_ids = PC.E2E_PROMPT
    tf = task.build_train_transform(dev, seed=6, ratio_range=(1, 1))
    m = _student(ocfg, sd, dev)
    kw = dict(prompt_ids=PC.E2E_PROMPT, keep=0.5, boundary=1)
    s = task.self_train_sample(m, raw, 4, confidence_weight=True, **kw)
    plain = task.self_train_sample(m, raw, 4, **kw)
    assert "target_weight" not in plain and torch.equal(plain["target"], s["target"])
    tw = s["target_weight"]
    assert tw.is_cuda and tw.dtype == torch.uint8 and tuple(tw.shape) == (3, P * P)
    res = task.pseudo_label_raw(m, raw, return_weight=True, **kw)
    assert all(r.weight is not None and torch.equal(r.weight == 0, r.labels == 255) for r in res)
    recs = tf.draw(raw, [r.labels for r in res], 4).cpu()
    cpu_tf = A.TrainTransform(P, n, task.seg_id_offset, device="cpu")
    assert torch.equal(tw.cpu(), cpu_tf.apply([x.cpu() for x in raw], [r.labels.cpu() for r in res], recs,
                                              weights=[r.weight.cpu() for r in res])[2])
    body = s["target"][:, :-1]
    assert bool((tw[body == task.seg_id_offset + n] == 0).all()) and bool((tw > 0).any())

    cw = torch.linspace(0.5, 2.0, n).tolist()
    crit = SegCriterion(task, unsupervised_segmentation=False, init_seg_with_text=False, class_weight=cw)
    m.train()
    with torch.no_grad():
        net_output = m(**s["net_input"], full_context_alignment=crit.full_context_alignment)
        base = SegCriterion(task, unsupervised_segmentation=False, init_seg_with_text=False)
        before, _, _ = base.compute_loss(m, net_output, plain, 0)
        fused, metrics, _ = crit.compute_loss(m, net_output, s, 0)
        ref, _, _ = crit.compute_loss_torch(m, net_output, s, 0)
        after, _, _ = base.compute_loss(m, net_output, plain, 0)
    assert abs(float(fused) - float(ref)) < 2e-4 * max(1.0, abs(float(ref))), (float(fused), float(ref))
    assert torch.equal(before, after) and float(before) != float(fused)

    tr = Trainer(m, SegCriterion(task, unsupervised_segmentation=False, init_seg_with_text=False, class_weight=cw), task, device=dev)
    p_before = tr.p32.clone()
    loss = float(tr.train_step([s])[0]["loss"])
    tr.check_overflow(wait=True)
    torch.cuda.synchronize()
    assert loss == loss and abs(loss) != float("inf") and loss > 0.0
    assert not torch.equal(tr.p32, p_before)

