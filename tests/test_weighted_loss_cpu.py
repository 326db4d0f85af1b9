"""CPU: the specifications of the weighted criterion path -- `weighted_loss_reference` against its closed formulas in float64,
`compute_loss_torch` with weights, `train_plane_reference` tied to the label tap's geometry, `pseudo_label_reference`'s weight
plane -- and the surface: header, dispatcher schema, fake shapes, refusals.  No kernel is launched."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import _train_load_cases as TC
from ifseg_amd import augment as A

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
F64 = torch.float64
SEG0 = 100


def _case(n=7, B=2, npix=40, seed=0, zero_class=2):
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(B, npix, n, generator=g, dtype=F64) * 2
    t = torch.randint(0, n + 1, (B, npix + 1), generator=g) + SEG0          # the ignore class <seg_n> among them
    t[0, 3], t[1, 5], t[:, -1] = 1, 2, 2                                    # pad, eos, the eos column
    t[0, 0] = SEG0 + zero_class                                             # the zero-weight class occurs
    cw = torch.rand(n, generator=g, dtype=F64) * 1.5 + 0.5
    cw[zero_class] = 0.0
    q = torch.randint(0, 256, (B, npix), generator=g, dtype=torch.uint8)
    q[0, :4], q[1, :4] = 0, 255
    return s, t, cw, q


def _closed(s, t, cw, q, eps, norm, n):
    """section 1 of the specification written out: -> (loss, d loss / d scores) in float64, no autograd"""
    B, npix, _ = s.shape
    tg = t[:, :npix]
    valid = ~((tg == 1) | (tg == 2) | (tg == SEG0 + n))
    y = (tg - SEG0).clamp(0, n - 1)
    cw = torch.ones(n, dtype=F64) if cw is None else cw
    qf = torch.ones(B, npix, dtype=F64) if q is None else q.to(F64)
    lse = torch.logsumexp(s, -1)
    vy = s.gather(-1, y[..., None])[..., 0]
    cwy = cw[y]
    scw = cw.sum()
    l = (1 - eps) * cwy * (lse - vy) + (eps / n) * (scw * lse - (s * cw).sum(-1))
    num = (qf * l)[valid].sum()
    Z = (qf * cwy)[valid].sum() if norm == "weights" else (255.0 if q is not None else 1.0) * valid.sum().to(F64)
    p = torch.softmax(s, -1)
    Aw = (1 - eps) * cwy + (eps / n) * scw
    d = qf[..., None] * (p * Aw[..., None] - F.one_hot(y, n).to(F64) * ((1 - eps) * cwy)[..., None] - (eps / n) * cw)
    d = d * valid[..., None].to(F64)
    if float(Z) == 0.0:
        return torch.zeros((), dtype=F64), torch.zeros_like(s)
    return num / Z, d / Z


@pytest.mark.parametrize("norm", ["weights", "pixels"])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("use_cw,use_q", [(True, True), (True, False), (False, True)])
def test_reference_is_the_closed_formula(eps, norm, use_cw, use_q):
    from ifseg_amd.criterions.seg_criterion import weighted_loss_reference
    n = 7
    s, t, cw, q = _case(n)
    cw, q = (cw if use_cw else None), (q if use_q else None)
    sg = s.clone().requires_grad_(True)
    loss = weighted_loss_reference(sg, t, SEG0, n, cw, q, eps, norm)
    loss.backward()
    want, dwant = _closed(s, t, cw, q, eps, norm, n)
    assert loss.dtype == F64 and abs(float(loss.detach()) - float(want)) <= 1e-12, (float(loss.detach()), float(want))
    assert float((sg.grad - dwant).abs().max()) <= 1e-12
    assert float(want) > 0.0


@pytest.mark.parametrize("norm", ["weights", "pixels"])
def test_reference_with_a_zero_normaliser(norm):
    """Z = 0: an all-zero plane under "weights", no valid pixel under either -> loss 0, gradient 0"""
    from ifseg_amd.criterions.seg_criterion import weighted_loss_reference
    n = 7
    s, t, cw, q = _case(n)
    cases = [(torch.full_like(t, SEG0 + n), q)]
    if norm == "weights":
        cases.append((t, torch.zeros_like(q)))
        only = t.clone()
        only[:, :-1] = SEG0 + 2                                             # every pixel of the zero-weight class
        cases.append((only, q))
    for tt, qq in cases:
        sg = s.clone().requires_grad_(True)
        loss = weighted_loss_reference(sg, tt, SEG0, n, cw, qq, 0.1 if norm == "pixels" else 0.0, norm)
        loss.backward()
        assert float(loss.detach()) == 0.0 and float(sg.grad.abs().max()) == 0.0


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_reference_without_weights_is_cross_entropy(eps):
    from ifseg_amd.criterions.seg_criterion import weighted_loss_reference
    n = 7
    s, t, _, _ = _case(n, seed=3)
    tg = t[:, :-1]
    mask = ~((tg == 1) | (tg == 2) | (tg == SEG0 + n))
    want = F.cross_entropy(s[mask], tg[mask] - SEG0, label_smoothing=eps)
    for norm in ("weights", "pixels"):
        got = weighted_loss_reference(s, t, SEG0, n, label_smoothing=eps, weight_norm=norm)
        assert abs(float(got) - float(want)) <= 1e-12
    # a trailing eos row of the scores is ignored as well
    s1 = torch.cat([s, torch.randn(2, 1, n, dtype=F64)], 1)
    assert abs(float(weighted_loss_reference(s1, t, SEG0, n, label_smoothing=eps)) - float(want)) <= 1e-12


def _crit(n, **kw):
    from ifseg_amd.criterions import SegCriterion
    return SegCriterion(None, unsupervised_segmentation="false", init_seg_with_text="false", num_seg_tokens=n, seg_id_offset=SEG0, **kw)


def _torch_inputs(n, B=2, hp=2, wp=3, seed=5):
    g = torch.Generator().manual_seed(seed)
    h, w = 16 * hp, 16 * wp
    low = torch.randn(B, hp * wp + 1, n, generator=g)
    tgt = torch.randint(0, n + 1, (B, h * w), generator=g) + SEG0
    tgt = torch.cat([tgt, torch.full((B, 1), 2)], 1)
    q = torch.randint(0, 256, (B, h * w), generator=g, dtype=torch.uint8)
    net_output = (low, {"encoder_returns": {"image_embed_shape": [(hp, wp)]}})
    sample = {"target": tgt, "net_input": {"patch_images": torch.zeros(B, 3, h, w)}}
    return net_output, sample, q, (hp, wp, h, w)


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_compute_loss_torch_honours_the_weights(eps):
    from ifseg_amd.criterions import SegCriterion
    from ifseg_amd.criterions.seg_criterion import weighted_loss_reference
    n = 6
    net_output, sample, q, (hp, wp, h, w) = _torch_inputs(n)
    low, tgt = net_output[0], sample["target"]
    scores = SegCriterion.upsample_logits(low.float(), hp, wp, h, w)
    # without weights: today's expression, bit for bit
    mask = (tgt == 1) | (tgt == SEG0 + n) | (tgt == 2)
    today = F.cross_entropy(scores[~mask], tgt[~mask] - SEG0, label_smoothing=eps)
    loss, metrics, ntok = _crit(n, label_smoothing=eps).compute_loss_torch(None, net_output, sample, 0)
    assert torch.equal(loss, today) and torch.equal(metrics["nll_loss"], today) and ntok == 1
    cw = torch.tensor([0.5, 2.0, 0.0, 1.0, 1.5, 0.75])
    for norm in ("weights", "pixels"):
        for use_cw, use_q in ((True, True), (True, False), (False, True)):
            crit = _crit(n, label_smoothing=eps, class_weight=cw if use_cw else None, weight_norm=norm)
            smp = dict(sample, target_weight=q) if use_q else sample
            got, m2, _ = crit.compute_loss_torch(None, net_output, smp, 0)
            want = weighted_loss_reference(scores[:, :-1], tgt, SEG0, n, cw if use_cw else None, q if use_q else None, eps, norm)
            assert torch.equal(got, want), (norm, use_cw, use_q, float(got), float(want))
            assert torch.equal(m2["area_label"], metrics["area_label"]) and torch.equal(m2["area_pred_label"], metrics["area_pred_label"])
    assert float(want) != float(today)


# ------------------------------------------------------------------------------------------------- the plane
@pytest.mark.parametrize("H0,W0", [(37, 53), (80, 41)])
@pytest.mark.parametrize("flip", [0, 1])
def test_plane_follows_the_label_tap(H0, W0, flip):
    """the label map itself as the plane: what comes out, remapped, is the target -- the plane's geometry is the target's"""
    P = 32
    lab = TC.label("random", H0, W0)
    img = TC.image(H0, W0, 1)
    nh, nw = A.resized_size(H0, W0, 45)
    recs = torch.tensor([TC.record(nh, nw, 0, 0, flip), TC.record(nh, nw, nh - P, nw - P, flip), TC.record(nh, nw, 5, 3, flip)],
                        dtype=torch.int32)
    tf = A.TrainTransform(P, TC.NSEG, TC.SEG0, device="cpu")
    out = tf.apply([img] * 3, [lab] * 3, recs, weights=[lab] * 3)
    assert len(out) == 3
    pi, target, plane = out
    two = tf.apply([img] * 3, [lab] * 3, recs)
    assert len(two) == 2 and torch.equal(two[0], pi) and torch.equal(two[1], target)
    assert plane.dtype == torch.uint8 and tuple(plane.shape) == (3, P * P)
    assert torch.equal(plane, A.train_plane_reference([lab] * 3, recs, P))
    assert torch.equal(A.remap_label(plane, TC.NSEG), target[:, :-1] - TC.SEG0)
    assert len(plane.unique()) > TC.NSEG                                     # raw values, 0 and 255 among them, not classes
    # the same independently of train_load_reference
    for b in range(3):
        assert torch.equal(A.remap_label(plane[b], TC.NSEG) + TC.SEG0, TC.target_of(lab, recs[b], P)[:-1])
    if flip:
        unflipped = A.train_plane_reference([lab], recs[:1].clone().index_fill_(1, torch.tensor([A.R_FLIP]), 0), P)
        assert torch.equal(plane[0].view(P, P), unflipped[0].view(P, P).flip(1))


def test_transform_call_with_weights_draws_the_same_records():
    P = 32
    imgs, labs = TC.ragged_batch()
    tf = A.TrainTransform(P, TC.NSEG, TC.SEG0, seed=9, device="cpu")
    pi, target, plane = tf(imgs, labs, 11, weights=labs)
    pi2, target2 = tf(imgs, labs, 11)
    assert torch.equal(pi, pi2) and torch.equal(target, target2)
    assert torch.equal(A.remap_label(plane, TC.NSEG), target[:, :-1] - TC.SEG0)
    with pytest.raises(ValueError, match="weight planes must be uint8"):
        tf(imgs, labs, 11, weights=[l.float() for l in labs])
    with pytest.raises(ValueError, match="weight planes must be uint8"):
        tf(imgs, labs, 11, weights=[l[:-1] for l in labs])
    with pytest.raises(ValueError, match="weight planes for"):
        tf(imgs, labs, 11, weights=labs[:-1])


# ------------------------------------------------------------------------------------------------- the pseudo-label weight
@pytest.mark.parametrize("r", [0, 1, 4])
@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16])
def test_pseudo_reference_weight(r, dtype):
    from ifseg_amd.predict import conf_bin, pseudo_label_reference
    n, H, W = 6, 33, 65
    g = torch.Generator().manual_seed(r)
    lab = torch.randint(0, n, (H // 16 + 1, W // 32 + 1), generator=g).repeat_interleave(16, 0).repeat_interleave(32, 1)[:H, :W].clone()
    lab[0, :3] = 255 if dtype == torch.uint8 else -1
    lab = lab.to(dtype)
    conf = torch.rand(H, W, generator=g)
    conf.view(-1)[:8] = torch.tensor([0.0, 1.0, float("nan"), float("inf"), float("-inf"), 1.7, -0.3, 255 / 256])
    conf[8, 14:18] = 0.001                                                   # bin 0, inside a block: away from every edge
    thr = torch.tensor([0, 256, 128, 0, 30, 0], dtype=torch.int32)
    thr[int(lab[8, 16])] = 0
    out, kept, wt = pseudo_label_reference(lab, conf, thr, n, r, weight=True)
    out2, kept2 = pseudo_label_reference(lab, conf, thr, n, r)
    assert torch.equal(out, out2) and torch.equal(kept, kept2)
    assert wt.dtype == torch.uint8 and wt.shape == out.shape
    assert torch.equal(wt == 0, out == 255)
    keep = out != 255
    assert torch.equal(wt[keep].long(), conf_bin(conf)[keep].clamp_min(1))
    assert bool(keep.any()) and bool((~keep).any())
    assert bool(((conf_bin(conf) == 0) & keep).any()) and int(wt[keep].min()) == 1   # a kept pixel of bin 0 weighs 1


# ------------------------------------------------------------------------------------------------- surface
def test_header_declares_the_entry_points_and_the_abi_stays():
    hdr = open(os.path.join(ROOT, "include", "ifseg_hip.h")).read()
    names = set(re.findall(r"\bint\s+(ifseg_\w+)\s*\(", hdr))
    assert {"ifseg_seg_loss_tiles_weighted", "ifseg_train_load_plane", "ifseg_seg_pseudo_weighted"} <= names
    assert {"ifseg_seg_loss_tiles", "ifseg_seg_loss_gather", "ifseg_seg_pseudo", "ifseg_train_load"} <= names
    assert int(re.search(r"#define IFSEG_ABI_VERSION (\d+)", hdr).group(1)) == 21
    from ifseg_amd import hip
    assert hip.ABI_VERSION == 21
    assert callable(hip.seg_loss_weighted) and callable(hip.train_load_plane)


def test_seg_loss_weighted_schema():
    import ifseg_amd.ops  # noqa: F401
    s = str(torch.ops.ifseg.seg_loss_weighted.default._schema)
    assert s == ("ifseg::seg_loss_weighted(Tensor logits, Tensor target, Tensor? pixel_weight, Tensor? class_weight, SymInt hp, "
                 "SymInt wp, SymInt H, SymInt W, SymInt seg_id_offset, float label_smoothing, bool norm_pixels) -> "
                 "(Tensor, Tensor, Tensor, Tensor)")
    assert str(torch.ops.ifseg.seg_loss.default._schema) == (
        "ifseg::seg_loss(Tensor logits, Tensor target, SymInt hp, SymInt wp, SymInt H, SymInt W, "
        "SymInt seg_id_offset, float label_smoothing) -> (Tensor, Tensor, Tensor, Tensor)")


@pytest.mark.parametrize("nseg,B,hp,wp", [(15, 2, 8, 8), (150, 1, 4, 6)])
def test_seg_loss_weighted_fake_shapes(nseg, B, hp, wp):
    from torch._subclasses.fake_tensor import FakeTensorMode
    from ifseg_amd import ops
    BF, F32 = torch.bfloat16, torch.float32
    H, W, npad = 16 * hp, 16 * wp, (nseg + 7) // 8 * 8
    meta = lambda t: (tuple(t.shape), t.dtype)
    with FakeTensorMode():
        e = lambda *shape, dtype=BF: torch.empty(*shape, dtype=dtype, device="cuda")
        logits, target = e(B, hp * wp + 1, nseg), e(B, H * W + 1, dtype=torch.int64)
        pw, cw = e(B, H * W, dtype=torch.uint8), e(nseg, dtype=F32)
        for a, b in ((pw, cw), (None, cw), (pw, None), (None, None)):
            loss, stats, dl, bad = ops.seg_loss_weighted(logits, target, a, b, hp, wp, H, W, 1000, 0.1, a is None)
            assert meta(loss) == ((), F32) and meta(stats) == ((2 + 3 * nseg,), F32)
            assert meta(dl) == ((B, hp * wp + 1, npad), BF) and meta(bad) == ((1,), torch.int32)
        assert meta(ops.seg_loss_bwd(e((), dtype=F32), dl, nseg)) == ((B, hp * wp + 1, nseg), BF)
        for args, what in (((e(B, H * W, dtype=torch.int32), cw), "pixel_weight must be uint8"),
                           ((e(B, H * W + 1, dtype=torch.uint8), cw), "pixel_weight must be uint8"),
                           ((pw, e(nseg + 1, dtype=F32)), "class_weight must be fp32"),
                           ((pw, e(nseg, dtype=torch.float64)), "class_weight must be fp32")):
            with pytest.raises(Exception, match=what):
                ops.seg_loss_weighted(logits, target, *args, hp, wp, H, W, 1000, 0.0, False)
        with pytest.raises(Exception, match="label_smoothing must lie"):
            ops.seg_loss_weighted(logits, target, pw, cw, hp, wp, H, W, 1000, -0.1, False)


def test_pseudo_label_result_keeps_its_four_positional_fields():
    from ifseg_amd.predict import PseudoLabelResult
    a, b, c, d, e = (torch.zeros(1) for _ in range(5))
    r = PseudoLabelResult(a, b, c, d)
    assert r.weight is None and r.kept is d and PseudoLabelResult._fields[-1] == "weight"
    assert PseudoLabelResult(a, b, c, d, e).weight is e


def test_refusals_come_before_any_launch():
    """every one is a ValueError raised from Python on CPU tensors: nothing was launched"""
    from ifseg_amd.criterions.seg_criterion import weighted_loss_reference
    n = 6
    net_output, sample, q, _ = _torch_inputs(n)
    s, t = torch.randn(2, 12, n), torch.randint(SEG0, SEG0 + n, (2, 13))
    for bad in ([1.0, -0.5, 1, 1, 1, 1], [1.0, float("nan"), 1, 1, 1, 1], [1.0, float("inf"), 1, 1, 1, 1], [1.0] * (n + 1)):
        with pytest.raises(ValueError, match="class_weight"):
            _crit(n, class_weight=bad)
        with pytest.raises(ValueError, match="class_weight"):
            weighted_loss_reference(s, t, SEG0, n, class_weight=torch.tensor(bad))
    with pytest.raises(ValueError, match="weight_norm"):
        _crit(n, weight_norm="mean")
    with pytest.raises(ValueError, match="weight_norm"):
        weighted_loss_reference(s, t, SEG0, n, weight_norm="sum")
    crit = _crit(n, class_weight=[1.0] * n)
    for plane in (q.float(), q.int(), q[:, :-1], q[:1], q.view(2, 32, -1)):
        for fn in (crit.compute_loss_torch, crit.compute_loss):
            with pytest.raises(ValueError, match="pixel_weight must be uint8"):
                fn(None, net_output, dict(sample, target_weight=plane), 0)
    with pytest.raises(ValueError, match="pixel_weight must be uint8"):
        weighted_loss_reference(s, t, SEG0, n, pixel_weight=torch.zeros(2, 13, dtype=torch.uint8))
