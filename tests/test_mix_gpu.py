"""GPU: the batch mix (csrc/mix.hip) against its specification, bit for bit -- `hip.mix_draw` against
`augment.mix_draw_reference`, `hip.mix_apply` against `augment.mix_apply_reference` (images through an integer view), in place
and twice, the refusals, the dispatcher ops, `BatchMix` on both devices, and `task.dacs_sample` through one training step on
the segofa_tiny fixture."""
import itertools

import pytest
import torch

import _mix_cases as MC
import _predict_cases as PC
from ifseg_amd import augment as A
from test_predict_views_gpu import e2e  # noqa: F401  (the segofa_tiny fixture with its three raw shapes)

pytestmark = pytest.mark.gpu

SEG0 = MC.SEG0


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ifseg_amd.ops  # noqa: F401
    return torch.device("cuda:0")


def _same(got, want):
    """device results against the specification's: images as integers, the plane present or absent in both"""
    gi, gt, gw = got
    wi, wt, ww = want
    ok = torch.equal(MC.as_int(gi).cpu(), MC.as_int(wi)) and gi.dtype == wi.dtype and torch.equal(gt.cpu(), wt)
    return ok and ((gw is None and ww is None) or (gw is not None and ww is not None and torch.equal(gw.cpu(), ww)))


def _draw_cases():
    """(name, nseg, target): every shape with every class count, the word boundary, no class at all, the full map"""
    cases = [("B%d P%d nseg %d" % (B, P, nseg), nseg, MC.block_target(B, P, nseg)) for (B, P), nseg in itertools.product(MC.SHAPES, MC.NSEGS)]
    cases.append(("classes 31 and 32, 'unknown' only, impostor and -1", 33, MC.special_target()))
    cases.append(("255 distinct classes", 255, MC.full_target()))
    cases.append(("one class", 255, MC.class_target([254])))
    return cases


# ------------------------------------------------------------------------------------------------- draw
@pytest.mark.parametrize("mask", ["class", "box"])
def test_draw_is_the_specification(mask):
    from ifseg_amd import hip
    dev = _dev()
    wrong = []
    for k, (name, nseg, tgt) in enumerate(_draw_cases()):
        first = 3 + 17 * k
        want = A.mix_draw_reference(tgt, nseg, SEG0, MC.SEED, first, mask)
        got = hip.mix_draw(tgt.to(dev), nseg, SEG0, MC.SEED, first, mask)
        assert got.dtype == torch.int32 and tuple(got.shape) == tuple(want.shape) and got.is_cuda
        again = hip.mix_draw(tgt.to(dev), nseg, SEG0, MC.SEED, first, mask, out=torch.full_like(got, -7))
        if not (torch.equal(got.cpu(), want) and torch.equal(again, got)):
            wrong.append((name, got.cpu().tolist(), want.tolist()))
    assert not wrong, wrong[:2]
    # the ordinal range ends at 2**32, and the seed is taken modulo 2**64
    tgt = MC.block_target(2, 16, 15)
    for seed, first in ((2 ** 64 - 3, 2 ** 32 - 2), (-1, 2 ** 31)):
        assert torch.equal(hip.mix_draw(tgt.to(dev), 15, SEG0, seed, first, mask).cpu(), A.mix_draw_reference(tgt, 15, SEG0, seed, first, mask))


# ------------------------------------------------------------------------------------------------- apply
def _records(st, nseg, B, P):
    """the three kinds of record: drawn classes, a drawn box, a caller's own with both (a box reaching outside the image)"""
    cls = A.mix_draw_reference(st, nseg, SEG0, MC.SEED, 2)
    return {"class": cls, "box": A.mix_draw_reference(st, nseg, SEG0, MC.SEED, 2, "box"), "both": MC.both_record(B, P, cls)}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,P", MC.SHAPES)
def test_apply_is_the_specification(B, P, dtype):
    from ifseg_amd import hip
    dev = _dev()
    wrong, ran = [], 0
    for nseg in (15, 255):
        st, dt = MC.block_target(B, P, nseg, 0), MC.block_target(B, P, nseg, 1)
        si, di = MC.images(B, P, dtype, 0), MC.images(B, P, dtype, 1)
        sw, dw = MC.weights(B, P, 0), MC.weights(B, P, 1)
        d = lambda t: None if t is None else t.to(dev)
        for (kind, rec), (a, b) in itertools.product(_records(st, nseg, B, P).items(), ((None, None), (sw, None), (None, dw), (sw, dw))):
            want = A.mix_apply_reference(rec, (si, st, a), (di, dt, b), nseg, SEG0)
            args = (d(rec), d(si), d(st), d(di), d(dt), nseg, SEG0)
            got = hip.mix_apply(*args, src_weight=d(a), dst_weight=d(b))
            twice = hip.mix_apply(*args, src_weight=d(a), dst_weight=d(b))
            # in place: out is the destination itself (a plane the destination lacks is a fresh one)
            di2, dt2, dw2 = d(di).clone(), d(dt).clone(), (d(b).clone() if b is not None else None)
            out_w = dw2 if dw2 is not None else (torch.empty(B, P * P, dtype=torch.uint8, device=dev) if a is not None else None)
            inplace = hip.mix_apply(d(rec), d(si), d(st), di2, dt2, nseg, SEG0, src_weight=d(a), dst_weight=dw2, out=(di2, dt2, out_w))
            ran += 1
            if not (_same(got, want) and _same(twice, want) and _same(inplace, want) and inplace[0] is di2 and inplace[1] is dt2):
                wrong.append((nseg, kind, a is not None, b is not None))
    assert ran == 24 and not wrong, wrong


def test_apply_special_targets():
    """no class at all, the 64-bit impostor, the word boundary and all 255 classes: nothing but chosen classes is pasted"""
    from ifseg_amd import hip
    dev = _dev()
    for nseg, st in ((33, MC.special_target()), (255, MC.full_target())):
        B, P = st.shape[0], 16
        dt = MC.block_target(B, P, 15, 1)
        si, di = MC.images(B, P, torch.float32, 0), MC.images(B, P, torch.float32, 1)
        rec = A.mix_draw_reference(st, nseg, SEG0, MC.SEED, 0)
        want = A.mix_apply_reference(rec, (si, st), (di, dt), nseg, SEG0)
        got = hip.mix_apply(rec.to(dev), si.to(dev), st.to(dev), di.to(dev), dt.to(dev), nseg, SEG0)
        assert _same(got, want) and got[2] is None
        wild = rec.clone()
        wild[:, 0] |= -(1 << 3) if nseg == 33 else 0                                # bit 3: the impostor's class in 32 bits
        sel = A.mix_selection(wild, st, nseg, SEG0)
        if nseg == 33:
            assert not bool(sel[1:].any()) and _same(hip.mix_apply(wild.to(dev), si.to(dev), st.to(dev), di.to(dev), dt.to(dev), nseg, SEG0),
                                                     A.mix_apply_reference(wild, (si, st), (di, dt), nseg, SEG0))


# ------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    from ifseg_amd import hip
    dev = _dev()
    B, P, nseg = 2, 16, 15
    st, dt = MC.block_target(B, P, nseg, 0).to(dev), MC.block_target(B, P, nseg, 1).to(dev)
    si, di = MC.images(B, P, torch.float32, 0).to(dev), MC.images(B, P, torch.float32, 1).to(dev)
    rec = hip.mix_draw(st, nseg, SEG0, 1, 0)
    bad_p = torch.zeros(B, 24 * 24 + 1, dtype=torch.int64, device=dev)
    calls = [lambda: hip.mix_draw(st, 0, SEG0, 1, 0), lambda: hip.mix_draw(st, 256, SEG0, 1, 0), lambda: hip.mix_draw(bad_p, nseg, SEG0, 1, 0),
             lambda: hip.mix_draw(st, nseg, SEG0, 1, 0, mask="circle"), lambda: hip.mix_draw(st, nseg, SEG0, 1, 2 ** 32 - 1),
             lambda: hip.mix_apply(rec, si.bfloat16(), st, di, dt, nseg, SEG0),                          # dtype mismatch
             lambda: hip.mix_apply(rec, si, st, di, dt, 0, SEG0), lambda: hip.mix_apply(rec, si, st, di, dt, 256, SEG0),
             lambda: hip.mix_apply(rec[:1], si[:1], st[:1], di, dt, nseg, SEG0),                         # unequal B
             lambda: hip.mix_apply(rec, torch.zeros(B, 3, 24, 24, device=dev), bad_p, torch.zeros(B, 3, 24, 24, device=dev), bad_p, nseg, SEG0),
             lambda: hip.mix_apply(rec, si, st, di, dt, nseg, SEG0, out=(si, torch.empty_like(dt), None)),   # out over the source
             lambda: hip.mix_apply(rec, si, st, di, dt, nseg, SEG0, out=(torch.empty_like(di), st, None)),
             lambda: hip.mix_apply(rec, si, st, di, dt, nseg, SEG0, out=(torch.empty_like(di), torch.empty_like(dt), torch.empty(B, P * P, dtype=torch.uint8, device=dev)))]
    for k, call in enumerate(calls):
        with pytest.raises(AssertionError):
            call()
            pytest.fail("call %d was not refused" % k)
    # the entry point itself refuses an output laid over the source (the binding's check aside): nothing is launched
    import ctypes
    p, ll = (lambda t: ctypes.c_void_p(t.data_ptr())), ctypes.c_longlong
    oi, ot = torch.empty_like(di), torch.empty_like(dt)
    entry = lambda out_i, out_t: hip.lib().ifseg_mix_apply(p(rec), p(si), p(st), None, p(di), p(dt), None, B, P, nseg, ll(SEG0), 4,
                                                           p(out_i), p(out_t), None, None)
    assert entry(si, ot) == -3 and entry(oi, st) == -3 and entry(oi, dt[1:]) == -3
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- ops and BatchMix
def test_ops_are_the_bindings():
    from ifseg_amd import hip
    dev = _dev()
    B, P, nseg = 3, 48, 15
    st, dt = MC.block_target(B, P, nseg, 0).to(dev), MC.block_target(B, P, nseg, 1).to(dev)
    si, di = MC.images(B, P, torch.bfloat16, 0).to(dev), MC.images(B, P, torch.bfloat16, 1).to(dev)
    sw = MC.weights(B, P, 0).to(dev)
    for mask in ("class", "box"):
        rec = torch.ops.ifseg.mix_draw(st, nseg, SEG0, MC.SEED, 9, mask)
        assert torch.equal(rec, hip.mix_draw(st, nseg, SEG0, MC.SEED, 9, mask))
        want = hip.mix_apply(rec, si, st, di, dt, nseg, SEG0, src_weight=sw)
        img, tgt, wgt = torch.ops.ifseg.mix_apply(rec, si, st, sw, di, dt, None, nseg, SEG0)
        assert torch.equal(MC.as_int(img), MC.as_int(want[0])) and torch.equal(tgt, want[1]) and torch.equal(wgt, want[2])
        assert torch.ops.ifseg.mix_apply(rec, si, st, None, di, dt, None, nseg, SEG0)[2].numel() == 0
    # non-contiguous inputs are copied
    wide = torch.zeros(B, 3, P, 2 * P, dtype=torch.bfloat16, device=dev)
    wide[..., ::2] = si
    img2 = torch.ops.ifseg.mix_apply(rec, wide[..., ::2], st, sw, di, dt, None, nseg, SEG0)[0]
    assert torch.equal(MC.as_int(img2), MC.as_int(img))
    with pytest.raises(ValueError):
        torch.ops.ifseg.mix_apply(rec, si.float(), st, None, di, dt, None, nseg, SEG0)


@pytest.mark.parametrize("mask", ["class", "box"])
def test_batch_mix_on_both_devices(mask):
    dev = _dev()
    B, P, nseg = 3, 48, 33
    src = (MC.images(B, P, torch.float32, 0), MC.block_target(B, P, nseg, 0), MC.weights(B, P, 0))
    dst = (MC.images(B, P, torch.float32, 1), MC.block_target(B, P, nseg, 1), MC.weights(B, P, 1))
    cpu, gpu = (A.BatchMix(P, nseg, SEG0, seed=MC.SEED, device=d, mask=mask) for d in ("cpu", dev))
    assert torch.equal(gpu.draw(src, 12).cpu(), cpu.draw(src, 12))
    got = gpu(src, dst, 12)
    assert all(t.is_cuda for t in got) and _same(got, cpu(src, dst, 12))


# ------------------------------------------------------------------------------------------------- end to end
def test_dacs_sample_through_one_training_step(e2e):  # noqa: F811
    """segofa_tiny at P = 128, as test_confidence_weighted_self_training_step: `dacs_sample`'s three tensors are
    `mix_apply_reference` of `train_sample` and `self_train_sample` at the stated ordinals, pasted pixels weigh 255, and one
    training step on the sample gives a finite loss and moves the weights"""
    from ifseg_amd.criterions import SegCriterion
    from ifseg_amd.tasks.mm_tasks import SegmentationTask
    from ifseg_amd.trainer import Trainer
    from test_weighted_loss_gpu import _student
    dev = _dev()
    _, raw, ocfg, _ = e2e
    _, sd, _, _ = PC.e2e_fixture()
    P, n = ocfg.patch_image_size, ocfg.num_seg_tokens
    task = SegmentationTask(num_seg_tokens=n, patch_image_size=P, n_base_vocab=ocfg.vocab_size - 1, category_token_ids=PC.E2E_NAMES)
    task.prompt_ids = PC.E2E_PROMPT
    task.build_train_transform(dev, seed=6, ratio_range=(1, 1))
    m = _student(ocfg, sd, dev)
    kw = dict(prompt_ids=PC.E2E_PROMPT, keep=0.5, boundary=1)
    # labelled photographs: the raw images with label maps of blocks in the label-PNG convention (0 and 255: 'unknown')
    g = torch.Generator().manual_seed(3)
    labels = [torch.randint(0, n + 1, ((h + 15) // 16, (w + 15) // 16), generator=g).repeat_interleave(16, 0).repeat_interleave(16, 1)[:h, :w]
              .to(torch.uint8).contiguous().to(dev) for h, w in (tuple(r.shape[:2]) for r in raw)]
    unlabeled = raw[::-1]
    first = 4
    for mask in ("class", "box"):
        s = task.dacs_sample(m, raw, labels, unlabeled, first, mask=mask, **kw)
        source = task.train_sample(raw, labels, first)
        target = task.self_train_sample(m, unlabeled, first + 2 ** 31, confidence_weight=True, **kw)
        rec = A.mix_draw_reference(source["target"].cpu(), n, task.seg_id_offset, 6, first, mask)
        img, tgt, wgt = A.mix_apply_reference(rec, source, target, n, task.seg_id_offset)
        assert s["net_input"]["patch_images"].is_cuda and set(s) == set(target)
        assert torch.equal(MC.as_int(s["net_input"]["patch_images"]).cpu(), MC.as_int(img))
        assert torch.equal(s["target"].cpu(), tgt) and torch.equal(s["target_weight"].cpu(), wgt)
        sel = A.mix_selection(rec, source["target"].cpu(), n, task.seg_id_offset)
        assert bool(sel.any()) and bool((~sel).any()) and bool((wgt[sel] == 255).all())
        assert torch.equal(wgt[~sel], target["target_weight"].cpu()[~sel])
        assert torch.equal(s["net_input"]["src_tokens"], target["net_input"]["src_tokens"])
    tr = Trainer(m, SegCriterion(task, unsupervised_segmentation=False, init_seg_with_text=False), task, device=dev)
    p_before = tr.p32.clone()
    loss = float(tr.train_step([s])[0]["loss"])
    tr.check_overflow(wait=True)
    torch.cuda.synchronize()
    assert loss == loss and abs(loss) != float("inf") and loss > 0.0
    assert not torch.equal(tr.p32, p_before)
