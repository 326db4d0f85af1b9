"""GPU: the strong augmentation (csrc/strong.hip) against its specification, bit for bit -- `hip.strong_draw` against
`augment.strong_draw_reference`, `hip.strong_apply` against `augment.strong_apply_reference` (images through an integer view),
into `out=` and twice, the refusals, the dispatcher ops, `StrongAugment` on both devices, and `task.dacs_sample(strong=True)`
through one training step on the segofa_tiny fixture."""
import itertools

import pytest
import torch

import _predict_cases as PC
import _strong_cases as SC
from ifseg_amd import augment as A
from test_predict_views_gpu import e2e  # noqa: F401  (the segofa_tiny fixture with its three raw shapes)

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ifseg_amd.ops  # noqa: F401
    return torch.device("cuda:0")


def _same(got, want):
    return got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape) and torch.equal(SC.as_int(got).cpu(), SC.as_int(want))


# ------------------------------------------------------------------------------------------------- draw
def test_draw_is_the_specification():
    from ifseg_amd import hip
    dev = _dev()
    wrong, ran = [], 0
    for B, seed, tail, (jp, bp) in itertools.product((1, 3, 8), (5, 2 ** 64 - 3, -1), (False, True), ((0, 0), (205, 128), (256, 256))):
        first = 2 ** 32 - B if tail else 0
        want = A.strong_draw_reference(B, seed, first, jp, bp)
        got = hip.strong_draw(B, seed, first, jp, bp, device=dev)
        assert got.dtype == torch.int32 and tuple(got.shape) == (B, 16) and got.is_cuda
        buf = torch.full((B, 16), -7, dtype=torch.int32, device=dev)
        again = hip.strong_draw(B, seed, first, jp, bp, out=buf)
        ran += 1
        if not (torch.equal(got.cpu(), want) and again is buf and torch.equal(again, got)):
            wrong.append((B, seed, first, jp, bp, got.cpu().tolist(), want.tolist()))
    assert ran == 54 and not wrong, wrong[:2]
    assert torch.equal(hip.strong_draw(8, 5, 0), hip.strong_draw(8, 5, 0)) and hip.strong_draw(8, 5, 0).device == dev   # the defaults


# ------------------------------------------------------------------------------------------------- apply
@pytest.mark.parametrize("dtype", SC.DTYPES)
@pytest.mark.parametrize("B,P", SC.SHAPES)
def test_apply_is_the_specification(B, P, dtype):
    from ifseg_amd import hip
    dev = _dev()
    wrong, ran = [], 0
    for kind, (name, rec) in itertools.product(SC.KINDS, SC.record_kinds(B).items()):
        img = SC.images(kind, B, P, dtype)
        want = A.strong_apply_reference(rec, img)
        got = hip.strong_apply(rec.to(dev), img.to(dev))
        twice = hip.strong_apply(rec.to(dev), img.to(dev))
        buf = torch.zeros(B, 3, P, P, dtype=dtype, device=dev)
        into = hip.strong_apply(rec.to(dev), img.to(dev), out=buf)
        ran += 1
        if not (_same(got, want) and _same(twice, want) and into is buf and _same(into, want)):
            wrong.append((kind, name, int((SC.as_int(got).cpu() != SC.as_int(want)).sum())))
        if name == "invalid":
            nan = torch.isnan(want.float()).flatten(1).all(1)
            assert bool(nan[:max(B - 1, 1)].all()) and (B == 1 or not bool(torch.isnan(want[B - 1].float()).any()))
    assert ran == 26 and not wrong, wrong


def test_apply_statistics_and_channel_order():
    """the ImageNet statistics in bf16 (the thinnest margin of the recovery), and reversed planes"""
    from ifseg_amd import hip
    dev = _dev()
    B, P = 3, 48
    rec = SC.drawn(B, True, True)[1]
    for dtype, stats, reverse in ((torch.bfloat16, "imagenet", False), (torch.float32, "half", True), (torch.bfloat16, "imagenet", True)):
        mean, std = SC.STATS[stats]
        img = SC.level_images(B, P, dtype, stats, reverse)
        for r in (rec, SC.records_of(B, SC.ALL_OFF)):
            want = A.strong_apply_reference(r, img, mean, std, reverse)
            assert _same(hip.strong_apply(r.to(dev), img.to(dev), mean, std, reverse), want), (dtype, stats, reverse)
        assert _same(hip.strong_apply(SC.records_of(B, SC.ALL_OFF).to(dev), img.to(dev), mean, std, reverse), img)
        lut = A.normalisation_table(mean, std).to(dev)
        assert _same(hip.strong_apply(rec.to(dev), img.to(dev), reverse_channels=reverse, lut=lut), A.strong_apply_reference(rec, img, mean, std, reverse))


def test_every_value_finds_its_level():
    """every table value, the neighbours of every midpoint and the specials, in both dtypes and both statistics, through the
    kernel with everything off: the output is the table at the literally counted level"""
    from ifseg_amd import hip
    dev = _dev()
    for dtype, stats in itertools.product(SC.DTYPES, ("half", "imagenet")):
        mean, std = SC.STATS[stats]
        x, count = SC.literal_levels(dtype, stats)
        P = 48
        assert x.shape[1] <= P * P
        img = A.normalisation_table(mean, std)[:, :1].to(dtype).expand(3, P * P).clone()
        img[:, :x.shape[1]] = x
        img = img.reshape(1, 3, P, P)
        got = hip.strong_apply(SC.records_of(1, SC.ALL_OFF).to(dev), img.to(dev), mean, std)
        lut = A.normalisation_table(mean, std)
        want = torch.stack([lut[c][count[c]] for c in range(3)]).to(dtype)
        assert torch.equal(SC.as_int(got).cpu().reshape(3, -1)[:, :x.shape[1]], SC.as_int(want)), (dtype, stats)


# ------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    from ifseg_amd import hip
    dev = _dev()
    B, P = 2, 16
    img = SC.level_images(B, P, torch.float32).to(dev)
    rec = hip.strong_draw(B, 1, 0, device=dev)
    wide = torch.zeros(B, 3, P, 2 * P, device=dev)
    both = torch.zeros(2 * B, 3, P, P, device=dev)
    calls = [lambda: hip.strong_draw(0, 1, 0, device=dev), lambda: hip.strong_draw(B, 1, -1, device=dev),
             lambda: hip.strong_draw(B, 1, 2 ** 32 - 1, device=dev), lambda: hip.strong_draw(B, 1, 0, 257, 128, device=dev),
             lambda: hip.strong_draw(B, 1, 0, 205, -1, device=dev), lambda: hip.strong_draw(B, 1, 0, out=torch.zeros(B, 16, device=dev)),
             lambda: hip.strong_draw(B, 1, 0, out=torch.zeros(B + 1, 16, dtype=torch.int32, device=dev)),
             lambda: hip.strong_apply(rec, img.double()), lambda: hip.strong_apply(rec, img.cpu()), lambda: hip.strong_apply(rec[:1], img),
             lambda: hip.strong_apply(rec.long(), img), lambda: hip.strong_apply(rec, wide[..., ::2]),
             lambda: hip.strong_apply(rec, torch.zeros(B, 3, 24, 24, device=dev)), lambda: hip.strong_apply(rec, img, std=(0.5, 0.0, 0.5)),
             lambda: hip.strong_apply(rec, img, out=img), lambda: hip.strong_apply(rec, img, out=torch.empty_like(img).bfloat16()),
             lambda: hip.strong_apply(rec, img, out=torch.empty(1, 3, P, P, device=dev)), lambda: hip.strong_apply(rec, both[:B], out=both[1:B + 1]),
             lambda: hip.strong_apply(rec, img, lut=torch.zeros(3, 256, dtype=torch.float64, device=dev))]
    for k, call in enumerate(calls):
        with pytest.raises(AssertionError):
            call()
            pytest.fail("call %d was not refused" % k)
    # the entry point itself refuses an output laid over the images (the binding's check aside), and P = 24: nothing is launched
    import ctypes
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    lut = A.normalisation_table().to(dev)
    entry = lambda images, out, P=P: hip.lib().ifseg_strong_apply(p(rec), p(images), B, P, 4, p(lut), 0, p(out), None)
    assert entry(img, img) == -3 and entry(both, both[1:]) == -3 and entry(both[1:], both) == -3
    assert entry(img, torch.empty_like(img), P=24) == -2
    assert entry(img, torch.empty_like(img)) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- ops and StrongAugment
def test_ops_are_the_bindings():
    from ifseg_amd import hip
    dev = _dev()
    B, P = 3, 48
    first = SC.drawn(B, True, True)[0]
    rec = torch.ops.ifseg.strong_draw(B, SC.SEED, first, 205, 128, dev)
    assert torch.equal(rec, hip.strong_draw(B, SC.SEED, first, device=dev)) and torch.equal(rec.cpu(), SC.drawn(B, True, True)[1])
    for dtype in SC.DTYPES:
        img = SC.level_images(B, P, dtype).to(dev)
        want = hip.strong_apply(rec, img)
        got = torch.ops.ifseg.strong_apply(rec, img, SC.HALF, SC.HALF, False)
        assert torch.equal(SC.as_int(got), SC.as_int(want)) and not torch.equal(SC.as_int(got), SC.as_int(img))
        # non-contiguous inputs are copied
        wide = torch.zeros(B, 3, P, 2 * P, dtype=dtype, device=dev)
        wide[..., ::2] = img
        assert torch.equal(SC.as_int(torch.ops.ifseg.strong_apply(rec, wide[..., ::2], SC.HALF, SC.HALF, False)), SC.as_int(want))
        recs = torch.zeros(B, 32, dtype=torch.int32, device=dev)
        recs[:, ::2] = rec
        assert torch.equal(SC.as_int(torch.ops.ifseg.strong_apply(recs[:, ::2], img, SC.HALF, SC.HALF, False)), SC.as_int(want))
    with pytest.raises(ValueError):
        torch.ops.ifseg.strong_apply(rec, img.half(), SC.HALF, SC.HALF, False)
    with pytest.raises(ValueError):
        torch.ops.ifseg.strong_apply(rec, img, SC.HALF, (0.5, 0.5, 0.0), False)


def test_strong_augment_on_both_devices():
    dev = _dev()
    B, P = 3, 48
    for dtype, stats, reverse in ((torch.float32, "half", False), (torch.bfloat16, "imagenet", True)):
        mean, std = SC.STATS[stats]
        img = SC.level_images(B, P, dtype, stats, reverse)
        cpu, gpu = (A.StrongAugment(P, mean, std, seed=SC.SEED, device=d, reverse_channels=reverse) for d in ("cpu", dev))
        first = SC.drawn(B, True, True)[0]
        assert torch.equal(gpu.draw(B, first).cpu(), cpu.draw(B, first))
        got = gpu(img, first)
        assert got.is_cuda and _same(got, cpu(img, first))
        buf = torch.empty(B, 3, P, P, dtype=dtype, device=dev)
        assert gpu.apply(cpu.draw(B, first), img, out=buf) is buf and _same(buf, cpu(img, first))


# ------------------------------------------------------------------------------------------------- end to end
def test_dacs_sample_strong_through_one_training_step(e2e):  # noqa: F811
    """segofa_tiny at P = 128, set up as test_dacs_sample_through_one_training_step: the images of `dacs_sample(strong=True)`
    are the specification applied to those of `strong=False`, everything else is `strong=False`'s bit for bit, and one
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
    g = torch.Generator().manual_seed(3)
    labels = [torch.randint(0, n + 1, ((h + 15) // 16, (w + 15) // 16), generator=g).repeat_interleave(16, 0).repeat_interleave(16, 1)[:h, :w]
              .to(torch.uint8).contiguous().to(dev) for h, w in (tuple(r.shape[:2]) for r in raw)]
    unlabeled = raw[::-1]
    B = len(raw)
    first = SC.drawn(B, True, True, seed=6)[0]
    plain = task.dacs_sample(m, raw, labels, unlabeled, first, **kw)
    s = task.dacs_sample(m, raw, labels, unlabeled, first, strong=True, **kw)
    rec = A.strong_draw_reference(B, 6, first)
    want = A.strong_apply_reference(rec, plain["net_input"]["patch_images"].cpu())
    got = s["net_input"]["patch_images"]
    assert got.is_cuda and _same(got, want) and not torch.equal(SC.as_int(got), SC.as_int(plain["net_input"]["patch_images"]))
    assert set(s) == set(plain) and set(s["net_input"]) == set(plain["net_input"])
    assert torch.equal(s["target"], plain["target"]) and torch.equal(s["target_weight"], plain["target_weight"])
    assert torch.equal(s["net_input"]["src_tokens"], plain["net_input"]["src_tokens"])
    tr = Trainer(m, SegCriterion(task, unsupervised_segmentation=False, init_seg_with_text=False), task, device=dev)
    p_before = tr.p32.clone()
    loss = float(tr.train_step([s])[0]["loss"])
    tr.check_overflow(wait=True)
    torch.cuda.synchronize()
    assert loss == loss and abs(loss) != float("inf") and loss > 0.0
    assert not torch.equal(tr.p32, p_before)
