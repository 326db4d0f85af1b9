"""GPU: the image-free sample kernels (csrc/imfree.hip) against the CPU specification in ifseg_amd/artificial.py, bit for
bit, and the generated sample through the model, the criterion and the trainer."""
import pytest
import torch

import segofa_ref as O

from ifseg_amd.artificial import ArtificialImageSampler

pytestmark = pytest.mark.gpu

BOS, PAD, EOS = 0, 1, 2
SEG0 = 1000
KEYS = ("ids", "ends", "prev_output_tokens", "text2seg_target")


def _names(nseg, lens, seed=0, hi=SEG0 - 1):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(4, hi, (lens[i % len(lens)],), generator=g) for i in range(nseg + 1)]


def _pair(names, hp, l, r, seed=1, seg0=SEG0):
    mk = lambda dev: ArtificialImageSampler(names, seg0, hp, hp, l, r, seed=seed, device=dev)
    return mk("cpu"), mk("cuda:0")


def _assert_same(got, want, B, P, Lmax):
    for k in KEYS:
        assert got[k].dtype == torch.long and got[k].shape == want[k].shape, k
        assert torch.equal(got[k].cpu(), want[k]), k
    # everything behind the last bag of a row is padding
    ids, last = got["ids"].cpu(), got["ends"].cpu().view(B, P)[:, -1]
    assert ids.shape == (B, P * Lmax)
    for b in range(B):
        assert (ids[b, int(last[b]):] == PAD).all(), b


def _supplied(maps, max_side):
    shapes = torch.tensor([list(m.shape) for m in maps], dtype=torch.int32)
    coarse = torch.zeros(len(maps), max_side * max_side, dtype=torch.int32)
    for b, m in enumerate(maps):
        coarse[b, : m.numel()] = m.reshape(-1).int()
    return shapes, coarse


@pytest.mark.parametrize("hp", [2, 32, 40])
def test_drawn_batch_equals_cpu_specification(hp):
    """rand_k-1-33, B = 3 (2 at the 40 x 40 grid): rows of the target start 16-byte aligned and not"""
    B, nseg = (2 if hp == 40 else 3), 150
    cpu, gpu = _pair(_names(nseg, (1, 2, 3, 5)), hp, 1, 33, seed=7)
    for first in (0, 4093):
        s_c, c_c = cpu.draw(B, first)
        s_g, c_g = gpu.draw(B, first)
        assert s_g.dtype == torch.int32 and c_g.dtype == torch.int32
        assert torch.equal(s_g.cpu(), s_c) and torch.equal(c_g.cpu(), c_c)
        _assert_same(gpu.expand(s_g, c_g), cpu.expand(s_c, c_c), B, hp * hp, 5)


def test_supplied_84x84_map_on_the_40x40_grid_uses_the_fp32_index_rule():
    """in = 84, out = 40 / 640: where floorf(dst * (in / out)) and (dst * in) / out differ"""
    nseg = 171
    cpu, gpu = _pair(_names(nseg, (1, 2, 3)), 40, 84, 85)
    g = torch.Generator().manual_seed(5)
    maps = [torch.randint(0, nseg, (84, 84), generator=g),
            (torch.arange(84 * 84).reshape(84, 84) * 7 + torch.arange(84).reshape(84, 1)) % nseg]
    shapes, coarse = _supplied(maps, 84)
    _assert_same(gpu.expand(shapes.cuda(), coarse.cuda()), cpu.expand(shapes, coarse), 2, 1600, 3)


def test_every_side_length_on_a_small_grid():
    """sample b is (b + 1) x (128 - b): every source size 1..128 goes through the row and the column index once"""
    nseg = 15
    cpu, gpu = _pair(_names(nseg, (1, 2)), 2, 1, 129)
    g = torch.Generator().manual_seed(9)
    maps = [torch.randint(0, nseg, (b + 1, 128 - b), generator=g) for b in range(128)]
    shapes, coarse = _supplied(maps, 128)
    _assert_same(gpu.expand(shapes.cuda(), coarse.cuda()), cpu.expand(shapes, coarse), 128, 4, 2)


@pytest.mark.parametrize("hp", [32, 40])
def test_scan_across_passes_with_full_length_names(hp):
    """P = 1024 / 1600 bags of Lmax = 16 tokens each: the running total crosses the 256-bag passes and fills the row"""
    P, nseg = hp * hp, 15
    cpu, gpu = _pair(_names(nseg, (16,)), hp, 1, 33, seed=3)
    s_c, c_c = cpu.draw(2, 17)
    got, want = gpu.expand(s_c.cuda(), c_c.cuda()), cpu.expand(s_c, c_c)
    _assert_same(got, want, 2, P, 16)
    ends = got["ends"].cpu().view(2, P)
    assert ends[:, -1].tolist() == [P * 16] * 2 and torch.equal(ends[0], torch.arange(1, P + 1) * 16)
    assert (got["ids"] != PAD).all()


def test_batch_with_a_1x1_sample_clamps_and_an_empty_name():
    """a 1 x 1 map, the 'unknown' class with an empty name, and out-of-range shapes / classes / name lengths (clamped)"""
    nseg = 5
    names = _names(nseg, (1, 2, 3))[:nseg] + [torch.zeros(0, dtype=torch.long)]
    cpu, gpu = _pair(names, 4, 1, 33)
    g = torch.Generator().manual_seed(2)
    maps = [torch.randint(0, nseg, (1, 1), generator=g), torch.randint(0, nseg + 1, (5, 9), generator=g),
            torch.randint(0, nseg, (32, 32), generator=g)]
    shapes, coarse = _supplied(maps, 32)
    _assert_same(gpu.expand(shapes.cuda(), coarse.cuda()), cpu.expand(shapes, coarse), 3, 16, 3)
    # hostile inputs: sides outside [1, 32], classes outside [0, nseg], a name length outside [0, Lmax]
    shapes = torch.tensor([[0, 77], [-3, 5], [40, 1]], dtype=torch.int32)
    coarse = torch.randint(-9, 99, (3, 32 * 32), generator=g, dtype=torch.int32)
    for s in (cpu, gpu):
        s.name_len[1], s.name_len[2] = 99, -4
    want = cpu.expand(shapes, coarse)
    _assert_same(gpu.expand(shapes.cuda(), coarse.cuda()), want, 3, 16, 3)
    assert int(want["ends"].max()) <= 16 * 3


def test_no_write_outside_the_output_tensors():
    """every output lives inside a larger buffer between two bands of a sentinel value, at an element offset that makes the
    first target row start off a 16-byte boundary: the bands stay untouched"""
    from ifseg_amd import hip
    dev = torch.device("cuda:0")
    B, hp, nseg, G = 3, 4, 15, 4096
    P, S = hp * hp, 16 * hp
    cpu, gpu = _pair(_names(nseg, (1, 2, 16)), hp, 1, 33, seed=7)

    def banded(n, dtype, off):
        buf = torch.full((G + off + n + G,), -77, dtype=dtype, device=dev)
        return buf, buf[G + off: G + off + n], G + off

    bufs = {"shapes": banded(B * 2, torch.int32, 1), "coarse": banded(B * 1024, torch.int32, 3),
            "ids": banded(B * P * 16, torch.long, 1), "ends": banded(B * P, torch.long, 1),
            "prev_output_tokens": banded(B * (P + 1), torch.long, 0), "text2seg_target": banded(B * (S * S + 1), torch.long, 1)}
    v = {k: b[1] for k, b in bufs.items()}
    assert v["text2seg_target"].data_ptr() % 16 == 8
    shapes, coarse = v["shapes"].view(B, 2), v["coarse"].view(B, 1024)
    hip.imfree_draw(7, 40, B, 1, 33, nseg, shapes, coarse)
    out = {"ids": v["ids"].view(B, P * 16), "ends": v["ends"], "prev_output_tokens": v["prev_output_tokens"].view(B, P + 1),
           "text2seg_target": v["text2seg_target"].view(B, S * S + 1)}
    hip.imfree_expand(shapes, coarse, gpu.name_ids, gpu.name_len, hp, hp, SEG0, BOS, EOS, PAD, out["ids"], out["ends"],
                      out["prev_output_tokens"], out["text2seg_target"])
    torch.cuda.synchronize()
    s_c, c_c = cpu.draw(B, 40)
    assert torch.equal(shapes.cpu(), s_c) and torch.equal(coarse.cpu(), c_c)
    _assert_same(out, cpu.expand(s_c, c_c), B, P, 16)
    for k, (buf, view, lo) in bufs.items():
        assert (buf[:lo] == -77).all() and (buf[lo + view.numel():] == -77).all(), k


def test_limits_are_refused_before_any_launch():
    """IFSEG_ERR_BAD_ARG (-3) / IFSEG_ERR_BAD_SHAPE (-2) from the host side of the entry points"""
    from ifseg_amd import hip
    dev = torch.device("cuda:0")
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)
    i64 = lambda *s: torch.zeros(*s, dtype=torch.long, device=dev)
    for l, r, nseg, first in ((0, 33, 15, 0), (5, 5, 15, 0), (1, 130, 15, 0), (1, 33, 0, 0), (1, 33, 15, -1), (1, 33, 15, 2 ** 32 - 1)):
        with pytest.raises(RuntimeError, match="code -3"):
            hip.imfree_draw(1, first, 2, l, r, nseg, i32(2, 2), i32(2, (r - 1) * (r - 1)))

    def expand(hp, wp, Lmax, side=32, nseg=15):
        P = hp * wp
        hip.imfree_expand(i32(1, 2), i32(1, side * side), i64(nseg + 1, Lmax), i32(nseg + 1), hp, wp, SEG0, BOS, EOS, PAD,
                          i64(1, P * Lmax), i64(P), i64(1, P + 1), i64(1, 256 * P + 1))
    expand(2, 2, 16)
    with pytest.raises(RuntimeError, match="code -3"):
        expand(2, 2, 17)
    with pytest.raises(RuntimeError, match="code -3"):
        expand(2, 2, 3, side=129)
    with pytest.raises(RuntimeError, match="code -2"):
        expand(65, 64, 1)
    torch.cuda.synchronize()


def test_device_word_ordinal_and_graph_replay():
    """the ordinal read from a device word gives the by-value bits; a captured draw + expand replayed after the word was
    incremented gives the next ordinals' samples"""
    dev = torch.device("cuda:0")
    B, hp, nseg = 2, 4, 15
    cpu, gpu = _pair(_names(nseg, (1, 2, 3)), hp, 1, 33, seed=7)
    src = torch.tensor([[BOS, 9, 8, EOS]] * B, device=dev)
    lens = torch.full((B,), 4, device=dev)
    word = torch.tensor([5], dtype=torch.long, device=dev)
    by_word, by_value = gpu.sample(B, word, src, lens), gpu.sample(B, 5, src, lens)
    torch.cuda.synchronize()
    flat = lambda s: {"ids": s["aux_input"]["patch_images"], "ends": s["aux_input"]["patch_masks"],
                      "prev_output_tokens": s["aux_input"]["prev_output_tokens"], "text2seg_target": s["text2seg_target"]}
    want = lambda n: cpu.expand(*cpu.draw(B, n))
    _assert_same(flat(by_word), want(5), B, hp * hp, 3)
    _assert_same(flat(by_value), want(5), B, hp * hp, 3)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = gpu.sample(B, word, src, lens)
    g.replay()
    torch.cuda.synchronize()
    _assert_same(flat(captured), want(5), B, hp * hp, 3)
    word.add_(B)
    g.replay()
    torch.cuda.synchronize()
    _assert_same(flat(captured), want(7), B, hp * hp, 3)
    assert not torch.equal(want(5)["text2seg_target"], want(7)["text2seg_target"])


# ----------------------------------------------------------------------------------------------- through the model
def _fixture(dev):
    import test_model_gpu as T
    ocfg = O.fixture_config(patch_image_size=512, orig_patch_image_size=512)
    sd = O.procedural_state_dict(ocfg)
    return ocfg, sd, (lambda: T._build(ocfg, sd, dev))


def _task(ocfg, on_device=False):
    from ifseg_amd.tasks.mm_tasks import SegmentationTask
    names = _names(ocfg.num_seg_tokens, (1, 2, 3), hi=ocfg.seg_id_offset - 1)[: ocfg.num_seg_tokens]
    task = SegmentationTask(num_seg_tokens=ocfg.num_seg_tokens, patch_image_size=512, n_base_vocab=ocfg.vocab_size - 1,
                            category_token_ids=names)
    task.cfg.artificial_image_type = "rand_k-1-33"
    task.cfg.artificial_image_on_device = on_device
    assert task.seg_id_offset == ocfg.seg_id_offset
    return task


def test_generated_sample_through_the_model():
    """logits and loss of the generated sample == those with `ids` trimmed to the batch maximum (the width the reference's
    collater pads to) == those with prev_output_tokens replaced by the [B, 1] placeholder (the engine reads its first
    column only), bit for bit"""
    from ifseg_amd.criterions import SegCriterion
    dev = torch.device("cuda:0")
    ocfg, sd, build = _fixture(dev)
    task = _task(ocfg)
    m = build()
    m.train()
    crit = SegCriterion(task, unsupervised_segmentation=True, init_seg_with_text=False)
    smp = task.build_artificial_sampler(dev, seed=1)
    B = 2
    src = O.synthetic_batch(ocfg, B, 12)["src_tokens"].to(dev)
    s = smp.sample(B, 3, src, torch.full((B,), 12, device=dev))

    def run(aux):
        _, extra = m(aux_input=aux)
        loss = crit.compute_imfree_loss(m, extra["aux_output"], {"text2seg_target": s["text2seg_target"]}, 0)
        torch.cuda.synchronize()
        return extra["aux_output"][0].float().clone(), loss.detach().clone()

    aux = s["aux_input"]
    l0, loss0 = run(aux)
    assert torch.isfinite(l0).all() and torch.isfinite(loss0)
    width = int(aux["patch_masks"].view(B, -1)[:, -1].max())
    assert width < aux["patch_images"].shape[1]
    l1, loss1 = run(dict(aux, patch_images=aux["patch_images"][:, :width].contiguous()))
    l2, loss2 = run(dict(aux, prev_output_tokens=torch.zeros(B, 1, dtype=torch.long, device=dev)))
    assert torch.equal(l0, l1) and torch.equal(loss0, loss1)
    assert torch.equal(l0, l2) and torch.equal(loss0, loss2)
    # another ordinal is another image
    l3, loss3 = run(smp.sample(B, 5, src, torch.full((B,), 12, device=dev))["aux_input"])
    assert not torch.equal(l0, l3)


# ----------------------------------------------------------------------------------------------- through the trainer
def _real_sample(ocfg, dev, B=2):
    batch = O.synthetic_batch(ocfg, B, 12)
    return {"net_input": {k: batch[k].to(dev) for k in ("src_tokens", "patch_images", "patch_masks", "prev_output_tokens")},
            "target": batch["target"].to(dev), "ntokens": 1, "nsentences": B}


def _train(build, task, sample, seed, updates=3):
    from ifseg_amd.criterions import SegCriterion
    from ifseg_amd.trainer import Trainer
    crit = SegCriterion(task, unsupervised_segmentation=True, init_seg_with_text=False)
    tr = Trainer(build(), crit, task, lr=1e-3, seed=seed, device=sample["target"].device)
    losses = [float(tr.train_step([sample])[0]["imfree_loss"]) for _ in range(updates)]
    tr.check_overflow(wait=True)
    torch.cuda.synchronize()
    return losses, tr.p32.clone(), crit


def test_trainer_draws_the_samples_a_batch_does_not_carry():
    dev = torch.device("cuda:0")
    ocfg, sd, build = _fixture(dev)
    sample = _real_sample(ocfg, dev)
    assert "aux_input" not in sample
    la, pa, crit = _train(build, _task(ocfg), sample, seed=1)
    assert all(l == l and abs(l) != float("inf") for l in la) and torch.isfinite(pa).all()
    assert crit._imfree_sampler is not None and crit._imfree_sampler.seed == 1
    assert crit.imfree_first_ordinal == 2 * 2          # update 2 (0-based), one micro-batch, one rank, batch 2
    lb, pb, _ = _train(build, _task(ocfg), sample, seed=1)
    assert la == lb and torch.equal(pa, pb)
    lc, pc, _ = _train(build, _task(ocfg), sample, seed=2)
    assert la != lc and not torch.equal(pa, pc)


def test_captured_step_draws_what_the_eager_step_draws():
    """Trainer.train_step(graph=True): the ordinal travels in a device word, so every replay of the captured update draws the
    images the eager update of the same number draws -- losses and parameters bit-equal"""
    from ifseg_amd.criterions import SegCriterion
    from ifseg_amd.trainer import Trainer
    dev = torch.device("cuda:0")
    ocfg, sd, build = _fixture(dev)
    sample = _real_sample(ocfg, dev)

    def run(graph_from):
        task = _task(ocfg)
        tr = Trainer(build(), SegCriterion(task, unsupervised_segmentation=True, init_seg_with_text=False), task, lr=1e-3, seed=1,
                     device=dev)
        losses = [float(tr.train_step([sample], graph=k >= graph_from)[0]["imfree_loss"]) for k in range(5)]
        tr.check_overflow(wait=True)
        torch.cuda.synchronize()
        return losses, tr.p32.clone()
    le, pe = run(99)
    lg, pg = run(2)
    assert len(set(le)) == 5                     # a new image every update
    assert le == lg and torch.equal(pe, pg)


def test_trainer_keeps_a_given_aux_input_unless_the_flag_is_set():
    dev = torch.device("cuda:0")
    ocfg, sd, build = _fixture(dev)
    task = _task(ocfg)
    sample = dict(_real_sample(ocfg, dev), **task.synthetic_aux_sample(2, dev))
    sample["aux_input"].update(src_tokens=sample["net_input"]["src_tokens"], src_lengths=torch.full((2,), 12, device=dev))
    la, pa, crit = _train(build, task, sample, seed=1)
    assert crit._imfree_sampler is None

    def refuse(*a, **k):
        raise AssertionError("the sampler must not be built when the batch carries aux_input and the flag is off")
    task2 = _task(ocfg)
    task2.build_artificial_sampler = refuse
    lb, pb, _ = _train(build, task2, sample, seed=1)
    assert la == lb and torch.equal(pa, pb)
    lc, pc, crit_c = _train(build, _task(ocfg, on_device=True), sample, seed=1)
    assert crit_c._imfree_sampler is not None
    assert la != lc and not torch.equal(pa, pc)
