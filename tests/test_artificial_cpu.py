"""CPU: the image-free sample generator (ifseg_amd/artificial.py) -- its flag parser, the CPU specification of the expand
step against an independent restatement of the reference's dataset code, the random stream against a numpy restatement, its
distribution, and the ordinal bookkeeping of the trainer.  No GPU."""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ifseg_amd.artificial import (ArtificialImageSampler, parse_artificial_image_type, trainer_first_ordinal)

BOS, PAD, EOS = 0, 1, 2
SEG0 = 1000


def _names(nseg, lens, seed=0):
    """nseg + 1 names whose lengths cycle through `lens`"""
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(4, SEG0 - 1, (lens[i % len(lens)],), generator=g) for i in range(nseg + 1)]


# ----------------------------------------------------------------------------------------------- parser
def test_parse_table_and_refusals_by_name():
    assert parse_artificial_image_type("rand_k") == (1, 33)
    assert parse_artificial_image_type("rand_k-1-33") == (1, 33)
    assert parse_artificial_image_type("rand_k-4-17") == (4, 17)
    assert parse_artificial_image_type("rand_k-84-85") == (84, 85)
    assert parse_artificial_image_type("none") is None
    with pytest.raises(NotImplementedError, match="norand_k"):
        parse_artificial_image_type("norand_k")
    for bad in ("random", "gt_seg", "upsampling", "rand_k-1", "rand_k-1-2-3", "rand_k_1_33", ""):
        with pytest.raises(NotImplementedError, match=repr(bad)[1:-1] if bad else "not supported"):
            parse_artificial_image_type(bad)
    for bad in ("rand_k-0-33", "rand_k-5-5", "rand_k-9-3", "rand_k-1-130", "rand_k-a-b"):
        with pytest.raises(ValueError, match=bad):
            parse_artificial_image_type(bad)


# ----------------------------------------------------------------------------------------------- expand
def _restated_expand(coarse2d, names, hp, S, Lmax):
    """segmentation_dataset.py:312-345 for ONE sample whose random map is `coarse2d` [sh, sw], then the collater's padding
    (:85-107) to the static width P * Lmax.  Both resizes are F.interpolate(mode="nearest") on the float map: what
    torchvision's tensor Resize(NEAREST) of the reference runs."""
    rand = coarse2d.reshape(1, 1, *coarse2d.shape)
    downsample = F.interpolate(rand.float(), size=(hp, hp), mode="nearest").long().reshape(-1).tolist()       # :316, :319
    upsample = F.interpolate(rand.float(), size=(S, S), mode="nearest").long().reshape(-1).tolist()           # :318
    text_length = [len(x) for x in names]
    ids, ends, run = [], [], 0
    for idx in downsample:                                                                                   # :325-326
        ids += names[idx].tolist()
        run += text_length[idx]
        ends.append(run)
    target = [SEG0 + c for c in upsample] + [EOS]                                                            # :320, :328
    prev = [BOS] + [SEG0 + c for c in downsample]                                                            # :321, :329
    assert len(ids) <= hp * hp * Lmax
    ids = ids + [PAD] * (hp * hp * Lmax - len(ids))
    return (torch.tensor(ids), torch.tensor(ends), torch.tensor(prev), torch.tensor(target))


COARSE_SHAPES = [(1, 1), (1, 32), (32, 1), (32, 32), (7, 13)]


@pytest.mark.parametrize("hp,S", [(2, 32), (4, 64), (32, 512), (40, 640)])
def test_cpu_expand_matches_restated_dataset_code(hp, S):
    nseg = 15
    names = _names(nseg, (1, 2, 3, 16))
    smp = ArtificialImageSampler(names, SEG0, hp, hp, 1, 33, seed=1, device="cpu")
    assert smp.Lmax == 16
    g = torch.Generator().manual_seed(hp)
    maps = [torch.randint(0, nseg, s, generator=g) for s in COARSE_SHAPES]
    shapes = torch.tensor([list(m.shape) for m in maps], dtype=torch.int32)
    coarse = torch.zeros(len(maps), 32 * 32, dtype=torch.int32)
    for b, m in enumerate(maps):
        coarse[b, : m.numel()] = m.reshape(-1).int()
    out = smp.expand(shapes, coarse)
    P = hp * hp
    assert out["ids"].shape == (len(maps), P * 16) and out["ends"].shape == (len(maps) * P,)
    assert out["prev_output_tokens"].shape == (len(maps), P + 1) and out["text2seg_target"].shape == (len(maps), S * S + 1)
    for b, m in enumerate(maps):
        ids, ends, prev, target = _restated_expand(m, names, hp, S, 16)
        assert torch.equal(out["ids"][b], ids), (b, "ids")
        assert torch.equal(out["ends"].view(len(maps), P)[b], ends), (b, "ends")
        assert torch.equal(out["prev_output_tokens"][b], prev), (b, "prev")
        assert torch.equal(out["text2seg_target"][b], target), (b, "target")
        assert all(t.dtype == torch.long for t in out.values())


def test_cpu_expand_uses_the_fp32_index_rule_not_the_integer_one():
    """84 -> 40 and 84 -> 640: floorf(dst * (84.f / out)) and (dst * 84) // out are different maps"""
    hp, S, nseg = 40, 640, 150
    for out_size in (hp, S):
        d = torch.arange(out_size)
        rule = F.interpolate(torch.arange(84.0).view(1, 1, 1, 84), size=(1, out_size), mode="nearest").long().reshape(-1)
        assert not torch.equal(rule, (d * 84) // out_size)
    names = _names(nseg, (1, 2, 3))
    smp = ArtificialImageSampler(names, SEG0, hp, hp, 84, 85, seed=1, device="cpu")
    # a map whose cells are all different from their neighbours: any index slip changes the output
    m = (torch.arange(84 * 84).reshape(84, 84) * 7 + torch.arange(84).reshape(84, 1)) % nseg
    out = smp.expand(torch.tensor([[84, 84]], dtype=torch.int32), m.reshape(1, -1).int())
    ids, ends, prev, target = _restated_expand(m, names, hp, S, smp.Lmax)
    assert torch.equal(out["ids"][0], ids) and torch.equal(out["ends"], ends)
    assert torch.equal(out["prev_output_tokens"][0], prev) and torch.equal(out["text2seg_target"][0], target)
    wrong = m[(torch.arange(S) * 84) // S][:, (torch.arange(S) * 84) // S].reshape(-1) + SEG0
    assert not torch.equal(out["text2seg_target"][0, :-1], wrong)


def test_sample_has_the_keys_the_model_and_criterion_consume():
    smp = ArtificialImageSampler(_names(5, (1, 2)), SEG0, 2, 2, 1, 33, seed=3, device="cpu")
    src = torch.tensor([[BOS, 7, 8, EOS]] * 3)
    s = smp.sample(3, 10, src, torch.full((3,), 4))
    assert set(s) == {"aux_input", "text2seg_target"}
    assert set(s["aux_input"]) == {"src_tokens", "src_lengths", "patch_images", "patch_masks", "prev_output_tokens"}
    assert s["aux_input"]["src_tokens"] is src and s["aux_input"]["patch_masks"].shape == (12,)
    assert s["text2seg_target"].shape == (3, 32 * 32 + 1) and (s["text2seg_target"][:, -1] == EOS).all()


# ----------------------------------------------------------------------------------------------- draw
def _restated_stream(seed, n, count):
    """u(n, i) = splitmix64(seed + (n << 32) + i) for i < count, in numpy uint64 (wrapping)"""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + (np.uint64(n) << np.uint64(32)) + np.arange(count, dtype=np.uint64)
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _restated_draw(seed, n, l, r, nseg):
    u = _restated_stream(seed, n, 2 + (r - 1) * (r - 1)) >> np.uint64(32)
    sh = l + int((u[0] * np.uint64(r - l)) >> np.uint64(32))
    sw = l + int((u[1] * np.uint64(r - l)) >> np.uint64(32))
    cells = ((u[2:2 + sh * sw] * np.uint64(nseg)) >> np.uint64(32)).astype(np.int64)
    return sh, sw, cells


def test_splitmix64_known_answer():
    """the first outputs of the published splitmix64 generator seeded with 0 (state + golden gamma, then the mix): the stream
    above at seed = 0, n = 0 is that generator's i-th output only for i = 0, which pins the constants"""
    assert int(_restated_stream(0, 0, 1)[0]) == 0xE220A8397B1DCDAF


@pytest.mark.parametrize("seed", [1, 7])
@pytest.mark.parametrize("nseg", [15, 150, 171])
def test_cpu_draw_matches_restated_stream(seed, nseg):
    smp = ArtificialImageSampler(_names(nseg, (1,)), SEG0, 2, 2, 1, 33, seed=seed, device="cpu")
    for first in (0, 1, 5, 1000, 2 ** 31, 2 ** 32 - 4):
        shapes, coarse = smp.draw(4, first)
        assert shapes.dtype == torch.int32 and coarse.dtype == torch.int32 and coarse.shape == (4, 32 * 32)
        for b in range(4):
            sh, sw, cells = _restated_draw(seed, first + b, 1, 33, nseg)
            assert shapes[b].tolist() == [sh, sw]
            assert coarse[b, : sh * sw].tolist() == cells.tolist()
            assert (coarse[b, sh * sw:] == 0).all()
    # another range of sides
    smp = ArtificialImageSampler(_names(nseg, (1,)), SEG0, 2, 2, 4, 17, seed=seed, device="cpu")
    shapes, coarse = smp.draw(3, 11)
    for b in range(3):
        sh, sw, cells = _restated_draw(seed, 11 + b, 4, 17, nseg)
        assert shapes[b].tolist() == [sh, sw] and coarse[b, : sh * sw].tolist() == cells.tolist()


@pytest.mark.parametrize("seed", [1, 7])
def test_draw_distribution(seed):
    """4096 ordinals of rand_k-1-33: every side length is drawn 128 times in expectation; a count is Binomial(4096, 1/32), and
    the class counts over all cells of the first 256 samples are Binomial(cells, 1/nseg).  5 standard deviations each; the
    stream is deterministic, so this cannot flake (simulated for these seeds: worst 2.9 sigma for the sides, 3.4 for the
    classes)."""
    n = 4096
    for nseg in (15, 150, 171):
        smp = ArtificialImageSampler(_names(nseg, (1,)), SEG0, 2, 2, 1, 33, seed=seed, device="cpu")
        shapes, coarse = smp.draw(n, 0)
        sd = (n * (1 / 32) * (31 / 32)) ** 0.5
        for col in (0, 1):
            cnt = torch.bincount(shapes[:, col].long(), minlength=33)
            assert cnt[0] == 0 and cnt.numel() == 33
            assert ((cnt[1:].double() - 128).abs() <= 5 * sd).all(), (col, cnt)
        assert int(shapes[:, 0].min()) == 1 and int(shapes[:, 0].max()) == 32
        cells = torch.cat([coarse[b, : int(shapes[b, 0]) * int(shapes[b, 1])] for b in range(256)]).long()
        assert int(cells.max()) == nseg - 1 and int(cells.min()) == 0
        cnt = torch.bincount(cells, minlength=nseg).double()
        m = cells.numel()
        assert ((cnt - m / nseg).abs() <= 5 * (m * (1 / nseg) * (1 - 1 / nseg)) ** 0.5).all(), (nseg, cnt)


# ----------------------------------------------------------------------------------------------- ordinals
def test_ordinal_properties():
    mk = lambda seed: ArtificialImageSampler(_names(15, (1,)), SEG0, 2, 2, 1, 33, seed=seed, device="cpu")
    a = mk(1)
    s0, c0 = a.draw(9, 0)
    for n in (0, 3, 8):
        s, c = a.draw(1, n)
        assert torch.equal(s[0], s0[n]) and torch.equal(c[0], c0[n])
    s7, c7 = mk(7).draw(9, 0)
    assert not torch.equal(s0, s7) and not torch.equal(c0, c7)
    s1, c1 = mk(1).draw(9, 0)
    assert torch.equal(s0, s1) and torch.equal(c0, c1)
    with pytest.raises(ValueError):
        a.draw(2, 2 ** 32 - 1)


def test_trainer_ordinal_formula_is_injective():
    for n_micro, world, batch in ((1, 1, 1), (1, 8, 8), (2, 3, 4), (3, 2, 5)):
        seen = {}
        for update, micro, rank in itertools.product(range(6), range(n_micro), range(world)):
            first = trainer_first_ordinal(update, micro, rank, n_micro, world, batch)
            for b in range(batch):
                assert first + b not in seen, ((update, micro, rank, b), seen[first + b])
                seen[first + b] = (update, micro, rank, b)
        assert sorted(seen) == list(range(6 * n_micro * world * batch))      # dense: nothing skipped either
    # a resumed run: the ordinal depends on the update counter alone
    assert trainer_first_ordinal(5, 1, 2, 2, 3, 4) == ((5 * 2 + 1) * 3 + 2) * 4


def test_task_builds_the_sampler_from_its_category_names():
    from ifseg_amd.tasks.mm_tasks import SegmentationTask
    names = _names(5, (1, 2, 3))[:5]
    task = SegmentationTask(num_seg_tokens=5, patch_image_size=64, n_base_vocab=SEG0, category_token_ids=names)
    assert task.cfg.artificial_image_on_device is False
    task.cfg.artificial_image_type = "rand_k-1-33"
    smp = task.build_artificial_sampler("cpu", seed=7)
    assert (smp.nseg, smp.hp, smp.wp, smp.l, smp.r, smp.seed, smp.seg_id_offset) == (5, 4, 4, 1, 33, 7, SEG0)
    assert smp.name_len.tolist() == [1, 2, 3, 1, 2, 0] and smp.Lmax == 3
    task.cfg.artificial_image_type = "random"
    with pytest.raises(NotImplementedError, match="random"):
        task.build_artificial_sampler("cpu")
