"""CPU: the specification of the strong augmentation (`ifseg_amd.augment`, third section) -- the blur weight table against its
formula and the library's copy, the grey-level recovery, the identities (all off, a constant image), the jitter against
`augment.photometric`, invalid records, the gate frequencies of the random stream -- and the surface: header, bindings, ops,
task keywords, `StrongAugment` on the CPU."""
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import _strong_cases as SC
from ifseg_amd import augment as A
from ifseg_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    if not os.path.exists(hip.LIB_PATH):
        from ifseg_amd.build import build
        build(verbose=False)
    return hip.lib()


# ------------------------------------------------------------------------------------------------- the weight table
def test_blur_weights_are_the_formula():
    W = A.BLUR_WEIGHTS
    assert tuple(W.shape) == (64, 5)
    margin = 1.0
    for s in range(64):
        sigma = 0.15 + s / 64.0
        g = [math.exp(-i * i / (2 * sigma * sigma)) for i in range(24)]
        Z = g[0] + 2 * sum(g[1:])
        prod = [4096 * v / Z for v in g]
        w = [math.floor(v + 0.5) for v in prod]
        assert not any(w[5:]), s                                                   # no tap beyond 4 rounds to a weight
        assert W[s].tolist() == [4096 - 2 * sum(w[1:5])] + w[1:5], s
        assert int(W[s, 0]) + 2 * int(W[s, 1:].sum()) == 4096 and W[s, 0] >= W[s, 1] and bool((W[s] >= 0).all())
        margin = min(margin, min(abs(v + 0.5 - round(v + 0.5)) for v in prod[1:]))
    assert margin > 1.3e-3, margin                                                 # a libm off by an ulp cannot change the table
    assert W[0].tolist() == list(SC.IDENTITY) and W[63].tolist() == [1440, 977, 304, 44, 3]
    assert SC.BOX[0] + 2 * sum(SC.BOX[1:]) == 4096


def test_library_table_is_the_formula():
    _lib()
    t = hip.strong_blur_table()
    assert t.dtype == torch.int32 and tuple(t.shape) == (64, 5) and np.array_equal(t.numpy(), A.BLUR_WEIGHTS)


# ------------------------------------------------------------------------------------------------- grey levels
@pytest.mark.parametrize("stats", ["half", "imagenet"])
@pytest.mark.parametrize("dtype", SC.DTYPES)
def test_grey_levels_are_the_count(dtype, stats):
    mean, std = SC.STATS[stats]
    x, want = SC.literal_levels(dtype, stats)
    got = A.grey_levels(x[:, :, None].contiguous(), mean, std)[:, :, 0]             # [3, N, 1]: plane c is row c
    assert np.array_equal(got, want.numpy())
    assert np.array_equal(got[:, :256], np.tile(np.arange(256), (3, 1)))            # every table value gives its index back
    n = x.shape[1]
    assert got[:, n - 8].tolist() == [0] * 3 and got[:, n - 7].tolist() == [255] * 3 and got[:, n - 6].tolist() == [0] * 3   # NaN, +inf, -inf


@pytest.mark.parametrize("reverse", [False, True])
def test_all_off_returns_a_table_valued_input(reverse):
    for dtype in SC.DTYPES:
        for stats in ("half", "imagenet"):
            mean, std = SC.STATS[stats]
            img = SC.level_images(3, 16, dtype, stats, reverse)
            out = A.strong_apply_reference(SC.records_of(3, SC.ALL_OFF), img, mean, std, reverse)
            assert out.dtype == dtype and torch.equal(SC.as_int(out), SC.as_int(img))
            # the true colours behind the planes are those the images were made of
            assert np.array_equal(SC.np_levels(img, stats, reverse), SC.grey(3, 16).permute(0, 2, 3, 1).numpy())


def test_blur_of_a_constant_image_is_the_image():
    lut = A.normalisation_table()
    q = torch.tensor([0, 97, 255])
    img = torch.stack([lut[c][q[c]].expand(32, 32) for c in range(3)])[None].contiguous()
    for w in (A.BLUR_WEIGHTS[63].tolist(), A.BLUR_WEIGHTS[20].tolist(), SC.BOX):
        out = A.strong_apply_reference(SC.records_of(1, SC.record(sigma=63, w=w)), img)
        assert torch.equal(SC.as_int(out), SC.as_int(img))


def test_blur_is_the_written_rule():
    """`blur_levels` against the two sums written out pixel by pixel with r(i)"""
    P = 16
    q = SC.grey(1, P)[0].permute(1, 2, 0).numpy()
    r = lambda i: -i if i < 0 else (2 * (P - 1) - i if i >= P else i)
    for w in (A.BLUR_WEIGHTS[63].tolist(), SC.BOX):
        h = np.zeros((P, P, 3), dtype=np.int64)
        v = np.zeros((P, P, 3), dtype=np.int64)
        for y in range(P):
            for x in range(P):
                h[y, x] = sum(w[abs(d)] * q[y, r(x + d)] for d in range(-4, 5))
        for y in range(P):
            for x in range(P):
                v[y, x] = sum(w[abs(d)] * h[r(y + d), x] for d in range(-4, 5))
        assert np.array_equal(A.blur_levels(q, w), (v + 2 ** 23) >> 24)


@pytest.mark.parametrize("reverse", [False, True])
def test_jitter_only_is_the_photometric_chain(reverse):
    B, P = 3, 16
    img = SC.level_images(B, P, torch.float32, "half", reverse)
    rgb = SC.grey(B, P).permute(0, 2, 3, 1).numpy()
    lut = A.normalisation_table()
    for name, rec in SC.record_kinds(B).items():
        if "mode" not in name:
            continue
        r = rec[0].tolist()
        train = [0] * 16
        train[A.R_BRIGHT], train[A.R_CONTRAST], train[A.R_SAT], train[A.R_HUE], train[A.R_MODE] = r[:5]
        train[A.R_BETA], train[A.R_ALPHA_C], train[A.R_ALPHA_S], train[A.R_DELTA] = r[5:9]
        want_q = torch.from_numpy(A.photometric(rgb, train).astype(np.int64)).permute(0, 3, 1, 2)
        if reverse:
            want_q = want_q.flip(1)
        want = torch.stack([lut[c][want_q[:, c]] for c in range(3)], 1)
        got = A.strong_apply_reference(rec, img, reverse_channels=reverse)
        assert torch.equal(SC.as_int(got), SC.as_int(want)), name
        assert not torch.equal(SC.as_int(got), SC.as_int(img)), name               # the operation did something


def test_delta_is_reduced_mod_180():
    img = SC.level_images(1, 16, torch.float32)
    a = A.strong_apply_reference(SC.records_of(1, SC.record(hue=1, delta=-11)), img)
    for delta in (169, -191, 169 + 180 * 1000):
        assert torch.equal(A.strong_apply_reference(SC.records_of(1, SC.record(hue=1, delta=delta)), img), a)


def test_invalid_records_poison_their_sample_only():
    B, P = 2, 16
    good = SC.invalid_records(B)[1]
    for kind in SC.KINDS:
        for dtype in SC.DTYPES:
            img = SC.images(kind, B, P, dtype)
            want = A.strong_apply_reference(torch.stack([good, good]), img)
            assert not bool(torch.isnan(want.float()).any())
            for name, rec in SC.invalid_ways():
                assert not A.strong_record_valid(rec), name
                out = A.strong_apply_reference(torch.stack([torch.tensor(rec, dtype=torch.int32), good]), img)
                assert bool(torch.isnan(out[0].float()).all()), name
                assert torch.equal(SC.as_int(out[1]), SC.as_int(want[1])), name
    assert A.strong_record_valid(good.tolist()) and A.strong_record_valid(SC.ALL_OFF)


# ------------------------------------------------------------------------------------------------- the random stream
@pytest.mark.parametrize("seed", [1, 5, 6])
def test_gate_frequencies(seed):
    rec = A.strong_draw_reference(4096, seed, 0)
    flags = rec[:, :4]
    # the gate itself: on iff (t192 >> 24) < 205
    gate = torch.tensor([(A.draws(seed, n, A.STRONG_SLOT + 1)[A.STRONG_SLOT] >> 24) < 205 for n in range(4096)])
    assert bool((flags[~gate] == 0).all())                                         # the four "on" bits are ANDed with the gate
    blur = rec[:, A.S_SIGMA] >= 0
    assert abs(float(gate.float().mean()) - 0.80) <= 0.03 and abs(float(blur.float().mean()) - 0.50) <= 0.03
    sig = torch.bincount(rec[blur, A.S_SIGMA].long(), minlength=64)
    assert int(sig.min()) >= 1 and sig.numel() == 64                               # every sigma index occurs
    W = torch.from_numpy(A.BLUR_WEIGHTS)
    assert torch.equal(rec[blur, A.S_W0:A.S_W0 + 5].long(), W[rec[blur, A.S_SIGMA].long()])
    assert bool((rec[~blur, A.S_W0:A.S_W0 + 5] == torch.tensor(SC.IDENTITY, dtype=torch.int32)).all()) and bool((rec[:, 15] == 0).all())
    # each operation fires for about half of the gated samples, the mode for half of all; parameters in their ranges
    for k in range(4):
        assert abs(float(flags[gate][:, k].float().mean()) - 0.5) <= 0.04
    assert abs(float(rec[:, A.S_MODE].float().mean()) - 0.5) <= 0.04
    f = lambda k: rec[:, k].contiguous().view(torch.float32)
    assert bool((f(A.S_BETA) >= -32).all()) and bool((f(A.S_BETA) < 32).all())
    for k in (A.S_ALPHA_C, A.S_ALPHA_S):
        assert bool((f(k) >= 0.5).all()) and bool((f(k) < 1.5).all())
    assert int(rec[:, A.S_DELTA].min()) >= -18 and int(rec[:, A.S_DELTA].max()) <= 17
    never, always = A.strong_draw_reference(4096, seed, 0, 0, 0), A.strong_draw_reference(4096, seed, 0, 256, 256)
    assert bool((never[:, :4] == 0).all()) and bool((never[:, A.S_SIGMA] == -1).all())
    assert bool((always[:, A.S_SIGMA] >= 0).all())
    bits = torch.tensor([A.draws(seed, n, A.STRONG_SLOT + 2)[A.STRONG_SLOT + 1] for n in range(4096)])
    assert torch.equal(always[:, :4].long(), torch.stack([(bits >> 1) & 1, (bits >> 3) & 1, (bits >> 4) & 1, (bits >> 5) & 1], 1))


def test_draw_is_a_pure_function_of_the_ordinal_and_uses_its_own_slots():
    a = A.strong_draw_reference(8, 5, 100)
    assert torch.equal(A.strong_draw_reference(3, 5, 104), a[4:7]) and a.dtype == torch.int32 and tuple(a.shape) == (8, 16)
    assert not torch.equal(A.strong_draw_reference(8, 6, 100), a)
    assert torch.equal(A.strong_draw_reference(2, -1, 2 ** 32 - 2), A.strong_draw_reference(2, 2 ** 64 - 1, 2 ** 32 - 2))
    assert A.STRONG_SLOT == 192 and A.MIX_SLOT_CLASS + 128 <= A.STRONG_SLOT
    # the parameters follow the transform's formulas, on slots 194..197
    t = A.draws(5, 100, 200)
    r = a[0].tolist()
    assert r[A.S_BETA] == A.f32_bits(((t[194] >> 9) - 2 ** 22) / 2.0 ** 17) and r[A.S_ALPHA_C] == A.f32_bits((2 ** 22 + (t[195] >> 9)) / 2.0 ** 23)
    assert r[A.S_ALPHA_S] == A.f32_bits((2 ** 22 + (t[196] >> 9)) / 2.0 ** 23) and r[A.S_DELTA] == ((t[197] * 36) >> 32) - 18
    for bad in (lambda: A.strong_draw_reference(0, 5, 0), lambda: A.strong_draw_reference(2, 5, -1), lambda: A.strong_draw_reference(2, 5, 2 ** 32 - 1),
                lambda: A.strong_draw_reference(2, 5, 0, 257, 128), lambda: A.strong_draw_reference(2, 5, 0, 205, -1)):
        with pytest.raises(ValueError):
            bad()


def test_apply_refusals():
    img = SC.level_images(2, 16, torch.float32)
    rec = SC.records_of(2, SC.ALL_OFF)
    for bad in (lambda: A.strong_apply_reference(rec, img, std=(0.5, 0.0, 0.5)), lambda: A.strong_apply_reference(rec, img, std=(0.5, -1, 0.5)),
                lambda: A.strong_apply_reference(rec[:1], img), lambda: A.strong_apply_reference(rec.long(), img),
                lambda: A.strong_apply_reference(rec, img.double()), lambda: A.strong_apply_reference(rec, torch.zeros(2, 3, 24, 24)),
                lambda: A.strong_apply_reference(rec, img[:, :2]), lambda: A.StrongAugment(24), lambda: A.StrongAugment(16, std=(1, 1, 0)),
                lambda: A.StrongAugment(16, jitter_p8=300), lambda: A.StrongAugment(32).apply(rec, img)):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------------------------------------- surface
def test_header_declares_the_entry_points_and_the_library_exports_them():
    with open(os.path.join(ROOT, "include", "ifseg_hip.h")) as f:
        header = f.read()
    for name in ("ifseg_strong_blur_table", "ifseg_strong_draw", "ifseg_strong_apply"):
        assert re.search(r"^int %s\(" % name, header, re.M), name
    assert re.search(r"#define\s+IFSEG_ABI_VERSION\s+21\b", header) and hip.ABI_VERSION == 21
    assert os.path.exists(os.path.join(ROOT, "ifseg_amd", "csrc", "strong.hip")) and os.path.exists(os.path.join(ROOT, "ifseg_amd", "csrc", "photo.h"))
    for name in ("strong_draw", "strong_apply", "strong_blur_table"):
        assert callable(getattr(hip, name))
    lib = _lib()
    assert all(hasattr(lib, n) for n in ("ifseg_strong_blur_table", "ifseg_strong_draw", "ifseg_strong_apply")) and lib.ifseg_abi_version() == 21


def test_entry_points_refuse_before_they_launch():
    """the C entry points check their arguments in front of the launch: on a machine without a GPU a refusal still comes back"""
    import ctypes
    lib = _lib()
    ll, p = ctypes.c_longlong, ctypes.c_void_p
    BAD_SHAPE, BAD_ARG = -2, -3
    assert lib.ifseg_strong_blur_table(None) == BAD_ARG
    draw = lambda B=2, first=0, jp=205, bp=128, rec=128: lib.ifseg_strong_draw(B, ctypes.c_uint64(1), ll(first), jp, bp, p(rec), None)
    assert draw(rec=0) == BAD_ARG and draw(rec=130) == BAD_ARG and draw(jp=-1) == BAD_ARG and draw(jp=257) == BAD_ARG
    assert draw(bp=-1) == BAD_ARG and draw(bp=257) == BAD_ARG and draw(first=-1) == BAD_ARG and draw(first=2 ** 32 - 1) == BAD_ARG
    assert draw(B=0) == BAD_SHAPE
    M = 1 << 24                                     # made-up addresses, one MiB-aligned slot per tensor: nothing is dereferenced
    slots = dict(rec=1, img=2, lut=3, out=4)

    def apply(B=2, P=16, eb=4, **kw):
        a = {k: v * M for k, v in slots.items()}
        a.update(kw)
        return lib.ifseg_strong_apply(p(a["rec"]), p(a["img"]), B, P, eb, p(a["lut"]), 0, p(a["out"]), None)
    assert apply(eb=3) == BAD_ARG and apply(eb=8) == BAD_ARG and apply(rec=0) == BAD_ARG and apply(img=0) == BAD_ARG
    assert apply(lut=0) == BAD_ARG and apply(out=0) == BAD_ARG
    assert apply(img=2 * M + 8) == BAD_ARG and apply(out=4 * M + 4) == BAD_ARG and apply(rec=M + 2) == BAD_ARG and apply(lut=3 * M + 2) == BAD_ARG
    assert apply(P=24) == BAD_SHAPE and apply(P=0) == BAD_SHAPE and apply(P=4112) == BAD_SHAPE and apply(B=0) == BAD_SHAPE
    assert apply(B=64, P=4096) == BAD_SHAPE
    # any byte shared between out and the images, the records or the table: there is no in-place form
    n = 2 * 3 * 16 * 16 * 4
    assert apply(out=2 * M) == BAD_ARG and apply(out=2 * M + 16) == BAD_ARG and apply(out=2 * M + n - 16) == BAD_ARG
    assert apply(out=2 * M - n + 16) == BAD_ARG and apply(out=1 * M) == BAD_ARG and apply(out=3 * M) == BAD_ARG
    assert apply(out=1 * M - n + 16) == BAD_ARG and apply(out=3 * M + 3056) == BAD_ARG


def test_ops_are_registered_with_fake_kernels():
    import ifseg_amd.ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    draw, apply = torch.ops.ifseg.strong_draw, torch.ops.ifseg.strong_apply
    cuda = torch.device("cuda:0")
    with FakeTensorMode():
        B, P = 3, 48
        rec = draw(B, 5, 7, 205, 128, cuda)
        assert tuple(rec.shape) == (B, 16) and rec.dtype == torch.int32 and rec.is_cuda
        for dtype in SC.DTYPES:
            img = torch.empty(B, 3, P, P, dtype=dtype, device="cuda")
            out = apply(rec, img, SC.HALF, SC.HALF, False)
            assert tuple(out.shape) == (B, 3, P, P) and out.dtype == dtype and out.is_cuda
        img = torch.empty(B, 3, P, P, device="cuda")
        for bad in (lambda: draw(0, 5, 7, 205, 128, cuda), lambda: draw(B, 5, -1, 205, 128, cuda), lambda: draw(B, 5, 2 ** 32 - 1, 205, 128, cuda),
                    lambda: draw(B, 5, 7, 257, 128, cuda), lambda: draw(B, 5, 7, 205, -1, cuda),
                    lambda: apply(rec, img.half(), SC.HALF, SC.HALF, False), lambda: apply(rec[:2], img, SC.HALF, SC.HALF, False),
                    lambda: apply(rec.long(), img, SC.HALF, SC.HALF, False), lambda: apply(rec, img, SC.HALF, (0.5, 0.0, 0.5), False),
                    lambda: apply(rec, torch.empty(B, 3, 24, 24, device="cuda"), SC.HALF, SC.HALF, False),
                    lambda: apply(rec, img[:, :2], SC.HALF, SC.HALF, False)):
            with pytest.raises(ValueError):
                bad()


# ------------------------------------------------------------------------------------------------- the layers above
def test_strong_augment_on_the_cpu_is_the_two_references():
    B, P = 3, 48
    for dtype, stats, reverse in ((torch.float32, "half", False), (torch.bfloat16, "imagenet", True)):
        mean, std = SC.STATS[stats]
        img = SC.level_images(B, P, dtype, stats, reverse)
        aug = A.StrongAugment(P, mean, std, seed=SC.SEED, reverse_channels=reverse)
        first = SC.drawn(B, True, True)[0]
        rec = aug.draw(B, first)
        assert torch.equal(rec, A.strong_draw_reference(B, SC.SEED, first))
        want = A.strong_apply_reference(rec, img, mean, std, reverse)
        assert torch.equal(SC.as_int(aug(img, first)), SC.as_int(want)) and torch.equal(SC.as_int(aug.apply(rec, img)), SC.as_int(want))
        assert not torch.equal(SC.as_int(want), SC.as_int(img))
    off = A.StrongAugment(P, seed=SC.SEED, jitter_p8=0, blur_p8=0)
    img = SC.level_images(B, P, torch.float32)
    assert torch.equal(SC.as_int(off(img, 0)), SC.as_int(img))


def _task(P=32, n=5):
    from ifseg_amd.tasks.mm_tasks import SegmentationTask
    task = SegmentationTask(num_seg_tokens=n, patch_image_size=P, n_base_vocab=100, category_token_ids=[[31], [32, 33], [34], [35], [36]])
    task.build_train_transform("cpu", seed=6)
    return task


def test_task_keywords_and_strong_augment_on_the_cpu_transform():
    from ifseg_amd.tasks.mm_tasks import SegmentationTask
    sig = inspect.signature(SegmentationTask.dacs_sample).parameters
    assert sig["strong"].default is False and sig["mask"].default == "class" and sig["trainer"].default is None
    assert list(inspect.signature(SegmentationTask.strong_augment).parameters)[:3] == ["self", "sample", "first_ordinal"]
    d = inspect.signature(A.StrongAugment.__init__).parameters
    assert (d["seed"].default, d["device"].default, d["jitter_p8"].default, d["blur_p8"].default, d["reverse_channels"].default) == (1, "cpu", 205, 128, False)
    d = inspect.signature(A.strong_draw_reference).parameters
    assert (d["jitter_p8"].default, d["blur_p8"].default) == (205, 128)
    d = inspect.signature(hip.strong_draw).parameters
    assert (d["jitter_p8"].default, d["blur_p8"].default, d["device"].default, d["out"].default) == (205, 128, None, None)
    d = inspect.signature(hip.strong_apply).parameters
    assert (d["reverse_channels"].default, d["out"].default, d["lut"].default) == (False, None, None)

    task = _task()
    aug = task.build_strong_augment()
    tf = task.train_transform
    assert aug is task.build_strong_augment() and aug is not task.build_strong_augment(blur_p8=256)
    assert (aug.P, aug.mean, aug.std, aug.seed, aug.device, aug.reverse_channels) == (tf.P, tf.mean, tf.std, tf.seed, tf.device, tf.reverse_channels)
    s = task.synthetic_sample(2, "cpu", seed=1)
    s["target_weight"] = torch.full((2, 32 * 32), 9, dtype=torch.uint8)
    first = SC.drawn(2, True, True, seed=6)[0]
    out = task.strong_augment(s, first)
    want = A.strong_apply_reference(A.strong_draw_reference(2, 6, first), s["net_input"]["patch_images"])
    assert torch.equal(SC.as_int(out["net_input"]["patch_images"]), SC.as_int(want))
    assert set(out) == set(s) and set(out["net_input"]) == set(s["net_input"])
    assert out["target"] is s["target"] and out["target_weight"] is s["target_weight"]
    assert out["net_input"]["src_tokens"] is s["net_input"]["src_tokens"] and out["net_input"]["patch_images"] is not s["net_input"]["patch_images"]
