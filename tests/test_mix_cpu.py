"""CPU: the specification of the batch mix (`ifseg_amd.augment`: mix_draw_reference, mix_apply_reference, BatchMix) by its
properties, `task.mix_samples` / `task.dacs_sample` on the CPU transform, the header, the library's exports, the refusals of
the C entry points in front of their launches, and the two ops under FakeTensorMode."""
import math
import os
import re

import pytest
import torch

import _mix_cases as MC
from ifseg_amd import augment as A
from ifseg_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG0 = MC.SEG0


def _bits(rec):
    """the chosen classes of one record"""
    return [c for c in range(256) if (int(rec[c >> 5]) >> (c & 31)) & 1]


# ------------------------------------------------------------------------------------------------- the chosen set
@pytest.mark.parametrize("nseg", MC.NSEGS)
def test_chosen_set_is_half_of_the_present_classes(nseg):
    for B, P in MC.SHAPES:
        tgt = MC.block_target(B, P, nseg)
        rec = A.mix_draw_reference(tgt, nseg, SEG0, MC.SEED, 11)
        assert rec.dtype == torch.int32 and tuple(rec.shape) == (B, 16)
        for b in range(B):
            c = tgt[b, :-1] - SEG0
            present = sorted(set(c[(c >= 0) & (c < nseg)].tolist()))
            chosen = _bits(rec[b])
            assert int(rec[b, 12]) == len(present) and int(rec[b, 13]) == len(chosen) == (len(present) + 1) // 2
            assert set(chosen) <= set(present) and rec[b, 8:12].tolist() == [0] * 4 and rec[b, 14:].tolist() == [0, 0]


def test_no_class_one_class_and_the_64_bit_rule():
    tgt = MC.special_target()
    rec = A.mix_draw_reference(tgt, 33, SEG0, MC.SEED, 0)
    assert int(rec[0, 12]) == 5 and int(rec[0, 13]) == 3 and set(_bits(rec[0])) <= {0, 7, 30, 31, 32}
    # 'unknown' only; the impostor seg_id_offset + 2**32 + 3, -1 and an id below the offset: nothing present, nothing chosen
    assert rec[1].tolist() == [0] * 16 and rec[2].tolist() == [0] * 16
    assert A.mix_classes(torch.tensor([MC.IMPOSTOR, -1, SEG0 + 3, SEG0 + 33, SEG0 - 1]), 33, SEG0) == [3]
    for c in (0, 31, 32, 254):
        one = A.mix_draw_reference(MC.class_target([c]), 255, SEG0, MC.SEED, 9)
        assert _bits(one[0]) == [c] and one[0, 12:14].tolist() == [1, 1]
    # across the word boundary: over ordinals both 31 and 32 get chosen, and the bits land in words 0 and 1
    words = torch.stack([A.mix_draw_reference(tgt[:1], 33, SEG0, MC.SEED, k)[0, :2] for k in range(16)])
    assert bool((words[:, 0] < 0).any()) and bool((words[:, 1] == 1).any())
    full = A.mix_draw_reference(MC.full_target(), 255, SEG0, MC.SEED, 3)
    assert full[0, 12:14].tolist() == [255, 128] and len(_bits(full[0])) == 128


@pytest.mark.parametrize("n", [2, 3, 7, 15, 255])
def test_selection_frequencies(n):
    """ordinals 0 .. 1999 at seed 5: every class is chosen with frequency within 5 standard deviations of m / n (binomial,
    N = 2000: at most 0.056)"""
    N, m = 2000, (n + 1) // 2
    present = list(range(n))
    hits = torch.zeros(n)
    for k in range(N):
        chosen = A.mix_choice(present, MC.SEED, k)
        assert len(set(chosen)) == m
        hits[chosen] += 1
    p = m / n
    bound = 5 * math.sqrt(p * (1 - p) / N)
    worst = float((hits / N - p).abs().max())
    print("n = %d: worst deviation %.4f, bound %.4f" % (n, worst, bound))
    assert bound <= 0.056 and worst <= bound
    # mix_draw_reference is this choice on the classes of the map
    rec = A.mix_draw_reference(MC.class_target(present), 255, SEG0, MC.SEED, 77)
    assert sorted(A.mix_choice(present, MC.SEED, 77)) == _bits(rec[0])


@pytest.mark.parametrize("P", [16, 48])
def test_box_bounds(P):
    tgt = MC.block_target(3, P, 15)
    seen = set()
    for first in range(0, 300, 3):
        rec = A.mix_draw_reference(tgt, 15, SEG0, MC.SEED, first, mask="box")
        for r in rec.tolist():
            y0, x0, y1, x1 = r[8:12]
            assert r[:8] == [0] * 8 and r[12:] == [0] * 4
            assert P // 4 <= y1 - y0 <= 3 * P // 4 and P // 4 <= x1 - x0 <= 3 * P // 4
            assert 0 <= y0 and y1 <= P and 0 <= x0 and x1 <= P
            seen.add((y1 - y0, x1 - x0))
    if P == 16:                                                             # nine heights: 300 draws reach both ends
        assert {h for h, _ in seen} >= {P // 4, 3 * P // 4} and {w for _, w in seen} >= {P // 4, 3 * P // 4}
    assert (A.mix_box(P, MC.SEED, 4)) == tuple(A.mix_draw_reference(tgt[:1], 15, SEG0, MC.SEED, 4, mask="box")[0, 8:12].tolist())


@pytest.mark.parametrize("mask", ["class", "box"])
def test_pure_function_of_the_ordinal(mask):
    tgt = MC.block_target(3, 16, 15)
    batch = A.mix_draw_reference(tgt, 15, SEG0, MC.SEED, 40, mask=mask)
    for b in range(3):
        assert torch.equal(batch[b], A.mix_draw_reference(tgt[b:b + 1], 15, SEG0, MC.SEED, 40 + b, mask=mask)[0])
    other = A.mix_draw_reference(tgt, 15, SEG0, MC.SEED + 1, 40, mask=mask)
    assert not torch.equal(batch, other)
    # the mix reads slots 28 and up: the transform's 28 draws of the same seed and ordinal are other values
    assert A.MIX_SLOT_BOX == 28 and A.MIX_SLOT_CLASS == 32 and len(A.draws(MC.SEED, 40)) == 28


def test_draw_refusals():
    tgt = MC.block_target(2, 16, 15)
    for kw in (dict(nseg=0), dict(nseg=256), dict(mask="circle"), dict(first_ordinal=-1), dict(first_ordinal=2 ** 32 - 1)):
        args = dict(src_target=tgt, nseg=15, seg_id_offset=SEG0, seed=1, first_ordinal=0)
        args.update(kw)
        with pytest.raises(ValueError):
            A.mix_draw_reference(**args)
    for bad in (tgt[:, :-1], tgt.int(), torch.zeros(2, 24 * 24 + 1, dtype=torch.int64), torch.zeros(2, 8 * 8 + 1, dtype=torch.int64)):
        with pytest.raises(ValueError):
            A.mix_draw_reference(bad, 15, SEG0, 1, 0)


# ------------------------------------------------------------------------------------------------- apply
def _loop(rec, src, dst, nseg):
    """an independent per-pixel loop over one sample's selection"""
    (si, st, sw), (di, dt, dw) = src, dst
    P = si.shape[-1]
    sel = torch.zeros(P * P, dtype=torch.bool)
    r = rec.tolist()
    for p in range(P * P):
        y, x = divmod(p, P)
        c = int(st[p]) - SEG0
        pick = 0 <= c < nseg and (r[c >> 5] >> (c & 31)) & 1 == 1
        sel[p] = pick or (r[8] <= y < r[10] and r[9] <= x < r[11])
    return sel


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_apply_is_the_union_of_box_and_classes(dtype):
    B, P, nseg = 3, 16, 15
    st, dt = MC.block_target(B, P, nseg, 0), MC.block_target(B, P, nseg, 1)
    si, di = MC.images(B, P, dtype, 0), MC.images(B, P, dtype, 1)
    sw, dw = MC.weights(B, P, 0), MC.weights(B, P, 1)
    rec = MC.both_record(B, P, A.mix_draw_reference(st, nseg, SEG0, MC.SEED, 0))
    img, tgt, wgt = A.mix_apply_reference(rec, (si, st, sw), (di, dt, dw), nseg, SEG0)
    assert img.dtype == dtype and tgt.dtype == torch.int64 and wgt.dtype == torch.uint8
    sel = torch.stack([_loop(rec[b], (si[b], st[b], sw[b]), (di[b], dt[b], dw[b]), nseg) for b in range(B)])
    assert torch.equal(sel, A.mix_selection(rec, st, nseg, SEG0)) and bool(sel.any()) and bool((~sel).any())
    s4 = sel.reshape(B, 1, P, P).expand(B, 3, P, P)
    assert torch.equal(MC.as_int(img)[s4], MC.as_int(si)[s4]) and torch.equal(MC.as_int(img)[~s4], MC.as_int(di)[~s4])
    assert torch.equal(tgt[:, :-1][sel], st[:, :-1][sel]) and torch.equal(tgt[:, :-1][~sel], dt[:, :-1][~sel])
    assert torch.equal(wgt[sel], sw[sel]) and torch.equal(wgt[~sel], dw[~sel])
    # the pixels without a class are pasted by the box alone
    c = st[:, :-1] - SEG0
    classless = (c < 0) | (c >= nseg)
    box_only = A.mix_selection(torch.cat([torch.zeros(B, 8, dtype=torch.int32), rec[:, 8:]], 1), st, nseg, SEG0)
    assert torch.equal(sel[classless], box_only[classless]) and bool(sel[classless].any())
    # a box that reaches outside the image selects less, and bits at or above nseg are never consulted
    wild = rec.clone()
    wild[:, 0] |= -(1 << nseg)
    wild[:, 1:8] = -1
    assert torch.equal(A.mix_selection(wild, st, nseg, SEG0), sel)


def test_apply_weights_and_eos():
    B, P, nseg = 2, 16, 15
    st, dt = MC.block_target(B, P, nseg, 0), MC.block_target(B, P, nseg, 1).clone()
    dt[:, -1] = 77                                                          # a marker in the destination's EOS column
    si, di = MC.images(B, P, torch.float32, 0), MC.images(B, P, torch.float32, 1)
    sw, dw = MC.weights(B, P, 0), MC.weights(B, P, 1)
    rec = A.mix_draw_reference(st, nseg, SEG0, MC.SEED, 0)
    sel = A.mix_selection(rec, st, nseg, SEG0)
    none = A.mix_apply_reference(rec, (si, st), (di, dt), nseg, SEG0)
    assert none[2] is None and none[1][:, -1].tolist() == [77, 77]
    only_src = A.mix_apply_reference(rec, (si, st, sw), (di, dt), nseg, SEG0)[2]
    only_dst = A.mix_apply_reference(rec, (si, st), (di, dt, dw), nseg, SEG0)[2]
    assert torch.equal(only_src[sel], sw[sel]) and bool((only_src[~sel] == 255).all())
    assert bool((only_dst[sel] == 255).all()) and torch.equal(only_dst[~sel], dw[~sel])
    # samples in train_sample's layout are taken as well
    as_sample = lambda i, t, w: {"net_input": {"patch_images": i}, "target": t, "target_weight": w}
    again = A.mix_apply_reference(rec, as_sample(si, st, sw), as_sample(di, dt, dw), nseg, SEG0)
    want = A.mix_apply_reference(rec, (si, st, sw), (di, dt, dw), nseg, SEG0)
    assert all(torch.equal(MC.as_int(a) if a.is_floating_point() else a, MC.as_int(b) if b.is_floating_point() else b)
               for a, b in zip(again, want))
    for bad in (lambda: A.mix_apply_reference(rec, (si.bfloat16(), st), (di, dt), nseg, SEG0),
                lambda: A.mix_apply_reference(rec, (si[:1], st[:1]), (di, dt), nseg, SEG0),
                lambda: A.mix_apply_reference(rec[:1], (si, st), (di, dt), nseg, SEG0),
                lambda: A.mix_apply_reference(rec, (si, st, sw.int()), (di, dt), nseg, SEG0),
                lambda: A.mix_apply_reference(rec, (si, st), (di, dt), 256, SEG0)):
        with pytest.raises(ValueError):
            bad()


def test_batch_mix_on_the_cpu():
    B, P, nseg = 3, 16, 15
    src = (MC.images(B, P, torch.float32, 0), MC.block_target(B, P, nseg, 0), MC.weights(B, P, 0))
    dst = (MC.images(B, P, torch.float32, 1), MC.block_target(B, P, nseg, 1))
    for mask in A.MIX_MASKS:
        mix = A.BatchMix(P, nseg, SEG0, seed=MC.SEED, device="cpu", mask=mask)
        rec = mix.draw(src, 21)
        assert torch.equal(rec, A.mix_draw_reference(src[1], nseg, SEG0, MC.SEED, 21, mask)) and torch.equal(rec, mix.draw(src[1], 21))
        got, want = mix(src, dst, 21), A.mix_apply_reference(rec, src, dst, nseg, SEG0)
        assert torch.equal(MC.as_int(got[0]), MC.as_int(want[0])) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
    with pytest.raises(ValueError):
        A.BatchMix(24, nseg, SEG0)
    with pytest.raises(ValueError):
        A.BatchMix(P, nseg, SEG0, mask="circle")
    with pytest.raises(ValueError):
        A.BatchMix(32, nseg, SEG0).draw(src, 0)


# ------------------------------------------------------------------------------------------------- the task
def _task(P=32, n=5):
    from ifseg_amd.tasks.mm_tasks import SegmentationTask
    task = SegmentationTask(num_seg_tokens=n, patch_image_size=P, n_base_vocab=100, category_token_ids=[[31], [32, 33], [34], [35], [36]])
    task.build_train_transform("cpu", seed=6)
    return task


def test_task_mix_samples_on_the_cpu_transform():
    task = _task()
    a, b = task.synthetic_sample(2, "cpu", seed=1), task.synthetic_sample(2, "cpu", seed=2)
    b["target_weight"] = torch.full((2, 32 * 32), 9, dtype=torch.uint8)
    for mask in ("class", "box"):
        s = task.mix_samples(a, b, 3, mask=mask)
        assert set(s) == set(task.synthetic_sample(2, "cpu")) | {"target_weight"}
        assert set(s["net_input"]) == set(b["net_input"]) and s["net_input"]["src_tokens"] is b["net_input"]["src_tokens"]
        rec = A.mix_draw_reference(a["target"], 5, task.seg_id_offset, 6, 3, mask)
        img, tgt, wgt = A.mix_apply_reference(rec, a, b, 5, task.seg_id_offset)
        assert torch.equal(s["net_input"]["patch_images"], img) and torch.equal(s["target"], tgt) and torch.equal(s["target_weight"], wgt)
        sel = A.mix_selection(rec, a["target"], 5, task.seg_id_offset)
        assert bool((wgt[sel] == 255).all()) and bool((wgt[~sel] == 9).all()) and bool(sel.any()) and bool((~sel).any())
        assert b["net_input"]["patch_images"] is not s["net_input"]["patch_images"] and "target_weight" in b
    plain = task.mix_samples(a, task.synthetic_sample(2, "cpu", seed=2), 3)
    assert set(plain) == set(task.synthetic_sample(2, "cpu"))
    with pytest.raises(ValueError):
        task.mix_samples(task.synthetic_sample(3, "cpu"), b, 3)                      # another B
    with pytest.raises(ValueError):
        task.mix_samples(task.synthetic_sample(2, "cpu", image_hw=(16, 16)), b, 3)   # another P
    short = task.synthetic_sample(2, "cpu")
    short["net_input"]["src_tokens"] = short["net_input"]["src_tokens"][:, :-1]
    with pytest.raises(ValueError):
        task.mix_samples(short, b, 3)                                                # another prompt length


def test_dacs_sample_ordinal_bound():
    task = _task()
    img, lab = torch.zeros(40, 40, 3, dtype=torch.uint8), torch.zeros(40, 40, dtype=torch.uint8)
    for first in (2 ** 31 - 1, 2 ** 31, -1):
        with pytest.raises(ValueError, match="2\\*\\*31"):
            task.dacs_sample(None, [img, img], [lab, lab], [img, img], first)


# ------------------------------------------------------------------------------------------------- surface and refusals
def _lib():
    if not os.path.exists(hip.LIB_PATH):
        from ifseg_amd.build import build
        build(verbose=False)
    return hip.lib()


def test_header_declares_the_entry_points_and_the_library_exports_them():
    with open(os.path.join(ROOT, "include", "ifseg_hip.h")) as f:
        header = f.read()
    assert re.search(r"^int ifseg_mix_draw\(", header, re.M) and re.search(r"^int ifseg_mix_apply\(", header, re.M)
    assert re.search(r"#define\s+IFSEG_ABI_VERSION\s+21\b", header) and hip.ABI_VERSION == 21
    assert os.path.exists(os.path.join(ROOT, "ifseg_amd", "csrc", "mix.hip"))
    lib = _lib()
    assert hasattr(lib, "ifseg_mix_draw") and hasattr(lib, "ifseg_mix_apply") and lib.ifseg_abi_version() == 21


def test_entry_points_refuse_before_they_launch():
    """the C entry points check their arguments in front of the launch: on a machine without a GPU a refusal still comes back"""
    import ctypes
    lib = _lib()
    ll, p = ctypes.c_longlong, ctypes.c_void_p
    draw = lambda tgt=64, B=2, P=16, nseg=15, first=0, box=0, rec=128: lib.ifseg_mix_draw(
        p(tgt), B, P, nseg, ll(SEG0), ctypes.c_uint64(1), ll(first), box, p(rec), None)
    BAD_SHAPE, BAD_ARG = -2, -3
    assert draw(tgt=0) == BAD_ARG and draw(tgt=68) == BAD_ARG and draw(rec=0) == BAD_ARG and draw(nseg=0) == BAD_ARG
    assert draw(nseg=256) == BAD_ARG and draw(box=2) == BAD_ARG and draw(first=-1) == BAD_ARG and draw(first=2 ** 32 - 1) == BAD_ARG
    assert draw(P=24) == BAD_SHAPE and draw(P=0) == BAD_SHAPE and draw(P=4112) == BAD_SHAPE and draw(B=0) == BAD_SHAPE
    M = 1 << 24                                     # made-up addresses, one MiB-aligned slot per tensor: nothing is dereferenced
    slots = dict(rec=1, si=2, st=3, sw=4, di=5, dt=6, dw=7, oi=8, ot=9, ow=10)

    def apply(B=2, P=16, nseg=15, eb=4, **kw):
        a = {k: v * M for k, v in slots.items()}
        a.update(kw)
        return lib.ifseg_mix_apply(p(a["rec"]), p(a["si"]), p(a["st"]), p(a["sw"]), p(a["di"]), p(a["dt"]), p(a["dw"]), B, P, nseg,
                                   ll(SEG0), eb, p(a["oi"]), p(a["ot"]), p(a["ow"]), None)
    assert apply(eb=3) == BAD_ARG and apply(nseg=0) == BAD_ARG and apply(nseg=256) == BAD_ARG and apply(si=0) == BAD_ARG
    assert apply(ow=0) == BAD_ARG and apply(sw=0, dw=0) == BAD_ARG                  # a plane out iff a plane in
    assert apply(si=2 * M + 8) == BAD_ARG and apply(ot=9 * M + 4) == BAD_ARG and apply(dw=7 * M + 4) == BAD_ARG
    assert apply(P=24) == BAD_SHAPE and apply(B=0) == BAD_SHAPE and apply(B=64, P=4096) == BAD_SHAPE
    # out over the source, the records or another tensor of the destination: refused; shifted against its own destination: refused
    assert apply(oi=2 * M) == BAD_ARG and apply(ot=3 * M) == BAD_ARG and apply(ow=4 * M) == BAD_ARG and apply(oi=1 * M) == BAD_ARG
    assert apply(oi=6 * M) == BAD_ARG and apply(oi=5 * M + 16) == BAD_ARG and apply(ot=8 * M) == BAD_ARG


def test_ops_are_registered_with_fake_kernels():
    import ifseg_amd.ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    draw, apply = torch.ops.ifseg.mix_draw, torch.ops.ifseg.mix_apply
    with FakeTensorMode():
        B, P = 3, 48
        e = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device="cuda")
        st, dt = e(B, P * P + 1, dt=torch.int64), e(B, P * P + 1, dt=torch.int64)
        for mask in ("class", "box"):
            rec = draw(st, 150, SEG0, 5, 7, mask)
            assert tuple(rec.shape) == (B, 16) and rec.dtype == torch.int32 and rec.is_cuda
        for dtype in (torch.float32, torch.bfloat16):
            si, di, w = e(B, 3, P, P, dt=dtype), e(B, 3, P, P, dt=dtype), e(B, P * P, dt=torch.uint8)
            for sw, dw in ((None, None), (w, None), (None, w), (w, w)):
                img, tgt, wgt = apply(rec, si, st, sw, di, dt, dw, 150, SEG0)
                assert tuple(img.shape) == (B, 3, P, P) and img.dtype == dtype and img.is_cuda
                assert tuple(tgt.shape) == (B, P * P + 1) and tgt.dtype == torch.int64
                assert wgt.dtype == torch.uint8 and tuple(wgt.shape) == ((0,) if sw is None and dw is None else (B, P * P))
        si, di = e(B, 3, P, P), e(B, 3, P, P)
        for bad in (lambda: draw(st, 0, SEG0, 5, 7, "class"), lambda: draw(st, 256, SEG0, 5, 7, "class"),
                    lambda: draw(st, 15, SEG0, 5, 7, "circle"), lambda: draw(st.int(), 15, SEG0, 5, 7, "class"),
                    lambda: draw(e(B, 24 * 24 + 1, dt=torch.int64), 15, SEG0, 5, 7, "class"), lambda: draw(st, 15, SEG0, 5, -1, "box"),
                    lambda: apply(rec, si.bfloat16(), st, None, di, dt, None, 15, SEG0), lambda: apply(rec, si[:2], st[:2], None, di, dt, None, 15, SEG0),
                    lambda: apply(rec[:2], si, st, None, di, dt, None, 15, SEG0), lambda: apply(rec, si, st, None, di, dt, None, 256, SEG0),
                    lambda: apply(rec, si, st, w.int(), di, dt, None, 15, SEG0), lambda: apply(rec.long(), si, st, None, di, dt, None, 15, SEG0)):
            with pytest.raises(ValueError):
                bad()
