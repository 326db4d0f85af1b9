"""GPU: hip.seg_regions and hip.seg_region_drop (csrc/regions.hip) against their specifications (`regions_reference`,
`region_drop_reference`) on every case of tests/_regions_cases.py, in views at element offsets 0, 1 and 3 between canaries,
batched, through the dispatcher, `Segmenter.pseudo_label_raw(min_region=)` end to end on the segofa_tiny fixture and
`task.self_train_sample(min_region=)` through one training step.  Everything is integer: every comparison is `torch.equal`."""
import ctypes

import pytest
import torch

import _predict_cases as PC
import _regions_cases as C
from test_predict_views_gpu import e2e  # noqa: F401  (the segofa_tiny fixture with its three raw shapes)

pytestmark = pytest.mark.gpu

BAD_SHAPE, BAD_ARG = -2, -3
OFFSETS = (0, 1, 3)
I32 = torch.int32


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ifseg_amd.ops  # noqa: F401
    return torch.device("cuda:0")


def _view(shape, dtype, off, canary, dev, src=None):
    """-> (a contiguous view of `shape` that starts `off` elements into a buffer filled with `canary`, the buffer)"""
    numel = 1
    for s in shape:
        numel *= s
    buf = torch.full((off + numel + 5,), canary, dtype=dtype, device=dev)
    view = buf[off:off + numel].view(shape)
    if src is not None:
        view.copy_(src)
    return view, buf


def _untouched(buf, off, numel, canary):
    return bool((buf[:off] == canary).all()) and bool((buf[off + numel:] == canary).all())


def _run_case(hip, key, conn, off, dev, flag):
    lab = C.labels_of(key)
    want_root, want_size = C.reference(key, conn)
    d, buf_l = _view(lab.shape, lab.dtype, off, 99, dev, lab)
    root, buf_r = _view(lab.shape, I32, off, -7, dev)
    size, buf_s = _view(lab.shape, I32, OFFSETS[(OFFSETS.index(off) + 1) % 3], -7, dev)
    got = hip.seg_regions(d, conn, root=root, size=size, flag=flag)
    assert got[0] is root and got[1] is size
    assert torch.equal(root.cpu(), want_root) and torch.equal(size.cpu(), want_size), (key, conn, off)
    assert _untouched(buf_r, off, lab.numel(), -7) and _untouched(buf_s, size.storage_offset(), lab.numel(), -7), (key, conn, off)
    assert torch.equal(buf_l[off:off + lab.numel()].view(lab.shape).cpu(), lab) and _untouched(buf_l, off, lab.numel(), 99)
    # a second call into the same output tensors gives the same bits
    first = (root.clone(), size.clone())
    hip.seg_regions(d, conn, root=root, size=size, flag=flag)
    assert torch.equal(root, first[0]) and torch.equal(size, first[1]), (key, conn, off)


@pytest.mark.parametrize("conn", C.CONNECTIVITIES)
@pytest.mark.parametrize("name", C.PATTERNS)
def test_seg_regions_equals_the_specification(name, conn):
    from ifseg_amd import hip
    dev = _dev()
    flag = torch.zeros(1, dtype=I32, device=dev)
    for i, key in enumerate(C.case_keys((name,))):
        _run_case(hip, key, conn, OFFSETS[i % 3], dev, flag)
    assert int(flag) == 0                                         # no loop ran out of its budget, anywhere


@pytest.mark.parametrize("conn", C.CONNECTIVITIES)
def test_seg_regions_batched(conn):
    """B = 3 where the last row of one image equals the first row of the next: regions do not join across images"""
    from ifseg_amd import hip
    dev = _dev()
    flag = torch.zeros(1, dtype=I32, device=dev)
    for i, key in enumerate(("batch", "batch_constant", "batch_short")):
        _run_case(hip, key, conn, OFFSETS[i % 3], dev, flag)
    assert int(flag) == 0
    # fresh outputs and a fresh flag when none are given
    lab = C.labels_of("batch").to(dev)
    root, size = hip.seg_regions(lab, conn)
    want = C.reference("batch", conn)
    assert root.dtype == I32 and size.dtype == I32 and torch.equal(root.cpu(), want[0]) and torch.equal(size.cpu(), want[1])


def test_seg_regions_op():
    from ifseg_amd import hip
    dev = _dev()
    regions_op, drop_op = torch.ops.ifseg.seg_regions, torch.ops.ifseg.seg_region_drop
    for key, conn in ((("blocks", 33, 129, True), 4), (("random2", 48, 200, False), 8), ("batch", 8)):
        lab = C.labels_of(key).to(dev)
        want = C.reference(key, conn)
        root, size = regions_op(lab, conn)
        assert torch.equal(root.cpu(), want[0]) and torch.equal(size.cpu(), want[1])
        ref = hip.seg_regions(lab, conn)
        assert torch.equal(root, ref[0]) and torch.equal(size, ref[1]) and root.data_ptr() != ref[0].data_ptr()
    lab = C.labels_of(("random2", 48, 200, False)).to(dev)
    # non-contiguous inputs are copied
    t_root, t_size = regions_op(lab.t(), 4)
    w_root, w_size = hip.seg_regions(lab.t().contiguous(), 4)
    assert torch.equal(t_root, w_root) and torch.equal(t_size, w_size)
    out, dropped, size = drop_op(lab, 4, 8, 255, 4, True)
    ref = hip.seg_region_drop(lab, 4, 8, 255, 4, True)
    assert all(torch.equal(a, b) for a, b in zip((out, dropped, size), ref))
    utils = ("test_schema", "test_autograd_registration", "test_faketensor")
    torch.library.opcheck(regions_op, (lab, 8), test_utils=utils)
    torch.library.opcheck(drop_op, (lab, 4, 8, 255, 4, True), test_utils=utils)
    # on a side stream the ops follow PyTorch's current stream
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        side = regions_op(lab, 4)
    st.synchronize()
    want = C.reference(("random2", 48, 200, False), 4)
    assert torch.equal(side[0].cpu(), want[0]) and torch.equal(side[1].cpu(), want[1])
    for bad in (lambda: regions_op(lab, 6), lambda: regions_op(lab.long(), 4), lambda: drop_op(lab, 4, 0, 255, 4, True)):
        with pytest.raises(ValueError, match="ifseg::seg_region"):
            bad()


@pytest.mark.parametrize("conn", C.CONNECTIVITIES)
def test_seg_region_drop_equals_the_specification(conn):
    from ifseg_amd import hip
    from ifseg_amd.predict import region_drop_reference
    dev = _dev()
    flag = torch.zeros(1, dtype=I32, device=dev)
    g = torch.Generator().manual_seed(11)
    keys = [("random2", 33, 129, False), ("random5", 48, 200, False), ("blocks", 48, 200, False), ("blocks", 17, 65, False),
            ("serpentine", 33, 129, False), ("constant", 1, 1, False), ("checkerboard", 3, 63, False), "batch"]
    for i, key in enumerate(keys):
        lab = C.labels_of(key)
        _, size = C.reference(key, conn)
        weight = torch.randint(1, 256, lab.shape, generator=g).to(torch.uint8)
        off = OFFSETS[i % 3]
        d, _ = _view(lab.shape, torch.uint8, off, 99, dev, lab)
        for K, fill, n, raw in ((1, 255, 4, True), (2, 255, 4, True), (8, 255, 5, False), (8, 0, 3, True), (2, 1, 254, True),
                                (lab[0].numel() + 1 if lab.dim() == 3 else lab.numel() + 1, 255, 255, False)):
            w_out, w_dropped, w_weight = region_drop_reference(lab, size, K, fill=fill, n=n, raw_labels=raw, weight=weight)
            # without the weight plane, into a canaried out
            out, buf_o = _view(lab.shape, torch.uint8, off, 77, dev)
            got = hip.seg_region_drop(d, conn, K, fill=fill, n=n, raw_labels=raw, out=out, flag=flag)
            assert got[0] is out and torch.equal(out.cpu(), w_out) and _untouched(buf_o, off, lab.numel(), 77), (key, K, fill, n, raw)
            assert got[1].dtype == torch.int64 and torch.equal(got[1].cpu(), w_dropped), (key, K, fill, n, raw)
            assert got[2].dtype == I32 and torch.equal(got[2].cpu(), size)
            # with it: zeroed in place where a pixel was dropped, and `dropped` is accumulated into
            wt, buf_w = _view(lab.shape, torch.uint8, OFFSETS[(i + 1) % 3], 55, dev, weight)
            again = hip.seg_region_drop(d, conn, K, fill=fill, n=n, raw_labels=raw, weight=wt, dropped=got[1], flag=flag)
            assert again[1] is got[1] and torch.equal(again[1].cpu(), 2 * w_dropped)
            assert torch.equal(again[0].cpu(), w_out) and torch.equal(wt.cpu(), w_weight), (key, K, fill, n, raw)
            assert _untouched(buf_w, wt.storage_offset(), lab.numel(), 55)
            assert torch.equal(d.cpu(), lab)                      # the input is only read
    assert int(flag) == 0


def test_c_entry_refusals_and_limits():
    from ifseg_amd import hip
    dev = _dev()
    L = hip.lib()
    assert hip.seg_regions_limits() == (C.TILE_ROWS, C.TILE_COLS, hip.SEG_REGION_MAX_CLASSES)
    assert L.ifseg_seg_regions_limit(ctypes.c_int(3)) == BAD_ARG
    B, H, W = 2, 17, 65
    lab = torch.zeros(B, H, W, dtype=torch.int16, device=dev)
    planes = torch.full((4, B * H * W + 4), -7, dtype=I32, device=dev)
    flag = torch.zeros(4, dtype=I32, device=dev)
    out = torch.full((B * H * W,), 77, dtype=torch.uint8, device=dev)
    dropped = torch.zeros(8, dtype=torch.int64, device=dev)
    p = lambda t, byte=0: ctypes.c_void_p(t.data_ptr() + byte)
    ci = ctypes.c_int

    def regions(labels=p(lab), lb=2, b=B, h=H, w=W, conn=4, work=p(planes[0]), count=p(planes[1]), root=p(planes[2]),
                size=p(planes[3]), fl=p(flag)):
        return L.ifseg_seg_regions(labels, ci(lb), ci(b), ci(h), ci(w), ci(conn), work, count, root, size, fl, None)

    def drop(labels=p(lab), b=B, h=H, w=W, conn=4, K=2, fill=255, n=8, o=p(out), wt=None, dr=p(dropped), work=p(planes[0])):
        return L.ifseg_seg_region_drop(labels, ci(b), ci(h), ci(w), ci(conn), ci(K), ci(fill), ci(n), ci(1), work, p(planes[1]),
                                       p(planes[2]), p(planes[3]), o, wt, dr, p(flag), None)

    for kw in (dict(labels=None), dict(work=None), dict(count=None), dict(root=None), dict(size=None), dict(fl=None), dict(lb=3),
               dict(lb=4), dict(labels=p(lab, 1)), dict(work=p(planes[0], 2)), dict(size=p(planes[3], 1)), dict(fl=p(flag, 2)),
               dict(conn=0), dict(conn=6), dict(root=p(planes[1])), dict(size=p(planes[0], 4)), dict(work=p(lab))):
        assert regions(**kw) == BAD_ARG, kw
    for kw in (dict(b=0), dict(h=0), dict(w=-1), dict(b=1 << 15, h=1 << 8, w=1 << 8)):
        assert regions(**kw) == BAD_SHAPE, kw
    for kw in (dict(o=None), dict(dr=None), dict(dr=p(dropped, 4)), dict(K=0), dict(K=-3), dict(fill=256), dict(fill=-1), dict(n=0),
               dict(n=256), dict(o=p(lab)), dict(wt=p(out)), dict(o=p(planes[2])), dict(conn=5), dict(work=None)):
        assert drop(**kw) == BAD_ARG, kw
    assert drop(h=0) == BAD_SHAPE
    torch.cuda.synchronize()
    # nothing was launched on a refusal
    assert bool((planes == -7).all()) and bool((out == 77).all()) and not flag.any() and not dropped.any()


# ------------------------------------------------------------------------------------------------- end to end
def test_pseudo_label_raw_min_region_end_to_end(e2e):  # noqa: F811
    """`pseudo_label_raw(min_region=8)` equals the reference rule applied to `pseudo_label_raw()`'s own result"""
    from ifseg_amd.predict import region_drop_reference, regions_reference
    m, raw, ocfg, mk = e2e
    n = ocfg.num_seg_tokens
    seg = mk()
    for kw in (dict(keep=0.5, boundary=1), dict(keep=0.9, return_weight=True, raw_labels=False, region_connectivity=8)):
        conn = kw.get("region_connectivity", 4)
        plain = seg.pseudo_label_raw(raw, **kw)
        res = seg.pseudo_label_raw(raw, min_region=8, **kw)
        assert len(res) == len(plain) == len(raw)
        some = 0
        for r, p in zip(res, plain):
            assert torch.equal(r.predicted, p.predicted) and torch.equal(r.conf, p.conf) and p.region_dropped is None
            lab = p.labels.cpu()
            _, size = regions_reference(lab, conn)
            ref = region_drop_reference(lab, size, 8, fill=255, n=n, raw_labels=kw.get("raw_labels", True),
                                        weight=p.weight.cpu() if p.weight is not None else None)
            assert r.labels.dtype == torch.uint8 and torch.equal(r.labels.cpu(), ref[0])
            assert r.region_dropped.dtype == torch.int64 and torch.equal(r.region_dropped.cpu(), ref[1])
            assert torch.equal(r.kept[0].cpu(), p.kept[0].cpu() - ref[1]) and torch.equal(r.kept[1], p.kept[1])
            assert int(r.kept[0].sum()) == int((r.labels != 255).sum())
            if p.weight is not None:
                assert torch.equal(r.weight.cpu(), ref[2]) and torch.equal(r.weight == 0, r.labels == 255)
            else:
                assert r.weight is None
            some += int(ref[1].sum())
        assert some > 0                                           # the filter found something to drop
    one = seg.pseudo_label_raw(raw, min_region=1, keep=0.5, boundary=1)
    assert all(torch.equal(a.labels, b.labels) and not a.region_dropped.any() for a, b in zip(one, seg.pseudo_label_raw(raw, keep=0.5, boundary=1)))


def test_self_train_sample_min_region_through_one_training_step(e2e):  # noqa: F811
    from ifseg_amd.criterions import SegCriterion
    from ifseg_amd.models.segofa import SegOFAModel, make_config
    from ifseg_amd.tasks.mm_tasks import SegmentationTask
    from ifseg_amd.trainer import Trainer
    dev = _dev()
    _, raw, ocfg, _ = e2e
    _, sd, _, src = PC.e2e_fixture()
    P, n = ocfg.patch_image_size, ocfg.num_seg_tokens
    task = SegmentationTask(num_seg_tokens=n, patch_image_size=P, n_base_vocab=ocfg.vocab_size - 1, category_token_ids=PC.E2E_NAMES)
    task.prompt_ids = PC.E2E_PROMPT
    task.build_train_transform(dev, seed=6, ratio_range=(1, 1))
    m = SegOFAModel(make_config("segofa_tiny", embed_dim=ocfg.embed_dim, ffn_dim=ocfg.ffn_dim, heads=ocfg.heads,
                                enc_layers=ocfg.enc_layers, dec_layers=ocfg.dec_layers, resnet_layers=ocfg.resnet_layers,
                                num_seg_tokens=n, vocab_size=ocfg.vocab_size, patch_image_size=P,
                                orig_patch_image_size=ocfg.orig_patch_image_size))
    torch.nn.Module.load_state_dict(m, sd, strict=False)
    m.cfg.dropout = m.cfg.encoder_drop_path_rate = m.cfg.decoder_drop_path_rate = 0.0
    m.to(dev)
    kw = dict(prompt_ids=PC.E2E_PROMPT, keep=0.5, boundary=1, min_region=8, region_connectivity=8)
    s = task.self_train_sample(m, raw, 4, **kw)
    pseudo = task.pseudo_label_raw(m, raw, **kw)
    assert all(r.region_dropped is not None for r in pseudo)
    ref = task.train_sample(raw, [r.labels for r in pseudo], 4)
    assert torch.equal(s["target"], ref["target"]) and torch.equal(s["net_input"]["patch_images"], ref["net_input"]["patch_images"])
    body = s["target"][:, :-1] - task.seg_id_offset
    assert int(body.min()) >= 0 and int(body.max()) == n and bool((body < n).any())      # kept classes and the ignore class
    weighted = task.self_train_sample(m, raw, 4, confidence_weight=True, **kw)
    assert "target_weight" in weighted and torch.equal(weighted["target"], s["target"])
    tr = Trainer(m, SegCriterion(task, unsupervised_segmentation=False, init_seg_with_text=False), task, device=dev)
    loss = float(tr.train_step([s])[0]["loss"])
    tr.check_overflow(wait=True)
    torch.cuda.synchronize()
    assert loss == loss and abs(loss) != float("inf") and loss > 0.0
