"""GPU: hip.train_draw / hip.train_load (csrc/trainload.hip) against the CPU specification of ifseg_amd/augment.py,
torch.ops.ifseg.train_load through the dispatcher, and SegmentationTask.train_sample through one Trainer.train_step on the
segofa_tiny fixture.  Inputs, records and the comparison rule are in tests/_train_load_cases.py.

Which path of the load kernel a case takes: with the default staging buffer every tile of the exact family and of the first
three general sources stages its source bytes in LDS; `staging_bytes=0` sends the same case down the direct-global path; the
1500 x 1000 source takes the direct path on its own (the footprint of a tile, some 250 rows of 3000 bytes, exceeds any buffer)."""
import ctypes

import numpy as np
import pytest
import torch

import _image_load_cases as IC
import _predict_cases as PC
import _train_load_cases as C
from ifseg_amd import augment as A

pytestmark = pytest.mark.gpu

PATHS = {"staged": None, "direct": 0}


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ifseg_amd.ops  # noqa: F401
    return torch.device("cuda:0")


def _to(ts, dev):
    return [t.to(dev) for t in ts]


# ------------------------------------------------------------------------------------------------- draw
@pytest.mark.parametrize("P", [64, 96])
def test_draw_matches_the_specification(P):
    from ifseg_amd import hip
    dev = _dev()
    imgs, labs = C.ragged_batch()
    shapes = [tuple(l.shape) for l in labs]
    dl = _to(labs, dev)
    ks = set()
    for first in C.DRAW_ORDINALS:
        for kw in ({}, {"photometric": False, "flip": False, "ratio_range": (1, 1)}, {"raw_labels": False}):
            want = A.draw_params(shapes, labs, P, C.NSEG, 12345, first, **kw)
            got = hip.train_draw(dl, P, C.NSEG, 12345, first, **kw)
            assert got.dtype == torch.int32 and got.shape == (len(labs), 16)
            assert torch.equal(got.cpu(), want), (P, first, kw, got.cpu().tolist(), want.tolist())
            ks |= set(want[:, 4].tolist())
    assert 0 in ks and 10 in ks
    # many ordinals of the mixed map (32 x 80 -> P x 2.5 P at ratio 1): the verdict patterns the ten workgroups can leave, into
    # a caller's tensor
    lab = C.label("mixed", 32, 80)
    out = torch.empty(32, 16, dtype=torch.int32, device=dev)
    assert hip.train_draw([lab.to(dev)] * 32, P, C.NSEG, C.CROP_SEED, 0, ratio_range=(1, 1), out=out) is out
    want = A.draw_params([(32, 80)] * 32, [lab] * 32, P, C.NSEG, C.CROP_SEED, 0, ratio_range=(1, 1))
    assert torch.equal(out.cpu(), want)
    assert len(set(want[:, 4].tolist())) >= 3


# ------------------------------------------------------------------------------------------------- load, exact family
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("which", [0, 1])
def test_load_exact_family_bit_for_bit(which, path):
    from ifseg_amd import hip
    dev = _dev()
    P, imgs, labs, params = C.exact_family(which)
    di, dl, sb = _to(imgs, dev), _to(labs, dev), PATHS[path]
    for rev in (False, True):
        n32, tgt, q, q0 = C.exact_reference(which, torch.float32, rev)
        o32, t32 = hip.train_load(di, dl, params.to(dev), P, C.NSEG, C.SEG0, reverse_channels=rev, staging_bytes=sb)
        assert o32.dtype == torch.float32 and o32.shape == (len(imgs), 3, P, P) and o32.is_contiguous()
        assert t32.dtype == torch.int64 and t32.shape == (len(imgs), P * P + 1)
        assert torch.equal(t32.cpu(), tgt)
        assert torch.equal(o32.cpu(), n32)
        o16, t16 = hip.train_load(di, dl, params, P, C.NSEG, C.SEG0, reverse_channels=rev, dtype=torch.bfloat16, staging_bytes=sb)
        assert o16.dtype == torch.bfloat16 and torch.equal(o16.cpu(), n32.to(torch.bfloat16)) and torch.equal(t16.cpu(), tgt)
    # the grey levels themselves, through the table that carries q
    oq, _ = hip.train_load(di, dl, params.to(dev), P, C.NSEG, C.SEG0, IC.Q_MEAN, IC.Q_STD, staging_bytes=sb)
    assert torch.equal(IC.q_of(oq).cpu().permute(0, 2, 3, 1), C.exact_reference(which)[2])
    # class ids as they are, per-channel statistics
    from ifseg_amd.imageio import IMAGENET_DEFAULT_MEAN as M, IMAGENET_DEFAULT_STD as S
    want = A.train_load_reference(imgs, labs, params, P, C.NSEG, C.SEG0, M, S, raw_labels=False, dtype=torch.float32)
    got = hip.train_load(di, dl, params.to(dev), P, C.NSEG, C.SEG0, M, S, raw_labels=False, staging_bytes=sb)
    assert torch.equal(got[0].cpu(), want[0]) and torch.equal(got[1].cpu(), want[1])


# ------------------------------------------------------------------------------------------------- load, general ratios
@pytest.mark.parametrize("i", range(len(C.GENERAL_SOURCES)))
def test_load_general_ratios(i):
    from ifseg_amd import hip
    from ifseg_amd.imageio import normalisation_table
    dev = _dev()
    P = 64
    img, lab, rec, ref, ys, xs = C.general_case(i)
    di, dl = [img.to(dev)], [lab.to(dev)]
    plain = rec.clone()
    plain[A.R_BRIGHT:A.R_HUE + 1] = 0
    lut = normalisation_table()
    paths = PATHS if i < 3 else {"direct on its own": None}
    for path, sb in paths.items():
        # 1. resize only: the device's grey levels obey the rule of _image_load_cases.Reference
        oq, tq = hip.train_load(di, dl, plain[None].to(dev), P, C.NSEG, C.SEG0, IC.Q_MEAN, IC.Q_STD, staging_bytes=sb)
        q_dev = IC.q_of(oq)[0].cpu().permute(1, 2, 0).contiguous()
        want_q = ref.q[0][:, ys][:, :, xs].permute(1, 2, 0)
        print(C.GENERAL_SOURCES[i], path, "grey levels off the reference: %d of %d" % (int((q_dev != want_q).sum()), q_dev.numel()))
        C.check_resize(ref, ys, xs, q_dev, what=(i, path))
        # 2. photometric on the device's own grey levels, through the table, everywhere and bit for bit
        want = torch.from_numpy(A.photometric(q_dev.numpy(), rec.tolist())).permute(2, 0, 1).long()
        assert (want != q_dev.permute(2, 0, 1)).any()
        norm = torch.stack([lut[c][want[c]] for c in range(3)])
        for dt in (torch.float32, torch.bfloat16):
            o, t = hip.train_load(di, dl, rec[None].to(dev), P, C.NSEG, C.SEG0, dtype=dt, staging_bytes=sb)
            assert torch.equal(o[0].cpu(), norm.to(dt)), (i, path, dt)
            # 3. target: exact everywhere
            assert torch.equal(t[0].cpu(), C.target_of(lab, rec, P)) and torch.equal(t, tq)


# ------------------------------------------------------------------------------------------------- alignment and bounds
def test_alignment_ragged_batch_and_canaries():
    """sources at all four byte alignments, samples of different shapes in one launch, canaries around both outputs, the staged
    and the direct path on the same bits"""
    from ifseg_amd import hip
    dev = _dev()
    P = 64
    imgs, labs = C.ragged_batch()
    B = len(imgs)
    params = A.draw_params([tuple(l.shape) for l in labs], labs, P, C.NSEG, 21, 1000)
    want = A.train_load_reference(imgs, labs, params, P, C.NSEG, C.SEG0, dtype=torch.float32)
    base = None
    N, NT = B * 3 * P * P, B * (P * P + 1)
    for shift in range(4):
        views_i, views_l = [], []
        for b, (img, lab) in enumerate(zip(imgs, labs)):
            bi = torch.zeros(img.numel() + 8, dtype=torch.uint8, device=dev)
            bl = torch.zeros(lab.numel() + 8, dtype=torch.uint8, device=dev)
            s = (shift + b) % 4
            vi, vl = bi[s:s + img.numel()].view(img.shape), bl[s:s + lab.numel()].view(lab.shape)
            vi.copy_(img.to(dev)); vl.copy_(lab.to(dev))
            assert vi.data_ptr() % 4 == (bi.data_ptr() + s) % 4
            views_i.append(vi); views_l.append(vl)
        for path, sb in PATHS.items():
            for dt in (torch.float32, torch.bfloat16):
                buf = torch.full((N + 64,), 7.0, dtype=dt, device=dev)
                tbuf = torch.full((NT + 16,), -5, dtype=torch.int64, device=dev)
                out, tgt = buf[32:32 + N].view(B, 3, P, P), tbuf[8:8 + NT].view(B, P * P + 1)
                assert out.data_ptr() % 16 == 0
                o, t = hip.train_load(views_i, views_l, params.to(dev), P, C.NSEG, C.SEG0, dtype=dt, staging_bytes=sb, out=out,
                                      target=tgt)
                assert o is out and t is tgt
                assert buf[:32].eq(7).all() and buf[32 + N:].eq(7).all() and tbuf[:8].eq(-5).all() and tbuf[8 + NT:].eq(-5).all()
                assert torch.equal(tgt.cpu(), want[1])
                if dt == torch.float32:
                    if base is None:
                        base = out.clone()
                        _check_against_own_grey_levels(views_i, views_l, imgs, labs, params, base, want, P, dev)
                    assert torch.equal(out, base), (shift, path)
                else:
                    assert torch.equal(out, base.to(torch.bfloat16)), (shift, path)


def _check_against_own_grey_levels(di, dl, imgs, labs, params, out, want, P, dev):
    """general ratios: the grey levels in front of the photometric stage are within one level of the fp32 specification's (FMA
    contraction and summation order move a value across at most the one rounding boundary next to it), and the output is the
    photometric stage of the device's OWN grey levels, through the table, bit for bit"""
    from ifseg_amd import hip
    from ifseg_amd.imageio import normalisation_table
    plain = params.clone()
    plain[:, A.R_BRIGHT:A.R_HUE + 1] = 0
    q0 = IC.q_of(hip.train_load(di, dl, plain.to(dev), P, C.NSEG, C.SEG0, IC.Q_MEAN, IC.Q_STD)[0]).cpu().permute(0, 2, 3, 1)
    off = q0 != want[3]
    print("%d of %d grey levels off the fp32 specification" % (int(off.sum()), off.numel()))
    assert (q0.int() - want[3].int()).abs().max().item() <= 1
    lut = normalisation_table()
    for b in range(len(imgs)):
        q = torch.from_numpy(A.photometric(q0[b].numpy(), params[b].tolist())).permute(2, 0, 1).long()
        assert torch.equal(out[b].cpu(), torch.stack([lut[c][q[c]] for c in range(3)])), b


def test_entry_point_refusals():
    """error codes only, nothing launched"""
    from ifseg_amd import hip
    dev = _dev()
    lib = hip.lib()
    P = 32
    img = torch.zeros(40, 48, 3, dtype=torch.uint8, device=dev)
    lab = torch.ones(40, 48, dtype=torch.uint8, device=dev)
    host, table = hip._train_table([img], [lab])
    out = torch.full((3 * P * P + 64,), 3.0, device=dev)
    tgt = torch.full((P * P + 9,), -5, dtype=torch.int64, device=dev)
    lut = torch.zeros(3, 256, device=dev)
    good = torch.tensor([C.record(40, 48, 8, 16)], dtype=torch.int32)
    params = torch.full((1, 16), -9, dtype=torch.int32, device=dev)
    i, ll, u64 = ctypes.c_int, ctypes.c_longlong, ctypes.c_uint64
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None

    def load(th=host, td=table, pd=good.to(dev), phost=good, B=1, P=P, nseg=5, lu=lut, o=out, ob=4, t=tgt):
        return lib.ifseg_train_load(p(th), p(td), p(pd), p(phost), i(B), i(P), i(nseg), i(1), ll(C.SEG0), ll(2), p(lu), i(0), p(o),
                                    i(ob), p(t), None)

    def draw(th=host, td=table, B=1, P=P, nseg=5, first=0, lo2=1, span2=3, pr=params):
        return lib.ifseg_train_draw(p(th), p(td), i(B), i(P), i(nseg), i(1), u64(1), ll(first), i(lo2), i(span2), i(3), p(pr), None)

    assert load(th=None) == -3 and load(td=None) == -3 and load(pd=None) == -3 and load(lu=None) == -3 and load(o=None) == -3
    assert load(t=None) == -3 and load(ob=1) == -3 and load(nseg=0) == -3 and load(nseg=256) == -3
    assert load(o=out[1:]) == -3 and load(o=out[2:], ob=2) == -3                       # 16-byte aligned output
    assert load(P=40) == -2 and load(P=8) == -2 and load(P=8192) == -2 and load(B=0) == -2
    bad = lambda **kw: torch.tensor([C.record(**dict(dict(new_h=40, new_w=48, off_h=8, off_w=16), **kw))], dtype=torch.int32)
    assert load(phost=bad(new_h=31)) == -2 and load(phost=bad(new_w=31)) == -2        # no window
    assert load(phost=bad(off_h=9)) == -2 and load(phost=bad(off_w=-1)) == -2         # a window outside the resized image
    assert load(phost=bad(new_h=2 ** 25, off_h=0)) == -2                               # 2 in out >= 2^31
    nul = host.clone()
    nul[0, 0] = 0
    assert load(th=nul) == -3                                                          # a null image pointer in the table
    nul = host.clone()
    nul[0, 2] = 0 | (48 << 32)
    assert load(th=nul) == -2                                                          # H0 = 0
    assert draw(th=None) == -3 and draw(td=None) == -3 and draw(pr=None) == -3 and draw(nseg=0) == -3
    assert draw(first=-1) == -3 and draw(first=2 ** 32) == -3 and draw(lo2=-1) == -3 and draw(lo2=60, span2=5) == -3
    assert draw(P=40) == -2 and draw(B=0) == -2
    tall = host.clone()
    tall[0, 2] = 2 ** 16 | (1 << 32)
    assert draw(th=tall) == -2                                                         # 2 in out >= 2^31 at the largest size
    torch.cuda.synchronize()
    assert out.eq(3).all() and tgt.eq(-5).all() and params.eq(-9).all()               # nothing was launched
    assert draw() == 0 and load(phost=None) == 0 and load() == 0
    torch.cuda.synchronize()
    assert params[0, 15] == 0 and params[0, 0] >= P
    # through the binding: RuntimeError with the code; records on the host are checked before they travel
    with pytest.raises(RuntimeError, match="train_load failed with code -2"):
        hip.train_load([img], [lab], bad(new_h=31), P, 5, C.SEG0)
    with pytest.raises(RuntimeError, match="train_draw failed with code -2"):
        hip.train_draw([lab], 40, 5, 1, 0)
    # the same record from device memory poisons its sample and nothing else
    two = torch.cat([bad(new_h=31), good]).to(dev)
    o, t = hip.train_load([img, img], [lab, lab], two, P, 5, C.SEG0)
    assert torch.isnan(o[0]).all() and t[0, :-1].eq(-1).all() and torch.isfinite(o[1]).all() and t[1, :-1].eq(C.SEG0).all()
    # the staging switch returns the previous limit, and the binding restores it
    prev = lib.ifseg_train_load_staging(i(1000))
    assert prev > 60000 and lib.ifseg_train_load_staging(i(-1)) == 1000 and lib.ifseg_train_load_staging(i(prev)) == prev
    hip.train_load([img], [lab], good, P, 5, C.SEG0, staging_bytes=0)
    assert lib.ifseg_train_load_staging(i(prev)) == prev
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- the op
def test_op_matches_binding_and_opcheck():
    from ifseg_amd import hip
    from ifseg_amd.imageio import IMAGENET_DEFAULT_MEAN as M, IMAGENET_DEFAULT_STD as S
    dev = _dev()
    P = 64
    imgs, labs = C.ragged_batch()
    di, dl = _to(imgs, dev), _to(labs, dev)
    params = hip.train_draw(dl, P, C.NSEG, 8, 50)
    op = torch.ops.ifseg.train_load
    for dt in (torch.float32, torch.bfloat16):
        o, t = op(di, dl, params, P, C.NSEG, C.SEG0, list(M), list(S), True, True, dt)
        wo, wt = hip.train_load(di, dl, params, P, C.NSEG, C.SEG0, M, S, True, True, dt)
        assert o.dtype == dt and torch.equal(o, wo) and torch.equal(t, wt)
    # a non-contiguous view is copied, not refused
    nc = di[0].transpose(0, 1).contiguous().transpose(0, 1)
    assert not nc.is_contiguous()
    ref_o, ref_t = hip.train_load(di, dl, params, P, C.NSEG, C.SEG0)
    o, t = op([nc] + di[1:], dl, params, P, C.NSEG, C.SEG0, [0.5] * 3, [0.5] * 3, False, True, torch.float32)
    assert torch.equal(o, ref_o) and torch.equal(t, ref_t)
    with pytest.raises((ValueError, RuntimeError), match="label maps must be uint8"):
        op(di, [dl[0][:-1]] + dl[1:], params, P, C.NSEG, C.SEG0, [0.5] * 3, [0.5] * 3, False, True, torch.float32)
    utils = ("test_schema", "test_autograd_registration", "test_faketensor")
    torch.library.opcheck(op, (di, dl, params, P, C.NSEG, C.SEG0, [0.5] * 3, [0.5] * 3, True, True, torch.float32), test_utils=utils)
    torch.library.opcheck(op, (di[:1], dl[:1], params[:1], P, C.NSEG, C.SEG0, list(M), list(S), False, False, torch.bfloat16),
                          test_utils=utils)
    # on a side stream the op follows PyTorch's current stream
    st2 = torch.cuda.Stream()
    st2.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st2):
        o3, t3 = op(di, dl, params, P, C.NSEG, C.SEG0, [0.5] * 3, [0.5] * 3, False, True, torch.float32)
    st2.synchronize()
    assert torch.equal(o3, ref_o) and torch.equal(t3, ref_t)


# ------------------------------------------------------------------------------------------------- end to end
def test_train_sample_through_one_training_step():
    """segofa_tiny at P = 128 (the fixture of _predict_cases): one Trainer.train_step on task.train_sample(...) from
    exact-family sources (32 x 48 and 48 x 32 at ratio 1: x4) -- a finite loss, the label check silent, and bit for bit the
    loss of the step from the same state on the tensors the CPU specification produced"""
    import segofa_ref as O  # noqa: F401  (the fixture's oracle: on the path through conftest)
    from ifseg_amd.criterions import SegCriterion
    from ifseg_amd.models.segofa import SegOFAModel, make_config
    from ifseg_amd.tasks.mm_tasks import SegmentationTask
    from ifseg_amd.trainer import Trainer
    dev = _dev()
    ocfg, sd, _, src = PC.e2e_fixture()
    P = ocfg.patch_image_size
    assert P == 128

    def task_on(device):
        task = SegmentationTask(num_seg_tokens=ocfg.num_seg_tokens, patch_image_size=P, n_base_vocab=ocfg.vocab_size - 1,
                                category_token_ids=PC.E2E_NAMES)
        assert task.seg_id_offset == ocfg.seg_id_offset
        task.prompt_ids = PC.E2E_PROMPT
        task.build_train_transform(device, seed=6, ratio_range=(1, 1))
        return task

    def step(task, sample):
        m = SegOFAModel(make_config("segofa_tiny", embed_dim=ocfg.embed_dim, ffn_dim=ocfg.ffn_dim, heads=ocfg.heads,
                                    enc_layers=ocfg.enc_layers, dec_layers=ocfg.dec_layers, resnet_layers=ocfg.resnet_layers,
                                    num_seg_tokens=ocfg.num_seg_tokens, vocab_size=ocfg.vocab_size, patch_image_size=P,
                                    orig_patch_image_size=ocfg.orig_patch_image_size))
        torch.nn.Module.load_state_dict(m, sd, strict=False)
        m.cfg.dropout = m.cfg.encoder_drop_path_rate = m.cfg.decoder_drop_path_rate = 0.0
        tr = Trainer(m.to(dev), SegCriterion(task, unsupervised_segmentation=False, init_seg_with_text=False), task, device=dev)
        loss = float(tr.train_step([sample])[0]["loss"])
        tr.check_overflow(wait=True)
        torch.cuda.synchronize()
        return loss

    imgs = [C.image(32, 48, 1), C.image(48, 32, 2)]
    labs = [C.label("mixed", 32, 48), C.label("random", 48, 32)]
    gpu, cpu = task_on(dev), task_on("cpu")
    s = gpu.train_sample(imgs, labs, 4)
    ref = cpu.train_sample(imgs, labs, 4)
    assert s["net_input"]["patch_images"].is_cuda and s["target"].is_cuda
    assert torch.equal(s["net_input"]["src_tokens"][0].cpu(), src)
    assert torch.equal(s["net_input"]["patch_images"].cpu(), ref["net_input"]["patch_images"])
    assert torch.equal(s["target"].cpu(), ref["target"])
    again = gpu.train_sample(imgs, labs, 4)
    assert torch.equal(again["net_input"]["patch_images"], s["net_input"]["patch_images"]) and torch.equal(again["target"], s["target"])
    nxt = gpu.train_sample(imgs, labs, 6)
    assert not torch.equal(nxt["net_input"]["patch_images"], s["net_input"]["patch_images"])

    def to_dev(x):
        if isinstance(x, dict):
            return {k: to_dev(v) for k, v in x.items()}
        return x.to(dev) if isinstance(x, torch.Tensor) else x

    loss = step(gpu, s)
    print("loss of the step on the device's batch: %r" % loss)
    assert np.isfinite(loss)
    assert loss == step(cpu, to_dev(ref))
