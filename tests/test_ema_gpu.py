"""GPU: hip.adam_ema_step and hip.ema_swap (csrc/optim.hip) against the specification of ifseg_amd/ema.py and against
hip.adam_step, bit for bit and between canaries; Trainer(store_ema=True) through its three optimizer paths against a host replay
of the specification; the teacher in use (`ema_weights`, `ema_state_dict`, `task.self_train_sample(trainer=)`) on the segofa_tiny
fixture.  Every comparison is exact."""
import pytest
import torch

import _predict_cases as PC

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 4, 5, 8, 1027, 512 * 256 * 4 + 1027)       # the last: one full grid-stride sweep, then 1024 + a tail of 3
OFFSETS = (0, 8, 24)                                      # the deferred optimizer's slices start at multiples of 8 elements
DECAYS = (0.0, 0.5, 0.9999)
LR, B1, B2, EPS, WD, STEP = 1e-3, 0.9, 0.999, 1e-8, 0.1, 3


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same(a, b):
    return a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def wide(n, g):
    """magnitudes from 1e-30 to 1e30, zeros of both signs and subnormals in front (as many as fit)"""
    x = torch.randn(n, generator=g) * torch.exp(torch.randn(n, generator=g) * 20).clamp(1e-30, 1e30)
    special = torch.tensor([-0.0, 0.0, 1e-39, -3e-40, 1e30, -1e-30])
    k = min(n, special.numel())
    idx = torch.randperm(n, generator=g)[:k]
    x[idx] = special[:k]
    return x


def arena(values, off, dev):
    """-> (buffer, view): `values` at element `off` of a buffer of canaries (in front when off > 0, 16 behind)"""
    canary = 7.25 if values.dtype == torch.float32 else -3.5
    buf = torch.full((off + values.numel() + 16,), canary, dtype=values.dtype)
    buf[off:off + values.numel()] = values
    buf = buf.to(dev)
    return buf, buf[off:off + values.numel()]


def make_case(n, off, seed, dev):
    g = torch.Generator().manual_seed(seed)
    host = {"p32": wide(n, g), "g": torch.randn(n, generator=g).to(torch.bfloat16), "m": torch.randn(n, generator=g) * 0.1,
            "v": torch.rand(n, generator=g) * 0.01, "e32": wide(n, g)}
    host["p16"] = host["p32"].to(torch.bfloat16)
    host["e16"] = host["e32"].to(torch.bfloat16)
    return {k: arena(v, off, dev) for k, v in host.items()}


def clone_case(case):
    out = {}
    for k, (buf, view) in case.items():
        b = buf.clone()
        off = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
        out[k] = (b, b[off:off + view.numel()])
    return out


def launch(case, ema, decay_rest, mode, dev, sumsq_value=None):
    """one optimizer launch; mode bit 0: clipping active, bit 1: the scalars through `hyper` (by-value ones are then decoys)"""
    from ifseg_amd import hip
    clip, by_hyper = bool(mode & 1), bool(mode & 2)
    sumsq = torch.tensor([1e4 if clip else 1e-4] if sumsq_value is None else [sumsq_value], dtype=torch.float32, device=dev)
    overflow = torch.zeros(1, dtype=torch.int32, device=dev)
    gscale, max_norm = 0.5, (1.0 if clip or mode & 4 else 0.0)
    hyper, lr, (d, r) = None, LR, decay_rest or (1.0, 0.0)
    if by_hyper:
        hyper = torch.tensor([LR, 1.0 - B1 ** STEP, 1.0 - B2 ** STEP, gscale, d, r], dtype=torch.float32, device=dev)
        lr, gscale, d, r = 0.123, 77.0, 0.25, 0.125
    v = {k: case[k][1] for k in case}
    if ema:
        hip.adam_ema_step(v["p32"], v["g"], v["m"], v["v"], v["p16"], v["e32"], v["e16"], lr, B1, B2, EPS, WD, STEP, d, r,
                          gscale, max_norm, sumsq, overflow, hyper=hyper)
    else:
        hip.adam_step(v["p32"], v["g"], v["m"], v["v"], v["p16"], lr, B1, B2, EPS, WD, STEP, gscale, max_norm, sumsq, overflow,
                      hyper=hyper)
    return overflow


@pytest.mark.parametrize("n", SIZES)
def test_adam_ema_step_is_adam_step_and_the_specification(n):
    """(p32, m, v, p16) bit-equal to hip.adam_step on copies of the same inputs (clip active / inactive, scalars by value /
    through `hyper`), (e32, e16) bit-equal to `ema_reference(e32 before, p16 after, decay)`, canaries intact"""
    from ifseg_amd.ema import ema_reference, ema_scalars
    dev = _dev()
    k = 0
    for off in OFFSETS:
        for decay in DECAYS:
            mode, k = k % 4, k + 1
            case = make_case(n, off, 1000 * n + 10 * off + k, dev)
            plain, fused = clone_case(case), clone_case(case)
            launch(plain, False, None, mode, dev)
            ovf = launch(fused, True, ema_scalars(decay), mode, dev)
            torch.cuda.synchronize()
            assert int(ovf) == 0
            for name in ("p32", "m", "v", "p16", "g"):
                assert same(fused[name][0], plain[name][0]), (name, off, decay, mode)
            assert not same(fused["p32"][1], case["p32"][1])                       # the update happened
            want32, want16 = ema_reference(case["e32"][1].cpu(), fused["p16"][1].cpu(), decay)
            for name, want in (("e32", want32), ("e16", want16)):
                whole = case[name][0].clone()
                whole[off:off + n] = want.to(dev)
                bad = (bits(fused[name][0]) != bits(whole)).nonzero().flatten()
                assert bad.numel() == 0, (name, off, decay, mode, bad[:8].tolist())


def test_decay_one_rest_zero_leaves_the_teacher_alone():
    dev = _dev()
    n = 1027
    for mode in (0, 2):                                  # by value, and as a captured step reads it
        case = make_case(n, 8, 77 + mode, dev)
        plain, fused = clone_case(case), clone_case(case)
        fused["e32"][1][5] = float("nan")                # bytes, not values: e * 1 + 0 * q would quieten nothing here, but be sure
        before32, before16 = fused["e32"][0].clone(), fused["e16"][0].clone()
        launch(plain, False, None, mode, dev)
        launch(fused, True, (1.0, 0.0), mode, dev)
        torch.cuda.synchronize()
        for name in ("p32", "m", "v", "p16"):
            assert same(fused[name][0], plain[name][0]), name
        assert same(fused["e32"][0], before32) and same(fused["e16"][0], before16)


def test_non_finite_norm_skips_student_and_teacher():
    dev = _dev()
    case = make_case(1027, 8, 91, dev)
    fused = clone_case(case)
    ovf = launch(fused, True, (0.5, 0.5), 4, dev, sumsq_value=float("inf"))
    torch.cuda.synchronize()
    assert int(ovf) == 1
    for name in case:
        assert same(fused[name][0], case[name][0]), name


@pytest.mark.parametrize("n", SIZES)
def test_ema_swap_exchanges_every_bit(n):
    from ifseg_amd import hip
    dev = _dev()
    for off in OFFSETS:
        case = make_case(n, off, 5000 + n + off, dev)
        work = clone_case(case)
        w = {k: work[k][1] for k in work}
        hip.ema_swap(w["p32"], w["p16"], w["e32"], w["e16"])
        torch.cuda.synchronize()
        for a, b in (("p32", "e32"), ("e32", "p32"), ("p16", "e16"), ("e16", "p16")):
            whole = case[a][0].clone()
            whole[off:off + n] = case[b][1]
            assert same(work[a][0], whole), (a, off)
        hip.ema_swap(w["p32"], w["p16"], w["e32"], w["e16"])
        torch.cuda.synchronize()
        for name in ("p32", "p16", "e32", "e16"):
            assert same(work[name][0], case[name][0]), (name, off)


# ------------------------------------------------------------------------------------------------- the Trainer
@pytest.fixture(scope="module")
def runs():
    """six updates of segofa_tiny (P = 128, 5 classes, B = 2, lr 1e-3, dropout as configured) over three synthetic samples,
    copied into one resident batch: without a teacher, with one (single launch, p16 kept after every update), with the
    deferred optimizer, and captured from the third update on"""
    from ifseg_amd.criterions import SegCriterion
    from ifseg_amd.tasks.mm_tasks import SegmentationTask
    from ifseg_amd.trainer import Trainer
    dev = _dev()
    task = SegmentationTask(num_seg_tokens=5, patch_image_size=128, arch="segofa_tiny")
    samples = [task.synthetic_sample(2, dev, seed=s) for s in range(3)]
    ema_kw = dict(store_ema=True, ema_decay=0.5, ema_start_update=2, ema_update_freq=2)

    def fill(dst, src):
        for k, v in src.items():
            if isinstance(v, dict):
                fill(dst[k], v)
            elif torch.is_tensor(v):
                dst[k].copy_(v)

    def run(ema=True, defer=False, graph_from=99, keep=False):
        torch.manual_seed(0)
        tr = Trainer(task.build_model(), SegCriterion(task, unsupervised_segmentation=False, init_seg_with_text=False), task,
                     lr=1e-3, device=dev, **(ema_kw if ema else {}))
        resident = task.synthetic_sample(2, dev, seed=0)
        n = tr.eng.n_train
        first = tuple(t.clone().cpu() for t in (tr.ema.e32, tr.ema.e16, tr.p32, tr.eng.p16[:n])) if ema else None
        losses, logs, snaps = [], [], []
        for k in range(6):
            fill(resident, samples[k % 3])
            lg = tr.train_step([resident], graph=k >= graph_from, defer_optimizer=defer)[0]
            losses.append(lg["loss"])
            logs.append(lg)
            if keep:
                snaps.append(tr.eng.p16[:n].clone())
        tr.params_ready()
        tr.check_overflow(wait=True)
        torch.cuda.synchronize()
        out = {"p32": tr.p32.clone(), "m": tr.m.clone(), "v": tr.v.clone(), "p16": tr.eng.p16.clone(),
               "losses": [float(x) for x in losses], "logs": logs, "snaps": [s.cpu() for s in snaps], "first": first,
               "graphs": len(tr._graphs), "own_stream": getattr(tr, "_opt_stream", None) is not None}
        if ema:
            out["e32"], out["e16"] = tr.ema.e32.clone(), tr.ema.e16.clone()
        tr.close()
        return out
    return {"off": run(ema=False), "eager": run(keep=True), "defer": run(defer=True), "graph": run(graph_from=2)}


def test_store_ema_leaves_the_student_alone(runs):
    off, on = runs["off"], runs["eager"]
    for name in ("p32", "m", "v", "p16"):
        assert same(on[name], off[name]), name
    assert on["losses"] == off["losses"] and len(set(on["losses"])) == 6
    assert all("ema_decay" not in lg for lg in off["logs"])
    assert [lg["ema_decay"] for lg in on["logs"]] == [0.0, 0.5, 0.5, 0.5, 0.5, 0.5]      # updates 1..6, ema_start_update = 2


def test_teacher_is_the_host_replay_of_the_specification(runs):
    """ema_update_freq = 2: the teacher steps after updates 2, 4 and 6, towards the bf16 weights of that update"""
    from ifseg_amd.ema import ema_decay_at, ema_reference
    on = runs["eager"]
    e32, e16, p32_first, p16_first = on["first"]
    assert same(e32, p32_first) and same(e16, p16_first)   # seeded as a copy of the student (nothing lazy in this criterion)
    for k, p16 in enumerate(on["snaps"]):
        updates = k + 1
        if updates % 2 == 0:
            e32, e16 = ema_reference(e32, p16, ema_decay_at(updates, 0.5, 2))
    assert same(on["e32"].cpu(), e32) and same(on["e16"].cpu(), e16)
    assert not same(on["e16"].cpu(), on["snaps"][-1])      # a teacher, not a copy of the last student


@pytest.mark.parametrize("path", ["defer", "graph"])
def test_deferred_and_captured_optimizers_keep_student_and_teacher(runs, path):
    """the per-slice launches on the optimizer's stream, and ONE capture replayed over on- and off-updates of ema_update_freq
    (the decay pair travels in the hyper row: (1, 0) on the off-updates): bit-equal to the single eager launch"""
    a, b = runs["eager"], runs[path]
    for name in ("p32", "m", "v", "p16", "e32", "e16"):
        assert same(a[name], b[name]), name
    assert a["losses"] == b["losses"]
    assert b["graphs"] == (1 if path == "graph" else 0) and b["own_stream"] == (path == "defer")
    assert a["graphs"] == 0 and not a["own_stream"]


# ------------------------------------------------------------------------------------------------- the teacher in use
@pytest.fixture(scope="module")
def taught():
    """the segofa_tiny fixture with its photographs, trained for three updates on its own pseudo-labels with ema_decay = 0.5;
    a second model loaded from `ema_state_dict()`"""
    from ifseg_amd.criterions import SegCriterion
    from ifseg_amd.models.segofa import SegOFAModel, make_config
    from ifseg_amd.tasks.mm_tasks import SegmentationTask
    from ifseg_amd.trainer import Trainer
    dev = _dev()
    ocfg, sd, img, src = PC.e2e_fixture()
    P, n = ocfg.patch_image_size, ocfg.num_seg_tokens
    base = ((img * 0.5 + 0.5) * 255).round().clamp(0, 255)
    raw = [torch.nn.functional.interpolate(base[k % 2:k % 2 + 1], size=s, mode="bilinear", align_corners=False)[0]
           .round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous() for k, s in enumerate([(60, 90), (90, 60), (64, 64)])]
    task = SegmentationTask(num_seg_tokens=n, patch_image_size=P, n_base_vocab=ocfg.vocab_size - 1, category_token_ids=PC.E2E_NAMES)
    task.prompt_ids = PC.E2E_PROMPT
    task.build_train_transform(dev, seed=6, ratio_range=(1, 1))

    def model(state):
        m = SegOFAModel(make_config("segofa_tiny", embed_dim=ocfg.embed_dim, ffn_dim=ocfg.ffn_dim, heads=ocfg.heads,
                                    enc_layers=ocfg.enc_layers, dec_layers=ocfg.dec_layers, resnet_layers=ocfg.resnet_layers,
                                    num_seg_tokens=n, vocab_size=ocfg.vocab_size, patch_image_size=P,
                                    orig_patch_image_size=ocfg.orig_patch_image_size))
        missing = torch.nn.Module.load_state_dict(m, state, strict=False)
        m.cfg.dropout = m.cfg.encoder_drop_path_rate = m.cfg.decoder_drop_path_rate = 0.0
        return m.to(dev), missing
    m, _ = model(sd)
    kw = dict(prompt_ids=PC.E2E_PROMPT, keep=0.5, boundary=1)
    tr = Trainer(m, SegCriterion(task, unsupervised_segmentation=False, init_seg_with_text=False), task, lr=1e-3, device=dev,
                 store_ema=True, ema_decay=0.5)
    for k in range(3):
        tr.train_step([task.self_train_sample(m, raw, 4 + 3 * k, **kw)])
    tr.check_overflow(wait=True)
    esd = tr.ema_state_dict()
    assert set(esd) == set(m.state_dict())
    m2, missing = model(esd)
    assert not missing.missing_keys and not missing.unexpected_keys
    return tr, m, m2, raw, task, kw


def _segment(m, raw):
    from ifseg_amd.predict import Segmenter
    res = Segmenter(m, category_token_ids=PC.E2E_NAMES, prompt_ids=PC.E2E_PROMPT).segment_raw(raw, return_conf=True)
    return [(r.labels.clone(), r.conf.clone()) for r in res]


def test_ema_weights_is_the_model_of_ema_state_dict_and_the_student_returns(taught):
    tr, m, m2, raw, task, kw = taught
    before = _segment(m, raw)                              # (a non-square photograph first: a resized-bias cache entry exists)
    student_p16, student_p32 = tr.eng.p16.clone(), tr.p32.clone()
    want = _segment(m2, raw)
    with tr.ema_weights() as inside:
        assert inside is tr
        got = _segment(m, raw)
        assert not same(tr.eng.p16, student_p16)
        with pytest.raises(RuntimeError, match="train_step inside"):
            tr.train_step([task.synthetic_sample(2, tr.device)])
        with pytest.raises(RuntimeError, match="inside"):
            with tr.ema_weights():
                pass
        with pytest.raises(RuntimeError, match="inside"):
            tr.ema_state_dict()
    after = _segment(m, raw)
    torch.cuda.synchronize()
    assert same(tr.eng.p16, student_p16) and same(tr.p32, student_p32)
    for (gl, gc), (wl, wc), (bl, bc), (al, ac) in zip(got, want, before, after):
        assert torch.equal(gl, wl) and same(gc, wc)        # the teacher, as a model of its own computes it
        assert torch.equal(al, bl) and same(ac, bc)        # the student is back: a stale bias of the teacher would show here
    assert any(not same(gc, bc) for (_, gc), (_, bc) in zip(got, before))       # teacher and student differ at all


def test_ema_state_dict_round_trip_and_refusals(taught):
    from ifseg_amd.criterions import SegCriterion
    from ifseg_amd.trainer import Trainer
    tr, m, m2, raw, task, kw = taught
    esd = tr.ema_state_dict()
    e32, e16 = tr.ema.e32.clone(), tr.ema.e16.clone()
    names = set(tr.eng.trainable_names())
    own = m.state_dict()
    for k in names:                                        # fp32 clones out of the teacher
        o = tr.eng.offs[k]
        assert esd[k].dtype == torch.float32 and same(esd[k].reshape(-1), e32[o:o + esd[k].numel()])
    shared = [k for k, v in esd.items() if v.data_ptr() == own[k].data_ptr()]
    assert shared and not names & set(shared)              # everything frozen is the model's own tensor
    tr.ema.e32.zero_()
    tr.ema.e16.zero_()
    tr.load_ema_state_dict(esd)
    torch.cuda.synchronize()
    assert same(tr.ema.e32, e32) and same(tr.ema.e16, e16) and not tr.ema.fresh
    plain = Trainer(m2, SegCriterion(task, unsupervised_segmentation=False, init_seg_with_text=False), task, device=tr.device)
    for call in (lambda: plain.ema_weights().__enter__(), plain.ema_state_dict, lambda: plain.load_ema_state_dict(esd)):
        with pytest.raises(RuntimeError, match="store_ema=False"):
            call()


def test_self_train_sample_labels_with_the_teacher(taught):
    tr, m, m2, raw, task, kw = taught
    got = task.self_train_sample(m, raw, 4, trainer=tr, **kw)
    pseudo = task.pseudo_label_raw(m2, raw, **kw)
    want = task.train_sample(raw, [r.labels for r in pseudo], 4)
    assert torch.equal(got["target"], want["target"])
    assert torch.equal(got["net_input"]["patch_images"], want["net_input"]["patch_images"])
    # without the trainer: today's result, the student's own labels
    alone = task.self_train_sample(m, raw, 4, **kw)
    mine = task.train_sample(raw, [r.labels for r in task.pseudo_label_raw(m, raw, **kw)], 4)
    assert torch.equal(alone["target"], mine["target"])
    assert torch.equal(alone["net_input"]["patch_images"], mine["net_input"]["patch_images"])
    with pytest.raises(ValueError, match="another model"):
        task.self_train_sample(m2, raw, 4, trainer=tr, **kw)
