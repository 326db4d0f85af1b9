"""Conformance of the eleven post-processing kernels of csrc/crf.hip, csrc/resize.hip and csrc/evalops.hip through the C ABI
(ifseg_amd.hip), in the style of test_rowops_conformance_gpu.py: operands and outputs are views inside larger allocations, 7s
around the inputs, a sentinel around the outputs (row padding and class rows beyond C included) that must be bit-identical after
the call.  Data, fp64 references, the derived bounds and the case tables are in _post_cases.py (its docstring holds the
derivations); test_post_conformance_cpu.py checks them without a GPU.

Part A: ifseg_crf_bilateral (all six instantiations, ragged pixel tiles), ifseg_crf_spatial (exact), ifseg_crf_update,
        ifseg_crf_norm per element against fp64; rgb_dense_crf end to end at 13 x 21 pixels with 40 and 150 classes.
Part B: ifseg_resize_rows_bilinear and ifseg_resized_rel_bias per element against two dense fp64 interpolation matrices; the
        engine's evaluation path against the training path of models/segofa/resized.py on the segofa_tiny fixture.
Part C: ifseg_l2norm_rows_bf16, ifseg_topk_rows_f32 (exact, NaN first), ifseg_softmax_rows, ifseg_gather_mean (exact),
        ifseg_seg_eval (histograms exact, loss per block against fp64).
Part D: argument rejection (return codes only).
profiles/post_conformance.txt: the kernels seen in a trace of this file, the worst ratios, the wrong variants it catches.
"""
import ctypes

import numpy as np
import pytest
import torch

import _post_cases as pc
from test_gemm_conformance_gpu import (BAD_ARG, BAD_SHAPE, BF16, F32, GUARD, SENTINEL, _assert_surroundings, _bits, _dev,
                                       _flat_guarded, _guarded)  # noqa: F401

pytestmark = pytest.mark.gpu
I32, I64 = torch.int32, torch.int64
i, ll, f = ctypes.c_int, ctypes.c_longlong, ctypes.c_float


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _ids(cases):
    return [c["id"] for c in cases]


# ------------------------------------------------------------------------------------------------ plumbing
def _t(a, dtype=F32):
    """numpy values (representable in `dtype`) -> torch CPU tensor; fp32 values travel bit for bit"""
    if dtype in (I32, I64):
        return torch.from_numpy(np.array(a)).to(dtype)
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(dtype)


def _in(a, dev, dtype=F32):
    """a dense operand with 16 guard elements on both sides"""
    fill = int(GUARD) if dtype in (I32, I64) else GUARD
    return _flat_guarded(_t(a, dtype), dtype, dev, fill)[1]


def _in_rows(a, dev, ld, dtype=BF16, zero_to=None):
    """a [R, C] operand as rows `ld` elements apart inside [3 + R + 2, ld] of 7s (columns [C, zero_to) zeroed)"""
    R, C = a.shape
    full = torch.full((3 + R + 2, ld), GUARD, dtype=dtype, device=dev)
    view = full[3:3 + R]
    if zero_to:
        view[:, C:zero_to] = 0
    view[:, :C] = _t(a, dtype).to(dev)
    return view


class _Out:
    """an output inside an allocation filled with the sentinel, the surroundings of which are compared bit for bit afterwards.
    ld: rows `ld` apart (the row padding belongs to the surroundings); alloc_rows: rows of the allocation the kernel is given
    (those beyond the logical ones belong to the surroundings as well); lead: leading dimensions in front of the rows"""

    def __init__(self, shape, dev, dtype=F32, ld=None, alloc_rows=None, zero=False):
        self.shape = tuple(shape)
        fill = int(SENTINEL) if dtype in (I32, I64) else SENTINEL
        if ld is None:
            self.full, self.view = _flat_guarded(self.shape, dtype, dev, fill)
            n = int(np.prod(self.shape))
            self.inner = lambda fl: fl[16:16 + n]
            self.arg = self.view
        else:
            lead, R, C = self.shape[:-2], self.shape[-2], self.shape[-1]
            RA = alloc_rows or R
            nl = int(np.prod(lead)) if lead else 1
            self.full = torch.full((16 + nl * RA * ld + 16,), fill, dtype=dtype, device=dev)
            body = lambda fl: fl[16:16 + nl * RA * ld].view(*lead, RA, ld)
            self.inner = lambda fl: body(fl)[..., :R, :C]
            self.view = self.inner(self.full)
            self.arg = body(self.full)[..., :C] if lead else body(self.full)          # what the binding is handed
        if zero:
            self.view.zero_()
        self.before = self.full.clone()

    def np(self):
        return self.view.double().cpu().numpy().reshape(self.shape)

    def check(self, what):
        _assert_surroundings(self.full, self.before, self.inner, what)


def _assert_within(what, out, ref, bound, got=None):
    got = out.np() if got is None else got
    r, at = pc.worst_ratio(got, ref, bound)
    print("[post] %s: worst |err|/bound %.3f at %s" % (what, r, at))
    assert r <= 1.0, "%s: |err| is %.3f of the bound at %s (got %r, ref %r)" % (what, r, at, got[at], ref[at])
    out.check(what)


def _assert_exact(what, out, ref):
    got = out.np()
    bad = got != ref
    assert not bad.any(), "%s: %d of %d elements differ; first at %s: got %r, expected %r" % (
        what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), got[bad][0], ref[bad][0])
    out.check(what)


# =========================================================================================================== part A
@pytest.mark.parametrize("case", pc.BILATERAL_CASES, ids=_ids(pc.BILATERAL_CASES))
def test_crf_bilateral(case):
    from ifseg_amd import hip
    dev = _dev()
    Cp, C, N, H, W, ldq = (case[k] for k in ("Cp", "C", "N", "H", "W", "ldq"))
    feat, gx, gy, _, _ = pc.bilateral_geometry(N)
    qn = _in_rows(pc.bilateral_qn(Cp, N, case["signed"]), dev, ldq, zero_to=(N + 63) // 64 * 64)
    out = _Out((Cp, N), dev)
    hip.crf_bilateral(_in(feat, dev), _in(gx, dev), _in(gy, dev), qn, out.view, H, W)
    torch.cuda.synchronize()
    ref, bound = pc.bilateral_ref(Cp, N, case["signed"])
    _assert_within("bilateral %s %s" % (case["id"], case["reach"]), out, ref, bound)
    assert not out.np()[C:].any(), "%s: a class row beyond C is not exactly zero" % case["id"]


@pytest.mark.parametrize("case", pc.SPATIAL_CASES, ids=_ids(pc.SPATIAL_CASES))
def test_crf_spatial(case):
    from ifseg_amd import hip
    dev = _dev()
    s = pc.spatial_case(case["R"], case["H"], case["W"], case["C"])
    out = _Out(s["q"].shape, dev)
    hip.crf_spatial(_in(s["q"], dev), _in(s["g"], dev), case["R"], out.view, case["H"], case["W"])
    torch.cuda.synchronize()
    _assert_exact("spatial " + case["id"], out, s["ref"])


@pytest.mark.parametrize("case", pc.UPDATE_CASES, ids=_ids(pc.UPDATE_CASES))
def test_crf_update(case):
    from ifseg_amd import hip
    dev = _dev()
    C, N = case["C"], case["N"]
    Cp, ldq = (C + 31) // 32 * 32, (N + 63) // 64 * 64 + case["extra_ld"]
    prob, mpos, mbi, npos, nbi = (_in(a, dev) for a in pc.update_inputs(C, N))
    if not case["msg"]:
        mpos = mbi = None
    if not case["norm"]:
        npos = nbi = None
    Q, qpos = _Out((C, N), dev), _Out((C, N), dev)
    qbi = _Out((C, N), dev, BF16, ld=ldq, alloc_rows=Cp)
    hip.crf_update(prob, mpos, mbi, npos, nbi, pc.WPOS, pc.WBI, Q.view, qpos.view, qbi.arg)
    torch.cuda.synchronize()
    ref = pc.update_ref(case)
    for name, out in (("Q", Q), ("qpos", qpos), ("qbi", qbi)):
        _assert_within("update %s %s" % (case["id"], name), out, ref[name], ref[name + "_b"])


def test_crf_norm():
    from ifseg_amd import hip
    dev = _dev()
    k1, ref, bound = pc.norm_case()
    out = _Out(k1.shape, dev)
    hip.crf_norm(_in(k1, dev), out.view)
    torch.cuda.synchronize()
    _assert_within("norm", out, ref, bound)


@pytest.mark.parametrize("case", pc.CRF_CASES, ids=_ids(pc.CRF_CASES))
def test_rgb_dense_crf_vs_exact_oracle(case):
    """N = 273 is no multiple of 64 and 40 / 150 classes take crf_bilateral_kernel<2> / <5>; the tolerances are those of
    test_dense_crf_meanfield_vs_exact_oracle, the argmax is compared where the oracle's top-2 gap is at least twice the value
    tolerance (test_post_conformance_cpu.py: all but 1 % of the pixels at most)"""
    import crf_ref
    from ifseg_amd.crf import rgb_dense_crf
    _dev()
    image, probs = pc.crf_inputs(case["h"], case["w"], case["c"], case["seed"])
    want = crf_ref.rgb_dense_crf_exact(np.array(image), np.array(probs), max_iter=case["iters"])
    got = torch.from_numpy(rgb_dense_crf(np.array(image), np.array(probs), max_iter=case["iters"]))
    assert got.shape == want.shape
    assert torch.allclose(got.sum(0), torch.ones(case["h"], case["w"]), atol=1e-4)
    top2 = want.double().topk(2, dim=0).values
    decided = (top2[0] - top2[1]) >= pc.CRF_GAP
    err = (got - want).abs().max().item()
    agree = (got.argmax(0) == want.argmax(0))[decided].float().mean().item()
    print("[post] dense CRF %s: max |dQ| %.4f, argmax agreement %.4f on %.1f %% decided pixels" % (case["id"], err, agree, 100 * decided.float().mean().item()))
    assert decided.float().mean().item() >= 1 - pc.MARGIN_CAP
    assert err <= pc.CRF_TOL and agree >= pc.CRF_AGREE


# =========================================================================================================== part B
@pytest.mark.parametrize("case", pc.ROWS_CASES, ids=_ids(pc.ROWS_CASES))
def test_resize_rows_bilinear(case):
    from ifseg_amd import hip
    dev = _dev()
    table = pc.rows_table(case["oh"], case["ow"], case["C"], case["stride"], case["off"], case["ints"])
    src = _in_rows(table, dev, case["ld_src"])[:, :case["C"]]
    out = _Out((case["h"] * case["w"], case["C"]), dev, BF16)
    hip.resize_rows_bilinear(src, out.view, case["h"], case["w"], case["oh"], case["ow"], case["stride"], case["off"])
    torch.cuda.synchronize()
    ref, bound = pc.rows_ref(case)
    if case["exact"]:
        _assert_exact("resize_rows " + case["id"], out, ref)
    _assert_within("resize_rows " + case["id"], out, ref, bound)


def _bias_out(case, dev):
    T = case["h"] * case["w"] + case["Lt"]
    return _Out((case["H"], T, T), dev, ld=(T + 3) // 4 * 4 if case["pad"] else T)


def _check_bias(what, out, ref, bound, exact):
    got = out.np()
    hidden = np.isneginf(ref)
    assert np.array_equal(np.isneginf(got), hidden), what + ": the -inf pattern differs"
    got, fin = np.where(hidden, 0.0, got), np.where(hidden, 0.0, ref)
    if exact:
        assert np.array_equal(got, fin), what + ": not bit-exact"
    tail = bound == 0
    assert np.array_equal(got[tail], fin[tail]), what + ": a tail value is not the table's"
    _assert_within(what, out, fin, bound, got=got)


@pytest.mark.parametrize("case", pc.BIAS_CASES, ids=_ids(pc.BIAS_CASES))
def test_resized_rel_bias(case):
    from ifseg_amd import hip
    dev = _dev()
    t2, r1, rx = pc.bias_tables(case["oh"], case["ow"], case["H"], case["Lt"], case["ints"])
    out = _bias_out(case, dev)
    hip.resized_rel_bias(out.arg, _in(t2, dev), _in(r1, dev) if case["tails"] else None, _in(rx, dev) if case["tails"] else None,
                         case["h"], case["w"], case["oh"], case["ow"], case["Lt"], causal=case["causal"])
    torch.cuda.synchronize()
    ref, bound = pc.bias_ref(case)
    if case["causal"] and case["Lt"] == 1:
        from ifseg_amd.models.segofa import resized
        assert np.array_equal(np.isneginf(ref[0]), resized.causal_mask(case["h"] * case["w"], torch.device("cpu")).numpy())
    _check_bias("resized_rel_bias " + case["id"], out, ref, bound, case["exact"])


def _tiny_model(dev):
    import segofa_ref as O
    from ifseg_amd.models.segofa import SegOFAModel, make_config
    ocfg = O.fixture_config()
    sd = O.procedural_state_dict(ocfg)
    m = SegOFAModel(make_config("segofa_tiny", embed_dim=ocfg.embed_dim, ffn_dim=ocfg.ffn_dim, heads=ocfg.heads, enc_layers=ocfg.enc_layers,
                                dec_layers=ocfg.dec_layers, resnet_layers=ocfg.resnet_layers, num_seg_tokens=ocfg.num_seg_tokens,
                                vocab_size=ocfg.vocab_size, patch_image_size=ocfg.patch_image_size,
                                orig_patch_image_size=ocfg.orig_patch_image_size))
    torch.nn.Module.load_state_dict(m, sd, strict=False)
    m.to(dev).eval()
    m.engine.pack(dev)
    return m


def _bias_bound(B0, h, w, oh, ow):
    """fp64 reference and bound of the grid block from the [H, P0, P0] gather on the trained grid"""
    M, mm = pc.interp2d(h, w, oh, ow)
    B0 = B0.double().cpu().numpy()
    ref = np.einsum("ia,hab,jb->hij", M, B0, M)
    A = np.abs(B0).reshape(B0.shape[0], -1).max(1)[:, None, None]
    return ref, 16 * pc.U * (mm[:, None] + mm[None, :])[None] * A + 16 * pc.U * np.einsum("ia,hab,jb->hij", np.abs(M), np.abs(B0), np.abs(M))


@pytest.mark.parametrize("hw", [(5, 11), (12, 6)], ids=["5x11", "12x6"])
def test_engine_resized_biases_against_the_training_path(hw):
    """engine._resized_biases (evaluation: csrc/resize.hip from the delta tables) and models/segofa/resized.py (training: torch
    ops on the gathered [H, P0, P0] bias) from the same weights: the grid block of both within the bound of the fp64 product
    Wq B0 Wk^T, the tail blocks identical, the causal pattern that of resized.causal_mask"""
    from ifseg_amd.models.segofa import resized as R
    dev = _dev()
    m = _tiny_model(dev)
    eng, cfg = m.engine, m.engine.cfg
    h, w = hw
    Pn, L = h * w, 5
    bufs = dict(m.named_buffers())
    oh, bsz, sb = cfg.orig_patch_image_size // 16, cfg.image_bucket_size, cfg.seg_bucket_size
    with torch.no_grad():
        got = eng._resized_biases("e", h, w, L, False).double().cpu().numpy()
        ids0 = R.grid_ids(oh, oh, bsz, dev)
        for l in range(cfg.enc_layers):
            tok = eng.W("encoder.token_rel_pos_table_list.%d.weight" % l).float()
            img = eng.W("encoder.image_rel_pos_table_list.%d.weight" % l).float()
            want = R.encoder_rel_bias(tok, img, bufs["encoder.token_rp_bucket"], bufs["encoder.image_rp_bucket"], (h, w), oh, bsz, L).double().cpu().numpy()
            B0 = img[bufs["encoder.image_rp_bucket"][ids0][:, ids0]].permute(2, 0, 1)
            ref, bound = _bias_bound(B0, h, w, oh, oh)
            for name, v in (("engine", got[l]), ("resized.py", want)):
                r, at = pc.worst_ratio(v[:, :Pn, :Pn], ref, bound)
                print("[post] encoder layer %d %dx%d %s: worst |err|/bound %.3f" % (l, h, w, name, r))
                assert r <= 1.0, (name, l, r, at)
            assert np.array_equal(got[l][:, Pn:], want[:, Pn:]) and np.array_equal(got[l][:, :Pn, Pn:], want[:, :Pn, Pn:]), "encoder tails, layer %d" % l
        hidden = R.causal_mask(Pn, dev).cpu().numpy()
        for causal in (False, True):
            got = eng._resized_biases("d", h, w, 1, causal).double().cpu().numpy()
            for l in range(cfg.dec_layers):
                seg = eng.W("decoder.seg_rel_pos_table_list.%d.weight" % l).float()
                want = R.decoder_rel_bias(seg, bufs["decoder.seg_rp_bucket"], (h, w), sb).double().cpu().numpy()
                g = got[l]
                if causal:
                    assert np.array_equal(np.isneginf(g), np.broadcast_to(hidden, g.shape)), "decoder causal pattern, layer %d" % l
                    g, want = np.where(hidden, 0.0, g), np.where(hidden, 0.0, want)
                else:
                    assert np.isfinite(g).all()
                B0 = seg[bufs["decoder.seg_rp_bucket"]].permute(2, 0, 1)[:, 1:, 1:]
                ref, bound = _bias_bound(B0, h, w, sb, sb)
                if causal:
                    ref = np.where(hidden[:Pn, :Pn], 0.0, ref)
                for name, v in (("engine", g), ("resized.py", want)):
                    r, at = pc.worst_ratio(v[:, :Pn, :Pn], ref, bound)
                    print("[post] decoder layer %d %dx%d causal %s %s: worst |err|/bound %.3f" % (l, h, w, causal, name, r))
                    assert r <= 1.0, (name, l, causal, r, at)
                assert np.array_equal(g[:, Pn:], want[:, Pn:]) and np.array_equal(g[:, :Pn, Pn:], want[:, :Pn, Pn:]), "decoder bos row / column, layer %d" % l


# =========================================================================================================== part C
@pytest.mark.parametrize("D", pc.L2_WIDTHS)
def test_l2norm_rows(D):
    from ifseg_amd import hip
    dev = _dev()
    x, ref, bound = pc.l2norm_case(D)
    out = _Out(x.shape, dev, BF16)
    assert hip.lib().ifseg_l2norm_rows_bf16(P(_in(x, dev, BF16)), P(out.view), i(pc.L2_ROWS), i(D), hip._stream()) == 0
    torch.cuda.synchronize()
    _assert_within("l2norm %d" % D, out, ref, bound)
    assert not out.np()[3].any(), "the all-zero row"


@pytest.mark.parametrize("N,k", pc.TOPK_CASES)
def test_topk_rows(N, k):
    """on its own: the index buffer is checked here and never handed to gather_mean"""
    from ifseg_amd import hip
    dev = _dev()
    rows = pc.topk_rows(N)
    out = _Out((pc.TOPK_ROWS, k), dev, I32)
    assert hip.lib().ifseg_topk_rows_f32(P(_in(rows, dev)), P(out.view), i(pc.TOPK_ROWS), i(N), i(k), hip._stream()) == 0
    torch.cuda.synchronize()
    got = out.view.cpu().numpy().astype(np.int64)
    assert got.min() >= 0 and got.max() < N and all(len(set(r)) == k for r in got), "an index outside the row or twice: %r" % got
    ref = pc.topk_ref(rows, k)
    assert np.array_equal(got, ref), "top-%d of %d: got %r, expected %r" % (k, N, got, ref)
    out.check("topk %d %d" % (N, k))


@pytest.mark.parametrize("case", pc.SOFTMAX_CASES, ids=_ids(pc.SOFTMAX_CASES))
def test_softmax_rows(case):
    from ifseg_amd import hip
    dev = _dev()
    n, rows = case["n"], case["rows"]
    x = pc.softmax_logits(n)
    ld = x.shape[2]
    out = _Out((rows, n), dev)
    assert hip.lib().ifseg_softmax_rows(P(_in(x, dev, BF16)), ll(pc.SOFTMAX_T * ld), i(pc.SOFTMAX_RPB), i(ld), P(out.view), i(rows), i(n),
                                        f(1.0 / case["temp"]), i(1 if case["softmax"] else 0), hip._stream()) == 0
    torch.cuda.synchronize()
    ref, bound = pc.softmax_ref(case)
    if case["softmax"]:
        _assert_within("softmax " + case["id"], out, ref, bound)
    else:
        _assert_exact("rows_to_f32 " + case["id"], out, ref)


def test_rows_to_f32_binding():
    """hip.rows_to_f32 on a padded [B, T, ld] tensor: the first rows of every sample"""
    from ifseg_amd import hip
    dev = _dev()
    n = 5
    x = pc.softmax_logits(n)
    pad = _in(x, dev, BF16)[:, :, :]
    got = hip.rows_to_f32(pad, n, 33).double().cpu().numpy()
    assert np.array_equal(got, x[:, :33, :n].astype(np.float64))
    got = hip.rows_to_f32(pad, n, 33, softmax=True, temperature=0.5).double().cpu().numpy()
    a = x[:, :33, :n].astype(np.float64) * 2
    e = np.exp(a - a.max(-1, keepdims=True))
    ref = e / e.sum(-1, keepdims=True)
    r, at = pc.worst_ratio(got, ref, (16 + 2 * n) * pc.U * ref)
    assert r <= 1.0, (r, at)


@pytest.mark.parametrize("k", pc.GATHER_KS)
def test_gather_mean(k):
    from ifseg_amd import hip
    dev = _dev()
    x, idx, ref = pc.gather_case(k)
    B, Pn, n = pc.GATHER_BPN
    assert idx.min() >= 0 and idx.max() < Pn
    out = _Out(x.shape, dev)
    assert hip.lib().ifseg_gather_mean(P(_in(x, dev)), P(_in(idx, dev, I32)), P(out.view), i(B), i(Pn), i(n), i(k), hip._stream()) == 0
    torch.cuda.synchronize()
    _assert_exact("gather_mean k %d" % k, out, ref.astype(np.float64))


@pytest.mark.parametrize("case", pc.EVAL_CASES, ids=_ids(pc.EVAL_CASES))
def test_seg_eval(case):
    from ifseg_amd import hip
    dev = _dev()
    hp, wp, h, w, n = (case[k] for k in ("hp", "wp", "h", "w", "n"))
    c = pc.seg_eval_case(hp, wp, h, w, n, case["all_ignored"])
    nblk = (h * w + 255) // 256
    hist, part = _Out((3, n), dev, I64, zero=True), _Out((nblk, 2), dev)
    assert hip.lib().ifseg_seg_eval(P(_in(c["scores"], dev)), i(hp), i(wp), i(n), P(_in(c["target"], dev, I64)), i(h), i(w), ll(pc.SEG0),
                                    P(hist.view), P(part.view), i(nblk), hip._stream()) == 0
    torch.cuda.synchronize()
    got = hist.view.cpu().numpy()
    assert np.array_equal(got, c["hist"]), "%s: histograms differ: got %r, expected %r" % (case["id"], got, c["hist"])
    hist.check("seg_eval hist " + case["id"])
    sums, bounds, cnt = pc.seg_eval_block_sums(c)
    p = part.np()
    assert np.array_equal(p[:, 1], cnt), "%s: counted pixels per block" % case["id"]
    if case["all_ignored"]:
        part.check("seg_eval partials " + case["id"])
        return
    _assert_within("seg_eval loss " + case["id"], part, sums, bounds, got=p[:, 0])
    # the binding: the mean over the counted pixels
    loss, hist2 = hip.seg_eval(_in(c["scores"], dev), hp, wp, _in(c["target"], dev, I64), h, w, pc.SEG0)
    assert np.array_equal(hist2.cpu().numpy(), c["hist"])
    want = sums.sum() / cnt.sum()
    assert abs(loss.item() - want) <= (bounds.sum() + (nblk + 16) * pc.U * np.abs(sums).sum()) / cnt.sum() + 4 * pc.U * abs(want)


# =========================================================================================================== part D
def test_bad_arguments_are_refused():
    """return codes only: every call below is refused before a launch, and nothing is written"""
    from ifseg_amd import hip
    dev = _dev()
    L, S = hip.lib(), hip._stream()
    big = 1 << 20                                  # every operand is large enough for any of the shapes named below
    X = torch.ones(big, dtype=F32, device=dev)
    XB = torch.ones(big, dtype=BF16, device=dev)
    IX = torch.zeros(big, dtype=I32, device=dev)
    TG = torch.zeros(big, dtype=I64, device=dev)
    Y = torch.full((big,), SENTINEL, dtype=F32, device=dev)
    YB = torch.full((big,), SENTINEL, dtype=BF16, device=dev)
    YI = torch.full((big,), int(SENTINEL), dtype=I32, device=dev)
    YH = torch.full((1024,), int(SENTINEL), dtype=I64, device=dev)
    want = [t.clone() for t in (Y, YB, YI, YH)]

    def bil(Cp=32, ldq=64, H=3, W=5):
        return L.ifseg_crf_bilateral(P(X), P(X), P(X), P(XB), i(ldq), P(Y), i(Cp), i(H), i(W), S)

    def bias(out=Y, tab=X, H=1, h=2, w=2, oh=2, ow=2, Lt=1, ld=0):
        return L.ifseg_resized_rel_bias(P(out), P(tab), None, None, i(H), i(h), i(w), i(oh), i(ow), i(Lt), i(0), i(ld), S)

    def rows(src=XB, dst=YB, C=8):
        return L.ifseg_resize_rows_bilinear(P(src), P(dst), i(C), i(2), i(2), i(2), i(2), i(2), i(0), i(8), S)

    def topk(N=4, k=1):
        return L.ifseg_topk_rows_f32(P(X), P(YI), i(2), i(N), i(k), S)

    def soft(n=4, rpb=2):
        return L.ifseg_softmax_rows(P(XB), ll(64), i(rpb), i(8), P(Y), i(4), i(n), f(1.0), i(1), S)

    calls = {
        "bilateral Cp % 32": (bil(Cp=48), BAD_SHAPE), "bilateral Cp < 32": (bil(Cp=0), BAD_SHAPE), "bilateral Cp > 192": (bil(Cp=224), BAD_SHAPE),
        "bilateral ldq % 64": (bil(ldq=96), BAD_SHAPE), "bilateral ldq below N rounded up": (bil(ldq=64, H=5, W=13), BAD_SHAPE),
        "bilateral W > 2048": (bil(ldq=2112, H=1, W=2049), BAD_SHAPE), "bilateral H > 2048": (bil(ldq=2112, H=2049, W=1), BAD_SHAPE),
        "rel_bias null out": (bias(out=None), BAD_ARG), "rel_bias null table": (bias(tab=None), BAD_ARG),
        "rel_bias H = 0": (bias(H=0), BAD_ARG), "rel_bias h = 0": (bias(h=0), BAD_ARG), "rel_bias w = -1": (bias(w=-1), BAD_ARG),
        "rel_bias oh = 0": (bias(oh=0), BAD_ARG), "rel_bias ow = 0": (bias(ow=0), BAD_ARG), "rel_bias Lt < 0": (bias(Lt=-1), BAD_ARG),
        "rel_bias 0 < ld < T": (bias(ld=4), BAD_ARG),
        "rel_bias 101 x 101 (161 604 bytes)": (bias(h=1, w=1, oh=101, ow=101, Lt=0), BAD_SHAPE),
        "resize_rows null src": (rows(src=None), BAD_ARG), "resize_rows null dst": (rows(dst=None), BAD_ARG),
        "resize_rows C = 0": (rows(C=0), BAD_ARG), "resize_rows C < 0": (rows(C=-8), BAD_ARG),
        "topk k = 0": (topk(k=0), BAD_ARG), "topk k = 9": (topk(N=16, k=9), BAD_ARG), "topk k > N": (topk(N=4, k=5), BAD_ARG),
        "softmax n = 0": (soft(n=0), BAD_ARG), "softmax n < 0": (soft(n=-1), BAD_ARG), "softmax rows_per_batch = 0": (soft(rpb=0), BAD_ARG),
        "softmax rows_per_batch < 0": (soft(rpb=-2), BAD_ARG),
        "gather_mean k = 0": (L.ifseg_gather_mean(P(X), P(IX), P(Y), i(2), i(7), i(5), i(0), S), BAD_ARG),
        "gather_mean k < 0": (L.ifseg_gather_mean(P(X), P(IX), P(Y), i(2), i(7), i(5), i(-1), S), BAD_ARG),
        "seg_eval nblocks + 1": (L.ifseg_seg_eval(P(X), i(2), i(2), i(5), P(TG), i(20), i(20), ll(0), P(YH), P(Y), i(3), S), BAD_ARG),
        "seg_eval nblocks - 1": (L.ifseg_seg_eval(P(X), i(2), i(2), i(5), P(TG), i(20), i(20), ll(0), P(YH), P(Y), i(1), S), BAD_ARG),
    }
    torch.cuda.synchronize()
    wrong = {k: v for k, v in calls.items() if v[0] != v[1]}
    assert not wrong, "return codes (got, expected): %s" % wrong
    for t, wv in zip((Y, YB, YI, YH), want):
        assert torch.equal(t, wv), "a refused call wrote to its output"
