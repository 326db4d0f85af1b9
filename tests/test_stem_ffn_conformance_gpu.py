"""Conformance of the trunk's entry (csrc/conv.hip: both stem kernels and the max-pool; nchw_to_nhwc of csrc/rowops.hip) and of the
FFN-LayerNorm fold (csrc/ffn_ln.hip: coef, rowstats, param_grads with its slab partials, final division and small-gain rescue)
through the C ABI (ifseg_amd.hip.lib()), in the style of test_loss_conformance_gpu.py: every operand is a view inside a larger
allocation that holds 7 around it (the row padding of ldw > N, lddy > J, ldt > J, ldu > N included), every output -- the 16 N float
workspace of param_grads too -- sits in a sentinel that must be bit-identical after the call.  Data, fp64 references, the derived
bounds and the case tables are in _stem_ffn_cases.py (its docstring holds the derivations); test_stem_ffn_conformance_cpu.py checks
them without a GPU.  Every bounded test prints `GPU <worst |err| / bound>`.

Part A: ifseg_nchw_to_nhwc_bf16, bit for bit.          Part B: the stem: exact, term isolation, random, second trip, non-finite.
Part C: ifseg_maxpool3x3s2, exact.                     Part D: ifseg_ffn_ln_coef.           Part E: ifseg_ffn_ln_rowstats.
Part F: ifseg_ffn_ln_param_grads: division, semantic check, rescue.                        Part G: refusals.
profiles/stem_ffn_conformance.txt: the kernels seen in a trace of this file, the worst ratios, the wrong variants it catches.
"""
import ctypes

import numpy as np
import pytest
import torch

import _stem_ffn_cases as sc
from test_gemm_conformance_gpu import BAD_ARG, BAD_SHAPE, BF16, F32, GUARD, _bits, _dev
from test_loss_conformance_gpu import P, _Buf, _flat

pytestmark = pytest.mark.gpu
ci = ctypes.c_int


def _lib():
    from ifseg_amd import hip
    _dev()
    return hip.lib(), hip._stream()


def _in(dev, vals, dtype=BF16, ld=None):
    """a guarded input [rows, cols] with row pitch ld (7 in the padding and around it)"""
    vals = np.asarray(vals)
    vals = vals.reshape(1, -1) if vals.ndim == 1 else vals.reshape(vals.shape[0], -1)
    src = vals if vals.dtype == np.float32 else vals.astype(np.float64)
    return _Buf(dev, dtype, 1, vals.shape[0], vals.shape[1], ld=ld, fill=GUARD, values=src)


def _out(dev, n, dtype=BF16):
    return _flat(dev, n, dtype)


def _within(what, got, ref, bound):
    r, at = sc.worst_ratio(got, ref, bound)
    print("[stem-ffn] %s: GPU %.3f" % (what, r))
    assert r <= 1.0, "%s: |err| is %.3f of the bound at %s (got %r, ref %r, bound %r)" % (
        what, r, at, np.asarray(got)[at], np.asarray(ref)[at], np.asarray(bound)[at])


def _exact(what, got, ref):
    got, ref = np.asarray(got), np.asarray(ref)
    bad = ~((got == ref) | (np.isnan(got) & np.isnan(ref)))
    assert not bad.any(), "%s: %d of %d elements differ; first at %s: got %r, expected %r" % (
        what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), got[bad][0], ref[bad][0])


def _ok(rc):
    assert rc == 0, "return code %d" % rc
    torch.cuda.synchronize()


# =========================================================================================================== part A
@pytest.mark.parametrize("f32", [True, False], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", sc.LAYOUT_SHAPES, ids=str)
def test_nchw_to_nhwc(shape, f32):
    """bf16(x) to nearest even (every tie of the hand-made vector), pad channels +0, -0 / inf / NaN kept: the bits"""
    lib, s = _lib()
    dev = _dev()
    B, C, H, W, Cp = shape
    x = sc.layout_input(shape, f32)
    xin = _in(dev, x.reshape(-1), F32 if f32 else BF16)
    if not f32:                                                            # (the bits as they are, NaN payloads included)
        xin.view.view(torch.int16).copy_(torch.from_numpy(sc.bits16(x).view(np.int16).reshape(1, 1, -1)))
        xin.before = xin.full.clone()
    out = _out(dev, B * H * W * Cp)
    _ok(lib.ifseg_nchw_to_nhwc_bf16(P(xin.view), ci(1 if f32 else 0), P(out.view), ci(B), ci(C), ci(H), ci(W), ci(Cp), s))
    got = out.view.view(torch.int16).cpu().numpy().view(np.uint16).reshape(B, H, W, Cp)
    _exact("nchw_to_nhwc %s" % (shape,), got, sc.layout_ref_bits(x, Cp))
    out.check("nchw_to_nhwc")
    assert xin.unchanged()


# =========================================================================================================== part B
class _Stem:
    def __init__(self, dev, x, w, shift):
        """x [B, H, W, 3] -> the NHWC(4) input with a zero fourth channel, the fp32 weights and their three-term form"""
        self.dev, (self.B, self.H, self.W) = dev, x.shape[:3]
        x4 = np.zeros(x.shape[:3] + (4,))
        x4[..., :3] = x
        self.x4 = _in(dev, x4.reshape(-1))
        self.w = _in(dev, np.asarray(w, dtype=np.float32).reshape(-1), F32)
        self.wt = _in(dev, sc.stem_wt(w).reshape(-1))
        self.shift = _in(dev, np.asarray(shift, dtype=np.float32), F32)
        self.OH, self.OW = sc.out_hw(self.H, self.W)

    def run(self, mfma):
        lib, s = _lib()
        out = _out(self.dev, self.B * self.OH * self.OW * 64)
        if mfma:
            rc = lib.ifseg_stem_conv7x7_mfma(P(self.x4.view), P(self.wt.view), P(self.shift.view), P(out.view), ci(self.B), ci(self.H), ci(self.W), s)
        else:
            rc = lib.ifseg_stem_conv7x7(P(self.x4.view), P(self.w.view), P(self.shift.view), P(out.view), ci(self.B), ci(self.H), ci(self.W), s)
        _ok(rc)
        out.check("stem")
        assert self.x4.unchanged() and self.w.unchanged() and self.wt.unchanged() and self.shift.unchanged(), "an input was written"
        return out, out.np().reshape(self.B, self.OH, self.OW, 64)


KERNELS = ((False, "direct"), (True, "mfma"))


@pytest.mark.parametrize("shape", sc.STEM_SHAPES, ids=str)
def test_stem_exact(shape):
    """integer images, two-term weights, integer shifts: one correct value per element, bf16(relu(ref))"""
    x, w, shift = sc.stem_data("exact", *shape)
    want = sc.bf(sc.relu(sc.stem_ref(x, w, shift)[0]))
    st = _Stem(_dev(), x, w, shift)
    for mfma, name in KERNELS:
        _exact("stem %s exact %s" % (name, shape), st.run(mfma)[1], want)


def test_stem_mfma_second_trip_of_the_tile_loop():
    """1030 one-tile images on the 1024 workgroups of the matrix-core kernel: workgroups 0..5 walk a second tile through the loop-top
    barrier.  Image b is pattern b mod 7 (1024 mod 7 = 2), so a tile computed from the previous trip's patch has another value"""
    B, H, W = sc.STEM_WRAP
    x, w, shift = sc.stem_data("exact", B, H, W, sc.WRAP_PERIOD)
    assert sc.stem_tiles(B, H, W) - sc.GRID_CAP == 6
    want7 = sc.bf(sc.relu(sc.stem_ref(x[:sc.WRAP_PERIOD], w, shift)[0]))
    st = _Stem(_dev(), x, w, shift)
    out, _ = st.run(True)
    got = out.view.reshape(B, -1)
    idx = torch.arange(B, device=got.device) % sc.WRAP_PERIOD
    want = torch.from_numpy(want7).to(BF16).to(got.device).view(sc.WRAP_PERIOD, -1)[idx]
    bad = (_bits(got) != _bits(want)).any(dim=1).nonzero().flatten().tolist()
    assert not bad, "images %s differ (second trip: images 1024 .. 1029)" % bad[:10]
    # random data on the same batch, per element against the bound (compared on the device: 17 M elements)
    x, w, shift = sc.stem_data("random", B, H, W, sc.WRAP_PERIOD)
    ref7, mag7 = sc.stem_ref(x[:sc.WRAP_PERIOD], w, shift, terms=True)
    out, _ = _Stem(_dev(), x, w, shift).run(True)
    got = out.view.reshape(B, -1).double()
    dev7 = lambda a: torch.from_numpy(a).to(got.device).view(sc.WRAP_PERIOD, -1)[idx]
    ratio = (got - dev7(sc.relu(ref7))).abs() / dev7(sc.stem_bound(ref7, mag7, sc.K_MFMA))
    worst = ratio.max(dim=1).values
    print("[stem-ffn] stem mfma %s: GPU %.3f (images 1024 .. 1029: %.3f)" % (sc.STEM_WRAP, worst.max().item(), worst[sc.GRID_CAP:].max().item()))
    assert worst.max().item() <= 1.0, "images %s exceed the bound" % (worst > 1).nonzero().flatten().tolist()[:10]


def test_stem_term_isolation():
    """delta images, w = 1 + 2^-9 + q 2^-23, shift -(1 + 2^-9): the output where a tap meets the pixel is q 2^-23 exactly, so a
    dropped, swapped or mis-pitched second or third weight term changes a representable value"""
    x, w, shift, want, _ = sc.iso_data()
    st = _Stem(_dev(), x, w, shift)
    for mfma, name in KERNELS:
        _exact("stem %s isolation" % name, st.run(mfma)[1], want)


@pytest.mark.parametrize("shape", sc.STEM_SHAPES, ids=str)
def test_stem_random(shape):
    """|out - relu(ref)| <= 2^-8 |ref| + (K + 4) 2^-23 mag per element, K = 147 resp. 3 * 224; the two kernels agree within the sum"""
    x, w, shift = sc.stem_data("random", *shape)
    st = _Stem(_dev(), x, w, shift)
    got, bounds = {}, {}
    for (mfma, name), K in zip(KERNELS, (sc.K_DIRECT, sc.K_MFMA)):
        ref, mag = sc.stem_ref(x, w, shift, terms=mfma)
        got[name], bounds[name] = st.run(mfma)[1], sc.stem_bound(ref, mag, K)
        assert np.isfinite(got[name]).all() and not np.signbit(got[name]).any()
        _within("stem %s %s" % (name, shape), got[name], sc.relu(ref), bounds[name])
    _within("stem direct vs mfma %s" % (shape,), got["direct"], got["mfma"], bounds["direct"] + bounds["mfma"])


def test_stem_and_pool_pass_non_finite_values_as_torch_does():
    """torch's contract: an output whose window holds a NaN is NaN, relu(+inf) = +inf, relu(-inf) = +0, a poisoned image leaves stem
    and pool all-NaN.  The matrix-core kernel multiplies the zero weights of its padded tap kx = 7 with real pixels, so a non-finite
    value in the input column 2 ox + 4, right of the window, gives NaN there as well (0 * NaN, 0 * inf), as the header says."""
    lib, s = _lib()
    x, w, shift = sc.nonfinite_data()
    clean = np.where(np.isfinite(x), x, 0.0)
    st = _Stem(_dev(), x, w, shift)
    for mfma, name in KERNELS:
        want, nan7 = sc.stem_nonfinite_expect(x, w, shift, mfma)
        out, got = st.run(mfma)
        assert np.isnan(got[nan7]).all(), "%s: a window that holds a NaN did not give NaN" % name
        assert np.array_equal(np.isnan(got), np.isnan(want)), "%s: NaN where none is expected, or none where one is" % name
        assert mfma or np.array_equal(np.isnan(got[..., 0]), nan7), "direct kernel: NaN exactly where the 7 x 7 window holds one"
        assert np.array_equal(np.isposinf(got), np.isposinf(want)) and np.isposinf(want).any() and not np.isneginf(got).any(), name
        assert np.isnan(got[1]).all() and np.isfinite(got[2]).all(), "%s: the poisoned image leaves the stem all-NaN" % name
        fin = np.isfinite(want)
        ref, mag = sc.stem_ref(clean, w, shift, terms=mfma)
        bound = sc.stem_bound(ref, mag, sc.K_MFMA if mfma else sc.K_DIRECT)
        zero_by_neg_inf = fin & sc.window_any(np.isneginf(x).any(axis=3))[..., None]              # relu(-inf): +0
        assert zero_by_neg_inf.any() and (got[zero_by_neg_inf] == 0).all() and not np.signbit(got[zero_by_neg_inf]).any()
        rest = fin & ~zero_by_neg_inf
        _within("stem %s non-finite, the finite rest" % name, got[rest], sc.relu(ref)[rest], bound[rest])
        # the pool on what the stem left
        B, OH, OW = st.B, st.OH, st.OW
        PH, PW = sc.out_hw(OH, OW)
        pooled = _out(st.dev, B * PH * PW * 64)
        _ok(lib.ifseg_maxpool3x3s2(P(out.view), P(pooled.view), ci(B), ci(OH), ci(OW), ci(64), s))
        pg = pooled.np().reshape(B, PH, PW, 64)
        _exact("pool of the %s stem" % name, pg, sc.pool_ref(got))
        assert np.isnan(pg[1]).all() and np.isfinite(pg[2]).all(), "%s: the poisoned image leaves the pool all-NaN" % name
        pooled.check("pool")


def test_a_poisoned_sample_is_caught_by_its_target():
    """a poisoned sample (ifseg_train_load: NaN images and target -1) is refused at engine level whatever its features do to the
    loss: the loss kernel counts its target of -1 as a bad label and the engine raises, in that call or the next"""
    import segofa_ref as O
    from ifseg_amd.criterions import SegCriterion
    from ifseg_amd.models.segofa import SegOFAModel, make_config
    dev = _dev()
    ocfg = O.fixture_config()
    sd = O.procedural_state_dict(ocfg)
    batch = O.synthetic_batch(ocfg, 2, 12)
    m = SegOFAModel(make_config("segofa_tiny", embed_dim=ocfg.embed_dim, ffn_dim=ocfg.ffn_dim, heads=ocfg.heads, enc_layers=ocfg.enc_layers,
                                dec_layers=ocfg.dec_layers, resnet_layers=ocfg.resnet_layers, num_seg_tokens=ocfg.num_seg_tokens,
                                vocab_size=ocfg.vocab_size, patch_image_size=128, orig_patch_image_size=128))
    torch.nn.Module.load_state_dict(m, sd, strict=False)
    m.to(dev).train()
    crit = SegCriterion(unsupervised_segmentation=False, init_seg_with_text=False, num_seg_tokens=ocfg.num_seg_tokens, seg_id_offset=ocfg.seg_id_offset)

    def sample(poison):
        net = {k: batch[k].to(dev).clone() for k in ("src_tokens", "patch_images", "patch_masks", "prev_output_tokens")}
        target = batch["target"].to(dev).clone()
        if poison:
            net["patch_images"][0] = float("nan")
            target[0, :-1] = -1
        return {"net_input": net, "target": target, "ntokens": 1, "nsentences": 2}

    loss, _, _ = crit(m, sample(False))
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all()
    with pytest.raises(IndexError, match="target label outside"):
        crit(m, sample(True))
        torch.cuda.synchronize()
        crit(m, sample(False))
        torch.cuda.synchronize()
        crit(m, sample(False))
    torch.cuda.synchronize()


# =========================================================================================================== part C
@pytest.mark.parametrize("nan", [False, True], ids=["finite", "nan"])
@pytest.mark.parametrize("shape", sc.POOL_SHAPES, ids=str)
def test_maxpool(shape, nan):
    """the fp64 window maximum, exactly: -0 / +0 pairs (compared as values), the lowest finite bf16, -inf, windows of -inf only; with
    NaN in the image, a window that holds one gives NaN, as F.max_pool2d does"""
    lib, s = _lib()
    dev = _dev()
    B, H, W, C = shape
    x = sc.pool_data(shape, nan)
    xin = _in(dev, x.reshape(-1))
    OH, OW = sc.out_hw(H, W)
    out = _out(dev, B * OH * OW * C)
    _ok(lib.ifseg_maxpool3x3s2(P(xin.view), P(out.view), ci(B), ci(H), ci(W), ci(C), s))
    _exact("maxpool %s" % (shape,), out.np().reshape(B, OH, OW, C), sc.pool_ref(x))
    out.check("maxpool")
    assert xin.unchanged()


# =========================================================================================================== part D
COEF_LAUNCHES = ((1, 0, True, "exact"), (1, 8, False, "random"), (3, 8, True, "exact"), (3, 0, False, "random"),
                 (32, 8, True, "random"), (32, 0, True, "exact"), (32, 8, False, "exact"))          # (L, ldw - N, b2 given, data)


@pytest.mark.parametrize("JN", sc.COEF_SHAPES, ids=str)
def test_ffn_ln_coef(JN):
    """a_j = sum_k gamma_k W2[j,k], wb_j = b2_j + sum_k beta_k W2[j,k]; L layers that differ in one launch through the test's own
    pointer tables, ldw = N and N + 8, b2 NULL and given.  Integers: equality; random: (d + 1) u sum |w gamma|, d = ceil(N / 512) + 13"""
    lib, s = _lib()
    dev = _dev()
    J, N = JN
    for L, pad, bias, kind in COEF_LAUNCHES:
        w2, gamma, beta, b2 = sc.coef_data(J, N, L, kind)
        ldw = N + pad
        W = _Buf(dev, BF16, L, J, N, ld=ldw, bs=J * ldw + 24, fill=GUARD, values=w2)
        G = _Buf(dev, F32, L, 1, N, bs=N + 12, fill=GUARD, values=gamma)
        Bt = _Buf(dev, F32, L, 1, N, bs=N + 4, fill=GUARD, values=beta)
        B2 = _Buf(dev, BF16, L, 1, J, bs=J + 3, fill=GUARD, values=b2)
        C = _Buf(dev, F32, L, 2, J, bs=2 * J + 5)
        tab = lambda b: (ctypes.c_void_p * L)(*[b.view[l].data_ptr() for l in range(L)])
        _ok(lib.ifseg_ffn_ln_coef(tab(W), ci(ldw), tab(G), tab(Bt), tab(B2) if bias else None, tab(C), ci(L), ci(J), ci(N), s))
        C.check("coef")
        assert all(b.unchanged() for b in (W, G, Bt, B2)), "an input was written"
        ref, bound = sc.coef_ref(w2, gamma, beta, b2 if bias else None)
        what = "coef J%d N%d L%d ldw+%d %s%s" % (J, N, L, pad, kind, "" if bias else " no b2")
        if kind == "exact":
            _exact(what, C.np(), ref)
        else:
            _within(what, C.np(), ref, bound)


# =========================================================================================================== part E
@pytest.mark.parametrize("J", sc.ROWSTATS_J)
def test_ffn_ln_rowstats(J):
    """c1 = (1/N) sum_j dY_j a_j, c2 = (1/N) sum_j dY_j (t_j - wb_j) from the test's own coef; lddy, ldt beyond J; one data set has t
    within a few bf16 ulps of wb, so the subtraction cancels"""
    lib, s = _lib()
    dev = _dev()
    for rows in sc.ROWSTATS_ROWS:
        for kind, Ns in (("exact", (8,)), ("random", sc.ROWSTATS_N), ("cancel", (3072,))):
            dy, t, coef = sc.rowstats_data(rows, J, kind)
            DY, Tt = _in(dev, dy, ld=J + 8), _in(dev, t, ld=J + 24)
            CO = _in(dev, coef.reshape(-1), F32)
            for N in Ns:
                c = _out(dev, 2 * rows, F32)
                _ok(lib.ifseg_ffn_ln_rowstats(P(DY.view), ci(J + 8), P(Tt.view), ci(J + 24), P(CO.view), P(c.view), ci(rows), ci(J), ci(N), s))
                c.check("rowstats")
                ref, bound = sc.rowstats_ref(dy, t, coef, N)
                what = "rowstats rows%d J%d N%d %s" % (rows, J, N, kind)
                got = c.np().reshape(rows, 2)
                if kind == "exact":
                    _exact(what, got, ref)
                else:
                    _within(what, got, ref, bound)
            assert DY.unchanged() and Tt.unchanged() and CO.unchanged()


# =========================================================================================================== part F
def _param_grads(dev, d, N, rescue=None):
    """-> (dgamma, dbeta) as float64 and their bits; `rescue`: dict with dy, u, mean, rstd (lddy = J + 8, ldu = N + 8)"""
    lib, s = _lib()
    J = d["w2"].shape[0]
    ins = [_in(dev, d["w2"]), _in(dev, d["dw2"]), _in(dev, d["db2"]), _in(dev, d["gamma"], F32), _in(dev, d["beta"], F32)]
    dg, db, ws = _out(dev, N), _out(dev, N), _out(dev, 16 * N, F32)
    tail = (None, ci(0), None, ci(0), None, None, ci(0))
    if rescue is not None:
        M = rescue["dy"].shape[0]
        ins += [_in(dev, rescue["dy"], ld=J + 8), _in(dev, rescue["u"], ld=N + 8), _in(dev, rescue["mean"], F32), _in(dev, rescue["rstd"], F32)]
        tail = (P(ins[5].view), ci(J + 8), P(ins[6].view), ci(N + 8), P(ins[7].view), P(ins[8].view), ci(M))
    _ok(lib.ifseg_ffn_ln_param_grads(*[P(b.view) for b in ins[:5]], P(dg.view), P(db.view), P(ws.view), ci(J), ci(N), *tail, s))
    for b in (dg, db, ws):
        b.check("param_grads")
    assert all(b.unchanged() for b in ins), "an input was written"
    return dg.np().reshape(-1), db.np().reshape(-1), _bits(dg.view).cpu().numpy().reshape(-1)


@pytest.mark.parametrize("J", sc.PG_J)
def test_ffn_ln_param_grads(J):
    """dbeta and dgamma without rescue operands: fewer rows than slabs, ragged slabs, ragged 128-column blocks; gamma == 0 gives +0"""
    dev = _dev()
    for N in sc.PG_N:
        for kind in ("exact", "random"):
            w2, dw2, db2, gamma, beta = sc.pg_data(J, N, kind)
            dg, db, bits = _param_grads(dev, dict(w2=w2, dw2=dw2, db2=db2, gamma=gamma, beta=beta), N)
            rg, rb, bg, bb = sc.pg_ref(w2, dw2, db2, gamma, beta)
            what = "param_grads J%d N%d %s" % (J, N, kind)
            assert (bits[gamma == 0] == 0).all(), "%s: gamma == 0 must give +0" % what
            if kind == "exact":
                _exact(what + " dgamma", dg, rg)
                _exact(what + " dbeta", db, rb)
            else:
                _within(what + " dgamma", dg, rg, bg)
                _within(what + " dbeta", db, rb, bb)


def test_ffn_ln_division_against_the_definition():
    """dW2, db2 = bf16 of the fp64 weight gradient of a real LN(gelu(u)) W2^T + b2; reference: the fp64 dgamma of the definition;
    bound: the kernel's plus the inputs' rounding 2^-8 (sum |W2 dW2| + |beta| sum |W2 db2|) / |gamma|.  Prints what the threshold
    0.05 costs: the worst |err| / max |dgamma| over the unflagged columns (recorded in profiles/stem_ffn_conformance.txt:
    0.0135 at gamma = 0.0501 with beta -0.9 on MI355X; nothing is tuned to it)"""
    d = sc.semantic_data()
    dg, db, _ = _param_grads(_dev(), d, sc.SEM_N)
    rg, rb, bg, bb = sc.pg_ref(d["w2"], d["dw2"], d["db2"], d["gamma"], d["beta"], input_terms=True)
    nz, keep = d["gamma"] != 0, ~d["flagged"]
    assert (dg[~nz] == 0).all()
    err = np.abs(dg - d["dgamma"])
    k = int(np.argmax(np.where(keep, err, 0)))
    print("[stem-ffn] semantic: unflagged worst |err| / max |dgamma| %.4g (column %d: gamma %g, beta %g); worst over the flagged non-zero gains %.4g"
          % (err[k] / np.abs(d["dgamma"]).max(), k, d["gamma"][k], d["beta"][k], err[nz & ~keep].max() / np.abs(d["dgamma"]).max()))
    _within("semantic dgamma (gamma != 0)", dg[nz], d["dgamma"][nz], bg[nz])
    _within("semantic dgamma, unflagged", dg[keep], d["dgamma"][keep], bg[keep])
    _within("semantic dbeta", db, d["dbeta"], bb + sc.U_BF16 * (np.abs(d["w2"] * d["db2"][:, None])).sum(0))


@pytest.mark.parametrize("MJ", sc.RESCUE_CASES + ((3, 8, "none"),), ids=str)
def test_ffn_ln_rescue(MJ):
    """the flagged columns (block edges 0, 255, 256, N - 1 and two neighbours) from the definition, lddy and ldu beyond the row; every
    other column keeps the bits of the division; with no flagged column the launch changes nothing"""
    dev = _dev()
    none = len(MJ) == 3
    d = sc.rescue_data(MJ[0], MJ[1], () if none else sc.RESCUE_FLAGGED)
    fl = np.flatnonzero(sc.gain_is_small(d["gamma"], d["beta"]))
    assert tuple(fl) == (() if none else sc.RESCUE_FLAGGED)
    dg, db, bits = _param_grads(dev, d, sc.RESCUE_N, rescue=d)
    dg0, db0, bits0 = _param_grads(dev, d, sc.RESCUE_N)
    rest = np.ones(sc.RESCUE_N, dtype=bool)
    rest[fl] = False
    assert np.array_equal(bits[rest], bits0[rest]) and np.array_equal(db, db0), "an unflagged column lost the division's bits"
    rg, rb, bg, bb = sc.pg_ref(d["w2"], d["dw2"], d["db2"], d["gamma"], d["beta"])
    _within("rescue M%d J%d division" % MJ[:2], dg[rest], rg[rest], bg[rest])
    if not none:
        ref, bound = sc.rescue_ref(d, list(fl))
        _within("rescue M%d J%d flagged" % MJ[:2], dg[fl], ref, bound)


# =========================================================================================================== part G
def test_refusals_before_any_launch():
    """every entry returns IFSEG_ERR_BAD_ARG or IFSEG_ERR_BAD_SHAPE for a null or misaligned pointer and for the shapes it cannot take,
    and writes nothing"""
    lib, s = _lib()
    dev = _dev()
    outs = []

    def O(n, dtype=BF16):
        outs.append(_out(dev, n, dtype))
        return outs[-1].view

    def refused(what, rc):
        assert rc in (BAD_ARG, BAD_SHAPE), "%s: return code %d" % (what, rc)

    def sweep(what, fn, args, ptrs, bad):
        """args: the valid call; ptrs: index -> byte offset that misaligns it (None: only null is refused); bad: index -> value"""
        for i, off in ptrs.items():
            a = list(args)
            a[i] = None
            refused("%s null argument %d" % (what, i), fn(*a, s))
            if off:
                a[i] = ctypes.c_void_p(args[i].value + off)
                refused("%s misaligned argument %d" % (what, i), fn(*a, s))
        for i, vals in bad.items():
            for v in vals:
                a = list(args)
                a[i] = ci(v)
                refused("%s argument %d = %d" % (what, i, v), fn(*a, s))

    x4 = _in(dev, np.zeros(2 * 8 * 8 * 4))
    w, wt, sh = _in(dev, np.zeros(147 * 64), F32), _in(dev, np.zeros(3 * 64 * 224)), _in(dev, np.zeros(64), F32)
    big = (1 << 20, 64, 64)
    args = [P(x4.view), P(w.view), P(sh.view), P(O(2 * 4 * 4 * 64)), ci(2), ci(8), ci(8)]
    sweep("stem", lib.ifseg_stem_conv7x7, args, {0: 4, 1: 2, 2: 2, 3: 8}, {4: (0, -1), 5: (0, -3), 6: (0, -1)})
    refused("stem 2^34 elements", lib.ifseg_stem_conv7x7(*args[:4], *[ci(v) for v in big], s))
    args[1] = P(wt.view)
    sweep("stem mfma", lib.ifseg_stem_conv7x7_mfma, args, {0: 4, 1: 8, 2: 8, 3: 8}, {4: (0, -1), 5: (0, -3), 6: (0, -1)})
    refused("stem mfma 2^34 elements", lib.ifseg_stem_conv7x7_mfma(*args[:4], *[ci(v) for v in big], s))
    pin = _in(dev, np.zeros(2 * 8 * 8 * 64))
    args = [P(pin.view), P(O(2 * 4 * 4 * 64)), ci(2), ci(8), ci(8), ci(64)]
    sweep("maxpool", lib.ifseg_maxpool3x3s2, args, {0: 8, 1: 8}, {2: (0, -1), 3: (0, -1), 4: (0, -1), 5: (0, -8, 4, 68)})
    refused("maxpool 2^38 elements", lib.ifseg_maxpool3x3s2(*args[:2], *[ci(v) for v in big], ci(64), s))
    lin = _in(dev, np.zeros(2 * 3 * 8 * 8), F32)
    args = [P(lin.view), ci(1), P(O(2 * 8 * 8 * 4)), ci(2), ci(3), ci(8), ci(8), ci(4)]
    sweep("nchw_to_nhwc", lib.ifseg_nchw_to_nhwc_bf16, args, {0: 2, 2: 1}, {3: (0, -1), 4: (0, -1), 5: (0, -1), 6: (0, -1), 7: (0, 2)})
    refused("nchw_to_nhwc 2^34 elements", lib.ifseg_nchw_to_nhwc_bf16(*args[:3], ci(big[0]), ci(3), ci(64), ci(64), ci(4), s))

    # ---- ffn_ln
    J, N, L = 8, 16, 2
    w2, g, b, b2 = (_in(dev, np.zeros((L, J * N))), _in(dev, np.zeros((L, N)), F32), _in(dev, np.zeros((L, N)), F32), _in(dev, np.zeros((L, J))))
    co = O(L * 2 * J, F32).view(L, 2 * J)
    tab = lambda t, off=0, null=-1: (ctypes.c_void_p * L)(*[None if l == null else t[l].data_ptr() + off for l in range(L)])
    V = lambda bf: bf.view[0]
    coef = lambda **k: [k.get("w2", tab(V(w2))), ci(k.get("ldw", N)), k.get("g", tab(V(g))), k.get("b", tab(V(b))), k.get("b2", tab(V(b2))),
                        k.get("co", tab(co)), ci(k.get("L", L)), ci(k.get("J", J)), ci(k.get("N", N))]
    assert lib.ifseg_ffn_ln_coef(*coef(), s) == 0
    torch.cuda.synchronize()
    outs.pop()                                                                      # (that one was written: a valid call)
    co = O(L * 2 * J, F32).view(L, 2 * J)
    for what, k in (("null w2", dict(w2=None)), ("null gamma", dict(g=None)), ("null beta", dict(b=None)), ("null coef", dict(co=None)),
                    ("null w2[1]", dict(w2=tab(V(w2), 0, 1))), ("null gamma[1]", dict(g=tab(V(g), 0, 1))), ("null beta[0]", dict(b=tab(V(b), 0, 0))),
                    ("null coef[1]", dict(co=tab(co, 0, 1))), ("L = 0", dict(L=0)), ("L = 33", dict(L=33)), ("J = 0", dict(J=0)), ("N = 0", dict(N=0)),
                    ("N % 8", dict(N=12)), ("ldw % 8", dict(ldw=20)), ("misaligned w2[l]", dict(w2=tab(V(w2), 8))),
                    ("misaligned gamma[l]", dict(g=tab(V(g), 4))), ("misaligned beta[l]", dict(b=tab(V(b), 8)))):
        refused("coef " + what, lib.ifseg_ffn_ln_coef(*coef(**k), s))
    dy, t, cf = _in(dev, np.zeros((4, 8))), _in(dev, np.zeros((4, 8))), _in(dev, np.zeros(16 + 4), F32)
    args = [P(dy.view), ci(8), P(t.view), ci(8), P(cf.view), P(O(8, F32)), ci(4), ci(8), ci(16)]
    sweep("rowstats", lib.ifseg_ffn_ln_rowstats, args, {0: 8, 2: 8, 4: 4, 5: 2}, {1: (12,), 3: (12,), 6: (0,), 7: (0, 12), 8: (0,)})
    Jr, M = 16, 4
    W2, DW, DB = _in(dev, np.zeros(Jr * N + 8)), _in(dev, np.zeros(Jr * N + 8)), _in(dev, np.zeros(Jr))
    DY, Uu, mr = _in(dev, np.zeros((M, Jr + 8))), _in(dev, np.zeros((M, N))), _in(dev, np.zeros(M), F32)
    args = [P(W2.view), P(DW.view), P(DB.view), P(V(g)), P(V(b)), P(O(N)), P(O(N)), P(O(16 * N, F32)), ci(Jr), ci(N),
            P(DY.view), ci(Jr), P(Uu.view), ci(N), P(mr.view), P(mr.view), ci(M)]
    sweep("param_grads", lib.ifseg_ffn_ln_param_grads, args, {0: 8, 1: 8, 2: 0, 3: 2, 4: 2, 5: 0, 6: 0, 7: 2, 12: 0, 14: 0, 15: 0},
          {8: (0, 12, 1032), 9: (0, 12), 11: (12,), 16: (0,)})
    a = list(args)
    a[10] = ctypes.c_void_p(args[10].value + 8)
    refused("param_grads misaligned dy", lib.ifseg_ffn_ln_param_grads(*a, s))
    a = list(args)
    a[8] = ci(1032)
    assert lib.ifseg_ffn_ln_param_grads(*a, s) == BAD_ARG, "dy given: J = 1032 is IFSEG_ERR_BAD_ARG"
    torch.cuda.synchronize()
    for o in outs:
        assert o.unchanged(), "a refused call wrote into an output"
