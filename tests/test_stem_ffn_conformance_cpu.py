"""The data, references, bounds and restatements of _stem_ffn_cases.py, checked without a GPU:
  1. the fp64 references against F.conv2d, F.max_pool2d, F.layer_norm and autograd in float64;
  2. an fp32 restatement of every kernel, in the kernel's summation order, inside its bound (printed: `restated`);
  3. wrong variants of the restatements outside TWICE the bound (where the case is exact: different from the one correct value);
  4. the conditions on the inputs, on the reference alone: exact cases representable in the output type, fewer than 10 % of the
     exact stem outputs zero behind the ReLU, the flagged-column counts as intended, the three-term weight decomposition.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _stem_ffn_cases as sc

F64 = torch.float64
T = lambda a: torch.from_numpy(np.array(a, dtype=np.float64))


def _inside(what, got, ref, bound):
    r, at = sc.worst_ratio(got, ref, bound)
    print("[stem-ffn] %s: restated %.3f" % (what, r))
    assert r <= 1.0, "%s: the restatement is %.3f of the bound at %s" % (what, r, at)


def _outside(what, got, ref, bound, share=0.0):
    """a wrong variant: some element (at least `share` of them) lies outside twice the bound"""
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    out = err > 2 * bound
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = np.nanmax(np.where(err > 0, err / bound, 0.0))
    print("[stem-ffn] variant %s: %d of %d outside twice the bound, worst %.3g x bound" % (what, int(out.sum()), out.size, worst))
    assert out.any() and out.mean() >= share, "%s stays inside twice the bound" % what


# ================================================================================================ 1. references
@pytest.mark.parametrize("shape", sc.STEM_SHAPES[:5], ids=str)
def test_stem_reference_is_conv2d(shape):
    x, w, shift = sc.stem_data("random", *shape)
    ref, mag = sc.stem_ref(x, w, shift)
    want = F.conv2d(T(x).permute(0, 3, 1, 2), T(w).permute(3, 2, 0, 1), T(shift), 2, 3).permute(0, 2, 3, 1).numpy()
    assert ref.shape == want.shape and np.abs(ref - want).max() <= 1e-12 * mag.max()
    assert (mag >= np.abs(ref) - 1e-12).all()


def test_stem_wrap_reference_has_the_period_of_its_images():
    B, H, W = sc.STEM_WRAP
    assert sc.stem_tiles(B, H, W) == 1030 and sc.stem_tiles(B, H, W) - sc.GRID_CAP == 6 and sc.GRID_CAP % sc.WRAP_PERIOD != 0
    x, w, shift = sc.stem_data("exact", B, H, W, sc.WRAP_PERIOD)
    ref, _ = sc.stem_ref(x, w, shift, period=sc.WRAP_PERIOD)
    one, _ = sc.stem_ref(x[1029:1030], w, shift)
    assert np.array_equal(ref[1029], one[0]) and np.array_equal(x[1029], x[1029 % 7])
    # the tile a workgroup would compute from the previous trip's patch differs from the expected one nearly everywhere
    stale, want = sc.bf(sc.relu(ref[np.arange(1024, 1030) - sc.GRID_CAP])), sc.bf(sc.relu(ref[1024:]))
    assert (stale != want).mean() > 0.9


@pytest.mark.parametrize("shape", sc.POOL_SHAPES, ids=str)
@pytest.mark.parametrize("nan", [False, True], ids=["finite", "nan"])
def test_pool_reference_is_max_pool2d(shape, nan):
    x = sc.pool_data(shape, nan)
    want = F.max_pool2d(T(x).permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).numpy()
    ref = sc.pool_ref(x)
    assert np.array_equal(ref, want, equal_nan=True) and np.isnan(ref).any() == nan
    if shape[1] > 1:
        assert np.isneginf(ref[0, 0, 0, 0]) and ref[0, 0, 0, 1] == sc.BF16_LOWEST and ref[0, 0, 0, 2] == 0


def test_nonfinite_contract_is_torchs():
    x, w, shift = sc.nonfinite_data()
    want = torch.relu(F.conv2d(T(x).permute(0, 3, 1, 2), T(w).permute(3, 2, 0, 1), T(shift), 2, 3)).permute(0, 2, 3, 1).numpy()
    got, nan7 = sc.stem_nonfinite_expect(x, w, shift, mfma=False)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isnan(got[..., 0]), nan7)
    assert np.array_equal(np.isposinf(got), np.isposinf(want)) and np.isposinf(got).sum() == 12 * 64
    assert np.isnan(got[1]).all() and np.isfinite(got[2]).all() and (got[0][np.isfinite(got[0])] >= 0).all()
    # -inf: zeros where it is the only non-finite value of the window
    assert (got[0, 6:9, 16:18] == 0).all()
    # the matrix-core kernel's zero-weight tap: one more column of NaN per non-finite pixel, nothing else changes
    gm, _ = sc.stem_nonfinite_expect(x, w, shift, mfma=True)
    extra = np.isnan(gm) & ~np.isnan(got)
    assert extra.any() and not (np.isnan(got) & ~np.isnan(gm)).any() and np.array_equal(gm[~extra], got[~extra], equal_nan=True)
    pooled = sc.pool_ref(got)
    assert np.isnan(pooled[1]).all() and np.isfinite(pooled[2]).all()


def test_ffn_references_are_autograd_in_float64():
    d = sc.semantic_data()
    u, w2, dy = T(d["u"]), T(d["w2"]).requires_grad_(), T(d["dy"])
    gamma, beta = T(d["gamma"]).requires_grad_(), T(d["beta"]).requires_grad_()
    b2 = torch.zeros(sc.SEM_J, dtype=F64, requires_grad=True)
    z = F.layer_norm(F.gelu(u), (sc.SEM_N,), gamma, beta, 1e-5)
    z.retain_grad()
    t = z @ w2.T + b2
    (t * dy).sum().backward()
    close = lambda a, b, tol=1e-9: np.abs(a - b.numpy()).max() <= tol * max(1.0, np.abs(b.numpy()).max())
    assert close(d["dgamma"], gamma.grad) and close(d["dbeta"], beta.grad)
    # param_grads' formula from the exact weight gradient is the definition (loose where it divides by 1e-4)
    dg, db, _, _ = sc.pg_ref(d["w2"], w2.grad.numpy(), b2.grad.numpy(), d["gamma"], d["beta"])
    nz = d["gamma"] != 0
    assert close(db, beta.grad) and np.abs(dg - gamma.grad.numpy())[nz].max() < 1e-8 and (dg[~nz] == 0).all()
    assert np.abs(sc.bf(w2.grad.numpy()) - d["dw2"]).max() == 0 and np.abs(sc.bf(b2.grad.numpy()) - d["db2"]).max() == 0
    # coef + rowstats are the two row means of the LayerNorm backward
    coef, _ = sc.coef_ref(d["w2"][None], d["gamma"][None], d["beta"][None], np.zeros((1, sc.SEM_J)))
    c, _ = sc.rowstats_ref(d["dy"], t.detach().numpy(), coef[0], sc.SEM_N)
    g64 = d["gamma"].astype(np.float64)
    xhat = (z.detach().numpy() - d["beta"].astype(np.float64)) / np.where(nz, g64, 1.0)
    dz = z.grad.numpy()
    assert np.abs(c[:, 0] - (g64 * dz).mean(1)).max() < 1e-12
    want2 = ((g64 * xhat * dz)[:, nz]).sum(1) / sc.SEM_N
    assert np.abs(c[:, 1] - want2).max() < 1e-10


def test_rescue_reference_is_the_definition():
    d = sc.rescue_data(257, 8)
    cols = list(sc.RESCUE_FLAGGED)
    ref, bound = sc.rescue_ref(d, cols)
    a = sc.gelu64(d["u"])
    xhat = (a - d["mean"].astype(np.float64)[:, None]) * d["rstd"].astype(np.float64)[:, None]
    want = ((d["dy"] @ d["w2"]) * xhat).sum(0)[cols]
    assert (np.abs(ref - want) <= bound).all() and np.abs(ref - want).max() < 1e-4 * np.abs(want).max()


# =========================================================================================== 2. + 3. the stem
def test_layout_reference_rounds_ties_to_even():
    t = np.array(sc.TIE_BITS, dtype=np.uint32).view(np.float32)
    assert np.array_equal(sc.bits16(sc.bf16_round(t)), np.array(sc.TIE_WANT, dtype=np.uint16))
    for shape in sc.LAYOUT_SHAPES:
        for f32 in (True, False):
            x = sc.layout_input(shape, f32)
            want = torch.zeros(shape[0], shape[2], shape[3], shape[4], dtype=torch.bfloat16)
            want[..., :shape[1]] = torch.from_numpy(x).permute(0, 2, 3, 1).to(torch.bfloat16)
            got, nan = sc.layout_ref_bits(x, shape[4]).view(np.int16), torch.isnan(want).numpy()     # (a NaN's payload is torch's own)
            assert np.array_equal(got[~nan], want.view(torch.int16).numpy()[~nan]) and (got[nan] & 0x7FC0 == 0x7FC0).all()


def test_stem_weights_three_terms():
    from ifseg_amd import hip
    g = torch.Generator().manual_seed(5)
    # 35 decades, 1e-28 .. 1e7 (three normalised bf16 terms exist down to 2^-126 + 24, about 2e-31; real stem weights are O(0.1))
    n = 107 * 9408                                                  # 1 006 656 weights: 107 filter banks of [7, 7, 3, 64]
    w = ((torch.randint(0, 2, (n,), generator=g) * 2 - 1) * 10.0 ** (torch.rand(n, generator=g, dtype=torch.float64) * 35 - 28)).float()
    for wk in w.view(107, 7, 7, 3, 64):                             # through the product's own function, bank by bank
        t = hip.stem_weights_mfma(wk)
        assert t.dtype == torch.bfloat16 and tuple(t.shape) == (3, 64, 224)
        t = t.float().view(3, 64, 7, 8, 4)
        assert (t[:, :, :, 7, :] == 0).all() and (t[:, :, :, :, 3] == 0).all(), "the kx = 7 and ci = 3 slots hold zero weights"
        t = t[:, :, :, :7, :3].permute(0, 2, 3, 4, 1)               # -> [3][ky][kx][ci][c]: k = ky*32 + kx*4 + ci
        assert torch.equal((t[0] + t[1]) + t[2], wk) and torch.equal(t[0] + (t[1] + t[2]), wk), "t0 + t1 + t2 == w bit for bit"
    t0, t1, t2 = (torch.from_numpy(t) for t in sc.stem_terms(w.numpy()))        # the suite's own restatement of it
    assert torch.equal((t0 + t1) + t2, w) and torch.equal(t0 + (t1 + t2), w)
    # the restatement of the whole layout is hip.stem_weights_mfma, bit for bit
    wk = torch.randn(7, 7, 3, 64, generator=g) * 0.1
    wt = hip.stem_weights_mfma(wk)
    assert wt.dtype == torch.bfloat16 and tuple(wt.shape) == (3, 64, 224)
    assert np.array_equal(wt.float().numpy(), sc.stem_wt(wk.numpy()))
    v = wt.float().view(3, 64, 7, 8, 4)
    assert (v[:, :, :, 7, :] == 0).all() and (v[:, :, :, :, 3] == 0).all()
    assert torch.equal(v[0, :, :, :7, :3], wk.to(torch.bfloat16).float().permute(3, 0, 1, 2))
    assert torch.equal(v.sum(0)[:, :, :7, :3], wk.permute(3, 0, 1, 2))
    # the isolation weights split into 1, 2^-9 and q 2^-23
    _, wi, _, _, q = sc.iso_data()
    vi = hip.stem_weights_mfma(torch.from_numpy(wi)).float().view(3, 64, 7, 8, 4)[:, :, :, :7, :3].permute(0, 2, 3, 4, 1).numpy()
    assert (vi[0] == 1).all() and (vi[1] == 2.0 ** -9).all() and np.array_equal(vi[2], q * 2.0 ** -23) and q.min() >= 1 and q.max() < 64


@pytest.mark.parametrize("shape", sc.STEM_SHAPES, ids=str)
def test_stem_exact_inputs(shape):
    x, w, shift = sc.stem_data("exact", *shape)
    ref, mag = sc.stem_ref(x, w, shift)
    assert np.array_equal(ref * 1024, np.round(ref * 1024)) and mag.max() * 1024 < 2 ** 24, "every partial sum fits 24 bits"
    t0, t1, t2 = sc.stem_terms(w)
    assert (t1 != 0).all() and (t2 == 0).all() and np.array_equal(t0.astype(np.float64) + t1, w.astype(np.float64)), "two bf16 terms"
    zf = (ref <= 0).mean()
    assert zf < 0.10, "%.1f %% of the expected outputs are zero behind the ReLU" % (100 * zf)
    want = sc.bf(sc.relu(ref))
    if shape[1] * shape[2] <= 13 * 70:
        assert np.array_equal(sc.stem_direct_emul(x, w, shift), want) and np.array_equal(sc.stem_mfma_emul(x, sc.stem_wt(w), shift), want)


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 7, 7), (2, 13, 70)], ids=str)
def test_stem_restatements_inside_the_bound(shape):
    x, w, shift = sc.stem_data("random", *shape)
    for name, terms, K, emul in (("direct", False, sc.K_DIRECT, lambda: sc.stem_direct_emul(x, w, shift)),
                                 ("mfma", True, sc.K_MFMA, lambda: sc.stem_mfma_emul(x, sc.stem_wt(w), shift))):
        ref, mag = sc.stem_ref(x, w, shift, terms)
        _inside("stem %s %s" % (name, shape), emul(), sc.relu(ref), sc.stem_bound(ref, mag, K))


def test_stem_wrong_variants():
    x, w, shift, want, _ = sc.iso_data()
    wt = sc.stem_wt(w)
    assert np.array_equal(sc.stem_mfma_emul(x, wt, shift), want) and np.array_equal(sc.stem_direct_emul(x, w, shift), want)
    assert sc.is_bf16(want) and (want > 0).sum() == 64 * 147, "every tap of every channel meets a pixel exactly once"
    zero = np.zeros_like(want)
    for v in ("term2_dropped", "term1_dropped", "terms12_swapped_pitch"):
        _outside("stem isolate " + v, sc.stem_mfma_emul(x, wt, shift, v), want, zero)
    # a non-zero weight in the kx = 7 slot, a patch pitch off by a pixel: on real data
    xr, wr, sr = sc.stem_data("random", 2, 13, 70)
    ref, mag = sc.stem_ref(xr, wr, sr, True)
    bound = sc.stem_bound(ref, mag, sc.K_MFMA)
    wbad = sc.stem_wt(wr).reshape(3, 64, 7, 8, 4).copy()
    wbad[0, :, :, 7, :3] = wbad[0, :, :, 6, :3]
    _outside("stem kx7_nonzero", sc.stem_mfma_emul(xr, wbad.reshape(3, 64, 224), sr), sc.relu(ref), bound, 0.3)
    _outside("stem pw_off", sc.stem_mfma_emul(xr, sc.stem_wt(wr), sr, "pw_off"), sc.relu(ref), bound, 0.3)
    # the loop-top barrier removed = a second-trip tile from the first trip's patch: covered exactly by
    # test_stem_wrap_reference_has_the_period_of_its_images (more than 90 % of such a tile differs from its one correct value)


# ======================================================================================= 2. + 3. ffn_ln kernels
@pytest.mark.parametrize("JN", sc.COEF_SHAPES, ids=str)
def test_coef_restated(JN):
    J, N = JN
    for kind in ("exact", "random"):
        w2, gamma, beta, b2 = sc.coef_data(J, N, 3, kind)
        for bias in (b2, None):
            ref, bound = sc.coef_ref(w2, gamma, beta, bias)
            got = sc.coef_emul(w2, gamma, beta, bias)
            if kind == "exact":
                assert sc.is_f32(ref) and np.array_equal(got, ref)
            else:
                _inside("coef J%d N%d%s" % (J, N, "" if bias is not None else " no b2"), got, ref, bound)
    if N >= 504:
        ref, bound = sc.coef_ref(w2, gamma, beta, b2)
        for v in ("no_b2", "beta_is_gamma") + (("last_trip_lost",) if N > 512 else ()):
            _outside("coef J%d N%d %s" % (J, N, v), sc.coef_emul(w2, gamma, beta, b2, v), ref, bound, 0.3)
    assert sc.coef_d(N) == {8: 14, 504: 14, 512: 14, 520: 15, 1032: 16, 3072: 19}[N]


@pytest.mark.parametrize("J", sc.ROWSTATS_J)
def test_rowstats_restated(J):
    for rows in sc.ROWSTATS_ROWS:
        dy, t, coef = sc.rowstats_data(rows, J, "exact")
        ref, _ = sc.rowstats_ref(dy, t, coef, 8)
        assert sc.is_f32(ref) and np.array_equal(sc.rowstats_emul(dy, t, coef, 8), ref)
        for kind in ("random", "cancel"):
            dy, t, coef = sc.rowstats_data(rows, J, kind)
            for N in sc.ROWSTATS_N:
                ref, bound = sc.rowstats_ref(dy, t, coef, N)
                _inside("rowstats rows%d J%d N%d %s" % (rows, J, N, kind), sc.rowstats_emul(dy, t, coef, N), ref, bound)
    dy, t, coef = sc.rowstats_data(9, J, "random")
    ref, bound = sc.rowstats_ref(dy, t, coef, 3072)
    for v in ("inv_from_J", "wb_not_subtracted", "a_for_wb"):
        _outside("rowstats J%d %s" % (J, v), sc.rowstats_emul(dy, t, coef, 3072, v), ref, bound, 0.4)
    assert sc.rowstats_d(J) == (14 if J <= 512 else 22) and sc.rowstats_extra(3072) == 1 and sc.rowstats_extra(8) == 0


@pytest.mark.parametrize("J", sc.PG_J)
def test_param_grads_restated(J):
    for N in sc.PG_N:
        w2, dw2, db2, gamma, beta = sc.pg_data(J, N, "exact")
        dg, db, _, _ = sc.pg_ref(w2, dw2, db2, gamma, beta)
        assert sc.is_bf16(dg) and sc.is_bf16(db), "the exact case is not representable in bf16"
        eg, eb = sc.pg_emul(w2, dw2, db2, gamma, beta)
        assert np.array_equal(eg, dg) and np.array_equal(eb, db) and not np.signbit(eg[gamma == 0]).any()
        w2, dw2, db2, gamma, beta = sc.pg_data(J, N, "random")
        dg, db, bg, bb = sc.pg_ref(w2, dw2, db2, gamma, beta)
        eg, eb = sc.pg_emul(w2, dw2, db2, gamma, beta)
        _inside("param_grads J%d N%d dgamma" % (J, N), eg, dg, bg)
        _inside("param_grads J%d N%d dbeta" % (J, N), eb, db, bb)
        assert (eg[gamma == 0] == 0).all() and (gamma == 0).sum() == 2
    if J >= 129:
        for v in ("slab_off_by_one", "beta_dbeta_kept", "no_division", "ragged_block_lost"):
            eg, eb = sc.pg_emul(w2, dw2, db2, gamma, beta, v)
            err = np.maximum(np.abs(eg - dg) / np.where(bg > 0, bg, np.inf), np.abs(eb - db) / bb)
            print("[stem-ffn] variant param_grads J%d N%d %s: worst %.3g x bound" % (J, N, v, err.max()))
            assert (err > 2).mean() >= (0.02 if v == "ragged_block_lost" else 0.3)


def test_semantic_inputs_and_restatement():
    d = sc.semantic_data()
    assert int(d["flagged"].sum()) == sc.SEM_FLAGGED, "flagged columns: %d" % int(d["flagged"].sum())
    assert (np.abs(d["gamma"][~d["flagged"]]) >= 0.05).all() and np.isclose(np.abs(d["gamma"]), 0.0501).sum() == 4
    dg, db, bg, bb = sc.pg_ref(d["w2"], d["dw2"], d["db2"], d["gamma"], d["beta"], input_terms=True)
    eg, eb = sc.pg_emul(d["w2"], d["dw2"], d["db2"], d["gamma"], d["beta"])
    nz = d["gamma"] != 0
    _inside("semantic dgamma (gamma != 0)", eg[nz], d["dgamma"][nz], bg[nz])
    keep = ~d["flagged"]
    print("[stem-ffn] semantic restated: unflagged worst |err| / max |dgamma| %.4g" % (
        np.abs(eg - d["dgamma"])[keep].max() / np.abs(d["dgamma"]).max()))


@pytest.mark.parametrize("MJ", sc.RESCUE_CASES, ids=str)
def test_rescue_restated(MJ):
    d = sc.rescue_data(*MJ)
    fl = np.flatnonzero(sc.gain_is_small(d["gamma"], d["beta"]))
    assert tuple(fl) == sc.RESCUE_FLAGGED, "flagged columns %s" % (fl,)
    cols = list(fl)
    ref, bound = sc.rescue_ref(d, cols)
    _inside("rescue M%d J%d" % MJ, sc.rescue_emul(d, cols), ref, bound)
    if MJ[0] >= 255:
        wrong = dict(d)
        flat = np.full(MJ[0] * (sc.RESCUE_N + 8), 7.0)
        np.lib.stride_tricks.as_strided(flat, d["u"].shape, ((sc.RESCUE_N + 8) * 8, 8))[:] = d["u"]        # rows ldu = N + 8 apart
        wrong["u_wrong"] = flat[:MJ[0] * sc.RESCUE_N].reshape(MJ[0], sc.RESCUE_N)                          # ... read with ldu = N
        for v in ("u_pitch_N", "mean_dropped") + (("rows_beyond_256_lost",) if MJ[0] > 256 else ()):
            _outside("rescue M%d J%d %s" % (MJ + (v,)), sc.rescue_emul(wrong, cols, v), ref, bound, 0.5)
    assert sc.rescue_depth(MJ[0]) == {1: 9, 255: 9, 256: 9, 257: 10, 600: 11}[MJ[0]]
