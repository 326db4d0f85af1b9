"""Conformance of the 23 kernels of csrc/rowops.hip through the C ABI (ifseg_amd.hip), in the style of
test_gemm_conformance_gpu.py: operands and outputs are views inside larger allocations, 7s around the inputs, a sentinel around
the outputs that must be bit-identical after the call.  Data, fp64 references, the derived bounds and the case tables are in
_rowops_cases.py (its docstring holds the derivations); test_rowops_conformance_cpu.py checks them without a GPU.

Part A: ifseg_ln_fwd / ifseg_ln_fwd_pair / ifseg_ln_bwd / ifseg_ln_bwd_drop per element against the fp64 reference, every
        instantiation, both sides of every dispatch edge, the grid-stride loop of the backward over several trips
        (LN_BWD_BLOCKS patched to 3), idle blocks (768 blocks for 5 rows), both row maps, bf16 and fp32 gains.
Part B: the masks of ifseg_dropout / ifseg_dropout_fill / the fused dropout of ln_fwd and ln_bwd / ifseg_droppath_scale against
        the numpy restatement of splitmix64 and drop8, exactly.
Part C: the side kernels on integer-valued data, exactly; the elementwise kernels bit for bit against the same expression in torch.
Part D: argument rejection (return codes only; nothing is launched with a bad argument).
profiles/rowops_conformance.txt: the kernels seen in a trace of this file, the worst ratios, the wrong variants it catches.
"""
import ctypes

import numpy as np
import pytest
import torch

import _rowops_cases as rc
from test_gemm_conformance_gpu import (BAD_ARG, BAD_SHAPE, BF16, F32, GUARD, SENTINEL, _assert_surroundings, _bits, _dev,
                                       _flat_guarded, _guarded)

pytestmark = pytest.mark.gpu
I64 = torch.int64


# ------------------------------------------------------------------------------------------------ plumbing
def _t(a, dtype):
    """numpy values (representable in `dtype`) -> torch CPU tensor"""
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(dtype)


def _split(rows):
    """rows = B * rpb with the smallest B > 1 (a prime row count: rpb = 1)"""
    for b in range(2, rows + 1):
        if rows % b == 0:
            return b, rows // b
    return 1, 1


def _in(a, dev, strided=False, dtype=BF16, fill=GUARD, dims3=True):
    """an operand inside a guarded allocation: [B, rpb, C] with a gap between the batches (the RowMap division path), or
    contiguous and viewed as [B, rpb, C] (bs == rpb * ld: the collapsed map); 1-D operands are always dense"""
    t = _t(a, dtype)
    if a.ndim == 2 and dims3:
        B, rpb = _split(a.shape[0])
        t = t.view(B, rpb, a.shape[1])
        if strided:
            return _guarded(t, dtype, dev, 8, fill)[1]
    return _flat_guarded(t, dtype, dev, fill)[1]


class _Out:
    """an output inside an allocation filled with the sentinel (or with `init` values inside), the surroundings of which are
    compared bit for bit afterwards"""

    def __init__(self, shape, dev, strided=False, dtype=BF16, init=None, dims3=True):
        self.shape = tuple(shape)
        if len(shape) == 2 and dims3:
            B, rpb = _split(shape[0])
            lay = (B, rpb, shape[1])
        else:
            lay = self.shape
        if strided and len(lay) == 3:
            self.full, self.view = _guarded(lay, dtype, dev, 8, SENTINEL)
            self.inner = lambda f: f[:, 3:3 + lay[1], :lay[2]]
        else:
            self.full, self.view = _flat_guarded(lay, dtype, dev, SENTINEL)
            n = int(np.prod(lay))
            self.inner = lambda f: f[16:16 + n]
        if init is not None:
            self.view.copy_(_t(init, dtype).view(lay).to(dev))
        self.before = self.full.clone()

    def np(self):
        return self.view.double().cpu().numpy().reshape(self.shape)

    def f32(self):
        return self.view.float().cpu().numpy().reshape(self.shape)

    def check(self, what):
        _assert_surroundings(self.full, self.before, self.inner, what)


def _assert_within(what, out, ref, bound):
    r, at = rc.worst_ratio(out.np(), ref, bound)
    print("[part A] %s: worst |err|/bound %.3f at %s" % (what, r, at))
    assert r <= 1.0, "%s: |err| is %.3f of the bound at %s (got %r, ref %r)" % (what, r, at, out.np()[at], ref[at])
    out.check(what)


def _assert_exact(what, out, ref):
    got = out.np()
    bad = got != ref
    assert not bad.any(), "%s: %d of %d elements differ; first at %s: got %r, expected %r" % (
        what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), got[bad][0], ref[bad][0])
    out.check(what)


def _drop(case, dev, dps=rc.DROP_DPSCALE):
    """(p, seed, DropPath scales on the device, rows_per_batch) of a case with fused dropout"""
    if not case["drop"]:
        return None
    nb = (case["rows"] + rc.DROP_RPB - 1) // rc.DROP_RPB
    return (rc.DROP_P, rc.DROP_SEED, _in(np.array(dps[:nb], dtype=np.float32), dev, dtype=F32), rc.DROP_RPB)


def _params(d, case, dev):
    pdt = F32 if case["pf32"] else BF16
    return _in(d["gamma"], dev, dtype=pdt), _in(d["beta"], dev, dtype=pdt)


def _ids(cases):
    return [c["id"] for c in cases]


# =========================================================================================== part A: forward
@pytest.mark.parametrize("case", rc.FWD_CASES, ids=_ids(rc.FWD_CASES))
def test_ln_fwd(case):
    from ifseg_amd import hip
    dev = _dev()
    rows, C, st = case["rows"], case["C"], case["strided"]
    d = rc.case_inputs(case)
    x = _in(d["x"], dev, st)
    gamma, beta = _params(d, case, dev)
    resid = _in(d["resid"], dev, st) if case["resid"] else None
    y = _Out((rows, C), dev, st)
    mean, rstd = _Out((rows,), dev, dtype=F32), _Out((rows,), dev, dtype=F32)
    hip.ln_fwd(x, gamma, beta, y.view, mean.view, rstd.view, resid=resid, gelu=case["gelu"], drop=_drop(case, dev))
    torch.cuda.synchronize()
    ref = rc.ln_fwd_ref(d["x"], d["gamma"], d["beta"], case["gelu"], d["resid"] if case["resid"] else None, rc.case_keepscale(case))
    for name, out in (("mean", mean), ("rstd", rstd), ("y", y)):
        _assert_within("%s %s %s" % (case["id"], case["reach"], name), out, ref[name], ref[name + "_b"])


@pytest.mark.parametrize("first", ["ln", "identity"])
@pytest.mark.parametrize("C", rc.LN_WIDTHS)
def test_ln_fwd_pair(C, first):
    """ifseg_ln_fwd_pair at every width (gamma = NULL: the identity first stage): both stages against the reference -- the
    second from y as the kernel stored it -- and bit-identical to two calls"""
    from ifseg_amd import hip
    dev = _dev()
    rows = 13
    case = dict(rows=rows, C=C, drop=True, pf32=(C // 8) % 2 == 0, strided=(C // 8) % 3 != 0)
    d = rc.ln_inputs(rows, C, 8000 + C)
    pdt, key = (F32, "32") if case["pf32"] else (BF16, "16")
    g1, b1 = d["gamma" + key], d["beta" + key]
    g2, b2 = np.ascontiguousarray(g1[::-1]), np.ascontiguousarray(b1[::-1])
    st = case["strided"]
    x, resid = _in(d["x"], dev, st), _in(d["resid"], dev, st)
    G1, B1, G2, B2 = (_in(v, dev, dtype=pdt) for v in (g1, b1, g2, b2))
    if first == "identity":
        G1 = B1 = None
    drop = _drop(case, dev)
    y, y2 = _Out((rows, C), dev, st), _Out((rows, C), dev, not st)
    st4 = [_Out((rows,), dev, dtype=F32) for _ in range(4)]
    m1, r1 = (st4[0].view, st4[1].view) if G1 is not None else (None, None)
    hip.ln_fwd_pair(x, G1, B1, y.view, m1, r1, G2, B2, y2.view, st4[2].view, st4[3].view, resid=resid, drop=drop)
    torch.cuda.synchronize()
    ks = rc.case_keepscale(case)
    ref = rc.ln_fwd_ref(d["x"], None if first == "identity" else g1, b1, False, d["resid"], ks)
    what = "pair-%s-13x%d" % (first, C)
    _assert_within(what + " y", y, ref["y"], ref["y_b"])
    if first == "ln":
        _assert_within(what + " mean", st4[0], ref["mean"], ref["mean_b"])
        _assert_within(what + " rstd", st4[1], ref["rstd"], ref["rstd_b"])
    ref2 = rc.ln_fwd_ref(y.f32(), g2, b2)
    _assert_within(what + " y2", y2, ref2["y"], ref2["y_b"])
    _assert_within(what + " mean2", st4[2], ref2["mean"], ref2["mean_b"])
    _assert_within(what + " rstd2", st4[3], ref2["rstd"], ref2["rstd_b"])
    # two calls
    ya, y2a = torch.empty(rows, C, dtype=BF16, device=dev), torch.empty(rows, C, dtype=BF16, device=dev)
    sa = [torch.empty(rows, dtype=F32, device=dev) for _ in range(4)]
    B, rpb = _split(rows)
    if first == "ln":
        hip.ln_fwd(x, G1, B1, ya.view(B, rpb, C), sa[0], sa[1], resid=resid, drop=drop)
    else:
        hip.dropout(x, resid, ya.view(B, rpb, C), drop[0], drop[1], drop[2], drop[3])
    hip.ln_fwd(ya, G2, B2, y2a, sa[2], sa[3])
    torch.cuda.synchronize()
    assert torch.equal(_bits(ya.view(-1)), _bits(y.view.reshape(-1))) and torch.equal(_bits(y2a.view(-1)), _bits(y2.view.reshape(-1)))
    for k in range(0 if first == "ln" else 2, 4):
        assert torch.equal(_bits(sa[k]), _bits(st4[k].view)), k


# ========================================================================================== part A: backward
def _stats(hip, x, gamma, beta, rows, C, gelu, dev):
    """mean / rstd as the forward kernel produces them"""
    mean, rstd = torch.empty(rows, dtype=F32, device=dev), torch.empty(rows, dtype=F32, device=dev)
    hip.ln_fwd(x, gamma, beta, torch.empty(x.shape, dtype=BF16, device=dev), mean, rstd, gelu=gelu)
    return mean, rstd


def _assert_partials(case, dgp, dbp):
    """no block leaves its slot unwritten; blocks that own no row write zeros"""
    per_block = 4 if rc.bwd_waves_per_row(case["C"], case["gelu"]) == 1 else 1
    owned = min(case["nblocks"], (case["rows"] + per_block - 1) // per_block)
    for p in (dgp, dbp):
        assert not bool((p.view == SENTINEL).any()), "%s: a block did not write its partial sums" % case["id"]
        assert bool((p.view[owned:] == 0).all()), "%s: a block without rows wrote non-zero partial sums" % case["id"]
        p.check(case["id"] + " partials")


def _reduce(hip, part, nb, C, dev):
    out = _Out((C,), dev, dtype=F32)
    hip.reduce_parts(part.view, out.view, 1, nb, C)
    return out


@pytest.mark.parametrize("case", rc.BWD_CASES, ids=_ids(rc.BWD_CASES))
def test_ln_bwd(case, monkeypatch):
    from ifseg_amd import hip
    dev = _dev()
    rows, C, st, nb = case["rows"], case["C"], case["strided"], case["nblocks"]
    monkeypatch.setattr(hip, "LN_BWD_BLOCKS", nb)
    d = rc.case_inputs(case, backward=True)
    x, dy = _in(d["x"], dev, st), _in(d["dy"], dev, st)
    gamma, beta = _params(d, case, dev)
    add = _in(d["add"], dev, st) if case["add"] else None
    mean, rstd = _stats(hip, x, gamma, beta, rows, C, case["gelu"], dev)
    dx = _Out((rows, C), dev, st)
    dgp, dbp = _Out((nb, C), dev, dtype=F32, dims3=False), _Out((nb, C), dev, dtype=F32, dims3=False)
    hip.ln_bwd(dy, x, gamma, mean, rstd, dx.view, dgp.view, dbp.view, dx_add=add, gelu=case["gelu"], drop=_drop(case, dev))
    dg, db = _reduce(hip, dgp, nb, C, dev), _reduce(hip, dbp, nb, C, dev)
    torch.cuda.synchronize()
    ref = rc.ln_bwd_ref(d["dy"], d["x"], d["gamma"], mean.cpu().numpy(), rstd.cpu().numpy(), case["gelu"],
                        d["add"] if case["add"] else None, rc.case_keepscale(case))
    what = "%s %s " % (case["id"], case["reach"])
    _assert_within(what + "dx", dx, ref["dx"], ref["dx_b"])
    _assert_within(what + "dgamma", dg, ref["dgamma"], ref["dgamma_b"])
    _assert_within(what + "dbeta", db, ref["dbeta"], ref["dbeta_b"])
    _assert_partials(case, dgp, dbp)


@pytest.mark.parametrize("case", rc.BWD_DROP_CASES, ids=_ids(rc.BWD_DROP_CASES))
def test_ln_bwd_drop(case, monkeypatch):
    """ifseg_ln_bwd_drop: dx and the partial sums against the reference, dx2 = drop2(dx as stored) against the restated mask, and
    everything bit-identical to ifseg_ln_bwd followed by ifseg_dropout"""
    from ifseg_amd import hip
    dev = _dev()
    rows, C, st, nb = case["rows"], case["C"], case["strided"], case["nblocks"]
    monkeypatch.setattr(hip, "LN_BWD_BLOCKS", nb)
    d = rc.case_inputs(case, backward=True)
    x, dy = _in(d["x"], dev, st), _in(d["dy"], dev, st)
    gamma, beta = _params(d, case, dev)
    add = _in(d["add"], dev, st) if case["add"] else None
    mean, rstd = _stats(hip, x, gamma, beta, rows, C, False, dev)
    drop = _drop(case, dev)
    dx, dx2 = _Out((rows, C), dev, st), _Out((rows, C), dev, not st)
    dgp, dbp = _Out((nb, C), dev, dtype=F32, dims3=False), _Out((nb, C), dev, dtype=F32, dims3=False)
    hip.ln_bwd_drop(dy, x, gamma, mean, rstd, dx.view, dgp.view, dbp.view, dx2.view, dx_add=add, drop2=drop)
    dg, db = _reduce(hip, dgp, nb, C, dev), _reduce(hip, dbp, nb, C, dev)
    torch.cuda.synchronize()
    ref = rc.ln_bwd_ref(d["dy"], d["x"], d["gamma"], mean.cpu().numpy(), rstd.cpu().numpy(), False, d["add"] if case["add"] else None)
    what = "%s %s " % (case["id"], case["reach"])
    _assert_within(what + "dx", dx, ref["dx"], ref["dx_b"])
    _assert_within(what + "dgamma", dg, ref["dgamma"], ref["dgamma_b"])
    _assert_within(what + "dbeta", db, ref["dbeta"], ref["dbeta_b"])
    _assert_partials(case, dgp, dbp)
    ks = rc.case_keepscale(case).astype(np.float64)
    want2 = dx.np() * ks                                             # one fp32 product, one rounding to bf16
    _assert_within(what + "dx2", dx2, want2, rc.U_BF16 * np.abs(want2) * (1 + 2.0 ** -10))
    nz = dx.np() != 0
    assert ((dx2.np() != 0) == (ks != 0))[nz].all(), what + "dx2: the keep pattern differs from the restated mask"
    # two calls
    B, rpb = _split(rows)
    dxa, dx2a = torch.empty(B, rpb, C, dtype=BF16, device=dev), torch.empty(B, rpb, C, dtype=BF16, device=dev)
    pga, pba = torch.empty(nb, C, dtype=F32, device=dev), torch.empty(nb, C, dtype=F32, device=dev)
    hip.ln_bwd(dy, x, gamma, mean, rstd, dxa, pga, pba, dx_add=add)
    hip.dropout(dxa, None, dx2a, drop[0], drop[1], drop[2], drop[3])
    torch.cuda.synchronize()
    assert torch.equal(_bits(dxa.view(-1)), _bits(dx.view.reshape(-1))) and torch.equal(_bits(dx2a.view(-1)), _bits(dx2.view.reshape(-1)))
    assert torch.equal(_bits(pga), _bits(dgp.view)) and torch.equal(_bits(pba), _bits(dbp.view))


# ================================================================================================== part B
SEED_ADD = 0xC3A5C85C97CB3127         # bit 63 set as well: seed + seed_add wraps


@pytest.mark.parametrize("use_add", [False, True], ids=["seed", "seed+add"])
@pytest.mark.parametrize("p", rc.MASK_PS)
@pytest.mark.parametrize("C", rc.MASK_WIDTHS)
def test_masks_against_the_restatement(C, p, use_add, monkeypatch):
    from ifseg_amd import hip
    dev = _dev()
    rows, rpb, seed = rc.MASK_ROWS, rc.DROP_RPB, rc.DROP_SEED
    monkeypatch.setattr(hip, "LN_BWD_BLOCKS", 3)
    d = rc.mask_ln_inputs(C)
    xv = np.where(d["x"] == 0, np.float32(1), d["x"])
    dps = np.array(rc.MASK_DPSCALE, dtype=np.float32)
    add_word = torch.tensor([SEED_ADD - (1 << 64)], dtype=I64, device=dev) if use_add else None
    keep = rc.drop_keep(rows, C, p, seed, SEED_ADD if use_add else 0)
    ks = rc.drop_keepscale(rows, C, p, seed, dps, rpb, SEED_ADD if use_add else 0)
    assert keep.all() if p == 0 else not keep.all()
    what = "masks %dx%d p%g%s: " % (rows, C, p, "+add" if use_add else "")
    prev = hip.set_seed_add(add_word)
    try:
        dps_t = _in(dps, dev, dtype=F32)
        # ifseg_dropout: strided in, contiguous out; then with a residual
        x = _in(xv, dev, True)
        out = _Out((rows, C), dev)
        hip.dropout(x, None, out.view, p, seed, dps_t, rpb)
        torch.cuda.synchronize()
        assert ((out.np() != 0) == keep).all(), what + "ifseg_dropout keeps other elements than the restatement"
        want = xv.astype(np.float64) * ks
        _assert_within(what + "dropout", out, want, rc.U_BF16 * np.abs(want) * (1 + 2.0 ** -10))
        res = rc.ln_inputs(rows, C, 4100 + C)["resid"]
        out = _Out((rows, C), dev, True)
        hip.dropout(x, _in(res, dev), out.view, p, seed, dps_t, rpb)
        torch.cuda.synchronize()
        want = want + res
        _assert_within(what + "dropout + resid", out, want, rc.U_BF16 * np.abs(want) + (1 + rc.U_BF16) * rc.U * 4 * (np.abs(want) + np.abs(res)))
        # ifseg_dropout_fill: no scale, no DropPath, dropped -> fill
        xf = _flat_guarded(_t(xv, BF16), BF16, dev, GUARD)[1]
        out = _Out((rows, C), dev, dims3=False)
        hip.dropout_fill(xf, out.view, p, seed, fill=-30.0)
        torch.cuda.synchronize()
        _assert_exact(what + "dropout_fill", out, np.where(keep, xv, np.float32(-30.0)).astype(np.float64))
        # the fused dropout of ln_fwd: the dropped positions, then the values
        gamma, beta = _in(d["gamma"], dev), _in(d["beta"], dev)
        x = _in(d["x"], dev, True)
        y = _Out((rows, C), dev, True)
        mean, rstd = _Out((rows,), dev, dtype=F32), _Out((rows,), dev, dtype=F32)
        hip.ln_fwd(x, gamma, beta, y.view, mean.view, rstd.view, drop=(p, seed, dps_t, rpb))
        torch.cuda.synchronize()
        assert ((y.np() == 0) == ~keep).all(), what + "ln_fwd drops other elements than the restatement"
        ref = rc.ln_fwd_ref(d["x"], d["gamma"], d["beta"], ks=ks)
        _assert_within(what + "ln_fwd y", y, ref["y"], ref["y_b"])
        # the adjoint in ln_bwd: the backward bound on the masked dy
        dy = _in(d["dy"], dev)
        dx = _Out((rows, C), dev)
        dgp, dbp = _Out((3, C), dev, dtype=F32, dims3=False), _Out((3, C), dev, dtype=F32, dims3=False)
        hip.ln_bwd(dy, x, gamma, mean.view, rstd.view, dx.view, dgp.view, dbp.view, drop=(p, seed, dps_t, rpb))
        dg, db = _reduce(hip, dgp, 3, C, dev), _reduce(hip, dbp, 3, C, dev)
        torch.cuda.synchronize()
        bref = rc.ln_bwd_ref(d["dy"], d["x"], d["gamma"], mean.f32(), rstd.f32(), ks=ks)
        _assert_within(what + "ln_bwd dx", dx, bref["dx"], bref["dx_b"])
        _assert_within(what + "ln_bwd dgamma", dg, bref["dgamma"], bref["dgamma_b"])
        _assert_within(what + "ln_bwd dbeta", db, bref["dbeta"], bref["dbeta_b"])
    finally:
        hip.set_seed_add(prev)


@pytest.mark.parametrize("use_add", [False, True], ids=["seed", "seed+add"])
def test_droppath_scale_against_the_restatement(use_add):
    from ifseg_amd import hip
    dev = _dev()
    keep = np.array([0.0, 0.25, 1.0, 0.25], dtype=np.float32)
    B = 65                                                   # 4 x 65 = 260 elements: two blocks
    want = rc.droppath_scale(keep, B, rc.DROP_SEED, SEED_ADD if use_add else 0)
    assert set(np.unique(want[1])) == {0.0, 4.0}
    out = _Out((4, B), dev, dtype=F32, dims3=False)
    prev = hip.set_seed_add(torch.tensor([SEED_ADD - (1 << 64)], dtype=I64, device=dev) if use_add else None)
    try:
        hip.droppath_scale(out.view, _in(keep, dev, dtype=F32), rc.DROP_SEED)
        torch.cuda.synchronize()
    finally:
        hip.set_seed_add(prev)
    _assert_exact("droppath_scale", out, want.astype(np.float64))


# ================================================================================================== part C
@pytest.mark.parametrize("ends", [False, True], ids=["mixed", "ends"])
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
@pytest.mark.parametrize("C", [8, 2056])
def test_rows_segment_sum(C, weighted, ends):
    from ifseg_amd import hip
    dev = _dev()
    c = rc.segment_sum_case(C, weighted, ends)
    src = _in(c["src"], dev, dims3=False)
    w = _in(c["w"], dev, dtype=F32) if weighted else None
    tg = _Out((c["V"], C), dev, init=c["prior"], dims3=False)
    hip.rows_segment_sum(src, torch.from_numpy(c["src_row"]).to(dev), w, torch.from_numpy(c["ids"]).to(dev), tg.view, skip_id=c["skip"])
    torch.cuda.synchronize()
    _assert_exact("rows_segment_sum C %d" % C, tg, c["ref"])
    idle = torch.from_numpy(~c["touched"]).to(dev)
    assert torch.equal(_bits(tg.view[idle]), _bits(tg.inner(tg.before).view(c["V"], C)[idle])), "an untouched table row changed"


@pytest.mark.parametrize("with_add", [True, False], ids=["add", "noadd"])
@pytest.mark.parametrize("C", rc.EMBED_WIDTHS)
def test_embed_rows_and_bags(C, with_add):
    from ifseg_amd import hip
    dev = _dev()
    e = rc.embed_case(C, rc.BAG_SIZES_EXACT, with_add)
    table = _in(e["table"], dev, dims3=False)
    add = _in(e["add"], dev) if with_add else None
    ids = torch.from_numpy(e["ids"]).to(dev)
    B, n = e["ids"].shape
    for strided in (True, False):
        full, view = _guarded((B, n, C), BF16, dev, 8, SENTINEL)
        if not strided:
            full, view = _flat_guarded((B * n, C), BF16, dev, SENTINEL)
        before = full.clone()
        hip.embed_rows(table, ids, add, view)
        torch.cuda.synchronize()
        got = view.double().cpu().numpy().reshape(B, n, C)
        assert (got == e["rows_ref"]).all(), "embed_rows C %d strided %s" % (C, strided)
        _assert_surroundings(full, before, (lambda f: f[:, 3:3 + n, :C]) if strided else (lambda f: f[16:16 + B * n * C]), "embed_rows")
    ends = torch.from_numpy(e["ends"].reshape(-1)).to(dev)
    P = e["ends"].shape[1]
    full, view = _guarded((B, P, C), BF16, dev, 8, SENTINEL)
    before = full.clone()
    hip.embed_bag_mean(table, ids, ends, add, view)
    torch.cuda.synchronize()
    assert (view.double().cpu().numpy() == e["bag_ref"]).all(), "embed_bag_mean C %d" % C
    _assert_surroundings(full, before, lambda f: f[:, 3:3 + P, :C], "embed_bag_mean")
    if with_add:      # bags of 3 and 5: 1 / n is rounded, one more rounding for the product and the sum each
        e = rc.embed_case(C, rc.BAG_SIZES_ROUNDED)
        out = _Out((B * P, C), dev, dims3=False)
        hip.embed_bag_mean(table, torch.from_numpy(e["ids"]).to(dev), torch.from_numpy(e["ends"].reshape(-1)).to(dev), add, out.view)
        torch.cuda.synchronize()
        ref = e["bag_ref"].reshape(B * P, C)
        _assert_within("embed_bag_mean (3, 5) C %d" % C, out, ref, rc.U_BF16 * np.abs(ref) + (1 + rc.U_BF16) * rc.U * 4 * e["bag_mag"].reshape(B * P, C))


@pytest.mark.parametrize("n,H", rc.REL_SHAPES)
def test_rel_gather_and_scatter(n, H):
    from ifseg_amd import hip
    dev = _dev()
    for L in (1, 16):
        r = rc.rel_case(n, H, L)
        tables = [_in(r["tables"][l], dev, dims3=False) for l in range(L)]
        idx = torch.from_numpy(r["idx"]).to(dev)
        out = _Out((L, H, n), dev, dtype=F32)
        hip.rel_gather_multi(tables, idx, out.view)
        torch.cuda.synchronize()
        _assert_exact("rel_gather_multi %dx%d L %d" % (n, H, L), out, r["gathered"])
    r = rc.rel_case(n, H, 1)
    out = _Out((H, n), dev, dtype=F32, dims3=False)
    hip.rel_gather(_in(r["tables"][0], dev, dims3=False), torch.from_numpy(r["idx"]).to(dev), out.view)
    acc = _Out((r["nb"], H), dev, dtype=F32, init=r["prior"], dims3=False)
    hip.rel_scatter_add(_in(r["d"], dev, dtype=F32, dims3=False), torch.from_numpy(r["idx"]).to(dev), acc.view)
    torch.cuda.synchronize()
    _assert_exact("rel_gather %dx%d" % (n, H), out, r["gathered"][0])
    _assert_exact("rel_scatter_add %dx%d" % (n, H), acc, r["acc"])


@pytest.mark.parametrize("N,C", rc.KPROJ_SHAPES)
def test_kproj_common_mode(N, C):
    from ifseg_amd import hip
    dev = _dev()
    k = rc.kproj_case(N, C)
    gw = _Out((N, C), dev, init=k["gw"], dims3=False)
    hip.kproj_common_mode(gw.view, _in(k["db"], dev), _in(k["xmean"], dev, dtype=F32))
    torch.cuda.synchronize()
    _assert_exact("kproj_common_mode %dx%d" % (N, C), gw, k["ref"])


@pytest.mark.parametrize("M,N", rc.COLSUM_SHAPES)
def test_colsum_and_col_mean(M, N):
    from ifseg_amd import hip
    dev = _dev()
    c = rc.colsum_case(M, N)
    for strided in (False, True):
        x = _in(c["x"], dev, strided)
        part = _Out((hip.COLSUM_BLOCKS, N), dev, dtype=F32, dims3=False)
        hip.colsum(x, part.view)
        out = _reduce(hip, part, hip.COLSUM_BLOCKS, N, dev)
        torch.cuda.synchronize()
        _assert_exact("colsum %dx%d" % (M, N), out, c["sum"])
        part.check("colsum partials")
    # the mean: the exact integer sum times fp32(1 / rows), one fp32 product (exact for a power-of-two row count)
    def mean_of(v):
        return (v.astype(np.float64).sum(0).astype(np.float32) * np.float32(1.0 / v.shape[0])).astype(np.float64)

    x2 = _in(c["x"], dev, dims3=False)
    ws = _Out((hip.COLSUM_BLOCKS + 1, N), dev, dtype=F32, dims3=False)
    got = hip.col_mean(x2, ws.view).double().cpu().numpy()
    assert (got == mean_of(c["x"])).all(), "col_mean %dx%d" % (M, N)
    got = hip.col_mean(x2, ws.view, every=8).double().cpu().numpy()
    sub = c["x"][:M // 8 * 8:8] if M >= 64 * 8 else c["x"]      # below 64 * every rows the mean is over every row
    assert (got == mean_of(sub)).all(), "col_mean every=8 %dx%d" % (M, N)
    ws.check("col_mean workspace")


@pytest.mark.parametrize("case", rc.REDUCE_CASES, ids=[c["reach"] + "-" + c["id"] for c in rc.REDUCE_CASES])
def test_reduce_parts(case):
    from ifseg_amd import hip
    dev = _dev()
    r = rc.reduce_case(case)
    inp = _flat_guarded(_t(r["inp"], F32), F32, dev, GUARD)[1]
    out = _Out((case["outer"], case["n"]), dev, dtype=BF16 if case["bf16"] else F32, init=r["prev"], dims3=False)
    hip.reduce_parts(inp, out.view, case["outer"], case["parts"], case["n"], accumulate=case["acc"], scale=case["scale"])
    torch.cuda.synchronize()
    _assert_exact("reduce_parts " + case["id"], out, r["ref"])


SIZES = (1, 3, 4, 5, 7, 8, 9, 1023, 1024, 1025)


def _specials(n, seed):
    """fp32 values with -0, subnormals, +-Inf and NaN among them"""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(n, generator=g) * 3
    sp = torch.tensor([-0.0, 1e-40, -3e-39, float("inf"), float("-inf"), float("nan"), 2.0 ** -126, 1.00390625, 3.3895314e38])
    k = torch.randperm(n, generator=g)[:min(n, sp.numel())]
    v[k] = sp[:k.numel()]
    return v


def _same(got, want, what):
    """bit for bit, NaN by isnan"""
    got, want = got.cpu(), want.cpu()
    assert torch.equal(torch.isnan(got.float()), torch.isnan(want.float())), what + ": NaNs differ"
    ok = ~torch.isnan(want.float())
    assert torch.equal(_bits(got.contiguous())[ok], _bits(want.contiguous())[ok]), what


@pytest.mark.parametrize("n", SIZES)
def test_elementwise_bit_for_bit(n):
    from ifseg_amd import hip
    dev = _dev()
    a32, b32 = _specials(n, n), _specials(n, n + 7)
    for scale in (1.0, 2.0):
        out = _Out((n,), dev)
        hip.cast_f32_bf16(_flat_guarded(a32, F32, dev, GUARD)[1], out.view, scale)
        torch.cuda.synchronize()
        _same(out.view, (a32 * scale).to(BF16), "cast_f32_bf16 n %d scale %g" % (n, scale))
        out.check("cast_f32_bf16")
    a16, b16 = a32.to(BF16), b32.to(BF16)
    out = _Out((n,), dev)
    hip.add_bf16(_flat_guarded(a16, BF16, dev, GUARD)[1], _flat_guarded(b16, BF16, dev, GUARD)[1], out.view)
    torch.cuda.synchronize()
    _same(out.view, (a16.float() + b16.float()).to(BF16), "add_bf16 n %d" % n)
    out.check("add_bf16")
    # sync_master: half of the entries still are the rounding of the master (with more precision than bf16 holds)
    master = _specials(n, n + 11)
    p16 = master.to(BF16)
    stale = torch.arange(n) % 2 == 1
    stale &= ~torch.isnan(master)
    p16[stale] = (p16[stale].float() * 1.5 + 1.0).to(BF16)
    stale &= _bits(p16) != _bits(master.to(BF16))
    full, view = _flat_guarded(master, F32, dev, SENTINEL)
    before = full.clone()
    hip.sync_master(view, _flat_guarded(p16, BF16, dev, GUARD)[1])
    torch.cuda.synchronize()
    _same(view, torch.where(stale, p16.float(), master), "sync_master n %d" % n)
    _assert_surroundings(full, before, lambda f: f[16:16 + n], "sync_master")


@pytest.mark.parametrize("shape", [(1, 1, 1, 1, 1), (1, 3, 11, 31, 3), (1, 3, 16, 16, 4), (1, 3, 5, 41, 5), (2, 3, 5, 7, 4)])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_nchw_to_nhwc_bit_for_bit(shape, dtype):
    from ifseg_amd import hip
    dev = _dev()
    B, C, H, W, Cp = shape
    x = _specials(B * C * H * W, 5).view(B, C, H, W).to(dtype)
    want = torch.zeros(B, H, W, Cp, dtype=BF16)
    want[..., :C] = x.permute(0, 2, 3, 1).to(BF16)
    out = _Out((B * H * W * Cp,), dev)
    hip.nchw_to_nhwc(_flat_guarded(x, dtype, dev, GUARD)[1], out.view, Cp)
    torch.cuda.synchronize()
    _same(out.view, want.view(-1), "nchw_to_nhwc %s %s" % (shape, dtype))
    out.check("nchw_to_nhwc")


def test_check_inputs_truth_tables():
    """all four modes; the verdict lands in one pinned byte whose neighbours keep their sentinel"""
    from ifseg_amd import hip
    dev = _dev()
    verdict = torch.full((16,), 0x5A, dtype=torch.uint8).pin_memory()
    L = hip.lib()

    def run(x, mode, value=0, row_len=1, n=None):
        verdict[7] = 0x33
        if n is None:
            hip.check_inputs(x, mode, verdict, 7, value, row_len)
        else:
            assert L.ifseg_check_inputs(ctypes.c_void_p(x.data_ptr()), ctypes.c_longlong(n), ctypes.c_int(mode), ctypes.c_longlong(value),
                                        ctypes.c_longlong(row_len), ctypes.c_void_p(verdict.data_ptr() + 7), hip._stream()) == 0
        torch.cuda.synchronize()
        v = int(verdict[7])
        assert v in (0, 1) and all(int(verdict[k]) == 0x5A for k in range(16) if k != 7), verdict
        return v

    spare = torch.full((8,), 9, dtype=I64, device=dev)
    for mode in (0, 1, 2):
        assert run(spare, mode, value=9, n=0) == 0                      # nothing to look at
    for n in (1, 255, 256, 257):
        for hit, want in ((None, 0), (0, 1), (n - 1, 1)):
            x = torch.full((n,), 4, dtype=I64)
            b = torch.ones(n, dtype=torch.bool)
            if hit is not None:
                x[hit], b[hit] = 9, False
            assert run(x.to(dev), 0, value=9) == want, ("mode 0", n, hit)
            assert run(b.to(dev), 2) == want, ("mode 2", n, hit)
        assert run(torch.full((n,), 4, dtype=I64, device=dev), 0, value=-4) == 0
    # mode 1: rows of row_len; `value` may only be a suffix of its row
    P = 9
    tables = [([[1, 2, P], [3, 4, 5]], 0),            # the value at the end of a row
              ([[1, 2, 3], [P, 4, P]], 1),            # at a row start
              ([[1, P, 3], [4, 5, 6]], 1),            # followed by a non-value
              ([[1, P, P], [2, 3, 4]], 0),            # a row ending in the value, the next starting with a non-value
              ([[1, 2, 3], [4, 5, 6]], 0), ([[1, 2, 3], [4, P, P]], 0), ([[1, 2, 3], [4, P, 5]], 1), ([[P, P, P], [1, 2, 3]], 1)]
    for rows_, want in tables:
        assert run(torch.tensor(rows_, dtype=I64, device=dev), 1, value=P, row_len=3) == want, rows_
    for n in (255, 256, 257):                          # one long row: the last entry / an entry before the last
        x = torch.full((1, n), 4, dtype=I64)
        x[0, n - 1] = P
        assert run(x.to(dev), 1, value=P, row_len=n) == 0
        x[0, n - 1], x[0, n - 2] = 4, P
        assert run(x.to(dev), 1, value=P, row_len=n) == 1
        x = torch.full((n, 1), 4, dtype=I64)           # n rows of one entry: a row start
        assert run(x.to(dev), 1, value=P, row_len=1) == 0
        x[n - 1, 0] = P
        assert run(x.to(dev), 1, value=P, row_len=1) == 1
    # mode 3: the flag is returned and cleared
    flag = torch.tensor([5, 77], dtype=torch.int32, device=dev)
    assert run(flag, 3) == 1
    assert flag.tolist() == [0, 77]
    assert run(flag, 3) == 0 and flag.tolist() == [0, 77]


# ================================================================================================== part D
def test_bad_arguments_are_refused():
    """return codes only: every call below is refused before a launch, and nothing is written"""
    from ifseg_amd import hip
    dev = _dev()
    L = hip.lib()
    i, ll, f, P = ctypes.c_int, ctypes.c_longlong, ctypes.c_float, lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    u64 = ctypes.c_ulonglong
    S = hip._stream()
    X = torch.ones(64, 8192, dtype=BF16, device=dev)
    G = torch.ones(8192, dtype=BF16, device=dev)
    Y = torch.full((64, 8192), SENTINEL, dtype=BF16, device=dev)
    Y2 = torch.full((64, 8192), SENTINEL, dtype=BF16, device=dev)
    ST = torch.full((4, 64), SENTINEL, dtype=F32, device=dev)
    PART = torch.full((8, 8192), SENTINEL, dtype=F32, device=dev)
    IDS = torch.zeros(64, dtype=I64, device=dev)
    want = [t.clone() for t in (Y, Y2, ST, PART)]
    m, r = ctypes.c_void_p(ST[0].data_ptr()), ctypes.c_void_p(ST[1].data_ptr())
    m2, r2 = ctypes.c_void_p(ST[2].data_ptr()), ctypes.c_void_p(ST[3].data_ptr())
    pg, pb = ctypes.c_void_p(PART[:4].data_ptr()), ctypes.c_void_p(PART[4:].data_ptr())
    GELU = 1

    def drop(p, rpb=4):
        return ctypes.byref(hip._DropArgs(p, 1, None, rpb, None))

    def fwd(C=64, ldx=8192, ldy=8192, ldr=8192, resid=None, flags=0, dr=None):
        return L.ifseg_ln_fwd(P(X), P(G), P(G), P(resid), P(Y), m, r, i(8), i(C), f(1e-5), i(flags), i(0), ll(0), i(ldx), ll(0), i(ldy),
                              ll(0), i(ldr), dr, S)

    def pair(C=64, flags=0, y2=Y2, g2=G, ldy2=8192, beta_only=False):
        return L.ifseg_ln_fwd_pair(P(X), None if beta_only else P(G), P(G), None, P(Y), m, r, P(g2), P(g2), P(y2), m2, r2, i(8), i(C), f(1e-5),
                                   i(flags), i(0), ll(0), i(8192), ll(0), i(8192), ll(0), i(0), ll(0), i(ldy2), None, S)

    def bwd(C=64, nb=4, lddy=8192, ldx=8192, lddx=8192, ldadd=8192, add=None, flags=0, dr=None):
        return L.ifseg_ln_bwd(P(X), P(X), P(G), m, r, P(add), P(Y), pg, pb, i(nb), i(8), i(C), i(flags), i(0), ll(0), i(lddy), ll(0), i(ldx),
                              ll(0), i(lddx), ll(0), i(ldadd), dr, S)

    def bwd_drop(C=64, nb=4, lddy=8192, lddx2=8192, ldadd=8192, add=None, flags=0, dx2=Y2, dr=None):
        return L.ifseg_ln_bwd_drop(P(X), P(X), P(G), m, r, P(add), P(Y), pg, pb, P(dx2), i(nb), i(8), i(C), i(flags), i(0), ll(0), i(lddy),
                                   ll(0), i(8192), ll(0), i(8192), ll(0), i(ldadd), ll(0), i(lddx2), dr, S)

    def dropout(C=64, p=0.1, ldx=8192, ldo=8192, ldr=8192, resid=None, rpb=0, x_bs=0, rows_per_batch=4):
        return L.ifseg_dropout(P(X), P(resid), P(Y), ll(8), i(C), f(p), u64(1), None, i(rows_per_batch), i(rpb), ll(x_bs), i(ldx), ll(0), i(ldr),
                               ll(0), i(ldo), None, S)

    def colsum(N=64, ldx=8192, nblk=4):
        return L.ifseg_colsum_bf16(P(X), pg, i(nblk), i(8), i(N), i(0), ll(0), i(ldx), S)

    def embed(C=64, ldo=8192):
        return L.ifseg_embed_rows(P(X), P(IDS), None, P(Y), i(8), i(C), i(0), ll(0), i(ldo), S)

    def bag(C=64, ldo=8192, maxlen=4):
        return L.ifseg_embed_bag_mean(P(X), P(IDS), P(IDS), None, P(Y), i(2), i(2), i(C), i(maxlen), i(0), ll(0), i(ldo), S)

    def check(n, mode, row_len=1, x=IDS):
        return L.ifseg_check_inputs(P(x), ll(n), i(mode), ll(0), ll(row_len), P(Y), S)

    tabs = (ctypes.c_void_p * 17)(*[X.data_ptr()] * 17)
    calls = {
        # ---- refused before this suite
        "ln_fwd C % 8": (fwd(C=60), BAD_SHAPE), "ln_fwd C > 4096": (fwd(C=4104), BAD_SHAPE), "ln_fwd ldx % 8": (fwd(ldx=8188), BAD_SHAPE),
        "ln_fwd ldy % 8": (fwd(ldy=8188), BAD_SHAPE), "ln_fwd ldr % 8": (fwd(resid=X, ldr=8188), BAD_SHAPE),
        "ln_fwd p = 1": (fwd(dr=drop(1.0)), BAD_ARG), "ln_fwd p < 0": (fwd(dr=drop(-0.1)), BAD_ARG),
        "ln_fwd rows_per_batch = 0": (fwd(dr=drop(0.1, 0)), BAD_ARG),
        "pair with GELU": (pair(flags=GELU), BAD_ARG), "pair without y2": (pair(y2=None), BAD_ARG),
        "pair without gamma2": (pair(g2=None), BAD_ARG), "pair with beta and no gamma": (pair(beta_only=True), BAD_ARG),
        "pair ldy2 % 8": (pair(ldy2=8188), BAD_SHAPE), "pair C > 4096": (pair(C=4104), BAD_SHAPE),
        "ln_bwd C % 8": (bwd(C=60), BAD_SHAPE), "ln_bwd C > 4096": (bwd(C=4104), BAD_SHAPE), "ln_bwd nblocks = 0": (bwd(nb=0), BAD_SHAPE),
        "ln_bwd nblocks < 0": (bwd(nb=-3), BAD_SHAPE), "ln_bwd p = 1": (bwd(dr=drop(1.0)), BAD_ARG),
        "ln_bwd_drop C > 1024": (bwd_drop(C=1032), BAD_SHAPE), "ln_bwd_drop C % 8": (bwd_drop(C=60), BAD_SHAPE),
        "ln_bwd_drop nblocks = 0": (bwd_drop(nb=0), BAD_SHAPE), "ln_bwd_drop without dx2": (bwd_drop(dx2=None), BAD_ARG),
        "ln_bwd_drop lddy % 8": (bwd_drop(lddy=8188), BAD_SHAPE), "ln_bwd_drop lddx2 % 8": (bwd_drop(lddx2=8188), BAD_SHAPE),
        "ln_bwd_drop ldadd % 8": (bwd_drop(add=X, ldadd=8188), BAD_SHAPE), "ln_bwd_drop p = 1": (bwd_drop(dr=drop(1.0)), BAD_ARG),
        "dropout C % 8": (dropout(C=60), BAD_ARG), "dropout p = 1": (dropout(p=1.0), BAD_ARG), "dropout p < 0": (dropout(p=-0.5), BAD_ARG),
        "dropout rows_per_batch = 0": (dropout(rows_per_batch=0), BAD_ARG),
        "dropout_fill n % 8": (L.ifseg_dropout_fill(P(X), P(Y), ll(60), f(0.1), u64(1), None, f(-30.0), S), BAD_ARG),
        "dropout_fill p = 1": (L.ifseg_dropout_fill(P(X), P(Y), ll(64), f(1.0), u64(1), None, f(-30.0), S), BAD_ARG),
        "rel_gather_multi L = 17": (L.ifseg_rel_gather_multi(tabs, i(17), P(IDS), P(ST), i(4), i(4), S), BAD_ARG),
        "colsum N % 8": (colsum(N=60), BAD_SHAPE), "embed_rows C % 8": (embed(C=60), BAD_SHAPE), "embed_bag_mean C % 8": (bag(C=60), BAD_SHAPE),
        "embed_bag_mean maxlen = 0": (bag(maxlen=0), BAD_SHAPE),
        "check_inputs mode 4": (check(8, 4), BAD_ARG), "check_inputs n < 0": (check(-1, 0), BAD_ARG),
        "check_inputs row_len = 0": (check(8, 1, 0), BAD_ARG), "check_inputs without x": (check(8, 0, x=None), BAD_ARG),
        "kproj C % 8": (L.ifseg_kproj_common_mode(P(Y), P(X), P(ST), i(4), i(60), S), BAD_ARG),
        "rows_segment_sum C % 8": (L.ifseg_rows_segment_sum(P(X), P(IDS), None, P(IDS), P(Y), ll(8), i(60), ll(4), ll(-1), S), BAD_ARG),
        # ---- refused since this suite
        "ln_bwd lddy % 8": (bwd(lddy=8188), BAD_SHAPE), "ln_bwd ldx % 8": (bwd(ldx=8188), BAD_SHAPE), "ln_bwd lddx % 8": (bwd(lddx=8188), BAD_SHAPE),
        "ln_bwd ldadd % 8": (bwd(add=X, ldadd=8188), BAD_SHAPE),
        "ln_bwd_drop with GELU": (bwd_drop(flags=GELU), BAD_ARG),
        "dropout ldx % 8": (dropout(ldx=8188), BAD_SHAPE), "dropout ldo % 8": (dropout(ldo=8188), BAD_SHAPE),
        "dropout ldr % 8": (dropout(resid=X, ldr=8188), BAD_SHAPE), "dropout x_bs % 8": (dropout(rpb=4, x_bs=8192 * 4 + 4), BAD_SHAPE),
        "colsum ldx % 8": (colsum(ldx=8188), BAD_SHAPE), "colsum nblk_rows = 0": (colsum(nblk=0), BAD_SHAPE),
        "embed_rows ldo % 8": (embed(ldo=8188), BAD_SHAPE), "embed_bag_mean ldo % 8": (bag(ldo=8188), BAD_SHAPE),
        "check_inputs ragged last row": (check(8, 1, 3), BAD_ARG),
        # ---- nothing to do
        "ln_fwd rows = 0": (L.ifseg_ln_fwd(P(X), P(G), P(G), None, P(Y), m, r, i(0), i(60), f(1e-5), i(0), i(0), ll(0), i(8192), ll(0), i(8192),
                                           ll(0), i(0), None, S), 0),
    }
    torch.cuda.synchronize()
    wrong = {k: v for k, v in calls.items() if v[0] != v[1]}
    assert not wrong, "return codes (got, expected): %s" % wrong
    for t, w in zip((Y, Y2, ST, PART), want):
        assert torch.equal(_bits(t), _bits(w)), "a refused call wrote to its output"
