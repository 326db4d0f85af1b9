"""The row-op conformance suite checked on its own, without a GPU (tests/_rowops_cases.py: see its docstring):
the case tables against the restated dispatch rules, the references' two properties for every part A case (an fp32
emulation stays inside the derived bound; a row with its neighbour's statistics leaves it), the GELU restatement against the
exact function at every bf16 input, the generator restatements against hand-checkable vectors, representability of the exact
cases' expected values."""
import math

import numpy as np
import pytest

import _rowops_cases as rc

F32 = np.float32


def _ids(cases):
    return [c["id"] for c in cases]


# ------------------------------------------------------------------------------------------- the tables
def test_case_ids_are_unique():
    for table in (rc.FWD_CASES, rc.BWD_CASES, rc.BWD_DROP_CASES):
        assert len(set(_ids(table))) == len(table)


def test_tables_reach_what_they_name():
    """every row against the restated rules of ln_fwd_impl / ifseg_ln_bwd / ifseg_ln_bwd_drop"""
    for c in rc.FWD_CASES:
        assert rc.fwd_reach(c["C"], c["gelu"]) == c["reach"], c["id"]
    for c in rc.BWD_CASES:
        assert rc.bwd_reach(c["C"], c["gelu"]) == c["reach"], c["id"]
    for c in rc.BWD_DROP_CASES:
        assert rc.bwd_drop_reach(c["C"]) == c["reach"] and not c["gelu"], c["id"]
    for c in rc.FWD_CASES + rc.BWD_CASES + rc.BWD_DROP_CASES:
        assert c["C"] % 8 == 0 and 8 <= c["C"] <= rc.LN_MAX_C and c["rows"] <= 25


def test_tables_cover_every_instantiation_width_and_row_count():
    reached = {c["reach"] for c in rc.FWD_CASES + rc.BWD_CASES + rc.BWD_DROP_CASES}
    assert reached == set(rc.LN_INSTANTIATIONS)
    for table in (rc.FWD_CASES, rc.BWD_CASES):
        assert {c["C"] for c in table} >= set(rc.LN_WIDTHS)
    assert {c["C"] for c in rc.BWD_DROP_CASES} == {C for C in rc.LN_WIDTHS if C <= 1024}
    assert {c["rows"] for c in rc.FWD_CASES} == {1, 3, 4, 5, 13}
    assert {(c["rows"], c["nblocks"]) for c in rc.BWD_CASES} == {(25, 3), (7, 3), (1, 3), (12, 3), (5, 768)}
    # both sides of each dispatch edge, the chunk counts around a wave and around four waves
    for lo, hi in ((1024, 1032), (3072, 3080)):
        assert rc.fwd_reach(lo, False) != rc.fwd_reach(hi, False)
    assert rc.bwd_reach(1024, True) != rc.bwd_reach(1032, True) and rc.bwd_reach(1024, False) != rc.bwd_reach(1032, False)
    assert {504 // 8, 512 // 8, 520 // 8, 2048 // 8, 2056 // 8} == {63, 64, 65, 256, 257}
    # every option is on and off for every instantiation
    for table, opts in ((rc.FWD_CASES, ("resid", "drop", "pf32", "strided")), (rc.BWD_CASES, ("add", "drop", "pf32", "strided"))):
        for k in {c["reach"] for c in table}:
            for o in opts:
                assert {c[o] for c in table if c["reach"] == k} == {False, True}, (k, o)


def test_multi_trip_rows():
    """with 3 blocks: 12 rows a trip for a wave per row, 3 for four waves per row"""
    for c in rc.BWD_CASES + rc.BWD_DROP_CASES:
        per_trip = c["nblocks"] * (4 if rc.bwd_waves_per_row(c["C"], c["gelu"]) == 1 else 1)
        if (c["rows"], c["nblocks"]) in ((25, 3), (7, 3)):
            assert c["rows"] > 2 * per_trip and c["rows"] % per_trip != 0, c["id"]


def test_designated_chunks():
    assert rc.designated_chunks(8, 64) == [0]
    assert rc.designated_chunks(520, 64) == [0, 63, 64]
    assert rc.designated_chunks(4096, 64) == [0, 63, 64, 128, 192, 256, 320, 384, 448, 511]
    assert rc.designated_chunks(4096, 256) == [0, 63, 256, 511]
    d = rc.ln_inputs(13, 4096, 1)
    assert d["x"][1, 1] == 64 and d["x"][10, 8 * 511 + 1] == 64 and d["dy"][3, 8 * 64 + 1] == 16
    assert (d["gamma16"] == 0).any() and (d["gamma16"] < 0).any() and d["gamma16"][1] != 0


def test_reduce_parts_rules():
    assert rc.reduce_reach(1, 31, 40) == "reduce_parts_kernel" and rc.reduce_reach(1, 32, 40) == "reduce_parts2d_kernel"
    assert rc.reduce_reach(1, 2047, 40) == "reduce_parts2d_kernel" and rc.reduce_reach(1, 2048, 40) == "reduce_parts_tall_kernel"
    assert rc.reduce_reach(1, 2048, 4096) == "reduce_parts_tall_kernel" and rc.reduce_reach(1, 2048, 4097) == "reduce_parts2d_kernel"
    for c in rc.REDUCE_CASES:
        assert rc.reduce_reach(c["outer"], c["parts"], c["n"]) == c["reach"], c


# -------------------------------------------------------------------- part A: the references on their own
def _neighbour(v):
    return np.roll(v, -1, axis=0)


@pytest.mark.parametrize("case", rc.FWD_CASES, ids=_ids(rc.FWD_CASES))
def test_forward_reference(case):
    d, ks = rc.case_inputs(case), rc.case_keepscale(case)
    resid = d["resid"] if case["resid"] else None
    ref = rc.ln_fwd_ref(d["x"], d["gamma"], d["beta"], case["gelu"], resid, ks)
    y, mu, rs = rc.ln_fwd_emul(d["x"], d["gamma"], d["beta"], case["gelu"], resid, ks)
    for name, got in (("y", y), ("mean", mu), ("rstd", rs)):
        r, at = rc.worst_ratio(got, ref[name], ref[name + "_b"])
        assert r <= 1.0, "%s %s: the fp32 emulation is at %.3f of the bound at %s" % (case["id"], name, r, at)
    if case["rows"] > 1:
        swapped = rc.ln_fwd_ref(d["x"], d["gamma"], d["beta"], case["gelu"], resid, ks, stats=(_neighbour(ref["mean"]), _neighbour(ref["rstd"])))
        # (left out of the count: columns whose gain is zero and elements the mask drops -- beta and resid alone)
        live = np.broadcast_to(d["gamma"][None, :] != 0, y.shape) & (True if ks is None else ks != 0)
        out = np.abs(swapped["y"] - ref["y"]) > 2 * ref["y_b"]
        assert out[live].mean() >= 0.8, "%s: only %.1f %% of the elements leave twice the bound" % (case["id"], 100 * out[live].mean())
        for name in ("mean", "rstd"):
            assert rc.fraction_outside(_neighbour(ref[name]), ref[name], ref[name + "_b"]) >= 0.8, (case["id"], name)


@pytest.mark.parametrize("case", rc.BWD_CASES + rc.BWD_DROP_CASES, ids=_ids(rc.BWD_CASES + rc.BWD_DROP_CASES))
def test_backward_reference(case):
    is_pair = case["reach"] == "ln_bwd_lean_kernel<2,true>"      # ifseg_ln_bwd_drop: the dropout is the second output's, not dy's
    d = rc.case_inputs(case, backward=True)
    ks = None if is_pair else rc.case_keepscale(case)
    add = d["add"] if case["add"] else None
    _, mu, rs = rc.ln_fwd_emul(d["x"], d["gamma"], d["beta"], case["gelu"])
    ref = rc.ln_bwd_ref(d["dy"], d["x"], d["gamma"], mu, rs, case["gelu"], add, ks)
    dx, dg, db = rc.ln_bwd_emul(d["dy"], d["x"], d["gamma"], mu, rs, case["gelu"], add, ks)
    for name, got in (("dx", dx), ("dgamma", dg), ("dbeta", db)):
        r, at = rc.worst_ratio(got, ref[name], ref[name + "_b"])
        assert r <= 1.0, "%s %s: the fp32 emulation is at %.3f of the bound at %s" % (case["id"], name, r, at)
    if case["rows"] > 1:
        swapped = rc.ln_bwd_ref(d["dy"], d["x"], d["gamma"], _neighbour(mu), _neighbour(rs), case["gelu"], add, ks)
        # (elements that cannot depend on the statistics are left out of the count: rows DropPath has zeroed, and with GELU
        # those the activation gates off -- act'(x) < 1/2, x < 0 -- whose dx is dx_add and little else)
        live = np.ones(dx.shape, dtype=bool) if ks is None else np.broadcast_to((ks != 0).any(1, keepdims=True), dx.shape)
        if case["gelu"]:
            live = live & (rc.gelu_grad_f32(d["x"]) >= 0.5)
        out = np.abs(swapped["dx"] - ref["dx"]) > 2 * ref["dx_b"]
        assert out[live].mean() >= 0.8, "%s: only %.1f %% of the elements leave twice the bound" % (case["id"], 100 * out[live].mean())
        assert rc.fraction_outside(swapped["dgamma"], ref["dgamma"], ref["dgamma_b"]) >= 0.8, case["id"]


def test_dropped_outputs_are_told_apart_on_the_reference():
    """part B reads the dropped positions of ln_fwd(..., drop=) off its output: the undropped output is never zero"""
    for C in rc.MASK_WIDTHS:
        d = rc.mask_ln_inputs(C)
        y = rc.ln_fwd_ref(d["x"], d["gamma"], d["beta"])
        assert (np.abs(y["y"]) > 1.0).all() and (y["y_b"] < 0.25).all() and all(v != 0 for v in rc.MASK_DPSCALE)


# --------------------------------------------------------------------------------------------------- GELU
def test_gelu_restatement_against_the_exact_function():
    """0.5 x (1 + erf(x / sqrt 2)) at every finite bf16 input in [-40, 40]: the polynomial's documented |erf err| <= 1.5e-7 and
    the fp32 evaluation (8 u on erf, 2 u relative on the product)"""
    x = rc.finite_bf16_in(-40.0, 40.0)
    assert x.size > 30000 and x[0] == -40 and x[-1] == 40
    exact_erf = np.array([math.erf(float(v) / math.sqrt(2.0)) for v in x])
    exact = 0.5 * x.astype(np.float64) * (1.0 + exact_erf)
    got = rc.gelu_f32(x).astype(np.float64)
    bound = 0.5 * np.abs(x) * (1.5e-7 + 8 * rc.U) + 2 * rc.U * np.abs(exact) + 1e-45
    assert (np.abs(got - exact) <= bound).all(), float((np.abs(got - exact) / bound).max())
    with np.errstate(under="ignore"):
        e = np.exp(-0.5 * x.astype(np.float64) ** 2)
    assert (np.abs(rc.erf_as(x, e.astype(F32)).astype(np.float64) - exact_erf) <= 1.5e-7 + 8 * rc.U).all()
    # the derivative: Phi(x) + x phi(x)
    dexact = 0.5 * (1.0 + exact_erf) + x * e / math.sqrt(2 * math.pi)
    assert (np.abs(rc.gelu_grad_f32(x).astype(np.float64) - dexact) <= 0.5 * (1.5e-7 + 8 * rc.U) + 4 * rc.U * (1 + np.abs(dexact))).all()
    # what dropout_fill relies on: gelu(-30) = -0 and gelu'(-30) = 0 exactly
    assert rc.gelu_f32(F32(-30.0)) == 0 and rc.gelu_grad_f32(F32(-30.0)) == 0


# ------------------------------------------------------------------------------------------- generators
def test_splitmix64_vectors():
    """the published test vectors of splitmix64 (seed 0: the first outputs are the function at 0, g, 2 g for the increment g,
    and the function adds g itself) and the python-integer form against the numpy form"""
    g = 0x9E3779B97F4A7C15
    assert rc.splitmix64_int(0) == 0xE220A8397B1DCDAF
    assert rc.splitmix64_int(g) == 0x6E789E6AA1B965F4
    assert rc.splitmix64_int(2 * g) == 0x06C45D188009454F
    z = [0, 1, g, rc.M64, 1 << 63, 0x0123456789ABCDEF, rc.DROP_SEED]
    got = rc.splitmix64(np.array(z, dtype=np.uint64))
    assert [int(v) for v in got] == [rc.splitmix64_int(v) for v in z]
    assert rc.DROP_SEED >> 63 == 1


def test_drop8_restatement_by_hand():
    """element e of chunk c8 reads bits 16 (e mod 4) .. of draw 2 c8 + (e div 4)"""
    seed, add, C, rows, p = rc.DROP_SEED, 12345, 24, 3, 0.1
    keep = rc.drop_keep(rows, C, p, seed, add)
    thr = rc.drop_threshold(p)
    assert thr == 6553 and rc.drop_threshold(0.0) == 0 and rc.drop_threshold(0.999) == 65470
    for row in range(rows):
        for col in range(C):
            c8, e = row * (C // 8) + col // 8, col % 8
            draw = rc.splitmix64_int((seed + add + 2 * c8 + e // 4) & rc.M64)
            assert bool(keep[row, col]) == (((draw >> (16 * (e % 4))) & 0xFFFF) >= thr)
    assert rc.drop_keep(5, 520, 0.0, seed).all()
    k = rc.drop_keep(64, 4096, 0.1, seed)
    assert abs(k.mean() - 0.9) < 3e-3
    # the eight elements of a chunk are independent draws: no column pattern
    assert all(abs(k.reshape(-1, 8)[:, e].mean() - 0.9) < 6e-3 for e in range(8))
    sc = rc.drop_scale(5, 0.1, (2.0, 0.0, 0.5), 2)
    assert sc.dtype == F32 and list(sc) == [F32(2.0) * (F32(1) / (F32(1) - F32(0.1)))] * 2 + [0.0, 0.0] + [F32(0.5) * (F32(1) / (F32(1) - F32(0.1)))]


def test_droppath_restatement():
    u = rc.droppath_uniform(3, 4, 99)
    assert u.shape == (3, 4) and ((u >= 0) & (u < 1)).all()
    z = rc.splitmix64_int((99 + 0x5851F42D4C957F2D * 6) & rc.M64)
    assert u[1, 1] == F32((z >> 40) / 16777216.0)
    out = rc.droppath_scale([0.0, 0.25, 1.0], 64, 99)
    assert (out[0] == 0).all() and (out[2] == 1).all() and set(np.unique(out[1])) == {0.0, 4.0}


# ------------------------------------------------------------------------------- part C: representability
@pytest.mark.parametrize("C", [8, 2056])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("ends", [False, True])
def test_segment_sum_case(C, weighted, ends):
    c = rc.segment_sum_case(C, weighted, ends)
    assert (np.diff(c["ids"]) >= 0).all()
    runs = {int(i): int((c["ids"] == i).sum()) for i in np.unique(c["ids"])}
    assert {1, 2, 33, 300} <= set(runs.values())
    assert c["skip"] in runs and (ends or (min(runs) < 0 and max(runs) >= c["V"]))
    if ends:
        assert 0 <= c["ids"][0] != c["skip"] and c["ids"][-1] < c["V"] and c["ids"][-1] != c["skip"]
    assert c["worst_partial"] <= 256 and np.abs(c["ref"]).max() <= 256
    assert rc.is_bf16(c["ref"]) and rc.is_bf16(c["src"]) and rc.is_bf16(c["prior"])
    assert c["touched"].any() and not c["touched"].all() and (c["prior"] != 0).any()


def test_exact_cases_are_representable():
    for c in rc.EXACT_CASES():
        assert c["ok"], c["what"]
