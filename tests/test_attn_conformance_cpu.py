"""The attention conformance suite without a GPU: the case tables against the restated dispatch rules, the validity of the
constructed inputs (select gap, poison, representability), the single-pair sensitivity of the uniform regime, and an emulation
of the kernels' number formats inside every part B bound.  Everything here runs on the references of _attn_cases.py alone."""
import numpy as np
import pytest

import _attn_cases as ac


def _ids(cases):
    return [c["id"] for c in cases]


def test_case_tables_reach_what_they_name():
    allc = ac.FWD_CASES + ac.BI_CASES + ac.RANDOM_CASES
    assert len({c["id"] for c in allc}) == len({id(c) for c in allc}), "duplicate case ids"
    for c in allc:
        assert ac.reach(c) == c["reach"], (c["id"], ac.reach(c), c["reach"])
        if c["gh"] or c["causal"]:
            assert c["P"] % 64 == 0 and c["P"] <= min(c["T"], c["S"]), c["id"]
        if c["causal"] and c["gh"]:
            assert c["Lt"] == 1, c["id"]
    reached = {c["reach"] for c in ac.FWD_CASES}
    for path in ("row32", "rowseg", "generic", "plain"):
        for pos in ("pos", "nopos"):
            assert any(r.startswith(path + "/" + pos) for r in reached), (path, pos)
    assert {"dfast/nopos", "dslow/nopos", "dfast/pos"} <= reached
    big = [c for c in ac.GRID_CASES if c["reach"].endswith("dkv8")]
    assert [(c["gh"], c["gw"], c["B"], c["H"], c["pos"]) for c in big] == [(40, 40, 1, 2, True), (40, 40, 1, 2, False)]
    assert ac.dense_ld(ac.by_id("dense-ld4-165")) % 4 == 0 and ac.dense_ld(ac.by_id("dense-ldodd-165")) % 4 != 0
    grids = {(c["gh"], c["gw"], c["grid_w"]) for c in ac.GRID_CASES}
    assert {(2, 32, 32), (8, 40, 40), (4, 48, 48), (8, 8, 8), (16, 12, 12), (16, 36, 36), (8, 16, 0), (40, 40, 40)} <= grids
    assert {c["Lt"] for c in ac.GRID_CASES} == {1, 37}
    # xcd_remap / the causal longest-first order: nq H B divisible by 8 and not
    for causal in (False, True):
        n = {(((c["T"] + 127) // 128) * c["H"] * c["B"]) % 8 == 0 for c in ac.FWD_CASES if c["causal"] == causal}
        assert n == {True, False}, causal
    edges = {(c["T"], c["S"]) for c in ac.PLAIN_CASES}
    assert {(1, 129), (129, 1), (65, 128)} <= edges and {1, 31, 64, 65, 127, 128, 129, 193} <= {x for e in edges for x in e}
    assert {c["B"] for c in ac.BI_CASES} == {1, 3, 4, 5, 9}
    assert {c["P"] for c in ac.BI_CASES if c["causal"]} == {64, 128}
    for c in ac.BI_CASES:
        for kv in c["kv_len"] or ():
            assert 1 <= kv <= c["S"]
    kinds = set()
    for c in ac.BI_CASES:
        for kv in c["kv_len"] or ():
            kinds |= {"S"} if kv == c["S"] else set()
            kinds |= {"S-1"} if kv == c["S"] - 1 else set()
            kinds |= {"32k"} if kv % 32 == 0 else set()
            kinds |= {"32k+1"} if kv % 32 == 1 and kv > 1 else set()
            kinds |= {"1"} if kv == 1 else set()
    assert kinds == {"S", "S-1", "32k", "32k+1", "1"}
    assert any(c["layout"] == "dense" for c in ac.FWD_CASES) and any(c["layout"] == "dense" for c in ac.BI_CASES)


def _representable(x):
    return bool((ac.bf16_round(x).astype(np.float64) == x).all())


@pytest.mark.parametrize("case", ac.FWD_CASES + ac.BI_CASES, ids=_ids(ac.FWD_CASES + ac.BI_CASES))
def test_select_inputs(case):
    """every row has one allowed key that beats every other allowed key by >= 200 log2 units, it is sel; every operand and every
    expected value is a bf16 value; every poisoned key beats every winner and is finite"""
    d = ac.select_inputs(case)
    T, S = case["T"], case["S"]
    assert d["allowed"].any(-1).all(), "a fully masked row"
    gap, arg = ac.select_gap_log2(case, d)
    if S > 1:
        assert gap.min() >= ac.GAP_MIN_LOG2, gap.min()
    assert (arg == d["sel"]).all()
    for name in ("q", "k", "v", "dout", "pq", "pk"):
        if d[name] is not None:
            assert _representable(d[name]) and np.isfinite(d[name]).all(), name
    keep = None
    if case["drop"]:
        keep = (np.random.default_rng(3).random((case["B"], case["H"], T, S)) < 0.5).astype(np.uint8)
    e = ac.select_expect(case, d, keep)
    assert _representable(e["out"]) and _representable(e["dv"])
    assert np.abs(e["lse"]).max() < 2.0 ** 12          # an ulp of the lse stays below 2^-11
    # poison: the raw score of every hidden key of the operand exceeds the best allowed score of the row
    s_all = np.einsum("bthd,bshd->bhts", d["q"], d["k"])
    if d["pq"] is not None:
        s_all = s_all + np.einsum("thd,shd->hts", d["pq"], d["pk"])[None]
    b = ac.bias_of(case, d)
    if b is not None:
        s_all = s_all + np.where(np.isfinite(b), b, 0)[None]
    hidden = ~d["allowed"] if b is None else ~d["allowed"] & np.isfinite(b)[None]
    if case["entry"] == "bi" and case["causal"]:
        hidden &= ~ac.causal_mask(T, S, case["P"])[None, None]      # the mask is the -inf of D there, not a score
    if hidden.any():
        best = np.where(d["allowed"], s_all, -np.inf).max(-1, keepdims=True)
        assert (np.where(hidden, s_all - best, np.inf) >= 1024).all(), "a hidden key does not beat the winner"
    # the guard rows of the K allocation (the GPU file paints them; pos_k guard rows hold zeros): POISON on every query row
    guard = np.zeros(64)
    guard[ac.POISON_COL:] = ac.POISON_K
    best_all = np.where(d["allowed"], s_all, -np.inf).max(-1)
    assert ((np.einsum("bthd,d->bht", d["q"], guard) - best_all) >= 1024).all(), "a guard row of K does not beat the winner"
    # the winners the issue asks for: key 0, the last allowed key, another tile for consecutive rows
    sel = d["sel"]
    if T >= 7 and S >= 130 and not case["causal"]:
        assert (sel == 0).any() and (sel == S - 1).any()
        assert (np.abs(np.diff(sel // 64, axis=-1)) > 0).mean() > 0.5


@pytest.mark.parametrize("case", [c for c in ac.FWD_CASES + ac.BI_CASES if c["T"] * c["S"] <= 300 * 300],
                         ids=_ids([c for c in ac.FWD_CASES + ac.BI_CASES if c["T"] * c["S"] <= 300 * 300]))
def test_select_emulation_is_exact(case):
    """the claims of the regime on an emulation of the number formats: out and dv bit for bit, dq and dk zero, lse within 4 ulps"""
    d = ac.select_inputs(case)
    ks = None
    keep = None
    if case["drop"]:
        keep = (np.random.default_rng(3).random(d["allowed"].shape) < 0.5).astype(np.uint8)
        ks = 2.0 * keep
    e = ac.select_expect(case, d, keep)
    out, lse = ac.emulate_forward(case, d, ks)
    assert (out == e["out"]).all()
    assert (np.abs(lse - e["lse"]) <= 4 * np.spacing(np.abs(e["lse"]).astype(np.float32))).all()
    r = ac.emulate_backward(case, d, out, lse, ks)
    assert (r["dv"] == e["dv"]).all() and not r["dq"].any() and not r["dk"].any()


@pytest.mark.parametrize("case", ac.UNIFORM_CASES, ids=_ids(ac.UNIFORM_CASES))
def test_uniform_single_pair_sensitivity(case):
    """removing any single allowed (t, j) pair, or adding any single forbidden one, moves some element of out[t] by at least
    twice the bound (rows with one allowed key cannot lose it: fully masked rows are out of scope)"""
    assert case["T"] <= 256 and case["S"] <= 256
    d = ac.uniform_inputs(case)
    al = d["allowed"]
    assert al.any(-1).all()
    n = al.sum(-1).astype(np.float64)[..., None, None]                       # [B, H, T, 1, 1]
    g = d["gain"][None, :, None, None]
    v = np.transpose(d["v"], (0, 2, 1, 3))                                   # [B, H, S, 64]
    m = np.einsum("bhts,bhsd->bhtd", al / n[..., 0], v)[:, :, :, None, :]    # mean [B, H, T, 1, 64]
    vj = v[:, :, None, :, :]
    thr = 2 * ac.uniform_bound(g[..., None] * m)
    with np.errstate(divide="ignore", invalid="ignore"):
        rem = np.abs(g[..., None] * (m - vj) / (n - 1))                      # the mean without key j moves by (m - v_j) / (n - 1)
    add = np.abs(g[..., None] * (vj - m) / (n + 1))
    ok_rem = (rem >= thr).any(-1) | ~al | (n[..., 0] == 1)
    ok_add = (add >= thr).any(-1) | al
    assert ok_rem.all(), "removing pair %s is not visible" % (tuple(np.argwhere(~ok_rem)[0]),)
    assert ok_add.all(), "adding pair %s is not visible" % (tuple(np.argwhere(~ok_add)[0]),)
    e = ac.uniform_expect(case, d)
    pow2 = (n[..., 0, 0] == 2.0 ** np.round(np.log2(n[..., 0, 0])))
    if pow2.all():
        assert (ac.bf16_round(e["out"]) == e["out"]).all()


@pytest.mark.parametrize("case", ac.RANDOM_CASES, ids=_ids(ac.RANDOM_CASES))
def test_emulation_stays_within_the_part_b_bounds(case):
    """fp32 scores, bf16-rounded P and dS, fp32 sums and one output rounding stay inside EVERY bound of part B: out, lse, dv, dq,
    dk, dgain_rows, the dbias slabs, the abs-pos partials and the three table partials (binned with the class-sum structure of
    the kernel on row32 / rowseg grids).  The ratios are in profiles/attn_conformance.txt"""
    c = case
    d = ac.random_inputs(c)
    ks = None
    if c["drop"]:
        ks = 2.0 * (np.random.default_rng(4).random(d["allowed"].shape) < 0.5)
    ref = ac.forward_ref(c, d, ks)
    out, lse = ac.emulate_forward(c, d, ks)
    worst = {"out": ac.worst_ratio(out, ref["out"], ref["out_b"])[0], "lse": ac.worst_ratio(lse, ref["lse"], ac.lse_bound(c, d, ref["lse"]))[0]}
    if not c["dense"]:
        b = ac.backward_ref(c, d, out, lse, ks, 0.5)
        r = ac.emulate_backward(c, d, out, lse, ks, 0.5, 0.25)
        for name in ("dv", "dq", "dk", "dgain_rows"):
            worst[name] = ac.worst_ratio(r[name], b[name], b[name + "_b"])[0]
        if c["entry"] == "bi":
            for g in range((c["B"] + 3) // 4):
                refg, bg = b["dS"][4 * g:4 * g + 4].sum(0), b["w"][4 * g:4 * g + 4].sum(0)
                worst["dbias"] = max(worst.get("dbias", 0), ac.worst_ratio(r["dbias"][g], refg, ac.U * np.abs(refg) + bg + 1e-30)[0])
        elif c["pos"]:
            worst["dpq"] = ac.worst_ratio(r["dpq"], 0.25 * b["dpq"], ac.U * 0.25 * np.abs(b["dpq"]) + 0.25 * b["dpq_b"] + 1e-30)[0]
            worst["dpk"] = ac.worst_ratio(r["dpk"], b["dpk"], ac.U * np.abs(b["dpk"]) + b["dpk_b"] + 1e-30)[0]
        if c["entry"] != "bi" and c["gh"]:
            refs, errs = ac.table_refs_and_bounds(c, d["tabs"], b)
            for name, got, rf, eb in zip(("drel2d", "drel1d", "drelx"), ac.emulate_table_bins(c, d["tabs"], r["dSk32"]), refs, errs):
                worst[name] = ac.worst_ratio(got, rf, eb)[0]
    print("[part B emulation] %-28s %s" % (c["id"], "  ".join("%s %.3f" % kv for kv in worst.items())))
    assert max(worst.values()) <= 1.0, worst
