"""Conformance of the attention kernels (csrc/attention.hip, attention_bi.hip, attention_ops.hip) through the C ABI
(ifseg_amd.hip), in the style of test_gemm_conformance_gpu.py and test_rowops_conformance_gpu.py.  Data, fp64 references, the
derived bounds and the case tables are in _attn_cases.py (its docstring holds the regimes and the derivations);
test_attn_conformance_cpu.py checks them without a GPU.

Layouts: q, k, v are column slices of ONE fused [B, rows, 3C + 8] allocation (row stride 3C + 8, a few rows before and after
every batch element), dq, dk, dv slices of one fused dqkv allocation; cross-attention shapes take q alone and k, v as slices of
a [B, rows, 2C + 8] buffer; "dense" cases run on contiguous tensors.  Guard rows of K hold a key that beats every winner, guard
rows of V a large finite value, so a row read outside an operand flips outputs.  Every written allocation (out, lse, delta, dq,
dk, dv, dgain_rows, the abs-pos partials, the table partials, the dbias slabs, D) holds a sentinel outside its logical extent
and is compared bit for bit afterwards.

Part A: select / poison (exact) and uniform (2^-8 |ref|) on constructed inputs, every dispatch path, `phases` split = single call.
Part B: random values per element against the fp64 reference within the derived bounds.
Part C: ifseg_attn_delta / ifseg_attn_bwd_reduce / ifseg_attn_dbias_grads / ifseg_attn_dense_bias exact on integers.
Part D: argument rejection (return codes only; nothing is launched with a bad argument).
kv_len = 0 and fully masked rows are out of scope (every row of every case keeps at least one key).
profiles/attn_conformance.txt: the kernels seen in a trace of this file, the part B ratios, the wrong variants it catches.
"""
import ctypes

import numpy as np
import pytest
import torch

import _attn_cases as ac
from test_gemm_conformance_gpu import (BAD_ARG, BAD_SHAPE, BF16, F32, GUARD, SENTINEL, _assert_surroundings, _bits, _dev,
                                       _flat_guarded, _guarded)

pytestmark = pytest.mark.gpu
I32 = torch.int32


# ------------------------------------------------------------------------------------------------ plumbing
def _t(a, dtype=BF16):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype)


def _ids(cases):
    return [c["id"] for c in cases]


def _paint(full, R, lo, C, H, kind):
    """guard rows of a [B, 3 + R + 2, W] allocation, columns [lo, lo + C): the poisoned key / the poisoned value"""
    rows = [0, 1, 2, 3 + R, 4 + R]
    if kind == "k":
        row = torch.zeros(C, dtype=BF16)
        row.view(H, 64)[:, ac.POISON_COL:] = ac.POISON_K
        full[:, rows, lo:lo + C] = row.to(full.device)
    else:
        full[:, rows, lo:lo + C] = ac.V_POISON


def _operands(c, d, dev):
    """q, k, v as views [B, T|S, C] in the layout of the case"""
    B, H, T, S = c["B"], c["H"], c["T"], c["S"]
    C = H * 64
    q, k, v = (_t(d[n].reshape(d[n].shape[0], d[n].shape[1], C)) for n in ("q", "k", "v"))
    if c["layout"] == "fused":
        assert T == S
        full, _ = _guarded((B, T, 3 * C), BF16, dev, 8, GUARD)
        _paint(full, T, C, C, H, "k")
        _paint(full, T, 2 * C, C, H, "v")
        views = [full[:, 3:3 + T, i * C:(i + 1) * C] for i in range(3)]
    elif c["layout"] == "cross":
        fq, vq = _guarded((B, T, C), BF16, dev, 8, GUARD)
        fkv, _ = _guarded((B, S, 2 * C), BF16, dev, 8, GUARD)
        _paint(fkv, S, 0, C, H, "k")
        _paint(fkv, S, C, C, H, "v")
        views = [vq, fkv[:, 3:3 + S, :C], fkv[:, 3:3 + S, C:2 * C]]
    else:
        views = [_flat_guarded((B, T, C), BF16, dev, GUARD)[1], _flat_guarded((B, S, C), BF16, dev, GUARD)[1],
                 _flat_guarded((B, S, C), BF16, dev, ac.V_POISON)[1]]
    for view, val in zip(views, (q, k, v)):
        view.copy_(val.to(dev))
    return views


class _Outs:
    """output tensors inside sentinel-filled allocations; check() compares everything outside them bit for bit"""

    def __init__(self, dev):
        self.dev, self.items = dev, []

    def flat(self, shape, dtype=F32, init=None):
        full, view = _flat_guarded(tuple(shape), dtype, self.dev, SENTINEL)
        if init is not None:
            view.fill_(init)
        n = int(np.prod(shape))
        self.items.append((full, None, lambda f: f[16:16 + n]))
        return view

    def rows(self, B, R, C, dtype=BF16):
        full, view = _guarded((B, R, C), dtype, self.dev, 24, SENTINEL)       # (row strides that differ from the inputs')
        self.items.append((full, None, lambda f: f[:, 3:3 + R, :C]))
        return view

    def grads(self, c):
        """dq, dk, dv in the layout of the case"""
        B, T, S, C = c["B"], c["T"], c["S"], c["H"] * 64
        if c["layout"] == "fused":
            full = _guarded((B, T, 3 * C), BF16, self.dev, 16, SENTINEL)[0]      # lddq = 3C + 16 != ldq = 3C + 8
            self.items.append((full, None, lambda f: f[:, 3:3 + T, :3 * C]))
            return [full[:, 3:3 + T, i * C:(i + 1) * C] for i in range(3)]
        if c["layout"] == "cross":
            dq = self.rows(B, T, C)
            full = _guarded((B, S, 2 * C), BF16, self.dev, 16, SENTINEL)[0]
            self.items.append((full, None, lambda f: f[:, 3:3 + S, :2 * C]))
            return [dq, full[:, 3:3 + S, :C], full[:, 3:3 + S, C:2 * C]]
        return [self.flat((B, T, C), BF16), self.flat((B, S, C), BF16), self.flat((B, S, C), BF16)]

    def freeze(self):
        self.items = [(f, f.clone() if b is None else b, i) for f, b, i in self.items]

    def check(self, what):
        for full, before, inner in self.items:
            _assert_surroundings(full, before, inner, what)


def _np(t):
    return t.double().cpu().numpy()


def _heads(t, H):
    """[B, R, C] device tensor -> fp64 [B, R, H, 64]"""
    return _np(t).reshape(t.shape[0], t.shape[1], H, 64)


def _rel(hip, c, d, dev):
    tb = d["tabs"]
    if tb is None:
        return None
    f = lambda a: _flat_guarded(_t(a, F32), F32, dev, ac.POISON_REL)[1]
    return hip.RelBias(c["P"], torch.from_numpy(tb["gcode"]).to(dev), tb["code_bias"], f(tb["rel2d"]), f(tb["rel1d"]), f(tb["relx"]),
                       grid_w=c["grid_w"])


def _pos(c, d, dev):
    if d["pq"] is None:
        return None, None
    C = c["H"] * 64
    return (_guarded(_t(d["pq"].reshape(1, c["T"], C)), BF16, dev, 8, GUARD)[1][0],
            _guarded(_t(d["pk"].reshape(1, c["S"], C)), BF16, dev, 8, 0.0)[1][0])     # zeros: the K guard row's POISON stands alone


def _dense_f32(c, d, dev):
    """the fp32 dense bias [H, T, S] with row stride dense_ld inside an allocation that holds POISON_REL elsewhere"""
    if d["dense"] is None:
        return None
    ld = ac.dense_ld(c)
    flat = torch.full((c["H"] * c["T"] * ld + 32,), ac.POISON_REL, dtype=F32, device=dev)
    view = flat[16:16 + c["H"] * c["T"] * ld].view(c["H"], c["T"], ld)[:, :, :c["S"]]
    view.copy_(_t(d["dense"], F32).to(dev))
    return view


def _exact(what, got, want):
    bad = got != want
    assert not bad.any(), "%s: %d of %d elements differ; first at %s: got %r, expected %r" % (
        what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]), got[bad][0], want[bad][0])


def _within(what, got, ref, bound, log=None):
    r, at = ac.worst_ratio(got, ref, bound)
    print("[attn] %s: worst |err|/bound %.3f at %s" % (what, r, at))
    if log is not None:
        log[what.split(" ")[-1]] = round(r, 3)
    assert r <= 1.0, "%s: |err| is %.3f of the bound at %s (got %r, ref %r)" % (what, r, at, got[at], ref[at])


def _lse_ok(what, lse, want):
    tol = 4 * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    bad = np.abs(lse - want) > tol
    assert not bad.any(), "%s: lse differs at %s: got %r, expected %r" % (what, tuple(np.argwhere(bad)[0]), lse[bad][0], want[bad][0])


def _gain(d, dev):
    return _flat_guarded(_t(d["gain"], F32), F32, dev, ac.POISON_REL)[1]


# ---------------------------------------------------------------------- the per-batch-element kernels (attention.hip)
def _run_fwd(hip, c, d, dev, ops=None):
    B, H, T, S = c["B"], c["H"], c["T"], c["S"]
    C = H * 64
    q, k, v = ops if ops is not None else _operands(c, d, dev)
    pq, pk = _pos(c, d, dev)
    o = _Outs(dev)
    out = o.rows(B, T, C) if c["layout"] != "dense" else o.flat((B, T, C), BF16)
    lse = o.flat((B, H, T))
    o.freeze()
    hip.attn_fwd(q, k, v, pq, pk, out, lse, B, H, T, S, rel=_rel(hip, c, d, dev), causal=c["causal"], P=c["P"],
                 dense_bias=_dense_f32(c, d, dev), gain=_gain(d, dev))
    torch.cuda.synchronize()
    o.check(c["id"] + " forward")
    return (q, k, v, pq, pk), out, lse


def _run_bwd(hip, c, d, dev, ops, out, lse, dq_scale=1.0, dpq_scale=1.0, phases=(0,), want_outs=False):
    B, H, T, S = c["B"], c["H"], c["T"], c["S"]
    C = H * 64
    q, k, v, pq, pk = ops
    o = _Outs(dev)
    dout = _guarded(_t(d["dout"].reshape(B, T, C)), BF16, dev, 8, GUARD)[1]
    dq, dk, dv = o.grads(c)
    delta, dgr = o.flat((B, H, T)), o.flat((B, H, T))
    dpq, dpk = (o.flat((B, T, C), BF16), o.flat((B, S, C), BF16)) if pq is not None else (None, None)
    nparts = B * ((S + 127) // 128)
    parts = [None] * 3
    rel = _rel(hip, c, d, dev)
    if rel is not None:
        parts = [o.flat((H, nparts, n)) for n in (d["tabs"]["n2d"], 2 * c["Lt"] - 1, 2)]
    o.freeze()
    for ph in phases:
        hip.attn_bwd(q, k, v, pq, pk, out, dout, lse, delta, dq, dk, dv, dpq, dpk, B, H, T, S, rel=rel, causal=c["causal"], P=c["P"],
                     gain=_gain(d, dev), dq_scale=dq_scale, dpq_scale=dpq_scale, drel2d_part=parts[0], drel1d_part=parts[1],
                     drelx_part=parts[2], nparts=nparts, phases=ph, dgain_rows=dgr)
    torch.cuda.synchronize()
    o.check(c["id"] + " backward")
    return dict(dq=dq, dk=dk, dv=dv, delta=delta, dgain_rows=dgr, dpq=dpq, dpk=dpk, parts=parts)


@pytest.mark.parametrize("case", ac.FWD_CASES, ids=_ids(ac.FWD_CASES))
def test_select_fwd_bwd(case):
    """select / poison through ifseg_attn_fwd and ifseg_attn_bwd: out and dv bit for bit, dq, dk, the abs-pos partials and the
    table partials exactly zero, lse within 4 ulps, dgain_rows within 2^-12"""
    from ifseg_amd import hip
    dev = _dev()
    c, H = case, case["H"]
    d = ac.select_inputs(c)
    e = ac.select_expect(c, d)
    ops, out, lse = _run_fwd(hip, c, d, dev)
    what = "%s %s " % (c["id"], c["reach"])
    _exact(what + "out", _heads(out, H), e["out"])
    _lse_ok(what, _np(lse), e["lse"])
    if c["dense"]:
        return
    r = _run_bwd(hip, c, d, dev, ops, out, lse, dq_scale=0.5, dpq_scale=0.25)
    _exact(what + "delta", _np(r["delta"]), (np.transpose(d["dout"], (0, 2, 1, 3)) * np.transpose(e["out"], (0, 2, 1, 3))).sum(-1))
    _exact(what + "dv", _heads(r["dv"], H), e["dv"])
    for name in ("dq", "dk") + (("dpq", "dpk") if c["pos"] else ()):
        _exact(what + name, _np(r[name]), np.zeros(r[name].shape))
    for p in r["parts"]:
        if p is not None:
            _exact(what + "table partials", _np(p), np.zeros(p.shape))
    dgr = _np(r["dgain_rows"])
    assert (np.abs(dgr - e["dgain_rows"]) <= 2.0 ** -12 * np.abs(e["dgain_rows"])).all(), what + "dgain_rows"


@pytest.mark.parametrize("case", [c for c in ac.UNIFORM_CASES if c["entry"] == "fwd"], ids=_ids([c for c in ac.UNIFORM_CASES if c["entry"] == "fwd"]))
def test_uniform_fwd_bwd(case):
    """q = 0, zero bias: out is the mean over the allowed set, dv = sum_t dout / n_t, within 2^-8 |ref| (1 + 2^-12)"""
    from ifseg_amd import hip
    dev = _dev()
    c, H = case, case["H"]
    u = ac.uniform_inputs(c)
    B, T, S = c["B"], c["T"], c["S"]
    d = dict(q=np.zeros((B, T, H, 64)), k=np.zeros((B, S, H, 64)), v=u["v"], dout=u["dout"], pq=None, pk=None, tabs=None,
             dense=u["dense"], gain=u["gain"])
    if c["pos"]:
        d["pq"], d["pk"] = np.zeros((T, H, 64)), np.zeros((S, H, 64))
    if c["gh"]:
        gcode, code_bias, n2d = ac.grid_codes(c["gh"], c["gw"])
        d["tabs"] = dict(gcode=gcode, code_bias=code_bias, n2d=n2d, rel2d=np.zeros((H, n2d)), rel1d=np.zeros((H, 2 * c["Lt"] - 1)),
                         relx=np.zeros((H, 2)))
    e = ac.uniform_expect(c, u)
    ops, out, lse = _run_fwd(hip, c, d, dev)
    what = "%s uniform " % c["id"]
    _within(what + "out", _heads(out, H), e["out"], e["out_b"] + 1e-30)
    if not c["dense"]:
        r = _run_bwd(hip, c, d, dev, ops, out, lse)
        _within(what + "dv", _heads(r["dv"], H), e["dv"], e["dv_b"] + 1e-30)


@pytest.mark.parametrize("case", [c for c in ac.GRID_CASES + ac.PLAIN_CASES if c["id"] in (
    "row32-2x32+37-pos", "rowseg-8x40+1-causal-pos", "generic-16x36+37", "plain-127x193")], ids=lambda c: c["id"])
def test_phases_give_the_bits_of_the_single_call(case):
    """DELTA, DKV, DQ alone and combined against phases = 0, on the random data of part B"""
    from ifseg_amd import hip
    dev = _dev()
    c = case
    d = ac.random_inputs(c) if c in ac.RANDOM_CASES else ac.select_inputs(c)
    ops, out, lse = _run_fwd(hip, c, d, dev)
    one = _run_bwd(hip, c, d, dev, ops, out, lse, 0.5, 0.25)
    for split in ((1, 2, 4), (1 | 2, 4), (1 | 4, 2), (1, 2 | 4)):
        r = _run_bwd(hip, c, d, dev, ops, out, lse, 0.5, 0.25, phases=split)
        for name in ("dq", "dk", "dv", "delta", "dgain_rows", "dpq", "dpk"):
            if one[name] is not None:
                assert torch.equal(_bits(one[name].contiguous()), _bits(r[name].contiguous())), (split, name)
        if c["grid_w"] >= 32 and c["grid_w"] % 8 == 0:      # other grid widths bin the table gradients with LDS float atomics
            for a, b in zip(one["parts"], r["parts"]):
                assert a is None or torch.equal(_bits(a), _bits(b)), split


# ------------------------------------------------------------------------ the batch-inner kernels (attention_bi.hip)
def _unread_tiles(T, S, P, dev):
    """causal: the elements of D no block schedule reads (ifseg_attn_dense_bias documents them as unwritten)"""
    i, j = torch.arange(T, device=dev)[:, None], torch.arange(S, device=dev)[None, :]
    return (j < P) & ((i // 32 * 32 >= P) | (j // 32 > i // 32 + 1))


def _bi_dense(hip, c, bias, dev, o):
    """D of a batch-inner case through ifseg_attn_bias_pack from the integer fp32 bias (every element is written: value or
    -inf, checked); under causal the tiles no schedule reads are then overwritten with a finite value above every winner"""
    H, T, S = c["H"], c["T"], c["S"]
    dense = hip.DenseBias(H, T, S, dev)
    dense.D = o.flat((H, dense.Tp, dense.Sp), BF16)
    o.freeze()
    b32 = _flat_guarded(_t(bias, F32), F32, dev, ac.POISON_REL)[1]
    hip.attn_bias_pack(dense, b32, causal=c["causal"], P=c["P"])
    torch.cuda.synchronize()
    want = np.full((H, dense.Tp, dense.Sp), -np.inf)
    want[:, :T, :S] = np.where(ac.causal_mask(T, S, c["P"])[None], -np.inf, bias) if c["causal"] else bias
    _exact(c["id"] + " D", _np(dense.D), want)
    o.check(c["id"] + " D")
    if c["causal"]:
        dense.D[:, :T, :S][:, _unread_tiles(T, S, c["P"], dev)] = ac.POISON_REL
    return dense


def _run_bi(hip, c, d, dev, dq_scale=1.0, phases=(0,)):
    B, H, T, S = c["B"], c["H"], c["T"], c["S"]
    C = H * 64
    q, k, v = _operands(c, d, dev)
    o = _Outs(dev)
    dense = _bi_dense(hip, c, d["bi_bias"], dev, o)
    kv = torch.tensor(list(c["kv_len"]), dtype=I32, device=dev) if c["kv_len"] else None
    drop = (0.5, ac.DROP_SEED) if c["drop"] else None
    o = _Outs(dev)
    out = o.rows(B, T, C) if c["layout"] != "dense" else o.flat((B, T, C), BF16)
    lse, delta, dgr = o.flat((B, H, T)), o.flat((B, H, T)), o.flat((B, H, T))
    dq, dk, dv = o.grads(c)
    ng = (B + 3) // 4
    dbias = o.flat((ng, H, T, dense.Sp), BF16, init=0.0 if c["causal"] else None)
    dout = _guarded(_t(d["dout"].reshape(B, T, C)), BF16, dev, 8, GUARD)[1]
    o.freeze()
    gain = _gain(d, dev)
    hip.attn_fwd_bi(q, k, v, dense, out, lse, B, H, T, S, causal=c["causal"], P=c["P"], gain=gain, kv_len=kv, drop=drop)
    hip.attn_delta(out, dout, delta, B, H, T)
    for ph in phases:
        hip.attn_bwd_bi(q, k, v, dout, lse, delta, dense, dq, dk, dv, dbias, B, H, T, S, causal=c["causal"], P=c["P"], gain=gain,
                        dq_scale=dq_scale, phases=ph, dgain_rows=dgr, kv_len=kv, drop=drop)
    torch.cuda.synchronize()
    o.check(c["id"] + " batch-inner")
    keep = _np(hip.attn_dropout_mask(B, H, T, S, 0.5, ac.DROP_SEED, dev)) if c["drop"] else None
    return dict(out=out, lse=lse, delta=delta, dgain_rows=dgr, dq=dq, dk=dk, dv=dv, dbias=dbias, keep=keep, dense=dense)


@pytest.mark.parametrize("case", ac.BI_CASES, ids=_ids(ac.BI_CASES))
def test_select_batch_inner(case):
    """select / poison through ifseg_attn_bias_pack, ifseg_attn_fwd_bi and ifseg_attn_bwd_bi (+- kv_len, +- dropout at p = 0.5)"""
    from ifseg_amd import hip
    dev = _dev()
    c, H = case, case["H"]
    d = ac.select_inputs(c)
    r = _run_bi(hip, c, d, dev, dq_scale=0.5)
    if c["drop"]:
        frac = r["keep"].mean()
        assert set(np.unique(r["keep"])) == {0.0, 1.0} and 0.4 < frac < 0.6, frac
    e = ac.select_expect(c, d, r["keep"])
    what = "%s %s " % (c["id"], c["reach"])
    _exact(what + "out", _heads(r["out"], H), e["out"])
    _lse_ok(what, _np(r["lse"]), e["lse"])
    _exact(what + "delta", _np(r["delta"]), (np.transpose(d["dout"], (0, 2, 1, 3)) * np.transpose(e["out"], (0, 2, 1, 3))).sum(-1))
    _exact(what + "dv", _heads(r["dv"], H), e["dv"])
    for name in ("dq", "dk", "dbias"):
        _exact(what + name, _np(r[name]), np.zeros(r[name].shape))
    dgr = _np(r["dgain_rows"])
    assert (np.abs(dgr - e["dgain_rows"]) <= 2.0 ** -12 * np.abs(e["dgain_rows"])).all(), what + "dgain_rows"
    # DKV and DQ alone give the bits of the single call
    r2 = _run_bi(hip, c, d, dev, dq_scale=0.5, phases=(2, 4))
    for name in ("dq", "dk", "dv", "dbias", "dgain_rows"):
        assert torch.equal(_bits(r[name].contiguous()), _bits(r2[name].contiguous())), name


@pytest.mark.parametrize("case", [c for c in ac.UNIFORM_CASES if c["entry"] == "bi"], ids=_ids([c for c in ac.UNIFORM_CASES if c["entry"] == "bi"]))
def test_uniform_batch_inner(case):
    from ifseg_amd import hip
    dev = _dev()
    c, H = case, case["H"]
    u = ac.uniform_inputs(c)
    B, T, S = c["B"], c["T"], c["S"]
    d = dict(q=np.zeros((B, T, H, 64)), k=np.zeros((B, S, H, 64)), v=u["v"], dout=u["dout"], bi_bias=np.zeros((H, T, S)), gain=u["gain"])
    e = ac.uniform_expect(c, u)
    r = _run_bi(hip, c, d, dev)
    what = "%s uniform " % c["id"]
    _within(what + "out", _heads(r["out"], H), e["out"], e["out_b"] + 1e-30)
    _within(what + "dv", _heads(r["dv"], H), e["dv"], e["dv_b"] + 1e-30)


# ================================================================================================== part B
@pytest.mark.parametrize("case", ac.RANDOM_CASES, ids=_ids(ac.RANDOM_CASES))
def test_random_per_element(case):
    """the `_rand` data of test_kernels_gpu.py, per element against the fp64 reference within the bounds of _attn_cases.py; the
    backward reference takes the kernel's own out and lse (both checked first)"""
    from ifseg_amd import hip
    dev = _dev()
    c, H = case, case["H"]
    d = ac.random_inputs(c)
    what = "%s " % c["id"]
    log = {}
    if c["entry"] == "bi":
        r = _run_bi(hip, c, d, dev, dq_scale=0.5)
        ks = 2.0 * r["keep"] if c["drop"] else None
        out, lse = r["out"], r["lse"]
    else:
        ops, out, lse = _run_fwd(hip, c, d, dev)
        ks = None
    ref = ac.forward_ref(c, d, ks)
    _within(what + "out", _heads(out, H), ref["out"], ref["out_b"], log)
    _within(what + "lse", _np(lse), ref["lse"], ac.lse_bound(c, d, ref["lse"]), log)
    if c["dense"]:
        print("[part B] %s %s" % (c["id"], log))
        return
    if c["entry"] != "bi":
        r = _run_bwd(hip, c, d, dev, ops, out, lse, dq_scale=0.5, dpq_scale=0.25)
    b = ac.backward_ref(c, d, _heads(out, H), _np(lse), ks, 0.5)
    _within(what + "delta", _np(r["delta"]), b["delta"], 2.0 ** -18 * (np.abs(np.transpose(d["dout"], (0, 2, 1, 3)) * np.transpose(_heads(out, H), (0, 2, 1, 3)))).sum(-1) + 1e-30, log)
    for name in ("dv", "dq", "dk"):
        _within(what + name, _heads(r[name], H), b[name], b[name + "_b"], log)
    _within(what + "dgain_rows", _np(r["dgain_rows"]), b["dgain_rows"], b["dgain_rows_b"], log)
    if c["entry"] == "bi":
        ng = (c["B"] + 3) // 4
        db = _np(r["dbias"])
        assert not db[..., c["S"]:].any(), what + "dbias beyond S"
        # ifseg_attn_dbias_sum over these slabs: fp32 additions in slab order (exactness is test_ops_gpu.py's subject)
        tot = _Outs(dev)
        dsum = tot.flat((H, c["T"], c["S"]))
        tot.freeze()
        hip.attn_dbias_sum(r["dbias"], c["S"], dsum)
        torch.cuda.synchronize()
        acc = np.zeros((H, c["T"], c["S"]), dtype=np.float32)
        for g in range(ng):
            acc = acc + db[g, :, :, :c["S"]].astype(np.float32)
        _exact(what + "dbias_sum", _np(dsum), acc.astype(np.float64))
        tot.check(what + "dbias_sum")
        for g in range(ng):
            sl = slice(4 * g, 4 * g + 4)
            refg, bg = b["dS"][sl].sum(0), b["w"][sl].sum(0)
            fin = np.isfinite(ac.scores(c, d)[sl]).any(0)
            _within(what + "slab%d dbias" % g, np.where(fin, db[g, :, :, :c["S"]], 0), refg, ac.U * np.abs(refg) + bg + 1e-30, log)
    elif c["pos"]:
        _within(what + "dpq", _np(r["dpq"]).reshape(c["B"], c["T"], H, 64), 0.25 * b["dpq"], ac.U * 0.25 * np.abs(b["dpq"]) + 0.25 * b["dpq_b"] + 1e-30, log)
        _within(what + "dpk", _np(r["dpk"]).reshape(c["B"], c["S"], H, 64), b["dpk"], ac.U * np.abs(b["dpk"]) + b["dpk_b"] + 1e-30, log)
    if c["entry"] != "bi" and c["gh"]:
        # the fp32 table partials (bounds: ac.table_refs_and_bounds; the class-sum term only on row32 / rowseg grids, d rel2d only)
        refs, errs = ac.table_refs_and_bounds(c, d["tabs"], b)
        for name, pt, rf, eb in zip(("drel2d", "drel1d", "drelx"), r["parts"], refs, errs):
            _within(what + name, _np(pt).sum(1), rf, eb, log)
    print("[part B] %s %s" % (c["id"], log))


# ================================================================================================== part C
def test_attn_delta_exact():
    from ifseg_amd import hip
    dev = _dev()
    for B, H, T in ((1, 1, 1), (2, 3, 65), (3, 2, 129)):
        C = H * 64
        rng = np.random.default_rng(T)
        o_, do_ = rng.integers(-4, 5, (B, T, C)).astype(np.float64), rng.integers(-4, 5, (B, T, C)).astype(np.float64)
        outs = _Outs(dev)
        delta = outs.flat((B, H, T))
        outs.freeze()
        out = _guarded(_t(o_), BF16, dev, 8, ac.V_POISON)[1]
        dout = _guarded(_t(do_), BF16, dev, 8, ac.V_POISON)[1]
        hip.attn_delta(out, dout, delta, B, H, T)
        torch.cuda.synchronize()
        _exact("attn_delta", _np(delta), np.transpose((o_ * do_).reshape(B, T, H, 64).sum(-1), (0, 2, 1)))
        outs.check("attn_delta")


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("grid", [(2, 32, 37), (8, 8, 1), (4, 40, 1)], ids=["2x32+37", "8x8+1", "4x40+1"])
def test_dense_bias_bit_for_bit(grid, causal):
    """ifseg_attn_dense_bias on integer pos operands (|pos_q . pos_k| <= 256) and integer tables: D bit for bit, the -inf pattern,
    and the tiles it documents as unwritten under causal untouched"""
    from ifseg_amd import hip
    dev = _dev()
    gh, gw, Lt = grid
    H, P = 2, gh * gw
    T = S = P + Lt
    C = H * 64
    rng = np.random.default_rng(gh * 100 + gw)
    pq, pk = rng.integers(-1, 2, (T, H, 64)).astype(np.float64), rng.integers(-1, 2, (S, H, 64)).astype(np.float64)
    c = dict(H=H, T=T, S=S, P=P, Lt=Lt, gh=gh, gw=gw, causal=causal)
    tabs = ac._bias_tables(c, rng, False)
    want = np.einsum("thd,shd->hts", pq, pk) + ac.dense_rel(c, tabs)
    assert np.abs(want).max() <= 256
    if causal:
        want = np.where(ac.causal_mask(T, S, P)[None], -np.inf, want)
    o = _Outs(dev)
    dense = hip.DenseBias(H, T, S, dev)
    dense.D = o.flat((H, dense.Tp, dense.Sp), BF16)
    o.freeze()
    before = dense.D.clone()
    f = lambda a: _flat_guarded(_t(a, F32), F32, dev, ac.POISON_REL)[1]
    rel = hip.RelBias(P, torch.from_numpy(tabs["gcode"]).to(dev), tabs["code_bias"], f(tabs["rel2d"]), f(tabs["rel1d"]), f(tabs["relx"]), grid_w=gw)
    pqt = _guarded(_t(pq.reshape(1, T, C)), BF16, dev, 8, GUARD)[1][0]
    pkt = _guarded(_t(pk.reshape(1, S, C)), BF16, dev, 8, GUARD)[1][0]
    hip.attn_dense_bias(dense, pqt, pkt, rel=rel, causal=causal, P=P)
    torch.cuda.synchronize()
    o.check("attn_dense_bias")
    full = np.full((H, dense.Tp, dense.Sp), -np.inf)
    full[:, :T, :S] = want
    got = _np(dense.D)
    if causal:
        i, j = np.arange(dense.Tp)[:, None], np.arange(dense.Sp)[None, :]
        unread = (j < P) & ((i // 32 * 32 >= P) | (j // 32 > i // 32 + 1))
        # unwritten tiles hold what they held or -inf; nothing finite that was not there before
        g_un, b_un = got[:, unread], _np(before)[:, unread]
        assert ((g_un == b_un) | np.isneginf(g_un)).all(), "a tile outside every schedule holds a new finite value"
        got = np.where(unread[None], full, got)
    _exact("attn_dense_bias %s causal %s" % (grid, causal), got, full)


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("acc", [False, True], ids=["store", "accumulate"])
def test_dbias_grads_exact(acc, causal):
    """ifseg_attn_dbias_grads on integer bf16 slabs and +-1 / 0 pos operands: dpq, dpk and the three table partials summed over
    NP are exact integers"""
    from ifseg_amd import hip
    dev = _dev()
    gh, gw, Lt, H, ng = 2, 32, (1 if causal else 5), 2, 3
    P = gh * gw
    T = S = P + Lt
    C, Sp = H * 64, (S + 31) // 32 * 32
    rng = np.random.default_rng(11 + acc)
    slabs = np.zeros((ng, H, T, Sp))
    slabs[..., :S] = rng.integers(-2, 3, (ng, H, T, S))
    if causal:
        slabs[..., :S] *= ~ac.causal_mask(T, S, P)[None, None]
    pq, pk = rng.integers(-1, 2, (T, H, 64)).astype(np.float64), rng.integers(-1, 2, (S, H, 64)).astype(np.float64)
    dB = slabs.sum(0)[..., :S]
    c = dict(H=H, T=T, S=S, P=P, Lt=Lt, gh=gh, gw=gw)
    gcode, code_bias, n2d = ac.grid_codes(gh, gw)
    want2, want1, wantx = ac.table_grads(c, dict(gcode=gcode, code_bias=code_bias, n2d=n2d), dB)
    prior_q, prior_k = rng.integers(-3, 4, (T, C)).astype(np.float64), rng.integers(-3, 4, (S, C)).astype(np.float64)
    o = _Outs(dev)
    dpq, dpk = o.flat((T, C)), o.flat((S, C))
    NP = hip.dbias_nparts()
    g2, g1, gx = o.flat((H, NP, n2d)), o.flat((H, NP, 2 * Lt - 1)), o.flat((H, NP, 2))
    dpq.copy_(_t(prior_q, F32)); dpk.copy_(_t(prior_k, F32))
    o.freeze()
    dbias = _flat_guarded(_t(slabs), BF16, dev, ac.V_POISON)[1]
    pqt = _guarded(_t(pq.reshape(1, T, C)), BF16, dev, 8, ac.V_POISON)[1][0]
    pkt = _guarded(_t(pk.reshape(1, S, C)), BF16, dev, 8, ac.V_POISON)[1][0]
    hip.attn_dbias_grads(dbias, S, pos_q=pqt, pos_k=pkt, dpq_acc=dpq, dpk_acc=dpk, accumulate_pos=acc, dpq_scale=0.5, P=P, grid_h=gh,
                         grid_w=gw, drel2d=g2, drel1d=g1, drelx=gx, causal=causal)
    torch.cuda.synchronize()
    o.check("attn_dbias_grads")
    wq = 0.5 * np.einsum("hts,shd->thd", dB, pk).reshape(T, C) + (prior_q if acc else 0)
    wk = np.einsum("hts,thd->shd", dB, pq).reshape(S, C) + (prior_k if acc else 0)
    _exact("dpq", _np(dpq), wq)
    _exact("dpk", _np(dpk), wk)
    _exact("drel2d", _np(g2).sum(1), want2)
    _exact("drel1d", _np(g1).sum(1), want1)
    _exact("drelx", _np(gx).sum(1), wantx)


def test_bwd_reduce_exact():
    """ifseg_attn_bwd_reduce on integers: the batch sums of the abs-pos partials (store and accumulate), the table partials
    scattered into their buckets, d c_attn = sum delta / gain with gains that divide exactly"""
    from ifseg_amd import hip
    dev = _dev()
    B, H, T, S, nparts = 3, 2, 65, 33, 5
    C = H * 64
    rng = np.random.default_rng(7)
    pq, pk = rng.integers(-3, 4, (B, T, C)).astype(np.float64), rng.integers(-3, 4, (B, S, C)).astype(np.float64)
    delta = rng.integers(-4, 5, (B, H, T)).astype(np.float64)
    gain = np.array([0.5, -2.0])
    n, nb = 37, 9
    part = rng.integers(-3, 4, (H, nparts, n)).astype(np.float64)
    idx = rng.integers(-1, nb, n).astype(np.int32)
    prior = rng.integers(-3, 4, (nb, H)).astype(np.float64)
    for acc in (False, True):
        o = _Outs(dev)
        aq, ak, tacc = o.flat((T, C)), o.flat((S, C)), o.flat((nb, H))
        dgain = o.flat((H,), BF16)
        aq.fill_(1.0); ak.fill_(2.0); tacc.copy_(_t(prior, F32))
        o.freeze()
        hip.attn_bwd_reduce(B, H, T, S, C, _flat_guarded(_t(pq), BF16, dev, ac.V_POISON)[1], _flat_guarded(_t(pk), BF16, dev, ac.V_POISON)[1],
                            aq, ak, acc, _flat_guarded(_t(delta, F32), F32, dev, ac.V_POISON)[1], _t(gain, F32).to(dev), dgain, nparts,
                            [(_flat_guarded(_t(part, F32), F32, dev, ac.V_POISON)[1], torch.from_numpy(idx).to(dev), tacc)])
        torch.cuda.synchronize()
        o.check("attn_bwd_reduce")
        _exact("dpos_q_acc", _np(aq), pq.sum(0) + (1.0 if acc else 0.0))
        _exact("dpos_k_acc", _np(ak), pk.sum(0) + (2.0 if acc else 0.0))
        want = prior.copy()
        for j in range(n):
            if idx[j] >= 0:
                want[idx[j]] += part[:, :, j].sum(1)
        _exact("table buckets", _np(tacc), want)
        _exact("dgain", _np(dgain), ac.bf16_round(delta.sum((0, 2)) / gain).astype(np.float64))     # fp32 sum and quotient exact, one rounding


# ================================================================================================== part D
def test_bad_arguments_are_refused():
    """return codes only: every call below is refused before a launch, and the sentinel-filled outputs stay untouched"""
    from ifseg_amd import hip
    dev = _dev()
    L = hip.lib()
    i, ll, P = ctypes.c_int, ctypes.c_longlong, lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    off = lambda t, n: ctypes.c_void_p(t.data_ptr() + n)
    St = hip._stream()
    B, H, T, S, C = 1, 1, 64, 64, 64
    X = torch.ones(B, T + 1, C + 8, dtype=BF16, device=dev)
    OUT = torch.full((B, T + 1, C + 8), SENTINEL, dtype=BF16, device=dev)
    D3 = [torch.full((B, T + 1, C + 8), SENTINEL, dtype=BF16, device=dev) for _ in range(5)]
    LSE = torch.full((3, B, H, T + 8), SENTINEL, dtype=F32, device=dev)
    DENSE = torch.zeros(H, T, 72, dtype=F32, device=dev)
    TAB = torch.zeros(H, 4096, dtype=F32, device=dev)
    PART = torch.full((3, H, 4096), SENTINEL, dtype=F32, device=dev)
    GC = torch.zeros(64, dtype=I32, device=dev)
    outs = [OUT, LSE, PART] + D3
    want = [t.clone() for t in outs]
    ld, bs = C + 8, (T + 1) * (C + 8)

    def fwd(q=P(X), pq=None, pk=None, ldq=ld, ldpq=ld, ldpk=ld, q_bs=bs, P_=64, rel=0, dense=None, dense_ld=0, causal=0, Tt=T):
        return L.ifseg_attn_fwd(q, P(X), P(X), pq, pk, P(OUT), P(LSE), i(B), i(H), i(Tt), i(S), i(ldq), i(ld), i(ld), i(ld), i(ldpq), i(ldpk),
                                ll(q_bs), ll(bs), ll(bs), ll(bs), i(rel), i(P_), P(GC) if rel else None, i(0), i(1), P(TAB) if rel else None,
                                P(TAB) if rel else None, P(TAB) if rel else None, i(causal), dense, None, i(0), i(dense_ld), St)

    def bwd(**kw):
        a = hip._AttnBwdArgs()
        for n in ("q", "k", "v", "out", "dout"):
            setattr(a, n, X.data_ptr())
        a.lse, a.delta, a.dgain_rows = LSE[0].data_ptr(), LSE[1].data_ptr(), LSE[2].data_ptr()
        a.dq, a.dk, a.dv, a.dpos_q_part, a.dpos_k_part = (t.data_ptr() for t in D3)
        a.B, a.H, a.T, a.S, a.P = B, H, T, S, S
        for n in ("ldq", "ldk", "ldv", "ldpq", "ldpk", "ldout", "lddo", "lddq", "lddk", "lddv"):
            setattr(a, n, ld)
        for n in ("q_bs", "k_bs", "v_bs", "out_bs", "do_bs", "dq_bs", "dk_bs", "dv_bs"):
            setattr(a, n, bs)
        a.dq_scale = a.dpq_scale = 1.0
        for k_, v_ in kw.items():
            setattr(a, k_, v_)
        return L.ifseg_attn_bwd(ctypes.byref(a), St)

    DB = torch.zeros(64 * 64 + 16, dtype=BF16, device=dev)
    DB16 = torch.full((64 * 64 + 16,), SENTINEL, dtype=BF16, device=dev)          # the D that ifseg_attn_dense_bias would write
    SLABIN = torch.zeros(H * T * 64 + 16, dtype=BF16, device=dev)
    SLAB = torch.full((1, H, T, 64), SENTINEL, dtype=BF16, device=dev)
    outs.append(SLAB)
    want.append(SLAB.clone())

    def bi(fn, **kw):
        a = hip._AttnBiArgs()
        a.q = a.k = a.v = a.dout = X.data_ptr()
        a.lse, a.delta, a.D = LSE[0].data_ptr(), LSE[1].data_ptr(), DB.data_ptr()
        a.dq, a.dk, a.dv, a.out, a.dbias = D3[0].data_ptr(), D3[1].data_ptr(), D3[2].data_ptr(), OUT.data_ptr(), SLAB.data_ptr()
        a.B, a.H, a.T, a.S, a.Sp, a.Tp = B, H, T, S, 64, 64
        for n in ("ldq", "ldk", "ldv", "lddo", "lddq", "lddk", "lddv", "ldout"):
            setattr(a, n, ld)
        for n in ("q_bs", "k_bs", "v_bs", "do_bs", "dq_bs", "dk_bs", "dv_bs", "out_bs"):
            setattr(a, n, bs)
        a.dq_scale = 1.0
        for k_, v_ in kw.items():
            setattr(a, k_, v_)
        return fn(ctypes.byref(a), St)

    rel_kw = dict(rel_mode=1, P=64, gcode=GC.data_ptr(), n2d=1, rel2d=TAB.data_ptr(), rel1d=TAB.data_ptr(), relx=TAB.data_ptr(), nparts=1,
                  T=65, S=65)
    parts = dict(drel2d_part=PART[0].data_ptr(), drel1d_part=PART[1].data_ptr(), drelx_part=PART[2].data_ptr())
    # positive controls: the argument sets the rows below alter one at a time are accepted as they stand
    assert fwd() == 0 and fwd(pq=P(X), pk=P(X)) == 0 and fwd(dense=P(DENSE), dense_ld=72) == 0
    assert bwd() == 0 and bwd(pos_q=X.data_ptr(), pos_k=X.data_ptr()) == 0 and bwd(**rel_kw, **parts) == 0
    assert bi(L.ifseg_attn_fwd_bi) == 0 and bi(L.ifseg_attn_bwd_bi) == 0
    torch.cuda.synchronize()
    for t, w in zip(outs, want):                      # (they wrote: refill the sentinels)
        t.copy_(w)

    def dense_bias(pq=P(X), pk=P(X)):
        return L.ifseg_attn_dense_bias(pq, pk, i(ld), i(ld), i(H), i(T), i(S), i(0), i(S), None, i(0), i(0), None, None, None, i(0), P(DB16),
                                       i(64), i(64), St)

    def dbias_grads(**kw):
        a = hip._AttnDbiasArgs()
        a.dbias, a.ng, a.H, a.T, a.S, a.Sp, a.C = SLABIN.data_ptr(), 1, H, T, S, 64, C
        a.pos_q = a.pos_k = X.data_ptr()
        a.ldpq = a.ldpk = ld
        a.dpos_q_acc, a.dpos_k_acc, a.dpq_scale = PART[0].data_ptr(), PART[1].data_ptr(), 1.0
        for k_, v_ in kw.items():
            setattr(a, k_, v_)
        return L.ifseg_attn_dbias_grads(ctypes.byref(a), St)

    assert dense_bias() == 0 and dbias_grads() == 0
    torch.cuda.synchronize()
    PART.fill_(SENTINEL)
    DB16.fill_(SENTINEL)
    outs.append(DB16)
    want.append(DB16.clone())
    calls = {
        # ---- refused before this suite
        "fwd ldq % 8": (fwd(ldq=ld + 4), BAD_SHAPE), "fwd q_bs % 8": (fwd(q_bs=bs + 4), BAD_SHAPE), "fwd q base % 16": (fwd(q=off(X, 8)), BAD_ARG),
        "fwd P % 64 (causal)": (fwd(P_=32, causal=1), BAD_SHAPE), "fwd dense_ld < S": (fwd(dense=P(DENSE), dense_ld=60), BAD_ARG),
        "bwd lddq % 8": (bwd(lddq=ld + 4), BAD_SHAPE), "bwd dq_bs % 8": (bwd(dq_bs=bs + 4), BAD_SHAPE),
        "bwd dq base % 16": (bwd(dq=D3[0].data_ptr() + 8), BAD_ARG),
        "bwd nparts != B ceil(S / 128)": (bwd(**dict(rel_kw, nparts=2), **parts), BAD_ARG),
        # ---- refused since this suite (the kernels read pos rows and dense-bias rows 16 bytes at a time and write every optional
        # output they are compiled for; none of this was verified by the host)
        "fwd ldpq % 8": (fwd(pq=P(X), pk=P(X), ldpq=ld + 4), BAD_SHAPE), "fwd ldpk % 8": (fwd(pq=P(X), pk=P(X), ldpk=ld + 4), BAD_SHAPE),
        "fwd pos_q base % 16": (fwd(pq=off(X, 8), pk=P(X)), BAD_ARG), "fwd pos_k base % 16": (fwd(pq=P(X), pk=off(X, 8)), BAD_ARG),
        "fwd pos_q without pos_k": (fwd(pq=P(X)), BAD_ARG), "fwd pos_k without pos_q": (fwd(pk=P(X)), BAD_ARG),
        "fwd dense base % 16 on the float4 path": (fwd(dense=off(DENSE, 4), dense_ld=68), BAD_ARG),
        "fwd rel_mode without tables": (L.ifseg_attn_fwd(P(X), P(X), P(X), None, None, P(OUT), P(LSE), i(B), i(H), i(T), i(S), i(ld), i(ld), i(ld),
                                                           i(ld), i(0), i(0), ll(bs), ll(bs), ll(bs), ll(bs), i(1), i(64), None, i(0), i(1), None,
                                                           None, None, i(0), None, None, i(0), i(0), St), BAD_ARG),
        "bwd ldpq % 8": (bwd(pos_q=X.data_ptr(), pos_k=X.data_ptr(), ldpq=ld + 4), BAD_SHAPE),
        "bwd pos_k base % 16": (bwd(pos_q=X.data_ptr(), pos_k=X.data_ptr() + 8), BAD_ARG),
        "bwd pos_q without pos_k": (bwd(pos_q=X.data_ptr()), BAD_ARG),
        "bwd pos without the abs-pos partials": (bwd(pos_q=X.data_ptr(), pos_k=X.data_ptr(), dpos_q_part=None), BAD_ARG),
        "bwd rel_mode without the table partials": (bwd(**rel_kw), BAD_ARG),
        "bwd rel_mode without tables": (bwd(**dict(rel_kw, rel2d=None), **parts), BAD_ARG),
        "bwd DKV without dk": (bwd(dk=None), BAD_ARG), "bwd DQ without dq": (bwd(dq=None), BAD_ARG),
        "bwd DELTA without delta": (bwd(delta=None), BAD_ARG),
        "bwd out base % 16": (bwd(out=X.data_ptr() + 8), BAD_ARG), "bwd out_bs % 8": (bwd(out_bs=bs + 4), BAD_SHAPE),
        "bwd dpos_q_part base % 16": (bwd(pos_q=X.data_ptr(), pos_k=X.data_ptr(), dpos_q_part=D3[3].data_ptr() + 8), BAD_ARG),
        "bwd dpos_k_part base % 16": (bwd(pos_q=X.data_ptr(), pos_k=X.data_ptr(), dpos_k_part=D3[4].data_ptr() + 8), BAD_ARG),
        "bwd_bi DQ without dq (nothing launched for DKV either)": (bi(L.ifseg_attn_bwd_bi, dq=None), BAD_ARG),
        "dense_bias pos_q base % 16": (dense_bias(pq=off(X, 8)), BAD_ARG), "dense_bias pos_k base % 16": (dense_bias(pk=off(X, 8)), BAD_ARG),
        "dbias_grads dbias base % 16": (dbias_grads(dbias=SLABIN.data_ptr() + 8), BAD_ARG),
        "dbias_grads pos_q base % 16": (dbias_grads(pos_q=X.data_ptr() + 8), BAD_ARG),
        "dbias_grads pos_k base % 16": (dbias_grads(pos_k=X.data_ptr() + 8), BAD_ARG),
        "fwd_bi D base % 16": (bi(L.ifseg_attn_fwd_bi, D=DB.data_ptr() + 8), BAD_ARG),
        "bwd_bi D base % 16": (bi(L.ifseg_attn_bwd_bi, D=DB.data_ptr() + 8), BAD_ARG),
        "bwd_bi without lse": (bi(L.ifseg_attn_bwd_bi, lse=None), BAD_ARG), "bwd_bi without delta": (bi(L.ifseg_attn_bwd_bi, delta=None), BAD_ARG),
        # ---- batch-inner, refused before this suite
        "fwd_bi Sp % 32": (bi(L.ifseg_attn_fwd_bi, Sp=72), BAD_ARG), "bwd_bi lddq % 8": (bi(L.ifseg_attn_bwd_bi, lddq=ld + 4), BAD_SHAPE),
        "bwd_bi dbias base % 16": (bi(L.ifseg_attn_bwd_bi, dbias=SLAB.data_ptr() + 8), BAD_ARG),
        "fwd_bi p = 1": (bi(L.ifseg_attn_fwd_bi, drop_p=1.0), BAD_ARG),
    }
    torch.cuda.synchronize()
    wrong = {k: v for k, v in calls.items() if v[0] != v[1]}
    assert not wrong, "return codes (got, expected): %s" % wrong
    for t, w in zip(outs, want):
        assert torch.equal(_bits(t), _bits(w)), "a refused call wrote to its output"
    # the aligned dense bias at a row stride that is no multiple of 4 is NOT refused: it takes the scalar path (part A runs it)
    assert ac.reach(ac.by_id("dense-ldodd-165")) == "dslow/nopos"
