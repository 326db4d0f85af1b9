"""GPU: the training-path ops of ifseg_amd/ops.py (attention_bias, bias_attention_bi, seg_loss), the two kernels behind
attention_bias (csrc/attention_ops.hip: ifseg_attn_bias_pack, ifseg_attn_dbias_sum) and ifseg_amd.modules.MultiheadAttention,
against plain PyTorch fp32 references / the oracle, through the dispatcher and autograd."""
import pytest
import torch
import torch.nn.functional as F

import segofa_ref as O

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
NEG = float("-inf")


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import ifseg_amd.ops  # noqa: F401
    return torch.device("cuda:0")


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-30)).item()


def _rand(shape, dev, seed, scale=1.0, dtype=BF):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dev).to(dtype)


def _causal_mask(T, S, P):
    """the engine's decoder order (P grid tokens first, the tail behind them): True = masked"""
    i = torch.arange(T)[:, None]
    j = torch.arange(S)[None, :]
    grid_key = j < P
    return (grid_key & ((i >= P) | (j > i))) | (~grid_key & (i >= P) & (j > i))


def _grid_codes(gh, gw):
    ys, xs = torch.meshgrid(torch.arange(gh), torch.arange(gw), indexing="ij")
    code = (ys * (2 * gw - 1) + xs).reshape(-1).int()
    return code, (gh - 1) * (2 * gw - 1) + (gw - 1), (2 * gh - 1) * (2 * gw - 1)


def _dense_rel_ad(H, T, S, P, gcode, code_bias, rel2d, rel1d, relx):
    """the rel-pos bias [H,T,S] from its tables, autograd friendly"""
    Lt = T - P
    idx = gcode[:, None] - gcode[None, :] + code_bias
    gg = rel2d[:, idx]
    if Lt == 0:
        return gg
    t = torch.arange(Lt, device=rel1d.device)
    tt = rel1d[:, t[:, None] - t[None, :] + Lt - 1]
    gt = relx[:, 0][:, None, None].expand(H, P, Lt)
    tg = relx[:, 1][:, None, None].expand(H, Lt, P)
    return torch.cat([torch.cat([gg, gt], 2), torch.cat([tg, tt], 2)], 1)


def _attn_ref(q, k, v, bias, gain, mask=None, km=None):
    """fp32: gain_h * (softmax(q k^T + bias [masked]) o km) v with ONE [H,T,S] bias broadcast over the batch; mask broadcastable
    to [B,H,T,S] (True = masked), km = keep / (1 - p) or None"""
    B, T, C = q.shape
    H, S = C // 64, k.shape[1]
    qh, kh, vh = (t.view(B, -1, H, 64).transpose(1, 2) for t in (q, k, v))
    s = qh @ kh.transpose(2, 3)
    if bias is not None:
        s = s + bias
    if mask is not None:
        s = s.masked_fill(mask, NEG)
    p = torch.softmax(s, -1)
    if km is not None:
        p = p * km
    o = p @ vh
    if gain is not None:
        o = o * gain.view(1, H, 1, 1)
    return o.transpose(1, 2).reshape(B, T, C)


def _pad32(n):
    return (n + 31) // 32 * 32


# ------------------------------------------------------------------------------------------------- 1. pack, exact
@pytest.mark.parametrize("T,S", [(76, 76), (1061, 1061), (1025, 1061), (65, 1024)])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("src", ["f32", "bf16", "f32_view", "bf16_view", "f32_padded_view", "none"])
def test_attn_bias_pack_is_exact(T, S, causal, src):
    from ifseg_amd import hip
    dev = _dev()
    H = 3
    P = (64 if min(T, S) < 1024 else 1024) if causal else None
    bias = None
    if src != "none":
        dt = F32 if src.startswith("f32") else BF
        if src.endswith("padded_view"):        # rows 16-byte aligned, row stride != S
            bias = _rand((H, T, _pad32(S) + 8), dev, 1, 3.0, dt)[:, :, :S]
        elif src.endswith("view"):             # odd offsets and strides: the element-wise path
            bias = _rand((H + 1, T + 3, S + 5), dev, 1, 3.0, dt)[1:, 2:T + 2, 3:S + 3]
        else:
            bias = _rand((H, T, S), dev, 1, 3.0, dt)
        assert bias.stride(2) == 1
    dense = hip.DenseBias(H, T, S, dev)
    dense.D.fill_(7.0)
    hip.attn_bias_pack(dense, bias, causal=causal, P=P)
    want = torch.full((H, dense.Tp, dense.Sp), NEG, dtype=BF, device=dev)
    want[:, :T, :S] = bias.to(BF) if bias is not None else 0.0
    if causal:
        want[:, :T, :S] = want[:, :T, :S].masked_fill(_causal_mask(T, S, P).to(dev), NEG)
    torch.cuda.synchronize()
    assert torch.equal(dense.D.view(torch.int16), want.view(torch.int16))


# ------------------------------------------------------------------------------------------------- 2. sum, exact
@pytest.mark.parametrize("H,T,S", [(2, 76, 76), (3, 101, 1061), (2, 65, 1024), (1, 33, 7)])
@pytest.mark.parametrize("ng", [1, 2, 3])
@pytest.mark.parametrize("out_kind", ["f32", "bf16", "f32_view", "bf16_view"])
def test_attn_dbias_sum_is_exact(H, T, S, ng, out_kind):
    from ifseg_amd import hip
    dev = _dev()
    Sp = _pad32(S)
    d = _rand((ng, H, T, Sp), dev, 2)
    dt = F32 if out_kind.startswith("f32") else BF
    if out_kind.endswith("view"):
        buf = torch.full((H + 1, T + 2, S + 3), 5.0, dtype=dt, device=dev)
        out = buf[1:, 1:T + 1, 2:S + 2]
    else:
        buf = out = torch.full((H, T, S), 5.0, dtype=dt, device=dev)
    hip.attn_dbias_sum(d, S, out)
    acc = d[0].float()
    for g in range(1, ng):
        acc += d[g].float()
    want = acc[:, :, :S].to(dt)
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    if out_kind.endswith("view"):              # nothing outside the view was touched
        keep = torch.full_like(buf, 5.0)
        keep[1:, 1:T + 1, 2:S + 2] = want
        assert torch.equal(buf, keep)


# ------------------------------------------------------------------------------------------------- 3. attention_bias vs fp32 autograd
def _inf_block_bias(H, T, S, dev, seed, dtype=F32):
    """finite random bias with -inf blocks: rows >= 40 see none of the first 40 keys (whole leading key blocks masked)"""
    b = _rand((H, T, S), dev, seed, 1.0, dtype)
    b[:, 40:, :40] = NEG
    return b


AB_CASES = {
    # name: (B, H, T, S, bias kind, bias dtype, op-causal P, kv_len, gain)
    "encoder": (8, 2, 1061, 1061, "rand", F32, None, False, True),
    "cross": (2, 2, 1025, 1061, "rand", BF, None, False, True),
    "b5": (5, 2, 164, 164, "rand", F32, None, False, True),
    "inf_blocks": (3, 2, 76, 76, "inf_blocks", F32, None, False, True),
    "inf_blocks_bf16": (3, 2, 164, 164, "inf_blocks", BF, None, False, True),
    "triu_causal": (2, 2, 100, 100, "triu", F32, None, False, True),
    "op_causal": (2, 2, 1025, 1025, "rand", F32, 1024, False, True),
    "kv_len": (4, 2, 164, 200, "rand", F32, None, True, True),
    "no_bias": (2, 2, 164, 164, None, F32, None, False, True),
    "no_gain": (2, 2, 164, 164, "rand", BF, None, False, False),
    "no_bias_no_gain": (5, 1, 76, 100, None, F32, None, False, False),
}


@pytest.mark.parametrize("case", sorted(AB_CASES))
def test_attention_bias_against_fp32_autograd(case):
    dev = _dev()
    B, H, T, S, kind, bdt, P, pad, use_gain = AB_CASES[case]
    C = H * 64
    q, k, v = _rand((B, T, C), dev, 20, 0.35), _rand((B, S, C), dev, 21), _rand((B, S, C), dev, 22)
    dout = _rand((B, T, C), dev, 25)
    bias = None
    if kind == "rand":
        bias = _rand((H, T, S), dev, 26, 1.0, bdt)
    elif kind == "inf_blocks":
        bias = _inf_block_bias(H, T, S, dev, 26, bdt)
    elif kind == "triu":
        bias = _rand((H, T, S), dev, 26, 1.0, bdt).masked_fill(torch.ones(T, S, dtype=torch.bool, device=dev).triu(1), NEG)
    gain = None
    if use_gain:
        gain = (1.0 + 0.2 * torch.randn(H, generator=torch.Generator().manual_seed(5))).to(dev)
        gain[0] = 0.0                      # head gains of exactly zero and of negative sign
        gain[H - 1] = -0.7
    kv_len, mask = None, None
    if pad:
        lens = [S, S - 7, S, S - 40][:B]   # two padded samples: a partly and a fully masked 32-key block
        kv_len = torch.tensor(lens, dtype=torch.int32, device=dev)
        mask = (torch.arange(S, device=dev)[None, :] >= kv_len[:, None].long())[:, None, None, :]
    if P is not None:
        mask = _causal_mask(T, S, P).to(dev)
    # ---- fp32 autograd reference
    qf, kf, vf = (t.float().clone().requires_grad_(True) for t in (q, k, v))
    bf_ = bias.float().clone().requires_grad_(True) if bias is not None else None
    gf = gain.clone().requires_grad_(True) if gain is not None else None
    o_ref = _attn_ref(qf, kf, vf, bf_, gf, mask)
    (o_ref * dout.float()).sum().backward()
    assert torch.isfinite(o_ref).all()
    # ---- the op
    for t in (q, k, v):
        t.requires_grad_(True)
    if bias is not None:
        bias.requires_grad_(True)
    if gain is not None:
        gain.requires_grad_(True)
    out, lse, packed = torch.ops.ifseg.attention_bias(q, k, v, bias, gain, kv_len, P is not None, P or 0, 0.0, 0)
    out.backward(dout)
    torch.cuda.synchronize()
    assert lse.shape == (B, H, T) and packed.shape == (H, _pad32(T), _pad32(S)) and not packed.requires_grad
    errs = {"out": _rel(out, o_ref), "dq": _rel(q.grad, qf.grad), "dk": _rel(k.grad, kf.grad), "dv": _rel(v.grad, vf.grad)}
    if gain is not None:
        errs["dgain"] = _rel(gain.grad, gf.grad)
        assert gf.grad[0].abs().item() > 0 and torch.isfinite(gain.grad).all()
    if bias is not None:
        assert bias.grad.dtype == bias.dtype and bias.grad.shape == bias.shape
        fin = torch.isfinite(bias.detach())
        errs["dbias"] = _rel(bias.grad[fin], bf_.grad[fin])
        exact0 = bias.grad[~fin].abs().max().item() if (~fin).any() else 0.0
        print(case, "dbias at -inf entries: max |.| =", exact0, "(%d entries)" % int((~fin).sum()))
        assert exact0 == 0.0
    print(case, {k_: round(v_, 5) for k_, v_ in errs.items()})
    assert all(torch.isfinite(t).all() for t in (out, q.grad, k.grad, v.grad))
    bound = {"out": 1e-2, "dq": 2e-2, "dk": 2e-2, "dv": 2e-2, "dgain": 2e-2, "dbias": 3e-2}
    for k_, v_ in errs.items():
        assert v_ < bound[k_], (k_, v_)
    if pad:
        for b, n in enumerate(lens):
            if n < S:
                assert k.grad[b, n:].abs().max().item() == 0.0 and v.grad[b, n:].abs().max().item() == 0.0


# ------------------------------------------------------------------------------------------------- 4. same kernels, same bits
def _bi_inputs(dev, B, H, gh, gw, Lt, seed=3):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).to(dev).to(BF)
    P = gh * gw
    T, C = P + Lt, H * 64
    q, k, v = (r(B, T, C, sc=s_) for s_ in (0.35, 1.0, 1.0))
    pq, pk = r(T, C, sc=0.35), r(T, C)
    gain = (1.0 + 0.2 * torch.randn(H, generator=g)).to(dev)
    gcode, code_bias, n2d = _grid_codes(gh, gw)
    tabs = [torch.randn(H, n, generator=g).to(dev) for n in (n2d, 2 * Lt - 1, 2)]
    go = r(B, T, C)
    return P, T, C, q, k, v, pq, pk, gain, gcode.to(dev), code_bias, tabs, go


def test_both_ops_run_the_same_kernels_bit_for_bit():
    from ifseg_amd import hip
    dev = _dev()
    B, H, gh, gw, Lt = 8, 2, 32, 32, 37
    P, T, C, q, k, v, pq, pk, gain, gcode, code_bias, tabs, go = _bi_inputs(dev, B, H, gh, gw, Lt)
    rel = hip.RelBias(P, gcode, code_bias, tabs[0], tabs[1], tabs[2], grid_w=gw)
    dense = hip.DenseBias(H, T, T, dev)
    hip.attn_dense_bias(dense, pq, pk, rel=rel, causal=False, P=P)
    bias = dense.D[:, :T, :T].clone()            # bf16: packing it loses nothing
    # ---- direct calls on that operand
    out_d, lse_d = torch.empty(B, T, C, dtype=BF, device=dev), torch.empty(B, H, T, device=dev)
    hip.attn_fwd_bi(q, k, v, dense, out_d, lse_d, B, H, T, T, gain=gain)
    delta = torch.empty(B, H, T, device=dev)
    dq_d, dk_d, dv_d = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    hip.attn_bwd(q, k, v, None, None, out_d, go, lse_d, delta, dq_d, dk_d, dv_d, None, None, B, H, T, T, phases=hip.ATTN_BWD_DELTA)
    slabs = torch.zeros((B + 3) // 4, H, T, dense.Sp, dtype=BF, device=dev)
    hip.attn_bwd_bi(q, k, v, go, lse_d, delta, dense, dq_d, dk_d, dv_d, slabs, B, H, T, T, gain=gain)
    # ---- the two ops
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    bl = bias.clone().requires_grad_(True)
    o1, l1, p1 = torch.ops.ifseg.attention_bias(*leaves, bl, gain, None, False, 0, 0.0, 0)
    g1 = torch.autograd.grad(o1, leaves + [bl], go, retain_graph=True)
    g1b = torch.autograd.grad(o1, leaves + [bl], go)
    leaves2 = [t.clone().requires_grad_(True) for t in (q, k, v)]
    extra = [t.clone().requires_grad_(True) for t in (pq, pk, gain, *tabs)]
    o2, l2, p2 = torch.ops.ifseg.bias_attention_bi(*leaves2, extra[0], extra[1], extra[2], gcode, extra[3], extra[4], extra[5], P,
                                                   code_bias, gw, False, None, 0.0, 0)
    g2 = torch.autograd.grad(o2, leaves2 + extra, go, retain_graph=True)
    g2b = torch.autograd.grad(o2, leaves2 + extra, go)
    torch.cuda.synchronize()
    assert torch.equal(p1.view(torch.int16), dense.D.view(torch.int16)) and torch.equal(p2.view(torch.int16), dense.D.view(torch.int16))
    assert torch.equal(o1, o2) and torch.equal(l1, l2) and torch.equal(o1, out_d) and torch.equal(l1, lse_d)
    for a_, b_, c_ in zip(g1[:3], g2[:3], (dq_d, dk_d, dv_d)):
        assert torch.equal(a_, c_) and torch.equal(b_, c_)
    # dbias of attention_bias == the slab sum of the direct launch
    acc = slabs[0].float()
    for g in range(1, slabs.shape[0]):
        acc += slabs[g].float()
    assert torch.equal(g1[3], acc[:, :, :T].to(BF))
    # two backward runs of each op: fixed order, no atomics
    for a_, b_ in zip(g1 + g2, g1b + g2b):
        assert torch.equal(a_, b_)


# ------------------------------------------------------------------------------------------------- 5. bias_attention_bi
@pytest.mark.parametrize("case", ["enc_16x40", "dec_causal_32x32"])
def test_bias_attention_bi_against_fp32_autograd_and_the_old_op(case):
    dev = _dev()
    causal = case.startswith("dec")
    B, H = 2, 2
    gh, gw, Lt = (16, 40, 37) if not causal else (32, 32, 1)
    P, T, C, q, k, v, pq, pk, gain, gcode, code_bias, tabs, go = _bi_inputs(dev, B, H, gh, gw, Lt)
    ts = [t.requires_grad_(True) for t in (q, k, v, pq, pk, gain)]
    tabs = [t.requires_grad_(True) for t in tabs]
    out, lse, packed = torch.ops.ifseg.bias_attention_bi(q, k, v, pq, pk, gain, gcode, tabs[0], tabs[1], tabs[2], P, code_bias, gw,
                                                         causal, None, 0.0, 0)
    out.backward(go)
    with torch.no_grad():
        out_old, _ = torch.ops.ifseg.bias_attention(q, k, v, pq, pk, gain, gcode, tabs[0], tabs[1], tabs[2], P, code_bias, gw, causal)
    qf, kf, vf, pqf, pkf, gf = (t.detach().float().requires_grad_(True) for t in ts)
    tl = [t.detach().clone().requires_grad_(True) for t in tabs]
    bias = _dense_rel_ad(H, T, T, P, gcode.long(), code_bias, *tl)
    bias = bias + pqf.view(T, H, 64).transpose(0, 1) @ pkf.view(T, H, 64).permute(1, 2, 0)
    mask = _causal_mask(T, T, P).to(dev) if causal else None
    o_ref = _attn_ref(qf, kf, vf, bias, gf, mask)
    o_ref.backward(go.float())
    torch.cuda.synchronize()
    e_out, e_old = _rel(out, o_ref), _rel(out, out_old)
    print(case, "out vs fp32 %.5f, vs bias_attention %.5f" % (e_out, e_old))
    assert e_out < 1e-2 and e_old < 1e-2
    for name, a_, b_ in (("dq", q.grad, qf.grad), ("dk", k.grad, kf.grad), ("dv", v.grad, vf.grad), ("dpq", pq.grad, pqf.grad),
                         ("dpk", pk.grad, pkf.grad), ("dgain", gain.grad, gf.grad)):
        print(case, name, round(_rel(a_, b_), 5))
        assert _rel(a_, b_) < 3e-2, (name, _rel(a_, b_))
    scale = max(t.grad.abs().max().item() for t in tl)
    for name, a_, b_ in zip(("drel2d", "drel1d", "drelx"), tabs, tl):
        e = ((a_.grad - b_.grad).abs().max() / scale).item()
        print(case, name, round(e, 5))
        assert e < 3e-2, name


# ------------------------------------------------------------------------------------------------- 6. dropout and key padding
@pytest.mark.parametrize("which", ["attention_bias", "bias_attention_bi"])
def test_dropout_and_key_padding_through_the_ops(which):
    from ifseg_amd import hip
    dev = _dev()
    B, H, gh, gw, Lt = 5, 2, 8, 16, 36
    p, seed = 0.2, 0x1234567890ABCDEF
    P, T, C, q, k, v, pq, pk, gain, gcode, code_bias, tabs, go = _bi_inputs(dev, B, H, gh, gw, Lt, seed=9)
    S = T
    lens = [S] + [S - (1 + (13 * i) % 40) for i in range(1, B)]
    kv_len = torch.tensor(lens, dtype=torch.int32, device=dev)
    kmask = (torch.arange(S, device=dev)[None, :] >= kv_len[:, None].long())[:, None, None, :]
    keep = hip.attn_dropout_mask(B, H, T, S, p, seed, dev)
    rate = keep.float().mean().item()
    assert abs(rate - (1 - p)) < 5e-3 and not torch.equal(keep, hip.attn_dropout_mask(B, H, T, S, p, seed + 1, dev)), rate
    km = keep.float() / (1 - p)
    with torch.no_grad():
        bias_full = _dense_rel_ad(H, T, S, P, gcode.long(), code_bias, *tabs) \
            + pq.float().view(T, H, 64).transpose(0, 1) @ pk.float().view(S, H, 64).permute(1, 2, 0)
    for t in (q, k, v):
        t.requires_grad_(True)
    qf, kf, vf = (t.detach().float().requires_grad_(True) for t in (q, k, v))
    if which == "attention_bias":
        bias = bias_full.clone().requires_grad_(True)
        bfl = bias_full.clone().requires_grad_(True)
        # a per-update seed word set by somebody else must not leak into the op: the seed is used as given
        word = torch.full((1,), 12345, dtype=torch.int64, device=dev)
        prev = hip.set_seed_add(word)
        try:
            out, lse, _ = torch.ops.ifseg.attention_bias(q, k, v, bias, gain, kv_len, False, 0, p, seed)
            out.backward(go)
            assert hip._seed_add[0] is word
        finally:
            hip.set_seed_add(prev)
        out0 = torch.ops.ifseg.attention_bias(q, k, v, bias, gain, kv_len, False, 0, 0.0, seed)[0]
    else:
        bfl = bias_full
        out, lse, _ = torch.ops.ifseg.bias_attention_bi(q, k, v, pq, pk, gain, gcode, tabs[0], tabs[1], tabs[2], P, code_bias, gw,
                                                        False, kv_len, p, seed)
        out.backward(go)
        out0 = torch.ops.ifseg.bias_attention_bi(q, k, v, pq, pk, gain, gcode, tabs[0], tabs[1], tabs[2], P, code_bias, gw,
                                                 False, kv_len, 0.0, seed)[0]
    o_ref = _attn_ref(qf, kf, vf, bfl, gain, kmask, km)
    o_ref.backward(go.float())
    torch.cuda.synchronize()
    errs = {"out": _rel(out, o_ref), "dq": _rel(q.grad, qf.grad), "dk": _rel(k.grad, kf.grad), "dv": _rel(v.grad, vf.grad)}
    if which == "attention_bias":
        errs["dbias"] = _rel(bias.grad, bfl.grad)
    print(which, "keep %.4f" % rate, lens, {k_: round(v_, 5) for k_, v_ in errs.items()})
    assert not torch.equal(out, out0)
    bound = {"out": 1e-2, "dq": 2e-2, "dk": 2e-2, "dv": 2e-2, "dbias": 3e-2}
    for k_, v_ in errs.items():
        assert v_ < bound[k_], (k_, v_)
    for b in range(1, B):
        assert k.grad[b, lens[b]:].abs().max().item() == 0.0 and v.grad[b, lens[b]:].abs().max().item() == 0.0


# ------------------------------------------------------------------------------------------------- 7. seg_loss
@pytest.mark.parametrize("nseg,B,hp,wp,eps", [(15, 2, 8, 8, 0.0), (150, 1, 4, 6, 0.0), (5, 2, 32, 32, 0.0),
                                                (15, 2, 8, 8, 0.1), (171, 1, 4, 6, 0.2), (300, 1, 3, 4, 0.0), (512, 1, 2, 3, 0.1)])
@pytest.mark.parametrize("layout", ["plain", "padded_view"])
def test_seg_loss_op(nseg, B, hp, wp, eps, layout):
    from ifseg_amd.criterions import SegCriterion
    dev = _dev()
    P, H, W = hp * wp, hp * 16, wp * 16
    npad = (nseg + 7) // 8 * 8
    seg0, up = 1000, 0.37
    g = torch.Generator().manual_seed(7)
    vals = (torch.randn(B, P + 1, nseg, generator=g) * 2).to(dev).to(BF)
    tgt = torch.randint(0, nseg + 1, (B, H * W), generator=g) + seg0        # includes the ignore label seg0 + nseg
    tgt = torch.cat([tgt, torch.full((B, 1), 2)], 1).to(dev)
    if layout == "plain":
        leaf = vals.clone().requires_grad_(True)
        logits = leaf
    else:
        leaf = torch.zeros(B, P + 1, npad + 8, dtype=BF, device=dev)
        leaf[:, :, :nseg] = vals
        leaf.requires_grad_(True)
        logits = leaf[:, :, :nseg]
    loss, stats, dl, bad = torch.ops.ifseg.seg_loss(logits, tgt, hp, wp, H, W, seg0, eps)
    (loss * up).backward()
    grad = leaf.grad if layout == "plain" else leaf.grad[:, :, :nseg]
    # reference
    lf = vals.float().clone().requires_grad_(True)
    scores = SegCriterion.upsample_logits(lf, hp, wp, H, W)
    mask = (tgt == 1) | (tgt == seg0 + nseg) | (tgt == 2)
    t = tgt[~mask] - seg0
    sc = scores[~mask]
    ref = F.cross_entropy(sc, t, label_smoothing=eps)
    (ref * up).backward()
    ai, ap, al, au = SegCriterion.compute_metric(sc.detach(), t)
    torch.cuda.synchronize()
    e_loss, e_grad = abs(loss.item() - ref.item()), _rel(grad, lf.grad)
    print(nseg, B, hp, wp, eps, layout, "loss %.6f vs %.6f, grad rel-L2 %.5f" % (loss.item(), ref.item(), e_grad))
    assert loss.shape == () and e_loss < 2e-4 * max(1.0, abs(ref.item())), (loss.item(), ref.item())
    assert e_grad < 6e-3, e_grad
    assert dl.shape == (B, P + 1, npad) and dl[:, :, nseg:].abs().sum() == 0 and dl[:, P].abs().sum() == 0
    if layout != "plain":
        assert leaf.grad[:, :, nseg:].abs().sum() == 0
    assert stats[1].item() == (~mask).sum().item()
    n = nseg
    assert (stats[2 + n:2 + 2 * n] - ap).abs().sum().item() <= 1e-4 * H * W * B + 2
    assert torch.equal(stats[2 + 2 * n:2 + 3 * n], al)
    assert (stats[2:2 + n] - ai).abs().sum().item() <= 1e-4 * H * W * B + 2
    assert bad.dtype == torch.int32 and bad.item() == 0
    tgt2 = tgt.clone()
    tgt2[0, 5] = seg0 + nseg + 3                   # neither a class nor pad / eos / ignore
    assert torch.ops.ifseg.seg_loss(logits.detach(), tgt2, hp, wp, H, W, seg0, eps)[3].item() != 0


# ------------------------------------------------------------------------------------------------- 8. the module against the oracle
def test_multihead_attention_module_against_the_oracle():
    from ifseg_amd.modules import MultiheadAttention
    dev = _dev()
    cfg = O.fixture_config()
    sd_all = O.procedural_state_dict(cfg)
    p = "encoder.layers.0.self_attn"
    sd = {k_: v_.clone().float().requires_grad_(True) for k_, v_ in sd_all.items() if k_.startswith(p + ".")}
    B, T, H, C = 3, 76, cfg.heads, cfg.embed_dim
    x = _rand((B, T, C), "cpu", 40)
    bias = _inf_block_bias(H, T, T, "cpu", 41)
    lens = [T, T - 6, T - 26]
    kpm = torch.arange(T)[None, :] >= torch.tensor(lens)[:, None]
    # the upstream gradient of a MEAN over the tokens (as the criterion's loss is in test_model_gpu): the absolute bound on the
    # key-bias gradient below is meant on that scale
    go = (_rand((B, T, C), "cpu", 42).float() / (B * T)).to(BF)
    # ---- oracle, fp32 on the CPU
    xo, bo = x.float().requires_grad_(True), bias.clone().requires_grad_(True)
    yo = O.mha(sd, p, cfg, xo, xo, bo, False, kpm)
    yo.backward(go.float())
    # ---- module
    m = MultiheadAttention(C, H, scale_factor=cfg.attn_scale_factor)
    m.load_state_dict({k_[len(p) + 1:]: v_.detach() for k_, v_ in sd.items()})
    m = m.to(dev, BF).train()
    xg, bg = x.to(dev).requires_grad_(True), bias.to(dev).requires_grad_(True)
    y = m(xg, attn_bias=bg, key_padding_mask=kpm.to(dev))
    y.backward(go.to(dev))
    torch.cuda.synchronize()
    e_out = _rel(y.cpu(), yo)
    print("module: out rel-L2 %.5f" % e_out)
    assert y.shape == (B, T, C) and y.dtype == BF and e_out <= 2e-2
    fin = torch.isfinite(bias)
    errs = {"x": _rel(xg.grad.cpu(), xo.grad), "bias": _rel(bg.grad.cpu()[fin], bo.grad[fin])}
    assert bg.grad.cpu()[~fin].abs().max().item() == 0.0
    named = dict(m.named_parameters())
    for k_, v_ in sd.items():
        name = k_[len(p) + 1:]
        hg = named[name].grad
        assert hg is not None, name
        if name == "k_proj.bias":
            # key biases shift every score of a query equally: zero gradient in exact arithmetic -- only check it is tiny
            print("module: |d k_proj.bias| = %.6f (|d q_proj.bias| = %.6f)" % (hg.float().norm().item(), named["q_proj.bias"].grad.float().norm().item()))
            assert hg.float().norm().item() < 2e-2
            continue
        errs[name] = _rel(hg.cpu(), v_.grad)
    print("module:", {k_: round(v_, 5) for k_, v_ in errs.items()})
    assert len(errs) == 2 + 8
    for k_, v_ in errs.items():
        assert v_ <= 6e-2, (k_, v_)
    # a mask that is not a suffix of the keys is refused
    bad = kpm.clone()
    bad[1, 3] = True
    with pytest.raises(ValueError, match="suffix"):
        m(xg, key_padding_mask=bad.to(dev))
    # dropout only while training
    m.eval()
    with torch.no_grad():
        assert torch.equal(m(xg, attn_bias=bg, key_padding_mask=kpm.to(dev), dropout_p=0.5, seed=3), y)


# ------------------------------------------------------------------------------------------------- 9. dispatcher hygiene
def test_opcheck_and_compile():
    dev = _dev()
    utils = ("test_schema", "test_autograd_registration", "test_faketensor")
    B, H, gh, gw, Lt = 2, 2, 8, 8, 12
    P, T, C, q, k, v, pq, pk, gain, gcode, code_bias, tabs, go = _bi_inputs(dev, B, H, gh, gw, Lt)
    kv_len = torch.tensor([T, T - 5], dtype=torch.int32, device=dev)
    bias = _inf_block_bias(H, T, T, dev, 26)
    rq = lambda *ts: [t.clone().requires_grad_(True) for t in ts]
    torch.library.opcheck(torch.ops.ifseg.attention_bias, tuple(rq(q, k, v, bias, gain)) + (kv_len, False, 0, 0.1, 7), test_utils=utils)
    torch.library.opcheck(torch.ops.ifseg.attention_bias, tuple(rq(q, k, v)) + (None, None, None, True, 64, 0.0, 0), test_utils=utils)
    a = rq(q, k, v, pq, pk, gain)
    t3 = rq(*tabs)
    torch.library.opcheck(torch.ops.ifseg.bias_attention_bi,
                          tuple(a) + (gcode, t3[0], t3[1], t3[2], P, code_bias, gw, True, kv_len, 0.1, 7), test_utils=utils)
    hp, wp, nseg = 2, 3, 15
    lg = _rand((1, hp * wp + 1, nseg), dev, 50).requires_grad_(True)
    tg = torch.cat([torch.randint(0, nseg + 1, (1, 32 * 48), generator=torch.Generator().manual_seed(1)) + 1000,
                    torch.full((1, 1), 2)], 1).to(dev)
    torch.library.opcheck(torch.ops.ifseg.seg_loss, (lg, tg, hp, wp, 32, 48, 1000, 0.1), test_utils=utils)

    # torch.compile (aot_eager: no code generator) of a differentiated function == eager, bit for bit
    def fn(q_, k_, v_, b_, g_):
        out = torch.ops.ifseg.attention_bias(q_, k_, v_, b_ * 0.5, g_, kv_len, False, 0, 0.1, 7)[0]
        return (out.float() * go.float()).sum()

    def run(f):
        leaves = rq(q, k, v, bias, gain)
        loss = f(*leaves)
        return [loss.detach()] + list(torch.autograd.grad(loss, leaves))

    eager = run(fn)
    compiled = run(torch.compile(fn, backend="aot_eager", fullgraph=True))
    torch.cuda.synchronize()
    for a_, b_ in zip(eager, compiled):
        assert torch.equal(a_, b_)
