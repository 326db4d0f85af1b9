"""CPU: the dispatcher surface of the training-path ops (ifseg_amd/ops.py: attention_bias, bias_attention_bi, seg_loss and
their backward ops) -- schemas, fake (meta) implementations under FakeTensorMode, the refusals by name -- and the state-dict
contract of ifseg_amd.modules.MultiheadAttention.  No kernel is launched and the library is not loaded."""
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import segofa_ref as O

BF, F32 = torch.bfloat16, torch.float32
NEW_OPS = ("attention_bias", "attention_bias_bwd", "bias_attention_bi", "bias_attention_bi_bwd", "seg_loss", "seg_loss_bwd")


def _ops():
    import ifseg_amd.ops  # noqa: F401
    return torch.ops.ifseg


def _meta(t):
    return tuple(t.shape), t.dtype


def test_the_six_new_ops_are_registered_with_their_schemas():
    ops = _ops()
    for n in NEW_OPS:
        assert hasattr(ops, n), n
    s = {n: str(getattr(ops, n).default._schema) for n in NEW_OPS}
    assert s["attention_bias"] == ("ifseg::attention_bias(Tensor q, Tensor k, Tensor v, Tensor? bias, Tensor? gain, Tensor? kv_len, "
                                   "bool causal, SymInt P, float dropout_p, SymInt seed) -> (Tensor, Tensor, Tensor)")
    assert s["attention_bias_bwd"] == ("ifseg::attention_bias_bwd(Tensor dout, Tensor q, Tensor k, Tensor v, Tensor? bias, Tensor? gain, "
                                       "Tensor? kv_len, Tensor out, Tensor lse, Tensor packed, bool causal, SymInt P, float dropout_p, "
                                       "SymInt seed) -> (Tensor, Tensor, Tensor, Tensor, Tensor)")
    assert s["bias_attention_bi"] == ("ifseg::bias_attention_bi(Tensor q, Tensor k, Tensor v, Tensor pos_q, Tensor pos_k, Tensor gain, "
                                      "Tensor? gcode, Tensor? rel2d, Tensor? rel1d, Tensor? relx, SymInt P, SymInt code_bias, "
                                      "SymInt grid_w, bool causal, Tensor? kv_len, float dropout_p, SymInt seed) -> (Tensor, Tensor, Tensor)")
    assert s["bias_attention_bi_bwd"].startswith("ifseg::bias_attention_bi_bwd(Tensor dout, Tensor q, Tensor k, Tensor v, Tensor pos_q, "
                                                 "Tensor pos_k, Tensor gain, Tensor out, Tensor lse, Tensor packed, Tensor? gcode,")
    assert s["bias_attention_bi_bwd"].endswith("-> (Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor, Tensor)")
    assert s["seg_loss"] == ("ifseg::seg_loss(Tensor logits, Tensor target, SymInt hp, SymInt wp, SymInt H, SymInt W, "
                             "SymInt seg_id_offset, float label_smoothing) -> (Tensor, Tensor, Tensor, Tensor)")
    assert s["seg_loss_bwd"] == "ifseg::seg_loss_bwd(Tensor grad_loss, Tensor dlogits, SymInt nseg) -> Tensor"
    # functional: nothing is mutated, nothing aliases
    for n in NEW_OPS:
        assert "!" not in s[n] and "(a" not in s[n], s[n]


def _e(*shape, dtype=BF):
    return torch.empty(*shape, dtype=dtype, device="cuda")


# (B, H, T, S, causal, P): self, cross (T != S), causal decoder layout
GEOMS = {"self": (3, 2, 76, 76, False, 0), "cross": (2, 3, 65, 100, False, 0), "causal": (5, 2, 65, 65, True, 64)}


@pytest.mark.parametrize("case", sorted(GEOMS))
@pytest.mark.parametrize("optional", [False, True])
@pytest.mark.parametrize("bias_dtype", [F32, BF])
def test_attention_bias_fake_shapes(case, optional, bias_dtype):
    ops = _ops()
    B, H, T, S, causal, P = GEOMS[case]
    C, Tp, Sp = H * 64, (T + 31) // 32 * 32, (S + 31) // 32 * 32
    with FakeTensorMode():
        q, k, v = _e(B, T, C), _e(B, S, C), _e(B, S, C)
        bias = _e(H, T, S, dtype=bias_dtype) if optional else None
        gain = _e(H, dtype=F32) if optional else None
        kv_len = _e(B, dtype=torch.int32) if optional else None
        p = 0.2 if optional else 0.0
        out, lse, packed = ops.attention_bias(q, k, v, bias, gain, kv_len, causal, P, p, 11)
        assert out.device.type == "cuda"
        assert _meta(out) == ((B, T, C), BF) and _meta(lse) == ((B, H, T), F32) and _meta(packed) == ((H, Tp, Sp), BF)
        dq, dk, dv, dbias, dgain = ops.attention_bias_bwd(_e(B, T, C), q, k, v, bias, gain, kv_len, out, lse, packed, causal, P, p, 11)
        assert _meta(dq) == ((B, T, C), BF) and _meta(dk) == ((B, S, C), BF) and _meta(dv) == ((B, S, C), BF)
        assert _meta(dbias) == (((H, T, S), bias_dtype) if optional else ((0,), F32))
        assert _meta(dgain) == ((H,), F32)
        # slices of a fused QKV projection are row-strided views
        qkv = _e(B, T, 3 * C)
        if T == S:
            out2, _, _ = ops.attention_bias(qkv[:, :, :C], qkv[:, :, C:2 * C], qkv[:, :, 2 * C:], bias, gain, kv_len, causal, P, p, 11)
            assert _meta(out2) == ((B, T, C), BF) and out2.is_contiguous()


def _bi_args(B, H, T, S, causal, P, grid_w, rel, optional):
    C = H * 64
    q, k, v = _e(B, T, C), _e(B, S, C), _e(B, S, C)
    pq, pk, gain = _e(T, C), _e(S, C), _e(H, dtype=F32)
    tabs = [None] * 4
    if rel:
        gh = P // grid_w
        tabs = [_e(P, dtype=torch.int32), _e(H, (2 * gh - 1) * (2 * grid_w - 1), dtype=F32), _e(H, 2 * (T - P) - 1, dtype=F32),
                _e(H, 2, dtype=F32)]
    kv_len = _e(B, dtype=torch.int32) if optional else None
    return [q, k, v, pq, pk, gain] + tabs + [P, 7, grid_w, causal, kv_len, 0.1 if optional else 0.0, 5]


@pytest.mark.parametrize("case,rel", [("self", True), ("self", False), ("cross", False), ("causal", True), ("causal", False)])
@pytest.mark.parametrize("optional", [False, True])
def test_bias_attention_bi_fake_shapes(case, rel, optional):
    ops = _ops()
    B, H, T, S, causal, P = GEOMS[case]
    if case == "self":
        P = 64
    C, Tp, Sp = H * 64, (T + 31) // 32 * 32, (S + 31) // 32 * 32
    with FakeTensorMode():
        a = _bi_args(B, H, T, S, causal, P, 8, rel, optional)
        out, lse, packed = ops.bias_attention_bi(*a)
        assert _meta(out) == ((B, T, C), BF) and _meta(lse) == ((B, H, T), F32) and _meta(packed) == ((H, Tp, Sp), BF)
        g = ops.bias_attention_bi_bwd(_e(B, T, C), *a[:6], out, lse, packed, *a[6:])
        assert len(g) == 9
        assert [_meta(t) for t in g[:6]] == [((B, T, C), BF), ((B, S, C), BF), ((B, S, C), BF), ((T, C), BF), ((S, C), BF), ((H,), F32)]
        for t, src in zip(g[6:], a[7:10]):
            assert _meta(t) == (_meta(src) if rel else ((0,), F32))


@pytest.mark.parametrize("nseg,B,hp,wp", [(15, 2, 8, 8), (150, 1, 4, 6), (512, 1, 2, 3), (16, 2, 2, 2)])
def test_seg_loss_fake_shapes(nseg, B, hp, wp):
    ops = _ops()
    H, W, npad = 16 * hp, 16 * wp, (nseg + 7) // 8 * 8
    with FakeTensorMode():
        logits = _e(B, hp * wp + 1, nseg)
        target = _e(B, H * W + 1, dtype=torch.int64)
        loss, stats, dl, bad = ops.seg_loss(logits, target, hp, wp, H, W, 1000, 0.1)
        assert _meta(loss) == ((), F32) and _meta(stats) == ((2 + 3 * nseg,), F32)
        assert _meta(dl) == ((B, hp * wp + 1, npad), BF) and _meta(bad) == ((1,), torch.int32)
        # a row-strided view into a padded buffer
        view = _e(B, hp * wp + 1, npad + 8)[:, :, :nseg]
        assert _meta(ops.seg_loss(view, target, hp, wp, H, W, 1000, 0.0)[2]) == ((B, hp * wp + 1, npad), BF)
        g = ops.seg_loss_bwd(_e((), dtype=F32), dl, nseg)
        assert _meta(g) == ((B, hp * wp + 1, nseg), BF)


def _refuses(match, fn, *args):
    with pytest.raises((RuntimeError, ValueError), match=match):
        fn(*args)


def test_refusals_by_name_fire_before_the_library_is_touched(monkeypatch):
    ops = _ops()
    from ifseg_amd import hip

    def no_lib():
        raise AssertionError("hip.lib() touched before the arguments were checked")
    monkeypatch.setattr(hip, "lib", no_lib)
    with FakeTensorMode():
        B, H, T, S = 2, 2, 65, 65
        C = H * 64
        q, k, v = _e(B, T, C), _e(B, S, C), _e(B, S, C)
        ab = ops.attention_bias
        ok = [q, k, v, None, None, None, False, 0, 0.0, 0]

        def with_(**kw):
            names = ["q", "k", "v", "bias", "gain", "kv_len", "causal", "P", "dropout_p", "seed"]
            a = list(ok)
            for n, val in kw.items():
                a[names.index(n)] = val
            return a
        _refuses("head dimension of 64", ab, *with_(q=_e(B, T, 80), k=_e(B, S, 80), v=_e(B, S, 80)))
        _refuses("contiguous last dimension", ab, *with_(q=_e(B, T, 2 * C)[:, :, ::2]))
        _refuses("contiguous last dimension", ab, *with_(bias=_e(H, T, 2 * S, dtype=F32)[:, :, ::2]))
        _refuses(r"P %% 64|P \(grid tokens\)", ab, *with_(causal=True, P=32))
        _refuses(r"P \(grid tokens\)", ab, *with_(causal=True, P=128))
        _refuses("kv_len must be int32", ab, *with_(kv_len=_e(B, dtype=torch.int64)))
        _refuses("kv_len must be int32", ab, *with_(kv_len=_e(B + 1, dtype=torch.int32)))
        _refuses(r"dropout_p must lie in \[0, 1\)", ab, *with_(dropout_p=1.0))
        _refuses(r"dropout_p must lie in \[0, 1\)", ab, *with_(dropout_p=-0.1))
        _refuses("gain must be fp32", ab, *with_(gain=_e(H)))
        _refuses("bias must be fp32 or bf16", ab, *with_(bias=_e(B, H, T, S, dtype=F32)))
        _refuses("bias must be fp32 or bf16", ab, *with_(bias=_e(H, T, S, dtype=torch.float16)))
        big = 32768
        _refuses(r"below 2\*\*31", ab, _e(1, big, 64), _e(1, big, 64), _e(1, big, 64), None, None, None, False, 0, 0.0, 0)
        # the backward op refuses the same things
        _refuses("head dimension of 64", ops.attention_bias_bwd, _e(B, T, 80), _e(B, T, 80), _e(B, S, 80), _e(B, S, 80), None, None,
                 None, _e(B, T, 80), _e(B, 1, T, dtype=F32), _e(1, 96, 96), False, 0, 0.0, 0)

        bi = ops.bias_attention_bi
        good = _bi_args(B, H, T, S, True, 64, 8, True, False)
        assert bi(*good)[0].shape == (B, T, C)

        def bi_with(idx, val, base=good):
            a = list(base)
            a[idx] = val
            return a
        _refuses("head dimension of 64", bi, *bi_with(0, _e(B, T, 80)))
        _refuses(r"P \(grid tokens\)", bi, *bi_with(10, 32))
        _refuses("grid_w must be a multiple of 8 and at most 64", bi, *bi_with(12, 4))
        _refuses("grid_w must be a multiple of 8 and at most 64", bi, *_bi_args(1, H, 257, 257, False, 256, 128, True, False))
        _refuses("grid_h \\* grid_w", bi, *bi_with(12, 24))
        _refuses("needs T == S", bi, *(lambda a: a[:1] + [_e(B, 100, C), _e(B, 100, C)] + a[3:4] + [_e(100, C)] + a[5:])(
            _bi_args(B, H, T, S, False, 64, 8, True, False)))
        _refuses("come together", bi, *bi_with(7, None))
        _refuses("kv_len must be int32", bi, *bi_with(14, _e(B, dtype=torch.int64)))
        _refuses(r"dropout_p must lie in \[0, 1\)", bi, *bi_with(15, 1.5))

        sl = ops.seg_loss
        hp, wp, n = 4, 6, 15
        lg, tg = _e(1, hp * wp + 1, n), _e(1, 64 * 96 + 1, dtype=torch.int64)
        assert sl(lg, tg, hp, wp, 64, 96, 1000, 0.0)[0].shape == ()
        _refuses("H == 16 \\* hp", sl, lg, tg, hp, wp, 63, 96, 1000, 0.0)
        _refuses("W == 16 \\* wp", sl, lg, _e(1, 64 * 80 + 1, dtype=torch.int64), hp, wp, 64, 80, 1000, 0.0)
        _refuses("FUSED_MAX_CLASSES", sl, _e(1, hp * wp + 1, 513), tg, hp, wp, 64, 96, 1000, 0.0)
        _refuses(r"target must be int64 \[B, H \* W \+ 1\]", sl, lg, _e(1, 64 * 96, dtype=torch.int64), hp, wp, 64, 96, 1000, 0.0)
        _refuses(r"hp \* wp \+ 1", sl, _e(1, hp * wp, n), tg, hp, wp, 64, 96, 1000, 0.0)


def test_seg_loss_class_limit_is_the_criterions():
    from ifseg_amd import ops
    from ifseg_amd.criterions.seg_criterion import FUSED_MAX_CLASSES
    assert ops.SEG_LOSS_MAX_CLASSES == FUSED_MAX_CLASSES


def test_multihead_attention_state_dict_keys_are_the_references():
    from ifseg_amd.modules import MultiheadAttention
    cfg = O.fixture_config()
    sd = O.procedural_state_dict(cfg)
    p = "encoder.layers.0.self_attn."
    want = {k[len(p):]: v for k, v in sd.items() if k.startswith(p)}
    m = MultiheadAttention(cfg.embed_dim, cfg.heads)
    have = m.state_dict()
    assert set(have) == set(want) and len(want) == 9
    for k in want:
        assert tuple(have[k].shape) == tuple(want[k].shape), k
    m.load_state_dict(want, strict=True)
    assert m.scaling == float(cfg.head_dim * cfg.attn_scale_factor) ** -0.5
    with pytest.raises(ValueError, match="head dimension of 64"):
        MultiheadAttention(160, 2)


def test_key_padding_mask_must_be_a_suffix():
    from ifseg_amd.modules import key_counts
    m = torch.zeros(3, 6, dtype=torch.bool)
    m[1, 4:] = True
    m[2, 5:] = True
    assert key_counts(m).tolist() == [6, 4, 5] and key_counts(m).dtype == torch.int32
    m[0, 2] = True
    with pytest.raises(ValueError, match="suffix"):
        key_counts(m)
    with pytest.raises(ValueError, match="suffix"):
        key_counts(torch.ones(1, 4, dtype=torch.bool))
