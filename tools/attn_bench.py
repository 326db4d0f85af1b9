"""Micro-benchmark of the attention kernels on the encoder / decoder shapes of SegOFA-Base (B=8)."""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ifseg_amd import hip

def main(kind="enc", iters=5):
    dev = torch.device("cuda:0")
    B, H, C = 8, 12, 768
    gh = gw = 32; P = 1024
    Lt = 1 if kind in ("dec", "decfull") else 36
    if os.environ.get("ATTN_BENCH_LARGE"):      # BASELINE configs[3] geometry: 640 x 640 -> 40 x 40 grid, 16 heads, L = 239
        B, H, C = 4, 16, 1024
        gh = gw = 40; P = 1600
        Lt = 1 if kind in ("dec", "decfull") else 239
    T = S = P + Lt
    causal = kind == "dec"
    g = torch.Generator().manual_seed(0)
    r = lambda *s: (torch.randn(*s, generator=g) * 0.5).to(dev).to(torch.bfloat16)
    qkv = r(B, T, 3 * C); pq, pk = r(T, C), r(S, C); dout = r(B, T, C)
    ys, xs = torch.meshgrid(torch.arange(gh), torch.arange(gw), indexing="ij")
    gcode = (ys * (2 * gw - 1) + xs).reshape(-1).int().to(dev)
    n2d = (2 * gh - 1) * (2 * gw - 1)
    rel = hip.RelBias(P, gcode, (gh - 1) * (2 * gw - 1) + gw - 1, torch.randn(H, n2d, generator=g).to(dev),
                      torch.randn(H, 2 * Lt - 1, generator=g).to(dev), torch.randn(H, 2, generator=g).to(dev), grid_w=gw)
    if kind == "cross":
        rel = None
    gain = torch.ones(H, device=dev, dtype=torch.bfloat16)
    out = torch.zeros(B, T, C, dtype=torch.bfloat16, device=dev); lse = torch.zeros(B, H, T, device=dev)
    dqkv = torch.zeros_like(qkv); delta = torch.zeros(B, H, T, device=dev)
    dpq = torch.zeros(B, T, C, device=dev, dtype=torch.bfloat16); dpk = torch.zeros(B, S, C, device=dev, dtype=torch.bfloat16)
    nparts = B * ((S + 127) // 128)
    parts = [torch.zeros(H, nparts, n, device=dev) for n in (n2d, 2 * Lt - 1, 2)] if rel is not None else [None] * 3
    q, k, v = qkv[:, :, :C], qkv[:, :, C:2 * C], qkv[:, :, 2 * C:]
    def step():
        hip.attn_fwd(q, k, v, pq, pk, out, lse, B, H, T, S, rel=rel, causal=causal, gain=gain)
        hip.attn_bwd(q, k, v, pq, pk, out, dout, lse, delta, dqkv[:, :, :C], dqkv[:, :, C:2 * C], dqkv[:, :, 2 * C:], dpq, dpk,
                     B, H, T, S, rel=rel, causal=causal, gain=gain, drel2d_part=parts[0], drel1d_part=parts[1],
                     drelx_part=parts[2], nparts=nparts)
    step(); torch.cuda.synchronize()
    hip.prof_reset(); hip.prof_enable(0x70)
    t0 = time.time()
    for _ in range(iters): step()
    torch.cuda.synchronize()
    for kd in (4, 5, 6):
        p = hip.prof_read(kd)
        print(kind, p["kind"], "avg us %.1f" % (p["ms"] * 1e3 / max(1, p["launches"])), "alg TF/s %.1f" % (p["flops"] / max(1e-9, p["ms"] * 1e-3) / 1e12))
    hip.prof_enable(0)
    def bwd(phases):
        hip.attn_bwd(q, k, v, pq, pk, out, dout, lse, delta, dqkv[:, :, :C], dqkv[:, :, C:2 * C], dqkv[:, :, 2 * C:], dpq, dpk,
                     B, H, T, S, rel=rel, causal=causal, gain=gain, drel2d_part=parts[0], drel1d_part=parts[1],
                     drelx_part=parts[2], nparts=nparts, phases=phases)
    def timeit(fn, n=10):
        fn(); torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n): fn()
        e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n
    print(kind, "dkv alone            us %.1f" % timeit(lambda: bwd(hip.ATTN_BWD_DKV)))
    print(kind, "dq kernel alone      us %.1f" % timeit(lambda: bwd(hip.ATTN_BWD_DQ)))


HBM_PEAK_TBS, HBM_MEASURED_TBS = 8.0, 6.29      # HBM3E: spec / measured float4 copy


def ops_ab(out_path=None, window_s=1.0, rounds=3):
    """`python tools/attn_bench.py ops [file]`: forward + backward through the dispatcher against the direct calls, and the two
    kernels of csrc/attention_ops.hip alone.  Variants alternate inside every round; each timing is a device-event window of
    about `window_s` seconds (repetitions sized from a first probe); the table holds the median over the rounds and the spread."""
    import ifseg_amd.ops  # noqa: F401
    dev = torch.device("cuda:0")
    BF = torch.bfloat16
    lines = []

    def say(*a):
        line = " ".join(str(x) for x in a)
        print(line, flush=True)
        lines.append(line)

    def window(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / n          # us per call

    def ab(variants):
        reps = {}
        for name, fn in variants:                     # warm up every variant, then size its window
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            reps[name] = max(3, int(window_s * 1e6 / max(window(fn, 3), 1.0)))
        res = {name: [] for name, _ in variants}
        for _ in range(rounds):
            for name, fn in variants:
                res[name].append(window(fn, reps[name]))
        return {name: (sorted(v)[len(v) // 2], min(v), max(v), reps[name]) for name, v in res.items()}

    say("# torch.ops.ifseg attention ops, forward + backward, MI355X; us per call: median of %d alternating windows of ~%.1f s [min .. max]" % (rounds, window_s))
    for label, B, H, gh, gw, Lt in (("Base  B=8 H=12 32x32+36 T=S=1060", 8, 12, 32, 32, 36), ("Large B=8 H=16 40x40+36 T=S=1636", 8, 16, 40, 40, 36)):
        P, C = gh * gw, H * 64
        T = S = P + Lt
        g = torch.Generator().manual_seed(0)
        r = lambda *s: (torch.randn(*s, generator=g) * 0.5).to(dev).to(BF)
        qkv = r(B, T, 3 * C).requires_grad_(True)
        pq, pk, dout = r(T, C).requires_grad_(True), r(S, C).requires_grad_(True), r(B, T, C)
        ys, xs = torch.meshgrid(torch.arange(gh), torch.arange(gw), indexing="ij")
        gcode = (ys * (2 * gw - 1) + xs).reshape(-1).int().to(dev)
        n2d, code_bias = (2 * gh - 1) * (2 * gw - 1), (gh - 1) * (2 * gw - 1) + gw - 1
        tabs = [torch.randn(H, n, generator=g).to(dev).requires_grad_(True) for n in (n2d, 2 * Lt - 1, 2)]
        gain = torch.ones(H, device=dev).requires_grad_(True)
        rel = hip.RelBias(P, gcode, code_bias, tabs[0].detach(), tabs[1].detach(), tabs[2].detach(), grid_w=gw)
        dense = hip.DenseBias(H, T, S, dev)
        hip.attn_dense_bias(dense, pq.detach(), pk.detach(), rel=rel, P=P)
        bias32 = dense.D[:, :T, :S].float().requires_grad_(True)         # "the ready fp32 bias"
        leaves = [qkv, pq, pk, gain, bias32] + tabs
        split = lambda: (qkv[:, :, :C], qkv[:, :, C:2 * C], qkv[:, :, 2 * C:])

        def fb(out):
            for t in leaves:
                t.grad = None
            out.backward(dout)

        def v_old():
            q, k, v = split()
            fb(torch.ops.ifseg.bias_attention(q, k, v, pq, pk, gain, gcode, tabs[0], tabs[1], tabs[2], P, code_bias, gw, False)[0])

        def v_bi():
            q, k, v = split()
            fb(torch.ops.ifseg.bias_attention_bi(q, k, v, pq, pk, gain, gcode, tabs[0], tabs[1], tabs[2], P, code_bias, gw, False,
                                                 None, 0.0, 0)[0])

        def v_ab():
            q, k, v = split()
            fb(torch.ops.ifseg.attention_bias(q, k, v, bias32, gain, None, False, 0, 0.0, 0)[0])

        qd = qkv.detach()
        q_, k_, v_ = qd[:, :, :C], qd[:, :, C:2 * C], qd[:, :, 2 * C:]
        out, lse, delta = torch.empty(B, T, C, dtype=BF, device=dev), torch.empty(B, H, T, device=dev), torch.empty(B, H, T, device=dev)
        dqkv = torch.empty_like(qd)
        slabs = torch.zeros((B + 3) // 4, H, T, dense.Sp, dtype=BF, device=dev)
        dgr = torch.empty(B, H, T, device=dev)
        gd = gain.detach()

        def v_direct():
            hip.attn_fwd_bi(q_, k_, v_, dense, out, lse, B, H, T, S, gain=gd)
            hip.attn_bwd(q_, k_, v_, None, None, out, dout, lse, delta, dqkv[:, :, :C], dqkv[:, :, C:2 * C], dqkv[:, :, 2 * C:], None, None,
                         B, H, T, S, phases=hip.ATTN_BWD_DELTA)
            hip.attn_bwd_bi(q_, k_, v_, dout, lse, delta, dense, dqkv[:, :, :C], dqkv[:, :, C:2 * C], dqkv[:, :, 2 * C:], slabs, B, H, T, S,
                            gain=gd, dgain_rows=dgr)

        res = ab([("(i)   ops.bias_attention (round-3 kernels)", v_old), ("(ii)  ops.bias_attention_bi", v_bi),
                  ("(iii) ops.attention_bias, ready fp32 bias", v_ab), ("(iv)  hip.attn_fwd_bi + delta + attn_bwd_bi, direct", v_direct)])
        say("\n" + label)
        for name, (med, lo, hi, n) in res.items():
            say("  %-52s %9.1f  [%9.1f .. %9.1f]  x%d" % (name, med, lo, hi, n))
        # ---- the two kernels alone, with the bytes they move
        bias_f, bias_b = bias32.detach(), dense.D[:, :T, :S].contiguous()
        d2 = hip.DenseBias(H, T, S, dev)
        o32, o16 = torch.empty(H, T, S, device=dev), torch.empty(H, T, S, dtype=BF, device=dev)
        ng = slabs.shape[0]
        wr = H * dense.Tp * dense.Sp * 2
        kern = [("attn_bias_pack fp32 -> bf16", lambda: hip.attn_bias_pack(d2, bias_f), H * T * S * 4 + wr),
                ("attn_bias_pack bf16 -> bf16", lambda: hip.attn_bias_pack(d2, bias_b), H * T * S * 2 + wr),
                ("attn_dbias_sum %d slabs -> fp32" % ng, lambda: hip.attn_dbias_sum(slabs, S, o32), ng * H * T * ((S + 7) // 8 * 8) * 2 + H * T * S * 4),
                ("attn_dbias_sum %d slabs -> bf16" % ng, lambda: hip.attn_dbias_sum(slabs, S, o16), ng * H * T * ((S + 7) // 8 * 8) * 2 + H * T * S * 2)]
        res = ab([(n_, f_) for n_, f_, _ in kern])
        for n_, _, nbytes in kern:
            med, lo, hi, n = res[n_]
            gbs = nbytes / med * 1e-3
            say("  %-52s %9.1f  [%9.1f .. %9.1f]  x%d  %.1f MB  %.0f GB/s = %.0f %% of %.1f TB/s peak (%.0f %% of the %.2f TB/s a copy reaches)"
                % (n_, med, lo, hi, n, nbytes / 1e6, gbs, gbs / (HBM_PEAK_TBS * 10), HBM_PEAK_TBS, gbs / (HBM_MEASURED_TBS * 10), HBM_MEASURED_TBS))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "ops":
        ops_ab(sys.argv[2] if len(sys.argv) > 2 else None)
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else "enc")
