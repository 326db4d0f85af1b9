"""Bit-compare (and time) the LayerNorm / reduction kernels of csrc/rowops.hip between two builds of the library.

    IFSEG_LIB=<library A> python tools/rowops_bits.py save PATH     # every output of every case -> PATH
    IFSEG_LIB=<library B> python tools/rowops_bits.py cmp PATH      # one line per output: bit-equal | n differ, max |diff|
    python tools/rowops_bits.py time                                # microseconds per call at the step's shapes

Inputs are the conformance generators of tests/_rowops_cases.py (FWD_CASES, ifseg_ln_fwd_pair at LN_WIDTHS with both first
stages, BWD_CASES, BWD_DROP_CASES, REDUCE_CASES: every remaining instantiation and dispatch path), then the step's shapes with
random data: forward and backward (plain / + dx_add / + dx_add + dropout, ifseg_ln_bwd_drop beside it) at 8480 x 768, 333 x 1024,
64 x 128 and 1001 x 256, forward and backward + dx_add with GELU at 8480 x 3072, and one three-task ifseg_reduce_parts_multi
call that mixes fp32 and accumulating bf16 outputs.  `cmp` exits 1 unless everything is bit-equal.
`time` (one process per sample; the library is whatever IFSEG_LIB selects): ln_fwd with GELU at 8480 x 3072 and reduce_parts
as the step calls it -- the LayerNorm partials (ops.py: outer 2, LN_BWD_BLOCKS parts, n 768), the loss statistics
(hip.seg_loss: 8 x 32 x 32 tiles, n = 2 + 3 x 150, the tall kernel) and a bias gradient's column sums (engine._bias_grad after
hip.colsum: COLSUM_BLOCKS parts, n 768, bf16); the LayerNorm lines at 8480 x 768 are tools/ln_bench.py's."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _rowops_cases as rc  # noqa: E402
from ifseg_amd import hip  # noqa: E402

dev = torch.device("cuda:0")
BF16, F32 = torch.bfloat16, torch.float32
BIG = ((8480, 768), (333, 1024), (64, 128), (1001, 256))
outs = {}


def split(rows):
    for b in range(2, rows + 1):
        if rows % b == 0:
            return b, rows // b
    return 1, 1


def view(rows, C, strided, init=None, dtype=BF16):
    """a [B, rpb, C] device view, the batches apart (the RowMap division path) or contiguous (the collapsed map)"""
    B, rpb = split(rows)
    full = torch.zeros((B, rpb + 5, C + 8) if strided else (B, rpb, C), dtype=dtype, device=dev)
    v = full[:, 3:3 + rpb, :C] if strided else full
    if init is not None:
        v.copy_(torch.from_numpy(np.array(init, dtype=np.float32)).view(B, rpb, C).to(dev))
    return v


def vec(a, dtype):
    return torch.from_numpy(np.array(a, dtype=np.float32)).to(dev, dtype)


def keep(name, **tensors):
    torch.cuda.synchronize()
    for k, t in tensors.items():
        outs["%s %s" % (name, k)] = t.detach().cpu().contiguous()


def case_drop(case):
    if not case["drop"]:
        return None
    nb = (case["rows"] + rc.DROP_RPB - 1) // rc.DROP_RPB
    return (rc.DROP_P, rc.DROP_SEED, vec(rc.DROP_DPSCALE[:nb], F32), rc.DROP_RPB)


def case_params(d, case):
    pdt = F32 if case["pf32"] else BF16
    return vec(d["gamma"], pdt), vec(d["beta"], pdt)


def stats(rows):
    return torch.zeros(rows, dtype=F32, device=dev), torch.zeros(rows, dtype=F32, device=dev)


def run_fwd(case):
    rows, C, st = case["rows"], case["C"], case["strided"]
    d = rc.case_inputs(case)
    gamma, beta = case_params(d, case)
    y, (mean, rstd) = view(rows, C, st), stats(rows)
    hip.ln_fwd(view(rows, C, st, d["x"]), gamma, beta, y, mean, rstd, resid=view(rows, C, st, d["resid"]) if case["resid"] else None,
               gelu=case["gelu"], drop=case_drop(case))
    keep(case["id"], y=y, mean=mean, rstd=rstd)


def run_pair(C, first):
    rows = 13
    case = dict(rows=rows, C=C, drop=True, pf32=(C // 8) % 2 == 0, strided=(C // 8) % 3 != 0)
    d = rc.ln_inputs(rows, C, 8000 + C)
    pdt, key = (F32, "32") if case["pf32"] else (BF16, "16")
    g1, b1 = d["gamma" + key], d["beta" + key]
    G1, B1, G2, B2 = (vec(v, pdt) for v in (g1, b1, g1[::-1], b1[::-1]))
    st = case["strided"]
    y, y2, (m1, r1), (m2, r2) = view(rows, C, st), view(rows, C, not st), stats(rows), stats(rows)
    ident = first == "identity"
    hip.ln_fwd_pair(view(rows, C, st, d["x"]), None if ident else G1, None if ident else B1, y, None if ident else m1,
                    None if ident else r1, G2, B2, y2, m2, r2, resid=view(rows, C, st, d["resid"]), drop=case_drop(case))
    keep("pair-%s-13x%d" % (first, C), y=y, y2=y2, mean=m1, rstd=r1, mean2=m2, rstd2=r2)


def run_bwd(case, second):
    """ifseg_ln_bwd, or ifseg_ln_bwd_drop with the case's dropout as the mask of the second output"""
    rows, C, st, nb = case["rows"], case["C"], case["strided"], case["nblocks"]
    hip.LN_BWD_BLOCKS = nb
    d = rc.case_inputs(case, backward=True)
    x, dy = view(rows, C, st, d["x"]), view(rows, C, st, d["dy"])
    gamma, beta = case_params(d, case)
    add = view(rows, C, st, d["add"]) if case["add"] else None
    mean, rstd = stats(rows)
    hip.ln_fwd(x, gamma, beta, torch.empty_like(x), mean, rstd, gelu=case["gelu"])
    dx, part = view(rows, C, st), torch.zeros(2, nb, C, dtype=F32, device=dev)
    if second:
        dx2 = view(rows, C, not st)
        hip.ln_bwd_drop(dy, x, gamma, mean, rstd, dx, part[0], part[1], dx2, dx_add=add, drop2=case_drop(case))
        keep("drop-" + case["id"], dx=dx, dx2=dx2, dgamma_part=part[0], dbeta_part=part[1])
    else:
        hip.ln_bwd(dy, x, gamma, mean, rstd, dx, part[0], part[1], dx_add=add, gelu=case["gelu"], drop=case_drop(case))
        keep(case["id"], dx=dx, dgamma_part=part[0], dbeta_part=part[1])


def run_reduce(c):
    r = rc.reduce_case(c)
    out = vec(r["prev"] if c["acc"] else np.zeros_like(r["prev"]), BF16 if c["bf16"] else F32)
    hip.reduce_parts(vec(r["inp"], F32), out, c["outer"], c["parts"], c["n"], accumulate=c["acc"], scale=c["scale"])
    keep("reduce " + c["reach"] + " " + c["id"], out=out)


def run_big(gen):
    def rnd(*s):
        return torch.randn(*s, device=dev, generator=gen).bfloat16()
    hip.LN_BWD_BLOCKS = 768
    for rows, C, gelu in [(r, c, False) for r, c in BIG] + [(8480, 3072, True)]:
        x, dy, add = rnd(rows, C), rnd(rows, C), rnd(rows, C)
        gam, bet = torch.randn(C, device=dev, generator=gen), torch.randn(C, device=dev, generator=gen)
        y, (mean, rstd) = torch.empty_like(x), stats(rows)
        variants = ((add, None),) if gelu else ((None, None), (add, None), (add, (0.1, 77, None, None)))
        for ci, (a, dr) in enumerate(variants):
            name = "big %dx%d%s v%d" % (rows, C, " gelu" if gelu else "", ci)
            hip.ln_fwd(x, gam, bet, y, mean, rstd, resid=a, gelu=gelu, drop=dr)
            keep(name + " fwd", y=y, mean=mean, rstd=rstd)
            dx, part = torch.empty_like(x), torch.zeros(2, 768, C, device=dev)
            hip.ln_bwd(dy, x, gam, mean, rstd, dx, part[0], part[1], dx_add=a, gelu=gelu, drop=dr)
            keep(name + " bwd", dx=dx, part=part)
            if not gelu:
                dx2, part2 = torch.empty_like(x), torch.zeros(2, 768, C, device=dev)
                hip.ln_bwd_drop(dy, x, gam, mean, rstd, dx, part2[0], part2[1], dx2, dx_add=a, drop2=dr)
                keep(name + " bwd_drop", dx=dx, dx2=dx2, part=part2)
    # three reductions in one launch: fp32, accumulating bf16 (n no multiple of 32), fp32 with one column
    ins = [torch.randn(o, p, n, device=dev, generator=gen) for o, p, n in ((2, 768, 768), (1, 37, 45), (3, 8, 1))]
    res = [torch.zeros(2, 768, device=dev), rnd(45), torch.zeros(3, 1, device=dev)]
    hip.reduce_parts_multi([(ins[0], res[0], 2, 768, 768, False), (ins[1], res[1], 1, 37, 45, True), (ins[2], res[2], 3, 8, 1, False)])
    keep("reduce_parts_multi 3 tasks", f32=res[0], bf16_acc=res[1], f32_one_column=res[2])


def run_all():
    for case in rc.FWD_CASES:
        run_fwd(case)
    for C in rc.LN_WIDTHS:
        for first in ("ln", "identity"):
            run_pair(C, first)
    for case in rc.BWD_CASES:
        run_bwd(case, False)
    for case in rc.BWD_DROP_CASES:
        run_bwd(case, True)
    for c in rc.REDUCE_CASES:
        run_reduce(c)
    run_big(torch.Generator(device=dev).manual_seed(3))


def timeit(f, n=200):
    for i in range(10):
        f(i)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(n):
        f(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


def run_time(nbuf=8):
    gen = torch.Generator(device=dev).manual_seed(1)
    rows, C = 8480, 3072
    X = [torch.randn(rows, C, device=dev, generator=gen).bfloat16() for _ in range(nbuf)]
    Y = [torch.empty_like(X[0]) for _ in range(nbuf)]
    gam, bet, (mean, rstd) = torch.ones(C, device=dev), torch.zeros(C, device=dev), stats(rows)
    print("%-52s %7.1f us" % ("ln_fwd gelu 8480x3072", timeit(lambda i: hip.ln_fwd(X[i % nbuf], gam, bet, Y[i % nbuf], mean, rstd, gelu=True))), flush=True)
    del X, Y
    for name, outer, parts, n, dt in (("reduce_parts LN partials 2x768x768 f32", 2, hip.LN_BWD_BLOCKS, 768, F32),
                                      ("reduce_parts loss statistics 1x8192x452 f32 (tall)", 1, 8 * 32 * 32, 2 + 3 * 150, F32),
                                      ("reduce_parts bias gradient 1x256x768 bf16", 1, hip.COLSUM_BLOCKS, 768, BF16)):
        P = [torch.randn(outer, parts, n, device=dev, generator=gen) for _ in range(nbuf)]
        out = torch.zeros(outer, n, dtype=dt, device=dev)
        print("%-52s %7.1f us" % (name, timeit(lambda i: hip.reduce_parts(P[i % nbuf], out, outer, parts, n))), flush=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "time":
        run_time()
    elif mode in ("save", "cmp") and len(sys.argv) == 3:
        run_all()
        if mode == "save":
            torch.save(outs, sys.argv[2])
            print("saved %d outputs of %s to %s" % (len(outs), hip.LIB_PATH, sys.argv[2]))
        else:
            ref = torch.load(sys.argv[2])
            assert ref.keys() == outs.keys()
            ndiff = 0
            for k, t in outs.items():
                bad = t.view(torch.int16 if t.dtype == BF16 else torch.int32) != ref[k].view(torch.int16 if t.dtype == BF16 else torch.int32)
                n = int(bad.sum())
                ndiff += n > 0
                print("%-64s %s" % (k, "bit-equal" if n == 0 else "%d of %d differ, max |diff| %.3g" % (
                    n, t.numel(), (t.double() - ref[k].double()).abs().max().item())))
            nzero = sum(1 for t in outs.values() if not bool(t.float().abs().sum() > 0))    # (expected: mean / rstd of the identity first stages)
            print("ROWOPS_BITS %d outputs (%d of them all zero), %s" % (len(outs), nzero, "all bit-equal" if ndiff == 0 else "%d differ" % ndiff))
            sys.exit(1 if ndiff else 0)
    else:
        sys.exit(__doc__)
