"""Element-wise gradient error per tensor family on the Base B=2 golden (tests/golden/base_c1_b2.npz): where the bf16 path is
least accurate (k_proj.weight: VERDICT r3 weak #2)."""
import os, sys, collections
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "oracle"))
import numpy as np, torch
import segofa_ref as O
import test_configs_gpu as T

dev = torch.device("cuda:0")
ocfg = O.base_config()
g = T._load_golden(os.path.join(ROOT, "tests", "golden"), "base_c1_b2.npz")
sd = O.procedural_state_dict(ocfg)
batch = O.synthetic_batch(ocfg, 2, int(g["src_len"]))
sd = T._golden_weights(g, sd, ocfg, batch)
m = T._base_model(ocfg, sd, dev).train()
loss, _, _ = T._crit(ocfg)(m, T._sample(batch, dev))
loss.backward(); torch.cuda.synchronize()
named = dict(m.named_parameters())
fam = collections.defaultdict(list)
for key in g.files:
    if not key.startswith("gsub:"): continue
    name = key[5:]
    ref = torch.from_numpy(g[key]); got = named[name].grad
    if got is None or ref.pow(2).mean().sqrt().item() < 1e-12: continue
    got = got.float().reshape(-1).cpu()[T._sub_index(name, got.numel())]
    r = ((got - ref).norm() / (ref.norm() + 1e-30)).item()
    f = ".".join(name.split(".")[-2:]) if "layers" in name else name
    if "layers" in name: f = name.split(".")[0][:3] + ":" + ".".join(name.split(".")[3:])
    fam[f].append(r)
for f, v in sorted(fam.items(), key=lambda kv: -max(kv[1]))[:14]:
    print("%-44s n=%2d  max %.4f  mean %.4f" % (f, len(v), max(v), sum(v) / len(v)))

# ---- where the k_proj.weight error comes from (encoder layer 0): the weight-gradient GEMM against an fp32 product of ITS OWN
# bf16 operands, and the size of the token-common component of the LayerNorm output the cancellation sum_j dK_j = 0 multiplies
eng = m.engine
C = eng.cfg.embed_dim
for tg, p in (("e0", "encoder.layers.0."), ("e5", "encoder.layers.5.")):
    s = eng.saved[tg + "_sa"]
    xn = s["xn"].float()                                   # [B*T, C] bf16 LayerNorm output (the forward's operand)
    key = [k for k in eng.ws if k.startswith("g_dqkv_") and k.endswith("@" + tg + "s")]
    dqkv = eng.ws[key[0]].float().view(-1, 3 * C)
    dk = dqkv[:, C:2 * C]
    G = named[p + "self_attn.k_proj.weight"].grad.float()
    Gf = dk.t() @ xn
    B_ = s["qkv"].shape[0]; T_ = xn.shape[0] // B_
    xb = xn.view(B_, T_, C); xm = xb.mean(1, keepdim=True)
    colsum = dk.view(B_, T_, C).sum(1)                     # sum_j dK_j per batch element: zero in exact arithmetic
    print("%s k_proj.weight: GEMM vs fp32 product of its own bf16 operands rel-L2 %.2e; |token-mean of xn| / |xn - mean| = %.1f; "
          "|sum_j dK_j| / (sqrt(T) rms|dK_j|) = %.3f" % (tg, ((G - Gf).norm() / Gf.norm()).item(), (xm.norm() * T_ ** 0.5 / (xb - xm).norm()).item() * B_ ** 0.5,
                                                      (colsum.norm() / (T_ ** 0.5 * dk.norm() / (B_ * T_) ** 0.5 * B_ ** 0.5)).item()))
    Gc = dk.view(B_, T_, C).transpose(1, 2) @ (xb - xm)   # the same gradient with the token mean removed from x (exact identity)
    Gc = Gc.sum(0)
    sub = T._sub_index(p + "self_attn.k_proj.weight", G.numel())
    ref = torch.from_numpy(g["gsub:" + p + "self_attn.k_proj.weight"])
    r = lambda a: ((a.reshape(-1).cpu()[sub] - ref).norm() / ref.norm()).item()
    dbk = named[p + "self_attn.k_proj.bias"].grad.float()           # = sum_{b,j} dK_bj: zero in exact arithmetic
    cbar = xn.mean(0)
    G1 = G - dbk[:, None] * cbar[None, :]                              # rank-1: the same identity with ONE mean over all rows
    print("   vs the reference: as computed %.4f, from fp32 product %.4f, with the token mean of x removed (fp32 product) %.4f, "
          "rank-1 correction G - db_k (x) mean(x) on the bf16 gradient %.4f" % (r(G), r(Gf), r(Gc), r(G1)))
