"""nn.Modules on top of `torch.ops.ifseg.*` for callers that keep the reference's module tree.

`MultiheadAttention` carries the parameters and state-dict keys of the reference attention module
(unify_multihead_attention.py:44-90 with `scale_heads`: `q_proj`, `k_proj`, `v_proj`, `out_proj` as nn.Linear, `c_attn`), so
a checkpoint's `*.self_attn.*` / `*.encoder_attn.*` entries load into it unchanged; its forward is composed of
`torch.ops.ifseg.linear` and `torch.ops.ifseg.attention_bias` only (hand-written gfx950 kernels, no PyTorch fall-back).
"""
from typing import Optional

import torch
import torch.nn as nn

from . import ops  # noqa: F401  (registers torch.ops.ifseg.*)


def key_counts(key_padding_mask: torch.Tensor) -> torch.Tensor:
    """[B, S] bool (True = padding) -> int32 [B] valid key counts.  The kernels take a COUNT per sample: the padding must be
    a suffix of the keys (right padding) and leave at least one key -- anything else raises ValueError (one host read)."""
    if key_padding_mask.dim() != 2 or key_padding_mask.dtype != torch.bool:
        raise ValueError("key_padding_mask must be a bool [batch, keys] tensor")
    m = key_padding_mask
    bad = (m[:, :-1] & ~m[:, 1:]).any() | m[:, 0].any()
    if bool(bad):
        raise ValueError("ifseg_amd.modules.MultiheadAttention: the padding of every sample must be a suffix of its keys "
                         "(right padding) and leave at least one key")
    return (~m).sum(1).to(torch.int32)


class MultiheadAttention(nn.Module):
    """Batch-first multi-head attention with a head dimension of 64 on the batch-inner attention kernels.

        forward(query [B,T,C], key_value=None [B,S,C], attn_bias=None [H,T,S], key_padding_mask=None [B,S] bool,
                dropout_p=0.0, seed=0) -> [B,T,C]

    q = q_proj(query) * scaling with scaling = (head_dim * scale_factor) ** -0.5; k, v = k_proj / v_proj(key_value or query);
    out_proj(c_attn_h * dropout(softmax(q k^T + attn_bias [+ key padding])) v).  `attn_bias` is batch-invariant, fp32 or bf16,
    -inf = masked (an ordinary causal mask goes here) and receives a gradient.  `key_padding_mask` must be a suffix of the keys
    (it becomes a key count per sample).  Attention dropout (`dropout_p`, the kernels' counter-based mask for `seed`) is applied
    only while `self.training`.  Activations, weights and biases are bf16 (`module.to(device, torch.bfloat16)`), `c_attn` is
    read as fp32.

    Out of scope: the reference's time-first layout, incremental decoding state, `need_weights`, `add_bias_kv`,
    `add_zero_attn`, separate key / value widths, head dimensions other than 64."""

    def __init__(self, embed_dim, num_heads, bias=True, scale_factor=2, scale_heads=True):
        super().__init__()
        if embed_dim != num_heads * 64:
            raise ValueError("MultiheadAttention: the attention kernels take a head dimension of 64 (embed_dim = %d, num_heads = %d)"
                             % (embed_dim, num_heads))
        self.embed_dim, self.num_heads, self.head_dim = embed_dim, num_heads, embed_dim // num_heads
        self.scaling = float(self.head_dim * scale_factor) ** -0.5
        self.c_attn = nn.Parameter(torch.ones(num_heads)) if scale_heads else None
        self.k_proj = nn.Linear(embed_dim, embed_dim, bias=bias)
        self.v_proj = nn.Linear(embed_dim, embed_dim, bias=bias)
        self.q_proj = nn.Linear(embed_dim, embed_dim, bias=bias)
        self.out_proj = nn.Linear(embed_dim, embed_dim, bias=bias)
        self.reset_parameters()

    def reset_parameters(self):
        # the reference's initialisation for equal q / k / v widths (unify_multihead_attention.py:97-111)
        for m in (self.k_proj, self.v_proj, self.q_proj):
            nn.init.xavier_uniform_(m.weight, gain=2 ** -0.5)
        nn.init.xavier_uniform_(self.out_proj.weight)
        if self.out_proj.bias is not None:
            nn.init.constant_(self.out_proj.bias, 0.0)

    def forward(self, query, key_value: Optional[torch.Tensor] = None, attn_bias: Optional[torch.Tensor] = None,
                key_padding_mask: Optional[torch.Tensor] = None, dropout_p: float = 0.0, seed: int = 0):
        lin = torch.ops.ifseg.linear
        kv = query if key_value is None else key_value
        q = lin(query, self.q_proj.weight, self.q_proj.bias) * self.scaling
        k = lin(kv, self.k_proj.weight, self.k_proj.bias)
        v = lin(kv, self.v_proj.weight, self.v_proj.bias)
        kv_len = key_counts(key_padding_mask) if key_padding_mask is not None else None
        gain = self.c_attn.float() if self.c_attn is not None else None
        p = float(dropout_p) if self.training else 0.0
        o = torch.ops.ifseg.attention_bias(q, k, v, attn_bias, gain, kv_len, False, 0, p, int(seed))[0]
        return lin(o, self.out_proj.weight, self.out_proj.bias)
