"""The CPU op emulator with the attention of ABI 308: `causal=`, head dims up to 512, and the two capability queries the engines ask before they replace a materialised
attention by one fused launch (engine/base.py::side_flash).  tests/emu_ops.py stays as it is - plain EmuOps answers neither query, so the engines keep giving it the
materialised sequence call for call.  The launch itself is tests/attn_wide_spec.py's statement of the two rules."""
import torch

import attn_wide_spec as WS
from attn_split_spec import SplitAttnEmuOps
from followyourclick_amd.ops import resolve_f32_products


class WideEmuOps(SplitAttnEmuOps):
    def __init__(self, acc=torch.float64, f32_products="exact"):
        super().__init__(acc=acc, f32_products=f32_products)
        self.calls = []      # (name, keyword arguments without tensors) of every attention launch

    def attention_causal_supported(self):
        return True

    def attention_max_head_dim(self):
        return 512

    def attention(self, q, k, vt, o, *, batch, heads, n_q, n_k, d, ldo, ldvt, scale, kv_batch_div=1, accumulate=False, o_scale=1.0, q_batch_mod=0, products=None,
                  causal=False):
        resolve_f32_products("attention", q.dtype, products, self.f32_products, fused_exact=False)
        assert d % 8 == 0 and d <= 512 and (d <= 160 or d % 32 == 0), d
        assert not causal or (n_q == n_k and q_batch_mod == 0)
        self.calls.append(("attention", dict(batch=batch, heads=heads, n_q=n_q, n_k=n_k, d=d, causal=causal)))
        WS.attention_rule(q, k, vt, o, batch=batch, heads=heads, n_q=n_q, n_k=n_k, d=d, ldo=ldo, ldvt=ldvt, scale=scale, kv_batch_div=kv_batch_div, accumulate=accumulate,
                          o_scale=o_scale, q_batch_mod=q_batch_mod, causal=causal)
