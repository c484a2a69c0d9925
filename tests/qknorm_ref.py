"""Float64 numpy reference for the q / k norm (Qwen3): arch_ref.ArchRef with an RMSNorm over
each head of q and of k between the clip and RoPE, the f16 KV cache and the sinks'
one-position rotation as they are. TEST INFRASTRUCTURE ONLY.

With the norm off (a config without qk_norm, or wrong="none" on one with it) the block is
ArchRef's own, so the numbers are ArchRef's bit for bit. The other `wrong` switches are the
models a mistaken kernel would compute on the same tensors (the CPU tests' margins):
  "none"     no norm at all
  "unit"     g = 1 (the scale alone)
  "swap"     gq and gk exchanged
  "reverse"  g reversed within the head
"""
import numpy as np

import arch_ref
import ref_numpy as R
from yalm_amd import models as M

WRONG = ("none", "unit", "swap", "reverse")


def head_rmsnorm(a, g, head_dim, eps):
    """a' = a / sqrt(mean(a^2 over the head) + eps) * g, per head of head_dim elements."""
    h = a.reshape(-1, head_dim)
    return (h / np.sqrt((h * h).sum(axis=1, keepdims=True) / head_dim + eps) * g[None, :]).reshape(-1)


class QKNormRef(arch_ref.ArchRef):
    def __init__(self, cfg: M.ModelConfig, tensors: dict, wrong=None, **kw):
        assert wrong is None or wrong in WRONG
        super().__init__(cfg, tensors, **kw)
        self.wrong = wrong
        self.norm_on = bool(cfg.qk_norm) and wrong != "none"

    def gains(self, l):
        g = M.qk_norm_names(l)
        gq, gk = self.t[g["gq"]].astype(np.float64), self.t[g["gk"]].astype(np.float64)
        if self.wrong == "unit":
            return np.ones_like(gq), np.ones_like(gk)
        if self.wrong == "swap":
            return gk, gq
        if self.wrong == "reverse":
            return gq[::-1], gk[::-1]
        return gq, gk

    def block(self, l, x, pos, kv_sink, kv_pos, kv_len):
        if not self.norm_on:
            return super().block(l, x, pos, kv_sink, kv_pos, kv_len)
        c, t = self.c, self.t
        n = M.layer_names(l)
        xb = R.rmsnorm(x, t[n["rms_att"]], c.norm_eps)
        clip = c.qkv_clip
        q, k, v = t[n["wq"]] @ xb, t[n["wk"]] @ xb, t[n["wv"]] @ xb
        q, k, v = np.clip(q, -clip, clip), np.clip(k, -clip, clip), np.clip(v, -clip, clip)
        gq, gk = self.gains(l)
        q = head_rmsnorm(q, gq, c.head_dim, c.norm_eps)
        k = head_rmsnorm(k, gk, c.head_dim, c.norm_eps)
        q = arch_ref.rope_table(q, c.head_dim, pos, self.table)
        k = arch_ref.rope_table(k, c.head_dim, pos, self.table)
        self.k[l][kv_pos] = k.astype(np.float16)
        self.v[l][kv_pos] = v.astype(np.float16)
        for r in range(kv_sink):
            kk = arch_ref.rope_table(self.k[l][r].astype(np.float64), c.head_dim, 1, self.table)
            self.k[l][r] = kk.astype(np.float16)
        G = c.n_heads // c.n_kv_heads
        K = self.k[l][:kv_len].astype(np.float64).reshape(kv_len, c.n_kv_heads, c.head_dim)
        V = self.v[l][:kv_len].astype(np.float64).reshape(kv_len, c.n_kv_heads, c.head_dim)
        out = np.zeros(c.q_dim)
        for h in range(c.n_heads):
            g = h // G
            s = K[:, g, :] @ q[h * c.head_dim:(h + 1) * c.head_dim] / np.sqrt(c.head_dim)
            p = np.exp(s - s.max())
            p /= p.sum()
            out[h * c.head_dim:(h + 1) * c.head_dim] = p @ V[:, g, :]
        x = x + self.allreduce(t[n["wo"]] @ out)
        xb = R.rmsnorm(x, t[n["rms_ffn"]], c.norm_eps)
        a = t[n["w1"]] @ xb
        hb = (R.silu(a) if c.act == M.SILU else R.gelu(a)) * (t[n["w3"]] @ xb)
        return x + self.allreduce(t[n["w2"]] @ hb)
