"""Float64 numpy reference for the two model-family forms the frozen oracle does not have:
a bias on the q / k / v projections (Qwen2) and the Llama-3.1 / 3.2 "llama3" RoPE scaling.
ref_numpy.RefModel (f64, f16 KV cache, the sinks' one-position rotation) with its block
restated: v = clip(W . xb + b), and every rope call over an explicit frequency table.
TEST INFRASTRUCTURE ONLY.

The table: without scaling it is RefModel's own f64 expression (so a model with a zero bias
and no scaling gives RefModel's numbers exactly); with scaling, the rule restated in f64 on
those f64 frequencies -- independent of models.rope_inv_freq and of the decoder's f32 table,
from which it differs by f32 roundings of the frequency (6e-8 relative: 1e-6 rad at the
positions the tests reach).
"""
import numpy as np

import ref_numpy as R
from yalm_amd import models as M


def llama3_f64(f, rs):
    """The llama3 rule on f64 frequencies f; rs = (type, factor, low, high, original_max_position)."""
    _, factor, low, high, orig = rs
    out = np.array(f, np.float64)
    for i, fi in enumerate(out):
        if fi == 0.0:
            continue
        wavelen = 2.0 * np.pi / fi
        if wavelen < orig / high:
            continue
        if wavelen > orig / low:
            out[i] = fi / factor
        else:
            s = (orig / wavelen - low) / (high - low)
            out[i] = (1.0 - s) * fi / factor + s * fi
    return out


def regimes(f, rs):
    """Per pair frequency: 0 kept, 1 blended, 2 divided by factor."""
    _, _, low, high, orig = rs
    f = np.asarray(f, np.float64)
    with np.errstate(divide="ignore"):
        w = 2.0 * np.pi / f
    return np.where(w < orig / high, 0, np.where(w > orig / low, 2, 1))


def freq_table(c: M.ModelConfig, rope_scaling="config"):
    """head_dim / 2 pair frequencies in f64; rope_scaling: "config" (c.rope_scaling), None or a tuple."""
    rs = c.rope_scaling if rope_scaling == "config" else rope_scaling
    j = np.arange(0, c.head_dim, 2)
    f = np.where(j >= c.rotary_dim, 0.0, 1.0 / np.power(float(np.float32(c.rope_theta)), j / c.rotary_dim))
    return f if rs is None else llama3_f64(f, rs)


def rope_table(v, head_dim, pos, table):
    """ref_numpy.rope over an explicit per-pair frequency table."""
    v = v.copy()
    i = np.arange(0, v.shape[0], 2)
    ang = pos * table[(i % head_dim) // 2]
    c, s = np.cos(ang), np.sin(ang)
    v0, v1 = v[i].copy(), v[i + 1].copy()
    v[i] = v0 * c - v1 * s
    v[i + 1] = v0 * s + v1 * c
    return v


class ArchRef(R.RefModel):
    """use_bias / rope_scaling switch a form off on the same tensors: the model a decoder
    that dropped it would compute (the CPU tests' margins)."""

    def __init__(self, cfg: M.ModelConfig, tensors: dict, use_bias: bool = True, rope_scaling="config", table=None):
        if cfg.weight_dtype == M.Q4:  # the exact f16 twin
            cfg, tensors = M.q4_twin(cfg, tensors)
        super().__init__(cfg, tensors)
        self.use_bias = bool(cfg.qkv_bias and use_bias)
        self.table = np.asarray(table, np.float64) if table is not None else freq_table(cfg, rope_scaling)

    def block(self, l, x, pos, kv_sink, kv_pos, kv_len):
        c, t = self.c, self.t
        n = M.layer_names(l)
        xb = R.rmsnorm(x, t[n["rms_att"]], c.norm_eps)
        clip = c.qkv_clip
        q, k, v = t[n["wq"]] @ xb, t[n["wk"]] @ xb, t[n["wv"]] @ xb
        if self.use_bias:
            b = M.bias_names(l)
            q, k, v = q + t[b["bq"]], k + t[b["bk"]], v + t[b["bv"]]
        q, k, v = np.clip(q, -clip, clip), np.clip(k, -clip, clip), np.clip(v, -clip, clip)
        q = rope_table(q, c.head_dim, pos, self.table)
        k = rope_table(k, c.head_dim, pos, self.table)
        self.k[l][kv_pos] = k.astype(np.float16)
        self.v[l][kv_pos] = v.astype(np.float16)
        for r in range(kv_sink):
            kk = rope_table(self.k[l][r].astype(np.float64), c.head_dim, 1, self.table)
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

    def greedy(self, token, pos, n):
        """n greedy tokens from (token, pos): (tokens, the logits of every step)."""
        toks, lgs = [], []
        for i in range(n):
            lg = self.forward(token, pos + i)
            token = int(np.argmax(lg))
            toks.append(token)
            lgs.append(lg)
        return toks, lgs
