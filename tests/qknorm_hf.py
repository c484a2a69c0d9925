"""A seeded tiny Qwen3 HF checkpoint directory (arch_hf.write_hf_dir plus the per-head
q_norm / k_norm weights) for the converter and host tests, and an HF-layout float64
restatement of the model (half-split RoPE on unpermuted weights) to hold the converter's
permutation against. TEST INFRASTRUCTURE ONLY.
"""
import json
import os

import numpy as np

import arch_hf
from golden.make_golden import TINY_HF
from yalm_amd.yalmfile import write_yalm

# Qwen3's config keys: an explicit head_dim, rope_theta 1e6, eps 1e-6, no attention bias,
# full attention in every layer
QWEN3_HF = dict(TINY_HF, head_dim=16, rope_theta=1000000.0, rms_norm_eps=1e-6, attention_bias=False,
                use_sliding_window=False, sliding_window=None, max_window_layers=2,
                layer_types=["full_attention", "full_attention"])
HOST_PROMPT, HOST_N = arch_hf.HOST_PROMPT, arch_hf.HOST_N


def write_qwen3(path, hf=QWEN3_HF, seed=8, tie=True):
    """Returns the HF tensors (name -> f32 array) it wrote; norm weights uniform in [0.5, 2.5)."""
    t = arch_hf.write_hf_dir(path, hf, "Qwen3ForCausalLM", seed=seed, tie=tie)
    hd = hf.get("head_dim", hf["hidden_size"] // hf["num_attention_heads"])
    assert hd * hf["num_attention_heads"] == hf["hidden_size"]  # (write_hf_dir sizes the projections so)
    rng = np.random.Generator(np.random.PCG64(seed + 1000))
    for l in range(hf["num_hidden_layers"]):
        for k in ("q_norm", "k_norm"):
            t[f"model.layers.{l}.self_attn.{k}.weight"] = rng.uniform(0.5, 2.5, hd).astype(np.float32)
    write_yalm(os.path.join(path, "model.safetensors"), t, {})
    return t


def rotate_half(v, head_dim, pos, theta):
    """HF's RoPE on [heads * head_dim]: pair (i, i + head_dim / 2) of every head."""
    h = v.reshape(-1, head_dim)
    half = head_dim // 2
    ang = pos * (1.0 / np.power(theta, np.arange(half) * 2.0 / head_dim))
    c, s = np.cos(ang), np.sin(ang)
    a, b = h[:, :half], h[:, half:]
    return np.concatenate([a * c - b * s, a * s + b * c], axis=1).reshape(-1)


def hf_forward_all(path, tokens):
    """Logits (len(tokens), vocab) of the HF directory's model in float64, as the HF modelling
    code states it: q_norm / k_norm per head on the projection, rotate-half RoPE, causal
    attention over the whole past; K and V rows rounded to f16 as the engine's cache holds them
    (an elementwise rounding: it commutes with the converter's permutation)."""
    with open(os.path.join(path, "config.json")) as f:
        cfg = json.load(f)
    from yalm_amd.yalmfile import read_yalm

    yd = read_yalm(os.path.join(path, "model.safetensors"))
    t = {k: np.array(v.data).reshape(v.shape).astype(np.float64) for k, v in yd.tensors.items()}
    yd.close()
    nh, nkv, hd = cfg["num_attention_heads"], cfg["num_key_value_heads"], cfg["head_dim"]
    eps, theta, L = cfg["rms_norm_eps"], cfg["rope_theta"], cfg["num_hidden_layers"]

    def rms(x, w):
        return x / np.sqrt(np.mean(x * x) + eps) * w

    def head_rms(v, w):
        h = v.reshape(-1, hd)
        return (h / np.sqrt(np.mean(h * h, axis=1, keepdims=True) + eps) * w).reshape(-1)

    K = [[] for _ in range(L)]
    V = [[] for _ in range(L)]
    out = []
    for pos, tok in enumerate(tokens):
        x = t["model.embed_tokens.weight"][tok].copy()
        for l in range(L):
            p = f"model.layers.{l}."
            xb = rms(x, t[p + "input_layernorm.weight"])
            q = head_rms(t[p + "self_attn.q_proj.weight"] @ xb, t[p + "self_attn.q_norm.weight"])
            k = head_rms(t[p + "self_attn.k_proj.weight"] @ xb, t[p + "self_attn.k_norm.weight"])
            v = t[p + "self_attn.v_proj.weight"] @ xb
            q, k = rotate_half(q, hd, pos, theta), rotate_half(k, hd, pos, theta)
            K[l].append(k.astype(np.float16).reshape(nkv, hd))
            V[l].append(v.astype(np.float16).reshape(nkv, hd))
            Kl, Vl = np.array(K[l]).astype(np.float64), np.array(V[l]).astype(np.float64)
            att = np.zeros(nh * hd)
            for h in range(nh):
                g = h // (nh // nkv)
                s = Kl[:, g, :] @ q[h * hd:(h + 1) * hd] / np.sqrt(hd)
                w = np.exp(s - s.max())
                att[h * hd:(h + 1) * hd] = (w / w.sum()) @ Vl[:, g, :]
            x = x + t[p + "self_attn.o_proj.weight"] @ att
            xb = rms(x, t[p + "post_attention_layernorm.weight"])
            a = t[p + "mlp.gate_proj.weight"] @ xb
            x = x + t[p + "mlp.down_proj.weight"] @ (a / (1.0 + np.exp(-a)) * (t[p + "mlp.up_proj.weight"] @ xb))
        x = rms(x, t["model.norm.weight"])
        out.append(t.get("lm_head.weight", t["model.embed_tokens.weight"]) @ x)
    return np.array(out)


def host_reference(path, prompt=HOST_PROMPT, n=HOST_N):
    """arch_hf.host_reference over qknorm_ref: (prompt ids, tokens, smallest top-2 gap / max|logit|)."""
    import qknorm_ref
    from yalm_amd.tokenizer import Tokenizer
    from yalm_amd.yalmfile import read_yalm

    yd = read_yalm(path)
    enc = Tokenizer.from_yalm(yd).encode(prompt)
    yd.close()
    cfg, t = arch_hf.load_yalm(path)
    m = qknorm_ref.QKNormRef(cfg, t)
    for pos, tk in enumerate(enc[:-1]):
        m.forward(tk, pos)
    lg, pos, out, gap = m.forward(enc[-1], len(enc) - 1), len(enc), [], np.inf
    for _ in range(n):
        s = np.sort(lg)
        gap = min(gap, float((s[-1] - s[-2]) / np.max(np.abs(lg))))
        nt = int(np.argmax(lg))
        out.append(nt)
        if nt == cfg.eos_token_id:
            break
        lg = m.forward(nt, pos)
        pos += 1
    return enc, out, gap
