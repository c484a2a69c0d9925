"""HF checkpoint dir (config.json, tokenizer.json, *.safetensors) -> .yalm.

Own converter with the semantics of the reference /root/reference/convert.py
(numpy, no torch): metadata normalisation (convert.py:22-81), tokenizer blob
with sentencepiece '▁' -> ' ' or GPT-2 byte decoding and NUL -> BEL
(convert.py:83-125), Q/K rotary permutation to interleaved pairs
(permute_reverse, convert.py:145-158), f32 norms, weights cast to fp32 /
fp16 (round-to-nearest-even) / fp8 E5M2 (torch's fp8e5m2_from_fp32_value:
RNE, >= 2^16 -> inf), tied classifier when ``tie_word_embeddings`` is not
False (convert.py:200). q4 (this engine's own format, models.q4_quantize): every weight
matrix, the embedding included, is quantised from its fp16 conversion and stored as a U8
tensor [rows, row_bytes(n)]; dense models only. e4m3 (this engine's own too, models.e4m3_quantize:
OCP E4M3 codes with one power-of-two f32 scale per row) is written the same way, as U8 tensors
[rows, n + 16], from the fp16 conversion; dense models only. Mixtral checkpoints (convert.py:54-56, 78-80, 188-193): the
router gate becomes ``moegate``, each layer's experts are stacked along a new
leading axis, and n_experts / n_experts_active go into the metadata.
Two forms the reference's converter and engine do not read (such a file is this engine's
alone, as q4 is): Qwen2 / Qwen2.5 (``Qwen2ForCausalLM``: the Llama block plus a bias on q, k
and v, written F32 as ``attn.{wq,wk,wv}.bias`` with the q / k rows permuted as their weights'
rows are; metadata ``qkv_bias``), and Llama-3.1 / 3.2 ``rope_scaling`` of type ``llama3``
(metadata ``rope_scaling_type`` / ``rope_scaling_factor`` / ``rope_low_freq_factor`` /
``rope_high_freq_factor`` / ``rope_original_max_position``). Any other scaling type raises.
Qwen3 dense models (``Qwen3ForCausalLM``) are a third: the Llama block plus an RMSNorm over each
head of q and k ahead of RoPE, written F32 as ``attn.{q_norm,k_norm}.weight`` (``head_dim``
elements) with the within-head permutation of the q / k rows, so each weight stays with its
element; metadata ``qk_norm``. Sliding-window layers and an attention bias raise.

Usage: python -m yalm_amd.convert [--dtype fp16] out.yalm hf_dir/
"""

from __future__ import annotations

import argparse
import json
import os

import numpy as np

from . import models as M
from .yalmfile import read_yalm, write_yalm

SUPPORTED_ARCHITECTURES = ["LlamaForCausalLM", "MistralForCausalLM", "MixtralForCausalLM", "Qwen2ForCausalLM",
                           "Qwen3ForCausalLM"]
SUPPORTED_DTYPES = ["fp32", "fp16", "fp8", "q4", "e4m3"]


def metadata_from_config(config: dict, dtype: str) -> dict:
    arch = config["architectures"][0]
    if arch not in SUPPORTED_ARCHITECTURES:
        raise ValueError(f"Architecture {arch} is not supported, must be one of {SUPPORTED_ARCHITECTURES}")
    if dtype not in SUPPORTED_DTYPES:
        raise ValueError(f"Data type {dtype} is not supported, must be one of {SUPPORTED_DTYPES}")
    if arch == "MixtralForCausalLM" and dtype == "q4":
        raise ValueError("q4 has no mixture-of-experts form")
    if arch == "MixtralForCausalLM" and dtype == "e4m3":
        raise ValueError("e4m3 has no mixture-of-experts form")
    head_dim = config.get("head_dim", config["hidden_size"] // config["num_attention_heads"])
    # (Llama's attention_bias also biases o_proj; Qwen2 has no such flag: its q / k / v bias is the architecture's)
    if config.get("attention_bias", False) or config.get("mlp_bias", False):
        raise ValueError("attention/mlp bias is not supported")
    qwen2 = arch == "Qwen2ForCausalLM"
    qwen3 = arch == "Qwen3ForCausalLM"
    if (qwen2 or qwen3) and config.get("use_sliding_window", False):
        raise ValueError(f"{arch[:5]} use_sliding_window is not supported")
    if qwen3 and any(t != "full_attention" for t in config.get("layer_types") or []):
        raise ValueError("Qwen3 layer_types other than full_attention are not supported")
    rope_scaling = rope_scaling_from_config(config)
    if config["hidden_act"] not in ("gelu", "silu"):
        raise ValueError(f"unsupported hidden_act {config['hidden_act']}")
    md = {
        "arch": arch,
        "dtype": dtype,
        "dim": config["hidden_size"],
        "hidden_dim": config["intermediate_size"],
        "head_dim": head_dim,
        "n_layers": config["num_hidden_layers"],
        "n_heads": config["num_attention_heads"],
        "n_kv_heads": config.get("num_key_value_heads", config["num_attention_heads"]),
        "vocab_size": config["vocab_size"],
        "max_seq_len": config["max_position_embeddings"],
        "bos_token_id": config["bos_token_id"],
        "eos_token_id": config["eos_token_id"],
        "rope_theta": config.get("rope_theta", 10000.0),
        "rotary_dim": int(head_dim * config.get("partial_rotary_factor", 1)),
        "norm_eps": config["rms_norm_eps"],
        "norm_type": "rmsnorm",
        "act_type": config["hidden_act"],
    }
    if arch == "MixtralForCausalLM":
        md["n_experts"] = config["num_local_experts"]
        md["n_experts_active"] = config["num_experts_per_tok"]
    if qwen2:
        md["qkv_bias"] = 1
    if qwen3:
        md["qk_norm"] = 1
    if rope_scaling is not None:
        md.update(M.rope_scaling_metadata(rope_scaling))
    # str() of the python value, as convert.py:63-80 does (floats print as 10000.0, 1e-05)
    return {k: str(v) for k, v in md.items()}


def rope_scaling_from_config(config: dict):
    """HF ``rope_scaling``: None / type "default" -> None; "llama3" -> the ModelConfig tuple;
    anything else (yarn, linear, dynamic, ...) raises instead of converting a model whose
    logits would not be the checkpoint's."""
    rs = config.get("rope_scaling")
    if rs is None:
        return None
    kind = rs.get("rope_type") or rs.get("type")
    if kind in (None, "default"):
        return None
    if kind != "llama3":
        raise ValueError(f"rope_scaling type {kind!r} is not supported (only 'llama3')")
    return M.check_rope_scaling(("llama3", rs["factor"], rs["low_freq_factor"], rs["high_freq_factor"],
                                 rs["original_max_position_embeddings"]))


def gpt2_bytes_to_unicode() -> dict:
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(ord("¡"), ord("¬") + 1)) + list(range(ord("®"), ord("ÿ") + 1))
    cs = bs[:]
    n = 0
    for b in range(2**8):
        if b not in bs:
            bs.append(b)
            cs.append(2**8 + n)
            n += 1
    return dict(zip(bs, [chr(c) for c in cs]))


def load_tokens(tokenizer_path: str, vocab_size: int) -> list:
    tokens = [""] * vocab_size
    with open(tokenizer_path, "r") as f:
        tok = json.load(f)
    gpt2 = not tok["model"].get("byte_fallback", False)
    vocab = tok["model"]["vocab"]
    if len(vocab) > vocab_size:
        raise ValueError("tokenizer vocab larger than vocab_size")
    for t, i in vocab.items():
        tokens[i] = t
    for added in tok["added_tokens"]:
        tokens[added["id"]] = added["content"]
    dec = {v: k for k, v in gpt2_bytes_to_unicode().items()}
    out = []
    for t in tokens:
        if gpt2:
            b = bytes([dec.get(c, 0) for c in t])
        else:
            b = t.replace("▁", " ").encode("utf-8")
        b = b.replace(b"\0", b"\7")
        out.append(b)
    return out


def permute_reverse(w: np.ndarray, heads: int, rotary_dim: int) -> np.ndarray:
    """Undo HF's rotate-half Q/K row order into interleaved (even, odd) pairs."""
    head_dim = w.shape[0] // heads
    assert rotary_dim <= head_dim
    w = w.reshape(heads, head_dim, -1)
    wr = w[:, :rotary_dim]
    wk = w[:, rotary_dim:]
    wr = wr.reshape(heads, 2, rotary_dim // 2, -1).transpose(0, 2, 1, 3).reshape(heads, rotary_dim, -1)
    return np.concatenate([wr, wk], axis=1).reshape(heads * head_dim, -1)


def f32_to_e5m2(x: np.ndarray) -> np.ndarray:
    """Round-to-nearest-even f32 -> OCP E5M2 bits (torch c10 fp8e5m2_from_fp32_value)."""
    f = np.ascontiguousarray(x, np.float32).view(np.uint32)
    sign = f & np.uint32(0x80000000)
    a = f ^ sign
    fp32_inf = np.uint32(255 << 23)
    fp8_max = np.uint32(143 << 23)
    denorm_mask = np.uint32(134 << 23)
    res = np.zeros(a.shape, np.uint32)
    big = a >= fp8_max
    res[big] = np.where(a[big] > fp32_inf, 0x7F, 0x7C)
    small = (~big) & (a < np.uint32(113 << 23))
    if small.any():
        s = (a[small].view(np.float32) + denorm_mask.view(np.float32)).astype(np.float32).view(np.uint32)
        res[small] = s - denorm_mask
    norm = (~big) & (~small)
    if norm.any():
        v = a[norm].astype(np.uint64)
        mant_odd = (v >> 21) & 1
        v = v + ((15 - 127) << 23 & 0xFFFFFFFF) + 0xFFFFF + mant_odd
        res[norm] = ((v & 0xFFFFFFFF) >> 21).astype(np.uint32)
    return ((res & 0xFF) | (sign >> 24)).astype(np.uint8)


def _to_f32(t) -> np.ndarray:
    if t.dtype == "BF16":
        return (t.data.astype(np.uint32) << 16).view(np.float32).reshape(t.shape)
    if t.dtype in ("F32", "F16"):
        return t.data.astype(np.float32).reshape(t.shape)
    raise ValueError(f"unsupported source dtype {t.dtype}")


def convert(hf_dir: str, out_path: str, dtype: str = "fp16") -> None:
    with open(os.path.join(hf_dir, "config.json")) as f:
        config = json.load(f)
    md = metadata_from_config(config, dtype)
    vocab_size = int(md["vocab_size"])
    tokens = load_tokens(os.path.join(hf_dir, "tokenizer.json"), vocab_size)
    files = sorted(os.path.join(hf_dir, f) for f in os.listdir(hf_dir) if f.endswith(".safetensors"))
    if not files:
        raise FileNotFoundError(f"no .safetensors files found in {hf_dir}")
    src = {}
    opened = []
    for p in files:
        yd = read_yalm(p)
        opened.append(yd)
        for k, t in yd.tensors.items():
            assert k not in src
            src[k] = t

    def conv(name):
        a = _to_f32(src[name])
        if dtype == "fp32":
            return a, "F32"
        if dtype == "fp16":
            return a.astype(np.float16), "F16"
        if dtype == "q4":  # from the fp16 conversion: |fp16 value - q4 value| <= scale / 2
            return M.q4_quantize(a.astype(np.float16).reshape(-1, a.shape[-1])), "U8"
        if dtype == "e4m3":  # from the fp16 conversion: relative error <= 2^-4 above the row's subnormals
            return M.e4m3_quantize(a.astype(np.float16).reshape(-1, a.shape[-1])), "U8"
        return f32_to_e5m2(a), "F8_E5M2"

    tensors, dtypes = {}, {}

    def put(key, arr_dt):
        tensors[key], dtypes[key] = arr_dt

    put("model.embed.weight", conv("model.embed_tokens.weight"))
    n_heads, n_kv, rot = int(md["n_heads"]), int(md["n_kv_heads"]), int(md["rotary_dim"])
    for l in range(int(md["n_layers"])):
        p, q = f"model.layers.{l}.", f"model.layers.{l}."
        put(q + "attn.norm.weight", (_to_f32(src[p + "input_layernorm.weight"]), "F32"))
        for key, hf, heads in (("wq", "q_proj", n_heads), ("wk", "k_proj", n_kv)):
            a = permute_reverse(_to_f32(src[p + f"self_attn.{hf}.weight"]), heads, rot)
            src_key = f"__perm_{key}"
            src[src_key] = _F32View(a)
            put(q + f"attn.{key}.weight", conv(src_key))
            if md.get("qkv_bias") == "1":  # the bias rows move with their weight rows
                bias = _to_f32(src[p + f"self_attn.{hf}.bias"]).reshape(-1, 1)
                put(q + f"attn.{key}.bias", (np.ascontiguousarray(permute_reverse(bias, heads, rot)[:, 0]), "F32"))
            if md.get("qk_norm") == "1":  # one head's weights, permuted as one head's rows are
                g = _to_f32(src[p + f"self_attn.{hf[0]}_norm.weight"]).reshape(-1, 1)
                put(q + f"attn.{hf[0]}_norm.weight", (np.ascontiguousarray(permute_reverse(g, 1, rot)[:, 0]), "F32"))
        put(q + "attn.wv.weight", conv(p + "self_attn.v_proj.weight"))
        if md.get("qkv_bias") == "1":
            put(q + "attn.wv.bias", (_to_f32(src[p + "self_attn.v_proj.bias"]).reshape(-1), "F32"))
        put(q + "attn.wo.weight", conv(p + "self_attn.o_proj.weight"))
        put(q + "mlp.norm.weight", (_to_f32(src[p + "post_attention_layernorm.weight"]), "F32"))
        if md["arch"] == "MixtralForCausalLM":
            put(q + "moegate.weight", conv(p + "block_sparse_moe.gate.weight"))
            for key in ("w1", "w2", "w3"):  # experts stacked along a new leading axis
                parts = [conv(p + f"block_sparse_moe.experts.{e}.{key}.weight") for e in range(int(md["n_experts"]))]
                put(q + f"mlp.{key}.weight", (np.stack([a for a, _ in parts]), parts[0][1]))
        else:
            put(q + "mlp.w1.weight", conv(p + "mlp.gate_proj.weight"))
            put(q + "mlp.w2.weight", conv(p + "mlp.down_proj.weight"))
            put(q + "mlp.w3.weight", conv(p + "mlp.up_proj.weight"))
    put("model.norm.weight", (_to_f32(src["model.norm.weight"]), "F32"))
    if config.get("tie_word_embeddings", None) == False:  # noqa: E712 (convert.py:200 semantics: absent -> tied)
        put("model.output.weight", conv("lm_head.weight"))
    blob = b"".join(t + b"\0" for t in tokens)
    put("tokenizer.tokens", (np.frombuffer(blob, np.uint8).copy(), "U8"))
    write_yalm(out_path, tensors, md, dtypes)
    for yd in opened:
        yd.close()


class _F32View:
    """Adapter so permuted f32 arrays go through the same conv() path."""

    dtype = "F32"

    def __init__(self, a):
        self.shape = a.shape
        self.data = np.ascontiguousarray(a, np.float32).reshape(-1)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("output", type=str)
    ap.add_argument("input", type=str)
    ap.add_argument("--dtype", type=str, default="fp16", choices=SUPPORTED_DTYPES)
    args = ap.parse_args(argv)
    convert(args.input, args.output, args.dtype)


if __name__ == "__main__":
    main()
