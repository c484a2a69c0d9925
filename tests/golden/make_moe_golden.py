"""Build the committed mixture-of-experts fixtures under tests/golden/.

A tiny HF-format Mixtral dir (dim 64, hidden 128, 2 layers, 4 heads, 2 kv heads, 4 experts,
2 active, vocab 384) -> tiny_moe_fp16.yalm / tiny_moe_fp8.yalm via the REFERENCE converter
(run where the reference is present only; its outputs are committed as data fixtures).
Run from the repo root: python tests/golden/make_moe_golden.py
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from golden.make_golden import TINY_HF, tiny_vocab  # noqa: E402

TINY_MOE_HF = dict(TINY_HF, num_local_experts=4, num_experts_per_tok=2)
SEED = 7


def write_moe_hf_dir(path, hf=TINY_MOE_HF, seed=SEED):
    """Synthetic HF Mixtral checkpoint dir (config.json, tokenizer.json, model.safetensors)."""
    import torch
    from safetensors.torch import save_file

    os.makedirs(path, exist_ok=True)
    cfg = dict(hf, architectures=["MixtralForCausalLM"], tie_word_embeddings=False)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(cfg, f, indent=1)
    vocab = tiny_vocab(hf["vocab_size"])
    tok = {"model": {"type": "BPE", "byte_fallback": True, "vocab": {t: i for i, t in enumerate(vocab)}},
           "added_tokens": []}
    with open(os.path.join(path, "tokenizer.json"), "w") as f:
        json.dump(tok, f, indent=1)
    rng = np.random.Generator(np.random.PCG64(seed))
    d, h, L = hf["hidden_size"], hf["intermediate_size"], hf["num_hidden_layers"]
    nh, nkv, E = hf["num_attention_heads"], hf["num_key_value_heads"], hf["num_local_experts"]
    hd = d // nh

    def w(*shape, s=0.1):
        return torch.from_numpy((rng.standard_normal(shape) * s).astype(np.float32))

    def norm():
        return torch.from_numpy((1 + 0.1 * rng.standard_normal(d)).astype(np.float32))

    t = {"model.embed_tokens.weight": w(hf["vocab_size"], d, s=0.5)}
    for l in range(L):
        p = f"model.layers.{l}."
        t[p + "input_layernorm.weight"] = norm()
        t[p + "self_attn.q_proj.weight"] = w(nh * hd, d)
        t[p + "self_attn.k_proj.weight"] = w(nkv * hd, d)
        t[p + "self_attn.v_proj.weight"] = w(nkv * hd, d)
        t[p + "self_attn.o_proj.weight"] = w(d, nh * hd)
        t[p + "post_attention_layernorm.weight"] = norm()
        t[p + "block_sparse_moe.gate.weight"] = w(E, d, s=0.5)
        for e in range(E):
            q = p + f"block_sparse_moe.experts.{e}."
            t[q + "w1.weight"] = w(h, d)
            t[q + "w2.weight"] = w(d, h)
            t[q + "w3.weight"] = w(h, d)
    t["model.norm.weight"] = norm()
    t["lm_head.weight"] = w(hf["vocab_size"], d, s=0.5)
    save_file(t, os.path.join(path, "model.safetensors"))


def reference_moe_fixtures():
    ref = "/root/reference/convert.py"
    if not os.path.exists(ref):
        print("reference not present; keeping committed tiny_moe_*.yalm fixtures")
        return
    with tempfile.TemporaryDirectory() as td:
        hfdir = os.path.join(td, "hf_moe")
        write_moe_hf_dir(hfdir)
        for dt in ("fp16", "fp8"):
            out = os.path.join(HERE, f"tiny_moe_{dt}.yalm")
            subprocess.run([sys.executable, ref, "--dtype", dt, out, hfdir], check=True, stdout=subprocess.DEVNULL)
            print("wrote", os.path.basename(out), os.path.getsize(out))


if __name__ == "__main__":
    reference_moe_fixtures()
