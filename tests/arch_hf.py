"""Seeded tiny HF checkpoint directories for the Qwen2 (q / k / v bias) and Llama-3 (llama3
RoPE scaling) converter and host tests, written as golden/make_golden.write_hf_dir writes its
Llama one (config.json, tokenizer.json, model.safetensors), with numpy only.
TEST INFRASTRUCTURE ONLY.
"""
import json
import os

import numpy as np

from golden.make_golden import TINY_HF, tiny_vocab
from yalm_amd.yalmfile import write_yalm

QWEN2_HF = dict(TINY_HF, rope_theta=1000000.0, use_sliding_window=False, sliding_window=32)
LLAMA3_SCALING = {"factor": 8.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0,
                  "original_max_position_embeddings": 32, "rope_type": "llama3"}
LLAMA3_HF = dict(TINY_HF, rope_scaling=LLAMA3_SCALING)
# shapes with the batched-prefill path (dims multiples of 128, head_dim 64), as test_host.py's
PF_DIMS = dict(hidden_size=256, intermediate_size=512, num_attention_heads=4, num_key_value_heads=2,
               max_position_embeddings=256)
BIAS_STD = 1.0


def write_hf_dir(path, hf, arch, seed=0, tie=False, bias=False):
    """Returns the HF tensors (name -> f32 array) it wrote."""
    os.makedirs(path, exist_ok=True)
    cfg = dict(hf, architectures=[arch], tie_word_embeddings=tie)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump(cfg, f, indent=1)
    vocab = tiny_vocab(hf["vocab_size"])
    tok = {"model": {"type": "BPE", "byte_fallback": True, "vocab": {t: i for i, t in enumerate(vocab)}},
           "added_tokens": []}
    with open(os.path.join(path, "tokenizer.json"), "w") as f:
        json.dump(tok, f, indent=1)
    rng = np.random.Generator(np.random.PCG64(seed))
    d, h, L = hf["hidden_size"], hf["intermediate_size"], hf["num_hidden_layers"]
    nh, nkv = hf["num_attention_heads"], hf["num_key_value_heads"]
    hd = d // nh

    def w(*shape, s=0.1):
        return (rng.standard_normal(shape) * s).astype(np.float32)

    def norm():
        return (1 + 0.1 * rng.standard_normal(d)).astype(np.float32)

    t = {"model.embed_tokens.weight": w(hf["vocab_size"], d, s=0.5)}
    for l in range(L):
        p = f"model.layers.{l}."
        t[p + "input_layernorm.weight"] = norm()
        for name, rows in (("q_proj", nh * hd), ("k_proj", nkv * hd), ("v_proj", nkv * hd)):
            t[p + f"self_attn.{name}.weight"] = w(rows, d)
            if bias:
                t[p + f"self_attn.{name}.bias"] = w(rows, s=BIAS_STD)
        t[p + "self_attn.o_proj.weight"] = w(d, nh * hd)
        t[p + "post_attention_layernorm.weight"] = norm()
        t[p + "mlp.gate_proj.weight"] = w(h, d)
        t[p + "mlp.up_proj.weight"] = w(h, d)
        t[p + "mlp.down_proj.weight"] = w(d, h)
    t["model.norm.weight"] = norm()
    if not tie:
        t["lm_head.weight"] = w(hf["vocab_size"], d, s=0.5)
    write_yalm(os.path.join(path, "model.safetensors"), t, {})
    return t


def write_qwen2(path, hf=QWEN2_HF, seed=5, tie=False):
    return write_hf_dir(path, hf, "Qwen2ForCausalLM", seed=seed, tie=tie, bias=True)


def write_llama3(path, hf=LLAMA3_HF, seed=6, tie=True):
    return write_hf_dir(path, hf, "LlamaForCausalLM", seed=seed, tie=tie)


def load_yalm(path, context=0):
    """(config, tensors) of a .yalm file, as the decode tests load one."""
    from yalm_amd import models as M
    from yalm_amd.yalmfile import read_yalm

    yd = read_yalm(path)
    cfg = M.config_from_metadata(yd.metadata, context=context, tied="model.output.weight" not in yd.tensors)
    t = {k: np.array(v.data).reshape(v.shape) for k, v in yd.tensors.items() if k != "tokenizer.tokens"}
    yd.close()
    return cfg, t


HOST_PROMPT = "the thin is"
HOST_N = 24
# name -> (writer, hf config): the models of tests/test_host_arch.py; test_arch_cpu.py checks that
# the reference's greedy path over HOST_PROMPT has no near-tie on them
HOST_MODELS = {
    "qwen2": (write_qwen2, QWEN2_HF),
    "llama3": (write_llama3, LLAMA3_HF),
}


def host_reference(path, prompt=HOST_PROMPT, n=HOST_N):
    """What `yalm <path> -m c -t 0 -n <n> -i <prompt>` must print, by arch_ref: (prompt ids,
    tokens, smallest top-2 gap / max|logit| on the way). The CLI hydrates the prompt, then feeds
    its own tokens and stops after an end-of-sequence token."""
    import arch_ref
    from yalm_amd.tokenizer import Tokenizer
    from yalm_amd.yalmfile import read_yalm

    yd = read_yalm(path)
    enc = Tokenizer.from_yalm(yd).encode(prompt)
    yd.close()
    cfg, t = load_yalm(path)
    m = arch_ref.ArchRef(cfg, t)
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
