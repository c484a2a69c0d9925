"""Inputs of the mixture-of-experts prefill tests (tests/test_gpu_moe_prefill.py), defined here
so that the CPU suite (tests/test_moe_prefill_cpu.py) can check the routing margin of every one
of them -- TEST INFRASTRUCTURE.

A router logit is a GEMV on the normalised x like the classifier's, and the project's bar for
logits behind a prefilled state is 5e-3 of max|logit| (test_gpu_prefill.py, test_host.py
passkey): two logits can therefore close a gap of 2 x 5e-3, so a selection is only comparable
where consecutive logits keep PREFILL_MARGIN = 1e-2 (in the sense of moe_ref.routing_margin).
safe_tokens() builds such sequences position by position on the CPU reference.
"""
from __future__ import annotations

import functools

import numpy as np

import moe_ref as R
import oracle_py as O
from yalm_amd import models as M

PREFILL_MARGIN = 1e-2
MAX_TRIES = 64
TENSOR_SEED, TOKEN_SEED = 3, 5

_BASE = M.ModelConfig(dim=256, hidden_dim=512, head_dim=64, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=512,
                      max_seq_len=320, rope_theta=1e6, act=M.SILU, weight_dtype=M.F16)
# name -> (config, positions)
CONFIGS = {
    "e4k2": (_BASE.with_(n_experts=4, n_experts_active=2), 200),
    "e8k2": (_BASE.with_(n_experts=8, n_experts_active=2), 200),
    "e8k3-gelu-4l": (_BASE.with_(n_experts=8, n_experts_active=3, act=M.GELU, n_layers=4), 120),
    "fp8": (_BASE.with_(n_experts=4, n_experts_active=2, weight_dtype=M.F8E5M2), 90),
    "small-moe": (M.SMALL_MOE, 200),
    "spike": (_BASE.with_(n_experts=4, n_experts_active=2), 70),
}

# The range-guard model ("spike"): channel SPIKE_CH of every embedding row is 4 (the other
# channels have std 0.02, so the normalised x there is ~16 at every position), and in layer 1
# rows SPIKE_ROWS of every expert's W1 and W3 read it with weight 64: act(W1 x) * (W3 x) is
# ~1e6 there, past the f16 range (65504); the W2 columns of those rows are scaled by 2^-16 so
# that the residual stream stays of order 1. The reference (and the decode engine) keep the
# product in f32 (infer.cpp:360-375).
SPIKE_CH, SPIKE_ROWS, SPIKE_LAYER = 37, (5, 300), 1


def tensors(name):
    cfg, _ = CONFIGS[name]
    t = O.synth_host_tensors_fast(cfg, seed=TENSOR_SEED)
    if name == "spike":
        t = {k: np.array(v) for k, v in t.items()}
        t["model.embed.weight"][:, SPIKE_CH] = np.float16(4.0)
        n = M.layer_names(SPIKE_LAYER)
        for r in SPIKE_ROWS:
            t[n["w1"]][:, r, SPIKE_CH] = np.float16(64.0)
            t[n["w3"]][:, r, SPIKE_CH] = np.float16(64.0)
            t[n["w2"]][:, :, r] = (t[n["w2"]][:, :, r].astype(np.float32) * np.float32(2.0 ** -16)).astype(np.float16)
    return t


def safe_tokens(cfg, t, n, seed=TOKEN_SEED, margin=PREFILL_MARGIN, first=None):
    """(tokens int32[n], tries, min margin): at each position candidate tokens are drawn from a
    seeded generator and the first whose router logits keep `margin` at every layer is kept (a
    rejected try only rewrites that position's KV row); `first`: tokens to start from (checked
    the same way, no substitutes)."""
    ref = R.MoeRef(cfg, t)
    rng = np.random.default_rng(seed)
    out, tries, worst = [], 0, np.inf
    for pos in range(n):
        for k in range(MAX_TRIES):
            tok = int(first[pos]) if first is not None and pos < len(first) else int(rng.integers(0, cfg.vocab_size))
            tries += 1
            ref.forward(tok, pos, 0)
            m = min(R.routing_margin(ref.router_logits[l], cfg.n_experts_active) for l in range(cfg.n_layers))
            if m >= margin:
                break
            assert first is None or pos >= len(first), f"fixed token at position {pos} has routing margin {m:.2e}"
        else:
            raise AssertionError(f"no token with routing margin >= {margin} at position {pos} in {MAX_TRIES} tries")
        out.append(tok)
        worst = min(worst, m)
    return np.array(out, np.int32), tries, float(worst)


@functools.lru_cache(maxsize=None)
def sequence(name):
    """(tokens, tries, min margin) of one CONFIGS entry."""
    cfg, n = CONFIGS[name]
    return safe_tokens(cfg, tensors(name), n)


def margins(cfg, t, tokens):
    """min routing margin over (position, layer) of a given sequence on the CPU reference."""
    ref = R.MoeRef(cfg, t)
    worst = np.inf
    for pos, tok in enumerate(tokens):
        ref.forward(int(tok), pos, 0)
        worst = min(worst, min(R.routing_margin(ref.router_logits[l], cfg.n_experts_active)
                               for l in range(cfg.n_layers)))
    return float(worst)


# ---- the FFN-row inputs (yalm_moe_ffn_rows): both sides route the same x, so moe_ref.MARGIN applies
# (id, T, dim, hidden, n_experts, n_active, dtype, act, seed); seeds chosen on the CPU
# (test_moe_prefill_cpu.py) so that every row clears MARGIN
FFN_ROW_CASES = [
    ("t1-silu", 1, 512, 1536, 8, 2, M.F16, M.SILU, 1),
    ("t37-silu", 37, 512, 1536, 8, 2, M.F16, M.SILU, 2),
    ("t300-silu", 300, 512, 1536, 8, 2, M.F16, M.SILU, 3),
    ("t600-silu", 600, 512, 1536, 8, 2, M.F16, M.SILU, 4),
    ("t37-gelu", 37, 512, 1536, 8, 2, M.F16, M.GELU, 5),
    ("t300-gelu", 300, 512, 1536, 8, 2, M.F16, M.GELU, 6),
    ("e5k1", 70, 512, 1536, 5, 1, M.F16, M.SILU, 7),
    ("k-eq-e", 70, 512, 1536, 4, 4, M.F16, M.SILU, 8),
    ("fp8", 70, 1024, 2048, 8, 2, M.F8E5M2, M.SILU, 9),
]


def ffn_rows_router_inputs(case):
    """(x (T, dim) f16-exact f32, moegate): rows are redrawn (same generator) until each clears
    moe_ref.MARGIN, at most MAX_TRIES draws per row."""
    _, T, dim, _, E, K, dtype, _, seed = case
    rng = np.random.default_rng(seed)
    gate = M.encode_weights(rng.standard_normal((E, dim), dtype=np.float32) * np.float32(1.0 / np.sqrt(dim)), dtype)
    g32 = M.decode_weights(gate, dtype).astype(np.float64)
    x = np.zeros((T, dim), np.float32)
    for t in range(T):
        for _ in range(MAX_TRIES):
            v = rng.standard_normal(dim, dtype=np.float32).astype(np.float16).astype(np.float32)
            if R.routing_margin((g32 @ v.astype(np.float64)).astype(np.float32), K) >= 2 * R.MARGIN:
                break
        else:
            raise AssertionError(f"row {t}: no draw clears the margin")
        x[t] = v
    return x, gate


def ffn_rows_inputs(case):
    """(x, moegate, w1, w2, w3) of one FFN_ROW_CASES entry, weights in storage dtype."""
    _, T, dim, hidden, E, _, dtype, _, seed = case
    x, gate = ffn_rows_router_inputs(case)
    rng = np.random.default_rng(1000 + seed)

    def w(shape, s):
        return M.encode_weights(rng.standard_normal(shape, dtype=np.float32) * np.float32(s), dtype)

    w1 = w((E, hidden, dim), 1.0 / np.sqrt(dim))
    w3 = w((E, hidden, dim), 1.0 / np.sqrt(dim))
    w2 = w((E, dim, hidden), 1.0 / np.sqrt(hidden))
    return x, gate, w1, w2, w3


def tie_inputs(dim=512, E=6):
    """(x (1, dim), moegate f16): gate rows 1 and 4 identical and by far the largest logit (as
    test_gpu_moe.py test_exact_ties_lowest_index_first)."""
    rng = np.random.default_rng(21)
    x = rng.standard_normal((1, dim), dtype=np.float32).astype(np.float16).astype(np.float32)
    g = rng.standard_normal((E, dim), dtype=np.float32) * np.float32(1.0 / np.sqrt(dim))
    g[4] = x[0] * np.float32(2.0 / np.sqrt(dim))
    g[1] = g[4]
    return x, M.encode_weights(g, M.F16)


# ---- the CLI test's model (tests/test_host_moe_prefill.py): a Mixtral HF dir at prefill-capable
# dims through the project's converter. HOST_SEED was chosen on the CPU (test_moe_prefill_cpu.py)
# so that the perplexity text's positions clear moe_ref.MARGIN (perplexity runs the split form,
# whose operands carry f32-level error), the hydrated prompt's clear PREFILL_MARGIN, and no greedy
# step of the completion is a near-tie (top-2 logit gap >= 2 x 5e-3 of max|logit|).
HOST_SEED = 12
HOST_PPL_TEXT = "the sky is blue and the grass is green and the sun is yellow here we go there and back again"
HOST_PROMPT = "the sky is blue and the grass is green"
HOST_GREEDY = 8


def host_yalm(tmp_dir, seed=HOST_SEED):
    """Path of the converted fp16 .yalm under tmp_dir."""
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden as G
    import make_moe_golden as GM
    from yalm_amd import convert

    hf = dict(G.TINY_HF, hidden_size=256, intermediate_size=512, num_attention_heads=4, num_key_value_heads=2,
              max_position_embeddings=256, vocab_size=384, num_local_experts=4, num_experts_per_tok=2)
    d = os.path.join(str(tmp_dir), f"hf_moe_{seed}")
    GM.write_moe_hf_dir(d, hf=hf, seed=seed)
    out = os.path.join(str(tmp_dir), f"moe_pf_{seed}.yalm")
    convert.convert(d, out, "fp16")
    return out


def host_margins(path):
    """(min routing margin over the perplexity text, over the prompt's hydrated positions, min
    relative top-2 logit gap over the completion's greedy steps) on the CPU reference."""
    from yalm_amd.tokenizer import Tokenizer
    from yalm_amd.yalmfile import read_yalm

    yd = read_yalm(path)
    tk = Tokenizer.from_yalm(yd)
    text, prompt = tk.encode(HOST_PPL_TEXT), tk.encode(HOST_PROMPT)
    yd.close()
    cfg, t = R.yalm_tensors(path)
    m_text = margins(cfg, t, text)
    ref = R.MoeRef(cfg, t)
    m_prompt, gap = np.inf, np.inf
    for pos, tok in enumerate(prompt[:-1]):
        ref.forward(int(tok), pos, 0)
        m_prompt = min(m_prompt, min(R.routing_margin(ref.router_logits[l], cfg.n_experts_active)
                                     for l in range(cfg.n_layers)))
    tok, pos = int(prompt[-1]), len(prompt) - 1
    for _ in range(HOST_GREEDY):
        lg = ref.forward(tok, pos)
        # the decode steps route on a state behind the prefilled cache too
        m_prompt = min(m_prompt, min(R.routing_margin(ref.router_logits[l], cfg.n_experts_active)
                                     for l in range(cfg.n_layers)))
        s = np.sort(lg)[::-1]
        gap = min(gap, float((s[0] - s[1]) / np.max(np.abs(lg))))
        tok, pos = int(np.argmax(lg)), pos + 1
    return float(m_text), float(m_prompt), float(gap)
