"""Model-level cases at the GQA groups of the published Qwen2.5 / Qwen3 shapes (G = 7, 5) and at
head_dim 256 (G = 8), long enough to leave head mode: shared by test_gqa_cpu.py (which checks
their margins on the CPU) and test_gpu_gqa.py (which runs them on the device). Configs, seeds
and the float64 results of arch_ref.ArchRef / qknorm_ref.QKNormRef, computed once per process.
TEST INFRASTRUCTURE ONLY.

Every case has two layers, vocabulary 1024 and max_seq_len 320 (5 chunks of 64 keys: head mode up
to 256 keys, key mode from 257). The fixed token walk of arch_cases.step_token runs positions
0 .. 329: head mode, key mode from kv_len 257, the ring wrap at 320 and ten positions with
rotating sinks. The greedy path starts on the walk's cache at position GREEDY_POS = 240 and runs
SPEC_GEN = 70 tokens (the speculative runs of the GPU test). Its first GREEDY_N = 24 tokens, which
cross the head / key switch, are the ones the device greedy loop is compared with: there the
reference keeps a top-2 gap of GAP = 10 bars of max|logit|, on the rest SPEC_GAP = 2 bars (the
margin of test_gpu_spec.py). An untied random model gives near-Gaussian logits over 1024 tokens,
where a step clears 10 bars with probability ~0.9: 24 such steps are what a seed search can meet.
"""
import functools

import numpy as np

import arch_cases as A
import qknorm_ref
from yalm_amd import models as M

LOGITS_BAR = A.LOGITS_BAR  # test_gpu_decode.py's literal
MSL, N_POS, TOKEN0 = 320, 330, A.TOKEN0
GREEDY_POS, GREEDY_N = 240, 24
SPEC_GEN, SPEC_ROWS = 70, 4
ROWS_POS = (254, 255, 300)  # 4 rows each: 254 and 255 straddle the head / key switch (kv_len 256 | 257)
PF_N = 300
GAP = 10 * LOGITS_BAR  # smallest top-2 gap / max|logit| on the greedy path
SPEC_GAP = 2 * LOGITS_BAR  # ... on the rest of the speculative path
step_token, relerr = A.step_token, A.relerr

_BASE = dict(n_layers=2, vocab_size=1024, max_seq_len=MSL, rope_theta=1e6, norm_eps=1e-6, act=M.SILU)
# Qwen2.5-0.5B's attention shape: 14 / 2 heads of 64, biased, tied
G7 = M.ModelConfig(dim=896, hidden_dim=1792, head_dim=64, n_heads=14, n_kv_heads=2, qkv_bias=True, tied=True, **_BASE)
# 10 / 2 heads of 128 with the q / k norm; q_dim 1280 != dim 640
G5 = M.ModelConfig(dim=640, hidden_dim=1280, head_dim=128, n_heads=10, n_kv_heads=2, qk_norm=True, **_BASE)
# 16 / 2 heads of 256: decode only (the prefill has no head_dim 256)
G8 = M.ModelConfig(dim=512, hidden_dim=1024, head_dim=256, n_heads=16, n_kv_heads=2, **_BASE)

# name -> (config, seed); seeds searched on the CPU for a greedy path without a near-tie
# (test_gqa_cpu.py::test_greedy_paths_have_no_near_tie)
CASES = {
    "g7-hd64-bias-f16": (G7, 4),
    "g7-hd64-bias-fp8": (G7.with_(weight_dtype=M.F8E5M2), 4),
    "g7-hd64-bias-q4": (G7.with_(weight_dtype=M.Q4), 2),
    "g5-hd128-qknorm-f16": (G5, 23),
    "g5-hd128-qknorm-fp8": (G5.with_(weight_dtype=M.F8E5M2), 40),
    "g8-hd256-f16": (G8, 2),
}
ROWS_CASES = [k for k in CASES if k.startswith(("g7", "g5")) and not k.endswith("q4")]  # (q4 has no multi-row step)
PREFILL_CASES = [k for k in CASES if k.startswith(("g7", "g5"))]
FORM_CASES = PREFILL_CASES  # the cases with a bias or a norm to drop
# first compared position: a bias moves the logits at position 0; the q / k norm cannot (one key:
# the softmax is 1 and the output is V), nor does a plain model have anything to show there
FIRST = {k: (1 if "qknorm" in k else 0) for k in CASES}


@functools.lru_cache(maxsize=None)
def tensors(name):
    cfg, seed = CASES[name]
    return M.synth_host_tensors(cfg, seed=seed)


def ref(name, variant="full"):
    """The float64 model; "plain": the same tensors without the case's bias / norm."""
    cfg = CASES[name][0]
    if variant == "full":
        return qknorm_ref.QKNormRef(cfg, tensors(name))
    return qknorm_ref.QKNormRef(cfg, tensors(name), wrong="none" if cfg.qk_norm else None, use_bias=False)


@functools.lru_cache(maxsize=None)
def walk_tokens(vocab=1024):
    toks = [TOKEN0]
    for _ in range(N_POS - 1):
        toks.append(step_token(toks[-1], vocab))
    return tuple(toks)


@functools.lru_cache(maxsize=None)
def _full(name, n_pos=N_POS):
    m = ref(name)
    toks = walk_tokens()
    out, greedy = [], None
    for pos in range(n_pos):
        if pos == GREEDY_POS:  # the greedy path, on a copy of the walk's cache
            g = ref(name)
            g.k, g.v = [a.copy() for a in m.k], [a.copy() for a in m.v]
            gt, lgs = g.greedy(toks[pos], pos, SPEC_GEN)
            lgs = np.array(lgs)
            srt = np.sort(lgs, axis=1)
            greedy = (gt, (srt[:, -1] - srt[:, -2]) / np.max(np.abs(lgs), axis=1))
        out.append(m.forward(toks[pos], pos))
    out = np.array(out)
    out.setflags(write=False)
    return out, greedy


def logits_run(name, variant="full"):
    """Logits of the fixed token walk at positions 0 .. N_POS - 1: (N_POS, vocab) f64."""
    return _full(name)[0] if variant == "full" else _plain(name)


@functools.lru_cache(maxsize=None)
def _plain(name):
    m = ref(name, "plain")
    out = np.array([m.forward(tok, pos) for pos, tok in enumerate(walk_tokens())])
    out.setflags(write=False)
    return out


def greedy_run(name):
    """(the SPEC_GEN greedy tokens from the walk's token at GREEDY_POS on the walk's cache, every
    step's top-2 gap / max|logit|)."""
    return _full(name)[1]
