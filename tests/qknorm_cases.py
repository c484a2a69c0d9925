"""The q / k norm decode cases shared by test_qknorm_cpu.py (which checks their margins on the
CPU) and test_gpu_qknorm.py (which runs them on the device): configs, seeds and the qknorm_ref
results, computed once per process. TEST INFRASTRUCTURE ONLY.

As arch_cases.py: every case runs positions 0 .. N_POS - 1 of a model with max_seq_len 16, so
the ring wraps and the sinks rotate over normed K rows. Logits are compared from position
FIRST = 1 on: at position 0 attention sees one key, its softmax is 1 and the output is V,
which the norm does not touch (test_qknorm_cpu.py::test_position_0_says_nothing).
"""
import functools

import numpy as np

import arch_cases as A
import qknorm_ref
from yalm_amd import models as M

LOGITS_BAR, BLOCK_BAR = A.LOGITS_BAR, A.BLOCK_BAR  # test_gpu_decode.py's literals
MSL, N_POS, N_GREEDY, TOKEN0 = A.MSL, A.N_POS, A.N_GREEDY, A.TOKEN0
FIRST = 1
step_token, relerr = A.step_token, A.relerr

_T = M.TINY.with_(max_seq_len=MSL, qk_norm=True)
_S = M.SMALL.with_(max_seq_len=MSL, qk_norm=True)
# test_gpu_attn_wo.py's BASE shape (head_dim 128): the fused
# attention + Wo launch runs on it
H128 = M.ModelConfig(dim=1024, hidden_dim=2048, head_dim=128, n_layers=3, n_heads=16, n_kv_heads=4, vocab_size=1536,
                     max_seq_len=MSL, rope_theta=10000.0, act=M.SILU, weight_dtype=M.F16, qk_norm=True)
Q4_BIG = A.Q4_BIG.with_(qkv_bias=False, qk_norm=True)

# name -> (config, seed)
CASES = {
    "tiny-f32": (_T.with_(weight_dtype=M.F32), 71),
    "tiny-f16": (_T, 72),
    "tiny-fp8": (_T.with_(weight_dtype=M.F8E5M2), 73),
    "tiny-q4": (_T.with_(weight_dtype=M.Q4), 174),
    "small-f16": (_S, 75),
    "small-fp8": (_S.with_(weight_dtype=M.F8E5M2), 76),
    "h128-f16": (H128, 277),
    "h128-fp8": (H128.with_(weight_dtype=M.F8E5M2), 78),
    "q4-2048": (Q4_BIG, 79),
}
H128_CASES = [k for k in CASES if k.startswith("h128-")]


@functools.lru_cache(maxsize=None)
def tensors(name):
    cfg, seed = CASES[name]
    return M.synth_host_tensors(cfg, seed=seed)


def ref(name, variant="full"):
    return qknorm_ref.QKNormRef(CASES[name][0], tensors(name), wrong=None if variant == "full" else variant)


@functools.lru_cache(maxsize=None)
def logits_run(name, variant="full"):
    """Logits of the fixed token walk at positions 0 .. N_POS - 1: array (N_POS, vocab) f64."""
    cfg = CASES[name][0]
    m = ref(name, variant)
    tok, out = TOKEN0, []
    for pos in range(N_POS):
        out.append(m.forward(tok, pos))
        tok = step_token(tok, cfg.vocab_size)
    out = np.array(out)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def blocks_run(name, variant="full"):
    """x after every layer of the same walk, each layer fed the FULL model's x before it (the
    hook tests re-synchronise per layer): (N_POS, n_layers, dim). The variant runs beside the
    full model on the full model's inputs. For "full": (that, the x fed to every layer, every
    layer's K cache row of position 0 as the f16 the reference stored: (n_layers, kv_dim))."""
    cfg = CASES[name][0]
    full = ref(name)
    var = ref(name, variant) if variant != "full" else None
    tok, out = TOKEN0, np.zeros((N_POS, cfg.n_layers, cfg.dim))
    xin = np.zeros_like(out)
    k0 = None
    for pos in range(N_POS):
        x = full.t["model.embed.weight"][tok].copy()
        kv = M.kv_indices(cfg.max_seq_len, pos)
        for l in range(cfg.n_layers):
            xin[pos, l] = x
            xf = full.block(l, x, pos, *kv)
            out[pos, l] = var.block(l, x, pos, *kv) if var is not None else xf
            x = xf
        if pos == 0:
            k0 = np.array([full.k[l][0].copy() for l in range(cfg.n_layers)])
        tok = step_token(tok, cfg.vocab_size)
    for a in (out, xin, k0):
        a.setflags(write=False)
    return (out, xin, k0) if var is None else out


@functools.lru_cache(maxsize=None)
def greedy_run(name, variant="full"):
    """(tokens, logits (N_POS, vocab)) of N_POS greedy steps from (TOKEN0, position 0)."""
    toks, lgs = ref(name, variant).greedy(TOKEN0, 0, N_POS)
    return toks, np.array(lgs)


# ---- the multi-row / speculative cases: normed SMALL models with room for the rows
SPEC = {
    "small-f16": (M.SMALL.with_(max_seq_len=64, qk_norm=True), 181),
    "small-fp8": (M.SMALL.with_(max_seq_len=64, qk_norm=True, weight_dtype=M.F8E5M2), 82),
}
SPEC_PROMPT, SPEC_GEN = A.SPEC_PROMPT, A.SPEC_GEN


@functools.lru_cache(maxsize=None)
def spec_case(name):
    """(tensors, per-position logits of the prompt, greedy continuation of SPEC_GEN + 4 tokens,
    the smallest top-2 gap / max|logit| on that path), as arch_cases.spec_case."""
    cfg, seed = SPEC[name]
    t = M.synth_host_tensors(cfg, seed=seed)
    m = qknorm_ref.QKNormRef(cfg, t)
    plog = [m.forward(tok, pos) for pos, tok in enumerate(SPEC_PROMPT)]
    seq, tok = [], int(np.argmax(plog[-1]))
    seq.append(tok)
    gaps = [np.diff(np.sort(plog[-1])[-2:])[0] / np.max(np.abs(plog[-1]))]
    for i in range(SPEC_GEN + 3):
        lg = m.forward(tok, len(SPEC_PROMPT) + i)
        gaps.append(np.diff(np.sort(lg)[-2:])[0] / np.max(np.abs(lg)))
        tok = int(np.argmax(lg))
        seq.append(tok)
    return t, np.array(plog), seq, float(min(gaps))
