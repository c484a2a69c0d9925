"""The decode cases shared by test_arch_cpu.py (which checks their margins on the CPU) and
test_gpu_arch.py (which runs them on the device): configs, seeds, and the arch_ref results,
computed once per process. TEST INFRASTRUCTURE ONLY.

Every case runs positions 0 .. N_POS - 1 of a model with max_seq_len 16, so the ring wraps and
the sinks rotate (positions >= 16) with biased / rescaled K rows in the cache. Logits are
compared from the case's `first` position on: a bias changes the logits at position 0 already,
a RoPE table changes nothing there (every angle is 0) and little at the next few positions, so
the scaled cases compare from SCALED_FIRST on -- the positions at which test_arch_cpu.py shows
the rescaled model 10 bars away from the plain one.
"""
import functools

import numpy as np

import arch_ref
import gemv_cases
import gemv_ref
from yalm_amd import models as M

# the decode bars of tests/test_gpu_decode.py (it asserts these literals; DESIGN.md "Parity"):
# max|gpu - ref| / max|ref| of the logits, and of x after one layer
LOGITS_BAR, BLOCK_BAR = 1e-3, 1e-4
MSL = 16
N_POS = 22
N_GREEDY = 16
# original_max_position 32 with factor 8, low 1, high 4 puts pairs of head_dim 16 and 64 at theta
# 10000 into all three regimes (wavelengths below 8 kept, above 32 divided, between blended)
SCALING = ("llama3", 8.0, 1.0, 4.0, 32)
SCALED_FIRST = 4

_T = M.TINY.with_(max_seq_len=MSL)
_S = M.SMALL.with_(max_seq_len=MSL)
Q4_BIG = M.ModelConfig(dim=2048, hidden_dim=2048, head_dim=64, n_layers=1, n_heads=8, n_kv_heads=2, vocab_size=512,
                       max_seq_len=MSL, weight_dtype=M.Q4, qkv_bias=True)

# name -> (config, seed, first compared position)
CASES = {
    "bias-tiny-f32": (_T.with_(weight_dtype=M.F32, qkv_bias=True), 21, 0),
    "bias-tiny-f16": (_T.with_(qkv_bias=True), 22, 0),
    "bias-tiny-fp8": (_T.with_(weight_dtype=M.F8E5M2, qkv_bias=True), 23, 0),
    "bias-small-f32": (_S.with_(weight_dtype=M.F32, qkv_bias=True), 24, 0),
    "bias-small-f16": (_S.with_(qkv_bias=True), 25, 0),
    "bias-small-fp8": (_S.with_(weight_dtype=M.F8E5M2, qkv_bias=True), 26, 0),
    "bias-q4-2048": (Q4_BIG, 27, 0),
    "bias-q4-64": (_T.with_(weight_dtype=M.Q4, qkv_bias=True), 28, 0),
    # (the TINY preset's logits move by only ~5e-3 under any llama3 parameters: too close to the bar
    # to prove anything, so head_dim 16 is SMALL's dims cut into 32 heads)
    "scaled-hd16-f16": (_S.with_(head_dim=16, n_heads=32, n_kv_heads=8, rotary_dim=16, rope_scaling=SCALING), 62,
                        SCALED_FIRST),
    "scaled-small-f16": (_S.with_(rope_scaling=SCALING), 61, SCALED_FIRST),
    "both-small-f16": (_S.with_(qkv_bias=True, rope_scaling=SCALING), 33, 0),
}
BIAS_CASES = [k for k in CASES if k.startswith("bias-")]
SCALED_CASES = [k for k in CASES if k.startswith("scaled-")]
TOKEN0 = 3


def step_token(tok, vocab):
    return (tok * 31 + 7) % vocab


@functools.lru_cache(maxsize=None)
def tensors(name):
    cfg, seed, _ = CASES[name]
    return M.synth_host_tensors(cfg, seed=seed)


def variant_kw(name, variant):
    """Constructor arguments of arch_ref.ArchRef: "full", or the model with the case's form
    dropped ("plain": what a decoder without the feature computes on the same weights)."""
    if variant == "full":
        return {}
    return {"use_bias": False, "rope_scaling": None}


@functools.lru_cache(maxsize=None)
def logits_run(name, variant="full"):
    """Logits of the fixed token walk at positions 0 .. N_POS - 1: array (N_POS, vocab) f64."""
    cfg = CASES[name][0]
    m = arch_ref.ArchRef(cfg, tensors(name), **variant_kw(name, variant))
    tok, out = TOKEN0, []
    for pos in range(N_POS):
        out.append(m.forward(tok, pos))
        tok = step_token(tok, cfg.vocab_size)
    out = np.array(out)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def blocks_run(name, variant="full", with_inputs=False):
    """x after every layer of the same walk, each layer fed the FULL model's x before it (the
    hook tests re-synchronise per layer, as test_gpu_decode.py does): array (N_POS, n_layers,
    dim); with_inputs: (that, the x fed to every layer). The variant runs beside the full
    model on the full model's inputs."""
    cfg = CASES[name][0]
    full = arch_ref.ArchRef(cfg, tensors(name))
    var = arch_ref.ArchRef(cfg, tensors(name), **variant_kw(name, variant)) if variant != "full" else None
    tok, out = TOKEN0, np.zeros((N_POS, cfg.n_layers, cfg.dim))
    xin = np.zeros_like(out)
    for pos in range(N_POS):
        x = full.t["model.embed.weight"][tok].copy()
        kv = M.kv_indices(cfg.max_seq_len, pos)
        for l in range(cfg.n_layers):
            xin[pos, l] = x
            xf = full.block(l, x, pos, *kv)
            out[pos, l] = var.block(l, x, pos, *kv) if var is not None else xf
            x = xf
        tok = step_token(tok, cfg.vocab_size)
    out.setflags(write=False)
    xin.setflags(write=False)
    return (out, xin) if with_inputs else out


@functools.lru_cache(maxsize=None)
def greedy_run(name, variant="full"):
    """(tokens, logits (N_POS, vocab)) of N_POS greedy steps from (TOKEN0, position 0): past
    max_seq_len, so the greedy walk crosses the wrap too (its first N_GREEDY tokens are the
    ones the issue's "16 greedy tokens" names)."""
    cfg = CASES[name][0]
    m = arch_ref.ArchRef(cfg, tensors(name), **variant_kw(name, variant))
    toks, lgs = m.greedy(TOKEN0, 0, N_POS)
    return toks, np.array(lgs)


# ---- the multi-row / speculative cases: biased SMALL models with room for the rows
SPEC = {
    "small-f16": (M.SMALL.with_(max_seq_len=64, qkv_bias=True), 41),
    "small-fp8": (M.SMALL.with_(max_seq_len=64, qkv_bias=True, weight_dtype=M.F8E5M2), 46),
}
SPEC_PROMPT = [1, 17, 300, 5, 42, 9]
SPEC_GEN = 24


@functools.lru_cache(maxsize=None)
def spec_case(name):
    """(tensors, per-position logits of the prompt, greedy continuation of SPEC_GEN + 4 tokens,
    the smallest top-2 gap / max|logit| on that path)."""
    cfg, seed = SPEC[name]
    t = M.synth_host_tensors(cfg, seed=seed)
    m = arch_ref.ArchRef(cfg, t)
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


def relerr(a, b):
    return float(np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-30))


# ------------------------------------------------------------------ the timing hook's GLU (test_gpu_arch.py)
# One dense layer whose W1|W3 and W2 launches run the row-block kernel (dim 512, hidden 1536: whole
# f16 chunks), attention and Wo as separate launches.
GLU_CFG = M.ModelConfig(dim=512, hidden_dim=1536, head_dim=128, n_layers=1, n_heads=4, n_kv_heads=4, vocab_size=256,
                        max_seq_len=16, act=M.GELU, weight_dtype=M.F16)
GLU_SEED = 23
# gemv_ref.rel_tol of the f16 GLU and residual cases (both families keep gemv_ref.REL_TOL)
GLU_BAR = max(gemv_ref.rel_tol(c) for c in gemv_cases.CASES if c.dtype == gemv_cases.F16 and c.family in ("glu", "residual"))


@functools.lru_cache(maxsize=None)
def glu_case(act):
    """x0 and x0 + 2 W2 (act(W1 xn) * (W3 xn)), xn the RMS-normed x0, in float64 with the oracle's
    f32 GELU constants: what yalm_time_kernel ids 3 then 4 (a warm-up and one iteration each, both
    on the only layer) leave in x."""
    cfg = GLU_CFG.with_(act=act)
    t = M.synth_host_tensors(cfg, seed=GLU_SEED)
    nm = M.layer_names(0)
    w1, w2, w3 = (t[nm[k]].astype(np.float64) for k in ("w1", "w2", "w3"))
    x0 = np.random.default_rng(GLU_SEED).standard_normal(cfg.dim).astype(np.float32)
    x = x0.astype(np.float64)
    xn = x / np.sqrt(np.mean(x * x) + cfg.norm_eps) * t[nm["rms_ffn"]].astype(np.float64)
    a = w1 @ xn
    if act == M.SILU:
        h = a / (1.0 + np.exp(-a))
    else:
        h = 0.5 * a * (1.0 + np.tanh(gemv_ref.GELU_C0 * (a + gemv_ref.GELU_C1 * a * a * a)))
    return cfg, t, x0, x + 2.0 * (w2 @ (h * (w3 @ xn)))
