"""The mixture-of-experts CPU reference -- TEST INFRASTRUCTURE.

The frozen oracle (oracle/) is dense-only, so the MoE forward is composed here from pieces
that are already pinned to the reference:
  * the attention half of a block: OracleModel.block() on a dense view of the layer whose W2
    is all zeros -- the FFN then adds exactly 0, so x after the call is the post-attention
    residual (infer.cpp:250-337);
  * xb = orc_rmsnorm(x, rms_ffn) (infer.cpp:339-345);
  * router logits by oracle_py.matmul (infer.cpp:348);
  * the gate, moe_gate(), a float32 restatement of infer.cpp:100-132;
  * per selected expert oracle_py.ffn(xb, w1[e], w2[e], w3[e]) and x += xb2 * weight in
    selection order (infer.cpp:355-384).
The full forward is the embedding, these blocks, the final norm and the classifier.
"""
from __future__ import annotations

import numpy as np

import oracle_py as O
from yalm_amd import models as M

FLT_MAX = np.float32(3.4028234663852886e38)


def moe_gate(logits, n_active: int):
    """infer.cpp:100-132: K rounds of a first-maximum scan (strict '>': among equal logits the
    lowest index wins; earlier picks are masked), weights = softmax over the selected logits
    with the global max subtracted. Returns (experts int32[K], weights float32[K])."""
    x = np.asarray(logits, np.float32)
    n = x.shape[0]
    max_val = -FLT_MAX
    for j in range(n):
        if x[j] > max_val:
            max_val = x[j]
    mask = 0
    wsum = np.float32(0.0)
    experts = np.zeros(n_active, np.int32)
    for k in range(n_active):
        best = -1
        for j in range(n):
            if (mask >> j) & 1 == 0 and (best == -1 or x[j] > x[best]):
                best = j
        experts[k] = best
        wsum = np.float32(wsum + np.exp(np.float32(x[best] - max_val), dtype=np.float32))
        mask |= 1 << best
    weights = np.zeros(n_active, np.float32)
    for k in range(n_active):
        weights[k] = np.float32(np.exp(np.float32(x[experts[k]] - max_val), dtype=np.float32) / wsum)
    return experts, weights


def rmsnorm(x, w, eps):
    x = np.ascontiguousarray(x, np.float32)
    w = np.ascontiguousarray(w, np.float32)
    out = np.zeros_like(x)
    O.olib.orc_rmsnorm(O.P(out), O.P(x), O.P(w), x.shape[0], eps)
    return out


def moe_ffn(xb, moegate, w1, w2, w3, n_active, act, dtype):
    """The FFN half on a normalised xb without the residual: (sum_k weight_k * ffn_k(xb),
    experts, weights, logits), accumulated in selection order as infer.cpp:355-384 does."""
    logits = O.matmul(xb, moegate, dtype)
    experts, weights = moe_gate(logits, n_active)
    out = np.zeros(w2.shape[1], np.float32)
    for e, wt in zip(experts, weights):
        out += O.ffn(xb, w1[e], w2[e], w3[e], act, dtype) * np.float32(wt)
    return out, experts, weights, logits


class MoeRef:
    """Model + InferenceState of a mixture-of-experts model on the CPU."""

    def __init__(self, cfg: M.ModelConfig, tensors: dict):
        assert cfg.n_experts > 0
        self.cfg = cfg
        self.t = {k: np.ascontiguousarray(v) for k, v in tensors.items()}
        dense = {k: v for k, v in self.t.items() if ".moegate." not in k}
        for l in range(cfg.n_layers):
            n = M.layer_names(l)
            dense[n["w1"]] = np.ascontiguousarray(self.t[n["w1"]][0])
            dense[n["w3"]] = np.ascontiguousarray(self.t[n["w3"]][0])
            dense[n["w2"]] = np.zeros_like(self.t[n["w2"]][0])  # the dense FFN adds exactly 0
        self.om = O.OracleModel(cfg.with_(n_experts=0, n_experts_active=0), dense)
        L, K = cfg.n_layers, cfg.n_experts_active
        self.experts = np.zeros((L, K), np.int32)   # the routing of the most recent forward / block
        self.weights = np.zeros((L, K), np.float32)
        self.router_logits = np.zeros((L, cfg.n_experts), np.float32)

    @property
    def x(self):
        return self.om.x

    def embed(self, token):
        return self.om.embed(token)

    def block(self, l, pos, kv_sink, kv_pos, kv_len):
        c, n = self.cfg, M.layer_names(l)
        self.om.block(l, pos, kv_sink, kv_pos, kv_len)
        xb = rmsnorm(self.om.x, self.t[n["rms_ffn"]], c.norm_eps)
        w1, w2, w3 = self.t[n["w1"]], self.t[n["w2"]], self.t[n["w3"]]
        logits = O.matmul(xb, self.t[M.moegate_name(l)], c.weight_dtype)
        experts, weights = moe_gate(logits, c.n_experts_active)
        for e, wt in zip(experts, weights):
            xb2 = O.ffn(xb, w1[e], w2[e], w3[e], c.act, c.weight_dtype)
            self.om.x[:] = self.om.x + xb2 * np.float32(wt)
        self.experts[l], self.weights[l], self.router_logits[l] = experts, weights, logits

    def forward(self, token: int, pos: int, mode: int = 1):
        c = self.cfg
        self.om.x[:] = self.embed(token)
        kv_sink, kv_pos, kv_len = M.kv_indices(c.max_seq_len, pos)
        for l in range(c.n_layers):
            self.block(l, pos, kv_sink, kv_pos, kv_len)
        if mode != 1:
            return None
        xb = rmsnorm(self.om.x, self.t["model.norm.weight"], c.norm_eps)
        wcls = self.t.get("model.output.weight", self.t["model.embed.weight"])
        return O.matmul(xb, wcls, c.weight_dtype)

    def greedy(self, token: int, pos: int, n: int):
        out = []
        for i in range(n):
            logits = self.forward(token, pos + i)
            token = int(O.olib.orc_sample_argmax(O.P(logits), self.cfg.vocab_size))
            out.append(token)
        return out



# ---- the inputs of the GPU tests (tests/test_gpu_moe.py), defined here so that the CPU suite
# (tests/test_moe_cpu.py) can check the routing margin of every one of them: a selection the
# device could flip by rounding alone would make "experts identical" a coin toss.
MARGIN = 1e-3  # min gap between consecutive selected logits (and the first one left out) / max|logit|


def routing_margin(logits, n_active: int) -> float:
    """The smallest gap, relative to max|logit|, between consecutive logits of the descending
    order down to the first one NOT selected: both the selected set and its order are then
    safe against a relative GEMV error far below it."""
    s = -np.sort(-np.asarray(logits, np.float32))
    last = min(n_active, len(s) - 1)
    return float(np.min(s[:last] - s[1:last + 1]) / np.max(np.abs(s)))


# (id, dim, hidden, n_experts, n_active, dtype, act, seed)
FFN_CASES = [
    ("rb-f16-silu", 512, 1536, 8, 2, M.F16, M.SILU, 1),
    ("rb-f16-gelu", 512, 1536, 8, 2, M.F16, M.GELU, 2),
    ("generic-f32-silu", 64, 128, 4, 2, M.F32, M.SILU, 3),
    ("generic-f16-gelu", 64, 128, 4, 2, M.F16, M.GELU, 4),
    ("fp8-silu", 1024, 2048, 8, 2, M.F8E5M2, M.SILU, 5),
    ("fp8-gelu", 1024, 2048, 8, 2, M.F8E5M2, M.GELU, 6),
    ("k1", 512, 1536, 8, 1, M.F16, M.SILU, 7),
    ("k-eq-e", 512, 1536, 4, 4, M.F16, M.SILU, 8),
    ("k-eq-e-generic", 64, 128, 4, 4, M.F32, M.GELU, 9),
    ("e5", 512, 1536, 5, 2, M.F16, M.SILU, 10),
    # more selected experts than one expert launch addresses (8): two W1|W3 launches, W2 per expert
    ("k12-generic", 64, 128, 16, 12, M.F16, M.SILU, 13),
    ("k12-rb", 512, 1536, 16, 12, M.F16, M.SILU, 13),
    # K * hidden = 65536 floats = 256 KB: past the LDS, so W2 runs once per selected expert
    ("lds-fallback", 512, 8192, 8, 8, M.F16, M.SILU, 11),
]


def ffn_case_router_inputs(case):
    """(x, moegate) alone: the first two draws of ffn_case_inputs' generator."""
    _, dim, _, E, _, dtype, _, seed = case
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(dim, dtype=np.float32)
    gate = M.encode_weights(rng.standard_normal((E, dim), dtype=np.float32) * np.float32(1.0 / np.sqrt(dim)), dtype)
    return x, gate


def ffn_case_inputs(case):
    """(x, moegate, w1, w2, w3) of one FFN_CASES entry, weights in storage dtype."""
    _, dim, hidden, E, _, dtype, _, seed = case
    rng = np.random.default_rng(seed)

    def w(shape, s):
        return M.encode_weights(rng.standard_normal(shape, dtype=np.float32) * np.float32(s), dtype)

    x = rng.standard_normal(dim, dtype=np.float32)
    gate = w((E, dim), 1.0 / np.sqrt(dim))
    w1 = w((E, hidden, dim), 1.0 / np.sqrt(dim))
    w3 = w((E, hidden, dim), 1.0 / np.sqrt(dim))
    w2 = w((E, dim, hidden), 1.0 / np.sqrt(hidden))
    return x, gate, w1, w2, w3


# The seeds below were chosen on the CPU so that every case clears MARGIN (test_moe_cpu.py).
# yalm_block, layer by layer (id, config, seed): positions 0 .. max_seq_len + 5, through the
# sliding-window wrap
BLOCK_CASES = [
    ("tiny-f16", M.TINY_MOE.with_(max_seq_len=16), 1),
    ("tiny-f32-gelu", M.TINY_MOE.with_(weight_dtype=M.F32, act=M.GELU, max_seq_len=16), 1),
    ("tiny-fp8", M.TINY_MOE.with_(weight_dtype=M.F8E5M2, max_seq_len=16), 3),
    ("small-f16", M.SMALL_MOE.with_(max_seq_len=16), 1),
]
# full forward on the small preset (id, config, seed): positions 0 .. 40 with max_seq_len 32
FORWARD_CASES = [
    ("small-f16", M.SMALL_MOE.with_(max_seq_len=32), 5),
    ("small-fp8", M.SMALL_MOE.with_(weight_dtype=M.F8E5M2, max_seq_len=32), 8),
]
FORWARD_POSITIONS = 41
GREEDY_STEPS = 16
FIXTURE_GREEDY = 40  # greedy tokens from <s> on the committed tiny_moe_*.yalm fixtures


def next_token(tok: int, vocab: int) -> int:
    return (tok * 31 + 7) % vocab


def block_case_trace(case):
    """The reference's run of one BLOCK_CASES entry: [(pos, layer, x_in, x_out, experts, weights,
    logits)] with x_in the x both sides start the block from."""
    _, cfg, seed = case
    ref = MoeRef(cfg, O.synth_host_tensors_fast(cfg, seed=seed))
    out, tok = [], 3
    for pos in range(cfg.max_seq_len + 6):
        ref.x[:] = ref.embed(tok)
        idx = M.kv_indices(cfg.max_seq_len, pos)
        for l in range(cfg.n_layers):
            x_in = ref.x.copy()
            ref.block(l, pos, *idx)
            out.append((pos, l, x_in, ref.x.copy(), ref.experts[l].copy(), ref.weights[l].copy(),
                        ref.router_logits[l].copy()))
        tok = next_token(tok, cfg.vocab_size)
    return out


def forward_case_trace(case):
    """The reference's run of one FORWARD_CASES entry: teacher-forced tokens over
    FORWARD_POSITIONS positions -> [(tok, pos, logits, experts, weights, router logits)], then
    (on a fresh state) GREEDY_STEPS greedy tokens from token 5 at position 0 with each step's
    router logits."""
    _, cfg, seed = case
    t = O.synth_host_tensors_fast(cfg, seed=seed)
    ref = MoeRef(cfg, t)
    steps, tok = [], 1
    for pos in range(FORWARD_POSITIONS):
        lg = ref.forward(tok, pos)
        steps.append((tok, pos, lg, ref.experts.copy(), ref.weights.copy(), ref.router_logits.copy()))
        tok = next_token(tok, cfg.vocab_size)
    ref = MoeRef(cfg, t)
    greedy, glogits, tok = [], [], 5
    for i in range(GREEDY_STEPS):
        lg = ref.forward(tok, i)
        tok = int(O.olib.orc_sample_argmax(O.P(lg), cfg.vocab_size))
        greedy.append(tok)
        glogits.append((ref.router_logits.copy(), lg))
    return steps, greedy, glogits


def yalm_tensors(path, context=0):
    """(config, tensors) of a .yalm file."""
    from yalm_amd.yalmfile import read_yalm

    yd = read_yalm(path)
    cfg = M.config_from_metadata(yd.metadata, context=context, tied="model.output.weight" not in yd.tensors)
    t = {k: np.array(v.data).reshape(v.shape) for k, v in yd.tensors.items()}
    yd.close()
    return cfg, t
