"""Model configuration (reference Config, model.h:41-68 / model.cpp:17-75),
.yalm tensor naming (model.cpp:347-378) and synthetic random-weight models
of real shapes (there is no network for checkpoints: see DESIGN.md).
"""

from __future__ import annotations

import dataclasses

import numpy as np

F32, F16, BF16, F8E5M2 = 0, 1, 2, 3
Q4 = 16  # YALM_Q4: 4-bit groups of 32 with an f16 scale (this engine's own format; "q4" below)
E4M3 = 17  # YALM_E4M3: OCP E4M3 codes with one f32 scale per row (this engine's own format; "e4m3" below)
GELU, SILU = 0, 1
FLT_MAX = 3.4028234663852886e38
KV_SINKS = 2  # model.h:12

DTYPE_NAMES = {"fp32": F32, "fp16": F16, "fp8": F8E5M2, "q4": Q4, "e4m3": E4M3}
DTYPE_STRINGS = {F32: "F32", F16: "F16", F8E5M2: "F8_E5M2", Q4: "U8", E4M3: "U8"}  # q4 / e4m3 rows are stored as U8 tensors
DTYPE_BYTES = {F32: 4, F16: 2, F8E5M2: 1}  # per element; q4 and e4m3 have no element size: row_bytes
Q4_GROUP = 32
E4M3_ROW_TAIL = 16  # the row's f32 scale and 12 zero bytes


def row_bytes(dtype: int, n: int) -> int:
    """Bytes of one row of n elements of a weight matrix (yalm_row_bytes). q4: n / 32 16-byte
    nibble blocks, n / 32 f16 scales, zero padding to a multiple of 16. e4m3: n codes, the f32
    scale, 12 zero bytes."""
    if dtype == E4M3:
        if n % 16:
            raise ValueError(f"e4m3: row length {n} is not a multiple of 16")
        return n + E4M3_ROW_TAIL
    if dtype == Q4:
        if n % Q4_GROUP:
            raise ValueError(f"q4: row length {n} is not a multiple of {Q4_GROUP}")
        return (n // 2 + n // 16 + 15) // 16 * 16
    return n * DTYPE_BYTES[dtype]


def matrix_bytes(dtype: int, shape) -> int:
    """Bytes of a stored weight tensor of logical shape (..., rows, n)."""
    return int(np.prod(shape[:-1])) * row_bytes(dtype, int(shape[-1]))


@dataclasses.dataclass
class ModelConfig:
    dim: int
    hidden_dim: int
    head_dim: int
    n_layers: int
    n_heads: int
    n_kv_heads: int
    vocab_size: int
    max_seq_len: int
    rope_theta: float = 10000.0
    rotary_dim: int = 0
    norm_eps: float = 1e-5
    act: int = SILU
    qkv_clip: float = FLT_MAX
    weight_dtype: int = F16
    tied: bool = False
    bos_token_id: int = 1
    eos_token_id: int = 2
    # mixture of experts (model.h:57-59): 0 = dense; else w1 / w2 / w3 are stacked per expert
    # and a router tensor (moegate) selects n_experts_active of them per token and layer
    n_experts: int = 0
    n_experts_active: int = 0
    # Qwen2 / Qwen2.5: a bias on the q, k and v projections (f32 tensors attn.{wq,wk,wv}.bias)
    qkv_bias: bool = False
    # Llama-3.1 / 3.2 "llama3" RoPE scaling: (type, factor, low_freq_factor, high_freq_factor,
    # original_max_position) with type "llama3", or None (rope_inv_freq has the rule)
    rope_scaling: tuple | None = None
    # Qwen3: an RMSNorm over each head of q and of k ahead of RoPE (f32 tensors
    # attn.{q_norm,k_norm}.weight of head_dim elements, shared by the layer's heads)
    qk_norm: bool = False

    def __post_init__(self):
        if not self.rotary_dim:
            self.rotary_dim = self.head_dim
        if self.rope_scaling is not None:
            self.rope_scaling = check_rope_scaling(self.rope_scaling)

    @property
    def q_dim(self):
        return self.n_heads * self.head_dim

    @property
    def kv_dim(self):
        return self.n_kv_heads * self.head_dim

    def with_(self, **kw) -> "ModelConfig":
        return dataclasses.replace(self, **kw)

    def weight_bytes_per_token(self) -> int:
        """Algorithmic HBM bytes read per decode token, excluding the KV cache
        (SURVEY.md §8d): every layer's weights + norms, one embedding row, the
        final norm and the classifier."""
        rb_dim, rb_q, rb_h = (row_bytes(self.weight_dtype, n) for n in (self.dim, self.q_dim, self.hidden_dim))
        per_layer = 2 * self.dim * 4
        per_layer += (self.q_dim + 2 * self.kv_dim) * rb_dim  # wq wk wv
        per_layer += self.dim * rb_q  # wo
        if self.qkv_bias:
            per_layer += (self.q_dim + 2 * self.kv_dim) * 4  # f32 q / k / v bias
        if self.qk_norm:
            per_layer += 2 * self.head_dim * 4  # f32 q / k norm weights
        if self.n_experts > 0:  # model.cpp:85-87: the router + the active experts
            per_layer += self.n_experts * rb_dim
            per_layer += self.n_experts_active * (2 * self.hidden_dim * rb_dim + self.dim * rb_h)
        else:
            per_layer += 2 * self.hidden_dim * rb_dim + self.dim * rb_h  # w1 w3, w2
        return self.n_layers * per_layer + rb_dim + self.dim * 4 + self.vocab_size * rb_dim

    def kv_bytes_per_token(self, kv_len: int) -> int:
        """fp16 K and V rows read by attention at kv_len (2 * 2 B * kv_dim per row, per layer)."""
        return self.n_layers * 2 * 2 * self.kv_dim * kv_len

    def metadata(self) -> dict:
        """__metadata__ strings as convert.py writes them (convert.py:59-81)."""
        inv = {v: k for k, v in DTYPE_NAMES.items()}
        md = {
            "arch": "MixtralForCausalLM" if self.n_experts > 0 else "MistralForCausalLM",
            "dtype": inv[self.weight_dtype],
            "dim": str(self.dim),
            "hidden_dim": str(self.hidden_dim),
            "head_dim": str(self.head_dim),
            "n_layers": str(self.n_layers),
            "n_heads": str(self.n_heads),
            "n_kv_heads": str(self.n_kv_heads),
            "vocab_size": str(self.vocab_size),
            "max_seq_len": str(self.max_seq_len),
            "bos_token_id": str(self.bos_token_id),
            "eos_token_id": str(self.eos_token_id),
            "rope_theta": str(self.rope_theta),
            "rotary_dim": str(self.rotary_dim),
            "norm_eps": str(self.norm_eps),
            "norm_type": "rmsnorm",
            "act_type": "silu" if self.act == SILU else "gelu",
        }
        if self.qkv_clip != FLT_MAX:
            md["qkv_clip"] = str(self.qkv_clip)
        if self.n_experts > 0:  # convert.py:78-80
            md["n_experts"] = str(self.n_experts)
            md["n_experts_active"] = str(self.n_experts_active)
        if self.n_experts == 0 and (self.qkv_bias or self.rope_scaling is not None):
            md["arch"] = "Qwen2ForCausalLM" if self.qkv_bias else "LlamaForCausalLM"
        if self.n_experts == 0 and self.qk_norm:
            md["arch"] = "Qwen3ForCausalLM"
        if self.qkv_bias:  # this engine's own keys (the reference reads none of these forms)
            md["qkv_bias"] = "1"
        if self.qk_norm:
            md["qk_norm"] = "1"
        if self.rope_scaling is not None:
            md.update(rope_scaling_metadata(self.rope_scaling))
        return md


ROPE_SCALING_KEYS = ("rope_scaling_type", "rope_scaling_factor", "rope_low_freq_factor", "rope_high_freq_factor",
                     "rope_original_max_position")


def check_rope_scaling(rs) -> tuple:
    """(type, factor, low, high, original_max_position) normalised, or ValueError (the rule of
    yalm_decoder_set_rope_scaling: factor >= 1, high > low > 0, original_max_position > 0)."""
    kind, factor, low, high, orig = rs
    if kind != "llama3":
        raise ValueError(f"unsupported rope scaling type {kind!r} (only 'llama3')")
    factor, low, high, orig = float(factor), float(low), float(high), int(orig)
    if not (factor >= 1.0 and high > low > 0.0 and orig > 0):
        raise ValueError("rope scaling: need factor >= 1, high_freq_factor > low_freq_factor > 0 and "
                         "original_max_position > 0")
    return (kind, factor, low, high, orig)


def rope_scaling_metadata(rs: tuple) -> dict:
    return dict(zip(ROPE_SCALING_KEYS, (str(v) for v in rs)))


def rope_scaling_from_metadata(md: dict):
    if "rope_scaling_type" not in md:
        return None
    return check_rope_scaling((md["rope_scaling_type"], float(md["rope_scaling_factor"]),
                               float(md["rope_low_freq_factor"]), float(md["rope_high_freq_factor"]),
                               int(md["rope_original_max_position"])))


def config_from_metadata(md: dict, context: int = 0, tied: bool = False) -> ModelConfig:
    """Config::from_yalm (model.cpp:17-75)."""
    dtype = md["dtype"]
    if dtype not in DTYPE_NAMES:
        raise ValueError(f"FATAL: unsupported dtype: {dtype}")
    max_seq_len = min(int(md["max_seq_len"]), 4096)  # model.cpp:33
    if context:
        max_seq_len = context
    act_str = md.get("act_type", "gelu")
    act = SILU if act_str == "silu" else GELU
    return ModelConfig(
        dim=int(md["dim"]),
        hidden_dim=int(md["hidden_dim"]),
        head_dim=int(md["head_dim"]),
        n_layers=int(md["n_layers"]),
        n_heads=int(md["n_heads"]),
        n_kv_heads=int(md["n_kv_heads"]),
        vocab_size=int(md["vocab_size"]),
        max_seq_len=max_seq_len,
        rope_theta=float(np.float32(float(md["rope_theta"]))),
        rotary_dim=int(md["rotary_dim"]),
        norm_eps=float(np.float32(float(md.get("norm_eps", "1e-5")))),
        act=act,
        qkv_clip=float(np.float32(float(md["qkv_clip"]))) if "qkv_clip" in md else FLT_MAX,
        weight_dtype=DTYPE_NAMES[dtype],
        tied=tied,
        bos_token_id=int(md.get("bos_token_id", "1")),
        eos_token_id=int(md.get("eos_token_id", "2")),
        n_experts=int(md.get("n_experts", "0")),  # model.cpp:25-29
        n_experts_active=int(md.get("n_experts_active", "0")),
        qkv_bias=md.get("qkv_bias", "0") not in ("0", "False", "false", ""),
        rope_scaling=rope_scaling_from_metadata(md),
        qk_norm=md.get("qk_norm", "0") not in ("0", "False", "false", ""),
    )


# Real shapes (HF config.json values). Weights are synthetic.
MISTRAL_7B = ModelConfig(
    dim=4096, hidden_dim=14336, head_dim=128, n_layers=32, n_heads=32, n_kv_heads=8, vocab_size=32000,
    max_seq_len=4096, rope_theta=1e6, norm_eps=1e-5, act=SILU, weight_dtype=F16, tied=False,
)
LLAMA_32_3B = ModelConfig(
    dim=3072, hidden_dim=8192, head_dim=128, n_layers=28, n_heads=24, n_kv_heads=8, vocab_size=128256,
    max_seq_len=4096, rope_theta=5e5, norm_eps=1e-5, act=SILU, weight_dtype=F16, tied=True,
)
# Qwen3-8B: the Llama block plus the q / k norm; every dimension a whole number of fp16, fp8
# and q4 chunks, an 8 KiB Wo row (the row-block GEMVs and the fused attention + Wo launch run)
QWEN3_8B = ModelConfig(
    dim=4096, hidden_dim=12288, head_dim=128, n_layers=36, n_heads=32, n_kv_heads=8, vocab_size=151936,
    max_seq_len=4096, rope_theta=1e6, norm_eps=1e-6, act=SILU, weight_dtype=F16, tied=False, qk_norm=True,
)
TINY = ModelConfig(
    dim=64, hidden_dim=128, head_dim=16, n_layers=2, n_heads=4, n_kv_heads=2, vocab_size=384, max_seq_len=64,
    rope_theta=10000.0, act=SILU, weight_dtype=F16,
)
SMALL = ModelConfig(
    dim=512, hidden_dim=1536, head_dim=64, n_layers=4, n_heads=8, n_kv_heads=2, vocab_size=2048, max_seq_len=256,
    rope_theta=10000.0, act=SILU, weight_dtype=F16,
)
# Mixture of experts: Mistral-7B dims with 8 experts, 2 active per token (Mixtral-8x7B)
MIXTRAL_8X7B = MISTRAL_7B.with_(n_experts=8, n_experts_active=2)
TINY_MOE = TINY.with_(n_experts=4, n_experts_active=2)
SMALL_MOE = SMALL.with_(n_experts=8, n_experts_active=2)
PRESETS = {"mistral-7b": MISTRAL_7B, "llama-3.2-3b": LLAMA_32_3B, "qwen3-8b": QWEN3_8B, "tiny": TINY, "small": SMALL,
           "mixtral-8x7b": MIXTRAL_8X7B, "tiny-moe": TINY_MOE, "small-moe": SMALL_MOE}


def layer_names(l: int) -> dict:
    p = f"model.layers.{l}."
    return {
        "rms_att": p + "attn.norm.weight",
        "rms_ffn": p + "mlp.norm.weight",
        "wq": p + "attn.wq.weight",
        "wk": p + "attn.wk.weight",
        "wv": p + "attn.wv.weight",
        "wo": p + "attn.wo.weight",
        "w1": p + "mlp.w1.weight",
        "w2": p + "mlp.w2.weight",
        "w3": p + "mlp.w3.weight",
    }


def bias_names(l: int) -> dict:
    """The q / k / v bias tensors of layer l (ModelConfig.qkv_bias), 1-D F32."""
    p = f"model.layers.{l}.attn."
    return {"bq": p + "wq.bias", "bk": p + "wk.bias", "bv": p + "wv.bias"}


def qk_norm_names(l: int) -> dict:
    """The q / k norm weights of layer l (ModelConfig.qk_norm), 1-D F32 of head_dim."""
    p = f"model.layers.{l}.attn."
    return {"gq": p + "q_norm.weight", "gk": p + "k_norm.weight"}


def moegate_name(l: int) -> str:
    return f"model.layers.{l}.moegate.weight"


def tensor_shapes(c: ModelConfig) -> dict:
    """name -> (shape, is_norm) in .yalm naming (model.cpp:351-377)."""
    out = {"model.embed.weight": ((c.vocab_size, c.dim), False), "model.norm.weight": ((c.dim,), True)}
    if not c.tied:
        out["model.output.weight"] = ((c.vocab_size, c.dim), False)
    for l in range(c.n_layers):
        n = layer_names(l)
        out[n["rms_att"]] = ((c.dim,), True)
        out[n["rms_ffn"]] = ((c.dim,), True)
        out[n["wq"]] = ((c.q_dim, c.dim), False)
        out[n["wk"]] = ((c.kv_dim, c.dim), False)
        out[n["wv"]] = ((c.kv_dim, c.dim), False)
        out[n["wo"]] = ((c.dim, c.q_dim), False)
        if c.qkv_bias:  # stored F32, as the norms are
            b = bias_names(l)
            out[b["bq"]] = ((c.q_dim,), True)
            out[b["bk"]] = ((c.kv_dim,), True)
            out[b["bv"]] = ((c.kv_dim,), True)
        if c.qk_norm:
            g = qk_norm_names(l)
            out[g["gq"]] = ((c.head_dim,), True)
            out[g["gk"]] = ((c.head_dim,), True)
        e = (c.n_experts,) if c.n_experts > 0 else ()  # model.cpp:160-164: stacked per expert
        if e:
            out[moegate_name(l)] = ((c.n_experts, c.dim), False)
        out[n["w1"]] = (e + (c.hidden_dim, c.dim), False)
        out[n["w2"]] = (e + (c.dim, c.hidden_dim), False)
        out[n["w3"]] = (e + (c.hidden_dim, c.dim), False)
    return out


# ---- tensor parallelism (include/yalm_hip.h "tensor parallelism") ----
def tp_shard(c: ModelConfig, name: str, rank: int, size: int):
    """Megatron split of one .yalm tensor for rank/size: ("rows"|"cols", start,
    count) of its [out][in] matrix, or None when replicated (norms, embedding).
    The classifier ("model.output.weight", or the tied embedding used as
    wcls) is split by vocabulary rows."""
    if size == 1:
        return None
    if name in ("model.output.weight", "tp.wcls"):
        n = c.vocab_size // size
        return ("rows", rank * n, n)
    kind = name.rsplit(".", 2)[-2] if name.startswith("model.layers.") else None
    if kind in ("wq",):
        n = c.q_dim // size
        return ("rows", rank * n, n)
    if kind in ("wk", "wv"):
        n = c.kv_dim // size
        return ("rows", rank * n, n)
    if kind == "wo":
        n = c.q_dim // size
        return ("cols", rank * n, n)
    if kind in ("w1", "w3"):
        n = c.hidden_dim // size
        return ("rows", rank * n, n)
    if kind == "w2":
        n = c.hidden_dim // size
        return ("cols", rank * n, n)
    return None


def tp_check(c: ModelConfig, size: int) -> None:
    if c.n_experts > 0:
        if not 1 <= c.n_experts_active <= c.n_experts <= 64:
            raise ValueError("mixture of experts: need 1 <= n_experts_active <= n_experts <= 64")
        if size > 1:
            raise ValueError("mixture-of-experts models run on one GPU (no tensor-parallel form)")
    if c.n_heads % size or c.n_kv_heads % size or c.hidden_dim % size or c.vocab_size % size:
        raise ValueError(f"tensor parallel size {size} must divide n_heads, n_kv_heads, hidden_dim and vocab_size")


def shard_array(c: ModelConfig, name: str, a, rank: int, size: int):
    """Host-side slice of a full tensor (numpy) for rank/size."""
    sh = tp_shard(c, name, rank, size)
    if sh is None:
        return a
    kind, start, n = sh
    return a[start:start + n] if kind == "rows" else a[:, start:start + n]


# ---- deterministic synthetic init (same hash on device and in the oracle) ----
WEIGHT_SCALE = 0.035  # uniform [-a, a): std 0.02, the usual init scale
NORM_SCALE, NORM_OFFSET = 0.2, 1.0
# synthetic q / k / v bias, uniform [-a, a): W . xb has a std of ~0.16 (dim 64) to ~1.3 (dim 4096)
# with these weights (trained Qwen2.5 biases reach tens), so a model run without its bias is
# unmistakably another model: its logits move by 1e-2 of their range or more at every shape tested
BIAS_SCALE = 4.0
# synthetic q / k norm weights, uniform [0.5, 2.5): trained ones are far from 1, and at the other
# norms' [0.8, 1.2) a kernel that exchanged gq and gk moved TINY's logits by only 1.3e-2
QKNORM_SCALE, QKNORM_OFFSET = 1.0, 1.5


def synth_seed(base: int, name: str) -> int:
    """Stable 64-bit seed per tensor name."""
    h = 1469598103934665603
    for ch in f"{base}:{name}".encode():
        h = ((h ^ ch) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def synth_params(name: str, is_norm: bool, peak: float = 1.0, real: "Realistic" = None, tied: bool = False):
    """(scale, offset) of a synthetic tensor. peak > 1 scales the final norm weight, so the
    logits spread peak x wider: the default model's logits have a std of ~1.2 (near-uniform
    next-token distributions). real: the realistic model's Wq / Wk gain and final-norm scale
    (its other features are patches, realistic_patch)."""
    if real is not None:
        peak = peak * real.final_norm
    if name.endswith(".bias"):  # q / k / v bias: the size of the projections' own outputs
        return BIAS_SCALE, 0.0
    if name.endswith((".attn.q_norm.weight", ".attn.k_norm.weight")):
        return QKNORM_SCALE, QKNORM_OFFSET
    if is_norm:
        k = peak if name == "model.norm.weight" else 1.0
        return NORM_SCALE * k, NORM_OFFSET * k
    if real is not None and name.endswith((".attn.wq.weight", ".attn.wk.weight")):
        return WEIGHT_SCALE * (real.qk_gain_tied if tied else real.qk_gain), 0.0
    if real is not None and name in ("model.embed.weight", "model.output.weight"):
        return WEIGHT_SCALE * (real.emb_gain_tied if tied else real.emb_gain), 0.0
    if real is not None and name.endswith((".attn.wo.weight", ".mlp.w2.weight")):
        return WEIGHT_SCALE * real.branch_gain, 0.0
    return WEIGHT_SCALE, 0.0


PEAKED = 8.0  # synth_params(peak=PEAKED): the final norm x 8 (round 5; a pure logit scale)


# ---- the realistic synthetic model ----
# Uniform random weights give hidden states no trained checkpoint has: near-uniform attention,
# no outlier channels, GLU products of order 1. This model keeps the deterministic synthetic
# weights and adds the regimes real checkpoints have (each a stated, seed-independent patch,
# applied identically to the device model and the oracle's host tensors):
#   * peaked attention softmax: Wq and Wk x qk_gain (reference infer.cpp:216-248 softmax);
#   * "massive activation" residual channels: three embedding columns set to outlier values of
#     10^2..10^3 (E5M2-exact), the W2 rows of those channels x w2_outlier_gain in every layer
#     (they keep growing), and -- as trained checkpoints have -- small norm weights there;
#   * a GLU spike: in one layer, glu_rows W1 / W3 rows read the largest outlier channel with
#     weight glu_value, so act(W1 x) * (W3 x) exceeds 65504 (the f16 range) at every position
#     (reference infer.cpp:360-375 keeps it in f32); their W2 columns x w2_spike_cols;
#   * a final-norm scale that is not a power of two (logits not an exact multiple of the
#     uniform model's);
#   * a residual stream that dominates its branches, as in trained models: the embedding and
#     classifier x emb_gain, Wo and W2 x branch_gain. With full-size branches a random-weight
#     model is chaotic (measured on the oracle, Mistral dims: a one-ulp change of ONE embedding
#     element moves the logits by 1.6e-3 at 16 layers with the other features on, 2.9e-4 for
#     the uniform model), so no two correct fp32 summation orders would agree to 1e-3 at 32
#     layers; with these gains it moves them by 4.4e-5 at 32 layers.
# Measured on the oracle (Mistral dims, 32 layers; Llama-3.2-3B dims, 28, tied): attention
# top weight median 0.89 / 0.86 in the last layers, residual outliers ~100 / 64 / 258 against
# other channels of std ~0.4 / 0.14, the layer-1 GLU product 1.6e5 / 8.4e4 at every position,
# top-1 next-token probability median 0.54 (Mistral) / 0.997 (Llama: the tied classifier
# favours the input token; log p of a uniformly random next token ~ -18).
@dataclasses.dataclass(frozen=True)
class Realistic:
    qk_gain: float = 24.0
    emb_gain: float = 16.0
    # tied models (the classifier IS the embedding): a residual dominated by a x16 embedding
    # makes the input token win by ~250 logits (measured, Llama dims); x4 leaves the layers'
    # updates a share of it (top-1 gap ~15, an unlikely token's log p ~ -18, finite in the
    # reference's f32 sample_prob), with the Wq / Wk gain raised to keep attention peaked
    emb_gain_tied: float = 4.0
    qk_gain_tied: float = 96.0
    branch_gain: float = 0.125
    final_norm: float = 4.5
    outliers: tuple = (96.0, -64.0, 256.0)
    outlier_norm: float = 1.0 / 64.0
    w2_outlier_gain: float = 8.0
    glu_value: float = 448.0
    glu_rows: int = 4
    w2_spike_cols: float = 1.0 / 4096.0


REALISTIC = Realistic()


def realistic_channels(c: ModelConfig) -> list:
    return [(c.dim * k) // 7 + 5 for k in (1, 3, 5)]


def realistic_glu_rows(c: ModelConfig, real: Realistic = REALISTIC) -> list:
    return [(c.hidden_dim * (k + 1)) // (real.glu_rows + 1) + 3 for k in range(real.glu_rows)]


def realistic_spike_layer(c: ModelConfig) -> int:
    return 1 if c.n_layers > 1 else 0


def realistic_names(c: ModelConfig) -> list:
    """The tensors realistic_patch changes."""
    out = ["model.embed.weight", "model.norm.weight"]
    for l in range(c.n_layers):
        n = layer_names(l)
        out += [n["rms_att"], n["rms_ffn"], n["w2"]]
        if l == realistic_spike_layer(c):
            out += [n["w1"], n["w3"]]
    return out


# ---- q4: symmetric 4-bit groups of 32 with a restricted f16 scale (include/yalm_hip.h) ----
# value = (u - 8) * s. The scale's low 3 mantissa bits are zero (8 significant bits), so every
# value is an exact f16: a q4 model has an exact f16 twin (q4_twin), as fp8 has.
def q4_restrict_scale(bits: np.ndarray) -> np.ndarray:
    """f16 bit patterns -> the nearest restricted ones (low 3 mantissa bits zero; ties up)."""
    return ((np.asarray(bits).astype(np.uint32) + 4) & ~np.uint32(7)).astype(np.uint16)


def q4_scales(amax: np.ndarray) -> np.ndarray:
    """Per group: the smallest restricted f16 scale s with 7 s >= amax (0 for amax 0), as f16 bits."""
    amax = np.asarray(amax, np.float64)
    with np.errstate(over="ignore"):
        h = (amax / 7.0).astype(np.float16)
    b = h.view(np.uint16).astype(np.uint32) & ~np.uint32(7)  # a restricted value at or below amax / 7
    b = np.minimum(b, 0x7BF8)  # the largest finite restricted f16 (65024)
    for _ in range(3):  # step up (8 in the bit pattern is the next restricted value) until 7 s >= amax
        s = b.astype(np.uint16).view(np.float16).astype(np.float64)
        b = np.where((7.0 * s < amax) & (b < 0x7BF8), b + 8, b)
    # ... and down while the one below still covers amax (h rounded up past a restricted value)
    lo = np.maximum(b.astype(np.int64) - 8, 0).astype(np.uint32)
    s_lo = lo.astype(np.uint16).view(np.float16).astype(np.float64)
    b = np.where((b >= 8) & (7.0 * s_lo >= amax), lo, b)
    return b.astype(np.uint16)


# nibble position (4-bit field index inside a 32-bit word) of element i of the word's 8:
# elements 2 k and 2 k + 1 sit 16 bits apart, so one mask of the word yields an adjacent pair
Q4_NIBBLE_POS = np.array([(i >> 1) + 4 * (i & 1) for i in range(8)])


def q4_pack(u: np.ndarray, scale_bits: np.ndarray) -> np.ndarray:
    """Nibbles u (rows, n) in 0..15 and f16 scale bits (rows, n / 32) -> uint8 rows
    (rows, row_bytes(Q4, n)): nibble blocks, scales, zero padding."""
    u = np.asarray(u)
    rows, n = u.shape
    rb = row_bytes(Q4, n)
    w = np.zeros((rows, n // 8), np.uint32)
    u8 = u.reshape(rows, n // 8, 8).astype(np.uint32)
    for i in range(8):
        w |= (u8[:, :, i] & 15) << np.uint32(4 * Q4_NIBBLE_POS[i])
    out = np.zeros((rows, rb), np.uint8)
    out[:, : n // 2] = w.astype("<u4").view(np.uint8).reshape(rows, n // 2)
    out[:, n // 2: n // 2 + n // 16] = np.ascontiguousarray(scale_bits, dtype="<u2").view(np.uint8).reshape(rows, n // 16)
    return out


def q4_unpack(a: np.ndarray, n: int):
    """uint8 rows (rows, row_bytes(Q4, n)) -> (nibbles (rows, n) uint8, scale bits (rows, n / 32) uint16)."""
    a = np.ascontiguousarray(a, dtype=np.uint8)
    rows = a.shape[0]
    w = np.ascontiguousarray(a[:, : n // 2]).view("<u4").astype(np.uint32)
    u = np.zeros((rows, n // 8, 8), np.uint8)
    for i in range(8):
        u[:, :, i] = (w >> np.uint32(4 * Q4_NIBBLE_POS[i])) & 15
    sb = np.ascontiguousarray(a[:, n // 2: n // 2 + n // 16]).view("<u2").astype(np.uint16)
    return u.reshape(rows, n), sb


def q4_quantize(v: np.ndarray) -> np.ndarray:
    """float matrix (rows, n), n % 32 == 0 -> q4 rows. Per group amax = max |w|, s = the smallest
    restricted f16 with 7 s >= amax, u = clip(rint(w / s), -7, 7) + 8 (all-zero group: s = 0,
    u = 8), so |w - (u - 8) s| <= s / 2 for every element."""
    v = np.asarray(v, np.float64)
    rows, n = v.shape
    g = v.reshape(rows, n // Q4_GROUP, Q4_GROUP)
    sb = q4_scales(np.abs(g).max(axis=2))
    s = sb.view(np.float16).astype(np.float64)[:, :, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(s > 0, np.rint(g / np.where(s > 0, s, 1.0)), 0.0)
    u = (np.clip(q, -7, 7) + 8).astype(np.uint8).reshape(rows, n)
    return q4_pack(u, sb)


def q4_dequantize(a: np.ndarray, n: int) -> np.ndarray:
    """q4 rows -> float32 (rows, n), exactly ((u - 8) * s; every value is an f16)."""
    u, sb = q4_unpack(a, n)
    s = sb.view(np.float16).astype(np.float32)
    return ((u.astype(np.float32) - 8.0).reshape(u.shape[0], -1, Q4_GROUP) * s[:, :, None]).reshape(u.shape[0], n)


# ---- e4m3: OCP E4M3 codes with one power-of-two f32 scale per row (include/yalm_hip.h) ----
# value = code * s, s = 2^k with -15 <= k <= 7: for exactly those k every finite code times s is
# an exact f16, so an e4m3 model has an exact f16 twin (e4m3_twin), as fp8 and q4 have.
E4M3_MAX = 448.0
E4M3_K_MIN, E4M3_K_MAX = -15, 7


def e4m3_table() -> np.ndarray:
    """The 256 code values as float32 (e4m3fn: S.EEEE.MMM, bias 7, subnormals m * 2^-9, no
    infinities, NaN at 0x7F and 0xFF)."""
    b = np.arange(256)
    e, m = (b >> 3) & 15, (b & 7).astype(np.float64)
    v = np.where(e == 0, m * 2.0 ** -9, (1.0 + m / 8.0) * 2.0 ** (e - 7.0))
    v = np.where((e == 15) & (m == 7), np.nan, v)
    return np.where(b >> 7, -v, v).astype(np.float32)


def e4m3_encode(v: np.ndarray) -> np.ndarray:
    """float -> E4M3 codes: round to nearest even, saturated to +-448 (never a NaN code)."""
    v = np.asarray(v, np.float64)
    a = np.minimum(np.abs(v), E4M3_MAX)
    _, ex = np.frexp(a)  # a = mant * 2^ex, mant in [0.5, 1)
    e = np.maximum(ex - 1, -6)  # the exponent whose 3 mantissa bits a is rounded to (subnormals: -6)
    q = np.rint(np.ldexp(a, 3 - e))  # in units of 2^(e - 3), ties to even; 0..16
    q = np.ldexp(q, e - 3)
    mant, ex = np.frexp(q)
    normal = q >= 2.0 ** -6
    code = np.where(normal, ((ex - 1 + 7) << 3) + np.rint((mant * 2.0 - 1.0) * 8.0).astype(np.int64),
                    np.rint(q * 512.0).astype(np.int64))
    return (code | np.where(np.signbit(v), 0x80, 0)).astype(np.uint8)


def e4m3_row_k(amax: np.ndarray) -> np.ndarray:
    """Per row: k = clip(ceil(log2(amax / 448)), -15, 7), 0 for amax 0 -- the smallest 2^k in range
    that puts 448 at or above amax."""
    amax = np.asarray(amax, np.float64)
    mant, ex = np.frexp(amax / E4M3_MAX)  # (exact where amax / 448 is a power of two)
    k = np.where(mant == 0.5, ex - 1, ex)
    return np.where(amax > 0, np.clip(k, E4M3_K_MIN, E4M3_K_MAX), 0).astype(np.int64)


def e4m3_pack(codes: np.ndarray, scales: np.ndarray) -> np.ndarray:
    """Codes (rows, n) uint8 and f32 scales (rows,) -> uint8 rows (rows, n + 16)."""
    codes = np.asarray(codes, np.uint8)
    rows, n = codes.shape
    out = np.zeros((rows, row_bytes(E4M3, n)), np.uint8)
    out[:, :n] = codes
    out[:, n: n + 4] = np.ascontiguousarray(scales, dtype="<f4").reshape(rows, 1).view(np.uint8)
    return out


def e4m3_unpack(a: np.ndarray, n: int):
    """uint8 rows (rows, n + 16) -> (codes (rows, n) uint8, scales (rows,) float32)."""
    a = np.ascontiguousarray(a, dtype=np.uint8)
    return a[:, :n], np.ascontiguousarray(a[:, n: n + 4]).view("<f4").astype(np.float32).reshape(-1)


def e4m3_quantize(v: np.ndarray) -> np.ndarray:
    """float matrix (rows, n), n % 16 == 0 -> e4m3 rows. Per row amax = max |w|, k = e4m3_row_k(amax),
    codes = w / 2^k rounded to nearest even onto E4M3 and saturated to +-448 (which only bites
    when amax > 448 * 2^7 = 57344)."""
    v = np.asarray(v, np.float64)
    k = e4m3_row_k(np.abs(v).max(axis=1))
    return e4m3_pack(e4m3_encode(np.ldexp(v, -k[:, None])), np.ldexp(1.0, k).astype(np.float32))


def e4m3_dequantize(a: np.ndarray, n: int) -> np.ndarray:
    """e4m3 rows -> float32 (rows, n): code * s (exact for the quantiser's scales)."""
    codes, s = e4m3_unpack(a, n)
    return (e4m3_table()[codes].astype(np.float64) * s.astype(np.float64)[:, None]).astype(np.float32)


def e4m3_twin(cfg: ModelConfig, tensors: dict):
    """The exact f16 twin of an e4m3 model: (f16 config, tensors with every e4m3 matrix as float16)."""
    out = {}
    for name, (shape, is_norm) in tensor_shapes(cfg).items():
        out[name] = tensors[name] if is_norm else decode_weights(tensors[name], E4M3, shape).astype(np.float16)
    return cfg.with_(weight_dtype=F16), out


def q4_twin(cfg: ModelConfig, tensors: dict):
    """The exact f16 twin of a q4 model: (f16 config, tensors with every q4 matrix as float16)."""
    out = {}
    for name, (shape, is_norm) in tensor_shapes(cfg).items():
        out[name] = tensors[name] if is_norm else decode_weights(tensors[name], Q4, shape).astype(np.float16)
    return cfg.with_(weight_dtype=F16), out


def decode_weights(a: np.ndarray, dtype: int, shape=None) -> np.ndarray:
    """Stored weights (f32 / f16 / E5M2 bytes / q4 rows / e4m3 rows) -> float32, exactly. q4 and
    e4m3 need the logical shape (rows, n)."""
    if dtype == F8E5M2:
        return e5m2_to_f32(a)
    if dtype == E4M3:
        return e4m3_dequantize(a.reshape(-1, a.shape[-1]), int(shape[-1])).reshape(shape)
    if dtype == Q4:
        return q4_dequantize(a.reshape(-1, a.shape[-1]), int(shape[-1])).reshape(shape)
    return a.astype(np.float32)


def encode_weights(v: np.ndarray, dtype: int) -> np.ndarray:
    """float32 -> stored weights: f16 round to nearest even; E5M2 through f16, then round
    to nearest even on the byte (the initialiser's rule, synth_array); q4: q4_quantize on the
    matrix (rows, n); e4m3: e4m3_quantize on the matrix."""
    v = np.asarray(v, np.float32)
    if dtype == F32:
        return v
    if dtype == E4M3:
        return e4m3_quantize(v.reshape(-1, v.shape[-1]))
    if dtype == Q4:
        return q4_quantize(v.reshape(-1, v.shape[-1]))
    h16 = v.astype(np.float16)
    if dtype == F16:
        return h16
    hb = h16.view(np.uint16).astype(np.uint32)
    return ((hb + 0x7F + ((hb >> 8) & 1)) >> 8).astype(np.uint8)


def realistic_patch(c: ModelConfig, name: str, a: np.ndarray, real: Realistic = REALISTIC) -> None:
    """Patch one synthetic tensor (numpy, storage dtype, in place) into the realistic model."""
    ch = realistic_channels(c)
    wt = c.weight_dtype
    if name == "model.embed.weight":
        for cc, v in zip(ch, real.outliers):
            a[:, cc] = encode_weights(np.full(a.shape[0], v, np.float32), wt)
        return
    if name == "model.norm.weight" or name.endswith((".attn.norm.weight", ".mlp.norm.weight")):
        a[ch] = (a[ch] * np.float32(real.outlier_norm)).astype(np.float32)
        return
    if not name.startswith("model.layers."):
        return
    l = int(name.split(".")[2])
    n = layer_names(l)
    spike = l == realistic_spike_layer(c)
    rows = realistic_glu_rows(c, real)
    if name == n["w2"]:
        a[ch, :] = encode_weights(decode_weights(a[ch, :], wt) * np.float32(real.w2_outlier_gain), wt)
        if spike:
            a[:, rows] = encode_weights(decode_weights(a[:, rows], wt) * np.float32(real.w2_spike_cols), wt)
    elif spike and name in (n["w1"], n["w3"]):
        for r in rows:
            a[r, ch[2]] = encode_weights(np.array([real.glu_value], np.float32), wt)[0]


def apply_realistic(c: ModelConfig, tensors: dict, real: Realistic = REALISTIC) -> dict:
    for name in realistic_names(c):
        realistic_patch(c, name, tensors[name], real)
    return tensors


def _splitmix64(x):
    x = (x + np.uint64(0x9E3779B97F4A7C15)).astype(np.uint64)
    x = ((x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)).astype(np.uint64)
    x = ((x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)).astype(np.uint64)
    return x ^ (x >> np.uint64(31))


def synth_array(n: int, dtype: int, seed: int, scale: float, offset: float = 0.0) -> np.ndarray:
    """numpy twin of the device/oracle initialiser (small sizes only)."""
    with np.errstate(over="ignore"):
        i = np.arange(n, dtype=np.uint64)
        h = _splitmix64(np.uint64(seed) ^ (i * np.uint64(0xD1B54A32D192ED03)))
    s = ((h >> np.uint64(40)).astype(np.int64) - 8388608).astype(np.float32)
    k = np.float32(scale) * np.float32(1.0 / 8388608.0)
    if dtype == F32:
        # fmaf(s, k, offset): exact product (24-bit x 24-bit fits in f64), one rounding
        return (s.astype(np.float64) * np.float64(k) + np.float64(np.float32(offset))).astype(np.float32)
    v = (s * k).astype(np.float32)
    h16 = v.astype(np.float16)
    if dtype == F16:
        return h16
    hb = h16.view(np.uint16).astype(np.uint32)
    return ((hb + 0x7F + ((hb >> 8) & 1)) >> 8).astype(np.uint8)


def synth_q4_array(rows: int, n: int, seed: int, scale: float) -> np.ndarray:
    """numpy twin of yalm_synth_q4: nibble byte i of the tensor (row-major, nibble bytes only) is
    bits 40..47 of hash i; every scale is the restricted f16 nearest scale / 7; padding zero."""
    with np.errstate(over="ignore"):
        i = np.arange(rows * (n // 2), dtype=np.uint64)
        h = _splitmix64(np.uint64(seed) ^ (i * np.uint64(0xD1B54A32D192ED03)))
    out = np.zeros((rows, row_bytes(Q4, n)), np.uint8)
    out[:, : n // 2] = ((h >> np.uint64(40)) & np.uint64(0xFF)).astype(np.uint8).reshape(rows, n // 2)
    sb = q4_restrict_scale((np.float32(scale) / np.float32(7.0)).astype(np.float16).view(np.uint16))
    out[:, n // 2: n // 2 + n // 16] = np.full((rows, n // 32), sb, "<u2").view(np.uint8).reshape(rows, n // 16)
    return out


def synth_e4m3_scale(scale: float) -> np.float32:
    """Every synthetic row's scale: 2^k for the smallest k in [-15, 7] with 448 * 2^k >= scale (7 if none)."""
    k = E4M3_K_MIN
    while k < E4M3_K_MAX and np.float32(np.ldexp(np.float32(E4M3_MAX), k)) < np.float32(scale):
        k += 1
    return np.float32(np.ldexp(1.0, k))


def synth_e4m3_array(rows: int, n: int, seed: int, scale: float) -> np.ndarray:
    """numpy twin of yalm_synth_e4m3: code byte i of the tensor (row-major, code bytes only) is bits
    40..47 of hash i, the NaN codes made finite by clearing their lowest bit (0x7F -> 0x7E, 0xFF ->
    0xFE); every row's scale is synth_e4m3_scale(scale); padding zero."""
    with np.errstate(over="ignore"):
        i = np.arange(rows * n, dtype=np.uint64)
        h = _splitmix64(np.uint64(seed) ^ (i * np.uint64(0xD1B54A32D192ED03)))
    c = ((h >> np.uint64(40)) & np.uint64(0xFF)).astype(np.uint8)
    c = np.where((c & 0x7F) == 0x7F, c & 0xFE, c).astype(np.uint8)
    return e4m3_pack(c.reshape(rows, n), np.full(rows, synth_e4m3_scale(scale), np.float32))


def synth_host_tensors(c: ModelConfig, seed: int = 1, peak: float = 1.0, real: Realistic = None) -> dict:
    """All tensors of a synthetic model as numpy arrays (norms f32, weights in
    c.weight_dtype storage: f32 / f16 / uint8 E5M2 bits / uint8 q4 rows / uint8 e4m3 rows); real:
    the realistic model (not for q4 or e4m3: its patches address elements of the stored array)."""
    if real is not None and c.weight_dtype == Q4:
        raise ValueError("the realistic synthetic model has no q4 form: quantise its f16 tensors (q4_quantize)")
    if real is not None and c.weight_dtype == E4M3:
        raise ValueError("the realistic synthetic model has no e4m3 form: quantise its f16 tensors (e4m3_quantize)")
    out = {}
    for name, (shape, is_norm) in tensor_shapes(c).items():
        scale, offset = synth_params(name, is_norm, peak, real, c.tied)
        dt = F32 if is_norm else c.weight_dtype
        n = int(np.prod(shape))
        if dt == Q4:
            out[name] = synth_q4_array(n // shape[-1], shape[-1], synth_seed(seed, name), scale)
        elif dt == E4M3:
            out[name] = synth_e4m3_array(n // shape[-1], shape[-1], synth_seed(seed, name), scale)
        else:
            out[name] = synth_array(n, dt, synth_seed(seed, name), scale, offset).reshape(shape)
    return apply_realistic(c, out, real) if real is not None else out


def e5m2_to_f32(b: np.ndarray) -> np.ndarray:
    """Exact: the E5M2 byte b is the f16 with bits b << 8."""
    return (b.astype(np.uint16) << 8).view(np.float16).astype(np.float32)


def rope_inv_freq(c: ModelConfig) -> np.ndarray:
    """The reference's compiled RoPE frequencies (infer.cpp:203 under -ffast-math:
    powf(theta, -(j * (1 / rotary_dim))), the form the decoder uploads); numpy's float32
    power stands in for glibc powf (may differ by an ulp: analysis tools only)."""
    j = np.arange(0, c.head_dim, 2).astype(np.float32)
    rinv = np.float32(1.0) / np.float32(c.rotary_dim)
    f = np.power(np.float32(c.rope_theta), -(j * rinv).astype(np.float32)).astype(np.float32)
    f[j >= c.rotary_dim] = 0.0
    if c.rope_scaling is None:
        return f.astype(np.float32)
    return llama3_scale(f, c.rope_scaling)


def llama3_scale(f: np.ndarray, rs: tuple) -> np.ndarray:
    """The "llama3" rule on f32 pair frequencies f (yalm_decoder_set_rope_scaling): with the
    wavelength w = 2 pi / f, w < orig / high keeps f, w > orig / low gives f / factor, between
    them s = (orig / w - low) / (high - low) blends (1 - s) f / factor + s f; in double, rounded
    once to f32."""
    _, factor, low, high, orig = check_rope_scaling(rs)
    f = np.asarray(f, np.float32).astype(np.float64)
    with np.errstate(divide="ignore"):
        w = 2.0 * np.pi / f
    s = (orig / w - low) / (high - low)
    out = np.where(w < orig / high, f, np.where(w > orig / low, f / factor, (1.0 - s) * f / factor + s * f))
    return np.where(f == 0.0, 0.0, out).astype(np.float32)


def kv_indices(max_seq_len: int, pos: int):
    """infer.cpp:483-485"""
    kv_sink = KV_SINKS if pos >= max_seq_len else 0
    kv_pos = kv_sink + (pos - kv_sink) % (max_seq_len - kv_sink)
    kv_len = max_seq_len if pos >= max_seq_len else pos + 1
    return kv_sink, kv_pos, kv_len


def nbytes_model(c: ModelConfig) -> int:
    tot = 0
    for _, (shape, is_norm) in tensor_shapes(c).items():
        tot += int(np.prod(shape)) * 4 if is_norm else matrix_bytes(c.weight_dtype, shape)
    return tot

