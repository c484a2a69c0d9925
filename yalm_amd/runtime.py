"""ctypes binding of libyalm_hip.so (C ABI: include/yalm_hip.h).

Python mirror of the reference's device-facing API: ``DeviceModel`` is
``Model::cuda()`` (model.cpp:380-394, weights uploaded once, tied embedding
not duplicated), ``Decoder`` is ``InferenceState::cuda()`` + ``Model::forward``
(model.cpp:323-345, 396-407). Every call goes through the HIP library; there
is no CPU path here (the CPU oracle lives in oracle/, test-only).
"""

from __future__ import annotations

import ctypes
import os

import numpy as np

from . import models as M

HERE = os.path.dirname(os.path.abspath(__file__))
# YALM_LIB: another build of the same ABI (A/B timing of two revisions, tools/build_ab_lib.sh)
LIB_PATH = os.environ.get("YALM_LIB") or os.path.join(HERE, "libyalm_hip.so")

if not os.path.exists(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} is missing: build it with `make -C {os.path.dirname(HERE)}` "
        "(or __graft_entry__.build()). There is no CPU fallback."
    )

lib = ctypes.CDLL(LIB_PATH)

c_void_p = ctypes.c_void_p
c_int = ctypes.c_int
c_float = ctypes.c_float
c_size_t = ctypes.c_size_t


class Config(ctypes.Structure):
    """yalm_config (model.h:41-68)."""

    _fields_ = [
        ("dim", c_int),
        ("hidden_dim", c_int),
        ("head_dim", c_int),
        ("n_layers", c_int),
        ("n_heads", c_int),
        ("n_kv_heads", c_int),
        ("vocab_size", c_int),
        ("max_seq_len", c_int),
        ("rope_theta", c_float),
        ("rotary_dim", c_int),
        ("norm_eps", c_float),
        ("act", c_int),
        ("qkv_clip", c_float),
        ("weight_dtype", c_int),
    ]

    @classmethod
    def from_model(cls, c: M.ModelConfig) -> "Config":
        return cls(
            c.dim, c.hidden_dim, c.head_dim, c.n_layers, c.n_heads, c.n_kv_heads, c.vocab_size, c.max_seq_len,
            c.rope_theta, c.rotary_dim, c.norm_eps, c.act, c.qkv_clip, c.weight_dtype,
        )


class Sampling(ctypes.Structure):
    """yalm_sampling: temperature > 0, top_k >= 0 (0 = off), top_p in (0, 1] (1 = off)."""

    _fields_ = [("temperature", c_float), ("top_k", c_int), ("top_p", c_float)]


class Spec(ctypes.Structure):
    """yalm_spec: rows 2..4, 1 <= ngram_min <= ngram_max <= 4, the draft_stream hook."""

    _fields_ = [("rows", c_int), ("ngram_max", c_int), ("ngram_min", c_int), ("draft_stream", c_void_p),
                ("draft_stream_len", c_int)]


class SpecModel(ctypes.Structure):
    """yalm_spec_model: rows 2..4, the draft_stream hook."""

    _fields_ = [("rows", c_int), ("draft_stream", c_void_p), ("draft_stream_len", c_int)]


class SpecStats(ctypes.Structure):
    """yalm_spec_stats."""

    _fields_ = [("spec_steps", c_int), ("accepted_drafts", c_int), ("plain_steps", c_int),
                ("launches_per_step", c_int)]


class BatchStats(ctypes.Structure):
    """yalm_batch_stats."""

    _fields_ = [("launches_per_step", c_int)]


class GemvGeometry(ctypes.Structure):
    """yalm_gemv_geometry: the plan of one single-row GEMV launch."""

    _fields_ = [(n, c_int) for n in ("generic", "threads", "unroll", "nb", "rows", "ngl_min", "ngl_max", "xregs")] + [
        ("lds", c_size_t)]


class GemvArgs(ctypes.Structure):
    """yalm_gemv_args: one single-row GEMV launch on host arrays (yalm_gemv_one)."""

    _fields_ = ([(n, c_int) for n in ("dtype", "policy", "kind", "n", "d", "norm", "act")] + [("eps", c_float)]
                + [(n, c_int) for n in ("threads", "unroll", "wpc", "cus", "rows")]
                + [(n, c_void_p) for n in ("x", "normw", "w", "w3", "wq", "wk", "wv", "out", "base")]
                + [(n, c_int) for n in ("out_len", "n_heads", "n_kv_heads", "head_dim", "kv_sink", "kv_pos",
                                        "cache_rows")]
                + [("qkv_clip", c_float)]
                + [(n, c_void_p) for n in ("rope", "rope_sink", "kcache", "vcache", "q_out", "raw")]
                + [("q_len", c_int), ("raw_len", c_int)] + [(n, c_void_p) for n in ("bq", "bk", "bv")])


class RopeScaling(ctypes.Structure):
    """yalm_rope_scaling: type 0 none, 1 llama3."""

    _fields_ = [("type", c_int), ("factor", c_float), ("low_freq_factor", c_float), ("high_freq_factor", c_float),
                ("original_max_position", c_int)]

    @classmethod
    def from_model(cls, rs) -> "RopeScaling":
        """From ModelConfig.rope_scaling (None: type 0)."""
        if rs is None:
            return cls(0, 1.0, 1.0, 4.0, 1)
        _, factor, low, high, orig = M.check_rope_scaling(rs)
        return cls(1, factor, low, high, orig)


class BlockWeights(ctypes.Structure):
    _fields_ = [(n, c_void_p) for n in ("rms_att", "rms_ffn", "wq", "wk", "wv", "wo", "w1", "w2", "w3",
                                        "key_cache", "value_cache")]


class ModelWeights(ctypes.Structure):
    _fields_ = [("token_embedding", c_void_p), ("rms_final", c_void_p), ("wcls", c_void_p),
                ("blocks", ctypes.POINTER(BlockWeights))]


def _sig(name, restype, argtypes):
    if os.environ.get("YALM_LIB") and not hasattr(lib, name):
        return None  # an older build under A/B timing may lack newer entry points
    f = getattr(lib, name)
    f.restype = restype
    f.argtypes = argtypes
    return f


_sig("yalm_last_error", ctypes.c_char_p, [])
_sig("yalm_set_device", c_int, [c_int])
_sig("yalm_upload", c_void_p, [c_void_p, c_size_t])
_sig("yalm_alloc", c_void_p, [c_size_t])
_sig("yalm_download", c_int, [c_void_p, c_void_p, c_size_t])
_sig("yalm_register_host", c_int, [c_void_p, c_size_t])
_sig("yalm_unregister_host", c_int, [c_void_p])
_sig("yalm_free", c_int, [c_void_p])
_sig("yalm_stream_create", c_int, [ctypes.POINTER(c_void_p)])
_sig("yalm_stream_destroy", c_int, [c_void_p])
_sig("yalm_stream_sync", c_int, [c_void_p])
_sig("yalm_synth", c_int, [c_void_p, c_size_t, c_int, ctypes.c_uint64, c_float, c_float, c_void_p])
_sig("yalm_row_bytes", c_size_t, [c_int, c_int])
_sig("yalm_synth_q4", c_int, [c_void_p, c_size_t, c_int, ctypes.c_uint64, c_float, c_void_p])
_sig("yalm_synth_e4m3", c_int, [c_void_p, c_size_t, c_int, ctypes.c_uint64, c_float, c_void_p])
_sig("yalm_decoder_create", c_int, [ctypes.POINTER(Config), ctypes.POINTER(ModelWeights), c_void_p,
                                     ctypes.POINTER(c_void_p)])
_sig("yalm_decoder_create_moe", c_int, [ctypes.POINTER(Config), c_void_p, ctypes.POINTER(ModelWeights), c_void_p,
                                         c_void_p, ctypes.POINTER(c_void_p)])
_sig("yalm_moe_routing", c_int, [c_void_p, c_void_p, c_void_p])
_sig("yalm_moe_ffn", c_int, [c_void_p] * 8 + [c_int] * 6)
_sig("yalm_prefill_routing", c_int, [c_void_p, c_void_p, c_void_p])
_sig("yalm_moe_gemm_f16", c_int, [c_void_p] * 4 + [c_int] * 4)
_sig("yalm_moe_ffn_rows", c_int, [c_void_p] * 4 + [c_int] + [c_void_p] * 4 + [c_int] * 6)
_sig("yalm_decoder_destroy", c_int, [c_void_p])
_sig("yalm_forward", c_int, [c_void_p, c_int, c_int, c_int, c_void_p])
_sig("yalm_generate_greedy", c_int, [c_void_p, c_int, c_int, c_int, c_void_p])
_sig("yalm_enqueue_greedy", c_int, [c_void_p, c_int])
_sig("yalm_generate_sampled", c_int, [c_void_p, c_int, c_int, c_int, ctypes.POINTER(Sampling), c_void_p, c_void_p])
_sig("yalm_sample", c_int, [c_void_p, c_int, ctypes.POINTER(Sampling), c_void_p, c_int, c_void_p, c_void_p, c_void_p])
_sig("yalm_device_step", c_int, [c_void_p, ctypes.POINTER(c_int), ctypes.POINTER(c_int)])
_sig("yalm_device_tokens", c_int, [c_void_p, c_void_p, c_int, ctypes.POINTER(c_int)])
_sig("yalm_block", c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int])
_sig("yalm_get_x", c_int, [c_void_p, c_void_p])
_sig("yalm_set_x", c_int, [c_void_p, c_void_p])
_sig("yalm_get_logits", c_int, [c_void_p, c_void_p])
_sig("yalm_time_kernel", c_int, [c_void_p, c_int, c_int, ctypes.POINTER(c_float)])
_sig("yalm_kernel_name", ctypes.c_char_p, [c_void_p, c_int])
_sig("yalm_set_gemv_config", c_int, [c_void_p, c_int, c_int, c_int, c_int])
_sig("yalm_stream_envelope", c_int, [ctypes.c_size_t, c_int, ctypes.POINTER(c_float)])
_sig("yalm_decoder_attn_wo", c_int, [c_void_p])
_sig("yalm_attn_wo_trace", c_int, [c_void_p, c_void_p, ctypes.c_size_t, ctypes.POINTER(c_int), ctypes.POINTER(c_int)])
_sig("yalm_matmul", c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int])
_sig("yalm_mha", c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int])
_sig("yalm_argmax", c_int, [c_void_p, c_int, c_int, ctypes.POINTER(c_int)])
_sig("yalm_ffn", c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int])
_sig("yalm_prefill", c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p])
_sig("yalm_tp_unique_id", c_int, [c_void_p])
_sig("yalm_decoder_create_tp", c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p])
_sig("yalm_tp_ipc_alloc", c_int, [c_void_p, c_int, c_void_p, ctypes.POINTER(c_void_p), c_void_p])
_sig("yalm_stream_create_cu_part", c_int, [c_int, c_int, ctypes.POINTER(c_void_p)])
_sig("yalm_decoder_set_launch", c_int, [c_void_p, c_int])
_sig("yalm_decoder_create_tp_ipc", c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p])
_sig("yalm_copy_2d", c_int, [c_void_p, ctypes.c_size_t, c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t])
_sig("yalm_prefill_time", c_int, [c_void_p, c_int, c_int, ctypes.POINTER(c_float)])
_sig("yalm_prefill_info", c_int, [c_void_p, ctypes.POINTER(c_int), ctypes.POINTER(c_int)])
_sig("yalm_set_prefill_precision", c_int, [c_void_p, c_int])
_sig("yalm_gemm_f16", c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int])
_sig("yalm_attn_prefill", c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int])
_sig("yalm_attn_prefill_rows", c_int, [c_void_p, c_int] + [c_void_p] * 3 + [c_int] * 7)
_sig("yalm_set_prefill_forms", c_int, [c_void_p, ctypes.c_char_p])
_sig("yalm_graph_kernels", c_int, [c_void_p, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int)])
_sig("yalm_attn_wo_plan", c_int, [c_void_p, c_int, ctypes.POINTER(c_int), ctypes.POINTER(c_int)])
_sig("yalm_forward_rows", c_int, [c_void_p, c_void_p, c_int, c_int, c_void_p])
_sig("yalm_generate_speculative", c_int, [c_void_p, c_int, c_int, c_int, ctypes.POINTER(Spec), c_void_p, c_int, c_void_p,
                                           ctypes.POINTER(SpecStats)])
_sig("yalm_spec_draft", c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p])
_sig("yalm_generate_speculative_sampled", c_int, [c_void_p, c_int, c_int, c_int, ctypes.POINTER(Spec),
                                                   ctypes.POINTER(Sampling), c_void_p, c_void_p, c_int, c_void_p,
                                                   ctypes.POINTER(SpecStats)])
_sig("yalm_generate_speculative_model", c_int, [c_void_p, c_void_p, c_int, c_int, c_int, ctypes.POINTER(SpecModel),
                                                 ctypes.POINTER(Sampling), c_void_p, c_void_p,
                                                 ctypes.POINTER(SpecStats)])
_sig("yalm_decoder_get_stream", c_int, [c_void_p, ctypes.POINTER(c_void_p)])
_sig("yalm_spec_sample_rows", c_int, [c_void_p, c_int, c_int, ctypes.POINTER(Sampling), c_void_p, c_void_p, c_void_p,
                                       c_void_p, ctypes.POINTER(c_int)])
_sig("yalm_decoder_set_rope_scaling", c_int, [c_void_p, ctypes.POINTER(RopeScaling)])
_sig("yalm_decoder_get_inv_freq", c_int, [c_void_p, c_void_p])
_sig("yalm_decoder_set_qkv_bias", c_int, [c_void_p, c_void_p, c_void_p, c_void_p])
_sig("yalm_decoder_set_qk_norm", c_int, [c_void_p, c_void_p, c_void_p])
_sig("yalm_rows_plan", c_int, [c_int] * 5 + [ctypes.POINTER(c_int)] * 4 + [ctypes.POINTER(c_size_t)])
_sig("yalm_matmul_rows", c_int, [c_void_p] * 5 + [c_float] + [c_int] * 8)
_sig("yalm_gemv_plan", c_int, [c_int] * 11 + [ctypes.POINTER(GemvGeometry)])
_sig("yalm_gemv_one", c_int, [ctypes.POINTER(GemvArgs)])
_sig("yalm_batch_create", c_int, [c_void_p, c_int, ctypes.POINTER(c_void_p)])
_sig("yalm_batch_destroy", c_int, [c_void_p])
_sig("yalm_batch_load", c_int, [c_void_p, c_int, c_int])
_sig("yalm_batch_forward", c_int, [c_void_p, c_void_p, c_void_p, c_void_p])
_sig("yalm_batch_generate_greedy", c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, ctypes.POINTER(BatchStats)])
_sig("yalm_batch_generate_sampled", c_int, [c_void_p, c_void_p, c_void_p, c_int, ctypes.POINTER(Sampling), c_void_p,
                                             c_void_p, ctypes.POINTER(BatchStats)])
_sig("yalm_batch_state", c_int, [c_void_p, c_void_p, c_void_p])
_sig("yalm_batch_set_launch", c_int, [c_void_p, c_int])
_sig("yalm_batch_buffers", c_int, [c_void_p, c_int, c_int] + [ctypes.POINTER(c_void_p)] * 3)

EXPORTED = [
    "yalm_last_error", "yalm_set_device", "yalm_upload", "yalm_alloc", "yalm_download", "yalm_register_host",
    "yalm_unregister_host", "yalm_free", "yalm_stream_create", "yalm_stream_destroy", "yalm_stream_sync",
    "yalm_synth", "yalm_decoder_create", "yalm_decoder_destroy", "yalm_forward", "yalm_generate_greedy",
    "yalm_enqueue_greedy", "yalm_device_step", "yalm_device_tokens", "yalm_block", "yalm_get_x", "yalm_set_x", "yalm_get_logits",
    "yalm_time_kernel", "yalm_kernel_name", "yalm_set_gemv_config", "yalm_matmul", "yalm_mha", "yalm_ffn",
    "yalm_prefill", "yalm_prefill_time", "yalm_gemm_f16", "yalm_attn_prefill", "yalm_tp_unique_id",
    "yalm_decoder_create_tp", "yalm_copy_2d", "yalm_tp_ipc_alloc", "yalm_decoder_create_tp_ipc",
    "yalm_decoder_attn_wo", "yalm_attn_wo_trace", "yalm_stream_envelope",
    "yalm_argmax", "yalm_set_prefill_forms", "yalm_attn_wo_plan", "yalm_graph_kernels",
    "yalm_stream_create_cu_part", "yalm_decoder_set_launch", "yalm_prefill_info", "yalm_set_prefill_precision",
    "yalm_decoder_create_moe", "yalm_moe_routing", "yalm_moe_ffn",
    "yalm_prefill_routing", "yalm_moe_gemm_f16", "yalm_moe_ffn_rows",
    "yalm_generate_sampled", "yalm_sample",
    "yalm_row_bytes", "yalm_synth_q4", "yalm_synth_e4m3",
    "yalm_forward_rows", "yalm_generate_speculative", "yalm_spec_draft",
    "yalm_generate_speculative_sampled", "yalm_spec_sample_rows",
    "yalm_decoder_set_rope_scaling", "yalm_decoder_get_inv_freq", "yalm_decoder_set_qkv_bias",
    "yalm_decoder_set_qk_norm",
    "yalm_rows_plan", "yalm_matmul_rows",
    "yalm_gemv_plan", "yalm_gemv_one",
    "yalm_attn_prefill_rows",
    "yalm_batch_create", "yalm_batch_destroy", "yalm_batch_load", "yalm_batch_forward",
    "yalm_batch_generate_greedy", "yalm_batch_generate_sampled", "yalm_batch_state", "yalm_batch_set_launch",
    "yalm_batch_buffers",
    "yalm_generate_speculative_model", "yalm_decoder_get_stream",
]
BATCH_ATTN_PER_SEQ = 1  # yalm_batch_set_launch
BATCH_GUARD_BYTES = 256  # YALM_BATCH_GUARD_BYTES
BATCH_MAX_SEQ = 4
PREFILL_FAST, PREFILL_SPLIT = 0, 1  # yalm_set_prefill_precision

HYDRATE_KV_CACHE, OUTPUT_LOGITS = 0, 1
# yalm_decoder_set_launch flags (include/yalm_hip.h)
LAUNCH_EAGER, LAUNCH_SYNC, LAUNCH_SEPARATE_ATTN_WO = 1, 2, 4
TP_HANDLE_BYTES = 128  # YALM_TP_HANDLE_BYTES: IPC handle + GPU UUID + CU mask


class YalmError(RuntimeError):
    pass


def check(rc: int) -> None:
    if rc != 0:
        raise YalmError(f"yalm error {rc}: {lib.yalm_last_error().decode()}")


def _ptr(a: np.ndarray) -> int:
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data


# ------------------------------------------------------------- kernel-level test API
def matmul(x: np.ndarray, w: np.ndarray, dtype: int) -> np.ndarray:
    """matmul_cuda (infer.cu:937-957): W (d, n) @ x (n,). q4 / e4m3: w is the uint8 rows
    (d, row_bytes(dtype, n)) of models.q4_quantize / e4m3_quantize; n is x's length."""
    d, n = w.shape
    x = np.ascontiguousarray(x, dtype=np.float32)
    if dtype in (M.Q4, M.E4M3):
        n = x.size
        assert w.dtype == np.uint8 and w.shape[1] == M.row_bytes(dtype, n)
    w = np.ascontiguousarray(w)
    out = np.zeros(d, np.float32)
    check(lib.yalm_matmul(_ptr(out), _ptr(x), _ptr(w), n, d, dtype))
    return out


def mha(kb, vb, q, head_dim, kv_len, max_seq_len, n_heads, n_kv_heads, att_init=None):
    """mha_cuda (infer.cu:890-935): returns (xout, att)."""
    kb = np.ascontiguousarray(kb, dtype=np.float16).view(np.uint16)
    vb = np.ascontiguousarray(vb, dtype=np.float16).view(np.uint16)
    q = np.ascontiguousarray(q, dtype=np.float32)
    xout = np.zeros(n_heads * head_dim, np.float32)
    att = np.zeros(n_heads * max_seq_len, np.float32) if att_init is None else np.array(att_init, np.float32)
    check(lib.yalm_mha(_ptr(xout), _ptr(att), _ptr(kb), _ptr(vb), _ptr(q), head_dim, kv_len, max_seq_len, n_heads,
                       n_kv_heads))
    return xout, att


def argmax(logits: np.ndarray, n_shards: int = 1) -> int:
    """Device argmax (sampler.cpp:27-38 semantics) of host logits; n_shards > 1:
    the tensor-parallel per-shard pairs + pick."""
    lg = np.ascontiguousarray(logits, dtype=np.float32)
    out = c_int()
    check(lib.yalm_argmax(_ptr(lg), lg.size, n_shards, ctypes.byref(out)))
    return out.value


def sample(logits: np.ndarray, temperature: float, top_k: int = 0, top_p: float = 1.0, uniforms=(0.5,)):
    """Device sampling of host logits (yalm_sample: one launch of the decode loop's sampling
    kernel per uniform). Returns (tokens, kept, q): the token and the kept-set size of every
    draw (int32 arrays) and the uint64 fixed-point weights q_i the kernel used."""
    lg = np.ascontiguousarray(logits, dtype=np.float32)
    u = np.ascontiguousarray(uniforms, dtype=np.float32).reshape(-1)
    s = Sampling(temperature, top_k, top_p)
    tokens = np.zeros(max(u.size, 1), np.int32)
    kept = np.zeros(max(u.size, 1), np.int32)
    q = np.zeros(max(lg.size, 1), np.uint64)
    check(lib.yalm_sample(_ptr(lg), lg.size, ctypes.byref(s), _ptr(u), u.size, _ptr(tokens), _ptr(kept), _ptr(q)))
    return tokens[:u.size], kept[:u.size], q[:lg.size]


def spec_draft(history, rows: int, ngram_max: int = 3, ngram_min: int = 1) -> list:
    """The n-gram drafter of the speculative loop on a given history (yalm_spec_draft: one launch
    of its kernel): the rows - 1 drafts, -1 for none."""
    h = np.ascontiguousarray(history, dtype=np.int32).reshape(-1)
    out = np.full(4, -1, np.int32)
    check(lib.yalm_spec_draft(_ptr(h) if h.size else None, h.size, rows, ngram_max, ngram_min, _ptr(out)))
    return out[:rows - 1].tolist()


def spec_sample_rows(logits, temperature: float, top_k: int = 0, top_p: float = 1.0, uniforms=(0.5,), drafts=()):
    """The draw and the accept launch of a sampled speculative step (yalm_spec_sample_rows) on
    host logits (T, n), row t drawn with uniforms[t], drafts[k - 1] the draft of row k (-1 =
    none). Returns (drawn, kept, a): every row's token and kept-set size (int32 arrays) and the
    number of tokens the step yields."""
    lg = np.ascontiguousarray(logits, dtype=np.float32)
    assert lg.ndim == 2
    T, n = lg.shape
    u = np.ascontiguousarray(uniforms, dtype=np.float32).reshape(-1)
    dr = np.full(4, -1, np.int32)
    d = np.asarray(drafts, np.int32).reshape(-1)
    if u.size != T or d.size != max(T - 1, 0):
        raise ValueError(f"spec_sample_rows: {T} rows need {T} uniforms and {T - 1} drafts")
    dr[:d.size] = d
    s = Sampling(temperature, top_k, top_p)
    drawn, kept, a = np.zeros(4, np.int32), np.zeros(4, np.int32), c_int()
    check(lib.yalm_spec_sample_rows(_ptr(lg), n, T, ctypes.byref(s), _ptr(u), _ptr(dr), _ptr(drawn), _ptr(kept),
                                    ctypes.byref(a)))
    return drawn[:T], kept[:T], a.value


def ffn(x, w1, w2, w3, act: int, dtype: int) -> np.ndarray:
    """ffn_cuda (infer.cu:959-1007). q4 / e4m3: w1 / w3 (hidden_dim, row_bytes(dtype, dim)) and w2
    (dim, row_bytes(dtype, hidden_dim)) uint8 rows."""
    hidden_dim, dim = w1.shape
    x = np.ascontiguousarray(x, dtype=np.float32)
    if dtype in (M.Q4, M.E4M3):
        dim = x.size
        assert w2.shape == (dim, M.row_bytes(dtype, hidden_dim)) and w1.shape[1] == M.row_bytes(dtype, dim)
    w1, w2, w3 = (np.ascontiguousarray(a) for a in (w1, w2, w3))
    out = np.zeros(dim, np.float32)
    check(lib.yalm_ffn(_ptr(out), _ptr(x), _ptr(w1), _ptr(w2), _ptr(w3), hidden_dim, dim, act, dtype))
    return out


def moe_ffn(x, moegate, w1, w2, w3, n_active: int, act: int, dtype: int):
    """yalm_moe_ffn: the router on x, then the selected experts' FFN summed with their
    weights (no norm, no residual). moegate (E, dim); w1 / w3 (E, hidden, dim), w2 (E, dim,
    hidden). Returns (xout, experts, weights), the routing in selection order."""
    n_experts, hidden_dim, dim = w1.shape
    x = np.ascontiguousarray(x, dtype=np.float32)
    moegate, w1, w2, w3 = (np.ascontiguousarray(a) for a in (moegate, w1, w2, w3))
    out = np.zeros(dim, np.float32)
    experts = np.zeros(max(n_active, 1), np.int32)
    weights = np.zeros(max(n_active, 1), np.float32)
    check(lib.yalm_moe_ffn(_ptr(out), _ptr(experts), _ptr(weights), _ptr(x), _ptr(moegate), _ptr(w1), _ptr(w2),
                           _ptr(w3), n_experts, n_active, hidden_dim, dim, act, dtype))
    return out, experts[:n_active], weights[:n_active]


def moe_ffn_rows(x, moegate, w1, w2, w3, n_active: int, act: int, dtype: int):
    """yalm_moe_ffn_rows: the batched router and the grouped expert FFN of the prefill on
    T already-normalised rows x (T, dim) (no norm, no residual). Returns (xout (T, dim),
    experts (T, K), weights (T, K)), the routing in selection order."""
    n_experts, hidden_dim, dim = w1.shape
    x = np.ascontiguousarray(x, dtype=np.float32)
    T = x.shape[0]
    moegate, w1, w2, w3 = (np.ascontiguousarray(a) for a in (moegate, w1, w2, w3))
    out = np.zeros((T, dim), np.float32)
    experts = np.zeros((T, max(n_active, 1)), np.int32)
    weights = np.zeros((T, max(n_active, 1)), np.float32)
    check(lib.yalm_moe_ffn_rows(_ptr(out), _ptr(experts), _ptr(weights), _ptr(x), T, _ptr(moegate), _ptr(w1),
                                _ptr(w2), _ptr(w3), n_experts, n_active, hidden_dim, dim, act, dtype))
    return out, experts, weights


def stream_envelope(nbytes: int, iters: int = 16) -> float:
    """ms of one pure HBM read pass over nbytes (yalm_stream_envelope)."""
    ms = c_float()
    check(lib.yalm_stream_envelope(nbytes, iters, ctypes.byref(ms)))
    return ms.value


class Stream:
    """A decoder stream; cu_part = (part, n_parts): restricted to CU block `part` of
    n_parts (yalm_stream_create_cu_part), so n_parts rank processes on one GPU run on
    disjoint CUs -- the one-GPU rehearsal of tensor parallelism."""

    def __init__(self, cu_part=None, borrowed=None):
        """borrowed: the handle of a stream someone else owns (Decoder.get_stream); close() leaves it."""
        self.owned = borrowed is None
        if borrowed is not None:
            self.h = c_void_p(borrowed)
            return
        self.h = c_void_p()
        if cu_part is None:
            check(lib.yalm_stream_create(ctypes.byref(self.h)))
        else:
            check(lib.yalm_stream_create_cu_part(cu_part[0], cu_part[1], ctypes.byref(self.h)))

    def close(self):
        if self.h and self.owned:
            check(lib.yalm_stream_destroy(self.h))
        self.h = None


def tp_unique_id() -> bytes:
    """RCCL unique id for yalm_decoder_create_tp (rank 0 makes it, all ranks use it)."""
    buf = ctypes.create_string_buffer(128)
    check(lib.yalm_tp_unique_id(buf))
    return buf.raw


def gemm_f16(a: np.ndarray, w: np.ndarray) -> np.ndarray:
    """MFMA GEMM of the prefill path: a (M, K) f16 @ w (N, K)^T f16 -> (M, N) f32."""
    a = np.ascontiguousarray(a, dtype=np.float16)
    w = np.ascontiguousarray(w, dtype=np.float16)
    (M, K), N = a.shape, w.shape[0]
    c = np.zeros((M, N), np.float32)
    check(lib.yalm_gemm_f16(_ptr(c), _ptr(a), _ptr(w), M, N, K))
    return c


def moe_gemm_f16(a: np.ndarray, w: np.ndarray, expert_of_row: np.ndarray) -> np.ndarray:
    """The grouped MFMA GEMM of the mixture-of-experts prefill: row r of a (M, K) f16 against
    w[expert_of_row[r]] of w (E, N, K) f16 -> (M, N) f32 (yalm_moe_gemm_f16)."""
    a = np.ascontiguousarray(a, dtype=np.float16)
    w = np.ascontiguousarray(w, dtype=np.float16)
    e = np.ascontiguousarray(expert_of_row, dtype=np.int32)
    (M, K), (E, N, _) = a.shape, w.shape
    c = np.zeros((M, N), np.float32)
    check(lib.yalm_moe_gemm_f16(_ptr(c), _ptr(a), _ptr(w), _ptr(e), M, N, K, E))
    return c


def set_gemm_forms(spec: str = "") -> None:
    """The prefill GEMM forms of the gemm_f16 test hook (yalm_set_prefill_forms(NULL, spec))."""
    check(lib.yalm_set_prefill_forms(None, spec.encode() if spec else None))


def attn_wo_plan(cfg: M.ModelConfig, slots: int):
    """(fused?, key splits, grid) of the fused attention + Wo launch for cfg at `slots`
    co-resident workgroups (yalm_attn_wo_plan: host arithmetic, no device)."""
    c = Config.from_model(cfg)
    s, g = c_int(), c_int()
    ok = lib.yalm_attn_wo_plan(ctypes.byref(c), slots, ctypes.byref(s), ctypes.byref(g))
    return bool(ok), s.value, g.value


ROWS_STORE, ROWS_RESIDUAL, ROWS_GLU = 0, 1, 2  # yalm_matmul_rows epilogues


def rows_plan(dtype: int, n: int, n_groups: int, T: int, cus: int = 0) -> dict:
    """kseg, nseg, gpw, blocks and lds of one multi-row GEMV launch (yalm_rows_plan: host
    arithmetic; cus = 0 asks for this device's CU count)."""
    k, s, g, b, l = c_int(), c_int(), c_int(), c_int(), c_size_t()
    check(lib.yalm_rows_plan(dtype, n, n_groups, T, cus, ctypes.byref(k), ctypes.byref(s), ctypes.byref(g),
                             ctypes.byref(b), ctypes.byref(l)))
    return dict(kseg=k.value, nseg=s.value, gpw=g.value, blocks=b.value, lds=l.value)


def matmul_rows(out, x, w, dtype: int, epilogue: int = ROWS_STORE, w3=None, normw=None, eps: float = 0.0,
                act: int = M.SILU, n=None) -> np.ndarray:
    """One multi-row GEMV launch (yalm_matmul_rows): x (T, xstride) f32, w (d, n) stored weights
    (w3 too for ROWS_GLU), out (T, ostride) f32 as it stands before the launch (sentinels, the
    residual's start). n defaults to w's row length (e4m3: w is the uint8 rows (d, n + 16)).
    Returns the whole out after the launch; the argument is not written."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.array(out, dtype=np.float32, order="C")
    w = np.ascontiguousarray(w)
    d = w.shape[0]
    if dtype == M.E4M3:
        n = w.shape[1] - M.E4M3_ROW_TAIL if n is None else n
        assert w.dtype == np.uint8 and w.shape[1] == M.row_bytes(M.E4M3, n)
    n = w.shape[1] if n is None else n
    w3 = None if w3 is None else np.ascontiguousarray(w3)
    normw = None if normw is None else np.ascontiguousarray(normw, dtype=np.float32)
    T = x.shape[0]
    assert x.ndim == 2 and out.ndim == 2 and out.shape[0] == T
    assert w3 is None or w3.shape == w.shape
    assert normw is None or normw.size == n
    check(lib.yalm_matmul_rows(_ptr(out), _ptr(x), _ptr(w), None if w3 is None else _ptr(w3),
                               None if normw is None else _ptr(normw), eps, T, n, d, x.shape[1], out.shape[1], dtype,
                               epilogue, act))
    return out


# yalm_gemv_plan / yalm_gemv_one policies and launch kinds (include/yalm_hip.h, decoder.h GK_*)
GEMV_STORE1, GEMV_STORE2, GEMV_RESIDUAL, GEMV_ADDTO, GEMV_GLU, GEMV_QKV, GEMV_QKVB, GEMV_QKVN = range(8)
GK_QKV, GK_WO, GK_GLU, GK_W2, GK_CLS = range(5)


def gemv_plan(dtype: int, policy: int, kind: int, n: int, n_groups: int, norm: bool = False, threads: int = 0,
              unroll: int = 0, wpc: int = 0, cus: int = 0, rows: int = -1) -> dict:
    """The geometry of one single-row GEMV launch (yalm_gemv_plan, the function the launcher itself
    calls; host arithmetic with cus > 0): generic, threads, unroll, nb, rows, ngl_min, ngl_max,
    xregs, lds."""
    g = GemvGeometry()
    check(lib.yalm_gemv_plan(dtype, policy, kind, n, n_groups, int(norm), threads, unroll, wpc, cus, rows,
                             ctypes.byref(g)))
    return {k: int(getattr(g, k)) for k, _ in GemvGeometry._fields_}


def gemv_one(dtype: int, policy: int, kind: int, n: int, x, *, d: int = 0, w=None, w3=None, out=None, base=None,
             normw=None, eps: float = 0.0, act: int = M.SILU, threads: int = 0, unroll: int = 0, wpc: int = 0,
             cus: int = 0, rows: int = -1, wq=None, wk=None, wv=None, n_heads: int = 0, n_kv_heads: int = 0,
             head_dim: int = 0, qkv_clip: float = 0.0, kv_sink: int = 0, kv_pos: int = 0, rope=None, rope_sink=None,
             kcache=None, vcache=None, q_out=None, raw=None, bq=None, bk=None, bv=None) -> dict:
    """One single-row GEMV launch through the decoder's launcher (yalm_gemv_one). Weights are the
    stored rows (q4 / e4m3: uint8 rows of row_bytes(dtype, n)). out / q_out / raw (f32) and kcache /
    vcache (uint16, (cache_rows, kv_dim)) are given as they stand before the launch and returned
    whole, as copies, in a dict under the same names; the arguments are not written."""
    keep = []

    def arr(a, dt, copy=False):
        if a is None:
            return None, None
        a = np.array(a, dtype=dt, order="C") if copy else np.ascontiguousarray(a, dtype=dt)
        keep.append(a)
        return a, _ptr(a)

    def wts(a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        rb = lib.yalm_row_bytes(dtype, n)  # (0: a row length the library refuses)
        assert rb == 0 or a.nbytes == a.shape[0] * rb, "weights: rows of row_bytes(dtype, n)"
        keep.append(a)
        return _ptr(a)

    a = GemvArgs()
    a.dtype, a.policy, a.kind, a.n, a.d, a.norm, a.act, a.eps = dtype, policy, kind, n, d, int(normw is not None), act, eps
    a.threads, a.unroll, a.wpc, a.cus, a.rows = threads, unroll, wpc, cus, rows
    x = np.ascontiguousarray(x, dtype=np.float32)
    assert x.size == n and (normw is None or np.asarray(normw).size == n)
    a.x = _ptr(x)
    a.normw = arr(normw, np.float32)[1]
    a.w, a.w3, a.wq, a.wk, a.wv = wts(w), wts(w3), wts(wq), wts(wk), wts(wv)
    res = {}
    res["out"], a.out = arr(out, np.float32, copy=True)
    a.out_len = 0 if out is None else res["out"].size
    assert base is None or np.asarray(base).size == d
    a.base = arr(base, np.float32)[1]
    a.n_heads, a.n_kv_heads, a.head_dim, a.kv_sink, a.kv_pos = n_heads, n_kv_heads, head_dim, kv_sink, kv_pos
    a.qkv_clip = qkv_clip
    for name, v in (("rope", rope), ("rope_sink", rope_sink)):
        assert v is None or np.asarray(v).size == head_dim
        setattr(a, name, arr(v, np.float32)[1])
    kv_dim, q_dim = n_kv_heads * head_dim, n_heads * head_dim
    res["kcache"], a.kcache = arr(kcache, np.uint16, copy=True)
    res["vcache"], a.vcache = arr(vcache, np.uint16, copy=True)
    a.cache_rows = 0
    if kcache is not None and kv_dim > 0:
        assert vcache is not None and res["kcache"].size == res["vcache"].size and res["kcache"].size % kv_dim == 0
        a.cache_rows = res["kcache"].size // kv_dim
    res["q_out"], a.q_out = arr(q_out, np.float32, copy=True)
    a.q_len = 0 if q_out is None else res["q_out"].size
    res["raw"], a.raw = arr(raw, np.float32, copy=True)
    a.raw_len = 0 if raw is None else res["raw"].size
    for name, v, ln in (("bq", bq, q_dim), ("bk", bk, kv_dim), ("bv", bv, kv_dim)):
        assert v is None or np.asarray(v).size == ln
        setattr(a, name, arr(v, np.float32)[1])
    check(lib.yalm_gemv_one(ctypes.byref(a)))
    return {k: v for k, v in res.items() if v is not None}


def attn_prefill(q, kc, vc, T, pos0, n_heads, n_kv_heads, head_dim) -> np.ndarray:
    """Causal GQA prefill attention: q (T, n_heads*D) f16, kc/vc (pos0+T, n_kv*D) f16 -> (T, n_heads*D) f16."""
    q = np.ascontiguousarray(q, dtype=np.float16)
    kc = np.ascontiguousarray(kc, dtype=np.float16)
    vc = np.ascontiguousarray(vc, dtype=np.float16)
    o = np.zeros((T, n_heads * head_dim), np.float16)
    check(lib.yalm_attn_prefill(_ptr(o), _ptr(q), _ptr(kc), _ptr(vc), T, pos0, n_heads, n_kv_heads, head_dim))
    return o


def attn_prefill_rows(o, q, kc, vc, T, pos0, n_heads, n_kv_heads, head_dim, split=False) -> np.ndarray:
    """yalm_attn_prefill_rows: the decoder's prefill attention launch with a decoder's buffers.
    kc / vc (cache_rows >= pos0 + T, n_kv*D) f16 with whatever lies past pos0 + T; o (o_rows >= T, W)
    f16 is uploaded as it comes and returned whole (a copy); W = n_heads*D, doubled when split:
    q (T, W) and o are then [hi | lo]."""
    W = n_heads * head_dim * (2 if split else 1)
    q = np.ascontiguousarray(q, dtype=np.float16)
    kc = np.ascontiguousarray(kc, dtype=np.float16)
    vc = np.ascontiguousarray(vc, dtype=np.float16)
    o = np.array(o, dtype=np.float16, order="C", copy=True)
    if q.shape != (T, W) or o.ndim != 2 or o.shape[1] != W or kc.shape != vc.shape or kc.ndim != 2 \
            or kc.shape[1] != n_kv_heads * head_dim:
        raise ValueError("attn_prefill_rows: q (T, W), o (o_rows, W), kc / vc (cache_rows, n_kv*D)")
    check(lib.yalm_attn_prefill_rows(_ptr(o), o.shape[0], _ptr(q), _ptr(kc), _ptr(vc), kc.shape[0], T, pos0, n_heads,
                                     n_kv_heads, head_dim, int(bool(split))))
    return o


# ------------------------------------------------------------- model + decoder
class DeviceModel:
    """Model::cuda(): all weights resident in HBM (one allocation per tensor;
    a tied classifier aliases the embedding instead of a second upload, unlike
    model.cpp:388/393)."""

    def __init__(self, cfg: M.ModelConfig):
        self.cfg = cfg
        self.ptrs: dict = {}
        self._owned: list = []
        self.tp = (0, 1)

    def _alloc(self, nbytes: int) -> int:
        p = lib.yalm_alloc(nbytes)
        if not p:
            raise YalmError(lib.yalm_last_error().decode())
        self._owned.append(p)
        return p

    @classmethod
    def from_arrays(cls, cfg: M.ModelConfig, tensors: dict, tp=(0, 1)) -> "DeviceModel":
        """Upload host tensors (numpy; names as in .yalm). tp = (rank, size):
        upload only this rank's shards (models.tp_shard)."""
        rank, size = tp
        M.tp_check(cfg, size)
        if cfg.weight_dtype == M.Q4 and size > 1:
            raise ValueError("q4 models run on one GPU (no tensor-parallel form)")
        if cfg.weight_dtype == M.E4M3 and size > 1:
            raise ValueError("e4m3 models run on one GPU (no tensor-parallel form)")
        self = cls(cfg)
        self.tp = tp
        items = dict(tensors)
        if size > 1 and cfg.tied:
            items["tp.wcls"] = tensors["model.embed.weight"]
        for name in list(M.tensor_shapes(cfg)) + (["tp.wcls"] if size > 1 and cfg.tied else []):
            a = np.ascontiguousarray(M.shard_array(cfg, name, items[name], rank, size))
            p = lib.yalm_upload(a.ctypes.data, a.nbytes)
            if not p:
                raise YalmError(lib.yalm_last_error().decode())
            self._owned.append(p)
            self.ptrs[name] = p
        return self

    @classmethod
    def from_yalm(cls, path: str, context: int = 0) -> "DeviceModel":
        from .yalmfile import read_yalm

        yd = read_yalm(path)
        tied = "model.output.weight" not in yd.tensors
        cfg = M.config_from_metadata(yd.metadata, context, tied)
        arrays = {k: t.data for k, t in yd.tensors.items()}
        try:
            return cls.from_arrays(cfg, arrays)
        finally:
            arrays.clear()
            yd.close()

    @classmethod
    def synthetic(cls, cfg: M.ModelConfig, seed: int = 1, tp=(0, 1), peak: float = 1.0,
                  real: "M.Realistic" = None) -> "DeviceModel":
        """Random-weight model of cfg's shape generated directly in HBM with the
        deterministic hash shared with the oracle (no PCIe upload). tp = (rank,
        size): keep only this rank's shards — each sharded tensor is generated
        whole in a scratch buffer and its slice copied out (yalm_copy_2d), so
        every rank holds exactly the slices of the same full model. real: the
        realistic model (models.Realistic): each patched tensor is downloaded, patched
        by models.realistic_patch and uploaded again (single GPU only)."""
        rank, size = tp
        M.tp_check(cfg, size)
        if real is not None and size > 1:
            raise ValueError("the realistic synthetic model is built for one GPU (tp size 1)")
        self = cls(cfg)
        self.tp = tp
        names = list(M.tensor_shapes(cfg).items())
        if size > 1 and cfg.tied:
            names.append(("tp.wcls", ((cfg.vocab_size, cfg.dim), False)))
        for name, (shape, is_norm) in names:
            n = int(np.prod(shape))
            dt = M.F32 if is_norm else cfg.weight_dtype
            src_name = "model.embed.weight" if name == "tp.wcls" else name
            scale, offset = M.synth_params(src_name, is_norm, peak, real, cfg.tied)
            if dt == M.Q4:  # padded rows with their scales: yalm_synth_q4 (never sharded: q4 runs on one GPU)
                if size > 1 or real is not None:
                    raise ValueError("q4 models are synthesised for one GPU, without the realistic patches")
                p = self._alloc(M.matrix_bytes(M.Q4, shape))
                check(lib.yalm_synth_q4(p, n // shape[-1], shape[-1], M.synth_seed(seed, src_name), scale, None))
                self.ptrs[name] = p
                continue
            if dt == M.E4M3:  # rows with their scale: yalm_synth_e4m3 (never sharded: e4m3 runs on one GPU)
                if size > 1 or real is not None:
                    raise ValueError("e4m3 models are synthesised for one GPU, without the realistic patches")
                p = self._alloc(M.matrix_bytes(M.E4M3, shape))
                check(lib.yalm_synth_e4m3(p, n // shape[-1], shape[-1], M.synth_seed(seed, src_name), scale, None))
                self.ptrs[name] = p
                continue
            eb = M.DTYPE_BYTES[dt]
            sh = M.tp_shard(cfg, name, rank, size)
            if sh is None or len(shape) != 2:  # (stacked expert tensors are never sharded: tp_check)
                p = self._alloc(n * eb)
                check(lib.yalm_synth(p, n, dt, M.synth_seed(seed, src_name), scale, offset, None))
            else:
                full = lib.yalm_alloc(n * eb)
                if not full:
                    raise YalmError(lib.yalm_last_error().decode())
                try:
                    check(lib.yalm_synth(full, n, dt, M.synth_seed(seed, src_name), scale, offset, None))
                    kind, start, cnt = sh
                    rows, cols = shape
                    if kind == "rows":
                        p = self._alloc(cnt * cols * eb)
                        check(lib.yalm_copy_2d(p, cols * eb, full + start * cols * eb, cols * eb, cols * eb, cnt))
                    else:
                        p = self._alloc(rows * cnt * eb)
                        check(lib.yalm_copy_2d(p, cnt * eb, full + start * eb, cols * eb, cnt * eb, rows))
                finally:
                    check(lib.yalm_stream_sync(None))
                    lib.yalm_free(full)
            self.ptrs[name] = p
        check(lib.yalm_stream_sync(None))
        if real is not None:
            shapes = M.tensor_shapes(cfg)
            for name in M.realistic_names(cfg):
                shape, is_norm = shapes[name]
                dt = M.F32 if is_norm else cfg.weight_dtype
                a = np.empty(shape, {M.F32: np.float32, M.F16: np.float16, M.F8E5M2: np.uint8}[dt])
                check(lib.yalm_download(a.ctypes.data, self.ptrs[name], a.nbytes))
                M.realistic_patch(cfg, name, a, real)
                p = lib.yalm_upload(a.ctypes.data, a.nbytes)
                if not p:
                    raise YalmError(lib.yalm_last_error().decode())
                old = self.ptrs[name]
                self._owned[self._owned.index(old)] = p
                lib.yalm_free(old)
                self.ptrs[name] = p
        return self

    def weights_struct(self):
        cfg = self.cfg
        blocks = (BlockWeights * cfg.n_layers)()
        for l in range(cfg.n_layers):
            n = M.layer_names(l)
            for k, name in n.items():
                setattr(blocks[l], k, self.ptrs[name])
        emb = self.ptrs["model.embed.weight"]
        wcls = self.ptrs.get("model.output.weight", self.ptrs.get("tp.wcls", emb))
        mw = ModelWeights(emb, self.ptrs["model.norm.weight"], wcls, blocks)
        return mw, blocks

    def close(self):
        for p in self._owned:
            lib.yalm_free(p)
        self._owned = []
        self.ptrs = {}


class Decoder:
    """InferenceState on the device + Model::forward (graph-replayed)."""

    def __init__(self, model: DeviceModel, tp_id: bytes = None, tp_gather=None, kv_caches=None,
                 cu_part=None, launch: int = 0, stream=None):
        """Tensor parallel over model.tp = (rank, size), one of:
        tp_id: the RCCL unique id (tp_unique_id() on rank 0, shared with the
        other ranks); tp_gather: a function mapping this rank's 128-byte rank
        record (IPC handle, GPU UUID, CU mask) to the list of every rank's record
        (e.g. via torch.distributed.all_gather_object) for the IPC exchange transport.
        Neither: a single-GPU decoder. kv_caches: optional per-layer (key, value)
        device pointers ([max_seq_len][kv_dim] f16 each, caller-owned), as
        Block::cuda() hands its own caches over (model.cpp:185-211); default: the
        decoder allocates zeroed caches. cu_part = (part, n_parts): decode on a
        stream restricted to that CU block (Stream). launch: yalm_decoder_set_launch
        flags (LAUNCH_*). stream: an existing Stream to create the decoder on (it stays the
        caller's; e.g. another decoder's get_stream(), for generate_speculative_model)."""
        if stream is not None and cu_part is not None:
            raise ValueError("Decoder: pass cu_part or stream, not both")
        self.model = model
        self.cfg = model.cfg
        self._c = Config.from_model(self.cfg)
        mw, self._blocks = model.weights_struct()
        if kv_caches is not None:
            for l, (kp, vp) in enumerate(kv_caches):
                self._blocks[l].key_cache = kp
                self._blocks[l].value_cache = vp
        self._mw = mw
        self.h = None
        self.stream = Stream(cu_part) if cu_part is not None else None
        self._on_stream = stream  # kept alive, never closed here
        sh = self.stream.h if self.stream else stream.h if stream is not None else None
        h = c_void_p()
        if tp_gather is not None:
            rank, size = getattr(model, "tp", (0, 1))
            buf = c_void_p()
            handle = ctypes.create_string_buffer(TP_HANDLE_BYTES)
            check(lib.yalm_tp_ipc_alloc(ctypes.byref(self._c), size, sh, ctypes.byref(buf), handle))
            handles = tp_gather(handle.raw)
            assert len(handles) == size and all(len(x) == TP_HANDLE_BYTES for x in handles)
            hb = ctypes.create_string_buffer(b"".join(handles), TP_HANDLE_BYTES * size)
            check(lib.yalm_decoder_create_tp_ipc(ctypes.byref(self._c), ctypes.byref(mw), rank, size, buf, hb, sh,
                                                 ctypes.byref(h)))
        elif self.cfg.n_experts > 0:
            if tp_id is not None:
                raise ValueError("mixture-of-experts models run on one GPU (no tensor-parallel form)")
            self._moe = (c_int * 2)(self.cfg.n_experts, self.cfg.n_experts_active)  # yalm_moe_config
            self._moegate = (c_void_p * self.cfg.n_layers)(
                *[model.ptrs[M.moegate_name(l)] for l in range(self.cfg.n_layers)])
            check(lib.yalm_decoder_create_moe(ctypes.byref(self._c), self._moe, ctypes.byref(mw), self._moegate, sh,
                                              ctypes.byref(h)))
        elif tp_id is None:
            check(lib.yalm_decoder_create(ctypes.byref(self._c), ctypes.byref(mw), sh, ctypes.byref(h)))
        else:
            rank, size = getattr(model, "tp", (0, 1))
            idb = ctypes.create_string_buffer(bytes(tp_id), 128)
            check(lib.yalm_decoder_create_tp(ctypes.byref(self._c), ctypes.byref(mw), rank, size, idb, sh,
                                             ctypes.byref(h)))
        self.h = h
        if launch:
            self.set_launch(launch)
        # the model family's forms (off unless the config has them)
        if self.cfg.rope_scaling is not None:
            self.set_rope_scaling(self.cfg.rope_scaling)
        if self.cfg.qkv_bias:
            self.set_qkv_bias(True)
        if self.cfg.qk_norm:
            self.set_qk_norm(True)

    def set_rope_scaling(self, rs) -> None:
        """yalm_decoder_set_rope_scaling: rs as ModelConfig.rope_scaling, a RopeScaling (passed as it
        is, so the tests can send bad parameters), or None = the plain table."""
        s = rs if isinstance(rs, RopeScaling) else RopeScaling.from_model(rs)
        check(lib.yalm_decoder_set_rope_scaling(self.h, ctypes.byref(s)))

    def inv_freq(self) -> np.ndarray:
        """The RoPE frequency table in use (yalm_decoder_get_inv_freq)."""
        out = np.empty(self.cfg.head_dim // 2, np.float32)
        check(lib.yalm_decoder_get_inv_freq(self.h, out.ctypes.data))
        return out

    def set_qkv_bias(self, on: bool = True) -> None:
        """yalm_decoder_set_qkv_bias with the model's attn.{wq,wk,wv}.bias tensors, or off."""
        if not on:
            check(lib.yalm_decoder_set_qkv_bias(self.h, None, None, None))
            return
        L = self.cfg.n_layers
        names = [M.bias_names(l) for l in range(L)]
        self._bias = [(c_void_p * L)(*[self.model.ptrs[n[k]] for n in names]) for k in ("bq", "bk", "bv")]
        check(lib.yalm_decoder_set_qkv_bias(self.h, *self._bias))

    def set_qk_norm(self, on: bool = True) -> None:
        """yalm_decoder_set_qk_norm with the model's attn.{q_norm,k_norm}.weight tensors, or off."""
        if not on:
            check(lib.yalm_decoder_set_qk_norm(self.h, None, None))
            return
        L = self.cfg.n_layers
        names = [M.qk_norm_names(l) for l in range(L)]
        self._qk_norm = [(c_void_p * L)(*[self.model.ptrs[n[k]] for n in names]) for k in ("gq", "gk")]
        check(lib.yalm_decoder_set_qk_norm(self.h, *self._qk_norm))

    def set_launch(self, flags: int) -> None:
        """yalm_decoder_set_launch: LAUNCH_EAGER | LAUNCH_SYNC | LAUNCH_SEPARATE_ATTN_WO (0 = default)."""
        check(lib.yalm_decoder_set_launch(self.h, flags))

    def forward(self, token: int, pos: int, mode: int = OUTPUT_LOGITS):
        if mode == OUTPUT_LOGITS:
            out = np.empty(self.cfg.vocab_size, np.float32)
            check(lib.yalm_forward(self.h, token, pos, mode, out.ctypes.data))
            return out
        check(lib.yalm_forward(self.h, token, pos, mode, None))
        return None

    def prefill(self, tokens, pos0: int = 0, logprobs: bool = True):
        """Batched MFMA prefill of positions pos0.. (fills the KV cache); returns
        log p(tokens[i+1] | ..tokens[i]) per position (last entry 0) or None."""
        tok = np.ascontiguousarray(tokens, dtype=np.int32)
        out = np.zeros(len(tok), np.float32) if logprobs else None
        check(lib.yalm_prefill(self.h, _ptr(tok), len(tok), pos0, _ptr(out) if logprobs else None))
        self._prefill_n = len(tok)
        return out

    def prefill_routing(self):
        """(experts, weights), each (n, n_layers, n_experts_active): the routing of the last
        prefill's n positions, in selection order (yalm_prefill_routing)."""
        shape = (getattr(self, "_prefill_n", 0), self.cfg.n_layers, max(self.cfg.n_experts_active, 1))
        experts, weights = np.zeros(shape, np.int32), np.zeros(shape, np.float32)
        check(lib.yalm_prefill_routing(self.h, _ptr(experts), _ptr(weights)))
        return experts, weights

    def set_prefill_precision(self, mode: int) -> None:
        """PREFILL_FAST (f16 activation operands) or PREFILL_SPLIT (every operand [hi | lo])."""
        check(lib.yalm_set_prefill_precision(self.h, mode))

    def prefill_info(self):
        """(passes, scaled layers) of the last prefill: the f16 range guard's re-runs."""
        p, n = c_int(), c_int()
        check(lib.yalm_prefill_info(self.h, ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    def set_prefill_forms(self, spec: str = "") -> None:
        """Select another exact prefill GEMM form (yalm_set_prefill_forms), "" = defaults."""
        check(lib.yalm_set_prefill_forms(self.h, spec.encode() if spec else None))

    def prefill_time(self, n: int, iters: int = 3) -> float:
        ms = c_float()
        check(lib.yalm_prefill_time(self.h, n, iters, ctypes.byref(ms)))
        return ms.value

    def generate_greedy(self, token: int, pos: int, n: int) -> list:
        out = np.zeros(max(n, 1), np.int32)
        check(lib.yalm_generate_greedy(self.h, token, pos, n, out.ctypes.data))
        return out[:n].tolist()

    def forward_rows(self, tokens, pos: int, logits: bool = True):
        """len(tokens) <= 4 tokens at positions pos.. in one pass over the weights
        (yalm_forward_rows); returns their logits (T, vocab) or None."""
        tok = np.ascontiguousarray(tokens, dtype=np.int32).reshape(-1)
        out = np.empty((tok.size, self.cfg.vocab_size), np.float32) if logits else None
        check(lib.yalm_forward_rows(self.h, _ptr(tok) if tok.size else None, tok.size, pos,
                                    _ptr(out) if logits else None))
        return out

    def generate_speculative(self, token: int, pos: int, n: int, rows: int = 4, ngram_max: int = 3,
                             ngram_min: int = 1, context=None, draft_stream=None):
        """n greedy tokens by speculative steps of `rows` rows (yalm_generate_speculative):
        (tokens, stats dict). context: the tokens before and including `token` (the n-gram
        drafter's history); draft_stream: the test / benchmark hook replacing the drafter."""
        ctx = np.ascontiguousarray(context if context is not None else [], dtype=np.int32).reshape(-1)
        ds = None if draft_stream is None else np.ascontiguousarray(draft_stream, dtype=np.int32).reshape(-1)
        keep = np.zeros(1, np.int32)  # a non-NULL pointer for an empty stream
        spec = Spec(rows, ngram_max, ngram_min,
                    None if ds is None else (_ptr(ds) if ds.size else _ptr(keep)), 0 if ds is None else ds.size)
        st = SpecStats()
        out = np.zeros(max(n, 1), np.int32)
        check(lib.yalm_generate_speculative(self.h, token, pos, n, ctypes.byref(spec), _ptr(ctx) if ctx.size else None,
                                            ctx.size, out.ctypes.data, ctypes.byref(st)))
        return out[:n].tolist(), {"spec_steps": st.spec_steps, "accepted_drafts": st.accepted_drafts,
                                  "plain_steps": st.plain_steps, "launches_per_step": st.launches_per_step}

    def generate_sampled(self, token: int, pos: int, n: int, temperature: float, top_k: int = 0,
                         top_p: float = 1.0, uniforms=None, seed: int = 0) -> list:
        """n tokens sampled on the device (yalm_generate_sampled): temperature, then top-k, then
        top-p, one uniform per step. uniforms None: numpy.random.default_rng(seed).random(n, float32)."""
        if uniforms is None:
            uniforms = np.random.default_rng(seed).random(n, dtype=np.float32)
        u = np.ascontiguousarray(uniforms, dtype=np.float32).reshape(-1)
        if u.size < n:
            raise ValueError(f"generate_sampled: {n} steps need {n} uniforms, got {u.size}")
        if u.size == 0:
            u = np.zeros(1, np.float32)
        s = Sampling(temperature, top_k, top_p)
        out = np.zeros(max(n, 1), np.int32)
        check(lib.yalm_generate_sampled(self.h, token, pos, n, ctypes.byref(s), _ptr(u), out.ctypes.data))
        return out[:n].tolist()

    def generate_speculative_sampled(self, token: int, pos: int, n: int, temperature: float, top_k: int = 0,
                                     top_p: float = 1.0, uniforms=None, seed: int = 0, rows: int = 4,
                                     ngram_max: int = 3, ngram_min: int = 1, context=None, draft_stream=None):
        """n sampled tokens by speculative steps of `rows` rows (yalm_generate_speculative_sampled):
        (tokens, stats dict); the tokens of generate_sampled for the same uniforms. uniforms / seed
        as generate_sampled, the rest as generate_speculative."""
        if uniforms is None:
            uniforms = np.random.default_rng(seed).random(n, dtype=np.float32)
        u = np.ascontiguousarray(uniforms, dtype=np.float32).reshape(-1)
        if u.size < n:
            raise ValueError(f"generate_speculative_sampled: {n} tokens need {n} uniforms, got {u.size}")
        if u.size == 0:
            u = np.zeros(1, np.float32)
        ctx = np.ascontiguousarray(context if context is not None else [], dtype=np.int32).reshape(-1)
        ds = None if draft_stream is None else np.ascontiguousarray(draft_stream, dtype=np.int32).reshape(-1)
        keep = np.zeros(1, np.int32)  # a non-NULL pointer for an empty stream
        spec = Spec(rows, ngram_max, ngram_min,
                    None if ds is None else (_ptr(ds) if ds.size else _ptr(keep)), 0 if ds is None else ds.size)
        s = Sampling(temperature, top_k, top_p)
        st = SpecStats()
        out = np.zeros(max(n, 1), np.int32)
        check(lib.yalm_generate_speculative_sampled(self.h, token, pos, n, ctypes.byref(spec), ctypes.byref(s), _ptr(u),
                                                    _ptr(ctx) if ctx.size else None, ctx.size, out.ctypes.data,
                                                    ctypes.byref(st)))
        return out[:n].tolist(), {"spec_steps": st.spec_steps, "accepted_drafts": st.accepted_drafts,
                                  "plain_steps": st.plain_steps, "launches_per_step": st.launches_per_step}

    def get_stream(self) -> Stream:
        """The stream this decoder enqueues on (yalm_decoder_get_stream), as a borrowed Stream: pass
        it as Decoder(..., stream=) to put a second decoder on it. It lives as long as its owner."""
        h = c_void_p()
        check(lib.yalm_decoder_get_stream(self.h, ctypes.byref(h)))
        return Stream(borrowed=h.value)

    def generate_speculative_model(self, draft: "Decoder", token: int, pos: int, n: int, rows: int = 4,
                                   temperature: float = 0.0, top_k: int = 0, top_p: float = 1.0, uniforms=None,
                                   draft_stream=None):
        """n tokens by speculative steps of `rows` rows whose drafts come from the decoder `draft` on
        the same stream (yalm_generate_speculative_model): (tokens, stats dict). temperature 0:
        greedy, the tokens of generate_speculative; else sampled with `uniforms` (n values), the
        tokens of generate_speculative_sampled. Hydrate [0, pos) on both decoders first.
        draft_stream: the test / benchmark hook replacing the draft's tokens (its forwards still run)."""
        ds = None if draft_stream is None else np.ascontiguousarray(draft_stream, dtype=np.int32).reshape(-1)
        keep = np.zeros(1, np.int32)  # a non-NULL pointer for an empty stream
        cfg = None if rows is None else SpecModel(  # rows None: a NULL cfg (the argument test)
            rows, None if ds is None else (_ptr(ds) if ds.size else _ptr(keep)), 0 if ds is None else ds.size)
        s, u = None, None
        if temperature != 0.0:
            if uniforms is None:
                raise ValueError("generate_speculative_model: sampling needs uniforms")
            u = np.ascontiguousarray(uniforms, dtype=np.float32).reshape(-1)
            if u.size < n:
                raise ValueError(f"generate_speculative_model: {n} tokens need {n} uniforms, got {u.size}")
            if u.size == 0:
                u = np.zeros(1, np.float32)
            s = Sampling(temperature, top_k, top_p)
        st = SpecStats()
        out = np.zeros(max(n, 1), np.int32)
        check(lib.yalm_generate_speculative_model(self.h, draft.h if draft is not None else None, token, pos, n,
                                                  ctypes.byref(cfg) if cfg is not None else None,
                                                  ctypes.byref(s) if s is not None else None,
                                                  _ptr(u) if u is not None else None, out.ctypes.data,
                                                  ctypes.byref(st)))
        return out[:n].tolist(), {"spec_steps": st.spec_steps, "accepted_drafts": st.accepted_drafts,
                                  "plain_steps": st.plain_steps, "launches_per_step": st.launches_per_step}

    def enqueue_greedy(self, n: int) -> None:
        check(lib.yalm_enqueue_greedy(self.h, n))

    def device_step(self):
        t, p = c_int(), c_int()
        check(lib.yalm_device_step(self.h, ctypes.byref(t), ctypes.byref(p)))
        return t.value, p.value

    def device_tokens(self, cap: int = 1 << 16) -> list:
        """Greedy tokens produced on the device since the last generate_greedy."""
        out = np.zeros(max(cap, 1), np.int32)
        n = c_int()
        check(lib.yalm_device_tokens(self.h, out.ctypes.data, cap, ctypes.byref(n)))
        return out[:min(n.value, cap)].tolist()

    def block(self, layer, pos, kv_sink, kv_pos, kv_len):
        check(lib.yalm_block(self.h, layer, pos, kv_sink, kv_pos, kv_len))

    def get_x(self) -> np.ndarray:
        out = np.empty(self.cfg.dim, np.float32)
        check(lib.yalm_get_x(self.h, out.ctypes.data))
        return out

    def set_x(self, x: np.ndarray) -> None:
        x = np.ascontiguousarray(x, dtype=np.float32)
        check(lib.yalm_set_x(self.h, x.ctypes.data))

    def get_logits(self) -> np.ndarray:
        out = np.empty(self.cfg.vocab_size, np.float32)
        check(lib.yalm_get_logits(self.h, out.ctypes.data))
        return out

    def moe_routing(self):
        """(experts, weights), each (n_layers, n_experts_active): the routing of the most
        recent forward / block, in selection order (yalm_moe_routing)."""
        shape = (self.cfg.n_layers, max(self.cfg.n_experts_active, 1))
        experts, weights = np.zeros(shape, np.int32), np.zeros(shape, np.float32)
        check(lib.yalm_moe_routing(self.h, _ptr(experts), _ptr(weights)))
        return experts, weights

    def time_kernel(self, kernel_id: int, iters: int) -> float:
        ms = c_float()
        check(lib.yalm_time_kernel(self.h, kernel_id, iters, ctypes.byref(ms)))
        return ms.value

    def set_gemv_config(self, kind: int, threads: int = 0, unroll: int = 0, gpw: int = 0) -> None:
        check(lib.yalm_set_gemv_config(self.h, kind, threads, unroll, gpw))

    @property
    def attn_wo(self) -> bool:
        """True when the launch path runs attention + Wo as one launch (attn_wo.h)."""
        return bool(lib.yalm_decoder_attn_wo(self.h))

    def attn_wo_trace(self):
        """((workgroups, 16) uint64 stamps, attention workgroups) of the last fused
        attention + Wo launch (decoder created with YALM_ATTN_WO_TRACE=1)."""
        buf = np.zeros(16 * 8192, np.uint64)
        nb, na = c_int(), c_int()
        check(lib.yalm_attn_wo_trace(self.h, buf.ctypes.data, buf.size, ctypes.byref(nb), ctypes.byref(na)))
        return buf[: 16 * nb.value].reshape(nb.value, 16), na.value

    def graph_kernels(self, mode: int = 2) -> int:
        """Kernel launches per forward of graph `mode` (2 = the device greedy step, 3 = the sampled one)."""
        k, n = c_int(), c_int()
        check(lib.yalm_graph_kernels(self.h, mode, ctypes.byref(k), ctypes.byref(n)))
        return k.value

    def kernel_name(self, kernel_id: int) -> str:
        return lib.yalm_kernel_name(self.h, kernel_id).decode()

    def close(self):
        if self.h:
            check(lib.yalm_decoder_destroy(self.h))
            self.h = None
        if getattr(self, "stream", None) is not None:
            self.stream.close()
            self.stream = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Batch:
    """Up to four independent sequences decoded together on one Decoder (yalm_batch_*): every
    weight matrix is streamed once per step for all of them. Prompts arrive through the decoder:
    hydrate it (Decoder.prefill / forward), then load(). The decoder must outlive the batch."""

    def __init__(self, decoder: Decoder, n_seq: int, launch: int = 0):
        self.decoder = decoder
        self.cfg = decoder.cfg
        self.n_seq = n_seq
        self.h = None
        h = c_void_p()
        check(lib.yalm_batch_create(decoder.h, n_seq, ctypes.byref(h)))
        self.h = h
        self.launch = 0
        if launch:
            self.set_launch(launch)

    def _rows(self, values, name: str) -> np.ndarray:
        a = np.ascontiguousarray(values, dtype=np.int32).reshape(-1)
        if a.size != self.n_seq:
            raise ValueError(f"Batch: {name} needs one entry per sequence ({self.n_seq}), got {a.size}")
        return a

    def set_launch(self, flags: int) -> None:
        """yalm_batch_set_launch: BATCH_ATTN_PER_SEQ or 0."""
        check(lib.yalm_batch_set_launch(self.h, flags))
        self.launch = flags

    def load(self, n_positions: int, seq: int = -1) -> None:
        """KV rows [0, n_positions) of the decoder's caches into sequence seq (-1: all)."""
        check(lib.yalm_batch_load(self.h, seq, n_positions))

    def forward(self, tokens, pos, logits: bool = True):
        """One step without a commit: row s feeds tokens[s] at pos[s]; logits (n_seq, vocab) or None."""
        t, p = self._rows(tokens, "tokens"), self._rows(pos, "pos")
        out = np.empty((self.n_seq, self.cfg.vocab_size), np.float32) if logits else None
        check(lib.yalm_batch_forward(self.h, _ptr(t), _ptr(p), _ptr(out) if logits else None))
        return out

    def generate_greedy(self, tokens, pos, n: int):
        """n greedy steps of every sequence: (tokens (n_seq, n) int32, stats dict)."""
        t, p = self._rows(tokens, "tokens"), self._rows(pos, "pos")
        out = np.zeros((self.n_seq, max(n, 1)), np.int32)
        st = BatchStats()
        check(lib.yalm_batch_generate_greedy(self.h, _ptr(t), _ptr(p), n, _ptr(out) if n > 0 else None,
                                             ctypes.byref(st)))
        res = np.ascontiguousarray(out[:, :n]) if n > 0 else np.zeros((self.n_seq, 0), np.int32)
        return res, {"launches_per_step": st.launches_per_step}

    def generate_sampled(self, tokens, pos, n: int, temperature: float, top_k: int = 0, top_p: float = 1.0,
                         uniforms=None, seed: int = 0):
        """n sampled steps of every sequence, row s of step i drawn with uniforms[s][i]
        (uniforms None: numpy.random.default_rng(seed).random((n_seq, n), float32))."""
        t, p = self._rows(tokens, "tokens"), self._rows(pos, "pos")
        if uniforms is None:
            uniforms = np.random.default_rng(seed).random((self.n_seq, n), dtype=np.float32)
        u = np.ascontiguousarray(uniforms, dtype=np.float32)
        if u.shape != (self.n_seq, n):
            raise ValueError(f"Batch.generate_sampled: uniforms must be ({self.n_seq}, {n}), got {u.shape}")
        if u.size == 0:
            u = np.zeros(1, np.float32)
        s = Sampling(temperature, top_k, top_p)
        out = np.zeros((self.n_seq, max(n, 1)), np.int32)
        st = BatchStats()
        check(lib.yalm_batch_generate_sampled(self.h, _ptr(t), _ptr(p), n, ctypes.byref(s), _ptr(u),
                                              _ptr(out) if n > 0 else None, ctypes.byref(st)))
        res = np.ascontiguousarray(out[:, :n]) if n > 0 else np.zeros((self.n_seq, 0), np.int32)
        return res, {"launches_per_step": st.launches_per_step}

    def state(self):
        """(tokens, pos): every sequence's next token and position (lists)."""
        t, p = np.zeros(self.n_seq, np.int32), np.zeros(self.n_seq, np.int32)
        check(lib.yalm_batch_state(self.h, _ptr(t), _ptr(p)))
        return t.tolist(), p.tolist()

    def stats(self) -> dict:
        """The launch count of one step in the current attention form."""
        z = np.zeros(self.n_seq, np.int32)
        st = BatchStats()
        check(lib.yalm_batch_generate_greedy(self.h, _ptr(z), _ptr(z), 0, None, ctypes.byref(st)))
        return {"launches_per_step": st.launches_per_step}

    def buffers(self, seq: int, layer: int = 0):
        """Test hook (yalm_batch_buffers): device pointers (kcache, vcache, tokens) of sequence seq."""
        k, v, t = c_void_p(), c_void_p(), c_void_p()
        check(lib.yalm_batch_buffers(self.h, seq, layer, ctypes.byref(k), ctypes.byref(v), ctypes.byref(t)))
        return k.value, v.value, t.value

    def close(self):
        if self.h:
            check(lib.yalm_batch_destroy(self.h))
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
