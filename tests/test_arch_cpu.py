"""CPU: the Qwen2 q / k / v bias and the Llama-3 "llama3" RoPE scaling below the device --
the float64 reference (arch_ref.py), models.rope_inv_freq, the converter, and the margins that
make the GPU tests of test_gpu_arch.py meaningful: on every decode case the reference WITH the
form is at least 10 bars from the reference without it at every compared position, so a decoder
that dropped the bias or the scaling cannot pass."""
import json
import os

import numpy as np
import pytest

import arch_cases as A
import arch_hf
import arch_ref
import gemv_ref
import ref_numpy
from yalm_amd import convert
from yalm_amd import models as M
from yalm_amd.yalmfile import read_yalm

LOGITS_BAR, BLOCK_BAR = A.LOGITS_BAR, A.BLOCK_BAR  # the GPU tests' bars

LLAMA31_8B = M.ModelConfig(dim=4096, hidden_dim=14336, head_dim=128, n_layers=32, n_heads=32, n_kv_heads=8,
                           vocab_size=128256, max_seq_len=4096, rope_theta=5e5,
                           rope_scaling=("llama3", 8.0, 1.0, 4.0, 8192))
LLAMA32_3B = M.LLAMA_32_3B.with_(rope_scaling=("llama3", 32.0, 1.0, 4.0, 8192))


def ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


# ---------------------------------------------------------------- the reference
@pytest.mark.parametrize("dtype", [M.F32, M.F16, M.F8E5M2])
def test_arch_ref_is_refmodel_without_the_forms(dtype):
    """Zero bias, no scaling: bit for bit RefModel, through the wrap and the sink rotation."""
    cfg = M.TINY.with_(max_seq_len=16, weight_dtype=dtype)
    t = M.synth_host_tensors(cfg, seed=3)
    bcfg = cfg.with_(qkv_bias=True)
    tb = dict(t)
    for name, (shape, _) in M.tensor_shapes(bcfg).items():
        if name.endswith(".bias"):
            tb[name] = np.zeros(shape, np.float32)
    plain, ref, zero = arch_ref.ArchRef(cfg, t), ref_numpy.RefModel(cfg, t), arch_ref.ArchRef(bcfg, tb)
    tok = 3
    for pos in range(20):
        lo = ref.forward(tok, pos)
        np.testing.assert_array_equal(plain.forward(tok, pos), lo)
        np.testing.assert_array_equal(zero.forward(tok, pos), lo)
        tok = A.step_token(tok, cfg.vocab_size)


def test_q4_goes_through_the_twin():
    cfg, seed, _ = A.CASES["bias-q4-64"]
    t = A.tensors("bias-q4-64")
    tcfg, tt = M.q4_twin(cfg, t)
    np.testing.assert_array_equal(arch_ref.ArchRef(cfg, t).forward(5, 0), arch_ref.ArchRef(tcfg, tt).forward(5, 0))
    assert tcfg.qkv_bias and M.bias_names(0)["bq"] in tt


# ---------------------------------------------------------------- rope_inv_freq
def plain_inv_freq(c):
    """models.rope_inv_freq as it was before rope_scaling existed."""
    j = np.arange(0, c.head_dim, 2).astype(np.float32)
    rinv = np.float32(1.0) / np.float32(c.rotary_dim)
    f = np.power(np.float32(c.rope_theta), -(j * rinv).astype(np.float32)).astype(np.float32)
    f[j >= c.rotary_dim] = 0.0
    return f.astype(np.float32)


@pytest.mark.parametrize("cfg", [M.TINY, M.SMALL, M.MISTRAL_7B, M.LLAMA_32_3B, M.SMALL.with_(rotary_dim=32)])
def test_inv_freq_without_scaling_is_unchanged(cfg):
    got = M.rope_inv_freq(cfg)
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got.view(np.uint32), plain_inv_freq(cfg).view(np.uint32))


@pytest.mark.parametrize("cfg", [LLAMA31_8B, LLAMA32_3B, A.CASES["scaled-small-f16"][0], A.CASES["scaled-hd16-f16"][0]],
                         ids=["llama-3.1-8b", "llama-3.2-3b", "small", "hd16"])
def test_inv_freq_llama3_against_f64_restatement(cfg):
    """Within 2 f32 ulps of the rule restated in f64 on the f32 table, and every regime (kept,
    blended, divided) holds at least one pair."""
    got = M.rope_inv_freq(cfg)
    base = plain_inv_freq(cfg)
    want = arch_ref.llama3_f64(base.astype(np.float64), cfg.rope_scaling)
    assert ulps(got, want.astype(np.float32)).max() <= 2
    reg = arch_ref.regimes(base, cfg.rope_scaling)
    assert set(reg.tolist()) == {0, 1, 2}, reg
    _, factor, _, _, _ = cfg.rope_scaling
    np.testing.assert_array_equal(got[reg == 0], base[reg == 0])
    assert ulps(got[reg == 2], (base[reg == 2].astype(np.float64) / factor).astype(np.float32)).max() <= 1
    lo, hi = base[reg == 1].astype(np.float64) / factor, base[reg == 1].astype(np.float64)
    assert np.all((got[reg == 1] > lo) & (got[reg == 1] < hi))
    # the f64 table of arch_ref (from f64 frequencies) is the same table to f32 rounding
    assert np.max(np.abs(arch_ref.freq_table(cfg) / got.astype(np.float64) - 1)) < 3e-7


@pytest.mark.parametrize("bad", [("yarn", 8.0, 1.0, 4.0, 32), ("llama3", 0.5, 1.0, 4.0, 32), ("llama3", 8.0, 4.0, 4.0, 32),
                                 ("llama3", 8.0, 1.0, 4.0, 0)])
def test_bad_scaling_parameters_raise(bad):
    with pytest.raises(ValueError):
        M.TINY.with_(rope_scaling=bad)


# ---------------------------------------------------------------- config and metadata
def test_metadata_round_trip_and_old_files():
    c = M.SMALL.with_(qkv_bias=True, rope_scaling=A.SCALING)
    md = c.metadata()
    for k in ("qkv_bias",) + M.ROPE_SCALING_KEYS:
        assert k in md
    back = M.config_from_metadata(md)
    assert back.qkv_bias is True and back.rope_scaling == A.SCALING
    plain = M.SMALL.metadata()
    assert not [k for k in plain if k == "qkv_bias" or k.startswith("rope_scaling") or k.startswith("rope_low")
                or k.startswith("rope_high") or k.startswith("rope_original")]
    back = M.config_from_metadata(plain)
    assert back.qkv_bias is False and back.rope_scaling is None
    names = M.tensor_shapes(c)
    b = M.bias_names(1)
    assert names[b["bq"]] == ((c.q_dim,), True) and names[b["bk"]] == ((c.kv_dim,), True)
    assert names[b["bv"]] == ((c.kv_dim,), True)
    assert not [n for n in M.tensor_shapes(M.SMALL) if n.endswith(".bias")]


@pytest.mark.parametrize("fname", ["tiny_fp16.yalm", "tiny_fp32.yalm", "tiny_fp8.yalm", "tiny_fp16_tied.yalm",
                                   "tiny_moe_fp16.yalm"])
def test_old_fixtures_parse_without_the_forms(golden_dir, fname):
    yd = read_yalm(os.path.join(golden_dir, fname))
    cfg = M.config_from_metadata(yd.metadata)
    yd.close()
    assert cfg.qkv_bias is False and cfg.rope_scaling is None


# ---------------------------------------------------------------- converter
@pytest.fixture(scope="module")
def qwen2(tmp_path_factory):
    d = tmp_path_factory.mktemp("qwen2")
    hf = arch_hf.write_qwen2(str(d / "hf"))
    out = str(d / "qwen2_fp32.yalm")
    convert.convert(str(d / "hf"), out, "fp32")
    return hf, out


def test_convert_qwen2_bias_tensors(qwen2):
    hf, path = qwen2
    yd = read_yalm(path)
    cfg = M.config_from_metadata(yd.metadata, tied="model.output.weight" not in yd.tensors)
    assert yd.metadata["arch"] == "Qwen2ForCausalLM" and cfg.qkv_bias and cfg.rope_scaling is None
    assert cfg.rope_theta == 1e6
    assert sorted(k for k in yd.tensors if k != "tokenizer.tokens") == sorted(M.tensor_shapes(cfg))
    rng = np.random.default_rng(0)
    x = rng.standard_normal(cfg.dim)
    for l in range(cfg.n_layers):
        p, b, n = f"model.layers.{l}.self_attn.", M.bias_names(l), M.layer_names(l)
        for key, hfn, heads in (("q", "q_proj", cfg.n_heads), ("k", "k_proj", cfg.n_kv_heads)):
            t = yd.tensors[b["b" + key]]
            assert t.dtype == "F32" and tuple(t.shape) == (heads * cfg.head_dim,)
            got = np.array(t.data).reshape(-1)
            want = convert.permute_reverse(hf[p + hfn + ".bias"][:, None], heads, cfg.rotary_dim)[:, 0]
            np.testing.assert_array_equal(got, want)
            assert not np.array_equal(got, hf[p + hfn + ".bias"])  # the permutation moved rows
            # the projection with its bias, row-permuted as a whole
            w = np.array(yd.tensors[n["w" + key]].data).reshape(yd.tensors[n["w" + key]].shape).astype(np.float64)
            y_hf = hf[p + hfn + ".weight"].astype(np.float64) @ x + hf[p + hfn + ".bias"]
            np.testing.assert_array_equal(w @ x + got,
                                          convert.permute_reverse(y_hf[:, None], heads, cfg.rotary_dim)[:, 0])
        t = yd.tensors[b["bv"]]
        assert t.dtype == "F32"
        np.testing.assert_array_equal(np.array(t.data).reshape(-1), hf[p + "v_proj.bias"])
    yd.close()


@pytest.mark.parametrize("dtype", ["fp16", "fp8", "q4"])
def test_convert_qwen2_other_dtypes_keep_f32_bias(tmp_path, dtype):
    hf = arch_hf.write_qwen2(str(tmp_path / "hf"))
    out = str(tmp_path / "q.yalm")
    convert.convert(str(tmp_path / "hf"), out, dtype)
    yd = read_yalm(out)
    t = yd.tensors[M.bias_names(0)["bv"]]
    assert t.dtype == "F32"
    np.testing.assert_array_equal(np.array(t.data).reshape(-1), hf["model.layers.0.self_attn.v_proj.bias"])
    yd.close()


def test_convert_llama3_scaling_round_trip(tmp_path):
    arch_hf.write_llama3(str(tmp_path / "hf"))
    out = str(tmp_path / "l3.yalm")
    convert.convert(str(tmp_path / "hf"), out, "fp16")
    yd = read_yalm(out)
    cfg = M.config_from_metadata(yd.metadata, tied="model.output.weight" not in yd.tensors)
    s = arch_hf.LLAMA3_SCALING
    assert cfg.rope_scaling == ("llama3", s["factor"], s["low_freq_factor"], s["high_freq_factor"],
                                s["original_max_position_embeddings"])
    assert cfg.qkv_bias is False and not [k for k in yd.tensors if k.endswith(".bias")]
    yd.close()


def _config(arch="LlamaForCausalLM", **kw):
    return dict(arch_hf.TINY_HF, architectures=[arch], **kw)


@pytest.mark.parametrize("kw", [
    {"rope_scaling": {"rope_type": "yarn", "factor": 4.0}},
    {"rope_scaling": {"type": "linear", "factor": 2.0}},
    {"rope_scaling": {"type": "dynamic", "factor": 2.0}},
    {"attention_bias": True},
    {"mlp_bias": True},
])
def test_convert_refuses(kw):
    with pytest.raises(ValueError):
        convert.metadata_from_config(_config(**kw), "fp16")


def test_convert_refuses_qwen2_sliding_window_and_mlp_bias():
    with pytest.raises(ValueError):
        convert.metadata_from_config(_config("Qwen2ForCausalLM", use_sliding_window=True), "fp16")
    with pytest.raises(ValueError):
        convert.metadata_from_config(_config("Qwen2ForCausalLM", mlp_bias=True), "fp16")
    md = convert.metadata_from_config(_config("Qwen2ForCausalLM", use_sliding_window=False), "fp16")
    assert md["qkv_bias"] == "1"


def test_convert_default_scaling_is_none():
    for rs in (None, {"rope_type": "default"}, {"type": "default"}):
        md = convert.metadata_from_config(_config(rope_scaling=rs), "fp16")
        assert "rope_scaling_type" not in md and "qkv_bias" not in md
    md = convert.metadata_from_config(_config(rope_scaling=dict(arch_hf.LLAMA3_SCALING, rope_type=None, type="llama3")),
                                      "fp16")
    assert md["rope_scaling_type"] == "llama3" and json.loads(md["rope_original_max_position"]) == 32


# ---------------------------------------------------------------- the GPU tests' margins
@pytest.mark.parametrize("name", list(A.CASES))
def test_margins_of_the_gpu_cases(name):
    """Every compared position: the model without the form is >= 10 x the GPU test's bar from
    the model with it (logits; for the biased cases the per-layer hook too), and every greedy
    step's top-2 gap clears 1e-3 of max|logit| (the GPU greedy tokens are then determined)."""
    cfg, _, first = A.CASES[name]
    full, plain = A.logits_run(name), A.logits_run(name, "plain")
    for pos in range(first, A.N_POS):
        d = A.relerr(plain[pos], full[pos])
        assert d >= 10 * LOGITS_BAR, (pos, d)
    if cfg.qkv_bias:
        bf, bp = A.blocks_run(name), A.blocks_run(name, "plain")
        for pos in range(A.N_POS):
            for l in range(cfg.n_layers):
                d = A.relerr(bp[pos, l], bf[pos, l])
                assert d >= 10 * BLOCK_BAR, (pos, l, d)
    toks, lg = A.greedy_run(name)
    srt = np.sort(lg, axis=1)
    gap = (srt[:, -1] - srt[:, -2]) / np.max(np.abs(lg), axis=1)
    assert gap.min() >= 1e-3, gap


def test_scaled_cases_change_nothing_at_position_zero():
    """Why the scaled cases compare from SCALED_FIRST on: every angle is 0 at position 0."""
    for name in A.SCALED_CASES:
        np.testing.assert_array_equal(A.logits_run(name)[0], A.logits_run(name, "plain")[0])


@pytest.mark.parametrize("name", sorted(arch_hf.HOST_MODELS))
def test_host_models_have_no_near_tie(tmp_path, name):
    """The files of tests/test_host_arch.py: the reference's greedy path over the CLI prompt
    clears 1e-3 of max|logit| at every step, and the form matters to it (the same file read
    without its bias / scaling takes another path or other logits)."""
    writer, _ = arch_hf.HOST_MODELS[name]
    writer(str(tmp_path / "hf"))
    out = str(tmp_path / "m.yalm")
    convert.convert(str(tmp_path / "hf"), out, "fp16")
    enc, toks, gap = arch_hf.host_reference(out)
    assert gap >= 1e-3 and len(toks) == arch_hf.HOST_N, (gap, toks)
    cfg, t = arch_hf.load_yalm(out)
    full = arch_ref.ArchRef(cfg, t)
    plain = arch_ref.ArchRef(cfg, t, use_bias=False, rope_scaling=None)
    last = None
    for pos, tk in enumerate(enc + toks[:8]):
        last = (full.forward(tk, pos), plain.forward(tk, pos))
    assert A.relerr(last[1], last[0]) >= 10 * LOGITS_BAR


@pytest.mark.parametrize("name", sorted(A.SPEC))
def test_spec_cases_have_no_near_tie(name):
    """The speculative tests compare token sequences: the reference's greedy path clears twice
    the logits bar at every step (seeds searched here, on the CPU)."""
    assert A.spec_case(name)[3] >= 2 * LOGITS_BAR


def test_glu_case_separates_the_activations():
    """test_gpu_arch.py test_time_kernel_glu_runs_the_models_activation: the SILU model's x is far
    outside the bar around the GELU model's, so a hook that ran the wrong activation fails there."""
    assert A.GLU_BAR == gemv_ref.REL_TOL
    assert A.relerr(A.glu_case(M.SILU)[3], A.glu_case(M.GELU)[3]) > 100 * A.GLU_BAR
