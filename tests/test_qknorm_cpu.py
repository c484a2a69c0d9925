"""CPU: the q / k norm (Qwen3) below the device -- the float64 reference (qknorm_ref.py), the
config / metadata / synthetic rule, the converter, and the margins that make the GPU tests of
test_gpu_qknorm.py meaningful: on every decode case the wrong models a mistaken kernel would
compute (no norm, g = 1, gq and gk exchanged, g reversed within the head) lie at least 10 bars
from the right one at every compared position, so such a kernel cannot pass."""
import os

import numpy as np
import pytest

import arch_hf
import arch_ref
import qknorm_cases as C
import qknorm_hf
import qknorm_ref
from yalm_amd import convert
from yalm_amd import models as M
from yalm_amd.yalmfile import read_yalm

LOGITS_BAR, BLOCK_BAR = C.LOGITS_BAR, C.BLOCK_BAR  # the GPU tests' bars


# ---------------------------------------------------------------- the reference
@pytest.mark.parametrize("dtype", [M.F32, M.F16, M.F8E5M2])
def test_qknorm_ref_is_archref_without_the_norm(dtype):
    """Norm off (by the config, or by the "none" switch on a normed model's tensors): bit for
    bit ArchRef, through the wrap and the sink rotation."""
    cfg = M.TINY.with_(max_seq_len=16, weight_dtype=dtype)
    ncfg = cfg.with_(qk_norm=True)
    tn = M.synth_host_tensors(ncfg, seed=3)
    t = {k: v for k, v in tn.items() if "_norm.weight" not in k}
    base, off, none = arch_ref.ArchRef(cfg, t), qknorm_ref.QKNormRef(cfg, t), qknorm_ref.QKNormRef(ncfg, tn, wrong="none")
    on = qknorm_ref.QKNormRef(ncfg, tn)
    tok = 3
    for pos in range(20):
        lo = base.forward(tok, pos)
        np.testing.assert_array_equal(off.forward(tok, pos), lo)
        np.testing.assert_array_equal(none.forward(tok, pos), lo)
        d = C.relerr(on.forward(tok, pos), lo)
        assert (d == 0) if pos == 0 else (d > 10 * LOGITS_BAR), (pos, d)
        tok = C.step_token(tok, cfg.vocab_size)


def test_head_rmsnorm_statement():
    rng = np.random.default_rng(0)
    a, g = rng.standard_normal(3 * 16), rng.uniform(0.5, 2.5, 16)
    got = qknorm_ref.head_rmsnorm(a, g, 16, 1e-6)
    for h in range(3):
        v = a[16 * h:16 * h + 16]
        np.testing.assert_allclose(got[16 * h:16 * h + 16], v * (1.0 / np.sqrt(np.sum(v * v) / 16 + 1e-6)) * g, rtol=1e-15)


def test_q4_goes_through_the_twin():
    cfg, _ = C.CASES["tiny-q4"]
    t = C.tensors("tiny-q4")
    tcfg, tt = M.q4_twin(cfg, t)
    np.testing.assert_array_equal(qknorm_ref.QKNormRef(cfg, t).forward(5, 1), qknorm_ref.QKNormRef(tcfg, tt).forward(5, 1))
    assert tcfg.qk_norm and M.qk_norm_names(0)["gq"] in tt


# ---------------------------------------------------------------- config, metadata, the synthetic rule
def test_metadata_round_trip_and_old_files(golden_dir):
    c = M.SMALL.with_(qk_norm=True)
    md = c.metadata()
    assert md["qk_norm"] == "1" and md["arch"] == "Qwen3ForCausalLM"
    assert M.config_from_metadata(md).qk_norm is True
    plain = M.SMALL.metadata()
    assert "qk_norm" not in plain and M.config_from_metadata(plain).qk_norm is False
    assert M.SMALL.with_(qkv_bias=True).metadata()["arch"] == "Qwen2ForCausalLM"
    names = M.tensor_shapes(c)
    g = M.qk_norm_names(1)
    assert g == {"gq": "model.layers.1.attn.q_norm.weight", "gk": "model.layers.1.attn.k_norm.weight"}
    assert names[g["gq"]] == ((c.head_dim,), True) and names[g["gk"]] == ((c.head_dim,), True)
    assert not [n for n in M.tensor_shapes(M.SMALL) if "_norm.weight" in n]
    assert c.weight_bytes_per_token() - M.SMALL.weight_bytes_per_token() == c.n_layers * 2 * c.head_dim * 4
    for fname in ("tiny_fp16.yalm", "tiny_fp8.yalm", "tiny_moe_fp16.yalm"):
        yd = read_yalm(os.path.join(golden_dir, fname))
        assert M.config_from_metadata(yd.metadata).qk_norm is False
        yd.close()


def test_synthetic_norm_weights_and_preset():
    assert (M.QKNORM_SCALE, M.QKNORM_OFFSET) == (1.0, 1.5)
    assert M.synth_params("model.layers.0.attn.q_norm.weight", True) == (1.0, 1.5)
    assert M.synth_params("model.layers.0.attn.k_norm.weight", True, peak=8.0) == (1.0, 1.5)
    assert M.synth_params("model.layers.0.attn.norm.weight", True) == (M.NORM_SCALE, M.NORM_OFFSET)
    t = C.tensors("small-f16")
    for l in range(C.CASES["small-f16"][0].n_layers):
        for name in M.qk_norm_names(l).values():
            a = t[name]
            assert a.dtype == np.float32 and a.shape == (64,) and 0.5 <= a.min() and a.max() < 2.5
            assert a.max() - a.min() > 1.0
    q = M.PRESETS["qwen3-8b"]
    assert q is M.QWEN3_8B and q.qk_norm and not q.qkv_bias
    assert (q.dim, q.hidden_dim, q.n_layers, q.n_heads, q.n_kv_heads, q.head_dim, q.vocab_size, q.rope_theta) == \
        (4096, 12288, 36, 32, 8, 128, 151936, 1e6)
    # whole fp16 / fp8 / q4 chunks (1024 B of a row per wave load) in every streamed dimension, an 8 KiB Wo row
    for n in (q.dim, q.hidden_dim, q.q_dim):
        assert n % 512 == 0 and n % 1024 == 0 and n % 2048 == 0
    assert M.row_bytes(M.F16, q.q_dim) == 8192


# ---------------------------------------------------------------- the GPU tests' margins
@pytest.mark.parametrize("name", list(C.CASES))
def test_margins_of_the_gpu_cases(name):
    """Every compared position (1 ..): each wrong model is >= 10 x the GPU test's bar from the
    right one in the per-layer hook's x (bar 1e-4) for every case, and in the logits (bar 1e-3)
    for every case whose logits can show it. q4-2048 (arch_cases.Q4_BIG's shape) cannot: its
    logits are led by the residual stream, and the wrong models move them by 0.9e-3 .. 6.1e-3 of
    their range over the seeds 79, 179 .. 679 (this seed: none 4.4e-3, unit 5.9e-3, swap 2.9e-3,
    reverse 5.2e-3), less with 2, 3 or 4 layers of the same dims (swap 1.1e-3, 7.3e-4, 4.9e-4).
    No smaller multiple is asserted in their place: that case is held by the intermediates the
    GPU test compares -- the layer's x (1.9e-2 .. 4.0e-2 here, 187 .. 400 hook bars) and the K
    row position 0 stored, which every wrong model moves by hundreds of f16 ulps.
    Every greedy step's top-2 gap clears 1e-3 of max|logit| (the GPU tokens are determined)."""
    cfg, _ = C.CASES[name]
    full = C.logits_run(name)
    bf, _, k0 = C.blocks_run(name)
    for wrong in qknorm_ref.WRONG:
        var, bv = C.logits_run(name, wrong), C.blocks_run(name, wrong)
        dl = min(C.relerr(var[pos], full[pos]) for pos in range(C.FIRST, C.N_POS))
        db = min(C.relerr(bv[pos, l], bf[pos, l]) for pos in range(C.FIRST, C.N_POS) for l in range(cfg.n_layers))
        # the K row of position 0 (every layer fed the right model's x): far outside the GPU
        # test's one-ulp bar |d| <= 2^-10 |ref| + 2^-24 on at least a tenth of the row
        m = C.ref(name, wrong)
        x = m.t["model.embed.weight"][C.TOKEN0].copy()
        m.block(0, x, 0, *M.kv_indices(cfg.max_seq_len, 0))
        kw, kf = m.k[0][0].astype(np.float64), k0[0].astype(np.float64)
        far = np.mean(np.abs(kw - kf) > 10 * (2.0 ** -10 * np.abs(kf) + 2.0 ** -24))
        print(f"{name} {wrong}: logits {dl:.2e}, hook {db:.2e}, K row elements past 10 ulp bars {far:.2f}")
        assert db >= 10 * BLOCK_BAR, (wrong, db)
        assert far >= 0.1, (wrong, far)
        if name != "q4-2048":
            assert dl >= 10 * LOGITS_BAR, (wrong, dl)
    toks, lg = C.greedy_run(name)
    srt = np.sort(lg, axis=1)
    gap = (srt[:, -1] - srt[:, -2]) / np.max(np.abs(lg), axis=1)
    assert gap.min() >= 1e-3, gap


@pytest.mark.parametrize("name", ["tiny-f16", "small-f16", "h128-f16"])
def test_position_0_says_nothing(name):
    """Why the logits are compared from position 1: with one key the softmax is 1 and the
    attention output is V, so neither q nor k -- normed or not -- reaches the logits."""
    full = C.logits_run(name)
    for wrong in qknorm_ref.WRONG:
        np.testing.assert_array_equal(C.logits_run(name, wrong)[0], full[0])
        assert C.relerr(C.logits_run(name, wrong)[1], full[1]) > 10 * LOGITS_BAR


@pytest.mark.parametrize("name", sorted(C.SPEC))
def test_spec_cases_have_no_near_tie(name):
    assert C.spec_case(name)[3] >= 2 * LOGITS_BAR


# ---------------------------------------------------------------- converter
@pytest.fixture(scope="module")
def qwen3(tmp_path_factory):
    d = tmp_path_factory.mktemp("qwen3")
    hf = qknorm_hf.write_qwen3(str(d / "hf"))
    out = str(d / "qwen3_fp32.yalm")
    convert.convert(str(d / "hf"), out, "fp32")
    return hf, str(d / "hf"), out


def test_convert_qwen3_norm_tensors(qwen3):
    hf, _, path = qwen3
    yd = read_yalm(path)
    cfg = M.config_from_metadata(yd.metadata, tied="model.output.weight" not in yd.tensors)
    assert yd.metadata["arch"] == "Qwen3ForCausalLM" and yd.metadata["qk_norm"] == "1"
    assert cfg.qk_norm and not cfg.qkv_bias and cfg.rope_scaling is None and cfg.tied
    assert cfg.rope_theta == 1e6 and cfg.head_dim == 16 and cfg.norm_eps == float(np.float32(1e-6))
    assert sorted(k for k in yd.tensors if k != "tokenizer.tokens") == sorted(M.tensor_shapes(cfg))
    assert M.config_from_metadata(cfg.metadata()).qk_norm
    for l in range(cfg.n_layers):
        p, g = f"model.layers.{l}.self_attn.", M.qk_norm_names(l)
        for key, hfn in (("gq", "q_norm"), ("gk", "k_norm")):
            t = yd.tensors[g[key]]
            assert t.dtype == "F32" and tuple(t.shape) == (cfg.head_dim,)
            got, src = np.array(t.data).reshape(-1), hf[p + hfn + ".weight"]
            assert src.min() >= 0.5 and src.max() - src.min() > 1.0  # non-trivial weights
            # one head's rows: HF element i of the first half -> 2 i, of the second half -> 2 i + 1
            half = cfg.head_dim // 2
            np.testing.assert_array_equal(got[0::2], src[:half])
            np.testing.assert_array_equal(got[1::2], src[half:])
            np.testing.assert_array_equal(got, convert.permute_reverse(src[:, None], 1, cfg.rotary_dim)[:, 0])
            assert not np.array_equal(got, src)
    yd.close()


def test_converted_file_is_the_hf_model(qwen3):
    """qknorm_ref on the converted file (interleaved pairs, permuted rows and norm weights)
    against the HF-layout restatement (rotate-half RoPE, the directory's own tensors): the
    permutation moves every norm weight with its element. A file whose norm vectors were left
    in HF order is another model."""
    _, hf_dir, path = qwen3
    cfg, t = arch_hf.load_yalm(path)
    tokens = [3, 100, 24, 7, 310, 55, 9, 201, 42, 17]
    want = qknorm_hf.hf_forward_all(hf_dir, tokens)
    m = qknorm_ref.QKNormRef(cfg, t)
    got = np.array([m.forward(tk, pos) for pos, tk in enumerate(tokens)])
    assert C.relerr(got, want) < 1e-9
    bad = dict(t)
    for l in range(cfg.n_layers):
        for key, hfn in (("gq", "q_norm"), ("gk", "k_norm")):
            yd = read_yalm(os.path.join(hf_dir, "model.safetensors"))
            bad[M.qk_norm_names(l)[key]] = np.array(yd.tensors[f"model.layers.{l}.self_attn.{hfn}.weight"].data).copy()
            yd.close()
    mb = qknorm_ref.QKNormRef(cfg, bad)
    gb = np.array([mb.forward(tk, pos) for pos, tk in enumerate(tokens)])
    assert C.relerr(gb[1:], want[1:]) > 10 * LOGITS_BAR


@pytest.mark.parametrize("dtype", ["fp16", "fp8", "q4"])
def test_convert_qwen3_other_dtypes_keep_f32_norms(tmp_path, dtype):
    hf = qknorm_hf.write_qwen3(str(tmp_path / "hf"), hf=dict(qknorm_hf.QWEN3_HF, **({"hidden_size": 128, "head_dim": 32}
                                                                                   if dtype == "q4" else {})))
    out = str(tmp_path / "q.yalm")
    convert.convert(str(tmp_path / "hf"), out, dtype)
    yd = read_yalm(out)
    t = yd.tensors[M.qk_norm_names(0)["gk"]]
    src = hf["model.layers.0.self_attn.k_norm.weight"]
    assert t.dtype == "F32"
    np.testing.assert_array_equal(np.array(t.data).reshape(-1), convert.permute_reverse(src[:, None], 1, len(src))[:, 0])
    yd.close()


def _config(arch="Qwen3ForCausalLM", **kw):
    return dict(qknorm_hf.QWEN3_HF, architectures=[arch], **kw)


@pytest.mark.parametrize("kw", [
    {"use_sliding_window": True},
    {"layer_types": ["full_attention", "sliding_attention"]},
    {"attention_bias": True},
    {"rope_scaling": {"rope_type": "yarn", "factor": 4.0}},
    {"rope_scaling": {"type": "linear", "factor": 2.0}},
])
def test_convert_refuses(kw):
    with pytest.raises(ValueError):
        convert.metadata_from_config(_config(**kw), "fp16")


def test_convert_accepts_qwen3_and_not_its_moe():
    md = convert.metadata_from_config(_config(), "fp16")
    assert md["qk_norm"] == "1" and md["head_dim"] == "16" and "qkv_bias" not in md
    md = convert.metadata_from_config(_config(layer_types=None), "fp16")
    assert md["qk_norm"] == "1"
    assert "qk_norm" not in convert.metadata_from_config(_config("LlamaForCausalLM"), "fp16")
    with pytest.raises(ValueError):
        convert.metadata_from_config(_config("Qwen3MoeForCausalLM"), "fp16")


def test_host_model_has_no_near_tie(tmp_path):
    """The file of tests/test_host_qknorm.py: the reference's greedy path over the CLI prompt
    clears 1e-3 of max|logit| at every step, and the norm matters to it."""
    qknorm_hf.write_qwen3(str(tmp_path / "hf"))
    out = str(tmp_path / "m.yalm")
    convert.convert(str(tmp_path / "hf"), out, "fp16")
    enc, toks, gap = qknorm_hf.host_reference(out)
    assert gap >= 1e-3 and len(toks) == qknorm_hf.HOST_N, (gap, toks)
    cfg, t = arch_hf.load_yalm(out)
    full, none = qknorm_ref.QKNormRef(cfg, t), qknorm_ref.QKNormRef(cfg, t, wrong="none")
    last = None
    for pos, tk in enumerate(enc + toks[:8]):
        last = (full.forward(tk, pos), none.forward(tk, pos))
    assert C.relerr(last[1], last[0]) >= 10 * LOGITS_BAR
