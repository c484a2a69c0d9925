"""GPU: e4m3 weights (include/yalm_hip.h "e4m3": OCP E4M3 codes with one power-of-two f32 scale
per row) through the decode GEMVs, the multi-row kernel, the fused attention + Wo launch, the
whole decoder, the prefill's exact upcast, the synthesiser and the refusals. The reference for
an e4m3 model is the CPU oracle (or the f16 engine) run on its exact f16 twin (models.e4m3_twin):
code * 2^k is an exact f16 for the quantiser's k, so the twin computes the same function."""
import ctypes

import numpy as np
import pytest

import arch_cases as A
import arch_ref
import oracle_py as O
import qknorm_cases as Q
import qknorm_ref
from yalm_amd import models as M

pytestmark = pytest.mark.gpu

REL_TOL = 2e-5  # tests/test_gpu_kernels.py: max|gpu - ref| / max|ref| for fp32-accumulated GEMVs
LP_ATOL = 0.02  # tests/test_gpu_prefill.py: nats, per position
ROWS_GLU_TOL = {M.SILU: 2e-5, M.GELU: 2.51e-5}  # tests/rows_ref.py REL_TOL / GELU_GLU_REL_TOL
SENTINEL = np.float32(-7.25)  # tests/rows_ref.py


def rt():
    from yalm_amd import runtime

    return runtime


def relerr(a, b):
    return float(np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-30))


def _e4m3_matrix(rng, d, n, scale):
    """Random weights, every row at a gain of its own (so every row has a scale of its own)."""
    gain = 2.0 ** rng.integers(-3, 3, size=(d, 1))
    return M.e4m3_quantize((rng.uniform(-scale, scale, size=(d, n)) * gain).astype(np.float16))


# ------------------------------------------------------------------ 1. every code, every kernel path
@pytest.mark.parametrize("n", [48, 1040, 1024, 2048])
def test_every_code_and_scale_exact(n):
    """Row r holds code r at every element and the scale 2^((r % 23) - 15); x is a unit vector
    at the row's first element and at each of its last 16 (n = 48: a row shorter than a chunk,
    1040: the generic kernel's ragged tail; 1024, 2048: the row-block kernel's last lanes). The
    output must be code(r) * s_r bit for bit, NaN for the two NaN codes: a wrong builtin, byte
    order, scale address or a neighbouring row's scale shows."""
    R = rt()
    codes = np.repeat(np.arange(256, dtype=np.uint8)[:, None], n, axis=1)
    s = (2.0 ** ((np.arange(256) % 23) - 15.0)).astype(np.float32)
    w = M.e4m3_pack(codes, s)
    want = (M.e4m3_table().astype(np.float64) * s.astype(np.float64)).astype(np.float32)
    nan = np.isnan(want)
    assert np.flatnonzero(nan).tolist() == [0x7F, 0xFF]
    for e in [0] + list(range(n - 16, n)):
        x = np.zeros(n, np.float32)
        x[e] = 1.0
        g = R.matmul(x, w, M.E4M3)
        assert np.isnan(g[nan]).all(), f"element {e}: the NaN codes"
        np.testing.assert_array_equal(g[~nan], want[~nan], err_msg=f"element {e}")


# ------------------------------------------------------------------ 2. yalm_matmul, yalm_ffn
# n on both sides of the 1024-element chunk: (48, 5), (1040, 7), (1536, 4): the generic kernel
# with a row below a chunk and a remainder of 16 / half a chunk; (1024, 3): one chunk, fewer rows
# than a group; (4096, 1030), (3072, 515): the row-block kernel's chunk and whole-row dealing
# with ragged row groups
@pytest.mark.parametrize("n,d", [(48, 5), (1040, 7), (1536, 4), (1024, 3), (4096, 1030), (3072, 515)])
def test_matmul_shapes(n, d):
    rng = np.random.default_rng(n + d)
    w = _e4m3_matrix(rng, d, n, 0.02)
    x = rng.standard_normal(n).astype(np.float32)
    g = rt().matmul(x, w, M.E4M3)
    ref = M.e4m3_dequantize(w, n).astype(np.float64) @ x.astype(np.float64)
    err = relerr(g, ref)
    print(f"e4m3 matmul n={n} d={d}: rel err {err:.3e}")
    assert err < REL_TOL


@pytest.mark.parametrize("act", [M.SILU, M.GELU])
def test_ffn_against_f16_twin(act):
    rng = np.random.default_rng(3)
    dim, hidden = 2048, 4096
    w1, w3 = _e4m3_matrix(rng, hidden, dim, 1 / 64), _e4m3_matrix(rng, hidden, dim, 1 / 64)
    w2 = _e4m3_matrix(rng, dim, hidden, 1 / 120)
    x = rng.standard_normal(dim).astype(np.float32)
    t1, t3 = (M.e4m3_dequantize(a, dim).astype(np.float16) for a in (w1, w3))
    t2 = M.e4m3_dequantize(w2, hidden).astype(np.float16)
    err = relerr(rt().ffn(x, w1, w2, w3, act, M.E4M3), O.ffn(x, t1, t2, t3, act, M.F16))
    print(f"e4m3 ffn act={act}: rel err {err:.3e}")
    assert err < 1e-4


# ------------------------------------------------------------------ 3. the whole decoder
def _quantised(c16, t16):
    """An f16 model's tensors quantised: (e4m3 config, tensors)."""
    c = c16.with_(weight_dtype=M.E4M3)
    return c, {name: (t16[name] if is_norm else M.e4m3_quantize(t16[name]))
               for name, (shape, is_norm) in M.tensor_shapes(c).items()}


def _random_e4m3_model(cfg, seed, scale=0.05):
    """cfg as e4m3: random f16 weights with a gain per row, quantised; norms around 1."""
    rng = np.random.default_rng(seed)
    c = cfg.with_(weight_dtype=M.E4M3)
    t = {}
    for name, (shape, is_norm) in M.tensor_shapes(c).items():
        if is_norm:
            t[name] = (1.0 + 0.1 * rng.standard_normal(shape)).astype(np.float32)
        else:
            t[name] = _e4m3_matrix(rng, shape[0], shape[1], scale)
    return c, t


def _check_against_reference(c, t, ref, positions, start=0, rb_kernel=None, fp8_launch_count=True, attn_wo=False):
    """test_gpu_q4.py's _check_against_oracle for e4m3: ref.forward(token, pos) gives the f16
    twin's logits. Logits within 1e-3 relative, the argmax equal or a near-tie, the greedy and
    sampled device loops continue the same sequence, as many launches per token as fp8."""
    R = rt()
    dm = R.DeviceModel.from_arrays(c, t)
    dec, dec2 = R.Decoder(dm), R.Decoder(dm)
    try:
        assert dec.attn_wo == attn_wo
        if rb_kernel is not None:
            assert dec.kernel_name(3).startswith("gemv_rb_kernel<WE4M3") == rb_kernel
            assert "WE4M3" in dec.kernel_name(3)
        tok, seq, worst = 3, [], 0.0
        for pos in range(positions):
            lg = dec.forward(tok, pos).astype(np.float64)
            lo = np.asarray(ref.forward(tok, pos), np.float64)
            if pos >= start:
                err = relerr(lg, lo)
                worst = max(worst, err)
                assert err < 1e-3, (pos, err)
                tg, to = int(np.argmax(lg)), int(np.argmax(lo))
                if tg != to:
                    top = np.sort(lo)[-2:]
                    assert (top[1] - top[0]) / np.max(np.abs(lo)) < 1e-3, (pos, tg, to)
            tok = int(np.argmax(lg))
            seq.append(tok)
        print(f"e4m3 decoder vs twin over {positions} positions: worst rel err {worst:.3e}")
        assert dec2.generate_greedy(3, 0, positions) == seq
        assert dec2.generate_sampled(3, 0, positions, temperature=0.7, top_k=1, uniforms=np.full(positions, 0.5)) == seq
        if fp8_launch_count:
            c8 = c.with_(weight_dtype=M.F8E5M2)
            dm8 = R.DeviceModel.synthetic(c8, seed=1)
            d8 = R.Decoder(dm8)
            try:
                assert dec.graph_kernels(2) == d8.graph_kernels(2)
            finally:
                d8.close()
                dm8.close()
    finally:
        dec.close()
        dec2.close()
        dm.close()


def _check_against_oracle(c, t, positions, **kw):
    c16, t16 = M.e4m3_twin(c, t)
    _check_against_reference(c, t, O.OracleModel(c16, t16), positions, **kw)


def test_small_model_vs_oracle_twin():
    c, t = _random_e4m3_model(M.SMALL, seed=1)
    _check_against_oracle(c, t, 8, rb_kernel=True)


def test_tiny_dims_model_vs_oracle_twin():
    """dim 64, hidden 128: every GEMV on the generic kernel (rows shorter than a chunk)."""
    c, t = _random_e4m3_model(M.TINY, seed=2, scale=0.2)
    _check_against_oracle(c, t, 8)


def test_realistic_small_model_vs_oracle_twin():
    t16 = M.synth_host_tensors(M.SMALL, seed=2, real=M.REALISTIC)
    c, t = _quantised(M.SMALL, t16)
    _check_against_oracle(c, t, 8, fp8_launch_count=False)


def test_tied_classifier_reads_the_e4m3_embedding():
    """The embedding row is dequantised by the step kernel and the tied classifier streams the
    same e4m3 tensor (Llama-3.2 layout, dim 576: the generic kernel)."""
    c, t = _random_e4m3_model(M.SMALL.with_(tied=True, dim=576, n_heads=9, n_kv_heads=3), seed=5)
    assert "model.output.weight" not in t
    _check_against_oracle(c, t, 2, fp8_launch_count=False)


def test_sliding_window_past_max_seq_len():
    c, t = _random_e4m3_model(M.SMALL.with_(max_seq_len=32, n_layers=2), seed=6)
    _check_against_oracle(c, t, 41, start=30, fp8_launch_count=False)


def test_qkv_bias_model_vs_reference_twin():
    """tests/arch_cases.py "bias-small-f16" quantised: PQKVB on the row-block kernel."""
    c16, seed, _ = A.CASES["bias-small-f16"]
    c, t = _quantised(c16, M.synth_host_tensors(c16, seed=seed))
    c16t, t16 = M.e4m3_twin(c, t)
    _check_against_reference(c, t, arch_ref.ArchRef(c16t, t16), 10, rb_kernel=True)


def test_qk_norm_model_vs_reference_twin():
    """tests/qknorm_cases.py "small-f16" quantised: PQKVN and the q / k norm launch."""
    c16, seed = Q.CASES["small-f16"]
    c, t = _quantised(c16, M.synth_host_tensors(c16, seed=seed))
    c16t, t16 = M.e4m3_twin(c, t)
    _check_against_reference(c, t, qknorm_ref.QKNormRef(c16t, t16), 10, rb_kernel=True)


# ------------------------------------------------------------------ 4. fused attention + Wo
# tests/test_gpu_attn_wo.py's BASE and its two fp8 cases, as e4m3
AWO_BASE = M.ModelConfig(dim=1024, hidden_dim=2048, head_dim=128, n_layers=3, n_heads=16, n_kv_heads=4,
                         vocab_size=1536, max_seq_len=72, rope_theta=10000.0, act=M.SILU, weight_dtype=M.F16)
AWO_CASES = {"xs1-g4": AWO_BASE.with_(n_heads=32, n_kv_heads=8), "xs2-g2": AWO_BASE.with_(n_heads=64, n_kv_heads=32)}


@pytest.mark.parametrize("name", sorted(AWO_CASES))
def test_attn_wo_fused_vs_oracle_twin_and_separate_launches(name):
    R = rt()
    c, t = _random_e4m3_model(AWO_CASES[name], seed=7, scale=0.035)
    _check_against_oracle(c, t, 12, attn_wo=True)
    dm = R.DeviceModel.from_arrays(c, t)
    dec, sep = R.Decoder(dm), R.Decoder(dm, launch=R.LAUNCH_SEPARATE_ATTN_WO)
    try:
        assert dec.attn_wo and not sep.attn_wo
        assert dec.kernel_name(8).startswith("attn_wo_kernel<WE4M3")
        tok, worst = 11, 0.0
        for pos in range(24):
            a, b = dec.forward(tok, pos), sep.forward(tok, pos)
            worst = max(worst, relerr(a, b), relerr(dec.get_x(), sep.get_x()))
            assert worst < 1e-4, (pos, worst)  # tests/test_gpu_attn_wo.py: fused against separate
            tok = int(np.argmax(b))
        print(f"e4m3 {name}: fused vs separate launches, worst rel err {worst:.3e}")
    finally:
        dec.close()
        sep.close()
        dm.close()


# ------------------------------------------------------------------ 5. the multi-row kernel by itself
def _rows_case(rng, T, n, d, ostride, epilogue, act=M.SILU):
    codes = M.e4m3_encode(rng.integers(-3, 4, (d, n)).astype(np.float64))
    s = (2.0 ** ((np.arange(d) % 7) - 3.0)).astype(np.float32)  # row j: 2^((j % 7) - 3)
    w = M.e4m3_pack(codes, s)
    wv = M.e4m3_dequantize(w, n).astype(np.float64)
    x = (rng.integers(-4, 5, (T, n)) * np.array([1.0, 2.0, 4.0, 8.0])[:T, None]).astype(np.float32)
    out0 = np.full((T, ostride), SENTINEL, np.float32)
    out0[:, :d] = rng.integers(-999, 1000, (T, d))
    a = x.astype(np.float64) @ wv.T
    return w, wv, x, out0, a


@pytest.mark.parametrize("n,Ts,nseg", [(1040, (1, 2, 3, 4), 1), (9216, (4,), 2)])
def test_matmul_rows_exact_and_glu(n, Ts, nseg):
    """Integer-valued codes and x (every partial sum an integer below 2^24, the row scales powers
    of two): STORE and RESIDUAL bit for bit at any summation order; GLU against float64 at
    tests/test_gpu_rows.py's bar. x staged whole (n = 1040: a chunk and a ragged end) and in two
    segments (n = 9216 at T = 4); an odd row count and a padded ostride whose sentinels must come
    back untouched."""
    R = rt()
    d, ostride = 37, 44
    for T in Ts:
        assert R.rows_plan(M.E4M3, n, (d + 1) // 2, T, 0)["nseg"] == nseg
        rng = np.random.default_rng(1000 * n + T)
        for epi in (R.ROWS_STORE, R.ROWS_RESIDUAL):
            w, wv, x, out0, a = _rows_case(rng, T, n, d, ostride, epi)
            assert (np.abs(x.astype(np.float64)) @ np.abs(wv).T).max() + 1000 < 2 ** 24
            got = R.matmul_rows(out0, x, w, M.E4M3, epi)
            want = out0.astype(np.float64)
            want[:, :d] = a if epi == R.ROWS_STORE else want[:, :d] + a
            np.testing.assert_array_equal(got, want.astype(np.float32), err_msg=f"T {T} epilogue {epi}")
            assert np.all(got[:, d:].view(np.uint32) == SENTINEL.view(np.uint32))
        for act in (M.SILU, M.GELU):
            w, wv, x, out0, a = _rows_case(rng, T, n, d, ostride, R.ROWS_GLU)
            w3 = _e4m3_matrix(rng, d, n, 0.035)
            x = (x * np.float32(0.01)).astype(np.float32)
            a = x.astype(np.float64) @ wv.T
            b = x.astype(np.float64) @ M.e4m3_dequantize(w3, n).astype(np.float64).T
            if act == M.SILU:
                want = a / (1.0 + np.exp(-a)) * b
            else:
                c0, c1 = float(np.float32(0.797885)), float(np.float32(0.044715))
                want = 0.5 * a * (1.0 + np.tanh(c0 * (a + c1 * a * a * a))) * b
            got = R.matmul_rows(out0, x, w, M.E4M3, R.ROWS_GLU, w3=w3, act=act)
            err = float((np.abs(got[:, :d] - want).max(axis=1) / np.abs(want).max(axis=1)).max())
            print(f"e4m3 rows GLU act={act} T={T} n={n}: {err:.3e}")
            assert err <= ROWS_GLU_TOL[act]
            assert np.all(got[:, d:].view(np.uint32) == SENTINEL.view(np.uint32))


# ------------------------------------------------------------------ 6. forward_rows, generate_speculative
def test_forward_rows_equals_single_forwards():
    R = rt()
    c, t = _random_e4m3_model(M.SMALL, seed=1)
    dm = R.DeviceModel.from_arrays(c, t)
    prompt = [1, 17, 300, 5, 42, 9, 250, 33, 2, 77]
    try:
        one = R.Decoder(dm)
        single = [one.forward(tok, p).copy() for p, tok in enumerate(prompt)]
        one.close()
        for pos in (0, 5):
            for T in (2, 3, 4):
                dec = R.Decoder(dm)
                try:
                    for p in range(pos):
                        dec.forward(prompt[p], p, R.HYDRATE_KV_CACHE)
                    lg = dec.forward_rows(prompt[pos:pos + T], pos)
                    for i in range(T):
                        e = relerr(lg[i], single[pos + i])
                        assert e < 1e-3, (pos, T, i, e)  # tests/test_gpu_spec.py's rows bar
                    assert relerr(dec.forward(prompt[pos + T], pos + T), single[pos + T]) < 1e-3
                finally:
                    dec.close()
    finally:
        dm.close()


def test_speculative_equals_plain_greedy():
    R = rt()
    c, t = _random_e4m3_model(M.SMALL, seed=1)
    dm = R.DeviceModel.from_arrays(c, t)
    prompt, n_gen = [1, 17, 300, 5, 42, 9], 24
    pos = len(prompt) - 1

    def hydrated():
        dec = R.Decoder(dm)
        for p, tok in enumerate(prompt[:-1]):
            dec.forward(tok, p, R.HYDRATE_KV_CACHE)
        return dec

    try:
        plain_dec = hydrated()
        plain = plain_dec.generate_greedy(prompt[-1], pos, n_gen)
        plain_dec.close()
        streams = {"true": plain, "wrong": [(tk + 1) % c.vocab_size for tk in plain]}
        for rows in (2, 4):
            for kind, stream in streams.items():
                dec = hydrated()
                try:
                    got, st = dec.generate_speculative(prompt[-1], pos, n_gen, rows=rows, ngram_max=3, ngram_min=1,
                                                       context=prompt, draft_stream=stream)
                    print(f"e4m3 speculative rows {rows} {kind}: {st}")
                    assert got == plain, (rows, kind)
                    if kind == "wrong":
                        assert st["accepted_drafts"] == 0
                    else:
                        assert st["accepted_drafts"] > 0
                finally:
                    dec.close()
    finally:
        dm.close()


# ------------------------------------------------------------------ 7. prefill
PF_CFG = M.ModelConfig(dim=512, hidden_dim=1024, head_dim=128, n_layers=3, n_heads=4, n_kv_heads=2, vocab_size=1024,
                       max_seq_len=320, rope_theta=1e6, act=M.SILU, weight_dtype=M.F16)  # tests/test_gpu_q4.py


def _decode_logprobs(dec, tokens):
    lp = []
    for pos, t in enumerate(tokens[:-1]):
        logits = dec.forward(int(t), pos).astype(np.float64)
        m = logits.max()
        lp.append(logits[tokens[pos + 1]] - m - np.log(np.exp(logits - m).sum()))
    return np.array(lp)


@pytest.mark.parametrize("n", [13, 300])
def test_prefill_equals_f16_twin(n):
    """log p and every K / V cache row bit for bit the f16 twin's; log p within LP_ATOL of the
    e4m3 decode path."""
    c4, t4 = _random_e4m3_model(PF_CFG, seed=11, scale=0.035)
    c16, t16 = M.e4m3_twin(c4, t4)
    R = rt()
    dm4, dm16 = R.DeviceModel.from_arrays(c4, t4), R.DeviceModel.from_arrays(c16, t16)
    kvb = c4.max_seq_len * c4.kv_dim * 2
    caches = [[R.lib.yalm_alloc(kvb) for _ in range(2 * c4.n_layers)] for _ in range(2)]
    d4 = R.Decoder(dm4, kv_caches=list(zip(caches[0][0::2], caches[0][1::2])))
    d16 = R.Decoder(dm16, kv_caches=list(zip(caches[1][0::2], caches[1][1::2])))
    dd = R.Decoder(dm4)
    try:
        tokens = np.random.default_rng(31 + n).integers(0, c4.vocab_size, size=n).astype(np.int32)
        lp4, lp16 = d4.prefill(tokens), d16.prefill(tokens)
        np.testing.assert_array_equal(lp4, lp16)
        for p4, p16 in zip(caches[0], caches[1]):
            a, b = np.empty(kvb, np.uint8), np.empty(kvb, np.uint8)
            R.check(R.lib.yalm_download(a.ctypes.data, p4, kvb))
            R.check(R.lib.yalm_download(b.ctypes.data, p16, kvb))
            np.testing.assert_array_equal(a, b)
        err = float(np.max(np.abs(lp4[: n - 1] - _decode_logprobs(dd, tokens))))
        print(f"e4m3 prefill n={n}: max |log p prefill - decode| {err:.3e}")
        assert err <= LP_ATOL
    finally:
        for h in (d4, d16, dd, dm4, dm16):
            h.close()
        for p in caches[0] + caches[1]:
            R.lib.yalm_free(p)


# ------------------------------------------------------------------ 8. the synthesiser
def test_synth_device_matches_host_bitwise():
    R = rt()
    rows, n = 37, 2064
    nb = rows * M.row_bytes(M.E4M3, n)
    p = R.lib.yalm_alloc(nb + 64)
    try:
        seed = M.synth_seed(9, "e4m3")
        R.check(R.lib.yalm_synth_e4m3(p, rows, n, seed, 0.035, None))
        R.check(R.lib.yalm_stream_sync(None))
        host = np.empty(nb + 64, np.uint8)
        R.check(R.lib.yalm_download(host.ctypes.data, p, nb + 64))
        np.testing.assert_array_equal(host[:nb].reshape(rows, -1), M.synth_e4m3_array(rows, n, seed, 0.035))
        assert not host[nb:].any(), "wrote past the tensor"
        assert R.lib.yalm_synth(p, rows * n, M.E4M3, seed, 0.035, 0.0, None) == 2  # needs the row length
        assert "e4m3" in R.lib.yalm_last_error().decode()
    finally:
        R.lib.yalm_free(p)


def test_synthetic_model_time_kernel_and_gemv_config():
    """DeviceModel.synthetic, yalm_time_kernel ids 0, 2, 3, 4, 5 and yalm_set_gemv_config on an
    e4m3 decoder; another geometry gives the same logits within the f32 summation order."""
    R = rt()
    cfg = M.ModelConfig(dim=2048, hidden_dim=4096, head_dim=64, n_layers=2, n_heads=32, n_kv_heads=8,
                        vocab_size=2048, max_seq_len=64, weight_dtype=M.E4M3)
    dm = R.DeviceModel.synthetic(cfg, seed=3)
    dec = R.Decoder(dm)
    try:
        base = dec.forward(1, 0)
        assert np.all(np.isfinite(base))
        for kid in (0, 2, 3, 4, 5):
            assert dec.time_kernel(kid, 2) > 0
            assert "WE4M3" in dec.kernel_name(kid)
        for kind in range(5):
            dec.set_gemv_config(kind, 256, 8, 2)
        assert relerr(dec.forward(1, 0), base) < 1e-4
    finally:
        dec.close()
        dm.close()


# ------------------------------------------------------------------ 9. refusals
def test_refusals_name_e4m3():
    R = rt()
    cfg = M.SMALL.with_(weight_dtype=M.E4M3)
    cc = R.Config.from_model(cfg)
    blocks = (R.BlockWeights * cfg.n_layers)()
    mw = R.ModelWeights(None, None, None, blocks)
    h = ctypes.c_void_p()
    dummy = ctypes.create_string_buffer(1024)
    moe = (ctypes.c_int * 2)(4, 2)
    gates = (ctypes.c_void_p * cfg.n_layers)(*[ctypes.addressof(dummy)] * cfg.n_layers)

    def refused(rc):
        assert rc == 3, rc
        assert "e4m3" in R.lib.yalm_last_error().decode()

    refused(R.lib.yalm_decoder_create_moe(ctypes.byref(cc), moe, ctypes.byref(mw), gates, None, ctypes.byref(h)))
    refused(R.lib.yalm_decoder_create_tp_ipc(ctypes.byref(cc), ctypes.byref(mw), 0, 2, dummy, dummy, None,
                                            ctypes.byref(h)))
    refused(R.lib.yalm_decoder_create_tp(ctypes.byref(cc), ctypes.byref(mw), 0, 2, dummy, None, ctypes.byref(h)))
    x = np.zeros(64, np.float32)
    w = np.zeros((4, 128, M.row_bytes(M.E4M3, 64)), np.uint8)
    with pytest.raises(R.YalmError, match="error 3.*e4m3"):
        R.moe_ffn(x, np.zeros((4, M.row_bytes(M.E4M3, 64)), np.uint8), w, w, w, 2, M.SILU, M.E4M3)
    with pytest.raises(R.YalmError, match="error 3.*e4m3"):
        R.moe_ffn_rows(x[None, :], np.zeros((4, M.row_bytes(M.E4M3, 64)), np.uint8), w, w, w, 2, M.SILU, M.E4M3)
    # a config whose dim is no multiple of 16: an argument error
    bad = M.TINY.with_(weight_dtype=M.E4M3, dim=72, n_heads=4, head_dim=16, n_kv_heads=4)
    cb = R.Config.from_model(bad)
    bb = (R.BlockWeights * bad.n_layers)()
    mb = R.ModelWeights(None, None, None, bb)
    assert R.lib.yalm_decoder_create(ctypes.byref(cb), ctypes.byref(mb), None, ctypes.byref(h)) == 2
    # an f16 decoder made afterwards still works
    c16 = M.TINY
    dm = R.DeviceModel.synthetic(c16, seed=1)
    dec = R.Decoder(dm)
    try:
        om = O.OracleModel(c16, O.synth_host_tensors_fast(c16, seed=1))
        assert relerr(dec.forward(5, 0), om.forward(5, 0)) < 1e-3
    finally:
        dec.close()
        dm.close()
