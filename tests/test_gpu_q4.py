"""GPU: q4 weights (include/yalm_hip.h "q4") through the decode GEMVs, the whole decoder, the
prefill's exact upcast and the refusals. The reference for a q4 model is the CPU oracle (or
the f16 engine) run on its exact f16 twin (models.q4_twin): the value of a q4 weight is
(u - 8) * s, an exact f16, so the twin computes the same function."""
import ctypes

import numpy as np
import pytest

import oracle_py as O
from yalm_amd import models as M

pytestmark = pytest.mark.gpu

REL_TOL = 2e-5  # tests/test_gpu_kernels.py: max|gpu - ref| / max|ref| for fp32-accumulated GEMVs
LP_ATOL = 0.02  # tests/test_gpu_prefill.py: nats, per position


def rt():
    from yalm_amd import runtime

    return runtime


def relerr(a, b):
    return float(np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-30))


def _q4_matrix(rng, d, n, scale):
    return M.q4_quantize(rng.uniform(-scale, scale, size=(d, n)).astype(np.float32))


# (64, 5), (2304, 7), (3072, 4): the generic kernel with a remainder below / above / at half a
# 2048-element chunk; (2048, 3): one chunk, fewer rows than a group; (4096, 1030), (6144, 515):
# the row-block kernel's chunk and whole-row dealing with ragged row groups
@pytest.mark.parametrize("n,d", [(64, 5), (2304, 7), (3072, 4), (2048, 3), (4096, 1030), (6144, 515)])
def test_matmul_shapes(n, d):
    rng = np.random.default_rng(n + d)
    w = _q4_matrix(rng, d, n, 0.02)
    x = rng.standard_normal(n).astype(np.float32)
    g = rt().matmul(x, w, M.Q4)
    ref = M.q4_dequantize(w, n).astype(np.float64) @ x.astype(np.float64)
    err = relerr(g, ref)
    print(f"q4 matmul n={n} d={d}: rel err {err:.3e}")
    assert err < REL_TOL


@pytest.mark.parametrize("n", [64, 2048])
def test_every_nibble_and_scale_exact(n):
    """Row r holds nibble (r + e) % 16 at element e, so every row sees every nibble value and
    every position of a block another one; x is a unit vector, once for each of the 32 positions
    of a block (the last block: the ragged tail of the generic kernel at 64, the last lanes of
    the row-block kernel at 2048) and for the row's first element; each group of a row has
    another scale, among them a subnormal, the smallest and the largest restricted f16. The
    output must be (u - 8) * s bit for bit: a wrong nibble order, offset fold or scale index
    shows."""
    R = rt()
    ng = n // 32
    bits = np.array([0x0008, 0x0400, 0x2C08, 0x3C00, 0x57F8, 0x7BF8, 0x0010, 0x3BF8], np.uint16)
    sb = bits[(np.arange(16)[:, None] + np.arange(ng)[None, :]) % len(bits)]  # row r, group g: scale (r + g) % 8
    u = ((np.arange(16)[:, None] + np.arange(n)[None, :]) % 16).astype(np.uint8)
    w = M.q4_pack(u, sb)
    s = sb.view(np.float16).astype(np.float64)
    for e in [0] + list(range(n - 32, n)):
        x = np.zeros(n, np.float32)
        x[e] = 1.0
        g = R.matmul(x, w, M.Q4)
        ref = ((u[:, e].astype(np.float64) - 8.0) * s[:, e // 32]).astype(np.float32)
        np.testing.assert_array_equal(g, ref, err_msg=f"element {e}")


@pytest.mark.parametrize("act", [M.SILU, M.GELU])
def test_ffn_against_f16_twin(act):
    rng = np.random.default_rng(3)
    dim, hidden = 2048, 4096
    w1, w3 = _q4_matrix(rng, hidden, dim, 1 / 64), _q4_matrix(rng, hidden, dim, 1 / 64)
    w2 = _q4_matrix(rng, dim, hidden, 1 / 120)
    x = rng.standard_normal(dim).astype(np.float32)
    t1, t3 = (M.q4_dequantize(a, dim).astype(np.float16) for a in (w1, w3))
    t2 = M.q4_dequantize(w2, hidden).astype(np.float16)
    err = relerr(rt().ffn(x, w1, w2, w3, act, M.Q4), O.ffn(x, t1, t2, t3, act, M.F16))
    print(f"q4 ffn act={act}: rel err {err:.3e}")
    assert err < 1e-4


def test_synth_device_matches_host_bitwise():
    R = rt()
    rows, n = 37, 2080
    nb = rows * M.row_bytes(M.Q4, n)
    p = R.lib.yalm_alloc(nb + 64)
    try:
        seed = M.synth_seed(9, "q4")
        R.check(R.lib.yalm_synth_q4(p, rows, n, seed, 0.035, None))
        R.check(R.lib.yalm_stream_sync(None))
        host = np.empty(nb + 64, np.uint8)
        R.check(R.lib.yalm_download(host.ctypes.data, p, nb + 64))
        np.testing.assert_array_equal(host[:nb].reshape(rows, -1), M.synth_q4_array(rows, n, seed, 0.035))
        assert not host[nb:].any(), "wrote past the tensor"
        assert R.lib.yalm_synth(p, rows * n, M.Q4, seed, 0.035, 0.0, None) == 2  # needs the row length
    finally:
        R.lib.yalm_free(p)


def _random_q4_model(cfg, seed, scale=0.05):
    """cfg as q4: random f16 weights quantised by q4_quantize, norms around 1."""
    rng = np.random.default_rng(seed)
    c = cfg.with_(weight_dtype=M.Q4)
    t = {}
    for name, (shape, is_norm) in M.tensor_shapes(c).items():
        if is_norm:
            t[name] = (1.0 + 0.1 * rng.standard_normal(shape)).astype(np.float32)
        else:
            t[name] = M.q4_quantize(rng.uniform(-scale, scale, size=shape).astype(np.float16))
    return c, t


def _realistic_q4_model(cfg):
    """models.REALISTIC on cfg, its f16 tensors quantised; None if a matrix quantises to all-zero scales."""
    c16 = cfg.with_(weight_dtype=M.F16)
    t16 = M.synth_host_tensors(c16, seed=2, real=M.REALISTIC)
    c = cfg.with_(weight_dtype=M.Q4)
    t = {}
    for name, (shape, is_norm) in M.tensor_shapes(c).items():
        t[name] = t16[name] if is_norm else M.q4_quantize(t16[name])
        if not is_norm and not M.q4_unpack(t[name], shape[1])[1].any():
            return None
    return c, t


def _check_against_oracle(c, t, positions, start=0, f16_launch_count=True):
    R = rt()
    c16, t16 = M.q4_twin(c, t)
    om = O.OracleModel(c16, t16)
    dm = R.DeviceModel.from_arrays(c, t)
    dec, dec2 = R.Decoder(dm), R.Decoder(dm)
    try:
        assert not dec.attn_wo and dec.kernel_name(3).startswith("gemv_rb_kernel<WQ4")
        tok, seq, worst = 3, [], 0.0
        for pos in range(positions):
            lg = dec.forward(tok, pos).astype(np.float64)
            lo = om.forward(tok, pos).astype(np.float64)
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
        print(f"q4 decoder vs oracle twin over {positions} positions: worst rel err {worst:.3e}")
        # the device loops continue the sequence forward + argmax gives
        assert dec2.generate_greedy(3, 0, positions) == seq
        assert dec2.generate_sampled(3, 0, positions, temperature=0.7, top_k=1, uniforms=np.full(positions, 0.5)) == seq
        if f16_launch_count:  # q4 adds no launches over f16 with separate attention and Wo launches
            dm16 = R.DeviceModel.from_arrays(c16, t16)
            d16 = R.Decoder(dm16, launch=R.LAUNCH_SEPARATE_ATTN_WO)
            try:
                assert dec.graph_kernels(2) == d16.graph_kernels(2)
            finally:
                d16.close()
                dm16.close()
    finally:
        dec.close()
        dec2.close()
        dm.close()


def test_small_model_vs_oracle_twin():
    c, t = _random_q4_model(M.SMALL, seed=1)
    _check_against_oracle(c, t, 8)


def test_tiny_dims_model_vs_oracle_twin():
    """dim 64, hidden 128: every GEMV on the generic kernel (rows shorter than a chunk)."""
    c, t = _random_q4_model(M.TINY, seed=2, scale=0.2)
    _check_against_oracle(c, t, 8)


def test_realistic_small_model_vs_oracle_twin():
    m = _realistic_q4_model(M.SMALL)
    assert m is not None, "models.REALISTIC on SMALL quantised to an all-zero matrix"
    _check_against_oracle(*m, 8, f16_launch_count=False)


def test_tied_classifier_reads_the_q4_embedding():
    """The embedding row is dequantised by the step kernel and the tied classifier streams the
    same q4 tensor: the first position's logits against the oracle twin (Llama-3.2 layout)."""
    c, t = _random_q4_model(M.SMALL.with_(tied=True, dim=576, n_heads=9, n_kv_heads=3), seed=5)
    assert "model.output.weight" not in t
    _check_against_oracle(c, t, 2, f16_launch_count=False)


def test_sliding_window_past_max_seq_len():
    c, t = _random_q4_model(M.SMALL.with_(max_seq_len=32, n_layers=2), seed=6)
    _check_against_oracle(c, t, 41, start=30, f16_launch_count=False)


PF_CFG = M.ModelConfig(dim=512, hidden_dim=1024, head_dim=128, n_layers=3, n_heads=4, n_kv_heads=2, vocab_size=1024,
                       max_seq_len=320, rope_theta=1e6, act=M.SILU, weight_dtype=M.F16)


def _decode_logprobs(dec, tokens):
    lp = []
    for pos, t in enumerate(tokens[:-1]):
        logits = dec.forward(int(t), pos).astype(np.float64)
        m = logits.max()
        lp.append(logits[tokens[pos + 1]] - m - np.log(np.exp(logits - m).sum()))
    return np.array(lp)


@pytest.mark.parametrize("n", [13, 40])
def test_prefill_equals_f16_twin(n):
    """The contract of test_gpu_prefill.py::test_fp8_prefill_equals_f16_twin for q4: log p and
    every K / V cache row bit for bit the f16 twin's; log p within LP_ATOL of the q4 decode
    engine; the decode step after the prefill matches the all-decode run."""
    c4, t4 = _random_q4_model(PF_CFG, seed=11, scale=0.035)
    c16, t16 = M.q4_twin(c4, t4)
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
        print(f"q4 prefill n={n}: max |log p prefill - decode| {err:.3e}")
        assert err <= LP_ATOL
        dd.forward(int(tokens[-1]), n - 1)
        lg_p, lg_d = d4.forward(7, n), dd.forward(7, n)
        assert relerr(lg_p, lg_d) < 5e-3  # tests/test_gpu_prefill.py: f16 MFMA activations in the cache rows
    finally:
        for h in (d4, d16, dd, dm4, dm16):
            h.close()
        for p in caches[0] + caches[1]:
            R.lib.yalm_free(p)


def test_refusals_name_q4():
    R = rt()
    cfg = M.SMALL.with_(weight_dtype=M.Q4)
    cc = R.Config.from_model(cfg)
    blocks = (R.BlockWeights * cfg.n_layers)()
    mw = R.ModelWeights(None, None, None, blocks)
    h = ctypes.c_void_p()
    dummy = ctypes.create_string_buffer(1024)
    moe = (ctypes.c_int * 2)(4, 2)
    gates = (ctypes.c_void_p * cfg.n_layers)(*[ctypes.addressof(dummy)] * cfg.n_layers)

    def refused(rc):
        assert rc == 3, rc
        assert "q4" in R.lib.yalm_last_error().decode()

    refused(R.lib.yalm_decoder_create_moe(ctypes.byref(cc), moe, ctypes.byref(mw), gates, None, ctypes.byref(h)))
    refused(R.lib.yalm_decoder_create_tp_ipc(ctypes.byref(cc), ctypes.byref(mw), 0, 2, dummy, dummy, None,
                                            ctypes.byref(h)))
    refused(R.lib.yalm_decoder_create_tp(ctypes.byref(cc), ctypes.byref(mw), 0, 2, dummy, None, ctypes.byref(h)))
    x = np.zeros(64, np.float32)
    w = np.zeros((4, 128, M.row_bytes(M.Q4, 64)), np.uint8)
    with pytest.raises(R.YalmError, match="error 3.*q4"):
        R.moe_ffn(x, np.zeros((4, M.row_bytes(M.Q4, 64)), np.uint8), w, w, w, 2, M.SILU, M.Q4)
    with pytest.raises(R.YalmError, match="error 3.*q4"):
        R.moe_ffn_rows(x[None, :], np.zeros((4, M.row_bytes(M.Q4, 64)), np.uint8), w, w, w, 2, M.SILU, M.Q4)
    # a q4 config whose dim is no multiple of the scale group: an argument error
    bad = M.TINY.with_(weight_dtype=M.Q4, dim=80, n_heads=5, head_dim=16, n_kv_heads=5)
    cb = R.Config.from_model(bad)
    bb = (R.BlockWeights * bad.n_layers)()
    mb = R.ModelWeights(None, None, None, bb)
    assert R.lib.yalm_decoder_create(ctypes.byref(cb), ctypes.byref(mb), None, ctypes.byref(h)) == 2
    assert "q4" in R.lib.yalm_last_error().decode()
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


def test_time_kernel_and_gemv_config_on_q4():
    """yalm_time_kernel ids 0, 2, 3, 4, 5 and yalm_set_gemv_config run on a q4 decoder, and
    another geometry gives the same logits within the f32 summation order."""
    R = rt()
    cfg = M.ModelConfig(dim=2048, hidden_dim=4096, head_dim=128, n_layers=2, n_heads=16, n_kv_heads=4,
                        vocab_size=2048, max_seq_len=64, weight_dtype=M.Q4)
    dm = R.DeviceModel.synthetic(cfg, seed=3)
    dec = R.Decoder(dm)
    try:
        base = dec.forward(1, 0)
        assert np.all(np.isfinite(base))
        for kid in (0, 2, 3, 4, 5):
            assert dec.time_kernel(kid, 2) > 0
            assert "WQ4" in dec.kernel_name(kid)
        for kind in range(5):
            dec.set_gemv_config(kind, 256, 8, 2)
        assert relerr(dec.forward(1, 0), base) < 1e-4
    finally:
        dec.close()
        dm.close()
