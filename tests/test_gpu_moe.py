"""Mixture-of-experts decode on the GPU (moe.h) against the composed CPU reference
(tests/moe_ref.py: the dense oracle's pieces + a restatement of the reference's moe_gate).

Bars: the expert FFN as the dense ffn parity test (test_gpu_kernels.py: 1e-4 of max|ref|), a
block as the dense per-layer test (test_gpu_decode.py: 1e-4), logits 1e-3; the routing is exact
(experts identical, in selection order) with weights within 1e-5 on the same input (and within
weight_tol() where the router's input already carries earlier error) -- every input's router logits
clear a 1e-3 margin (test_moe_cpu.py), ~50x the GEMV parity, so no selection hangs on rounding.
"""
import functools
import os

import numpy as np
import pytest

import moe_ref as R
import oracle_py as O
from yalm_amd import models as M

pytestmark = pytest.mark.gpu

FFN_TOL = 1e-4    # test_gpu_kernels.py test_ffn_mistral_shape
BLOCK_TOL = 1e-4  # test_gpu_decode.py test_block_by_block
LOGITS_TOL = 1e-3  # test_gpu_decode.py test_forward_logits_and_greedy
WEIGHT_TOL = 1e-5  # yalm_moe_ffn: both sides route the same x


def weight_tol(logits, bar):
    """Routing weights inside a block / forward, where the router reads a hidden state that
    already carries the attention half's (or the earlier layers') error: a router logit is a
    GEMV on the normalised x like the classifier's, so it may move by bar * max|logit| (the
    project's bar on such outputs), and softmax weights move by at most half the largest logit
    shift: |dw_i| = w_i |d_i - sum_j w_j d_j| <= w_i (1 - w_i) * 2 eps <= eps / 2."""
    return 0.5 * bar * float(np.max(np.abs(logits)))


def rt():
    from yalm_amd import runtime

    return runtime


def relerr(a, b):
    return float(np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-30))


# ---------------------------------------------------------------- 1. yalm_moe_ffn
@pytest.mark.parametrize("case", R.FFN_CASES, ids=[c[0] for c in R.FFN_CASES])
def test_moe_ffn_matches_reference(case):
    _, dim, hidden, E, K, dtype, act, _ = case
    x, gate, w1, w2, w3 = R.ffn_case_inputs(case)
    want, experts, weights, _ = R.moe_ffn(x, gate, w1, w2, w3, K, act, dtype)
    got, ge, gw = rt().moe_ffn(x, gate, w1, w2, w3, K, act, dtype)
    e = relerr(got, want)
    print(f"{case[0]}: experts {ge.tolist()} rel err {e:.2e} max weight err {np.max(np.abs(gw - weights)):.1e}")
    assert ge.tolist() == experts.tolist()
    assert np.max(np.abs(gw - weights)) <= WEIGHT_TOL
    assert e < FFN_TOL


# ---------------------------------------------------------------- 2. exact ties
@pytest.mark.parametrize("dim,hidden,dtype", [(64, 128, M.F32), (512, 1536, M.F16)], ids=["generic-f32", "rb-f16"])
def test_exact_ties_lowest_index_first(dim, hidden, dtype):
    """Two identical moegate rows: their logits come from the same code on the same bytes, so
    they are bit-equal, and the strict '>' scan must take the lower index first."""
    E, K = 6, 3
    rng = np.random.default_rng(21)
    x = rng.standard_normal(dim, dtype=np.float32)
    g = rng.standard_normal((E, dim), dtype=np.float32) * np.float32(1.0 / np.sqrt(dim))
    g[4] = x * np.float32(2.0 / np.sqrt(dim))  # by far the largest logit ...
    g[1] = g[4]                                 # ... twice
    gate = M.encode_weights(g, dtype)
    assert np.array_equal(gate[1], gate[4])

    def w(shape, s):
        return M.encode_weights(rng.standard_normal(shape, dtype=np.float32) * np.float32(s), dtype)

    w1, w3, w2 = w((E, hidden, dim), dim ** -0.5), w((E, hidden, dim), dim ** -0.5), w((E, dim, hidden), hidden ** -0.5)
    want, experts, weights, logits = R.moe_ffn(x, gate, w1, w2, w3, K, M.SILU, dtype)
    assert logits[1] == logits[4] and experts.tolist()[:2] == [1, 4]
    rest = np.delete(logits, [1, 4])
    assert R.routing_margin(rest, 1) >= R.MARGIN  # the third pick is no near-tie
    got, ge, gw = rt().moe_ffn(x, gate, w1, w2, w3, K, M.SILU, dtype)
    assert ge.tolist() == experts.tolist()
    assert gw[0] == gw[1]
    assert np.max(np.abs(gw - weights)) <= WEIGHT_TOL
    assert relerr(got, want) < FFN_TOL


# ---------------------------------------------------------------- 3. yalm_block
@pytest.mark.parametrize("case", R.BLOCK_CASES, ids=[c[0] for c in R.BLOCK_CASES])
def test_block_by_block(case):
    _, cfg, seed = case
    trace = R.block_case_trace(case)
    runtime = rt()
    dm = runtime.DeviceModel.from_arrays(cfg, O.synth_host_tensors_fast(cfg, seed=seed))
    dec = runtime.Decoder(dm)
    try:
        worst = 0.0
        for pos, l, x_in, x_out, experts, weights, logits in trace:
            dec.set_x(x_in)  # re-synced every layer so errors do not compound
            dec.block(l, pos, *M.kv_indices(cfg.max_seq_len, pos))
            ge, gw = dec.moe_routing()
            assert ge[l].tolist() == experts.tolist(), (pos, l)
            assert np.max(np.abs(gw[l] - weights)) <= weight_tol(logits, BLOCK_TOL), (pos, l)
            e = relerr(dec.get_x(), x_out)
            worst = max(worst, e)
            assert e < BLOCK_TOL, (pos, l, e)
        print(f"{case[0]}: worst per-block rel err {worst:.2e}")
    finally:
        dec.close()
        dm.close()


# ---------------------------------------------------------------- 4. full forward
@functools.lru_cache(maxsize=None)
def _forward_trace(i):
    return R.forward_case_trace(R.FORWARD_CASES[i])


@pytest.mark.parametrize("i", range(len(R.FORWARD_CASES)), ids=[c[0] for c in R.FORWARD_CASES])
def test_forward_logits_routing_greedy(i):
    """Positions 0 .. 40 with max_seq_len 32 (through the sliding-window wrap, sinks rotating):
    logits, the whole forward's routing, the device greedy loop; graph replay and eager
    launches give the same bits."""
    _, cfg, seed = R.FORWARD_CASES[i]
    steps, greedy, _ = _forward_trace(i)
    runtime = rt()
    dm = runtime.DeviceModel.from_arrays(cfg, O.synth_host_tensors_fast(cfg, seed=seed))
    dec = runtime.Decoder(dm)
    eager = runtime.Decoder(dm, launch=runtime.LAUNCH_EAGER)
    try:
        worst = 0.0
        for tok, pos, lo, experts, weights, rlogits in steps:
            lg = dec.forward(tok, pos)
            ge, gw = dec.moe_routing()
            assert np.array_equal(ge, experts), (pos, ge.tolist(), experts.tolist())
            for l in range(cfg.n_layers):
                assert np.max(np.abs(gw[l] - weights[l])) <= weight_tol(rlogits[l], LOGITS_TOL), (pos, l)
            e = relerr(lg, lo)
            worst = max(worst, e)
            assert e < LOGITS_TOL, (pos, e)
            np.testing.assert_array_equal(eager.forward(tok, pos), lg)
        print(f"{R.FORWARD_CASES[i][0]}: worst logits rel err {worst:.2e}")
        assert dec.generate_greedy(5, 0, R.GREEDY_STEPS) == greedy
        assert eager.generate_greedy(5, 0, R.GREEDY_STEPS) == greedy
    finally:
        eager.close()
        dec.close()
        dm.close()


# ---------------------------------------------------------------- 5. the committed fixtures
@pytest.mark.parametrize("fname", ["tiny_moe_fp16.yalm", "tiny_moe_fp8.yalm"])
def test_reference_converted_fixture(golden_dir, fname):
    runtime = rt()
    path = os.path.join(golden_dir, fname)
    cfg, t = R.yalm_tensors(path)
    dm = runtime.DeviceModel.from_yalm(path)
    assert dm.cfg == cfg and cfg.n_experts == 4
    dec = runtime.Decoder(dm)
    try:
        assert dec.generate_greedy(1, 0, R.FIXTURE_GREEDY) == R.MoeRef(cfg, t).greedy(1, 0, R.FIXTURE_GREEDY)
    finally:
        dec.close()
        dm.close()


# ---------------------------------------------------------------- 7. dense decoders, error codes
def test_dense_decoder_unaffected_and_error_codes():
    import ctypes

    runtime = rt()
    lib = runtime.lib
    # the dense TINY model's per-token graphs: step + 2 layers x (QKV, attention, Wo, W1|W3, W2) +
    # logits (+ argmax): the counts of the commit before mixture of experts
    cfg = M.TINY
    dm = runtime.DeviceModel.from_arrays(cfg, M.synth_host_tensors(cfg, seed=1))
    dec = runtime.Decoder(dm)
    try:
        assert (dec.graph_kernels(0), dec.graph_kernels(1), dec.graph_kernels(2)) == (11, 12, 13)
        n = cfg.n_layers * 2
        e, w = np.zeros(n, np.int32), np.zeros(n, np.float32)
        assert lib.yalm_moe_routing(dec.h, e.ctypes.data, w.ctypes.data) == 2  # YALM_ERR_ARG
        ms = ctypes.c_float()
        assert lib.yalm_time_kernel(dec.h, 9, 1, ctypes.byref(ms)) == 2
    finally:
        dec.close()
        dm.close()
    mcfg = M.TINY_MOE
    dm = runtime.DeviceModel.from_arrays(mcfg, M.synth_host_tensors(mcfg, seed=1))
    dec = runtime.Decoder(dm)
    try:
        # + the router and a second W2 launch per layer (hidden 128 is below one 64-lane chunk,
        # so W2 runs once per selected expert)
        assert dec.graph_kernels(2) == 13 + 2 * 2
        tok = np.array([1, 2, 3, 4], np.int32)
        assert lib.yalm_prefill(dec.h, tok.ctypes.data, 4, 0, None) == 3  # YALM_ERR_UNSUPPORTED
        assert dec.forward(1, 0).shape == (mcfg.vocab_size,)  # ... and the decoder still works
        for kid in (3, 4, 9):
            assert dec.time_kernel(kid, 2) > 0
        assert "moe_router" in dec.kernel_name(9) and "PMoeGlu" in dec.kernel_name(3)
        mw, _blocks = dm.weights_struct()
        c = runtime.Config.from_model(mcfg)
        gates = (ctypes.c_void_p * mcfg.n_layers)(*[dm.ptrs[M.moegate_name(l)] for l in range(mcfg.n_layers)])
        for E, K in ((4, 5), (65, 2), (4, 0)):
            h = ctypes.c_void_p()
            moe = (ctypes.c_int * 2)(E, K)
            assert lib.yalm_decoder_create_moe(ctypes.byref(c), moe, ctypes.byref(mw), gates, None,
                                               ctypes.byref(h)) == 2, (E, K)
    finally:
        dec.close()
        dm.close()
    sm = runtime.Decoder(runtime.DeviceModel.synthetic(M.SMALL_MOE.with_(max_seq_len=32), seed=1))
    try:  # one W2 launch for both experts: step + 4 x (QKV, attention, Wo, router, W1|W3, W2) + logits + argmax
        assert sm.graph_kernels(2) == 1 + 4 * 6 + 2
    finally:
        sm.close()
        sm.model.close()
