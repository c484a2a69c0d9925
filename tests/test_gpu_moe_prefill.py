"""Batched MFMA prefill of mixture-of-experts models (moe_prefill.h): the grouped GEMM against
int64 numpy, the router + grouped expert FFN against the CPU reference (tests/moe_ref.py) row by
row, and the whole prefill against the MoE decode engine (pinned to the reference by
test_gpu_moe.py), position by position.

Bars: the dense prefill's (test_gpu_prefill.py: LP_ATOL per position, 5e-3 of max|logit| on the
next decode step); routing exact -- every input keeps a margin of 1e-2 between consecutive router
logits (test_moe_prefill_cpu.py), twice the logit bar -- with weights within
test_gpu_moe.weight_tol at the prefill bar.
"""
import functools

import numpy as np
import pytest

import moe_prefill_inputs as I
import moe_ref as R
from yalm_amd import models as M

pytestmark = pytest.mark.gpu

LP_ATOL = 0.02     # test_gpu_prefill.py
NEXT_TOL = 5e-3    # test_gpu_prefill.py test_prefill_matches_decode
FFN_TOL = 1e-4     # test_gpu_moe.py: the f32 sums
WEIGHT_TOL = 1e-5  # test_gpu_moe.py: both sides route the same x

G16_ALL = "qkv:{0},wo:{0},glu:{0},w2:{0},cls:{0},test:{0}"  # test_gpu_prefill.py FORMS
FORMS = {"auto": "", "g16-256": G16_ALL.format(256), "g16-256-2ph": G16_ALL.format(256) + ",8p:0",
         "g16-128": G16_ALL.format(128), "g16-192": G16_ALL.format(192),
         "g16-256-nopersist": G16_ALL.format(256) + ",persist:0"}


def rt():
    from yalm_amd import runtime

    return runtime


# ---------------------------------------------------------------- 1. grouped GEMM, exact
def _assign(M_, E, kind):
    rng = np.random.default_rng(M_ + E)
    if kind == "random":
        return rng.integers(0, E, size=M_).astype(np.int32)
    if kind == "sparse":  # most experts empty
        return rng.choice(np.array([3, 17, 40, 63]), size=M_).astype(np.int32)
    if kind == "one":
        return np.full(M_, E - 2, np.int32)
    if kind == "257-256-1":
        e = np.array([0] * 257 + [1] * 256 + [2], np.int32)
        return e[rng.permutation(M_)]
    raise ValueError(kind)


GEMM_CASES = [(1, 128, 64, 4, "random"), (70, 256, 192, 64, "sparse"), (300, 384, 128, 4, "one"),
              (514, 512, 320, 3, "257-256-1"), (700, 768, 448, 8, "random"), (1100, 5120, 192, 8, "random"),
              # 12 M tiles x 24 column tiles = 288 > 256 CUs: the persistent loop with its early exits
              (2300, 6144, 64, 6, "random")]


_WIDTH = {"auto": 128, "g16-128": 128, "g16-192": 192}  # every other form forces 256
GEMM_PARAMS = [(f,) + c for c in GEMM_CASES for f in FORMS if c[1] % _WIDTH.get(f, 256) == 0]


@pytest.mark.parametrize("form,M_,N,K,E,kind", GEMM_PARAMS)
def test_grouped_gemm_exact(form, M_, N, K, E, kind):
    """c[r] = a[r] . w[expert_of_row[r]]^T on f16-exact small integers (data as
    test_gpu_prefill.py test_gemm_forms_exact): the grouping pass, the tile table, the A-row
    gather, the expert's B rows and the scatter back are exact or a wrong integer shows."""
    rng = np.random.default_rng(M_ + N + K)
    a = rng.integers(-4, 5, size=(M_, K)).astype(np.float16)
    w = rng.integers(-4, 5, size=(E, N, K)).astype(np.float16)
    w[:, :, 0] += (np.arange(N, dtype=np.float16) % 7)[None, :]
    w[:, :, 1] += (np.arange(E, dtype=np.float16) % 5)[:, None]  # experts differ systematically too
    e = _assign(M_, E, kind)
    rt().set_gemm_forms(FORMS[form])
    try:
        c = rt().moe_gemm_f16(a, w, e)
    finally:
        rt().set_gemm_forms("")
    ref = np.zeros((M_, N), np.int64)
    for x in range(E):
        ref[e == x] = a[e == x].astype(np.int64) @ w[x].astype(np.int64).T
    np.testing.assert_array_equal(c, ref.astype(np.float32))


# ---------------------------------------------------------------- 2. router + grouped FFN rows
@pytest.mark.parametrize("case", I.FFN_ROW_CASES, ids=[c[0] for c in I.FFN_ROW_CASES])
def test_ffn_rows_match_reference(case):
    """yalm_moe_ffn_rows against moe_ref.moe_ffn per row. x is f16-exact, so the only rounding
    the reference lacks is H's: |got - ref| <= 1.1 * 2^-11 * sum_k w_k (|W2_e| . |h_e|) (each h
    element's f16 rounding carried through W2) + FFN_TOL * max|ref| (the f32 sums)."""
    _, T, dim, hidden, E, K, dtype, act, _ = case
    x, gate, w1, w2, w3 = I.ffn_rows_inputs(case)
    got, ge, gw = rt().moe_ffn_rows(x, gate, w1, w2, w3, K, act, dtype)
    f1, f2, f3 = (M.decode_weights(a, dtype).astype(np.float64) for a in (w1, w2, w3))
    worst_w = worst = 0.0
    for t in range(T):
        want, experts, weights, _ = R.moe_ffn(x[t], gate, w1, w2, w3, K, act, dtype)
        assert ge[t].tolist() == experts.tolist(), t
        worst_w = max(worst_w, float(np.max(np.abs(gw[t] - weights))))
        bound = np.zeros(dim)
        for e, wt in zip(experts, weights):
            a, b = f1[e] @ x[t].astype(np.float64), f3[e] @ x[t].astype(np.float64)
            if act == M.SILU:
                h = a / (1.0 + np.exp(-a)) * b
            else:
                h = 0.5 * a * (1.0 + np.tanh(0.797885 * (a + 0.044715 * a ** 3))) * b
            bound += float(wt) * (np.abs(f2[e]) @ np.abs(h))
        tol = 1.1 * 2.0 ** -11 * bound + FFN_TOL * np.max(np.abs(want))
        err = np.abs(got[t] - want)
        worst = max(worst, float(np.max(err / tol)))
        assert np.all(err <= tol), (t, float(np.max(err / tol)))
    print(f"{case[0]}: worst |err| / bound {worst:.3f}, worst weight err {worst_w:.1e}")
    assert worst_w <= WEIGHT_TOL


def test_ffn_rows_exact_tie_lowest_index_first():
    x, gate = I.tie_inputs()
    dim, E, hidden, K = x.shape[1], gate.shape[0], 256, 3
    rng = np.random.default_rng(22)

    def w(shape, s):
        return M.encode_weights(rng.standard_normal(shape, dtype=np.float32) * np.float32(s), M.F16)

    w1, w3, w2 = w((E, hidden, dim), dim ** -0.5), w((E, hidden, dim), dim ** -0.5), w((E, dim, hidden), hidden ** -0.5)
    _, experts, weights, _ = R.moe_ffn(x[0], gate, w1, w2, w3, K, M.SILU, M.F16)
    _, ge, gw = rt().moe_ffn_rows(x, gate, w1, w2, w3, K, M.SILU, M.F16)
    assert ge[0].tolist() == experts.tolist() and ge[0].tolist()[:2] == [1, 4]
    assert gw[0][0] == gw[0][1]
    assert np.max(np.abs(gw[0] - weights)) <= WEIGHT_TOL


# ---------------------------------------------------------------- 3. whole prefill vs decode
def _logprob(logits, target):
    lg = logits.astype(np.float64)
    m = lg.max()
    return lg[target] - m - np.log(np.exp(lg - m).sum())


@functools.lru_cache(maxsize=None)
def _decode_trace(name):
    """The decode engine over the config's whole safe sequence, once: per position the log p of
    the next token and the routing."""
    cfg, n = I.CONFIGS[name]
    tokens = I.sequence(name)[0]
    runtime = rt()
    dm = runtime.DeviceModel.from_arrays(cfg, I.tensors(name))
    dec = runtime.Decoder(dm)
    try:
        lps, experts, weights = [], [], []
        for pos in range(n):
            lg = dec.forward(int(tokens[pos]), pos)
            e, w = dec.moe_routing()
            experts.append(e.copy())
            weights.append(w.copy())
            lps.append(_logprob(lg, tokens[pos + 1]) if pos + 1 < n else 0.0)
        return np.array(lps), np.array(experts), np.array(weights)
    finally:
        dec.close()
        dm.close()


NEXT_TOKEN = 7


@functools.lru_cache(maxsize=None)
def _max_router_logit(name):
    """max |router logit| per (position, layer) on the CPU reference: the routing weights' bar is
    test_gpu_moe.py's weight_tol at the prefill bar, 0.5 * NEXT_TOL * max|logit|."""
    cfg, n = I.CONFIGS[name]
    ref = R.MoeRef(cfg, I.tensors(name))
    out = np.zeros((n, cfg.n_layers))
    for pos, tok in enumerate(I.sequence(name)[0]):
        ref.forward(int(tok), pos, 0)
        out[pos] = np.max(np.abs(ref.router_logits), axis=1)
    return out


def _check_prefill(name, n, forms="", split=False, pos0=0, passes=None, lp_atol=LP_ATOL):
    """Prefill positions pos0 .. n - 1 of the safe sequence (after a prefill of 0 .. pos0 - 1) and
    compare with the decode engine: routing, log p, the next decode step."""
    cfg, _ = I.CONFIGS[name]
    tokens = I.sequence(name)[0][:n]
    lp_d, ex_d, wt_d = _decode_trace(name)
    rmax = _max_router_logit(name)
    runtime = rt()
    dm = runtime.DeviceModel.from_arrays(cfg, I.tensors(name))
    dec, dd = runtime.Decoder(dm), runtime.Decoder(dm)
    try:
        dec.set_prefill_forms(forms)  # (resets the precision form too: set it after)
        if split:
            dec.set_prefill_precision(runtime.PREFILL_SPLIT)
        if pos0:
            dec.prefill(tokens[:pos0], logprobs=False)
        lp = dec.prefill(tokens[pos0:], pos0)
        if passes is not None:
            assert dec.prefill_info()[0] == passes, dec.prefill_info()
        ex, wt = dec.prefill_routing()
        assert ex.shape == (n - pos0, cfg.n_layers, cfg.n_experts_active)
        np.testing.assert_array_equal(ex, ex_d[pos0:n])
        werr = np.abs(wt - wt_d[pos0:n]).max(axis=2)
        wtol = 0.5 * NEXT_TOL * rmax[pos0:n]
        assert np.all(werr <= wtol), float(np.max(werr / wtol))
        assert lp[-1] == 0.0
        lerr = float(np.max(np.abs(lp[:-1] - lp_d[pos0:n - 1]))) if n - pos0 > 1 else 0.0
        assert lerr <= lp_atol, lerr
        # the next decode step on the prefilled cache against a decoder that decoded the prefix
        for pos in range(n):
            dd.forward(int(tokens[pos]), pos, runtime.HYDRATE_KV_CACHE)
        lg_p, lg_d = dec.forward(NEXT_TOKEN, n), dd.forward(NEXT_TOKEN, n)
        nerr = float(np.max(np.abs(lg_p - lg_d)) / np.max(np.abs(lg_d)))
        print(f"{name} n {n} forms '{forms}' split {split} pos0 {pos0}: max |d log p| {lerr:.2e} (bar {lp_atol}), "
              f"weights {float(np.max(werr / wtol)):.3f} of their bar, next step {nerr:.2e} (bar {NEXT_TOL})")
        assert nerr < NEXT_TOL, nerr
        return lp
    finally:
        dec.close()
        dd.close()
        dm.close()


@pytest.mark.parametrize("n", [1, 13, 61, 200])
@pytest.mark.parametrize("name", ["e4k2", "e8k2", "e8k3-gelu-4l", "small-moe"])
def test_prefill_matches_decode(name, n):
    _check_prefill(name, min(n, I.CONFIGS[name][1]))


@pytest.mark.parametrize("n", [13, 200])
@pytest.mark.parametrize("name", ["e4k2", "e8k3-gelu-4l", "small-moe"])
def test_prefill_split_form_matches_decode(name, n):
    _check_prefill(name, min(n, I.CONFIGS[name][1]), split=True)


@pytest.mark.parametrize("form", ["g16-256", "g16-256-2ph", "g16-128", "g16-256-nopersist", "glu:128,w2:192"])
def test_prefill_forced_forms_match_decode(form):
    _check_prefill("small-moe", 200, forms=FORMS.get(form, form))


def test_prefill_at_pos0_above_zero():
    _check_prefill("e8k2", 90, pos0=40)


# ---------------------------------------------------------------- 4. fp8 == f16 twin
def _f16_twin(cfg8, t8):
    t16 = {}
    for name, a in t8.items():
        t16[name] = a if a.dtype == np.float32 else (a.astype(np.uint16) << 8).view(np.float16)
    return cfg8.with_(weight_dtype=M.F16), t16


@pytest.mark.parametrize("n", [13, 90])
def test_fp8_prefill_equals_f16_twin(n):
    """An fp8 (E5M2) expert model through yalm_prefill (per-layer exact upcast of the stacked
    expert tensors and of the router's gate) is bit for bit the prefill of
    its f16 twin -- log p, routing and every K / V cache row -- and matches the fp8 decode engine."""
    cfg8, _ = I.CONFIGS["fp8"]
    t8 = I.tensors("fp8")
    cfg16, t16 = _f16_twin(cfg8, t8)
    tokens = I.sequence("fp8")[0][:n]
    runtime = rt()
    dm8, dm16 = runtime.DeviceModel.from_arrays(cfg8, t8), runtime.DeviceModel.from_arrays(cfg16, t16)
    kvb = cfg8.max_seq_len * cfg8.kv_dim * 2
    caches = [[runtime.lib.yalm_alloc(kvb) for _ in range(2 * cfg8.n_layers)] for _ in range(2)]
    d8 = runtime.Decoder(dm8, kv_caches=list(zip(caches[0][0::2], caches[0][1::2])))
    d16 = runtime.Decoder(dm16, kv_caches=list(zip(caches[1][0::2], caches[1][1::2])))
    try:
        lp8, lp16 = d8.prefill(tokens), d16.prefill(tokens)
        np.testing.assert_array_equal(lp8, lp16)
        (e8, w8), (e16, w16) = d8.prefill_routing(), d16.prefill_routing()
        np.testing.assert_array_equal(e8, e16)
        np.testing.assert_array_equal(w8, w16)
        for p8, p16 in zip(caches[0], caches[1]):
            a, b = np.empty(kvb, np.uint8), np.empty(kvb, np.uint8)
            runtime.check(runtime.lib.yalm_download(a.ctypes.data, p8, kvb))
            runtime.check(runtime.lib.yalm_download(b.ctypes.data, p16, kvb))
            np.testing.assert_array_equal(a, b)
    finally:
        for h in (d8, d16, dm8, dm16):
            h.close()
        for p in caches[0] + caches[1]:
            runtime.lib.yalm_free(p)
    _check_prefill("fp8", n)


# ---------------------------------------------------------------- 5. determinism
def test_prefill_is_deterministic():
    """Two prefills of the same 200 tokens (separate decoders): the same bits (no float atomics,
    a stable grouping order)."""
    cfg, n = I.CONFIGS["small-moe"]
    tokens = I.sequence("small-moe")[0]
    runtime = rt()
    dm = runtime.DeviceModel.from_arrays(cfg, I.tensors("small-moe"))
    a, b = runtime.Decoder(dm), runtime.Decoder(dm)
    try:
        lpa, lpb = a.prefill(tokens), b.prefill(tokens)
        lpa2 = a.prefill(tokens)
        np.testing.assert_array_equal(lpa, lpb)
        np.testing.assert_array_equal(lpa, lpa2)
        (ea, wa), (eb, wb) = a.prefill_routing(), b.prefill_routing()
        np.testing.assert_array_equal(ea, eb)
        np.testing.assert_array_equal(wa, wb)
        np.testing.assert_array_equal(a.forward(NEXT_TOKEN, n), b.forward(NEXT_TOKEN, n))
    finally:
        a.close()
        b.close()
        dm.close()


# ---------------------------------------------------------------- 6. range guard
@pytest.mark.parametrize("n", [17, 70])
def test_prefill_range_guard(n):
    """GLU products past 65504 in one layer of every expert (moe_prefill_inputs "spike"): the
    pass runs twice (RG_H, the scaled H, W2's epilogue undoing the scale) and meets check 3's bars."""
    lp = _check_prefill("spike", n, passes=2)
    assert np.all(np.isfinite(lp))


# ---------------------------------------------------------------- 7. error codes, dense decoders
def test_error_codes_and_dense_unchanged():
    import ctypes

    runtime = rt()
    lib = runtime.lib
    cfg = M.TINY
    dm = runtime.DeviceModel.from_arrays(cfg, M.synth_host_tensors(cfg, seed=1))
    dec = runtime.Decoder(dm)
    try:
        assert (dec.graph_kernels(0), dec.graph_kernels(1), dec.graph_kernels(2)) == (11, 12, 13)
        e, w = np.zeros(64, np.int32), np.zeros(64, np.float32)
        assert lib.yalm_prefill_routing(dec.h, e.ctypes.data, w.ctypes.data) == 2  # YALM_ERR_ARG: dense
    finally:
        dec.close()
        dm.close()
    mcfg = M.TINY_MOE
    dm = runtime.DeviceModel.from_arrays(mcfg, M.synth_host_tensors(mcfg, seed=1))
    dec = runtime.Decoder(dm)
    try:
        tok = np.array([1, 2, 3, 4], np.int32)
        assert lib.yalm_prefill(dec.h, tok.ctypes.data, 4, 0, None) == 3  # dim 64: the shape check, as before
        e, w = np.zeros(64, np.int32), np.zeros(64, np.float32)
        assert lib.yalm_prefill_routing(dec.h, e.ctypes.data, w.ctypes.data) == 2  # no prefill has run
        ms = ctypes.c_float()
        assert lib.yalm_prefill_time(dec.h, 4, 1, ctypes.byref(ms)) == 3
    finally:
        dec.close()
        dm.close()
    # a dense prefill: two forms that were bit-equal before (the persistent tile loop or one
    # workgroup per tile: the same tiles, the same MFMA sequence) still are
    dcfg = M.ModelConfig(dim=512, hidden_dim=1024, head_dim=128, n_layers=2, n_heads=4, n_kv_heads=2,
                         vocab_size=1024, max_seq_len=320, rope_theta=1e6, act=M.SILU, weight_dtype=M.F16)
    dm = runtime.DeviceModel.synthetic(dcfg, seed=4)
    a, b = runtime.Decoder(dm), runtime.Decoder(dm)
    try:
        b.set_prefill_forms("persist:0")
        tokens = np.random.default_rng(5).integers(0, dcfg.vocab_size, size=200).astype(np.int32)
        np.testing.assert_array_equal(a.prefill(tokens), b.prefill(tokens))
    finally:
        a.close()
        b.close()
        dm.close()


def test_prefill_time_runs_on_expert_decoder():
    cfg, _ = I.CONFIGS["e4k2"]
    runtime = rt()
    dm = runtime.DeviceModel.from_arrays(cfg, I.tensors("e4k2"))
    dec = runtime.Decoder(dm)
    try:
        assert dec.prefill_time(100, 1) > 0
    finally:
        dec.close()
        dm.close()
