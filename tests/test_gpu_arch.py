"""GPU: the Qwen2 q / k / v bias (yalm_decoder_set_qkv_bias) and the Llama-3 "llama3" RoPE
scaling (yalm_decoder_set_rope_scaling) through decode, the multi-row verify step, the
speculative loop and the batched prefill, against the float64 reference of arch_ref.py.

The frozen CPU oracle has neither form. tests/test_arch_cpu.py shows, for every decode case
here, that the reference without the form is at least 10 bars from the reference with it at
every compared position: a decoder that dropped the bias or the scaling fails these tests.
Bars: the decode bars of test_gpu_decode.py (logits 1e-3, one layer 1e-4, relative to the
largest magnitude), the prefill bars of test_gpu_prefill.py."""
import ctypes
import functools

import numpy as np
import pytest

import arch_cases as A
import arch_ref
import oracle_py as O
import spec_ref as S
from test_gpu_prefill import LP_ATOL, _decode_logprobs
from yalm_amd import models as M

pytestmark = pytest.mark.gpu
LOGITS_BAR, BLOCK_BAR = A.LOGITS_BAR, A.BLOCK_BAR
PF_LOGITS_BAR = 5e-3  # test_gpu_prefill.py: the decode step after a fast-form prefill (f16 MFMA activations in the cache rows)
PF_SPLIT_LOGITS_BAR = 1e-3  # ... after a split-form prefill (test_prefill_split_precision_form)


def rt():
    from yalm_amd import runtime

    return runtime


relerr = A.relerr


def make(name):
    R = rt()
    cfg = A.CASES[name][0]
    dm = R.DeviceModel.from_arrays(cfg, A.tensors(name))
    return R, cfg, dm


def plain_of(cfg, tensors):
    """The same weights as a model without the forms (no bias tensors, no scaling)."""
    pc = cfg.with_(qkv_bias=False, rope_scaling=None)
    return pc, {k: v for k, v in tensors.items() if not k.endswith(".bias")}


# ------------------------------------------------------------------ 1. decode against arch_ref
@pytest.mark.parametrize("name", list(A.CASES))
def test_decode_against_arch_ref(name):
    """yalm_block layer by layer, yalm_forward logits and the device greedy loop, positions
    0 .. 21 of a 16-position window (ring wrap and sink rotation over biased / rescaled K rows).
    TINY and the dim-64 q4 model run the generic GEMV, SMALL and the dim-2048 q4 model the
    row-block one."""
    R, cfg, dm = make(name)
    first = A.CASES[name][2]
    ref_blocks, ref_xin = A.blocks_run(name, with_inputs=True)
    ref_logits = A.logits_run(name)
    ref_tokens, _ = A.greedy_run(name)
    dec_b, dec_f, dec_g = R.Decoder(dm), R.Decoder(dm), R.Decoder(dm)
    try:
        wt = {M.F32: "WF32", M.F16: "WF16", M.F8E5M2: "WF8", M.Q4: "WQ4"}[cfg.weight_dtype]
        assert dec_f.kernel_name(0) == f"gemv_rb_kernel<{wt}, " + ("PQKVB<" if cfg.qkv_bias else "PQKV<")
        worst_b = worst_l = 0.0
        tok = A.TOKEN0
        for pos in range(A.N_POS):
            kv = M.kv_indices(cfg.max_seq_len, pos)
            for l in range(cfg.n_layers):
                dec_b.set_x(ref_xin[pos, l])
                dec_b.block(l, pos, *kv)
                e = relerr(dec_b.get_x().astype(np.float64), ref_blocks[pos, l])
                worst_b = max(worst_b, e)
                assert e < BLOCK_BAR, (pos, l, e)
            lg = dec_f.forward(tok, pos).astype(np.float64)
            if pos >= first:
                e = relerr(lg, ref_logits[pos])
                worst_l = max(worst_l, e)
                assert e < LOGITS_BAR, (pos, e)
            tok = A.step_token(tok, cfg.vocab_size)
        print(f"{name}: worst block {worst_b:.2e}, worst logits {worst_l:.2e}")
        got = dec_g.generate_greedy(A.TOKEN0, 0, A.N_POS)
        assert got[:A.N_GREEDY] == ref_tokens[:A.N_GREEDY]
        assert got == ref_tokens
    finally:
        for h in (dec_b, dec_f, dec_g, dm):
            h.close()


# ------------------------------------------------------------------ 2. mechanics
def _walk(dec, cfg, n=6, start=0):
    tok, out = A.TOKEN0, []
    for pos in range(start, start + n):
        out.append(dec.forward(tok, pos))
        tok = A.step_token(tok, cfg.vocab_size)
    return out


@pytest.mark.parametrize("name", ["bias-small-f16", "bias-tiny-fp8"])
def test_bias_mechanics(name):
    R, cfg, dm = make(name)
    pc, pt = plain_of(cfg, A.tensors(name))
    dmp = R.DeviceModel.from_arrays(pc, pt)
    fresh, eager = R.Decoder(dm), R.Decoder(dm, launch=R.LAUNCH_EAGER)
    late, plain = R.Decoder(dm), R.Decoder(dmp)
    try:
        want = _walk(fresh, cfg)
        # graph replay and eager launches: the same kernels, the same bits
        for a, b in zip(_walk(eager, cfg), want):
            np.testing.assert_array_equal(a, b)
        # the bias removed: the plain decoder's bits, its kernel and its launch counts
        late.set_qkv_bias(False)
        assert late.kernel_name(0).endswith("PQKV<") and plain.kernel_name(0).endswith("PQKV<")
        pl = _walk(plain, pc)
        for a, b in zip(_walk(late, cfg), pl):
            np.testing.assert_array_equal(a, b)
        assert relerr(pl[0], want[0]) > 10 * LOGITS_BAR
        # ... and set after those forwards (their graphs dropped): a fresh biased decoder's bits
        late.set_qkv_bias(True)
        assert late.kernel_name(0).endswith("PQKVB<")
        for a, b in zip(_walk(late, cfg), want):
            np.testing.assert_array_equal(a, b)
        # an unbiased decoder launches what it launched before (and a biased one as many kernels)
        separate = cfg.n_layers * 5 + 3  # begin, per layer QKV / attention / Wo / W1|W3 / W2, logits, argmax
        assert not plain.attn_wo
        for mode in range(4):
            assert plain.graph_kernels(mode) == fresh.graph_kernels(mode)
        assert plain.graph_kernels(2) == separate
    finally:
        for h in (fresh, eager, late, plain, dm, dmp):
            h.close()


# ------------------------------------------------------------------ 2b. the timing hook's GLU
# arch_cases.glu_case: one dense GELU / SILU layer; tests/test_arch_cpu.py shows that the two are far apart
GLU_BAR, glu_case = A.GLU_BAR, A.glu_case


@pytest.mark.parametrize("act", [M.GELU, M.SILU], ids=["gelu", "silu"])
def test_time_kernel_glu_runs_the_models_activation(act):
    """yalm_time_kernel launches what the forward launches: the GLU of a GELU model is GELU."""
    R = rt()
    cfg, t, x0, want = glu_case(act)
    other = glu_case(M.SILU if act == M.GELU else M.GELU)[3]
    dm = R.DeviceModel.from_arrays(cfg, t)
    dec = R.Decoder(dm, launch=R.LAUNCH_SEPARATE_ATTN_WO)
    try:
        assert not dec.attn_wo and dec.kernel_name(3) == "gemv_rb_kernel<WF16, PGlu<"
        dec.set_x(x0)
        dec.time_kernel(3, 1)
        dec.time_kernel(4, 1)
        got = dec.get_x().astype(np.float64)
        e, off = relerr(got, want), relerr(got, other)
        print(f"act {act}: rel err {e:.3e}, against the other activation {off:.3e}")
        assert e < GLU_BAR, e
        assert off > GLU_BAR, off
    finally:
        dec.close()
        dm.close()


# ------------------------------------------------------------------ 3. scaled RoPE
def ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.mark.parametrize("name", A.SCALED_CASES)
def test_rope_table_and_restore(name):
    R, cfg, dm = make(name)
    pc, pt = plain_of(cfg, A.tensors(name))
    dmp = R.DeviceModel.from_arrays(pc, pt)
    dec, plain = R.Decoder(dm), R.Decoder(dmp)
    try:
        assert ulps(dec.inv_freq(), M.rope_inv_freq(cfg)).max() <= 2
        assert ulps(plain.inv_freq(), M.rope_inv_freq(pc)).max() <= 2  # (numpy's f32 power stands in for glibc's powf)
        scaled = _walk(dec, cfg, n=8)
        pl = _walk(plain, pc, n=8)
        np.testing.assert_array_equal(scaled[0], pl[0])  # position 0: every angle 0
        assert relerr(scaled[7], pl[7]) > 10 * LOGITS_BAR
        dec.set_rope_scaling(None)  # type 0: the plain table and the plain decoder's bits
        np.testing.assert_array_equal(dec.inv_freq(), plain.inv_freq())
        for a, b in zip(_walk(dec, cfg, n=8), pl):
            np.testing.assert_array_equal(a, b)
        # Llama-3.1 / 3.2 parameters through the same setter: the rule on the decoder's own plain
        # table (glibc's powf; numpy's f32 power may sit an ulp away, and in the blended regime the
        # rule multiplies a relative difference of the input by up to ~10)
        for rs in (("llama3", 8.0, 1.0, 4.0, 8192), ("llama3", 32.0, 1.0, 4.0, 8192)):
            dec.set_rope_scaling(rs)
            assert ulps(dec.inv_freq(), M.llama3_scale(plain.inv_freq(), rs)).max() <= 2
    finally:
        for h in (dec, plain, dm, dmp):
            h.close()


def test_rope_scaling_on_a_moe_decoder():
    """The expert decoder takes the call: its table is the rule's, its logits move, and type 0
    restores its bits. (moe_ref.py runs the frozen C oracle, which has no table argument, so the
    scaled expert model has no CPU reference here; its attention half is the dense decoder's,
    which the cases above pin.)"""
    R = rt()
    cfg = M.TINY_MOE.with_(max_seq_len=A.MSL)
    dm = R.DeviceModel.synthetic(cfg, seed=7)
    dec = R.Decoder(dm)
    try:
        base = _walk(dec, cfg, n=10)
        dec.set_rope_scaling(A.SCALING)
        assert ulps(dec.inv_freq(), M.rope_inv_freq(cfg.with_(rope_scaling=A.SCALING))).max() <= 2
        moved = _walk(dec, cfg, n=10)
        np.testing.assert_array_equal(moved[0], base[0])
        assert relerr(moved[9], base[9]) > LOGITS_BAR
        dec.set_rope_scaling(None)
        for a, b in zip(_walk(dec, cfg, n=10), base):
            np.testing.assert_array_equal(a, b)
    finally:
        dec.close()
        dm.close()


# ------------------------------------------------------------------ 4. multi-row step and speculative loop
SPEC, SPEC_PROMPT, SPEC_GEN, spec_case = A.SPEC, A.SPEC_PROMPT, A.SPEC_GEN, A.spec_case


@pytest.mark.parametrize("name", sorted(SPEC))
def test_forward_rows_and_speculative_with_bias(name):
    R = rt()
    cfg, _ = SPEC[name]
    t, plog, seq, gap = spec_case(name)
    assert gap >= 2 * LOGITS_BAR, gap  # (tests/test_arch_cpu.py checks it without a GPU)
    dm = R.DeviceModel.from_arrays(cfg, t)
    try:
        for rows in (2, 4):  # the prompt in steps of `rows` rows (the last step: what is left)
            dec = R.Decoder(dm)
            try:
                for p0 in range(0, len(SPEC_PROMPT), rows):
                    lg = dec.forward_rows(SPEC_PROMPT[p0:p0 + rows], p0)
                    for k in range(lg.shape[0]):
                        e = relerr(lg[k].astype(np.float64), plog[p0 + k])
                        assert e < LOGITS_BAR, (rows, p0 + k, e)
            finally:
                dec.close()
        pos = len(SPEC_PROMPT) - 1

        def hydrated():
            d = R.Decoder(dm)
            for p, tk in enumerate(SPEC_PROMPT[:-1]):
                d.forward(tk, p, R.HYDRATE_KV_CACHE)
            return d

        twin = hydrated()
        plain = twin.generate_greedy(SPEC_PROMPT[-1], pos, SPEC_GEN)
        twin.close()
        assert plain == seq[:SPEC_GEN]
        for rows in (2, 4):
            for stream in (None, [(x + 1) % cfg.vocab_size if j % 3 == 2 else x for j, x in enumerate(plain)]):
                dec = hydrated()
                try:
                    got, st = dec.generate_speculative(SPEC_PROMPT[-1], pos, SPEC_GEN, rows=rows, context=SPEC_PROMPT,
                                                       draft_stream=stream)
                    assert got == plain, (rows, stream is None)
                    _, want, _ = S.predict(seq, SPEC_PROMPT[-1], SPEC_GEN, rows, ngram_max=3, ngram_min=1,
                                           context=SPEC_PROMPT, stream=stream, pos=pos, max_seq_len=cfg.max_seq_len,
                                           vocab=cfg.vocab_size)
                    assert {k: st[k] for k in want} == want, (rows, st, want)
                finally:
                    dec.close()
    finally:
        dm.close()


def test_q4_rows_refusal_stays_with_a_bias():
    R, cfg, dm = make("bias-q4-64")
    dec = R.Decoder(dm)
    try:
        with pytest.raises(R.YalmError, match="error 3.*q4"):
            dec.forward_rows([1, 2], 0)
    finally:
        dec.close()
        dm.close()


# ------------------------------------------------------------------ 5. prefill
# test_gpu_q4.py's PF_CFG (the prefill's shape rules: dims multiples of 128, head_dim 128) with
# both forms on; the llama3 parameters put head_dim 128's pairs at theta 1e6 into all three regimes
PF_SCALING = ("llama3", 8.0, 1.0, 4.0, 64)
PF_CFG = M.ModelConfig(dim=512, hidden_dim=1024, head_dim=128, n_layers=3, n_heads=4, n_kv_heads=2, vocab_size=1024,
                       max_seq_len=320, rope_theta=1e6, act=M.SILU, weight_dtype=M.F16, qkv_bias=True,
                       rope_scaling=PF_SCALING)


def test_pf_scaling_reaches_every_regime():
    reg = arch_ref.regimes(M.rope_inv_freq(PF_CFG.with_(rope_scaling=None)), PF_SCALING)
    assert set(reg.tolist()) == {0, 1, 2}


@functools.lru_cache(maxsize=None)
def pf_tensors(dtype=M.F16):
    return M.synth_host_tensors(PF_CFG.with_(weight_dtype=dtype), seed=17)


@pytest.mark.parametrize("n", [13, 192])  # the skinny split-K path; the large tiles with one partial tile
@pytest.mark.parametrize("split", [False, True], ids=["fast", "split"])
def test_prefill_with_bias_and_scaling(n, split):
    R = rt()
    dm = R.DeviceModel.from_arrays(PF_CFG, pf_tensors())
    pc, pt = plain_of(PF_CFG, pf_tensors())
    dmp = R.DeviceModel.from_arrays(pc, pt)
    dec_p, dec_c, dec_d, dec_n = R.Decoder(dm), R.Decoder(dm), R.Decoder(dm), R.Decoder(dmp)
    if split:
        dec_p.set_prefill_precision(R.PREFILL_SPLIT)
        dec_c.set_prefill_precision(R.PREFILL_SPLIT)
        dec_n.set_prefill_precision(R.PREFILL_SPLIT)
    try:
        tokens = np.random.default_rng(50 + n).integers(0, PF_CFG.vocab_size, size=n).astype(np.int32)
        lp = dec_p.prefill(tokens)
        ld = _decode_logprobs(dec_d, tokens)
        err = float(np.max(np.abs(lp[: n - 1] - ld)))
        # the model without the forms, through the same prefill: far from this one
        off = float(np.max(np.abs(dec_n.prefill(tokens)[: n - 1] - ld)))
        print(f"prefill T {n} {'split' if split else 'fast'}: max |d log p| {err:.3e} (forms dropped: {off:.3e})")
        assert err <= (LP_ATOL / 10 if split else LP_ATOL), err
        assert off >= 10 * LP_ATOL, off
        # the cache rows it wrote drive the next decode step
        dec_d.forward(int(tokens[-1]), n - 1)
        lg_p, lg_d = dec_p.forward(7, n), dec_d.forward(7, n)
        assert relerr(lg_p, lg_d) < (PF_SPLIT_LOGITS_BAR if split else PF_LOGITS_BAR)
        # continuation at pos0 > 0: the first 5 positions, then the rest, against the one-pass run
        # (a pass has no target for its last row: position 4's log p is not produced)
        lp_a = dec_c.prefill(tokens[:5], pos0=0)
        lp_b = dec_c.prefill(tokens[5:], pos0=5)
        cont = np.concatenate([lp_a[:4], lp_b[: n - 6]])
        assert float(np.max(np.abs(cont - np.concatenate([ld[:4], ld[5:]])))) <= (LP_ATOL / 10 if split else LP_ATOL)
        assert relerr(dec_c.forward(7, n), lg_d) < (PF_SPLIT_LOGITS_BAR if split else PF_LOGITS_BAR)
    finally:
        for h in (dec_p, dec_c, dec_d, dec_n, dm, dmp):
            h.close()


@pytest.mark.parametrize("dtype", [M.F8E5M2, M.Q4], ids=["fp8", "q4"])
@pytest.mark.parametrize("n", [13, 192])
def test_prefill_fp8_q4_equal_their_f16_twins(dtype, n):
    """fp8 and q4 go through the per-layer exact f16 upcast: log p bit for bit the f16 twin's
    carrying the same bias and table."""
    R = rt()
    cfg = PF_CFG.with_(weight_dtype=dtype)
    t = pf_tensors(dtype)
    if dtype == M.Q4:
        c16, t16 = M.q4_twin(cfg, t)
    else:
        c16 = cfg.with_(weight_dtype=M.F16)
        t16 = {k: (M.e5m2_to_f32(v).astype(np.float16) if v.dtype == np.uint8 else v) for k, v in t.items()}
    dm, dm16 = R.DeviceModel.from_arrays(cfg, t), R.DeviceModel.from_arrays(c16, t16)
    d, d16 = R.Decoder(dm), R.Decoder(dm16)
    try:
        tokens = np.random.default_rng(60 + n).integers(0, cfg.vocab_size, size=n).astype(np.int32)
        np.testing.assert_array_equal(d.prefill(tokens), d16.prefill(tokens))
        # the decode step on those (bit-equal) cache rows: exact weights on both sides, f32 sums in another order
        assert relerr(d.forward(7, n), d16.forward(7, n)) < LOGITS_BAR
    finally:
        for h in (d, d16, dm, dm16):
            h.close()


# ------------------------------------------------------------------ 6. refusals
def test_refusals():
    R = rt()
    cfg = M.SMALL.with_(max_seq_len=32)
    L = cfg.n_layers
    dm = R.DeviceModel.synthetic(cfg, seed=1)
    dmm = R.DeviceModel.synthetic(M.TINY_MOE, seed=1)
    dummy = R.lib.yalm_alloc(4 * cfg.q_dim)
    ptrs = (ctypes.c_void_p * L)(*[dummy] * L)
    made = []
    try:
        # (a tensor-parallel decoder of one rank over the IPC transport: no communicator to set up)
        for dec in (R.Decoder(dm, tp_gather=lambda h: [h]), R.Decoder(dmm)):
            made.append(dec)
            assert R.lib.yalm_decoder_set_qkv_bias(dec.h, ptrs, ptrs, ptrs) == 3
            assert "bias" in R.lib.yalm_last_error().decode()
        dec = R.Decoder(dm)
        made.append(dec)
        base = dec.forward(5, 0)
        holes = (ctypes.c_void_p * L)(*([dummy] * (L - 1) + [None]))
        assert R.lib.yalm_decoder_set_qkv_bias(dec.h, ptrs, holes, ptrs) == 2  # a null layer pointer
        assert R.lib.yalm_decoder_set_qkv_bias(dec.h, ptrs, None, ptrs) == 2   # two of three arrays
        for bad in (R.RopeScaling(1, 0.5, 1.0, 4.0, 32), R.RopeScaling(1, 8.0, 4.0, 4.0, 32),
                    R.RopeScaling(1, 8.0, 1.0, 4.0, 0), R.RopeScaling(2, 8.0, 1.0, 4.0, 32)):
            assert R.lib.yalm_decoder_set_rope_scaling(dec.h, ctypes.byref(bad)) == 2
        assert R.lib.yalm_decoder_set_rope_scaling(dec.h, None) == 2
        assert R.lib.yalm_decoder_get_inv_freq(dec.h, None) == 2
        np.testing.assert_array_equal(dec.forward(5, 0), base)  # the refused calls changed nothing
        # a plain f16 decoder made afterwards still matches the oracle
        d2 = R.Decoder(dm)
        made.append(d2)
        om = O.OracleModel(cfg, O.synth_host_tensors_fast(cfg, seed=1))
        assert relerr(d2.forward(5, 0), om.forward(5, 0)) < LOGITS_BAR
    finally:
        for h in made:
            h.close()
        R.lib.yalm_free(dummy)
        dm.close()
        dmm.close()
