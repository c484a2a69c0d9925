"""GPU: the q / k norm (Qwen3, yalm_decoder_set_qk_norm) through decode, the multi-row verify
step and the speculative loop, against the float64 reference of qknorm_ref.py, and through the
batched prefill against the decode path.

The frozen CPU oracle has no such norm. tests/test_qknorm_cpu.py shows, for every decode case
here, how far the wrong models (no norm, g = 1, gq and gk exchanged, g reversed) lie from the
right one at every compared position, so a kernel that computed one of them fails these tests.
Bars: the decode bars of test_gpu_decode.py (logits 1e-3, one layer 1e-4, relative to the
largest magnitude), the prefill bars of test_gpu_prefill.py."""
import ctypes
import functools

import numpy as np
import pytest

import oracle_py as O
import qknorm_cases as C
import spec_ref as S
from test_gpu_arch import PF_CFG as A_PF_CFG
from test_gpu_arch import PF_LOGITS_BAR, PF_SPLIT_LOGITS_BAR
from test_gpu_prefill import LP_ATOL, _decode_logprobs
from yalm_amd import models as M

pytestmark = pytest.mark.gpu
LOGITS_BAR, BLOCK_BAR = C.LOGITS_BAR, C.BLOCK_BAR
relerr = C.relerr
WT = {M.F32: "WF32", M.F16: "WF16", M.F8E5M2: "WF8", M.Q4: "WQ4"}


def rt():
    from yalm_amd import runtime

    return runtime


def make(name):
    R = rt()
    cfg = C.CASES[name][0]
    return R, cfg, R.DeviceModel.from_arrays(cfg, C.tensors(name))


def plain_of(cfg, tensors):
    """The same weights as a model without the norm (no q_norm / k_norm tensors)."""
    return cfg.with_(qk_norm=False), {k: v for k, v in tensors.items() if "_norm.weight" not in k}


def download_f16(R, ptr, n):
    out = np.empty(n, np.float16)
    R.check(R.lib.yalm_download(out.ctypes.data, ptr, 2 * n))
    return out


# ------------------------------------------------------------------ 1. decode against qknorm_ref
@pytest.mark.parametrize("name", list(C.CASES))
def test_decode_against_qknorm_ref(name):
    """yalm_block layer by layer (from position 0), yalm_forward logits (from position 1: position
    0 says nothing about q or k) and the device greedy loop, positions 0 .. 21 of a 16-position
    window (ring wrap and sink rotation over normed K rows). By their row lengths TINY takes the
    generic GEMV and SMALL, the head_dim-128 model and the dim-2048 q4 model the row-block one
    (yalm_kernel_name names the policy, PQKVN, under one kernel prefix whichever runs: the numbers
    below are what holds both instantiations); on the head_dim-128
    model attention and Wo are the fused launch. The K row every layer wrote at position 0 (the
    hook run: each layer fed the reference's own x), read back from caller-owned caches, is the
    reference's f16 row to one f16 ulp."""
    R, cfg, dm = make(name)
    ref_blocks, ref_xin, ref_k0 = C.blocks_run(name)
    ref_logits = C.logits_run(name)
    ref_tokens, _ = C.greedy_run(name)
    nb = 2 * cfg.max_seq_len * cfg.kv_dim
    caches = [(R.lib.yalm_alloc(nb), R.lib.yalm_alloc(nb)) for _ in range(cfg.n_layers)]
    dec_b, dec_f, dec_g = R.Decoder(dm, kv_caches=caches), R.Decoder(dm), R.Decoder(dm)
    try:
        assert dec_f.kernel_name(0) == f"gemv_rb_kernel<{WT[cfg.weight_dtype]}, PQKVN<"
        if name in C.H128_CASES:
            assert dec_f.attn_wo and dec_g.attn_wo and dec_b.attn_wo
        worst_b = worst_l = worst_k = 0.0
        tok = C.TOKEN0
        for pos in range(C.N_POS):
            kv = M.kv_indices(cfg.max_seq_len, pos)
            for l in range(cfg.n_layers):
                dec_b.set_x(ref_xin[pos, l])
                dec_b.block(l, pos, *kv)
                e = relerr(dec_b.get_x().astype(np.float64), ref_blocks[pos, l])
                worst_b = max(worst_b, e)
                assert e < BLOCK_BAR, (pos, l, e)
                if pos == 0:  # the f16 rounding, which the f32 arithmetic may flip once
                    got = download_f16(R, caches[l][0], cfg.kv_dim).astype(np.float64)
                    want = ref_k0[l].astype(np.float64)
                    assert np.abs(want).max() > 0.1
                    d = np.abs(got - want)
                    bar = 2.0 ** -10 * np.abs(want) + 2.0 ** -24
                    worst_k = max(worst_k, float(np.max(d / bar)))
                    assert np.all(d <= bar), (l, int(np.argmax(d - bar)), float(np.max(d - bar)))
            lg = dec_f.forward(tok, pos).astype(np.float64)
            if pos >= C.FIRST:
                e = relerr(lg, ref_logits[pos])
                worst_l = max(worst_l, e)
                assert e < LOGITS_BAR, (pos, e)
            tok = C.step_token(tok, cfg.vocab_size)
        print(f"{name}: worst block {worst_b:.2e}, worst logits {worst_l:.2e}, worst K row / its bar {worst_k:.2f}")
        got = dec_g.generate_greedy(C.TOKEN0, 0, C.N_POS)
        assert got[:C.N_GREEDY] == ref_tokens[:C.N_GREEDY]
        assert got == ref_tokens
    finally:
        for h in (dec_b, dec_f, dec_g, dm):
            h.close()
        for kp, vp in caches:
            R.lib.yalm_free(kp)
            R.lib.yalm_free(vp)


# ------------------------------------------------------------------ 2. mechanics
def _walk(dec, cfg, n=6):
    tok, out = C.TOKEN0, []
    for pos in range(n):
        out.append(dec.forward(tok, pos))
        tok = C.step_token(tok, cfg.vocab_size)
    return out


@pytest.mark.parametrize("name", ["small-f16", "tiny-fp8", "h128-f16"])
def test_mechanics(name):
    R, cfg, dm = make(name)
    pc, pt = plain_of(cfg, C.tensors(name))
    dmp = R.DeviceModel.from_arrays(pc, pt)
    fresh, eager = R.Decoder(dm), R.Decoder(dm, launch=R.LAUNCH_EAGER)
    late, plain = R.Decoder(dm), R.Decoder(dmp)
    try:
        want = _walk(fresh, cfg)
        # graph replay, eager launches and a second run: the same kernels, the same bits
        for a, b in zip(_walk(eager, cfg), want):
            np.testing.assert_array_equal(a, b)
        for a, b in zip(_walk(fresh, cfg), want):
            np.testing.assert_array_equal(a, b)
        # kernel counts: one more launch per layer with the norm, in every graph
        with_norm = [late.graph_kernels(mode) for mode in range(4)]
        without = [plain.graph_kernels(mode) for mode in range(4)]
        assert [a - b for a, b in zip(with_norm, without)] == [cfg.n_layers] * 4
        if not plain.attn_wo:  # begin, per layer QKV / attention / Wo / W1|W3 / W2, logits, argmax
            assert without[2] == cfg.n_layers * 5 + 3
        # the norm removed: the plain decoder's bits, its kernel and its launch counts
        late.set_qk_norm(False)
        assert late.kernel_name(0).endswith("PQKV<") and plain.kernel_name(0).endswith("PQKV<")
        assert late.kernel_name(11) == ""
        assert [late.graph_kernels(mode) for mode in range(4)] == without
        pl = _walk(plain, pc)
        for a, b in zip(_walk(late, cfg), pl):
            np.testing.assert_array_equal(a, b)
        assert relerr(pl[3], want[3]) > 10 * LOGITS_BAR
        # ... and set after those forwards (their graphs dropped): a fresh normed decoder's bits
        late.set_qk_norm(True)
        assert late.kernel_name(0).endswith("PQKVN<")
        assert [late.graph_kernels(mode) for mode in range(4)] == with_norm
        for a, b in zip(_walk(late, cfg), want):
            np.testing.assert_array_equal(a, b)
        # id 11 names the launch and times it; without the norm it is an argument error
        assert late.kernel_name(11).startswith("qk_norm_rope_kernel<")
        ms = late.time_kernel(11, 20)
        assert 0.0 < ms < 1.0, ms
        ms = ctypes.c_float()
        assert R.lib.yalm_time_kernel(plain.h, 11, 4, ctypes.byref(ms)) == 2
        assert "norm" in R.lib.yalm_last_error().decode()
        # (the timing hook rewrote q and the last step's K rows, as timing the QKV launch does: a
        # walk from position 0 writes every row again before it reads it)
        for a, b in zip(_walk(late, cfg), want):
            np.testing.assert_array_equal(a, b)
    finally:
        for h in (fresh, eager, late, plain, dm, dmp):
            h.close()


# ------------------------------------------------------------------ 3. refusals
def test_refusals():
    R = rt()
    cfg = M.SMALL.with_(max_seq_len=32)
    L = cfg.n_layers
    dm = R.DeviceModel.synthetic(cfg, seed=1)
    dmm = R.DeviceModel.synthetic(M.TINY_MOE, seed=1)
    dummy = R.lib.yalm_alloc(4 * cfg.q_dim)
    ptrs = (ctypes.c_void_p * L)(*[dummy] * L)
    made = []

    def err():
        return R.lib.yalm_last_error().decode()

    try:
        # (a tensor-parallel decoder of one rank over the IPC transport: no communicator to set up)
        for dec in (R.Decoder(dm, tp_gather=lambda h: [h]), R.Decoder(dmm)):
            made.append(dec)
            assert R.lib.yalm_decoder_set_qk_norm(dec.h, ptrs, ptrs) == 3
            assert "q / k norm" in err()
        dec = R.Decoder(dm)
        made.append(dec)
        base = dec.forward(5, 0)
        # a biased decoder takes no norm; a normed decoder no bias
        assert R.lib.yalm_decoder_set_qkv_bias(dec.h, ptrs, ptrs, ptrs) == 0
        assert R.lib.yalm_decoder_set_qk_norm(dec.h, ptrs, ptrs) == 3
        assert "q / k norm" in err() and "bias" in err()
        assert R.lib.yalm_decoder_set_qkv_bias(dec.h, None, None, None) == 0
        assert R.lib.yalm_decoder_set_qk_norm(dec.h, ptrs, ptrs) == 0
        assert R.lib.yalm_decoder_set_qkv_bias(dec.h, ptrs, ptrs, ptrs) == 3
        assert "q / k norm" in err()
        assert R.lib.yalm_decoder_set_qkv_bias(dec.h, None, None, None) == 0  # removing a bias it has not: fine
        assert R.lib.yalm_decoder_set_qk_norm(dec.h, None, None) == 0
        # argument errors
        holes = (ctypes.c_void_p * L)(*([dummy] * (L - 1) + [None]))
        assert R.lib.yalm_decoder_set_qk_norm(dec.h, ptrs, holes) == 2  # a null layer pointer
        assert R.lib.yalm_decoder_set_qk_norm(dec.h, ptrs, None) == 2   # one of two arrays
        assert R.lib.yalm_decoder_set_qk_norm(dec.h, None, ptrs) == 2
        odd = (ctypes.c_void_p * L)(*([dummy] * (L - 1) + [dummy + 4]))
        assert R.lib.yalm_decoder_set_qk_norm(dec.h, odd, ptrs) == 2    # an entry that is not 8-byte aligned
        assert "aligned" in err()
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


# ------------------------------------------------------------------ 4. multi-row step and speculative loop
SPEC, SPEC_PROMPT, SPEC_GEN = C.SPEC, C.SPEC_PROMPT, C.SPEC_GEN


@pytest.mark.parametrize("name", sorted(SPEC))
def test_forward_rows_and_speculative_with_the_norm(name):
    R = rt()
    cfg, _ = SPEC[name]
    t, plog, seq, gap = C.spec_case(name)
    assert gap >= 2 * LOGITS_BAR, gap  # (tests/test_qknorm_cpu.py checks it without a GPU)
    dm = R.DeviceModel.from_arrays(cfg, t)
    try:
        for rows in (1, 2, 3, 4):  # the prompt in steps of `rows` rows (the last step: what is left)
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
            for stream in (list(plain), [(x + 1) % cfg.vocab_size if j % 3 == 2 else x for j, x in enumerate(plain)]):
                dec = hydrated()
                try:
                    got, st = dec.generate_speculative(SPEC_PROMPT[-1], pos, SPEC_GEN, rows=rows, context=SPEC_PROMPT,
                                                       draft_stream=stream)
                    assert got == plain, (rows, stream == plain)
                    _, want, _ = S.predict(seq, SPEC_PROMPT[-1], SPEC_GEN, rows, ngram_max=3, ngram_min=1,
                                           context=SPEC_PROMPT, stream=stream, pos=pos, max_seq_len=cfg.max_seq_len,
                                           vocab=cfg.vocab_size)
                    assert {k: st[k] for k in want} == want, (rows, st, want)
                    assert st["launches_per_step"] == 4 + cfg.n_layers * (5 + rows)
                finally:
                    dec.close()
    finally:
        dm.close()


def test_q4_rows_refusal_stays_with_the_norm():
    R, cfg, dm = make("tiny-q4")
    dec = R.Decoder(dm)
    try:
        with pytest.raises(R.YalmError, match="error 3.*q4"):
            dec.forward_rows([1, 2], 0)
    finally:
        dec.close()
        dm.close()


# ------------------------------------------------------------------ 5. prefill
# test_gpu_arch.py's PF_CFG (the prefill's shape rules: dims multiples of 128, head_dim 128) with the
# norm, without bias and scaling
PF_CFG = A_PF_CFG.with_(qkv_bias=False, rope_scaling=None, qk_norm=True)


@functools.lru_cache(maxsize=None)
def pf_tensors(dtype=M.F16):
    return M.synth_host_tensors(PF_CFG.with_(weight_dtype=dtype), seed=17)


@pytest.mark.parametrize("n", [13, 192])  # the skinny split-K path; the large tiles with one partial tile
@pytest.mark.parametrize("split", [False, True], ids=["fast", "split"])
def test_prefill_with_the_norm(n, split):
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
        # the model without the norm, through the same prefill: far from this one
        off = float(np.max(np.abs(dec_n.prefill(tokens)[: n - 1] - ld)))
        print(f"prefill T {n} {'split' if split else 'fast'}: max |d log p| {err:.3e} (norm dropped: {off:.3e})")
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
    carrying the same norm weights."""
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
        assert relerr(d.forward(7, n), d16.forward(7, n)) < LOGITS_BAR
    finally:
        for h in (d, d16, dm, dm16):
            h.close()
