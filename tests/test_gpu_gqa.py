"""GPU: whole models at the GQA groups of the published Qwen2.5 / Qwen3 shapes (G = 7 with the
q / k / v bias, G = 5 with the q / k norm) and at head_dim 256 (G = 8), run far enough to leave
head mode: decode, the device greedy loop, the multi-row verify step and the speculative loop
with rows on both sides of the head / key switch, and the batched prefill, against the float64
reference of gqa_cases.py (arch_ref.ArchRef / qknorm_ref.QKNormRef).

None of these shapes can take the fused attention + Wo launch (it needs head_dim 128 and a
power-of-two n_heads): every layer runs the standalone attn_decode_kernel<D, 8>, with one masked
head at G = 7 and three at G = 5. tests/test_gqa_cpu.py shows that dropping the bias or the norm
moves the logits by at least 10 bars at every compared position and that the greedy paths have
no near-tie. Bars: the decode bar of test_gpu_decode.py (logits 1e-3 of max|logit|), the
multi-row bar of test_gpu_spec.py, the prefill bars of test_gpu_prefill.py."""
import numpy as np
import pytest

import gqa_cases as C
from test_gpu_arch import PF_LOGITS_BAR
from test_gpu_prefill import LP_ATOL, _decode_logprobs

pytestmark = pytest.mark.gpu
LOGITS_BAR = C.LOGITS_BAR
ROWS_BAR = 1e-3  # test_gpu_spec.py: a row's logits against the sequential forwards
relerr = C.relerr


def rt():
    from yalm_amd import runtime

    return runtime


def make(name):
    R = rt()
    cfg = C.CASES[name][0]
    return R, cfg, R.DeviceModel.from_arrays(cfg, C.tensors(name))


def hydrated(R, dm, n):
    """A decoder whose cache holds positions 0 .. n - 1 of the walk (single-row forwards)."""
    dec = R.Decoder(dm)
    for pos, tok in enumerate(C.walk_tokens()[:n]):
        dec.forward(tok, pos, R.HYDRATE_KV_CACHE)
    return dec


# ------------------------------------------------------------------ 1. the walk and the greedy loop
@pytest.mark.parametrize("name", list(C.CASES))
def test_walk_and_greedy_against_reference(name):
    """yalm_forward over positions 0 .. 329 of a 320-position window: logits at every position
    from FIRST on; then the device greedy loop from position 240 across the head / key switch."""
    R, cfg, dm = make(name)
    ref_logits = C.logits_run(name)
    ref_tokens, _ = C.greedy_run(name)
    toks = C.walk_tokens()
    dec_f, dec_g = R.Decoder(dm), R.Decoder(dm)
    try:
        assert not dec_f.attn_wo  # the standalone attention kernel
        worst = (0.0, -1)
        for pos in range(C.N_POS):
            lg = dec_f.forward(toks[pos], pos).astype(np.float64)
            assert np.all(np.isfinite(lg)), pos
            if pos < C.GREEDY_POS:
                dec_g.forward(toks[pos], pos, R.HYDRATE_KV_CACHE)
            if pos >= C.FIRST[name]:
                e = relerr(lg, ref_logits[pos])
                worst = max(worst, (e, pos))
                assert e < LOGITS_BAR, (pos, e)
        print(f"{name}: worst logits error {worst[0]:.2e} at position {worst[1]}")
        got = dec_g.generate_greedy(toks[C.GREEDY_POS], C.GREEDY_POS, C.SPEC_GEN)
        assert got[:C.GREEDY_N] == ref_tokens[:C.GREEDY_N]
        assert got == ref_tokens
        if cfg.head_dim == 256:  # decode only: the prefill says so
            with pytest.raises(R.YalmError, match="error 3.*head_dim"):
                dec_g.prefill(np.array(toks[:16], np.int32))
    finally:
        for h in (dec_f, dec_g, dm):
            h.close()


# ------------------------------------------------------------------ 2. the multi-row step in key mode
@pytest.mark.parametrize("name", C.ROWS_CASES)
def test_rows_across_the_head_key_switch(name):
    """forward_rows of 4 rows at positions 254, 255 (rows on both sides of the switch: the T
    attention launches of a layer share one partial buffer, told apart by their epochs) and 300
    (all four in key mode), on a cache hydrated by single-row forwards: every row against the
    reference and against the decoder's own single-row forward, and the same step again on the
    same decoder bit for bit (a stale partial of the first step would show)."""
    R, cfg, dm = make(name)
    ref_logits = C.logits_run(name)
    toks = C.walk_tokens()
    last = max(C.ROWS_POS) + C.SPEC_ROWS
    single, rows = R.Decoder(dm), R.Decoder(dm)
    try:
        own = {}
        for pos in range(last):
            if pos < min(C.ROWS_POS):
                single.forward(toks[pos], pos, R.HYDRATE_KV_CACHE)
            else:
                own[pos] = single.forward(toks[pos], pos)
        for pos in range(last):
            if pos in C.ROWS_POS:
                lg = rows.forward_rows(toks[pos:pos + C.SPEC_ROWS], pos)
                assert lg.shape == (C.SPEC_ROWS, cfg.vocab_size)
                for r in range(C.SPEC_ROWS):
                    e_ref = relerr(lg[r].astype(np.float64), ref_logits[pos + r])
                    e_own = relerr(lg[r], own[pos + r])
                    print(f"{name} pos {pos} row {r}: vs reference {e_ref:.2e}, vs single-row {e_own:.2e}")
                    assert e_ref < LOGITS_BAR, (pos, r, e_ref)
                    assert e_own < ROWS_BAR, (pos, r, e_own)
                again = rows.forward_rows(toks[pos:pos + C.SPEC_ROWS], pos)
                np.testing.assert_array_equal(again.view(np.uint32), lg.view(np.uint32))
            rows.forward(toks[pos], pos, R.HYDRATE_KV_CACHE)
    finally:
        for h in (single, rows, dm):
            h.close()


@pytest.mark.parametrize("name", C.ROWS_CASES)
def test_speculative_across_the_head_key_switch(name):
    """70 tokens from position 240 in steps of 4 rows, with an all-correct and an all-wrong
    draft stream: plain greedy's tokens either way (which are the reference's)."""
    R, cfg, dm = make(name)
    ref_tokens, _ = C.greedy_run(name)
    toks = C.walk_tokens()
    pos, n = C.GREEDY_POS, C.SPEC_GEN
    try:
        twin = hydrated(R, dm, pos)
        plain = twin.generate_greedy(toks[pos], pos, n)
        twin.close()
        assert plain == ref_tokens
        for kind, stream in (("true", list(plain)), ("wrong", [(t + 1) % cfg.vocab_size for t in plain])):
            dec = hydrated(R, dm, pos)
            try:
                got, st = dec.generate_speculative(toks[pos], pos, n, rows=C.SPEC_ROWS, context=list(toks[:pos + 1]),
                                                   draft_stream=stream)
                print(f"{name} {kind}: {st}")
                assert got == plain, kind
                assert st["spec_steps"] + st["accepted_drafts"] + st["plain_steps"] == n, (kind, st)
                if kind == "true":
                    assert st["spec_steps"] == -(-n // C.SPEC_ROWS) and st["plain_steps"] == 0
                else:
                    assert st["spec_steps"] == n and st["accepted_drafts"] == 0
            finally:
                dec.close()
    finally:
        dm.close()


# ------------------------------------------------------------------ 3. prefill
@pytest.mark.parametrize("name", C.PREFILL_CASES)
def test_prefill_matches_decode(name):
    """300 positions in one prefill pass (causal attention at G = 7 / G = 5 over five key tiles)
    against the decode engine position by position, and the decode step on the rows it wrote."""
    R, cfg, dm = make(name)
    n = C.PF_N
    tokens = np.random.default_rng(70 + cfg.head_dim).integers(0, cfg.vocab_size, size=n).astype(np.int32)
    dec_p, dec_d = R.Decoder(dm), R.Decoder(dm)
    try:
        lp = dec_p.prefill(tokens)
        ld = _decode_logprobs(dec_d, tokens)
        err = float(np.max(np.abs(lp[: n - 1] - ld)))
        print(f"{name}: prefill T {n}: max |d log p| {err:.3e}")
        assert err <= LP_ATOL, err
        dec_d.forward(int(tokens[-1]), n - 1)
        e = relerr(dec_p.forward(7, n), dec_d.forward(7, n))
        assert e < PF_LOGITS_BAR, e
    finally:
        for h in (dec_p, dec_d, dm):
            h.close()
