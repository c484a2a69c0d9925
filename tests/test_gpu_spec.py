"""GPU: the multi-row forward (yalm_forward_rows, csrc/gemv_rows.h) and speculative greedy
decode (yalm_generate_speculative, csrc/spec.h).

Bars: every row's logits within the project's 1e-3 (max|gpu - oracle| / max|oracle|) of the CPU
oracle's sequential forwards; speculative tokens EXACTLY those of the plain greedy loop on a twin
decoder, on seeds whose oracle greedy path keeps a top-2 gap of 2 x 1e-3 x max|logit| at every
step (asserted here on the oracle; two paths that each meet 1e-3 cannot order such a pair
differently); the step counts exactly those tests/spec_ref.py predicts from the tokens.
"""
import functools

import numpy as np
import pytest

import oracle_py as O
import spec_ref as S
from test_spec_cpu import DRAFT_CASES, long_history
from yalm_amd import models as M

pytestmark = pytest.mark.gpu

GAP = 2e-3  # 2 x the 1e-3 logits bar, relative to max|logit|


def rt():
    from yalm_amd import runtime

    return runtime


def relerr(a, b):
    return float(np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-30))


# ------------------------------------------------------------------ 1. rows parity
PARITY = {
    "small-f16": (M.SMALL, 11),
    "small-fp8": (M.SMALL.with_(weight_dtype=M.F8E5M2), 11),
    "small-f32": (M.SMALL.with_(weight_dtype=M.F32), 11),
    "tiny-f16": (M.TINY, 1),  # dim 64: a row shorter than one 64-lane chunk
}
PROMPT = [1, 17, 300, 5, 42, 9, 250, 33, 2, 77]


@functools.lru_cache(maxsize=None)
def parity_reference(name):
    """Oracle logits of PROMPT position by position (computed once, never changed)."""
    cfg, seed = PARITY[name]
    host = O.synth_host_tensors_fast(cfg, seed=seed)
    om = O.OracleModel(cfg, host)
    ref = [om.forward(t, p) for p, t in enumerate(PROMPT)]
    for r in ref:
        r.setflags(write=False)
    return host, ref


@pytest.mark.parametrize("name", sorted(PARITY))
def test_rows_match_oracle_and_fill_the_cache(name):
    R = rt()
    cfg, seed = PARITY[name]
    host, ref = parity_reference(name)
    dm = R.DeviceModel.from_arrays(cfg, host)
    try:
        for pos in (0, 5):
            for T in (1, 2, 3, 4):
                dec = R.Decoder(dm)
                try:
                    for p in range(pos):  # hydration by the single-row path
                        dec.forward(PROMPT[p], p, R.HYDRATE_KV_CACHE)
                    lg = dec.forward_rows(PROMPT[pos:pos + T], pos)
                    assert lg.shape == (T, cfg.vocab_size)
                    for t in range(T):
                        e = relerr(lg[t], ref[pos + t])
                        print(f"{name} pos {pos} T {T} row {t}: rel err {e:.2e}")
                        assert e < 1e-3, (pos, T, t, e)
                    # the KV rows the call wrote serve a plain forward at pos + T
                    e = relerr(dec.forward(PROMPT[pos + T], pos + T), ref[pos + T])
                    print(f"{name} pos {pos} T {T} next forward: rel err {e:.2e}")
                    assert e < 1e-3, (pos, T, "next", e)
                finally:
                    dec.close()
    finally:
        dm.close()


def test_rows_window_bound():
    R = rt()
    cfg = M.TINY
    dm = R.DeviceModel.synthetic(cfg, seed=1)
    dec = R.Decoder(dm)
    try:
        dec.forward_rows([1, 2, 3], cfg.max_seq_len - 3)  # pos + T == max_seq_len: accepted
        with pytest.raises(R.YalmError, match="error 2.*max_seq_len"):
            dec.forward_rows([1, 2, 3], cfg.max_seq_len - 2)
        with pytest.raises(R.YalmError, match="error 2"):
            dec.forward_rows([1, 2, 3, 4, 5], 0)
        with pytest.raises(R.YalmError, match="error 2"):
            dec.forward_rows([cfg.vocab_size], 0)
    finally:
        dec.close()
        dm.close()


# ------------------------------------------------------------------ 2. the LDS capacity shape
@pytest.mark.parametrize("dtype", [M.F16, M.F8E5M2], ids=["f16", "fp8"])
def test_rows_at_mistral_dims(dtype):
    """MISTRAL_7B dims, 2 layers, T = 4: W2's four f32 rows (4 x 14336 x 4 B = 229 KB) exceed
    the LDS, so x is staged by K segments; the smallest shape that takes that path."""
    R = rt()
    cfg = M.MISTRAL_7B.with_(n_layers=2, weight_dtype=dtype)
    host = O.synth_host_tensors_fast(cfg, seed=3)
    om = O.OracleModel(cfg, host)
    dm = R.DeviceModel.synthetic(cfg, seed=3)
    dec = R.Decoder(dm)
    try:
        toks = [1, 415, 3195, 28713, 264]
        lg = dec.forward_rows(toks[:4], 0)
        for t in range(4):
            e = relerr(lg[t], om.forward(toks[t], t))
            print(f"mistral dims {dtype} row {t}: rel err {e:.2e}")
            assert e < 1e-3, (t, e)
        e = relerr(dec.forward(toks[4], 4), om.forward(toks[4], 4))
        assert e < 1e-3, ("next", e)
    finally:
        dec.close()
        dm.close()


# ------------------------------------------------------------------ 3. tokens equal plain greedy
# (config, tensor seed, prompt seed): seeds searched on the CPU oracle for a greedy path without
# a near-tie (asserted in greedy_case)
GREEDY = {
    "small-f16": (M.SMALL, 5, 105),
    "small-fp8": (M.SMALL.with_(weight_dtype=M.F8E5M2), 1, 101),
}
N_PROMPT, N_GEN = 13, 64


@functools.lru_cache(maxsize=None)
def greedy_case(name, n_prompt=N_PROMPT, n_gen=N_GEN):
    """(host tensors, prompt, the oracle's greedy continuation of n_gen + 4 tokens); asserts the
    path has no near-tie."""
    cfg, seed, pseed = GREEDY_ALL[name]
    host = O.synth_host_tensors_fast(cfg, seed=seed)
    om = O.OracleModel(cfg, host)
    prompt = [int(t) for t in np.random.default_rng(pseed).integers(1, cfg.vocab_size, n_prompt)]
    for p, t in enumerate(prompt[:-1]):
        om.forward(t, p, 0)
    tok, pos, seq, worst = prompt[-1], n_prompt - 1, [], np.inf
    for i in range(n_gen + 4):
        lg = om.forward(tok, pos + i)
        s = np.sort(lg)
        worst = min(worst, float((s[-1] - s[-2]) / np.max(np.abs(lg))))
        tok = int(O.olib.orc_sample_argmax(O.P(lg), cfg.vocab_size))
        seq.append(tok)
    assert worst >= GAP, f"{name}: the oracle's greedy path has a near-tie (top-2 gap {worst:.2e} of max|logit|)"
    return host, prompt, seq


GREEDY_ALL = dict(GREEDY, **{"tiny-window": (M.TINY, 4, 104)})


def hydrated(R, dm, prompt):
    dec = R.Decoder(dm)
    for p, t in enumerate(prompt[:-1]):
        dec.forward(t, p, R.HYDRATE_KV_CACHE)
    return dec


def streams(seq, n, vocab):
    true = seq[:n]
    return {
        "ngram": None,
        "true": true,
        "wrong": [(t + 1) % vocab for t in true],
        "third": [(t + 1) % vocab if j % 3 == 2 else t for j, t in enumerate(true)],
    }


@pytest.mark.parametrize("name", sorted(GREEDY))
def test_speculative_equals_plain_greedy(name):
    R = rt()
    cfg = GREEDY[name][0]
    host, prompt, seq = greedy_case(name)
    pos = len(prompt) - 1
    dm = R.DeviceModel.from_arrays(cfg, host)
    try:
        twin = hydrated(R, dm, prompt)
        plain = twin.generate_greedy(prompt[-1], pos, N_GEN)
        plain_next = twin.generate_greedy(plain[-1], pos + N_GEN, 4)
        twin.close()
        assert plain == seq[:N_GEN]  # the device greedy loop is the oracle's (no near-tie on this seed)
        for rows in (2, 3, 4):
            for kind, stream in streams(seq, N_GEN, cfg.vocab_size).items():
                dec = hydrated(R, dm, prompt)
                try:
                    got, st = dec.generate_speculative(prompt[-1], pos, N_GEN, rows=rows, ngram_max=3, ngram_min=1,
                                                       context=prompt, draft_stream=stream)
                    assert got == plain, (rows, kind)
                    _, want, _ = S.predict(seq, prompt[-1], N_GEN, rows, ngram_max=3, ngram_min=1, context=prompt,
                                           stream=stream, pos=pos, max_seq_len=cfg.max_seq_len, vocab=cfg.vocab_size)
                    print(f"{name} rows {rows} {kind}: {st}")
                    assert {k: st[k] for k in want} == want, (rows, kind, st, want)
                    assert st["launches_per_step"] == 4 + cfg.n_layers * (4 + rows)
                    if kind == "true":
                        assert st["spec_steps"] == -(-N_GEN // rows)
                    if kind == "wrong":
                        assert st["spec_steps"] == N_GEN and st["accepted_drafts"] == 0
                    assert dec.device_step() == (plain[-1], pos + N_GEN)
                    assert dec.device_tokens() == plain
                    assert dec.generate_greedy(plain[-1], pos + N_GEN, 4) == plain_next
                finally:
                    dec.close()
    finally:
        dm.close()


# ------------------------------------------------------------------ 4. the drafter rule
@pytest.mark.parametrize("name", sorted(DRAFT_CASES))
def test_drafter_kernel_on_crafted_histories(name):
    h, rows, gmax, gmin, want = DRAFT_CASES[name]
    assert S.draft(h, rows, gmax, gmin) == want
    assert rt().spec_draft(h, rows, gmax, gmin) == want


def test_drafter_kernel_long_history():
    h = long_history()
    want = S.draft(h.tolist(), 4, 2, 2)
    assert want[:2] == [777, 778]
    assert rt().spec_draft(h, 4, 2, 2) == want
    for g in (1, 2, 3, 4):  # and the other lengths agree with the reference on the same history
        assert rt().spec_draft(h[-4096:], 4, g, 1) == S.draft(h[-4096:].tolist(), 4, g, 1)


# ------------------------------------------------------------------ 5. the window's end
def test_window_end_finishes_with_plain_steps():
    R = rt()
    cfg = M.TINY  # window 64
    n_prompt, n = 41, 40
    host, prompt, seq = greedy_case("tiny-window", n_prompt, n)
    pos = n_prompt - 1
    dm = R.DeviceModel.from_arrays(cfg, host)
    try:
        twin = hydrated(R, dm, prompt)
        plain = twin.generate_greedy(prompt[-1], pos, n)
        twin.close()
        assert plain == seq[:n]
        for rows, stream in ((4, None), (4, seq[:n]), (2, None)):
            dec = hydrated(R, dm, prompt)
            try:
                got, st = dec.generate_speculative(prompt[-1], pos, n, rows=rows, context=prompt, draft_stream=stream)
                assert got == plain
                _, want, _ = S.predict(seq, prompt[-1], n, rows, ngram_max=3, ngram_min=1, context=prompt,
                                       stream=stream, pos=pos, max_seq_len=cfg.max_seq_len, vocab=cfg.vocab_size)
                assert {k: st[k] for k in want} == want, (st, want)
                assert st["plain_steps"] > 0 and st["spec_steps"] > 0
                assert dec.device_step() == (plain[-1], pos + n)
            finally:
                dec.close()
        # a call that starts past the window is plain throughout
        dec = hydrated(R, dm, prompt)
        try:
            dec.generate_greedy(prompt[-1], pos, n)
            a, st = dec.generate_speculative(plain[-1], pos + n, 6, rows=4, context=prompt + plain)
            assert st["spec_steps"] == 0 and st["plain_steps"] == 6
            twin = hydrated(R, dm, prompt)
            twin.generate_greedy(prompt[-1], pos, n)
            assert a == twin.generate_greedy(plain[-1], pos + n, 6)
            twin.close()
        finally:
            dec.close()
    finally:
        dm.close()


# ------------------------------------------------------------------ 6. refusals
def _refused(R, dec, what):
    with pytest.raises(R.YalmError, match=f"error 3.*{what}"):
        dec.forward_rows([1, 2], 0)
    with pytest.raises(R.YalmError, match=f"error 3.*{what}"):
        dec.generate_speculative(1, 0, 4, rows=2)


def test_refusals():
    R = rt()
    # q4
    c4 = M.SMALL.with_(weight_dtype=M.Q4, n_layers=1)
    dm = R.DeviceModel.synthetic(c4, seed=1)
    dec = R.Decoder(dm)
    try:
        _refused(R, dec, "q4")
        dec.forward(1, 0)  # the q4 decoder itself still works
    finally:
        dec.close()
        dm.close()
    # mixture of experts
    dm = R.DeviceModel.synthetic(M.TINY_MOE, seed=1)
    dec = R.Decoder(dm)
    try:
        _refused(R, dec, "mixture-of-experts")
    finally:
        dec.close()
        dm.close()
    # tensor parallel (one rank over the IPC transport)
    dm = R.DeviceModel.synthetic(M.SMALL, seed=1)
    dec = R.Decoder(dm, tp_gather=lambda h: [h])
    try:
        _refused(R, dec, "tensor-parallel")
    finally:
        dec.close()
    # argument errors on a decoder that supports the call
    dec = R.Decoder(dm)
    try:
        for kw in (dict(rows=1), dict(rows=5), dict(ngram_min=3, ngram_max=2), dict(ngram_min=0), dict(ngram_max=5)):
            with pytest.raises(R.YalmError, match="error 2"):
                dec.generate_speculative(1, 0, 4, **kw)
        with pytest.raises(R.YalmError, match="error 2.*token buffer"):
            dec.generate_speculative(1, 0, 65537, rows=2)
        with pytest.raises(R.YalmError, match="error 2.*context"):
            dec.generate_speculative(1, 0, 4, rows=2, context=[1, 2])
        assert R.lib.yalm_spec_draft(None, 0, 4, 3, 1, None) == 2
        # and the decoder still decodes
        assert len(dec.generate_speculative(1, 0, 4, rows=2)[0]) == 4
    finally:
        dec.close()
        dm.close()
