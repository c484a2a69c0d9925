"""GPU: speculative decode with a draft model (yalm_generate_speculative_model, csrc/spec.h).

Bars. The delivered tokens never depend on the draft, so against the n-gram calls at the same rows
(the same multi-row kernels on the same inputs) every comparison is EXACT, whatever the draft: its
format, its vocabulary, a cache that was never hydrated. Against the plain greedy loop the tokens
are compared as test_gpu_spec.py compares them: on seeds whose plain path keeps its top-1 to top-2
gap above 1e-3 of the logit range at every delivered position (asserted here on the plain decoder's
own logits; the seeds were chosen on the CPU oracle). With a draft that is a second decoder over the
target's own weights that same gap makes every draft the target's choice, so the acceptance counts
are exact too: ceil(n / rows) steps. A missing KV-only forward, a sync one position off or a gather
shifted by one all lose acceptances there (tests/test_spec_model_cpu.py shows each on the numpy model).
"""
import functools

import numpy as np
import pytest

from yalm_amd import models as M

pytestmark = pytest.mark.gpu

TGT = M.SMALL  # dim 512, 4 layers, vocabulary 2048, window 256
DRAFT = M.TINY.with_(vocab_size=2048, max_seq_len=256)
N_PROMPT, N = 13, 96
GAP = 1e-3  # of the logit range
TEMP, TOP_K, TOP_P = 0.8, 40, 0.9
DT = {"f32": M.F32, "f16": M.F16, "fp8": M.F8E5M2, "e4m3": M.E4M3, "q4": M.Q4}
# target format -> (tensor seed, prompt seed): plain greedy paths without a near-tie over N + 4 tokens
# (f16 / f32 / fp8 searched on the CPU oracle; e4m3, which has no oracle twin of the synthetic model, on the device)
SEEDS = {"f16": (8, 108), "f32": (8, 108), "fp8": (1, 101), "e4m3": (10, 110)}
OWN = (8, 108)  # the f16 PEAKED target of the acceptance cases


def rt():
    from yalm_amd import runtime

    return runtime


def prompt_of(pseed, n=N_PROMPT, vocab=TGT.vocab_size):
    return [int(t) for t in np.random.default_rng(pseed).integers(1, vocab, n)]


def hydrated(R, dm, prompt, stream=None, hydrate=True):
    dec = R.Decoder(dm, stream=stream)
    if hydrate:
        for p, t in enumerate(prompt[:-1]):
            dec.forward(min(t, dm.cfg.vocab_size - 1), p, R.HYDRATE_KV_CACHE)
    return dec


class Pair:
    """A hydrated target and a draft decoder on the target's stream."""

    def __init__(self, R, tdm, ddm, prompt, hydrate_draft=True):
        self.tgt = hydrated(R, tdm, prompt)
        self.draft = hydrated(R, ddm, prompt, stream=self.tgt.get_stream(), hydrate=hydrate_draft)

    def __enter__(self):
        return self.tgt, self.draft

    def __exit__(self, *exc):
        self.draft.close()
        self.tgt.close()


def plain_path(R, dm, prompt, n):
    """(tokens, worst top-1 to top-2 gap / logit range) of n plain forwards, from their logits."""
    dec = hydrated(R, dm, prompt)
    try:
        tok, pos, out, worst = prompt[-1], len(prompt) - 1, [], np.inf
        for i in range(n):
            lg = dec.forward(tok, pos + i)
            top = np.partition(lg, -2)[-2:]
            worst = min(worst, float((top[1] - top[0]) / (lg.max() - lg.min())))
            tok = int(np.argmax(lg))
            out.append(tok)
        return out, worst
    finally:
        dec.close()


def identity(st, n):
    return st["spec_steps"] + st["accepted_drafts"] + st["plain_steps"] == n


def formula(R, tgt, draft, rows, sampled=False):
    """launches_per_step as include/yalm_hip.h states it."""
    own = (5 if sampled else 4) + tgt.cfg.n_layers * ((5 if tgt.cfg.qk_norm else 4) + rows)
    return own + 1 + (rows - 1) * draft.graph_kernels(2) + draft.graph_kernels(R.HYDRATE_KV_CACHE)


# ------------------------------------------------------------------ 1. the tokens do not depend on the draft
PAIRS = [("f16", "f16"), ("fp8", "fp8"), ("e4m3", "q4"), ("f32", "f16"), ("f16", "q4"), ("fp8", "f16")]


@pytest.mark.parametrize("tdt,ddt", PAIRS)
def test_greedy_tokens_are_the_ngram_calls_and_plain_greedy(tdt, ddt):
    R = rt()
    seed, pseed = SEEDS[tdt]
    prompt, pos = prompt_of(pseed), N_PROMPT - 1
    tdm = R.DeviceModel.synthetic(TGT.with_(weight_dtype=DT[tdt]), seed=seed)
    ddm = R.DeviceModel.synthetic(DRAFT.with_(weight_dtype=DT[ddt]), seed=3)
    try:
        plain, worst = plain_path(R, tdm, prompt, N + 4)
        print(f"target {tdt}: worst top-2 gap {worst:.2e} of the logit range")
        assert worst > GAP, f"precondition: the plain path of this seed has a near-tie ({worst:.2e} of the range)"
        twin = hydrated(R, tdm, prompt)
        assert twin.generate_greedy(prompt[-1], pos, N) == plain[:N]
        twin.close()
        for rows in (2, 3, 4):
            twin = hydrated(R, tdm, prompt)
            ngram, _ = twin.generate_speculative(prompt[-1], pos, N, rows=rows, context=prompt)
            twin.close()
            with Pair(R, tdm, ddm, prompt) as (tgt, draft):
                got, st = tgt.generate_speculative_model(draft, prompt[-1], pos, N, rows=rows)
                print(f"target {tdt} draft {ddt} rows {rows}: {st}")
                assert got == ngram, (rows, "n-gram call")
                assert got == plain[:N], (rows, "plain greedy")
                assert identity(st, N) and st["plain_steps"] == 0
                assert st["launches_per_step"] == formula(R, tgt, draft, rows)
                assert tgt.device_step() == (plain[N - 1], pos + N)
                assert tgt.device_tokens() == plain[:N]
                assert tgt.generate_greedy(plain[N - 1], pos + N, 4) == plain[N:]
    finally:
        ddm.close()
        tdm.close()


@pytest.mark.parametrize("tdt,ddt", [("f16", "fp8"), ("fp8", "q4"), ("e4m3", "f16"), ("f32", "f16")])
def test_sampled_tokens_are_the_ngram_sampled_call(tdt, ddt):
    R = rt()
    seed, pseed = SEEDS[tdt]
    prompt, pos = prompt_of(pseed), N_PROMPT - 1
    u = np.random.default_rng(7).random(N, dtype=np.float32)
    tdm = R.DeviceModel.synthetic(TGT.with_(weight_dtype=DT[tdt]), seed=seed)
    ddm = R.DeviceModel.synthetic(DRAFT.with_(weight_dtype=DT[ddt]), seed=3)
    try:
        for rows in (2, 3, 4):
            twin = hydrated(R, tdm, prompt)
            want, _ = twin.generate_speculative_sampled(prompt[-1], pos, N, TEMP, TOP_K, TOP_P, uniforms=u, rows=rows,
                                                        context=prompt)
            twin.close()
            assert len(set(want)) > 4
            with Pair(R, tdm, ddm, prompt) as (tgt, draft):
                got, st = tgt.generate_speculative_model(draft, prompt[-1], pos, N, rows=rows, temperature=TEMP,
                                                         top_k=TOP_K, top_p=TOP_P, uniforms=u)
                assert got == want, rows
                assert identity(st, N)
                assert st["launches_per_step"] == formula(R, tgt, draft, rows, sampled=True)
                assert tgt.device_step() == (want[-1], pos + N)
    finally:
        ddm.close()
        tdm.close()


def test_qk_norm_target_bias_draft_and_an_unhydrated_draft():
    R = rt()
    prompt, pos = prompt_of(108), N_PROMPT - 1
    u = np.random.default_rng(9).random(N, dtype=np.float32)
    tdm = R.DeviceModel.synthetic(TGT.with_(qk_norm=True), seed=8)
    ddm = R.DeviceModel.synthetic(DRAFT.with_(qkv_bias=True), seed=3)
    try:
        for rows in (2, 4):
            twin = hydrated(R, tdm, prompt)
            ngram, _ = twin.generate_speculative(prompt[-1], pos, N, rows=rows, context=prompt)
            twin.close()
            twin = hydrated(R, tdm, prompt)
            smp, _ = twin.generate_speculative_sampled(prompt[-1], pos, N, TEMP, TOP_K, TOP_P, uniforms=u, rows=rows)
            twin.close()
            for hyd in (True, False):  # a draft whose prompt was never hydrated: the tokens are still exact
                with Pair(R, tdm, ddm, prompt, hydrate_draft=hyd) as (tgt, draft):
                    got, st = tgt.generate_speculative_model(draft, prompt[-1], pos, N, rows=rows)
                    assert got == ngram and identity(st, N), (rows, hyd)
                    assert st["launches_per_step"] == formula(R, tgt, draft, rows)
                with Pair(R, tdm, ddm, prompt, hydrate_draft=hyd) as (tgt, draft):
                    got, st = tgt.generate_speculative_model(draft, prompt[-1], pos, N, rows=rows, temperature=TEMP,
                                                             top_k=TOP_K, top_p=TOP_P, uniforms=u)
                    assert got == smp and identity(st, N), (rows, hyd)
    finally:
        ddm.close()
        tdm.close()


# ------------------------------------------------------------------ 2. acceptance, exact
@functools.lru_cache(maxsize=None)
def own_case():
    """(prompt, the plain path of N + 4 tokens) of the PEAKED f16 target; asserts the gap."""
    R = rt()
    prompt = prompt_of(OWN[1])
    dm = R.DeviceModel.synthetic(TGT, seed=OWN[0], peak=M.PEAKED)
    try:
        plain, worst = plain_path(R, dm, prompt, N + 4)
    finally:
        dm.close()
    print(f"own-weights case: worst top-2 gap {worst:.2e} of the logit range")
    assert worst > GAP, f"precondition: the plain path of this seed has a near-tie ({worst:.2e} of the range)"
    assert len(set(plain)) > 4, "precondition: the path is not one repeated token"
    return prompt, plain


@pytest.mark.parametrize("rows", [2, 3, 4])
def test_own_weights_draft_is_accepted_at_every_row(rows):
    R = rt()
    prompt, plain = own_case()
    pos = N_PROMPT - 1
    dm = R.DeviceModel.synthetic(TGT, seed=OWN[0], peak=M.PEAKED)
    try:
        with Pair(R, dm, dm, prompt) as (tgt, draft):
            got, st = tgt.generate_speculative_model(draft, prompt[-1], pos, N, rows=rows)
            print(f"own weights rows {rows}: {st}")
            assert got == plain[:N]
            steps = -(-N // rows)
            assert st["spec_steps"] == steps and st["accepted_drafts"] == N - steps and st["plain_steps"] == 0
    finally:
        dm.close()


# ------------------------------------------------------------------ 3. a random draft
def test_random_draft_costs_acceptance_only():
    R = rt()
    prompt, plain = own_case()
    pos = N_PROMPT - 1
    tdm = R.DeviceModel.synthetic(TGT, seed=OWN[0], peak=M.PEAKED)
    ddm = R.DeviceModel.synthetic(DRAFT, seed=21)
    try:
        with Pair(R, tdm, ddm, prompt) as (tgt, draft):
            got, st = tgt.generate_speculative_model(draft, prompt[-1], pos, N, rows=4)
            print(f"random draft: {st}")
            assert got == plain[:N] and identity(st, N)
            # an unrelated model names the target's next token among 2048 by chance alone
            assert st["accepted_drafts"] <= N // 8
    finally:
        ddm.close()
        tdm.close()


# ------------------------------------------------------------------ 4. the draft_stream hook
def test_draft_stream_hook_and_launch_formula():
    R = rt()
    prompt, plain = own_case()
    pos = N_PROMPT - 1
    wrong = [(t + 1) % TGT.vocab_size for t in plain]
    tdm = R.DeviceModel.synthetic(TGT, seed=OWN[0], peak=M.PEAKED)
    ddm = R.DeviceModel.synthetic(DRAFT, seed=21)
    try:
        for rows in (2, 3, 4):
            with Pair(R, tdm, ddm, prompt) as (tgt, draft):
                got, st = tgt.generate_speculative_model(draft, prompt[-1], pos, N, rows=rows, draft_stream=plain)
                steps = -(-N // rows)
                assert got == plain[:N] and st["spec_steps"] == steps and st["accepted_drafts"] == N - steps
                G, H = draft.graph_kernels(2), draft.graph_kernels(R.HYDRATE_KV_CACHE)
                assert st["launches_per_step"] == 4 + TGT.n_layers * (4 + rows) + 1 + (rows - 1) * G + H
            with Pair(R, tdm, tdm, prompt) as (tgt, draft):  # the perfect draft model, overruled by the stream
                got, st = tgt.generate_speculative_model(draft, prompt[-1], pos, N, rows=rows, draft_stream=wrong)
                assert got == plain[:N] and st["spec_steps"] == N and st["accepted_drafts"] == 0
    finally:
        ddm.close()
        tdm.close()


# ------------------------------------------------------------------ 5. vocabulary mismatch
@pytest.mark.parametrize("dvocab", [1024, 4096])
def test_vocabulary_mismatch(dvocab):
    R = rt()
    prompt, plain = own_case()
    pos = N_PROMPT - 1
    if dvocab < TGT.vocab_size:
        assert max(plain[:N]) >= dvocab, "precondition: tokens the draft does not have occur in the run"
    tdm = R.DeviceModel.synthetic(TGT, seed=OWN[0], peak=M.PEAKED)
    ddm = R.DeviceModel.synthetic(DRAFT.with_(vocab_size=dvocab), seed=21)
    try:
        for rows in (2, 4):
            with Pair(R, tdm, ddm, prompt) as (tgt, draft):
                got, st = tgt.generate_speculative_model(draft, prompt[-1], pos, N, rows=rows)
                assert got == plain[:N] and identity(st, N)
                # the error word is clean: both decoders go on (a raised word fails the next call)
                assert tgt.generate_greedy(plain[N - 1], pos + N, 4) == plain[N:]
                draft.forward(1, 0)
    finally:
        ddm.close()
        tdm.close()


# ------------------------------------------------------------------ 6. the window's end
WINDOW_PSEED = 202  # chosen on the CPU oracle as SEEDS were


def test_window_end_finishes_with_plain_steps():
    R = rt()
    prompt = prompt_of(WINDOW_PSEED, TGT.max_seq_len - 9)
    pos, n = len(prompt) - 1, 24
    assert pos == TGT.max_seq_len - 10
    dm = R.DeviceModel.synthetic(TGT, seed=OWN[0], peak=M.PEAKED)
    try:
        plain, worst = plain_path(R, dm, prompt, n + 4)
        assert worst > GAP, f"precondition: the plain path of this seed has a near-tie ({worst:.2e} of the range)"
        with Pair(R, dm, dm, prompt) as (tgt, draft):
            got, st = tgt.generate_speculative_model(draft, prompt[-1], pos, n, rows=4)
            print(f"window end: {st}")
            assert got == plain[:n]
            assert st["plain_steps"] > 0 and st["spec_steps"] > 0 and identity(st, n)
            assert tgt.device_step() == (plain[n - 1], pos + n)
            assert tgt.generate_greedy(plain[n - 1], pos + n, 4) == plain[n:]
    finally:
        dm.close()


def test_second_call_finds_the_draft_cache_whole():
    R = rt()
    prompt, plain = own_case()
    pos = N_PROMPT - 1
    dm = R.DeviceModel.synthetic(TGT, seed=OWN[0], peak=M.PEAKED)
    try:
        for rows, first in ((4, 48), (3, 46)):  # (a first call without an overshoot, and one with)
            with Pair(R, dm, dm, prompt) as (tgt, draft):
                a, _ = tgt.generate_speculative_model(draft, prompt[-1], pos, first, rows=rows)
                rest = N - first
                b, st = tgt.generate_speculative_model(draft, a[-1], pos + first, rest, rows=rows)
                assert a + b == plain[:N]
                steps = -(-rest // rows)
                assert st["spec_steps"] == steps and st["accepted_drafts"] == rest - steps, (rows, st)
    finally:
        dm.close()


# ------------------------------------------------------------------ 7. refusals and arguments
def test_refusals_and_arguments():
    R = rt()
    tdm = R.DeviceModel.synthetic(TGT, seed=1)
    ddm = R.DeviceModel.synthetic(DRAFT, seed=2)
    tgt = R.Decoder(tdm)
    s = tgt.get_stream()
    draft = R.Decoder(ddm, stream=s)
    made = []

    def bad(code, what, d=tgt, dr=draft, n=4, **kw):
        with pytest.raises(R.YalmError, match=f"error {code}.*{what}"):
            d.generate_speculative_model(dr, 1, 0, n, **kw)

    try:
        # YALM_ERR_UNSUPPORTED: the draft
        mdm = R.DeviceModel.synthetic(M.TINY_MOE.with_(max_seq_len=256), seed=1)
        moe = R.Decoder(mdm, stream=s)
        made += [moe, mdm]
        bad(3, "mixture-of-experts draft", dr=moe)
        tp = R.Decoder(tdm, tp_gather=lambda h: [h], stream=s)  # (one rank over the IPC transport)
        made.insert(0, tp)
        bad(3, "tensor-parallel draft", dr=tp)
        # YALM_ERR_UNSUPPORTED: the target, in the multi-row path's words
        qdm = R.DeviceModel.synthetic(TGT.with_(weight_dtype=M.Q4, n_layers=1), seed=1)
        q4 = R.Decoder(qdm)
        made += [q4, qdm]
        bad(3, "q4 weights have no multi-row form", d=q4, dr=draft)
        bad(3, "mixture-of-experts decoders have no multi-row form", d=moe, dr=draft)
        # YALM_ERR_ARG
        bad(2, "must not be the target", dr=tgt)
        other = R.Decoder(ddm)  # a stream of its own
        made.insert(0, other)
        bad(2, "yalm_decoder_get_stream", dr=other)
        sdm = R.DeviceModel.synthetic(DRAFT.with_(max_seq_len=128), seed=2)
        short = R.Decoder(sdm, stream=s)
        made += [short, sdm]
        bad(2, "max_seq_len", dr=short)
        bad(2, "rows must be 2..4", rows=1)
        bad(2, "rows must be 2..4", rows=5)
        bad(2, "null argument", rows=None)
        assert R.lib.yalm_generate_speculative_model(tgt.h, None, 1, 0, 4, None, None, None, None, None) == 2
        bad(2, "token buffer", n=65537)
        for kw in (dict(temperature=float("nan")), dict(temperature=-1.0), dict(top_k=-1), dict(top_p=0.0),
                   dict(top_p=1.5), dict(uniforms=[0.5, -0.1, 0.5, 0.5]), dict(uniforms=[0.5, 0.5, 0.5, 1.1])):
            args = dict(temperature=1.0, uniforms=[0.5] * 4, rows=2)
            args.update(kw)
            bad(2, "", **args)
        with pytest.raises(R.YalmError, match="error 2"):
            tgt.generate_speculative_model(draft, TGT.vocab_size, 0, 4)
        with pytest.raises(R.YalmError, match="error 2"):
            tgt.generate_speculative_model(draft, 1, -1, 4)
        assert tgt.generate_speculative_model(draft, 1, 0, 0)[0] == []
        # and the pair still decodes
        got, st = tgt.generate_speculative_model(draft, 1, 0, 6, rows=3)
        assert len(got) == 6 and identity(st, 6)
    finally:
        for x in made:
            x.close()
        draft.close()
        tgt.close()
        ddm.close()
        tdm.close()


# ------------------------------------------------------------------ 8. bystanders unchanged
def test_graph_kernels_of_both_decoders_do_not_move():
    R = rt()
    prompt = prompt_of(108)
    tdm = R.DeviceModel.synthetic(TGT, seed=8)
    ddm = R.DeviceModel.synthetic(DRAFT, seed=3)
    try:
        fresh = R.Decoder(tdm)
        want_t = [fresh.graph_kernels(m) for m in (2, 3)]
        fresh.close()
        fresh = R.Decoder(ddm)
        want_d = [fresh.graph_kernels(m) for m in (2, 3)]
        fresh.close()
        with Pair(R, tdm, ddm, prompt) as (tgt, draft):
            before = [d.graph_kernels(m) for d in (tgt, draft) for m in (2, 3)]
            assert before == want_t + want_d
            tgt.generate_speculative_model(draft, prompt[-1], N_PROMPT - 1, 16, rows=4)
            u = np.random.default_rng(1).random(16, dtype=np.float32)
            tgt.generate_speculative_model(draft, prompt[-1], N_PROMPT - 1, 16, rows=2, temperature=TEMP, top_k=TOP_K,
                                           top_p=TOP_P, uniforms=u)
            assert [d.graph_kernels(m) for d in (tgt, draft) for m in (2, 3)] == before
            # the plain loops of both decoders run what they ran before
            a = tgt.generate_greedy(prompt[-1], N_PROMPT - 1, 8)
            twin = hydrated(R, tdm, prompt)
            assert a == twin.generate_greedy(prompt[-1], N_PROMPT - 1, 8)
            twin.close()
    finally:
        ddm.close()
        tdm.close()
