"""CPU: the loop of speculative decode with a draft model (yalm_generate_speculative_model) as a
numpy model over two CPU oracle models (tests/spec_model_ref.py), on TINY-sized models.

On the CPU the target's rows and the plain loop are the same oracle forwards, so every equality
here is exact: the delivered tokens never depend on the draft, a draft over the target's own
weights is accepted at every row, and each deliberate slip of the step (spec_model_ref.SLIPS)
shows in the tokens or in the acceptance count of those same cases.
"""
import functools

import numpy as np
import pytest

import oracle_py as O
import spec_model_ref as SM
from yalm_amd import models as M

CFG = M.TINY  # vocabulary 384, window 64
N_PROMPT, N = 13, 40
PRM = (0.8, 40, 0.9)


@functools.lru_cache(maxsize=None)
def tensors(seed, vocab=CFG.vocab_size, peak=M.PEAKED):
    t = O.synth_host_tensors_fast(CFG.with_(vocab_size=vocab), seed=seed, peak=peak)
    for a in t.values():
        a.setflags(write=False)
    return t


def prompt(n=N_PROMPT, vocab=CFG.vocab_size):
    return [int(t) for t in np.random.default_rng(100 + n).integers(1, vocab, n)]


def model(seed, toks, vocab=CFG.vocab_size, hydrate=True):
    om = O.OracleModel(CFG.with_(vocab_size=vocab), tensors(seed, vocab))
    if hydrate:
        for p, t in enumerate(toks[:-1]):
            om.forward(min(t, vocab - 1), p, 0)
    return om


def plain(seed, toks, n, prm=None, u=None):
    om, tok, out = model(seed, toks), toks[-1], []
    for i in range(n):
        lg = om.forward(tok, len(toks) - 1 + i)
        tok = SM.argmax(lg) if prm is None else SM.draw(lg, prm, u[i])
        out.append(tok)
    return out


def identity(st, n):
    return st["spec_steps"] + st["accepted_drafts"] + st["plain_steps"] == n


# ------------------------------------------------------------------ the draft over the target's weights
@pytest.mark.parametrize("rows", [2, 3, 4])
def test_own_weights_draft_is_accepted_everywhere(rows):
    toks = prompt()
    want = plain(5, toks, N)
    got, st, trace = SM.run(model(5, toks), model(5, toks), toks[-1], N_PROMPT - 1, N, rows)
    assert got == want
    steps = -(-N // rows)
    assert st == {"spec_steps": steps, "accepted_drafts": N - steps, "plain_steps": 0}
    assert all(a == rows for _, _, a in trace)


def test_second_call_continues_with_a_whole_draft_cache():
    toks = prompt()
    want = plain(5, toks, N)
    tgt, dr = model(5, toks), model(5, toks)
    a, st = SM.run(tgt, dr, toks[-1], N_PROMPT - 1, 20, 4)[:2]
    b, st2 = SM.run(tgt, dr, a[-1], N_PROMPT - 1 + 20, 20, 4)[:2]
    assert a + b == want
    assert st2 == {"spec_steps": 5, "accepted_drafts": 15, "plain_steps": 0}


def test_window_end_finishes_with_plain_steps():
    toks = prompt(CFG.max_seq_len - 9)  # the call starts at pos = max_seq_len - 10
    pos, n = len(toks) - 1, 24
    assert pos == CFG.max_seq_len - 10
    want = plain(5, toks, n + 4)
    tgt = model(5, toks)
    got, st, _ = SM.run(tgt, model(5, toks), toks[-1], pos, n, 4)
    assert got == want[:n]
    assert st["plain_steps"] > 0 and st["spec_steps"] > 0 and identity(st, n)
    assert st["spec_steps"] + st["accepted_drafts"] == 8  # steps at pos 54 and 58; 62 + 4 > 64
    nxt, tok = [], got[-1]
    for i in range(4):  # the target continues as the plain loop does
        tok = SM.argmax(tgt.forward(tok, pos + n + i))
        nxt.append(tok)
    assert nxt == want[n:]


# ------------------------------------------------------------------ the tokens never depend on the draft
@pytest.mark.parametrize("rows", [2, 4])
def test_random_and_unhydrated_drafts_cost_acceptance_only(rows):
    toks = prompt()
    want = plain(5, toks, N)
    for dseed, hyd in ((9, True), (5, False)):
        got, st, _ = SM.run(model(5, toks), model(dseed, toks, hydrate=hyd), toks[-1], N_PROMPT - 1, N, rows)
        assert got == want and identity(st, N)
        assert st["accepted_drafts"] < N - -(-N // rows)


@pytest.mark.parametrize("rows", [2, 3, 4])
def test_sampled_tokens_are_the_plain_sampled_loop(rows):
    toks = prompt()
    u = np.random.default_rng(7).random(N, dtype=np.float32)
    want = plain(5, toks, N, PRM, u)
    assert len(set(want)) > 4
    for dseed in (5, 9):
        got, st, _ = SM.run(model(5, toks), model(dseed, toks), toks[-1], N_PROMPT - 1, N, rows, prm=PRM, uniforms=u)
        assert got == want and identity(st, N)


def test_draft_stream_replaces_the_drafts():
    toks = prompt()
    want = plain(5, toks, N)
    wrong = [(t + 1) % CFG.vocab_size for t in want]
    got, st, _ = SM.run(model(5, toks), model(9, toks), toks[-1], N_PROMPT - 1, N, 4, draft_stream=want)
    assert got == want and st["spec_steps"] == N // 4 and st["accepted_drafts"] == N - N // 4
    got, st, _ = SM.run(model(5, toks), model(5, toks), toks[-1], N_PROMPT - 1, N, 4, draft_stream=wrong)
    assert got == want and st["spec_steps"] == N and st["accepted_drafts"] == 0


@pytest.mark.parametrize("dvocab", [192, 768])
def test_vocabulary_mismatch(dvocab):
    toks = prompt()
    want = plain(5, toks, N)
    if dvocab < CFG.vocab_size:
        assert max(want) >= dvocab  # tokens the draft does not have occur
    got, st, trace = SM.run(model(5, toks), model(9, toks, vocab=dvocab), toks[-1], N_PROMPT - 1, N, 4)
    assert got == want and identity(st, N)
    assert all(0 <= x < CFG.vocab_size or x == -1 for _, d, _ in trace for x in d)


# ------------------------------------------------------------------ every slip shows
@pytest.mark.parametrize("slip", ["no-hydrate", "sync-stale", "gather-shift", "draft-pos"])
def test_slip_costs_acceptance_with_the_own_weights_draft(slip):
    toks = prompt()
    want = plain(5, toks, N)
    got, st, _ = SM.run(model(5, toks), model(5, toks), toks[-1], N_PROMPT - 1, N, 4, slip=slip)
    assert got == want and identity(st, N)  # the tokens still do not depend on the draft
    assert st["accepted_drafts"] < N - N // 4, slip


def test_slip_no_hydrate_shows_in_the_second_call():
    toks = prompt()
    tgt, dr = model(5, toks), model(5, toks)
    a = SM.run(tgt, dr, toks[-1], N_PROMPT - 1, 20, 4, slip="no-hydrate")[0]
    st2 = SM.run(tgt, dr, a[-1], N_PROMPT - 1 + 20, 20, 4)[1]
    assert st2["accepted_drafts"] < 15  # the holes the first call left in the draft's cache


def test_slip_uniforms_by_step_changes_the_tokens():
    toks = prompt()
    u = np.random.default_rng(7).random(N, dtype=np.float32)
    want = plain(5, toks, N, PRM, u)
    got = SM.run(model(5, toks), model(5, toks), toks[-1], N_PROMPT - 1, N, 4, prm=PRM, uniforms=u, slip="u-by-step")[0]
    assert got != want


def test_slip_no_clear_proposes_drafts_of_a_token_never_fed():
    """After a feed of token 0 in place of a token the draft does not have, uncleared drafts are
    the continuation of a token that was never produced: the cleared run proposes none there."""
    toks = prompt()
    clean = SM.run(model(5, toks), model(9, toks, vocab=192), toks[-1], N_PROMPT - 1, N, 4)[2]
    slip = SM.run(model(5, toks), model(9, toks, vocab=192), toks[-1], N_PROMPT - 1, N, 4, slip="no-clear")[2]
    none = [i for i, (_, d, _) in enumerate(clean) if d == [-1, -1, -1]]
    assert none and any(slip[i][1] != [-1, -1, -1] for i in none if i < len(slip))
