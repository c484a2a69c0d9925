"""CPU: the Python reference of speculative greedy decode (tests/spec_ref.py) -- whatever is
drafted, the loop reproduces the greedy sequence of the next-token function, one to `rows`
tokens per step; and the drafter rule on the crafted histories the GPU test runs."""
import numpy as np
import pytest

import spec_ref as S


def lcg_model(vocab, period):
    """A fixed next-token function of the prefix: depends on the last two tokens and the length
    modulo `period`, so its greedy sequences repeat often enough for n-gram drafts to hit."""

    def f(prefix):
        a = prefix[-1]
        b = prefix[-2] if len(prefix) > 1 else 0
        return (a * 7 + b * 3 + len(prefix) % period) % vocab

    return f


def greedy(f, ctx, n):
    p, out = list(ctx), []
    for _ in range(n):
        out.append(f(p))
        p.append(out[-1])
    return out


@pytest.mark.parametrize("rows", [2, 3, 4])
@pytest.mark.parametrize("kind", ["ngram", "random", "true", "wrong", "third"])
def test_simulation_reproduces_greedy(rows, kind):
    vocab, n = 11, 57
    f = lcg_model(vocab, 1 if kind == "ngram" else 3)
    ctx = [3, 1, 4, 1, 5]
    want = greedy(f, ctx, n + rows)
    rng = np.random.default_rng(rows)
    stream = {"ngram": None, "random": rng.integers(0, vocab, n).tolist(), "true": want[:n],
              "wrong": [(t + 1) % vocab for t in want[:n]],
              "third": [(t + 1) % vocab if j % 3 == 2 else t for j, t in enumerate(want[:n])]}[kind]
    got, st, per = S.simulate(f, ctx[-1], n, rows, 3, 1, context=ctx, stream=stream)
    assert got == want[:n]
    assert all(1 <= a <= rows for a in per)
    assert st["spec_steps"] == len(per) and st["plain_steps"] == 0
    assert st["spec_steps"] + st["accepted_drafts"] == n
    if kind == "true":
        assert st["spec_steps"] == -(-n // rows)
    if kind == "wrong":
        assert st["spec_steps"] == n and st["accepted_drafts"] == 0
    if kind == "ngram":
        assert st["accepted_drafts"] > 0  # the period-1 model loops: the drafter must profit
    # predict() from the known sequence gives the same counts without running the model on drafts
    got2, st2, per2 = S.predict(want, ctx[-1], n, rows, ngram_max=3, ngram_min=1, context=ctx, stream=stream)
    assert (got2, st2, per2) == (got, st, per)


def test_window_end_turns_plain():
    f = lcg_model(13, 2)
    ctx = [5, 6]
    want = greedy(f, ctx, 30)
    got, st, _ = S.simulate(f, ctx[-1], 30, 4, context=ctx, stream=want, pos=50, max_seq_len=64)
    assert got == want
    assert st["plain_steps"] > 0 and st["spec_steps"] > 0
    assert st["spec_steps"] + st["accepted_drafts"] + st["plain_steps"] == 30


# (history, rows, ngram_max, ngram_min, expected drafts): the cases of tests/test_gpu_spec.py
DRAFT_CASES = {
    "no-match": ([1, 2, 3, 4, 5], 4, 3, 1, [-1, -1, -1]),
    "g1-only": ([7, 9, 8, 2, 3, 9], 4, 3, 1, [8, 2, 3]),
    "latest-wins": ([1, 2, 5, 1, 2, 6, 1, 2], 3, 2, 1, [6, 1]),
    "longest-g-first": ([4, 1, 2, 8, 3, 2, 9, 1, 2], 3, 3, 1, [8, 3]),
    "runs-into-end": ([5, 6, 5], 4, 3, 1, [6, 5, -1]),
    "overlap-aaaa": ([3, 3, 3, 3], 4, 4, 1, [3, -1, -1]),
    "length-1": ([42], 4, 3, 1, [-1, -1, -1]),
    "shorter-than-min": ([1, 1], 4, 4, 3, [-1, -1, -1]),
    "min-2-skips-g1": ([7, 9, 8, 2, 3, 9], 4, 3, 2, [-1, -1, -1]),
}


@pytest.mark.parametrize("name", sorted(DRAFT_CASES))
def test_drafter_rule_on_crafted_histories(name):
    h, rows, gmax, gmin, want = DRAFT_CASES[name]
    assert S.draft(h, rows, gmax, gmin) == want


def long_history():
    """65536 tokens whose only match of the final 2-gram is at index 0."""
    h = (np.arange(65536, dtype=np.int64) % 1000 + 10).astype(np.int32)
    h[0], h[1], h[2], h[3] = 5, 6, 777, 778
    h[-2], h[-1] = 5, 6
    return h


def test_long_history_single_match_at_zero():
    h = long_history()
    assert S.draft(h.tolist(), 4, 2, 2) == [777, 778, int(h[4])]
