"""Python restatement of speculative greedy decode's integer rules (include/yalm_hip.h,
yalm_generate_speculative): the n-gram drafter, the acceptance rule and the step loop --
TEST INFRASTRUCTURE. NONE (-1) stands for "no draft".
"""
from __future__ import annotations

NONE = -1
HISTORY_CAP = 65536  # the context keeps its last 65536 tokens


def draft(history, rows: int, ngram_max: int, ngram_min: int) -> list:
    """The rows - 1 drafts from history H[0, m), H[m - 1] the token to feed next: for g =
    ngram_max down to ngram_min the LARGEST i with i + g <= m - 1 and H[i, i + g) == H[m - g, m);
    the first g with such an i wins; d_k = H[i + g + k - 1] while that index is < m, else NONE."""
    h = list(history)
    m = len(h)
    for g in range(ngram_max, ngram_min - 1, -1):
        if g > m - 1:
            continue
        tail = h[m - g:]
        for i in range(m - 1 - g, -1, -1):
            if h[i:i + g] == tail:
                return [h[i + g + k - 1] if i + g + k - 1 < m else NONE for k in range(1, rows)]
    return [NONE] * (rows - 1)


def stream_drafts(stream, produced: int, rows: int) -> list:
    """The draft_stream hook: d_k = stream[produced + k - 1], NONE past its end."""
    return [int(stream[produced + k - 1]) if produced + k - 1 < len(stream) else NONE for k in range(1, rows)]


def accept(drafts, argmaxes) -> int:
    """a = 1 + the longest prefix of drafts with d_k == argmax of row k - 1 (NONE never matches)."""
    a = 1
    while a <= len(drafts) and drafts[a - 1] != NONE and drafts[a - 1] == argmaxes[a - 1]:
        a += 1
    return a


def simulate(next_token, token: int, n: int, rows: int, ngram_max: int = 3, ngram_min: int = 1, context=None,
             stream=None, pos: int = 0, max_seq_len: int = 1 << 30, vocab: int = 1 << 30):
    """Speculative decode of n tokens over next_token(prefix) -> the greedy next token after the
    token sequence `prefix` (which ends with the token fed). Returns (tokens, stats, per-step
    produced counts). A step whose rows would cross max_seq_len, and every step after it, is a
    plain one. Drafts outside [0, vocab) are NONE."""
    ctx = list(context) if context else [token]
    assert ctx[-1] == token
    ctx = ctx[-HISTORY_CAP:]
    out, per_step = [], []
    steps = accepted = plain = 0
    while len(out) < n:
        if pos + len(out) + rows > max_seq_len:
            out.append(next_token(ctx + out))
            plain += 1
            continue
        d = stream_drafts(stream, len(out), rows) if stream is not None else draft(ctx + out, rows, ngram_max, ngram_min)
        d = [x if 0 <= x < vocab else NONE for x in d]
        fed, am = ctx + out, []
        for k in range(rows):  # row k sees the history, then the drafts before it (NONE rows feed token 0)
            am.append(next_token(fed))
            if k < rows - 1:
                fed = fed + [d[k] if d[k] != NONE else 0]
        a = accept(d, am)
        out += am[:a]
        per_step.append(a)
        steps += 1
        accepted += a - 1
    over = len(out) - n  # what the last step accepted past the request is not delivered
    return out[:n], {"spec_steps": steps, "accepted_drafts": accepted - over, "plain_steps": plain}, per_step


def predict(seq, token: int, n: int, rows: int, **kw):
    """simulate() over a known greedy continuation: seq[j] is the j-th greedy token after feeding
    `token` (at least n + rows of them), whatever drafts are tried."""
    base = len(kw["context"]) if kw.get("context") else 1
    base = min(base, HISTORY_CAP)

    def next_token(prefix):
        j = len(prefix) - base
        # a prefix that left the greedy path (a wrong draft was fed) has no known continuation:
        # the rule never looks at it (acceptance stops at the wrong draft)
        return int(seq[j]) if j < len(seq) and list(prefix[base:]) == [int(x) for x in seq[:j]] else -2

    return simulate(next_token, token, n, rows, **kw)
