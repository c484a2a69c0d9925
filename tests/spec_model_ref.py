"""Numpy model of speculative decode with a draft model (include/yalm_hip.h,
yalm_generate_speculative_model) over two CPU oracle models -- TEST INFRASTRUCTURE.

The target's rows are sequential oracle forwards (row t at pos + t sees keys 0 .. pos + t and
writes its KV row, as the multi-row step does); the draft is a second oracle model with a cache
of its own. `slip` breaks one piece of the step on purpose, so that the CPU tests can show that
the acceptance cases notice each of them:

  no-hydrate    no KV-only forward of the last draft
  sync-stale    the draft is synchronised to the position before the previous step's accept
  gather-shift  d_k read from the draft's token buffer at k, not k - 1
  no-clear      drafts kept after an out-of-vocabulary feed (the draft was fed token 0)
  u-by-step     uniforms indexed by step, not by output index
  draft-pos     the draft fed d_k at pos + k - 1, not pos + k
"""
from __future__ import annotations

import numpy as np

import sampling_ref as SR
import spec_ref as S

SLIPS = ("no-hydrate", "sync-stale", "gather-shift", "no-clear", "u-by-step", "draft-pos")


def argmax(logits) -> int:
    return SR.first_max(logits)[1]


def draw(logits, prm, u) -> int:
    """The sampling rule on numpy f32 weights (sampling_ref)."""
    temperature, top_k, top_p = prm
    return SR.Rule(logits, SR.weights_f32(logits, temperature), top_k, top_p).draw(u)


def run(target, draft, token: int, pos: int, n: int, rows: int, prm=None, uniforms=None, draft_stream=None,
        slip: str = None):
    """(tokens, stats, trace): trace[i] = (pos, drafts after the gather, accepted count) of step i.
    prm = (temperature, top_k, top_p) with `uniforms` (n values): the sampled call; None: greedy."""
    assert slip is None or slip in SLIPS
    tv, dv, msl = target.cfg.vocab_size, draft.cfg.vocab_size, target.cfg.max_seq_len
    out, trace = [], []
    steps = acc = plain = 0
    tok, p, prev_p = token, pos, pos
    dbuf = [0] * 8  # the draft decoder's token buffer

    def choose(lg, ui):
        return argmax(lg) if prm is None else draw(lg, prm, uniforms[min(ui, n - 1)])

    while len(out) < n:
        if p + rows > msl:  # the window's end: plain steps of the target alone
            t = choose(target.forward(tok, p), len(out))
            out.append(t)
            tok, p, plain = t, p + 1, plain + 1
            continue
        # 1. sync
        none = not (0 <= tok < dv)
        dtok, dpos = (0 if none else tok), (prev_p if slip == "sync-stale" else p)
        # 2. rows - 1 greedy forwards, then the KV-only forward of the last draft
        for k in range(1, rows):
            dtok = argmax(draft.forward(dtok, dpos))
            dbuf[k - 1] = dtok
            if not (slip == "draft-pos" and k == 1):
                dpos += 1
        if slip != "no-hydrate":
            draft.forward(dtok, dpos, 0)
        # 3. gather
        if draft_stream is not None:
            d = S.stream_drafts(draft_stream, len(out), rows)
        elif none and slip != "no-clear":
            d = [S.NONE] * (rows - 1)
        else:
            d = [dbuf[k] if slip == "gather-shift" else dbuf[k - 1] for k in range(1, rows)]
        d = [x if 0 <= x < tv else S.NONE for x in d]
        # 4. the target's rows, each choice with the uniform of the output index it would fill
        fed = [tok] + [x if x != S.NONE else 0 for x in d]
        base = steps if slip == "u-by-step" else len(out)
        chosen = [choose(target.forward(fed[t], p + t), base + t) for t in range(rows)]
        a = S.accept(d, chosen)
        trace.append((p, d, a))
        out += chosen[:a]
        prev_p = p
        tok, p, steps, acc = chosen[a - 1], p + a, steps + 1, acc + a - 1
    over = len(out) - n
    return out[:n], {"spec_steps": steps, "accepted_drafts": acc - over, "plain_steps": plain}, trace
