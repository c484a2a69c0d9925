#!/usr/bin/env python3
"""Speculative sampled decode against the plain sampled loop and against speculative greedy
decode: step cost, upper bound and the price of a miss, fp16 and fp8, in one process.

Builds synthetic Mistral-7B-shaped fp16 and fp8 models in HBM and, after the same hydrated
13-token prompt, times (the legs in alternation, `--reps` times each, every rep listed), at
temperature 0.8, top_k 40, top_p 0.9 with the same uniforms in every leg:

  plain      yalm_generate_sampled, `--tokens` tokens (ms per step = ms per token)
  perfect    yalm_generate_speculative_sampled with a draft stream equal to the sequence the call
             itself delivers, rows 2, 3, 4: every draft is accepted (the step's cost, the upper
             bound). That sequence is the plain sampled one unless a draw fell within the two
             paths' rounding of a boundary (`paths`: where they part, the largest logit difference
             at the first position and the distance between the 40th and 41st logit there)
  wrong      a draft stream that is wrong everywhere, rows 2, 3, 4: one token per step
  greedy4    yalm_generate_speculative at rows 4 with its own perfect stream: the same step with
             the verify launch in the place of the draw and the accept launch

`bar`: tok/s of perfect rows = 4 above the plain sampled loop's by more than the repeat spread
(max - min of the reps) of either leg. `sampled_vs_greedy`: ms per step of perfect rows 4,
sampled minus greedy, beside the per-launch times (yalm_time_kernel) of the draw launch (12),
the accept launch (13) and the verify launch (14) on the rows' logits.

There is no trained checkpoint here, so the n-gram drafter's acceptance under sampling on real
text is not measured. Every leg runs under the tool's own time limit (--leg-timeout seconds).

Prints one JSON line per measurement; --out appends them to a file.

Usage: python tools/bench_spec_sampled.py [--reps 3] [--tokens 96] [--layers N] [--out FILE]
"""
import argparse
import json
import os
import signal
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PROMPT_LEN = 13
TEMP, TOP_K, TOP_P = 0.8, 40, 0.9


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tokens", type=int, default=96)
    ap.add_argument("--layers", type=int, default=0, help="fewer layers = a smaller model of the same shapes")
    ap.add_argument("--kernel-iters", type=int, default=200)
    ap.add_argument("--leg-timeout", type=int, default=120)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)

    from yalm_amd import models as M
    from yalm_amd import runtime

    runtime.check(runtime.lib.yalm_set_device(0))
    signal.signal(signal.SIGALRM, signal.SIG_DFL)  # a leg that does not return ends the process
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    def timed(fn):
        signal.alarm(args.leg_timeout)
        t0 = time.perf_counter()
        r = fn()
        dt = time.perf_counter() - t0
        signal.alarm(0)
        return r, dt * 1e3

    base = M.MISTRAL_7B.with_(n_layers=args.layers) if args.layers else M.MISTRAL_7B
    cfgs = {"fp16": base.with_(weight_dtype=M.F16), "fp8": base.with_(weight_dtype=M.F8E5M2)}
    dms = {k: runtime.DeviceModel.synthetic(c, seed=1) for k, c in cfgs.items()}
    decs = {k: runtime.Decoder(dm) for k, dm in dms.items()}
    prompt = [(7 * i + 1) % base.vocab_size for i in range(PROMPT_LEN)]  # bench.py's prompt
    tok0, pos0 = prompt[-1], PROMPT_LEN - 1
    n = args.tokens
    u = np.random.default_rng(1).random(n, dtype=np.float32)
    smp = dict(temperature=TEMP, top_k=TOP_K, top_p=TOP_P, uniforms=u)
    try:
        truth, gtruth = {}, {}
        for k, dec in decs.items():
            for pos, t in enumerate(prompt[:-1]):
                dec.forward(t, pos, runtime.HYDRATE_KV_CACHE)
            truth[k], _ = timed(lambda: dec.generate_sampled(tok0, pos0, n, **smp))  # warm-up, and the draft stream
            gtruth[k], _ = timed(lambda: dec.generate_greedy(tok0, pos0, n))
            timed(lambda: dec.generate_speculative_sampled(tok0, pos0, 8, TEMP, TOP_K, TOP_P, uniforms=u[:8], rows=4,
                                                           context=prompt, draft_stream=truth[k]))
        # the sequence each row count delivers (every draft wrong: all tokens from row 0), as its perfect stream
        own = {}
        for k, dec in decs.items():
            wrong = [(t + 1) % base.vocab_size for t in truth[k]]
            for rows in (2, 3, 4):
                (own[k, rows], _), _ = timed(lambda: dec.generate_speculative_sampled(
                    tok0, pos0, n, rows=rows, context=prompt, draft_stream=wrong, **smp))
            first = [next((i for i in range(n) if own[k, r][i] != truth[k][i]), None) for r in (2, 3, 4)]
            l1 = dec.forward(tok0, pos0).copy()
            l4 = dec.forward_rows([tok0, truth[k][0], truth[k][1], truth[k][2]], pos0)[0]
            top = np.sort(l1)[::-1]
            emit({"leg": "paths", "dtype": k, "first_token_differing_from_plain_rows234": first,
                  "max_abs_dlogit_pos0": float(np.max(np.abs(l1 - l4))), "logit_40_minus_41_pos0": float(top[39] - top[40]),
                  "logit_max_minus_40_pos0": float(top[0] - top[39])})
        legs = ([("plain", 0)] + [("perfect", r) for r in (2, 3, 4)] + [("wrong", r) for r in (2, 3, 4)]
                + [("greedy4", 4)])
        res = {k: {leg: [] for leg in legs} for k in decs}
        for _ in range(args.reps):
            for leg in legs:
                for k, dec in decs.items():
                    kind, rows = leg
                    if kind == "plain":
                        toks, ms = timed(lambda: dec.generate_sampled(tok0, pos0, n, **smp))
                        st = {"spec_steps": 0, "accepted_drafts": 0, "plain_steps": n,
                              "launches_per_step": dec.graph_kernels(3)}
                        eq = toks == truth[k]
                    elif kind == "greedy4":
                        (toks, st), ms = timed(lambda: dec.generate_speculative(tok0, pos0, n, rows=rows, context=prompt,
                                                                                draft_stream=gtruth[k]))
                        eq = toks == gtruth[k]
                    else:
                        ref = own[k, rows]
                        stream = ref if kind == "perfect" else [(t + 1) % base.vocab_size for t in ref]
                        (toks, st), ms = timed(lambda: dec.generate_speculative_sampled(
                            tok0, pos0, n, rows=rows, context=prompt, draft_stream=stream, **smp))
                        eq = toks == ref
                    res[k][leg].append((ms, st, eq))
        for k, dec in decs.items():
            plain_ms = [ms / n for ms, _, _ in res[k][("plain", 0)]]
            for leg in legs:
                kind, rows = leg
                runs = res[k][leg]
                st = runs[0][1]
                steps = st["spec_steps"] + st["plain_steps"]
                per_step = [ms / steps for ms, _, _ in runs]
                tok_s = [n / ms * 1e3 for ms, _, _ in runs]
                emit({"leg": kind, "dtype": k, "rows": rows, "tokens": n, "steps": steps, "n_layers": base.n_layers,
                      "accepted_drafts": st["accepted_drafts"], "launches_per_step": st["launches_per_step"],
                      "tokens_equal_reference_leg": all(eq for _, _, eq in runs),
                      "ms_per_step": round(min(per_step), 4), "ms_per_step_all": [round(x, 4) for x in per_step],
                      "tok_s": round(max(tok_s), 1), "tok_s_all": [round(x, 1) for x in tok_s],
                      "spread_tok_s": round(max(tok_s) - min(tok_s), 1),
                      "step_ratio_to_plain": round(min(per_step) / min(plain_ms), 3),
                      "tok_s_ratio_to_plain": round(max(tok_s) / (1e3 / min(plain_ms)), 3)})
            p = [n / ms * 1e3 for ms, _, _ in res[k][("plain", 0)]]
            s4 = [n / ms * 1e3 for ms, _, _ in res[k][("perfect", 4)]]
            spread = max(max(p) - min(p), max(s4) - min(s4))
            emit({"leg": "bar", "dtype": k, "perfect4_minus_plain_tok_s": round(max(s4) - max(p), 1),
                  "repeat_spread_tok_s": round(spread, 1), "perfect4_faster_beyond_spread": bool(max(s4) - max(p) > spread)})
            step = {leg: [ms / runs_st["spec_steps"] for ms, runs_st, _ in res[k][leg]]
                    for leg in (("perfect", 4), ("greedy4", 4))}
            kern = {name: round(dec.time_kernel(kid, args.kernel_iters) * 1e3, 2)
                    for name, kid in (("draw_rows4", 12), ("accept", 13), ("verify_rows4", 14), ("draw_1row", 10))}
            emit({"leg": "sampled_vs_greedy", "dtype": k, "rows": 4,
                  "sampled_ms_per_step": round(min(step[("perfect", 4)]), 4),
                  "greedy_ms_per_step": round(min(step[("greedy4", 4)]), 4),
                  "difference_us": round((min(step[("perfect", 4)]) - min(step[("greedy4", 4)])) * 1e3, 1),
                  "launch_us": kern,
                  "launches_difference_us": round(kern["draw_rows4"] + kern["accept"] - kern["verify_rows4"], 2)})
    finally:
        for d in decs.values():
            d.close()
        for d in dms.values():
            d.close()
        if args.out and lines:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
