#!/usr/bin/env python3
"""Speculative decode with a draft model against the plain greedy loop and the n-gram loop:
step cost, the draft's share of it and the break-even acceptance, fp16 and fp8, in one process.

Builds synthetic Mistral-7B-shaped fp16 and fp8 targets and, for each, a synthetic draft of the
same vocabulary at a 1B shape (dim 2048, hidden 8192, 16 layers, 32 / 8 heads of 64) in the same
format, on the target's stream. After the same hydrated 13-token prompt on both it times (the
legs in alternation, `--reps` times each, every rep listed):

  plain          the target's device greedy loop, `--tokens` tokens
  model-perfect  yalm_generate_speculative_model, rows 2, 3, 4, with a draft stream equal to the
                 plain loop's own tokens: the draft's forwards run and are paid for, every draft is
                 accepted -- a draft model's true step cost at acceptance 1
  model-own      the same with the draft's own proposals (random weights: acceptance near 0, the
                 other end -- one token per step at the full step cost)
  ngram-perfect  yalm_generate_speculative with the same perfect stream, rows 2, 3, 4: the step
                 without a draft model

`draft_share`: (ms_step(model-perfect) - ms_step(ngram-perfect)) / ms_step(model-perfect) at the
same rows. `break_even`: the accepted drafts per step at which a step pays for itself,
ms_step(model-perfect) / ms_plain - 1, per rows. `bar`: tok/s of model-perfect at its best row
count above the plain loop's by more than the larger repeat spread (max - min of the reps) of the
two legs.

There is no trained checkpoint pair here, so a draft model's acceptance on real text is not
measured. Every leg runs under the tool's own time limit (--leg-timeout seconds: the process is
ended by SIGALRM if a leg does not return).

Prints one JSON line per measurement; --out appends them to a file.

Usage: python tools/bench_spec_model.py [--reps 3] [--tokens 96] [--layers N] [--out FILE]
"""
import argparse
import json
import os
import signal
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PROMPT_LEN = 13


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tokens", type=int, default=96)
    ap.add_argument("--layers", type=int, default=0, help="fewer target layers = a smaller model of the same shapes")
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
    small = base.with_(dim=2048, hidden_dim=8192, n_layers=16, n_heads=32, n_kv_heads=8, head_dim=64, rotary_dim=64)
    dts = {"fp16": M.F16, "fp8": M.F8E5M2}
    dms = {k: runtime.DeviceModel.synthetic(base.with_(weight_dtype=d), seed=1) for k, d in dts.items()}
    ddms = {k: runtime.DeviceModel.synthetic(small.with_(weight_dtype=d), seed=2) for k, d in dts.items()}
    decs = {k: runtime.Decoder(dm) for k, dm in dms.items()}
    drafts = {k: runtime.Decoder(ddms[k], stream=decs[k].get_stream()) for k in dts}
    prompt = [(7 * i + 1) % base.vocab_size for i in range(PROMPT_LEN)]  # bench.py's prompt
    tok0, pos0 = prompt[-1], PROMPT_LEN - 1
    n = args.tokens
    try:
        truth = {}
        for k, dec in decs.items():
            for pos, t in enumerate(prompt[:-1]):
                dec.forward(t, pos, runtime.HYDRATE_KV_CACHE)
                drafts[k].forward(t, pos, runtime.HYDRATE_KV_CACHE)
            truth[k], _ = timed(lambda: dec.generate_greedy(tok0, pos0, n))  # warm-up, and the draft stream
            timed(lambda: dec.generate_speculative(tok0, pos0, 8, rows=4, context=prompt, draft_stream=truth[k]))
            timed(lambda: dec.generate_speculative_model(drafts[k], tok0, pos0, 8, rows=4, draft_stream=truth[k]))
        legs = ([("plain", 0)] + [("model-perfect", r) for r in (2, 3, 4)] + [("model-own", r) for r in (2, 3, 4)]
                + [("ngram-perfect", r) for r in (2, 3, 4)])
        res = {k: {leg: [] for leg in legs} for k in decs}
        for _ in range(args.reps):
            for leg in legs:
                for k, dec in decs.items():
                    kind, rows = leg
                    if kind == "plain":
                        toks, ms = timed(lambda: dec.generate_greedy(tok0, pos0, n))
                        st = {"spec_steps": 0, "accepted_drafts": 0, "plain_steps": n,
                              "launches_per_step": dec.graph_kernels(2)}
                    elif kind == "ngram-perfect":
                        (toks, st), ms = timed(lambda: dec.generate_speculative(tok0, pos0, n, rows=rows, context=prompt,
                                                                                draft_stream=truth[k]))
                    else:
                        stream = truth[k] if kind == "model-perfect" else None
                        (toks, st), ms = timed(lambda: dec.generate_speculative_model(drafts[k], tok0, pos0, n, rows=rows,
                                                                                      draft_stream=stream))
                    res[k][leg].append((ms, st, toks == truth[k]))
        for k in decs:
            plain_ms = min(ms / n for ms, _, _ in res[k][("plain", 0)])
            step_ms = {}
            for leg in legs:
                kind, rows = leg
                runs = res[k][leg]
                st = runs[0][1]
                steps = st["spec_steps"] + st["plain_steps"]
                per_step = [ms / steps for ms, _, _ in runs]
                tok_s = [n / ms * 1e3 for ms, _, _ in runs]
                step_ms[leg] = min(per_step)
                emit({"leg": kind, "dtype": k, "rows": rows, "tokens": n, "steps": steps, "n_layers": base.n_layers,
                      "draft_layers": small.n_layers, "accepted_drafts": st["accepted_drafts"],
                      "launches_per_step": st["launches_per_step"], "tokens_equal_plain": all(eq for _, _, eq in runs),
                      "ms_per_step": round(min(per_step), 4), "ms_per_step_all": [round(x, 4) for x in per_step],
                      "tok_s": round(max(tok_s), 1), "tok_s_all": [round(x, 1) for x in tok_s],
                      "spread_tok_s": round(max(tok_s) - min(tok_s), 1),
                      "step_ratio_to_plain": round(min(per_step) / plain_ms, 3),
                      "tok_s_ratio_to_plain": round(max(tok_s) / (1e3 / plain_ms), 3)})
            share = {str(r): round(1.0 - step_ms[("ngram-perfect", r)] / step_ms[("model-perfect", r)], 3) for r in (2, 3, 4)}
            emit({"leg": "draft_share", "dtype": k, "draft_forwards_share_of_step": share})
            be = {str(r): round(step_ms[("model-perfect", r)] / plain_ms - 1.0, 3) for r in (2, 3, 4)}
            emit({"leg": "break_even", "dtype": k, "accepted_drafts_per_step_needed": be})
            p = [n / ms * 1e3 for ms, _, _ in res[k][("plain", 0)]]
            best = max((2, 3, 4), key=lambda r: max(n / ms for ms, _, _ in res[k][("model-perfect", r)]))
            s = [n / ms * 1e3 for ms, _, _ in res[k][("model-perfect", best)]]
            spread = max(max(p) - min(p), max(s) - min(s))
            emit({"leg": "bar", "dtype": k, "best_rows": best, "model_perfect_minus_plain_tok_s": round(max(s) - max(p), 1),
                  "repeat_spread_tok_s": round(spread, 1), "tok_s_ratio_to_plain": round(max(s) / max(p), 3),
                  "model_perfect_faster_beyond_spread": bool(max(s) - max(p) > spread)})
    finally:
        for d in drafts.values():
            d.close()
        for d in decs.values():
            d.close()
        for d in list(ddms.values()) + list(dms.values()):
            d.close()
        if args.out and lines:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
