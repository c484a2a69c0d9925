#!/usr/bin/env python3
"""Speculative greedy decode against the plain greedy loop: step cost, upper bound and the
price of a miss, fp16 and fp8, in one process.

Builds synthetic Mistral-7B-shaped fp16 and fp8 models in HBM and, after the same hydrated
13-token prompt, times (the legs in alternation, `--reps` times each, every rep listed):

  plain      the device greedy loop, `--tokens` tokens (ms per step = ms per token)
  perfect    yalm_generate_speculative with a draft stream equal to the plain loop's own tokens,
             rows 2, 3, 4: every draft is accepted, so this is the multi-row step's cost and the
             upper bound of the speed-up (tokens / rows steps)
  wrong      a draft stream that is wrong everywhere, rows 2 and 4: one token per step, the price
             of a miss

`bar`: tok/s of perfect rows = 4 above the plain loop's by more than the repeat spread (max -
min of the reps) of either leg. `break_even`: the accepted drafts per step a drafter needs at
rows r for the step to pay for itself, ms_step(r) / ms_plain - 1.

There is no trained checkpoint here, so the n-gram drafter's acceptance on real text is not
measured. Every leg runs under the tool's own time limit (--leg-timeout seconds: the process is
ended by SIGALRM if a leg does not return).

--profile: a short run for `rocprofv3 --kernel-trace --stats` (per dtype 8 plain steps and 8
perfect steps at rows 2, 3, 4, eager launches): the per-kernel times of the five row GEMVs
(gemv_rows_kernel<.., T, ..>) beside their single-row kernels (gemv_rb_kernel).

Prints one JSON line per measurement; --out appends them to a file.

Usage: python tools/bench_spec.py [--reps 3] [--tokens 96] [--layers N] [--profile] [--out FILE]
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
    ap.add_argument("--tokens", type=int, default=96, help="tokens per leg (rows = 4: tokens / 4 steps)")
    ap.add_argument("--layers", type=int, default=0, help="fewer layers = a smaller model of the same shapes")
    ap.add_argument("--leg-timeout", type=int, default=120)
    ap.add_argument("--profile", action="store_true")
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
    decs = {k: runtime.Decoder(dm, launch=runtime.LAUNCH_EAGER if args.profile else 0) for k, dm in dms.items()}
    prompt = [(7 * i + 1) % base.vocab_size for i in range(PROMPT_LEN)]  # bench.py's prompt
    tok0, pos0 = prompt[-1], PROMPT_LEN - 1
    n = 32 if args.profile else args.tokens
    try:
        truth = {}
        for k, dec in decs.items():
            for pos, t in enumerate(prompt[:-1]):
                dec.forward(t, pos, runtime.HYDRATE_KV_CACHE)
            truth[k], _ = timed(lambda: dec.generate_greedy(tok0, pos0, n))  # warm-up, and the draft stream
            timed(lambda: dec.generate_speculative(tok0, pos0, 8, rows=4, context=prompt, draft_stream=truth[k]))
        if args.profile:
            for k, dec in decs.items():
                timed(lambda: dec.generate_greedy(tok0, pos0, 8))
                for rows in (2, 3, 4):
                    timed(lambda: dec.generate_speculative(tok0, pos0, 8 * rows, rows=rows, context=prompt,
                                                           draft_stream=truth[k]))
            emit({"leg": "profile", "done": True})
            return
        legs = [("plain", 0)] + [("perfect", r) for r in (2, 3, 4)] + [("wrong", r) for r in (2, 4)]
        res = {k: {leg: [] for leg in legs} for k in decs}
        for _ in range(args.reps):
            for leg in legs:
                for k, dec in decs.items():
                    kind, rows = leg
                    if kind == "plain":
                        toks, ms = timed(lambda: dec.generate_greedy(tok0, pos0, n))
                        st = {"spec_steps": 0, "accepted_drafts": 0, "plain_steps": n, "launches_per_step": dec.graph_kernels(2)}
                    else:
                        stream = truth[k] if kind == "perfect" else [(t + 1) % base.vocab_size for t in truth[k]]
                        (toks, st), ms = timed(lambda: dec.generate_speculative(tok0, pos0, n, rows=rows, context=prompt,
                                                                                draft_stream=stream))
                    res[k][leg].append((ms, st, toks == truth[k]))
        for k in decs:
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
                      "tokens_equal_plain": all(eq for _, _, eq in runs),
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
            be = {}
            for rows in (2, 3, 4):
                st = res[k][("perfect", rows)][0][1]
                ms_step = min(ms / st["spec_steps"] for ms, _, _ in res[k][("perfect", rows)])
                be[str(rows)] = round(ms_step / min(plain_ms) - 1.0, 3)
            emit({"leg": "break_even", "dtype": k, "accepted_drafts_per_step_needed": be})
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
