#!/usr/bin/env python3
"""Batched decode against the plain greedy loop and the speculative step, fp16 and fp8, in one
process.

Builds synthetic Mistral-7B-shaped fp16 and fp8 models in HBM and, after the same hydrated
13-token prompt, times (the legs in alternation, `--reps` times each, every rep listed):

  plain      the device greedy loop, `--steps` steps (one token per step)
  spec       yalm_generate_speculative with a draft stream equal to the plain loop's own tokens,
             rows B = 2, 3, 4, B * steps tokens: every draft is accepted, so a step is the multi-row
             verify step (draft, rows begin, per layer 4 + B launches, logits, verify)
  batch      yalm_batch_generate_greedy, B = 2, 3, 4 sequences loaded with the same prompt, `--steps`
             steps, in both attention forms ("one": one attention launch per layer for all
             sequences; "per_seq": one per sequence)

Reports ms per step and aggregate tok/s (B tokens per step). The claims, each against legs of
this run:
  1. batch B = 4 aggregate tok/s above the plain loop's by more than the repeat spread of either leg;
  2. the batch step at B rows no slower than the speculative step at the same rows, within the spread;
  3. which attention form is faster, and whether by more than the spread.

Every leg runs under the tool's own time limit (--leg-timeout seconds: the process is ended by
SIGALRM if a leg does not return).

--profile: a short run for `rocprofv3 --kernel-trace --stats` (per dtype 8 steps of the batch at
B = 4 in each attention form).

Prints one JSON line per measurement; --out appends them to a file.

Usage: python tools/bench_batch.py [--reps 3] [--steps 96] [--layers N] [--profile] [--out FILE]
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
    ap.add_argument("--steps", type=int, default=96)
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
    decs = {k: runtime.Decoder(dm) for k, dm in dms.items()}
    prompt = [(7 * i + 1) % base.vocab_size for i in range(PROMPT_LEN)]  # bench.py's prompt
    tok0, pos0 = prompt[-1], PROMPT_LEN - 1
    n = 8 if args.profile else args.steps
    FORMS = {"one": 0, "per_seq": runtime.BATCH_ATTN_PER_SEQ}
    batches = {}
    try:
        truth = {}
        for k, dec in decs.items():
            for pos, t in enumerate(prompt[:-1]):
                dec.forward(t, pos, runtime.HYDRATE_KV_CACHE)
            truth[k], _ = timed(lambda: dec.generate_greedy(tok0, pos0, 4 * n))  # warm-up, and the draft stream
            for B in (2, 3, 4):
                b = runtime.Batch(dec, B)
                b.load(pos0)
                batches[k, B] = b
                for flags in FORMS.values():  # warm-up of both forms
                    b.set_launch(flags)
                    timed(lambda: b.generate_greedy([tok0] * B, [pos0] * B, 4))
            timed(lambda: dec.generate_speculative(tok0, pos0, 8, rows=4, context=prompt, draft_stream=truth[k]))
        if args.profile:
            for k in decs:
                for flags in FORMS.values():
                    batches[k, 4].set_launch(flags)
                    timed(lambda: batches[k, 4].generate_greedy([tok0] * 4, [pos0] * 4, n))
            emit({"leg": "profile", "done": True})
            return
        legs = [("plain", 1, "")] + [("spec", B, "") for B in (2, 3, 4)] + \
               [("batch", B, f) for B in (2, 3, 4) for f in FORMS]
        res = {k: {leg: [] for leg in legs} for k in decs}
        for _ in range(args.reps):
            for leg in legs:
                kind, B, form = leg
                for k, dec in decs.items():
                    if kind == "plain":
                        toks, ms = timed(lambda: dec.generate_greedy(tok0, pos0, n))
                        ok, launches = toks == truth[k][:n], dec.graph_kernels(2)
                    elif kind == "spec":
                        (toks, st), ms = timed(lambda: dec.generate_speculative(tok0, pos0, B * n, rows=B, context=prompt,
                                                                                draft_stream=truth[k]))
                        ok = toks == truth[k][:B * n] and st["spec_steps"] == n
                        launches = st["launches_per_step"]
                    else:
                        b = batches[k, B]
                        b.set_launch(FORMS[form])
                        (toks, st), ms = timed(lambda: b.generate_greedy([tok0] * B, [pos0] * B, n))
                        ok = all(row == toks[0].tolist() for row in toks.tolist())  # one prompt: one greedy path
                        launches = st["launches_per_step"]
                    res[k][leg].append((ms, ok, launches))
        for k in decs:
            def tok_s(leg):
                return [leg[1] * n / ms * 1e3 for ms, _, _ in res[k][leg]]

            def spread(leg):
                return max(tok_s(leg)) - min(tok_s(leg))

            def step_ms(leg):
                return [ms / n for ms, _, _ in res[k][leg]]

            for leg in legs:
                kind, B, form = leg
                emit({"leg": kind, "dtype": k, "rows": B, "attention": form, "steps": n, "n_layers": base.n_layers,
                      "launches_per_step": res[k][leg][0][2], "tokens_ok": all(ok for _, ok, _ in res[k][leg]),
                      "ms_per_step": round(min(step_ms(leg)), 4), "ms_per_step_all": [round(x, 4) for x in step_ms(leg)],
                      "tok_s": round(max(tok_s(leg)), 1), "tok_s_all": [round(x, 1) for x in tok_s(leg)],
                      "spread_tok_s": round(spread(leg), 1)})
            plain = ("plain", 1, "")
            best4 = max((("batch", 4, f) for f in FORMS), key=lambda l: max(tok_s(l)))
            sp = max(spread(plain), spread(best4))
            emit({"leg": "claim1", "dtype": k, "batch4_form": best4[2],
                  "batch4_minus_plain_tok_s": round(max(tok_s(best4)) - max(tok_s(plain)), 1),
                  "repeat_spread_tok_s": round(sp, 1), "holds": bool(max(tok_s(best4)) - max(tok_s(plain)) > sp)})
            for B in (2, 3, 4):
                s = ("spec", B, "")
                for f in FORMS:
                    bl = ("batch", B, f)
                    sp_ms = max(max(step_ms(s)) - min(step_ms(s)), max(step_ms(bl)) - min(step_ms(bl)))
                    d = min(step_ms(bl)) - min(step_ms(s))
                    emit({"leg": "claim2", "dtype": k, "rows": B, "attention": f, "batch_minus_spec_ms_per_step": round(d, 4),
                          "repeat_spread_ms": round(sp_ms, 4), "holds": bool(d <= sp_ms)})
                one, per = ("batch", B, "one"), ("batch", B, "per_seq")
                sp_ms = max(max(step_ms(one)) - min(step_ms(one)), max(step_ms(per)) - min(step_ms(per)))
                d = min(step_ms(per)) - min(step_ms(one))
                emit({"leg": "claim3", "dtype": k, "rows": B, "per_seq_minus_one_ms_per_step": round(d, 4),
                      "repeat_spread_ms": round(sp_ms, 4), "one_launch_faster_beyond_spread": bool(d > sp_ms),
                      "per_seq_faster_beyond_spread": bool(-d > sp_ms)})
    finally:
        for b in batches.values():
            b.close()
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
