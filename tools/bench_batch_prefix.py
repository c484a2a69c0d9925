#!/usr/bin/env python3
"""Batched decode with the prompt shared (yalm_batch_share_prefix) against the prompt copied into
every sequence (yalm_batch_load), fp16 and fp8, in one process.

Builds synthetic Mistral-7B-shaped fp16 and fp8 models in HBM. For every prompt length of
`--prompt-len` (default 13, 1024, 4096) the decoder is hydrated with that prompt by the batched
prefill, and a batch of `--seqs` sequences (default 4) runs `--steps` greedy steps from the prompt's
last token, `--reps` times in each form, the forms in alternation, every rep listed:

  loaded   the prompt's rows copied into every sequence, one attention launch per layer
  shared   the prompt's rows read where they are: the two launches of csrc/batch_prefix.h

Reports ms per step per form and the claim "the shared step is shorter than the loaded step of the
same run by more than the repeat spread of either" per (dtype, prompt length), with both numbers.
tokens_equal says whether the two forms produced the same greedy tokens (they may part where the
model's top-two margin is inside the attention's rounding; a synthetic model's margins are small).

Every leg runs under the tool's own time limit (--leg-timeout seconds: the process is ended by
SIGALRM if a leg does not return). Prints one JSON line per measurement; --out appends them.

Usage: python tools/bench_batch_prefix.py [--prompt-len 13 1024 4096] [--seqs 4] [--reps 3]
                                          [--steps 32] [--layers N] [--out FILE]
"""
import argparse
import json
import os
import signal
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--prompt-len", type=int, nargs="+", default=[13, 1024, 4096])
    ap.add_argument("--seqs", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--layers", type=int, default=0, help="fewer layers = a smaller model of the same shapes")
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

    B, n = args.seqs, args.steps
    base = M.MISTRAL_7B.with_(max_seq_len=max(args.prompt_len) + n + 64)
    if args.layers:
        base = base.with_(n_layers=args.layers)
    for k, wd in (("fp16", M.F16), ("fp8", M.F8E5M2)):
        dm = runtime.DeviceModel.synthetic(base.with_(weight_dtype=wd), seed=1)
        dec = runtime.Decoder(dm)
        loaded, shared = runtime.Batch(dec, B), runtime.Batch(dec, B)
        try:
            for plen in args.prompt_len:
                prompt = [(7 * i + 1) % base.vocab_size for i in range(plen)]  # bench.py's prompt, continued
                tok0, pos0 = prompt[-1], plen - 1
                timed(lambda: dec.prefill(prompt[:-1], 0))
                loaded.load(pos0)
                shared.share_prefix(pos0)
                forms = {"loaded": loaded, "shared": shared}
                for b in forms.values():  # warm-up
                    timed(lambda: b.generate_greedy([tok0] * B, [pos0] * B, 4))
                ms, toks, launches = {f: [] for f in forms}, {}, {}
                for _ in range(args.reps):
                    for f, b in forms.items():
                        (t, st), dt = timed(lambda: b.generate_greedy([tok0] * B, [pos0] * B, n))
                        ms[f].append(dt / n)
                        toks[f], launches[f] = t, st["launches_per_step"]
                for f in forms:
                    emit({"leg": f, "dtype": k, "prompt_len": plen, "seqs": B, "steps": n, "n_layers": base.n_layers,
                          "launches_per_step": launches[f], "ms_per_step": round(min(ms[f]), 4),
                          "ms_per_step_all": [round(x, 4) for x in ms[f]]})
                spread = max(max(v) - min(v) for v in ms.values())
                gain = min(ms["loaded"]) - min(ms["shared"])
                emit({"leg": "claim", "dtype": k, "prompt_len": plen, "loaded_minus_shared_ms_per_step": round(gain, 4),
                      "repeat_spread_ms": round(spread, 4), "shared_shorter_beyond_spread": bool(gain > spread),
                      "tokens_equal": bool((toks["loaded"] == toks["shared"]).all())})
        finally:
            loaded.close()
            shared.close()
            dec.close()
            dm.close()
    if args.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
