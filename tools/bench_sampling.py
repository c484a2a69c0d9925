#!/usr/bin/env python3
"""Device sampling benchmark: what a sampled token costs against a greedy one.

Builds a synthetic fp16 model in HBM (yalm_synth) at Mistral-7B (vocabulary 32000) and
Llama-3.2-3B (vocabulary 128256) shapes and times, from the same position after the same
hydrated prompt, `--reps` times each in alternation inside one process:

  greedy        yalm_generate_greedy, `--steps` tokens in one call (the device loop)
  sampled       yalm_generate_sampled, temperature 1, no truncation, one call
  sampled_kp    the same with top_k = 40, top_p = 0.9
  step_sampled  `--steps` one-step yalm_generate_sampled calls: what the CLI does with -k / -p
  step_logits   `--steps` one-step yalm_forward calls with the logits copied to the host: what
                the CLI does without them, before its host softmax passes (not timed here)

Every figure is wall time of calls that end in a stream synchronise, divided by the steps;
the best of the reps is reported beside all of them. kernel_us is yalm_time_kernel id 10, the
sampling launch alone on the decoder's logits, for both parameter sets. The argmax launch
has no timing id: sampled - greedy, from the same run, is the difference a user sees.

Prints one JSON line per model; --out appends them to a file.

Usage: python tools/bench_sampling.py [--steps 128] [--reps 3] [--layers N] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PROMPT_LEN = 16
TOP_K, TOP_P = 40, 0.9


def run_model(runtime, name, cfg, args):
    dm = runtime.DeviceModel.synthetic(cfg, seed=1)
    dec = runtime.Decoder(dm)
    n = args.steps
    u = np.random.default_rng(1).random(n, dtype=np.float32)
    prompt = [(7 * i + 1) % cfg.vocab_size for i in range(PROMPT_LEN)]
    tok0, pos0 = prompt[-1], PROMPT_LEN - 1
    try:
        for pos, t in enumerate(prompt[:-1]):
            dec.forward(t, pos, runtime.HYDRATE_KV_CACHE)
        fed = dec.generate_sampled(tok0, pos0, n, 1.0, uniforms=u)  # warm-up, and the tokens step_logits feeds
        dec.generate_greedy(tok0, pos0, args.warmup)
        dec.forward(tok0, pos0)

        def step_sampled():
            t = tok0
            for i in range(n):
                t = dec.generate_sampled(t, pos0 + i, 1, 1.0, TOP_K, TOP_P, uniforms=u[i:i + 1])[0]

        def step_logits():
            t = tok0
            for i in range(n):
                dec.forward(t, pos0 + i)
                t = fed[i]

        legs = {
            "greedy": lambda: dec.generate_greedy(tok0, pos0, n),
            "sampled": lambda: dec.generate_sampled(tok0, pos0, n, 1.0, uniforms=u),
            "sampled_kp": lambda: dec.generate_sampled(tok0, pos0, n, 1.0, TOP_K, TOP_P, uniforms=u),
            "step_sampled": step_sampled,
            "step_logits": step_logits,
        }
        ms = {k: [] for k in legs}
        for _ in range(args.reps):
            for k, f in legs.items():
                t0 = time.perf_counter()
                f()
                ms[k].append((time.perf_counter() - t0) / n * 1e3)
        kern = {}
        dec.generate_sampled(tok0, pos0, 1, 1.0, uniforms=u[:1])
        kern["sampled"] = round(dec.time_kernel(10, args.kernel_iters) * 1e3, 2)
        dec.generate_sampled(tok0, pos0, 1, 1.0, TOP_K, TOP_P, uniforms=u[:1])
        kern["sampled_kp"] = round(dec.time_kernel(10, args.kernel_iters) * 1e3, 2)
        best = {k: min(v) for k, v in ms.items()}
        return {
            "model": name, "dtype": "fp16", "n_layers": cfg.n_layers, "vocab_size": cfg.vocab_size,
            "steps": n, "reps": args.reps, "top_k": TOP_K, "top_p": TOP_P,
            "ms_per_token": {k: round(v, 4) for k, v in best.items()},
            "ms_per_token_all": {k: [round(x, 4) for x in v] for k, v in ms.items()},
            "sampled_over_greedy": round(best["sampled"] / best["greedy"], 4),
            "sampled_kp_over_greedy": round(best["sampled_kp"] / best["greedy"], 4),
            "sampled_minus_greedy_us": round((best["sampled"] - best["greedy"]) * 1e3, 2),
            "sampled_kp_minus_greedy_us": round((best["sampled_kp"] - best["greedy"]) * 1e3, 2),
            "step_sampled_minus_step_logits_us": round((best["step_sampled"] - best["step_logits"]) * 1e3, 2),
            "logits_bytes_per_token": 4 * cfg.vocab_size,
            "kernel_us": kern, "kernel_name": dec.kernel_name(10),
            "kernels_per_token": [dec.graph_kernels(2), dec.graph_kernels(3)],
        }
    finally:
        dec.close()
        dm.close()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--layers", type=int, default=0, help="fewer layers = a smaller model of the same shapes")
    ap.add_argument("--kernel-iters", type=int, default=200)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)

    from yalm_amd import models as M
    from yalm_amd import runtime

    runtime.check(runtime.lib.yalm_set_device(0))
    lines = []
    for name, cfg in (("mistral-7b", M.MISTRAL_7B), ("llama-3.2-3b", M.LLAMA_32_3B)):
        if args.layers:
            cfg = cfg.with_(n_layers=args.layers)
        lines.append(json.dumps(run_model(runtime, name, cfg, args)))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
