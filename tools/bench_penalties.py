#!/usr/bin/env python3
"""Penalised device sampling benchmark: what repetition / frequency / presence penalties and
min-p cost against the plain device sampler of the same run.

Builds a synthetic fp16 model in HBM at Mistral-7B (vocabulary 32000) and Llama-3.2-3B
(vocabulary 128256) shapes, as tools/bench_sampling.py does, and measures in one process:

  kernel_us     the sampling launch alone on the decoder's logits, `--reps` times each in
                alternation: yalm_time_kernel id 10 (plain) and id 15 (penalised) with a window
                of 64 and of 1024 tokens over a context of 1024 tokens, for no truncation and
                for top_k = 40, top_p = 0.9
  ms_per_token  yalm_generate_sampled against yalm_generate_sampled_ex (window 64 and 1024),
                `--steps` tokens in one call each, alternated `--reps` times: wall time of calls
                that end in a stream synchronise, divided by the steps

Every repeat is listed beside the best. Prints one JSON line per model; --out appends them.

Usage: python tools/bench_penalties.py [--steps 128] [--reps 5] [--layers N] [--out FILE]
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
PEN = dict(repetition=1.2, frequency=0.2, presence=0.1, min_p=0.05)
WINDOWS = (64, 1024)


def run_model(runtime, name, cfg, args):
    dm = runtime.DeviceModel.synthetic(cfg, seed=1)
    dec = runtime.Decoder(dm)
    n = args.steps
    u = np.random.default_rng(1).random(n, dtype=np.float32)
    prompt = [(7 * i + 1) % cfg.vocab_size for i in range(PROMPT_LEN)]
    tok0, pos0 = prompt[-1], PROMPT_LEN - 1
    # 1024 context tokens, every one twice: the window is full from the first step, 512 logits are patched
    ctx = np.tile(np.random.default_rng(2).integers(0, cfg.vocab_size, 512), 2)
    try:
        for pos, t in enumerate(prompt[:-1]):
            dec.forward(t, pos, runtime.HYDRATE_KV_CACHE)
        dec.generate_sampled(tok0, pos0, args.warmup, 1.0, uniforms=u)
        dec.forward(tok0, pos0)

        def plain(k, p, steps=n):
            return dec.generate_sampled(tok0, pos0, steps, 1.0, k, p, uniforms=u)

        def pen(w, k, p, steps=n):
            return dec.generate_sampled(tok0, pos0, steps, 1.0, k, p, uniforms=u, penalties=dict(PEN, window=w),
                                        context=ctx)

        legs = {"sampled_kp": lambda: plain(TOP_K, TOP_P)}
        for w in WINDOWS:
            legs[f"penalised_kp_w{w}"] = lambda w=w: pen(w, TOP_K, TOP_P)
        ms = {k: [] for k in legs}
        for _ in range(args.reps):
            for k, f in legs.items():
                t0 = time.perf_counter()
                f()
                ms[k].append((time.perf_counter() - t0) / n * 1e3)
        # the launch alone: each timed on the logits of the same one-step call's forward
        kern = {}
        for _ in range(args.reps):
            for tag, (k, p) in (("", (0, 1.0)), ("_kp", (TOP_K, TOP_P))):
                plain(k, p, 1)
                kern.setdefault("sampled" + tag, []).append(round(dec.time_kernel(10, args.kernel_iters) * 1e3, 2))
                for w in WINDOWS:
                    pen(w, k, p, 1)
                    kern.setdefault(f"penalised{tag}_w{w}", []).append(
                        round(dec.time_kernel(15, args.kernel_iters) * 1e3, 2))
        best = {k: min(v) for k, v in ms.items()}
        kbest = {k: min(v) for k, v in kern.items()}
        return {
            "model": name, "dtype": "fp16", "n_layers": cfg.n_layers, "vocab_size": cfg.vocab_size, "steps": n,
            "reps": args.reps, "top_k": TOP_K, "top_p": TOP_P, "penalties": PEN, "context": int(ctx.size),
            "ms_per_token": {k: round(v, 4) for k, v in best.items()},
            "ms_per_token_all": {k: [round(x, 4) for x in v] for k, v in ms.items()},
            "penalised_minus_sampled_us": {f"w{w}": round((best[f"penalised_kp_w{w}"] - best["sampled_kp"]) * 1e3, 2)
                                           for w in WINDOWS},
            "kernel_us": kbest, "kernel_us_all": kern,
            "kernel_names": [dec.kernel_name(10), dec.kernel_name(15)],
            "kernels_per_token": [dec.graph_kernels(3), dec.graph_kernels(4)],
        }
    finally:
        dec.close()
        dm.close()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
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
