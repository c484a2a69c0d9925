#!/usr/bin/env python3
"""Decode over the q8 kv shadow against the f16 KV cache, in one process.

Builds synthetic Mistral-7B-shaped models in fp16, fp8 and q4 in HBM and, per format and window
(`--windows`, 4096 and 16384), two decoders on the same weights: q8 kv off and on
(Decoder.set_kv_q8). Both prefill a whole window and decode past it, so every timed step reads a
full window with two sink rows. Then `--steps` greedy steps each, off and on in alternation,
`--reps` times: ms/step (the best rep; every rep is listed, so the spread is on the page), and the
attention launch alone through yalm_time_kernel id 1 (the f16 decoder with separate attention
and Wo launches, so that id 1 is what it would run beside a Wo launch; its step keeps the fused
launch where it has one).

`bar`: per (format, window), the q8 step below the f16-KV step by more than the spread
(max - min) of the reps of either leg.

Prints one JSON line per measurement; --out appends them to a file.

Usage: python tools/bench_kv_q8.py [--reps 3] [--steps 20] [--layers N] [--windows 4096,16384] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--layers", type=int, default=0, help="fewer layers = a smaller model of the same shapes")
    ap.add_argument("--windows", type=str, default="4096,16384")
    ap.add_argument("--formats", type=str, default="fp16,fp8,q4")
    ap.add_argument("--kernel-iters", type=int, default=200)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)

    from yalm_amd import models as M
    from yalm_amd import runtime

    runtime.check(runtime.lib.yalm_set_device(0))
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    base = M.MISTRAL_7B.with_(n_layers=args.layers) if args.layers else M.MISTRAL_7B
    fmts = {"fp16": M.F16, "fp8": M.F8E5M2, "q4": M.Q4}
    for name in args.formats.split(","):
        for window in (int(w) for w in args.windows.split(",")):
            cfg = base.with_(weight_dtype=fmts[name], max_seq_len=window)
            dm = runtime.DeviceModel.synthetic(cfg, seed=1)
            decs = {"f16kv": runtime.Decoder(dm), "q8kv": runtime.Decoder(dm)}
            try:
                decs["q8kv"].set_kv_q8(True)
                prompt = [(7 * i + 1) % cfg.vocab_size for i in range(window)]
                for dec in decs.values():
                    dec.prefill(prompt, 0, logprobs=False)
                    dec.generate_greedy(prompt[-1], window, 8)  # past the window: the sink regime; warm-up
                pos0 = window + 8
                ms = {k: [] for k in decs}
                for _ in range(args.reps):
                    for k, dec in decs.items():
                        t0 = time.perf_counter()
                        dec.generate_greedy(1, pos0, args.steps)
                        ms[k].append((time.perf_counter() - t0) / args.steps * 1e3)
                for k, v in ms.items():
                    emit({"leg": "greedy", "dtype": name, "window": window, "kv": k, "steps": args.steps,
                          "n_layers": cfg.n_layers, "ms_per_step": round(min(v), 4),
                          "ms_per_step_all": [round(x, 4) for x in v], "spread_ms": round(max(v) - min(v), 4),
                          "attn_wo_fused": decs[k].attn_wo, "kernels_per_token": decs[k].graph_kernels(2)})
                f, q = ms["f16kv"], ms["q8kv"]
                gap, spread = min(f) - min(q), max(max(q) - min(q), max(f) - min(f))
                emit({"leg": "bar", "dtype": name, "window": window, "f16kv_minus_q8kv_ms": round(gap, 4),
                      "repeat_spread_ms": round(spread, 4), "q8_faster_beyond_spread": bool(gap > spread)})
                decs["f16kv"].set_launch(runtime.LAUNCH_SEPARATE_ATTN_WO)
                rec = {"leg": "kernel", "id": 1, "dtype": name, "window": window}
                for k, dec in decs.items():
                    dec.forward(1, pos0, runtime.HYDRATE_KV_CACHE)  # the step state of a full window
                    us = [dec.time_kernel(1, args.kernel_iters) * 1e3 for _ in range(args.reps)]
                    rec[k] = {"us": round(min(us), 2), "us_all": [round(x, 2) for x in us], "name": dec.kernel_name(1)}
                emit(rec)
            finally:
                for d in decs.values():
                    d.close()
                dm.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
