#!/usr/bin/env python3
"""Mixture-of-experts decode benchmark: a synthetic Mixtral-8x7B-shaped fp16 model (built in
HBM by yalm_synth, ~93 GB) against a dense twin in the same process -- Mistral-7B dims with
hidden_dim = 2 x 14336, which streams the same FFN bytes per token through the dense kernels.

Both run bench.py's timed loop (prompt hydrated, warm-up, then `--steps` device-greedy tokens
enqueued back to back between syncs), `--reps` times each, and report tok/s, ms/step, the
bytes/token roofline fraction and the per-kernel times of yalm_time_kernel (3 = W1|W3 + GLU,
4 = W2, 9 = the router). The comparison the design asks for:

    moe_ms_per_step - n_layers x router_ms   vs   twin_ms_per_step (+- the twin's own spread)

Prints one JSON line per model and one for the comparison; --out appends them to a file.

--prefill N (repeatable) measures the batched prefill instead: yalm_prefill_time of N positions
on the expert model and on the dense twin (same FFN FLOPs per token), fast and split-operand
forms, and -- in the same process -- N per-position hydration forwards on the expert decoder,
the path these models took before the grouped expert prefill.

Usage: python tools/bench_moe.py [--steps 128] [--warmup 16] [--reps 3] [--layers 32] [--out FILE]
       python tools/bench_moe.py --prefill 4096 --prefill 13 [--layers 32] [--prefill-iters 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PROMPT_LEN = 16
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E peak, the denominator bench.py's roofline uses


def timed_decode(runtime, dec, cfg, steps, warmup):
    """bench.py's loop: seconds for exactly `steps` greedy tokens enqueued back to back."""
    prompt = [(7 * i + 1) % cfg.vocab_size for i in range(PROMPT_LEN)]
    for pos, t in enumerate(prompt[:-1]):
        dec.forward(t, pos, runtime.HYDRATE_KV_CACHE)
    dec.generate_greedy(prompt[-1], PROMPT_LEN - 1, 1)
    if warmup:
        dec.enqueue_greedy(warmup)
    _, pos0 = dec.device_step()
    t0 = time.perf_counter()
    dec.enqueue_greedy(steps)
    dec.device_step()
    el = time.perf_counter() - t0
    _, pos1 = dec.device_step()
    assert pos1 - pos0 == steps, (pos0, pos1)
    return el


def run_model(runtime, name, cfg, args, kernel_ids):
    dm = runtime.DeviceModel.synthetic(cfg, seed=1)
    dec = runtime.Decoder(dm)
    try:
        secs = [timed_decode(runtime, dec, cfg, args.steps, args.warmup) for _ in range(args.reps)]
        ms = sorted(s / args.steps * 1e3 for s in secs)
        best = ms[0]
        kv_len = PROMPT_LEN + args.warmup + args.steps // 2
        bytes_tok = cfg.weight_bytes_per_token() + cfg.kv_bytes_per_token(kv_len)
        kern = {str(k): round(dec.time_kernel(k, args.kernel_iters) * 1e3, 3) for k in kernel_ids}
        names = {str(k): dec.kernel_name(k) for k in kernel_ids}
        return {
            "model": name, "dtype": "fp16", "n_layers": cfg.n_layers, "n_experts": cfg.n_experts,
            "n_experts_active": cfg.n_experts_active, "hidden_dim": cfg.hidden_dim,
            "model_gb": round(runtime.M.nbytes_model(cfg) / 1e9, 2),
            "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(best, 4), "ms_per_step_all": [round(m, 4) for m in ms],
            "spread_ms": round(ms[-1] - ms[0], 4), "tok_s": round(1e3 / best, 2),
            "bytes_per_token": bytes_tok, "gbs": round(bytes_tok / best / 1e6, 1),
            "roofline_frac": round(bytes_tok / best / 1e6 / HBM_PEAK_GBS, 4),
            "kernel_us": kern, "kernel_names": names, "kernels_per_token": dec.graph_kernels(2),
            "attn_wo_fused": dec.attn_wo,
        }
    finally:
        dec.close()
        dm.close()


def prefill_model(runtime, name, cfg, args):
    """yalm_prefill_time per N in both precision forms; expert models: N per-position forwards too."""
    dm = runtime.DeviceModel.synthetic(cfg, seed=1)
    dec = runtime.Decoder(dm)
    out = []
    try:
        for n in args.prefill:
            row = {"model": name, "prefill_n": n, "n_layers": cfg.n_layers, "n_experts": cfg.n_experts,
                   "n_experts_active": cfg.n_experts_active, "hidden_dim": cfg.hidden_dim}
            for form, mode in (("fast", runtime.PREFILL_FAST), ("split", runtime.PREFILL_SPLIT)):
                dec.set_prefill_precision(mode)
                ms = sorted(dec.prefill_time(n, args.prefill_iters) for _ in range(args.reps))
                row[f"{form}_ms"] = round(ms[0], 3)
                row[f"{form}_ms_all"] = [round(m, 3) for m in ms]
            dec.set_prefill_precision(runtime.PREFILL_FAST)
            # FFN GEMM FLOPs per pass (W1, W3, W2 of the active experts / of the twin's one FFN)
            k = max(cfg.n_experts_active, 1)
            row["ffn_tflop"] = round(6.0 * n * k * cfg.hidden_dim * cfg.dim * cfg.n_layers / 1e12, 3)
            if cfg.n_experts > 0 and not args.skip_per_position:
                dec.forward(1, 0, runtime.HYDRATE_KV_CACHE)  # warm-up (graph capture)
                runtime.check(runtime.lib.yalm_stream_sync(None))
                t0 = time.perf_counter()
                for pos in range(n - 1):
                    dec.forward((7 * pos + 1) % cfg.vocab_size, pos, runtime.HYDRATE_KV_CACHE)
                dec.forward(3, n - 1)  # the last one with logits: its copy-back waits for them all
                row["per_position_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
                row["per_position_over_fast"] = round(row["per_position_ms"] / row["fast_ms"], 2)
            out.append(row)
        return out
    finally:
        dec.close()
        dm.close()


def main_prefill(runtime, M, args):
    moe_cfg = M.MIXTRAL_8X7B.with_(n_layers=args.layers)
    twin_cfg = M.MISTRAL_7B.with_(n_layers=args.layers, hidden_dim=moe_cfg.n_experts_active * moe_cfg.hidden_dim)
    moe = prefill_model(runtime, "mixtral-8x7b", moe_cfg, args)
    twin = prefill_model(runtime, "dense-twin", twin_cfg, args)
    rows = moe + twin
    for m, t in zip(moe, twin):
        rows.append({"compare": "moe_prefill_vs_twin", "prefill_n": m["prefill_n"],
                     "fast_ms_moe_vs_twin": [m["fast_ms"], t["fast_ms"]],
                     "fast_ratio": round(m["fast_ms"] / t["fast_ms"], 4),
                     "split_ms_moe_vs_twin": [m["split_ms"], t["split_ms"]],
                     "split_ratio": round(m["split_ms"] / t["split_ms"], 4),
                     "per_position_ms": m.get("per_position_ms"),
                     "per_position_over_fast": m.get("per_position_over_fast")})
    return [json.dumps(x) for x in rows]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--layers", type=int, default=32, help="fewer layers = a smaller model of the same shapes")
    ap.add_argument("--kernel-iters", type=int, default=64)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--prefill", type=int, action="append", default=None,
                    help="measure the batched prefill of N positions instead of decode (repeatable)")
    ap.add_argument("--prefill-iters", type=int, default=3)
    ap.add_argument("--skip-per-position", action="store_true",
                    help="--prefill: leave out the per-position forwards (kernel-stats runs under a profiler: "
                         "the per-token graph replay is not what they measure)")
    args = ap.parse_args(argv)

    from yalm_amd import models as M
    from yalm_amd import runtime

    runtime.M = M
    runtime.check(runtime.lib.yalm_set_device(0))
    if args.prefill:
        lines = main_prefill(runtime, M, args)
        for l in lines:
            print(l, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write("\n".join(lines) + "\n")
        return
    moe_cfg = M.MIXTRAL_8X7B.with_(n_layers=args.layers)
    twin_cfg = M.MISTRAL_7B.with_(n_layers=args.layers, hidden_dim=moe_cfg.n_experts_active * moe_cfg.hidden_dim)
    moe = run_model(runtime, "mixtral-8x7b", moe_cfg, args, (3, 4, 9))
    twin = run_model(runtime, "dense-twin", twin_cfg, args, (3, 4))
    router_ms = moe["kernel_us"]["9"] * 1e-3
    net = moe["ms_per_step"] - moe_cfg.n_layers * router_ms
    cmp_ = {
        "compare": "moe_minus_router_vs_twin", "router_us": moe["kernel_us"]["9"],
        "moe_ms_per_step": moe["ms_per_step"], "moe_minus_router_ms": round(net, 4),
        "twin_ms_per_step": twin["ms_per_step"], "twin_spread_ms": twin["spread_ms"],
        "ratio": round(net / twin["ms_per_step"], 4),
        "within_twin_spread": bool(abs(net - twin["ms_per_step"]) <= twin["spread_ms"]),
        "glu_us_moe_vs_twin": [moe["kernel_us"]["3"], twin["kernel_us"]["3"]],
        "w2_us_moe_vs_twin": [moe["kernel_us"]["4"], twin["kernel_us"]["4"]],
    }
    lines = [json.dumps(x) for x in (moe, twin, cmp_)]
    for l in lines:
        print(l, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
