#!/usr/bin/env python3
"""e4m3 against fp8 (E5M2): decode step, per-launch times and prefill, in one process.

Builds synthetic Mistral-7B-shaped models in fp8 (E5M2) and e4m3 in HBM (yalm_synth /
yalm_synth_e4m3) and, after the same hydrated 13-token prompt, times the device greedy loop of
each at `--steps` 20 and 256, the formats in alternation, `--reps` times each: ms/step, tok/s
and the fraction of the format's own weight + KV bytes/token roofline at 8 TB/s (the best rep;
every rep is listed, so the spread is on the page). Then yalm_time_kernel ids 0, 2 or -- where
the decoder fuses attention and Wo -- 8, 3, 4, 5 (QKV, Wo / attention + Wo, W1|W3 + GLU, W2,
logits) for both formats, and the 13- and 4096-position prefill times (both run the f16 MFMA
path over a per-layer exact upcast).

The E5M2 leg is the yardstick. `bar`: e4m3's ms/step may exceed E5M2's by the larger repeat
spread (max - min) of the two legs plus the format's extra bytes (16 per row), as a fraction of
E5M2's ms/step.

Prints one JSON line per measurement; --out appends them to a file.

Usage: python tools/bench_e4m3.py [--reps 3] [--layers N] [--no-prefill] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # bench.py: HBM3E 8.0 TB/s spec
PROMPT_LEN = 13


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--layers", type=int, default=0, help="fewer layers = a smaller model of the same shapes")
    ap.add_argument("--kernel-iters", type=int, default=200)
    ap.add_argument("--no-prefill", action="store_true")
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
    fmts = {"fp8": M.F8E5M2, "e4m3": M.E4M3}
    cfgs = {k: base.with_(weight_dtype=v) for k, v in fmts.items()}
    dms = {k: runtime.DeviceModel.synthetic(c, seed=1) for k, c in cfgs.items()}
    decs = {k: runtime.Decoder(dm) for k, dm in dms.items()}
    prompt = [(7 * i + 1) % base.vocab_size for i in range(PROMPT_LEN)]  # bench.py's prompt
    tok0, pos0 = prompt[-1], PROMPT_LEN - 1
    try:
        for dec in decs.values():
            for pos, t in enumerate(prompt[:-1]):
                dec.forward(t, pos, runtime.HYDRATE_KV_CACHE)
            dec.generate_greedy(tok0, pos0, 16)  # warm-up
        for steps in (20, 256):
            ms = {k: [] for k in decs}
            for _ in range(args.reps):
                for k, dec in decs.items():
                    t0 = time.perf_counter()
                    dec.generate_greedy(tok0, pos0, steps)
                    ms[k].append((time.perf_counter() - t0) / steps * 1e3)
            bpt = {}
            for k, v in ms.items():
                c = cfgs[k]
                bpt[k] = c.weight_bytes_per_token() + c.kv_bytes_per_token(pos0 + 1 + steps // 2)
                best = min(v)
                emit({"leg": "greedy", "dtype": k, "steps": steps, "n_layers": c.n_layers,
                      "ms_per_step": round(best, 4), "ms_per_step_all": [round(x, 4) for x in v],
                      "spread_ms": round(max(v) - min(v), 4), "tok_s": round(1e3 / best, 1),
                      "bytes_per_token": bpt[k], "roofline_frac": round(bpt[k] / (best * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                      "kernels_per_token": decs[k].graph_kernels(2), "attn_wo": bool(decs[k].attn_wo)})
            e, f = ms["e4m3"], ms["fp8"]
            gap, spread = min(e) - min(f), max(max(e) - min(e), max(f) - min(f))
            extra = (bpt["e4m3"] / bpt["fp8"] - 1.0) * min(f)
            emit({"leg": "bar", "steps": steps, "e4m3_minus_fp8_ms": round(gap, 4), "repeat_spread_ms": round(spread, 4),
                  "extra_bytes_ms": round(extra, 4), "allowed_ms": round(spread + extra, 4),
                  "e4m3_at_fp8_speed": bool(gap <= spread + extra)})
        fused = all(d.attn_wo for d in decs.values())
        kernels = {0: "qkv", (8 if fused else 2): "attn_wo" if fused else "wo", 3: "w1w3_glu", 4: "w2", 5: "logits"}
        for kid, kname in kernels.items():
            rec = {"leg": "kernel", "id": kid, "kernel": kname}
            for k, dec in decs.items():
                c = cfgs[k]
                rows_n = {0: (c.q_dim + 2 * c.kv_dim, c.dim), 2: (c.dim, c.q_dim), 8: (c.dim, c.q_dim),
                          3: (2 * c.hidden_dim, c.dim), 4: (c.dim, c.hidden_dim), 5: (c.vocab_size, c.dim)}[kid]
                nbytes = rows_n[0] * M.row_bytes(c.weight_dtype, rows_n[1])
                us = [dec.time_kernel(kid, args.kernel_iters) * 1e3 for _ in range(args.reps)]
                rec[k] = {"us": round(min(us), 2), "us_all": [round(x, 2) for x in us],
                          "gbs": round(nbytes / (min(us) * 1e-6) / 1e9, 1)}
            rec["name_e4m3"] = decs["e4m3"].kernel_name(kid)
            emit(rec)
        if not args.no_prefill:
            for n in (13, 4096):
                rec = {"leg": "prefill", "positions": n}
                for k, dec in decs.items():
                    dec.prefill_time(n, 1)
                    ms = [dec.prefill_time(n, 2) for _ in range(args.reps)]
                    rec[k] = {"ms": round(min(ms), 3), "ms_all": [round(x, 3) for x in ms]}
                emit(rec)
    finally:
        for d in decs.values():
            d.close()
        for d in dms.values():
            d.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
