#!/usr/bin/env python3
"""What the q / k norm (Qwen3) costs: its one extra launch per layer.

Legs (one JSON line per measurement; --out appends them to a file):

  launch    yalm_time_kernel id 11 (qk_norm_rope_kernel) alone at the Qwen3-8B shape (40 waves:
            32 q heads + 8 k heads of head_dim 128), fp16 weights, `--reps` repeats, all listed.
  decode    a synthetic Qwen3-8B-shaped model (models.QWEN3_8B) in fp16, fp8 and q4: greedy
            ms/step at 20 steps with the norm on and with it removed on the SAME decoder
            (yalm_decoder_set_qk_norm), legs alternated, best of `--reps`, every repeat listed;
            the difference per layer; tok/s and the fraction of each format's own weight + KV
            bytes/token roofline at 8 TB/s with the norm on; kernels per token, which kernel the
            QKV launch runs and whether attention + Wo fuse.

  prefill   Llama-3.2-3B shape with the norm weights added, 4096 positions, the norm on and off in
            alternation on one decoder (yalm_prefill_time): with it the QKV GEMM stores raw f32 rows
            and a row kernel norms, rotates and stores.

Usage: python tools/bench_qknorm.py [--legs launch,decode,prefill] [--reps 3] [--out FILE]
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
    ap.add_argument("--legs", type=str, default="launch,decode,prefill")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-iters", type=int, default=400)
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)

    from yalm_amd import models as M
    from yalm_amd import runtime

    runtime.check(runtime.lib.yalm_set_device(0))
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    base = M.QWEN3_8B
    prompt = [(7 * i + 1) % base.vocab_size for i in range(PROMPT_LEN)]
    tok0, pos0, steps = prompt[-1], PROMPT_LEN - 1, 20
    for name, dt in (("fp16", M.F16), ("fp8", M.F8E5M2), ("q4", M.Q4)):
        legs = [l for l in args.legs.split(",") if l == "decode" or (l == "launch" and name == "fp16")]
        if not legs:
            continue
        cfg = base.with_(weight_dtype=dt)
        dm = runtime.DeviceModel.synthetic(cfg, seed=1)
        dec = runtime.Decoder(dm)
        try:
            for pos, t in enumerate(prompt[:-1]):
                dec.forward(t, pos, runtime.HYDRATE_KV_CACHE)
            if "launch" in legs:
                dec.time_kernel(11, 50)
                us = [round(dec.time_kernel(11, args.kernel_iters) * 1e3, 3) for _ in range(args.reps)]
                emit({"leg": "launch", "shape": "qwen3-8b", "kernel": dec.kernel_name(11) + " (id 11)",
                      "waves": cfg.n_heads + cfg.n_kv_heads, "us": min(us), "us_all": us,
                      "spread_us": round(max(us) - min(us), 3)})
            if "decode" in legs:
                ms = {"norm": [], "plain": []}
                info = {}
                for _ in range(args.reps):
                    for state in ms:
                        dec.set_qk_norm(state == "norm")
                        dec.generate_greedy(tok0, pos0, 8)  # graphs re-captured, caches warm
                        t0 = time.perf_counter()
                        dec.generate_greedy(tok0, pos0, steps)
                        ms[state].append(round((time.perf_counter() - t0) / steps * 1e3, 4))
                        info[state] = (dec.graph_kernels(2), dec.kernel_name(0))
                bpt = cfg.weight_bytes_per_token() + cfg.kv_bytes_per_token(pos0 + 1 + steps // 2)
                best = {k: min(v) for k, v in ms.items()}
                emit({"leg": "decode", "shape": "qwen3-8b", "dtype": name, "steps": steps,
                      "norm": {"ms_per_step": best["norm"], "ms_per_step_all": ms["norm"],
                               "kernels_per_token": info["norm"][0], "qkv_kernel": info["norm"][1]},
                      "plain": {"ms_per_step": best["plain"], "ms_per_step_all": ms["plain"],
                                "kernels_per_token": info["plain"][0], "qkv_kernel": info["plain"][1]},
                      "norm_minus_plain_us_per_layer": round((best["norm"] - best["plain"]) * 1e3 / cfg.n_layers, 3),
                      "spread_us_per_layer": round(max(max(v) - min(v) for v in ms.values()) * 1e3 / cfg.n_layers, 3),
                      "tok_s": round(1e3 / best["norm"], 1), "bytes_per_token": bpt,
                      "roofline_frac": round(bpt / (best["norm"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                      "attn_wo_fused": bool(dec.attn_wo)})
        finally:
            dec.close()
            dm.close()
    if "prefill" in args.legs.split(","):
        cfg = M.LLAMA_32_3B.with_(qk_norm=True)
        dm = runtime.DeviceModel.synthetic(cfg, seed=1)
        dec = runtime.Decoder(dm)
        try:
            n = 4096
            dec.prefill_time(n, 1)
            ms = {"norm": [], "plain": []}
            for _ in range(args.reps):
                for state in ms:
                    dec.set_qk_norm(state == "norm")
                    ms[state].append(round(dec.prefill_time(n, 2), 3))
            emit({"leg": "prefill", "shape": "llama-3.2-3b + q / k norm", "positions": n,
                  "norm": {"ms": min(ms["norm"]), "ms_all": ms["norm"]},
                  "plain": {"ms": min(ms["plain"]), "ms_all": ms["plain"]}})
        finally:
            dec.close()
            dm.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
