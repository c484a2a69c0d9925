#!/usr/bin/env python3
"""What the q / k / v bias (Qwen2) and the llama3 RoPE scaling (Llama-3.1 / 3.2) cost.

Legs (one JSON line per measurement; --out appends them to a file):

  bias      yalm_time_kernel id 0 (the QKV launch) at the Mistral-7B shape, fp16 and fp8, one
            decoder per format with the bias switched on and off in alternation, `--reps`
            times each, every repeat listed. With --parent-lib (a build of the parent commit,
            tools/build_ab_lib.sh), a child process times the same unbiased launch on that
            library in the same session.
  qwen      a synthetic Qwen2.5-7B-shaped model (dim 3584, 28 heads, 4 kv heads, head_dim 128,
            hidden 18944, 28 layers, vocabulary 152064, bias on) in fp16, fp8 and q4: greedy
            ms/step at 20 steps (best of `--reps`, all listed), the fraction of each format's
            own weight + KV bytes/token roofline at 8 TB/s, the per-kernel times, which GEMV
            kernel each launch runs (3584 is a whole number of fp16 chunks of 512 elements but
            not of fp8's 1024 or q4's 2048) and whether attention + Wo fuse.
  prefill   Llama-3.2-3B shape, 4096 positions, the scaling on and off in alternation (only the
            table's values change), and the parent library's time with --parent-lib.

Usage: python tools/bench_arch.py [--legs bias,qwen,prefill] [--reps 3] [--parent-lib PATH] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # bench.py: HBM3E 8.0 TB/s spec
PROMPT_LEN = 13
KERNELS = {0: "qkv", 1: "attention", 2: "wo", 3: "w1w3_glu", 4: "w2", 5: "logits"}
LLAMA3_32 = ("llama3", 32.0, 1.0, 4.0, 8192)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", type=str, default="bias,qwen,prefill")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-iters", type=int, default=200)
    ap.add_argument("--parent-lib", type=str, default=None)
    ap.add_argument("--child", type=str, default=None, help="internal: the parent library's part of a leg")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args(argv)

    from yalm_amd import models as M
    from yalm_amd import runtime

    runtime.check(runtime.lib.yalm_set_device(0))
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    def parent(leg):
        """The parent library's figures, from a fresh process that loads it (YALM_LIB)."""
        if not args.parent_lib:
            return
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, "--reps", str(args.reps),
                            "--kernel-iters", str(args.kernel_iters)], capture_output=True, text=True,
                           env=dict(os.environ, YALM_LIB=os.path.abspath(args.parent_lib)), timeout=600)
        if r.returncode != 0:
            raise RuntimeError(r.stderr[-2000:])
        for ln in r.stdout.splitlines():
            if ln.startswith("{"):
                emit(dict(json.loads(ln), library="parent"))

    def qkv_times(cfg, toggle):
        """yalm_time_kernel id 0 on one synthetic model: {state: [us per repeat]}, alternated."""
        dm = runtime.DeviceModel.synthetic(cfg, seed=1)
        dec = runtime.Decoder(dm)
        try:
            dec.forward(1, 0)
            us = {"plain": [], "bias": []} if toggle else {"plain": []}
            for _ in range(args.reps):
                for state in us:
                    if toggle:
                        dec.set_qkv_bias(state == "bias")
                    dec.time_kernel(0, 20)
                    us[state].append(round(dec.time_kernel(0, args.kernel_iters) * 1e3, 3))
            return us, dec.kernel_name(0)
        finally:
            dec.close()
            dm.close()

    def leg_bias(child):
        for name, dt in (("fp16", M.F16), ("fp8", M.F8E5M2)):
            cfg = M.MISTRAL_7B.with_(weight_dtype=dt) if child else M.MISTRAL_7B.with_(weight_dtype=dt, qkv_bias=True)
            us, kname = qkv_times(cfg, toggle=not child)
            rec = {"leg": "bias", "shape": "mistral-7b", "dtype": name, "kernel": "qkv (id 0)"}
            for state, v in us.items():
                rec[state] = {"us": min(v), "us_all": v, "spread_us": round(max(v) - min(v), 3)}
            if "bias" in us:
                rec["bias_minus_plain_us"] = round(min(us["bias"]) - min(us["plain"]), 3)
            emit(rec)

    def leg_prefill(child):
        cfg = M.LLAMA_32_3B
        dm = runtime.DeviceModel.synthetic(cfg, seed=1)
        dec = runtime.Decoder(dm)
        try:
            n = 4096
            dec.prefill_time(n, 1)
            ms = {"plain": []} if child else {"plain": [], "llama3": []}
            for _ in range(args.reps):
                for state in ms:
                    if not child:
                        dec.set_rope_scaling(LLAMA3_32 if state == "llama3" else None)
                    ms[state].append(round(dec.prefill_time(n, 2), 3))
            rec = {"leg": "prefill", "shape": "llama-3.2-3b", "positions": n}
            for state, v in ms.items():
                rec[state] = {"ms": min(v), "ms_all": v}
            emit(rec)
        finally:
            dec.close()
            dm.close()

    def leg_qwen():
        base = M.ModelConfig(dim=3584, hidden_dim=18944, head_dim=128, n_layers=28, n_heads=28, n_kv_heads=4,
                             vocab_size=152064, max_seq_len=4096, rope_theta=1e6, norm_eps=1e-6, act=M.SILU,
                             qkv_bias=True)
        prompt = [(7 * i + 1) % base.vocab_size for i in range(PROMPT_LEN)]
        tok0, pos0, steps = prompt[-1], PROMPT_LEN - 1, 20
        for name, dt in (("fp16", M.F16), ("fp8", M.F8E5M2), ("q4", M.Q4)):
            cfg = base.with_(weight_dtype=dt)
            dm = runtime.DeviceModel.synthetic(cfg, seed=1)
            dec = runtime.Decoder(dm)
            try:
                for pos, t in enumerate(prompt[:-1]):
                    dec.forward(t, pos, runtime.HYDRATE_KV_CACHE)
                dec.generate_greedy(tok0, pos0, 16)
                ms = []
                for _ in range(args.reps):
                    t0 = time.perf_counter()
                    dec.generate_greedy(tok0, pos0, steps)
                    ms.append(round((time.perf_counter() - t0) / steps * 1e3, 4))
                bpt = cfg.weight_bytes_per_token() + cfg.kv_bytes_per_token(pos0 + 1 + steps // 2)
                chunk = 64 * {M.F16: 8, M.F8E5M2: 16, M.Q4: 32}[dt]
                rec = {"leg": "qwen", "shape": "qwen2.5-7b", "dtype": name, "steps": steps, "ms_per_step": min(ms),
                       "ms_per_step_all": ms, "tok_s": round(1e3 / min(ms), 1), "bytes_per_token": bpt,
                       "roofline_frac": round(bpt / (min(ms) * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                       "kernels_per_token": dec.graph_kernels(2), "attn_wo_fused": bool(dec.attn_wo),
                       "qkv_kernel": dec.kernel_name(0),
                       "row_block_gemv": {"dim_rows": cfg.dim % chunk == 0, "hidden_rows": cfg.hidden_dim % chunk == 0}}
                kern = {}
                for kid, kname in KERNELS.items():
                    if kid == 1 and dec.attn_wo:
                        continue
                    us = [dec.time_kernel(kid, args.kernel_iters) * 1e3 for _ in range(args.reps)]
                    kern[kname] = {"us": round(min(us), 2), "us_all": [round(x, 2) for x in us]}
                rec["kernels_us"] = kern
                emit(rec)
            finally:
                dec.close()
                dm.close()

    if args.child:
        {"bias": leg_bias, "prefill": leg_prefill}[args.child](True)
        return
    for leg in args.legs.split(","):
        if leg == "bias":
            leg_bias(False)
            parent("bias")
        elif leg == "prefill":
            leg_prefill(False)
            parent("prefill")
        elif leg == "qwen":
            leg_qwen()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
