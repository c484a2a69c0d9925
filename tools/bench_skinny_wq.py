#!/usr/bin/env python3
"""Short-prompt prefill of quantised decoders: the native-weight skinny GEMMs against the upcast.

Synthetic Mistral-7B-shaped fp8 (E5M2), e4m3 and q4 decoders (and the f16 one, the stream-rate
yardstick) in one process: wall time of a synchronous n-position prefill without log-probs at
n = 1, 13, 64, the default (native, prefill_skinny_wq.h) and skq:0 (the per-layer f16 upcast) in
alternation, `--reps` repeats of `--iters` prefills each; the best repeat, every repeat and the
spread (max - min) are printed, and the achieved bytes/s of the layer weights in the format's own
bytes. With --parent-lib (a build of the parent commit: tools/build_ab_lib.sh) a fresh process
measures that library's default the same way; `bar`: native at n = 13 faster than the parent by
more than the larger repeat spread of the two.

Prints one JSON line per measurement; --out appends them to a file.

Usage: python tools/bench_skinny_wq.py [--reps 3] [--iters 5] [--layers N] [--parent-lib PATH] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LENGTHS = (1, 13, 64)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--layers", type=int, default=0, help="fewer layers = a smaller model of the same shapes")
    ap.add_argument("--parent-lib", type=str, default=None)
    ap.add_argument("--child", action="store_true", help="internal: the parent library's part")
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
    fmts = {"f16": M.F16, "fp8": M.F8E5M2, "e4m3": M.E4M3, "q4": M.Q4}
    forms = {"default": ""} if args.child else {"native": "", "upcast": "skq:0"}
    best = {}
    for name, dt in fmts.items():
        c = base.with_(weight_dtype=dt)
        layer_bytes = c.n_layers * sum(r * M.row_bytes(dt, n) for r, n in (
            (c.q_dim + 2 * c.kv_dim, c.dim), (c.dim, c.q_dim), (2 * c.hidden_dim, c.dim), (c.dim, c.hidden_dim)))
        dm = runtime.DeviceModel.synthetic(c, seed=1)
        dec = runtime.Decoder(dm)
        try:
            for n in LENGTHS:
                tokens = [(7 * i + 1) % c.vocab_size for i in range(n)]
                ms = {k: [] for k in forms}
                for rep in range(args.reps + 1):  # (repeat 0 warms up)
                    for k, spec in forms.items():
                        if name == "f16" and k == "upcast":
                            continue
                        dec.set_prefill_forms(spec)
                        t0 = time.perf_counter()
                        for _ in range(args.iters):
                            dec.prefill(tokens, logprobs=False)
                        if rep:
                            ms[k].append((time.perf_counter() - t0) / args.iters * 1e3)
                for k, v in ms.items():
                    if not v:
                        continue
                    best[(name, n, k)] = (min(v), max(v) - min(v))
                    emit({"leg": "prefill", "library": "parent" if args.child else "this", "dtype": name, "form": k,
                          "positions": n, "n_layers": c.n_layers, "ms": round(min(v), 3),
                          "ms_all": [round(x, 3) for x in v], "spread_ms": round(max(v) - min(v), 3),
                          "layer_weight_gbs": round(layer_bytes / (min(v) * 1e-3) / 1e9, 1)})
        finally:
            dec.close()
            dm.close()
    if args.parent_lib and not args.child:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps), "--iters", str(args.iters),
               "--layers", str(args.layers)]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=900,
                             env=dict(os.environ, YALM_LIB=os.path.abspath(args.parent_lib)))
        if out.returncode:
            raise SystemExit(f"parent run failed: {out.stderr[-2000:]}")
        for ln in out.stdout.splitlines():
            if not ln.startswith("{"):
                continue
            rec = json.loads(ln)
            lines.append(ln)
            print(ln, flush=True)
            if rec["positions"] == 13 and rec["dtype"] != "f16":
                nat, spread = best[(rec["dtype"], 13, "native")]
                allowed = max(spread, rec["spread_ms"])
                emit({"leg": "bar", "dtype": rec["dtype"], "native_ms": round(nat, 3), "parent_ms": rec["ms"],
                      "repeat_spread_ms": round(allowed, 3), "faster_than_parent": bool(rec["ms"] - nat > allowed)})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
