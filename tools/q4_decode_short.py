#!/usr/bin/env python3
"""A short q4 decode for a profiler: a synthetic Mistral-7B-shaped q4 model, bench.py's 13-token
prompt hydrated, then 20 greedy steps launched eagerly (profilers mis-handle graph replay).

Usage: rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o q4 -- python tools/q4_decode_short.py
(counters, e.g. --pmc SQ_ACTIVE_INST_VALU SQ_BUSY_CYCLES, in a run of their own)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from yalm_amd import models as M  # noqa: E402
from yalm_amd import runtime  # noqa: E402

cfg = M.MISTRAL_7B.with_(weight_dtype=M.DTYPE_NAMES[sys.argv[1] if len(sys.argv) > 1 else "q4"])
dm = runtime.DeviceModel.synthetic(cfg, seed=1)
dec = runtime.Decoder(dm, launch=runtime.LAUNCH_EAGER)
prompt = [(7 * i + 1) % cfg.vocab_size for i in range(13)]
for pos, t in enumerate(prompt[:-1]):
    dec.forward(t, pos, runtime.HYDRATE_KV_CACHE)
print(dec.generate_greedy(prompt[-1], len(prompt) - 1, 20))
dec.close()
dm.close()
