"""bench.py as the driver runs it, on the small model: a plain run times exactly --steps
steps, prints one JSON line with the headline fields and none of the --full legs, and
--dump-outputs writes what the timed greedy loop computed in its last step -- checked
against the CPU oracle on the same synthetic weights (DESIGN.md §Parity bars: greedy
tokens identical, logits within 1e-3 relative)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_py as O
from yalm_amd import models as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP = 6, 2


def test_plain_run_line_and_dumped_outputs(tmp_path):
    import bench

    out_dir = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--model", "small",
                        "--steps", str(STEPS), "--warmup", str(WARMUP), "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    assert d["unit"] == "tok/s" and d["higher_is_better"] is True and d["dtype"] == "f16"
    assert d["steps"] == STEPS and d["warmup"] == WARMUP
    assert d["ms_per_step"] > 0 and abs(d["value"] * d["ms_per_step"] / 1e3 - 1) < 1e-2
    # a plain run measures nothing beside the headline
    assert d["roofline"] is None and d["gpu_state"] is None and d["cpu_baseline"] is None
    assert not {"fp8", "prefill", "long_context"} & set(d)

    got = {n: np.load(out_dir / n) for n in sorted(os.listdir(out_dir))}
    assert sorted(got) == ["last_step.npy", "logits.npy", "tokens.npy"]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    tokens, logits, last = got["tokens.npy"], got["logits.npy"], got["last_step.npy"]

    cfg = M.PRESETS["small"]
    om = O.OracleModel(cfg, O.synth_host_tensors_fast(cfg, seed=1))
    prompt = [(7 * i + 1) % cfg.vocab_size for i in range(bench.PROMPT_LEN)]
    for pos, t in enumerate(prompt[:-1]):
        om.forward(t, pos, 0)
    ref, tok = [], prompt[-1]
    for i in range(1 + WARMUP + STEPS):
        lo = om.forward(tok, bench.PROMPT_LEN - 1 + i, 1)
        tok = int(O.olib.orc_sample_argmax(O.P(lo), cfg.vocab_size))
        ref.append(tok)
    assert tokens.astype(np.int64).tolist() == ref
    assert last.tolist() == [ref[-1], bench.PROMPT_LEN + WARMUP + STEPS]
    assert logits.shape == (cfg.vocab_size,)
    err = float(np.max(np.abs(logits - lo)) / np.max(np.abs(lo)))
    print(f"last timed step: logits rel err vs oracle {err:.2e}")
    assert err < 1e-3
