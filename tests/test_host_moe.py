"""The yalm CLI on the committed Mixtral fixture (tiny_moe_fp16.yalm, written by the reference
converter) against the composed mixture-of-experts reference (tests/moe_ref.py): greedy
completion and position-by-position perplexity."""
import os
import re
import subprocess

import numpy as np
import pytest

import moe_ref as R
from yalm_amd.tokenizer import Tokenizer
from yalm_amd.yalmfile import read_yalm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "yalm_amd", "host")
FIXTURE = "tiny_moe_fp16.yalm"
PROMPT = "the thin is"
PPL_TEXT = "the sky is blue and the grass is green and the sun is yellow here we go there and back again"

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host_built():
    subprocess.run(["make", "-C", HOST, "-j4"], check=True, capture_output=True)
    return HOST


def _encode(path, text):
    yd = read_yalm(path)
    ids = Tokenizer.from_yalm(yd).encode(text)
    yd.close()
    return ids


def test_cli_greedy_matches_reference(host_built, golden_dir):
    """yalm <file> -d hip -m c -t 0 -n 24: generated ids == the reference's greedy tokens."""
    path = os.path.join(golden_dir, FIXTURE)
    n = 24
    r = subprocess.run([os.path.join(host_built, "yalm"), path, "-d", "hip", "-m", "c", "-t", "0", "-n", str(n), "-i",
                        PROMPT], capture_output=True, env=dict(os.environ, YALM_PRINT_TOKENS="1"), timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    line = [l for l in r.stderr.decode().split("\n") if l.startswith("TOKENS:")][0]
    got = [int(t) for t in line[len("TOKENS:"):].split()]

    cfg, t = R.yalm_tensors(path)
    ref = R.MoeRef(cfg, t)
    enc = _encode(path, PROMPT)
    for pos, tk in enumerate(enc[:-1]):
        ref.forward(tk, pos, 0)
    want = []
    lg = ref.forward(enc[-1], len(enc) - 1)
    pos = len(enc)
    for _ in range(n):
        nt = int(np.argmax(lg))
        want.append(nt)
        if nt == cfg.eos_token_id:
            break
        lg = ref.forward(nt, pos)
        pos += 1
    assert got == want


def test_cli_perplexity_matches_reference(host_built, golden_dir):
    """-m perplexity on a mixture-of-experts file runs position by position (yalm_prefill
    returns YALM_ERR_UNSUPPORTED) and gives the reference's mean log p per position within
    1e-3 nats, the bar of test_host.py's perplexity test."""
    path = os.path.join(golden_dir, FIXTURE)
    r = subprocess.run([os.path.join(host_built, "yalm"), path, "-d", "hip", "-m", "perplexity", "-i", PPL_TEXT],
                       capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    out = r.stdout.decode()
    assert "batched prefill" not in out
    m = re.search(r"perplexity: ([0-9.eE+-]+)", out)
    assert m, out
    ppl = float(m.group(1))

    cfg, t = R.yalm_tensors(path)
    ref = R.MoeRef(cfg, t)
    enc = _encode(path, PPL_TEXT)
    assert len(enc) <= cfg.max_seq_len
    lps = []
    for pos in range(len(enc) - 1):
        lg = ref.forward(enc[pos], pos).astype(np.float64)
        lps.append(lg[enc[pos + 1]] - lg.max() - np.log(np.sum(np.exp(lg - lg.max()))))
    want = -float(np.mean(lps))
    print(f"log ppl: cli {np.log(ppl):.6f} reference {want:.6f}")
    assert abs(np.log(ppl) - want) < 1e-3, (ppl, np.exp(want))
