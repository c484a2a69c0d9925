"""The yalm CLI on a Mixtral model with prefill-capable dims (hidden_size 256, 4 experts, 2
active; written as an HF dir and converted by the project's converter): -m perplexity and prompt
hydration go through the batched expert prefill and agree with the position-by-position run
(YALM_NO_PREFILL=1). The model's seed keeps every routing decision clear of rounding
(tests/test_moe_prefill_cpu.py)."""
import os
import re
import subprocess

import numpy as np
import pytest

import moe_prefill_inputs as I

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "yalm_amd", "host")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host_built():
    subprocess.run(["make", "-C", HOST, "-j4"], check=True, capture_output=True)
    return HOST


@pytest.fixture(scope="module")
def model_path(tmp_path_factory):
    return I.host_yalm(tmp_path_factory.mktemp("moe_pf"))


def test_cli_perplexity_prefill_matches_sequential(host_built, model_path):
    exe = os.path.join(host_built, "yalm")

    def ppl(extra_env):
        r = subprocess.run([exe, model_path, "-d", "hip", "-m", "perplexity", "-i", I.HOST_PPL_TEXT], capture_output=True,
                           env=dict(os.environ, **extra_env), timeout=120)
        assert r.returncode == 0, r.stderr.decode()
        out = r.stdout.decode()
        m = re.search(r"perplexity: ([0-9.eE+-]+)", out)
        assert m, out
        return float(m.group(1)), out

    p_batched, out_b = ppl({})
    p_seq, out_s = ppl({"YALM_NO_PREFILL": "1"})
    assert "batched prefill" in out_b and "batched prefill" not in out_s
    print(f"|d log ppl| batched vs sequential {abs(np.log(p_batched) - np.log(p_seq)):.2e}")
    assert abs(np.log(p_batched) - np.log(p_seq)) < 1e-3, (p_batched, p_seq)


def test_cli_completion_prefill_same_tokens(host_built, model_path):
    exe = os.path.join(host_built, "yalm")

    def toks(extra_env):
        r = subprocess.run([exe, model_path, "-d", "hip", "-m", "c", "-t", "0", "-n", str(I.HOST_GREEDY), "-i",
                            I.HOST_PROMPT], capture_output=True,
                           env=dict(os.environ, YALM_PRINT_TOKENS="1", **extra_env), timeout=120)
        assert r.returncode == 0, r.stderr.decode()
        return [l for l in r.stderr.decode().split("\n") if l.startswith("TOKENS:")][0]

    assert toks({}) == toks({"YALM_NO_PREFILL": "1"})
