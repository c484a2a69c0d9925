"""GPU: the yalm CLI's -s <rows> (speculative greedy completion, -t 0 only) prints the tokens
of the plain greedy completion; any other temperature with -s is a usage error."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "yalm_amd", "host")
PROMPT = "the thin is"


@pytest.fixture(scope="module")
def host_built():
    subprocess.run(["make", "-C", HOST, "-j4"], check=True, capture_output=True)
    return HOST


def run_cli(host, path, *flags):
    cmd = [os.path.join(host, "yalm"), path, "-d", "hip", "-m", "c", *flags, "-i", PROMPT]
    return subprocess.run(cmd, capture_output=True, env=dict(os.environ, YALM_SEED="7", YALM_PRINT_TOKENS="1"),
                          timeout=120)


def tokens(r):
    assert r.returncode == 0, r.stderr.decode()
    line = [l for l in r.stderr.decode().split("\n") if l.startswith("TOKENS:")][0]
    return [int(t) for t in line[len("TOKENS:"):].split()]


def test_cli_speculative_prints_the_greedy_tokens(host_built, golden_dir):
    path = os.path.join(golden_dir, "tiny_fp16.yalm")
    plain = run_cli(host_built, path, "-t", "0", "-n", "24")
    spec = run_cli(host_built, path, "-t", "0", "-s", "4", "-n", "24")
    want = tokens(plain)
    assert len(want) >= 1
    assert tokens(spec) == want
    out = spec.stdout.decode(errors="replace")  # (a random-weight model prints arbitrary bytes)
    assert "speculative:" in out and "accepted drafts" in out
    assert "speculative:" not in plain.stdout.decode(errors="replace")  # off by default: nothing existing changes


def test_cli_speculative_needs_temperature_zero(host_built, golden_dir):
    path = os.path.join(golden_dir, "tiny_fp16.yalm")
    for flags in (("-s", "4", "-t", "0.8"), ("-s", "4"), ("-s", "5", "-t", "0"), ("-s", "4", "-t", "0", "-m", "perplexity")):
        r = run_cli(host_built, path, *flags)
        assert r.returncode == 1
        assert "Usage:" in r.stderr.decode()
