"""GPU: the yalm CLI's -D <draft checkpoint> (with -s <rows>: the drafts come from a second model)
prints the tokens of the same command without -D, greedy and sampled on the device; -D without -s,
with -N or outside completion mode is a usage error."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "yalm_amd", "host")
PROMPT = "the thin is"
MODES = {"greedy": ("-t", "0"), "sampled": ("-t", "0.8", "-k", "20")}


@pytest.fixture(scope="module")
def host_built():
    subprocess.run(["make", "-C", HOST, "-j4"], check=True, capture_output=True)
    return HOST


def run_cli(host, path, *flags, mode="c"):
    cmd = [os.path.join(host, "yalm"), path, "-d", "hip", "-m", mode, *flags, "-i", PROMPT]
    return subprocess.run(cmd, capture_output=True, env=dict(os.environ, YALM_SEED="7", YALM_PRINT_TOKENS="1"),
                          timeout=120)


def tokens(r):
    assert r.returncode == 0, r.stderr.decode()
    line = [l for l in r.stderr.decode().split("\n") if l.startswith("TOKENS:")][0]
    return [int(t) for t in line[len("TOKENS:"):].split()]


@pytest.fixture(scope="module")
def without_draft(host_built, golden_dir):
    """The tokens of -s 4 without -D, per mode (run once, shared)."""
    path = os.path.join(golden_dir, "tiny_fp16.yalm")
    out = {m: tokens(run_cli(host_built, path, *f, "-s", "4", "-n", "40")) for m, f in MODES.items()}
    assert all(len(t) >= 1 for t in out.values())
    return out


@pytest.mark.parametrize("draft", ["tiny_fp16.yalm", "tiny_fp8.yalm"])
@pytest.mark.parametrize("mode", sorted(MODES))
def test_cli_draft_model_prints_the_same_tokens(host_built, golden_dir, without_draft, mode, draft):
    path, dpath = os.path.join(golden_dir, "tiny_fp16.yalm"), os.path.join(golden_dir, draft)
    r = run_cli(host_built, path, *MODES[mode], "-s", "4", "-D", dpath, "-n", "40")
    assert tokens(r) == without_draft[mode]
    out = r.stdout.decode(errors="replace")  # (a random-weight model prints arbitrary bytes)
    assert "speculative:" in out and "accepted drafts" in out
    assert "draft model: " + dpath in out and "drafts accepted" in out


def test_cli_draft_model_usage_errors(host_built, golden_dir):
    path = os.path.join(golden_dir, "tiny_fp16.yalm")
    cases = [
        (("-D", path, "-t", "0"), "c"),  # without -s
        (("-D", path, "-N", "2", "-t", "0.8", "-k", "20"), "c"),  # with -N
        (("-D", path, "-s", "4", "-N", "2", "-t", "0.8", "-k", "20"), "c"),
        (("-D", path), "perplexity"),
        (("-D", path, "-s", "4", "-t", "0"), "perplexity"),
        (("-D", path, "-s", "4", "-t", "0.8"), "c"),  # -s's own rule: the host sampler has no speculative form
    ]
    for flags, mode in cases:
        r = run_cli(host_built, path, *flags, mode=mode)
        assert r.returncode == 1, flags
        assert "Usage:" in r.stderr.decode() and "-D <path>" in r.stderr.decode()
