"""GPU: the yalm CLI's -s <rows> with -t > 0 and -k / -p (speculative sampled completion) prints the
tokens of the same line without -s; -s with -t > 0 alone stays a usage error."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import sampling_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "yalm_amd", "host")
PROMPT = "the thin is"
SEED = 7
TEMP, TOP_K, TOP_P, N = 0.8, 40, 0.9, 24


@pytest.fixture(scope="module")
def host_built():
    subprocess.run(["make", "-C", HOST, "-j4"], check=True, capture_output=True)
    return HOST


def run_cli(host, path, *flags):
    cmd = [os.path.join(host, "yalm"), path, "-d", "hip", "-m", "c", *flags, "-i", PROMPT]
    return subprocess.run(cmd, capture_output=True, env=dict(os.environ, YALM_SEED=str(SEED), YALM_PRINT_TOKENS="1"),
                          timeout=120)


def tokens(r):
    assert r.returncode == 0, r.stderr.decode()
    line = [l for l in r.stderr.decode().split("\n") if l.startswith("TOKENS:")][0]
    return [int(t) for t in line[len("TOKENS:"):].split()]


def cli_uniforms(n):
    """The CLI's draws: std::rand() / (float)RAND_MAX after std::srand(YALM_SEED)."""
    libc = ctypes.CDLL("libc.so.6")
    libc.srand(SEED)
    return np.array([np.float32(libc.rand()) / np.float32(2147483647) for _ in range(n)], np.float32)


def test_cli_speculative_sampled_prints_the_sampled_tokens(host_built, golden_dir):
    """YALM_SEED = 7. Every draw of the plain completion lies inside its token's kept interval by
    more than the two paths' logits can move a cumulative share (the check of
    test_gpu_spec_sampled.test_equals_plain_sampled_loop, on the CLI's own uniforms): the smallest
    distance met to an interval's end is printed with the bound and asserted above it, so the two
    completions cannot differ at this seed by a boundary draw. Measured on one MI355X: the
    smallest margin met is 7.83e-4 of S, the two paths' logits were equal bit for bit (bound 0)."""
    from yalm_amd import runtime
    from yalm_amd.tokenizer import Tokenizer
    from yalm_amd.yalmfile import read_yalm

    path = os.path.join(golden_dir, "tiny_fp16.yalm")
    flags = ("-t", str(TEMP), "-k", str(TOP_K), "-p", str(TOP_P), "-n", str(N))
    plain = run_cli(host_built, path, *flags)
    spec = run_cli(host_built, path, *flags, "-s", "4")
    want = tokens(plain)
    assert len(want) == N and len(set(want)) > 4

    # the margin of every draw, on the plain path's logits
    prompt = Tokenizer.from_yalm(read_yalm(path)).encode(PROMPT, True)
    u = cli_uniforms(N)
    dm = runtime.DeviceModel.from_yalm(path)
    a, b = runtime.Decoder(dm), runtime.Decoder(dm)
    try:
        for p, t in enumerate(prompt[:-1]):
            a.forward(t, p, runtime.HYDRATE_KV_CACHE)
            b.forward(t, p, runtime.HYDRATE_KV_CACHE)
        pos, fed = len(prompt) - 1, [prompt[-1]] + want[:-1]
        margin, delta = 1.0, 0.0
        for j in range(0, N, 4):
            rows = b.forward_rows(fed[j:j + 4], pos + j)
            for t in range(rows.shape[0]):
                l = a.forward(fed[j + t], pos + j + t).copy()
                delta = max(delta, float(np.max(np.abs(rows[t] - l))))
                rule = R.Rule(l, runtime.sample(l, TEMP, 0, 1.0, [0.5])[2], TOP_K, TOP_P)
                tok = want[j + t]
                assert rule.draw(u[j + t]) == tok, (j + t, tok)
                hi = int(rule.cum[tok]) / rule.S
                lo = (int(rule.cum[tok - 1]) if tok > 0 else 0) / rule.S
                margin = min(margin, float(u[j + t]) - lo, hi - float(u[j + t]))
        shift = 2 * float(np.expm1(2 * delta / TEMP))
        print(f"seed {SEED}: smallest margin {margin:.3e}, max |dlogit| {delta:.3e}, shift bound {shift:.3e}")
        assert margin > shift
    finally:
        a.close()
        b.close()
        dm.close()

    assert tokens(spec) == want
    out = spec.stdout.decode(errors="replace")
    assert "speculative:" in out and "accepted drafts" in out
    assert "speculative:" not in plain.stdout.decode(errors="replace")


def test_cli_speculative_with_host_sampler_is_a_usage_error(host_built, golden_dir):
    path = os.path.join(golden_dir, "tiny_fp16.yalm")
    for flags in (("-s", "4", "-t", "0.8"), ("-s", "5", "-t", "0.8", "-k", "40"), ("-s", "4", "-t", "-1", "-k", "40")):
        r = run_cli(host_built, path, *flags)
        assert r.returncode == 1
        assert "Usage:" in r.stderr.decode()
