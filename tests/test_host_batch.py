"""The yalm CLI's -N <2..4> (completions of one prompt, decoded together): the refusals need no
GPU (the usage error comes before any device work); on the GPU the completions printed are those
of Batch.generate_sampled with the uniforms handed out in the documented order -- chunk by chunk
of 16 steps, inside a chunk sequence by sequence -- and each is cut at its EOS."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "yalm_amd", "host")
PROMPT = "the thin is"
SEED = 7
TEMP, TOP_K, TOP_P, N_STEPS, CHUNK = 0.8, 40, 0.9, 24, 16


@pytest.fixture(scope="module")
def host_built():
    subprocess.run(["make", "-C", HOST, "-j4"], check=True, capture_output=True)
    return HOST


def run_cli(host, path, *flags, mode="c"):
    cmd = [os.path.join(host, "yalm"), path, "-d", "hip", "-m", mode, *flags, "-i", PROMPT]
    return subprocess.run(cmd, capture_output=True, env=dict(os.environ, YALM_SEED=str(SEED), YALM_PRINT_TOKENS="1"),
                          timeout=120)


def test_cli_N_refusals(host_built, golden_dir):
    """-N outside 2..4, greedy, the host sampler (-t > 0 alone), with -s, outside completion mode:
    the usage text and exit status 1, before the model is loaded."""
    path = os.path.join(golden_dir, "tiny_fp16.yalm")
    dev = ("-t", "0.8", "-k", "40")
    for flags, mode in ((("-N", "1") + dev, "c"), (("-N", "5") + dev, "c"), (("-N", "-2") + dev, "c"),
                        (("-N", "3", "-t", "0"), "c"), (("-N", "3", "-t", "0", "-k", "40"), "c"),
                        (("-N", "3", "-t", "0.8"), "c"), (("-N", "3", "-s", "2") + dev, "c"),
                        (("-N", "3") + dev, "perplexity")):
        r = run_cli(host_built, path, *flags, mode=mode)
        assert r.returncode == 1, flags
        err = r.stderr.decode()
        assert "Usage:" in err and "-N <int>" in err, flags
        assert "Using HIP" not in r.stdout.decode()


def cli_uniforms(n):
    """The CLI's draws: std::rand() / (float)RAND_MAX after std::srand(YALM_SEED)."""
    libc = ctypes.CDLL("libc.so.6")
    libc.srand(SEED)
    return np.array([np.float32(libc.rand()) / np.float32(2147483647) for _ in range(n)], np.float32)


def hand_out(stream, n_seq, n_steps, chunk=CHUNK):
    """uniforms[s][i] as the CLI hands the RNG stream out: chunk by chunk, sequence-major inside."""
    u = np.zeros((n_seq, n_steps), np.float32)
    k = 0
    for c0 in range(0, n_steps, chunk):
        c = min(chunk, n_steps - c0)
        for s in range(n_seq):
            u[s, c0:c0 + c] = stream[k:k + c]
            k += c
    return u, k


def test_hand_out_order():
    u, used = hand_out(np.arange(72, dtype=np.float32), 3, 24)
    assert used == 72
    assert u[0, :16].tolist() == list(range(16)) and u[1, :16].tolist() == list(range(16, 32))
    assert u[2, :16].tolist() == list(range(32, 48))
    assert u[0, 16:].tolist() == list(range(48, 56)) and u[2, 16:].tolist() == list(range(64, 72))


@pytest.mark.gpu
@pytest.mark.parametrize("n_seq", [2, 4])
def test_cli_N_prints_the_batch_completions(host_built, golden_dir, n_seq):
    from yalm_amd import runtime
    from yalm_amd.tokenizer import Tokenizer
    from yalm_amd.yalmfile import read_yalm

    path = os.path.join(golden_dir, "tiny_fp16.yalm")
    r = run_cli(host_built, path, "-t", str(TEMP), "-k", str(TOP_K), "-p", str(TOP_P), "-n", str(N_STEPS), "-N", str(n_seq))
    assert r.returncode == 0, r.stderr.decode()
    got = {}
    for l in r.stderr.decode().split("\n"):
        if l.startswith("TOKENS["):
            got[int(l[7:l.index("]")])] = [int(t) for t in l[l.index(":") + 1:].split()]
    assert sorted(got) == list(range(n_seq))
    out = r.stdout.decode(errors="replace")
    for q in range(n_seq):
        assert f"--- completion {q + 1} of {n_seq} ---" in out

    yd = read_yalm(path)
    tok = Tokenizer.from_yalm(yd)
    prompt = tok.encode(PROMPT, True)
    u, _ = hand_out(cli_uniforms(n_seq * N_STEPS), n_seq, N_STEPS)
    dm = runtime.DeviceModel.from_yalm(path)
    dec = runtime.Decoder(dm)
    try:
        for p, t in enumerate(prompt[:-1]):  # the CLI hydrates through the prefill where the model has one: the
            dec.forward(t, p, runtime.HYDRATE_KV_CACHE)  # tiny model (dim 64) has none, so these are its calls
        b = runtime.Batch(dec, n_seq)
        try:
            b.load(len(prompt) - 1)
            want, _ = b.generate_sampled([prompt[-1]] * n_seq, [len(prompt) - 1] * n_seq, N_STEPS, TEMP, TOP_K, TOP_P,
                                         uniforms=u)
        finally:
            b.close()
    finally:
        dec.close()
        dm.close()
    stops = {tok.eos_id, getattr(tok, "eot_id", -1)}
    for q in range(n_seq):
        w = want[q].tolist()
        cut = next((i + 1 for i, t in enumerate(w) if t in stops), len(w))
        assert got[q] == w[:cut], q
    assert len({tuple(v) for v in got.values()}) == n_seq  # the completions differ
