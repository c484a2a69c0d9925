"""GPU: the yalm CLI with -k / -p samples on the device (Model::forward_sampled), one
std::rand() / (float)RAND_MAX per generated token from the stream YALM_SEED seeded; a Python
replay with libc's srand / rand and Decoder.generate_sampled gives the same tokens."""
import ctypes
import ctypes.util
import os
import subprocess

import numpy as np
import pytest

from yalm_amd.tokenizer import Tokenizer
from yalm_amd.yalmfile import read_yalm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "yalm_amd", "host")
PROMPT = "the thin is"
RAND_MAX = 2147483647  # glibc


@pytest.fixture(scope="module")
def host_built():
    subprocess.run(["make", "-C", HOST, "-j4"], check=True, capture_output=True)
    return HOST


def run_cli(host, path, *flags):
    cmd = [os.path.join(host, "yalm"), path, "-d", "hip", "-m", "c", *flags, "-i", PROMPT]
    r = subprocess.run(cmd, capture_output=True, env=dict(os.environ, YALM_SEED="7", YALM_PRINT_TOKENS="1"),
                       timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    line = [l for l in r.stderr.decode().split("\n") if l.startswith("TOKENS:")][0]
    return line, [int(t) for t in line[len("TOKENS:"):].split()]


def test_cli_device_sampling_matches_python_replay(host_built, golden_dir):
    from yalm_amd import runtime

    path = os.path.join(golden_dir, "tiny_fp16.yalm")
    n, T, k, p = 24, 0.8, 40, 0.9
    _, got = run_cli(host_built, path, "-t", str(T), "-k", str(k), "-p", str(p), "-n", str(n))

    libc = ctypes.CDLL(ctypes.util.find_library("c"))
    libc.srand(7)
    u = np.array([np.float32(libc.rand()) / np.float32(RAND_MAX) for _ in range(n)], np.float32)
    yd = read_yalm(path)
    tok = Tokenizer.from_yalm(yd)
    yd.close()
    enc = tok.encode(PROMPT)
    dm = runtime.DeviceModel.from_yalm(path)
    dec = runtime.Decoder(dm)
    try:
        for pos, t in enumerate(enc[:-1]):
            dec.forward(t, pos, runtime.HYDRATE_KV_CACHE)
        want, t, pos = [], enc[-1], len(enc) - 1
        for i in range(n):
            t = dec.generate_sampled(t, pos, 1, T, k, p, uniforms=u[i:i + 1])[0]
            want.append(t)
            pos += 1
            if t in (tok.eos_id, getattr(tok, "eot_id", -1)):
                break
    finally:
        dec.close()
        dm.close()
    assert got == want


def test_cli_top_k_one_is_greedy(host_built, golden_dir):
    path = os.path.join(golden_dir, "tiny_fp16.yalm")
    sampled, _ = run_cli(host_built, path, "-t", "0.8", "-k", "1", "-p", "0.9", "-n", "24")
    greedy, _ = run_cli(host_built, path, "-t", "0", "-n", "24")
    assert sampled == greedy
    # -t 0 keeps the greedy path whatever -p and -k say
    assert run_cli(host_built, path, "-t", "0", "-k", "40", "-p", "0.9", "-n", "24")[0] == greedy
