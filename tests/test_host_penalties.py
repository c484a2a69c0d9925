"""GPU: the yalm CLI's --repeat-penalty / --frequency-penalty / --presence-penalty / --min-p /
--penalty-window sample on the device over the prompt and the generated tokens; a Python replay
with the same uniforms (as test_host_sampling) and Decoder.generate_sampled gives the same tokens."""
import ctypes
import ctypes.util
import os
import subprocess

import numpy as np
import pytest

from test_host_sampling import PROMPT, RAND_MAX, host_built, run_cli  # noqa: F401  (host_built: a fixture)
from yalm_amd.tokenizer import Tokenizer
from yalm_amd.yalmfile import read_yalm

pytestmark = pytest.mark.gpu


def test_cli_penalties_match_python_replay(host_built, golden_dir):
    from yalm_amd import runtime

    path = os.path.join(golden_dir, "tiny_fp16.yalm")
    n, T, k = 24, 0.8, 40
    pen = dict(repetition=1.2, frequency=0.2, presence=0.1, min_p=0.05, window=6)
    base = ["-t", str(T), "-k", str(k), "-n", str(n)]
    got = run_cli(host_built, path, *base, "--repeat-penalty", "1.2", "--frequency-penalty", "0.2",
                  "--presence-penalty", "0.1", "--min-p", "0.05", "--penalty-window", "6")[1]
    libc = ctypes.CDLL(ctypes.util.find_library("c"))
    libc.srand(7)
    u = np.array([np.float32(libc.rand()) / np.float32(RAND_MAX) for _ in range(n)], np.float32)
    yd = read_yalm(path)
    tok = Tokenizer.from_yalm(yd)
    yd.close()
    hist, want = list(tok.encode(PROMPT)), []
    dm = runtime.DeviceModel.from_yalm(path)
    dec = runtime.Decoder(dm)
    try:
        for pos, t in enumerate(hist[:-1]):
            dec.forward(t, pos, runtime.HYDRATE_KV_CACHE)
        for i in range(n):
            want.append(dec.generate_sampled(hist[-1], len(hist) - 1, 1, T, k, uniforms=u[i:i + 1], penalties=pen,
                                             context=hist[:-1])[0])
            hist.append(want[-1])
            if want[-1] in (tok.eos_id, getattr(tok, "eot_id", -1)):
                break
    finally:
        dec.close()
        dm.close()
    assert got == want and got != run_cli(host_built, path, *base)[1]


def test_cli_refuses_penalties_with_speculative_rows(host_built, golden_dir):
    cmd = [os.path.join(host_built, "yalm"), os.path.join(golden_dir, "tiny_fp16.yalm"), "-t", "0.8", "-s", "4",
           "--repeat-penalty", "1.2", "-i", PROMPT]
    r = subprocess.run(cmd, capture_output=True, timeout=120)
    assert r.returncode != 0 and b"--repeat-penalty" in r.stderr and b"go with neither -s nor -N" in r.stderr
