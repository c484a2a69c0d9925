"""GPU: the yalm CLI on an e4m3 file (yalm_amd/host): the committed tiny fp16 fixture quantised
to e4m3 at test time, and its exact f16 twin file beside it."""
import os
import re
import subprocess

import numpy as np
import pytest

from yalm_amd import models as M
from yalm_amd.tokenizer import Tokenizer
from yalm_amd.yalmfile import read_yalm, write_yalm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "yalm_amd", "host")
TEXT = ("the sky is blue and the grass is green and the sun is yellow here we go there and back again "
        "remember this important info the pass key is hidden inside a lot of irrelevant text")


@pytest.fixture(scope="module")
def host_built():
    subprocess.run(["make", "-C", HOST, "-j4"], check=True, capture_output=True)
    return os.path.join(HOST, "yalm")


@pytest.fixture(scope="module")
def e4m3_files(tmp_path_factory, golden_dir):
    """(e4m3 file, f16 twin file) of tests/golden/tiny_fp16.yalm."""
    d = tmp_path_factory.mktemp("e4m3")
    yd = read_yalm(os.path.join(golden_dir, "tiny_fp16.yalm"))
    cfg = M.config_from_metadata(yd.metadata).with_(weight_dtype=M.E4M3)
    shapes = M.tensor_shapes(cfg)
    t8, dt8 = {}, {}
    for k, v in yd.tensors.items():
        a = np.array(v.data).reshape(v.shape)
        is_weight = k in shapes and not shapes[k][1]
        t8[k] = M.e4m3_quantize(a) if is_weight else a
        dt8[k] = "U8" if is_weight else v.dtype
    md = dict(yd.metadata)
    yd.close()
    _, t16 = M.e4m3_twin(cfg, t8)
    t16 = {k: t16.get(k, v) for k, v in t8.items()}
    dt16 = {k: ("F16" if k in shapes and not shapes[k][1] else v) for k, v in dt8.items()}
    p8, p16 = str(d / "tiny_e4m3.yalm"), str(d / "tiny_e4m3_twin.yalm")
    write_yalm(p8, t8, dict(md, dtype="e4m3"), dt8)
    write_yalm(p16, t16, dict(md, dtype="fp16"), dt16)
    return p8, p16


def _cli_tokens(host_built, path, n, extra=()):
    r = subprocess.run([host_built, path, "-d", "hip", "-m", "c", "-t", "0", "-n", str(n), "-i", "the thin is", *extra],
                       capture_output=True, env=dict(os.environ, YALM_PRINT_TOKENS="1"), timeout=120)
    assert r.returncode == 0, r.stderr.decode()
    line = [l for l in r.stderr.decode().split("\n") if l.startswith("TOKENS:")][0]
    return [int(t) for t in line[len("TOKENS:"):].split()], r.stdout.decode(errors="replace")


def test_cli_greedy_matches_python_runtime_and_speculative(host_built, e4m3_files):
    """yalm <e4m3 file> -d hip -m c -t 0 -n 24 prints the tokens the Python runtime's greedy loop
    gives on the same file, and -s 4 (speculative steps of 4 rows) prints the same tokens."""
    from yalm_amd import runtime

    p8, _ = e4m3_files
    n = 24
    got, out = _cli_tokens(host_built, p8, n)
    assert "dtype: E4M3" in out  # (random-weight text decodes to any bytes)

    yd = read_yalm(p8)
    enc = Tokenizer.from_yalm(yd).encode("the thin is")
    yd.close()
    dm = runtime.DeviceModel.from_yalm(p8)
    dec = runtime.Decoder(dm)
    try:
        assert dm.cfg.weight_dtype == M.E4M3
        for pos, tk in enumerate(enc[:-1]):
            dec.forward(tk, pos, runtime.HYDRATE_KV_CACHE)
        ref = dec.generate_greedy(enc[-1], len(enc) - 1, n)
    finally:
        dec.close()
        dm.close()
    if dm.cfg.eos_token_id in ref:  # the CLI stops at the end-of-sequence token
        ref = ref[: ref.index(dm.cfg.eos_token_id) + 1]
    assert got == ref
    spec, out = _cli_tokens(host_built, p8, n, ("-s", "4"))
    assert "speculative:" in out
    assert spec == got


def test_cli_perplexity_matches_f16_twin(host_built, e4m3_files):
    """-m perplexity on the e4m3 file within 1e-3 nats (log ppl) of the same CLI on the twin."""

    def log_ppl(path):
        r = subprocess.run([host_built, path, "-d", "hip", "-m", "perplexity", "-i", TEXT], capture_output=True,
                           timeout=120)
        assert r.returncode == 0, r.stderr.decode()
        m = re.search(r"perplexity: ([0-9.eE+-]+)", r.stdout.decode())
        assert m, r.stdout.decode()
        return float(np.log(float(m.group(1))))

    a, b = log_ppl(e4m3_files[0]), log_ppl(e4m3_files[1])
    print(f"log ppl e4m3 {a:.6f} twin {b:.6f}")
    assert abs(a - b) < 1e-3


def test_cli_sampling_flags_run_on_e4m3(host_built, e4m3_files):
    r = subprocess.run([host_built, e4m3_files[0], "-d", "hip", "-m", "c", "-t", "0.8", "-k", "20", "-p", "0.9", "-n",
                        "8", "-i", "the thin is"], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode()
