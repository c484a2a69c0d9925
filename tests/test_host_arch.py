"""C++20 host layer on Qwen2 (q / k / v bias) and Llama-3 (llama3 RoPE scaling) files: a tiny
HF directory of each family converted by yalm_amd.convert, then the yalm CLI end to end on the
GPU -- greedy completion (plain and by speculative steps, -s 4) against the Python decoder and
the float64 reference of arch_ref.py, and -m perplexity through the batched prefill against
the position-by-position loop within test_host.py's bar. No CLI flag selects the forms: the
file's metadata does."""
import os
import re
import subprocess

import numpy as np
import pytest

import arch_hf
from yalm_amd import convert

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "yalm_amd", "host")
PPL_BAR = 1e-3  # test_host.py::test_cli_perplexity_prefill_matches_sequential: |d log ppl|, nats per position
PPL_TEXT = ("the sky is blue and the grass is green and the sun is yellow here we go there and back again "
            "remember this important info the pass key is hidden inside a lot of irrelevant text")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host_built():
    subprocess.run(["make", "-C", HOST, "-j4"], check=True, capture_output=True)
    return HOST


def converted(tmp_path, name, dims=None, dtype="fp16"):
    writer, hf = arch_hf.HOST_MODELS[name]
    writer(str(tmp_path / "hf"), hf=dict(hf, **(dims or {})))
    out = str(tmp_path / f"{name}_{dtype}.yalm")
    convert.convert(str(tmp_path / "hf"), out, dtype)
    return out


def cli_tokens(exe, path, extra=()):
    cmd = [exe, path, "-d", "hip", "-m", "c", "-t", "0", "-n", str(arch_hf.HOST_N), "-i", arch_hf.HOST_PROMPT, *extra]
    r = subprocess.run(cmd, capture_output=True, env=dict(os.environ, YALM_PRINT_TOKENS="1"), timeout=120)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    line = [l for l in r.stderr.decode(errors="replace").split("\n") if l.startswith("TOKENS:")][0]
    return [int(t) for t in line[len("TOKENS:"):].split()]


@pytest.mark.parametrize("name", sorted(arch_hf.HOST_MODELS))
def test_cli_greedy_matches_python_and_reference(host_built, tmp_path, name):
    from yalm_amd import runtime as R

    path = converted(tmp_path, name)
    enc, ref, gap = arch_hf.host_reference(path)
    assert gap >= 1e-3, gap  # (test_arch_cpu.py::test_host_models_have_no_near_tie)
    exe = os.path.join(host_built, "yalm")
    got = cli_tokens(exe, path)
    assert got == ref
    assert cli_tokens(exe, path, ("-s", "4")) == ref
    dm = R.DeviceModel.from_yalm(path)
    dec = R.Decoder(dm)
    try:
        assert dm.cfg.qkv_bias == (name == "qwen2") and (dm.cfg.rope_scaling is not None) == (name == "llama3")
        for pos, tk in enumerate(enc[:-1]):
            dec.forward(tk, pos, R.HYDRATE_KV_CACHE)
        assert dec.generate_greedy(enc[-1], len(enc) - 1, len(ref)) == ref
    finally:
        dec.close()
        dm.close()


@pytest.mark.parametrize("name", sorted(arch_hf.HOST_MODELS))
def test_cli_perplexity_prefill_matches_sequential(host_built, tmp_path, name):
    path = converted(tmp_path, name, dims=arch_hf.PF_DIMS)
    exe = os.path.join(host_built, "yalm")

    def ppl(extra_env):
        r = subprocess.run([exe, path, "-d", "hip", "-m", "perplexity", "-i", PPL_TEXT], capture_output=True,
                           env=dict(os.environ, **extra_env), timeout=120)
        assert r.returncode == 0, r.stderr.decode(errors="replace")
        out = r.stdout.decode(errors="replace")
        m = re.search(r"perplexity: ([0-9.eE+-]+)", out)
        assert m, out
        return float(m.group(1)), out

    p_batched, out_b = ppl({})
    p_seq, _ = ppl({"YALM_NO_PREFILL": "1"})
    assert "batched prefill" in out_b
    d = abs(np.log(p_batched) - np.log(p_seq))
    print(f"{name}: |d log ppl| batched vs sequential {d:.2e}")
    assert d < PPL_BAR, (p_batched, p_seq)
