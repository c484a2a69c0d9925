"""C++20 host layer on a Qwen3 file (q / k norm): a tiny HF directory converted by
yalm_amd.convert, then the yalm CLI end to end on the GPU -- greedy completion (plain and by
speculative steps, -s 4) against the Python decoder and the float64 reference of qknorm_ref.py,
and -m perplexity through the batched prefill against the position-by-position loop within test_host.py's bar. No CLI flag
selects the norm: the file's metadata does."""
import os
import re
import subprocess

import numpy as np
import pytest

import arch_hf
import qknorm_hf
from test_host_arch import PPL_BAR, PPL_TEXT
from yalm_amd import convert

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "yalm_amd", "host")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def host_built():
    subprocess.run(["make", "-C", HOST, "-j4"], check=True, capture_output=True)
    return HOST


def converted(tmp_path, dims=None, dtype="fp16"):
    qknorm_hf.write_qwen3(str(tmp_path / "hf"), hf=dict(qknorm_hf.QWEN3_HF, **(dims or {})))
    out = str(tmp_path / f"qwen3_{dtype}.yalm")
    convert.convert(str(tmp_path / "hf"), out, dtype)
    return out


def cli_tokens(exe, path, extra=()):
    cmd = [exe, path, "-d", "hip", "-m", "c", "-t", "0", "-n", str(qknorm_hf.HOST_N), "-i", qknorm_hf.HOST_PROMPT, *extra]
    r = subprocess.run(cmd, capture_output=True, env=dict(os.environ, YALM_PRINT_TOKENS="1"), timeout=120)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    line = [l for l in r.stderr.decode(errors="replace").split("\n") if l.startswith("TOKENS:")][0]
    return [int(t) for t in line[len("TOKENS:"):].split()]


def test_cli_greedy_matches_python_and_reference(host_built, tmp_path):
    from yalm_amd import runtime as R

    path = converted(tmp_path)
    enc, ref, gap = qknorm_hf.host_reference(path)
    assert gap >= 1e-3, gap  # (test_qknorm_cpu.py::test_host_model_has_no_near_tie)
    exe = os.path.join(host_built, "yalm")
    assert cli_tokens(exe, path) == ref
    assert cli_tokens(exe, path, ("-s", "4")) == ref
    dm = R.DeviceModel.from_yalm(path)
    dec = R.Decoder(dm)
    try:
        assert dm.cfg.qk_norm and not dm.cfg.qkv_bias
        assert dec.kernel_name(0).endswith("PQKVN<")
        for pos, tk in enumerate(enc[:-1]):
            dec.forward(tk, pos, R.HYDRATE_KV_CACHE)
        assert dec.generate_greedy(enc[-1], len(enc) - 1, len(ref)) == ref
    finally:
        dec.close()
        dm.close()


def test_cli_perplexity_prefill_matches_sequential(host_built, tmp_path):
    path = converted(tmp_path, dims=dict(arch_hf.PF_DIMS, head_dim=64))
    exe = os.path.join(host_built, "yalm")

    def ppl(extra_env):
        r = subprocess.run([exe, path, "-d", "hip", "-m", "perplexity", "-i", PPL_TEXT], capture_output=True,
                           env=dict(os.environ, **extra_env), timeout=120)
        assert r.returncode == 0, r.stderr.decode(errors="replace")
        out = r.stdout.decode(errors="replace")
        m = re.search(r"perplexity: ([0-9.eE+-]+)", out)
        assert m, out
        return float(m.group(1)), out

    (p_batched, out_b), (p_seq, out_s) = ppl({}), ppl({"YALM_NO_PREFILL": "1"})
    assert "batched prefill" in out_b and "batched prefill" not in out_s
    d = abs(np.log(p_batched) - np.log(p_seq))
    print(f"qwen3: |d log ppl| batched vs sequential {d:.2e}")
    assert d < PPL_BAR, (p_batched, p_seq)
