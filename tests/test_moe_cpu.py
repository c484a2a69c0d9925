"""Mixture of experts without a GPU: the gate restatement against hand-computed cases, converter
parity with the reference converter's committed Mixtral fixtures, the configuration round trip,
the C++ host accepting a Mixtral file, and the routing margins of every input the GPU tests use
(tests/moe_ref.py)."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import moe_ref as R
from golden import make_moe_golden
from yalm_amd import convert, models as M, yalmfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "yalm_amd", "host")


# ---------------------------------------------------------------- 1. the gate
def _softmax_sel(vals):
    v = np.asarray(vals, np.float64)
    e = np.exp(v - v.max())
    return e / e.sum()


def test_gate_k1():
    e, w = R.moe_gate([0.5, 2.0, -1.0, 1.5], 1)
    assert e.tolist() == [1] and w.tolist() == [1.0]


def test_gate_k_equals_e_descending_order():
    lg = [0.25, -3.0, 4.0, 1.0]
    e, w = R.moe_gate(lg, 4)
    assert e.tolist() == [2, 3, 0, 1]
    np.testing.assert_allclose(w, _softmax_sel([4.0, 1.0, 0.25, -3.0]), rtol=1e-6)
    assert abs(float(w.sum()) - 1.0) < 1e-6


def test_gate_exact_ties_lowest_index_first():
    e, _ = R.moe_gate([1.0, 7.0, 3.0, 7.0, 7.0, 0.0], 2)
    assert e.tolist() == [1, 3]
    e, w = R.moe_gate([2.0, 2.0, 2.0, 2.0], 3)
    assert e.tolist() == [0, 1, 2]
    np.testing.assert_allclose(w, [1 / 3] * 3, rtol=1e-6)


def test_gate_five_experts():
    lg = [0.0, np.log(2.0), -5.0, np.log(6.0), 1e-3]
    e, w = R.moe_gate(lg, 2)
    assert e.tolist() == [3, 1]
    np.testing.assert_allclose(w, [0.75, 0.25], rtol=1e-6)  # 6 / (6 + 2), 2 / (6 + 2)
    assert abs(float(w.sum()) - 1.0) < 1e-6


def test_gate_weights_use_the_global_max():
    """max_val is the maximum over ALL experts (infer.cpp:104-110), here also the first pick."""
    e, w = R.moe_gate([-100.0, -101.0, -103.0], 2)
    assert e.tolist() == [0, 1]
    np.testing.assert_allclose(w, _softmax_sel([-100.0, -101.0]), rtol=1e-6)


# ---------------------------------------------------------------- 2. converter parity
def _header(path):
    d = open(path, "rb").read()
    n = struct.unpack("<Q", d[:8])[0]
    h = json.loads(d[8:8 + n])
    md = h.pop("__metadata__")
    return md, h, [k for k in h], d[8 + n:]


@pytest.mark.parametrize("dt", ["fp16", "fp8"])
def test_converter_matches_reference_on_mixtral(tmp_path, golden_dir, dt):
    """Our converter vs the reference convert.py's committed output on the same (seeded) HF
    Mixtral dir: identical metadata, tensor layout and data bytes."""
    hf = tmp_path / "hf"
    make_moe_golden.write_moe_hf_dir(str(hf))
    out = tmp_path / "out.yalm"
    convert.convert(str(hf), str(out), dt)
    md1, h1, k1, b1 = _header(os.path.join(golden_dir, f"tiny_moe_{dt}.yalm"))
    md2, h2, k2, b2 = _header(str(out))
    assert md1 == md2 and md1["n_experts"] == "4" and md1["n_experts_active"] == "2"
    assert k1 == k2
    assert h1 == h2
    assert b1 == b2


# ---------------------------------------------------------------- 3. configuration
def test_fixture_config_and_shapes_round_trip(golden_dir):
    yd = yalmfile.read_yalm(os.path.join(golden_dir, "tiny_moe_fp16.yalm"))
    cfg = M.config_from_metadata(yd.metadata)
    assert (cfg.dim, cfg.hidden_dim, cfg.n_layers, cfg.n_heads, cfg.n_kv_heads, cfg.vocab_size) == (
        64, 128, 2, 4, 2, 384)
    assert (cfg.n_experts, cfg.n_experts_active) == (4, 2)
    shapes = M.tensor_shapes(cfg)
    assert shapes["model.layers.1.moegate.weight"] == ((4, 64), False)
    assert shapes["model.layers.0.mlp.w1.weight"] == ((4, 128, 64), False)
    assert shapes["model.layers.0.mlp.w2.weight"] == ((4, 64, 128), False)
    for name, (shape, is_norm) in shapes.items():
        t = yd.tensors[name]
        assert t.shape == shape, name
        assert t.dtype == ("F32" if is_norm else "F16")
    assert set(yd.tensors) == set(shapes) | {"tokenizer.tokens"}
    md = cfg.metadata()
    assert {k: yd.metadata[k] for k in ("arch", "n_experts", "n_experts_active")} == {
        k: md[k] for k in ("arch", "n_experts", "n_experts_active")}
    assert M.config_from_metadata(md) == cfg
    yd.close()
    # dense configurations are untouched
    assert "n_experts" not in M.TINY.metadata() and M.config_from_metadata(M.TINY.metadata()).n_experts == 0


def test_mixtral_bytes_per_token_hand_sum():
    c = M.MIXTRAL_8X7B
    assert (c.dim, c.hidden_dim, c.n_layers, c.n_experts, c.n_experts_active) == (4096, 14336, 32, 8, 2)
    per_layer = 2 * 4096 * 4  # norms
    per_layer += (4096 + 2 * 1024) * 4096 * 2  # wq wk wv
    per_layer += 4096 * 4096 * 2  # wo
    per_layer += 8 * 4096 * 2  # router (model.cpp:86)
    per_layer += 2 * 3 * 4096 * 14336 * 2  # the two active experts (model.cpp:87)
    want = 32 * per_layer + 4096 * 2 + 4096 * 4 + 32000 * 4096 * 2
    assert c.weight_bytes_per_token() == want
    # all experts are resident: 8 x 3 matrices per layer
    dense = M.MISTRAL_7B
    extra = 32 * (7 * 3 * 4096 * 14336 * 2 + 8 * 4096 * 2)
    assert M.nbytes_model(c) == M.nbytes_model(dense) + extra
    with pytest.raises(ValueError):
        M.tp_check(c, 2)
    with pytest.raises(ValueError):
        M.tp_check(c.with_(n_experts_active=9), 1)
    with pytest.raises(ValueError):
        M.tp_check(c.with_(n_experts=65), 1)


# ---------------------------------------------------------------- 4. the C++ host
def test_host_accepts_mixtral_file(golden_dir):
    """The CLI loads the Mixtral fixture (Config::from_yalm, the 3-D expert shape checks of
    Block) and gets as far as the device: without a GPU that is the HIP-only error (or, for
    -d cpu, the CLI's own rejection), never a complaint about experts."""
    subprocess.run(["make", "-C", HOST, "-j4"], check=True, capture_output=True)
    r = subprocess.run([os.path.join(HOST, "yalm"), os.path.join(golden_dir, "tiny_moe_fp16.yalm"), "-d", "cpu",
                        "-i", "x"], capture_output=True)
    err = r.stderr.decode()
    assert r.returncode == 1 and "-d cpu" in err, err
    assert "expert" not in err and "tensor mismatch" not in err and "missing tensor" not in err, err


# ---------------------------------------------------------------- 5. routing margins
@pytest.mark.parametrize("case", R.FFN_CASES, ids=[c[0] for c in R.FFN_CASES])
def test_ffn_case_routing_margin(case):
    import oracle_py as O

    x, gate = R.ffn_case_router_inputs(case)
    np.testing.assert_array_equal(gate, R.ffn_case_inputs(case)[1]) if case[2] <= 2048 else None

    lg = O.matmul(x, gate, case[5])
    assert R.routing_margin(lg, case[4]) >= R.MARGIN, (case[0], np.sort(lg)[::-1])


@pytest.mark.parametrize("case", R.BLOCK_CASES, ids=[c[0] for c in R.BLOCK_CASES])
def test_block_case_routing_margin(case):
    K = case[1].n_experts_active
    worst = min(R.routing_margin(lg, K) for *_, lg in R.block_case_trace(case))
    assert worst >= R.MARGIN, (case[0], worst)


@pytest.mark.parametrize("case", R.FORWARD_CASES, ids=[c[0] for c in R.FORWARD_CASES])
def test_forward_case_routing_margin(case):
    K = case[1].n_experts_active
    steps, _, glogits = R.forward_case_trace(case)
    worst = min(R.routing_margin(lg, K) for s in steps for lg in s[5])
    worst = min(worst, min(R.routing_margin(lg, K) for rl, _ in glogits for lg in rl))
    assert worst >= R.MARGIN, (case[0], worst)


@pytest.mark.parametrize("fname", ["tiny_moe_fp16.yalm", "tiny_moe_fp8.yalm"])
def test_fixture_greedy_routing_margin(golden_dir, fname):
    cfg, t = R.yalm_tensors(os.path.join(golden_dir, fname))
    ref = R.MoeRef(cfg, t)
    tok, worst = 1, np.inf
    for pos in range(R.FIXTURE_GREEDY):
        lg = ref.forward(tok, pos)
        worst = min(worst, min(R.routing_margin(r, cfg.n_experts_active) for r in ref.router_logits))
        tok = int(np.argmax(lg))
    assert worst >= R.MARGIN, (fname, worst)
