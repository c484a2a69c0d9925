"""CPU: the e4m3 weight format (include/yalm_hip.h "e4m3") -- code table, quantiser, scale
limits, the exact f16 twin, its error against E5M2, the host arithmetic of the ABI, the
converter and the synthetic rule. No device is touched."""
import ctypes

import numpy as np
import pytest
import torch

from golden import make_golden
from yalm_amd import convert, models as M, yalmfile


def _torch_codes(v):
    """torch.float8_e4m3fn of float32 values, as bytes."""
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def test_code_table_equals_torch():
    t = M.e4m3_table()
    ref = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).to(torch.float32).numpy()
    assert t.dtype == np.float32 and t.shape == (256,)
    assert np.flatnonzero(np.isnan(t)).tolist() == [0x7F, 0xFF]
    assert np.flatnonzero(np.isnan(ref)).tolist() == [0x7F, 0xFF]
    fin = ~np.isnan(t)
    np.testing.assert_array_equal(t[fin].view(np.uint32), ref[fin].view(np.uint32))  # (-0.0 at 0x80 included)
    assert t[0x7E] == 448.0 and t[0xFE] == -448.0 and t[0x01] == 2.0 ** -9 and t[0x08] == 2.0 ** -6


def _check_quantised(w):
    """The quantiser's contract on an f16 matrix (rows, n); returns the rows' k."""
    n = w.shape[1]
    q = M.e4m3_quantize(w)
    assert q.dtype == np.uint8 and q.shape == (w.shape[0], n + 16) and M.row_bytes(M.E4M3, n) == n + 16
    codes, s = M.e4m3_unpack(q, n)
    assert not q[:, n + 4:].any(), "the 12 bytes after the scale are zero"
    assert not np.any((codes & 0x7F) == 0x7F), "the quantiser never emits NaN"
    k = np.log2(s.astype(np.float64))
    assert np.all(k == np.rint(k)) and k.min() >= -15 and k.max() <= 7
    w64 = w.astype(np.float64)
    amax = np.abs(w64).max(axis=1)
    with np.errstate(divide="ignore"):
        want = np.where(amax > 0, np.clip(np.ceil(np.log2(amax / 448.0)), -15, 7), 0)
    np.testing.assert_array_equal(k, want)
    # codes: torch's cast of w / 2^k (exact in f32: a power-of-two scaling of an f16), saturated as the format says
    scaled = np.clip((w64 / s.astype(np.float64)[:, None]), -448.0, 448.0).astype(np.float32)
    np.testing.assert_array_equal(codes, _torch_codes(scaled))
    d = M.e4m3_dequantize(q, n).astype(np.float64)
    sk = s.astype(np.float64)[:, None] * np.ones_like(w64)
    sat = np.abs(w64) > 448.0 * sk
    big = (np.abs(w64) >= 2.0 ** -6 * sk) & ~sat
    small = np.abs(w64) < 2.0 ** -6 * sk
    assert np.all(np.abs(w64 - d)[big] <= 2.0 ** -4 * np.abs(w64)[big])  # half an ulp of 3 mantissa bits
    assert np.all(np.abs(w64 - d)[small] <= 2.0 ** -10 * sk[small])  # half a subnormal step
    assert np.all(np.abs(d[sat]) == 448.0 * sk[sat])
    return k


@pytest.mark.parametrize("scale", [1e-5, 1e-3, 0.035, 1.0, 300.0, 9e3])
def test_quantiser_random_f16(scale):
    rng = np.random.default_rng(int(scale * 1e6) % 1000 + 1)
    w = (rng.standard_normal((16, 256)) * scale * rng.uniform(0.2, 2.0, (16, 1))).astype(np.float16)
    _check_quantised(w)


def test_scale_limits():
    n = 32
    w = np.zeros((5, n), np.float16)
    w[1, :4] = [57312.0, -3.0, 1e-3, 100.0]  # the f16 just below 448 * 2^7 = 57344
    w[2, :4] = [-57376.0, 65504.0, 7.0, -1e-4]  # just above it: k stays 7, 448 * 128 saturates
    w[3, :4] = [0.013, -6e-8, 3e-5, 1e-6]  # amax below 448 * 2^-15 = 0.013672: k stays -15
    w[4, :4] = [448.0 * 2.0 ** -15, 0.0, -2.0 ** -24, 2.0 ** -15]  # exactly 448 * 2^-15
    k = _check_quantised(w)
    np.testing.assert_array_equal(k, [0, 7, 7, -15, -15])
    q = M.e4m3_quantize(w)
    codes, s = M.e4m3_unpack(q, n)
    assert not codes[0].any() and s[0] == 1.0  # an all-zero row: k = 0, every code +0
    d = M.e4m3_dequantize(q, n)
    assert d[2, 0] == -57344.0 and d[2, 1] == 57344.0  # saturated to +-448 * 2^7
    assert d[1, 0] == 57344.0  # 57312 rounds up to 448 * 128 without saturation
    assert d[4, 0] == np.float32(448.0 * 2.0 ** -15)


def test_twin_is_exact():
    """code * 2^k is an exact f16 for every finite code at k = -15, 0, 7 (the range's ends), and
    not for every code one step outside it."""
    t = M.e4m3_table().astype(np.float64)
    fin = ~np.isnan(t)
    with np.errstate(over="ignore"):
        for k in (-15, 0, 7):
            v = t[fin] * 2.0 ** k
            assert np.all(v.astype(np.float16).astype(np.float64) == v), k
        for k in (-16, 8):
            v = t[fin] * 2.0 ** k
            assert not np.all(v.astype(np.float16).astype(np.float64) == v), k
    # e4m3_twin on a model: every matrix an f16 equal to the dequantised value
    cfg = M.TINY.with_(weight_dtype=M.E4M3)
    rng = np.random.default_rng(5)
    tens = {}
    for name, (shape, is_norm) in M.tensor_shapes(cfg).items():
        v = rng.standard_normal(shape).astype(np.float32) * 0.05
        tens[name] = (1.0 + v) if is_norm else M.encode_weights(v, M.E4M3)
    c16, t16 = M.e4m3_twin(cfg, tens)
    assert c16.weight_dtype == M.F16
    for name, (shape, is_norm) in M.tensor_shapes(cfg).items():
        if is_norm:
            continue
        assert t16[name].dtype == np.float16 and t16[name].shape == shape
        np.testing.assert_array_equal(t16[name].astype(np.float32), M.decode_weights(tens[name], M.E4M3, shape))


def test_rms_error_below_e5m2_on_realistic_small():
    t = M.synth_host_tensors(M.SMALL, real=M.REALISTIC)
    worst, count = 0.0, 0
    for name, (shape, is_norm) in M.tensor_shapes(M.SMALL).items():
        if is_norm:
            continue
        w = t[name].astype(np.float64)
        e4 = M.e4m3_dequantize(M.e4m3_quantize(t[name]), shape[1]).astype(np.float64)
        e5 = M.e5m2_to_f32(M.encode_weights(t[name].astype(np.float32), M.F8E5M2)).astype(np.float64)
        r4, r5 = np.sqrt(np.mean((w - e4) ** 2)), np.sqrt(np.mean((w - e5) ** 2))
        assert r4 < r5, (name, r4, r5)
        worst = max(worst, r4 / r5)
        count += 1
    print(f"rms error e4m3 / E5M2 over {count} matrices: at most {worst:.3f}")
    assert count == 30


def test_row_bytes_and_model_bytes():
    assert M.row_bytes(M.E4M3, 16) == 32 and M.row_bytes(M.E4M3, 4096) == 4112
    with pytest.raises(ValueError):
        M.row_bytes(M.E4M3, 40)
    assert M.matrix_bytes(M.E4M3, (7, 64)) == 7 * 80
    c = M.MISTRAL_7B.with_(weight_dtype=M.E4M3)
    c8 = M.MISTRAL_7B.with_(weight_dtype=M.F8E5M2)
    r = c.weight_bytes_per_token() / c8.weight_bytes_per_token()
    assert 1.0 < r < 1.004  # 16 bytes per row: 0.4 % at n = 4096, 0.1 % at 14336
    assert M.nbytes_model(M.TINY.with_(weight_dtype=M.E4M3)) > M.nbytes_model(M.TINY.with_(weight_dtype=M.F8E5M2))
    assert M.DTYPE_NAMES["e4m3"] == M.E4M3 == 17


def test_row_bytes_abi():
    from yalm_amd import runtime

    assert "yalm_synth_e4m3" in runtime.EXPORTED
    for n in (16, 48, 1040, 2048, 4096, 14336):
        assert runtime.lib.yalm_row_bytes(17, n) == n + 16 == M.row_bytes(M.E4M3, n)
    for n in (8, 40, 4100, 0, -16):
        assert runtime.lib.yalm_row_bytes(17, n) == 0
    assert ctypes.sizeof(ctypes.c_size_t) == 8


def test_plans_are_fp8s():
    from yalm_amd import runtime as R

    for cfg in (M.MISTRAL_7B, M.LLAMA_32_3B, M.QWEN3_8B, M.SMALL, M.TINY):
        for n, groups in ((cfg.dim, (cfg.q_dim + 2 * cfg.kv_dim) // 2), (cfg.q_dim, (cfg.dim + 1) // 2),
                          (cfg.dim, cfg.hidden_dim), (cfg.hidden_dim, (cfg.dim + 1) // 2),
                          (cfg.dim, (cfg.vocab_size + 1) // 2)):
            for T in (1, 2, 3, 4):
                assert R.rows_plan(M.E4M3, n, groups, T, 256) == R.rows_plan(M.F8E5M2, n, groups, T, 256)

    def plan(cfg):
        cc = R.Config.from_model(cfg)
        return R.lib.yalm_attn_wo_plan(ctypes.byref(cc), 512, None, None)

    assert plan(M.MISTRAL_7B.with_(weight_dtype=M.E4M3)) == 1
    assert plan(M.MISTRAL_7B.with_(weight_dtype=M.F8E5M2)) == 1
    # a 2048-byte Wo row: fused for E5M2 (a tensor-parallel rank's), not for e4m3 (one GPU only)
    half = M.MISTRAL_7B.with_(n_heads=16, n_kv_heads=4)
    assert plan(half.with_(weight_dtype=M.F8E5M2)) == 1
    assert plan(half.with_(weight_dtype=M.E4M3)) == 0


def test_yalm_file_roundtrip(tmp_path):
    cfg = M.TINY.with_(weight_dtype=M.E4M3)
    rng = np.random.default_rng(3)
    t = {}
    for name, (shape, is_norm) in M.tensor_shapes(cfg).items():
        v = rng.standard_normal(shape).astype(np.float32) * 0.05
        t[name] = (1.0 + v) if is_norm else M.encode_weights(v, M.E4M3)
    assert cfg.metadata()["dtype"] == "e4m3"
    p = tmp_path / "m.yalm"
    yalmfile.write_yalm(str(p), t, cfg.metadata())
    yd = yalmfile.read_yalm(str(p))
    got = M.config_from_metadata(yd.metadata)
    assert got.weight_dtype == M.E4M3 and got.dim == cfg.dim
    for name, (shape, is_norm) in M.tensor_shapes(cfg).items():
        tt = yd.tensors[name]
        if is_norm:
            assert tt.dtype == "F32"
        else:
            assert tt.dtype == "U8" and tuple(tt.shape) == (shape[0], shape[1] + 16)
        np.testing.assert_array_equal(np.asarray(tt.data).reshape(t[name].shape), t[name])
    yd.close()


def test_convert_e4m3(tmp_path):
    """convert.py --dtype e4m3 on the checkpoint the golden tiny_fp16.yalm is made from: the
    metadata says e4m3, every matrix is e4m3_quantize of the fp16 conversion's."""
    hf = tmp_path / "hf"
    make_golden.write_hf_dir(str(hf))
    convert.convert(str(hf), str(tmp_path / "e4m3.yalm"), "e4m3")
    convert.convert(str(hf), str(tmp_path / "f16.yalm"), "fp16")
    ye, yf = yalmfile.read_yalm(str(tmp_path / "e4m3.yalm")), yalmfile.read_yalm(str(tmp_path / "f16.yalm"))
    cfg = M.config_from_metadata(ye.metadata)
    assert cfg.weight_dtype == M.E4M3 and ye.metadata["dtype"] == "e4m3"
    assert ye.tensors["tokenizer.tokens"].data.tobytes() == yf.tensors["tokenizer.tokens"].data.tobytes()
    n_mat = 0
    for name, (shape, is_norm) in M.tensor_shapes(cfg).items():
        a, b = ye.tensors[name], yf.tensors[name]
        if is_norm:
            np.testing.assert_array_equal(np.asarray(a.data), np.asarray(b.data))
            continue
        assert a.dtype == "U8" and tuple(a.shape) == (shape[0], shape[1] + 16)
        rows = np.asarray(a.data).reshape(a.shape)
        f16 = np.asarray(b.data).reshape(shape)
        np.testing.assert_array_equal(rows, M.e4m3_quantize(f16))
        np.testing.assert_array_equal(M.e4m3_dequantize(rows, shape[1]),
                                      M.e4m3_dequantize(M.e4m3_quantize(f16), shape[1]))
        n_mat += 1
    assert n_mat > 0
    ye.close()
    yf.close()
    with pytest.raises(ValueError, match="e4m3"):
        convert.metadata_from_config(dict(architectures=["MixtralForCausalLM"]), "e4m3")


def test_synthetic_rule():
    cfg = M.SMALL.with_(weight_dtype=M.E4M3, n_layers=1, vocab_size=256)
    a, b = M.synth_host_tensors(cfg, seed=4), M.synth_host_tensors(cfg, seed=4)
    c = M.synth_host_tensors(cfg, seed=5)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
    assert any(not np.array_equal(a[k], c[k]) for k in a)
    _, twin = M.e4m3_twin(cfg, a)
    for name, (shape, is_norm) in M.tensor_shapes(cfg).items():
        assert np.isfinite(twin[name].astype(np.float32)).all()
        if is_norm:
            continue
        codes, s = M.e4m3_unpack(a[name], shape[1])
        assert not np.any((codes & 0x7F) == 0x7F), "no NaN code"
        assert len(np.unique(codes)) == 254
        k = np.log2(s.astype(np.float64))
        assert np.all(k == np.rint(k)) and np.all(k >= -15) and np.all(k <= 7)
        scale = M.synth_params(name, False)[0]
        assert np.all(448.0 * s >= scale) and np.all(448.0 * s / 2 < scale)  # 448 at or just above scale
        assert not a[name][:, shape[1] + 4:].any()
    assert M.synth_e4m3_scale(1e-9) == np.float32(2.0 ** -15) and M.synth_e4m3_scale(1e9) == np.float32(2.0 ** 7)
    assert M.synth_e4m3_scale(448.0) == 1.0 and M.synth_e4m3_scale(448.5) == 2.0
    with pytest.raises(ValueError):
        M.synth_host_tensors(cfg, real=M.REALISTIC)
