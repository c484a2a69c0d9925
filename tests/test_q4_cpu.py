"""CPU: the q4 weight format (include/yalm_hip.h "q4") -- quantiser, packing, files, the
synthetic rule and the row-bytes ABI. No device is touched."""
import ctypes

import numpy as np
import pytest

from golden import make_golden
from yalm_amd import convert, models as M, yalmfile

F16_MAX = 65504.0


def _groups(w):
    return np.asarray(w, np.float64).reshape(w.shape[0], -1, 32)


def _check_quantised(w):
    """The quantiser's contract on a float matrix (rows, n)."""
    n = w.shape[1]
    q = M.q4_quantize(w)
    assert q.dtype == np.uint8 and q.shape == (w.shape[0], M.row_bytes(M.Q4, n))
    u, sb = M.q4_unpack(q, n)
    s = sb.view(np.float16).astype(np.float64)
    amax = np.abs(_groups(w)).max(axis=2)
    assert np.all(sb & 7 == 0), "scale bits: low 3 mantissa bits must be zero"
    assert np.all(7.0 * s >= amax)
    # the smallest such scale: the restricted value below (8 less in the bit pattern) does not cover amax
    below = np.maximum(sb.astype(np.int64) - 8, 0).astype(np.uint16).view(np.float16).astype(np.float64)
    assert np.all((sb == 0) | (7.0 * below < amax))
    assert np.all(u[np.repeat(sb, 32, axis=1) == 0] == 8), "an all-zero group is s = 0, u = 8"
    assert u.min() >= 1 and u.max() <= 15, "the quantiser clips to -7 .. 7"
    d = M.q4_dequantize(q, n)
    assert d.dtype == np.float32
    assert np.all(np.abs(_groups(w) - _groups(d)) <= s[:, :, None] / 2)
    return sb


def _check_all_nibbles_exact(scale_bits):
    """(u - 8) * s for all 16 nibbles of every scale: exact in f32 always, and an exact f16
    wherever it lies inside f16's range (|8 s| <= 65504; a larger scale needs a group maximum
    above 7 * 8184 = 57288, and its f16 twin saturates)."""
    sb = np.unique(scale_bits)
    s = sb.view(np.float16).astype(np.float64)
    v = (np.arange(16, dtype=np.float64)[None, :] - 8.0) * s[:, None]
    assert np.all(v.astype(np.float32).astype(np.float64) == v)
    fits = np.abs(v) <= F16_MAX
    assert np.all(fits[8.0 * s <= F16_MAX])
    with np.errstate(over="ignore"):
        assert np.all(v.astype(np.float16).astype(np.float64)[fits] == v[fits])


@pytest.mark.parametrize("scale", [1e-5, 1e-3, 0.035, 1.0, 300.0, 9e3])
def test_quantiser_gaussian(scale):
    rng = np.random.default_rng(int(scale * 1e6) % 1000 + 1)
    w = (rng.standard_normal((16, 256)) * scale).astype(np.float32)
    sb = _check_quantised(w)
    _check_all_nibbles_exact(sb)


def test_quantiser_constructed_cases():
    rng = np.random.default_rng(5)
    w = (rng.standard_normal((6, 64)) * 0.02).astype(np.float32)
    w[0, :32] = 0.0  # an all-zero group
    w[1, 32:] = 0.0
    w[1, 40] = 3.0  # one outlier in an otherwise zero group
    w[2, 7] = -50.0  # one outlier among small values
    s0 = np.array([0x2C08], np.uint16).view(np.float16).astype(np.float32)[0]  # a restricted scale value
    w[3, :32] = 0.0
    w[3, 3] = 7.0 * s0  # amax exactly on 7 x a scale value: that scale is chosen
    w[4, :32] = np.linspace(-F16_MAX, F16_MAX, 32)  # values up to the f16 maximum
    w[5, :] = 6e-8  # inside the f16 subnormals
    sb = _check_quantised(w)
    assert sb[0, 0] == 0 and sb[1, 0] != 0
    assert sb[3, 0] == 0x2C08
    u, _ = M.q4_unpack(M.q4_quantize(w), 64)
    assert u[1, 40] == 15 and np.all(np.delete(u[1, 32:], 8) == 8)
    assert u[2, 7] == 1
    _check_all_nibbles_exact(sb)
    # every scale the format allows below the f16 range limit, not only those produced above
    every = np.arange(0, 0x7C00, 8, dtype=np.uint16)
    _check_all_nibbles_exact(every)


@pytest.mark.parametrize("n", [32, 64, 2048, 3072])
def test_pack_roundtrip_and_padding(n):
    rng = np.random.default_rng(n)
    u = rng.integers(0, 16, (5, n), dtype=np.uint8)
    sb = (rng.integers(0, 0x7C00 // 8, (5, n // 32)) * 8).astype(np.uint16)
    a = M.q4_pack(u, sb)
    rb = M.row_bytes(M.Q4, n)
    assert rb % 16 == 0 and rb >= n // 2 + n // 16 and rb - (n // 2 + n // 16) < 16
    assert a.shape == (5, rb)
    u2, sb2 = M.q4_unpack(a, n)
    np.testing.assert_array_equal(u2, u)
    np.testing.assert_array_equal(sb2, sb)
    assert not a[:, n // 2 + n // 16:].any(), "padding must be zero"
    # the documented position of element e: word e / 8 of its block, nibble (i >> 1) + 4 (i & 1), i = e % 8
    words = np.ascontiguousarray(a[:, : n // 2]).view("<u4")
    for e in (0, 1, 2, 7, 8, 31, n - 1):
        i = e % 8
        got = (words[:, e // 8] >> np.uint32(4 * ((i >> 1) + 4 * (i & 1)))) & 15
        np.testing.assert_array_equal(got, u[:, e])


def test_row_bytes_values():
    assert M.row_bytes(M.Q4, 32) == 32 and M.row_bytes(M.Q4, 64) == 48
    assert M.row_bytes(M.Q4, 4096) == 2304 and M.row_bytes(M.Q4, 2080) == 1184
    assert M.row_bytes(M.F16, 100) == 200 and M.row_bytes(M.F32, 100) == 400 and M.row_bytes(M.F8E5M2, 100) == 100
    with pytest.raises(ValueError):
        M.row_bytes(M.Q4, 48)
    c = M.MISTRAL_7B.with_(weight_dtype=M.Q4)
    # 9/16 byte per weight
    assert abs(c.weight_bytes_per_token() / M.MISTRAL_7B.weight_bytes_per_token() - 9 / 32) < 1e-3
    assert M.nbytes_model(M.TINY.with_(weight_dtype=M.Q4)) < M.nbytes_model(M.TINY.with_(weight_dtype=M.F8E5M2))


def test_yalm_file_roundtrip(tmp_path):
    cfg = M.TINY.with_(weight_dtype=M.Q4)
    rng = np.random.default_rng(3)
    t = {}
    for name, (shape, is_norm) in M.tensor_shapes(cfg).items():
        v = rng.standard_normal(shape).astype(np.float32) * 0.05
        t[name] = (1.0 + v) if is_norm else M.encode_weights(v, M.Q4)
    assert cfg.metadata()["dtype"] == "q4"
    p = tmp_path / "m.yalm"
    yalmfile.write_yalm(str(p), t, cfg.metadata())
    yd = yalmfile.read_yalm(str(p))
    got = M.config_from_metadata(yd.metadata)
    assert got.weight_dtype == M.Q4 and got.dim == cfg.dim
    for name, (shape, is_norm) in M.tensor_shapes(cfg).items():
        tt = yd.tensors[name]
        if is_norm:
            assert tt.dtype == "F32"
        else:
            assert tt.dtype == "U8" and tuple(tt.shape) == (shape[0], M.row_bytes(M.Q4, shape[1]))
        np.testing.assert_array_equal(np.asarray(tt.data).reshape(t[name].shape), t[name])
    yd.close()
    c16, t16 = M.q4_twin(cfg, t)
    assert c16.weight_dtype == M.F16
    for name, (shape, is_norm) in M.tensor_shapes(cfg).items():
        if not is_norm:
            assert t16[name].dtype == np.float16 and t16[name].shape == shape
            np.testing.assert_array_equal(t16[name].astype(np.float32), M.decode_weights(t[name], M.Q4, shape))


def test_convert_q4_against_fp16_conversion(tmp_path):
    hf = tmp_path / "hf"
    make_golden.write_hf_dir(str(hf))
    convert.convert(str(hf), str(tmp_path / "q4.yalm"), "q4")
    convert.convert(str(hf), str(tmp_path / "f16.yalm"), "fp16")
    yq, yf = yalmfile.read_yalm(str(tmp_path / "q4.yalm")), yalmfile.read_yalm(str(tmp_path / "f16.yalm"))
    cfg = M.config_from_metadata(yq.metadata)
    assert cfg.weight_dtype == M.Q4 and yq.metadata["dtype"] == "q4"
    assert yq.tensors["tokenizer.tokens"].data.tobytes() == yf.tensors["tokenizer.tokens"].data.tobytes()
    for name, (shape, is_norm) in M.tensor_shapes(cfg).items():
        a, b = yq.tensors[name], yf.tensors[name]
        if is_norm:
            np.testing.assert_array_equal(np.asarray(a.data), np.asarray(b.data))
            continue
        assert a.dtype == "U8" and tuple(a.shape) == (shape[0], M.row_bytes(M.Q4, shape[1]))
        rows = np.asarray(a.data).reshape(a.shape)
        ref = np.asarray(b.data).reshape(shape).astype(np.float64)
        _, sb = M.q4_unpack(rows, shape[1])
        s = sb.view(np.float16).astype(np.float64)
        d = M.q4_dequantize(rows, shape[1]).astype(np.float64)
        assert np.all(np.abs(_groups(ref) - _groups(d)) <= s[:, :, None] / 2), name
    yq.close()
    yf.close()
    with pytest.raises(ValueError):
        convert.metadata_from_config(dict(architectures=["MixtralForCausalLM"]), "q4")


def test_synthetic_rule():
    cfg = M.SMALL.with_(weight_dtype=M.Q4, n_layers=1, vocab_size=256)
    a, b = M.synth_host_tensors(cfg, seed=4), M.synth_host_tensors(cfg, seed=4)
    c = M.synth_host_tensors(cfg, seed=5)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
    assert any(not np.array_equal(a[k], c[k]) for k in a)
    _, twin = M.q4_twin(cfg, a)
    for name, (shape, is_norm) in M.tensor_shapes(cfg).items():
        assert np.isfinite(twin[name].astype(np.float32)).all()
        if is_norm:
            continue
        u, sb = M.q4_unpack(a[name], shape[1])
        want = M.q4_restrict_scale((np.float32(M.WEIGHT_SCALE) / np.float32(7.0)).astype(np.float16).view(np.uint16))
        assert np.all(sb == want) and want & 7 == 0
        assert len(np.unique(u)) == 16
        assert not a[name][:, shape[1] // 2 + shape[1] // 16:].any()
    with pytest.raises(ValueError):
        M.synth_host_tensors(cfg, real=M.REALISTIC)


def test_row_bytes_abi():
    """yalm_row_bytes agrees with models.row_bytes (pure host arithmetic: no device)."""
    from yalm_amd import runtime

    assert "yalm_row_bytes" in runtime.EXPORTED and "yalm_synth_q4" in runtime.EXPORTED
    for dt in (M.F32, M.F16, M.F8E5M2, M.Q4):
        for n in (32, 64, 2048, 2080, 3072, 4096, 14336):
            assert runtime.lib.yalm_row_bytes(dt, n) == M.row_bytes(dt, n), (dt, n)
    assert runtime.lib.yalm_row_bytes(M.Q4, 48) == 0 and runtime.lib.yalm_row_bytes(7, 64) == 0
    assert runtime.lib.yalm_row_bytes(M.F16, 0) == 0
    assert isinstance(runtime.lib.yalm_row_bytes(M.Q4, 64), int) and ctypes.sizeof(ctypes.c_size_t) == 8
