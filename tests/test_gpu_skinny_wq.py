"""GPU: the native-weight skinny split-K GEMM (prefill_skinny_wq.h): fp8 (E5M2), e4m3 and q4 rows
streamed as stored at T <= 64 and turned into f16 MFMA fragments in registers.

1. yalm_gemm_wq against float64, and bit for bit against the f16 GEMM hook on the exact f16 twin
   and against the upcast form (skq:0).
2. whole dense decoders: default (native) against skq:0, every K / V cache row and the next
   decode step's logits bit for bit.

The f16 reference of 1: yalm_gemm_f16 runs the large-tile kernel, which sums K in one chain; the
skinny path sums each of its ks K chunks in a chain of its own and adds the chunks in order from
0 (skinny_reduce_kernel). So the twin's bits are 0 + gemm_f16 over chunk 0 + chunk 1 ...: for
ks = 1 gemm_f16(a, twin) itself. ks is the host's split (prefill.hip sk_pick_ks): chunks of a
multiple of 256 columns, at most 32 KB of A rows, the fewest that give 512 workgroups, else the
most."""
import functools

import numpy as np
import pytest

import arch_cases as A
import qknorm_cases as Q
from yalm_amd import models as M

pytestmark = pytest.mark.gpu


def rt():
    from yalm_amd import runtime

    return runtime


def sk_ks(N, K, m):
    tp = 16 * ((m + 15) // 16)
    ok = [s for s in range(1, K // 256 + 1) if K % s == 0 and (K // s) % 256 == 0 and tp * (K // s) * 2 <= 32768]
    return next((s for s in ok if N // 64 * s >= 512), ok[-1])


@functools.lru_cache(maxsize=2)
def weights(dtype, N, K, kind):
    """(stored rows, exact f16 twin). kind "int": small integers with unit scales; "edge": random
    codes over the whole format (no inf / NaN) with the extreme codes and scales forced in."""
    rng = np.random.default_rng(1000 * dtype + N + K)
    r, g = np.arange(N)[:, None], np.arange(K // 32)[None, :]
    if kind == "int":
        v = rng.integers(-4, 5, size=(N, K))
        if dtype == M.F8E5M2:
            w = M.encode_weights(v.astype(np.float32), M.F8E5M2)
        elif dtype == M.E4M3:
            w = M.e4m3_pack(M.e4m3_encode(v), np.ones(N, np.float32))
        else:
            w = M.q4_pack(v + 8, np.full((N, K // 32), 0x3C00, np.uint16))
    elif dtype == M.Q4:  # every row and group its own restricted scale in [2^-6, 4); nibbles 0 and 15
        u = rng.integers(0, 16, size=(N, K))
        u[:, 0], u[:, 1] = 0, 15
        w = M.q4_pack(u, ((9 + (r + g) % 8) << 10 | ((131 * r + 17 * g) % 128) << 3).astype(np.uint16))
    else:
        w = rng.integers(0, 256, size=(N, K)).astype(np.uint8)
        if dtype == M.F8E5M2:  # exponent 31 (inf / NaN) -> 15; +-0, subnormals, +-57344
            w[(w & 0x7C) == 0x7C] ^= 0x40
            w[:, :6] = [0x00, 0x80, 0x01, 0x83, 0x7B, 0xFB]
        else:  # NaN codes -> 448; +-0, subnormals, +-448; scales 2^-15 .. 2^7 over the rows
            w[(w & 0x7F) == 0x7F] ^= 0x01
            w[:, :6] = [0x00, 0x80, 0x01, 0x87, 0x7E, 0xFE]
            w = M.e4m3_pack(w, np.ldexp(1.0, -15 + np.arange(N) % 23).astype(np.float32))
    twin = M.decode_weights(w, dtype, (N, K))
    assert np.isfinite(twin).all() and (twin.astype(np.float16) == twin).all()
    return w, twin.astype(np.float16)


def twin_bits(a, twin, ks):
    """The f16 path's result on the twin, by yalm_gemm_f16 per K chunk (N padded to its 128)."""
    pad = np.zeros((-twin.shape[0] % 128, twin.shape[1]), np.float16)
    c = np.zeros((a.shape[0], twin.shape[0] + pad.shape[0]), np.float32)
    for ka, kw in zip(np.split(a, ks, axis=1), np.split(np.vstack([twin, pad]), ks, axis=1)):
        c = c + rt().gemm_f16(ka, kw)
    return c[:, : twin.shape[0]]


# (N, K): one workgroup, one chunk of one stage (fewer than the ring's 3) | ks 2 | q4's scale tail
# past one 16-byte line, ks 4 | at m <= 16 one chunk of 4 stages: the ring wraps (ks 2, 4 above)
SHAPES = [(64, 256), (192, 512), (128, 1024), (32768, 1024)]
CASES = [(N, K, "edge") for N, K in SHAPES] + [(192, 512, "int")]


@pytest.mark.parametrize("m", [1, 16, 17, 64])
@pytest.mark.parametrize("N,K,kind", CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("dtype", [M.F8E5M2, M.E4M3, M.Q4], ids=["fp8", "e4m3", "q4"])
def test_gemm_wq(dtype, N, K, kind, m):
    R = rt()
    w, twin = weights(dtype, N, K, kind)
    rng = np.random.default_rng(m + K)
    a = (rng.integers(-4, 5, size=(m, K)) if kind == "int" else rng.standard_normal((m, K))).astype(np.float16)
    a64, w64 = a.astype(np.float64), twin.astype(np.float64)
    ref, bound = a64 @ w64.T, K * 2.0 ** -23 * (np.abs(a64) @ np.abs(w64).T)
    c, native = R.gemm_wq(a, w, dtype)
    assert native
    print(f"max |c - ref64| / bound = {np.max(np.abs(c - ref) / np.maximum(bound, 1e-300)):.3f}")
    assert (np.abs(c - ref) <= bound).all()
    if kind == "int":
        np.testing.assert_array_equal(c.astype(np.float64), ref)
    np.testing.assert_array_equal(c.view(np.uint32), twin_bits(a, twin, sk_ks(N, K, m)).view(np.uint32))
    R.set_gemm_forms("skq:0")
    try:
        c0, native0 = R.gemm_wq(a, w, dtype)
    finally:
        R.set_gemm_forms("")
    assert not native0
    np.testing.assert_array_equal(c0.view(np.uint32), c.view(np.uint32))
    if m == 64 and N == 192:  # one more row: the large tiles over the upcast
        a65 = np.vstack([a, a[:1]])
        c65, native65 = R.gemm_wq(a65, w, dtype)
        assert not native65
        assert (np.abs(c65[:64] - ref) <= bound).all() and (np.abs(c65[64] - ref[0]) <= bound[0]).all()


ARCH = {"plain": M.SMALL, "bias": A.CASES["bias-small-f16"][0], "qknorm": Q.CASES["small-f16"][0]}


@functools.lru_cache(maxsize=None)
def model(dtype, arch):
    c = ARCH[arch].with_(weight_dtype=dtype, max_seq_len=96)
    return c, M.synth_host_tensors(c, seed=7)


@pytest.mark.parametrize("pos0", [0, 5])
@pytest.mark.parametrize("n", [1, 13, 64])
@pytest.mark.parametrize("dtype,arch", [(M.F8E5M2, "plain"), (M.E4M3, "plain"), (M.Q4, "plain"), (M.E4M3, "bias"),
                                        (M.Q4, "qknorm")], ids=["fp8", "e4m3", "q4", "e4m3-bias", "q4-qknorm"])
def test_decoder_native_equals_upcast(dtype, arch, n, pos0):
    R = rt()
    c, t = model(dtype, arch)
    dm = R.DeviceModel.from_arrays(c, t)
    kvb = c.max_seq_len * c.kv_dim * 2
    caches = [[R.lib.yalm_alloc(kvb) for _ in range(2 * c.n_layers)] for _ in range(2)]
    decs = [R.Decoder(dm, kv_caches=list(zip(cs[0::2], cs[1::2]))) for cs in caches]
    decs[1].set_prefill_forms("skq:0")
    try:
        tokens = np.random.default_rng(n + pos0).integers(0, c.vocab_size, size=pos0 + n + 1).astype(np.int32)
        logits = []
        for d in decs:
            if pos0:
                d.prefill(tokens[:pos0], logprobs=False)
            d.prefill(tokens[pos0: pos0 + n], pos0=pos0, logprobs=False)
            assert d.prefill_info()[0] == 1
            logits.append(d.forward(int(tokens[pos0 + n]), pos0 + n))
        np.testing.assert_array_equal(logits[0].view(np.uint32), logits[1].view(np.uint32))
        rows = (pos0 + n + 1) * c.kv_dim * 2
        for p0, p1 in zip(*caches):
            k0, k1 = np.empty(rows, np.uint8), np.empty(rows, np.uint8)
            R.check(R.lib.yalm_download(k0.ctypes.data, p0, rows))
            R.check(R.lib.yalm_download(k1.ctypes.data, p1, rows))
            np.testing.assert_array_equal(k0, k1)
    finally:
        for h in decs + [dm]:
            h.close()
        for p in caches[0] + caches[1]:
            R.lib.yalm_free(p)
