"""The q8 kv shadow (attention_q8.h) on the device: the quantiser bit for bit against
models.kv_q8_quantize, attn_decode_q8_kernel against float64 attention over the exact values it
reads, a whole q8 decoder against a float64 restatement over the rows the device stored, and the
refusals."""
import zlib

import numpy as np
import pytest

import attn_ref as A
from ref_numpy import RefModel
from ref_numpy import rmsnorm as ref_rmsnorm, rope as ref_rope, silu as ref_silu
from yalm_amd import models as M
from yalm_amd import runtime

pytestmark = pytest.mark.gpu
N_KV = 2


def _poison(a, n, kind):
    """Rows >= n (msl, n_kv, D): all NaN or all +inf, and in both cases one +inf per head row, so that
    the hook's quantiser gives every such shadow row an inf scale (fmaxf drops NaN: an all-NaN row
    alone would quantise to scale 0) and codes from inf * 0."""
    u = a.view(np.uint16)
    u[n:] = A.POISONS[kind]
    u[n:, :, 0] = A.POISONS["inf"]


@pytest.mark.parametrize("D", [64, 128])
def test_quantiser_bits(D):
    rows, nkv = 70, 3
    rng = np.random.default_rng(D)
    K = (rng.standard_normal((rows, nkv, D)) * rng.uniform(0.01, 30, (rows, nkv, 1))).astype(np.float16)
    V = rng.standard_normal((rows, nkv, D)).astype(np.float16)
    K[3, 1] = 0                                        # an all-zero head row
    K[4, 0, 5] = 65504                                 # the largest f16
    V[5, 2] = 0
    V[5, 2].view(np.uint16)[:] = rng.integers(0, 1024, D)   # subnormals only
    half = np.arange(D) % 11 - 5 + 0.5                 # a = 127: inv = 1 and x * inv lands on .5
    K[6, 2], V[6, 0] = half, -half
    K[6, 2, 0] = V[6, 0, 0] = 127
    q = rng.standard_normal((nkv, D)).astype(np.float32)
    _, kc, ks, vc, vs = runtime.mha_q8(K, V, q, D, 0, rows - 1, rows, rows, nkv, nkv)
    for got_c, got_s, x in ((kc, ks, K), (vc, vs, V)):
        want_c, want_s = M.kv_q8_quantize(x)
        np.testing.assert_array_equal(got_c, want_c)
        np.testing.assert_array_equal(got_s.view(np.uint32), want_s.view(np.uint32))


def _case(D, G, msl, n, seed):
    """f16 caches with one dominant key per head and poison past n, and q."""
    rng = np.random.default_rng(zlib.crc32(f"{D}-{G}-{msl}-{n}-{seed}".encode()))
    K = rng.standard_normal((msl, N_KV, D)).astype(np.float16)
    V = rng.standard_normal((msl, N_KV, D)).astype(np.float16)
    q = (rng.standard_normal((N_KV * G, D)) * 2).astype(np.float32)
    for h in range(N_KV * G):   # score 9 above the random keys' ~N(0, 4)
        K[(h * 37 + 5) % n, h // G] = (q[h] * (9 * np.sqrt(D) / float(q[h] @ q[h]))).astype(np.float16)
    for a in (K, V):
        _poison(a, n, ("nan", "inf")[(n + G) % 2])
    return K, V, q


def _read_values(x, kv_sink, kv_pos):
    """What the kernel reads of cache x (msl, n_kv, D), float64: c * s, or the f16 row itself."""
    with np.errstate(all="ignore"):
        c, s = M.kv_q8_quantize(x)
        r = (c.astype(np.float64) - 128) * s.astype(np.float64)[..., None]
    for t in [*range(kv_sink), kv_pos]:
        r[t] = x[t].astype(np.float64)
    return r


def _attn64(Kr, Vr, q, n, G):
    out = np.zeros(q.shape)
    for h in range(q.shape[0]):
        s = Kr[:n, h // G] @ q[h].astype(np.float64) / np.sqrt(q.shape[1])
        p = np.exp(s - s.max())
        out[h] = (p / p.sum()) @ Vr[:n, h // G]
    return out.reshape(-1)


def _check_launches(D, G, msl, n, combos):
    K, V, q = _case(D, G, msl, n, 0)
    worst = 0.0
    for i, (splits, kv_sink, where) in enumerate(combos):
        if kv_sink >= n:
            continue
        kv_pos = {"first": kv_sink, "middle": (kv_sink + n - 1) // 2, "last": n - 1}[where]
        want = _attn64(_read_values(K, kv_sink, kv_pos), _read_values(V, kv_sink, kv_pos), q, n, G)
        got, kc, ks, _, _ = runtime.mha_q8(K, V, q, D, kv_sink, kv_pos, n, msl, N_KV * G, N_KV, splits)
        b = A.bars(got, want, A.X_ATOL, A.X_RTOL)
        print(f"d{D} g{G} kv{n} splits{splits} sink{kv_sink} pos{kv_pos}: {b:.3f} bars")
        worst = max(worst, b)
        # (the hook quantised every row before the launch, row kv_pos too: this cannot tell whether the
        # launch's own quantisation of row kv_pos ran; test_whole_decoder sees that, step by step)
        wc, ws = M.kv_q8_quantize(K[:n])
        np.testing.assert_array_equal(kc[:n], wc)
        np.testing.assert_array_equal(ks[:n], ws)
        if i == 0:   # a second call gives the same bits
            again = runtime.mha_q8(K, V, q, D, kv_sink, kv_pos, n, msl, N_KV * G, N_KV, splits)[0]
            np.testing.assert_array_equal(got.view(np.uint32), again.view(np.uint32))
    assert worst < 1.0, f"{worst:.3f} bars"


COMBOS = [(s, k, w) for s in (1, 3, 0) for k in (0, 2) for w in ("first", "middle", "last")]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 256, 257, 330])
@pytest.mark.parametrize("G", [1, 4, 7, 8])
@pytest.mark.parametrize("D", [64, 128])
def test_kernel_vs_float64(D, G, n):
    _check_launches(D, G, 330, n, COMBOS)


def test_kernel_vs_float64_long():
    _check_launches(128, 4, 4224, 4224, [(0, 2, "middle"), (3, 0, "last")])


class Q8Ref(RefModel):
    """RefModel's step over given cache values: `read[l]` = (K, V) float64 (rows, kv_dim) as the q8
    attention reads them; the step's own k / v are not stored (the device's rows are in `read`)."""

    def block(self, l, x, pos, kv_sink, kv_pos, kv_len):
        c, t, n = self.c, self.t, M.layer_names(l)
        xb = ref_rmsnorm(x, t[n["rms_att"]], c.norm_eps)
        q = ref_rope(np.clip(t[n["wq"]] @ xb, -c.qkv_clip, c.qkv_clip), c.head_dim, pos, c.rope_theta, c.rotary_dim)
        K, V = (a[:kv_len].reshape(kv_len, c.n_kv_heads, c.head_dim) for a in self.read[l])
        out = _attn64(K, V, q.reshape(c.n_heads, c.head_dim), kv_len, c.n_heads // c.n_kv_heads)
        x = x + t[n["wo"]] @ out
        xb = ref_rmsnorm(x, t[n["rms_ffn"]], c.norm_eps)
        return x + t[n["w2"]] @ (ref_silu(t[n["w1"]] @ xb) * (t[n["w3"]] @ xb))


BAR = 1e-3  # the decode tests' relative bar on the logits


@pytest.mark.parametrize("dtype,seed", [(M.F16, 184), (M.Q4, 4)])
def test_whole_decoder(dtype, seed):
    """Prefill 40 positions, decode to position 80 (ring wrap at 64, two sinks). Every step's logits
    and greedy token against Q8Ref over the rows the device holds after that step. The seeds are the
    first for which a CPU-only float64 run of the same model over its own quantised cache keeps the
    top-2 logit gap above 2 % of the largest logit at every step (f16 0.024, q4 0.049)."""
    cfg = M.TINY.with_(dim=128, hidden_dim=256, head_dim=64, weight_dtype=dtype)   # (the prefill's dims: multiples of 128)
    t = M.synth_host_tensors(cfg, seed=seed)
    tw_cfg, tw = M.q4_twin(cfg, t) if dtype == M.Q4 else (cfg, t)
    ref = Q8Ref(tw_cfg, tw)
    dm = runtime.DeviceModel.from_arrays(cfg, t)
    dec = runtime.Decoder(dm)
    try:
        dec.set_kv_q8(True)
        assert dec.kv_q8 and not dec.attn_wo
        prompt = [(7 * i + 3) % cfg.vocab_size for i in range(40)]
        dec.prefill(prompt, 0, logprobs=False)
        tok = prompt[-1] + 1
        for pos in range(40, 81):
            lg = dec.forward(tok, pos)
            kv_sink, kv_pos, kv_len = M.kv_indices(cfg.max_seq_len, pos)
            ref.read = []
            for l in range(cfg.n_layers):
                k16, v16, kc, ks, vc, vs = dec.get_kv_q8(l)
                live = [r for r in range(kv_sink, kv_len)]
                for c_, s_, x in ((kc, ks, k16), (vc, vs, v16)):   # the shadow is the quantiser of the f16 rows
                    wc, ws = M.kv_q8_quantize(x[live])
                    np.testing.assert_array_equal(c_[live], wc)
                    np.testing.assert_array_equal(s_[live], ws)
                ref.read.append(tuple(_read_values(x, kv_sink, kv_pos).reshape(cfg.max_seq_len, -1) for x in (k16, v16)))
            want = ref.forward(tok, pos)
            err = float(np.max(np.abs(lg - want)) / np.max(np.abs(want)))
            top = np.sort(want)[-2:]
            assert err < BAR, f"pos {pos}: {err:.2e}"
            assert (top[1] - top[0]) / np.max(np.abs(want)) > 10 * BAR, f"pos {pos}: the reference has a near-tie"
            assert int(np.argmax(lg)) == int(np.argmax(want))
            tok = int(np.argmax(want))
    finally:
        dec.close()
        dm.close()


def _refused(fn, code=3):
    with pytest.raises(runtime.YalmError, match=f"yalm error {code}.*" + ("q8 kv" if code == 3 else "")):
        fn()


PREFILLABLE = M.TINY.with_(dim=128, hidden_dim=256, head_dim=64)   # (the prefill's dims: multiples of 128)


def test_refusals_and_state():
    cfg = PREFILLABLE
    dm = runtime.DeviceModel.from_arrays(cfg, M.synth_host_tensors(cfg, seed=2))
    dec = runtime.Decoder(dm)
    try:
        off = [dec.kernel_name(k) for k in range(16)], dec.graph_kernels(2)
        assert "attn_decode_kernel<" in off[0] and not dec.kv_q8
        dec.set_kv_q8(True)
        names = [dec.kernel_name(k) for k in range(16)]
        assert names[1] == "attn_decode_q8_kernel<" and names[:1] + names[2:] == off[0][:1] + off[0][2:]
        assert dec.graph_kernels(2) == off[1] and not dec.attn_wo
        dec.set_kv_q8(False)
        assert ([dec.kernel_name(k) for k in range(16)], dec.graph_kernels(2)) == off
        dec.set_kv_q8(True)
        _refused(lambda: dec.forward_rows([1, 2], 0))
        _refused(lambda: dec.generate_speculative(1, 0, 4))
        _refused(lambda: dec.generate_speculative_sampled(1, 0, 4, 1.0))
        _refused(lambda: dec.generate_speculative_model(dec, 1, 0, 4))
        _refused(lambda: runtime.Batch(dec, 2))
        dec.forward(1, 0)
        _refused(lambda: dec.set_kv_q8(False), code=2)
        for on in (False, True):   # a prefill writes positions too: neither switch is taken after it
            d2 = runtime.Decoder(dm)
            try:
                d2.set_kv_q8(on)
                d2.prefill([1, 2, 3], 0, logprobs=False)
                _refused(lambda: d2.set_kv_q8(not on), code=2)
                assert d2.kv_q8 == on
            finally:
                d2.close()
    finally:
        dec.close()
        dm.close()


@pytest.mark.parametrize("kind", ["moe", "head_dim", "caches", "tp", "tp_ipc"])
def test_refused_decoders(kind):
    q8able = M.TINY.with_(dim=512, hidden_dim=512, head_dim=64)   # (the IPC transport: dim a multiple of 512 in f16)
    cfg = {"moe": M.TINY_MOE.with_(head_dim=64), "head_dim": M.TINY}.get(kind, q8able)
    dm = runtime.DeviceModel.from_arrays(cfg, M.synth_host_tensors(cfg, seed=2))
    bufs = [runtime.lib.yalm_alloc(2 * cfg.max_seq_len * cfg.kv_dim) for _ in range(2 * cfg.n_layers)]
    caches = list(zip(bufs[::2], bufs[1::2])) if kind == "caches" else None
    # one-rank tensor-parallel decoders of either transport, in this process (as test_gpu_tp.py)
    tp = {"tp_id": runtime.tp_unique_id()} if kind == "tp" else {"tp_gather": lambda h: [h]} if kind == "tp_ipc" else {}
    dec = runtime.Decoder(dm, kv_caches=caches, **tp)
    try:
        _refused(lambda: dec.set_kv_q8(True))
        assert not dec.kv_q8
    finally:
        dec.close()
        dm.close()
        for b in bufs:
            runtime.lib.yalm_free(b)
