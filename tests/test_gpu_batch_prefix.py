"""GPU: batched decode over a shared prompt prefix (yalm_batch_share_prefix, csrc/batch_prefix.h).

Kernel (yalm_attn_batch_prefix, the step's own two launches): every output row against float64
softmax attention over [shared rows 0 .. prefix) + own rows [prefix, kv_len[s])] at the decode
attention's bars (attn_ref.X_ATOL / X_RTOL). Every row no sequence may read is poison (f16 NaN or
+inf): own rows below prefix and from kv_len[s] on, shared rows from prefix on. Keys with a score far
above the rest and a V row of their own sit at both ends of both segments, so a lost edge key or a
row read from the wrong cache moves the output by thousands of bars.

Whole step: a batch that shares the decoder's rows against one that loaded them, at the project's
1e-3 relative logits bar. Layer 0's K / V rows must be equal bit for bit (the QKV path is
untouched); a deeper layer's rows are computed from an attention output with another rounding, so
they are held to the logits bar instead.
"""
import numpy as np
import pytest

from attn_ref import X_ATOL, X_RTOL, bars
from test_gpu_batch import CONFIGS, Plain, _cfg, batch_kv_row, bits, rt
from yalm_amd import models as M

pytestmark = pytest.mark.gpu

N_KV = 2
OWN = (65, 1, 64, 1)  # own rows per sequence: both sides of the 64-key tile
POISON = (0x7E00, 0x7C00)  # f16 NaN, +inf
worst = {"bars": 0.0, "case": ""}


def make_case(D, G, n_seq, prefix, seed):
    rng = np.random.default_rng(seed)
    kv_dim, H = N_KV * D, N_KV * G
    kv_len = [prefix + OWN[s] for s in range(n_seq)]
    rows = prefix + 70
    q = (rng.standard_normal((n_seq, H, D)) * 2).astype(np.float32)
    caches = rng.standard_normal((2, 1 + n_seq, rows, kv_dim)).astype(np.float16)  # [K | V][shared, seq 0, ..]
    K, V = caches[0], caches[1]

    def plant(c, row, seqs, v):  # the minimum-norm K row whose score with every head of `seqs` is 7
        for g in range(N_KV):
            Q = q[seqs, g * G:(g + 1) * G].reshape(-1, D).astype(np.float64)
            K[c, row, g * D:(g + 1) * D] = (np.linalg.pinv(Q) @ np.full(Q.shape[0], 7.0 * np.sqrt(D))).astype(np.float16)
        V[c, row] = v

    plant(0, 0, list(range(n_seq)), 8.0)
    plant(0, prefix - 1, list(range(n_seq)), -6.0)
    for s in range(n_seq):
        plant(1 + s, prefix, [s], 4.0 + s)
        plant(1 + s, kv_len[s] - 1, [s], -3.0 - s)
    bad = caches.view(np.uint16)
    bad[:, 0, prefix:] = POISON[seed % 2]
    for s in range(n_seq):
        bad[:, 1 + s, :prefix] = POISON[(seed + s) % 2]
        bad[:, 1 + s, kv_len[s]:] = POISON[(seed + s + 1) % 2]
    want = np.empty((n_seq, H, D))
    for s in range(n_seq):
        k = np.concatenate([K[0, :prefix], K[1 + s, prefix:kv_len[s]]]).astype(np.float64)
        v = np.concatenate([V[0, :prefix], V[1 + s, prefix:kv_len[s]]]).astype(np.float64)
        for h in range(H):
            g = h // G
            sc = k[:, g * D:(g + 1) * D] @ q[s, h].astype(np.float64) / np.sqrt(D)
            p = np.exp(sc - sc.max())
            want[s, h] = (p / p.sum()) @ v[:, g * D:(g + 1) * D]
    return q, K, V, kv_len, want


@pytest.mark.parametrize("prefix", [1, 63, 64, 65, 130, 2200])  # 2200: 35 tiles over 32 splits, two tiles in three of them
@pytest.mark.parametrize("n_seq", [1, 3, 4])
@pytest.mark.parametrize("G", [1, 4, 8])
@pytest.mark.parametrize("D", [64, 128])
def test_kernel_against_float64(D, G, n_seq, prefix):
    R = rt()
    q, K, V, kv_len, want = make_case(D, G, n_seq, prefix, seed=D + 7 * G + 3 * n_seq + prefix)
    H = N_KV * G
    out = np.full((n_seq, H * D), -7.25, np.float32)
    got = R.attn_batch_prefix(out, q.reshape(n_seq, -1), K[0], V[0], list(K[1:]), list(V[1:]), prefix, kv_len, H, N_KV, D)
    b = bars(got.reshape(want.shape), want, X_ATOL, X_RTOL)
    name = f"d{D}-g{G}-n{n_seq}-p{prefix}"
    if b > worst["bars"]:
        worst.update(bars=b, case=name)
    print(f"{name}: {b:.4f} bars (worst so far {worst['bars']:.4f} at {worst['case']})")
    assert b <= 1.0, f"{name}: {b:.2f} bars"


STEP_CONFIGS = ["f16-d64-g4", "fp8-d64-g1-bias", "f16-d64-g4-qknorm", "e4m3-d128-g4"]


@pytest.mark.parametrize("n_seq", [1, 4])
@pytest.mark.parametrize("name", STEP_CONFIGS)
def test_shared_step_against_loaded_step(name, n_seq):
    R = rt()
    cfg = CONFIGS[name]
    n, L = 70, cfg.n_layers
    pl = Plain(R, cfg, n=n)
    toks, pos = [5, 17, 101, 250][:n_seq], [n, n + 3, n + 64, n + 65][:n_seq]
    norm = L if cfg.qk_norm else 0
    A, B = R.Batch(pl.dec, n_seq), R.Batch(pl.dec, n_seq)
    try:
        A.load(n)
        lgA = A.forward(toks, pos)
        rowsA = [batch_kv_row(R, A, cfg, s, pos[s]) for s in range(n_seq)]
        B.share_prefix(n)
        lgB = B.forward(toks, pos)
        assert B.stats()["launches_per_step"] == 3 + 6 * L + norm
        scale = np.abs(lgA).max(axis=1, keepdims=True)
        assert (np.abs(lgB - lgA) / scale).max() < 1e-3
        per_layer = 2 * 2 * cfg.kv_dim  # bytes of one layer's K and V row
        for s in range(n_seq):
            rowB = batch_kv_row(R, B, cfg, s, pos[s])
            np.testing.assert_array_equal(rowB[:per_layer], rowsA[s][:per_layer], err_msg=f"{name}: layer 0 KV row")
            a, b = (r.view(np.float16).astype(np.float64) for r in (rowsA[s], rowB))
            assert np.abs(a - b).max() <= 1e-3 * np.abs(a).max()
        # off again: the loaded form's launches and bits
        B.load(n)
        B.share_prefix(0)
        assert B.stats()["launches_per_step"] == 3 + 5 * L + norm
        np.testing.assert_array_equal(bits(B.forward(toks, pos)), bits(lgA))
        B.share_prefix(n)
        gA, gB = A.generate_greedy(toks, pos, 3)[0], B.generate_greedy(toks, pos, 3)[0]
        top2 = np.sort(lgA, axis=1)[:, -2:]
        for s in range(n_seq):  # the first token wherever the loaded form's margin exceeds the bar
            if top2[s, 1] - top2[s, 0] > 1e-3 * scale[s, 0]:
                assert gA[s, 0] == gB[s, 0]
    finally:
        A.close()
        B.close()
        pl.close()


def test_refusals():
    R = rt()
    cfg = CONFIGS["f16-d64-g4"]
    pl = Plain(R, cfg, n=40)
    b = R.Batch(pl.dec, 2)
    try:
        for bad in (-1, cfg.max_seq_len + 1):
            with pytest.raises(R.YalmError, match="error 2.*n_positions"):
                b.share_prefix(bad)
        b.share_prefix(40)
        before = b.forward([5, 17], [40, 45])
        for call in (lambda: b.forward([5, 17], [40, 39]), lambda: b.generate_greedy([5, 17], [39, 40], 2),
                     lambda: b.generate_sampled([5, 17], [0, 40], 2, 1.0)):
            with pytest.raises(R.YalmError, match="error 2.*shared prefix"):
                call()
        assert b.state() == ([5, 17], [40, 45])
        np.testing.assert_array_equal(bits(b.forward([5, 17], [40, 45])), bits(before))
    finally:
        b.close()
        pl.close()
    small = _cfg(dim=128, hidden_dim=256, head_dim=32, n_heads=4, n_kv_heads=2, weight_dtype=M.F16)
    dm = R.DeviceModel.synthetic(small, seed=1)
    dec = R.Decoder(dm)
    try:
        b = R.Batch(dec, 2)
        with pytest.raises(R.YalmError, match="error 3: yalm_batch_share_prefix.*head_dim 64 or 128"):
            b.share_prefix(8)
        b.close()
    finally:
        dec.close()
        dm.close()
