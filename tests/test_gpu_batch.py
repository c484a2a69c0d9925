"""GPU: batched decode (yalm_batch_*, csrc/batch.h): up to four independent sequences per pass
over the weights.

Bars. Row s of a batched step must equal yalm_forward_rows(T = 1) of the same token at the same
position over the same history BIT FOR BIT (logits and the KV row written): a row of
gemv_rows_kernel depends on neither T nor the other rows, and the attention body is the decode
kernel's. The one-launch attention must equal the per-sequence launches bit for bit. Greedy tokens
equal the CPU oracle's on seeds whose oracle path keeps a top-2 gap of 2 x 1e-3 x max|logit| at
every step (asserted on the oracle, as tests/test_gpu_spec.py does), and yalm_generate_greedy's on
the golden models. Sampled tokens equal the host restatement of the rule (sampling_ref.Rule) on
the logits of a lock-step yalm_batch_forward replay with the weights q the device computed.

Every config has max_seq_len 320: five 64-key chunks, so positions >= 256 run the attention in key
mode (splits + mergers) and lower ones in head mode.
"""
import functools
import os

import numpy as np
import pytest

import oracle_py as O
import sampling_ref as SR
from yalm_amd import models as M

pytestmark = pytest.mark.gpu

MSL = 320
GAP = 2e-3


def rt():
    from yalm_amd import runtime

    return runtime


def _cfg(**kw):
    base = dict(n_layers=2, vocab_size=384, max_seq_len=MSL, rope_theta=10000.0, act=M.SILU)
    base.update(kw)
    return M.ModelConfig(**base)


# dim 64..256, head_dim 64 and 128, GQA group 1 and 4, every weight type with a multi-row form, one
# biased config, one with the q / k norm
CONFIGS = {
    "f16-d64-g4": _cfg(dim=128, hidden_dim=256, head_dim=64, n_heads=4, n_kv_heads=1, weight_dtype=M.F16),
    "f32-d128-g1": _cfg(dim=256, hidden_dim=384, head_dim=128, n_heads=2, n_kv_heads=2, weight_dtype=M.F32,
                        vocab_size=300),
    "fp8-d64-g1-bias": _cfg(dim=64, hidden_dim=192, head_dim=64, n_heads=2, n_kv_heads=2, weight_dtype=M.F8E5M2,
                            qkv_bias=True),
    "e4m3-d128-g4": _cfg(dim=256, hidden_dim=512, head_dim=128, n_heads=4, n_kv_heads=1, weight_dtype=M.E4M3,
                         act=M.GELU),
    "f16-d64-g4-qknorm": _cfg(dim=192, hidden_dim=256, head_dim=64, n_heads=4, n_kv_heads=1, weight_dtype=M.F16,
                              qk_norm=True),
}
# both sides of the 64-key chunk edge (63 | 64) and of the head / key mode switch (255 | 256), the
# first and the last position of the window
LAYOUTS = [(0, 63, 64, 300), (319, 256, 255, 200)]


def history(cfg, seed=7):
    return [int(t) for t in np.random.default_rng(seed).integers(1, cfg.vocab_size, MSL)]


class Plain:
    """A plain decoder with caller-owned KV caches (so the tests can read them), hydrated with
    `hist` by single-row forwards."""

    def __init__(self, R, cfg, seed=3, hist=None, n=MSL):
        self.R, self.cfg = R, cfg
        self.dm = R.DeviceModel.synthetic(cfg, seed=seed)
        self.kvb = 2 * cfg.max_seq_len * cfg.kv_dim
        self.caches = [(R.lib.yalm_alloc(self.kvb), R.lib.yalm_alloc(self.kvb)) for _ in range(cfg.n_layers)]
        self.dec = R.Decoder(self.dm, kv_caches=self.caches)
        self.hist = hist if hist is not None else history(cfg)
        for p in range(n):
            self.dec.forward(self.hist[p], p, R.HYDRATE_KV_CACHE)

    def kv_row(self, pos):
        return np.concatenate([download(self.R, ptr + 2 * pos * self.cfg.kv_dim, 2 * self.cfg.kv_dim)
                               for kv in self.caches for ptr in kv])

    def close(self):
        self.dec.close()
        for kv in self.caches:
            for p in kv:
                self.R.lib.yalm_free(p)
        self.dm.close()


def download(R, ptr, nbytes):
    """nbytes at device pointer ptr; the caller has synchronised the decoder's stream (a forward
    with logits, Batch.state)."""
    a = np.empty(nbytes, np.uint8)
    R.check(R.lib.yalm_stream_sync(None))
    R.check(R.lib.yalm_download(a.ctypes.data, ptr, nbytes))
    return a


def upload(R, ptr, arr):
    a = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    tmp = R.lib.yalm_upload(a.ctypes.data, a.nbytes)
    assert tmp
    try:
        R.check(R.lib.yalm_copy_2d(ptr, a.nbytes, tmp, a.nbytes, a.nbytes, 1))
        R.check(R.lib.yalm_stream_sync(None))
    finally:
        R.lib.yalm_free(tmp)


def batch_kv_row(R, batch, cfg, seq, pos):
    out = []
    for l in range(cfg.n_layers):
        k, v, _ = batch.buffers(seq, l)
        out += [download(R, k + 2 * pos * cfg.kv_dim, 2 * cfg.kv_dim), download(R, v + 2 * pos * cfg.kv_dim, 2 * cfg.kv_dim)]
    return np.concatenate(out)


def guards_intact(R, batch, cfg):
    g = R.BATCH_GUARD_BYTES
    kvb, tb = 2 * cfg.max_seq_len * cfg.kv_dim, 4 * 65536
    batch.state()  # sync
    for s in range(batch.n_seq):
        bufs = [(p, kvb) for l in range(cfg.n_layers) for p in batch.buffers(s, l)[:2]] + [(batch.buffers(s, 0)[2], tb)]
        for p, n in bufs:
            if not (download(R, p - g, g) == 0xA5).all() or not (download(R, p + n, g) == 0xA5).all():
                return False
    return True


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def expected_launches(cfg, n_seq, per_seq):
    L = cfg.n_layers
    return 3 + L * ((4 + n_seq if per_seq else 5) + (1 if cfg.qk_norm else 0))


# ------------------------------------------------------------------ 1. bit identity, both attention forms
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_rows_equal_single_sequence_path_bit_for_bit(name):
    R = rt()
    cfg = CONFIGS[name]
    pl = Plain(R, cfg)
    toks = [5, 17, 101, 250]
    try:
        for layout in LAYOUTS:
            for n_seq in (1, 2, 3, 4):
                pos = list(layout[:n_seq])
                got = {}
                for per_seq in (False, True):
                    b = R.Batch(pl.dec, n_seq, launch=R.BATCH_ATTN_PER_SEQ if per_seq else 0)
                    try:
                        for s in range(n_seq):
                            b.load(pos[s], seq=s)
                        lg = b.forward(toks[:n_seq], pos)
                        rows = [batch_kv_row(R, b, cfg, s, pos[s]) for s in range(n_seq)]
                        assert b.stats()["launches_per_step"] == expected_launches(cfg, n_seq, per_seq)
                        assert b.state() == (toks[:n_seq], pos)  # set, not advanced
                        assert guards_intact(R, b, cfg)
                    finally:
                        b.close()
                    got[per_seq] = (lg, rows)
                lg, rows = got[False]
                np.testing.assert_array_equal(bits(lg), bits(got[True][0]), err_msg=f"{name} {pos}: attention forms")
                for s in range(n_seq):
                    np.testing.assert_array_equal(rows[s], got[True][1][s], err_msg=f"{name} {pos}: KV, forms")
                    want = pl.dec.forward_rows([toks[s]], pos[s])[0]
                    want_row = pl.kv_row(pos[s])
                    pl.dec.forward(pl.hist[pos[s]], pos[s], R.HYDRATE_KV_CACHE)  # the history's row again
                    assert np.isfinite(want).all()
                    np.testing.assert_array_equal(bits(lg[s]), bits(want), err_msg=f"{name} {pos} row {s}: logits")
                    np.testing.assert_array_equal(rows[s], want_row, err_msg=f"{name} {pos} row {s}: KV row")
    finally:
        pl.close()


# ------------------------------------------------------------------ 2. independence
@pytest.mark.parametrize("per_seq", [False, True], ids=["one-launch", "per-seq"])
def test_sequences_are_independent(per_seq):
    R = rt()
    cfg = CONFIGS["f16-d64-g4"]
    pl = Plain(R, cfg)
    pos, toks = [300, 0, 64, 130], [5, 17, 101, 250]
    b = R.Batch(pl.dec, 4, launch=R.BATCH_ATTN_PER_SEQ if per_seq else 0)
    try:
        for s in range(4):
            b.load(pos[s], seq=s)
        base = b.forward(toks, pos)
        assert len({base[s].tobytes() for s in range(4)}) == 4  # the rows really differ
        # everything a row must not read: the rows past each sequence's kv_len -- for sequence 1,
        # at position 0, all of its cache but the row it writes -- as NaN keys and +inf values
        for s in range(4):
            n = cfg.max_seq_len - pos[s] - 1
            if n == 0:
                continue
            for l in range(cfg.n_layers):
                k, v, _ = b.buffers(s, l)
                off = 2 * (pos[s] + 1) * cfg.kv_dim
                upload(R, k + off, np.full(n * cfg.kv_dim, 0x7E00, np.uint16))
                upload(R, v + off, np.full(n * cfg.kv_dim, 0x7C00, np.uint16))
        again = b.forward(toks, pos)
        np.testing.assert_array_equal(bits(again), bits(base))
        # another token in one sequence changes that row alone
        for s in range(4):
            t2 = list(toks)
            t2[s] = 33
            lg = b.forward(t2, pos)
            for r in range(4):
                same = np.array_equal(bits(lg[r]), bits(base[r]))
                assert same == (r != s), (s, r)
            b.forward(toks, pos)  # row pos[s] of sequence s as it was
        np.testing.assert_array_equal(bits(b.forward(toks, pos)), bits(base))
        assert guards_intact(R, b, cfg)
    finally:
        b.close()
        pl.close()


# ------------------------------------------------------------------ 3. greedy against the oracle and the plain loop
# (config, tensor seed, prompt seeds of the four sequences, prompt lengths): searched on the CPU
# oracle for greedy paths without a near-tie (asserted in oracle_greedy)
SMALL320 = M.SMALL.with_(max_seq_len=MSL)
ORACLE = {
    "small-f16": (SMALL320, 5, (108, 105, 105, 106), (13, 1, 6, 9)),
    "small-fp8": (SMALL320.with_(weight_dtype=M.F8E5M2), 1, (101, 105, 107, 104), (13, 1, 6, 9)),
}
N_GEN = 24


@functools.lru_cache(maxsize=None)
def oracle_greedy(name):
    cfg, seed, pseeds, plens = ORACLE[name]
    host = O.synth_host_tensors_fast(cfg, seed=seed)
    prompts, seqs = [], []
    for ps, n in zip(pseeds, plens):
        om = O.OracleModel(cfg, host)
        prompt = [int(t) for t in np.random.default_rng(ps).integers(1, cfg.vocab_size, n)]
        for p, t in enumerate(prompt[:-1]):
            om.forward(t, p, 0)
        tok, seq, worst = prompt[-1], [], np.inf
        for i in range(N_GEN):
            lg = om.forward(tok, n - 1 + i)
            s = np.sort(lg)
            worst = min(worst, float((s[-1] - s[-2]) / np.max(np.abs(lg))))
            tok = int(O.olib.orc_sample_argmax(O.P(lg), cfg.vocab_size))
            seq.append(tok)
        assert worst >= GAP, f"{name} prompt seed {ps}: near-tie on the oracle's greedy path (gap {worst:.2e})"
        prompts.append(prompt)
        seqs.append(seq)
    return host, prompts, seqs


@pytest.mark.parametrize("name", sorted(ORACLE))
def test_greedy_equals_oracle(name):
    R = rt()
    cfg = ORACLE[name][0]
    host, prompts, seqs = oracle_greedy(name)
    dm = R.DeviceModel.from_arrays(cfg, host)
    dec = R.Decoder(dm)
    try:
        for n_seq, per_seq in ((4, False), (4, True), (2, False)):
            b = R.Batch(dec, n_seq, launch=R.BATCH_ATTN_PER_SEQ if per_seq else 0)
            try:
                for s in range(n_seq):  # each prompt hydrated on the decoder, then loaded
                    for p, t in enumerate(prompts[s][:-1]):
                        dec.forward(t, p, R.HYDRATE_KV_CACHE)
                    b.load(len(prompts[s]) - 1, seq=s)
                toks = [prompts[s][-1] for s in range(n_seq)]
                pos = [len(prompts[s]) - 1 for s in range(n_seq)]
                out, st = b.generate_greedy(toks, pos, N_GEN)
                assert out.tolist() == [seqs[s] for s in range(n_seq)], (n_seq, per_seq)
                assert st["launches_per_step"] == expected_launches(cfg, n_seq, per_seq)
                assert b.state() == ([seqs[s][-1] for s in range(n_seq)], [p + N_GEN for p in pos])
                # the token buffers hold each sequence's own tokens
                for s in range(n_seq):
                    tb = download(R, b.buffers(s)[2], 4 * N_GEN).view(np.int32)
                    assert tb.tolist() == seqs[s]
                assert guards_intact(R, b, cfg)
            finally:
                b.close()
    finally:
        dec.close()
        dm.close()


def test_greedy_equals_plain_loop_on_golden_models(golden_dir):
    R = rt()
    from yalm_amd.yalmfile import read_yalm

    for fname in ("tiny_fp16.yalm", "tiny_fp32.yalm", "tiny_fp8.yalm", "tiny_fp16_tied.yalm"):
        yd = read_yalm(os.path.join(golden_dir, fname))
        tied = "model.output.weight" not in yd.tensors
        cfg = M.config_from_metadata(yd.metadata, tied=tied).with_(max_seq_len=MSL)
        t = {k: np.array(v.data).reshape(v.shape) for k, v in yd.tensors.items()}
        yd.close()
        dm = R.DeviceModel.from_arrays(cfg, t)
        dec = R.Decoder(dm)
        try:
            starts = [1, 7, 19, 40]
            want = [dec.generate_greedy(tok, 0, N_GEN) for tok in starts]
            b = R.Batch(dec, 4)
            try:
                out, _ = b.generate_greedy(starts, [0, 0, 0, 0], N_GEN)
                assert out.tolist() == want, fname
            finally:
                b.close()
        finally:
            dec.close()
            dm.close()


# ------------------------------------------------------------------ 4. sampled
@pytest.mark.parametrize("name,temp,top_k,top_p", [("f16-d64-g4", 1.0, 0, 1.0), ("fp8-d64-g1-bias", 0.7, 40, 0.9),
                                                   ("f32-d128-g1", 1.3, 0, 0.8)])
def test_sampled_tokens_follow_the_rule(name, temp, top_k, top_p):
    R = rt()
    cfg = CONFIGS[name]
    n, pos, toks = 10, [20, 20, 250], [9, 9, 77]  # sequences 0 and 1: one prompt, their own uniforms
    pl = Plain(R, cfg, n=256)
    u = np.random.default_rng(11).random((3, n), dtype=np.float32)
    try:
        b = R.Batch(pl.dec, 3)
        try:
            for s in range(3):
                b.load(pos[s], seq=s)
            out, st = b.generate_sampled(toks, pos, n, temp, top_k, top_p, uniforms=u)
            assert st["launches_per_step"] == expected_launches(cfg, 3, False)
            assert b.state() == (out[:, -1].tolist(), [p + n for p in pos])
            assert guards_intact(R, b, cfg)
        finally:
            b.close()
        b = R.Batch(pl.dec, 3)  # the lock-step replay
        try:
            for s in range(3):
                b.load(pos[s], seq=s)
            cur = list(toks)
            for i in range(n):
                lg = b.forward(cur, [p + i for p in pos])
                if i == 0:
                    np.testing.assert_array_equal(bits(lg[0]), bits(lg[1]))
                for s in range(3):
                    q = R.sample(lg[s], temp, 0, 1.0, [0.5])[2]
                    want = SR.Rule(lg[s], q, top_k, top_p).draw(u[s, i])
                    assert int(out[s, i]) == want, (s, i)
                cur = out[:, i].tolist()
        finally:
            b.close()
        assert out[0].tolist() != out[1].tolist()  # one prompt, two completions
    finally:
        pl.close()


# ------------------------------------------------------------------ 5. load
def test_load_copies_rows_and_nothing_else():
    R = rt()
    cfg = CONFIGS["f16-d64-g4"]
    pl = Plain(R, cfg, n=100)
    b = R.Batch(pl.dec, 3)
    kvb = 2 * cfg.max_seq_len * cfg.kv_dim
    rowb = 2 * cfg.kv_dim
    try:
        mark = np.full(kvb // 2, 0x1234, np.uint16)
        for s in range(3):
            for l in range(cfg.n_layers):
                for p in b.buffers(s, l)[:2]:
                    upload(R, p, mark)
        b.load(70, seq=1)
        b.state()  # sync
        for s in range(3):
            for l in range(cfg.n_layers):
                for src, p in zip(pl.caches[l], b.buffers(s, l)[:2]):
                    got = download(R, p, kvb)
                    if s == 1:
                        assert np.array_equal(got[:70 * rowb], download(R, src, 70 * rowb))
                        assert np.array_equal(got[70 * rowb:], mark.view(np.uint8)[70 * rowb:])
                    else:
                        assert np.array_equal(got, mark.view(np.uint8))
        b.load(0, seq=0)  # nothing
        b.state()
        assert np.array_equal(download(R, b.buffers(0, 0)[0], kvb), mark.view(np.uint8))
        b.load(10)  # every sequence
        b.state()
        for s in range(3):
            for l in range(cfg.n_layers):
                for src, p in zip(pl.caches[l], b.buffers(s, l)[:2]):
                    got = download(R, p, kvb)
                    assert np.array_equal(got[:10 * rowb], download(R, src, 10 * rowb))
                    if s != 1:
                        assert np.array_equal(got[10 * rowb:], mark.view(np.uint8)[10 * rowb:])
        for kw in (dict(n_positions=-1), dict(n_positions=cfg.max_seq_len + 1), dict(n_positions=1, seq=3),
                   dict(n_positions=1, seq=-2)):
            with pytest.raises(R.YalmError, match="error 2"):
                b.load(**kw)
        b.load(cfg.max_seq_len, seq=2)  # the whole window: accepted
        assert guards_intact(R, b, cfg)
    finally:
        b.close()
        pl.close()


# ------------------------------------------------------------------ 6. refusals and arguments
def test_refusals_and_arguments():
    R = rt()
    # q4, mixture of experts, tensor parallel: UNSUPPORTED in the words of the multi-row path
    for cfg, kw, why in ((M.TINY.with_(weight_dtype=M.Q4), {}, "q4 weights have no multi-row form"),
                         (M.TINY_MOE, {}, "mixture-of-experts decoders have no multi-row form"),
                         (M.SMALL, dict(tp_gather=lambda h: [h]), "tensor-parallel decoders have no multi-row form")):
        dm = R.DeviceModel.synthetic(cfg, seed=1)
        dec = R.Decoder(dm, **kw)
        try:
            with pytest.raises(R.YalmError, match=f"error 3: yalm_batch_create: {why}"):
                R.Batch(dec, 2)
        finally:
            dec.close()
            dm.close()
    # a vocabulary the sampler does not take
    big = _cfg(dim=64, hidden_dim=64, head_dim=64, n_heads=1, n_kv_heads=1, n_layers=1, weight_dtype=M.F8E5M2,
               vocab_size=131076)
    dm = R.DeviceModel.synthetic(big, seed=1)
    dec = R.Decoder(dm)
    try:
        b = R.Batch(dec, 2)
        with pytest.raises(R.YalmError, match="error 2.*vocabulary above 131072"):
            b.generate_sampled([1, 2], [0, 0], 2, 1.0, uniforms=np.full((2, 2), 0.5, np.float32))
        assert b.generate_greedy([1, 2], [0, 0], 2)[0].shape == (2, 2)  # greedy has no such limit
        b.close()
    finally:
        dec.close()
        dm.close()
    cfg = CONFIGS["f16-d64-g4"]
    pl = Plain(R, cfg, n=64)
    try:
        for n_seq in (0, 5, -1):
            with pytest.raises(R.YalmError, match="error 2.*n_seq"):
                R.Batch(pl.dec, n_seq)
        b = R.Batch(pl.dec, 2)
        try:
            b.load(64)
            toks, pos = [5, 17], [64, 10]
            base = b.forward(toks, pos)
            V = cfg.vocab_size
            u = np.full((2, 4), 0.5, np.float32)
            bad = [
                lambda: b.forward([5, V], pos),
                lambda: b.forward([-1, 5], pos),
                lambda: b.forward(toks, [MSL, 0]),
                lambda: b.forward(toks, [0, -1]),
                lambda: b.generate_greedy(toks, [MSL - 3, 0], 4),
                lambda: b.generate_greedy(toks, [0, MSL - 3], 4),
                lambda: b.generate_greedy([V, 0], pos, 4),
                lambda: b.generate_greedy(toks, pos, -1),
                lambda: b.generate_sampled(toks, [MSL - 3, 0], 4, 1.0, uniforms=u),
                lambda: b.generate_sampled(toks, pos, 4, 0.0, uniforms=u),
                lambda: b.generate_sampled(toks, pos, 4, float("inf"), uniforms=u),
                lambda: b.generate_sampled(toks, pos, 4, 1.0, top_k=-1, uniforms=u),
                lambda: b.generate_sampled(toks, pos, 4, 1.0, top_p=0.0, uniforms=u),
                lambda: b.generate_sampled(toks, pos, 4, 1.0, top_p=1.5, uniforms=u),
                lambda: b.generate_sampled(toks, pos, 4, 1.0, uniforms=np.array([[0.5] * 4, [0.5, 0.5, 1.5, 0.5]], np.float32)),
                lambda: b.set_launch(2),
            ]
            for f in bad:
                with pytest.raises(R.YalmError, match="error 2"):
                    f()
            with pytest.raises(R.YalmError, match="error 2.*token buffer"):
                R.check(R.lib.yalm_batch_generate_greedy(b.h, np.zeros(2, np.int32).ctypes.data,
                                                         np.zeros(2, np.int32).ctypes.data, 65537,
                                                         np.zeros(1, np.int32).ctypes.data, None))
            # a refused call changed nothing
            np.testing.assert_array_equal(bits(b.forward(toks, pos)), bits(base))
            assert b.generate_greedy(toks, [MSL - 4, 0], 4)[0].shape == (2, 4)  # pos + n == max_seq_len: accepted
        finally:
            b.close()
    finally:
        pl.close()
