"""CPU: the batched decode interface (yalm_batch_*) is declared, exported and wrapped
consistently, and a numpy model of one batched step -- rows, per-sequence caches, per-sequence
partial buffers, commit -- shows that the cases of tests/test_gpu_batch.py separate a correct
kernel from each of a handful of plausible slips: a row reading or writing another sequence's
cache, a partial buffer shared by the sequences, kv_len taken from row 0, a commit into the wrong
token buffer, uniforms indexed by the step only. (The pattern of tests/test_rows_cpu.py: the GPU
cases are only worth their time if a wrong kernel could not pass them.)"""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["yalm_batch_create", "yalm_batch_destroy", "yalm_batch_load", "yalm_batch_forward",
       "yalm_batch_generate_greedy", "yalm_batch_generate_sampled", "yalm_batch_state", "yalm_batch_set_launch",
       "yalm_batch_buffers"]


def header():
    with open(os.path.join(ROOT, "include", "yalm_hip.h")) as f:
        return f.read()


def test_header_exports_and_wrapper_agree():
    from yalm_amd import runtime as R

    src = header()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW:
        assert re.search(rf"\bint {name}\s*\(", code), f"{name}: not declared in include/yalm_hip.h"
        assert name in R.EXPORTED and hasattr(R.lib, name), name
        assert getattr(R.lib, name).argtypes is not None, f"{name}: no ctypes signature"
    assert int(re.search(r"#define YALM_BATCH_ATTN_PER_SEQ (\d+)", src).group(1)) == R.BATCH_ATTN_PER_SEQ
    assert int(re.search(r"#define YALM_BATCH_GUARD_BYTES (\d+)", src).group(1)) == R.BATCH_GUARD_BYTES
    assert re.search(r"typedef struct yalm_batch_stats \{\s*int launches_per_step;", code)
    assert [f[0] for f in R.BatchStats._fields_] == ["launches_per_step"]
    for m in ("load", "forward", "generate_greedy", "generate_sampled", "state", "stats", "set_launch", "close"):
        assert callable(getattr(R.Batch, m)), m
    # the device code is in its own header, and the headers the batch reuses are included, not copied
    with open(os.path.join(ROOT, "yalm_amd", "csrc", "batch.h")) as f:
        b = f.read()
    for k in ("batch_begin_kernel", "attn_decode_batch_kernel", "batch_commit_kernel", "batch_sample_kernel", "BQKVN"):
        assert k in b, k


# ------------------------------------------------------------------ the numpy model of a batched step
MSL, D, V, CHUNK, HEAD_MAX, CAP = 320, 8, 24, 64, 4, 64
SLIPS = ["cache_read", "cache_write", "shared_part", "kv_len_row0", "commit_buffer", "uniform_by_step"]


class Toy:
    """A one-layer model in float64: x = E[tok]; (k, v) = rot(pos)(x Wk), x Wv into row pos of
    the sequence's cache; attention over rows [0, kv_len) -- directly up to HEAD_MAX chunks, else
    through per-chunk partials in the sequence's partial buffer, merged after EVERY sequence has
    written its partials (the sequences of one launch are concurrent); logits = (x + att) Wc."""

    def __init__(self, n_seq, slip=None, seed=0):
        g = np.random.default_rng(seed)
        self.E, self.Wk, self.Wv, self.Wc = (g.standard_normal(s) for s in ((V, D), (D, D), (D, D), (D, V)))
        self.n_seq, self.slip = n_seq, slip
        self.k = np.zeros((n_seq, MSL, D))
        self.v = np.zeros((n_seq, MSL, D))
        self.part = np.zeros((n_seq, MSL // CHUNK, D + 2))
        self.tokens = np.full((n_seq, CAP), -1)
        self.n_gen = np.zeros(n_seq, int)
        self.tok = np.zeros(n_seq, int)
        self.pos = np.zeros(n_seq, int)

    def load(self, hist_k, hist_v, seq, n):
        self.k[seq, :n], self.v[seq, :n] = hist_k[:n], hist_v[:n]

    def kv_of(self, tok, pos):
        x = self.E[tok]
        return np.roll(x @ self.Wk, pos % D) * np.cos(0.01 * pos), x @ self.Wv

    def forward(self, toks, pos):
        n, slip = self.n_seq, self.slip
        xs, scores = [], []
        for s in range(n):  # QKV: the KV row of row s
            kk, vv = self.kv_of(toks[s], pos[s])
            dst = (s + 1) % n if slip == "cache_write" else s
            self.k[dst, pos[s]], self.v[dst, pos[s]] = kk, vv
            xs.append(self.E[toks[s]])
        att = [None] * n
        pending = []
        for s in range(n):  # attention units
            src = 0 if slip == "cache_read" else s
            kv_len = (pos[0] if slip == "kv_len_row0" else pos[s]) + 1
            sc = self.k[src, :kv_len] @ xs[s]
            ns = -(-kv_len // CHUNK)
            if ns <= HEAD_MAX:
                w = np.exp(sc - sc.max())
                att[s] = (w / w.sum()) @ self.v[src, :kv_len]
                continue
            buf = 0 if slip == "shared_part" else s
            for c in range(ns):
                a, b = c * CHUNK, min(kv_len, (c + 1) * CHUNK)
                m = sc[a:b].max()
                w = np.exp(sc[a:b] - m)
                self.part[buf, c] = np.concatenate([w @ self.v[src, a:b], [m, w.sum()]])
            pending.append((s, buf, ns))
        for s, buf, ns in pending:  # mergers
            p = self.part[buf, :ns]
            M = p[:, D].max()
            c = np.exp(p[:, D] - M)
            att[s] = (c @ p[:, :D]) / (c @ p[:, D + 1])
        return np.stack([(xs[s] + att[s]) @ self.Wc for s in range(n)])

    def generate(self, toks, pos, n_steps, uniforms=None):
        self.tok, self.pos, self.n_gen[:] = np.array(toks), np.array(pos), 0
        for i in range(n_steps):
            lg = self.forward(self.tok, self.pos)
            for s in range(self.n_seq):
                if uniforms is None:
                    t = int(np.argmax(lg[s]))
                else:
                    u = uniforms[0 if self.slip == "uniform_by_step" else s][self.n_gen[s]]
                    t = draw(lg[s], u)
                dst = 0 if self.slip == "commit_buffer" else s
                self.tokens[dst, self.n_gen[s]] = t
                self.n_gen[s] += 1
                self.tok[s], self.pos[s] = t, self.pos[s] + 1
        return self.tokens[:, :n_steps].copy()


def draw(logits, u):
    w = np.exp(logits - logits.max())
    return int(np.searchsorted(np.cumsum(w / w.sum()), u, side="left").clip(0, V - 1))


def hist_kv(toy, hist):
    kv = [toy.kv_of(t, p) for p, t in enumerate(hist)]
    return np.stack([a for a, _ in kv]), np.stack([b for _, b in kv])


def gpu_cases_pass(slip):
    """The checks of tests/test_gpu_batch.py on the model with `slip`; the reference is the
    model without a slip at n_seq = 1 (the single-sequence path). Returns the failed checks."""
    import test_gpu_batch as G  # the very layouts the GPU test uses

    failed = set()
    hist = [int(t) for t in np.random.default_rng(7).integers(1, V, MSL)]
    toks = [5, 17, 11, 2]

    def loaded(n_seq, pos, slip):
        t = Toy(n_seq, slip)
        hk, hv = hist_kv(t, hist)
        for s in range(n_seq):
            t.load(hk, hv, s, pos[s])
        return t

    def single(tok, pos):
        t = loaded(1, [pos], None)
        lg = t.forward([tok], [pos])[0]
        return lg, t.k[0, pos].copy(), t.v[0, pos].copy()

    # 1. identity with the single-sequence path, logits and KV row
    for layout in G.LAYOUTS:
        for n_seq in (1, 2, 3, 4):
            pos = list(layout[:n_seq])
            t = loaded(n_seq, pos, slip)
            lg = t.forward(toks[:n_seq], pos)
            for s in range(n_seq):
                wl, wk, wv = single(toks[s], pos[s])
                if not (np.array_equal(lg[s], wl) and np.array_equal(t.k[s, pos[s]], wk) and np.array_equal(t.v[s, pos[s]], wv)):
                    failed.add("identity")
    # 2. independence: junk past every kv_len
    pos = [300, 0, 64, 130]
    t = loaded(4, pos, slip)
    base = t.forward(toks, pos)
    for s in range(4):
        t.k[s, pos[s] + 1:], t.v[s, pos[s] + 1:] = np.nan, np.inf
    with np.errstate(all="ignore"):
        if not np.array_equal(t.forward(toks, pos), base):
            failed.add("independence")
    # 3. greedy: each sequence's tokens, in its own token buffer, equal the single-sequence loop
    pos = [12, 0, 5, 8]
    t = loaded(4, pos, slip)
    out = t.generate(toks, pos, 6)
    for s in range(4):
        one = loaded(1, [pos[s]], None)
        if out[s].tolist() != one.generate([toks[s]], [pos[s]], 6)[0].tolist():
            failed.add("greedy")
    # 4. sampled: sequences 0 and 1 share a prompt and differ by their uniforms; every token is the
    # rule's on the replayed logits with uniforms[s][i]
    pos, tk = [20, 20, 250], [9, 9, 13]
    u = np.random.default_rng(11).random((3, 10))
    t = loaded(3, pos, slip)
    out = t.generate(tk, pos, 10, uniforms=u)
    r = loaded(3, pos, None)
    cur = list(tk)
    for i in range(10):
        lg = r.forward(cur, [p + i for p in pos])
        if any(out[s, i] != draw(lg[s], u[s, i]) for s in range(3)):
            failed.add("sampled")
            break
        cur = out[:, i].tolist()
    if out[0].tolist() == out[1].tolist():
        failed.add("sampled")
    return failed


def test_the_model_without_a_slip_passes_every_case():
    assert gpu_cases_pass(None) == set()


@pytest.mark.parametrize("slip", SLIPS)
def test_the_gpu_cases_catch_each_slip(slip):
    failed = gpu_cases_pass(slip)
    print(slip, "->", sorted(failed))
    assert failed, f"{slip}: every case of test_gpu_batch.py would pass a kernel with this slip"
    want = {"cache_read": "identity", "cache_write": "identity", "shared_part": "identity", "kv_len_row0": "identity",
            "commit_buffer": "greedy", "uniform_by_step": "sampled"}[slip]
    assert want in failed, (slip, failed)


def test_shared_partial_buffer_needs_two_sequences_in_key_mode():
    """Why LAYOUTS has two positions >= 256 in one batch: with one key-mode sequence a shared
    partial buffer goes unnoticed."""
    import test_gpu_batch as G

    assert any(sum(p >= HEAD_MAX * CHUNK for p in lay[:n]) >= 2 for lay in G.LAYOUTS for n in (2, 3, 4))
    assert G.MSL == MSL and HEAD_MAX * CHUNK == 256
