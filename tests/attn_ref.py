"""Float64 numpy reference of decode attention (yalm_mha) and the case table shared by
test_attn_cpu.py (which checks the table and the reference on the CPU) and test_gpu_attention.py
(which runs every case on the device). TEST INFRASTRUCTURE ONLY.

The table: every (head_dim, G = n_heads / n_kv_heads) pair the dispatcher accepts, head_dim in
{16, 32, 64, 128, 256} x G in 1 .. 8, with two kv heads (so the group index matters, and for a G
that is no template width the last group's masked heads sit beside nothing). Windows and key
lengths are chosen from the kernel's constants (64-key chunks, head mode up to 4 chunks, at most
32 key splits):
  max_seq_len  330: 6 chunks, S = 6, the last chunk partial; head mode up to 256 keys, key mode
                    from 257 (one chunk per split)
  max_seq_len 4224: 66 chunks, S = 32: every split holds 2 or 3 chunks (the A / B prefetch loop)
  max_seq_len   64: one chunk, S = 1: head mode whatever the key count
Every case is seeded by its name. K and V rows t < kv_len are random normal and q is 2 x random
normal (as test_gpu_kernels.py::test_mha_shapes), with planted keys: flavour "ends" gives key 0
and key kv_len - 1, for every head of the group at once, the score that puts about a quarter of
the head's probability on each; flavour "last" makes key kv_len - 1 alone hold about half of it
(the largest score of the row sits in the last live chunk, so the running-max rescale fires on
the final chunk of a unit) and key 0 e^-3 of that. Rows t >= kv_len are poison: f16 NaN (0x7E00)
or +inf. mha_ref never reads them.
"""
import functools
import zlib

import numpy as np

CHUNK, HEAD_MAX, SPLITS = 64, 4, 32  # attention.h: attn_chunk, ATTN_HEAD_MAX, ATTN_SPLITS
N_KV = 2
HEAD_DIMS = (16, 32, 64, 128, 256)
GROUPS = tuple(range(1, 9))
PAIRS = [(d, g) for d in HEAD_DIMS for g in GROUPS]
WINDOWS = {330: (1, 63, 64, 65, 256, 257, 320, 321, 330), 4224: (2049, 4097, 4224), 64: (1, 64)}
FLAVOURS = ("ends", "last")
POISONS = {"nan": 0x7E00, "inf": 0x7C00}
SENTINEL = -7.25  # att entries t >= kv_len must come back as they went in
# the project's bars of test_mha_shapes, here against float64
X_ATOL, X_RTOL = 2e-5, 1e-4
A_ATOL, A_RTOL = 2e-6, 1e-4


def mode_of(kv_len, max_seq_len):
    """"head" or "key": the launch's mode (yalm_hip.hip launch_attn_D / attn_head_max)."""
    nchunks = -(-max_seq_len // CHUNK)
    S = min(nchunks, SPLITS)
    hmax = nchunks if S <= 1 else HEAD_MAX
    return "head" if -(-kv_len // CHUNK) <= hmax else "key"


def mha_ref(kb, vb, q, head_dim, kv_len, max_seq_len, n_heads, n_kv_heads, att_init=None, q_of_head=None, drop=()):
    """(xout, att) of O.mha in float64: head h reads kv head h // G, scores q . k / sqrt(head_dim),
    rows t < kv_len only. att (n_heads * max_seq_len) starts as att_init (zeros without one) and
    only entries t < kv_len are written. The mutants of test_attn_cpu.py: q_of_head maps a head to
    the head whose q it uses; drop lists keys left out (their att entries stay as they were)."""
    kv_dim = n_kv_heads * head_dim
    K = np.asarray(kb, np.float16).reshape(-1, kv_dim)[:kv_len].astype(np.float64)
    V = np.asarray(vb, np.float16).reshape(-1, kv_dim)[:kv_len].astype(np.float64)
    q = np.asarray(q, np.float32).astype(np.float64).reshape(n_heads, head_dim)
    G = n_heads // n_kv_heads
    keep = np.setdiff1d(np.arange(kv_len), np.asarray(drop, np.int64))
    xout = np.zeros((n_heads, head_dim))
    att = np.zeros(n_heads * max_seq_len) if att_init is None else np.array(att_init, np.float64)
    att = att.reshape(n_heads, max_seq_len)
    for g in range(n_kv_heads if keep.size else 0):
        Kg, Vg = (a[keep, g * head_dim:(g + 1) * head_dim] for a in (K, V))
        for h in range(g * G, (g + 1) * G):  # head h reads kv head h // G
            s = Kg @ q[h if q_of_head is None else q_of_head(h)] / np.sqrt(head_dim)
            p = np.exp(s - s.max())
            p /= p.sum()
            xout[h] = p @ Vg
            att[h, keep] = p
    return xout.reshape(-1), att.reshape(-1)


def next_head_in_group(G, n_heads):
    """The first mutant's map: head h uses head h + 1's q, wrapping inside the group. A group of
    one head has no other head: G = 1 wraps over all the heads instead (the other kv head's)."""
    if G == 1:
        return lambda h: (h + 1) % n_heads
    return lambda h: (h // G) * G + (h % G + 1) % G


class Case:
    __slots__ = ("name", "head_dim", "G", "max_seq_len", "kv_len", "flavour", "poison", "mode", "n_heads", "n_kv")

    def __init__(self, head_dim, G, max_seq_len, kv_len, flavour, poison):
        self.head_dim, self.G, self.max_seq_len, self.kv_len = head_dim, G, max_seq_len, kv_len
        self.flavour, self.poison = flavour, poison
        self.n_kv, self.n_heads = N_KV, N_KV * G
        self.mode = mode_of(kv_len, max_seq_len)
        self.name = f"d{head_dim}-g{G}-w{max_seq_len}-kv{kv_len}-{flavour}-{poison}"

    def __repr__(self):
        return self.name


def _table():
    out = []
    for pi, (d, g) in enumerate(PAIRS):
        n = 0
        for msl, kvs in WINDOWS.items():
            for kv in kvs:
                for fi, fl in enumerate(FLAVOURS):
                    if fl == "last" and kv <= CHUNK:
                        continue  # one live chunk: nothing before the last chunk to rescale
                    # poisons alternate along a pair's key lengths, the two flavours of a length
                    # take one each, and every second pair starts with the other: each pair has
                    # both poisons with both flavours in both modes
                    out.append(Case(d, g, msl, kv, fl, ("nan", "inf")[(n + pi + fi) % 2]))
                n += 1
    return out


CASES = _table()
BY_PAIR = {p: [c for c in CASES if (c.head_dim, c.G) == p] for p in PAIRS}


def _plant(K, q, c, key, scores):
    """K row `key`: for each kv head the minimum-norm row whose score with head h of its group
    is scores[h] (G <= 8 equations, head_dim >= 16 unknowns), rounded to f16."""
    D, G = c.head_dim, c.G
    for g in range(c.n_kv):
        Q = q[g * G:(g + 1) * G].astype(np.float64)
        K[key, g * D:(g + 1) * D] = (np.linalg.pinv(Q) @ (scores[g * G:(g + 1) * G] * np.sqrt(D))).astype(np.float16)


@functools.lru_cache(maxsize=4)
def inputs(name):
    """(kb, vb, q) of the case: f16 (max_seq_len * kv_dim), f16, f32 (n_heads * head_dim); read-only."""
    c = {k.name: k for k in CASES}[name]
    D, n = c.head_dim, c.kv_len
    kv_dim = c.n_kv * D
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    K = np.empty((c.max_seq_len, kv_dim), np.float16)
    V = np.empty((c.max_seq_len, kv_dim), np.float16)
    K[:n] = rng.standard_normal((n, kv_dim)).astype(np.float16)
    V[:n] = rng.standard_normal((n, kv_dim)).astype(np.float16)
    q = (rng.standard_normal((c.n_heads, D)) * 2).astype(np.float32)
    # the sum of e^score over the keys that are not planted, per head
    rest = np.zeros(c.n_heads)
    mid = slice(1, n - 1)
    for g in range(c.n_kv):
        s = K[mid, g * D:(g + 1) * D].astype(np.float64) @ q[g * c.G:(g + 1) * c.G].astype(np.float64).T / np.sqrt(D)
        rest[g * c.G:(g + 1) * c.G] = np.exp(s).sum(axis=0)
    if n <= 2:  # nothing but planted keys
        s_last = np.ones(c.n_heads)
        s_first = s_last if c.flavour == "ends" else s_last - 3.0
    elif c.flavour == "ends":  # e^s = rest / 2 each: a quarter of the mass each
        s_last = s_first = np.log(rest / 2)
    else:  # e^s_last = rest + e^s_first, s_first = s_last - 3
        s_last = np.log(rest / (1.0 - np.exp(-3.0)))
        s_first = s_last - 3.0
    _plant(K, q, c, 0, s_first)
    if n > 1:
        _plant(K, q, c, n - 1, s_last)
    K.view(np.uint16)[n:] = POISONS[c.poison]
    V.view(np.uint16)[n:] = POISONS[c.poison]
    kb, vb, q = K.reshape(-1), V.reshape(-1), q.reshape(-1)
    for a in (kb, vb, q):
        a.setflags(write=False)
    return kb, vb, q


def att_init(c):
    return np.full(c.n_heads * c.max_seq_len, SENTINEL, np.float32)


def reference(c):
    """mha_ref of the case over a sentinel-filled att."""
    kb, vb, q = inputs(c.name)
    return mha_ref(kb, vb, q, c.head_dim, c.kv_len, c.max_seq_len, c.n_heads, c.n_kv, att_init=att_init(c))


def live(c, att):
    """att (n_heads * max_seq_len) -> (entries t < kv_len, entries t >= kv_len), per head."""
    a = np.asarray(att).reshape(c.n_heads, c.max_seq_len)
    return a[:, :c.kv_len], a[:, c.kv_len:]


def bars(got, want, atol, rtol):
    """max |got - want| / (atol + rtol |want|): 1.0 is numpy.testing.assert_allclose's edge."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.abs(got - want) / (atol + rtol * np.abs(want)))) if want.size else 0.0
