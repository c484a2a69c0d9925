"""CPU: the conditions that keep tests/test_gpu_attention.py honest -- the case table of
attn_ref.py is complete, its float64 reference is what the f32 oracle computes to within the GPU
test's bars, and three wrong attentions are far from it at every case."""
import numpy as np
import pytest

import attn_ref as A
import oracle_py as O

# the oracle at the 4224-key window: head dims small / mid / large x a one-head group, a group
# that is no template width and the widest
BIG_WINDOW_PAIRS = [(16, 7), (64, 1), (64, 8), (128, 5), (256, 3), (256, 8)]
MUTANT_BARS = 10.0


def test_table_is_complete():
    """All 40 (head_dim, G) pairs; for each, every key length of every window, head mode and key
    mode each with both poisons and both flavours; every name unique."""
    assert len(A.PAIRS) == 40 and set(A.PAIRS) == {(d, g) for d in (16, 32, 64, 128, 256) for g in range(1, 9)}
    assert A.WINDOWS == {330: (1, 63, 64, 65, 256, 257, 320, 321, 330), 4224: (2049, 4097, 4224), 64: (1, 64)}
    assert len({c.name for c in A.CASES}) == len(A.CASES)
    assert set(A.BY_PAIR) == set(A.PAIRS)
    for pair, cases in A.BY_PAIR.items():
        assert all(c.n_kv == 2 and c.n_heads == 2 * c.G for c in cases)
        for msl, kvs in A.WINDOWS.items():
            for kv in kvs:
                fl = {c.flavour for c in cases if (c.max_seq_len, c.kv_len) == (msl, kv)}
                assert fl == ({"ends", "last"} if kv > A.CHUNK else {"ends"}), (pair, msl, kv)
        for mode in ("head", "key"):
            got = {(c.poison, c.flavour) for c in cases if c.mode == mode}
            assert got == {(p, f) for p in A.POISONS for f in A.FLAVOURS}, (pair, mode, got)
    # the modes as the launch decides them (attention.h / yalm_hip.hip constants)
    assert [A.mode_of(kv, 330) for kv in (256, 257)] == ["head", "key"]
    assert A.mode_of(64, 64) == "head" and A.mode_of(2049, 4224) == "key"
    assert (A.CHUNK, A.HEAD_MAX, A.SPLITS) == (64, 4, 32)


def test_poison_and_planted_mass():
    """Rows past kv_len are the poison bit pattern, rows before it finite; the planted keys hold
    roughly half of every head's probability ("ends": both ends together; "last": the last key)
    and "last" has its largest score in the last live chunk."""
    for c in A.BY_PAIR[(16, 8)] + A.BY_PAIR[(128, 5)] + A.BY_PAIR[(256, 1)]:
        kb, vb, _ = A.inputs(c.name)
        kv_dim = c.n_kv * c.head_dim
        for b in (kb, vb):
            r = b.view(np.uint16).reshape(c.max_seq_len, kv_dim)
            assert np.all(r[c.kv_len:] == A.POISONS[c.poison])
            assert np.all(np.isfinite(b.reshape(c.max_seq_len, kv_dim)[:c.kv_len].astype(np.float32)))
        if c.kv_len <= 2:
            continue
        _, att = A.reference(c)
        p, _ = A.live(c, att)
        if c.flavour == "ends":
            mass = p[:, 0] + p[:, -1]
            assert np.all(p[:, 0] > 0.15) and np.all(p[:, -1] > 0.15), c
        else:
            mass = p[:, -1]
            assert np.all(np.argmax(p, axis=1) == c.kv_len - 1), c
            assert np.all(p[:, 0] > 0.01), c
        assert np.all((mass > 0.4) & (mass < 0.6)), (c, mass)


def _oracle_bars(c):
    kb, vb, q = A.inputs(c.name)
    xo, ao = O.mha(kb, vb, q, c.head_dim, c.kv_len, c.max_seq_len, c.n_heads, c.n_kv)
    xr, ar = A.reference(c)
    assert np.all(np.isfinite(xo))
    return (A.bars(xo, xr, A.X_ATOL, A.X_RTOL), A.bars(A.live(c, ao)[0], A.live(c, ar)[0], A.A_ATOL, A.A_RTOL))


@pytest.mark.parametrize("window", sorted(A.WINDOWS))
def test_oracle_meets_the_gpu_bars(window):
    """The f32 oracle (O.mha, the reference's CPU attention) against mha_ref at the GPU test's
    bars (xout 2e-5 + 1e-4 |x|, att 2e-6 + 1e-4 |p|): every pair and key length of the two small
    windows, BIG_WINDOW_PAIRS at the 4224-key one. The oracle takes every head_dim and reads
    only rows t < kv_len, so no case is ruled out. A correct f32 attention therefore reaches the
    bars with planted keys at 4224 keys; the GPU test keeps them for every window. Measured worst
    error in bars (xout, att): window 64: 0.094, 0.030; window 330: 0.144, 0.045; window 4224:
    0.093, 0.046 -- all under half a bar, so no window has a bar of its own."""
    worst = [0.0, 0.0]
    for c in A.CASES:
        if c.max_seq_len != window or (window == 4224 and (c.head_dim, c.G) not in BIG_WINDOW_PAIRS):
            continue
        bx, ba = _oracle_bars(c)
        worst = [max(worst[0], bx), max(worst[1], ba)]
        assert bx < 1.0 and ba < 1.0, (c, bx, ba)
    print(f"window {window}: the oracle's worst error in bars: xout {worst[0]:.3f}, att {worst[1]:.3f}")
    assert max(worst) < 0.5, worst  # above half a bar the GPU bar of that window would be re-derived


@pytest.mark.parametrize("head_dim", A.HEAD_DIMS)
def test_mutants_are_far(head_dim):
    """Three wrong attentions are at least 10 bars from mha_ref in xout at every case: head h
    using the next head's q (wrapping inside the group; G = 1: over all heads), key kv_len - 1
    dropped, key 0 dropped. With one key the softmax is 1 whatever q is, so the first mutant is
    the true attention at kv_len = 1 and is not asked there (the dropped key is: xout = 0)."""
    for c in A.CASES:
        if c.head_dim != head_dim:
            continue
        kb, vb, q = A.inputs(c.name)
        args = (kb, vb, q, c.head_dim, c.kv_len, c.max_seq_len, c.n_heads, c.n_kv)
        xr, _ = A.reference(c)
        mutants = {"last key dropped": dict(drop=(c.kv_len - 1,)), "key 0 dropped": dict(drop=(0,))}
        if c.kv_len > 1:
            mutants["next head's q"] = dict(q_of_head=A.next_head_in_group(c.G, c.n_heads))
        for what, kw in mutants.items():
            xm, _ = A.mha_ref(*args, **kw)
            d = A.bars(xm, xr, A.X_ATOL, A.X_RTOL)
            assert d >= MUTANT_BARS, (c, what, d)
