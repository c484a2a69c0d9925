"""GPU: speculative sampled decode (yalm_generate_speculative_sampled, csrc/spec.h + sampler.h).

Everything is exact. The hook's rows against the integer rule of tests/sampling_ref.py fed the
device's own weights; the loop against a step-by-step host replay on a second decoder (the same
kernels on the same inputs give the same bits, as test_gpu_sampling.test_sampled_loop relies on);
and against the plain sampled loop on uniforms placed mid-interval, with the room to the interval's
ends checked against the measured difference between the two paths' logits.
"""
import functools

import numpy as np
import pytest

import sampling_ref as R
import spec_ref as S
from test_gpu_sampling import combos, make_logits
from yalm_amd import models as M

pytestmark = pytest.mark.gpu

ROW_KINDS = ["gauss3", "plateaus", "neginf", "gauss8"]  # row t of a call: a different vector each


def rt():
    from yalm_amd import runtime

    return runtime


# ------------------------------------------------------------------ 1. the hook against the rule
@functools.lru_cache(maxsize=None)
def hook_rows(n):
    rows = np.stack([make_logits(ROW_KINDS[t], n, seed=t + 1) for t in range(4)])
    rows.setflags(write=False)
    return rows


def some_combos(n):
    c = combos(n)
    return c if len(c) <= 12 else c[3::5]  # 12 of the 60 of a small vocabulary, every T, k and p among them


def draft_kinds(want):
    """name -> drafts for rows 1..T-1 given the rule's draws `want`."""
    T = len(want)
    right = [int(x) for x in want[:-1]]
    out = {"right": right}
    if T > 1:
        out["first-wrong"] = [right[0] + 1] + right[1:]
        out["last-wrong"] = right[:-1] + [right[-1] + 1]
    if T > 2:
        out["none-middle"] = right[:1] + [S.NONE] + right[2:]
    return out


@pytest.mark.parametrize("n,Ts", [(512, (1, 2, 3, 4)), (4096, (1, 2, 3, 4)), (32000, (1, 2, 3, 4)),
                                  (131072, (1, 2, 3, 4)), (4097, (4,)), (4098, (4,)), (4099, (4,))])
def test_hook_rows_match_rule(n, Ts):
    runtime = rt()
    rows = hook_rows(n)
    u_all = np.random.default_rng(n).random((len(some_combos(n)), 4), dtype=np.float32)
    u_all[0] = [0.0, 1.0, 0.5, 1.0]
    q_of = {}
    seen = set()
    for ci, (temp, k, p) in enumerate(some_combos(n)):
        for t in range(4):
            if (t, temp) not in q_of:
                q_of[t, temp] = runtime.sample(rows[t], temp, 0, 1.0, [0.5])[2]
        rules = [R.Rule(rows[t], q_of[t, temp], k, p) for t in range(4)]
        u = u_all[ci]
        want = [rules[t].draw(u[t]) for t in range(4)]
        for T in Ts:
            kinds = draft_kinds(want[:T])
            name = sorted(kinds)[ci % len(kinds)]
            d = kinds[name]
            drawn, kept, a = runtime.spec_sample_rows(rows[:T], temp, k, p, u[:T], d)
            assert drawn.tolist() == want[:T], (n, T, temp, k, p)
            assert kept.tolist() == [r.kept for r in rules[:T]], (n, T, temp, k, p)
            assert a == S.accept(d, want[:T]), (n, T, name, d, want[:T])
            seen.add(name)
    assert seen == {"right", "first-wrong", "last-wrong", "none-middle"}
    # rows really differ: reading row 0 for every t would have given row 0's token everywhere
    plain = [R.Rule(rows[t], q_of[t, 1.0], 0, 1.0).draw(0.5) for t in range(4)]
    assert len(set(plain)) == 4


@pytest.mark.parametrize("n", [4096, 4099])
def test_hook_plateau_cut_in_one_row(n):
    """Row 1 alone has plateaus: top_k = 50 keeps 20 of its 40 logits at +5 (the lowest indices),
    top_p = 0.5 part of its 30 at +6; the other rows have no equal logits at the cut."""
    runtime = rt()
    rows = hook_rows(n)
    u = np.array([0.3, 0.97, 0.6, 0.1], np.float32)
    q = [runtime.sample(rows[t], 1.0, 0, 1.0, [0.5])[2] for t in range(4)]
    for k, p in ((50, 1.0), (0, 0.5), (50, 0.5)):
        rules = [R.Rule(rows[t], q[t], k, p) for t in range(4)]
        want = [rules[t].draw(u[t]) for t in range(4)]
        drawn, kept, a = runtime.spec_sample_rows(rows, 1.0, k, p, u, want[:3])
        assert drawn.tolist() == want and kept.tolist() == [r.kept for r in rules] and a == 4
    r50 = R.Rule(rows[1], q[1], 50, 1.0)
    five = np.flatnonzero(rows[1] == 5.0)
    assert np.array_equal(np.flatnonzero(r50.mask & (rows[1] == 5.0)), five[:20])
    assert 0 < R.Rule(rows[1], q[1], 0, 0.5).kept < 30
    for t in (0, 2, 3):  # the cut of the other rows is between distinct logits
        l = np.sort(rows[t][np.isfinite(rows[t])])[::-1]
        assert l[49] != l[50]


def test_hook_none_draft_after_a_draw_of_token_0():
    runtime = rt()
    rows = hook_rows(512).copy()
    rows[0, 0] = 40.0  # row 0 draws token 0 whatever the uniform
    for d in ([S.NONE, 5, 5], [0, S.NONE, 5]):
        drawn, _, a = runtime.spec_sample_rows(rows, 1.0, 40, 0.9, [0.7, 0.2, 0.4, 0.9], d)
        assert drawn[0] == 0
        assert a == S.accept(d, drawn.tolist())
    drawn, _, a = runtime.spec_sample_rows(rows, 1.0, 40, 0.9, [0.7, 0.2, 0.4, 0.9], [S.NONE, 5, 5])
    assert a == 1  # "none" is not token 0


# ------------------------------------------------------------------ 2. the loop against a host replay
TEMP, TOP_K, TOP_P = 0.8, 40, 0.9
PROMPT = [1, 17, 300, 5, 42, 9, 250, 33, 2, 77, 5]
DTYPES = {"f32": M.F32, "f16": M.F16, "fp8": M.F8E5M2, "e4m3": M.E4M3}


def hydrated(runtime, dm, prompt):
    dec = runtime.Decoder(dm)
    for p, t in enumerate(prompt[:-1]):
        dec.forward(t, p, runtime.HYDRATE_KV_CACHE)
    return dec


def streams(true, vocab):
    true = [int(t) for t in true]
    return {
        "ngram": None,
        "true": true,
        "wrong": [(t + 1) % vocab for t in true],
        "third": [(t + 1) % vocab if j % 3 == 2 else t for j, t in enumerate(true)],
    }


def replay(runtime, dec, prompt, n, rows, u, stream, cfg, prm=(TEMP, TOP_K, TOP_P)):
    """The call step by step on the host: forward_rows, the yalm_sample hook per row with
    uniforms[n_gen + t], spec_ref's drafts and acceptance."""
    ctx, token, pos, out = list(prompt), prompt[-1], len(prompt) - 1, []
    steps = acc = plain = 0
    while len(out) < n:
        ng = len(out)
        if pos + rows > cfg.max_seq_len:
            t = dec.generate_sampled(token, pos, 1, *prm, uniforms=u[ng:ng + 1])[0]
            out.append(t)
            token, pos, plain = t, pos + 1, plain + 1
            continue
        d = S.stream_drafts(stream, ng, rows) if stream is not None else S.draft(ctx + out, rows, 3, 1)
        d = [x if 0 <= x < cfg.vocab_size else S.NONE for x in d]
        lg = dec.forward_rows([token] + [x if x != S.NONE else 0 for x in d], pos)
        drawn = [int(runtime.sample(lg[t], *prm, [u[min(ng + t, n - 1)]])[0][0]) for t in range(rows)]
        a = S.accept(d, drawn)
        out += drawn[:a]
        token, pos, steps, acc = drawn[a - 1], pos + a, steps + 1, acc + a - 1
    over = len(out) - n
    return out[:n], {"spec_steps": steps, "accepted_drafts": acc - over, "plain_steps": plain}


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("size", ["tiny", "small"])
def test_loop_matches_host_replay(size, dtype):
    runtime = rt()
    cfg = (M.TINY if size == "tiny" else M.SMALL).with_(max_seq_len=64, weight_dtype=DTYPES[dtype])
    n, pos = 24, len(PROMPT) - 1
    u = np.random.default_rng(7).random(n, dtype=np.float32)
    dm = runtime.DeviceModel.synthetic(cfg, seed=3)
    try:
        twin = hydrated(runtime, dm, PROMPT)
        plain = twin.generate_sampled(PROMPT[-1], pos, n, TEMP, TOP_K, TOP_P, uniforms=u)
        twin.close()
        distinct = 0
        for rows in (2, 3, 4):
            for kind, stream in streams(plain, cfg.vocab_size).items():
                dec, ref = hydrated(runtime, dm, PROMPT), hydrated(runtime, dm, PROMPT)
                try:
                    want, wst = replay(runtime, ref, PROMPT, n, rows, u, stream, cfg)
                    got, st = dec.generate_speculative_sampled(PROMPT[-1], pos, n, TEMP, TOP_K, TOP_P, uniforms=u,
                                                               rows=rows, context=PROMPT, draft_stream=stream)
                    assert got == want, (rows, kind)
                    assert {k: st[k] for k in wst} == wst, (rows, kind, st, wst)
                    assert st["launches_per_step"] == 5 + cfg.n_layers * (4 + rows)
                    distinct = max(distinct, len(set(got)))
                    assert dec.device_step() == (got[-1], pos + n)
                    assert dec.device_tokens() == got
                    dec.enqueue_greedy(3)
                    assert dec.device_step()[1] == pos + n + 3
                    cont = dec.device_tokens()
                    assert cont[:n] == got and len(cont) == n + 3
                    assert cont[n:] == ref.generate_greedy(got[-1], pos + n, 3)
                finally:
                    dec.close()
                    ref.close()
        assert distinct > 4
    finally:
        dm.close()


# ------------------------------------------------------------------ 3. equality with the plain sampled loop
SHARE = 0.02  # the chosen token's kept interval is at least this share of S; u sits at its centre


def unstable_mass(l, q, delta, eps):
    """Share of S held by tokens whose place in the kept set can differ between two logit vectors
    within delta of each other: those within 2 delta of a top-k cut that is itself closer than 2
    delta, and those at which the top-p prefix is within 4 eps of top_p."""
    order = np.lexsort((np.arange(l.size), -l.astype(np.float64)))
    ls, qs = l[order].astype(np.float64), q[order].astype(np.float64)
    kk = min(TOP_K, l.size)
    bad = np.zeros(l.size, bool)
    if kk < l.size and ls[kk - 1] - ls[kk] <= 2 * delta:
        bad |= (np.abs(ls - ls[kk - 1]) <= 2 * delta) | (np.abs(ls - ls[kk]) <= 2 * delta)
    before = np.concatenate([[0.0], np.cumsum(qs[:kk])[:-1]]) / max(qs[:kk].sum(), 1.0)
    bad[:kk] |= np.abs(before - TOP_P) <= 4 * eps
    kept_S = float(R.Rule(l, q, TOP_K, TOP_P).S)
    return float(qs[bad].sum() / max(kept_S, 1.0))


EQ_CASES = [("tiny", "f16"), ("small", "f16"), ("small", "fp8"), ("small", "e4m3")]


@pytest.mark.parametrize("size,dtype", EQ_CASES)
def test_equals_plain_sampled_loop(size, dtype):
    """u[i] = the centre of the kept interval of a token picked by a seeded generator among the
    kept tokens with at least SHARE of S, on the plain path's logits. Two logit vectors within
    delta of each other give weights within a factor e^(2 delta / T) (both l_i and m move), so
    every cumulative share moves by at most 2 eps, eps = e^(2 delta / T) - 1, plus twice the share
    of tokens whose membership of the kept set can change (unstable_mass). delta is measured: the
    largest |forward_rows - forward| over the positions the sequence visits, rows 2, 3 and 4."""
    runtime = rt()
    cfg = (M.TINY if size == "tiny" else M.SMALL).with_(max_seq_len=64, weight_dtype=DTYPES[dtype])
    n, pos = 32, len(PROMPT) - 1
    rng = np.random.default_rng(5)
    dm = runtime.DeviceModel.synthetic(cfg, seed=3)
    try:
        a = hydrated(runtime, dm, PROMPT)
        u, seq, logits, qs, tok = np.zeros(n, np.float32), [], [], [], PROMPT[-1]
        for i in range(n):
            l = a.forward(tok, pos + i).copy()
            q = runtime.sample(l, TEMP, 0, 1.0, [0.5])[2]
            rule = R.Rule(l, q, TOP_K, TOP_P)
            cum = rule.cum.astype(np.float64)
            lo = np.concatenate([[0.0], cum[:-1]])
            wide = np.flatnonzero(rule.mask & ((cum - lo) >= SHARE * rule.S))
            assert wide.size > 0, f"step {i}: no kept token holds {SHARE} of S"
            t = int(rng.choice(wide))
            u[i] = np.float32((lo[t] + cum[t]) / 2 / rule.S)
            assert rule.draw(u[i]) == t
            seq.append(t)
            logits.append(l)
            qs.append(q)
            tok = t
        a.close()
        assert len(set(seq)) > 4
        # the two paths' logits along the sequence
        fed = [PROMPT[-1]] + seq[:-1]
        delta = 0.0
        for rows in (2, 3, 4):
            b = hydrated(runtime, dm, PROMPT)
            for j in range(0, n, rows):
                lg = b.forward_rows(fed[j:j + rows], pos + j)
                for t in range(lg.shape[0]):
                    delta = max(delta, float(np.max(np.abs(lg[t] - logits[j + t]))))
            b.close()
        eps = float(np.expm1(2 * delta / TEMP))
        shift = max(2 * eps + 2 * unstable_mass(logits[i], qs[i], delta, eps) for i in range(n))
        print(f"{size}-{dtype}: max |dlogit| {delta:.3e}, cumulative shift bound {shift:.3e}, margin {SHARE / 2}")
        assert shift < SHARE / 2

        b = hydrated(runtime, dm, PROMPT)
        plain = b.generate_sampled(PROMPT[-1], pos, n, TEMP, TOP_K, TOP_P, uniforms=u)
        b.close()
        assert plain == seq
        for rows in (2, 3, 4):
            for kind, stream in streams(seq, cfg.vocab_size).items():
                d = hydrated(runtime, dm, PROMPT)
                try:
                    got, st = d.generate_speculative_sampled(PROMPT[-1], pos, n, TEMP, TOP_K, TOP_P, uniforms=u,
                                                             rows=rows, context=PROMPT, draft_stream=stream)
                    assert got == plain, (rows, kind)
                    if kind == "true":
                        _, want, _ = S.predict(seq + [0] * 4, PROMPT[-1], n, rows, context=PROMPT, stream=stream,
                                               pos=pos, max_seq_len=cfg.max_seq_len, vocab=cfg.vocab_size)
                        assert {k: st[k] for k in want} == want and st["spec_steps"] == -(-n // rows)
                    # top_k = 1 is the greedy speculative loop whatever the uniforms
                    g1, _ = d.generate_speculative_sampled(PROMPT[-1], pos, n, TEMP, 1, 1.0, uniforms=u, rows=rows,
                                                           context=PROMPT, draft_stream=stream)
                    g2, _ = d.generate_speculative(PROMPT[-1], pos, n, rows=rows, context=PROMPT, draft_stream=stream)
                    assert g1 == g2, (rows, kind)
                finally:
                    d.close()
    finally:
        dm.close()


# ------------------------------------------------------------------ 4. the window's end
def test_window_end():
    runtime = rt()
    cfg = M.TINY.with_(max_seq_len=24)
    n, pos = 24, len(PROMPT) - 1
    u = np.random.default_rng(9).random(n + 6, dtype=np.float32)
    dm = runtime.DeviceModel.synthetic(cfg, seed=3)
    try:
        for rows, kind in ((4, "ngram"), (4, "true"), (2, "ngram")):
            twin = hydrated(runtime, dm, PROMPT)
            plain = twin.generate_sampled(PROMPT[-1], pos, n, TEMP, TOP_K, TOP_P, uniforms=u[:n])
            twin.close()
            stream = streams(plain, cfg.vocab_size)[kind]
            dec, ref = hydrated(runtime, dm, PROMPT), hydrated(runtime, dm, PROMPT)
            try:
                want, wst = replay(runtime, ref, PROMPT, n, rows, u[:n], stream, cfg)
                got, st = dec.generate_speculative_sampled(PROMPT[-1], pos, n, TEMP, TOP_K, TOP_P, uniforms=u[:n],
                                                           rows=rows, context=PROMPT, draft_stream=stream)
                assert got == want and {k: st[k] for k in wst} == wst
                assert st["plain_steps"] > 0 and st["spec_steps"] > 0
                assert dec.device_step() == (got[-1], pos + n)
                # a call that starts past the window runs the plain sampled kernels alone
                more, st2 = dec.generate_speculative_sampled(got[-1], pos + n, 6, TEMP, TOP_K, TOP_P, uniforms=u[n:],
                                                             rows=rows, context=PROMPT + got)
                assert st2["spec_steps"] == 0 and st2["plain_steps"] == 6
                assert more == ref.generate_sampled(got[-1], pos + n, 6, TEMP, TOP_K, TOP_P, uniforms=u[n:])
            finally:
                dec.close()
                ref.close()
    finally:
        dm.close()


# ------------------------------------------------------------------ 5. refusals and arguments
def test_refusals_and_arguments():
    runtime = rt()

    def refused(dec, what):
        with pytest.raises(runtime.YalmError, match=f"error 3.*{what}"):
            dec.generate_speculative_sampled(1, 0, 4, 1.0, rows=2)

    dm = runtime.DeviceModel.synthetic(M.SMALL.with_(weight_dtype=M.Q4, n_layers=1), seed=1)
    dec = runtime.Decoder(dm)
    try:
        refused(dec, "q4")
        dec.forward(1, 0)
    finally:
        dec.close()
        dm.close()
    dm = runtime.DeviceModel.synthetic(M.TINY_MOE, seed=1)
    dec = runtime.Decoder(dm)
    try:
        refused(dec, "mixture-of-experts")
    finally:
        dec.close()
        dm.close()
    dm = runtime.DeviceModel.synthetic(M.SMALL, seed=1)
    dec = runtime.Decoder(dm, tp_gather=lambda h: [h])
    try:
        refused(dec, "tensor-parallel")
    finally:
        dec.close()
    dec = runtime.Decoder(dm)
    try:
        bad = [dict(temperature=0.0), dict(temperature=float("nan")), dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.5),
               dict(uniforms=[0.5, -0.1, 0.5, 0.5]), dict(uniforms=[0.5, 0.5, 0.5, 1.1]), dict(rows=1), dict(rows=5),
               dict(context=[1, 2])]
        for kw in bad:
            args = dict(temperature=1.0, top_k=0, top_p=1.0, uniforms=[0.5] * 4, rows=2)
            args.update(kw)
            with pytest.raises(runtime.YalmError, match="yalm error 2"):
                dec.generate_speculative_sampled(1, 0, 4, **args)
        with pytest.raises(runtime.YalmError, match="error 2.*token buffer"):
            dec.generate_speculative_sampled(1, 0, 65537, 1.0, uniforms=np.zeros(65537, np.float32), rows=2)
        assert dec.generate_speculative_sampled(1, 0, 0, 1.0)[0] == []
        with pytest.raises(runtime.YalmError, match="yalm error 2"):
            runtime.spec_sample_rows(np.zeros((2, 16), np.float32), 0.0, uniforms=[0.5, 0.5], drafts=[1])
        with pytest.raises(runtime.YalmError, match="yalm error 2"):
            runtime.spec_sample_rows(np.zeros((1, 131073), np.float32), 1.0, uniforms=[0.5])
        # and the decoder still decodes
        got, st = dec.generate_speculative_sampled(1, 0, 6, 0.8, 40, 0.9, seed=3, rows=3)
        assert len(got) == 6 and st["launches_per_step"] == 5 + M.SMALL.n_layers * (4 + 3)
        assert got == dec.generate_speculative_sampled(1, 0, 6, 0.8, 40, 0.9, rows=3,
                                                       uniforms=np.random.default_rng(3).random(6, dtype=np.float32))[0]
        assert dec.time_kernel(12, 2) > 0 and dec.time_kernel(13, 2) > 0 and dec.time_kernel(14, 2) > 0
        assert dec.kernel_name(13) == "spec_accept_kernel"
    finally:
        dec.close()
        dm.close()
