"""GPU: device-side temperature / top-k / top-p sampling (csrc/sampler.h).

Everything except the weight bound is exact equality against the integer rule of
tests/sampling_ref.py fed the device's own fixed-point weights (yalm_sample's weights_out).

Weight bound: |q_i 2^-40 - exp((l_i - m) / T) in f64| <= 1e-5 w + 2^-40: the argument's two f32
roundings at |a| <= 27.7 (below that q is 0) move w by 3.3e-6 w, expf adds its ulps, the
truncation to 40 fractional bits at most 2^-40.
"""
import numpy as np
import pytest

import sampling_ref as R
from yalm_amd import models as M

pytestmark = pytest.mark.gpu

VS = [1, 5, 1000, 4099, 32000, 128256]
KINDS = ["gauss3", "gauss8", "equal", "plateaus", "neginf", "all_neginf"]
TS = [0.25, 1.0, 4.0]
TOP_PS = [1.0, 0.9, 0.5, 1e-6]


def rt():
    from yalm_amd import runtime

    return runtime


def make_logits(kind, V, seed=0):
    rng = np.random.default_rng(seed + 17 * V)
    if kind == "gauss3":
        return (rng.standard_normal(V) * 3).astype(np.float32)
    if kind == "gauss8":
        return (rng.standard_normal(V) * 8).astype(np.float32)
    if kind == "equal":
        return np.full(V, -1.25, np.float32)
    if kind == "plateaus":
        # two plateaus of equal logits above everything else, scattered over the index range:
        # 30 at +6 and 40 at +5 (fewer at small V), so that top_k = 2 or 50 and, with them or
        # alone, top_p = 0.5 or 0.9 cut inside a plateau and i* decides who stays
        l = (rng.standard_normal(V) * 0.5).astype(np.float32)
        a, b = min(30, max(1, V // 3)), min(40, max(1, V // 3))
        idx = rng.permutation(V)
        l[idx[:a]] = 6.0
        l[idx[a:a + b]] = 5.0
        return l
    if kind == "neginf":
        l = (rng.standard_normal(V) * 3).astype(np.float32)
        l[rng.random(V) < 0.3] = -np.inf
        return l
    assert kind == "all_neginf"
    return np.full(V, -np.inf, np.float32)


def combos(V):
    ks = sorted({0, 1, 2, 50, V})
    if V < 10000:
        return [(T, k, p) for T in TS for k in ks for p in TOP_PS]
    # the large vocabularies: every temperature plain, every top_k and top_p alone, mixed pairs
    return [(0.25, 0, 1.0), (1.0, 0, 1.0), (4.0, 0, 1.0), (1.0, 1, 1.0), (1.0, 2, 0.5), (1.0, 50, 1.0),
            (4.0, V, 0.9), (1.0, 0, 0.9), (0.25, 0, 0.5), (4.0, 0, 1e-6), (1.0, 50, 0.9), (4.0, 50, 0.5)]


def check_weights(l, T, q):
    m, _ = R.first_max(l)
    with np.errstate(all="ignore"):
        w = np.exp((l.astype(np.float64) - np.float64(m)) / np.float64(np.float32(T)))
    w = np.where(np.isfinite(w), w, 0.0)
    err = np.abs(q.astype(np.float64) * 2.0 ** -40 - w)
    bound = 1e-5 * w + 2.0 ** -40
    worst = float(np.max(err / bound))
    assert np.all(err <= bound), (T, worst)
    return worst


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("V", VS)
def test_hook_matches_rule(V, kind):
    runtime = rt()
    l = make_logits(kind, V)
    amax = runtime.argmax(l)
    assert amax == R.first_max(l)[1]
    u0 = np.concatenate([np.array([0.0, 1.0], np.float32), np.random.default_rng(3).random(64, dtype=np.float32)])
    worst_w, n_boundary, repeated = 0.0, 0, False
    for T, k, p in combos(V):
        tok, kept, q = runtime.sample(l, T, k, p, u0)
        if k == 0 and p == 1.0:
            worst_w = max(worst_w, check_weights(l, T, q))
        rule = R.Rule(l, q, k, p)
        assert np.array_equal(tok, rule.draws(u0)), (T, k, p)
        assert np.all(kept == rule.kept), (T, k, p, kept[0], rule.kept)
        if k == 1:
            assert np.all(tok == amax), (T, k, p)
        if kind == "all_neginf":
            assert np.all(tok == 0)
        if rule.S > 0:
            # the uniforms at which the token changes, from the device's own q, with both f32 neighbours
            ki = np.flatnonzero(rule.mask & (q > 0))
            ub = rule.boundary_uniforms(ki[[0, len(ki) // 2, -1]])
            tb, kb, qb = runtime.sample(l, T, k, p, ub)
            assert np.array_equal(qb, q)
            assert np.array_equal(tb, rule.draws(ub)), (T, k, p, ub)
            assert np.all(kb == rule.kept)
            n_boundary += ub.size
        if not repeated and (k, p) != (0, 1.0):
            t2, k2, q2 = runtime.sample(l, T, k, p, u0)
            assert np.array_equal(t2, tok) and np.array_equal(k2, kept) and np.array_equal(q2, q)
            repeated = True
    print(f"V={V} {kind}: {len(combos(V))} parameter sets, worst weight error {worst_w:.3f} of the bound, "
          f"{n_boundary} boundary uniforms")


def test_hook_plateau_cuts_use_istar():
    """The plateau case really cuts inside a plateau: top_k = 50 keeps 20 of the 40 logits at +5
    (those of lowest index), top_p = 0.5 keeps only part of the 30 at +6."""
    runtime = rt()
    l = make_logits("plateaus", 4099)
    _, kept, q = runtime.sample(l, 1.0, 50, 1.0, [0.5])
    rule = R.Rule(l, q, 50, 1.0)
    five = np.flatnonzero(l == 5.0)
    assert kept[0] == 50 and np.array_equal(np.flatnonzero(rule.mask & (l == 5.0)), five[:20])
    _, kept, _ = runtime.sample(l, 1.0, 0, 0.5, [0.5])
    assert 0 < kept[0] < 30 and kept[0] == R.Rule(l, q, 0, 0.5).kept


LOOP_CASES = [
    ("tiny-fp16", M.TINY, M.F16), ("tiny-fp8", M.TINY, M.F8E5M2), ("tiny-fp32", M.TINY, M.F32),
    ("small-fp16", M.SMALL, M.F16), ("small-fp8", M.SMALL, M.F8E5M2), ("small-fp32", M.SMALL, M.F32),
    ("tiny-moe-fp16", M.TINY_MOE, M.F16),
]


@pytest.mark.parametrize("case", LOOP_CASES, ids=[c[0] for c in LOOP_CASES])
def test_sampled_loop(case):
    """max_seq_len 24, 40 steps: the ring buffer and the attention sinks are crossed."""
    runtime = rt()
    _, base, dtype = case
    cfg = base.with_(max_seq_len=24, weight_dtype=dtype)
    n, tok0 = 40, 1
    T, k, p = 0.8, 40, 0.9
    u = np.random.default_rng(11).random(n, dtype=np.float32)
    dm = runtime.DeviceModel.synthetic(cfg, seed=3)
    dec = runtime.Decoder(dm)
    try:
        assert dec.graph_kernels(3) == dec.graph_kernels(2)
        # one step at a time: the logits the step sampled from, through the hook, give its token
        seq, tok = [], tok0
        for i in range(n):
            t = dec.generate_sampled(tok, i, 1, T, k, p, uniforms=u[i:i + 1])[0]
            ht, _, _ = runtime.sample(dec.get_logits(), T, k, p, u[i:i + 1])
            assert t == ht[0], (i, t, ht[0])
            seq.append(t)
            tok = t
        assert len(set(seq)) > 4  # a sampled sequence, not one token repeated
        assert dec.generate_sampled(tok0, 0, n, T, k, p, uniforms=u) == seq
        assert dec.device_step() == (seq[-1], n)
        assert dec.device_tokens() == seq
        dec.enqueue_greedy(3)
        assert dec.device_step()[1] == n + 3
        cont = dec.device_tokens()
        assert cont[:n] == seq and len(cont) == n + 3
        assert dec.generate_sampled(tok0, 0, n, T, k, p, uniforms=u) == seq
        assert dec.generate_greedy(seq[-1], n, 3) == cont[n:]
        # plain temperature sampling, and seeded uniforms
        plain = dec.generate_sampled(tok0, 0, n, 1.0, uniforms=u)
        assert dec.generate_sampled(tok0, 0, n, 1.0, seed=5) == dec.generate_sampled(
            tok0, 0, n, 1.0, uniforms=np.random.default_rng(5).random(n, dtype=np.float32))
        assert plain == dec.generate_sampled(tok0, 0, n, 1.0, uniforms=u)
        # top_k = 1 is the greedy loop whatever the uniforms
        assert dec.generate_sampled(tok0, 0, n, T, 1, 1.0, uniforms=u) == dec.generate_greedy(tok0, 0, n)
        assert dec.graph_kernels(3) == dec.graph_kernels(2)
        assert dec.time_kernel(10, 3) > 0
        assert dec.kernel_name(10) == "sample_kernel"
    finally:
        dec.close()
        dm.close()


def test_argument_errors():
    runtime = rt()
    l = np.zeros(16, np.float32)
    bad = [dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("inf")),
           dict(temperature=float("nan")), dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.5),
           dict(top_p=float("nan")), dict(uniforms=[0.5, -0.1]), dict(uniforms=[1.1]), dict(uniforms=[float("nan")])]
    for kw in bad:
        args = dict(temperature=1.0, top_k=0, top_p=1.0, uniforms=[0.5])
        args.update(kw)
        with pytest.raises(runtime.YalmError, match="yalm error 2"):
            runtime.sample(l, **args)
    with pytest.raises(runtime.YalmError, match="yalm error 2"):
        runtime.sample(np.zeros(131073, np.float32), 1.0)
    assert runtime.sample(np.zeros(131072, np.float32), 1.0, uniforms=[1.0])[0][0] == 131071

    dm = runtime.DeviceModel.synthetic(M.TINY, seed=3)
    dec = runtime.Decoder(dm)
    try:
        for kw in bad:
            args = dict(temperature=1.0, top_k=0, top_p=1.0, uniforms=[0.5])
            args.update(kw)
            with pytest.raises(runtime.YalmError, match="yalm error 2"):
                dec.generate_sampled(1, 0, len(args["uniforms"]), **args)
        with pytest.raises(runtime.YalmError, match="yalm error 2"):
            dec.generate_sampled(1, 0, 65537, 1.0, uniforms=np.zeros(65537, np.float32))
        assert dec.generate_sampled(1, 0, 0, 1.0) == []
    finally:
        dec.close()
        dm.close()
