"""CPU: the case table, the float64 reference, the numpy model of attn_prefill_kernel and the
bars of test_gpu_prefill_attention.py (tests/pf_attn_ref.py): the table reaches both sides of
every integer decision of the tile loop, the flavours drive the rescale branch as they claim, the
model of the correct kernel is well inside the bars, the split bar is the measured one, a kernel
that loses f16 subnormals is outside it, and twelve plausible kernel bugs are at least 10 bars
from the reference."""
import numpy as np
import pytest

import pf_attn_ref as P


def _n_keys(c):
    return c.pos0 + c.T


def test_table_shape():
    assert len(P.CASES) == len(set(c.name for c in P.CASES)) == 2 * 2 * 5 * len(P.PAIRS)
    assert len(P.GROUPS) == 20 and all(len(v) == len(P.PAIRS) for v in P.GROUPS.values())
    assert {c.G for c in P.CASES} == {1, 3, 4, 8} and {c.n_kv for c in P.CASES} == {1, 2}
    blocks = {-(-T // P.AQ) for T, *_ in P.PAIRS}
    assert blocks == {1, 2, 3}
    # an idle-wave tail block: a last block whose rows fill one wave only
    assert any(T % P.AQ and T % P.AQ <= P.WQ and T > P.AQ for T, *_ in P.PAIRS)
    for key, cases in P.GROUPS.items():  # both poisons in every test
        assert {c.poison for c in cases} == set(P.POISONS), key


def test_edges_are_covered():
    """Both sides of each of the five integer decisions, by exactly one key, from the integers."""
    seen = {}
    for T, pos0, *_ in P.PAIRS:
        for e in P.edges(T, pos0):
            seen.setdefault(e, []).append((T, pos0))
    for cond in ("diag", "skip", "ntile", "fetch", "clamp"):
        for side in (True, False):
            print(f"{cond} {'true' if side else 'false'} by one key: {seen.get((cond, side))}")
            assert seen.get((cond, side)), (cond, side)
    # the pairs the module docstring names
    named = {("diag", True): [(129, 62), (97, 30)], ("diag", False): [(65, 63), (33, 31)],
             ("skip", True): [(130, 33), (129, 1)], ("skip", False): [(128, 0), (257, 0)],
             ("ntile", True): [(1, 0), (1, 64)], ("ntile", False): [(1, 63), (32, 32), (33, 31)],
             ("fetch", True): [(1, 64), (129, 1)], ("fetch", False): [(65, 63), (128, 0)],
             ("clamp", True): [(97, 30), (129, 62)], ("clamp", False): [(1, 63), (64, 0)]}
    for e, pairs in named.items():
        for p in pairs:
            assert p in seen[e], (e, p)


def test_inputs_poison_and_guards():
    for c in P.CASES[::7]:
        q, kc, vc, o_init = P.inputs(c.name)
        n, W = _n_keys(c), c.n_heads * c.head_dim * (2 if c.split else 1)
        assert q.shape == (c.T, W) and o_init.shape == (c.T + P.GUARDS, W)
        assert kc.shape == vc.shape == (n + P.TAIL, c.n_kv * c.head_dim) and P.TAIL > P.KT
        for a in (kc, vc):
            assert np.all(np.isfinite(a[:n])) and np.all(a.view(np.uint16)[n:] == c.poison)
            assert np.abs(a[:n].astype(np.float32)).max() < 4096.0  # far inside the f16 range
        assert np.all(np.isfinite(q)) and np.all(o_init.view(np.uint16)[c.T:] == P.SENTINEL)


def test_reference_is_plain_causal_attention():
    """attn_f64 against a loop over rows and heads written out here."""
    c = P.BY_NAME["d64-split-sink-T33-p31-g1x2"]
    q, kc, vc, _ = P.inputs(c.name)
    o, A = P.reference(c.name)
    D, qd = c.head_dim, c.n_heads * c.head_dim
    qv = q[:, :qd].astype(np.float64) + q[:, qd:].astype(np.float64)
    for r in (0, 1, 32):
        for h in range(c.n_heads):
            g = h // c.G
            K = kc[:c.pos0 + r + 1, g * D:(g + 1) * D].astype(np.float64)
            V = vc[:c.pos0 + r + 1, g * D:(g + 1) * D].astype(np.float64)
            s = K @ qv[r, h * D:(h + 1) * D] / np.sqrt(D)
            p = np.exp(s - s.max())
            p /= p.sum()
            np.testing.assert_allclose(o[r, h * D:(h + 1) * D], p @ V, rtol=1e-12, atol=1e-14)
            np.testing.assert_allclose(A[r, h * D:(h + 1) * D], p @ np.abs(V), rtol=1e-12, atol=1e-14)
    assert P.in_bars(P.out_value(c, np.full((c.T, 2 * qd), np.nan)), o, P.bar_of(c, o, A)) == float("inf")


@pytest.fixture(scope="module")
def model_runs():
    """name -> (bars of the fast bar, stats) of the model on every case; split: (.., .., flush bars)."""
    out = {}
    for c in P.CASES:
        q, kc, vc, _ = P.inputs(c.name)
        o64, A = P.reference(c.name)
        fb = P.fast_bar(o64, A)
        om, stats = P.model(c, q, kc, vc)
        assert om.shape == q.shape and om.dtype == np.float16
        b = P.in_bars(P.out_value(c, om), o64, fb)
        fl = None
        if c.split and c.flavour in ("ramp", "step"):  # the flavours that tell the two apart
            fl = P.in_bars(P.out_value(c, P.model(c, q, kc, vc, flush=True)[0]), o64, fb)
        out[c.name] = (b, stats, fl)
    return out


def test_model_is_inside_the_bars(model_runs):
    """Fast: the model under 0.6 bars on every case. Split: the worst value of the
    subnormals-kept model, in units of fast bar / 1024, is what pf_attn_ref records, and the bar is
    four times it; the flush variant is outside that bar on at least one case."""
    worst_fast = max((b, n) for n, (b, _, _) in model_runs.items() if not P.BY_NAME[n].split)
    worst_split = max((b * 1024, n) for n, (b, _, _) in model_runs.items() if P.BY_NAME[n].split)
    print(f"fast: worst {worst_fast[0]:.3f} bars ({worst_fast[1]})")
    print(f"split: worst {worst_split[0]:.2f} units of fast bar / 1024 ({worst_split[1]}); bar {P.SPLIT_UNITS} units")
    for fl in P.FLAVOURS:
        w = max(b * 1024 for n, (b, _, _) in model_runs.items() if P.BY_NAME[n].split and P.BY_NAME[n].flavour == fl)
        print(f"  split {fl}: worst {w:.2f} units")
    assert worst_fast[0] < 0.6
    # (10 % either way: the float64 partial sums of the model go through the platform's BLAS)
    assert 0.9 * P.MEASURED_SPLIT_WORST <= worst_split[0] <= 1.1 * P.MEASURED_SPLIT_WORST
    assert P.SPLIT_UNITS == 4.0 * P.MEASURED_SPLIT_WORST
    flushed = {n: f * 1024 for n, (_, _, f) in model_runs.items() if f is not None}
    outside = [n for n, u in flushed.items() if u > P.SPLIT_UNITS]
    print(f"flush variant outside the split bar on {len(outside)} of {len(flushed)} ramp / step cases, "
          f"worst {max(flushed.values()):.0f} units")
    assert outside


def test_flavours_drive_the_rescale(model_runs):
    stale = {"slow": 0, "step": 0}
    for name, (_, st, _) in model_runs.items():
        c = P.BY_NAME[name]
        n = _n_keys(c)
        assert st["pmax"] <= 2.0 ** P.RESCALE_LOG2 * (1 + 1e-5), name  # P stays in the f16 range
        if c.flavour == "flat":
            assert st["rescales"] == 0, name
        if (c.flavour, n >= 96) == ("ramp", True) or (c.flavour, n >= 160) == ("slow", True) \
                or (c.flavour, n >= 65) == ("step", True):
            assert st["rescales"] > 0, name
        if c.flavour in stale and n >= 128:
            assert st["stale"] > 0, name
            if n >= 160:
                assert st["pmax"] > 16.0, name  # the stale max really is below the scores
    long_ramp = model_runs["d64-fast-ramp-T64-p1100-g8x2"][1]["rescales"]
    assert long_ramp >= 17 * 2 * 16 - 16  # every tile after tile 0, two waves, sixteen heads


MUTANT_CASES = [c for c in P.CASES if c.head_dim == 64 and c.form == "fast"]
MODEL_MUTANT_PAIRS = ((129, 62), (200, 64), (40, 600))


def test_mutants_are_far_outside():
    """Each of the twelve is at least 10 fast bars from float64 on some case; the two rescale
    mutants also 10 split bars in the split form."""
    caught = {}
    for c in MUTANT_CASES:
        q, kc, vc, _ = P.inputs(c.name)
        o64, A = P.reference(c.name)
        bar = P.bar_of(c, o64, A)
        for name, kw in P.reference_mutants(c).items():
            if kw is None:
                continue
            d = P.in_bars(P.attn_f64(c, q, kc, vc, **kw)[0], o64, bar)
            if d >= 10.0:
                caught.setdefault((name, "fast"), []).append((d, c.name))
    for c in P.CASES:
        if c.head_dim != 64 or (c.T, c.pos0) not in MODEL_MUTANT_PAIRS or c.flavour not in ("ramp", "slow", "step"):
            continue
        q, kc, vc, _ = P.inputs(c.name)
        o64, A = P.reference(c.name)
        bar = P.bar_of(c, o64, A)
        for name, mut in P.MODEL_MUTANTS.items():
            d = P.in_bars(P.out_value(c, P.model(c, q, kc, vc, mutant=mut)[0]), o64, bar)
            if d >= 10.0:
                caught.setdefault((name, c.form), []).append((d, c.name))
    names = sorted({n for n, _ in caught} | set(P.MODEL_MUTANTS) | set(P.reference_mutants(MUTANT_CASES[0])),
                   key=lambda s: int(s.split()[0]))
    assert len(names) == 12
    for n in names:
        for form in ("fast", "split") if n in P.MODEL_MUTANTS else ("fast",):
            hits = caught.get((n, form), [])
            best = max(hits) if hits else None
            print(f"mutant {n} [{form}]: {len(hits)} cases at >= 10 bars"
                  + (f", worst {best[0]:.3g} bars at {best[1]}" if best else ""))
            assert hits, (n, form)


def test_hook_rejects_bad_arguments():
    """yalm_attn_prefill_rows checks its arguments before it touches the device."""
    from yalm_amd import runtime as r

    c = P.GROUPS[(64, "fast", "flat")][0]
    q, kc, vc, o_init = P.inputs(c.name)
    good = dict(o_rows=o_init.shape[0], cache_rows=kc.shape[0], T=c.T, pos0=c.pos0, n_heads=c.n_heads, n_kv=c.n_kv,
                D=c.head_dim, split=0)
    for kw in ({"o_rows": c.T - 1}, {"cache_rows": c.pos0 + c.T - 1}, {"T": 0}, {"pos0": -1}, {"n_kv": 3},
               {"n_kv": 0}, {"D": 0}, {"split": 2}, {"q": None}):
        a = dict(good, q=r._ptr(q))
        a.update(kw)
        rc = r.lib.yalm_attn_prefill_rows(r._ptr(o_init.copy()), a["o_rows"], a["q"], r._ptr(kc), r._ptr(vc),
                                          a["cache_rows"], a["T"], a["pos0"], a["n_heads"], a["n_kv"], a["D"],
                                          a["split"])
        assert rc == 2, kw  # YALM_ERR_ARG
        assert b"yalm_attn_prefill_rows" in r.lib.yalm_last_error()
