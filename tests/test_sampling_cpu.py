"""CPU: the fixed-point sampling rule (tests/sampling_ref.py, the rule the device kernel
implements) against the reference's sampler in f64, its truncation edge cases, and the new
names in the header, the library, the Python binding and the CLI."""
import os
import re
import subprocess

import numpy as np
import pytest

import sampling_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "yalm_amd", "host")

# (vocabulary, logit scale): the distributions the rule was prototyped on
DISTS = [(32000, 3.0), (128256, 3.0), (1000, 8.0)]


def _interior_uniforms(l, T, rng, count):
    x = l.astype(np.float64) / T
    p = np.exp(x - x.max())
    cdf = np.cumsum(p / p.sum())
    u0 = rng.random(64 * count)
    tok = np.minimum(np.searchsorted(cdf, u0, side="left"), l.size - 1)
    lo, hi = np.where(tok > 0, cdf[np.maximum(tok - 1, 0)], 0.0), cdf[tok]
    wide = hi - lo > 5e-5
    u = np.clip(u0, lo + 2e-5, hi - 2e-5)[wide][:count].astype(np.float32)
    assert u.size == count
    return u


@pytest.mark.parametrize("V,scale", DISTS)
@pytest.mark.parametrize("T", [0.25, 1.0, 4.0])
def test_rule_matches_f64_inverse_cdf(V, scale, T):
    """top_k = 0, top_p = 1: the rule is the reference's temperature sampler (sampler.cpp:43-59)
    wherever u is more than 1e-5 from a boundary of the cumulative distribution; at most 5% of
    the 300 uniforms may be that close.

    The uniforms are built for that: random draws, each moved 2e-5 inside the interval of the
    token it hit, and draws that hit an interval narrower than 5e-5 are not used (with plain
    random uniforms the boundaries themselves, 8e-6 apart on average at V = 128256, put most
    draws inside the margin: 35 of 300 at V = 32000, T = 1). The 300 that remain are checked as
    stated: the count inside the margin is asserted, the others must agree."""
    rng = np.random.default_rng(1000 * V + int(T * 100))
    l = (rng.standard_normal(V) * scale).astype(np.float32)
    u = _interior_uniforms(l, T, rng, 300)
    ref, far = R.inverse_cdf_f64(l, T, u)
    dropped = int((~far).sum())
    print(f"V={V} scale={scale} T={T}: {dropped} of {u.size} uniforms within 1e-5 of a boundary")
    assert dropped <= 0.05 * u.size
    rule = R.Rule(l, R.weights_f32(l, T))
    assert rule.kept == V
    got = rule.draws(u)
    assert np.array_equal(got[far], ref[far])


def test_flat_logits_top_p_half_keeps_first_half():
    l = np.full(1000, 1.5, np.float32)
    rule = R.Rule(l, R.weights_f32(l, 1.0), top_k=0, top_p=0.5)
    assert rule.kept == 500 and np.array_equal(np.flatnonzero(rule.mask), np.arange(500))
    assert rule.draw(0.0) == 0 and rule.draw(1.0) == 499


def test_top_k_one_is_first_maximum_with_ties():
    rng = np.random.default_rng(5)
    l = rng.standard_normal(777).astype(np.float32)
    l[[400, 123, 650]] = l.max() + 1.0  # three equal maxima: the first one wins
    for T in (0.25, 1.0, 4.0):
        rule = R.Rule(l, R.weights_f32(l, T), top_k=1)
        assert rule.kept == 1
        for u in (0.0, 0.5, 1.0):
            assert rule.draw(u) == 123 == R.first_max(l)[1]


def test_plateau_cuts_and_fallback():
    """The top-k and the top-p cut inside a plateau of equal logits keep its lowest indices;
    all -inf falls back to token 0 with an empty nucleus."""
    l = np.zeros(64, np.float32)
    l[10:20] = 5.0
    l[40:50] = 5.0
    rule = R.Rule(l, R.weights_f32(l, 1.0), top_k=13)
    assert np.array_equal(np.flatnonzero(rule.mask), np.r_[10:20, 40:43])
    rule = R.Rule(l, R.weights_f32(l, 1.0), top_k=13, top_p=0.5)
    assert np.array_equal(np.flatnonzero(rule.mask), np.r_[10:17])  # ceil(6.5) of 13 equal weights
    ninf = np.full(33, -np.inf, np.float32)
    q = R.weights_f32(ninf, 1.0)
    assert not q.any()
    assert R.Rule(ninf, q).draw(0.7) == 0 and R.Rule(ninf, q, top_p=0.9).kept == 0


def test_keys_preserve_logit_order():
    l = np.array([-np.inf, -3.5, -0.0, 0.0, 1e-30, 2.0, np.inf, np.nan], np.float32)
    k = R.keys(l)
    assert k[2] == k[3] and k[7] == 0
    assert np.all(np.diff(k[[0, 1, 2, 4, 5, 6]].astype(np.int64)) > 0)


def _declared():
    src = open(os.path.join(ROOT, "include", "yalm_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return src


def test_new_names_in_header_library_and_binding():
    from yalm_amd import runtime

    src = _declared()
    assert re.search(r"typedef struct yalm_sampling\s*\{\s*float temperature;\s*int top_k;\s*float top_p;", src)
    out = subprocess.run(["nm", "-D", "--defined-only", runtime.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    for name in ("yalm_generate_sampled", "yalm_sample"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert re.search(r"\bT %s\b" % name, out), name
        assert name in runtime.EXPORTED and hasattr(runtime.lib, name)
    assert callable(runtime.sample) and callable(runtime.Decoder.generate_sampled)
    assert [f[0] for f in runtime.Sampling._fields_] == ["temperature", "top_k", "top_p"]


def test_cli_usage_lists_top_k_and_top_p():
    subprocess.run(["make", "-C", HOST, "-j4"], check=True, capture_output=True)
    r = subprocess.run([os.path.join(HOST, "yalm")], capture_output=True)
    assert r.returncode == 1
    usage = r.stderr.decode()
    assert re.search(r"^\s*-k <int>", usage, re.M) and re.search(r"^\s*-p <float>", usage, re.M)
