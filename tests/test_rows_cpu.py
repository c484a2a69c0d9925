"""CPU: what keeps tests/test_gpu_rows.py honest -- the launch plan of the multi-row GEMV
(yalm_rows_plan, the function launch_rows itself calls) holds its invariants at the preset
dimensions, every case of rows_cases.py reaches the path it names, an f32 restatement of the
kernel's order stays under a fifth of the GPU test's bar on every float case, and each of the
index slips of rows_ref.DEFECTS is seen by at least one case.

Measured, the f32 restatement's worst relative error per activation row against float64: RStore
8.5e-7, RResidual 6.8e-7, RGlu with SiLU 2.87e-6 -- all under a fifth of REL_TOL = 2e-5 -- and RGlu
with GELU 5.015e-6 (f16-glu-T3-n13360-d5-norm-gelu), which is above it: GELU-GLU's bar is therefore
5 x 5.02e-6 = 2.51e-5 (rows_ref.GELU_GLU_REL_TOL), every other case keeps REL_TOL."""
import numpy as np
import pytest

import rows_cases as C
import rows_ref as RR
from yalm_amd import models as M

LDS_PER_CU = 160 * 1024
MUTANT_BARS = 10.0


def rt():
    from yalm_amd import runtime

    return runtime


def test_constants_match_the_project():
    assert (C.F32, C.F16, C.F8) == (M.F32, M.F16, M.F8E5M2) and (C.GELU, C.SILU) == (M.GELU, M.SILU)
    assert (RR.WEIGHT_SCALE, RR.NORM_SCALE, RR.NORM_OFFSET) == (M.WEIGHT_SCALE, M.NORM_SCALE, M.NORM_OFFSET)
    assert (C.STORE, C.RESIDUAL, C.GLU) == (rt().ROWS_STORE, rt().ROWS_RESIDUAL, rt().ROWS_GLU)
    assert [C.kcap(dt, 3) for dt in C.DTYPES] == [10752, 10752, 10240]
    assert [C.kcap(C.F16, T) for T in (1, 2, 4)] == [32768, 16384, 8192]
    rng = np.random.default_rng(0)
    v = (rng.standard_normal(4096) * 3).astype(np.float32)
    for dt in C.DTYPES:
        assert np.array_equal(RR.encode(v, dt), M.encode_weights(v, dt))
        assert np.array_equal(RR.decode(RR.encode(v, dt), dt), M.decode_weights(M.encode_weights(v, dt), dt))


def _launches():
    """(n, n_groups) of every multi-row launch of a dense model: QKV, Wo, W1 | W3, W2, logits."""
    shapes = [(c.dim, c.hidden_dim, c.n_heads * c.head_dim, c.n_kv_heads * c.head_dim, c.vocab_size)
              for c in (M.MISTRAL_7B, M.LLAMA_32_3B, M.QWEN3_8B)]
    shapes += [(3584, 18944, 3584, 512, 151936), (8192, 28672, 8192, 1024, 128256)]
    out = set()
    for dim, hidden, q_dim, kv_dim, vocab in shapes:
        out |= {(dim, (q_dim + 2 * kv_dim) // 2), (q_dim, (dim + 1) // 2), (dim, hidden), (hidden, (dim + 1) // 2),
                (dim, (vocab + 1) // 2)}
    return sorted(out)


def test_plan_invariants():
    """yalm_rows_plan at 256 CUs, T 1..4 x the three types x every launch of the presets and of
    dim 3584 / hidden 18944, hidden 28672, vocab 128256 and 151936: the invariants the kernel
    relies on, and the restated plan of rows_cases.py (which the case table is built on)."""
    launches = _launches()
    assert {14336, 8192, 12288, 18944, 28672} <= {n for n, _ in launches}
    assert {64128, 75968, 16000} <= {g for _, g in launches}
    for dt in C.DTYPES:
        ch = C.CH[dt]
        for T in (1, 2, 3, 4):
            for n, n_groups in launches:
                p = rt().rows_plan(dt, n, n_groups, T, C.PLAN_CUS)
                assert p == C.plan(dt, n, n_groups, T), (dt, T, n, n_groups)
                assert p["kseg"] > 0 and p["kseg"] % ch == 0
                assert T * p["kseg"] * 4 <= C.ROWS_X_BYTES
                assert p["nseg"] * p["kseg"] >= n > (p["nseg"] - 1) * p["kseg"]
                assert p["nseg"] == 1 or p["gpw"] == 1
                assert p["gpw"] >= 1 and p["blocks"] * C.WAVES * p["gpw"] >= n_groups
                assert (p["blocks"] - 1) * C.WAVES * p["gpw"] < n_groups  # no workgroup without a group
                assert p["lds"] == (T * p["kseg"] + T * 16) * 4 <= LDS_PER_CU
                assert all((s * p["kseg"]) % ch == 0 for s in range(p["nseg"]))


def test_plan_of_the_mistral_launches_is_pinned():
    """The geometry launch_rows computed for Mistral-7B's W2 and logits at T = 4 (fp16, 256 CUs)
    before the plan became a function of its own, from its arithmetic by hand."""
    assert rt().rows_plan(M.F16, 14336, 2048, 4, 256) == dict(kseg=8192, nseg=2, gpw=1, blocks=256, lds=131328)
    assert rt().rows_plan(M.F16, 4096, 16000, 4, 256) == dict(kseg=4096, nseg=1, gpw=7, blocks=286, lds=65792)
    assert rt().rows_plan(M.F8E5M2, 14336, 2048, 4, 256) == dict(kseg=8192, nseg=2, gpw=1, blocks=256, lds=131328)
    assert rt().rows_plan(M.F32, 4096, 16000, 4, 256)["gpw"] == 7


def test_plan_refusals():
    with pytest.raises(rt().YalmError, match="q4 weights have no multi-row form"):
        rt().rows_plan(M.Q4, 4096, 2048, 4, 256)
    for bad in ((M.F16, 4096, 2048, 0), (M.F16, 4096, 2048, 5), (M.F16, 0, 2048, 1), (M.F16, 4096, 0, 1),
                (M.BF16, 4096, 2048, 1)):
        with pytest.raises(rt().YalmError):
            rt().rows_plan(*bad, 256)


def test_every_case_reaches_its_path():
    """At 256 CUs, by the library's plan; and each (type, epilogue) has every T, a strided case,
    gpw > 1 at T 1, 3, 4 with a partly idle wave, and segmented cases at every T."""
    for c in C.CASES:
        p = rt().rows_plan(c.dtype, c.n, c.n_groups, c.T, C.PLAN_CUS)
        assert p == C.plan(c.dtype, c.n, c.n_groups, c.T), c
        assert not C.reaches(c, p), (c, C.reaches(c, p))
        assert c.n % 16 == 0 and c.xstride % 4 == 0 and c.ostride % 4 == 0
        assert c.xstride >= c.n and c.ostride >= c.d
        w_bytes = c.d * c.n * M.DTYPE_BYTES[c.dtype] * (2 if c.epilogue == C.GLU else 1)
        assert w_bytes <= 8 << 20, (c, w_bytes)  # no case is model-sized
    for dt in C.DTYPES:
        for ep in (C.STORE, C.RESIDUAL, C.GLU):
            cs = C.BY_KIND[(dt, ep)]
            f = [(c, C.facts(c, C.plan(c.dtype, c.n, c.n_groups, c.T))) for c in cs]
            assert {c.T for c, _ in f} == {1, 2, 3, 4}
            assert any(c.xstride != c.n and c.ostride != c.d for c, _ in f), (dt, ep)
            assert {c.T for c, k in f if k["gpw"] > 1} == {1, 3, 4}, (dt, ep)
            assert any(k["gpw"] > 1 and k["partial"] for c, k in f), (dt, ep)
            assert any(k["nseg"] > 1 and c.norm for c, k in f) or ep == C.RESIDUAL, (dt, ep)
            if ep == C.GLU:
                assert {c.act for c in cs} == {C.SILU, C.GELU} and all(c.norm for c in cs)
            else:
                for T in (1, 2, 3, 4):  # segmented at every T, all three of the last segment's parts together
                    assert any(c.T == T and k["nseg"] == 2 and k["uloop"] and k["tail"] and k["ragged"] and k["idle"]
                               for c, k in f), (dt, ep, T)
                assert any(k["nseg"] == 3 for c, k in f), (dt, ep)
                assert any(k["clamp"] for c, k in f)


def _detects(c, got):
    want = RR.reference(c.name)
    if c.exact:
        return not np.array_equal(got, want)  # (a NaN is unequal)
    return not RR.pads_intact(c, got) or RR.bars(c, got, want) >= MUTANT_BARS


def test_model_without_a_defect_passes_every_case():
    """The float64 traversal is the reference at every case: equal on the exact family, within a
    thousandth of a bar on the float family, sentinels intact."""
    for c in C.CASES:
        got = RR.model(c, C.plan(c.dtype, c.n, c.n_groups, c.T))
        want = RR.reference(c.name)
        assert RR.pads_intact(c, got), c
        if c.exact:
            np.testing.assert_array_equal(got, want, err_msg=c.name)
        else:
            assert RR.bars(c, got, want) < 1e-3, c


@pytest.mark.parametrize("epilogue", [C.STORE, C.RESIDUAL, C.GLU], ids=["store", "residual", "glu"])
def test_f32_restatement_is_well_inside_the_bar(epilogue):
    """An honest f32 evaluation in the kernel's order (lane chains of fused multiply-adds, the
    wave_sum butterfly, the norm in stage_x's statement order, f32 activations) stays under a
    fifth of the case's bar (rows_ref.rel_tol) per activation row on every float case. Measured
    worst case: RStore 0.042 bars, RResidual 0.034, RGlu 0.144 with SiLU -- bars of REL_TOL -- and
    0.251 bars of REL_TOL with GELU, whose bar is therefore 5 x that measured error (0.1998 of it
    here by construction). On the exact family the restatement must be exact."""
    worst, at = 0.0, None
    for c in C.CASES:
        if c.epilogue != epilogue or (c.exact and (c.n > 4096 or c.d > 64)):
            continue  # (the exact family: the unsegmented small cases are enough for the order's exactness)
        got = RR.model(c, C.plan(c.dtype, c.n, c.n_groups, c.T), f32=True)
        assert got.dtype == np.float32 and RR.pads_intact(c, got), c
        if c.exact:
            np.testing.assert_array_equal(got, RR.reference(c.name), err_msg=c.name)
            continue
        b = RR.bars(c, got, RR.reference(c.name))
        if b > worst:
            worst, at = b, c
        assert b < 0.2, (c, b)
    print(f"{C.EPILOGUE_NAMES[epilogue]}: the f32 restatement's worst error {worst:.4f} bars at {at}")


def _applies(defect, c, k):
    """Cases on which the defect changes what is read or written (the others are not tried)."""
    return {
        "segment offset dropped from the weight address": k["nseg"] > 1,
        "first chunk of the second segment read at the first segment's x":
            k["nseg"] > 2 or (k["nseg"] == 2 and (k["uloop"] or k["tail"])),
        "chunk tail skipped": k["tail"],
        "ragged end skipped": k["ragged"],
        "ragged end on every lane": k["ragged"] and k["nseg"] > 1,
        "normw read without k0": k["nseg"] > 1 and c.norm,
        "row t's scale taken from row 0": c.norm and c.T > 1,
        "x rows at stride n": c.xstride != c.n and c.T > 1,
        "out rows at stride d": c.ostride != c.d and c.T > 1,
        "clamped row stored": k["clamp"],
        "last gpw iteration dropped": k["gpw"] > 1,
    }[defect]


@pytest.mark.parametrize("defect", RR.DEFECTS)
def test_every_defect_is_seen(defect):
    """Each index slip, switched into the traversal model, makes an exact case unequal or a float
    case miss by at least 10 bars -- in EVERY case the slip applies to that is tried (the smallest
    twelve), not just one: a slip that some case lets through would be a case that proves less
    than it seems to."""
    tried = []
    for c in sorted(C.CASES, key=lambda c: c.n * c.d * c.T):
        p = C.plan(c.dtype, c.n, c.n_groups, c.T)
        if not _applies(defect, c, C.facts(c, p)):
            continue
        assert _detects(c, RR.model(c, p, defect=defect)), (defect, c)
        tried.append(c)
        if len(tried) == 12:
            break
    assert tried, f"no case for: {defect}"
    assert any(c.exact for c in tried) or defect in ("normw read without k0", "row t's scale taken from row 0")
    print(f"{defect}: seen by {', '.join(c.name for c in tried)}")
